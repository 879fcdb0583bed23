"""Merged records (graph_framework_amd/csrc/merge.hpp, GFHIP_MERGE) on the device: the kernels written for a merged item
compute, bit for bit, what the oracle computes for the item as it arrived — in the window of the shared-reciprocal
division and, through the redo launch and the IEEE function, outside it.  The CPU side is tests/test_merge.py."""
import re

import numpy as np
import pytest

import gfir_random
from gfir_random import ADD, DIV, FMA, GATHER1, GATHER2, MUL, NONE, SQRT
from oracle import gfir

pytestmark = pytest.mark.gpu


def _run_against_the_oracle(blob, columns, in_keys, out_keys, passes=2):
    """`passes` launches of `blob` on `columns` against the oracle; returns (status flags, kernel info)."""
    from graph_framework_amd import Context
    from test_gpu_division import _same
    oracle_item = gfir.Item(blob)
    rays = columns[0].size
    context = Context(0)
    kernel = context.add_kernel(blob, rays)
    context.compile()
    kernel.create_kernel_call(in_keys, out_keys, columns)
    info = kernel.info()
    expected = [c.copy() for c in columns]
    with np.errstate(all="ignore"):
        for launch in range(passes):
            expected_out, _ = oracle_item.run(expected)
            kernel.run(1)
            context.wait()
            for key, want in zip(in_keys + out_keys, expected + expected_out):
                got = context.copy_to_host(key, np.empty(rays, dtype=oracle_item.np_dtype))
                assert _same(got, want), (key, launch)
    flags = context.flags()
    context.close()
    return flags, info


@pytest.mark.parametrize("body", ["assembly", "compiled"])
def test_planted_item_on_the_device(monkeypatch, tmp_path, body):
    """The planted item of tests/test_merge.py (a duplicated denominator, quotient and square root, powers that share
    their prefixes, twins the pass leaves alone) on 4096 rays whose rows include the division edges, so that the window
    check fails and the redo launch (assembly body) or the IEEE function (compiled body) does real work."""
    from graph_framework_amd.backend import generate_piece_sources
    from test_merge import edge_values, planted_item, rays_with_edges
    monkeypatch.setenv("GFHIP_CACHE_DIR", str(tmp_path))
    if body == "assembly":
        monkeypatch.setenv("GFHIP_ASM_MIN_NODES", "0")
    else:
        monkeypatch.setenv("GFHIP_ASM", "0")
    blob, _, merges, _ = planted_item()
    text = generate_piece_sources(blob)[0][0]
    assert ("v_rcp_f64_e32" in text) == (body == "assembly")
    names = r"; alias r\d+ = r\d+" if body == "assembly" else r"const real r\d+ = r\d+;"
    assert len(re.findall(names, text)) >= len(merges)
    columns = rays_with_edges(6, np.float64, random_rays=4096 - 7*edge_values(np.float64).size)
    assert columns[0].size == 4096
    flags, info = _run_against_the_oracle(blob, columns, ["in%d" % i for i in range(6)], ["out%d" % i for i in range(6)])
    assert flags & 1                                                  # lanes did leave the window
    assert info.segments == (1 if body == "assembly" else 0)


def test_rk4_item_merged_against_unmerged(monkeypatch):
    """solver_kernel on 4096 rays of the example's distribution, 20 steps, in two contexts: the default lowering and
    GFHIP_MERGE=0 (the kernel of the commit before the pass).  All eight state arrays come out with the same bits."""
    from graph_framework_amd.xrays import Rk4ColdPlasmaEfit, STATE, cli_distribution
    n = 4096
    rays = {k: np.ascontiguousarray(v[:n]) for k, v in cli_distribution(n, seed=0).items()}
    results = {}
    for merge in ("1", "0"):
        monkeypatch.setenv("GFHIP_MERGE", merge)
        solve = Rk4ColdPlasmaEfit({k: v.copy() for k, v in rays.items()})
        solve.init("kx")
        solve.compile()
        for _ in range(20):
            solve.step()
        results[merge] = {k: v.copy() for k, v in solve.sync_host().items()}
        solve.work.context.close()
    for k in STATE:
        assert np.array_equal(results["1"][k].view(np.uint64), results["0"][k].view(np.uint64)), k
    assert not np.array_equal(results["1"]["x"], rays["x"])


def _stress_item_with_duplicates():
    """tests/gfir_random.py's division stress item (quotients that share a denominator, a quotient inside a denominator,
    as a gather argument and under a square root) with, appended, records equal to some of its first ones: cut into three
    segments, a duplicate and what it is merged into lie on two sides of a cut."""
    rng = np.random.default_rng(5)
    b = gfir_random.Builder(rng, "f64", 5)
    n0, n1, d0, d1, x = b.inputs
    q0 = b.emit(DIV, n0, d0)
    q1 = b.emit(DIV, n1, d0)
    product = b.emit(MUL, n0, n1)
    q2 = b.emit(DIV, product, d1)
    two = b.constant(2.0)
    shifted = b.emit(ADD, q0, two)
    q3 = b.emit(DIV, x, shifted)
    table = b.table(1, 16)
    g = b.emit(GATHER1, q1, aux=table, imm=(0.25, -2.0, 0.0, 0.0))
    table2 = b.table(5, 6)
    g2 = b.emit(GATHER2, q0, q2, aux=table2, imm=(0.5, -1.0, 0.5, -1.0))
    s = b.emit(SQRT, b.emit(MUL, q0, q0))
    mix = b.emit(FMA, g, q3, b.emit(MUL, g2, s))

    def raw(op, a=NONE, bb=NONE, c=NONE):
        b.code.append((op, a, bb, c, 0, (0.0, 0.0, 0.0, 0.0)))
        b.bound.append(1.0)
        return len(b.code) - 1

#  (padding, so that three segments have something each, then the duplicates at the far end)
    chain = mix
    for _ in range(12):
        chain = raw(FMA, chain, q1, x)
    q0_again = raw(DIV, n0, d0)                             # a quotient of the first segment
    shifted_again = raw(ADD, q0_again, two)                 # ... the denominator made of it
    q3_again = raw(DIV, x, shifted_again)                   # ... and the quotient by that denominator
    product_again = raw(MUL, n0, n1)
    tail = raw(FMA, q3_again, product_again, chain)
    outputs = [q0, q1, q2, q3, mix, tail]
    setters = [(b.emit(DIV, x, d1), 4)]
    return gfir_random.serialize(b, outputs, setters, 5, "division_stress_merged")


def test_segmented_item_hands_over_representatives(monkeypatch, tmp_path):
    """The hand-over path: the division stress item with duplicates across the cuts, three segments and the redo launch,
    on the division edges.  The hand-over buffers hold one chunk of at least 16 384 rays (gf_hip.cpp): 16 384 + 8192
    rays are two chunks, the second of 8192."""
    from graph_framework_amd.backend import export_pieces
    from test_gpu_division import _operands
    monkeypatch.setenv("GFHIP_SEGMENTS", "3")
    monkeypatch.setenv("GFHIP_SEGMENTS_MIN_NODES", "10")
    monkeypatch.setenv("GFHIP_HANDOVER_BYTES", "1")
    monkeypatch.setenv("GFHIP_CACHE_DIR", str(tmp_path))
    blob = _stress_item_with_duplicates()
    pieces = export_pieces(blob)
    assert len(pieces) == 3
    columns = _operands("f64", tiny_numerators=False)
    rays = 16384 + 8192
    columns = [np.tile(c, rays//c.size + 1)[:rays].copy() for c in columns]
    flags, info = _run_against_the_oracle(blob, columns, ["n0", "n1", "d0", "d1", "x"], ["q0", "q1", "q2", "q3", "mix", "tail"])
    assert info.segments == 3
    assert flags & 1                                                  # lanes did leave the window
