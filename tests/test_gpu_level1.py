"""Lowering level 1 on the device (graph_framework_amd/csrc/options.hpp `level`): the assembly
statement with sign records and negated tables folded into `neg` modifiers and commutative twins and equal square roots
computed once stores the bits of level 0 — NaNs included, bit for bit, because every lane that stores a non-finite value
is computed again by the redo kernel, which is the same kernel at both levels."""
import os

import numpy as np
import pytest

import level1_items
from oracle import gfir
from planted_tables import differing, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(array):
    return np.ascontiguousarray(array).view(np.uint64)


PLANTED_CASES = [  # seed, inputs, nodes, first register of the pool, LDS budget of the staged tables
    (61, 6, 200, 64, 65536), (71, 6, 150, 224, 65536), (73, 6, 150, 224, 0), (63, 8, 500, 160, 0),
]


def _run(blob, level, initial, launches, rays):
    from graph_framework_amd import Context
    inputs, outputs = len(initial), 3
    context = Context(0)
    in_keys = ["in%d" % i for i in range(inputs)]
    out_keys = ["out%d" % i for i in range(outputs)]
    kernel = context.add_kernel(blob, rays, level)
    context.compile()
    assert kernel.info().level == level
    kernel.create_kernel_call(in_keys, out_keys, initial)
    results = []
    for steps in launches:
        kernel.run(steps)
        context.wait()
        results.append([context.copy_to_host(key, np.empty(rays, dtype=np.float64)) for key in in_keys + out_keys])
    flags = context.flags()
    context.close()
    return results, flags


@pytest.mark.parametrize("seed,inputs,nodes,pool,budget", PLANTED_CASES, ids=["%d-nodes-pool-%d-lds-%d" % c[2:] for c in PLANTED_CASES])
def test_planted_items_are_bit_exact_at_level_1(monkeypatch, tmp_path, seed, inputs, nodes, pool, budget):
    """Random items with every fold planted (tests/level1_items.py), 2048 rays, level 1 through small register pools:
    the oracle's bits on every lane, and level 0's bits on every lane with NaNs compared as bits.  Sixteen lanes start
    from NaN, infinities and zeros of both signs, so that the redo launch has work to do."""
    from graph_framework_amd.backend import generate_piece_sources
    monkeypatch.setenv("GFHIP_ASM_MIN_NODES", "0")
    monkeypatch.setenv("GFHIP_ASM_POOL_LO", str(pool))
    monkeypatch.setenv("GFHIP_ASM_WAVES", "1")
    monkeypatch.setenv("GFHIP_LDS_BUDGET", str(budget))
    monkeypatch.setenv("GFHIP_CACHE_DIR", str(tmp_path))
    rays = 2048
    blob, planted = level1_items.planted_item(seed, inputs, nodes)
    text0, text1 = generate_piece_sources(blob, 0)[0][0], generate_piece_sources(blob, 1)[0][0]
    assert "v_rcp_f64" in text0 and text1 != text0 and "; alias r" in text1
    oracle_item = gfir.Item(blob)
    rng = np.random.default_rng(3000 + seed)
    initial = [rng.uniform(-1.0, 1.0, rays).astype(np.float64) for _ in range(inputs)]
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, -np.nan]
    for lane in range(16):
        initial[lane % inputs][100 + 67*lane] = special[lane % len(special)]
    launches = (1, 1, 3)
    level1, flags1 = _run(blob, 1, initial, launches, rays)
    level0, flags0 = _run(blob, 0, initial, launches, rays)
    assert flags1 == flags0 and flags1 & 1              # lanes did leave the window: the redo launch ran
    expected = [c.copy() for c in initial]
    with np.errstate(all="ignore"):
        for launch, steps in enumerate(launches):
            expected_out, _ = oracle_item.run(expected, steps=steps)
            for k, want in enumerate(expected + expected_out):
                got = level1[launch][k]
                assert same_bits(got, want), (k, launch, differing(got, want)[:5])
                assert np.array_equal(bits(got), bits(level0[launch][k])), (k, launch, np.flatnonzero(bits(got) != bits(level0[launch][k]))[:5])


def _rk4(level, state, steps):
    from graph_framework_amd.xrays import STATE, RaySolver
    solver = RaySolver(state)
    solver.solver_level = level
    solver.compile()
    info = solver.solver.kernel.info()
    assert info.level == level and info.from_cache
    for _ in range(steps):
        solver.step()
    host = solver.sync_host()
    out = {k: host[k].copy() for k in STATE}
    out["residual"] = solver.residual().copy()
    flags = solver.work.context.flags()
    solver.work.context.close()
    return out, info.source_hash, flags


@pytest.mark.parametrize("rays_kind", ["bench", "cli"])
def test_rk4_step_level_1_against_level_0(rays_kind):
    """solver_kernel_f64, 4096 rays x 25 steps, level 1 against level 0: every array byte-identical — on the benchmark's
    identical rays and on the CLI beam (a few of its rays blow up and take the redo path), each with four lanes planted
    with NaN, infinite and zero state."""
    from graph_framework_amd.xrays import STATE, cli_distribution
    rays = 4096
    if rays_kind == "bench":
        state = {k: np.full(rays, v) for k, v in dict(t=0.0, w=500.0, x=2.5, y=0.0, z=0.0, kx=-600.0, ky=0.0, kz=0.0).items()}
    else:
        state = cli_distribution(rays, seed=0)
    state = {k: np.array(state[k], dtype=np.float64) for k in STATE}
    state["kx"][17] = np.nan
    state["x"][1234] = np.inf
    state["kz"][2049] = -np.inf
    for k in ("x", "y", "z", "kx", "ky", "kz"):
        state[k][4000] = 0.0
    level1, hash1, flags1 = _rk4(1, state, 25)
    level0, hash0, flags0 = _rk4(0, state, 25)
    assert hash1 != hash0 and flags1 == flags0 and flags1 & 1
    for k in level0:
        assert np.array_equal(bits(level1[k]), bits(level0[k])), (k, np.flatnonzero(bits(level1[k]) != bits(level0[k]))[:5])
    finite = np.isfinite(level1["x"])
    assert 0 < np.count_nonzero(~finite) < rays//2


def test_front_end_asks_for_level_1(monkeypatch):
    """Rk4ColdPlasmaEfit lowers its step at level 1 and says so; GFHIP_LEVEL=0 brings back level 0 and the code object
    of the lowering without a level (the same source hash)."""
    from graph_framework_amd import backend
    from graph_framework_amd.xrays import Rk4ColdPlasmaEfit, workload

    def info():
        solve = Rk4ColdPlasmaEfit({k: np.full(64, v) for k, v in dict(t=0.0, w=500.0, x=2.5, y=0.0, z=0.0, kx=-600.0, ky=0.0, kz=0.0).items()})
        solve.compile()
        solve.step()
        solve.work.wait()
        out = solve.solver.kernel.info()
        solve.work.context.close()
        return out

    with open(workload("solver_kernel"), "rb") as f:
        blob = f.read()
    default = info()
    assert default.level == 1 and default.from_cache and default.source_hash == backend.generate_source(blob, 1)[1]
    monkeypatch.setenv("GFHIP_LEVEL", "0")
    plain = info()
    monkeypatch.delenv("GFHIP_LEVEL")
    assert plain.level == 0 and plain.from_cache and plain.source_hash == backend.generate_source(blob, 0)[1]
    assert plain.source_hash != default.source_hash
