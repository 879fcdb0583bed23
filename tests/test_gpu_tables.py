"""Gathers and index nodes on the device against the numpy model of tests/planted_tables.py (itself held to the oracle
in tests/test_tables.py), on planted tables — zeros of both signs, subnormals, the largest finite value, an infinity, a
NaN, exact multiples of one another — and on arguments that sit on the cell boundaries, under every lowering that
touches a gather: compaction on and off, packs in LDS and in global memory, the compiled and the assembly body, the
three division modes, parking, segments with a redo launch.  Every lane, every output and every input after the
setters has the model's bits, the sign of a zero included, over two passes.

No test asserts a clean status word: the lanes with an infinite or NaN argument leave the window of the shared-reciprocal
division on purpose, which puts the gathers of the IEEE function and of the redo launch under the same comparison."""
import functools

import numpy as np
import pytest

import planted_tables
from planted_tables import differing, same_bits

pytestmark = pytest.mark.gpu

PASSES = 2
SEGMENTED_RAYS = 16384 + 8192            # a hand-over chunk holds at least 16 384 rays (tests/test_gpu_merge.py): two chunks
ASSEMBLY = {"GFHIP_ASM": "1", "GFHIP_ASM_MIN_NODES": "0"}
ENVIRONMENTS = {
    "default": {},
    "compiled": {"GFHIP_ASM": "0"},
    "assembly_7": ASSEMBLY,                                             # (the tables of one length each: the outputs of an
    "assembly_16": ASSEMBLY,                                            # assembly body stay in registers to its end, and
    "assembly_33": ASSEMBLY,                                            # 17 of them fit next to its register pool)
    "assembly_small_pool": dict(ASSEMBLY, GFHIP_ASM_POOL_LO="224"),     # values go through LDS slots and back
    "global_packs": {"GFHIP_LDS_BUDGET": "0"},
    "split_packs": {"GFHIP_LDS_BUDGET": None},                          # the budget of test_tables.staging_budget()
    "uncompacted": {"GFHIP_COMPACT_TABLES": "0"},
    "ieee": {"GFHIP_DIVISION": "ieee"},
    "checked": {"GFHIP_DIVISION": "checked"},
    "parked": {"GFHIP_PARK": "heavy"},                                  # parked derived gathers are defined at once
    "segmented": {"GFHIP_SEGMENTS": "3", "GFHIP_SEGMENTS_MIN_NODES": "10", "GFHIP_HANDOVER_BYTES": "1"},
}
GATHER_CASES = [(dtype, name) for name in ENVIRONMENTS for dtype in ("f64", "f32")
                if dtype == "f64" or not name.startswith("assembly")]    # the assembly body is fp64 only
#  The part of the probe a case takes (planted_tables.gather_probe); every other case takes all of it.
PARTS = {
    "assembly_7": dict(lengths=(7,), two_d=False),
    "assembly_16": dict(lengths=(16,), two_d=False),
    "assembly_33": dict(lengths=(33,), two_d=False),
#  16 register pairs: the gathers of ordinary values of two lengths woven into two chains, 16 values live at the turn
    "assembly_small_pool": dict(lengths=(16, 33), names=planted_tables.ORDINARY + ("base", "flipped"),
                                stored=("base", "flipped"), weave=True),
    "segmented": dict(padding=12),                                      # an FMA chain, so that three segments have something each
}
INDEX_CASES = [(dtype, name) for name in ("default", "compiled", "ieee") for dtype in ("f64", "f32")]


@functools.lru_cache(maxsize=None)
def _modelled(kind, dtype, part=""):
    """(probe, initial columns, [(columns after pass p, outputs of pass p)]) — computed once per probe; read only."""
    columns = planted_tables.probe_arguments(dtype)
    if kind == "gather":
        probe = planted_tables.gather_probe(dtype, **PARTS.get(part, {}))
    else:
        probe, buffers = planted_tables.index_probe(dtype, columns[0].size)
        columns = columns + buffers
    state = [c.copy() for c in columns]
    passes = []
    for _ in range(PASSES):
        outputs = probe.model(state)
        passes.append(([c.copy() for c in state], outputs))
    return probe, columns, passes


def _run(monkeypatch, tmp_path, kind, dtype, environment, rays=None, part=""):
    """Build the probe under `environment`, run it twice and hold every lane to the model.  Returns (flags, info).
    Lanes are independent, so the model of `rays` tiled lanes is the tiled model."""
    from graph_framework_amd import Context
    for key, value in environment.items():
        monkeypatch.setenv(key, value)
    monkeypatch.setenv("GFHIP_CACHE_DIR", str(tmp_path))
    probe, columns, passes = _modelled(kind, dtype, part)
    assert probe.records < 100
    lanes = columns[0].size
    rays = rays or lanes

    def tiled(a):
        return a.copy() if rays == lanes else np.tile(a, rays//lanes + 1)[:rays].copy()

    context = Context(0)
    kernel = context.add_kernel(probe.blob, rays)
    context.compile()
    kernel.create_kernel_call(probe.in_keys, probe.out_keys, [tiled(c) for c in columns])
    info = kernel.info()
    for launch, (state, outputs) in enumerate(passes):
        kernel.run(1)
        context.wait()
        for key, want in zip(probe.in_keys + probe.out_keys, state + outputs):
            want = tiled(want)
            got = context.copy_to_host(key, np.empty(rays, dtype=want.dtype))
            assert same_bits(got, want), (key, launch, differing(got, want)[:8])
    flags = context.flags()
    context.close()
    return flags, info


@pytest.mark.parametrize("dtype,name", GATHER_CASES, ids=["%s-%s" % c for c in GATHER_CASES])
def test_gathers_on_planted_tables(monkeypatch, tmp_path, dtype, name):
    from graph_framework_amd.backend import generate_piece_sources
    environment = dict(ENVIRONMENTS[name])
    if name == "split_packs":
        from test_tables import staging_budget
        environment["GFHIP_LDS_BUDGET"] = str(staging_budget(dtype))
    segmented = name == "segmented"
    if name.startswith("assembly"):
        for key, value in environment.items():
            monkeypatch.setenv(key, value)
        text = generate_piece_sources(_modelled("gather", dtype, name)[0].blob)[0][0]
        assert "v_cvt_u32_f64" in text                                  # the assembly body's own clamp and convert
        if name == "assembly_small_pool":
            assert "ds_write_b64" in text and "ds_read_b64" in text
    flags, info = _run(monkeypatch, tmp_path, "gather", dtype, environment, SEGMENTED_RAYS if segmented else None, name)
    if segmented:
        assert info.segments >= 2
    if dtype == "f64" and name != "ieee":
        assert flags & 1                                                # lanes did leave the window and were redone


@pytest.mark.parametrize("dtype,name", INDEX_CASES, ids=["%s-%s" % c for c in INDEX_CASES])
def test_index_nodes_on_planted_buffers(monkeypatch, tmp_path, dtype, name):
    flags, _ = _run(monkeypatch, tmp_path, "index", dtype, ENVIRONMENTS[name])
    if dtype == "f64" and name != "ieee":
        assert flags & 1
