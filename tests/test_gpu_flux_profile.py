"""Flux-surface profiles on the device (csrc/flux_profile.hip through gfhip_flux_*): labels against the numpy model of
tests/flux_model.py bit for bit; every cell's limbs against rational arithmetic byte for byte, the three counters
exactly; and the same bytes whatever route the samples take — workgroup-private sums or not, any order, any split.
There is no tolerance anywhere: the label's arithmetic is fixed and the sums are exact."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, STATE

import flux_model
from test_flux_label import all_points, same_bits

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 255, 256, 257, 4099)


@pytest.fixture(scope="module")
def context():
    from graph_framework_amd import Context
    context = Context(0)
    yield context
    context.close()


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(os.path.join(GOLDEN, "efit_tables.npz")))


@pytest.fixture(scope="module")
def pool(tables):
    """(x, y, z) of the label tests' points and their labels by the model, computed once."""
    points = all_points(tables, np.load(os.path.join(GOLDEN, "flux_golden.npz")))
    labels = flux_model.label(tables, *points)
    labels.setflags(write=False)
    return points, labels


def upload(context, tag, columns, names=("x", "y", "z", "value"), dtype=None):
    from graph_framework_amd import _lib, key_of
    keys = []
    for name, column in zip(names, columns):
        key = "%s_%s" % (tag, name)
        context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), len(column),
                                                         _lib.GFIR_F64 if dtype is None else dtype))
        context.copy_to_device(key, column)
        keys.append(key)
    return keys


def samples(pool, n, seed, planted=()):
    """n samples of the pool's points, those with the labels `planted` among them (in a block of mixed points).  Values over the whole exponent range with subnormals, 1e308, both signs, +-0,
    NaN and +-inf.  Every other block of 64 (a wave) repeats ONE point with values of ONE exponent (the wave-uniform
    pre-sum), the blocks between them mix points and exponents; cancelling pairs share a cell."""
    (px, py, pz), _ = pool
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, px.size, n)
    value = rng.uniform(-1.0, 1.0, n)*2.0**rng.integers(-1074, 1001, n).astype(np.float64)
    tiny = rng.random(n) < 0.1
    value[tiny] = rng.integers(-4000, 4000, int(tiny.sum()))*5e-324
    value[rng.random(n) < 0.05] = 1.0e308
    value[rng.random(n) < 0.05] = -1.0e308
    for start in range(0, n, 128):
        stop = min(start + 64, n)
        pick[start:stop] = pick[start]
        value[start:stop] = rng.uniform(1.0, 2.0, stop - start)*rng.choice([-1.0, 1.0], stop - start)*2.0**int(rng.integers(-1000, 1000))
    for k, label in enumerate(planted):
        pick[64 + 5*k:64 + 5*k + 2] = np.flatnonzero(pool[1] == label)[0]
        value[64 + 5*k:64 + 5*k + 2] = (1.5 + k, 2.0**-1060)
    half = n//4
    pick[3*half:4*half] = pick[2*half:3*half]
    value[3*half:4*half] = -value[2*half:3*half]
    bad = rng.random(n) < 0.03
    value[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf]), int(bad.sum()))
    zero = rng.random(n) < 0.02
    value[zero] = rng.choice(np.array([0.0, -0.0]), int(zero.sum()))
    return [px[pick], py[pick], pz[pick], value]


def edges_for(kind, pool, cap=256):
    _, labels = pool
    if kind == "one":
        return np.array([0.25, 0.75])
    if kind == "seven_on_labels":                                           # labels of the pool: samples sit exactly on the edges
        finite = np.unique(labels[(labels > 0.2) & (labels < 0.8)])
        return finite[np.linspace(0, finite.size - 1, 8).astype(int)]
    cells = {"cap": cap, "cap_plus_one": cap + 1, "1024": 1024}[kind]
    return 0.15 + 0.7*np.linspace(0.0, 1.0, cells + 1)**1.5                 # not uniform; part of the pool is outside


def check(profile, model, divisor=1.0):
    assert profile.counts() == model.counts
    assert profile.state().tobytes() == model.state().tobytes()
    same_bits(profile.read(divisor), model.bins(divisor))


@pytest.mark.parametrize("sqrt_label", [False, True], ids=["s", "sqrt_s"])
def test_labels_equal_the_model_bit_for_bit(context, tables, pool, sqrt_label):
    from graph_framework_amd.flux import FluxProfile
    (x, y, z), labels = pool
    profile = FluxProfile(context, tables, [0.0, 1.0], sqrt_label=sqrt_label)
    keys = upload(context, "label", [x, y, z, np.full(x.size, 7.0)], ("x", "y", "z", "label"))
    profile.label(*keys, x.size)
    got = np.empty(x.size)
    context.copy_to_host(keys[3], got)
    same_bits(got, flux_model.label(tables, x, y, z, sqrt_label=sqrt_label))
    if not sqrt_label:
        same_bits(got, labels)
    assert profile.counts() == dict(samples=0, outside=0, skipped=0)        # labelling deposits nothing
    profile.close()


@pytest.mark.parametrize("kind", ["one", "seven_on_labels", "cap", "cap_plus_one", "1024"])
def test_deposits_against_the_model(context, tables, pool, kind):
    """Every count on both paths where the private one exists; the last add is longer than a full grid of workgroups,
    so that the grid-stride loop takes a second trip."""
    from graph_framework_amd.flux import FluxProfile
    probe = FluxProfile(context, tables, [0.0, 1.0])
    cap = probe.info()["cap_cells"]
    probe.close()
    assert cap == 256
    edges = edges_for(kind, pool, cap)
    cells = edges.size - 1
    expect_private = cells <= cap
    base = samples(pool, 4099, 100 + cells, edges if kind == "seven_on_labels" else ())
    if kind == "seven_on_labels":                                           # a sample on edge i belongs to cell i, on the last edge to none
        on_an_edge = flux_model.label(tables, *[c[64:64 + 5*8] for c in base[:3]])
        assert (flux_model.cells_of(edges, on_an_edge)[::5] == [0, 1, 2, 3, 4, 5, 6, -1]).all()
        assert (on_an_edge[::5] == edges).all()
    routes = (True, False) if expect_private else (True,)
    for count in COUNTS + ("long",):
        if count == "long":
            probe = FluxProfile(context, tables, edges)
            info = probe.info()
            probe.close()
            count = 2*info["max_workgroups"]*info["workgroup_size"] + 77
        columns = [np.resize(c, count) for c in base]                       # the base tiled
        model = flux_model.Profile(tables, edges).add(*columns)
        if count >= 4099:
            assert model.counts["outside"] and model.counts["skipped"] and any(total < 0 for total in model.units)
            assert sum(total != 0 for total in model.units) >= min(cells, 7)//2 + 1
        keys = upload(context, "grid%d" % count, columns)             # a key keeps its first size
        for private in routes:
            profile = FluxProfile(context, tables, edges, private=private)
            info = profile.info()
            assert info["private_sums"] == (private and expect_private)
            assert info["workgroup_size"] == (1024 if info["private_sums"] else 256)
            if info["private_sums"]:
                assert info["lds_bytes"] == cells*536 + (cells + 1)*8 <= 160*1024
            assert count <= 4099 or count > info["max_workgroups"]*info["workgroup_size"]      # the loop's second trip
            profile.add(*keys, count)
            check(profile, model)
            check(profile, model, 3.0)                                      # reading again changes nothing
            profile.close()


def test_a_small_profile_does_not_take_the_large_ones_lds(context, tables, pool):
    """The dynamic LDS a launch may ask for is a setting of the kernel on the device, not of a profile: a 7-cell profile
    created while the cap profile lives must leave the cap profile's launches (139,272 B) possible."""
    from graph_framework_amd.flux import FluxProfile
    edges = edges_for("cap", pool)
    columns = samples(pool, 4099, 9)
    keys = upload(context, "lds", columns)
    large = FluxProfile(context, tables, edges)
    assert large.info()["private_sums"] and large.info()["lds_bytes"] == 139272
    small_edges = edges_for("seven_on_labels", pool)
    small = FluxProfile(context, tables, small_edges)
    assert small.info()["private_sums"] and small.info()["lds_bytes"] < 65536
    small.add(*keys, 4099)
    large.add(*keys, 4099)
    check(large, flux_model.Profile(tables, edges).add(*columns))
    check(small, flux_model.Profile(tables, small_edges).add(*columns))
    large.close()
    small.close()


def test_same_bytes_whatever_the_route(context, tables, pool):
    from graph_framework_amd.deposition import Deposition
    from graph_framework_amd.flux import FluxProfile
    edges = edges_for("seven_on_labels", pool)
    columns = samples(pool, 4099, 7, edges)
    keys = upload(context, "route", columns)
    model = flux_model.Profile(tables, edges).add(*columns)

    whole = FluxProfile(context, tables, edges)
    whole.add(*keys, 4099)
    check(whole, model)
    want, counts = whole.state().tobytes(), whole.counts()

    plain = FluxProfile(context, tables, edges, private=False)              # without the on-chip sums
    assert whole.info()["private_sums"] and not plain.info()["private_sums"]
    plain.add(*keys, 4099)
    assert plain.state().tobytes() == want and plain.counts() == counts

    order = np.random.default_rng(8).permutation(4099)                      # any order
    shuffled = FluxProfile(context, tables, edges)
    shuffled.add(*upload(context, "shuffled", [c[order] for c in columns]), 4099)
    assert shuffled.state().tobytes() == want and shuffled.counts() == counts

    pieces = FluxProfile(context, tables, edges)                            # seven adds
    cuts = [0, 1, 64, 700, 701, 2048, 4000, 4099]
    for p, (low, high) in enumerate(zip(cuts[:-1], cuts[1:])):
        pieces.add(*upload(context, "piece%d" % p, [c[low:high] for c in columns]), high - low)
    assert pieces.state().tobytes() == want and pieces.counts() == counts

    merged = FluxProfile(context, tables, edges)                            # two profiles, one of them without private sums
    for h, part in enumerate((order[:1777], order[1777:])):
        shard = FluxProfile(context, tables, edges, private=bool(h))
        shard.add(*upload(context, "shard%d" % h, [c[part] for c in columns]), part.size)
        merged.merge(shard.state(), **shard.counts())
        shard.close()
    assert merged.state().tobytes() == want and merged.counts() == counts
    same_bits(merged.read(5.0), whole.read(5.0))

    labels = flux_model.label(tables, *columns[:3])                         # the 3-D grid on the labels as x
    grid = Deposition(context, edges, np.array([-1.0, 1.0]), np.array([-1.0, 1.0]))
    grid.add(*upload(context, "grid3d", [labels, np.zeros(4099), np.zeros(4099), columns[3]]), 4099)
    assert grid.state().reshape(-1, 67).tobytes() == want and grid.counts() == counts
    for each in (whole, plain, shuffled, pieces, merged, grid):
        each.close()


def edges_on_labels(pool, cells):
    """cells + 1 edges whose first, last and (with more than one cell) one inner edge are labels of the pool's points:
    (edges, the pool indices of those points, their labels)."""
    _, labels = pool
    finite = np.unique(labels[(labels > 0.2) & (labels < 0.8)])
    first, inner, last = finite[1], finite[finite.size//2], finite[-2]
    edges = np.linspace(first, last, cells + 1)
    on = [first, last]
    if cells > 1:
        at = int(np.searchsorted(edges, inner))                             # edges[at - 1] < inner <= edges[at]
        assert 0 < at < cells
        edges[at] = inner
        on = [first, inner, last]
    assert edges[0] == first and edges[-1] == last and (np.diff(edges) > 0.0).all()
    return edges, [int(np.flatnonzero(labels == label)[0]) for label in on], np.array(on)


@pytest.mark.parametrize("private", [True, False], ids=["private", "global"])
@pytest.mark.parametrize("cells", [1, 256, 257])
def test_the_grid_and_the_profile_are_one_rule(context, tables, pool, cells, private):
    """The profile's own labels binned as the x column of a 3-D grid with the profile's edges (y and z: one cell around
    zeros) give the profile's bytes: deposit_kernel, flux_deposit_kernel<true> (1 and 256 cells) and
    flux_deposit_kernel<false> are three callers of the pieces of csrc/cell_deposit.hpp.  2*1024 + 37 samples: more
    than one private workgroup, a multiple of neither 64 nor 1024."""
    from graph_framework_amd.deposition import Deposition
    from graph_framework_amd.flux import FluxProfile
    (px, py, pz), labels = pool
    n = 2*1024 + 37
    edges, on, on_labels = edges_on_labels(pool, cells)
    columns = samples(pool, n, 300 + cells)                                # mixed and wave-uniform blocks, off-map points
    inside = on[0]                                                          # on the first edge: in cell 0
    specials = [0.0, -0.0, 15e-324, 1.797e308, -1.797e308, 1.797e308, np.nan, np.inf, -np.inf, 2.0**-1060]
    for c, p in zip(columns[:3], (px, py, pz)):
        c[200:200 + len(specials)] = p[inside]
        c[220:220 + len(on)] = p[on]                                        # exactly on an edge; the last one on the last edge
        c[128:192] = p[inside]                                              # one whole wave of identical samples
    columns[3][200:200 + len(specials)] = specials
    columns[3][220:220 + len(on)] = 1.5
    columns[3][128:192] = 0.1
    picked = flux_model.label(tables, *columns[:3])
    assert np.isnan(picked).any()                                           # points off the map
    assert (picked[220:220 + len(on)] == on_labels).all() and np.isin(on_labels, edges).all() and on_labels[-1] == edges[-1]

    profile = FluxProfile(context, tables, edges, private=private)
    assert profile.info()["private_sums"] == (private and cells <= 256)
    keys = upload(context, "rule%d" % cells, columns)
    label_key = upload(context, "rule_label%d" % cells, [np.zeros(n)], ("label",))[0]
    profile.label(*keys[:3], label_key, n)
    device_labels = np.empty(n)
    context.copy_to_host(label_key, device_labels)
    same_bits(device_labels, picked)
    profile.add(*keys, n)

    grid = Deposition(context, edges, np.array([-1.0, 1.0]), np.array([-1.0, 1.0]))
    grid_keys = upload(context, "rule_grid%d" % cells, [device_labels, np.zeros(n), np.zeros(n), columns[3]])
    grid.add(*grid_keys, n)
    counts = profile.counts()
    assert counts["samples"] == n and counts["outside"] >= int(np.isnan(picked).sum()) + 1 and counts["skipped"] >= 3
    assert grid.state().reshape(cells, 67).tobytes() == profile.state().tobytes() and profile.state().any()
    assert grid.counts() == counts
    same_bits(grid.read(3.0).reshape(cells), profile.read(3.0))
    grid.close()
    profile.close()


def test_records_accumulate_and_state_does_not_disturb_them(context, tables, pool):
    from graph_framework_amd.flux import FluxProfile
    edges = edges_for("cap", pool)
    records = [samples(pool, 300, 40 + r) for r in range(4)]
    profile = FluxProfile(context, tables, edges)
    model = flux_model.Profile(tables, edges)
    keys = upload(context, "record", records[0])
    for r, record in enumerate(records):
        for key, column in zip(keys, record):
            context.copy_to_device(key, column)
        profile.add(*keys, 300)
        model.add(*record)
        if r == 1:
            assert profile.state().tobytes() == model.state().tobytes()     # canonical in place, between two adds
    check(profile, model, 1200.0)
    profile.close()


def test_misuse_is_refused_before_anything_runs(context, tables, pool):
    import ctypes
    from graph_framework_amd import GfHipError, _lib
    from graph_framework_amd.flux import FluxProfile, flux_map
    lib = context.lib

    def create(given, edges, cells=None):
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        return lib.gfhip_flux_create(context.handle, ctypes.byref(given) if given is not None else None,
                                     edges.ctypes.data if edges.size else None, edges.size - 1 if cells is None else cells)

    def refused(match, given, edges, cells=None):
        assert not create(given, edges, cells)
        assert match in lib.gfhip_last_error(context.handle).decode(), lib.gfhip_last_error(context.handle).decode()

    good, keep = flux_map(tables)
    unit = np.array([0.0, 0.5, 1.0])
    refused("needs a map and edges", None, unit)
    refused("needs a map and edges", good, np.array([]), 2)
    refused("1 to 4096 cells", good, unit, 0)
    refused("1 to 4096 cells", good, np.arange(4098.0))
    for edges in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 1.0], [0.0, np.inf]):
        refused("strictly increasing", good, np.array(edges))
    for field, value, match in (("numr", 0, "numr >= 1"), ("numz", 0, "numr >= 1"), ("numr", 1 << 31, "2^31 cells"),
                                ("numz", (1 << 31) + 1, "2^31 cells"), ("dr", 0.0, "finite and non-zero"),
                                ("dz", np.nan, "finite and non-zero"), ("span", np.inf, "finite and non-zero"),
                                ("span", 0.0, "finite and non-zero"), ("flags", 4, "unknown flag bits"),
                                ("flags", 1 << 31, "unknown flag bits"), ("reserved", 1, "reserved"),
                                ("coefficients", None, "coefficient tables")):
        broken, keep_too = flux_map(tables)
        setattr(broken, field, value)
        refused(match, broken, unit)

    columns = [np.full(64, 1.9), np.zeros(64), np.zeros(64), np.full(64, 3.0)]
    assert 0.0 < flux_model.label(tables, *[c[:1] for c in columns[:3]])[0] < 1.0
    ok = upload(context, "ok", columns)
    narrow = upload(context, "narrow", columns, dtype=_lib.GFIR_F32)
    profile = FluxProfile(context, tables, unit)
    other = FluxProfile(context, tables, [0.0, 1.0])
    for method in (profile.add, profile.label):
        with pytest.raises(GfHipError, match="fp64"):
            method(ok[0], ok[1], ok[2], narrow[3], 64)
        with pytest.raises(GfHipError, match="shorter"):
            method(*ok, 65)
        with pytest.raises(GfHipError, match="unknown buffer"):
            method(ok[0], ok[1], "no such buffer", ok[3], 64)
    with pytest.raises(GfHipError, match="another shape"):
        profile.merge(other.state(), samples=5)
    for call, arguments in ((lib.gfhip_flux_state, (None,)), (lib.gfhip_flux_read, (1.0, None)), (lib.gfhip_flux_info, (None,)),
                            (lib.gfhip_flux_merge, (None, 2, 1, 0, 0))):
        assert call(profile.handle, *arguments) == 1
        assert "needs a" in lib.gfhip_last_error(context.handle).decode()
    for call, arguments in ((lib.gfhip_flux_add, (1, 2, 3, 4, 1)), (lib.gfhip_flux_label, (1, 2, 3, 4, 1)),
                            (lib.gfhip_flux_counts, (None, None, None)), (lib.gfhip_flux_state, (None,)),
                            (lib.gfhip_flux_merge, (None, 1, 0, 0, 0)), (lib.gfhip_flux_read, (1.0, None)),
                            (lib.gfhip_flux_info, (None,))):
        assert call(None, *arguments) == 1                                  # a null profile
    lib.gfhip_flux_destroy(None)
    assert profile.counts() == dict(samples=0, outside=0, skipped=0)        # nothing was launched
    assert not profile.state().any()
    got = np.empty(64)
    context.copy_to_host(ok[3], got)
    assert (got == 3.0).all()                                               # the refused label() wrote nothing
    profile.add(*ok, 64)                                                    # and the profile still works
    check(profile, flux_model.Profile(tables, unit).add(*columns))
    profile.close()
    other.close()


RAYS = 264
BOX = (np.linspace(1.7, 2.4, 5), np.linspace(-0.2, 0.05, 4), np.linspace(-0.15, 0.15, 6))


def test_pipeline_gives_one_state_on_every_route(tmp_path, tables):
    """The 21 golden records tiled to 264 rays: bin_power(flux=), OnePass(flux=) and flux_deposition over the written file
    give one state; a deposition grid given alongside is what it is alone."""
    from graph_framework_amd import Context
    from graph_framework_amd.deposition import Deposition
    from graph_framework_amd.flux import FluxProfile, flux_deposition
    from graph_framework_amd.output import RAY_VARIABLES, ResultFile
    from test_gpu_one_pass import golden_records
    from graph_framework_amd.absorption import bin_power, run_absorption
    from graph_framework_amd.pipeline import OnePass
    from graph_framework_amd import _lib
    from graph_framework_amd.backend import key_of
    records = golden_records()
    saved = records.shape[0]
    edges = np.linspace(0.0, 1.0, 17)
    context = Context(0)
    alone, beside = Deposition(context, *BOX), Deposition(context, *BOX)
    staged, direct, from_file = (FluxProfile(context, tables, edges) for _ in range(3))

    staged_dir, grid_dir = tmp_path / "staged", tmp_path / "grid"
    staged_dir.mkdir()
    grid_dir.mkdir()
    path = str(staged_dir / "result0.nc")
    trace = ResultFile(path, RAYS)
    for name, _ in RAY_VARIABLES:
        trace.create_variable(name)
    column = {k: i for i, k in enumerate(STATE + ("residual",))}
    for r in range(saved):
        trace.write({name: records[r, column[key]] for name, key in RAY_VARIABLES})
    trace.close()
    run_absorption(path, saved - 1)
    shutil.copy(path, str(grid_dir / "result0.nc"))
    bin_power(str(grid_dir / "result0.nc"), saved - 1, deposition=alone)    # the grid alone
    bin_power(path, saved - 1, deposition=beside, flux=staged)              # both

    source = Context(0)
    names = STATE + ("residual",)
    for name in names:
        source._check(source.lib.gfhip_allocate_buffer(source.handle, key_of(name), RAYS, _lib.GFIR_F64))
    pipeline = OnePass(source, RAYS, str(tmp_path / "direct0.nc"), flux=direct)         # flux alone
    for r in range(saved):
        for i, name in enumerate(names):
            source.copy_to_device(name, records[r, i])
        pipeline.record()
    pipeline.close()
    source.close()

    bins, counts = flux_deposition(str(staged_dir), 1, tables, 16, 0.0, 1.0, profile=from_file)

    result = ResultFile(path)
    x, y, z, d_power = (np.stack([result.read(name, r) for r in range(saved)]).reshape(-1) for name in ("x", "y", "z", "d_power"))
    result.close()
    model = flux_model.Profile(tables, edges).add(x, y, z, d_power)
    assert model.counts["samples"] == saved*RAYS and sum(total != 0 for total in model.units) >= 2
    for profile in (staged, direct, from_file):
        check(profile, model, RAYS)
    assert counts == model.counts
    same_bits(bins, model.bins(RAYS))
    assert beside.state().tobytes() == alone.state().tobytes() and beside.counts() == alone.counts()
    assert alone.counts()["samples"] == saved*RAYS

    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    written = H5File(str(staged_dir / "flux_bins.nc"))
    same_bits(written.read("bins"), bins)
    same_bits(written.read("sbins"), edges)
    written.close()
    for each in (alone, beside, staged, direct, from_file):
        each.close()
    context.close()


def test_example_writes_equal_flux_bins_on_both_routes(tmp_path):
    """examples/trace_rays.py --flux-bins 16 with and without --one-pass, a child process each: 11 records of 512 rays
    (at 2000 steps this beam has absorbed nothing yet and every bin is an exact zero; at 4000 it has)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    got = []
    for flag, prefix in (([], str(tmp_path / "staged")), (["--one-pass"], str(tmp_path / "direct"))):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "trace_rays.py"), "--rays", "512", "--dispersion",
                              "ordinary_wave", "--steps", "4000", "--sub-steps", "400", "--output", prefix,
                              "--absorption-model", "weak_damping", "--flux-bins", "16", "--flux-tables",
                              os.path.join(GOLDEN, "efit_tables.npz")] + flag, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr      # the second process starts only behind a clean first
        assert "flux profile on 16 cells of s: 5632 samples" in out.stdout, out.stdout
        f = H5File(prefix + "_flux0.nc")
        got.append((f.read("bins"), f.read("sbins")))
        assert f.read("ns").shape == (16,) and f.read("nsp").shape == (17,)
        f.close()
    same_bits(got[0][0], got[1][0])
    same_bits(got[0][1], np.linspace(0.0, 1.0, 17))
    assert got[0][0].shape == (16,) and np.isfinite(got[0][0]).all() and got[0][0].sum() > 0.0
