"""Deposition on the device (csrc/deposition.hip through gfhip_bins_*): every bin against rational arithmetic,
bit for bit, and the three counters exactly.

The oracle: a sample belongs to cell numpy.searchsorted(edges, c, side="right") - 1 on each axis if
edges[0] <= c < edges[-1] (false for a NaN) — bin.py's `mask` — and is `outside` otherwise; an inside sample whose
value is NaN or infinite is `skipped`; every other inside sample is added as an integer count of 2^-1074
(test_deposition.units); a bin is the correctly rounded sum (test_deposition.rounded) divided by the divisor in
IEEE arithmetic.  There is no tolerance anywhere: the sums are exact."""
import os
import shutil
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, STATE
from test_deposition import LIMBS, canonical_limbs, rounded, units

pytestmark = pytest.mark.gpu

XEDGES = np.array([-1.0, 0.0, 1.0, 2.0])
YEDGES = np.array([0.0, 0.5, 1.0])
ZEDGES = np.array([-2.0, 0.25, 2.0])
EDGES = (XEDGES, YEDGES, ZEDGES)


@pytest.fixture(scope="module")
def context():
    from graph_framework_amd import Context
    context = Context(0)
    yield context
    context.close()


def upload(context, tag, columns, dtype=None):
    """Four arrays into context buffers of their own; returns the keys."""
    from graph_framework_amd import _lib, key_of
    keys = []
    for name, column in zip(("x", "y", "z", "value"), columns):
        key = "%s_%s" % (tag, name)
        context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), len(column),
                                                         _lib.GFIR_F64 if dtype is None else dtype))
        context.copy_to_device(key, column)
        keys.append(key)
    return keys


class Oracle:
    def __init__(self, edges):
        self.edges = edges
        self.shape = tuple(e.size - 1 for e in edges)
        self.units = {}
        self.counts = dict(samples=0, outside=0, skipped=0)

    def add(self, x, y, z, value):
        inside = np.ones(x.size, dtype=bool)
        index = []
        for edges, c in zip(self.edges, (x, y, z)):
            with np.errstate(invalid="ignore"):
                inside &= (c >= edges[0]) & (c < edges[-1])
            index.append(np.searchsorted(edges, c, side="right") - 1)
        finite = np.isfinite(value)
        self.counts["samples"] += x.size
        self.counts["outside"] += int((~inside).sum())
        self.counts["skipped"] += int((inside & ~finite).sum())
        for s in np.flatnonzero(inside & finite):
            cell = (index[0][s], index[1][s], index[2][s])
            self.units[cell] = self.units.get(cell, 0) + units(value[s])
        return self

    def bins(self, divisor=1.0):
        out = np.zeros(self.shape)
        for cell, total in self.units.items():
            out[cell] = rounded(total)
        with np.errstate(over="ignore", invalid="ignore"):
            return out/np.float64(divisor)

    def state(self):
        out = np.zeros(self.shape + (LIMBS,), dtype=np.int64)
        for cell, total in self.units.items():
            out[cell] = canonical_limbs(total)
        return out


def same_bits(got, want):
    assert got.shape == want.shape
    assert got.tobytes() == want.tobytes(), np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:5]


def check(deposition, oracle, divisor=1.0):
    same_bits(deposition.read(divisor), oracle.bins(divisor))
    assert deposition.counts() == oracle.counts
    assert deposition.state().tobytes() == oracle.state().tobytes()


def edge_samples(n, seed):
    """Coordinates on and around every edge, values over the whole exponent range with cancelling pairs."""
    rng = np.random.default_rng(seed)
    special_x = np.array([-1.0, 0.0, -0.0, 1.0, 2.0, np.nextafter(2.0, 0.0), np.nextafter(-1.0, -2.0), -1.5, 2.5, np.nan,
                          np.nextafter(0.0, -1.0), np.nextafter(1.0, 0.0), np.inf, -np.inf])
    special_y = np.array([0.0, -0.0, 0.5, np.nextafter(0.5, 0.0), 1.0, np.nextafter(1.0, 0.0), -5e-324, np.nan, 0.75])
    special_z = np.array([-2.0, 0.25, np.nextafter(0.25, 0.0), 2.0, np.nextafter(2.0, 0.0), -2.5, np.nan, 0.0, -0.0])
    columns = []
    for special, (low, high) in zip((special_x, special_y, special_z), ((-1.2, 2.2), (-0.1, 1.1), (-2.2, 2.2))):
        c = rng.uniform(low, high, n)
        pick = rng.random(n) < 0.4
        c[pick] = rng.choice(special, int(pick.sum()))
        columns.append(c)
    value = rng.uniform(-1.0, 1.0, n)*2.0**rng.integers(-1074, 1001, n).astype(np.float64)
    tiny = rng.random(n) < 0.1
    value[tiny] = rng.integers(-4000, 4000, int(tiny.sum()))*5e-324                     # subnormals
    half = n//4
    for c in columns:                                                                   # cancelling pairs share a cell
        c[half:2*half] = c[:half]
    value[half:2*half] = -value[:half]
    bad = rng.random(n) < 0.03
    value[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf]), int(bad.sum()))
    value[rng.random(n) < 0.02] = 0.0
    order = rng.permutation(n)
    return [c[order] for c in columns] + [value[order]]


def test_edges_tails_and_the_whole_exponent_range(context):
    """1000 samples (15 full waves and a tail of 40 lanes) on a 3x2x2 grid."""
    from graph_framework_amd.deposition import Deposition
    columns = edge_samples(1000, 11)
    oracle = Oracle(EDGES).add(*columns)
    assert oracle.counts["outside"] > 100 and oracle.counts["skipped"] > 5 and len(oracle.units) == 12
    assert any(total < 0 for total in oracle.units.values())
    deposition = Deposition(context, *EDGES)
    deposition.add(*upload(context, "edge", columns), 1000)
    check(deposition, oracle)
    check(deposition, oracle, 3.0)                      # reading again changes nothing; the division is IEEE
    deposition.close()


def fast_path_cases():
    inside = (0.5, 0.25, 1.0)
    cases = {}
    cases["identical"] = [np.full(256, c) for c in inside] + [np.full(256, 0.1)]
    one_elsewhere = [np.full(64, c) for c in inside] + [np.full(64, 0.1)]
    one_elsewhere[0][37] = 1.5
    cases["one lane in another bin"] = one_elsewhere
    two_limbs = [np.full(64, c) for c in inside] + [np.full(64, 1.0)]
    two_limbs[3][::3] = 2.0**40
    cases["two first limbs"] = two_limbs
    some_outside = [np.full(100, c) for c in inside] + [np.full(100, -0.3)]
    some_outside[1][5:60:2] = 7.0                       # outside lanes do not break the wave's agreement
    some_outside[3][70:80] = np.nan
    cases["some lanes add nothing"] = some_outside
    negative = [np.full(192, c) for c in inside] + [np.tile([2.0**-1070, -2.0**-1071, 5e-324], 64)]
    cases["mixed signs in the lowest limb"] = negative
    return cases


@pytest.mark.parametrize("name", list(fast_path_cases()))
def test_wave_uniform_path_and_its_exits(context, name):
    from graph_framework_amd.deposition import Deposition
    columns = fast_path_cases()[name]
    oracle = Oracle(EDGES).add(*columns)
    deposition = Deposition(context, *EDGES)
    deposition.add(*upload(context, "fast%d" % len(columns[0]), columns), len(columns[0]))
    check(deposition, oracle)
    deposition.close()


def test_records_accumulate_and_state_does_not_disturb_them(context):
    from graph_framework_amd.deposition import Deposition
    records = [edge_samples(130, 20 + r) for r in range(5)]
    oracle = Oracle(EDGES)
    deposition = Deposition(context, *EDGES)
    keys = upload(context, "record", records[0])
    for record in records:
        for key, column in zip(keys, record):
            context.copy_to_device(key, column)
        deposition.add(*keys, 130)
        oracle.add(*record)
    check(deposition, oracle, 650.0)
    deposition.close()

    a, b = edge_samples(300, 31), edge_samples(300, 32)
    deposition = Deposition(context, *EDGES)
    deposition.add(*upload(context, "first", a), 300)
    assert deposition.state().tobytes() == Oracle(EDGES).add(*a).state().tobytes()      # canonical in place
    deposition.add(*upload(context, "second", b), 300)
    check(deposition, Oracle(EDGES).add(*a).add(*b))
    deposition.close()


def test_order_and_shards_do_not_matter(context):
    from graph_framework_amd.deposition import Deposition
    columns = edge_samples(1000, 41)
    whole = Deposition(context, *EDGES)
    whole.add(*upload(context, "whole", columns), 1000)
    order = np.random.default_rng(42).permutation(1000)
    halves = []
    for h, part in enumerate((order[:437], order[437:])):
        shard = Deposition(context, *EDGES)
        shard.add(*upload(context, "half%d" % h, [c[part] for c in columns]), part.size)
        halves.append(shard)
    merged = Deposition(context, *EDGES)
    for shard in halves:
        merged.merge(shard.state(), **shard.counts())
    assert merged.state().tobytes() == whole.state().tobytes()
    same_bits(merged.read(7.0), whole.read(7.0))
    assert merged.counts() == whole.counts()
    check(merged, Oracle(EDGES).add(*columns))
    for deposition in halves + [merged, whole]:
        deposition.close()


def test_misuse_is_refused_before_anything_runs(context):
    from graph_framework_amd import GfHipError, _lib
    from graph_framework_amd.deposition import Deposition
    for edges in (np.array([0.0, 1.0, 1.0]), np.array([0.0, 2.0, 1.0]), np.array([0.0, np.nan, 1.0]), np.array([0.0, np.inf])):
        with pytest.raises(GfHipError, match="strictly increasing"):
            Deposition(context, edges, YEDGES, ZEDGES)
    with pytest.raises(GfHipError, match="2047"):
        Deposition(context, np.arange(2049.0), YEDGES, ZEDGES)
    with pytest.raises(GfHipError, match="2\\^25"):
        Deposition(context, np.arange(1025.0), np.arange(1025.0), np.arange(65.0))
    columns = [np.full(64, 0.5), np.full(64, 0.25), np.full(64, 1.0), np.full(64, 3.0)]
    good = upload(context, "good", columns)
    narrow = upload(context, "narrow", columns, _lib.GFIR_F32)
    deposition = Deposition(context, *EDGES)
    with pytest.raises(GfHipError, match="fp64"):
        deposition.add(good[0], good[1], good[2], narrow[3], 64)
    with pytest.raises(GfHipError, match="shorter"):
        deposition.add(*good, 65)
    with pytest.raises(GfHipError, match="unknown buffer"):
        deposition.add(good[0], good[1], "no such buffer", good[3], 64)
    lib = context.lib
    for call, arguments in ((lib.gfhip_bins_state, (None,)), (lib.gfhip_bins_merge, (None, 1, 0, 0)),
                            (lib.gfhip_bins_read, (1.0, None))):
        assert call(deposition.handle, *arguments) == 1                                 # a null pointer on a live grid
    for call, arguments in ((lib.gfhip_bins_add, (1, 2, 3, 4, 1)), (lib.gfhip_bins_counts, (None, None, None)),
                            (lib.gfhip_bins_state, (None,)), (lib.gfhip_bins_merge, (None, 0, 0, 0)),
                            (lib.gfhip_bins_read, (1.0, None))):
        assert call(None, *arguments) == 1                                              # a null grid
    lib.gfhip_bins_destroy(None)
    assert deposition.counts() == dict(samples=0, outside=0, skipped=0)                 # nothing was launched
    assert not deposition.state().any()
    deposition.add(*good, 64)                                                           # and the grid still works
    check(deposition, Oracle(EDGES).add(*columns))
    deposition.close()


def test_like_gives_an_empty_twin_whose_state_merges_back(context):
    """64*3 + 5 samples: half added to the grid, half to its twin on another context and merged, against all of them
    added to one grid directly."""
    from graph_framework_amd import Context
    from graph_framework_amd.deposition import Deposition
    n = 64*3 + 5
    columns = edge_samples(n, 51)
    direct = Deposition(context, *EDGES)
    direct.add(*upload(context, "like_all", columns), n)
    original = Deposition(context, *EDGES)
    original.add(*upload(context, "like_first", [c[:100] for c in columns]), 100)
    elsewhere = Context(0)
    twin = original.like(elsewhere)
    assert twin.context is elsewhere and twin.handle != original.handle
    assert twin.shape == original.shape == (3, 2, 2)
    assert all(np.array_equal(ours, theirs) for ours, theirs in zip(twin.edges, original.edges)) and len(twin.edges) == 3
    assert twin.counts() == dict(samples=0, outside=0, skipped=0) and not twin.state().any()
    twin.add(*upload(elsewhere, "like_rest", [c[100:] for c in columns]), n - 100)
    original.merge(twin.state(), **twin.counts())
    assert original.state().tobytes() == direct.state().tobytes()
    assert original.counts() == direct.counts()
    check(original, Oracle(EDGES).add(*columns))
    twin.close()
    elsewhere.close()
    original.close()
    direct.close()


def _read_bins(path):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    f = H5File(path)
    out = {name: f.read(name) for name in ("bins", "xbins", "ybins", "zbins")}
    f.close()
    return out


def test_pipeline_from_a_trajectory_file_to_bins_nc(tmp_path):
    """trace file -> kamp -> power, d_power -> bins.nc, as xrays followed by utilities/bin.py; the same profile from
    bin_power's fused binning; and from two copies of the file."""
    from graph_framework_amd import Context
    from graph_framework_amd.absorption import bin_power, run_absorption
    from graph_framework_amd.deposition import Deposition, bin_deposition
    from graph_framework_amd.output import RAY_VARIABLES, ResultFile
    golden = np.load(os.path.join(GOLDEN, "absorption_golden.npz"))
    records = golden["records"]
    saved, _, n = records.shape
    one, fused, two = (tmp_path / name for name in ("one", "fused", "two"))
    for directory in (one, fused, two):
        directory.mkdir()
    path = str(one / "result0.nc")
    trace = ResultFile(path, n)
    for name, _ in RAY_VARIABLES:
        trace.create_variable(name)
    column = {k: i for i, k in enumerate(STATE + ("residual",))}
    for r in range(saved):
        trace.write({name: records[r, column[key]] for name, key in RAY_VARIABLES})
    trace.close()
    run_absorption(path, saved - 1)
    shutil.copy(path, str(fused / "result0.nc"))
    bin_power(path, saved - 1)

    result = ResultFile(path)
    x, y, z, d_power = (np.stack([result.read(name, r) for r in range(saved)]).reshape(-1) for name in ("x", "y", "z", "d_power"))
    result.close()
    box = []
    for c in (x, y, z):
        low, high = np.nanmin(c), np.nanmax(c)
        pad = 0.01*(high - low) + 1.0e-6
        box.append((low - pad, high + pad))
    cells = (5, 3, 4)
    arguments = []
    for count, (low, high) in zip(cells, box):
        arguments += [count, low, high]
    edges = [np.linspace(low, high, count + 1) for count, (low, high) in zip(cells, box)]
    oracle = Oracle(edges).add(x, y, z, d_power)
    assert oracle.counts["outside"] == 0 and sum(total != 0 for total in oracle.units.values()) >= 3

    bins, counts = bin_deposition(str(one), 1, *arguments)
    assert counts == oracle.counts
    same_bits(bins, oracle.bins(n))
    written = _read_bins(str(one / "bins.nc"))
    same_bits(written["bins"], oracle.bins(n))
    for name, want in zip(("xbins", "ybins", "zbins"), edges):
        same_bits(written[name], want)

    context = Context(0)
    deposition = Deposition(context, *edges)
    bin_power(str(fused / "result0.nc"), saved - 1, deposition=deposition)
    check(deposition, oracle, n)
    deposition.close()
    context.close()
    result = ResultFile(str(fused / "result0.nc"))                                      # the default behaviour is untouched
    assert np.array_equal(np.stack([result.read("d_power", r) for r in range(saved)]).reshape(-1), d_power, equal_nan=True)
    result.close()

    for copy in ("result0.nc", "result1.nc"):
        shutil.copy(path, str(two / copy))
    twice, counts = bin_deposition(str(two), 2, *arguments)
    assert counts == {name: 2*value for name, value in oracle.counts.items()}
    same_bits(twice, bins)
