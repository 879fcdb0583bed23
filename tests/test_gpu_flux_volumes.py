"""Flux volumes on the device (flux_volume_kernel of csrc/flux_profile.hip through gfhip_flux_add_volumes): the state and
the counters against the numpy model of tests/flux_volume_model.py and against the host path byte for byte, on both
deposit paths, for every launch shape and split of the point range; the window; the two derived yardsticks of
tests/test_flux_volumes.py (the whole map in rational arithmetic, the analytic solid); the refusals; the Python surface."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, STATE

import flux_model
import flux_volume_model as volume_model
from test_flux_label import same_bits
from test_flux_volumes import (BROKEN_MAPS, WHOLE_MAP_EDGES, check_solid, check_whole_map, edge_sets, refusals)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def context():
    from graph_framework_amd import Context
    context = Context(0)
    yield context
    context.close()


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(os.path.join(GOLDEN, "efit_tables.npz")))


def check(profile, model):
    assert profile.counts() == model.counts
    assert profile.state().tobytes() == model.state().tobytes()
    same_bits(profile.read(), model.bins())


@pytest.mark.parametrize("sqrt_label", [False, True], ids=["s", "sqrt_s"])
@pytest.mark.parametrize("sub", [1, 2, 3])
def test_bytes_equal_the_model_and_the_host(context, tables, sub, sqrt_label):
    """1, 7, 256 (the cap) and 257 cells (the global path) on [0, 1] and seven cells between labels of the points
    themselves, with and without the private sums where they exist."""
    from graph_framework_amd.flux import FluxProfile, volumes_host
    for edges in edge_sets(tables, sub, sqrt_label):
        model = volume_model.model(tables, edges, sub, sqrt_label=sqrt_label)
        limbs, counts = volumes_host(tables, edges, sub, sqrt_label=sqrt_label)
        assert limbs.tobytes() == model.state().tobytes() and counts == model.counts
        for private in (True, False) if edges.size - 1 <= 256 else (True,):
            profile = FluxProfile(context, tables, edges, sqrt_label=sqrt_label, private=private)
            assert profile.info()["private_sums"] == (private and edges.size - 1 <= 256)
            profile.add_volumes(sub)
            check(profile, model)
            profile.close()


@pytest.fixture(scope="module")
def large(context, tables):
    """(sub, edges, the model of the whole point range): more points than one full grid of private workgroups holds."""
    from graph_framework_amd.flux import FluxProfile
    edges = np.linspace(0.0, 1.0, 8)
    probe = FluxProfile(context, tables, edges)
    info = probe.info()
    probe.close()
    assert info["private_sums"]
    sub = 12
    while volume_model.total_points(tables, sub) <= info["max_workgroups"]*info["workgroup_size"]:
        sub += 4
    return sub, edges, volume_model.model(tables, edges, sub)


def test_launch_shapes_and_splits(context, tables, large):
    """The range cut at 1, 63, 4099 and in the middle of a gz row, none a multiple of 64, 256 or 1024: the pieces in
    shuffled order into one profile, and into two profiles that are merged, give the bytes of one call and of the model,
    with and without the private sums."""
    from graph_framework_amd.flux import FluxProfile
    sub, edges, model = large
    total = volume_model.total_points(tables, sub)
    row = 64*sub
    cuts = [0, 1, 63, 4099, row*301 + row//2 + 1, total]
    assert all(cut % 64 for cut in cuts[1:-1]) and cuts[4] % row not in (0, row - 1)
    pieces = list(zip(cuts[:-1], np.diff(cuts)))
    order = np.random.default_rng(11).permutation(len(pieces))
    for private in (True, False):
        whole = FluxProfile(context, tables, edges, private=private)
        info = whole.info()
        assert info["private_sums"] == private
        assert not private or total > info["max_workgroups"]*info["workgroup_size"]     # the loop's second trip
        whole.add_volumes(sub)
        check(whole, model)
        whole.add_volumes(sub, first=77, count=0)                           # nothing
        check(whole, model)

        shuffled = FluxProfile(context, tables, edges, private=private)
        for p in order:
            shuffled.add_volumes(sub, first=pieces[p][0], count=pieces[p][1])
        check(shuffled, model)

        merged = FluxProfile(context, tables, edges, private=private)
        for h, part in enumerate((order[:2], order[2:])):
            shard = FluxProfile(context, tables, edges, private=bool(h))
            for p in part:
                shard.add_volumes(sub, first=pieces[p][0], count=pieces[p][1])
            merged.merge(shard.state(), **shard.counts())
            shard.close()
        check(merged, model)
        for each in (whole, shuffled, merged):
            each.close()


def test_window(context, tables):
    from graph_framework_amd.flux import FluxProfile
    edges = np.linspace(0.0, 1.0, 8)
    sub = 2
    _, _, r, z, _ = volume_model.points(tables, sub)
    columns, rows = np.unique(r), np.unique(z)
    window = (columns[20], columns[90], rows[7], rows[100])                 # lo on a generated coordinate: in; hi on one: out
    inside = volume_model.in_window(window, r, z)
    assert inside.sum() == 70*93 and inside[r == columns[20]].any() and not inside[r == columns[90]].any()
    assert inside[z == rows[7]].any() and not inside[z == rows[100]].any()
    whole = volume_model.model(tables, edges, sub)
    for given, model in ((window, volume_model.model(tables, edges, sub, window)), (volume_model.WHOLE, whole), (None, whole)):
        for private in (True, False):
            profile = FluxProfile(context, tables, edges, private=private)
            profile.add_volumes(sub, given)
            check(profile, model)
            profile.close()
    profile = FluxProfile(context, tables, edges)
    profile.add_volumes(sub, (100.0, 101.0, -1.0, 1.0))                     # off the map
    assert not profile.state().any() and profile.counts() == dict(samples=r.size, outside=r.size, skipped=0)
    profile.close()


def test_whole_map_identity(context, tables):
    from graph_framework_amd.flux import FluxProfile
    profile = FluxProfile(context, tables, WHOLE_MAP_EDGES)
    profile.add_volumes(8)
    check_whole_map(tables, profile.read()[0], profile.counts())
    profile.close()


def test_solid_of_revolution(context):
    """The device holds the host's bytes, which tests/test_flux_volumes.py holds to the bound for every sub; one
    assertion against the analytic volumes here."""
    from graph_framework_amd.flux import FluxProfile, volumes_host
    tables = volume_model.solid_tables()
    profile = FluxProfile(context, tables, volume_model.SOLID_EDGES, **volume_model.SOLID_RANGE)
    for sub in (4, 8, 16, 32):
        twin = profile.like(context)
        twin.add_volumes(sub)
        limbs, counts = volumes_host(tables, volume_model.SOLID_EDGES, sub, **volume_model.SOLID_RANGE)
        assert twin.state().tobytes() == limbs.tobytes() and twin.counts() == counts
        twin.close()
    volume, _ = profile.volumes(32)
    check_solid(volume, 32, volume_model.solid_bound(32))
    profile.close()


def test_refusals_launch_nothing(context, tables):
    from graph_framework_amd import GfHipError
    from graph_framework_amd.flux import FluxProfile
    edges = np.linspace(0.0, 1.0, 8)
    profile = FluxProfile(context, tables, edges)
    profile.add_volumes(1)
    model = volume_model.model(tables, edges, 1)
    check(profile, model)
    for keywords, message in refusals(tables):
        with pytest.raises(GfHipError, match=message):
            profile.add_volumes(**keywords)
    check(profile, model)
    lib = context.lib
    assert lib.gfhip_flux_add_volumes(None, 1, None, 0, 1) == 1             # a null profile
    assert lib.gfhip_flux_add_volumes(profile.handle, 0, None, 0, 1) == 1
    assert "sub must be" in lib.gfhip_last_error(context.handle).decode()
    profile.add_volumes(1, (-np.inf, np.inf, 0.0, np.inf))                  # infinite bounds are allowed
    profile.close()
    for name, factor in BROKEN_MAPS:                                        # maps the other entry points keep accepting
        odd = FluxProfile(context, dict(tables, **{name: np.float64(factor*float(tables[name]))}), edges)
        with pytest.raises(GfHipError, match="dr > 0, dz > 0 and rmin >= 0"):
            odd.add_volumes(1)
        assert not odd.state().any() and odd.counts() == dict(samples=0, outside=0, skipped=0)
        odd.close()


def test_volumes_and_density(context, tables):
    from graph_framework_amd.flux import FluxProfile
    from test_gpu_flux_profile import upload
    edges = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 1.0e6, 2.0e6])            # no point of the map reaches the last cell
    sub = 3
    model = volume_model.model(tables, edges, sub)
    assert model.units[5] == 0 and all(model.units[:5])
    columns = [np.linspace(1.2, 2.2, 64), np.zeros(64), np.linspace(-0.5, 0.5, 64), np.linspace(1.0, 2.0, 64)]
    profile = FluxProfile(context, tables, edges)
    profile.add(*upload(context, "density", columns), 64)
    power = flux_model.Profile(tables, edges).add(*columns)
    assert sum(total != 0 for total in power.units) >= 3

    volume, counts = profile.volumes(sub)
    same_bits(volume, model.bins()*(2.0*np.pi))
    assert counts == model.counts and volume[5] == 0.0
    assert profile.counts() == power.counts                                 # the twin took the points, not the profile
    assert profile.state().tobytes() == power.state().tobytes()
    density = profile.density(64.0, sub)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = profile.read(64.0)/volume
    assert np.isnan(density[5]) and np.isnan(want[5])
    same_bits(density[:5], want[:5])
    window = (1.5, 2.0, -0.25, 0.25)
    windowed, _ = profile.volumes(sub, window)
    same_bits(windowed, volume_model.model(tables, edges, sub, window).bins()*(2.0*np.pi))
    assert (windowed[:4] == 0.0).any() and (windowed[:4] > 0.0).any()       # the window leaves cells with power empty
    with np.errstate(divide="ignore", invalid="ignore"):
        same_bits(profile.density(1.0, sub, window), np.where(windowed == 0.0, np.nan, profile.read()/windowed))
    profile.close()


RAYS = 264


def test_flux_deposition_writes_the_density(tmp_path, tables):
    """flux_deposition over a small written result0.nc: with density=True volume, density, sub and window in flux_bins.nc;
    without it the bytes write_flux_bins gives for the six positional arguments and the counts."""
    import sys
    from conftest import ROOT
    from graph_framework_amd import Context
    from graph_framework_amd.absorption import bin_power, run_absorption
    from graph_framework_amd.flux import FluxProfile, flux_deposition
    from graph_framework_amd.output import RAY_VARIABLES, ResultFile, write_flux_bins
    from test_deposition import _hdf5_reader
    from test_gpu_one_pass import golden_records
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    records = golden_records()
    saved = records.shape[0]
    path = str(tmp_path / "result0.nc")
    trace = ResultFile(path, RAYS)
    for name, _ in RAY_VARIABLES:
        trace.create_variable(name)
    column = {k: i for i, k in enumerate(STATE + ("residual",))}
    for r in range(saved):
        trace.write({name: records[r, column[key]] for name, key in RAY_VARIABLES})
    trace.close()
    run_absorption(path, saved - 1)
    bin_power(path, saved - 1)

    edges = np.linspace(0.0, 1.0, 17)
    psi0, span = flux_model.default_range(tables)
    for _ in range(3):                                                      # a dataset's header holds the second it was created in
        bins, counts = flux_deposition(str(tmp_path), 1, tables, 16, 0.0, 1.0)
        write_flux_bins(str(tmp_path / "today.nc"), bins, edges, psi0, span, "s", **counts)
        if int(os.path.getmtime(str(tmp_path / "flux_bins.nc"))) == int(os.path.getmtime(str(tmp_path / "today.nc"))):
            break
    assert open(str(tmp_path / "flux_bins.nc"), "rb").read() == open(str(tmp_path / "today.nc"), "rb").read()

    window = (1.0, 2.4, -1.0, 1.0)
    again, counts_again = flux_deposition(str(tmp_path), 1, tables, 16, 0.0, 1.0, density=True, sub=2, window=window)
    same_bits(again, bins)
    assert counts_again == counts
    volume = volume_model.model(tables, edges, 2, window).bins()*(2.0*np.pi)
    written = H5File(str(tmp_path / "flux_bins.nc"))
    same_bits(written.read("bins"), bins)
    same_bits(written.read("volume"), volume)
    with np.errstate(divide="ignore", invalid="ignore"):
        same_bits(written.read("density"), np.where(volume == 0.0, np.nan, bins/volume))
    written.close()
    assert (volume > 0.0).sum() >= 8 and bins.sum() > 0.0
    lib = _hdf5_reader()
    file = lib.H5Fopen(str(tmp_path / "flux_bins.nc").encode(), 0, 0)
    attribute = lib.H5Aopen(file, b"sub", 0)
    value = ctypes.c_int64()
    assert attribute >= 0 and lib.H5Aread(attribute, ctypes.c_int64.in_dll(lib, "H5T_NATIVE_INT64_g").value, ctypes.byref(value)) >= 0
    assert value.value == 2
    lib.H5Aclose(attribute)
    attribute = lib.H5Aopen(file, b"window", 0)
    four = (ctypes.c_double*4)()
    assert attribute >= 0 and lib.H5Aread(attribute, ctypes.c_int64.in_dll(lib, "H5T_NATIVE_DOUBLE_g").value, four) >= 0
    assert tuple(four) == window
    lib.H5Aclose(attribute)
    lib.H5Fclose(file)
