"""Flux volumes on the host (gfhip_flux_volumes_host): the quadrature of include/gf_hip.h against the numpy model of
tests/flux_volume_model.py byte for byte, and against two yardsticks that need no other code: rational arithmetic for
the whole map and an analytic solid of revolution.

The two tolerances are derived, not measured.  Whole map: the midpoint rule is exact for the integrand R, so the sum
differs from (rmax^2 - rmin^2)(zmax - zmin)/2 only by roundings: three in R, three in the area, one in w and the final
one, a relative 8 x 2^-53 (the sum has positive terms only).  Measured: 0.08 x 2^-53.  The solid: see
flux_volume_model.solid_bound; measured errors 0.35 (sub 4) to 0.03 (sub 32) m^3 against bounds 5.5 to 0.6."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN

import flux_model
import flux_volume_model as volume_model
from test_deposition import rounded


@pytest.fixture(scope="module")
def built():
    from graph_framework_amd import build
    build.build_library()


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(os.path.join(GOLDEN, "efit_tables.npz")))


def edges_on_labels(tables, sub, sqrt_label):
    """Eight edges among the labels of the quadrature's own points: some points sit exactly on an edge."""
    _, _, r, z, _ = volume_model.points(tables, sub)
    labels = flux_model.label(tables, r, np.zeros(r.size), z, sqrt_label=sqrt_label)
    finite = np.unique(labels[(labels > 0.2) & (labels < 0.8)])
    edges = finite[np.linspace(0, finite.size - 1, 8).astype(int)]
    assert np.isin(edges, labels).all() and (np.diff(edges) > 0.0).all()
    return edges


def edge_sets(tables, sub, sqrt_label):
    return [np.linspace(0.0, 1.0, cells + 1) for cells in (1, 7, 256, 257)] + [edges_on_labels(tables, sub, sqrt_label)]


def read(limbs):
    """What FluxProfile.read() gives for a canonical state: every cell's exact sum, rounded once."""
    return np.array([rounded(sum(int(limb) << (32*k) for k, limb in enumerate(cell))) for cell in limbs])


def check(got, model):
    limbs, counts = got
    assert counts == model.counts
    assert limbs.tobytes() == model.state().tobytes()


@pytest.mark.parametrize("sqrt_label", [False, True], ids=["s", "sqrt_s"])
@pytest.mark.parametrize("sub", [1, 2, 3])
def test_host_bytes_equal_the_model(built, tables, sub, sqrt_label):
    from graph_framework_amd.flux import volumes_host
    for edges in edge_sets(tables, sub, sqrt_label):
        model = volume_model.model(tables, edges, sub, sqrt_label=sqrt_label)
        assert model.counts["samples"] == 64*64*sub*sub and model.counts["skipped"] == 0 and any(model.units)
        check(volumes_host(tables, edges, sub, sqrt_label=sqrt_label), model)


def test_host_pieces_add_up(built, tables):
    """Any split of the point range gives the whole's numbers: the pieces' exact sums and counters added."""
    from graph_framework_amd.flux import volumes_host
    edges = np.linspace(0.0, 1.0, 8)
    sub = 3
    total = volume_model.total_points(tables, sub)
    whole = volume_model.model(tables, edges, sub)
    cuts = [0, 1, 64, 4163, 64*sub*100 + 91, total]                        # the last cut in the middle of a gz row
    pieces = flux_model.Profile(tables, edges)
    for low, high in zip(cuts[:-1], cuts[1:]):
        limbs, counts = volumes_host(tables, edges, sub, first=low, count=high - low)
        check((limbs, counts), volume_model.model(tables, edges, sub, first=low, count=high - low))
        volume_model.deposit(pieces, tables, sub, first=low, count=high - low)
    assert pieces.units == whole.units and pieces.counts == whole.counts
    limbs, counts = volumes_host(tables, edges, sub, first=77, count=0)     # nothing
    assert not limbs.any() and counts == dict(samples=0, outside=0, skipped=0)


def test_host_window(built, tables):
    from graph_framework_amd.flux import volumes_host
    edges = np.linspace(0.0, 1.0, 8)
    sub = 2
    _, _, r, z, _ = volume_model.points(tables, sub)
    columns, rows = np.unique(r), np.unique(z)
    window = (columns[20], columns[90], rows[7], rows[100])                 # lo on a generated coordinate: in; hi on one: out
    model = volume_model.model(tables, edges, sub, window)
    inside = volume_model.in_window(window, r, z)
    assert inside.sum() == 70*93 and inside[r == columns[20]].any() and not inside[r == columns[90]].any()
    assert inside[z == rows[7]].any() and not inside[z == rows[100]].any()
    check(volumes_host(tables, edges, sub, window), model)
    whole = volume_model.model(tables, edges, sub)
    assert model.units != whole.units
    check(volumes_host(tables, edges, sub, volume_model.WHOLE), whole)      # +-inf is no window
    off = volumes_host(tables, edges, sub, (100.0, 101.0, -1.0, 1.0))
    assert not off[0].any() and off[1] == dict(samples=r.size, outside=r.size, skipped=0)


def whole_map_exact(tables):
    """(rmax^2 - rmin^2)(zmax - zmin)/2 from the stored scalars, a rational number."""
    numr, numz = tables["psi_c00"].shape
    rmin, dr, zmin, dz = (Fraction(float(tables[k])) for k in ("rmin", "dr", "zmin", "dz"))
    rmax = rmin + numr*dr
    return (rmax*rmax - rmin*rmin)*(numz*dz)/2


WHOLE_MAP_EDGES = np.array([-1.0e300, 1.0e300])


def check_whole_map(tables, value, counts):
    assert counts["outside"] == 0 and counts["samples"] > 0                 # every point has a label
    exact = whole_map_exact(tables)
    error = abs(Fraction(float(value)) - exact)/exact
    print("whole map: relative error %.3f x 2^-53" % float(error*2**53))
    assert error <= Fraction(8, 2**53)


@pytest.mark.parametrize("sub", [1, 3, 8])
def test_host_whole_map_identity(built, tables, sub):
    from graph_framework_amd.flux import volumes_host
    limbs, counts = volumes_host(tables, WHOLE_MAP_EDGES, sub)
    check_whole_map(tables, read(limbs)[0], counts)


def check_solid(volume, sub, bound):
    error = np.abs(volume - volume_model.solid_exact())
    print("solid, sub %d: errors %s, bounds %s" % (sub, error, bound))
    assert (error <= bound).all()


def test_host_solid_of_revolution(built):
    from graph_framework_amd.flux import volumes_host
    tables = volume_model.solid_tables()
    bounds = {}
    for sub in (4, 8, 16, 32):
        limbs, counts = volumes_host(tables, volume_model.SOLID_EDGES, sub, **volume_model.SOLID_RANGE)
        check((limbs, counts), volume_model.model(tables, volume_model.SOLID_EDGES, sub, **volume_model.SOLID_RANGE))
        bounds[sub] = volume_model.solid_bound(sub)
        check_solid(read(limbs)*(2.0*np.pi), sub, bounds[sub])
    assert (bounds[32] < bounds[4]).all()


def refusals(tables):
    """(keywords of volumes_host beside tables and edges, part of the message) of every call that must be refused."""
    total = volume_model.total_points(tables, 2)
    nan = np.nan
    cases = [(dict(sub=0), "sub must be"), (dict(sub=257), "sub must be"),
             (dict(sub=2, first=0, count=total + 1), "count exceeds"), (dict(sub=2, first=total, count=1), "count exceeds"),
             (dict(sub=2, first=2**64 - 1, count=2), "count exceeds")]
    for window in ((nan, 2.0, 0.0, 1.0), (1.0, nan, 0.0, 1.0), (1.0, 2.0, nan, 1.0), (1.0, 2.0, 0.0, nan),
                   (2.0, 2.0, 0.0, 1.0), (2.0, 1.0, 0.0, 1.0), (1.0, 2.0, 1.0, 1.0), (1.0, 2.0, 1.0, -np.inf)):
        cases.append((dict(sub=2, window=window), "window"))
    return cases


BROKEN_MAPS = (("dr", -1.0), ("dz", -1.0), ("rmin", -1.0))                  # times the fixture's value


def test_host_refusals(built, tables):
    from graph_framework_amd import GfHipError, _lib
    from graph_framework_amd.flux import flux_map, volumes_host
    edges = np.linspace(0.0, 1.0, 8)
    for keywords, message in refusals(tables):
        with pytest.raises(GfHipError, match=message):
            volumes_host(tables, edges, **keywords)
    for name, factor in BROKEN_MAPS:
        with pytest.raises(GfHipError, match="dr > 0, dz > 0 and rmin >= 0"):
            volumes_host(dict(tables, **{name: np.float64(factor*float(tables[name]))}), edges, 2)
    with pytest.raises(GfHipError, match="strictly increasing"):
        volumes_host(tables, [0.0, 1.0, 1.0], 2)
    lib = _lib.load()
    given, keep = flux_map(tables)
    limbs, counters = np.zeros((7, 67), dtype=np.int64), np.zeros(3, dtype=np.uint64)
    arguments = [ctypes.byref(given), edges.ctypes.data, 7, 2, None, 0, 16, limbs.ctypes.data, counters.ctypes.data]
    for missing in (0, 1, 7, 8):
        broken = list(arguments)
        broken[missing] = None
        assert lib.gfhip_flux_volumes_host(*broken) == 1 and "needs a map" in lib.gfhip_last_error(None).decode()
    assert not limbs.any() and not counters.any()                           # the refused calls wrote nothing
    assert lib.gfhip_flux_volumes_host(*arguments) == 0 and counters[0] == 16
    assert lib.gfhip_flux_volumes_host(*arguments) == 0 and counters[0] == 32          # added to


def test_flux_bins_file_with_volumes(tmp_path):
    """write_flux_bins with volume and density: two more f8 variables on ns, sub and window as global attributes; without
    them the bytes of the file as it was."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    from graph_framework_amd.output import write_flux_bins
    from test_deposition import _hdf5_reader
    bins = np.array([0.5, 5e-324, -3.0, 0.0])
    edges = np.linspace(0.0, 1.0, 5)**2
    volume = np.array([2.5, 7.0, 0.0, 11.0])
    density = np.array([0.2, 0.0, np.nan, 0.0])
    counts = dict(samples=9, outside=1, skipped=0)
    plain, again, full = (str(tmp_path / name) for name in ("plain.nc", "again.nc", "full.nc"))
    for _ in range(3):                                                      # a dataset's header holds the second it was created in
        write_flux_bins(plain, bins, edges, 0.125, 0.5, "s", **counts)
        write_flux_bins(again, bins, edges, 0.125, 0.5, "s", volume=None, density=None, sub=None, window=None, **counts)
        if int(os.path.getmtime(plain)) == int(os.path.getmtime(again)):
            break
    assert open(plain, "rb").read() == open(again, "rb").read()
    for window, stored in ((None, volume_model.WHOLE), ((1.0, 2.0, -0.5, np.inf), (1.0, 2.0, -0.5, np.inf))):
        write_flux_bins(full, bins, edges, 0.125, 0.5, "s", volume=volume, density=density, sub=12, window=window, **counts)
        f = H5File(full)
        for name, want in (("bins", bins), ("sbins", edges), ("volume", volume), ("density", density)):
            got = f.read(name)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
        f.close()
        lib = _hdf5_reader()
        file = lib.H5Fopen(full.encode(), 0, 0)
        attribute = lib.H5Aopen(file, b"sub", 0)
        value = ctypes.c_int64()
        assert attribute >= 0 and lib.H5Aread(attribute, ctypes.c_int64.in_dll(lib, "H5T_NATIVE_INT64_g").value, ctypes.byref(value)) >= 0
        assert value.value == 12
        lib.H5Aclose(attribute)
        attribute = lib.H5Aopen(file, b"window", 0)
        four = (ctypes.c_double*4)()
        assert attribute >= 0 and lib.H5Aread(attribute, ctypes.c_int64.in_dll(lib, "H5T_NATIVE_DOUBLE_g").value, four) >= 0
        assert tuple(four) == tuple(stored)
        lib.H5Aclose(attribute)
        lib.H5Fclose(file)
    with pytest.raises(ValueError):
        write_flux_bins(full, bins, edges, 0.125, 0.5, "s", volume=volume)
    with pytest.raises(ValueError):
        write_flux_bins(full, bins, edges, 0.125, 0.5, "s", volume=volume, density=density)
