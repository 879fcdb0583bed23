"""The flux label (csrc/flux_label.hpp) on the host: gfhip_flux_label_host against the numpy model of
tests/flux_model.py bit for bit, the model against the reference graph layer's psi (tests/golden/flux_golden.npz, made by
tests/golden/make_flux_golden.py through oracle/_ref/gf_ref), and flux_bins.nc's layout.

The tolerance of the second comparison: psi is evaluated as a polynomial in the GLOBAL normalised coordinates (the
tracer's own form), which fp64 conditions only to about 1e-7 of the span.  The fixture carries `noise`, the largest
distance of the reference's own fp64 psi from an 80-bit evaluation of the same polynomial; the model is another fp64
evaluation that errs by about as much, so 2 x noise is the expected worst case and the bound is 4 x noise.  Measured when
the fixture was made (4096 points): noise 3.98e-8 (7.5e-8 of the span), model against reference 5.61e-8 = 1.41 x noise,
model against 80 bits 6.48e-8; the 1e-6 guard band of the cell test left out 0, 0 and 0 points for 7, 64 and 256 cells."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

import flux_model


@pytest.fixture(scope="module")
def built():
    from graph_framework_amd import build
    build.build_library()


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(os.path.join(GOLDEN, "efit_tables.npz")))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "flux_golden.npz"))


def lifted(golden, seed=5):
    """The fixture's (r, z) as (x, y, z) at random toroidal angles.  The points on the table's lower rim (tr exactly 0)
    stay at angle 0, where sqrt(x*x + y*y) gives r back exactly: a rounding in the lift would put them off the map."""
    angle = np.random.default_rng(seed).uniform(0.0, 2.0*np.pi, golden["r"].size)
    angle[golden["r"] == golden["r"].min()] = 0.0
    return golden["r"]*np.cos(angle), golden["r"]*np.sin(angle), golden["z"].copy()


def planted(tables):
    """Points on and off the rim of the map, and coordinates that are no numbers."""
    numr, numz = tables["psi_c00"].shape
    rmin, dr, zmin, dz = (float(tables[k]) for k in ("rmin", "dr", "zmin", "dz"))
    z_mid = zmin + 20.5*dz
    r_mid = rmin + 30.25*dr
    r_top = rmin + numr*dr
    while (r_top - rmin)/dr < numr:                                         # tr exactly numr or just above: outside
        r_top = np.nextafter(r_top, np.inf)
    rows = [(rmin, 0.0, z_mid),                                             # tr exactly 0
            (0.0, -rmin, z_mid),
            (r_top, 0.0, z_mid),
            (np.nextafter(rmin, 0.0), 0.0, z_mid), (rmin + (numr + 3)*dr, 0.0, z_mid),                # off the map in r
            (r_mid, 0.0, np.nextafter(zmin, -np.inf)), (r_mid, 0.0, zmin + (numz + 1)*dz),            # ... and in z
            (r_mid, 0.0, zmin), (r_mid, 0.0, np.nextafter(zmin + numz*dz, -np.inf)),
            (0.0, 0.0, z_mid), (-0.0, -0.0, z_mid), (-0.0, r_mid, z_mid), (r_mid, -0.0, -0.0), (-r_mid, 0.0, 0.0),
            (np.nan, 0.0, z_mid), (r_mid, np.nan, z_mid), (r_mid, 0.0, np.nan),
            (np.inf, 0.0, z_mid), (r_mid, -np.inf, z_mid), (r_mid, 0.0, np.inf), (r_mid, 0.0, -np.inf),
            (1.0e200, 1.0e200, z_mid), (1.0e-200, 1.0e-200, z_mid)]
    return tuple(np.array(column) for column in zip(*rows))


def all_points(tables, golden):
    return tuple(np.concatenate(pair) for pair in zip(lifted(golden), planted(tables)))


def same_bits(got, want):
    assert got.shape == want.shape
    differ = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert differ.size == 0, (differ[:5], got[differ[:5]], want[differ[:5]])


def test_planted_points_are_where_they_should_be(tables):
    x, y, z = planted(tables)
    label = flux_model.label(tables, x, y, z)
    assert np.isfinite(label[[0, 1, 7, 11, 12, 13]]).all()                  # on the rim and inside
    assert np.isnan(label[[2, 3, 4, 5, 6, 9, 10]]).all() and np.isnan(label[14:]).all()
    numr = tables["psi_c00"].shape[0]
    tr, _ = flux_model.normalised(tables, np.hypot(x[:3], y[:3]), z[:3])
    assert tr[0] == 0.0 and tr[1] == 0.0 and tr[2] >= numr and tr[2] - numr < 1.0e-9


@pytest.mark.parametrize("sqrt_label", [False, True], ids=["s", "sqrt_s"])
def test_host_labels_equal_the_model_bit_for_bit(built, tables, golden, sqrt_label):
    from graph_framework_amd.flux import label_host
    x, y, z = all_points(tables, golden)
    want = flux_model.label(tables, x, y, z, sqrt_label=sqrt_label)
    same_bits(label_host(tables, x, y, z, sqrt_label=sqrt_label), want)
    assert np.isfinite(want).sum() > (3000 if sqrt_label else 4096)         # sqrt: NaN outside the axis value's contour
    psi0, span = 0.25, -0.125                                               # the caller's range, span of either sign
    same_bits(label_host(tables, x, y, z, psi0, span, sqrt_label), flux_model.label(tables, x, y, z, psi0, span, sqrt_label))


def test_host_labels_refuse_a_broken_map(built, tables):
    from graph_framework_amd import GfHipError
    from graph_framework_amd.flux import flux_map, label_host
    from graph_framework_amd import _lib
    point = (np.array([1.5]), np.array([0.0]), np.array([0.0]))
    for broken, message in ((dict(span=0.0), "span"), (dict(span=np.inf), "span"), (dict(psi0=np.nan), "psi0")):
        with pytest.raises(GfHipError, match=message):
            label_host(tables, *point, **dict(dict(psi0=0.1, span=0.5), **broken))
    for name in ("dr", "dz"):
        for value in (0.0, np.nan):
            with pytest.raises(GfHipError, match="dr, dz and span"):
                label_host(dict(tables, **{name: np.float64(value)}), *point)
    lib = _lib.load()
    out = np.zeros(1)
    for flags, reserved, message in ((4, 0, "unknown flag"), (0, 1, "reserved")):
        given, keep = flux_map(tables, flags=flags)
        given.reserved = reserved
        assert lib.gfhip_flux_label_host(ctypes.byref(given), *[c.ctypes.data for c in point], 1, out.ctypes.data) == 1
        assert message in lib.gfhip_last_error(None).decode()
    assert lib.gfhip_flux_label_host(None, *[c.ctypes.data for c in point], 1, out.ctypes.data) == 1
    given, keep = flux_map(tables)
    assert lib.gfhip_flux_label_host(ctypes.byref(given), None, point[1].ctypes.data, point[2].ctypes.data, 1, out.ctypes.data) == 1
    given.numr = 0
    assert lib.gfhip_flux_label_host(ctypes.byref(given), *[c.ctypes.data for c in point], 1, out.ctypes.data) == 1
    assert "numr" in lib.gfhip_last_error(None).decode()


def test_fixture_is_what_its_maker_describes(tables, golden):
    numr, numz = tables["psi_c00"].shape
    r, z = golden["r"], golden["z"]
    assert r.shape == z.shape == golden["psi"].shape == (4096,)
    tr, tz = flux_model.normalised(tables, r, z)
    assert (tr >= 0).all() and (tr < numr).all() and (tz >= 0).all() and (tz < numz).all()
    assert (np.abs(tr - np.rint(tr)) < 1e-9).sum() >= 190 and (np.abs(tz - np.rint(tz)) < 1e-9).sum() >= 190
    assert len(set(zip(tr.astype(int), tz.astype(int)))) > 2000                                 # all over the table
    assert 1.0e-9 < float(golden["noise"]) < 1.0e-6


def test_model_lies_within_four_noises_of_the_reference(tables, golden):
    psi = flux_model.psi_rz(tables, *flux_model.normalised(tables, golden["r"], golden["z"]))
    distance = float(np.abs(psi - golden["psi"]).max())
    noise = float(golden["noise"])
    print("model against reference %.3e, noise %.3e, ratio %.2f" % (distance, noise, distance/noise))
    assert distance <= 4.0*noise
    assert distance == float(golden["model_distance"])                      # what DESIGN.md quotes


@pytest.mark.parametrize("cells", [7, 64, 256])
def test_labels_fall_into_the_reference_cells(built, tables, golden, cells):
    """psi0 = psimin, span = dpsi*137; a point whose reference label is 1e-6 or more from every edge must land in the
    reference's cell; the band may leave out 0.1 % of the points at the most."""
    from graph_framework_amd.flux import label_host
    psi0, span = float(tables["psimin"]), float(tables["dpsi"])*137
    assert (psi0, span) == flux_model.default_range(tables)
    edges = np.linspace(0.0, 1.0, cells + 1)
    reference = (golden["psi"] - psi0)/span
    clear = np.abs(reference[:, None] - edges[None, :]).min(axis=1) >= 1.0e-6
    dropped = int((~clear).sum())
    print("%d cells: the band leaves out %d of %d points" % (cells, dropped, clear.size))
    assert dropped <= clear.size//1000
    assert dropped == int(golden["band_dropped"][list(golden["band_cells"]).index(cells)])
    want = flux_model.cells_of(edges, reference)
    assert (want >= 0).sum() > 500                                          # the unit interval holds a good part of the table
    x, y, z = lifted(golden, seed=cells)
    for labels in (flux_model.label(tables, x, y, z), label_host(tables, x, y, z)):
        got = flux_model.cells_of(edges, labels)
        assert np.array_equal(got[clear], want[clear]), np.flatnonzero(clear & (got != want))[:5]


def test_flux_bins_file_has_its_layout(tmp_path):
    """output.write_flux_bins: dimensions ns, nsp; f8 bins(ns), sbins(nsp); the counters, psi0, span and the label kind as
    global attributes; NetCDF-4's on-disk conventions as bins.nc."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    from graph_framework_amd.output import write_flux_bins
    from test_deposition import _hdf5_reader
    bins = np.array([0.5, 5e-324, -3.0, 0.0, 7.25])
    edges = np.linspace(0.0, 1.0, 6)**2
    counts = dict(samples=(1 << 33) + 5, outside=11, skipped=2)
    path = str(tmp_path / "flux_bins.nc")
    write_flux_bins(path, bins, edges, 0.125, 0.53, "sqrt_s", **counts)
    f = H5File(path)
    for name, want in (("bins", bins), ("sbins", edges)):
        got = f.read(name)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
    assert f.read("ns").shape == (5,) and f.read("nsp").shape == (6,)
    f.close()

    lib = _hdf5_reader()
    hid = ctypes.c_int64
    file = lib.H5Fopen(path.encode(), 0, 0)
    assert file >= 0 and lib.H5Aexists(file, b"_NCProperties") > 0
    int64 = hid.in_dll(lib, "H5T_NATIVE_INT64_g").value
    double = hid.in_dll(lib, "H5T_NATIVE_DOUBLE_g").value
    for name, want in counts.items():
        attribute = lib.H5Aopen(file, name.encode(), 0)
        value = ctypes.c_int64()
        assert attribute >= 0 and lib.H5Aread(attribute, int64, ctypes.byref(value)) >= 0 and value.value == want, name
        lib.H5Aclose(attribute)
    for name, want in (("psi0", 0.125), ("span", 0.53)):
        attribute = lib.H5Aopen(file, name.encode(), 0)
        value = ctypes.c_double()
        assert attribute >= 0 and lib.H5Aread(attribute, double, ctypes.byref(value)) >= 0 and value.value == want, name
        lib.H5Aclose(attribute)
    attribute = lib.H5Aopen(file, b"label", 0)
    assert attribute >= 0
    lib.H5Aget_type.restype = hid
    lib.H5Aget_type.argtypes = [hid]
    kind = lib.H5Aget_type(attribute)
    text = ctypes.create_string_buffer(lib.H5Tget_size(kind))
    assert lib.H5Aread(attribute, kind, text) >= 0 and text.value == b"sqrt_s"
    lib.H5Tclose(kind)
    lib.H5Aclose(attribute)
    for dimid, name in enumerate(("ns", "nsp")):
        dataset = lib.H5Dopen2(file, name.encode(), 0)
        assert dataset >= 0 and lib.hl.H5DSis_scale(dataset) > 0, name
        lib.H5Dclose(dataset)
    for name, axis in (("bins", "ns"), ("sbins", "nsp")):
        dataset = lib.H5Dopen2(file, name.encode(), 0)
        scale = lib.H5Dopen2(file, axis.encode(), 0)
        kind = lib.H5Dget_type(dataset)
        assert lib.H5Tget_class(kind) == 1 and lib.H5Tget_size(kind) == 8, name                  # H5T_FLOAT, f8
        assert lib.hl.H5DSis_attached(dataset, scale, 0) > 0, name
        lib.H5Tclose(kind)
        lib.H5Dclose(scale)
        lib.H5Dclose(dataset)
    lib.H5Fclose(file)
