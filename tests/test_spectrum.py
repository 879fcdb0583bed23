"""The field direction and the parallel refractive index N (csrc/flux_label.hpp) on the host: gfhip_spectrum_npar_host
against the numpy model of tests/spectrum_model.py bit for bit; the model's field against the reference-held gold
(tests/golden/efit_gold.npz, Mathematica's bx, by, bz on a 51 x 101 grid at y = 0); and spectrum_bins.nc's layout.

The tolerance of the second comparison is DESIGN section 10's: the gold is held to what an 80-bit evaluation of the same
polynomial gives (`noise`: how far the spline itself is from the gold), plus 4 x the distance of the fp64 evaluation from
the 80-bit one (two fp64 evaluations, the model's and any other, each err by about that much), all as a share of |B|.
Measured on the 5000 of the gold's 51 x 101 grid points that the contract's inside test keeps: 80 bits against the gold
3.157e-8, fp64 against 80 bits 1.403e-8, the fp64 model against the gold 4.243e-8 (bound 8.770e-8; 4.08e-8 T in the worst
component); the 1e-6 guard band of the cell test left out 1 and 1 points for 16 and 64 cells."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

import flux_model
import spectrum_model
from test_flux_label import lifted, planted, same_bits


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


def waves(n, seed):
    """Seeded (kx, ky, kz, w): wave vectors of either sign over a few decades, frequencies around the CLI beam's."""
    rng = np.random.default_rng(seed)
    k = rng.normal(size=(3, n))*10.0**rng.uniform(-1.0, 3.0, n)
    w = rng.uniform(0.5, 2.0, n)*1.0e11*rng.choice([-1.0, 1.0], n)
    return k[0], k[1], k[2], w


def golden_samples(golden, seed=5):
    x, y, z = lifted(golden, seed)
    return (x, y, z) + waves(x.size, seed + 1)


def planted_samples(tables):
    """The rim points of test_flux_label.planted with ordinary waves, and one good point with every input in turn made
    +-0, NaN or +-inf; w = +-0 and k = 0 among them."""
    x, y, z = planted(tables)
    kx, ky, kz, w = waves(x.size, 11)
    rows = [np.stack([x, y, z, kx, ky, kz, w], axis=1)]
    good = np.array([float(tables["rmin"]) + 30.25*float(tables["dr"]), 0.3, float(tables["zmin"]) + 20.5*float(tables["dz"]),
                     12.0, -7.0, 3.0, 2.5e11])
    for column in range(7):
        for value in (0.0, -0.0, np.nan, np.inf, -np.inf):
            row = good.copy()
            row[column] = value
            rows.append(row[None, :])
    still = good.copy()
    still[3:6] = 0.0                                                        # k = 0: N = +-0
    rows.append(still[None, :])
    rows.append(good[None, :])
    return tuple(np.ascontiguousarray(c) for c in np.concatenate(rows).T)


def host_equals_model(tables, columns, **options):
    from graph_framework_amd.spectrum import npar_host
    want = spectrum_model.label_npar(tables, *columns, **options)
    got = npar_host(tables, *columns, **options)
    same_bits(got[0], want[0])
    same_bits(got[1], want[1])
    return want


@pytest.mark.parametrize("sqrt_label", [False, True], ids=["s", "sqrt_s"])
def test_host_equals_the_model_on_the_golden_points(built, tables, golden, sqrt_label):
    columns = golden_samples(golden)
    label, npar = host_equals_model(tables, columns, sqrt_label=sqrt_label)
    same_bits(label, np.where(np.isnan(label), np.nan, flux_model.label(tables, *columns[:3], sqrt_label=sqrt_label)))
    assert label.size == 4096 and np.isfinite(npar).all() and (np.abs(npar) > 1.0e-6).sum() > 4000
    host_equals_model(tables, columns, psi0=0.25, span=-0.125, c=1.0, sqrt_label=sqrt_label)


def test_host_equals_the_model_on_planted_points(built, tables):
    columns = planted_samples(tables)
    label, npar = host_equals_model(tables, columns)
    assert np.isfinite(label[[0, 1]]).all() and np.isfinite(npar[[0, 1]]).all()                 # tr exactly 0
    assert np.isnan(label[2]) and np.isnan(npar[2])                                             # tr exactly numr
    inputs = 23 + 5*np.arange(7)[:, None] + np.arange(5)[None, :]           # [column][0.0, -0.0, nan, inf, -inf]
    assert np.isinf(npar[inputs[6, :2]]).all() and npar[inputs[6, 0]] == -npar[inputs[6, 1]]    # w = +-0
    assert np.isfinite(label[inputs[6]]).all() and (npar[inputs[6, 3:]] == 0.0).all()           # w = +-inf: N = +-0
    assert not np.isfinite(npar[inputs[:6, 2:].reshape(-1)]).any()          # a NaN or an infinity in a coordinate or in k
    assert np.isnan(npar[inputs[:6, 2]]).all() and np.isnan(npar[inputs[:3, 2:].reshape(-1)]).all()
    assert np.isnan(npar[inputs[6, 2]])
    assert np.isnan(label[inputs[0, :2]]).all()                             # x = 0 leaves R = |y| below the map
    assert np.isfinite(npar[inputs[1:6, :2].reshape(-1)]).all()             # a zero coordinate or component is a number
    assert npar[-2] == 0.0 and np.isfinite(npar[-1]) and npar[-1] != 0.0    # k = 0


def test_host_equals_the_model_on_planted_maps(built, tables, golden):
    columns = tuple(c[:512] for c in golden_samples(golden, seed=9))
    numr, numz = tables["psi_c00"].shape

    origin = dict(tables, rmin=np.float64(0.0))                             # x = y = 0 is on this map: R = 0 divides
    at_origin = [c.copy() for c in columns]
    at_origin[0][:8] = (0.0, -0.0, 0.0, -0.0, 0.0, 0.0, 1.0e-200, 0.0)
    at_origin[1][:8] = (0.0, 0.0, -0.0, -0.0, 0.0, 0.0, 1.0e-200, 0.0)
    at_origin[3][4:6] = 0.0                                                 # ... 0/0 where k is along z
    at_origin[4][4:6] = 0.0
    label, npar = host_equals_model(origin, at_origin)
    assert np.isfinite(label[:8]).all() and not np.isfinite(npar[:8]).any()

    zero = dict(tables, **{name: np.zeros((numr, numz)) for name in flux_model.TABLE_NAMES})
    zero.update({name: np.zeros_like(tables[name]) for name in spectrum_model.FPOL_NAMES})
    label, npar = host_equals_model(zero, columns)                          # a zero field: 0/0
    assert np.isnan(npar).all() and (np.isfinite(label) | np.isnan(flux_model.label(tables, *columns[:3]))).all()

    psi = flux_model.psi_rz(tables, *flux_model.normalised(tables, np.hypot(columns[0], columns[1]), columns[2]))
    numpsi = tables["fpol_c0"].size
    for psimin, dpsi, interval in ((psi.max() + 1.0, tables["dpsi"], 0),    # psi below the table: q = 0
                                   (psi.min() - 1.0, tables["dpsi"]*1.0e-3, numpsi - 1),          # above: q = numpsi - 1
                                   (psi.min() - 1.0, -tables["dpsi"], 0)):
        moved = dict(tables, psimin=np.float64(psimin), dpsi=np.float64(dpsi))
        _, npar = host_equals_model(moved, columns, psi0=0.1, span=0.5)
        r = np.hypot(columns[0], columns[1])
        tr, tz = flux_model.normalised(tables, r, columns[2])
        assert (spectrum_model.field_rz(moved, r, tr, tz)[5] == interval).all() and np.isfinite(npar).all()

    broken = dict(tables, psi_c21=tables["psi_c21"].copy())                 # an infinite coefficient: tp is NaN, q = 0
    i, j = (int(v[0]) for v in flux_model.normalised(tables, np.hypot(columns[0][:1], columns[1][:1]), columns[2][:1]))
    broken["psi_c21"][i, j] = np.inf
    label, npar = host_equals_model(broken, columns)
    assert np.isnan(npar[0]) and np.isfinite(npar).sum() > 400


def test_host_refuses_a_broken_field(built, tables):
    from graph_framework_amd import GfHipError, _lib
    from graph_framework_amd.flux import flux_map
    from graph_framework_amd.spectrum import npar_host, spectrum_field
    point = tuple(np.array([v]) for v in (1.9, 0.0, 0.0, 1.0, 2.0, 3.0, 1.0e11))
    for broken, message in ((dict(dpsi=np.float64(0.0)), "dpsi and c"), (dict(dpsi=np.float64(np.nan)), "dpsi and c"),
                            (dict(psimin=np.float64(np.inf)), "psimin"), (dict(dr=np.float64(0.0)), "dr, dz and span")):
        with pytest.raises(GfHipError, match=message):
            npar_host(dict(tables, **broken), *point, psi0=0.1, span=0.5)
    for c in (0.0, np.inf, np.nan):
        with pytest.raises(GfHipError, match="dpsi and c"):
            npar_host(tables, *point, c=c)
    lib = _lib.load()
    out = np.zeros(2)
    pointers = (ctypes.c_void_p*7)(*[c.ctypes.data for c in point])

    def call(given, field, columns=pointers, label=out[:1].ctypes.data, npar=out[1:].ctypes.data):
        return lib.gfhip_spectrum_npar_host(ctypes.byref(given) if given is not None else None,
                                            ctypes.byref(field) if field is not None else None, columns, 1, label, npar)

    given, keep = flux_map(tables)
    field, keep_field = spectrum_field(tables)
    assert call(given, field) == 0 and np.isfinite(out).all()
    for name, value, message in (("numpsi", 0, "numpsi"), ("numpsi", 1 << 31, "numpsi"), ("reserved", 1, "reserved")):
        field, keep_field = spectrum_field(tables)
        setattr(field, name, value)
        assert call(given, field) == 1 and message in lib.gfhip_last_error(None).decode()
    field, keep_field = spectrum_field(tables)
    field.fpol[2] = None
    assert call(given, field) == 1 and "four fpol tables" in lib.gfhip_last_error(None).decode()
    field, keep_field = spectrum_field(tables)
    for arguments in ((None, field), (given, None), (given, field, None), (given, field, pointers, None),
                      (given, field, pointers, out.ctypes.data, None)):
        assert call(*arguments) == 1 and "needs a map" in lib.gfhip_last_error(None).decode()
    missing = (ctypes.c_void_p*7)(*[c.ctypes.data for c in point])
    missing[4] = None
    assert call(given, field, missing) == 1
    given.flags = 4
    assert call(given, field) == 1 and "unknown flag" in lib.gfhip_last_error(None).decode()


@pytest.fixture(scope="module")
def gold_field(tables):
    """The gold's grid points inside the map, at y = 0: (r, z, tr, tz, B of the gold as three columns, |B|)."""
    g = np.load(os.path.join(GOLDEN, "efit_gold.npz"))
    numr, numz = tables["psi_c00"].shape
    r, z = (v.ravel() for v in np.meshgrid(g["r_grid"], g["z_grid"], indexing="ij"))
    tr, tz = flux_model.normalised(tables, r, z)
    inside = (tr >= 0.0) & (tr < numr) & (tz >= 0.0) & (tz < numz)
    b = np.stack([g[name].ravel()[inside].astype(np.longdouble) for name in ("bx_grid", "by_grid", "bz_grid")])
    return r[inside], z[inside], tr[inside], tz[inside], b, np.sqrt((b*b).sum(axis=0))


def field_of(tables, r, tr, tz, dtype):
    """(B_R, B_phi, B_z) = (gZ, fpol, -gR)/R in `dtype` arithmetic."""
    _, gr, gz, f, _, _ = spectrum_model.field_rz(tables, r, tr, tz, dtype)
    return np.stack([gz/r.astype(dtype), f/r.astype(dtype), -gr/r.astype(dtype)])


def test_the_contract_lies_within_the_margin_of_the_gold_field(tables, gold_field):
    r, z, tr, tz, gold, size = gold_field
    assert r.size == 5000                                                   # of the 51 x 101: tr < 64 and tz < 64
    wide = field_of(tables, r, tr, tz, np.longdouble)
    model = field_of(tables, r, tr, tz, np.float64)
    noise = float((np.abs(wide - gold)/size).max())
    rounding = float((np.abs(model - wide)/size).max())
    distance = float((np.abs(model - gold)/size).max())
    print("80 bits against the gold %.3e, fp64 against 80 bits %.3e, the model against the gold %.3e of |B| (bound %.3e); "
          "worst component %.3e T" % (noise, rounding, distance, noise + 4.0*rounding, float(np.abs(model - gold).max())))
    assert 1.0e-9 < noise < 1.0e-6 and rounding < noise
    assert distance <= noise + 4.0*rounding


@pytest.mark.parametrize("cells", [16, 64])
def test_npar_falls_into_the_gold_fields_cells(built, tables, gold_field, cells):
    """Seeded |N| <= 1.2 with w = c = 1: a point whose N from the gold field (80 bits) is 1e-6 of the range or more from
    every edge must land in the gold's cell; the band may leave out 1 % of the points at the most."""
    from graph_framework_amd.spectrum import npar_host
    r, z, tr, tz, gold, size = gold_field
    rng = np.random.default_rng(cells)
    k = rng.normal(size=(3, r.size))
    k *= rng.uniform(0.0, 1.2, r.size)/np.sqrt((k*k).sum(axis=0))
    reference = ((k.astype(np.longdouble)*gold).sum(axis=0)/size).astype(np.float64)
    assert np.abs(reference).max() <= 1.2
    edges = np.linspace(-1.25, 1.25, cells + 1)
    clear = np.abs(reference[:, None] - edges[None, :]).min(axis=1) >= 1.0e-6*2.5
    dropped = int((~clear).sum())
    want = flux_model.cells_of(edges, reference)
    columns = (r, np.zeros(r.size), z, k[0], k[1], k[2], np.ones(r.size))
    model = spectrum_model.label_npar(tables, *columns, c=1.0)[1]
    print("%d cells: the band leaves out %d of %d points; N of the contract against the gold's %.3e"
          % (cells, dropped, clear.size, float(np.abs(model - reference).max())))
    assert dropped <= clear.size//100 and (want >= 0).all() and np.unique(want).size >= 3*cells//4
    for npar in (model, npar_host(tables, *columns, c=1.0)[1]):
        got = flux_model.cells_of(edges, npar)
        assert np.array_equal(got[clear], want[clear]), np.flatnonzero(clear & (got != want))[:5]


def test_default_c_is_the_dispersion_relations(tables):
    from graph_framework_amd import spectrum
    assert spectrum.C == spectrum_model.C and abs(spectrum.C - 299792458.0) < 1.0
    field, keep = spectrum.spectrum_field(tables)
    assert field.c == spectrum.C and field.numpsi == 138 and field.reserved == 0


def test_spectrum_bins_file_has_its_layout(tmp_path):
    """output.write_spectrum_bins: dimensions ns, nsp, nn, nnp; f8 bins(ns, nn), sbins(nsp), nbins(nnp); the counters,
    psi0, span, c and the label kind as global attributes; NetCDF-4's on-disk conventions as flux_bins.nc."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    from graph_framework_amd.output import write_spectrum_bins
    from test_deposition import _hdf5_reader
    bins = np.array([[0.5, 5e-324, -3.0], [0.0, 7.25, 1.0e300]])
    sbins = np.array([0.0, 0.25, 1.0])
    nbins = np.array([-1.0, -0.5, 0.125, 1.0])
    counts = dict(samples=(1 << 33) + 5, outside=11, skipped=2)
    path = str(tmp_path / "spectrum_bins.nc")
    write_spectrum_bins(path, bins, sbins, nbins, 0.125, 0.53, "sqrt_s", 299792458.5, **counts)
    f = H5File(path)
    for name, want in (("bins", bins), ("sbins", sbins), ("nbins", nbins)):
        got = f.read(name)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
    assert [f.read(name).shape for name in ("ns", "nsp", "nn", "nnp")] == [(2,), (3,), (3,), (4,)]
    f.close()
    with pytest.raises(ValueError):
        write_spectrum_bins(path + "x", bins.reshape(-1), sbins, nbins, 0.0, 1.0)

    lib = _hdf5_reader()
    file = lib.H5Fopen(path.encode(), 0, 0)
    assert file >= 0 and lib.H5Aexists(file, b"_NCProperties") > 0
    int64 = ctypes.c_int64.in_dll(lib, "H5T_NATIVE_INT64_g").value
    double = ctypes.c_int64.in_dll(lib, "H5T_NATIVE_DOUBLE_g").value
    for name, want in counts.items():
        attribute = lib.H5Aopen(file, name.encode(), 0)
        value = ctypes.c_int64()
        assert attribute >= 0 and lib.H5Aread(attribute, int64, ctypes.byref(value)) >= 0 and value.value == want, name
        lib.H5Aclose(attribute)
    for name, want in (("psi0", 0.125), ("span", 0.53), ("c", 299792458.5)):
        attribute = lib.H5Aopen(file, name.encode(), 0)
        value = ctypes.c_double()
        assert attribute >= 0 and lib.H5Aread(attribute, double, ctypes.byref(value)) >= 0 and value.value == want, name
        lib.H5Aclose(attribute)
    assert lib.H5Aexists(file, b"label") > 0
    for name in ("ns", "nsp", "nn", "nnp"):
        dataset = lib.H5Dopen2(file, name.encode(), 0)
        assert dataset >= 0 and lib.hl.H5DSis_scale(dataset) > 0, name
        lib.H5Dclose(dataset)
    for name, axes in (("bins", ("ns", "nn")), ("sbins", ("nsp",)), ("nbins", ("nnp",))):
        dataset = lib.H5Dopen2(file, name.encode(), 0)
        kind = lib.H5Dget_type(dataset)
        assert lib.H5Tget_class(kind) == 1 and lib.H5Tget_size(kind) == 8, name                  # H5T_FLOAT, f8
        for index, axis in enumerate(axes):
            scale = lib.H5Dopen2(file, axis.encode(), 0)
            assert lib.hl.H5DSis_attached(dataset, scale, index) > 0, (name, axis)
            lib.H5Dclose(scale)
        lib.H5Tclose(kind)
        lib.H5Dclose(dataset)
    lib.H5Fclose(file)
