"""The pitch cosine xi = (u.B)/(|u||B|) (csrc/flux_label.hpp) on the host: gfhip_phase_coordinates_host against the numpy
model of tests/phase_model.py bit for bit, fp64 and fp32 columns; the model against its own lines in 80 bits; the plain
C++ pieces under the sanitizers (tests/phase_host_check.cpp, a program of its own); pitch_edges and phase_bins.nc's
layout.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import flux_model
import phase_model
from test_flux_label import same_bits


@pytest.fixture(scope="module")
def built():
    from graph_framework_amd import build
    build.build_library()


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(os.path.join(GOLDEN, "efit_tables.npz")))


def map_box(tables):
    numr, numz = tables["psi_c00"].shape
    rmin, dr, zmin, dz = (float(tables[k]) for k in ("rmin", "dr", "zmin", "dz"))
    return rmin, rmin + numr*dr, zmin, zmin + numz*dz


def random_particles(tables, n, seed, off=0.25):
    """Seeded (x, y, z, ux, uy, uz, gamma): positions all over the map at any toroidal angle, the share `off` of them
    beyond it in R or z; momenta of either sign over three decades; gamma = sqrt(1 + u.u)."""
    rng = np.random.default_rng(seed)
    rlo, rhi, zlo, zhi = map_box(tables)
    r = rng.uniform(rlo, rhi, n)
    z = rng.uniform(zlo, zhi, n)
    away = rng.random(n) < off
    side = rng.integers(0, 4, n)
    r = np.where(away & (side == 0), rhi + rng.uniform(0.0, 1.0, n), np.where(away & (side == 1), rlo*rng.uniform(0.0, 0.99, n), r))
    z = np.where(away & (side == 2), zhi + rng.uniform(0.0, 1.0, n), np.where(away & (side == 3), zlo - rng.uniform(1e-9, 1.0, n), z))
    angle = rng.uniform(0.0, 2.0*np.pi, n)
    u = rng.normal(size=(3, n))*10.0**rng.uniform(-2.0, 1.0, n)
    gamma = np.sqrt(1.0 + (u*u).sum(axis=0))
    return r*np.cos(angle), r*np.sin(angle), z, u[0], u[1], u[2], gamma


def aligned_particles(tables, n, seed):
    """Particles inside the map with u = +-t B from the model's own field, t over three decades: xi is +-1 up to the
    rounding of its lines."""
    rng = np.random.default_rng(seed)
    rlo, rhi, zlo, zhi = map_box(tables)
    r = rng.uniform(rlo, np.nextafter(rhi, 0.0), n)
    z = rng.uniform(zlo, np.nextafter(zhi, -np.inf), n)
    angle = rng.uniform(0.0, 2.0*np.pi, n)
    x, y = r*np.cos(angle), r*np.sin(angle)
    inside, radius, gr, gz, f, _ = phase_model.field_at(tables, x, y, z)
    assert inside.sum() >= n - 2                                            # the lift may push a rim point off the map
    x, y, z, radius = x[inside], y[inside], z[inside], radius[inside]
    t = 10.0**rng.uniform(-1.0, 2.0, x.size)*np.where(np.arange(x.size) % 2 == 0, 1.0, -1.0)
    size = np.sqrt(gz*gz + f*f + gr*gr)
    ur, up, uz = t*gz/size, t*f/size, -t*gr/size                            # R B = (gZ, fpol, -gR)
    ux = (ur*x - up*y)/radius
    uy = (ur*y + up*x)/radius
    return x, y, z, ux, uy, uz, np.sqrt(1.0 + t*t), np.sign(t)


def planted_particles(tables):
    """One good particle, then: u = 0; every column in turn made NaN, +inf and -inf; gamma exactly on the first, an inner
    and the last edge of GAMMA_EDGES."""
    rmin, dr, zmin, dz = (float(tables[k]) for k in ("rmin", "dr", "zmin", "dz"))
    good = np.array([rmin + 30.25*dr, 0.3, zmin + 20.5*dz, 0.4, -1.25, 0.75, 1.8])
    rows = [good.copy()]
    still = good.copy()
    still[3:6] = 0.0
    rows.append(still)
    for column in range(7):
        for value in (np.nan, np.inf, -np.inf):
            row = good.copy()
            row[column] = value
            rows.append(row)
    for gamma in (GAMMA_EDGES[0], GAMMA_EDGES[2], GAMMA_EDGES[-1]):
        row = good.copy()
        row[6] = gamma
        rows.append(row)
    return tuple(np.ascontiguousarray(c) for c in np.array(rows).T)


GAMMA_EDGES = np.array([1.0, 1.5, 2.0, 2.5, 3.0])


def host_equals_model(tables, columns, **options):
    """coordinates_host on fp64 columns and on their fp32 roundings against the model fed the same values."""
    from graph_framework_amd.distribution import coordinates_host
    out = []
    for dtype in (np.float64, np.float32):
        given = [np.asarray(c).astype(dtype) for c in columns[:7]]
        want = phase_model.label_pitch(tables, *given[:6], **options)
        got = coordinates_host(tables, given, **options)
        same_bits(got[0], want[0])
        same_bits(got[1], want[1])
        out.append(want)
    return out[0]


@pytest.mark.parametrize("sqrt_label", [False, True], ids=["s", "sqrt_s"])
def test_host_equals_the_model_on_random_particles(built, tables, sqrt_label):
    columns = random_particles(tables, 4099, 3)
    label, xi = host_equals_model(tables, columns, sqrt_label=sqrt_label)
    outside = np.isnan(flux_model.label(tables, *columns[:3]))
    assert 800 < outside.sum() < 1300 and np.isnan(xi[outside]).all() and np.isfinite(xi[~outside]).all()
    assert (np.abs(xi[~outside]) <= 1.0).all() and (xi[~outside] > 0.5).sum() > 300 and (xi[~outside] < -0.5).sum() > 300
    host_equals_model(tables, columns, psi0=0.25, span=-0.125, sqrt_label=sqrt_label)


def test_host_equals_the_model_where_the_quotient_exceeds_one(built, tables):
    from graph_framework_amd.distribution import pitch_edges
    columns = aligned_particles(tables, 2048, 4)
    sign = columns[7]
    _, xi, raw = phase_model.label_pitch(tables, *columns[:6], unclamped=True)
    above = int((np.abs(raw) > 1.0).sum())
    print("the unclamped quotient exceeds 1 in %d of %d particles, by up to %.3e" % (above, raw.size, float(np.abs(raw).max() - 1.0)))
    assert above >= 1 and (raw > 1.0).any() and (raw < -1.0).any()
    host_equals_model(tables, columns)
    assert (np.abs(xi) <= 1.0).all() and (xi[np.abs(raw) > 1.0] == sign[np.abs(raw) > 1.0]).all()
    cell = flux_model.cells_of(pitch_edges(8), xi)
    assert (cell[sign > 0] == 7).all() and (cell[sign < 0] == 0).all()
    assert (flux_model.cells_of(np.linspace(-1.0, 1.0, 9), xi[xi == 1.0]) == -1).all() and (xi == 1.0).any()


def test_host_equals_the_model_on_planted_particles(built, tables):
    from graph_framework_amd.distribution import coordinates_host
    columns = planted_particles(tables)
    label, xi = host_equals_model(tables, columns)
    assert np.isfinite(label[0]) and -1.0 < xi[0] < 1.0 and xi[0] != 0.0
    assert np.isfinite(label[1]) and np.isnan(xi[1])                        # u = 0: 0/0
    at = 2 + 3*np.arange(7)[:, None] + np.arange(3)[None, :]                # [column][nan, inf, -inf]
    assert np.isnan(label[at[:3].reshape(-1)]).all() and np.isnan(xi[at[:3].reshape(-1)]).all()       # a position that is no number
    assert np.isfinite(label[at[3:].reshape(-1)]).all() and np.isnan(xi[at[3:6].reshape(-1)]).all()   # u: nan, or inf/inf
    same_bits(xi[at[6]], np.full(3, xi[0]))                                 # gamma takes no part in xi
    same_bits(xi[-3:], np.full(3, xi[0]))
    gamma = columns[6]
    assert list(flux_model.cells_of(GAMMA_EDGES, gamma[-3:])) == [0, 2, -1]                           # on an edge: the cell above
    assert list(flux_model.cells_of(GAMMA_EDGES, gamma[at[6]])) == [-1, -1, -1]
    with pytest.raises(ValueError):
        coordinates_host(tables, columns[:6])
    with pytest.raises(ValueError):
        coordinates_host(tables, [c[:k] for k, c in zip((5, 5, 5, 5, 5, 5, 4), columns)])


def test_xi_lies_within_its_rounding_bound_of_the_80_bit_lines(tables):
    """xi of the fp64 model against the same lines in numpy.longdouble (80 bits, unit roundoff v = 2^-64), both clamped
    (the clamp is 1-Lipschitz).  Both evaluations start from the same fp64 x, y, z, u, R, tr and tz; they differ in the
    field (gR, gZ, f), which each evaluates in its own arithmetic, and in the roundings of the lines from there on.

    The field.  xi = u^ . b^ with b^ = B/|B| and |u^| = 1; a change dB of B moves b^ by at most 2 |dB|/|B|.  dB is the
    fp64 field minus the 80-bit one, known here point by point: the same quantity the spectrum test calls `rounding` and
    takes its bound for N from, used per point instead of as a maximum.

    The lines, with unit roundoff w and T = ((|ux x| + |uy y|) |gZ| + (|uy x| + |ux y|) |f|)/R + |uz gR|, the sum of the
    absolute values of num's terms.  An input of num passes at most 6 roundings (product, a or b, times gZ or f, the sum,
    the quotient by R, the difference): |num~ - num| <= 6 w T.  den: three roundings under the root, which halves them, and
    the root's own, under 3 w relative; p likewise; the two quotients, the spectrum's num/den and the new cosine/p, add w
    each, and sqrt and quotient of p are the two roundings the spectrum's N does not have.  To first order
        |xi~ - xi| <= 6 w T/(den p) + 8 w |xi|,
    taken for w = 2^-53 and, for the 80-bit lines' own error, w = v; the factor 1.01 covers the higher orders (14 w)."""
    columns = [np.concatenate(pair) for pair in zip(random_particles(tables, 4099, 3, off=0.0)[:6],
                                                     aligned_particles(tables, 2048, 4)[:6])]
    x, y, z, ux, uy, uz = columns
    wide = np.longdouble
    assert np.finfo(wide).nmant == 63
    with np.errstate(invalid="ignore"):
        inside, r, gr, gz, f, _ = phase_model.field_at(tables, x, y, z)
        _, _, wgr, wgz, wf, _ = phase_model.field_at(tables, x, y, z, wide)
        x, y, r, ux, uy, uz = (v[inside] for v in (x, y, r, ux, uy, uz))
        model = phase_model.clamped(phase_model.quotient_from(phase_model.cosine_from(x, y, r, ux, uy, uz, gr, gz, f), ux, uy, uz))
        exact = phase_model.clamped(phase_model.quotient_from(phase_model.cosine_from(x, y, r, ux, uy, uz, wgr, wgz, wf, wide),
                                                              ux, uy, uz, wide))
    assert model.dtype == np.float64 and exact.dtype == wide and model.size > 6000
    X, Y, R, UX, UY, UZ = (v.astype(wide) for v in (x, y, r, ux, uy, uz))
    size = np.sqrt(wgz*wgz + wf*wf + wgr*wgr)
    moved = np.sqrt((gz - wgz)**2 + (f - wf)**2 + (gr - wgr)**2)/size
    terms = ((abs(UX*X) + abs(UY*Y))*abs(wgz) + (abs(UY*X) + abs(UX*Y))*abs(wf))/R + abs(UZ*wgr)
    momentum = np.sqrt(UX*UX + UY*UY + UZ*UZ)
    roundoff = wide(2.0)**-53 + wide(2.0)**-64
    bound = 2.0*moved + wide(1.01)*roundoff*(6.0*terms/(size*momentum) + 8.0*abs(exact))
    error = abs(model.astype(wide) - exact)
    worst = int(np.argmax(error/bound))
    print("xi, fp64 against 80 bits: largest error %.3e (bound there %.3e), largest share of the bound %.3f; the field moves "
          "by up to %.3e of |B|" % (float(error.max()), float(bound[np.argmax(error)]), float((error/bound).max()), float(moved.max())))
    assert (error <= bound).all(), (worst, float(error[worst]), float(bound[worst]))
    assert float(bound.max()) < 1.0e-6                                      # the bound says something


def test_pitch_edges_hold_one():
    from graph_framework_amd.distribution import pitch_edges
    for n in (1, 4, 7, 8):
        edges = pitch_edges(n)
        want = np.linspace(-1.0, 1.0, n + 1)
        assert edges.size == n + 1 and edges[-1] == np.nextafter(1.0, 2.0) and edges[0] == -1.0
        same_bits(edges[:-1], want[:-1])
        assert list(flux_model.cells_of(edges, np.array([-1.0, 1.0, np.nextafter(1.0, 2.0)]))) == [0, n - 1, -1]


def test_the_plain_cpp_pieces_under_the_sanitizers(tmp_path):
    """tests/phase_host_check.cpp: pitch_of and a host cell finder (cell_deposit.hpp's rule) over planted inputs, built
    with -fsanitize=address,undefined and run as a child process."""
    binary = str(tmp_path/"phase_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "graph_framework_amd", "csrc"), "-o", binary,
                           os.path.join(ROOT, "tests", "phase_host_check.cpp")])
    out = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0
    last = out.stdout.split()
    assert last[-4] == "cases" and int(last[-3]) > 1000 and last[-2:] == ["failures", "0"]


def test_phase_bins_file_has_its_layout(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    from graph_framework_amd.output import write_phase_bins
    bins = np.arange(2*2*3*4, dtype=np.float64).reshape(2, 2, 3, 4)
    bins[1, 1, 2, 3] = 5e-324
    edges = (np.array([0.0, 0.25, 1.0]), np.array([-1.0, -0.5, 0.125, 1.0]), GAMMA_EDGES)
    counts = dict(samples=[3001, 3001], outside=[0, 2], skipped=[0, 1])
    path = str(tmp_path/"phase_bins.nc")
    write_phase_bins(path, bins, *edges, 0.125, 0.53, "sqrt_s", steps=[25, 50], **counts)
    f = H5File(path)
    for name, want in (("bins", bins), ("sbins", edges[0]), ("pbins", edges[1]), ("gbins", edges[2]),
                       ("steps", np.array([25.0, 50.0])), ("outside", np.array([0.0, 2.0])), ("samples", np.array([3001.0, 3001.0])),
                       ("skipped", np.array([0.0, 1.0]))):
        got = f.read(name)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
    assert [f.read(name).shape for name in ("time", "ns", "nsp", "np", "npp", "ng", "ngp")] == [(2,), (2,), (3,), (3,), (4,), (4,), (5,)]
    f.close()
    write_phase_bins(path, bins[0], *edges, 0.0, 1.0)                       # one snapshot
    f = H5File(path)
    assert f.read("bins").shape == (1, 2, 3, 4) and f.read("steps").tobytes() == np.zeros(1).tobytes()
    f.close()
    with pytest.raises(ValueError):
        write_phase_bins(path + "x", bins.reshape(-1), *edges, 0.0, 1.0)
