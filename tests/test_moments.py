"""The moments of a particle per flux surface (csrc/flux_label.hpp's moments_of, csrc/moments_host.hpp) on the host:
gfhip_moments_values_host and gfhip_moments_add_host against the numpy model of tests/moments_model.py bit for bit and
byte for byte, fp64 and fp32 columns; the model against its own lines in 80 bits; the plain C++ pieces under the
sanitizers (tests/moments_host_check.cpp, a program of its own); moment_bins.nc's layout; means, totals and densities
against the model's rationals.  No GPU."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import flux_model
import moments_model
import phase_model
from test_deposition import UNIT, rounded
from test_flux_label import same_bits
from test_phase import aligned_particles, planted_particles, random_particles

#  The seed of the random particles of the deposit tests: with it the model meets the condition that
#  test_add_host_equals_the_model_byte_for_byte checks before it compares anything.
SEED = 3


@pytest.fixture(scope="module")
def built():
    from graph_framework_amd import build
    build.build_library()


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(os.path.join(GOLDEN, "efit_tables.npz")))


def edges_of(ns):
    """Label edges inside the range the map's labels cover (0 to 1.008): particles fall off both ends."""
    return np.linspace(0.02, 0.98, ns + 1)


def extras(tables):
    """One good particle, then: u = 0; gamma = 0; gamma = +inf; a NaN in each column in turn; the grid point nearest the
    magnetic axis (the smallest (psi - psi0)/span of a 257 x 257 grid over the map) and its four neighbours."""
    rmin, dr, zmin, dz = (float(tables[k]) for k in ("rmin", "dr", "zmin", "dz"))
    numr, numz = tables["psi_c00"].shape
    good = np.array([rmin + 30.25*dr, 0.3, zmin + 20.5*dz, 0.4, -1.25, 0.75, 1.8])
    rows = [good.copy() for _ in range(4)]
    rows[1][3:6] = 0.0
    rows[2][6] = 0.0
    rows[3][6] = np.inf
    for column in range(7):
        row = good.copy()
        row[column] = np.nan
        rows.append(row)
    r, z = np.meshgrid(rmin + dr*numr*(np.arange(257) + 0.5)/257.0, zmin + dz*numz*(np.arange(257) + 0.5)/257.0, indexing="ij")
    s = flux_model.label(tables, r.reshape(-1), np.zeros(r.size), z.reshape(-1))
    at = int(np.nanargmin(s))
    for shift_r, shift_z in ((0.0, 0.0), (1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0)):
        row = good.copy()
        radius = r.reshape(-1)[at] + shift_r*dr*numr/257.0
        row[0], row[1], row[2] = radius*np.cos(0.7), radius*np.sin(0.7), z.reshape(-1)[at] + shift_z*dz*numz/257.0
        rows.append(row)
    return tuple(np.ascontiguousarray(c) for c in np.array(rows).T)


def host_equals_model(tables, columns, **options):
    """values_host on fp64 columns and on their fp32 roundings against the model fed the same values."""
    from graph_framework_amd.moments import values_host
    out = []
    for dtype in (np.float64, np.float32):
        given = [np.asarray(c).astype(dtype) for c in columns[:7]]
        want = moments_model.label_values(tables, *given, **options)
        got = values_host(tables, given, **options)
        assert got[1].shape == (given[0].size, 4)
        same_bits(got[0], want[0])
        for k in range(4):
            same_bits(got[1][:, k], want[1][:, k])
        out.append(want)
    return out[0]


@pytest.mark.parametrize("sqrt_label", [False, True], ids=["s", "sqrt_s"])
def test_values_equal_the_model_on_random_aligned_and_planted_particles(built, tables, sqrt_label):
    columns = random_particles(tables, 4099, SEED)
    label, values = host_equals_model(tables, columns, sqrt_label=sqrt_label)
    outside = np.isnan(label)
    assert 800 < outside.sum() < 1300 and np.isnan(values[outside]).all() and np.isfinite(values[~outside]).all()
    assert (values[~outside, 0] == 1.0).all() and (np.abs(values[~outside, 1]) < 1.0).all() and (values[~outside, 2] > 0.0).all()
    assert (values[~outside, 3] >= 0.0).all() and (values[~outside, 1] > 0.1).sum() > 300 and (values[~outside, 1] < -0.1).sum() > 300
    host_equals_model(tables, columns, psi0=0.25, span=-0.125, sqrt_label=sqrt_label)
    host_equals_model(tables, aligned_particles(tables, 2048, 4), sqrt_label=sqrt_label)
    host_equals_model(tables, planted_particles(tables), sqrt_label=sqrt_label)


def test_values_equal_the_model_on_the_planted_extras(built, tables):
    from graph_framework_amd.moments import values_host
    columns = extras(tables)
    label, values = host_equals_model(tables, columns)
    assert np.isfinite(label[0]) and np.isfinite(values[0]).all() and values[0, 3] > 0.0
    assert list(values[1]) == [1.0, 0.0, 0.8, 0.0]                          # u = 0: not a NaN anywhere
    assert np.isinf(values[2, 1]) and values[2, 2] == -1.0 and np.isfinite(values[2, 3])      # gamma = 0 with u != 0: upar/0, no number either
    assert values[3, 1] == 0.0 and values[3, 2] == np.inf                   # gamma = inf
    assert np.isnan(label[4:7]).all() and np.isnan(values[4:7]).all()       # a position that is no number
    assert np.isfinite(label[7:11]).all() and np.isnan(values[7:10, 1]).all() and np.isnan(values[7:10, 3]).all()
    assert np.isnan(values[10, 1]) and np.isnan(values[10, 2]) and np.isfinite(values[10, 3])            # gamma NaN: rad has no gamma
    axis = host_equals_model(tables, columns, sqrt_label=True)[0][11:]
    plain = label[11:]
    print("labels at and around the axis: s = %r, sqrt(s) = %r" % (list(plain), list(axis)))
    assert (np.abs(plain) < 2.0e-3).all()                                   # on the axis: s is 0 up to the grid's step
    assert (np.isnan(axis) == (plain < 0.0)).all()                          # sqrt of a negative s is no label
    with pytest.raises(ValueError):
        values_host(tables, columns[:6])
    with pytest.raises(ValueError):
        values_host(tables, [c[:k] for k, c in zip((5, 5, 5, 5, 5, 5, 4), columns)])


def test_gamma_zero_with_u_zero_is_zero_over_zero(built, tables):
    columns = [c[:1].copy() for c in extras(tables)]
    for c in columns[3:7]:
        c[:] = 0.0
    _, values = host_equals_model(tables, columns)
    assert np.isnan(values[0, 1]) and values[0, 2] == -1.0 and values[0, 3] == 0.0


def test_a_negative_difference_is_clamped_to_plus_zero(built, tables):
    """u along B: uu - upup cancels and comes out below zero in part of the cases; rad is then +0, bit for bit."""
    from graph_framework_amd.moments import values_host
    columns = aligned_particles(tables, 2048, 4)[:7]
    label, values, inside, parts = moments_model.label_values(tables, *columns, parts=True)
    negative = parts["raw"] < 0.0
    print("uu - upup is negative in %d of %d aligned particles, down to %.3e of uu"
          % (int(negative.sum()), negative.size, float((parts["raw"]/parts["uu"]).min())))
    assert inside.all() and negative.sum() >= 1
    got = values_host(tables, columns)[1]
    same_bits(got[:, 3], values[:, 3])
    assert (got[negative, 3].view(np.uint64) == 0).all()                    # +0.0, not -0.0 and not a small negative number
    assert (got[:, 3] >= 0.0).all() and (got[~negative, 3] > 0.0).any()


def seeded_weights(n, dtype, inside):
    """Weights of both signs over the type's exponent range with zeros of both signs, and a NaN and +-inf on particles
    that lie in a cell."""
    rng = np.random.default_rng(21)
    span = 100 if dtype == np.float32 else 900
    weight = (rng.uniform(-1.0, 1.0, n)*2.0**rng.integers(-span, span, n).astype(np.float64)).astype(dtype)
    weight[rng.random(n) < 0.05] = 0.0
    weight[rng.random(n) < 0.02] = -0.0
    weight[inside[5]], weight[inside[70]], weight[inside[71]] = np.nan, np.inf, -np.inf
    return weight


def deposit_columns(tables, dtype):
    """The random particles with the planted ones of test_phase and the extras above among them."""
    parts = [random_particles(tables, 4099, SEED), planted_particles(tables), extras(tables)]
    return [np.concatenate(c).astype(dtype) for c in zip(*parts)]


@pytest.mark.parametrize("kind", ["f64", "f32"])
@pytest.mark.parametrize("ns", [3, 64])
def test_add_host_equals_the_model_byte_for_byte(built, tables, ns, kind):
    from graph_framework_amd.moments import add_host
    dtype = {"f64": np.float64, "f32": np.float32}[kind]
    columns = deposit_columns(tables, dtype)
    n = columns[0].size
    edges = edges_of(ns)
    plain = moments_model.Moments(tables, edges).add(*columns)
    surface = plain.weighted(*columns)[0]
    weight = seeded_weights(n, dtype, np.flatnonzero(surface >= 0))
    weighted = moments_model.Moments(tables, edges).add(*columns, weight=weight)
#  The condition, on the model alone (seed 3).
    for model in (plain, weighted):
        counts = model.counts
        assert counts["samples"] - counts["outside"] >= n//2 and counts["skipped"] >= 3 and counts["outside"] >= n//5
    if ns == 3:
        assert (plain.bins()[:, 0] > 0.0).all() and (plain.bins()[:, 2] > 0.0).all()
    assert any(total < 0 for total in weighted.units) and any(total > 0 for total in weighted.units)
    for given, first in ((None, plain), (weight, weighted)):
        model = moments_model.Moments(tables, edges)
        limbs, counters = None, None
        for piece in (slice(0, 1500), slice(1500, 1501), slice(1501, n)):  # three adds in a row, into the same arrays
            part = [c[piece] for c in columns]
            model.add(*part, weight=None if given is None else given[piece])
            limbs, counters = add_host(tables, edges, part, None if given is None else given[piece], limbs, counters)
            assert limbs.tobytes() == model.state().tobytes()
            assert dict(zip(("samples", "outside", "skipped"), (int(c) for c in counters))) == model.counts
        assert limbs.tobytes() == first.state().tobytes() and model.counts == first.counts


def test_a_particle_deposits_all_four_or_none(built, tables):
    """A finite weight and gamma = 0: vpar is not finite, so none of the particle's four cells moves and `skipped` goes
    up by one; the same particle with gamma = 1.8 moves all four."""
    from graph_framework_amd.moments import add_host
    columns = [c[:1].copy() for c in extras(tables)]
    edges = edges_of(3)
    limbs, counters = add_host(tables, edges, columns, np.array([2.5]))
    surface = int(moments_model.Moments(tables, edges).weighted(*columns)[0][0])
    assert surface >= 0 and list(counters) == [1, 0, 0]
    assert [bool(limbs[surface, k].any()) for k in range(4)] == [True]*4 and not np.delete(limbs, surface, axis=0).any()
    before = limbs.copy()
    columns[6][0] = 0.0
    add_host(tables, edges, columns, np.array([2.5]), limbs, counters)
    assert limbs.tobytes() == before.tobytes() and list(counters) == [2, 0, 1]
    model = moments_model.Moments(tables, edges).add(*columns, weight=np.array([2.5]))
    assert model.counts == dict(samples=1, outside=0, skipped=1) and not any(model.units)


def test_moments_lie_within_their_rounding_bounds_of_the_80_bit_lines(tables):
    """The moments of the fp64 model against the same lines in numpy.longdouble (80 bits, unit roundoff 2^-64).  Both
    evaluations start from the same fp64 x, y, z, u, gamma, R, tr and tz; they differ in the field (gR, gZ, f), which each
    evaluates in its own arithmetic, and in the roundings of the lines from there on.  w below is 2^-53 + 2^-64, the fp64
    lines' roundoff and the 80-bit lines' own; `moved` is |dB|/|B| of the two fields, known point by point, as in
    test_xi_lies_within_its_rounding_bound_of_the_80_bit_lines; 1.01 covers the higher orders.

    upar = num/den = u . b^.  The field: a change dB moves b^ by at most 2 |dB|/|B|, so upar by 2 moved |u|.  The lines:
    |num~ - num| <= 6 w T with T the sum of the absolute values of num's terms (test_phase.py); den has three roundings
    under the root, halved, and the root's own, under 3 w relative; the quotient adds w:
        E = |upar~ - upar| <= 2 moved |u| + 1.01 w (6 T/den + 4 |upar|).
    vpar = upar/gamma, gamma the same number in both, one more rounding:   |vpar~ - vpar| <= E/gamma + 1.01 w |vpar|.
    kin = gamma - 1.0, one rounding:                                        |kin~ - kin| <= w |kin|.
    rad = perp*bsq.  uu is a sum of three squares, every term positive and through at most three roundings: 3 w uu.
    upup = upar*upar: 2 |upar| E + w upup.  The difference adds w |uu - upup| <= w uu, and upup <= uu, so
        |perp~ - perp| <= 5 w uu + 2 |upar| E                               (the clamp is 1-Lipschitz).
    bsq = bsum/rr: bsum as uu (3 w), rr one rounding, the quotient one, and |B|^2 moves by 2 moved relative:
        |bsq~ - bsq| <= (5 w + 2 moved) bsq.
    The product adds w rad, and perp <= uu:
        |rad~ - rad| <= bsq (5 w uu + 2 |upar| E) + rad (6 w + 2 moved) <= uu bsq (1.01*11 w + 2 moved) + 1.01*2 |upar| E bsq.
    This bound is absolute in units of uu*bsq: for u along B perp cancels and rad has no relative accuracy at all."""
    columns = [np.concatenate(pair) for pair in zip(random_particles(tables, 4099, SEED, off=0.0),
                                                     aligned_particles(tables, 2048, 4)[:7])]
    x, y, z, ux, uy, uz, gamma = columns
    wide = np.longdouble
    assert np.finfo(wide).nmant == 63
    with np.errstate(invalid="ignore"):
        inside, r, gr, gz, f, _ = phase_model.field_at(tables, x, y, z)
        _, _, wgr, wgz, wf, _ = phase_model.field_at(tables, x, y, z, wide)
        x, y, r, ux, uy, uz, gamma = (v[inside] for v in (x, y, r, ux, uy, uz, gamma))
        model = moments_model.moments_from(x, y, r, ux, uy, uz, gamma, gr, gz, f)
        exact, parts = moments_model.moments_from(x, y, r, ux, uy, uz, gamma, wgr, wgz, wf, wide, parts=True)
    assert model.dtype == np.float64 and exact.dtype == wide and model.shape[0] > 6000
    X, Y, R, UX, UY, UZ, G = (v.astype(wide) for v in (x, y, r, ux, uy, uz, gamma))
    size = np.sqrt(wgz*wgz + wf*wf + wgr*wgr)
    moved = np.sqrt((gz - wgz)**2 + (f - wf)**2 + (gr - wgr)**2)/size
    terms = ((abs(UX*X) + abs(UY*Y))*abs(wgz) + (abs(UY*X) + abs(UX*Y))*abs(wf))/R + abs(UZ*wgr)
    uu, bsq, upar = parts["uu"], parts["bsq"], abs(parts["upar"])
    w = wide(2.0)**-53 + wide(2.0)**-64
    more = wide(1.01)
    e_upar = 2.0*moved*np.sqrt(uu) + more*w*(6.0*terms/size + 4.0*upar)
    bounds = {1: e_upar/G + more*w*abs(exact[:, 1]), 2: w*abs(exact[:, 2]),
              3: uu*bsq*(more*11.0*w + 2.0*moved) + more*2.0*upar*e_upar*bsq}
    scales = {1: np.ones(uu.shape, dtype=wide), 2: np.ones(uu.shape, dtype=wide), 3: uu*bsq}
    assert (model[:, 0] == 1.0).all() and (exact[:, 0] == 1.0).all()
    for k in (1, 2, 3):
        error = abs(model[:, k].astype(wide) - exact[:, k])
        worst = int(np.argmax(error/bounds[k]))
        print("%s, fp64 against 80 bits: largest error %.3e, largest bound %.3e (both in units of %s), largest share of the bound %.3f"
              % (moments_model.MOMENTS[k], float((error/scales[k]).max()), float((bounds[k]/scales[k]).max()),
                 "uu*bsq" if k == 3 else "1", float((error/bounds[k]).max())))
        assert (error <= bounds[k]).all(), (k, worst, float(error[worst]), float(bounds[k][worst]))
        assert float((bounds[k]/scales[k]).max()) < 1.0e-6                  # the bound says something


def test_the_plain_cpp_pieces_under_the_sanitizers(tmp_path):
    """tests/moments_host_check.cpp: moments_host.hpp over planted particles and every edge's neighbours, as float and as
    double, with and without weights, against a plain restatement; built with -fsanitize=address,undefined and run as a
    child process."""
    binary = str(tmp_path/"moments_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "graph_framework_amd", "csrc"), "-o", binary,
                           os.path.join(ROOT, "tests", "moments_host_check.cpp")])
    out = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0
    last = out.stdout.split()
    assert last[-4] == "cases" and int(last[-3]) > 1000 and last[-2:] == ["failures", "0"]


def test_moment_bins_file_has_its_layout(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    from graph_framework_amd.output import write_moment_bins
    bins = np.arange(2*3*4, dtype=np.float64).reshape(2, 3, 4) - 7.0
    bins[1, 2, 3] = 5e-324
    edges = np.array([0.0, 0.25, 0.5, 1.0])
    totals = np.arange(8.0).reshape(2, 4)
    counts = dict(samples=[3001, 3001], outside=[0, 2], skipped=[0, 1])
    volume = np.array([1.0, 2.0, 4.0])
    path = str(tmp_path/"moment_bins.nc")
    write_moment_bins(path, bins, edges, 0.125, 0.53, "sqrt_s", totals=totals, steps=[25, 50], volume=volume,
                      density=bins/volume[None, :, None], sub=4, **counts)
    f = H5File(path)
    for name, want in (("bins", bins), ("totals", totals), ("sbins", edges), ("steps", np.array([25.0, 50.0])),
                       ("outside", np.array([0.0, 2.0])), ("samples", np.array([3001.0, 3001.0])), ("skipped", np.array([0.0, 1.0])),
                       ("volume", volume), ("density", bins/volume[None, :, None])):
        got = f.read(name)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
    assert [f.read(name).shape for name in ("time", "ns", "nsp", "nm")] == [(2,), (3,), (4,), (4,)]
    f.close()
    raw = open(path, "rb").read()
    assert b"density,current,energy,radiation" in raw and b"normalised" in raw and b"sqrt_s" in raw
    write_moment_bins(path, bins[0], edges, 0.0, 1.0)                       # one snapshot, totals summed, no volumes
    f = H5File(path)
    assert f.read("bins").shape == (1, 3, 4) and f.read("steps").tobytes() == np.zeros(1).tobytes()
    assert f.read("totals").tobytes() == bins[0].sum(axis=0)[None].tobytes()
    f.close()
    for broken in (dict(bins=bins.reshape(-1)), dict(bins=bins[:, :, :3]), dict(sbins=edges[:3]), dict(volume=volume),
                   dict(volume=volume, density=bins), dict(totals=totals[:1]), dict(volume=volume[:2], density=bins, sub=4)):
        arguments = dict(bins=bins, sbins=edges)
        arguments.update(broken)
        with pytest.raises(ValueError):
            write_moment_bins(path + "x", arguments.pop("bins"), arguments.pop("sbins"), 0.0, 1.0, **arguments)


def test_means_and_totals_of_the_model_are_the_rationals_rounded_once(built, tables):
    """What FluxMoments.means(), totals() and densities() compute from read(), on the host's limbs: the cells' exact
    rationals from add_host's state, rounded once, against the model's; the quotients as IEEE divisions of those."""
    from graph_framework_amd.moments import add_host
    columns = deposit_columns(tables, np.float64)
    edges = edges_of(5)
    model = moments_model.Moments(tables, edges).add(*columns)
    limbs, _ = add_host(tables, edges, columns)
    exact = [[sum(int(limb) << (32*k) for k, limb in enumerate(cell)) for cell in surface] for surface in limbs]
    assert [total for surface in exact for total in surface] == model.units
    read = np.array([[rounded(total) for total in surface] for surface in exact])
    same_bits(read.reshape(-1), model.bins().reshape(-1))
    totals = np.array([rounded(sum(surface[k] for surface in exact)) for k in range(4)])
    same_bits(totals, model.totals())
    assert totals[0] == model.counts["samples"] - model.counts["outside"] - model.counts["skipped"]
    for k in (1, 2, 3):                                                     # the mean per particle: three roundings, two sums and the quotient
        ratio = Fraction(sum(surface[k] for surface in exact), UNIT)/Fraction(sum(surface[0] for surface in exact), UNIT)
        assert abs(Fraction(float(totals[k]/totals[0])) - ratio) <= abs(ratio)*(Fraction(3, 2**53) + Fraction(1, 2**100))
