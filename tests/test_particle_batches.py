"""Batches of particles on the host: gfhip_moments_add_particles_host and gfhip_phase_add_particles_host against the numpy
model of tests/particle_batch_model.py byte for byte on the limbs and exact on the counters; the slabs summed against the
plain deposit; batches.ratio_error_of against its formula in rational arithmetic, within a bound derived from its
operation count, and its statistical sense on a numpy model; the plain C++ under the sanitizers
(tests/particle_batches_check.cpp, a program of its own); the new variables of moment_bins.nc and phase_bins.nc.  No GPU.

The sizes.  G in {1, 2, 3, 16, 64}, n in {1, 63, 64, 65, 64G - 1, 64G, 64G + 1, 4099}, first in {0, 1, 63, 65, 2^40 + 5},
fp32 and fp64, with and without weights, ns = 3 and 64 for the moments and 3 x 2 x 2 for the distribution.  Every G meets
every n, every type and both kinds of weights; `first` goes round its five values along the (G, n) pairs, shifted by the
type and the weights, and the 4099-particle case of G = 3 and G = 16 meets all five, so that every first meets every G,
whole and partial first chunks included."""
import decimal
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import moments_model
import particle_batch_model as model_of
import phase_model
from test_moments import edges_of, seeded_weights
from test_phase import random_particles

BATCHES = (1, 2, 3, 16, 64)
FIRSTS = (0, 1, 63, 65, 2**40 + 5)
PARTICLES = 4099
GAMMA_EDGES = np.array([1.0, 2.0, 50.0])


@pytest.fixture(scope="module")
def built():
    from graph_framework_amd import build
    build.build_library()


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(os.path.join(GOLDEN, "efit_tables.npz")))


def counts_of(batch_count):
    return sorted({1, 63, 64, 65, 64*batch_count - 1, 64*batch_count, 64*batch_count + 1, PARTICLES})


def cases(shift):
    """(G, n, first): see the module's docstring."""
    out = []
    for i, batch_count in enumerate(BATCHES):
        for j, n in enumerate(counts_of(batch_count)):
            out.append((batch_count, n, FIRSTS[(i + j + shift) % len(FIRSTS)]))
        if batch_count in (3, 16):
            out += [(batch_count, PARTICLES, first) for first in FIRSTS]
    return sorted(set(out))


def particles_of(tables, dtype):
    """test_phase's random particles (a quarter off the map), gamma = 0 planted on the first, the 40th and the 41st, and
    on every 97th after them, of those that lie inside ns = 3's edges: the moments skip them."""
    columns = [np.array(c) for c in random_particles(tables, PARTICLES, 3)]
    surface = moments_model.Moments(tables, edges_of(3)).weighted(*columns)[0]
    inside = np.flatnonzero(surface >= 0)
    columns[6][inside[[0, 40, 41]]] = 0.0
    columns[6][inside[100::97]] = 0.0
    return [c.astype(dtype) for c in columns], inside


def weights_of(dtype, inside):
    return seeded_weights(PARTICLES, dtype, inside)


def counters_of(counters):
    return dict(zip(("samples", "outside", "skipped"), (int(c) for c in counters)))


def test_the_model_fills_every_batch_and_leaves_empty_slabs(tables):
    """The conditions on the model alone: 4099 particles in 16 batches deposit in every batch and skip at least three;
    one particle in 64 batches leaves 63 slabs empty."""
    columns, inside = particles_of(tables, np.float64)
    for weight in (None, weights_of(np.float64, inside)):
        full = model_of.moments(tables, edges_of(3), 16).add(columns, 0, weight)
        assert (full.deposited() >= 1).all() and full.counts["skipped"] >= 3 and full.counts["outside"] >= PARTICLES//5
        assert all(any(model.units) for model in full.models)
        spread = model_of.phase(tables, edges_of(3), pitch(), GAMMA_EDGES, 16).add(columns, 0, weight)
        assert (spread.deposited() >= 1).all()
    one = model_of.moments(tables, edges_of(3), 64).add([c[inside[1]:inside[1] + 1] for c in columns], 0)
    assert one.deposited().sum() == 1 and sum(1 for m in one.models if not any(m.units)) == 63
    assert sum(1 for slab in one.state() if not slab.any()) == 63


def pitch():
    from graph_framework_amd.distribution import pitch_edges
    return pitch_edges(2)


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("kind", ["f64", "f32"])
@pytest.mark.parametrize("ns", [3, 64])
def test_moments_add_particles_host_equals_the_model_byte_for_byte(built, tables, ns, kind, weighted):
    from graph_framework_amd.moments import add_host, add_particles_host
    dtype = {"f64": np.float64, "f32": np.float32}[kind]
    columns, inside = particles_of(tables, dtype)
    weight = weights_of(dtype, inside) if weighted else None
    edges = edges_of(ns)
    plain = {}
    for batch_count, n, first in cases(2*(kind == "f32") + weighted):
        part = [c[:n] for c in columns]
        w = None if weight is None else weight[:n]
        want = model_of.moments(tables, edges, batch_count).add(part, first, w)
        limbs, counters = add_particles_host(tables, edges, batch_count, part, first, w)
        assert limbs.shape == (batch_count, ns, 4, 67) and limbs.tobytes() == want.state().tobytes(), (batch_count, n, first)
        assert counters_of(counters) == want.counts, (batch_count, n, first)
        if n not in plain:
            plain[n] = add_host(tables, edges, part, w)
        assert model_of.merged_limbs(limbs).tobytes() == plain[n][0].tobytes() and list(counters) == list(plain[n][1])
        if n == PARTICLES:
            assert want.counts["skipped"] >= 3
    #  Two adds into the same arrays are one.
    limbs, counters = add_particles_host(tables, edges, 3, [c[:100] for c in columns], 65, None if weight is None else weight[:100])
    add_particles_host(tables, edges, 3, [c[100:] for c in columns], 165, None if weight is None else weight[100:], limbs, counters)
    whole = add_particles_host(tables, edges, 3, columns, 65, weight)
    assert limbs.tobytes() == whole[0].tobytes() and list(counters) == list(whole[1])


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_phase_add_particles_host_equals_the_model_byte_for_byte(built, tables, kind, weighted):
    """The plain deposit of the distribution on the host is the one-batch deposit, held to phase_model.Phase itself."""
    from graph_framework_amd.distribution import add_particles_host
    dtype = {"f64": np.float64, "f32": np.float32}[kind]
    columns, inside = particles_of(tables, dtype)
    weight = weights_of(dtype, inside) if weighted else None
    axes = (edges_of(3), pitch(), GAMMA_EDGES)
    plain = {}
    for batch_count, n, first in cases(1 + 2*(kind == "f32") + weighted):
        part = [c[:n] for c in columns]
        w = None if weight is None else weight[:n]
        want = model_of.phase(tables, *axes, batch_count).add(part, first, w)
        limbs, counters = add_particles_host(tables, *axes, batch_count, part, first, w)
        assert limbs.shape == (batch_count, 3, 2, 2, 67) and limbs.tobytes() == want.state().tobytes(), (batch_count, n, first)
        assert counters_of(counters) == want.counts, (batch_count, n, first)
        if n not in plain:
            one = add_particles_host(tables, *axes, 1, part, 0, w)
            reference = phase_model.Phase(tables, *axes).add(*part, weight=w)
            assert one[0][0].tobytes() == reference.state().tobytes() and counters_of(one[1]) == reference.counts
            plain[n] = one
        assert model_of.merged_limbs(limbs).tobytes() == plain[n][0][0].tobytes() and list(counters) == list(plain[n][1])
        if n == PARTICLES and weighted:
            assert want.counts["skipped"] >= 3


def test_the_host_calls_refuse_what_they_cannot_take(built, tables):
    from graph_framework_amd.backend import GfHipError
    from graph_framework_amd import distribution, moments
    columns, _ = particles_of(tables, np.float64)
    part = [c[:10] for c in columns]
    for batch_count in (0, 257):
        with pytest.raises(GfHipError):
            moments.add_particles_host(tables, edges_of(3), batch_count, part, 0)
        with pytest.raises(GfHipError):
            distribution.add_particles_host(tables, edges_of(3), pitch(), GAMMA_EDGES, batch_count, part, 0)
    with pytest.raises(GfHipError):
        moments.add_particles_host(tables, edges_of(3), 4, part, 2**64 - 5)
    with pytest.raises(GfHipError):
        distribution.add_particles_host(tables, edges_of(3), pitch(), GAMMA_EDGES, 4, part, 2**64 - 5)
    with pytest.raises(ValueError):
        moments.add_particles_host(tables, edges_of(3), 4, part, 0, limbs=np.zeros((3, 3, 4, 67), dtype=np.int64),
                                   counters=np.zeros(3, dtype=np.uint64))
    limbs, counters = moments.add_particles_host(tables, edges_of(3), 4, part, 2**64 - 11)                  # the last ten there are
    assert int(counters[0]) == 10


#  Planted batch sums (numerator, denominator) of one cell.
PLANTED = {
    "equal batches": ([3.0, 3.5, 2.75, 3.25], [1.0, 1.0, 1.0, 1.0]),
    "unequal batches": ([1.0e3, -2.5, 7.125e-3, 40.0, 0.1], [900.0, 3.0, 0.007, 41.5, 0.3]),
    "an empty batch": ([3.0, 0.0, 2.75, 3.25], [1.0, 0.0, 1.0, 1.5]),
    "a numerator of zero": ([0.0, 0.2, 0.0, -0.1], [2.0, 1.0, 3.0, 1.0]),
    "sixty-four batches": (list(np.random.default_rng(5).normal(10.0, 3.0, 64)), list(np.random.default_rng(6).uniform(50.0, 70.0, 64))),
    "wide range": ([1.0e100, 3.0e99, -2.0e100], [1.0e-30, 2.0e-30, 1.5e-30]),
}


def test_ratio_error_of_lies_within_its_rounding_bound_of_the_rationals(capsys):
    from graph_framework_amd.batches import ratio_error_of
    worst = Fraction(0)
    for name, (num, den) in PLANTED.items():
        got = float(ratio_error_of(np.array(num), np.array(den)))
        exact = model_of.exact_ratio_error(num, den)
        bound = model_of.ratio_error_bound(num, den)
        error = abs(decimal.Context(prec=model_of.DIGITS + 10).subtract(decimal.Decimal(got), exact))
        print("%s: got %.17g, exact %.20s, error %.3e, bound %.3e" % (name, got, exact, error, bound))
        assert exact is not None and exact > 0 and error <= bound, name
        assert bound < exact*decimal.Decimal("1e-9"), name                  # the bound says something
        worst = max(worst, Fraction(error)/Fraction(bound))
    print("the worst ratio of the error to the bound: %.4f" % float(worst))
    #  Cells side by side, each with its own batches.
    num = np.array([PLANTED["equal batches"][0], PLANTED["an empty batch"][0]]).T
    den = np.array([PLANTED["equal batches"][1], PLANTED["an empty batch"][1]]).T
    both = ratio_error_of(num, den)
    assert both.shape == (2,)
    assert both[0] == ratio_error_of(num[:, 0], den[:, 0]) and both[1] == ratio_error_of(num[:, 1], den[:, 1])


def test_ratio_error_of_says_nan_and_zero_where_it_must():
    from graph_framework_amd.batches import ratio_error_of
    assert np.isnan(ratio_error_of(np.array([3.0]), np.array([1.0])))                                     # m = 1
    assert np.isnan(ratio_error_of(np.array([3.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])))                 # one batch with particles
    assert np.isnan(ratio_error_of(np.zeros(4), np.zeros(4)))                                             # none
    assert np.isnan(ratio_error_of(np.array([1.0, 2.0]), np.array([0.0, 3.0])))                           # S0 - S0_1 = 0
    assert np.isnan(ratio_error_of(np.array([1.0, 2.0, 3.0]), np.array([1.0, -1.0, 1.0])))                # S0 - S0_2 = 0 ... by cancellation
    assert model_of.exact_ratio_error([1.0, 2.0], [0.0, 3.0]) is None and model_of.exact_ratio_error([3.0], [1.0]) is None
    equal = ratio_error_of(np.array([2.0, 4.0, 6.0, 0.0]), np.array([1.0, 2.0, 3.0, 0.0]))                # every R_(g) = 2
    assert equal == 0.0 and not np.signbit(equal)
    assert model_of.exact_ratio_error([2.0, 4.0, 6.0, 0.0], [1.0, 2.0, 3.0, 0.0]) == 0
    with pytest.raises(ValueError):
        ratio_error_of(np.zeros((3, 2)), np.zeros((3, 3)))


def test_the_jackknife_error_agrees_with_the_delta_method():
    """65536 particles in 64 batches, each with a noisy numerator a and a noisy denominator b, correlated: the jackknife
    error of sum a/sum b against the delta-method value sqrt(sum (a - R b)^2)/sum b.  The jackknife's variance estimate has
    63 degrees of freedom, a relative spread of its root of 1/sqrt(126) = 0.089: the interval [2/3, 3/2] is more than
    3.7 sigma wide on either side."""
    from graph_framework_amd.batches import ratio_error_of
    n, batch_count = 65536, 64
    batch = model_of.batch_index(0, n, batch_count)
    ratios = []
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        b = rng.uniform(0.5, 1.5, n)
        a = 3.0*b + rng.normal(0.0, 2.0, n) + rng.exponential(1.0, n)
        num = np.bincount(batch, weights=a, minlength=batch_count)
        den = np.bincount(batch, weights=b, minlength=batch_count)
        r = a.sum()/b.sum()
        delta = np.sqrt(((a - r*b)**2).sum())/b.sum()
        ratios.append(float(ratio_error_of(num, den))/delta)
    print("jackknife/delta over 20 seeds: %.3f to %.3f" % (min(ratios), max(ratios)))
    assert all(2.0/3.0 <= ratio <= 1.5 for ratio in ratios), ratios


def test_the_plain_cpp_pieces_under_the_sanitizers(tmp_path):
    """tests/particle_batches_check.cpp: both host adds over the sizes above, as float and as double, with and without
    weights, against a plain restatement; built with -fsanitize=address,undefined and run as a child process."""
    binary = str(tmp_path/"particle_batches_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "graph_framework_amd", "csrc"), "-o", binary,
                           os.path.join(ROOT, "tests", "particle_batches_check.cpp")])
    out = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0
    last = out.stdout.split()
    assert last[-4] == "cases" and int(last[-3]) > 1000 and last[-2:] == ["failures", "0"]


def read_all(path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    return H5File(path)


def test_moment_bins_file_takes_the_batch_variables(tmp_path):
    from graph_framework_amd.output import write_moment_bins
    bins = np.arange(2*3*4, dtype=np.float64).reshape(2, 3, 4) - 7.0
    edges = np.array([0.0, 0.25, 0.5, 1.0])
    stderr = bins*0.125
    stderr[1, 2, 3] = np.nan
    batch_bins = np.arange(2*5*3*4, dtype=np.float64).reshape(2, 5, 3, 4)
    batch_particles = np.array([[64, 64, 64, 64, 3], [64, 64, 64, 64, 3]])
    means_stderr = np.arange(2*3*3, dtype=np.float64).reshape(2, 3, 3)
    before, after = str(tmp_path/"before.nc"), str(tmp_path/"after.nc")
    write_moment_bins(before, bins, edges, 0.125, 0.53, "sqrt_s", steps=[25, 50])
    write_moment_bins(after, bins, edges, 0.125, 0.53, "sqrt_s", steps=[25, 50], stderr=None, batch_bins=None,
                      batch_particles=None, means_stderr=None)
    assert open(before, "rb").read() == open(after, "rb").read()
    write_moment_bins(after, bins, edges, 0.125, 0.53, "sqrt_s", steps=[25, 50], stderr=stderr, batch_bins=batch_bins,
                      batch_particles=batch_particles, means_stderr=means_stderr)
    f = read_all(after)
    for name, want in (("bins", bins), ("stderr", stderr), ("batch_bins", batch_bins),
                       ("batch_particles", batch_particles.astype(np.float64)), ("means_stderr", means_stderr)):
        got = f.read(name)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
    assert [f.read(name).shape for name in ("time", "ns", "nm", "nb", "nr")] == [(2,), (3,), (4,), (5,), (3,)]
    f.close()
    raw = open(after, "rb").read()
    assert raw.index(b"stderr") > raw.index(b"sbins")                      # written after what the file had
    write_moment_bins(after, bins[0], edges, 0.0, 1.0, stderr=stderr[0], batch_bins=batch_bins[0], batch_particles=batch_particles[0],
                      means_stderr=means_stderr[0])                         # one snapshot
    f = read_all(after)
    assert f.read("stderr").shape == (1, 3, 4) and f.read("batch_bins").shape == (1, 5, 3, 4)
    assert f.read("batch_particles").shape == (1, 5) and f.read("means_stderr").shape == (1, 3, 3)
    f.close()
    for broken in (dict(stderr=stderr[:, :2]), dict(stderr=stderr[:1]), dict(batch_bins=batch_bins[:, :, :2]),
                   dict(batch_bins=batch_bins.reshape(-1)), dict(batch_particles=batch_particles[:1]),
                   dict(batch_bins=batch_bins, batch_particles=batch_particles[:, :4]), dict(means_stderr=means_stderr[:, :, :2]),
                   dict(means_stderr=stderr)):
        with pytest.raises(ValueError):
            write_moment_bins(str(tmp_path/"broken.nc"), bins, edges, 0.0, 1.0, **broken)
        assert not os.path.exists(str(tmp_path/"broken.nc"))


def test_phase_bins_file_takes_the_batch_variables(tmp_path):
    from graph_framework_amd.output import write_phase_bins
    bins = np.arange(2*2*3*4, dtype=np.float64).reshape(2, 2, 3, 4)
    edges = (np.array([0.0, 0.25, 1.0]), np.array([-1.0, -0.5, 0.125, 1.0]), np.array([1.0, 1.5, 2.0, 2.5, 3.0]))
    stderr = bins/16.0
    batch_bins = np.arange(2*3*2*3*4, dtype=np.float64).reshape(2, 3, 2, 3, 4)
    batch_particles = np.array([1000, 1001, 1000])
    before, after = str(tmp_path/"before.nc"), str(tmp_path/"after.nc")
    write_phase_bins(before, bins, *edges, 0.125, 0.53, "s", steps=[25, 50])
    write_phase_bins(after, bins, *edges, 0.125, 0.53, "s", steps=[25, 50], stderr=None, batch_bins=None, batch_particles=None)
    assert open(before, "rb").read() == open(after, "rb").read()
    write_phase_bins(after, bins, *edges, 0.125, 0.53, "s", steps=[25, 50], stderr=stderr, batch_bins=batch_bins,
                     batch_particles=batch_particles)
    f = read_all(after)
    for name, want in (("bins", bins), ("stderr", stderr), ("batch_bins", batch_bins),
                       ("batch_particles", np.array([batch_particles, batch_particles], dtype=np.float64))):
        got = f.read(name)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
    assert f.read("nb").shape == (3,)
    f.close()
    for broken in (dict(stderr=stderr[:, :, :2]), dict(batch_bins=batch_bins[:1]), dict(batch_particles=np.zeros((3, 3))),
                   dict(batch_bins=batch_bins, batch_particles=batch_particles[:2])):
        with pytest.raises(ValueError):
            write_phase_bins(str(tmp_path/"broken.nc"), bins, *edges, 0.0, 1.0, **broken)
