"""The tail of a launch in every family that deposits by the grid-stride loop and by csrc/flux_sums.hpp's batched loops
(flux profile, spectrum, distribution, moment profile): 1, 63, 64, 65, 1023, 1024, 1025 and 2*1024 + 37 samples, on the
private route (4 cells) and with private=False, plain and in 3 batches from first = 61.  state() and counts() against the numpy models (rays)
and the host entry points (particles), byte for byte and exactly.  In every case the last sample lies outside the map
and the one before it has a non-finite value (with one sample that sample is both, and counts as outside), so `outside`
and `skipped` are met in the last, partly filled wave.  There is no tolerance: the sums are exact."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import flux_batch_model
import flux_model
import spectrum_model
import test_gpu_flux_profile as flux_tests
import test_gpu_spectrum as spectrum_tests
from test_gpu_phase import NAMES, upload
from test_particle_batches import counters_of, particles_of, weights_of

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 2*1024 + 37)
BATCHES, FIRST = 3, 61
ROUTES = (True, False)
FAR = 1.0e6                                                                 # x of a point off every map


@pytest.fixture(scope="module")
def context():
    from graph_framework_amd import Context
    context = Context(0)
    yield context
    context.close()


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(os.path.join(GOLDEN, "efit_tables.npz")))


def planted(base, n, value_column, bad):
    """The first n samples of the columns, the last one off the map and the value before it (the last one's when n = 1)
    non-finite."""
    columns = [np.array(c[:n]) for c in base]
    columns[0][n - 1] = FAR
    columns[value_column][max(n - 2, 0)] = bad
    return columns


def batched_model(make, columns, n):
    """(state, counts) of 3 batches: slab g is the model fed batch g's samples alone."""
    batch = flux_batch_model.batch_index(FIRST, n, BATCHES)
    models = [make().add(*[c[batch == g] for c in columns]) for g in range(BATCHES)]
    counts = {name: sum(model.counts[name] for model in models) for name in ("samples", "outside", "skipped")}
    return b"".join(model.state().tobytes() for model in models), counts


def check_rays(context, tag, make_object, make_model, base, value_column):
    for n in COUNTS:
        columns = planted(base, n, value_column, np.inf if n % 2 else np.nan)
        plain = make_model().add(*columns)
        assert plain.counts["outside"] >= 1 and (n == 1 or plain.counts["skipped"] >= 1)
        batched = batched_model(make_model, columns, n)
        keys = flux_tests.upload(context, "%s%d" % (tag, n), columns, ["c%d" % k for k in range(len(columns))])
        for private in ROUTES:
            one = make_object(private, None)
            assert one.info()["private_sums"] == private
            one.add(*keys, n)
            assert one.counts() == plain.counts and one.state().tobytes() == plain.state().tobytes()
            one.close()
            many = make_object(private, BATCHES)
            many.add_rays(*keys, n, FIRST)
            assert many.counts() == batched[1] and many.state().tobytes() == batched[0]
            many.close()


def test_flux_profile_tails(context, tables):
    from graph_framework_amd.flux import FluxProfile
    points = flux_tests.all_points(tables, np.load(os.path.join(GOLDEN, "flux_golden.npz")))
    pool = (points, flux_model.label(tables, *points))
    base = flux_tests.samples(pool, COUNTS[-1], 11)
    edges = np.array([0.2, 0.35, 0.5, 0.65, 0.8])
    check_rays(context, "tail_flux", lambda private, batches: FluxProfile(context, tables, edges, private=private, batches=batches),
               lambda: flux_model.Profile(tables, edges), base, 3)


def test_spectrum_tails(context, tables):
    from graph_framework_amd.spectrum import FluxSpectrum
    golden = np.load(os.path.join(GOLDEN, "flux_golden.npz"))
    columns = tuple(np.concatenate(pair) for pair in zip(spectrum_tests.golden_samples(golden), spectrum_tests.planted_samples(tables)))
    base = spectrum_tests.samples((columns, None, None), COUNTS[-1], 12)
    sedges, nedges = np.array([0.2, 0.5, 0.8]), np.array([-2.0, 0.0, 2.0])
    check_rays(context, "tail_spectrum",
               lambda private, batches: FluxSpectrum(context, tables, sedges, nedges, private=private, batches=batches),
               lambda: spectrum_model.Spectrum(tables, sedges, nedges), base, 7)


def check_particles(context, tables, tag, make_object, host_plain, host_batched):
    """fp32 particles with weights against the host entry points."""
    base, inside = particles_of(tables, np.float32)
    base.append(weights_of(np.float32, inside))
    for n in COUNTS:
        columns = planted(base, n, 7, np.float32(np.inf if n % 2 else np.nan))
        plain = host_plain([c for c in columns[:7]], columns[7])
        assert plain[1][1] >= 1 and (n == 1 or plain[1][2] >= 1)
        batched = host_batched([c for c in columns[:7]], columns[7])
        keys = upload(context, "%s%d" % (tag, n), columns, NAMES + ("w",), np.float32)
        for private in ROUTES:
            one = make_object(private, None)
            assert one.info()["private_sums"] == private
            one.add(*keys[:7], n, weight=keys[7])
            assert one.counts() == counters_of(plain[1]) and one.state().tobytes() == plain[0].tobytes()
            one.close()
            many = make_object(private, BATCHES)
            many.add_particles(*keys[:7], n, FIRST, weight=keys[7])
            assert many.counts() == counters_of(batched[1]) and many.state().tobytes() == batched[0].tobytes()
            many.close()


def test_distribution_tails(context, tables):
    from graph_framework_amd.distribution import PhaseDistribution, add_particles_host, pitch_edges
    edges = (np.array([0.02, 0.5, 0.98]), pitch_edges(2), np.array([1.0, 50.0]))
    check_particles(context, tables, "tail_phase",
                    lambda private, batches: PhaseDistribution(context, tables, *edges, private=private, batches=batches),
                    lambda columns, weight: add_particles_host(tables, *edges, 1, columns, 0, weight),       # one batch: the plain state
                    lambda columns, weight: add_particles_host(tables, *edges, BATCHES, columns, FIRST, weight))


def test_moment_profile_tails(context, tables):
    from graph_framework_amd.moments import FluxMoments, add_host, add_particles_host
    edges = np.array([0.02, 0.98])
    check_particles(context, tables, "tail_moments",
                    lambda private, batches: FluxMoments(context, tables, edges, private=private, batches=batches),
                    lambda columns, weight: add_host(tables, edges, columns, weight),
                    lambda columns, weight: add_particles_host(tables, edges, BATCHES, columns, FIRST, weight))
