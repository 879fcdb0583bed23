"""Batches of particles on the device (moment_deposit_particles_kernel and phase_deposit_particles_kernel through
gfhip_moments_* and gfhip_phase_*): the batch-major states against the host's add_particles_host byte for byte and the
counters exactly, on the private and the global path, for fp32 and fp64 particles with and without weights; slab g against
a plain object fed batch g's particles; total() against the plain object; splits, shards, orders and first particles;
the statistics against the numpy functions fed the model's sums; a running push through Korc.bin; the refusals; and the
example.  There is no tolerance anywhere: the arithmetic is fixed and the sums are exact."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

import flux_model
import moments_model
import particle_batch_model as model_of
import phase_model
from test_flux_label import same_bits
from test_gpu_phase import DTYPES, NAMES, upload
from test_moments import edges_of
from test_particle_batches import BATCHES, FIRSTS, GAMMA_EDGES, PARTICLES, counters_of, counts_of, particles_of, weights_of

pytestmark = pytest.mark.gpu

#  ns, private: 12 cells in LDS; 256 cells, the cap; 260 cells, above it; 12 cells barred from LDS
MOMENT_CASES = ((3, True), (64, True), (65, True), (3, False))
#  (ns, np, ng), private: 12 cells in LDS; 256 cells, the cap; 257 cells, above it
PHASE_CASES = (((3, 2, 2), True), ((8, 8, 4), True), ((257, 1, 1), True))


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
def pools(context, tables):
    """Per type: the 4099 particles of test_particle_batches.py and their weights, on the host and uploaded once."""
    out = {}
    for kind, dtype in DTYPES.items():
        columns, inside = particles_of(tables, dtype)
        columns.append(weights_of(dtype, inside))
        out[kind] = (columns, upload(context, "pool_" + kind, columns, NAMES + ("w",), dtype))
    return out


def phase_edges(shape):
    from graph_framework_amd.distribution import pitch_edges
    if shape == (3, 2, 2):
        return edges_of(3), pitch_edges(2), GAMMA_EDGES
    return np.linspace(0.0, 1.2, shape[0] + 1), pitch_edges(shape[1]), 1.0 + 49.0*np.linspace(0.0, 1.0, shape[2] + 1)**2


def same_as_host(batched, limbs, counters):
    assert batched.state().tobytes() == limbs.tobytes()
    assert batched.counts() == counters_of(counters)


@pytest.mark.parametrize("kind", sorted(DTYPES))
@pytest.mark.parametrize("ns,private", MOMENT_CASES)
def test_moments_against_the_host_on_every_path(context, tables, pools, ns, private, kind):
    """Every G with every count and every first particle; the weights take turns along them."""
    from graph_framework_amd.moments import FluxMoments, add_particles_host
    columns, keys = pools[kind]
    edges = edges_of(ns)
    for i, batch_count in enumerate(BATCHES):
        for j, (n, first) in enumerate((n, first) for n in counts_of(batch_count) for first in FIRSTS):
            weighted = (i + j) % 2 == 0
            moments = FluxMoments(context, tables, edges, private=private, batches=batch_count)
            info = moments.info()
            assert moments.shape == (batch_count, ns, 4) and moments.batches == batch_count and moments.cell_shape == (ns, 4)
            assert info["private_sums"] == (private and ns*4 <= 256) and info["workgroup_size"] == (1024 if info["private_sums"] else 256)
            assert info["lds_bytes"] == (ns*4*536 if info["private_sums"] else 0) + (ns + 1)*8       # one batch's cells
            moments.add_particles(*keys[:7], n, first, weight=keys[7] if weighted else None)
            want = add_particles_host(tables, edges, batch_count, [c[:n] for c in columns[:7]], first, columns[7][:n] if weighted else None)
            same_as_host(moments, *want)
            moments.close()


@pytest.mark.parametrize("kind", sorted(DTYPES))
@pytest.mark.parametrize("shape,private", PHASE_CASES)
def test_phase_against_the_host_on_every_path(context, tables, pools, shape, private, kind):
    from graph_framework_amd.distribution import PhaseDistribution, add_particles_host
    columns, keys = pools[kind]
    edges = phase_edges(shape)
    cells = int(np.prod(shape))
    for i, batch_count in enumerate(BATCHES):
        for j, (n, first) in enumerate((n, first) for n in counts_of(batch_count) for first in FIRSTS):
            weighted = (i + j) % 2 == 1
            distribution = PhaseDistribution(context, tables, *edges, private=private, batches=batch_count)
            info = distribution.info()
            assert distribution.shape == (batch_count,) + shape and info["private_sums"] == (cells <= 256)
            assert info["lds_bytes"] == (cells*536 if info["private_sums"] else 0) + (sum(shape) + 3)*8
            distribution.add_particles(*keys[:7], n, first, weight=keys[7] if weighted else None)
            want = add_particles_host(tables, *edges, batch_count, [c[:n] for c in columns[:7]], first, columns[7][:n] if weighted else None)
            same_as_host(distribution, *want)
            distribution.close()
    plain = PhaseDistribution(context, tables, *phase_edges((3, 2, 2)), private=False, batches=3)        # 12 cells barred from LDS
    assert not plain.info()["private_sums"]
    plain.add_particles(*keys[:7], PARTICLES, 65, weight=keys[7])
    same_as_host(plain, *add_particles_host(tables, *phase_edges((3, 2, 2)), 3, columns[:7], 65, columns[7]))
    plain.close()


@pytest.mark.parametrize("batch_count", BATCHES)
def test_a_slab_is_the_plain_object_fed_its_batch(context, tables, pools, batch_count):
    """Slab g against a plain object fed batch g's particles, selected in numpy; total() against a plain object fed
    everything; the model's bytes as well.  fp64 with weights for the moments, fp32 without for the distribution."""
    from graph_framework_amd.distribution import PhaseDistribution
    from graph_framework_amd.moments import FluxMoments
    first = FIRSTS[batch_count % len(FIRSTS)]
    batch = model_of.batch_index(first, PARTICLES, batch_count)
    columns, keys = pools["f64"]
    edges = edges_of(3)
    moments = FluxMoments(context, tables, edges, batches=batch_count)
    moments.add_particles(*keys[:7], PARTICLES, first, weight=keys[7])
    state = moments.state()
    model = model_of.moments(tables, edges, batch_count).add(columns[:7], first, columns[7])
    assert state.tobytes() == model.state().tobytes() and moments.counts() == model.counts
    everything = FluxMoments(context, tables, edges)
    everything.add(*keys[:7], PARTICLES, weight=keys[7])
    total = moments.total()
    assert total.batches is None and total.state().tobytes() == everything.state().tobytes() == model.total_state().tobytes()
    assert total.counts() == everything.counts() == moments.counts()
    same_bits(moments.totals(), everything.totals())
    same_bits(moments.means().reshape(-1), everything.means().reshape(-1))
    marginal, other = moments.profile(), everything.profile()
    assert marginal.state().tobytes() == other.state().tobytes() and marginal.counts() == other.counts()
    for each in (total, everything, marginal, other):
        each.close()
    narrow, narrow_keys = pools["f32"]
    axes = phase_edges((3, 2, 2))
    distribution = PhaseDistribution(context, tables, *axes, batches=batch_count)
    distribution.add_particles(*narrow_keys[:7], PARTICLES, first)
    grid = distribution.state()
    for g in range(batch_count):
        chosen = np.flatnonzero(batch == g)
        part = upload(context, "slab%d_%d" % (batch_count, g), [c[chosen] for c in columns], NAMES + ("w",))
        plain = FluxMoments(context, tables, edges)
        if chosen.size:
            plain.add(*part[:7], chosen.size, weight=part[7])
        assert plain.state().tobytes() == state[g].tobytes(), g
        plain.close()
        part = upload(context, "slab32_%d_%d" % (batch_count, g), [c[chosen] for c in narrow[:7]], dtype=np.float32)
        plain = PhaseDistribution(context, tables, *axes)
        plain.add(*part, chosen.size)
        assert plain.state().tobytes() == grid[g].tobytes(), g
        plain.close()
    total = distribution.total()
    everything = PhaseDistribution(context, tables, *axes)
    everything.add(*narrow_keys[:7], PARTICLES)
    assert total.state().tobytes() == everything.state().tobytes() and total.counts() == everything.counts() == distribution.counts()
    marginal, other = distribution.profile(), everything.profile()
    assert marginal.state().tobytes() == other.state().tobytes() and marginal.counts() == other.counts()
    for each in (moments, distribution, total, everything, marginal, other):
        each.close()


def test_one_batch_is_add_and_one_add_is_two(context, tables, pools):
    from graph_framework_amd.distribution import PhaseDistribution
    from graph_framework_amd.moments import FluxMoments
    columns, keys = pools["f64"]
    edges, axes = edges_of(16), phase_edges((3, 2, 2))
    for make in (lambda batches: FluxMoments(context, tables, edges, batches=batches),
                 lambda batches: PhaseDistribution(context, tables, *axes, batches=batches)):
        plain, single = make(None), make(1)
        plain.add(*keys[:7], PARTICLES, weight=keys[7])
        single.add_particles(*keys[:7], PARTICLES, 2**40 + 5, weight=keys[7])
        assert single.state()[0].tobytes() == plain.state().tobytes() and single.counts() == plain.counts()
        whole = make(3)
        whole.add_particles(*keys[:7], PARTICLES, 63, weight=keys[7])
        for cut in (1, 63, 64, 65, 100):
            head = upload(context, "head%d" % cut, [c[:cut] for c in columns], NAMES + ("w",))
            tail = upload(context, "tail%d" % cut, [c[cut:] for c in columns], NAMES + ("w",))
            halves = make(3)
            halves.add_particles(*head[:7], cut, 63, weight=head[7])
            halves.add_particles(*tail[:7], PARTICLES - cut, 63 + cut, weight=tail[7])
            assert halves.state().tobytes() == whole.state().tobytes() and halves.counts() == whole.counts(), cut
            halves.close()
        for each in (plain, single, whole):
            each.close()


def test_shards_on_two_contexts_merge_and_whole_chunks_may_change_places(context, tables, pools):
    from graph_framework_amd import Context
    from graph_framework_amd.distribution import PhaseDistribution
    from graph_framework_amd.moments import FluxMoments
    columns, keys = pools["f32"]
    second = Context(0)
    edges, axes = edges_of(8), phase_edges((3, 2, 2))
    cut, first, batch_count = 1777, 2**40 + 5, 16
    for make in (lambda where, batches=batch_count: FluxMoments(where, tables, edges, batches=batches),
                 lambda where, batches=batch_count: PhaseDistribution(where, tables, *axes, batches=batches)):
        whole = make(context)
        whole.add_particles(*keys[:7], PARTICLES, first, weight=keys[7])
        here, there = make(context), whole.like(second)
        assert there.batches == batch_count and there.context is second
        head = upload(context, "shard0", [c[:cut] for c in columns], NAMES + ("w",), np.float32)
        tail = upload(second, "shard1", [c[cut:] for c in columns], NAMES + ("w",), np.float32)
        here.add_particles(*head[:7], cut, first, weight=head[7])
        there.add_particles(*tail[:7], PARTICLES - cut, first + cut, weight=tail[7])
        here.merge(there.state(), **there.counts())
        assert here.state().tobytes() == whole.state().tobytes() and here.counts() == whole.counts()
        for each in (whole, here, there):
            each.close()
    second.close()
#  Chunks of 64 particles of one batch in another order: first = 0, G = 4, chunk c and chunk c + 4k change places.
    n, batch_count = 64*4*6, 4
    order = np.arange(n).reshape(6, 4, 64)
    order = order[np.random.default_rng(3).permutation(6)].reshape(-1)
    wide, wide_keys = pools["f64"]
    moved = upload(context, "moved", [c[order] for c in wide], NAMES + ("w",))
    for make in (lambda: FluxMoments(context, tables, edges, batches=batch_count),
                 lambda: PhaseDistribution(context, tables, *axes, batches=batch_count)):
        straight, shuffled = make(), make()
        straight.add_particles(*wide_keys[:7], n, 0, weight=wide_keys[7])
        shuffled.add_particles(*moved[:7], n, 0, weight=moved[7])
        assert straight.state().tobytes() == shuffled.state().tobytes() and straight.state().any()
        assert straight.counts() == shuffled.counts()
        straight.close()
        shuffled.close()


def test_waves_that_are_all_outside_all_on_one_surface_or_a_tail_of_one(context, tables):
    """test_gpu_moments.py's blocks of 64 particles, a wave each, through the batched kernels on both paths."""
    from graph_framework_amd.distribution import PhaseDistribution, add_particles_host as phase_host
    from graph_framework_amd.moments import FluxMoments, add_particles_host
    from test_phase import random_particles
    random = random_particles(tables, PARTICLES, 3)
    label, _ = moments_model.label_values(tables, *random)
    surface = flux_model.cells_of(edges_of(64), label)
    off = np.flatnonzero(np.isnan(label))[:64]
    same = np.repeat(np.flatnonzero(surface == 20)[:1], 64)
    one_surface = np.resize(np.flatnonzero(surface == 20), 64)
    tail = np.flatnonzero(surface == 7)[:1]
    order = np.concatenate([off, same, one_surface, off, same, tail])
    columns = [c[order] for c in random]
    keys = upload(context, "batched_waves", columns)
    for ns, private in ((64, True), (65, True), (64, False)):
        for n in (64, 128, order.size):
            moments = FluxMoments(context, tables, edges_of(ns), private=private, batches=3)
            moments.add_particles(*keys, n, 0)
            same_as_host(moments, *add_particles_host(tables, edges_of(ns), 3, [c[:n] for c in columns], 0))
            if n == 64:
                assert moments.counts() == dict(samples=64, outside=64, skipped=0) and not moments.state().any()
            moments.close()
    for shape in ((8, 8, 4), (257, 1, 1)):
        distribution = PhaseDistribution(context, tables, *phase_edges(shape), batches=2)
        distribution.add_particles(*keys, order.size, 64)
        same_as_host(distribution, *phase_host(tables, *phase_edges(shape), 2, columns, 64))
        distribution.close()


def test_the_statistics_are_numpys_on_the_models_sums(context, tables, pools):
    from graph_framework_amd import batches
    from graph_framework_amd.distribution import PhaseDistribution
    from graph_framework_amd.moments import FluxMoments
    columns, keys = pools["f64"]
    first, batch_count, edges = 65, 16, edges_of(5)
    moments = FluxMoments(context, tables, edges, batches=batch_count)
    moments.add_particles(*keys[:7], PARTICLES, first)
    model = model_of.moments(tables, edges, batch_count).add(columns[:7], first)
    sums, total = model.bins(), model.total_bins()
    particles = np.bincount(model_of.batch_index(first, PARTICLES, batch_count), minlength=batch_count)
    assert list(moments.batch_rays(first, PARTICLES)) == list(particles)
    same_bits(moments.read().reshape(-1), sums.reshape(-1))
    mean, stderr, used = moments.standard_error(first, PARTICLES)
    want = batches.standard_error_of(sums, total, particles, PARTICLES)
    same_bits(mean.reshape(-1), want[0].reshape(-1))
    same_bits(stderr.reshape(-1), want[1].reshape(-1))
    assert used == want[2] == batch_count and np.isfinite(stderr).all() and (stderr[:, 2] > 0.0).all()
    same_bits(moments.batch_means(first, PARTICLES).reshape(-1), (sums/particles[:, None, None]).reshape(-1))
    error = moments.means_error()
    assert error.shape == (5, 3) and np.isfinite(error).all() and (error > 0.0).all()
    for k in (1, 2, 3):
        same_bits(error[:, k - 1], batches.ratio_error_of(sums[:, :, k], sums[:, :, 0]))
    variables = moments.sum_error_variables(first, PARTICLES)
    same_bits(variables["stderr"].reshape(-1), (PARTICLES*want[1]).reshape(-1))
    assert list(variables["batch_particles"]) == list(particles)
    with pytest.raises(ValueError):
        FluxMoments(context, tables, edges).means_error()
    moments.close()
    axes = phase_edges((3, 2, 2))
    distribution = PhaseDistribution(context, tables, *axes, batches=batch_count)
    distribution.add_particles(*keys[:7], PARTICLES, first, weight=keys[7])
    model = model_of.phase(tables, *axes, batch_count).add(columns[:7], first, columns[7])
    mean, stderr, used = distribution.standard_error(first, PARTICLES)
    want = batches.standard_error_of(model.bins(), model.total_bins(), particles, PARTICLES)
    same_bits(mean.reshape(-1), want[0].reshape(-1))
    same_bits(stderr.reshape(-1), want[1].reshape(-1))
    distribution.close()


@pytest.mark.parametrize("kind,first", [("f32", 0), ("f64", 4096)])
def test_batches_behind_the_push(tables, kind, first):
    """The 3001-particle push of test_gpu_phase.py binned after 25 and 50 steps through Korc.bin with the shard's first
    particle, against the model fed the sync_host() states, plain and under a Confinement's alive weights."""
    from graph_framework_amd import korc
    from graph_framework_amd.confinement import CONFINED, Confinement
    from graph_framework_amd.distribution import PhaseDistribution, pitch_edges
    from graph_framework_amd.moments import FluxMoments
    rng = np.random.default_rng(17)
    n, batch_count = 3001, 4
    particles = dict(x=rng.uniform(1.5, 1.9, n), y=rng.uniform(-0.2, 0.2, n), z=rng.uniform(-0.3, 0.3, n),
                     ux=rng.uniform(-0.3, 0.3, n), uy=rng.uniform(0.3, 0.85, n), uz=rng.uniform(-0.3, 0.3, n),
                     gamma=np.zeros(n))
    push = korc.Korc(particles, kind, first_particle=first)
    assert push.first_particle == first and korc.Korc.__init__.__defaults__[-1] == 0
    push.compile()
    push.pre_run()
    where = push.work.context
    edges = np.linspace(-0.01, 0.25, 9)
    axes = (np.linspace(-0.01, 0.25, 5), pitch_edges(4), np.linspace(1.0, 3.0, 5))
    moments, confined = (FluxMoments(where, tables, edges, batches=batch_count) for _ in range(2))
    grid, confined_grid = (PhaseDistribution(where, tables, *axes, batches=batch_count) for _ in range(2))
    plain = FluxMoments(where, tables, edges)
    tracker = Confinement(where, tables, [1.0, 2.5], [-1.0, 1.0], [1.0, 3.0], n, kind, limit=0.06)
    models = [model_of.moments(tables, edges, batch_count) for _ in range(2)] + [model_of.phase(tables, *axes, batch_count) for _ in range(2)]
    for _ in range(2):
        push.run(25)
        push.bin(moments)
        push.bin(grid)
        push.bin(plain)
        push.track(tracker)
        push.bin(confined, weight=tracker.alive_key)
        push.bin(confined_grid, weight=tracker.alive_key)
        host = [push.sync_host()[k].copy() for k in korc.PARTICLE]
        alive = (tracker.lost_steps() == CONFINED).astype(DTYPES[kind])
        assert 0 < alive.sum() < n
        for model, weight in zip(models, (None, alive, None, alive)):
            model.add(host, first, weight)
    for got, model in zip((moments, confined, grid, confined_grid), models):
        assert got.state().tobytes() == model.state().tobytes() and got.counts() == model.counts
    total = moments.total()
    assert total.state().tobytes() == plain.state().tobytes() and moments.counts() == dict(samples=2*n, outside=0, skipped=0)
    assert np.isfinite(confined.means_error()[confined.total().read()[:, 0] > 0.0]).all()
    for each in (moments, confined, grid, confined_grid, plain, total, tracker):
        each.close()
    where.close()


def test_misuse_is_refused_before_anything_runs(context, tables, pools):
    from graph_framework_amd import GfHipError
    from graph_framework_amd.distribution import PhaseDistribution
    from graph_framework_amd.moments import FluxMoments
    lib = context.lib
    columns, keys = pools["f64"]
    _, narrow = pools["f32"]
    edges, axes = edges_of(3), phase_edges((3, 2, 2))
    for make, name in ((lambda **more: FluxMoments(context, tables, edges, **more), "moments"),
                       (lambda **more: PhaseDistribution(context, tables, *axes, **more), "phase")):
        for batch_count in (0, 257):
            with pytest.raises(GfHipError, match="1 to 256 batches"):
                make(batches=batch_count)
        plain, batched = make(), make(batches=4)
        with pytest.raises(GfHipError, match="only a batched object"):
            plain.add_particles(*keys[:7], 64, 0)
        with pytest.raises(GfHipError, match="with their index"):
            batched.add(*keys[:7], 64)
        with pytest.raises(GfHipError, match="overflows 64 bits"):
            batched.add_particles(*keys[:7], 64, 2**64 - 5)
        with pytest.raises(GfHipError, match="one type"):
            batched.add_particles(*keys[:6], narrow[6], 64, 0)
        with pytest.raises(GfHipError, match="one type"):
            batched.add_particles(*keys[:7], 64, 0, weight=narrow[7])
        with pytest.raises(GfHipError, match="unknown buffer"):
            batched.add_particles(*keys[:6], "no such buffer", 64, 0)
        with pytest.raises(GfHipError, match="shorter"):
            batched.add_particles(*keys[:7], PARTICLES + 1, 0)
        if name == "moments":
            with pytest.raises(GfHipError, match="at least one particle"):
                batched.add_particles(*keys[:7], 0, 0)
        other = make(batches=3)
        with pytest.raises(GfHipError, match="another shape"):
            batched.merge(other.state(), samples=5)                             # another batch count
        with pytest.raises(GfHipError, match="another shape"):
            batched.merge(batched.state()[:, :2], samples=5)                    # another shape
        with pytest.raises(GfHipError, match="another shape"):
            plain.merge(batched.state()[0][:2])
        with pytest.raises(ValueError):
            batched.merge(plain.state())                                        # a plain state into a batched object
        with pytest.raises(ValueError):
            plain.merge(batched.state())
        merge_plain, merge_batches = getattr(lib, "gfhip_%s_merge" % name), getattr(lib, "gfhip_%s_merge_batches" % name)
        limbs = batched.state()
        shape = limbs.shape[1:-1]
        assert merge_plain(batched.handle, limbs.ctypes.data, *shape, 1, 0, 0) == 1                    # merge on a batched object
        assert "another shape" in lib.gfhip_last_error(context.handle).decode()
        assert merge_batches(plain.handle, limbs.ctypes.data, 4, *shape, 1, 0, 0) == 1                 # merge_batches on a plain one
        assert "another shape" in lib.gfhip_last_error(context.handle).decode()
        assert merge_batches(batched.handle, None, 4, *shape, 1, 0, 0) == 1 and merge_batches(None, limbs.ctypes.data, 4, *shape, 1, 0, 0) == 1
        add_particles = getattr(lib, "gfhip_%s_add_particles" % name)
        seven = (ctypes.c_uint64*7)(*range(1, 8))
        assert add_particles(batched.handle, None, 0, 0, 1, 0) == 1 and add_particles(None, seven, 0, 0, 1, 0) == 1
        with pytest.raises(ValueError):
            plain.total()
        with pytest.raises(ValueError):
            plain.standard_error(0, 64)
        for each in (plain, batched, other):
            assert each.counts() == dict(samples=0, outside=0, skipped=0) and not each.state().any()      # nothing was launched
        batched.add_particles(*keys[:7], 64, 2**64 - 65, weight=keys[7])        # the last 64 particles there are; it still works
        assert batched.counts()["samples"] == 64
        plain.add(*keys[:7], 64, weight=keys[7])
        total = batched.total()
        assert total.state().tobytes() == plain.state().tobytes()
        for each in (plain, batched, other, total):
            each.close()


@pytest.mark.parametrize("loss", [False, True], ids=["all", "confined"])
def test_example_writes_error_bars(tmp_path, loss):
    """examples/push_particles.py --moments 8 --particle-batches 4 as a child process, and again with --loss-limit: stderr
    is finite wherever bins is not zero, the batch means times the batches' particles add up to the bins, and the
    totals are printed with their errors."""
    import subprocess
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    prefix = str(tmp_path / "korc")
    command = [sys.executable, os.path.join(ROOT, "examples", "push_particles.py"), "--particles", "3001", "--steps", "50",
               "--every", "25", "--label-bins", "4", "--pitch-bins", "4", "--gamma-bins", "4", "--flux-tables",
               os.path.join(GOLDEN, "efit_tables.npz"), "--output", prefix, "--moments", "8", "--particle-batches", "4"]
    out = subprocess.run(command + (["--loss-limit", "0.06"] if loss else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("total current") == 2 and out.stdout.count("+-") == 4, out.stdout
    for name, cells in (("moment", (8, 4)), ("phase", (4, 4, 4))):
        f = H5File(prefix + "_%s_bins.nc" % name)
        bins, stderr, batch_bins, batch_particles = (f.read(v) for v in ("bins", "stderr", "batch_bins", "batch_particles"))
        assert bins.shape == stderr.shape == (2,) + cells and batch_bins.shape == (2, 4) + cells and batch_particles.shape == (2, 4)
        assert list(batch_particles[0]) == list(np.bincount(model_of.batch_index(0, 3001, 4)).astype(np.float64)) and bins.any()
        assert np.isfinite(stderr[bins != 0.0]).all() and (stderr[bins != 0.0] > 0.0).all()
        if name == "moment":
            means = f.read("means_stderr")
            assert means.shape == (2, 8, 3) and np.isfinite(means[bins[:, :, 0] > 16.0]).all()
            counted = (batch_bins[:, :, :, 0]*batch_particles[:, :, None]).sum(axis=1)
            assert np.abs(counted - bins[:, :, 0]).max() < 1.0e-9          # the batch means are quotients: rounded
        f.close()
