"""Moments of particles per flux surface on the device (csrc/moment_bins.hip through gfhip_moments_*): every cell's limbs
against rational arithmetic byte for byte and the three counters exactly, for fp64 and fp32 particles, on the private and
the global path; the same bytes whatever the route, the order or the shards; labels and moments against the host's bit for
bit; moment 0 against FluxProfile.add; totals, means and densities; the moments of a running push against the model fed
the push's own states, with and without a tracker's alive weights; and the refusals.  There is no tolerance anywhere: the
arithmetic is fixed and the sums are exact."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

import flux_model
import moments_model
from test_flux_label import same_bits
from test_gpu_phase import DTYPES, NAMES, upload
from test_moments import SEED, deposit_columns, seeded_weights
from test_phase import random_particles

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 1025, 4099)
#  ns, private: 12 cells in LDS; 256 cells, the cap; 260 cells, above it; 12 cells barred from LDS
CASES = ((3, True), (64, True), (65, True), (3, False))


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
def pool(tables):
    """4099 + 52 particles, computed once and shuffled: the random ones (a quarter off the map), the planted ones and
    the extras of test_moments.py."""
    columns = deposit_columns(tables, np.float64)
    order = np.random.default_rng(12).permutation(columns[0].size)
    columns = [c[order] for c in columns]
    for c in columns:
        c.setflags(write=False)
    return columns


def edges_of(ns):
    return np.linspace(0.02, 0.98, ns + 1)


def check(moments, model):
    assert moments.counts() == model.counts
    assert moments.state().tobytes() == model.state().tobytes()
    same_bits(moments.read().reshape(-1), model.bins().reshape(-1))


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_deposits_against_the_model_on_every_path(context, tables, pool, kind):
    from graph_framework_amd.moments import FluxMoments, add_host
    dtype = DTYPES[kind]
    typed = [c.astype(dtype) for c in pool]
    surface = moments_model.Moments(tables, edges_of(3)).weighted(*typed)[0]
    weight = seeded_weights(typed[0].size, dtype, np.flatnonzero(surface >= 0))
    for n in COUNTS:
        columns = [c[:n] for c in typed] + [weight[:n]]
        keys = upload(context, "paths_%s_%d" % (kind, n), columns, NAMES + ("w",), dtype)
        states = {}
        for ns, private in CASES:
            edges = edges_of(ns)
            for given in (None, columns[7]):
                model = moments_model.Moments(tables, edges).add(*columns[:7], weight=given)
                moments = FluxMoments(context, tables, edges, private=private)
                info = moments.info()
                assert moments.shape == (ns, 4) and info["cap_cells"] == 256
                assert info["private_sums"] == (private and ns*4 <= 256)
                assert info["workgroup_size"] == (1024 if info["private_sums"] else 256)
                assert info["lds_bytes"] == (ns*4*536 if info["private_sums"] else 0) + (ns + 1)*8 <= 160*1024
                moments.add(*keys[:7], n, weight=None if given is None else keys[7])
                check(moments, model)
                check(moments, model)                                       # reading again changes nothing
                limbs, counters = add_host(tables, edges, columns[:7], given)
                assert limbs.tobytes() == moments.state().tobytes() and [int(c) for c in counters] == list(model.counts.values())
                states[ns, private, given is None] = moments.state().tobytes()
                moments.close()
        for plain in (True, False):
            assert states[3, True, plain] == states[3, False, plain]        # the same bytes without the on-chip sums
    assert model.counts["skipped"] >= 3 and model.counts["outside"] >= n//5


def test_waves_that_are_all_outside_all_on_one_surface_or_spread(context, tables):
    """Blocks of 64 particles, a wave each: all off the map; ONE particle repeated without weights (on the global path the
    pre-sum's shared limbs for moment 0, and for every moment here); 64 particles on 64 different surfaces; and a tail wave
    of one particle."""
    from graph_framework_amd.moments import FluxMoments
    random = random_particles(tables, 4099, SEED)
    label, _ = moments_model.label_values(tables, *random)
    edges = edges_of(64)
    surface = flux_model.cells_of(edges, label)
    off = np.flatnonzero(np.isnan(label))[:64]
    same = np.repeat(np.flatnonzero(surface == 20)[:1], 64)
    spread = np.array([np.flatnonzero(surface == s)[0] for s in range(64) if (surface == s).any()])
    assert off.size == 64 and spread.size >= 48
    spread = np.resize(spread, 64)
    one_surface = np.resize(np.flatnonzero(surface == 20), 64)              # different particles of one surface
    tail = np.flatnonzero(surface == 7)[:1]
    order = np.concatenate([off, same, spread, one_surface, off, same, tail])
    columns = [c[order] for c in random]
    assert order.size == 6*64 + 1
    keys = upload(context, "waves", columns)
    for ns, private in ((64, True), (65, True), (64, False)):
        for n in (64, 128, 192, 256, order.size):
            moments = FluxMoments(context, tables, edges_of(ns), private=private)
            moments.add(*keys, n)
            check(moments, moments_model.Moments(tables, edges_of(ns)).add(*[c[:n] for c in columns]))
            if n == 64:
                assert moments.counts() == dict(samples=64, outside=64, skipped=0) and not moments.state().any()
            moments.close()


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_values_equal_the_hosts_bit_for_bit(context, tables, pool, kind):
    from graph_framework_amd.moments import FluxMoments, values_host
    dtype = DTYPES[kind]
    n = pool[0].size
    columns = [c.astype(dtype) for c in pool]
    keys = upload(context, "values_" + kind, columns, dtype=dtype)
    out = upload(context, "values_out_" + kind, [np.full(n, 7.0), np.full(4*n, 7.0)], ("label", "values"))
    for options in (dict(), dict(sqrt_label=True), dict(psi0=0.25, span=-0.125)):
        moments = FluxMoments(context, tables, [0.0, 1.0], **options)
        moments.values(*keys, *out, n)
        label = context.copy_to_host(out[0], np.empty(n))
        values = context.copy_to_host(out[1], np.empty(4*n)).reshape(n, 4)
        for want in (values_host(tables, columns, **options), moments_model.label_values(tables, *columns, **options)):
            same_bits(label, want[0])
            same_bits(values.reshape(-1), want[1].reshape(-1))
        assert moments.counts() == dict(samples=0, outside=0, skipped=0)   # nothing is deposited
        moments.close()
    assert np.isnan(values[:, 1]).sum() > 800 and np.isfinite(values[:, 3]).sum() > 2000


def test_same_bytes_in_any_order_from_shards_and_for_widened_columns(context, tables, pool):
    from graph_framework_amd.moments import FluxMoments
    n = pool[0].size
    narrow = [c.astype(np.float32) for c in pool]
    columns = [c.astype(np.float64) for c in narrow]                        # the fp64 widening of the fp32 columns
    edges = edges_of(16)
    whole = FluxMoments(context, tables, edges)
    whole.add(*upload(context, "order", columns), n)
    check(whole, moments_model.Moments(tables, edges).add(*columns))
    want, counts = whole.state().tobytes(), whole.counts()
    as_f32 = FluxMoments(context, tables, edges)
    as_f32.add(*upload(context, "order32", narrow, dtype=np.float32), n)
    assert as_f32.state().tobytes() == want and as_f32.counts() == counts
    order = np.random.default_rng(8).permutation(n)
    shuffled = FluxMoments(context, tables, edges)
    shuffled.add(*upload(context, "shuffled", [c[order] for c in columns]), n)
    assert shuffled.state().tobytes() == want and shuffled.counts() == counts
    merged = whole.like(context)
    for h, part in enumerate((order[:1777], order[1777:3000], order[3000:])):
        shard = FluxMoments(context, tables, edges, private=h != 1)
        shard.add(*upload(context, "shard%d" % h, [c[part] for c in columns]), part.size)
        merged.merge(shard.state(), **shard.counts())
        shard.close()
    assert merged.state().tobytes() == want and merged.counts() == counts
    same_bits(merged.read(5.0).reshape(-1), whole.read(5.0).reshape(-1))
    for each in (whole, as_f32, shuffled, merged):
        each.close()


def test_profile_totals_means_and_densities(context, tables):
    """An input with skipped == 0: profile() has the bytes and the counts of a FluxProfile fed the same particles and
    weights; totals() is the state of a one-surface FluxMoments fed everything, and the model's rationals rounded once;
    means() and densities() are IEEE quotients of read()."""
    from graph_framework_amd.flux import FluxProfile
    from graph_framework_amd.moments import FluxMoments
    columns = list(random_particles(tables, 4099, SEED))
    n = columns[0].size
    weight = np.random.default_rng(5).uniform(-0.5, 2.0, n)
    edges = edges_of(8)
    keys = upload(context, "profile", columns + [weight], NAMES + ("w",))
    moments = FluxMoments(context, tables, edges)
    moments.add(*keys[:7], n, weight=keys[7])
    model = moments_model.Moments(tables, edges).add(*columns, weight=weight)
    check(moments, model)
    assert moments.counts()["skipped"] == 0
    profile = FluxProfile(context, tables, edges)
    profile.add(keys[0], keys[1], keys[2], keys[7], n)
    marginal = moments.profile()
    assert marginal.state().tobytes() == profile.state().tobytes() and marginal.state().any()
    assert marginal.counts() == profile.counts() == moments.counts()
    single = FluxMoments(context, tables, edges[[0, -1]])
    single.add(*keys[:7], n, weight=keys[7])
    totals = moments.totals()
    same_bits(totals, single.read()[0])
    same_bits(totals, model.totals())
    bins = moments.read()
    with np.errstate(divide="ignore", invalid="ignore"):
        same_bits(moments.means().reshape(-1), (bins[:, 1:]/bins[:, :1]).reshape(-1))
        volume, _ = profile.volumes(4)
        assert (volume > 0.0).all()
        same_bits(moments.densities(4).reshape(-1), (bins/volume[:, None]).reshape(-1))
    empty = FluxMoments(context, tables, edges)
    assert np.isnan(empty.means()).all() and (empty.totals() == 0.0).all()
    for each in (moments, profile, marginal, single, empty):
        each.close()


@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_moments_behind_the_push(tables, kind):
    """The ensemble of test_gpu_phase.test_bins_behind_the_push: 25 steps, bin, 25 steps, bin, on the push's own context
    and stream, against the model fed the two sync_host() states; then the same under a Confinement's alive weights,
    against the model fed the confined particles only."""
    from graph_framework_amd import korc
    from graph_framework_amd.confinement import CONFINED, Confinement
    from graph_framework_amd.moments import FluxMoments
    rng = np.random.default_rng(17)
    n = 3001
    particles = dict(x=rng.uniform(1.5, 1.9, n), y=rng.uniform(-0.2, 0.2, n), z=rng.uniform(-0.3, 0.3, n),
                     ux=rng.uniform(-0.3, 0.3, n), uy=rng.uniform(0.3, 0.85, n), uz=rng.uniform(-0.3, 0.3, n),
                     gamma=np.zeros(n))
    push = korc.Korc(particles, kind)
    push.compile()
    push.pre_run()
    edges = np.linspace(-0.01, 0.25, 9)
    moments = FluxMoments(push.work.context, tables, edges)
    confined = FluxMoments(push.work.context, tables, edges)
    tracker = Confinement(push.work.context, tables, [1.0, 2.5], [-1.0, 1.0], [1.0, 3.0], n, kind, limit=0.06)
    model, confined_model = moments_model.Moments(tables, edges), moments_model.Moments(tables, edges)
    for _ in range(2):
        push.run(25)
        push.bin(moments)
        push.track(tracker)
        push.bin(confined, weight=tracker.alive_key)
        host = push.sync_host()
        assert host["x"].dtype == DTYPES[kind]
        model.add(*[host[k] for k in korc.PARTICLE])
        alive = tracker.lost_steps() == CONFINED
        confined_model.add(*[host[k] for k in korc.PARTICLE], weight=alive.astype(np.float64))
        only = moments_model.Moments(tables, edges).add(*[host[k][alive] for k in korc.PARTICLE])
        assert 0 < alive.sum() < n
    check(moments, model)
    check(confined, confined_model)
    assert moments.counts() == dict(samples=2*n, outside=0, skipped=0)
    assert moments.read()[:, 0].sum() == 2*n and (moments.read()[:, 1] != 0.0).sum() >= 4
    last = moments_model.Moments(tables, edges).add(*[host[k] for k in korc.PARTICLE], weight=alive.astype(np.float64))
    assert last.units == only.units                                         # a weight of 0 deposits nothing: the confined particles only
    same_bits(confined.totals(), confined_model.totals())
    for each in (moments, confined, tracker):
        each.close()
    push.work.context.close()


def test_misuse_is_refused_before_anything_runs(context, tables):
    from graph_framework_amd import GfHipError
    from graph_framework_amd.flux import flux_map
    from graph_framework_amd.moments import FluxMoments
    from graph_framework_amd.spectrum import spectrum_field
    lib = context.lib

    def refused(match, given, field, edges, size=None):
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        handle = lib.gfhip_moments_create(context.handle, ctypes.byref(given) if given is not None else None,
                                          ctypes.byref(field) if field is not None else None,
                                          edges.ctypes.data if edges.size else None, edges.size - 1 if size is None else size)
        assert not handle
        assert match in lib.gfhip_last_error(context.handle).decode(), lib.gfhip_last_error(context.handle).decode()

    good, keep = flux_map(tables)
    field, keep_field = spectrum_field(tables)
    unit = np.array([0.0, 0.5, 1.0])
    refused("needs a map", None, field, unit)
    refused("needs a map", good, None, unit)
    refused("needs a map", good, field, np.array([]), 2)
    refused("at least two edges", good, field, np.array([0.5]))
    refused("1 to 4096 surfaces", good, field, np.arange(4098.0))
    refused("at most 2^20 cells", good, field, np.arange(2.0**18 + 2.0))
    for edges in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 1.0], [0.0, np.inf]):
        refused("strictly increasing", good, field, np.array(edges))
    broken, keep_broken = spectrum_field(tables)
    broken.fpol[1] = None
    refused("four fpol tables", good, broken, unit)
    broken, keep_broken = spectrum_field(tables)
    broken.reserved = 3
    refused("reserved", good, broken, unit)
    broken_map, keep_map = flux_map(tables)
    broken_map.reserved = 1
    refused("reserved", broken_map, field, unit)
    broken_map, keep_map = flux_map(tables, flags=4)
    refused("unknown flag", broken_map, field, unit)
    with pytest.raises(ValueError):
        FluxMoments(context, tables, [0.0])

    n = 64
    columns = [np.full(n, v) for v in (1.9, 0.0, 0.0, 0.3, 0.5, 0.1, 1.5)]
    label, _ = moments_model.label_values(tables, *[c[:1] for c in columns])
    assert 0.0 < label[0] < 1.0
    ok = upload(context, "ok", columns + [np.full(n, 3.0)], NAMES + ("w",))
    narrow = upload(context, "narrow", columns + [np.full(n, 3.0)], NAMES + ("w",), np.float32)
    paired = upload(context, "paired", columns + [np.full(n, 3.0)], NAMES + ("w",), np.complex128)
    out = upload(context, "out", [np.full(n, 3.0), np.full(4*n, 3.0)], ("label", "values"))
    short = upload(context, "short", [np.full(4*n - 1, 3.0)], ("values",))
    moments = FluxMoments(context, tables, unit)
    for slot in (0, 4, 6, 7):
        mixed = list(ok)
        mixed[slot] = narrow[slot]
        with pytest.raises(GfHipError, match="one type"):
            moments.add(*mixed[:7], n, weight=mixed[7])
        mixed[slot] = paired[slot]
        with pytest.raises(GfHipError, match="fp32 or fp64"):
            moments.add(*mixed[:7], n, weight=mixed[7])
        mixed[slot] = "no such buffer"
        with pytest.raises(GfHipError, match="unknown buffer"):
            moments.add(*mixed[:7], n, weight=mixed[7])
    with pytest.raises(GfHipError, match="fp32 or fp64"):
        moments.add(*paired[:7], n)
    with pytest.raises(GfHipError, match="at least one particle"):
        moments.add(*ok[:7], 0)
    with pytest.raises(GfHipError, match="shorter"):
        moments.add(*ok[:7], n + 1)
    with pytest.raises(GfHipError, match="shorter"):
        moments.add(*narrow[:7], n + 1, weight=narrow[7])
    with pytest.raises(GfHipError, match="one type"):
        moments.values(*ok[:6], narrow[6], *out, n)
    with pytest.raises(GfHipError, match="fp64"):
        moments.values(*ok[:7], out[0], narrow[7], n)
    with pytest.raises(GfHipError, match="fp64"):
        moments.values(*ok[:7], narrow[7], out[1], n)
    with pytest.raises(GfHipError, match="shorter"):
        moments.values(*ok[:7], out[0], short[0], n)
    with pytest.raises(GfHipError, match="shorter"):
        moments.values(*ok[:7], *out, n + 1)
    with pytest.raises(GfHipError, match="at least one particle"):
        moments.values(*ok[:7], *out, 0)
    other = FluxMoments(context, tables, [0.0, 1.0])
    with pytest.raises(GfHipError, match="another shape"):
        moments.merge(other.state(), samples=5)
    with pytest.raises(GfHipError, match="another shape"):
        moments.merge(moments.state()[:, :3], samples=5)                    # nm != 4
    with pytest.raises(GfHipError, match="another shape"):
        moments.merge(np.zeros((2, 5, 67), dtype=np.int64))
    with pytest.raises(ValueError):
        moments.merge(moments.state()[0])
    seven = (ctypes.c_uint64*7)(*range(1, 8))
    for call, arguments in ((lib.gfhip_moments_state, (None,)), (lib.gfhip_moments_read, (1.0, None)), (lib.gfhip_moments_info, (None,)),
                            (lib.gfhip_moments_merge, (None, 2, 4, 1, 0, 0)), (lib.gfhip_moments_add, (None, 0, 0, 1)),
                            (lib.gfhip_moments_values, (None, 1, 2, 1))):
        assert call(moments.handle, *arguments) == 1
        assert "needs" in lib.gfhip_last_error(context.handle).decode()
        assert call(None, *arguments) == 1                                  # a null profile
    assert lib.gfhip_moments_add(None, seven, 0, 0, 1) == 1 and lib.gfhip_moments_counts(None, None, None, None) == 1
    lib.gfhip_moments_destroy(None)
    assert moments.counts() == dict(samples=0, outside=0, skipped=0)       # nothing was launched
    assert not moments.state().any()
    for key, size in zip(out, (n, 4*n)):
        assert (context.copy_to_host(key, np.empty(size)) == 3.0).all()     # the refused values() wrote nothing
    moments.add(*ok[:7], n, weight=ok[7])                                   # and the profile still works
    check(moments, moments_model.Moments(tables, unit).add(*columns, weight=np.full(n, 3.0)))
    moments.add(*narrow[:7], n)                                             # fp32 particles into the same cells
    assert moments.read()[:, 0].sum() == 3.0*n + n
    for each in (moments, other):
        each.close()


@pytest.mark.parametrize("loss", [False, True], ids=["all", "confined"])
def test_example_writes_the_moments_of_a_push(tmp_path, loss):
    """examples/push_particles.py --moments 8 as a child process, and again with --loss-limit: the file's density column
    holds every particle the counters do not call outside (the confined ones under --loss-limit), totals are the columns'
    sums, and the phase file is the one the example writes without --moments."""
    import subprocess
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    prefix = str(tmp_path / "korc")
    command = [sys.executable, os.path.join(ROOT, "examples", "push_particles.py"), "--particles", "3001", "--steps", "50",
               "--every", "25", "--label-bins", "4", "--pitch-bins", "4", "--gamma-bins", "4", "--flux-tables",
               os.path.join(GOLDEN, "efit_tables.npz"), "--output", prefix, "--moments", "8", "--moments-density", "4"]
    out = subprocess.run(command + (["--loss-limit", "0.06"] if loss else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "moments on 8 surfaces of s" in out.stdout and out.stdout.count("total current") == 2, out.stdout
    f = H5File(prefix + "_moment_bins.nc")
    bins, totals, samples, outside, skipped = (f.read(name) for name in ("bins", "totals", "samples", "outside", "skipped"))
    volume, density = f.read("volume"), f.read("density")
    assert bins.shape == (2, 8, 4) and totals.shape == (2, 4) and list(f.read("steps")) == [25.0, 50.0]
    same_bits(f.read("sbins"), np.linspace(0.0, 0.4, 9))
    f.close()
    assert list(samples) == [3001.0, 3001.0] and (skipped == 0.0).all() and (outside < 300).all()
    assert list(totals[:, 0]) == list(bins[:, :, 0].sum(axis=1))           # small integers: exact either way
    if loss:
        assert (totals[:, 0] <= samples - outside).all() and totals[-1, 0] < (samples - outside)[-1] and (totals[:, 0] > 0.0).all()
    else:
        assert list(totals[:, 0]) == list(samples - outside)
    assert (totals[:, 2] > 0.0).all() and (bins[:, :, 3] >= 0.0).all() and volume.shape == (8,)
    same_bits(density.reshape(-1), np.where(volume[None, :, None] == 0.0, np.nan, bins/volume[None, :, None]).reshape(-1))
    phase = H5File(prefix + "_phase_bins.nc")
    assert phase.read("bins").shape == (2, 4, 4, 4)
    phase.close()
