"""Particle distributions over the flux label, the pitch cosine and gamma on the device (csrc/phase_bins.hip through
gfhip_phase_*): every cell's limbs against rational arithmetic byte for byte and the three counters exactly, for fp64 and
fp32 particles, on the private and the global path; the same bytes whatever the route, the order or the shards; labels and
xi against the host's bit for bit; the marginal over pitch and gamma against FluxProfile.add; the bins of a running push
against the model fed the push's own states; and the refusals.  There is no tolerance anywhere: the arithmetic is fixed
and the sums are exact."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

import flux_model
import phase_model
from test_flux_label import same_bits
from test_phase import aligned_particles, planted_particles, random_particles

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 1025, 4099, 70001)
NAMES = ("x", "y", "z", "ux", "uy", "uz", "gamma")
DTYPES = {"f64": np.float64, "f32": np.float32}
#  (ns, np, ng), private: two private grids (the second at the cap of 256 cells), one above the cap, one barred from LDS
CASES = (((4, 4, 4), True), ((8, 8, 4), True), ((5, 9, 7), True), ((4, 4, 4), False))


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
    """70001 particles, computed once: 2040 along +-B and random ones of which a quarter lie off the map; every other block of 64
    (a wave) repeats ONE particle (the wave-uniform pre-sum of the global path); the planted ones and two with gamma on an
    edge sit among the first 128."""
    parts = [aligned_particles(tables, 2040, 4)[:7]]
    rest = COUNTS[-1] - parts[0][0].size
    parts.append(random_particles(tables, rest, 3))
    columns = [np.concatenate(c) for c in zip(*parts)]
    order = np.random.default_rng(12).permutation(COUNTS[-1])
    columns = [c[order] for c in columns]
    for start in range(0, COUNTS[-1], 128):
        for c in columns:
            c[start:start + 64] = c[start]
    planted = planted_particles(tables)
    on_edges = [np.repeat(c[:1], 2) for c in planted]                       # the good particle with gamma on an inner and on the
    on_edges[6] = np.array([2.5, 25.0])                                     # last edge of edges_of((4, 4, 4))
    assert list(flux_model.cells_of(edges_of((4, 4, 4))[2], np.array([1.0, 2.5, 25.0]))) == [0, 1, -1]
    for c, few, more in zip(columns, on_edges, planted):                    # in a block of mixed particles
        c[70:72] = few
        c[72:72 + more.size] = more
    for c in columns:
        c.setflags(write=False)
    return columns


def edges_of(shape):
    """Uniform label edges, pitch_edges and uneven gamma edges (the finder's search past its first guess)."""
    from graph_framework_amd.distribution import pitch_edges
    return np.linspace(0.0, 1.2, shape[0] + 1), pitch_edges(shape[1]), 1.0 + 24.0*np.linspace(0.0, 1.0, shape[2] + 1)**2


def upload(context, tag, columns, names=NAMES, dtype=np.float64):
    from graph_framework_amd import _lib, key_of
    kinds = {np.float64: _lib.GFIR_F64, np.float32: _lib.GFIR_F32, np.complex128: _lib.GFIR_C64}
    keys = []
    for name, column in zip(names, columns):
        key = "%s_%s" % (tag, name)
        context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), len(column), kinds[dtype]))
        context.copy_to_device(key, column)
        keys.append(key)
    return keys


def check(distribution, model, divisor=1.0):
    assert distribution.counts() == model.counts
    assert distribution.state().tobytes() == model.state().tobytes()
    same_bits(distribution.read(divisor), model.bins(divisor))


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_deposits_against_the_model_on_every_path(context, tables, pool, kind):
    from graph_framework_amd.distribution import PhaseDistribution
    dtype = DTYPES[kind]
    typed = [c.astype(dtype) for c in pool]
    for n in COUNTS:
        columns = [c[:n] for c in typed]
        keys = upload(context, "paths_%s_%d" % (kind, n), columns, dtype=dtype)
        states = {}
        for shape, private in CASES:
            edges = edges_of(shape)
            model = phase_model.Phase(tables, *edges).add(*columns)
            distribution = PhaseDistribution(context, tables, *edges, private=private)
            info = distribution.info()
            cells, edge_count = int(np.prod(shape)), sum(shape) + 3
            assert distribution.shape == shape and info["cap_cells"] == 256
            assert info["private_sums"] == (private and cells <= 256)
            assert info["workgroup_size"] == (1024 if info["private_sums"] else 256)
            assert info["lds_bytes"] == (cells*536 if info["private_sums"] else 0) + edge_count*8 <= 160*1024
            distribution.add(*keys, n)
            check(distribution, model)
            check(distribution, model, 3.0)                                 # reading again changes nothing
            states[shape, private] = distribution.state().tobytes()
            if n == COUNTS[-1]:
                assert model.counts["outside"] > n//5 and model.counts["skipped"] == 0
                assert sum(total != 0 for total in model.units) >= cells//2
                bins = model.bins()
                assert bins.sum() == n - model.counts["outside"] and bins[:, 0, :].sum() > 500 and bins[:, -1, :].sum() > 500
            distribution.close()
        assert states[(4, 4, 4), True] == states[(4, 4, 4), False]          # the same bytes without the on-chip sums


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_weights(context, tables, pool, kind):
    """No weight is a weight column of ones; seeded weights of both signs over the type's exponent range, with zeros, a
    NaN and an infinity among them, against the model, `skipped` included."""
    from graph_framework_amd.distribution import PhaseDistribution
    dtype = DTYPES[kind]
    n = 4099
    columns = [c[:n].astype(dtype) for c in pool]
    keys = upload(context, "weights_" + kind, columns, dtype=dtype)
    rng = np.random.default_rng(21)
    span = 120 if dtype == np.float32 else 1000
    weight = (rng.uniform(-1.0, 1.0, n)*2.0**rng.integers(-span, span, n).astype(np.float64)).astype(dtype)
    weight[rng.random(n) < 0.05] = 0.0
    weight[rng.random(n) < 0.02] = -0.0
    label, xi = phase_model.label_pitch(tables, *columns[:6])
    gamma = columns[6].astype(np.float64)
    inside = np.flatnonzero((label > 0.0) & (label < 1.2) & np.isfinite(xi) & (gamma > 1.0) & (gamma < 25.0))      # in a cell of every grid
    weight[inside[5]], weight[inside[70]], weight[inside[71]] = np.nan, np.inf, -np.inf
    ones, = upload(context, "weights_ones_" + kind, [np.ones(n)], ("w",), dtype)
    seeded, = upload(context, "weights_seeded_" + kind, [weight], ("w",), dtype)
    for shape, private in CASES[1:3]:                                       # the cap's grid in LDS, and the global path
        edges = edges_of(shape)
        plain, with_ones, with_weights = (PhaseDistribution(context, tables, *edges, private=private) for _ in range(3))
        plain.add(*keys, n)
        with_ones.add(*keys, n, weight=ones)
        assert plain.state().tobytes() == with_ones.state().tobytes() and plain.counts() == with_ones.counts()
        check(plain, phase_model.Phase(tables, *edges).add(*columns))
        model = phase_model.Phase(tables, *edges).add(*columns, weight=weight)
        assert model.counts["skipped"] >= 1 and any(total < 0 for total in model.units) and any(total > 0 for total in model.units)
        with_weights.add(*keys, n, weight=seeded)
        check(with_weights, model)
        for each in (plain, with_ones, with_weights):
            each.close()


def test_same_bytes_in_any_order_and_from_shards(context, tables, pool):
    from graph_framework_amd.distribution import PhaseDistribution
    n = 4099
    columns = [c[:n] for c in pool]
    edges = edges_of((4, 4, 4))
    whole = PhaseDistribution(context, tables, *edges)
    whole.add(*upload(context, "order", columns), n)
    check(whole, phase_model.Phase(tables, *edges).add(*columns))
    want, counts = whole.state().tobytes(), whole.counts()
    order = np.random.default_rng(8).permutation(n)
    shuffled = PhaseDistribution(context, tables, *edges)
    shuffled.add(*upload(context, "shuffled", [c[order] for c in columns]), n)
    assert shuffled.state().tobytes() == want and shuffled.counts() == counts
    merged = whole.like(context)
    for h, part in enumerate((order[:1777], order[1777:3000], order[3000:])):
        shard = PhaseDistribution(context, tables, *edges, private=h != 1)
        shard.add(*upload(context, "shard%d" % h, [c[part] for c in columns]), part.size)
        merged.merge(shard.state(), **shard.counts())
        shard.close()
    assert merged.state().tobytes() == want and merged.counts() == counts
    same_bits(merged.read(5.0), whole.read(5.0))
    for each in (whole, shuffled, merged):
        each.close()


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_coordinates_equal_the_hosts_bit_for_bit(context, tables, pool, kind):
    from graph_framework_amd.distribution import PhaseDistribution, coordinates_host
    dtype = DTYPES[kind]
    n = 4099
    columns = [c[:n].astype(dtype) for c in pool]
    keys = upload(context, "coordinates_" + kind, columns, dtype=dtype)
    out = upload(context, "coordinates_out_" + kind, [np.full(n, 7.0), np.full(n, 7.0)], ("label", "pitch"))
    for options in (dict(), dict(sqrt_label=True), dict(psi0=0.25, span=-0.125)):
        distribution = PhaseDistribution(context, tables, [0.0, 1.0], [-1.0, 1.0], [1.0, 2.0], **options)
        distribution.coordinates(*keys, *out, n)
        got = [context.copy_to_host(key, np.empty(n)) for key in out]
        want = coordinates_host(tables, columns, **options)
        same_bits(got[0], want[0])
        same_bits(got[1], want[1])
        model = phase_model.label_pitch(tables, *columns[:6], **options)
        same_bits(got[0], model[0])
        same_bits(got[1], model[1])
        assert distribution.counts() == dict(samples=0, outside=0, skipped=0)                   # nothing is deposited
        distribution.close()
    assert np.isnan(want[1]).sum() > 500 and (np.abs(want[1]) > 1.0 - 1.0e-12).sum() > 20
    if kind == "f64":                                                       # fp32 momenta are no longer along B to the last bit
        assert (want[1] == 1.0).any() and (want[1] == -1.0).any()


def test_the_marginal_over_pitch_and_gamma_is_the_flux_profile(context, tables, pool):
    """Pitch and gamma edges that hold every particle on the map with u != 0: profile() is FluxProfile.add's state on
    the same positions with a column of ones, byte for byte; the planted particles whose xi or gamma is no number are
    `outside` here and inside there."""
    from graph_framework_amd.distribution import PhaseDistribution, pitch_edges
    from graph_framework_amd.flux import FluxProfile
    n = 4099
    columns = [c[:n].copy() for c in pool]
    for c, planted in zip(columns, planted_particles(tables)):
        c[64:64 + planted.size] = planted                                   # a block of mixed particles
    sedges = np.linspace(0.0, 1.2, 9)
    label, xi = phase_model.label_pitch(tables, *columns[:6])
    undefined = (flux_model.cells_of(sedges, label) >= 0) & ~(np.isfinite(xi) & np.isfinite(columns[6]))
    assert 13 <= undefined.sum() < 64                                       # u = 0, 9 x u and 3 x gamma that are no numbers
    gedges = np.array([0.5, 2.0, 1.0e3])
    keys = upload(context, "marginal", columns + [np.ones(n)], NAMES + ("one",))
    distribution = PhaseDistribution(context, tables, sedges, pitch_edges(3), gedges)
    distribution.add(*keys[:7], n)
    profile = FluxProfile(context, tables, sedges)
    profile.add(keys[0], keys[1], keys[2], keys[7], n)
    defined = PhaseDistribution(context, tables, sedges, pitch_edges(3), gedges)               # the same without those particles
    kept = [c[~undefined] for c in columns]
    defined.add(*upload(context, "marginal_defined", kept), kept[0].size)
    exact = FluxProfile(context, tables, sedges)
    exact.add(*upload(context, "marginal_defined_xyz1", kept[:3] + [np.ones(kept[0].size)], ("x", "y", "z", "one")), kept[0].size)
    marginal, marginal_defined = distribution.profile(), defined.profile()
    assert marginal_defined.state().tobytes() == exact.state().tobytes() and exact.state().any()
    assert marginal_defined.counts() == exact.counts() == defined.counts()
    assert marginal.state().tobytes() == marginal_defined.state().tobytes()
    ours, theirs = marginal.counts(), profile.counts()
    assert ours == distribution.counts() and ours["samples"] == theirs["samples"] == n
    assert ours["outside"] == theirs["outside"] + int(undefined.sum()) and ours["skipped"] == theirs["skipped"] == 0
    same_bits(marginal.read(2.0), exact.read(2.0))
    for each in (distribution, profile, defined, exact, marginal, marginal_defined):
        each.close()


@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_bins_behind_the_push(tables, kind):
    """The ensemble of test_korc_random_particles_bit_exact_against_the_oracle: 25 steps, bin, 25 steps, bin, on the
    push's own context and stream; the state is the model's fed the two sync_host() states, and no particle is left out."""
    from graph_framework_amd import Context, korc
    from graph_framework_amd.distribution import PhaseDistribution, pitch_edges
    rng = np.random.default_rng(17)
    n = 3001
    particles = dict(x=rng.uniform(1.5, 1.9, n), y=rng.uniform(-0.2, 0.2, n), z=rng.uniform(-0.3, 0.3, n),
                     ux=rng.uniform(-0.3, 0.3, n), uy=rng.uniform(0.3, 0.85, n), uz=rng.uniform(-0.3, 0.3, n),
                     gamma=np.zeros(n))
    push = korc.Korc(particles, kind)
    push.compile()
    push.pre_run()
    edges = (np.linspace(-0.01, 0.25, 5), pitch_edges(4), np.linspace(1.0, 3.0, 5))
    distribution = PhaseDistribution(push.work.context, tables, *edges)
    model = phase_model.Phase(tables, *edges)
    for _ in range(2):
        push.run(25)
        push.bin(distribution)
        host = push.sync_host()
        assert host["x"].dtype == DTYPES[kind]
        model.add(*[host[k] for k in korc.PARTICLE])
    check(distribution, model)
    counts = distribution.counts()
    assert counts == dict(samples=2*n, outside=0, skipped=0)
    assert distribution.read().sum() == 2*n and (distribution.read() != 0.0).sum() >= 8
    elsewhere = Context(0)
    foreign = distribution.like(elsewhere)
    with pytest.raises(ValueError):
        push.bin(foreign)                                                   # not on the push's context
    foreign.close()
    elsewhere.close()
    distribution.close()
    push.work.context.close()


def test_misuse_is_refused_before_anything_runs(context, tables, pool):
    from graph_framework_amd import GfHipError
    from graph_framework_amd.distribution import PhaseDistribution
    from graph_framework_amd.flux import flux_map
    from graph_framework_amd.spectrum import spectrum_field
    lib = context.lib

    def refused(match, given, field, *axes, sizes=None):
        axes = [np.ascontiguousarray(e, dtype=np.float64) for e in axes]
        sizes = sizes or [e.size - 1 for e in axes]
        arguments = []
        for e, size in zip(axes, sizes):
            arguments += [e.ctypes.data if e.size else None, size]
        handle = lib.gfhip_phase_create(context.handle, ctypes.byref(given) if given is not None else None,
                                        ctypes.byref(field) if field is not None else None, *arguments)
        assert not handle
        assert match in lib.gfhip_last_error(context.handle).decode(), lib.gfhip_last_error(context.handle).decode()

    good, keep = flux_map(tables)
    field, keep_field = spectrum_field(tables)
    unit, pair = np.array([0.0, 0.5, 1.0]), np.array([-1.0, 1.0])
    refused("needs a map", None, field, unit, pair, pair)
    refused("needs a map", good, None, unit, pair, pair)
    for axis in range(3):
        axes = [unit, pair, pair]
        axes[axis] = np.array([])
        refused("needs a map", good, field, *axes, sizes=[2, 1, 1])
        axes[axis] = np.array([0.5])                                        # one edge: no cell
        refused("at least two edges", good, field, *axes)
        axes[axis] = np.arange(4098.0)
        refused("1 to 4096 cells per axis", good, field, *axes)
        for edges in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 1.0], [0.0, np.inf]):
            axes[axis] = np.array(edges)
            refused("strictly increasing", good, field, *axes)
    refused("at most 2^20 cells", good, field, np.arange(129.0), np.arange(129.0), np.arange(66.0))
    broken, keep_broken = spectrum_field(tables)
    broken.fpol[1] = None
    refused("four fpol tables", good, broken, unit, pair, pair)
    broken, keep_broken = spectrum_field(tables)
    broken.reserved = 3
    refused("reserved", good, broken, unit, pair, pair)
    broken_map, keep_map = flux_map(tables)
    broken_map.reserved = 1
    refused("reserved", broken_map, field, unit, pair, pair)
    ignored, keep_ignored = spectrum_field(tables)
    ignored.c = 0.0                                                         # c takes no part: accepted
    handle = lib.gfhip_phase_create(context.handle, ctypes.byref(good), ctypes.byref(ignored), unit.ctypes.data, 2, pair.ctypes.data, 1,
                                    pair.ctypes.data, 1)
    assert handle
    lib.gfhip_phase_destroy(handle)
    with pytest.raises(ValueError):
        PhaseDistribution(context, tables, [0.0], pair, pair)

    n = 64
    columns = [np.full(n, v) for v in (1.9, 0.0, 0.0, 0.3, 0.5, 0.1, 1.5)]
    label, xi = phase_model.label_pitch(tables, *[c[:1] for c in columns[:6]])
    assert 0.0 < label[0] < 1.0 and -1.0 < xi[0] < 1.0
    ok = upload(context, "ok", columns + [np.full(n, 3.0)], NAMES + ("w",))
    narrow = upload(context, "narrow", columns + [np.full(n, 3.0)], NAMES + ("w",), np.float32)
    paired = upload(context, "paired", columns + [np.full(n, 3.0)], NAMES + ("w",), np.complex128)
    out = upload(context, "out", [np.full(n, 3.0), np.full(n, 3.0)], ("label", "pitch"))
    gedges = np.array([1.0, 2.0])
    distribution = PhaseDistribution(context, tables, unit, pair, gedges)
    for slot in (0, 4, 6, 7):
        mixed = list(ok)
        mixed[slot] = narrow[slot]
        with pytest.raises(GfHipError, match="one type"):
            distribution.add(*mixed[:7], n, weight=mixed[7])
        mixed[slot] = paired[slot]
        with pytest.raises(GfHipError, match="fp32 or fp64"):
            distribution.add(*mixed[:7], n, weight=mixed[7])
        mixed[slot] = "no such buffer"
        with pytest.raises(GfHipError, match="unknown buffer"):
            distribution.add(*mixed[:7], n, weight=mixed[7])
    with pytest.raises(GfHipError, match="fp32 or fp64"):
        distribution.add(*paired[:7], n)
    with pytest.raises(GfHipError, match="shorter"):
        distribution.add(*ok[:7], n + 1)
    with pytest.raises(GfHipError, match="shorter"):
        distribution.add(*narrow[:7], n + 1, weight=narrow[7])
    with pytest.raises(GfHipError, match="one type"):
        distribution.coordinates(*ok[:6], narrow[6], *out, n)
    with pytest.raises(GfHipError, match="fp64"):
        distribution.coordinates(*ok[:7], out[0], narrow[7], n)
    with pytest.raises(GfHipError, match="shorter"):
        distribution.coordinates(*ok[:7], *out, n + 1)
    others = [PhaseDistribution(context, tables, *axes) for axes in ((pair, unit, gedges), (unit, pair, [1.0, 1.5, 2.0]),
                                                                      (pair, pair, gedges), (unit, unit, gedges))]
    for another in others:
        with pytest.raises(GfHipError, match="another shape"):
            distribution.merge(another.state(), samples=5)
    with pytest.raises(ValueError):
        distribution.merge(others[0].state()[0])
    seven = (ctypes.c_uint64*7)(*range(1, 8))
    for call, arguments in ((lib.gfhip_phase_state, (None,)), (lib.gfhip_phase_read, (1.0, None)), (lib.gfhip_phase_info, (None,)),
                            (lib.gfhip_phase_merge, (None, 2, 1, 1, 1, 0, 0)), (lib.gfhip_phase_add, (None, 0, 0, 1)),
                            (lib.gfhip_phase_coordinates, (None, 1, 2, 1))):
        assert call(distribution.handle, *arguments) == 1
        assert "needs" in lib.gfhip_last_error(context.handle).decode()
        assert call(None, *arguments) == 1                                  # a null distribution
    assert lib.gfhip_phase_add(None, seven, 0, 0, 1) == 1 and lib.gfhip_phase_counts(None, None, None, None) == 1
    lib.gfhip_phase_destroy(None)
    assert distribution.counts() == dict(samples=0, outside=0, skipped=0)  # nothing was launched
    assert not distribution.state().any()
    for key in out:
        assert (context.copy_to_host(key, np.empty(n)) == 3.0).all()        # the refused coordinates() wrote nothing
    distribution.add(*ok[:7], n, weight=ok[7])                              # and the distribution still works
    check(distribution, phase_model.Phase(tables, unit, pair, gedges).add(*columns, weight=np.full(n, 3.0)))
    distribution.add(*narrow[:7], n)                                        # fp32 particles into the same cells
    assert distribution.read().sum() == 3.0*n + n
    for each in [distribution] + others:
        each.close()


def test_example_writes_the_snapshots_of_a_push(tmp_path):
    """examples/push_particles.py as a child process: 3001 fp32 particles, a snapshot every 25 of 50 steps; the file's
    bins hold every particle that the counters do not call outside, and the gamma marginal is reported."""
    import subprocess
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    from graph_framework_amd.distribution import pitch_edges
    prefix = str(tmp_path / "korc")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "push_particles.py"), "--particles", "3001", "--steps", "50",
                          "--every", "25", "--label-bins", "4", "--pitch-bins", "4", "--gamma-bins", "4", "--flux-tables",
                          os.path.join(GOLDEN, "efit_tables.npz"), "--output", prefix], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "2 snapshots on 4x4x4 cells of s, xi and gamma" in out.stdout, out.stdout
    assert "largest change of the gamma marginal between the first and the last snapshot:" in out.stdout
    f = H5File(prefix + "_phase_bins.nc")
    bins, samples, outside = f.read("bins"), f.read("samples"), f.read("outside")
    assert bins.shape == (2, 4, 4, 4) and list(f.read("steps")) == [25.0, 50.0] and list(samples) == [3001.0, 3001.0]
    same_bits(f.read("pbins"), pitch_edges(4))
    same_bits(f.read("sbins"), np.linspace(0.0, 0.4, 5))
    same_bits(f.read("gbins"), np.linspace(1.0, 3.0, 5))
    f.close()
    assert list(bins.sum(axis=(1, 2, 3))) == list(samples - outside) and (outside < 300).all() and (bins.sum(axis=(1, 3)) > 0).all()
