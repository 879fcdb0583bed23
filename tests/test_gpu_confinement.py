"""First-exit tracking on the device (csrc/confinement.hip through gfhip_confine_*): lost_step, alive, the exit buffers,
newly_lost, every cell's limbs and the three counters against the model of tests/confinement_model.py byte for byte, for
fp64 and fp32 particles, over three checks in a row; whole waves confined, lost, lost into one cell and lost into 64
cells; weights; the same cells whatever the order or the shards; a running push; Korc.bin under the alive weights; the
refusals; the example.  There is no tolerance anywhere: the arithmetic is fixed and the sums are exact."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

import confinement_model
import flux_model
import phase_model
from test_confinement import CONFINED, DTYPES, STEPS, ensembles, loss_edges, map_box, weights_of
from test_flux_label import same_bits
from test_gpu_phase import NAMES, upload

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 1025, 4099)


@pytest.fixture(scope="module")
def context():
    from graph_framework_amd import Context
    context = Context(0)
    yield context
    context.close()


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(os.path.join(GOLDEN, "efit_tables.npz")))


def exits_of(context, tag, n):
    return upload(context, tag, [np.full(n, 7.0), np.full(n, 7.0)], ("exit_r", "exit_z"))


def equals_model(context, tracker, model, exit_keys=None):
    n = model.lost_step.size
    assert tracker.lost_steps().tobytes() == model.lost_step.tobytes()
    alive = context.copy_to_host(tracker.alive_key, np.empty(n, dtype=tracker.dtype))
    assert alive.astype(np.float64).tobytes() == model.alive.tobytes()
    if exit_keys is not None:
        same_bits(context.copy_to_host(exit_keys[0], np.empty(n)), model.exit_r)
        same_bits(context.copy_to_host(exit_keys[1], np.empty(n)), model.exit_z)
    history = tracker.history()
    assert list(history["steps"]) == model.steps and list(history["newly_lost"]) == model.newly_lost
    assert list(history["confined"]) == list(model.confined()) and tracker.confined() == (model.confined()[-1] if model.steps else n)
    assert tracker.counts() == model.counts
    assert tracker.state().tobytes() == model.state().tobytes()
    same_bits(tracker.read(), model.bins())


def run_checks(context, tables, tag, states, limit, dtype, edges, weight=None, with_exit=True, steps=STEPS, **options):
    """A tracker and its model after one check per state, compared after every check."""
    from graph_framework_amd.confinement import Confinement
    n = states[0][0].size
    tracker = Confinement(context, tables, *edges, n, dtype, limit=limit, alive=tag + "_alive", capacity=len(states), **options)
    model = confinement_model.Confinement(tables, *edges, n, limit, **options)
    exit_keys = exits_of(context, tag, n) if with_exit else None
    weight_key = None if weight is None else upload(context, tag, [weight], ("w",), dtype)[0]
    equals_model(context, tracker, model)
    for number, (columns, step) in enumerate(zip(states, steps)):
        keys = upload(context, "%s_%d" % (tag, number), columns, dtype=dtype)
        tracker.check(*keys, step, weight=weight_key, exit=exit_keys)
        model.check(*columns, step, weight)
        equals_model(context, tracker, model, exit_keys)
    return tracker, model


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_three_checks_against_the_model(context, tables, kind):
    dtype = DTYPES[kind]
    edges = loss_edges(tables)
    for n in COUNTS:
        states, limit, rows = ensembles(tables, n, dtype)
        tracker, model = run_checks(context, tables, "checks_%s_%d" % (kind, n), states, limit, dtype, edges)
        info = tracker.info()
        assert tracker.shape == (5, 6, 4) and not info["private_sums"] and info["workgroup_size"] == 256
        assert info["lds_bytes"] == (5 + 6 + 4 + 3)*8
        if n == COUNTS[-1]:
            assert all(k > 0 for k in model.newly_lost) and model.confined()[-1] > 0 and model.counts["outside"] > 0
            came_back = (model.lost_step == STEPS[0]) & (model.labels(*states[1][:3]) < limit)
            assert came_back.sum() > 50 and model.deposits.max() == 1       # settled once, whatever a later step does
            assert model.lost_step[rows["equal"]] == STEPS[0] and model.lost_step[rows["below"]] == CONFINED
            assert model.lost_step[rows["below_rmin"]] == STEPS[0] and model.labels(*(c[1:2] for c in states[2][:3]))[0] < limit
        tracker.close()


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_whole_waves_confined_lost_and_lost_into_one_and_into_64_cells(context, tables, kind):
    """256 particles, four waves: all confined; all lost at one point, without weights (the pre-sum's shared limbs); 64
    lanes lost into the 64 cells of an 8 x 8 x 1 footprint; mixed.  Then 4099 all confined and 4099 all lost."""
    dtype = DTYPES[kind]
    rlo, rhi, zlo, zhi = map_box(tables)
    edges = (np.linspace(rlo, rhi, 9), np.linspace(zlo, zhi, 9), np.array([1.0, 25.0]))
    limit = 0.05
    states, _, rows = ensembles(tables, 256, dtype)
    first = states[0]
    centres = [0.5*(e[1:] + e[:-1]) for e in edges[:2]]
    for c, inside, lost, across in zip(first[:3], (first[0][rows["axis"]], 0.0, first[2][rows["axis"]]), (rhi - 0.3, 0.0, 0.7),
                                       (np.repeat(centres[0], 8), np.zeros(64), np.tile(centres[1], 8))):
        c[:64], c[64:128], c[128:192] = inside, lost, across
    first[6][:192] = 1.8
    first = [c.astype(dtype) for c in first]
    tracker, model = run_checks(context, tables, "waves_" + kind, [first] + states[1:], limit, dtype, edges)
    at_first = confinement_model.Confinement(tables, *edges, 256, limit).check(*first, STEPS[0])
    assert (at_first.lost_step[:64] == CONFINED).all() and (at_first.lost_step[64:192] == STEPS[0]).all()
    bins = model.bins()
    one = flux_model.cells_of(edges[0], np.array([rhi - 0.3]))[0], flux_model.cells_of(edges[1], np.array([np.float64(dtype(0.7))]))[0]
    assert bins[one[0], one[1], 0] >= 65                                    # the wave, and one of the 64
    r, z = confinement_model.radius(first[0][128:192], first[1][128:192]), first[2][128:192].astype(np.float64)
    cells = flux_model.cells_of(edges[0], r)*8 + flux_model.cells_of(edges[1], z)
    assert sorted(cells) == list(range(64))
    tracker.close()
    n = 4099
    states, _, rows = ensembles(tables, n, dtype)
    kept = [[np.full(n, c[rows["axis"]]) for c in columns] for columns in states]
    tracker, model = run_checks(context, tables, "kept_" + kind, kept, limit, dtype, edges)
    assert model.newly_lost == [0, 0, 0] and tracker.confined() == n and not tracker.state().any()
    tracker.close()
    gone = [[c.copy() for c in columns] for columns in states]
    for columns in gone:
        columns[0][:] += dtype(10.0)                                        # off the map, and outside the footprint
        columns[0][::2] = dtype(rhi - 0.3)
        columns[1][::2] = 0.0
        columns[2][::2] = dtype(0.7)
    tracker, model = run_checks(context, tables, "gone_" + kind, gone, limit, dtype, edges)
    assert model.newly_lost == [n, 0, 0] and tracker.confined() == 0 and model.counts["outside"] > 1000
    tracker.close()


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_weights_and_the_marginals(context, tables, kind):
    """Seeded weights of both signs with zeros, a NaN and +-inf among the lost; footprint() and spectrum() are the
    model's cells summed over gamma, and over R and z, in rational arithmetic and rounded once."""
    dtype = DTYPES[kind]
    n = 4099
    states, limit, _ = ensembles(tables, n, dtype)
    edges = loss_edges(tables)
    plain = confinement_model.Confinement(tables, *edges, n, limit).check(*states[0], STEPS[0])
    in_cell = [i for i in np.flatnonzero(plain.lost_step == STEPS[0]) if np.isfinite(plain.exit_r[i]) and all(
        flux_model.cells_of(e, np.array([v]))[0] >= 0 for e, v in zip(edges, (plain.exit_r[i], plain.exit_z[i], np.float64(states[0][6][i]))))]
    weight = weights_of(n, dtype)
    weight[in_cell[0]], weight[in_cell[1]], weight[in_cell[2]] = np.nan, np.inf, -np.inf
    tracker, model = run_checks(context, tables, "weights_" + kind, states, limit, dtype, edges, weight=weight)
    assert model.counts["skipped"] == 3 and any(total < 0 for total in model.units) and any(total > 0 for total in model.units)
    units = np.array(model.units, dtype=object).reshape(model.shape)
    same_bits(tracker.footprint(), np.array([[phase_model.rounded(int(total)) for total in row] for row in units.sum(axis=2)]))
    same_bits(tracker.spectrum(), np.array([phase_model.rounded(int(total)) for total in units.sum(axis=(0, 1))]))
    tracker.close()
    ones = np.ones(n, dtype=dtype)                                          # no weight is a weight column of ones
    with_ones, _ = run_checks(context, tables, "ones_" + kind, states, limit, dtype, edges, weight=ones)
    without, _ = run_checks(context, tables, "none_" + kind, states, limit, dtype, edges)
    assert with_ones.state().tobytes() == without.state().tobytes() and with_ones.counts() == without.counts()
    with_ones.close()
    without.close()


def test_same_cells_in_any_order_from_shards_and_without_exit_buffers(context, tables):
    n = 4099
    dtype = np.float64
    states, limit, _ = ensembles(tables, n, dtype)
    edges = loss_edges(tables)
    weight = weights_of(n, dtype)
    whole, model = run_checks(context, tables, "whole", states, limit, dtype, edges, weight=weight)
    want, counts, steps = whole.state().tobytes(), whole.counts(), whole.lost_steps()
    order = np.random.default_rng(8).permutation(n)
    shuffled, _ = run_checks(context, tables, "shuffled", [[c[order] for c in columns] for columns in states], limit, dtype, edges,
                             weight=weight[order])
    assert shuffled.state().tobytes() == want and shuffled.counts() == counts
    assert shuffled.lost_steps().tobytes() == steps[order].tobytes()
    merged = whole.like(context, alive="merged_alive", count=1)
    for h, part in enumerate((order[:1777], order[1777:3000], order[3000:])):
        shard, _ = run_checks(context, tables, "shard%d" % h, [[c[part] for c in columns] for columns in states], limit, dtype, edges,
                              weight=weight[part])
        merged.merge(shard.state(), **shard.counts())
        shard.close()
    assert merged.state().tobytes() == want and merged.counts() == counts
    same_bits(merged.read(5.0), whole.read(5.0))
    bare, _ = run_checks(context, tables, "bare", states, limit, dtype, edges, weight=weight, with_exit=False)
    assert bare.state().tobytes() == want and bare.counts() == counts and bare.lost_steps().tobytes() == steps.tobytes()
    assert bare.history()["newly_lost"].tobytes() == whole.history()["newly_lost"].tobytes()
    for each in (whole, shuffled, merged, bare):
        each.close()


@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_tracking_and_binning_behind_the_push(tables, kind):
    """The 3001-particle push of tests/test_gpu_phase.py, tracked after 25 and after 50 steps on the push's own context
    and stream, against the model fed the two sync_host() states.  The limit is the median of the model's finite labels at
    step 25 (the oracle's push of this ensemble loses 1501 particles at step 25 and one more at step 50, in both types).
    Then Korc.bin under the alive weights: the snapshot is the model's of the confined particles only."""
    from graph_framework_amd import korc
    from graph_framework_amd.confinement import Confinement
    from graph_framework_amd.distribution import PhaseDistribution, pitch_edges
    rng = np.random.default_rng(17)
    n = 3001
    particles = dict(x=rng.uniform(1.5, 1.9, n), y=rng.uniform(-0.2, 0.2, n), z=rng.uniform(-0.3, 0.3, n),
                     ux=rng.uniform(-0.3, 0.3, n), uy=rng.uniform(0.3, 0.85, n), uz=rng.uniform(-0.3, 0.3, n),
                     gamma=np.zeros(n))
    push = korc.Korc(particles, kind)
    push.compile()
    push.pre_run()
    context = push.work.context
    assert push.steps_done == 0
    push.run(25)
    first = {k: v.copy() for k, v in push.sync_host().items()}
    label = flux_model.label(tables, *(first[k].astype(np.float64) for k in "xyz"))
    limit = float(np.median(label[np.isfinite(label)]))
    edges = (np.linspace(1.2, 2.2, 9), np.linspace(-0.6, 0.6, 7), np.linspace(1.0, 3.0, 5))
    tracker = Confinement(context, tables, *edges, n, kind, limit=limit, capacity=2)
    model = confinement_model.Confinement(tables, *edges, n, limit)
    exit_keys = exits_of(context, "push", n)
    push.track(tracker, exit=exit_keys)
    model.check(*[first[k] for k in korc.PARTICLE], 25)
    equals_model(context, tracker, model, exit_keys)
    push.run(25)
    assert push.steps_done == 50
    push.track(tracker, exit=exit_keys)
    host = push.sync_host()
    assert host["x"].dtype == DTYPES[kind]
    model.check(*[host[k] for k in korc.PARTICLE], 50)
    assert model.newly_lost[0] >= 1 and model.newly_lost[1] >= 1 and model.confined()[-1] >= 1
    equals_model(context, tracker, model, exit_keys)
    assert model.steps == [25, 50] and tracker.read().sum() == sum(model.newly_lost) - model.counts["outside"]
    sedges = (np.linspace(-0.01, 0.25, 5), pitch_edges(4), np.linspace(1.0, 3.0, 5))
    snapshot = PhaseDistribution(context, tables, *sedges)
    push.bin(snapshot, weight=tracker.alive_key)
    columns = [host[k] for k in korc.PARTICLE]
    weighted = phase_model.Phase(tables, *sedges).add(*columns, weight=model.alive)
    confined = model.lost_step == CONFINED
    only = phase_model.Phase(tables, *sedges).add(*[c[confined] for c in columns])
    assert snapshot.state().tobytes() == weighted.state().tobytes() == only.state().tobytes()
    assert snapshot.counts() == weighted.counts and snapshot.read().sum() == confined.sum() - only.counts["outside"]
    everyone = PhaseDistribution(context, tables, *sedges)
    push.bin(everyone)
    assert everyone.read().sum() > snapshot.read().sum()                   # the lost ones dropped out
    with pytest.raises(ValueError):
        push.track(tracker.like(context, alive="short_alive", count=n - 1))
    for each in (snapshot, everyone, tracker):
        each.close()
    context.close()


def test_misuse_is_refused_before_anything_runs(context, tables):
    from graph_framework_amd import GfHipError, key_of
    from graph_framework_amd.confinement import Confinement
    from graph_framework_amd.flux import flux_map
    lib = context.lib

    def refused(match, given, *axes, sizes=None, limit=1.0, count=64, capacity=4):
        axes = [np.ascontiguousarray(e, dtype=np.float64) for e in axes]
        sizes = sizes or [e.size - 1 for e in axes]
        arguments = []
        for e, size in zip(axes, sizes):
            arguments += [e.ctypes.data if e.size else None, size]
        handle = lib.gfhip_confine_create(context.handle, ctypes.byref(given) if given is not None else None, limit, *arguments,
                                          count, 0, key_of("refused_alive"), capacity)
        assert not handle
        assert match in lib.gfhip_last_error(context.handle).decode(), lib.gfhip_last_error(context.handle).decode()

    good, keep = flux_map(tables)
    unit, pair = np.array([1.0, 1.5, 2.5]), np.array([-1.0, 1.0])
    refused("needs a map", None, unit, pair, pair)
    for axis in range(3):
        axes = [unit, pair, pair]
        axes[axis] = np.array([])
        refused("needs a map", good, *axes, sizes=[2, 1, 1])
        axes[axis] = np.array([0.5])                                        # one edge: no cell
        refused("at least two edges", good, *axes)
        axes[axis] = np.arange(4098.0)
        refused("1 to 4096 cells per axis", good, *axes)
        for edges in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 1.0], [0.0, np.inf]):
            axes[axis] = np.array(edges)
            refused("strictly increasing", good, *axes)
    refused("at most 2^20 cells", good, np.arange(129.0), np.arange(129.0), np.arange(66.0))
    broken, keep_broken = flux_map(tables)
    broken.reserved = 1
    refused("reserved", broken, unit, pair, pair)
    refused("NaN", good, unit, pair, pair, limit=np.nan)
    refused("at least one particle", good, unit, pair, pair, count=0)
    refused("at least one check", good, unit, pair, pair, capacity=0)
    with pytest.raises(GfHipError, match="unknown buffer"):
        context.buffer_info("refused_alive")                                # no refused tracker left a buffer behind
    with pytest.raises(ValueError):
        Confinement(context, tables, [1.0], pair, pair, 64, "f64")
    with pytest.raises(ValueError):
        Confinement(context, tables, unit, pair, pair, 64, np.complex128)

    n = 64
    rlo, rhi, zlo, zhi = map_box(tables)
    columns = [np.full(n, v) for v in (rhi - 0.3, 0.0, 0.7, 0.3, 0.5, 0.1, 1.5)]                # lost at the limit below, in a cell
    gedges = np.array([1.0, 2.0])
    edges = (np.array([rlo, 1.7, rhi]), np.array([zlo, zhi]), gedges)
    assert flux_model.label(tables, *[c[:1] for c in columns[:3]])[0] > 0.05
    ok = upload(context, "c_ok", columns + [np.full(n, 3.0)], NAMES + ("w",))
    narrow = upload(context, "c_narrow", columns + [np.full(n, 3.0)], NAMES + ("w",), np.float32)
    paired = upload(context, "c_paired", columns + [np.full(n, 3.0)], NAMES + ("w",), np.complex128)
    short = upload(context, "c_short", [c[:-1] for c in columns], NAMES)
    out = exits_of(context, "c_out", n)
    narrow_out = upload(context, "c_narrow_out", [np.full(n, 7.0), np.full(n - 1, 7.0)], ("exit_r", "exit_z"), np.float32)
    short_out = upload(context, "c_short_out", [np.full(n - 1, 7.0)], ("exit_z",))
    tracker = Confinement(context, tables, *edges, n, "f64", limit=0.05, alive="c_alive", capacity=2)
    single = Confinement(context, tables, *edges, n, "f32", limit=0.05, alive="c_alive32", capacity=2)
    for slot in (0, 2, 6, 7):
        mixed = list(ok)
        mixed[slot] = narrow[slot]
        with pytest.raises(GfHipError, match="one type"):
            tracker.check(*mixed[:7], 1, weight=mixed[7])
        mixed[slot] = paired[slot]
        with pytest.raises(GfHipError, match="fp32 or fp64"):
            tracker.check(*mixed[:7], 1, weight=mixed[7])
        mixed[slot] = "no such buffer"
        with pytest.raises(GfHipError, match="unknown buffer"):
            tracker.check(*mixed[:7], 1, weight=mixed[7])
    with pytest.raises(GfHipError, match="tracker's type"):
        tracker.check(*narrow[:7], 1)
    with pytest.raises(GfHipError, match="tracker's type"):
        single.check(*ok[:7], 1, weight=ok[7])
    with pytest.raises(GfHipError, match="shorter"):
        tracker.check(*short, 1)                                            # count above the buffers' length
    with pytest.raises(GfHipError, match="fp64"):
        tracker.check(*ok[:7], 1, exit=(out[0], narrow_out[0]))
    with pytest.raises(GfHipError, match="shorter"):
        tracker.check(*ok[:7], 1, exit=(out[0], short_out[0]))
    with pytest.raises(GfHipError, match="unknown buffer"):
        tracker.check(*ok[:7], 1, exit=(out[0], "no such buffer"))
    with pytest.raises(GfHipError, match="0xFFFFFFFF"):
        tracker.check(*ok[:7], CONFINED, exit=out)
    with pytest.raises(ValueError):
        tracker.check(*ok[:7], CONFINED + 1)
    with pytest.raises(TypeError):
        tracker.add(*ok[:4], n)
    others = [Confinement(context, tables, *axes, 1, "f64", alive="c_other%d" % k, capacity=1)
              for k, axes in enumerate(((edges[1], edges[0], gedges), (edges[0], edges[1], [1.0, 1.5, 2.0]), (edges[1], edges[1], gedges)))]
    for another in others:
        with pytest.raises(GfHipError, match="another shape"):
            tracker.merge(another.state(), samples=5)
    with pytest.raises(ValueError):
        tracker.merge(others[0].state()[0])
    seven = (ctypes.c_uint64*7)(*range(1, 8))
    size = ctypes.c_size_t()
    for call, arguments in ((lib.gfhip_confine_state, (None,)), (lib.gfhip_confine_read, (1.0, None)), (lib.gfhip_confine_info, (None,)),
                            (lib.gfhip_confine_merge, (None, 2, 1, 1, 1, 0, 0)), (lib.gfhip_confine_check, (None, 0, 0, 0, 0, 0, 1)),
                            (lib.gfhip_confine_lost_steps, (None,)), (lib.gfhip_confine_history, (None, None, None))):
        assert call(tracker.handle, *arguments) == 1
        assert "needs" in lib.gfhip_last_error(context.handle).decode()
        assert call(None, *arguments) == 1                                  # a null tracker
    assert lib.gfhip_confine_check(None, seven, 0, 0, 0, 0, 0, 1) == 1 and lib.gfhip_confine_counts(None, None, None, None) == 1
    assert lib.gfhip_confine_history(None, None, None, ctypes.byref(size)) == 1
    lib.gfhip_confine_destroy(None)

    def untouched(each):
        assert each.counts() == dict(samples=0, outside=0, skipped=0) and not each.state().any()
        assert (each.lost_steps() == CONFINED).all() and each.history()["steps"].size == 0 and each.confined() == n
        assert (context.copy_to_host(each.alive_key, np.empty(n, dtype=each.dtype)) == 1).all()

    untouched(tracker)
    untouched(single)
    for key in out:
        assert (context.copy_to_host(key, np.empty(n)) == 7.0).all()        # no refused check wrote an exit
    tracker.check(*ok[:7], 5, weight=ok[7], exit=out)                       # and the tracker still works
    model = confinement_model.Confinement(tables, *edges, n, 0.05).check(*columns, 5, np.full(n, 3.0))
    equals_model(context, tracker, model, out)
    assert model.newly_lost == [n] and tracker.read().sum() == 3.0*n
    with pytest.raises(GfHipError, match="below the previous"):
        tracker.check(*ok[:7], 4, exit=out)
    tracker.check(*ok[:7], 5, exit=out)                                     # the same step again is allowed
    model.check(*columns, 5)
    with pytest.raises(GfHipError, match="capacity"):
        tracker.check(*ok[:7], 6, exit=out)
    equals_model(context, tracker, model, out)
    single.check(*narrow[:7], 0)                                            # fp32 particles of equal values: the same cells
    assert single.read().sum() == n and single.lost_steps().tobytes() == np.zeros(n, dtype=np.uint32).tobytes()
    for each in [tracker, single] + others:
        each.close()


def test_example_tracks_the_losses_of_a_push(tmp_path):
    """examples/push_particles.py as a child process with the loss flags: every particle is confined at the end or was
    counted lost once; the snapshots hold no more than the confined."""
    import subprocess
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    prefix = str(tmp_path / "korc")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "push_particles.py"), "--particles", "3001", "--steps", "50",
                          "--every", "25", "--label-bins", "4", "--pitch-bins", "4", "--gamma-bins", "4", "--loss-limit", "0.06",
                          "--loss-bins", "8,6,4", "--loss-box", "1.2,2.2,-0.6,0.6", "--flux-tables",
                          os.path.join(GOLDEN, "efit_tables.npz"), "--output", prefix], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "first exits through s = 0.06, on 8x6x4 cells of R, z and gamma:" in out.stdout, out.stdout
    assert out.stdout.count("confined fraction") == 2 and "2 snapshots on 4x4x4 cells" in out.stdout
    f = H5File(prefix + "_loss_bins.nc")
    bins, steps, newly, confined = (f.read(name) for name in ("bins", "steps", "newly_lost", "confined"))
    same_bits(f.read("rbins"), np.linspace(1.2, 2.2, 9))
    same_bits(f.read("zbins"), np.linspace(-0.6, 0.6, 7))
    same_bits(f.read("gbins"), np.linspace(1.0, 3.0, 5))
    f.close()
    assert bins.shape == (8, 6, 4) and list(steps) == [25.0, 50.0]
    assert confined[-1] + newly.sum() == 3001 and newly[0] > 0 and confined[-1] > 0 and bins.sum() <= newly.sum()
    f = H5File(prefix + "_phase_bins.nc")
    snapshots = f.read("bins")
    f.close()
    assert (snapshots.sum(axis=(1, 2, 3)) <= confined).all() and (snapshots.sum(axis=(1, 2, 3)) > 0).all()
