"""The particle source on the device (csrc/particle_source.hip through gfhip_source_*): the seven columns, the placed column
and the four counters against the numpy model of tests/source_model.py and against gfhip_source_fill_host byte for byte,
on both routes, fp32 and fp64, with one workgroup walking all tiles; whole waves unplaced and a wave's last particles
settling while other lanes have nothing left to take; shards; Korc.load against a push built from the host-filled columns;
the diagnostics after a load with unplaced particles; misuse; the example.  There is no tolerance anywhere."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import flux_model
import moments_model
import source_model
from test_particle_source import DTYPES, EASY, HARD_RANGE, PROFILE, SPEED, cases, hard, same_fill

pytestmark = pytest.mark.gpu

NAMES = ("x", "y", "z", "ux", "uy", "uz", "gamma")
ROUTES = {"plain": dict(plain=True), "refill": dict(refill=True)}


@pytest.fixture(scope="module")
def context():
    from graph_framework_amd import Context
    context = Context(0)
    yield context
    context.close()


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(os.path.join(GOLDEN, "efit_tables.npz")))


def device_fill(context, tables, tag, dtype, case, with_placed=True, **options):
    """(columns, placed, counters) of one source's fill into fresh buffers `<tag>_<name>`."""
    from graph_framework_amd.source import ParticleSource
    case = dict(case)
    count, first = case.pop("count"), case.pop("first_particle", 0)
    source = ParticleSource(context, tables, dtype=dtype, **case, **options)
    keys = ["%s_%s" % (tag, name) for name in NAMES]
    source.fill(*keys, count, first, placed=tag + "_placed" if with_placed else None)
    counters = source.counts()
    columns = [context.copy_to_host(key, np.empty(count, dtype=dtype)) for key in keys]
    placed = context.copy_to_host(tag + "_placed", np.empty(count, dtype=dtype)) if with_placed else None
    source.close()
    return columns, placed, counters


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_device_equals_the_model_and_the_host(context, tables, kind, route):
    """The 24 cases of the host test with max_workgroups = 1: four waves walk and refill across all the tiles."""
    from graph_framework_amd.source import fill_host
    dtype = DTYPES[kind]
    for number, case in enumerate(cases(tables)):
        with_placed = number % 5 != 0
        got = device_fill(context, tables, "case_%s_%s_%d" % (kind, route, number), dtype, case, with_placed, max_workgroups=1,
                          **ROUTES[route])
        columns, placed, counters = source_model.fill(tables, dtype=dtype, **case)
        same_fill(got, (columns, placed if with_placed else None, counters))
        same_fill(got, fill_host(tables, dtype=dtype, placed=with_placed, **case))


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_whole_waves_unplaced_last_particles_and_the_default_launch(context, tables, kind, route):
    """One attempt in a thin shell: whole waves stay unplaced.  64 attempts in the hard region with 65 and 257 particles in
    one workgroup: the last particles of a wave's tiles settle while its other lanes have nothing left to take.  5000
    particles with the launch rule's own number of workgroups."""
    dtype = DTYPES[kind]
    thin = dict(hard(tables), speed_range=SPEED, count=257, attempts=1, seed=3)
    got = device_fill(context, tables, "thin_%s_%s" % (kind, route), dtype, thin, max_workgroups=1, **ROUTES[route])
    model = source_model.fill(tables, dtype=dtype, **thin)
    assert (model[1].reshape(-1)[:256].reshape(4, 64).sum(axis=1) == 0).any() and model[2]["placed"] >= 1
    same_fill(got, model)
    for count in (65, 257):
        last = dict(hard(tables), speed_range=SPEED, count=count, attempts=64, seed=count, first_particle=2**32 - 40)
        got = device_fill(context, tables, "last_%s_%s_%d" % (kind, route, count), dtype, last, max_workgroups=1, **ROUTES[route])
        model = source_model.fill(tables, dtype=dtype, **last)
        assert model[2]["position_tries"] > 20*count and 0 < model[2]["unplaced"] < count
        same_fill(got, model)
    wide = dict(EASY, speed_range=SPEED, count=5000, profile=PROFILE, seed=8)
    same_fill(device_fill(context, tables, "wide_%s_%s" % (kind, route), dtype, wide, **ROUTES[route]),
              source_model.fill(tables, dtype=dtype, **wide))


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_shards_and_routes_are_one_fill(context, tables, kind):
    """[0, k) by one route and [k, n) by the other, each by a source of its own, against one fill of [0, n); the library's
    own choice of route gives the same bytes, and a second fill adds to the counters."""
    from graph_framework_amd.source import ParticleSource
    dtype = DTYPES[kind]
    n, first = 1000, 2**32 - 300
    arguments = dict(hard(tables), speed_range=SPEED, seed=77, attempts=16, profile=PROFILE)
    whole = source_model.fill(tables, dtype=dtype, count=n, first_particle=first, **arguments)
    for k in (1, 300, 999):
        low = device_fill(context, tables, "low_%s_%d" % (kind, k), dtype, dict(arguments, count=k, first_particle=first),
                          max_workgroups=1, plain=True)
        high = device_fill(context, tables, "high_%s_%d" % (kind, k), dtype, dict(arguments, count=n - k, first_particle=first + k),
                           max_workgroups=2, refill=True)
        joined = ([np.concatenate(pair) for pair in zip(low[0], high[0])], np.concatenate([low[1], high[1]]),
                  {name: low[2][name] + high[2][name] for name in low[2]})
        same_fill(joined, whole)
    source = ParticleSource(context, tables, dtype=dtype, **arguments)
    assert source.info()["workgroup_size"] == 256 and source.info()["lds_bytes"] == (2*PROFILE[1].size + 1)*8
    keys = ["own_%s_%s" % (kind, name) for name in NAMES]
    source.fill(*keys, n, first, placed="own_%s_placed" % kind)
    source.fill(*keys, n, first, placed="own_%s_placed" % kind)
    assert source.counts() == {name: 2*value for name, value in whole[2].items()}
    got = [context.copy_to_host(key, np.empty(n, dtype=dtype)) for key in keys]
    same_fill((got, context.copy_to_host("own_%s_placed" % kind, np.empty(n, dtype=dtype)), whole[2]), whole)
    source.close()


@pytest.mark.parametrize("device_state", (False, True))
@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_load_then_five_steps_equal_a_push_of_the_host_filled_columns(tables, kind, device_state):
    """Korc.load, pre_run and 5 steps against a Korc built from gfhip_source_fill_host's columns, bit for bit, unplaced
    particles included; load() outside its place raises; a tracker and a moment profile see the unplaced as lost and
    outside, and `placed` as the weight leaves the sums of the placed."""
    from graph_framework_amd import korc
    from graph_framework_amd.confinement import Confinement
    from graph_framework_amd.moments import FluxMoments
    from graph_framework_amd.source import ParticleSource, fill_host
    dtype = DTYPES[kind]
    n, first = 3001, 2**32 - 1000
    arguments = dict(EASY, speed_range=SPEED, seed=11, attempts=2)
    columns, placed, counters = fill_host(tables, dtype=dtype, count=n, first_particle=first, **arguments)
    assert counters["placed"] > 1000 and counters["unplaced"] > 300

    push = korc.Korc(korc.blank(n), kind, device_state=device_state, first_particle=first)
    context = push.work.context
    source = ParticleSource(context, tables, dtype=dtype, **arguments)
    with pytest.raises(RuntimeError, match="after compile"):
        push.load(source)
    push.compile()
    with pytest.raises(ValueError, match="columns"):
        push.load(ParticleSource(context, tables, dtype=np.float32 if kind == "f64" else np.float64, **arguments))
    push.load(source, placed="placed")
    assert source.counts() == counters
    if device_state:
        push.wait()
        import torch
        torch.cuda.synchronize()
        for name, column in zip(NAMES, columns):
            assert push.device[name].cpu().numpy().tobytes() == column.tobytes(), name
    push.pre_run()
    with pytest.raises(RuntimeError, match="before pre_run"):
        push.load(source)

    medges = np.linspace(0.0, 0.4, 5)
    at_start = {k: v.copy() for k, v in push.sync_host().items()}
    start = [at_start[k] for k in korc.PARTICLE]
    tracker = Confinement(context, tables, np.linspace(1.0, 2.4, 5), np.linspace(-1.2, 1.2, 5), np.linspace(1.0, 3.0, 3), n, kind,
                          limit=1.0, capacity=1)
    push.track(tracker)
    assert tracker.counts() == dict(samples=counters["unplaced"], outside=counters["unplaced"], skipped=0)
    assert (tracker.lost_steps() == 0xFFFFFFFF).tobytes() == (placed == 1).tobytes()
    unweighted, weighted = FluxMoments(context, tables, medges), FluxMoments(context, tables, medges)
    push.bin(unweighted)
    push.bin(weighted, weight="placed")
    kept = placed == 1
    only = moments_model.Moments(tables, medges).add(*[c[kept] for c in start])
    assert weighted.state().tobytes() == unweighted.state().tobytes() == only.state().tobytes()
    assert unweighted.counts()["outside"] == counters["unplaced"] + only.counts["outside"] == weighted.counts()["outside"]
    assert unweighted.counts()["skipped"] == 0 and weighted.read()[:, 0].sum() == counters["placed"] - only.counts["outside"]

    push.run(5)
    loaded = {k: v.copy() for k, v in push.sync_host().items()}
    context.close()

    reference = korc.Korc(dict(zip(korc.PARTICLE, columns)), kind, first_particle=first)
    reference.compile()
    reference.pre_run()
    begun = {k: v.copy() for k, v in reference.sync_host().items()}
    reference.run(5)
    stepped = reference.sync_host()
    for name in korc.PARTICLE:
        assert at_start[name].tobytes() == begun[name].tobytes(), name
        assert loaded[name].tobytes() == stepped[name].tobytes(), name
    assert np.isfinite(loaded["gamma"][kept]).all() and (loaded["gamma"][kept] > 1.0).all() and np.isnan(loaded["x"][~kept]).all()
    reference.work.context.close()


def test_misuse_is_refused_with_the_buffers_untouched(context, tables):
    from graph_framework_amd import GfHipError, _lib, key_of
    from graph_framework_amd.source import ParticleSource
    from test_gpu_phase import upload
    n = 100
    arguments = dict(EASY, speed_range=SPEED)
    for changed, match in ((dict(box=(2.3, 1.2, -1, 1)), "box"), (dict(label_range=(0.4, 0.0)), "label range"),
                           (dict(speed_range=(0.3, 1.0)), "speed range"), (dict(pitch_range=(-1.5, 0.5)), "pitch range"),
                           (dict(attempts=0), "attempts"), (dict(attempts=4097), "attempts"), (dict(plain=True, refill=True), "one route"),
                           (dict(profile=(PROFILE[0], np.array([1.0, 2.0, 0.25, 0.0, 0.75]))), r"\[0, 1\]"),
                           (dict(profile=(np.linspace(0.0, 0.4, 258), np.full(257, 0.5))), "256"), (dict(span=0.0), "non-zero")):
        with pytest.raises(GfHipError, match=match):
            ParticleSource(context, tables, **dict(arguments, **changed))
    source = ParticleSource(context, tables, dtype=np.float32, **arguments)
    planted = [np.full(n, 7.0)]*7
    keys = upload(context, "misuse", planted, dtype=np.float32)
    wrong = upload(context, "misuse64", planted[:1])

    def refused(match, count=n, first=0, placed=None, **replaced):
        with pytest.raises(GfHipError, match=match):
            source.fill(*[replaced.get(name, key) for name, key in zip(NAMES, keys)], count, first, placed=placed)

    refused("at least one particle", count=0)
    refused("shorter", count=n + 1)
    refused("overflows", first=2**64 - 50)
    refused("type", ux=wrong[0])
    refused("type", placed=wrong[0])
    refused("twice", uy=keys[0])
    refused("twice", placed=keys[6])
    refused("shorter", count=n + 1, gamma="misuse_absent")                  # nothing is allocated before everything is looked at
    with pytest.raises(GfHipError, match="unknown buffer"):
        context.buffer_info("misuse_absent")
    for key in keys:
        assert (context.copy_to_host(key, np.empty(n, dtype=np.float32)) == 7.0).all()
    assert source.counts() == dict(placed=0, unplaced=0, position_tries=0, gyro_tries=0)
    source.fill(*keys[:6], "misuse_absent", n, placed="misuse_absent_placed")   # absent buffers are allocated
    assert context.buffer_info("misuse_absent") == (n, np.float32) and source.counts()["placed"] == n
    source.close()


def test_the_example_loads_its_ensemble(tmp_path):
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "push_particles.py"), "--particles", "3001", "--steps", "50",
                          "--every", "25", "--label-bins", "4", "--pitch-bins", "4", "--gamma-bins", "4", "--load-label-range", "0,0.06",
                          "--load-attempts", "16", "--load-speed", "0.3,0.8", "--flux-tables", os.path.join(GOLDEN, "efit_tables.npz")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    line = [text for text in out.stdout.splitlines() if text.startswith("loaded between s = 0 and 0.06:")]
    assert len(line) == 1, out.stdout
    words = line[0].replace(",", "").split()
    placed, unplaced = int(words[words.index("placed") - 1]), int(words[words.index("unplaced") - 1])
    assert placed + unplaced == 3001 and placed > 500 and unplaced > 500
    first = [text for text in out.stdout.splitlines() if text.startswith("  step     25:")][0].replace(",", "").split()
    assert int(first[2]) <= placed and "2 snapshots on 4x4x4 cells" in out.stdout
