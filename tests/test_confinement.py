"""First-exit tracking (csrc/confinement.hip's rule) on the host: gfhip_confine_check_host against the numpy model of
tests/confinement_model.py byte for byte, fp64 and fp32 columns, both label kinds, over three checks in a row on random
and planted particles; the plain C++ rule under the sanitizers (tests/confinement_host_check.cpp, a program of its own);
loss_bins.nc's layout.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import confinement_model
import flux_model
from test_flux_label import same_bits
from test_phase import map_box, random_particles

CONFINED = confinement_model.CONFINED
DTYPES = {"f64": np.float64, "f32": np.float32}
STEPS = (25, 25, 4000000000)                                                # an equal step is allowed; the last is near the sentinel


@pytest.fixture(scope="module")
def built():
    from graph_framework_amd import build
    build.build_library()


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(os.path.join(GOLDEN, "efit_tables.npz")))


def loss_edges(tables, shape=(5, 6, 4)):
    """Uniform R edges over the map, uneven z edges inside it (the finder's search past its first guess; particles
    beyond them are `outside`) and uneven gamma edges."""
    rlo, rhi, zlo, zhi = map_box(tables)
    return (np.linspace(rlo, rhi, shape[0] + 1), 0.9*zhi*np.linspace(-1.0, 1.0, shape[1] + 1)**3,
            1.0 + 24.0*np.linspace(0.0, 1.0, shape[2] + 1)**2)


def axis_of(tables):
    """(R, z) of the smallest label on a 400 x 400 grid of the map: the magnetic axis to a cell."""
    rlo, rhi, zlo, zhi = map_box(tables)
    r, z = np.meshgrid(np.linspace(rlo, rhi, 400, endpoint=False), np.linspace(zlo, zhi, 400, endpoint=False), indexing="ij")
    at = np.nanargmin(flux_model.label(tables, r.ravel(), np.zeros(r.size), z.ravel()))
    return r.ravel()[at], z.ravel()[at]


def neighbours(tables, dtype, **options):
    """Two particles (x, y, z) of `dtype` whose labels by the model are neighbours in fp64, the first's the larger one:
    found among 20001 positions one unit of `dtype` apart, in z for fp64 and, for fp32, in a small y, where a unit moves R
    by less than one of its own."""
    rmin, dr, zmin, dz = (float(tables[k]) for k in ("rmin", "dr", "zmin", "dz"))
    x0, z0 = dtype(rmin + 30.25*dr), dtype(zmin + 20.5*dz)
    walk = [dtype(3.0e-5) if dtype == np.float32 else z0]
    for _ in range(20000):
        walk.append(np.nextafter(walk[-1], dtype(np.inf)))
    walk = np.array(walk, dtype=dtype)
    x = np.full(walk.size, x0)
    y, z = (walk, np.full(walk.size, z0)) if dtype == np.float32 else (np.full(walk.size, dtype(0.3)), walk)
    label = flux_model.label(tables, *(c.astype(np.float64) for c in (x, y, z)), **options)
    values, first = np.unique(label, return_index=True)
    pair = np.flatnonzero(np.nextafter(values[1:], -np.inf) == values[:-1])
    assert pair.size, "no two labels one unit apart among %d" % values.size
    above, below = first[pair[0] + 1], first[pair[0]]
    assert label[below] == np.nextafter(label[above], -np.inf)
    return [np.array([c[above], c[below]]) for c in (x, y, z)], label[above]


def planted_losses(tables, dtype, **options):
    """(columns, limit, rows): one particle on the axis; one with R < rmin; a NaN, +inf and -inf in x, y and z in turn; one
    whose label equals `limit`, the model's label of it, and one whose label is nextafter below."""
    rmin = float(tables["rmin"])
    (x, y, z), limit = neighbours(tables, dtype, **options)
    r_axis, z_axis = axis_of(tables)
    good = np.array([r_axis, 0.0, z_axis])
    rows = [good.copy(), np.array([0.5*rmin, 0.0, 0.0])]
    for column in range(3):
        for value in (np.nan, np.inf, -np.inf):
            row = good.copy()
            row[column] = value
            rows.append(row)
    rows = np.array(rows).T.astype(dtype)
    position = [np.concatenate([few, pair]) for few, pair in zip(rows, (x, y, z))]
    n = position[0].size
    momenta = [np.full(n, v, dtype=dtype) for v in (0.4, -1.25, 0.75)]
    columns = position + momenta + [np.full(n, 1.8, dtype=dtype)]
    return columns, limit, dict(axis=0, below_rmin=1, no_number=range(2, 11), equal=n - 2, below=n - 1)


def ensembles(tables, n, dtype, **options):
    """Three states of n particles, what a push might hand to three checks in a row, and the limit: independent seeded
    draws all over the map, a quarter of each beyond it, so that particles leave at every check and lost ones come back;
    the planted particles in front, of which the one below rmin is back inside, just under the limit, for checks 2 and 3."""
    planted, limit, rows = planted_losses(tables, dtype, **options)
    states = []
    for seed in (3, 4, 5):
        columns = [c.astype(dtype) for c in random_particles(tables, n, seed)]
        for c, few in zip(columns, planted):
            c[:min(n, few.size)] = few[:n]
        states.append(columns)
    if n > rows["below_rmin"]:
        for columns in states[1:]:
            for c in columns[:3]:
                c[rows["below_rmin"]] = c[rows["below"]]
    return states, limit, rows


def weights_of(n, dtype, seed=21):
    """Seeded weights of both signs over the type's exponent range, with zeros of both signs."""
    rng = np.random.default_rng(seed)
    span = 120 if dtype == np.float32 else 1000
    weight = (rng.uniform(-1.0, 1.0, n)*2.0**rng.integers(-span, span, n).astype(np.float64)).astype(dtype)
    weight[rng.random(n) < 0.05] = 0.0
    weight[rng.random(n) < 0.02] = -0.0
    return weight


class HostTracker:
    """The arrays a caller of check_host owns."""

    def __init__(self, tables, edges, count, dtype, limit, **options):
        self.tables, self.edges, self.limit, self.options = tables, edges, limit, options
        self.lost_step = np.full(count, CONFINED, dtype=np.uint32)
        self.alive = np.ones(count, dtype=dtype)
        self.exit = (np.full(count, np.nan), np.full(count, np.nan))
        self.limbs = np.zeros(tuple(e.size - 1 for e in edges) + (confinement_model.LIMBS,), dtype=np.int64)
        self.counters = np.zeros(3, dtype=np.uint64)
        self.newly_lost = []

    def check(self, columns, step, weight=None):
        from graph_framework_amd.confinement import check_host
        self.newly_lost.append(check_host(self.tables, columns, step, self.lost_step, self.alive, self.limit, weight, self.exit,
                                          self.edges, self.limbs, self.counters, **self.options))


def equals_model(tracker, model):
    assert tracker.lost_step.tobytes() == model.lost_step.tobytes()
    assert tracker.alive.astype(np.float64).tobytes() == model.alive.tobytes()
    same_bits(tracker.exit[0], model.exit_r)
    same_bits(tracker.exit[1], model.exit_z)
    assert list(tracker.newly_lost) == model.newly_lost
    assert tracker.limbs.tobytes() == model.state().tobytes()
    assert dict(zip(("samples", "outside", "skipped"), (int(v) for v in tracker.counters))) == model.counts


@pytest.mark.parametrize("sqrt_label", [False, True], ids=["s", "sqrt_s"])
@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_host_equals_the_model_over_three_checks(built, tables, kind, sqrt_label):
    dtype = DTYPES[kind]
    n = 4099
    options = dict(sqrt_label=sqrt_label)
    states, limit, rows = ensembles(tables, n, dtype, **options)
    edges = loss_edges(tables)
    off_map = np.isnan(flux_model.label(tables, *(c.astype(np.float64) for c in states[0][:3])))
    assert 800 < off_map.sum() < 1300
    weight = weights_of(n, dtype)
    for weighted in (False, True):
        tracker = HostTracker(tables, edges, n, dtype, limit, **options)
        model = confinement_model.Confinement(tables, *edges, n, limit, **options)
        if weighted:                                                        # a NaN and +-inf among the first check's lost in a cell
            in_cell = np.flatnonzero((plain.deposits == 1) & (plain.lost_step == STEPS[0]) & np.isfinite(plain.exit_r))
            in_cell = [i for i in in_cell if all(flux_model.cells_of(e, np.array([v]))[0] >= 0 for e, v in
                                                 zip(edges, (plain.exit_r[i], plain.exit_z[i], np.float64(states[0][6][i]))))]
            weight[in_cell[0]], weight[in_cell[1]], weight[in_cell[2]] = np.nan, np.inf, -np.inf
        for columns, step in zip(states, STEPS):
            tracker.check(columns, step, weight if weighted else None)
            model.check(*columns, step, weight if weighted else None)
            equals_model(tracker, model)
        plain = model
        assert all(k > 0 for k in model.newly_lost) and model.confined()[-1] > 0
        assert model.counts["outside"] > 0 and model.counts["skipped"] == (3 if weighted else 0)
        assert model.deposits.max() == 1                                    # nobody is settled twice
        came_back = (model.lost_step == STEPS[0]) & (model.labels(*states[1][:3]) < limit)
        assert came_back.sum() > 50 and (tracker.alive[came_back] == 0).all()
        lost = model.lost_step
        on_axis = model.labels(*(c[rows["axis"]:rows["axis"] + 1] for c in states[0][:3]))[0]
        assert np.isnan(on_axis) if sqrt_label else abs(on_axis) < 1.0e-3     # s is a little below 0 there: sqrt(s) is no number
        assert lost[rows["axis"]] == (STEPS[0] if sqrt_label else CONFINED) and tracker.alive[rows["axis"]] == (not sqrt_label)
        assert np.isnan(tracker.exit[0][rows["axis"]]) == (not sqrt_label)
        assert lost[rows["below_rmin"]] == STEPS[0] and tracker.alive[rows["below_rmin"]] == 0     # back inside at checks 2 and 3
        assert model.labels(*(c[rows["below_rmin"]:rows["below_rmin"] + 1] for c in states[2][:3]))[0] < limit
        assert (lost[list(rows["no_number"])] == STEPS[0]).all()
        assert lost[rows["equal"]] == STEPS[0] and lost[rows["below"]] == CONFINED
        equal, below = (model.labels(*(c[rows[k]:rows[k] + 1] for c in states[0][:3]))[0] for k in ("equal", "below"))
        assert equal == limit and below == np.nextafter(limit, -np.inf)
        assert tracker.exit[0][rows["equal"]] == confinement_model.radius(states[0][0], states[0][1])[rows["equal"]]


def test_host_without_exit_arrays_and_without_cells(built, tables):
    from graph_framework_amd.confinement import check_host
    n = 1025
    states, limit, _ = ensembles(tables, n, np.float64)
    edges = loss_edges(tables)
    model = confinement_model.Confinement(tables, *edges, n, limit)
    lost_step, alive = np.full(n, CONFINED, dtype=np.uint32), np.ones(n)
    for columns, step in zip(states, STEPS):
        model.check(*columns, step)
        assert check_host(tables, columns, step, lost_step, alive, limit) == model.newly_lost[-1]
        assert lost_step.tobytes() == model.lost_step.tobytes() and alive.tobytes() == model.alive.tobytes()


def test_host_refusals_leave_the_arrays_alone(built, tables):
    from graph_framework_amd import GfHipError
    from graph_framework_amd.confinement import check_host
    n = 65
    states, limit, _ = ensembles(tables, n, np.float64)
    edges = loss_edges(tables)
    tracker = HostTracker(tables, edges, n, np.float64, limit)

    def refused(match, error=GfHipError, **changed):
        arguments = dict(tables=tables, columns=states[0], step=3, lost_step=tracker.lost_step, alive=tracker.alive, limit=limit,
                         exit=tracker.exit, edges=edges, limbs=tracker.limbs, counters=tracker.counters)
        arguments.update(changed)
        with pytest.raises(error, match=match):
            check_host(**arguments)

    refused("NaN", limit=np.nan)
    refused("0xFFFFFFFF", step=CONFINED)
    refused("strictly increasing", edges=(edges[0], edges[1][::-1], edges[2]))
    refused("at least two edges", edges=(edges[0][:1], edges[1], edges[2]), limbs=np.zeros((0, 6, 4, 67), dtype=np.int64))
    refused("7 are needed", ValueError, columns=states[0][:6])
    refused("differ in length", ValueError, columns=[c[:-1] for c in states[0]])
    refused("in place", ValueError, lost_step=tracker.lost_step.astype(np.int64))
    refused("float32 or float64", ValueError, alive=np.ones(n, dtype=np.int32))
    refused("in place", ValueError, exit=(tracker.exit[0].astype(np.float32), tracker.exit[1]))
    refused("limbs of shape", ValueError, limbs=tracker.limbs[:-1].copy())
    assert (tracker.lost_step == CONFINED).all() and (tracker.alive == 1).all() and np.isnan(tracker.exit[0]).all()
    assert not tracker.limbs.any() and not tracker.counters.any()


def test_the_plain_cpp_rule_under_the_sanitizers(tmp_path):
    """tests/confinement_host_check.cpp: the host rule over planted inputs and every edge's neighbours against a plain
    restatement, built with -fsanitize=address,undefined and run as a child process."""
    binary = str(tmp_path/"confinement_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "graph_framework_amd", "csrc"), "-o", binary,
                           os.path.join(ROOT, "tests", "confinement_host_check.cpp")])
    out = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0
    last = out.stdout.split()
    assert last[-4] == "cases" and int(last[-3]) > 1000 and last[-2:] == ["failures", "0"]


def test_loss_bins_file_has_its_layout(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    from graph_framework_amd.output import write_loss_bins
    bins = np.arange(2*3*4, dtype=np.float64).reshape(2, 3, 4)
    bins[1, 2, 3] = 5e-324
    edges = (np.array([1.0, 1.25, 2.5]), np.array([-1.0, -0.5, 0.125, 1.0]), np.array([1.0, 1.5, 2.0, 2.5, 3.0]))
    path = str(tmp_path/"loss_bins.nc")
    write_loss_bins(path, bins, *edges, 0.95, 0.125, 0.53, "sqrt_s", steps=[25, 50], newly_lost=[7, 2], confined=[2994, 2992],
                    samples=9, outside=1, skipped=0)
    f = H5File(path)
    for name, want in (("bins", bins), ("rbins", edges[0]), ("zbins", edges[1]), ("gbins", edges[2]), ("steps", np.array([25.0, 50.0])),
                       ("newly_lost", np.array([7.0, 2.0])), ("confined", np.array([2994.0, 2992.0]))):
        got = f.read(name)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
    assert [f.read(name).shape for name in ("nr", "nrp", "nz", "nzp", "ng", "ngp", "check")] == [(2,), (3,), (3,), (4,), (4,), (5,), (2,)]
    f.close()
    write_loss_bins(path, bins, *edges, 1.0, 0.0, 1.0)                      # no check yet
    f = H5File(path)
    assert f.read("steps").tobytes() == np.zeros(1).tobytes() and f.read("confined").shape == (1,)
    f.close()
    with pytest.raises(ValueError):
        write_loss_bins(path + "x", bins.reshape(-1), *edges, 1.0, 0.0, 1.0)
    with pytest.raises(ValueError):
        write_loss_bins(path + "x", bins[:, :2], *edges, 1.0, 0.0, 1.0)
    with pytest.raises(ValueError):
        write_loss_bins(path + "x", bins, edges[0], edges[1], edges[2][:-1], 1.0, 0.0, 1.0)
    with pytest.raises(ValueError):
        write_loss_bins(path + "x", bins, *edges, 1.0, 0.0, 1.0, steps=[25, 50], newly_lost=[7])
    assert not os.path.exists(path + "x")
