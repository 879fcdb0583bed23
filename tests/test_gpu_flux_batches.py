"""Batches of rays on the device (flux_deposit_rays_kernel and spectrum_deposit_rays_kernel through gfhip_flux_* and
gfhip_spectrum_*): slab g of a batched profile or spectrum against a plain one that was fed batch g's samples alone,
selected in numpy by tests/flux_batch_model.py; total() against a plain one fed everything; any split of the rays
over calls, records, shards and routes.  Byte for byte on the states and exact on the counters: there is no tolerance
anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, STATE

import flux_batch_model as model
import flux_model
import spectrum_model
import test_gpu_flux_profile as plain_flux
import test_gpu_spectrum as plain_spectrum
from test_flux_label import all_points, same_bits
from test_spectrum import golden_samples, planted_samples

pytestmark = pytest.mark.gpu

FAR = 2**40 + 5
BATCHES = (1, 2, 3, 16, 64)
CELLS = (1, 3, 256, 257)
LONGEST = 2*256*1024 + 1                                                     # beyond any max_workgroups x workgroup_size here


@pytest.fixture
def context():
    """A context per test: its buffers go with it."""
    from graph_framework_amd import Context
    context = Context(0)
    yield context
    context.close()


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(os.path.join(GOLDEN, "efit_tables.npz")))


@pytest.fixture(scope="module")
def pool(tables):
    points = all_points(tables, np.load(os.path.join(GOLDEN, "flux_golden.npz")))
    labels = flux_model.label(tables, *points)
    labels.setflags(write=False)
    return points, labels


@pytest.fixture(scope="module")
def wave_pool(tables):
    golden = np.load(os.path.join(GOLDEN, "flux_golden.npz"))
    columns = tuple(np.concatenate(pair) for pair in zip(golden_samples(golden), planted_samples(tables)))
    label, npar = spectrum_model.label_npar(tables, *columns)
    return columns, label, npar


@pytest.fixture(scope="module")
def long_samples(pool):
    """The samples of test_gpu_flux_profile.py (every exponent, NaN, inf, waves of one point, cancelling pairs), enough
    for the longest add; computed once and left as they are."""
    columns = plain_flux.samples(pool, LONGEST, 4242)
    for column in columns:
        column.setflags(write=False)
    return columns


def edges_of(cells):
    return 0.15 + 0.7*np.linspace(0.0, 1.0, cells + 1)**1.5                     # not uniform; part of the pool is outside


def same(a, b):
    """Two objects hold the same bytes and the same counters."""
    return a.state().tobytes() == b.state().tobytes() and a.counts() == b.counts()


def check_against_plain(context, batched, plain_of, add_plain, columns, first_ray, tag):
    """`batched` (any number of them, all fed `columns` as the rays first_ray ..) slab by slab against plain objects fed
    the samples of one batch each, and total() against a plain one fed all.  plain_of(): an empty plain object;
    add_plain(object, tag, columns): upload and add."""
    count = len(columns[0])
    batches = batched[0].batches
    index = model.batch_index(first_ray, count, batches)
    assert (batched[0].batch_rays(first_ray, count) == np.bincount(index, minlength=batches)).all()
    states = [each.state() for each in batched]
    counts = dict(samples=0, outside=0, skipped=0)
    for g in range(batches):
        chosen = index == g
        alone = plain_of()
        if chosen.any():
            add_plain(alone, "%s_b%d" % (tag, g), [c[chosen] for c in columns])
        want = alone.state()
        for name, value in alone.counts().items():
            counts[name] += value
        alone.close()
        for state in states:
            assert state.shape == (batches,) + want.shape
            assert state[g].tobytes() == want.tobytes(), (tag, g)
    whole = plain_of()
    add_plain(whole, tag + "_all", columns)
    assert whole.counts() == counts and counts["samples"] == count
    for each in batched:
        assert each.counts() == counts, tag
        total = each.total()
        assert total.batches is None and same(total, whole), tag
        same_bits(total.read(3.0), whole.read(3.0))
        total.close()
    whole.close()


def flux_counts(batches, info):
    return (1, 63, 64, 65, 64*batches - 1, 64*batches + 1, 4099, info["max_workgroups"]*info["workgroup_size"] + 1)


@pytest.mark.parametrize("batches", BATCHES)
@pytest.mark.parametrize("cells", CELLS)
def test_slabs_and_total_against_plain_profiles(context, tables, long_samples, cells, batches):
    """Every count on both routes where the private one exists (up to 256 cells per batch, whatever the batches); the
    last add is one sample longer than a full grid of workgroups.  count = 1 with 64 batches leaves 63 batches without
    a sample and one workgroup to walk all of them."""
    from graph_framework_amd.flux import FluxProfile
    edges = edges_of(cells)

    def add_plain(profile, tag, columns):
        profile.add(*plain_flux.upload(context, tag, columns), len(columns[0]))

    probe = FluxProfile(context, tables, edges, batches=batches)
    info = probe.info()
    probe.close()
    assert info["private_sums"] == (cells <= 256) and info["cap_cells"] == 256
    for count in flux_counts(batches, info):
        assert count <= LONGEST
        columns = [c[:count] for c in long_samples]
        keys = plain_flux.upload(context, "n%d" % count, columns)
        batched = [FluxProfile(context, tables, edges, batches=batches, private=private)
                   for private in ((True, False) if cells <= 256 else (True,))]
        assert [each.info()["private_sums"] for each in batched] == [cells <= 256, False][:len(batched)]
        for each in batched:
            each.add_rays(*keys, count, 0)
        check_against_plain(context, batched, lambda: FluxProfile(context, tables, edges), add_plain, columns, 0,
                            "c%d_g%d_n%d" % (cells, batches, count))
        if batches == 1:                                                    # one batch is the plain profile
            plain = FluxProfile(context, tables, edges)
            plain.add(*keys, count)
            for each in batched:
                assert each.state()[0].tobytes() == plain.state().tobytes() and each.counts() == plain.counts()
            plain.close()
        for each in batched:
            each.close()


def test_the_private_path_serves_256_cells_in_64_batches(context, tables):
    from graph_framework_amd.flux import FluxProfile
    profile = FluxProfile(context, tables, edges_of(256), batches=64)
    plain = FluxProfile(context, tables, edges_of(256))
    info = profile.info()
    assert info["private_sums"] and info == plain.info()                     # the launch is that of ONE batch's cells
    assert info["lds_bytes"] == 256*67*8 + 257*8
    assert profile.state().shape == (64, 256, 67) and profile.read().shape == (64, 256)
    assert profile.like(context).batches == 64
    profile.close()
    plain.close()


@pytest.mark.parametrize("private", [True, False], ids=["private", "global"])
def test_any_split_of_the_rays_gives_the_same_bytes(context, tables, long_samples, private):
    """One add_rays of [0, N) against two calls split at a (the second with first_ray = a), against seven records in
    shuffled order, against a first ray of 2^40 + 5 (by the model), and two shards on two contexts merged."""
    from graph_framework_amd import Context
    from graph_framework_amd.flux import FluxProfile
    count, batches = 4099, 16
    edges = edges_of(16)
    columns = [c[:count] for c in long_samples]

    def fresh(where=context):
        return FluxProfile(where, tables, edges, batches=batches, private=private)

    def add(profile, tag, low, high, shift=0, where=context):
        profile.add_rays(*plain_flux.upload(where, tag, [c[low:high] for c in columns]), high - low, low + shift)

    whole = fresh()
    add(whole, "whole", 0, count)
    assert whole.state().any() and whole.info()["private_sums"] == private
    for a in (1, 63, 64, 65, 100):
        halves = fresh()
        add(halves, "head%d" % a, 0, a)
        add(halves, "tail%d" % a, a, count)
        assert same(halves, whole), a
        halves.close()
    cuts = [0, 1, 64, 700, 701, 2048, 4000, count]
    records = fresh()
    for p in np.random.default_rng(3).permutation(7):
        add(records, "record%d" % p, cuts[p], cuts[p + 1])
        if p == 3:
            records.state()                                                 # canonical in place, between two adds
    assert same(records, whole)
    records.close()

    far = fresh()                                                           # the same samples as other rays: other batches
    add(far, "far", 0, count, FAR)
    assert not same(far, whole)

    def add_plain(profile, tag, selected):
        profile.add(*plain_flux.upload(context, tag, selected), len(selected[0]))

    check_against_plain(context, [far], lambda: FluxProfile(context, tables, edges), add_plain, columns, FAR, "far")
    far.close()

    other = Context(0)
    shards = [fresh(), fresh(other)]
    add(shards[0], "shard0", 0, 1777)
    add(shards[1], "shard1", 1777, count, where=other)
    merged = fresh()
    for shard in shards:
        merged.merge(shard.state(), **shard.counts())
        shard.close()
    other.close()
    assert same(merged, whole)
    same_bits(merged.read(5.0), whole.read(5.0))
    mean, stderr, used = whole.standard_error(0, count)
    assert used == batches and mean.shape == stderr.shape == (16,)
    total = whole.total()
    same_bits(mean, total.read(count))
    total.close()
    merged.close()
    whole.close()


def spectrum_columns(wave_pool, tables, sedges, count, seed):
    """Samples for a spectrum whose N axis holds every finite N: those inside a label cell with an undefined N get the
    value 0, as in test_gpu_spectrum.py's marginal test."""
    columns = plain_spectrum.samples(wave_pool, count, seed)
    label, npar = spectrum_model.label_npar(tables, *columns[:7])
    columns[7][(flux_model.cells_of(sedges, label) >= 0) & ~np.isfinite(npar)] = 0.0
    finite = npar[np.isfinite(npar)]
    return columns, finite.min() - 1.0, finite.max() + 1.0


@pytest.mark.parametrize("batches", [3, 16])
@pytest.mark.parametrize("shape", [(3, 5), (16, 16)], ids=["3x5", "16x16"])
def test_spectrum_slabs_total_and_splits(context, tables, wave_pool, shape, batches):
    from graph_framework_amd.flux import FluxProfile
    from graph_framework_amd.spectrum import FluxSpectrum
    ns, nn = shape
    count = 4099
    sedges, _, _ = plain_spectrum.edges_on_values(wave_pool, ns, 1)
    columns, low, high = spectrum_columns(wave_pool, tables, sedges, count, 50 + ns)
    nedges = np.linspace(low, high, nn + 1)
    keys = plain_spectrum.upload(context, "whole", columns)

    def add_plain(spectrum, tag, selected):
        spectrum.add(*plain_spectrum.upload(context, tag, selected), len(selected[0]))

    batched = [FluxSpectrum(context, tables, sedges, nedges, private=private, batches=batches) for private in (True, False)]
    assert [each.info()["private_sums"] for each in batched] == [True, False]
    for each in batched:
        each.add_rays(*keys, count, 0)
        assert each.state().shape == (batches, ns, nn, 67) and each.state().any()
    check_against_plain(context, batched, lambda: FluxSpectrum(context, tables, sedges, nedges), add_plain, columns, 0,
                        "s%dx%d_g%d" % (ns, nn, batches))
    for a in (1, 63, 64, 65, 100):
        halves = FluxSpectrum(context, tables, sedges, nedges, batches=batches)
        halves.add_rays(*plain_spectrum.upload(context, "head%d" % a, [c[:a] for c in columns]), a, 0)
        halves.add_rays(*plain_spectrum.upload(context, "tail%d" % a, [c[a:] for c in columns]), count - a, a)
        assert same(halves, batched[0]), a
        halves.close()

    profile = FluxProfile(context, tables, sedges, batches=batches)          # the marginal over N, batch by batch and in all
    profile.add_rays(keys[0], keys[1], keys[2], keys[7], count, 0)
    marginal = batched[0].profile()
    assert marginal.batches == batches and marginal.state().tobytes() == profile.state().tobytes()
    totals = [batched[0].total(), profile.total()]
    totals.append(totals[0].profile())
    assert totals[2].state().tobytes() == totals[1].state().tobytes() and totals[1].state().any()
    for each in batched + [profile, marginal] + totals:
        each.close()


def test_misuse_is_refused_and_the_objects_stay_usable(context, tables, long_samples):
    from graph_framework_amd import GfHipError
    from graph_framework_amd.flux import FluxProfile
    from graph_framework_amd.spectrum import FluxSpectrum
    edges = edges_of(3)
    columns = [c[:64] for c in long_samples]
    keys = plain_flux.upload(context, "ok", columns)
    eight = keys[:3] + keys[:3] + [keys[0], keys[3]]
    for batches in (0, 257):
        with pytest.raises(GfHipError, match="1 to 256 batches"):
            FluxProfile(context, tables, edges, batches=batches)
        with pytest.raises(GfHipError, match="1 to 256 batches"):
            FluxSpectrum(context, tables, edges, edges, batches=batches)
    with pytest.raises(GfHipError, match="2\\^20"):                          # 4096 cells x 256 batches is 2^20, the most
        FluxProfile(context, tables, edges_of(4097), batches=256)
    with pytest.raises(GfHipError, match="2\\^20"):
        FluxSpectrum(context, tables, edges_of(256), edges_of(256), batches=17)
    batched = FluxProfile(context, tables, edges, batches=3)
    plain = FluxProfile(context, tables, edges)
    spectrum = FluxSpectrum(context, tables, edges, np.array([-5.0, 0.0, 5.0]), batches=3)
    plain_spectrum_ = FluxSpectrum(context, tables, edges, np.array([-5.0, 0.0, 5.0]))
    with pytest.raises(GfHipError, match="overflows 64 bits"):
        batched.add_rays(*keys, 64, 2**64 - 64)
    with pytest.raises(GfHipError, match="overflows 64 bits"):
        spectrum.add_rays(*eight, 64, 2**64 - 1)
    with pytest.raises(GfHipError, match="gfhip_flux_add_rays"):
        batched.add(*keys, 64)
    with pytest.raises(GfHipError, match="gfhip_spectrum_add_rays"):
        spectrum.add(*eight, 64)
    with pytest.raises(GfHipError, match="does not take them"):
        batched.add_volumes(2)
    with pytest.raises(GfHipError, match="only a batched object"):
        plain.add_rays(*keys, 64, 0)
    with pytest.raises(GfHipError, match="only a batched object"):
        plain_spectrum_.add_rays(*eight, 64, 0)
    other = FluxProfile(context, tables, edges, batches=2)
    wider = FluxProfile(context, tables, edges_of(4), batches=3)
    for state in (other.state(), wider.state()):
        with pytest.raises(GfHipError, match="another shape"):
            batched.merge(state, samples=5)
    with pytest.raises(ValueError):
        batched.merge(plain.state())
    with pytest.raises(ValueError):
        plain.merge(batched.state())
    lib = context.lib
    assert lib.gfhip_flux_merge(batched.handle, plain.state().ctypes.data, 3, 0, 0, 0) == 1
    assert "another shape" in lib.gfhip_last_error(context.handle).decode()
    assert lib.gfhip_flux_merge_batches(plain.handle, batched.state().ctypes.data, 1, 3, 0, 0, 0) == 1
    assert "another shape" in lib.gfhip_last_error(context.handle).decode()
    assert lib.gfhip_spectrum_merge_batches(spectrum.handle, spectrum.state().ctypes.data, 2, 3, 2, 0, 0, 0) == 1
    assert "another shape" in lib.gfhip_last_error(context.handle).decode()
    assert lib.gfhip_flux_merge_batches(batched.handle, None, 3, 3, 0, 0, 0) == 1
    assert "needs a state" in lib.gfhip_last_error(context.handle).decode()
    assert lib.gfhip_flux_add_rays(None, 1, 2, 3, 4, 1, 0) == 1 and lib.gfhip_spectrum_add_rays(None, None, 1, 0) == 1
    assert lib.gfhip_flux_create_batched(None, None, None, 1, 1) is None
    for method, arguments in ((plain.total, ()), (plain.batch_rays, (0, 64)), (plain.standard_error, (0, 64))):
        with pytest.raises(ValueError):
            method(*arguments)
    for each in (batched, spectrum):                                        # nothing was deposited, and everything still works
        assert each.counts() == dict(samples=0, outside=0, skipped=0) and not each.state().any()
    batched.add_rays(*keys, 64, 2**64 - 65)                                  # the last rays there are
    spectrum.add_rays(*eight, 64, 0)
    plain.add(*keys, 64)
    assert batched.counts()["samples"] == spectrum.counts()["samples"] == 64
    total = batched.total()
    assert same(total, plain)
    for each in (batched, plain, spectrum, plain_spectrum_, other, wider, total):
        each.close()


RAYS = 264
SEDGES = np.linspace(0.0, 1.0, 9)
NEDGES = np.linspace(0.0, 0.5, 7)


def test_pipeline_gives_one_state_on_every_route(tmp_path, tables):
    """The golden records tiled to 264 rays as the rays 1000 .. 1263 of an ensemble: bin_power, OnePass and flux_deposition
    / spectrum_deposition with 16 batches give one state, that of add_rays record by record; the files hold stderr,
    batch_bins and batch_rays."""
    from graph_framework_amd import Context, _lib
    from graph_framework_amd.absorption import bin_power, run_absorption
    from graph_framework_amd.backend import key_of
    from graph_framework_amd.flux import FluxProfile, flux_deposition
    from graph_framework_amd.output import RAY_VARIABLES, ResultFile
    from graph_framework_amd.pipeline import OnePass
    from graph_framework_amd.spectrum import FluxSpectrum, spectrum_deposition
    from test_gpu_one_pass import golden_records
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    first, batches = 1000, 16
    records = golden_records()
    saved = records.shape[0]
    context = Context(0)
    profiles = [FluxProfile(context, tables, SEDGES, batches=batches) for _ in range(4)]
    spectra = [FluxSpectrum(context, tables, SEDGES, NEDGES, c=1.0, batches=batches) for _ in range(4)]

    staged_dir = tmp_path/"staged"
    staged_dir.mkdir()
    path = str(staged_dir/"result0.nc")
    trace = ResultFile(path, RAYS)
    for name, _ in RAY_VARIABLES:
        trace.create_variable(name)
    column = {k: i for i, k in enumerate(STATE + ("residual",))}
    for r in range(saved):
        trace.write({name: records[r, column[key]] for name, key in RAY_VARIABLES})
    trace.close()
    run_absorption(path, saved - 1)
    bin_power(path, saved - 1, flux=profiles[0], spectrum=spectra[0], first_ray=first)

    source = Context(0)
    names = STATE + ("residual",)
    for name in names:
        source._check(source.lib.gfhip_allocate_buffer(source.handle, key_of(name), RAYS, _lib.GFIR_F64))
    pipeline = OnePass(source, RAYS, str(tmp_path/"direct0.nc"), flux=profiles[1], spectrum=spectra[1], first_ray=first)
    for r in range(saved):
        for i, name in enumerate(names):
            source.copy_to_device(name, records[r, i])
        pipeline.record()
    pipeline.close()
    source.close()

    bins, counts = flux_deposition(str(staged_dir), 1, tables, 8, 0.0, 1.0, profile=profiles[2], batches=batches, first_ray=first)
    wave_bins, wave_counts = spectrum_deposition(str(staged_dir), 1, tables, 8, 0.0, 1.0, 6, 0.0, 0.5, c=1.0, spectrum=spectra[2],
                                                 batches=batches, first_ray=first)

    result = ResultFile(path)                                               # by hand: every record is the same 264 rays
    for r in range(saved):
        columns = [result.read(name, r) for name in ("x", "y", "z", "kx", "ky", "kz", "w", "d_power")]
        keys = plain_spectrum.upload(context, "hand%d" % r, columns)
        profiles[3].add_rays(keys[0], keys[1], keys[2], keys[7], RAYS, first)
        spectra[3].add_rays(*keys, RAYS, first)
    result.close()
    assert profiles[3].state().any() and spectra[3].state().any()
    assert profiles[3].counts()["samples"] == saved*RAYS
    for each in profiles[:3]:
        assert same(each, profiles[3])
    for each in spectra[:3]:
        assert same(each, spectra[3])
    assert counts == profiles[3].counts() and wave_counts == spectra[3].counts()

    rays = model.batch_rays(first, RAYS, batches)
    for name, cells, got in (("flux_bins.nc", profiles[3], bins), ("spectrum_bins.nc", spectra[3], wave_bins)):
        total = cells.total()
        same_bits(got, total.read(RAYS))
        total.close()
        mean, stderr, used = cells.standard_error(first, RAYS)
        assert used == int((rays > 0).sum()) >= 2
        written = H5File(str(staged_dir/name))
        same_bits(written.read("bins"), got)
        same_bits(written.read("stderr"), stderr)
        same_bits(written.read("batch_rays"), rays.astype(np.float64))
        same_bits(written.read("batch_bins"), cells.batch_means(first, RAYS))
        assert written.read("batch_bins").shape == (batches,) + got.shape
        written.close()
        assert (got != 0.0).any() and np.isfinite(stderr[got != 0.0]).all()    # (tiled rays: some batches hold the same rays)
    for each in profiles + spectra:
        each.close()
    context.close()


def test_example_writes_equal_files_on_both_routes(tmp_path):
    """examples/trace_rays.py --flux-bins 16 --npar-bins 8 --flux-batches 4 with and without --one-pass, a child process
    each: 11 records of 512 rays; bins, stderr, batch_bins and batch_rays of both files are the same bits, and stderr
    is finite wherever bins is not zero."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    got = []
    for flag, prefix in (([], str(tmp_path/"staged")), (["--one-pass"], str(tmp_path/"direct"))):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "trace_rays.py"), "--rays", "512", "--dispersion",
                              "ordinary_wave", "--steps", "4000", "--sub-steps", "400", "--output", prefix,
                              "--absorption-model", "weak_damping", "--flux-bins", "16", "--flux-tables",
                              os.path.join(GOLDEN, "efit_tables.npz"), "--npar-bins", "8", "--npar-range", "-1,1",
                              "--flux-batches", "4"] + flag, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr      # the second process starts only behind a clean first
        assert "flux profile in 4 batches of rays: largest relative standard error" in out.stdout, out.stdout
        assert "spectrum in 4 batches of rays: largest relative standard error" in out.stdout, out.stdout
        files = []
        for name in ("_flux0.nc", "_spectrum0.nc"):
            f = H5File(prefix + name)
            files.append({variable: f.read(variable) for variable in ("bins", "stderr", "batch_bins", "batch_rays")})
            f.close()
        got.append(files)
    for staged, direct in zip(*got):
        for variable in staged:
            same_bits(staged[variable], direct[variable])
        bins, stderr = staged["bins"], staged["stderr"]
        assert bins.shape == stderr.shape and (bins != 0.0).any() and np.isfinite(stderr[bins != 0.0]).all()
        assert staged["batch_bins"].shape == (4,) + bins.shape
        assert (staged["batch_rays"] == 128.0).all()
