"""Spectra over the flux label and N on the device (csrc/flux_spectrum.hip through gfhip_spectrum_*): labels and N against
the numpy model of tests/spectrum_model.py bit for bit; every cell's limbs against rational arithmetic byte for byte, the
three counters exactly; the same bytes whatever route the samples take; the marginal over N against FluxProfile.add; and
the pipeline's three routes.  There is no tolerance anywhere: the arithmetic is fixed and the sums are exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, STATE

import flux_model
import spectrum_model
from test_flux_label import same_bits
from test_spectrum import golden_samples, planted_samples

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 4099)
SHAPES = ((1, 1), (3, 5), (16, 16), (257, 1), (1, 257))
NAMES = ("x", "y", "z", "kx", "ky", "kz", "w", "value")


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
    """The seven columns of the host tests' samples (4096 golden points with seeded waves, then the planted ones) and
    their labels and N by the model, computed once."""
    golden = np.load(os.path.join(GOLDEN, "flux_golden.npz"))
    columns = tuple(np.concatenate(pair) for pair in zip(golden_samples(golden), planted_samples(tables)))
    label, npar = spectrum_model.label_npar(tables, *columns)
    for array in columns + (label, npar):
        array.setflags(write=False)
    return columns, label, npar


def upload(context, tag, columns, names=NAMES, dtype=None):
    from graph_framework_amd import _lib, key_of
    keys = []
    for name, column in zip(names, columns):
        key = "%s_%s" % (tag, name)
        context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), len(column),
                                                         _lib.GFIR_F64 if dtype is None else dtype))
        context.copy_to_device(key, column)
        keys.append(key)
    return keys


def edges_on_values(pool, ns, nn):
    """(sedges, nedges, per axis the pool indices of samples that sit exactly on its first, an inner (if any) and its last
    edge): the edges are labels and N of the pool's own points."""
    _, label, npar = pool
    out, on = [], []
    for values, cells, low, high in ((label, ns, 0.2, 0.8), (npar, nn, -2.0, 2.0)):
        finite = np.unique(values[(values > low) & (values < high)])
        assert finite.size > cells + 1
        edges = finite[np.linspace(0, finite.size - 1, cells + 1).astype(int)]
        assert (np.diff(edges) > 0.0).all()
        out.append(edges)
        on.append([int(np.flatnonzero(values == edge)[0]) for edge in edges[sorted({0, cells//2, cells})]])
    return out[0], out[1], on


def samples(pool, n, seed, planted=()):
    """n samples of the pool's points, the pool indices `planted` among them.  Values over the whole exponent range with
    subnormals, 1e308, both signs, +-0, NaN and +-inf.  Every other block of 64 (a wave) repeats ONE point with values of
    ONE exponent (the wave-uniform pre-sum), the blocks between them mix points and exponents; cancelling pairs share a
    cell."""
    columns, _, _ = pool
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, columns[0].size, n)
    value = rng.uniform(-1.0, 1.0, n)*2.0**rng.integers(-1074, 1001, n).astype(np.float64)
    tiny = rng.random(n) < 0.1
    value[tiny] = rng.integers(-4000, 4000, int(tiny.sum()))*5e-324
    value[rng.random(n) < 0.05] = 1.0e308
    value[rng.random(n) < 0.05] = -1.0e308
    for start in range(0, n, 128):
        stop = min(start + 64, n)
        pick[start:stop] = pick[start]
        value[start:stop] = rng.uniform(1.0, 2.0, stop - start)*rng.choice([-1.0, 1.0], stop - start)*2.0**int(rng.integers(-1000, 1000))
    for k, index in enumerate(planted):
        pick[64 + 5*k:64 + 5*k + 2] = index
        value[64 + 5*k:64 + 5*k + 2] = (1.5 + k, 2.0**-1060)
    half = n//4
    pick[3*half:4*half] = pick[2*half:3*half]
    value[3*half:4*half] = -value[2*half:3*half]
    bad = rng.random(n) < 0.03
    value[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf]), int(bad.sum()))
    zero = rng.random(n) < 0.02
    value[zero] = rng.choice(np.array([0.0, -0.0]), int(zero.sum()))
    return [c[pick] for c in columns] + [value]


def check(spectrum, model, divisor=1.0):
    assert spectrum.counts() == model.counts
    assert spectrum.state().tobytes() == model.state().tobytes()
    same_bits(spectrum.read(divisor), model.bins(divisor))


@pytest.mark.parametrize("sqrt_label", [False, True], ids=["s", "sqrt_s"])
def test_labels_and_npar_equal_the_model_bit_for_bit(context, tables, pool, sqrt_label):
    from graph_framework_amd.spectrum import FluxSpectrum
    columns, label, npar = pool
    n = columns[0].size
    spectrum = FluxSpectrum(context, tables, [0.0, 1.0], [-1.0, 1.0], sqrt_label=sqrt_label)
    keys = upload(context, "npar", list(columns) + [np.full(n, 7.0), np.full(n, 7.0)], NAMES[:7] + ("label", "npar"))
    spectrum.npar(*keys, n)
    got = [np.empty(n), np.empty(n)]
    context.copy_to_host(keys[7], got[0])
    context.copy_to_host(keys[8], got[1])
    want = spectrum_model.label_npar(tables, *columns, sqrt_label=sqrt_label)
    same_bits(got[0], want[0])
    same_bits(got[1], want[1])
    if not sqrt_label:
        same_bits(got[0], label)
        same_bits(got[1], npar)
    assert np.isfinite(want[1]).sum() > 3000 and np.isinf(want[1]).any() and np.isnan(want[1]).any()
    assert spectrum.counts() == dict(samples=0, outside=0, skipped=0)       # labelling deposits nothing
    other = FluxSpectrum(context, tables, [0.0, 1.0], [-1.0, 1.0], psi0=0.25, span=-0.125, c=1.0, private=False)
    other.npar(*keys, n)
    context.copy_to_host(keys[7], got[0])
    context.copy_to_host(keys[8], got[1])
    want = spectrum_model.label_npar(tables, *columns, psi0=0.25, span=-0.125, c=1.0)
    same_bits(got[0], want[0])
    same_bits(got[1], want[1])
    spectrum.close()
    other.close()


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % shape for shape in SHAPES])
def test_deposits_against_the_model(context, tables, pool, shape):
    """Every count on both paths where the private one exists; the last add is one sample longer than a full grid of
    workgroups, so that the grid-stride loop takes a second trip in one workgroup."""
    from graph_framework_amd.spectrum import FluxSpectrum
    ns, nn = shape
    sedges, nedges, on = edges_on_values(pool, ns, nn)
    expect_private = ns*nn <= 256
    base = samples(pool, 4099, 100 + 7*ns + nn, on[0] + on[1])
    label, npar = spectrum_model.label_npar(tables, *base[:7])
    at = 64 + 5*np.arange(len(on[0]) + len(on[1]))
    per_axis = len(on[0])
    assert np.isin(label[at[:per_axis]], sedges).all() and np.isin(npar[at[per_axis:]], nedges).all()
    assert label[at[per_axis - 1]] == sedges[-1] and npar[at[-1]] == nedges[-1]                  # on the last edge: outside
    assert flux_model.cells_of(sedges, label[at[:1]])[0] == 0 and flux_model.cells_of(nedges, npar[at[per_axis:per_axis + 1]])[0] == 0
    routes = (True, False) if expect_private else (True,)
    for count in COUNTS + ("long",):
        if count == "long":
            probe = FluxSpectrum(context, tables, sedges, nedges)
            info = probe.info()
            probe.close()
            count = info["max_workgroups"]*info["workgroup_size"] + 1
        columns = [np.resize(c, count) for c in base]                       # the base tiled
        model = spectrum_model.Spectrum(tables, sedges, nedges).add(*columns)
        if count >= 4099:
            assert model.counts["outside"] and model.counts["skipped"]
            assert ns*nn == 1 or any(total < 0 for total in model.units)
            assert sum(total != 0 for total in model.units) >= min(ns*nn, 7)//2 + 1
            if shape == (3, 5):                                             # a transposed index gives another state
                bins = model.bins()
                assert not np.array_equal(bins.reshape(-1), bins.T.reshape(-1)) and (bins != 0.0).sum() >= 8
        keys = upload(context, "grid%dx%d_%d" % (ns, nn, count), columns)   # a key keeps its first size
        for private in routes:
            spectrum = FluxSpectrum(context, tables, sedges, nedges, private=private)
            info = spectrum.info()
            assert spectrum.shape == shape and info["cap_cells"] == 256
            assert info["private_sums"] == (private and expect_private)
            assert info["workgroup_size"] == (1024 if info["private_sums"] else 256)
            if info["private_sums"]:
                assert info["lds_bytes"] == ns*nn*536 + (ns + nn + 2)*8 <= 160*1024
            else:
                assert info["lds_bytes"] == (ns + nn + 2)*8
            assert count <= 4099 or count > info["max_workgroups"]*info["workgroup_size"] or not private
            spectrum.add(*keys, count)
            check(spectrum, model)
            check(spectrum, model, 3.0)                                     # reading again changes nothing
            spectrum.close()


def test_same_bytes_whatever_the_route(context, tables, pool):
    from graph_framework_amd.spectrum import FluxSpectrum
    sedges, nedges, on = edges_on_values(pool, 3, 5)
    columns = samples(pool, 4099, 7, on[0] + on[1])
    keys = upload(context, "route", columns)
    model = spectrum_model.Spectrum(tables, sedges, nedges).add(*columns)

    def fresh(private=True):
        return FluxSpectrum(context, tables, sedges, nedges, private=private)

    whole = fresh()
    whole.add(*keys, 4099)
    check(whole, model)
    want, counts = whole.state().tobytes(), whole.counts()

    plain = fresh(False)                                                    # without the on-chip sums
    assert whole.info()["private_sums"] and not plain.info()["private_sums"]
    plain.add(*keys, 4099)
    assert plain.state().tobytes() == want and plain.counts() == counts

    order = np.random.default_rng(8).permutation(4099)                      # any order
    shuffled = fresh()
    shuffled.add(*upload(context, "shuffled", [c[order] for c in columns]), 4099)
    assert shuffled.state().tobytes() == want and shuffled.counts() == counts

    pieces = fresh()                                                        # seven adds: records
    cuts = [0, 1, 64, 700, 701, 2048, 4000, 4099]
    for p, (low, high) in enumerate(zip(cuts[:-1], cuts[1:])):
        pieces.add(*upload(context, "piece%d" % p, [c[low:high] for c in columns]), high - low)
        if p == 3:
            pieces.state()                                                  # canonical in place, between two adds
    assert pieces.state().tobytes() == want and pieces.counts() == counts

    merged = fresh()                                                        # two spectra, one of them without private sums
    for h, part in enumerate((order[:1777], order[1777:])):
        shard = fresh(bool(h))
        shard.add(*upload(context, "shard%d" % h, [c[part] for c in columns]), part.size)
        merged.merge(shard.state(), **shard.counts())
        shard.close()
    assert merged.state().tobytes() == want and merged.counts() == counts
    same_bits(merged.read(5.0), whole.read(5.0))
    for each in (whole, plain, shuffled, pieces, merged):
        each.close()


def test_the_marginal_over_npar_is_the_flux_profile(context, tables, pool):
    """N edges that cover every finite N of the samples: the spectrum's profile() is FluxProfile.add's state on the same
    samples byte for byte.  Samples whose N is undefined (w = +-0, planted with a zero value so that they add nothing)
    are `outside` for the spectrum and inside for the profile: the counts differ by exactly those."""
    from graph_framework_amd.flux import FluxProfile
    from graph_framework_amd.spectrum import FluxSpectrum
    sedges, _, _ = edges_on_values(pool, 16, 1)
    columns = samples(pool, 4099, 21)
    label, npar = spectrum_model.label_npar(tables, *columns[:7])
    in_a_cell = flux_model.cells_of(sedges, label) >= 0
    undefined = in_a_cell & ~np.isfinite(npar)
    columns[7][undefined] = 0.0                                             # those from the pool's planted points
    good = np.flatnonzero(in_a_cell & np.isfinite(npar))[:6]
    for c in columns[:6]:
        c[900:906] = c[good]
    columns[6][900:906] = (0.0, -0.0, 0.0, -0.0, 0.0, -0.0)                 # w = +-0: N is +-inf
    columns[7][900:906] = 0.0
    label, npar = spectrum_model.label_npar(tables, *columns[:7])
    undefined = (flux_model.cells_of(sedges, label) >= 0) & ~np.isfinite(npar)
    assert undefined.sum() >= 6 and np.isinf(npar[900:906]).all() and (columns[7][undefined] == 0.0).all()
    finite = npar[np.isfinite(npar)]
    nedges = np.linspace(finite.min() - 1.0, finite.max() + 1.0, 12)

    keys = upload(context, "marginal", columns)
    spectrum = FluxSpectrum(context, tables, sedges, nedges)
    spectrum.add(*keys, 4099)
    check(spectrum, spectrum_model.Spectrum(tables, sedges, nedges).add(*columns))
    profile = FluxProfile(context, tables, sedges)
    profile.add(keys[0], keys[1], keys[2], keys[7], 4099)
    marginal = spectrum.profile()
    assert marginal.state().tobytes() == profile.state().tobytes() and profile.state().any()
    same_bits(marginal.read(2.0), profile.read(2.0))
    ours, theirs = marginal.counts(), profile.counts()
    assert ours == spectrum.counts()
    assert ours["samples"] == theirs["samples"] == 4099 and ours["skipped"] == theirs["skipped"] > 0
    assert ours["outside"] == theirs["outside"] + int(undefined.sum())
    for each in (spectrum, profile, marginal):
        each.close()


def test_misuse_is_refused_before_anything_runs(context, tables, pool):
    import ctypes
    from graph_framework_amd import GfHipError, _lib
    from graph_framework_amd.flux import flux_map
    from graph_framework_amd.spectrum import FluxSpectrum, spectrum_field
    lib = context.lib

    def refused(match, given, field, sedges, nedges, ns=None, nn=None):
        sedges, nedges = (np.ascontiguousarray(e, dtype=np.float64) for e in (sedges, nedges))
        handle = lib.gfhip_spectrum_create(context.handle, ctypes.byref(given) if given is not None else None,
                                           ctypes.byref(field) if field is not None else None,
                                           sedges.ctypes.data if sedges.size else None, sedges.size - 1 if ns is None else ns,
                                           nedges.ctypes.data if nedges.size else None, nedges.size - 1 if nn is None else nn)
        assert not handle
        assert match in lib.gfhip_last_error(context.handle).decode(), lib.gfhip_last_error(context.handle).decode()

    good, keep = flux_map(tables)
    field, keep_field = spectrum_field(tables)
    unit, pair = np.array([0.0, 0.5, 1.0]), np.array([-1.0, 1.0])
    refused("needs a map", None, field, unit, pair)
    refused("needs a map", good, None, unit, pair)
    refused("needs a map", good, field, np.array([]), pair, ns=2)
    refused("needs a map", good, field, unit, np.array([]), nn=1)
    refused("1 to 4096 cells per axis", good, field, unit, pair, ns=0)
    refused("1 to 4096 cells per axis", good, field, unit, pair, nn=0)
    refused("1 to 4096 cells per axis", good, field, np.arange(4098.0), pair)
    refused("1 to 4096 cells per axis", good, field, unit, np.arange(4098.0))
    refused("at most 65536 cells", good, field, np.arange(258.0), np.arange(258.0))
    for edges in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 1.0], [0.0, np.inf]):
        refused("strictly increasing", good, field, np.array(edges), pair)
        refused("strictly increasing", good, field, unit, np.array(edges))
    for name, value, match in (("dpsi", 0.0, "dpsi and c"), ("dpsi", np.inf, "dpsi and c"), ("c", 0.0, "dpsi and c"),
                               ("c", np.nan, "dpsi and c"), ("numpsi", 0, "numpsi"), ("psimin", np.nan, "psimin"),
                               ("reserved", 3, "reserved")):
        broken, keep_broken = spectrum_field(tables)
        setattr(broken, name, value)
        refused(match, good, broken, unit, pair)
    broken, keep_broken = spectrum_field(tables)
    broken.fpol[0] = None
    refused("four fpol tables", good, broken, unit, pair)
    for name, value, match in (("numr", 0, "numr >= 1"), ("numz", (1 << 31) + 1, "2^31 cells"), ("dr", 0.0, "finite and non-zero"),
                               ("span", np.inf, "finite and non-zero"), ("flags", 4, "unknown flag bits"),
                               ("reserved", 1, "reserved"), ("coefficients", None, "coefficient tables")):
        broken_map, keep_map = flux_map(tables)
        setattr(broken_map, name, value)
        refused(match, broken_map, field, unit, pair)

    columns = [np.full(64, 1.9), np.zeros(64), np.zeros(64), np.full(64, 1.0), np.full(64, 2.0), np.full(64, 3.0),
               np.full(64, 5.0e9), np.full(64, 3.0)]
    label, npar = spectrum_model.label_npar(tables, *[c[:1] for c in columns[:7]])
    assert 0.0 < label[0] < 1.0 and -1.0 < npar[0] < 1.0
    ok = upload(context, "ok", columns)
    narrow = upload(context, "narrow", columns, dtype=_lib.GFIR_F32)
    out = upload(context, "out", [np.full(64, 3.0), np.full(64, 3.0)], ("label", "npar"))
    spectrum = FluxSpectrum(context, tables, unit, pair)
    other = FluxSpectrum(context, tables, pair + 1.0, [-1.0, 0.0, 1.0])             # 1 x 2 against 2 x 1
    wider = FluxSpectrum(context, tables, unit, [-1.0, 0.0, 1.0])                   # 2 x 2: the same ns
    shorter = FluxSpectrum(context, tables, pair + 1.0, pair)                       # 1 x 1: the same nn
    for slot in (0, 4, 7):
        mixed = list(ok)
        mixed[slot] = narrow[slot]
        with pytest.raises(GfHipError, match="fp64"):
            spectrum.add(*mixed, 64)
        mixed[slot] = "no such buffer"
        with pytest.raises(GfHipError, match="unknown buffer"):
            spectrum.add(*mixed, 64)
    with pytest.raises(GfHipError, match="shorter"):
        spectrum.add(*ok, 65)
    with pytest.raises(GfHipError, match="fp64"):
        spectrum.npar(*ok[:7], out[0], narrow[7], 64)
    with pytest.raises(GfHipError, match="shorter"):
        spectrum.npar(*ok[:7], *out, 65)
    with pytest.raises(GfHipError, match="unknown buffer"):
        spectrum.npar(*ok[:6], "no such buffer", *out, 64)
    for another in (other, wider, shorter):
        with pytest.raises(GfHipError, match="another shape"):
            spectrum.merge(another.state(), samples=5)
    with pytest.raises(ValueError):
        spectrum.merge(other.state()[0])
    for call, arguments in ((lib.gfhip_spectrum_state, (None,)), (lib.gfhip_spectrum_read, (1.0, None)),
                            (lib.gfhip_spectrum_info, (None,)), (lib.gfhip_spectrum_merge, (None, 2, 1, 1, 0, 0)),
                            (lib.gfhip_spectrum_add, (None, 1)), (lib.gfhip_spectrum_npar, (None, 1, 2, 1))):
        assert call(spectrum.handle, *arguments) == 1
        assert "needs" in lib.gfhip_last_error(context.handle).decode()
    eight = (ctypes.c_uint64*8)(*range(1, 9))
    for call, arguments in ((lib.gfhip_spectrum_add, (eight, 1)), (lib.gfhip_spectrum_npar, (eight, 8, 9, 1)),
                            (lib.gfhip_spectrum_counts, (None, None, None)), (lib.gfhip_spectrum_state, (None,)),
                            (lib.gfhip_spectrum_merge, (None, 1, 1, 0, 0, 0)), (lib.gfhip_spectrum_read, (1.0, None)),
                            (lib.gfhip_spectrum_info, (None,))):
        assert call(None, *arguments) == 1                                  # a null spectrum
    lib.gfhip_spectrum_destroy(None)
    assert spectrum.counts() == dict(samples=0, outside=0, skipped=0)       # nothing was launched
    assert not spectrum.state().any()
    got = np.empty(64)
    for key in out:
        context.copy_to_host(key, got)
        assert (got == 3.0).all()                                           # the refused npar() wrote nothing
    spectrum.add(*ok, 64)                                                   # and the spectrum still works
    check(spectrum, spectrum_model.Spectrum(tables, unit, pair).add(*columns))
    assert spectrum.read().sum() == 192.0
    for each in (spectrum, other, wider, shorter):
        each.close()


RAYS = 264
SEDGES = np.linspace(0.0, 1.0, 9)
NEDGES = np.linspace(0.0, 0.5, 7)


def test_pipeline_gives_one_state_on_every_route(tmp_path, tables):
    """The 21 golden records tiled to 264 rays: bin_power(spectrum=), OnePass(spectrum=) and spectrum_deposition over the
    written file give one state; a flux profile given alongside is what the spectrum's marginal is.  The tracer's files
    hold w in units of c, so c = 1 here."""
    from graph_framework_amd import Context
    from graph_framework_amd.flux import FluxProfile
    from graph_framework_amd.spectrum import FluxSpectrum, spectrum_deposition
    from graph_framework_amd.output import RAY_VARIABLES, ResultFile
    from test_gpu_one_pass import golden_records
    from graph_framework_amd.absorption import bin_power, run_absorption
    from graph_framework_amd.pipeline import OnePass
    from graph_framework_amd import _lib
    from graph_framework_amd.backend import key_of
    records = golden_records()
    saved = records.shape[0]
    context = Context(0)
    staged, direct, from_file = (FluxSpectrum(context, tables, SEDGES, NEDGES, c=1.0) for _ in range(3))
    beside = FluxProfile(context, tables, SEDGES)

    staged_dir = tmp_path / "staged"
    staged_dir.mkdir()
    path = str(staged_dir / "result0.nc")
    trace = ResultFile(path, RAYS)
    for name, _ in RAY_VARIABLES:
        trace.create_variable(name)
    column = {k: i for i, k in enumerate(STATE + ("residual",))}
    for r in range(saved):
        trace.write({name: records[r, column[key]] for name, key in RAY_VARIABLES})
    trace.close()
    run_absorption(path, saved - 1)
    bin_power(path, saved - 1, flux=beside, spectrum=staged)                # next to a profile

    source = Context(0)
    names = STATE + ("residual",)
    for name in names:
        source._check(source.lib.gfhip_allocate_buffer(source.handle, key_of(name), RAYS, _lib.GFIR_F64))
    pipeline = OnePass(source, RAYS, str(tmp_path / "direct0.nc"), spectrum=direct)               # alone
    for r in range(saved):
        for i, name in enumerate(names):
            source.copy_to_device(name, records[r, i])
        pipeline.record()
    pipeline.close()
    source.close()

    bins, counts = spectrum_deposition(str(staged_dir), 1, tables, 8, 0.0, 1.0, 6, 0.0, 0.5, c=1.0, spectrum=from_file)

    result = ResultFile(path)
    columns = [np.stack([result.read(name, r) for r in range(saved)]).reshape(-1)
               for name in ("x", "y", "z", "kx", "ky", "kz", "w", "d_power")]
    result.close()
    model = spectrum_model.Spectrum(tables, SEDGES, NEDGES, c=1.0).add(*columns)
    assert model.counts["samples"] == saved*RAYS and sum(total != 0 for total in model.units) >= 2
    for spectrum in (staged, direct, from_file):
        check(spectrum, model, RAYS)
    assert counts == model.counts
    same_bits(bins, model.bins(RAYS))
    marginal = staged.profile()
    assert model.counts["outside"] == beside.counts()["outside"]            # N of every sample on the label axis is on its own
    assert marginal.state().tobytes() == beside.state().tobytes() and marginal.counts() == beside.counts()

    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    written = H5File(str(staged_dir / "spectrum_bins.nc"))
    same_bits(written.read("bins"), bins)
    same_bits(written.read("sbins"), SEDGES)
    same_bits(written.read("nbins"), NEDGES)
    written.close()
    for each in (staged, direct, from_file, beside, marginal):
        each.close()
    context.close()


def test_example_writes_equal_spectrum_bins_on_both_routes(tmp_path):
    """examples/trace_rays.py --flux-bins 16 --npar-bins 8 with and without --one-pass, a child process each: 11 records
    of 512 rays, as the flux example's test."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    got = []
    for flag, prefix in (([], str(tmp_path / "staged")), (["--one-pass"], str(tmp_path / "direct"))):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "trace_rays.py"), "--rays", "512", "--dispersion",
                              "ordinary_wave", "--steps", "4000", "--sub-steps", "400", "--output", prefix,
                              "--absorption-model", "weak_damping", "--flux-bins", "16", "--flux-tables",
                              os.path.join(GOLDEN, "efit_tables.npz"), "--npar-bins", "8", "--npar-range", "-1,1"] + flag,
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr      # the second process starts only behind a clean first
        assert "spectrum on 16x8 cells of s and N: 5632 samples" in out.stdout, out.stdout
        f = H5File(prefix + "_spectrum0.nc")
        flux = H5File(prefix + "_flux0.nc")
        got.append((f.read("bins"), f.read("sbins"), f.read("nbins"), flux.read("bins")))
        assert f.read("ns").shape == (16,) and f.read("nnp").shape == (9,)
        f.close()
        flux.close()
    same_bits(got[0][0], got[1][0])
    same_bits(got[0][1], np.linspace(0.0, 1.0, 17))
    same_bits(got[0][2], np.linspace(-1.0, 1.0, 9))
    assert got[0][0].shape == (16, 8) and np.isfinite(got[0][0]).all() and got[0][0].sum() > 0.0
    np.testing.assert_allclose(got[0][0].sum(axis=1), got[0][3], rtol=1.0e-12, atol=0.0)          # N in [-1, 1] holds it all
