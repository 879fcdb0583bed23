"""Every route through the converge loop on residuals dictated by data (tests/scripted_item.py), held to the loop
of tests/max_model.py: the iteration count, the last maximum — exactly — and, on every ray, the number of passes
that ran (the item counts them in `c`).  The scripts leave the loop through each of its clauses, on the first, a
middle and the last pass of a launch of 1 to 5 passes."""
import collections
import functools
import os

import numpy as np
import pytest

import scripted_item
from max_model import converge, max_element, scripted

pytestmark = pytest.mark.gpu

NUMPY = scripted_item.NUMPY
REPORT = "Workitem failed to converge"
Case = collections.namedtuple("Case", "name classes columns per_ray tolerance limit iterations last passes")


@pytest.fixture(scope="module", autouse=True)
def kernel_cache(tmp_path_factory):
    """One directory of compiled kernels for the module (the same item at another ensemble size is not built again)."""
    before = os.environ.get("GFHIP_CACHE_DIR")
    os.environ["GFHIP_CACHE_DIR"] = str(tmp_path_factory.mktemp("kernels"))
    yield
    if before is None:
        del os.environ["GFHIP_CACHE_DIR"]
    else:
        os.environ["GFHIP_CACHE_DIR"] = before


@functools.lru_cache(maxsize=None)
def expected(dtype, rays):
    """scripted_item.ensembles with what the model's loop makes of them: computed once."""
    kind = NUMPY[dtype]
    out = []
    for name, classes, tolerance, limit in scripted_item.ensembles(dtype):
        columns, per_ray = scripted_item.columns(dtype, classes, rays)
        maxima = scripted_item.maxima(dtype, classes, per_ray)
        iterations, last, passes = converge(scripted(maxima, kind), kind, tolerance, limit)
        assert passes < scripted_item.K - 1, name        # the script is longer than the loop
        out.append(Case(name, classes, columns, per_ray, tolerance, limit, iterations, last, passes))
    return out


def same(got, want, note):
    """The double the C ABI returns is the model's last maximum (its modulus for a complex item)."""
    if np.iscomplexobj(want):
        with np.errstate(all="ignore"):
            want = np.abs(want)
    if np.isnan(want):
        assert np.isnan(got), (note, got)
    elif want == 0:
        assert got == 0, (note, got)
    else:
        assert type(want)(got).tobytes() == want.tobytes() and float(want) == got, (note, got, want)


def make(dtype, rays, padding=0):
    from graph_framework_amd import Context
    context = Context(0)
    kernel = context.add_kernel(scripted_item.blob(dtype, padding), rays)
    context.compile()
    columns, _ = scripted_item.columns(dtype, [[1.0]], rays)
    kernel.create_kernel_call(["c", "base", "v"], ["residual"], columns)
    return context, kernel


def load(context, columns):
    for key, values in zip(("c", "base", "v"), columns):
        context.copy_to_device(key, values)


def passes_of(context, kind, rays):
    return context.copy_to_host("c", np.empty(rays, dtype=kind))


def exits_cover_the_launch(dtype, rays, batch):
    """The scripts end the loop on the first, the last and (from 3 passes per launch) a middle pass of a launch."""
    seen = {(case.passes - 1) % batch for case in expected(dtype, rays)}
    assert seen == set(range(batch)), seen


@pytest.mark.parametrize("batch", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_device_decided_loop(monkeypatch, capfd, dtype, batch):
    """Kernel.converge: passes queued ahead of the host, `batch` per launch, the test on the device; the launch the
    loop ended in is redone with the loop's passes.  Each case twice in a row on the same kernel."""
    monkeypatch.setenv("GFHIP_CONVERGE_BATCH", str(batch))
    kind = NUMPY[dtype]
    for rays in (300, 4099):
        exits_cover_the_launch(dtype, rays, batch)
        context, kernel = make(dtype, rays)
        assert int(kernel.info().converge_batch) == (batch if batch > 1 else 0)
        assert kernel.info().num_instructions < 1500
        for name, classes, columns, per_ray, tolerance, limit, iterations, last, passes in expected(dtype, rays):
            for again in range(2):
                note = (name, rays, again)
                load(context, columns)
                capfd.readouterr()
                got_iterations, got_last = kernel.converge(tolerance, limit)
                reports = capfd.readouterr().err.count(REPORT)
                print(note, "device", got_iterations, got_last, "model", iterations, last, passes)
                assert got_iterations == iterations, note
                same(got_last, last, note)
                assert reports == (1 if iterations > limit else 0), note
                assert np.array_equal(passes_of(context, kind, rays), np.full(rays, passes, dtype=kind)), note
                final = scripted_item.outputs(dtype, classes, per_ray, passes - 1)
                assert np.array_equal(context.copy_to_host("residual", np.empty(rays, dtype=kind)), final, equal_nan=True), note
        context.close()


def sampled_launches(count, passes, batch, every):
    """(event pairs one Kernel.converge leaves, the kernel's launch count afterwards), from the count before it.
    The loop queues 16, 32, 64, ... single passes (6, 12, 24, ... launches of `batch` passes) per host synchronisation
    until the test has come out false; every queued launch takes a number, the `every`-th ones are bracketed, and of
    those only the pairs of the ceil(passes/batch) launches that ran are kept.  A loop that ended inside a launch
    redoes that launch: one more number, one more pair if it is an `every`-th."""
    ran = -(-passes//batch)
    queued, most = (6, 24) if batch > 1 else (16, 64)
    total = queued
    while total < ran:
        queued = min(2*queued, most)
        total += queued
    kept = sum(1 for launch in range(count, count + ran) if launch % every == 0)
    count += total
    if batch > 1 and passes % batch:
        kept += count % every == 0
        count += 1
    return kept, count


@pytest.mark.parametrize("batch", [1, 3])
def test_device_decided_loop_keeps_the_timing_of_the_launches_that_ran(monkeypatch, batch):
    """Launch timing under Kernel.converge: one sample per launch that ran — not per launch that was queued and
    returned at once — plus the redo launch; around every launch, then around every second one."""
    monkeypatch.setenv("GFHIP_CONVERGE_BATCH", str(batch))
    dtype, rays = "f64", 300
    context, kernel = make(dtype, rays)
    assert int(kernel.info().converge_batch) == (batch if batch > 1 else 0)
    count = 0
    for every in (1, 2):
        context.enable_timing(True, every)
        for case in expected(dtype, rays):
            load(context, case.columns)
            assert kernel.converge(case.tolerance, case.limit)[0] == case.iterations, case.name
            samples = kernel.timing_samples()
            want, count = sampled_launches(count, case.passes, batch, every)
            print(case.name, "every", every, "passes", case.passes, "samples", len(samples), "want", want)
            assert len(samples) == want, (case.name, every)
            if every == 1:
                assert want == -(-case.passes//batch) + (batch > 1 and case.passes % batch != 0), case.name
            assert all(ms >= 0.0 for ms in samples), case.name
#  Nothing is left pending: no event pair of a launch that returned at once stayed behind.
            assert kernel.timing() == (0.0, 0), (case.name, every)
            assert kernel.timing_samples() == [], (case.name, every)
    context.close()


@pytest.mark.parametrize("between", ["streak", "wait"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_host_loop_on_run_max(dtype, between):
    """The reference's own loop on the host, one gfhip_run_max per pass: as an unbroken streak (from the second call
    the library runs passes ahead and answers from their maxima) and with a wait() between the calls (plain `_max`
    launches).  Whatever comes after the loop first takes back the passes nobody asked for."""
    kind = NUMPY[dtype]
    rays = 300
    context, kernel = make(dtype, rays)
    assert int(kernel.info().converge_batch) >= 2          # the streak has passes to run ahead with

    def max_kernel():
        if between == "wait":
            context.wait()
        return kernel.run_max()

    for name, classes, columns, per_ray, tolerance, limit, iterations, last, passes in expected(dtype, rays):
        load(context, columns)
        got_iterations, got_last, got_passes = converge(max_kernel, kind, tolerance, limit)
        context.wait()                                     # an unrelated entry point: the state is settled
        print(name, "device", got_iterations, got_last, "model", iterations, last, passes)
        assert (got_iterations, got_passes) == (iterations, passes), name
        same(float(got_last), last, name)
        assert np.array_equal(passes_of(context, kind, rays), np.full(rays, passes, dtype=kind)), name
    context.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_host_decided_loop_of_a_long_item(capfd, dtype):
    """converge_loop<T>: an item past 1500 nodes has no `_max` entry; Kernel.converge runs the loop on the host with the
    separate reduction kernel."""
    kind = NUMPY[dtype]
    rays = 300
    context, kernel = make(dtype, rays, padding=1600)
    assert kernel.info().num_instructions > 1500
    for name, classes, columns, per_ray, tolerance, limit, iterations, last, passes in expected(dtype, rays):
        load(context, columns)
        capfd.readouterr()
        got_iterations, got_last = kernel.converge(tolerance, limit)
        reports = capfd.readouterr().err.count(REPORT)
        print(name, "device", got_iterations, got_last, "model", iterations, last, passes)
        assert got_iterations == iterations, name
        same(got_last, last, name)
        assert reports == (1 if iterations > limit else 0), name
        assert np.array_equal(passes_of(context, kind, rays), np.full(rays, passes, dtype=kind)), name
    context.close()


@pytest.mark.parametrize("dtype", ["c32", "c64"])
def test_complex_loop(capfd, dtype):
    """converge_loop<std::complex>: the element of largest modulus, the loop on moduli; last and off_last start at 0."""
    kind = NUMPY[dtype]
    for rays in (2, 300):
        context, kernel = make(dtype, rays)
        for name, classes, columns, per_ray, tolerance, limit, iterations, last, passes in expected(dtype, rays):
            load(context, columns)
            capfd.readouterr()
            got_iterations, got_last = kernel.converge(tolerance, limit)
            reports = capfd.readouterr().err.count(REPORT)
            print(name, rays, "device", got_iterations, got_last, "model", iterations, last, passes)
            assert got_iterations == iterations, (name, rays)
            same(got_last, last, (name, rays))
            assert reports == (1 if iterations > limit else 0), (name, rays)
            assert np.array_equal(passes_of(context, kind, rays), np.full(rays, passes, dtype=kind)), (name, rays)
        context.close()


@pytest.mark.parametrize("rays", [1, 64, 65, 200])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_per_ray_loop(dtype, rays):
    """converge_per_ray: every ray leaves where the loop leaves on that ray's own script — the classes interleaved
    inside a wavefront, so the ballot sees stalled and running lanes side by side."""
    kind = NUMPY[dtype]
    context, kernel = make(dtype, rays)
    for name, classes, tolerance, limit in scripted_item.ensembles(dtype):
        columns, per_ray = scripted_item.columns(dtype, classes, rays)
        alone = [converge(scripted(scripted_item.table(dtype, classes)[k], kind), kind, tolerance, limit)
                 for k in range(len(classes))]
        iterations = max(alone[k][0] for k in per_ray)
        passes = np.array([alone[k][2] for k in per_ray])
        final = scripted_item.table(dtype, classes)[per_ray, passes - 1]
        load(context, columns)
        got_iterations, got_last = kernel.converge_per_ray(tolerance, limit)
        print(name, "device", got_iterations, got_last, "model", iterations, final[max_element(final)])
        assert got_iterations == iterations, name
        assert np.array_equal(passes_of(context, kind, rays), passes.astype(kind)), name
        assert np.array_equal(context.copy_to_host("residual", np.empty(rays, dtype=kind)), final, equal_nan=True), name
        same(got_last, final[max_element(final)], name)
    context.close()
