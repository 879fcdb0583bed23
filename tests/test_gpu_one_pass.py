"""pipeline.OnePass against the three stages it replaces (trace file -> run_absorption -> bin_power,
graph_driver/xrays.cpp:1100-1105): the same work items on the same values in the same order, so every record of every
variable is compared as 64-bit patterns, with no tolerance.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, STATE

pytestmark = pytest.mark.gpu

VARIABLES = ("time", "residual", "w", "x", "y", "z", "kx", "ky", "kz", "kamp", "power", "d_power")
RAYS = 264                                                   # 33 x the golden's 8: past one workgroup, no multiple of 64
EDGES = (np.linspace(1.7, 2.4, 5), np.linspace(-0.2, 0.05, 4), np.linspace(-0.15, 0.15, 6))     # part of the beam is outside


def read_all(path):
    """{variable: (records, rays) uint64} (kamp: (records, 2, rays)) and the number of records."""
    from graph_framework_amd.output import ResultFile
    result = ResultFile(path)
    out = {}
    for name in VARIABLES:
        if name == "kamp":
            rows = [np.stack([result.read(name, r), result.read(name, r, part=1)]) for r in range(result.records)]
        else:
            rows = [result.read(name, r) for r in range(result.records)]
        out[name] = np.stack(rows).view(np.uint64)
    records = result.records
    result.close()
    return out, records


def golden_records():
    records = np.load(os.path.join(GOLDEN, "absorption_golden.npz"))["records"]
    assert records.shape == (21, 9, 8)
    return np.ascontiguousarray(np.tile(records, (1, 1, RAYS//8)))


def three_stages(path, records, model, deposition):
    from graph_framework_amd.absorption import bin_power, run_absorption
    from graph_framework_amd.output import RAY_VARIABLES, ResultFile
    saved = records.shape[0]
    trace = ResultFile(path, RAYS)
    for name, _ in RAY_VARIABLES:
        trace.create_variable(name)
    column = {k: i for i, k in enumerate(STATE + ("residual",))}
    for r in range(saved):
        trace.write({name: records[r, column[key]] for name, key in RAY_VARIABLES})
    trace.close()
    absorption = run_absorption(path, saved - 1, model=model)
    bin_power(path, saved - 1, deposition=deposition)
    return getattr(absorption, "iterations", None)


def one_pass(path, records, model, deposition):
    """The same records fed to a bare context of nine fp64 buffers, record() after each."""
    from graph_framework_amd import Context, _lib
    from graph_framework_amd.backend import key_of
    from graph_framework_amd.pipeline import OnePass
    source = Context(0)
    names = STATE + ("residual",)
    for name in names:
        source._check(source.lib.gfhip_allocate_buffer(source.handle, key_of(name), RAYS, _lib.GFIR_F64))
    pipeline = OnePass(source, RAYS, path, model=model, deposition=deposition)
    for r in range(records.shape[0]):
        for i, name in enumerate(names):
            source.copy_to_device(name, records[r, i])
        pipeline.record()
    pipeline.close()
    source.close()
    return pipeline.iterations


def grids():
    from graph_framework_amd import Context
    from graph_framework_amd.deposition import Deposition
    context = Context(0)
    return context, Deposition(context, *EDGES), Deposition(context, *EDGES)


@pytest.mark.parametrize("model,binned", [("weak_damping", False), ("root_find", False), ("weak_damping", True)],
                         ids=["weak_damping", "root_find", "weak_damping_with_a_grid"])
def test_one_pass_equals_the_three_stages(tmp_path, model, binned):
    records = golden_records()
    context, first, second = grids() if binned else (None, None, None)
    staged = three_stages(str(tmp_path / "staged0.nc"), records, model, first)
    direct = one_pass(str(tmp_path / "direct0.nc"), records, model, second)
    want, saved = read_all(str(tmp_path / "staged0.nc"))
    got, count = read_all(str(tmp_path / "direct0.nc"))
    assert saved == count == records.shape[0]
    for name in VARIABLES:
        assert got[name].shape == want[name].shape, name
        differ = np.argwhere(got[name] != want[name])
        assert differ.size == 0, "%s: %d words differ, the first at %r" % (name, len(differ), differ[0])
    assert want["kamp"][:, 1].any()
    if model == "weak_damping":
        assert (want["power"].view(np.float64)[-1] < 0.5).all()                                # the pass did absorb
    if model == "root_find":
        assert len(staged) == saved and list(direct) == list(staged)
    if binned:
        assert first.counts() == second.counts()
        counts = first.counts()
        assert counts["samples"] == saved*RAYS and 0 < counts["outside"] < counts["samples"]
        assert first.state().tobytes() == second.state().tobytes()
        assert first.read(1.0).sum() > 0.0
        first.close()
        second.close()
        context.close()


def test_writer_errors_surface_on_the_next_call(tmp_path):
    """A write that fails in the writer thread is raised by the next record() or close()."""
    from graph_framework_amd import Context, _lib
    from graph_framework_amd.backend import key_of
    from graph_framework_amd.pipeline import OnePass
    records = golden_records()
    source = Context(0)
    names = STATE + ("residual",)
    for i, name in enumerate(names):
        source._check(source.lib.gfhip_allocate_buffer(source.handle, key_of(name), RAYS, _lib.GFIR_F64))
        source.copy_to_device(name, records[0, i])
    pipeline = OnePass(source, RAYS, str(tmp_path / "broken0.nc"))

    def refuse(record, index=None):
        raise IOError("the disk is full")
    pipeline.file.write = refuse
    pipeline.record()
    with pytest.raises(IOError, match="disk is full"):
        pipeline.record()
    pipeline.record()                                        # the error was taken; this write fails in its turn
    with pytest.raises(IOError, match="disk is full"):
        pipeline.close()
    source.close()


def test_example_in_one_pass_writes_the_file_of_the_three_stages(tmp_path):
    """examples/trace_rays.py with and without --one-pass, a child process each: 11 records, all twelve variables
    bit for bit, the same summary line."""
    outputs = []
    for flag, prefix in (([], str(tmp_path / "staged")), (["--one-pass"], str(tmp_path / "direct"))):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "trace_rays.py"), "--rays", "512", "--dispersion",
                              "ordinary_wave", "--steps", "4000", "--sub-steps", "400", "--output", prefix,
                              "--absorption-model", "weak_damping"] + flag, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr      # the second process starts only behind a clean first
        assert "transmitted power" in out.stdout
        outputs.append(out.stdout)
    want, saved = read_all(str(tmp_path / "staged0.nc"))
    got, count = read_all(str(tmp_path / "direct0.nc"))
    assert saved == count == 11
    for name in VARIABLES:
        assert np.array_equal(got[name], want[name]), name
    assert want["x"].shape == (11, 512)
    transmitted = [text.split("transmitted power")[1] for text in outputs]
    assert transmitted[0] == transmitted[1]
