"""bench.py as the driver runs it, at small sizes: the one-GPU line's contract keys, and the
multi-rank path rehearsed on ONE GPU (two ranks sharing device 0 over gloo; RCCL refuses two ranks
on one device) through bench.py's own launcher."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(arguments, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + arguments, env=env,
                         capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_one_gpu_line_has_the_contract_keys():
    line = _bench(["--rays-per-gpu", "200000", "--steps", "20", "--warmup", "2", "--warmup-seconds", "0.05",
                   "--no-cpu-baseline"])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in line, key
    assert line["n_gpus"] == 1 and line["steps"] == 20 and line["dtype"] == "f64" and line["vs_baseline"] is None
    roof = line["roofline"]
    assert roof["bound"] == "hbm" and roof["peak"] == 8000.0 and 0.0 < roof["frac"] < 1.0
    assert abs(roof["frac"] - roof["achieved"]/roof["peak"]) < 1.0e-12
    assert roof["traffic"] is None or roof["traffic"] > 0
    assert roof["kernel_ms"] <= line["ms_per_step"]*1.05
    assert line["newton_iterations"] == 24
    extra = line["roofline_extra"]
#  25 passes of the Newton loop in launches of up to 3 passes: 9 launches, the loop ends on the first pass of the 9th, which is redone alone
    assert extra["loss_kernel"]["passes"] == 25 and extra["loss_kernel"]["passes_per_launch"] == 3 and extra["loss_kernel"]["launches"] == 10
    assert extra["korc_step_f32"]["frac"] > 0.1
    assert line["value_with_sync_host"] < line["value"]


def test_two_ranks_on_one_gpu_through_the_own_launcher():
    line = _bench(["--gpus", "2", "--share-gpu", "--backend", "gloo", "--total-rays", "400001", "--steps", "10",
                   "--warmup", "2", "--warmup-seconds", "0.05", "--no-extra"])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong"
    assert line["config"]["total_rays"] == 400001 and line["config"]["rays_per_gpu"] == 200001   # rank 0: the larger shard
    assert line["distributed"] == {"world_size": 2, "launcher": "bench.py", "backend": "gloo", "forced_for_one_rank": False,
                                   "rccl_version": line["distributed"]["rccl_version"]}
    assert line["all_gather_seconds"] > 0 and line["all_gather_bytes"] == 400001*8*8
    assert line["value"] > 1.0e8


def test_rccl_code_path_runs_with_a_one_rank_group():
    """the `nccl` (= RCCL) branches of distributed.py and bench.py had never
    executed.  `--gpus 1 --backend nccl --force-collectives` initialises a ONE-rank RCCL group and
    sends the item broadcast (uint8 on the device), the all-gather of the eight fp64 state arrays
    from the device tensors the kernels write, the max-over-ranks all-reduce and the barriers
    through RCCL: a wrong dtype, device or API use fails here, not on the first 8-GPU run."""
    line = _bench(["--gpus", "1", "--backend", "nccl", "--force-collectives", "--rays-per-gpu", "200000", "--steps", "10",
                   "--warmup", "2", "--warmup-seconds", "0.05", "--no-cpu-baseline", "--no-extra"])
    assert line["n_gpus"] == 1 and line["newton_iterations"] == 24
    assert line["distributed"]["backend"] == "nccl" and line["distributed"]["forced_for_one_rank"] is True
    assert line["distributed"]["rccl_version"]
    assert line["all_gather_seconds"] > 0 and line["all_gather_bytes"] == 200000*8*8


def test_korc_leg_over_rccl_with_a_one_rank_group():
    """The xkorc leg (BASELINE configs[4]) through RCCL: four items broadcast, seven fp32 device
    arrays all-gathered; identical particles, so the gathered checksum is 7 sums of n equal values."""
    line = _bench(["--workload", "korc", "--gpus", "1", "--backend", "nccl", "--force-collectives",
                   "--total-rays", "300000", "--steps", "10", "--warmup", "2", "--warmup-seconds", "0.05"])
    assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["unit"] == "particle-steps/s" and line["cpu_baseline"]["value"] > 1.0e6
    assert line["unit"] == "particle-steps/s" and line["dtype"] == "f32" and line["n_gpus"] == 1
    assert line["distributed"]["backend"] == "nccl"
    assert line["all_gather_bytes"] == 300000*4*7 and line["all_gather_checksum"] != 0.0
    assert line["config"]["axis_newton_iterations"] > 0 and 1.0 < line["config"]["b0"] < 2.0
    assert 0.0 < line["roofline"]["frac"] < 1.0


def test_korc_leg_two_ranks_on_one_gpu():
    """C5's sharded leg rehearsed on one GPU: two ranks share device 0 over gloo, 1e6+1 particles
    split 500001 + 500000 as graph_korc/xkorc.cpp:20-25 splits them; the gathered ensemble is the
    one-rank ensemble (identical particles: same checksum as the one-rank run of the same size)."""
    arguments = ["--workload", "korc", "--total-rays", "1000001", "--steps", "12", "--warmup", "3", "--warmup-seconds", "0.0",
                 "--no-cpu-baseline"]
    two = _bench(arguments + ["--gpus", "2", "--share-gpu", "--backend", "gloo"])
    one = _bench(arguments + ["--gpus", "1", "--backend", "gloo", "--force-collectives"])
    assert two["n_gpus"] == 2 and two["scaling"] == "strong"
    assert two["config"]["particles_per_gpu"] == 500001 and two["config"]["total_particles"] == 1000001
    assert two["distributed"]["backend"] == "gloo" and two["distributed"]["launcher"] == "bench.py"
    assert two["all_gather_bytes"] == 1000001*4*7
    assert two["all_gather_checksum"] == one["all_gather_checksum"]
    assert two["config"]["b0"] == one["config"]["b0"]


def _dumped(directory):
    import numpy as np
    return {name[:-4]: np.load(os.path.join(directory, name)) for name in sorted(os.listdir(directory))}


def test_dump_outputs_are_the_state_of_the_last_timed_step(tmp_path):
    """--dump-outputs writes what the timed steps computed: the same arrays as a direct run of --steps RK4 steps from
    the Newton init, bit for bit, whatever the warm-up did before the timed region."""
    import numpy as np
    import torch
    from graph_framework_amd.xrays import Rk4ColdPlasmaEfit, STATE
    rays, steps = 200000, 7
    arguments = ["--rays-per-gpu", str(rays), "--steps", str(steps), "--no-cpu-baseline", "--no-extra"]
    line = _bench(arguments + ["--warmup", "2", "--warmup-seconds", "0.05", "--dump-outputs", str(tmp_path/"a")])
    _bench(arguments + ["--warmup", "5", "--warmup-seconds", "0.3", "--dump-outputs", str(tmp_path/"b")])
    assert line["steps"] == steps and line["ms_per_step"] > 0.0
    a, b = _dumped(tmp_path/"a"), _dumped(tmp_path/"b")
    assert sorted(a) == sorted(STATE + ("residual", "sample_index"))
    for name in a:
        assert a[name].dtype == np.float64 and a[name].shape == (rays,), name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    np.testing.assert_array_equal(a["sample_index"], np.arange(rays))

    solve = Rk4ColdPlasmaEfit({k: np.full(rays, v) for k, v in
                               dict(t=0.0, w=500.0, x=2.5, y=0.0, z=0.0, kx=-600.0, ky=0.0, kz=0.0).items()},
                              device_state=True)
    solve.init("kx")
    solve.compile()
    for _ in range(steps):
        solve.step()
    host = solve.sync_host()
    torch.cuda.synchronize()
    residual = solve.device["residual"].cpu().numpy()
    solve.work.context.close()
    for k in STATE:
        np.testing.assert_array_equal(a[k], host[k], err_msg=k)
    np.testing.assert_array_equal(a["residual"], residual)
    assert a["t"][0] != 0.0


def test_dump_outputs_sample_a_large_ensemble_at_fixed_indices(tmp_path):
    """Above bench.DUMP_SAMPLE rays the dump is a seeded sample: the same indices on every run, the values of those rays."""
    import numpy as np
    import bench
    from graph_framework_amd.xrays import Rk4ColdPlasmaEfit, STATE, cli_distribution
    rays, steps = bench.DUMP_SAMPLE + 100003, 3
    _bench(["--distribution", "cli", "--rays-per-gpu", str(rays), "--steps", str(steps), "--warmup", "2",
            "--warmup-seconds", "0.05", "--no-cpu-baseline", "--no-extra", "--dump-outputs", str(tmp_path)])
    dump = _dumped(tmp_path)
    index = dump["sample_index"].astype(np.int64)
    assert index.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(index) > 0) and 0 <= index[0] and index[-1] < rays
    assert sum(os.path.getsize(tmp_path/name) for name in os.listdir(tmp_path)) <= 64*2**20
    solve = Rk4ColdPlasmaEfit(cli_distribution(rays, seed=0), device_state=True)
    solve.init("kx")
    solve.compile()
    for _ in range(steps):
        solve.step()
    host = solve.sync_host()
    solve.work.context.close()
    for k in STATE:
        np.testing.assert_array_equal(dump[k], host[k][index], err_msg=k)


def test_korc_dump_outputs_do_not_depend_on_the_warm_up(tmp_path):
    import numpy as np
    from graph_framework_amd import korc as gk
    arguments = ["--workload", "korc", "--total-rays", "100000", "--steps", "5", "--no-cpu-baseline"]
    _bench(arguments + ["--warmup", "1", "--warmup-seconds", "0.0", "--dump-outputs", str(tmp_path/"a")])
    _bench(arguments + ["--warmup", "4", "--warmup-seconds", "0.2", "--dump-outputs", str(tmp_path/"b")])
    a, b = _dumped(tmp_path/"a"), _dumped(tmp_path/"b")
    assert sorted(a) == sorted(tuple(gk.PARTICLE) + ("sample_index",))
    for k in gk.PARTICLE:
        assert a[k].dtype == np.float32 and a[k].shape == (100000,)
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
