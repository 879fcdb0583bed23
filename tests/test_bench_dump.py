"""bench.py's --steps and --dump-outputs on the host: the argument check and the sampled dump of a state."""
import os

import numpy as np
import pytest
import torch

import bench


def test_steps_must_be_positive():
    assert bench.parse_arguments(["--steps", "3"]).steps == 3
    with pytest.raises(SystemExit):
        bench.parse_arguments(["--steps", "0"])


def test_dump_of_a_small_ensemble_is_the_whole_state(tmp_path):
    state = {"x": torch.arange(10, dtype=torch.float64), "gamma": torch.arange(10, dtype=torch.float32)*0.5}
    bench.dump_outputs(str(tmp_path), state, 10, 0, 1)
    assert sorted(os.listdir(tmp_path)) == ["gamma.npy", "sample_index.npy", "x.npy"]
    np.testing.assert_array_equal(np.load(tmp_path/"x.npy"), np.arange(10.0))
    gamma = np.load(tmp_path/"gamma.npy")
    assert gamma.dtype == np.float32
    np.testing.assert_array_equal(gamma, np.arange(10, dtype=np.float32)*0.5)
    np.testing.assert_array_equal(np.load(tmp_path/"sample_index.npy"), np.arange(10.0))


def test_dump_of_a_large_ensemble_is_a_fixed_sample(tmp_path):
    total = bench.DUMP_SAMPLE*3 + 7
    values = torch.from_numpy(np.random.default_rng(5).standard_normal(total))
    bench.dump_outputs(str(tmp_path/"a"), {"kx": values}, total, 0, 1)
    bench.dump_outputs(str(tmp_path/"b"), {"kx": values}, total, 0, 1)
    index = np.load(tmp_path/"a"/"sample_index.npy")
    assert index.dtype == np.float64 and index.shape == (bench.DUMP_SAMPLE,)
    assert np.all(np.diff(index) > 0) and index[0] >= 0 and index[-1] < total
    np.testing.assert_array_equal(index, np.load(tmp_path/"b"/"sample_index.npy"))
    np.testing.assert_array_equal(np.load(tmp_path/"a"/"kx.npy"), values.numpy()[index.astype(np.int64)])


def test_dump_stays_under_64_mib():
    per_ray = 9*8 + 8        # the eight fp64 state arrays and the residual, and the indices
    assert bench.DUMP_SAMPLE*per_ray <= 64*2**20
