"""csrc/converge_state.hpp — the one place the library has the converge loop's test, the decision a launch's maxima
get on the device, and the integer image those maxima travel in — on the host alone: tests/converge_step_check.cpp,
built with -fsanitize=address,undefined, run as a child process on scripted maxima and held to tests/max_model.py.
No GPU."""
import functools
import os
import subprocess

import numpy as np
import pytest

import scripted_item
from max_model import converge, scripted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMPY = scripted_item.NUMPY
BASE = {"f32": np.float32, "f64": np.float64, "c32": np.float32, "c64": np.float64}
NAN, INF = float("nan"), float("inf")
LENGTH = 60             # every script is continued with its last element to this length: a multiple of 1 .. 5
FALLING = [64.0, 32.0, 16.0, 8.0, 4.0, 2.0]


def by_hand(dtype):
    """[(name, script, tolerance, limit)]: the scripts of test_max_model.py's tests of the loop."""
    big = float(np.finfo(BASE[dtype]).max)
    out = [([8.0, 4.0, 0.5, 99.0], 1.0, 100), ([0.5, 99.0], 1.0, 100), ([8.0, 1.0, 99.0], 1.0, 100),
           ([8.0, 5.0, 5.0, 99.0], 0.25, 100), ([8.0, 3.0, 8.0, 3.0, 8.0, 3.0], 0.25, 100),
           ([9.0, 8.0, 3.0, 8.0, 3.0, 8.0], 0.25, 100), ([8.0, 4.0, NAN, 1.0], 0.25, 100), ([NAN, 1.0], 0.25, 100),
           (FALLING, 0.25, 0), (FALLING, 0.25, 1), (FALLING, 0.25, 2), (FALLING, 0.25, 4),
           ([8.0, 4.0, 0.5, 99.0], -1.0, 100), ([INF, 7.0, 0.5], 1.0, 100), ([INF, INF, 0.5], 1.0, 100),
#  test_starting_values_of_last
           ([big, 1.0], 0.5, 10), ([big, 3.0, 0.25], 0.5, 10),
#  test_the_tolerance_is_narrowed_to_the_items_type
           ([4.0, 1.0e-40, 1.0e-44, 1.0e-44, 9.0], 1.0e-50, 100), ([4.0, 0.0, 9.0], 1.0e-50, 100),
           ([4.0, 1.0e-60, 9.0], 1.0e-50, 100),
#  test_fp32_compares_in_float
           (scripted_item.FLOAT_CASE, 0.1, 100)]
    return [("hand%d" % n, script, tolerance, limit) for n, (script, tolerance, limit) in enumerate(out)]


@functools.lru_cache(maxsize=None)
def cases(dtype):
    """[(name, maxima in `dtype`, tolerance, limit, the model's (iterations, last, passes))]: the scripts by hand and
    the per-pass maxima of every scripted_item.ensembles case at 7 rays."""
    kind = NUMPY[dtype]
    scripts = by_hand(dtype)
    for name, classes, tolerance, limit in scripted_item.ensembles(dtype):
        _, per_ray = scripted_item.columns(dtype, classes, 7)
        scripts.append((name, scripted_item.maxima(dtype, classes, per_ray), tolerance, limit))
    out = []
    for name, script, tolerance, limit in scripts:
        with np.errstate(all="ignore"):
            maxima = np.asarray(script, dtype=kind)
        maxima = np.concatenate([maxima, np.full(LENGTH - len(maxima), maxima[-1])])
        model = converge(scripted(maxima, kind), kind, tolerance, limit)
        assert model[2] <= LENGTH - 5, name                 # the loop ends inside the script, whatever the launch
        out.append((name, maxima, tolerance, limit, model))
    return out


def unsigned(dtype):
    return np.uint32 if dtype in (np.float32, np.complex64) else np.uint64


def words(values):
    """The bits of every number of `values`, in hexadecimal (complex: re im)."""
    return " ".join("%x" % b for b in np.ascontiguousarray(values).view(unsigned(values.dtype)))


def line(dtype, mode, maxima, tolerance, limit):
    return "%s %s %d %s %s" % (dtype, words(np.array([tolerance], dtype=np.float64)), limit, mode, words(maxima))


def key_values(dtype):
    """Sorted: -inf, -max, ordinary, -subnormal, -0, +0, ... +inf."""
    kind = NUMPY[dtype]
    info = np.finfo(kind)
    positive = [0.0, float(info.smallest_subnormal), float(info.smallest_subnormal)*5, float(info.tiny), 0.1, 1.0, 1.5, 1000.25,
                float(info.max), INF]
    return np.array([-x for x in reversed(positive)] + positive, dtype=kind)


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """Every case through one run of the sanitized program: {input line: the numbers it printed}."""
    binary = str(tmp_path_factory.mktemp("converge_step")/"converge_step_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", binary, os.path.join(ROOT, "tests", "converge_step_check.cpp")])
    lines = []
    for dtype in ("f32", "f64", "c32", "c64"):
        for name, maxima, tolerance, limit, _ in cases(dtype):
            lines.append(line(dtype, "loop", maxima, tolerance, limit))
            if dtype in ("f32", "f64"):
                lines += [line(dtype, "decide %d" % count, maxima, tolerance, limit) for count in range(1, 6)]
    for dtype in ("f32", "f64"):
        lines.append("%s keys %s" % (dtype, words(key_values(dtype))))
    out = subprocess.run([binary], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    printed = out.stdout.splitlines()
    assert len(printed) == len(lines)
    return dict(zip(lines, printed))


def same_bits(got, want, note):
    """`got`: the printed words of one value; `want`: the model's scalar.  Bit for bit, or both a NaN (the reduction
    hands on a canonical NaN, not the element's payload)."""
    want = np.array([want])
    got = np.array([int(word, 16) for word in got], dtype=unsigned(want.dtype)).view(want.dtype)
    assert got.tobytes() == want.tobytes() or (np.isnan(got[0]) and np.isnan(want[0])), (note, got, want)


@pytest.mark.parametrize("dtype", ["f32", "f64", "c32", "c64"])
def test_the_loop_on_the_step_is_the_model(answers, dtype):
    parts = 2 if dtype in ("c32", "c64") else 1
    for name, maxima, tolerance, limit, (iterations, last, passes) in cases(dtype):
        got = answers[line(dtype, "loop", maxima, tolerance, limit)].split()
        print(name, got, "model", iterations, last, passes)
        assert len(got) == 2 + parts, name
        assert int(got[0]) == iterations, name
        same_bits(got[1:1 + parts], last, name)
        assert int(got[-1]) == passes, name


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_decision_on_the_maxima_of_a_launch_is_the_model(answers, dtype, count):
    ends = set()
    for name, maxima, tolerance, limit, (iterations, last, passes) in cases(dtype):
        got = answers[line(dtype, "decide %d" % count, maxima, tolerance, limit)].split()
        print(name, got, "model", iterations, last, passes)
        assert len(got) == 8, name
        consumed, ran, batch_passes, extra, cleared, idle = (int(word) for word in got[2:])
        assert ran == passes, name
        assert batch_passes == (passes - 1) % count + 1, name
        assert extra == count - batch_passes, name
        assert int(got[0]) == iterations, name
        same_bits(got[1:2], last, name)
        assert consumed == passes + extra, name             # whole launches, and none after the one the loop ended in
        assert cleared == 1, name                           # every slot left zero for the next launch's atomicMax
        assert idle == 1, name                              # once done, a decide touches neither state nor slots
        ends.add((passes - 1) % count)
    assert ends == set(range(count)), ends                  # the loop ends on every position of a launch


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_ordered_key_is_increasing_and_comes_back(answers, dtype):
    values = key_values(dtype)
    assert np.all(values[:-1] <= values[1:]) and np.signbit(values[len(values)//2 - 1]) and not np.signbit(values[len(values)//2])
    pairs = [pair.split(":") for pair in answers["%s keys %s" % (dtype, words(values))].split()]
    assert [back for _, back in pairs] == words(values).split()
    keys = [int(key, 16) for key, _ in pairs]
    assert all(a < b for a, b in zip(keys, keys[1:])), keys  # strictly: +0 images above -0
    assert max(keys) < (1 << 8*values.dtype.itemsize) - 1    # below the all-ones key that stands for a NaN at element 0
