"""A converge item whose residuals are dictated by data, for the tests of the converge loops.

    inputs   c     per ray: the number of passes that ran on this ray (starts at 0)
             base  per ray: class*K
             v     a buffer of CLASSES scripts of K elements each
    output   v[c + base]            (index_1D with scale 1 and offset 0: the element itself)
    setter   c <- c + 1

Ray r belongs to class r % len(classes), so the classes are interleaved inside a wavefront.  One compiled
kernel serves every script; after a loop, c == passes run, on every ray.  Test infrastructure only.
"""
import numpy as np

from test_gpu_generic import ADD, INDEX1, INPUT, MUL, Item

K = 40                  # script length
CLASSES = 8
LENGTH = K*CLASSES      # what the index node addresses
NUMPY = {"f32": np.float32, "f64": np.float64, "c32": np.complex64, "c64": np.complex128}
NAN, INF = float("nan"), float("inf")


def blob(dtype, padding=0):
    """The item as GFIR bytes.  `padding` appends that many multiplications by one to the output (the same bits,
    a longer item: past 1500 nodes an item has no `_max` entry)."""
    it = Item(dtype, False, ["c", "base", "v"], name="scripted" + (str(padding) if padding else ""))
    c, base = it.emit(INPUT, a=0), it.emit(INPUT, a=1)
    picked = it.emit(INDEX1, it.emit(ADD, c, base), c=2, aux=LENGTH, imm=(1.0, 0.0, 0.0, 0.0))
    one = it.constant(1.0)
    for _ in range(padding):
        picked = it.emit(MUL, picked, one)
    return it.blob([picked], [(it.emit(ADD, c, one), 0)])


def identity_blob(dtype):
    """A real item without setters whose output is its input bit for bit (times one)."""
    it = Item(dtype, False, ["a"], name="identity")
    return it.blob([it.emit(MUL, it.emit(INPUT, a=0), it.constant(1.0))], [])


def table(dtype, classes):
    """(CLASSES, K) array of the scripts, each continued with its last element, unused classes zero."""
    assert 1 <= len(classes) <= CLASSES
    out = np.zeros((CLASSES, K), dtype=NUMPY[dtype])
    for row, script in zip(out, classes):
        assert 1 <= len(script) <= K
        row[:len(script)] = script
        row[len(script):] = script[-1]
    return out


def columns(dtype, classes, rays):
    """([c, base, v], class of every ray) for an ensemble of `rays` rays; v is as long as the ensemble at least."""
    kind = NUMPY[dtype]
    per_ray = np.arange(rays) % len(classes)
    v = np.zeros(max(LENGTH, rays), dtype=kind)
    v[:LENGTH] = table(dtype, classes).ravel()
    return [np.zeros(rays, dtype=kind), (per_ray*K).astype(kind), v], per_ray


def outputs(dtype, classes, per_ray, at):
    """The output of pass `at`, numpy in `dtype`."""
    return table(dtype, classes)[per_ray, min(at, K - 1)]


def maxima(dtype, classes, per_ray):
    """What max_element selects from the output of passes 0 .. K-1."""
    from max_model import max_element
    picked = []
    for at in range(K):
        values = outputs(dtype, classes, per_ray, at)
        picked.append(values[max_element(values)])
    return np.array(picked, dtype=NUMPY[dtype])


def quiet(script):
    """A companion class that never holds the maximum of a script of non-negative values."""
    return [x/2 if np.isfinite(x) else 1.0 for x in script]


def falling(count, first=20):
    """2^first, 2^(first-1), ...: strictly decreasing, exact in every type."""
    return [2.0**(first - j) for j in range(count)]


U = 2.0**-27
FLOAT_CASE = [26843548*U, 13421775*U, 0.05, 99.0]       # see test_max_model.test_fp32_compares_in_float


def cases(dtype):
    """[(name, script, tolerance, limit)]: every exit of the loop, each on several passes, so that with 1 to 5
    passes per launch every exit falls on the first, a middle and the last pass of a launch."""
    out = []
    for at in range(8):
        out.append(("tol@%d" % at, falling(at) + [0.125, 99.0, 98.0], 0.25, 100))
    for at in range(1, 8):
        out.append(("constant@%d" % at, falling(at) + [2.0**(21 - at), 99.0, 98.0], 0.25, 100))
    for start in range(5):
        out.append(("period2@%d" % start, falling(start) + [7.0, 3.0]*8, 0.25, 100))
    for limit in (0, 1, 2, 7):
        out.append(("limit%d" % limit, falling(K), 1.0e-30, limit))
    for at in (0, 1, 2, 3, 4, 5):
        out.append(("nan@%d" % at, falling(at) + [NAN, 99.0, 98.0], 0.25, 100))
    out.append(("inf falls", [INF] + falling(3) + [0.125, 99.0], 0.25, 100))
    out.append(("inf twice", [5.0, INF, INF, 99.0], 0.25, 100))
    out.append(("negative tolerance", falling(4) + [0.125, 99.0], -0.25, 100))
    out.append(("tolerance 0.0f", [4.0, 1.0e-40, 1.0e-44, 1.0e-44, 9.0, 8.0], 1.0e-50, 100))
    out.append(("exact zero", [4.0, 2.0, 0.0, 9.0], 1.0e-50, 100))
    out.append(("float tolerance", FLOAT_CASE, 0.1, 100))
    return out


def ensembles(dtype):
    """[(name, classes, tolerance, limit)]: cases() with a quiet second class, and the ones that need the classes
    to differ: a NaN hidden at a later ray, and a maximum that moves between rays."""
    out = [(name, [script, quiet(script)], tolerance, limit) for name, script, tolerance, limit in cases(dtype)]
    loud = falling(6) + [0.125, 99.0]
    for at in (1, 2, 3):
        hidden = falling(at, first=10) + [NAN]*(7 - at)                 # ray 1, 4, ...: skipped, the loop goes on
        out.append(("hidden nan@%d" % at, [loud, hidden, quiet(loud)], 0.25, 100))
    moving_a = [900.0, 10.0, 700.0, 8.0, 500.0, 0.125, 0.0625, 99.0]
    moving_b = [20.0, 800.0, 9.0, 600.0, 7.0, 0.0625, 0.125, 98.0]
    out.append(("moving maximum", [moving_a, moving_b, quiet(moving_a)], 0.25, 100))
    if dtype in ("c32", "c64"):
        turned_a = [x*(0.6 + 0.8j) for x in moving_a]
        turned_b = [x*(-0.8 + 0.6j) for x in moving_b]
        out.append(("moving modulus", [turned_a, turned_b, quiet(moving_a)], 0.25, 100))
        first_nan = [complex(64.0, 0), complex(NAN, 1.0), complex(99.0, 0)]
        others = [complex(0, 32.0), complex(0, 500.0), complex(0, 98.0)]
        out.append(("nan modulus at ray 0", [first_nan, others], 0.25, 100))
        out.append(("nan modulus at ray 1", [others, first_nan], 0.25, 100))
    return out
