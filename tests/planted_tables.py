"""Planted coefficient tables and gather arguments for the table tests (tests/test_tables.py on the CPU,
tests/test_gpu_tables.py on the device).

The lowering rewrites a gather more than any other operation (graph_framework_amd/csrc/tables.hpp drops tables that
are a constant multiple of another, packs the rest per shape and stages packs in LDS; codegen.hpp and asm_body.hpp
each compute the clamped index with a shared-reciprocal quotient), and random tables with random arguments meet none
of the places where that can go wrong.  Here the tables hold zeros of both signs, subnormals, the largest finite
value, an infinity and a NaN, and are the multiples of one another that the compaction looks for; the arguments sit
on the cell boundaries fl(offset + k*scale) and within three units in the last place of them.

`model()` of a probe is a numpy restatement of the item, written from include/gfir.h and the reference's
piecewise.hpp:26-65: q = (x - offset)/scale in the item's precision, the cell trunc(min(max(q, 0), length - 1)).
"""
import ctypes
import ctypes.util

import numpy as np

from test_gpu_division import _bits, _same
from test_gpu_generic import Item, INPUT, DIV, FMA, GATHER1, GATHER2, INDEX1, INDEX2

REAL = {"f64": np.float64, "f32": np.float32}
LENGTHS = (7, 16, 33)
ROWS, COLS = 5, 6
#  (scale, offset) of the index of each table length (rounded to the item's precision where they are used): 0.1 and
#  0.3 have no finite binary expansion, the third is what tests/gfir_random.py draws, 0.25 / -2.0 is exact.
ARGUMENTS = {33: (0.1, -1.0), 16: (0.3, -0.7), 7: (2.2/7*0.83, -0.91), ROWS: (0.25, -2.0), COLS: (0.3, -0.7)}
#  1 x L tables that certainly are derived / certainly stay stored (tests/test_tables.py)
DERIVED = {"flipped": ("base", -1.0), "minus_two_c": ("c", -2.0)}
ORDINARY = ("three_c", "c", "minus_two_c", "back", "d", "ulp_off", "d_third", "d_tenth")      # finite values of O(1)
STORED = ("base", "unflipped", "zeros", "negative_zeros", "infinity", "nan", "ulp_off")


def same_bits(got, want):
    """Bit equality, the sign of a zero included; NaNs must coincide (payloads may differ)."""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and _same(got, want)


def differing(got, want):
    """Lanes that same_bits() objects to (for assertion messages)."""
    nan = np.isnan(want)
    return np.flatnonzero((np.isnan(got) != nan) | (~nan & (_bits(got) != _bits(want))))


def _row(real, length, head, rng):
    """`head` followed by ordinary values of full mantissa, as a 1 x length float64 array of `real` values."""
    rest = rng.uniform(-1.0, 1.0, length - len(head)).astype(real)
    return np.concatenate([np.array(head, dtype=real), rest]).astype(np.float64).reshape(1, length)


def planted_tables(dtype):
    """[(name, float64 array)]: the tables of gather_probe(dtype) in item order.  Every value is a `dtype` value and
    every product is taken in `dtype`, so that `k*parent` below has the bits the device's multiply gives."""
    real = REAL[dtype]
    info = np.finfo(real)
    tiny = float(np.nextafter(real(0), real(1)))
    tables = []
    with np.errstate(all="ignore"):
        for length in LENGTHS:
            rng = np.random.default_rng(100 + length)

            def multiple(k, t):
                return (real(k)*t.astype(real)).astype(np.float64)

            def add(name, t):
                tables.append(("%s_%d" % (name, length), t))
                return t

#  The largest magnitude sits in the last cell; half a table further on is an ordinary value (tables.hpp's two-cell
#  pre-test looks at these two).
            base = add("base", _row(real, length, [0.0, -0.0, 0.75], rng))
            base[0, -3:] = [tiny, 3.0*tiny, float(info.max)]
#  The only negative power of two that is exact on both the smallest subnormal and the largest finite value is
#  -2^0: the zeros' signs flip and nothing else changes, so this one MUST be derived ...
            flipped = add("flipped", multiple(-1.0, base))
#  ... and with the zeros' signs of the base it is no multiple of it: k*(+0) is -0 for every negative k.
            unflipped = add("unflipped", flipped.copy())
            unflipped[0, :2] = base[0, :2]
#  (a largest cell of 1: 3*c is exact there, which is where the lowering takes its candidate factors from)
            c = _row(real, length, [0.0, -0.0, 1.0], rng)
            add("three_c", multiple(3.0, c))                   # met before c: the second, re-parenting pass
            add("c", c)
            minus_two_c = add("minus_two_c", multiple(-2.0, c))
            add("back", multiple(-0.5, minus_two_c))           # a chain: the bits of c again
            add("zeros", np.zeros((1, length)))
            add("negative_zeros", -np.zeros((1, length)))
            infinity = add("infinity", _row(real, length, [], rng))
            infinity[0, length//3] = np.inf
            nan = add("nan", _row(real, length, [], rng))
            nan[0, 2*length//3] = np.nan
#  (a table of its own and not c's: (-4/3)*three_c may well have the bits of a seven-cell -4*c that is one ulp off)
            d = add("d", _row(real, length, [0.0, -0.0, 1.0], rng))
            ulp_off = add("ulp_off", multiple(-4.0, d))
            ulp_off[0, length//2] = float(np.nextafter(real(ulp_off[0, length//2]), real(0)))
            add("d_third", (d.astype(real)/real(3.0)).astype(np.float64))      # correctly rounded quotients and products:
            add("d_tenth", multiple(0.1, d))                                   # derivable or not, the invariant holds
        rng = np.random.default_rng(100)
        base2 = rng.uniform(-1.0, 1.0, (ROWS, COLS)).astype(real).astype(np.float64)
        base2[0, 0], base2[2, 3], base2[ROWS - 1, COLS - 1], base2[1, 1] = 0.0, -0.0, 0.0, 3.0*tiny
        tables.append(("base_%dx%d" % (ROWS, COLS), base2))
        tables.append(("multiple_%dx%d" % (ROWS, COLS), (real(-4.0)*base2.astype(real)).astype(np.float64)))
    return tables


def planted_arguments(real, scale, offset, length):
    """Arguments whose quotient (x - offset)/scale lies on or within rounding of an integer — fl(offset + k*scale) for
    k = 0 .. length + 1 with three neighbours on either side — and the values an index has to clamp."""
    scale, offset = real(scale), real(offset)
    info = np.finfo(real)
    tiny = np.nextafter(real(0), real(1))
    values = []
    for k in range(length + 2):
        x = real(offset + real(k)*scale)
        below = above = x
        values.append(x)
        for _ in range(3):
            below, above = np.nextafter(below, real(-np.inf)), np.nextafter(above, real(np.inf))
            values += [below, above]
    values += [0.0, -0.0, tiny, -tiny, offset, info.max, -info.max, np.inf, -np.inf, np.nan,
               offset - real(1000.0)*scale, offset + real(1000.0 + length)*scale, real(-1.0e30), real(1.0e30)]
    return np.array(values, dtype=real)


def cell(real, x, scale, offset, length):
    """The cell a gather reads, in the item's precision (piecewise.hpp:26-65).  A NaN argument is undefined in the
    reference (std::max / std::min hand it on into an integer cast); this project reads cell 0 for it, which is what
    fmax(NaN, 0) gives, and the model pins that choice."""
    with np.errstate(all="ignore"):
        q = (x - real(offset))/real(scale)
        return np.trunc(np.fmin(np.fmax(q, real(0)), real(length - 1))).astype(np.int64)


def _fma(real, a, b, c):
    """Correctly rounded a*b + c, lane by lane (libm's fma / fmaf; numpy has none)."""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    kind = ctypes.c_double if real == np.float64 else ctypes.c_float
    f = libm.fma if real == np.float64 else libm.fmaf
    f.restype, f.argtypes = kind, [kind]*3
    return np.array([f(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=real)


class Probe:
    """A work item with its numpy model: `blob`, `in_keys`, `out_keys`, `records`, and model(columns), which
    returns the outputs of one pass and applies the setters to `columns` in place."""

    def __init__(self, dtype):
        self.dtype, self.real = dtype, REAL[dtype]
        self.steps = []                                        # ("cell1" | "cell2" | "fma" | "quotient", ...) per value, in order
        self.stored = []                                       # the values that are outputs
        self.setter = None                                     # (value, column it is stored to)

    def model(self, columns):
        real = self.real
        values = []
        for step in self.steps:
            if step[0] == "cell1":
                _, data, column, (scale, offset) = step
                flat = data.astype(real).ravel()
                values.append(flat[cell(real, columns[column], scale, offset, flat.size)])
            elif step[0] == "cell2":
                _, data, first, second, (xs, xo), (ys, yo) = step
                rows, cols = data.shape
                at = cell(real, columns[first], xs, xo, rows)*cols + cell(real, columns[second], ys, yo, cols)
                values.append(data.astype(real).ravel()[at])
            elif step[0] == "fma":
                _, a, b, c = step
                with np.errstate(all="ignore"):
                    values.append(_fma(real, values[a], values[b], values[c]))
            else:
                _, column = step
                x = columns[column]
                with np.errstate(all="ignore"):
                    values.append(real(1.0)/_fma(real, x, x, np.full(x.size, 2.0, dtype=real)))
        if self.setter is not None:
            columns[self.setter[1]][:] = values[self.setter[0]]
        return [values[v] for v in self.stored]


def _quotient(it, probe, x):
    """1/(x*x + 2) as one more value.  An item that divides nothing is lowered without the shared-reciprocal division,
    and with it go the index quotients through gf_div, the window check and the assembly body: one DIV record brings
    them in.  The numerator is a constant (the default mode does not track subnormal numerators, prelude.hpp); an
    infinite or NaN x leaves the window."""
    node = it.emit(DIV, it.constant(1.0), it.emit(FMA, x, x, it.constant(2.0)))
    probe.steps.append(("quotient", 0))
    return node


def _rounded(real, pair):
    return float(real(pair[0])), float(real(pair[1]))


def gather_probe(dtype, padding=0, lengths=LENGTHS, names=None, two_d=True, stored=None, weave=False):
    """Inputs x, y.  One GATHER1 per planted 1 x L table on x (one index group per L), one GATHER2 per planted 2-D
    table on (x, y); every gather is an output, an FMA of three derived gathers is one more (a deferred `k*parent`
    consumed by arithmetic), a quotient another (_quotient), and y <- the gather of the longest base table, so that a
    second pass gathers with a gathered argument (zeros of both signs, subnormals and the largest finite value).
    `padding` FMA records lengthen the item for the lowerings that cut it into segments.  `lengths`, `names` (of the
    1 x L tables, without their length) and `two_d` take a part of the tables and `stored` makes only some of the 1 x L
    gathers outputs: every output of the assembly body stays in a register to the end of its statement, which bounds
    their number.  `weave` adds a chain a_i = fma(a_(i-1), g_i, g_i) over the gathers of ordinary values and a second
    one that consumes a_i and g_i in reverse order: all of them are live at the turn, more than a small register pool
    holds."""
    real = REAL[dtype]
    probe = Probe(dtype)
    it = Item(dtype, False, ["x", "y"], name="gather_probe")
    x, y = it.emit(INPUT, a=0), it.emit(INPUT, a=1)
    nodes, index = [], {}
    for name, data in planted_tables(dtype):
        if data.shape[0] == 1:
            if data.shape[1] not in lengths or (names is not None and name.rsplit("_", 1)[0] not in names):
                continue
        elif not two_d:
            continue
        it.tables.append(data)
        table = len(it.tables) - 1
        if data.shape[0] == 1:
            pair = _rounded(real, ARGUMENTS[data.shape[1]])
            nodes.append(it.emit(GATHER1, x, aux=table, imm=pair + (0.0, 0.0)))
            probe.steps.append(("cell1", data, 0, pair))
        else:
            first, second = _rounded(real, ARGUMENTS[ROWS]), _rounded(real, ARGUMENTS[COLS])
            nodes.append(it.emit(GATHER2, x, y, aux=table, imm=first + second))
            probe.steps.append(("cell2", data, 0, 1, first, second))
        index[name] = len(nodes) - 1
    probe.stored = [v for name, v in index.items()
                    if stored is None or probe.steps[v][0] == "cell2" or name.rsplit("_", 1)[0] in stored]
    mix = [index["%s_%d" % (name, lengths[i % len(lengths)])] for i, name in enumerate(("flipped", "minus_two_c", "three_c"))]
    nodes.append(it.emit(FMA, *[nodes[v] for v in mix]))
    probe.steps.append(("fma",) + tuple(mix))
    probe.stored.append(len(nodes) - 1)
    nodes.append(_quotient(it, probe, x))
    probe.stored.append(len(nodes) - 1)
    if weave:
        ordinary = [v for name, v in index.items() if name.rsplit("_", 1)[0] in ORDINARY]
        chain = [ordinary[0]]
        for g in ordinary[1:]:
            nodes.append(it.emit(FMA, nodes[chain[-1]], nodes[g], nodes[g]))
            probe.steps.append(("fma", chain[-1], g, g))
            chain.append(len(nodes) - 1)
        for a, g in zip(reversed(chain[:-1]), reversed(ordinary[:-1])):
            nodes.append(it.emit(FMA, nodes[-1], nodes[a], nodes[g]))
            probe.steps.append(("fma", len(nodes) - 2, a, g))
        probe.stored.append(len(nodes) - 1)
    for _ in range(padding):                                   # a chain across the cuts; its end is stored
        a, b = index["c_%d" % lengths[0]], index["back_%d" % lengths[1 % len(lengths)]]
        nodes.append(it.emit(FMA, nodes[-1], nodes[a], nodes[b]))
        probe.steps.append(("fma", len(nodes) - 2, a, b))
    if padding:
        probe.stored.append(len(nodes) - 1)
    probe.setter = (index["base_%d" % lengths[-1]], 1)
    probe.blob = it.blob([nodes[v] for v in probe.stored], [(nodes[probe.setter[0]], 1)])
    probe.in_keys, probe.out_keys = ["x", "y"], ["o%d" % i for i in range(len(probe.stored))]
    probe.names, probe.records = index, len(it.code)
    return probe


def index_probe(dtype, rays):
    """INDEX1 on a buffer per L and INDEX2 on a 5 x 6 buffer, filled with the planted base tables' cells (an input
    buffer holds at least one element per ray: the rest is a value no index may reach), on the arguments of
    gather_probe, and the quotient of _quotient.  Returns (probe, buffers)."""
    real = REAL[dtype]
    probe = Probe(dtype)
    tables = dict(planted_tables(dtype))
    names = ["base_%d" % length for length in LENGTHS] + ["base_%dx%d" % (ROWS, COLS)]
    it = Item(dtype, False, ["x", "y"] + names, name="index_probe")
    x, y = it.emit(INPUT, a=0), it.emit(INPUT, a=1)
    outputs, buffers = [], []
    for number, name in enumerate(names):
        data = tables[name]
        assert data.size <= rays
        buffers.append(np.concatenate([data.astype(real).ravel(), np.full(rays - data.size, 12345.0, dtype=real)]))
        if data.shape[0] == 1:
            pair = _rounded(real, ARGUMENTS[data.shape[1]])
            outputs.append(it.emit(INDEX1, x, c=2 + number, aux=data.shape[1], imm=pair + (0.0, 0.0)))
            probe.steps.append(("cell1", data, 0, pair))
        else:
            first, second = _rounded(real, ARGUMENTS[ROWS]), _rounded(real, ARGUMENTS[COLS])
            outputs.append(it.emit(INDEX2, x, y, c=2 + number, aux=COLS, reserved=ROWS, imm=first + second))
            probe.steps.append(("cell2", data, 0, 1, first, second))
    outputs.append(_quotient(it, probe, x))
    probe.stored = list(range(len(outputs)))
    probe.blob = it.blob(outputs, [])
    probe.in_keys, probe.out_keys = ["x", "y"] + names, ["o%d" % i for i in range(len(outputs))]
    probe.records = len(it.code)
    return probe, buffers


def probe_arguments(dtype):
    """The lanes of both probes: x runs through the planted arguments of every index it feeds, y through the same
    values in another order, so that the 2-D cells meet every row boundary with several columns."""
    real = REAL[dtype]
    x = np.concatenate([planted_arguments(real, *_rounded(real, ARGUMENTS[length]), length)
                        for length in LENGTHS + (ROWS,)])
    y = np.roll(x[::-1], 17).copy()
    return [x, y]
