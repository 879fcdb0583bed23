"""The max reductions of converge items against std::max_element as tests/max_model.py models it, on data planted
where the kernels' structure could lose, duplicate or misorder an element: the alignment head, the 16-byte pairs,
the odd tail, the 64-lane waves, the blocks, the grid capped at the CU count with its stride loop.

Every comparison is exact.  The device's result has the bits of `values[max_element(values)]`, except that a zero is
compared as a number (-0 == +0: which zero the ordered-integer atomicMax keeps depends on the layout) and that a NaN
— selected only at element 0 — is required to be a NaN (the real reductions return a canonical one).
"""
import ctypes
import os

import numpy as np
import pytest

from max_model import max_element
from scripted_item import identity_blob
from test_gpu_generic import ADD, INPUT, Item

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
NUMPY = {"f32": np.float32, "f64": np.float64, "c32": np.complex64, "c64": np.complex128}
COUNTS = {}                                               # reductions compared, per test: reported at the end


@pytest.fixture(scope="module", autouse=True)
def kernel_cache(tmp_path_factory):
    """One directory of compiled kernels for the module: the same item at another ensemble size is not built again."""
    before = os.environ.get("GFHIP_CACHE_DIR")
    os.environ["GFHIP_CACHE_DIR"] = str(tmp_path_factory.mktemp("kernels"))
    yield
    if before is None:
        del os.environ["GFHIP_CACHE_DIR"]
    else:
        os.environ["GFHIP_CACHE_DIR"] = before
    print("\nreductions compared:", COUNTS)


def same_real(got, values, note):
    """`got` (the double the C ABI returns) is values[max_element(values)]."""
    COUNTS[note[0]] = COUNTS.get(note[0], 0) + 1
    want = values[max_element(values)]
    if np.isnan(want):
        assert np.isnan(got), (note, got)
    elif want == 0:
        assert got == 0, (note, got)
    else:
        assert values.dtype.type(got).tobytes() == want.tobytes() and float(want) == got, (note, got, want)


def nan_with(dtype, negative, payload=1):
    """A quiet NaN with a payload and, if asked, the sign bit."""
    if dtype == np.float32:
        return np.array([0x7FC00000 | payload | (0x80000000 if negative else 0)], dtype=np.uint32).view(np.float32)[0]
    return np.array([0x7FF8000000000000 | payload | (0x8000000000000000 if negative else 0)], dtype=np.uint64).view(np.float64)[0]


def structural_places(n, head, grid_pairs):
    """Where a maximum could go missing in max_reduce_kernel: `head` elements in front of the first 16-byte boundary
    (one lane each in block 0), then pairs, pair t to thread t of the grid, then an odd tail element."""
    pairs = (n - head)//2
    places = {0, head - 1, head, head + 1, n - 1}
    if pairs:
        places |= {head + 2*(pairs - 1), head + 2*(pairs - 1) + 1}
    for thread in (63, 64, 255, 256):                     # lanes 63 | 64 of a block, thread 255 | the next block
        places |= {head + 2*thread, head + 2*thread + 1}
    places |= {head + 2*grid_pairs, head + 2*grid_pairs + 1}          # the first pair of the second stride trip
    places |= {head + 4*grid_pairs, head + 4*grid_pairs + 1}          # ... and of the third
    return sorted(p for p in places if 0 <= p < n)


def real_sizes(cus):
    whole = 2*256*cus                                      # the elements one trip of the capped grid covers
    return [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1025,
            whole - 1, whole, whole + 1, whole + 513, 3*whole + 7]


@pytest.mark.parametrize("dtype,offset", [("f32", 0), ("f32", 1), ("f32", 2), ("f32", 3), ("f64", 0), ("f64", 1)])
def test_separate_reduction_on_planted_data(dtype, offset):
    """max_reduce_kernel through gfhip_reduce_max on tensors that start `offset` elements past a 16-byte boundary."""
    import torch
    from graph_framework_amd import Context
    from graph_framework_amd.backend import key_of
    kind = NUMPY[dtype]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_line = 16//np.dtype(kind).itemsize
    head_of = (per_line - offset) % per_line
    rng = np.random.default_rng(100*offset + per_line)
    sizes = real_sizes(cus)
    storage = torch.zeros(max(sizes) + per_line, dtype={"f32": torch.float32, "f64": torch.float64}[dtype], device="cuda")
    assert storage.data_ptr() % 16 == 0
    context = Context(0)
    value = (ctypes.c_double*2)()
    note = "separate %s+%d" % (dtype, offset)

    def reduce(key):
        torch.cuda.synchronize()
        context._check(context.lib.gfhip_reduce_max(context.handle, key_of(key), value))
        return value[0]

    def put(view, values, places=None):
        if places is None:
            view.copy_(torch.from_numpy(values))
        else:
            for place in places:
                view[place:place + 1].copy_(torch.from_numpy(values[place:place + 1]))

    special = {5, 257, 1025, sizes[-2]}                    # the sizes that also get the value cases
    for n in sizes:
        view = storage[offset:offset + n]
        assert view.data_ptr() % 16 == offset*np.dtype(kind).itemsize
        key = "n%d" % n
        context.set_buffer(key, view)
        head = min(head_of, n)
        pairs = (n - head)//2
        grid_pairs = 256*min(max((pairs + 255)//256, 1), cus)
        places = structural_places(n, head, grid_pairs)
        if n > 2*grid_pairs + head:
            assert head + 2*grid_pairs in places           # the stride loop's second trip is met
        background = rng.uniform(-1000.0, -1.0, n).astype(kind)
        put(view, background)
        same_real(reduce(key), background, (note, n, "background"))
        planted = places + [int(p) for p in rng.integers(0, n, 3)]
        for place in planted:                              # a unique maximum, negative like everything else
            values = background.copy()
            values[place] = -0.5
            put(view, values, [place])
            assert max_element(values) == place
            same_real(reduce(key), values, (note, n, "unique", place))
            put(view, background, [place])
        if n not in special:
            continue
        tiny, big = np.finfo(kind).smallest_subnormal, np.finfo(kind).max
        cases = [("all -inf", np.full(n, -INF, dtype=kind)), ("all -max", np.full(n, -big, dtype=kind)),
                 ("subnormals", (rng.integers(-9, 10, n)*tiny).astype(kind)),
                 ("negative subnormals", (rng.integers(-9, 0, n)*tiny).astype(kind))]
        zeros = np.full(n, -1.0, dtype=kind)
        zeros[0], zeros[-1] = -0.0, 0.0
        cases += [("-0 ... +0", zeros), ("+0 ... -0", zeros[::-1].copy()), ("all -0", np.full(n, -0.0, dtype=kind))]
        for place in places:
            values = background.copy()
            values[place] = INF
            cases.append(("+inf@%d" % place, values))
            for negative in (False, True):
                values = background.copy()
                values[place] = nan_with(kind, negative)   # taken at 0, skipped elsewhere
                cases.append(("%snan@%d" % ("-" if negative else "", place), values))
            values = background.copy()
            values[[place, places[-1 - places.index(place)]]] = 7.5       # a tie of the maximum at two places
            cases.append(("tie@%d" % place, values))
        values = np.full(n, NAN, dtype=kind)
        cases.append(("all nan", values))
        values = background.copy()
        values[1:] = NAN                                   # every comparison false: element 0 stays
        cases.append(("nan but the first", values))
        for name, values in cases:
            put(view, values)
            same_real(reduce(key), values, (note, n, name))
    context.close()


def test_signed_zeros_return_a_zero():
    """[-0.0, ..., +0.0] and its reverse: std::max_element returns element 0 of each (-0 of the first, +0 of the second);
    the device returns a zero for both, and which one is not pinned."""
    import torch
    from graph_framework_amd import Context
    from graph_framework_amd.backend import key_of
    value = (ctypes.c_double*2)()
    context = Context(0)
    for n in (2, 3, 700):
        for kind, tensor_kind in ((np.float32, torch.float32), (np.float64, torch.float64)):
            for reverse in (False, True):
                values = np.full(n, -3.0, dtype=kind)
                values[0], values[-1] = (0.0, -0.0) if reverse else (-0.0, 0.0)
                assert max_element(values) == 0 and np.signbit(values[0]) == (not reverse)
                tensor = torch.from_numpy(values).cuda()
                key = "z%d%s%d" % (n, kind.__name__, reverse)
                context.set_buffer(key, tensor)
                torch.cuda.synchronize()
                context._check(context.lib.gfhip_reduce_max(context.handle, key_of(key), value))
                assert value[0] == 0.0 and not np.isnan(value[0]), (n, kind, reverse, value[0])
    context.close()


# ---------------------------------------------------------------------------------------------------------
#  max_modulus_kernel: one workgroup of 1024 threads, thread t scans t, t + 1024, ..., then a tree over LDS.

def same_complex(got, values, note):
    COUNTS[note[0]] = COUNTS.get(note[0], 0) + 1
    want = values[max_element(values)]
    for g, w in ((got.real, want.real), (got.imag, want.imag)):
        assert (np.isnan(g) and np.isnan(w)) or g == w, (note, got, want)


def separated(values, tied=()):
    """The condition on the inputs: apart from the places tied by symmetry, no modulus is within 1e-6 relative of
    the largest, so a last-bit difference between the device's hypot and numpy's cannot change the index."""
    with np.errstate(all="ignore"):
        moduli = np.abs(values.astype(np.complex128))
    best = max_element(values)
    if np.isnan(moduli[best]) or moduli[best] == 0:
        return
    others = np.delete(moduli, [best] + list(tied))
    others = others[~np.isnan(others)]
    if np.isinf(moduli[best]):
        assert not np.isinf(others).any()
    else:
        assert others.size == 0 or others.max() <= moduli[best]*(1.0 - 1.0e-6)


def complex_cases(kind, n, rng):
    """[(name, values, places tied with the selected one)]"""
    def background():
        angle, radius = rng.uniform(0, 2*np.pi, n), rng.uniform(1.0, 2.0, n)
        return (radius*np.exp(1j*angle)).astype(kind)
    out = []
    corners = sorted({p for p in (0, 1, 1023, 1024, 1025, 2047, 2048, n//2, n - 1) if p < n})
    for place in corners:
        values = background()
        values[place] = 3.0 - 4.0j
        out.append(("unique@%d" % place, values, []))
    a, b = 3.0, 4.0
    forms = [complex(a, b), complex(-a, b), complex(a, -b), complex(b, a), complex(-b, -a)]
    groups = [(5, 5 + 1024), (5 + 1024, 5 + 2048, 5), (1023, 1024), (200, 700), (700, 200, 1723), (0, n - 1), (n - 1, 1, 513)]
    for group in groups:                                   # the same thread's stride, neighbours, the halves of the tree
        if max(group) >= n or len(set(group)) < len(group):
            continue
        values = background()
        for place, form in zip(group, forms):
            values[place] = form
        first = min(group)
        out.append(("tie%s" % (group,), values, [p for p in group if p != first]))
    for place in corners:
        values = background()
        values[n//3] = 30.0 + 40.0j
        values[place] = complex(NAN, 2.5)                  # at 0: it stays; elsewhere: skipped
        out.append(("nan@%d" % place, values, []))
        values = background()
        values[place] = complex(INF, NAN)                  # modulus inf
        out.append(("(inf, nan)@%d" % place, values, []))
    values = np.full(n, complex(NAN, 1.0), dtype=kind)
    values[0] = complex(NAN, 7.0)
    out.append(("all nan", values, []))
    values = np.full(n, complex(1.0, NAN), dtype=kind)
    values[0] = 2.0 + 2.0j
    out.append(("nan but the first", values, []))
    big = float(np.finfo(kind).max)
    group = sorted({n//2, min(n//2 + 1024, n - 1), n - 1})
    values = background()
    for place, form in zip(group, (complex(big, big), complex(-big, 0.75*big), complex(INF, 0.0))):
        values[place] = form                               # overflowing moduli are inf and tie: the first wins
    out.append(("overflow", values, group[1:]))
    values = np.zeros(n, dtype=kind)
    values[0] = complex(-0.0, 0.0)
    values[n - 1] = complex(0.0, -0.0)
    out.append(("zeros", values, []))
    return out


@pytest.mark.parametrize("dtype", ["c32", "c64"])
def test_complex_reduction_on_planted_data(dtype):
    """max_modulus_kernel through gfhip_reduce_max on the input buffer of a trivial complex item, and once per case
    class through run_max_complex on its output (the input plus zero)."""
    from graph_framework_amd import Context
    from graph_framework_amd.backend import key_of
    kind = NUMPY[dtype]
    it = Item(dtype, False, ["z"], name="same")
    blob = it.blob([it.emit(ADD, it.emit(INPUT, a=0), it.constant(0.0))], [])
    rng = np.random.default_rng(29)
    value = (ctypes.c_double*2)()
    for n in (1, 2, 1023, 1024, 1025, 2047, 2049, 5000):
        context = Context(0)
        kernel = context.add_kernel(blob, n)
        context.compile()
        kernel.create_kernel_call(["z"], ["out"], [np.zeros(n, dtype=kind)])
        through_the_item = set()
        for name, values, tied in complex_cases(kind, n, rng):
            separated(values, tied)
            context.copy_to_device("z", values)
            context._check(context.lib.gfhip_reduce_max(context.handle, key_of("z"), value))
            same_complex(complex(value[0], value[1]), values, ("modulus " + dtype, n, name))
            family = name.split("@")[0].split("(")[0]
            if family not in through_the_item or name == "nan@0":
                through_the_item.add(family)
                same_complex(kernel.run_max_complex(), values, ("run_max_complex " + dtype, n, name))
        context.close()


# ---------------------------------------------------------------------------------------------------------
#  The `_max` epilogue generated into an item's own launch.

@pytest.mark.parametrize("per_cu", [None, "1"], ids=["grid", "one workgroup per CU"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_max_epilogue_on_planted_data(monkeypatch, dtype, per_cu):
    """run_max of an item whose output is its input bit for bit (scripted_item.identity_blob; held to the oracle on
    the CPU in test_max_model.py): the maximum planted by lane, wave, block and stride trip of the item's own grid.
    The largest ensemble needs several workgroups per CU; with one workgroup per CU the stride loop takes several trips."""
    from graph_framework_amd import Context
    if per_cu:                                             # the grid capped at the CU count: the stride loop takes trips
        monkeypatch.setenv("GFHIP_GRID_PER_CU", per_cu)
    kind = NUMPY[dtype]
    blob = identity_blob(dtype)
    rng = np.random.default_rng(41)
    context = Context(0)
    probe = context.add_kernel(blob, 64)
    context.compile()
    block = int(probe.info().block_size)
    context.close()
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert block % 64 == 0 and block >= 64
    note = "epilogue " + dtype
    sizes = (1, 63, 64, 65, block - 1, block, block + 1, 2*block + 1, 5*block*cus + 77)
    for n in (sizes[-1], block*cus + 1, 2*block*cus + 65) if per_cu else sizes:
        context = Context(0)
        kernel = context.add_kernel(blob, n)
        context.compile()
        assert kernel.info().num_instructions < 1500      # it has a `_max` entry
        background = rng.uniform(-1000.0, -1.0, n).astype(kind)
        kernel.create_kernel_call(["a"], ["o"], [background])
        grid = int(kernel.info().grid_size)
        assert grid == cus if per_cu else grid*block >= n or grid > cus
        trip = grid*block if grid else 0
        places = {0, 1, 31, 32, 63, 64, 65, 127, 128, block - 1, block, block + 63, block + 64, 2*block - 1, 2*block,
                  trip - 1, trip, trip + 63, 2*trip, n - 65, n - 64, n - 2, n - 1}
        places = sorted(p for p in places if 0 <= p < n) + [int(p) for p in rng.integers(0, n, 3)]

        def run(values, name):
            context.copy_to_device("a", values)
            got = kernel.run_max()
            same_real(got, values, (note, n, name))
            out = context.copy_to_host("o", np.empty(n, dtype=kind))
            assert np.array_equal(out, values, equal_nan=True) and np.array_equal(np.signbit(out), np.signbit(values))

        run(background, "background")
        for place in places:
            values = background.copy()
            values[place] = -0.5
            run(values, "unique@%d" % place)
        for place in places[:12] + places[-5:]:
            values = background.copy()
            values[place] = NAN                            # taken at ray 0 only
            run(values, "nan@%d" % place)
        values = background.copy()
        values[0] = nan_with(kind, True)
        run(values, "-nan@0")
        values = background.copy()
        values[[places[len(places)//2], n - 1]] = 7.5
        run(values, "tie")
        run(np.full(n, -INF, dtype=kind), "all -inf")      # a lane past n that contributed anything would show here
        run(np.full(n, -np.finfo(kind).max, dtype=kind), "all -max")
        run((rng.integers(-9, 0, n)*np.finfo(kind).smallest_subnormal).astype(kind), "negative subnormals")
        zeros = np.full(n, -1.0, dtype=kind)
        zeros[0], zeros[-1] = -0.0, 0.0
        run(zeros, "-0 ... +0")
        run(zeros[::-1].copy(), "+0 ... -0")
        values = np.full(n, NAN, dtype=kind)
        run(values, "all nan")
        context.close()
