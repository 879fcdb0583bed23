"""gfhip_hand_over on the device (include/gf_hip.h, csrc/hand_over.hip): arrays from one context's buffers to another's,
bit for bit.

Everything is compared as unsigned integers of the element's width: the kernel moves words, so there is no tolerance.
The planted values are the ones arithmetic would change: quiet and signalling NaNs with payloads, both zeros, both
infinities, the smallest subnormal.  Sizes 1, 63, 64, 65, 257 and 1000 cover a lone element, the wavefront's edges, a
second workgroup and every tail of the 16-byte path (1000 f32 widening pairs leave none, 257 leaves one, 63 complex
parts leave three).
"""
import numpy as np
import pytest

import conftest  # noqa: F401
from test_gpu_generic import ADD, INPUT, Item

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 1000)
REAL = {"f64": np.float64, "f32": np.float32}
COMPLEX = {"f64": np.complex128, "f32": np.complex64}
WORD = {"f64": np.uint64, "f32": np.uint32}
GFIR = {np.float32: 0, np.float64: 1, np.complex64: 2, np.complex128: 3}
#  quiet NaN with a payload, signalling NaN with a payload, negative quiet NaN, -0, +0, +inf, -inf, smallest subnormal,
#  largest subnormal, 1.0, an ordinary value
SPECIAL = {"f64": [0x7FF8000000ABCDEF, 0x7FF0000000000123, 0xFFF8DEADBEEF0001, 0x8000000000000000, 0, 0x7FF0000000000000,
                   0xFFF0000000000000, 1, 0x000FFFFFFFFFFFFF, 0x3FF0000000000000, 0xC05EDD2F1A9FBE77],
           "f32": [0x7FC0ABCD, 0x7F800123, 0xFFC1BEEF, 0x80000000, 0, 0x7F800000, 0xFF800000, 1, 0x007FFFFF, 0x3F800000, 0xC2F6E979]}


def words(base, count, seed):
    """`count` words of the base type: the special patterns first, in an order that depends on the seed, then random bits."""
    rng = np.random.default_rng(seed)
    special = np.array(SPECIAL[base], dtype=WORD[base])
    out = rng.integers(0, np.iinfo(WORD[base]).max, count, dtype=WORD[base], endpoint=True)
    head = rng.permutation(special)[:count]
    out[:head.size] = head
    return out


def planted(base, kind, count, seed):
    """An array of `count` elements (kind: "real" or "complex") whose words are words()."""
    if kind == "real":
        return words(base, count, seed).view(REAL[base])
    return words(base, 2*count, seed).view(COMPLEX[base])


def bits(array):
    """The array as unsigned words of its base type's width (a complex element is two)."""
    array = np.ascontiguousarray(array)
    return array.view(np.uint64 if array.dtype in (np.float64, np.complex128) else np.uint32)


def allocate(context, key, values):
    from graph_framework_amd.backend import key_of
    values = np.ascontiguousarray(values)
    context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), values.size, GFIR[values.dtype.type]))
    if values.size:
        context.copy_to_device(key, values)


def fetch(context, key):
    count, dtype = context.buffer_info(key)
    return context.copy_to_host(key, np.empty(count, dtype=dtype))


def expected_bits(source, to_kind, part=0):
    """What the destination holds, as words: the host statement of the conversions."""
    raw = bits(source)
    if np.iscomplexobj(source) == (to_kind == "complex"):
        return raw
    if to_kind == "complex":
        out = np.zeros(2*raw.size, dtype=raw.dtype)                  # +0.0 imaginary parts: all bits clear
        out[0::2] = raw
        return out
    return raw[part::2]


@pytest.fixture(scope="module")
def contexts():
    from graph_framework_amd import Context
    pair = Context(0), Context(0)                                   # private streams: the events are in play
    yield pair
    for context in pair:
        context.close()


CONVERSIONS = [("real", "real", 0), ("complex", "complex", 0), ("real", "complex", 0), ("complex", "real", 0), ("complex", "real", 1)]


@pytest.mark.parametrize("base", ["f64", "f32"])
def test_every_legal_conversion(contexts, base):
    to, source = contexts
    entries, want = [], {}
    for count in SIZES:
        for number, (from_kind, to_kind, part) in enumerate(CONVERSIONS):
            name = "%s_%d_%d" % (base, count, number)
            values = planted(base, from_kind, count, 100*count + number)
            allocate(source, "from_" + name, values)
            sentinel = planted(base, to_kind, count, 7)
            allocate(to, "to_" + name, sentinel)
            entries.append(("to_" + name, "from_" + name, part))
            want[name] = (values, expected_bits(values, to_kind, part))
    assert len(entries) == 30
    to.hand_over(source, entries)                                    # two launches: the table holds 16
    for name, (values, expected) in want.items():
        got = bits(fetch(to, "to_" + name))
        assert np.array_equal(got, expected), name
        assert np.array_equal(bits(fetch(source, "from_" + name)), bits(values)), name      # the source is only read
    widened = bits(fetch(to, "to_%s_1000_2" % base))
    assert not widened[1::2].any() and widened[0::2].any()


def test_zero_elements_take_no_launch(contexts):
    to, source = contexts
    allocate(source, "empty_from", np.zeros(0))
    allocate(to, "empty_to", np.zeros(0, dtype=np.complex128))
    to.hand_over(source, [("empty_to", "empty_from")])
    to.hand_over(source, [])


def adopt(context, key, tensor):
    context.set_buffer(key, tensor)


@pytest.mark.parametrize("shift", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["aligned", "to_off", "from_off", "both_off"])
@pytest.mark.parametrize("base", ["f64", "f32"])
def test_guard_elements_around_adopted_slices(base, shift):
    """Destinations and sources are slices of larger torch tensors; the elements on both sides of every destination keep
    their planted bits.  shift = (1, *) starts the destination slice, (*, 1) the source slice, one element past a
    16-byte boundary: aligned for its elements, not for 16-byte accesses."""
    import torch
    from graph_framework_amd import Context
    to, source = Context(0), Context(0)
    device = torch.device("cuda", 0)
    guard = 8
    cases = []
    for count in SIZES:
        for number, (from_kind, to_kind, part) in enumerate(CONVERSIONS):
            values = planted(base, from_kind, count + 2*guard + 1, 31*count + number)
            whole_from = torch.from_numpy(values.copy()).to(device)
            whole_to_host = planted(base, to_kind, count + 2*guard + 1, 17*count + number)
            whole_to = torch.from_numpy(whole_to_host.copy()).to(device)
#  torch allocations are at least 256-byte aligned; a real slice that starts at an even element (f64) or a multiple of
#  four (f32) and a complex slice at an even element (c32) keep 16 bytes, one element further loses them
            first_to, first_from = guard + shift[0], guard + shift[1]
            assert whole_to.data_ptr() % 16 == 0 and whole_from.data_ptr() % 16 == 0
            name = "%d_%d" % (count, number)
            adopt(to, "to_" + name, whole_to[first_to:first_to + count])
            adopt(source, "from_" + name, whole_from[first_from:first_from + count])
            for tensor, first, off in ((whole_to, first_to, shift[0]), (whole_from, first_from, shift[1])):
                assert (tensor[first:].data_ptr() % 16 != 0) == bool(off) or tensor.element_size() == 16
            cases.append((name, part, values[first_from:first_from + count], to_kind, whole_to, whole_to_host, first_to, count))
    torch.cuda.synchronize()
    to.hand_over(source, [("to_" + name, "from_" + name, part) for name, part, *_ in cases])
    to.wait()
    for name, part, values, to_kind, whole_to, before, first, count in cases:
        after = whole_to.cpu().numpy()
        per = 2 if to_kind == "complex" else 1
        got, planted_bits = bits(after), bits(before)
        assert np.array_equal(got[per*first:per*(first + count)], expected_bits(values, to_kind, part)), name
        assert np.array_equal(got[:per*first], planted_bits[:per*first]), name + ": the guard below"
        assert np.array_equal(got[per*(first + count):], planted_bits[per*(first + count):]), name + ": the guard above"
    to.close()
    source.close()


def test_seventeen_entries_in_one_call(contexts):
    to, source = contexts
    entries, want = [], []
    for number in range(17):
        values = planted("f64", "real", 300 + number, number)
        allocate(source, "many_from_%d" % number, values)
        allocate(to, "many_to_%d" % number, np.zeros(values.size, dtype=np.complex128))
        entries.append(("many_to_%d" % number, "many_from_%d" % number))
        want.append(expected_bits(values, "complex"))
    to.hand_over(source, entries)
    for number, expected in enumerate(want):
        assert np.array_equal(bits(fetch(to, "many_to_%d" % number)), expected), number


def test_within_one_context(contexts):
    context = contexts[0]
    values = planted("f64", "real", 1000, 3)
    allocate(context, "x", values)
    allocate(context, "x_last", np.zeros(1000))
    allocate(context, "x_wide", np.ones(1000, dtype=np.complex128))
    context.hand_over(context, [("x_last", "x"), ("x_wide", "x"), ("x", "x")])
    assert np.array_equal(bits(fetch(context, "x_last")), bits(values))
    assert np.array_equal(bits(fetch(context, "x_wide")), expected_bits(values, "complex"))
    assert np.array_equal(bits(fetch(context, "x")), bits(values))


def test_two_contexts_on_private_streams():
    """A source item advances `a` (fp64), the hand-over widens it into the other context's `z`, an item there adds z to
    `acc` (complex): 40 rounds with nothing waiting in between, so that only the stream order gfhip_hand_over sets up
    keeps a round's kernels apart.  Every value is a small integer: the host model is exact."""
    from graph_framework_amd import Context
    rays = 300001
    advance = Item("f64", False, ["a", "s"], name="advance")
    advance_blob = advance.blob([], [(advance.emit(ADD, advance.emit(INPUT, a=0), advance.emit(INPUT, a=1)), 0)])
    gather = Item("c64", False, ["acc", "z"], name="accumulate")
    gather_blob = gather.blob([], [(gather.emit(ADD, gather.emit(INPUT, a=0), gather.emit(INPUT, a=1)), 0)])
    source, to = Context(0), Context(0)
    first = source.add_kernel(advance_blob, rays)
    second = to.add_kernel(gather_blob, rays)
    source.compile()
    to.compile()
    a = np.arange(rays, dtype=np.float64) % 1000
    s = 1.0 + np.arange(rays, dtype=np.float64) % 7
    first.create_kernel_call(["a", "s"], [], [a, s])
    second.create_kernel_call(["acc", "z"], [], [np.zeros(rays, dtype=np.complex128), np.zeros(rays, dtype=np.complex128)])
    acc = np.zeros(rays, dtype=np.complex128)
    snapshots = []
    for round_number in range(40):
        first.run()
        to.hand_over(source, [("z", "a")])
        second.run()
        a = a + s
        acc = acc + a
        if round_number % 13 == 5:                                   # a few rounds are looked at, most are not waited for
            to.wait()
            snapshots.append((round_number, fetch(to, "acc"), acc.copy()))
    to.wait()
    got = fetch(to, "acc")
    got_a = fetch(source, "a")
    source.close()
    to.close()
    for round_number, seen, model in snapshots:
        assert np.array_equal(bits(seen), bits(model)), round_number
    assert np.array_equal(bits(got), bits(acc))
    assert np.array_equal(bits(got_a), bits(a))


def test_every_refusal_leaves_a_message_and_the_destination(contexts):
    from graph_framework_amd import _lib
    from graph_framework_amd.backend import GfHipError, key_of
    to, source = contexts
    lib = to.lib
    n = 65
    f64 = planted("f64", "real", n, 1)
    allocate(source, "r_f64", f64)
    allocate(source, "r_f32", planted("f32", "real", n, 2))
    allocate(source, "r_c64", planted("f64", "complex", n, 3))
    allocate(source, "r_short", planted("f64", "real", n - 1, 4))
    kept = {}
    for key, values in (("d_f64", planted("f64", "real", n, 5)), ("d_c64", planted("f64", "complex", n, 6)),
                        ("d_c32", planted("f32", "complex", n, 7)), ("d_f32", planted("f32", "real", n, 8))):
        allocate(to, key, values)
        kept[key] = bits(values)
    good = ("d_f64", "r_f64")
    refusals = {
        "precision f64 -> f32": [("d_f32", "r_f64")],
        "precision f32 -> f64": [("d_f64", "r_f32")],
        "precision f64 -> c32": [("d_c32", "r_f64")],
        "precision c64 -> f32": [("d_f32", "r_c64")],
        "part > 1": [("d_f64", "r_c64", 2)],
        "part = 1 of a real source": [("d_f64", "r_f64", 1)],
        "part = 1 into a complex destination": [("d_c64", "r_c64", 1)],
        "unknown source key": [("d_f64", "nobody")],
        "unknown destination key": [("nobody", "r_f64")],
        "unequal element counts": [("d_f64", "r_short")],
    }
    for note, bad in refusals.items():
        for entries in (bad, [good] + bad, bad + [good]):           # a legal entry next to it is not launched either
            with pytest.raises(GfHipError) as raised:
                to.hand_over(source, entries)
            assert "gfhip_hand_over" in str(raised.value), note
            assert lib.gfhip_last_error(source.handle), note
    entry = (_lib.HandOverEntry*2)()
    entry[0].to_key, entry[0].from_key = key_of("d_f64"), key_of("r_f64")
    entry[1].to_key, entry[1].from_key, entry[1].reserved = key_of("d_f64"), key_of("r_f64"), 1
    for arguments, context in (((to.handle, source.handle, entry, 2), to),          # reserved != 0
                               ((to.handle, source.handle, None, 1), to),           # null entries, count > 0
                               ((None, source.handle, entry, 1), source), ((to.handle, None, entry, 1), to)):
        assert lib.gfhip_hand_over(*arguments) != 0
        assert b"gfhip_hand_over" in lib.gfhip_last_error(context.handle)
    assert lib.gfhip_hand_over(None, None, entry, 1) != 0 and b"gfhip_hand_over" in lib.gfhip_last_error(None)
    import torch
    if torch.cuda.device_count() > 1:                                # contexts on different devices
        from graph_framework_amd import Context
        other = Context(1)
        allocate(other, "r_f64", f64)
        with pytest.raises(GfHipError, match="different devices"):
            to.hand_over(other, [good])
        other.close()
    for key, before in kept.items():
        assert np.array_equal(bits(fetch(to, key)), before), key
    assert np.array_equal(bits(fetch(source, "r_f64")), bits(f64))
    to.hand_over(source, [good])                                     # and the legal entry alone does move
    assert np.array_equal(bits(fetch(to, "d_f64")), bits(f64))
