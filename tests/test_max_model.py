"""tests/max_model.py — the model the GPU reductions and converge loops are held to — pinned on cases
small enough to work by hand, and oracle/gfir.py's Item.converge held to it.  No GPU."""
import numpy as np
import pytest

from max_model import converge, max_element, scripted

NAN, INF = float("nan"), float("inf")
REAL = [np.float32, np.float64]
COMPLEX = [np.complex64, np.complex128]


def plant(size, background, places, value, dtype):
    """`background` everywhere, `value` at `places` (an empty list: no maximum planted, no ties)."""
    values = np.full(size, background, dtype=dtype)
    for place in places:
        values[place] = value
    return values


@pytest.mark.parametrize("dtype", REAL)
def test_real_max_element_by_hand(dtype):
    def at(values):
        return max_element(np.array(values, dtype=dtype))
    assert at([1.0]) == 0
    assert at([1.0, 2.0, 3.0]) == 2 and at([3.0, 2.0, 1.0]) == 0 and at([1.0, 3.0, 2.0]) == 1
    assert at([2.0, 5.0, 5.0, 1.0, 5.0]) == 1                       # the first of equals
    assert at([-3.0, -3.0]) == 0
    assert at([-0.0, 0.0]) == 0 and at([0.0, -0.0]) == 0            # -0 < +0 is false either way
    assert at([-1.0, -0.0, 0.0]) == 1 and at([-1.0, 0.0, -0.0]) == 1
    assert at([NAN, 7.0, 9.0]) == 0                                 # every `NaN < x` is false
    assert at([7.0, NAN, 9.0]) == 2 and at([9.0, NAN, 7.0]) == 0    # `m < NaN` is false
    assert at([7.0, 9.0, NAN]) == 1
    assert at([NAN, NAN]) == 0 and at([1.0, NAN, NAN]) == 0
    assert at([-INF, -INF, -INF]) == 0 and at([-INF, NAN, -INF]) == 0
    assert at([-INF, NAN, -5.0]) == 2
    assert at([1.0, INF, INF]) == 1
    tiny = np.finfo(dtype).smallest_subnormal
    assert at([-tiny, 0.0, tiny, tiny]) == 2
    assert at([]) == 0                                              # an empty range: its end
    assert max_element(plant(9, -2.0, [], 5.0, dtype)) == 0         # an empty tie list: all equal, element 0
    assert max_element(plant(9, -2.0, [4], 5.0, dtype)) == 4
    assert max_element(plant(9, -2.0, [7, 3], 5.0, dtype)) == 3


@pytest.mark.parametrize("dtype", COMPLEX)
def test_complex_max_element_by_hand(dtype):
    def at(values):
        return max_element(np.array(values, dtype=dtype))
    assert at([1 + 1j, 3 - 4j, 0.5j]) == 1                          # moduli sqrt 2, 5, 0.5
    assert at([3 + 4j, -3 + 4j, 3 - 4j, 4 + 3j, -5.0, 5j]) == 0     # all of modulus exactly 5: the first
    assert at([1.0, 4 + 3j, 3 + 4j]) == 1
    assert at([0j, -0.0 + 0j, complex(0.0, -0.0)]) == 0             # all of modulus 0
    assert at([complex(-0.0, -0.0), 0j]) == 0
    assert at([complex(NAN, 0), 100.0, 2.0]) == 0                   # a NaN modulus first: it stays
    assert at([complex(0, NAN), 100.0]) == 0
    assert at([1.0, complex(NAN, 0), 100.0]) == 2 and at([100.0, complex(NAN, NAN), 1.0]) == 0
    assert at([1.0, 100.0, complex(0, NAN)]) == 1
    assert at([complex(NAN, NAN), complex(NAN, 1)]) == 0
    assert at([1.0, complex(INF, NAN), 1.0e30]) == 1                # |(inf, nan)| is inf
    assert at([complex(INF, NAN), complex(NAN, 0)]) == 0
    assert at([1.0, complex(0, -INF), complex(INF, NAN)]) == 1      # inf ties with inf: the first
    big = np.finfo(dtype).max
    assert at([1.0, complex(big, big), complex(-big, big), INF]) == 1    # overflowing moduli are inf and tie
    assert at([]) == 0


def test_large_arrays_follow_the_serial_scan():
    """The vectorised rule against the scan itself, written out, on arrays with ties, zeros and NaNs."""
    rng = np.random.default_rng(5)
    for trial in range(60):
        size = int(rng.integers(1, 40))
        values = rng.integers(-2, 3, size).astype(np.float64)
        values[rng.random(size) < 0.2] = NAN
        values[rng.random(size) < 0.2] = -0.0
        if trial % 2:
            values = values*(1 + 0j) if trial % 4 == 1 else values*1j
        key = np.abs(values) if np.iscomplexobj(values) else values
        best = 0
        for i in range(1, size):
            if key[best] < key[i]:
                best = i
        assert max_element(values) == best, values
    wide = np.full(300000, -1.0)
    wide[[123456, 250000]] = 4.0
    assert max_element(wide) == 123456


@pytest.mark.parametrize("dtype", REAL + COMPLEX)
def test_every_exit_of_the_loop_by_hand(dtype):
    def run(script, tolerance, limit):
        iterations, last, passes = converge(scripted(script, dtype), dtype, tolerance, limit)
        assert type(last) is dtype
        return iterations, last, passes
#  |max| <= tol on the third pass: two iterations were counted before it
    assert run([8.0, 4.0, 0.5, 99.0], 1.0, 100) == (2, 0.5, 3)
#  ... on the very first pass
    assert run([0.5, 99.0], 1.0, 100) == (0, 0.5, 1)
#  |max| == tol is not `>`
    assert run([8.0, 1.0, 99.0], 1.0, 100) == (1, 1.0, 2)
#  a constant sequence: pass 2 equals `last`
    assert run([8.0, 5.0, 5.0, 99.0], 0.25, 100) == (2, 5.0, 3)
#  period 2: 8 3 8 3.  After pass 1 iterations is 1 (odd: off_last untouched), after pass 2 iterations is 2 and
#  off_last = 3... by hand: i=0, m=8 -> go, i=1, last=8; m=3 -> go, i=2, last=3, off=3; m=8: |3-8| and |3-8| -> go, i=3,
#  last=8; m=3: |8-3| > tol but |off_last - 3| = 0 -> stop.  Four passes, three iterations.
    assert run([8.0, 3.0, 8.0, 3.0, 8.0, 3.0], 0.25, 100) == (3, 3.0, 4)
#  the other parity: 9 first, then the same oscillation.  i=1 last=9; m=8: i=2 last=8 off=8; m=3: i=3 last=3; m=8:
#  |off_last - 8| = 0 -> stop.  Four passes again, the oscillation caught one pass younger.
    assert run([9.0, 8.0, 3.0, 8.0, 3.0, 8.0], 0.25, 100) == (3, 8.0, 4)
#  a NaN stops the loop: |NaN| > tol is false
    iterations, last, passes = run([8.0, 4.0, NAN, 1.0], 0.25, 100)
    assert (iterations, passes) == (2, 3) and np.isnan(last)
    iterations, last, passes = run([NAN, 1.0], 0.25, 100)
    assert (iterations, passes) == (0, 1) and np.isnan(last)
#  the limit: `iterations++ < limit` counts the failed test too
    falling = [64.0, 32.0, 16.0, 8.0, 4.0, 2.0]
    assert run(falling, 0.25, 0) == (1, 64.0, 1)
    assert run(falling, 0.25, 1) == (2, 32.0, 2)
    assert run(falling, 0.25, 2) == (3, 16.0, 3)
    assert run(falling, 0.25, 4) == (5, 4.0, 5)
#  a negative tolerance is its modulus
    assert run([8.0, 4.0, 0.5, 99.0], -1.0, 100) == (2, 0.5, 3)
#  an inf that later falls: |inf - max| is inf, the loop goes on
    assert run([INF, 7.0, 0.5], 1.0, 100) == (2, 0.5, 3)
#  inf twice: inf - inf is NaN, `NaN > tol` is false
    assert run([INF, INF, 0.5], 1.0, 100) == (1, INF, 2)


def test_starting_values_of_last():
    """last and off_last start at numeric_limits<T>::max(): the largest finite value for real types, T() = 0
    for complex ones — so a complex loop whose first maximum is within tol of 0... has left through clause
    one already, and one whose first maximum is the real type's largest value stops at once."""
    for dtype in REAL:
        big = np.finfo(dtype).max
        assert converge(scripted([big, 1.0], dtype), dtype, 0.5, 10) == (0, big, 1)
    for dtype in COMPLEX:
        big = np.finfo(dtype).max
        iterations, last, passes = converge(scripted([big, 3.0, 0.25], dtype), dtype, 0.5, 10)
        assert (iterations, last, passes) == (2, 0.25, 3)


def test_the_tolerance_is_narrowed_to_the_items_type():
    for dtype in (np.float32, np.complex64):
#  1e-50 is 0.0f: only an exact repeat (or an exact zero) stops the loop
        assert converge(scripted([4.0, 1.0e-40, 1.0e-44, 1.0e-44, 9.0], dtype), dtype, 1.0e-50, 100)[::2] == (3, 4)
        assert converge(scripted([4.0, 0.0, 9.0], dtype), dtype, 1.0e-50, 100)[::2] == (1, 2)
#  in double 1e-50 is a number and 1e-60 is below it
    assert converge(scripted([4.0, 1.0e-60, 9.0], np.float64), np.float64, 1.0e-50, 100)[::2] == (1, 2)


def test_fp32_compares_in_float():
    """Where the loop in `float` and the loop in `double` part.

    The subtraction itself cannot be the place: the loop reaches `|last - max| > tol` only with |last| > tol and
    |max| > tol, and two floats of one sign that both exceed tol and differ by about tol lie within a factor two
    of each other, so their difference is exact in float (Sterbenz) as it is in double.  What differs is the
    tolerance the difference is compared with: the reference narrows it to float first.  With u = 2^-27:

        tolerance 0.1          as a float 13421773 u  (0.100000001490116...), above the double 0.1
        pass 0:   26843548 u   (0.2000000179...; 13421774 * 2^-26, a float)
        pass 1:   13421775 u   (0.1000000163...; a float)

    Pass 1 in float:  |max| = 13421775 u > 13421773 u, go on;  |last - max| = 13421773 u exactly, which is not
    greater than the float tolerance: stop, 1 iteration, 2 passes.
    Pass 1 with the tolerance left a double: 0.100000001490116 > 0.1: the loop goes on to pass 2.
    """
    u = 2.0**-27
    script = [26843548*u, 13421775*u, 0.05, 99.0]
    as_float = np.array(script, dtype=np.float32)
    assert [float(v) for v in as_float[:2]] == script[:2]               # both are floats
    assert float(np.float32(0.1)) == 13421773*u
    assert float(as_float[0] - as_float[1]) == 13421773*u
    iterations, last, passes = converge(scripted(script, np.float32), np.float32, 0.1, 100)
    assert (iterations, float(last), passes) == (1, 13421775*u, 2)
    iterations, last, passes = converge(scripted(script, np.float64), np.float64, 0.1, 100)
    assert (iterations, float(last), passes) == (2, 0.05, 3)


# ---------------------------------------------------------------------------------------------------------
#  oracle/gfir.py's Item.converge is the same loop on the same selection.

DTYPES = {"f32": 0, "f64": 1, "c32": 2, "c64": 3}
NUMPY = {"f32": np.float32, "f64": np.float64, "c32": np.complex64, "c64": np.complex128}


def test_the_oracle_selects_as_the_model():
    from oracle import gfir
    rng = np.random.default_rng(17)
    for trial in range(200):
        size = int(rng.integers(1, 12))
        values = rng.integers(-2, 3, size).astype(np.float64)
        values[rng.random(size) < 0.25] = NAN
        values[rng.random(size) < 0.2] = -0.0
        for kind in (np.float32, np.float64, np.complex64, np.complex128):
            array = (values*(1j if trial % 2 else 1)).astype(kind) if np.iscomplexobj(kind(0)) else values.astype(kind)
            assert gfir.max_element(array) == max_element(array)
    assert gfir.max_element(np.array([1.0, complex(NAN, 0), 3.0])) == 2     # not np.argmax's first NaN
    assert gfir.max_element(np.array([-0.0, 0.0])) == 0


@pytest.mark.parametrize("dtype", ["f32", "f64", "c32", "c64"])
def test_the_oracle_converges_as_the_model(dtype):
    """Item.converge on the scripted item of tests/scripted_item.py: every pass reads its script element (so the
    index arithmetic c + base is settled), the loop leaves where the model leaves, and the pass counter says how
    often the kernel ran."""
    from oracle import gfir
    import scripted_item
    kind = NUMPY[dtype]
    item = gfir.Item(scripted_item.blob(dtype))
    for name, classes, tolerance, limit in scripted_item.ensembles(dtype):
        for rays in (1, 7):
            columns, per_ray = scripted_item.columns(dtype, classes, rays)
            iterations, last, outs = item.converge(columns, tolerance, limit)
            maxima = scripted_item.maxima(dtype, classes, per_ray)
            want_iterations, want_last, passes = converge(scripted(maxima, kind), kind, tolerance, limit)
            assert iterations == want_iterations, (name, rays)
            assert last == want_last or (np.isnan(last) and np.isnan(want_last)), (name, rays)
            assert np.array_equal(columns[0], np.full(rays, passes, dtype=kind)), (name, rays)
            final = scripted_item.outputs(dtype, classes, per_ray, passes - 1)
            assert np.array_equal(outs[-1], final, equal_nan=True), (name, rays)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_identity_item_keeps_every_bit(dtype):
    """scripted_item.identity_blob, the item the `_max` epilogue is tested on: its output is its input, signed zeros,
    infinities, subnormals and NaNs included."""
    from oracle import gfir
    import scripted_item
    kind = NUMPY[dtype]
    tiny = np.finfo(kind).smallest_subnormal
    values = np.array([0.0, -0.0, 1.5, -2.5, INF, -INF, NAN, tiny, -tiny, np.finfo(kind).max, -np.finfo(kind).max], dtype=kind)
    outs, _ = gfir.Item(scripted_item.identity_blob(dtype)).run([values.copy()])
    assert np.array_equal(outs[0], values, equal_nan=True)
    assert np.array_equal(np.signbit(outs[0]), np.signbit(values))
