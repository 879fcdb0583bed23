"""What a converge item means, as a model in plain numpy: which element `std::max_element` selects, and
when the loop that tests that element stops.

Real types compare with `<`, complex types with `abs(a) < abs(b)` in their base precision.  The scan
starts at element 0 and a later element replaces the current one only if `current < later` is true,
so the first of equals wins, +0 and -0 are equal, and a NaN — for which every comparison is false — is
selected only at element 0, where it then stays whatever follows.

The loop is

    max = max_kernel()
    while (|max| > |tol| && |last - max| > |tol| && |off_last - max| > |tol| && iterations++ < limit) {
        last = max;  if (!(iterations % 2)) off_last = max;  max = max_kernel();
    }

with every value and every operation in the item's own type.  Test infrastructure only.
"""
import numpy as np


def modulus(values):
    """The key `max_element` compares: the value itself, or abs in the base precision for complex types."""
    values = np.asarray(values)
    if np.iscomplexobj(values):
        with np.errstate(all="ignore"):
            return np.abs(values)
    return values


def max_element(values):
    """Index that std::max_element returns (0 for an empty range: its end)."""
    key = modulus(values).ravel()
    if key.size == 0 or np.isnan(key[0]):
        return 0
#  From here on the current maximum is never a NaN and no NaN replaces it (`m < NaN` is false), so the
#  NaNs may be given any value that never wins; argmax returns the first of equal maxima (-0 == +0).
    return int(np.argmax(np.where(np.isnan(key), -np.inf, key)))


def converge(max_kernel, dtype, tolerance, limit):
    """The loop on the values `max_kernel()` returns one per call.  Returns (iterations, last max as a
    `dtype` scalar, number of calls = passes run).  A loop that runs out of iterations returns limit + 1."""
    dtype = np.dtype(dtype).type
    is_complex = issubclass(dtype, np.complexfloating)
    with np.errstate(all="ignore"):
        tol = abs(dtype(tolerance))                  # narrowed to the item's type first
        big = dtype(0) if is_complex else dtype(np.finfo(dtype).max)   # numeric_limits<complex<B>>::max() is T()
        last = off_last = big
        iterations = 0
        maximum = dtype(max_kernel())
        passes = 1
        while abs(maximum) > tol and abs(dtype(last - maximum)) > tol and abs(dtype(off_last - maximum)) > tol:
            took = iterations < limit                # iterations++ < limit
            iterations += 1
            if not took:
                break
            last = maximum
            if not iterations % 2:
                off_last = maximum
            maximum = dtype(max_kernel())
            passes += 1
    return iterations, maximum, passes


def scripted(script, dtype):
    """A max_kernel that returns script[0], script[1], ... in `dtype`."""
    values = iter(np.asarray(script, dtype=dtype))
    return lambda: next(values)
