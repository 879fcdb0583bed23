"""The model of the batches of rays (graph_framework_amd/batches.py, csrc/ray_batches.hpp): the batch of every sample
ray by ray, the rays of a batch by counting, the standard error in rational arithmetic with the square root taken last,
and a numpy tally for the statistics.  Nothing here is in closed form and nothing is shared with the code under test."""
import decimal
from fractions import Fraction

import numpy as np

DIGITS = 50


def batch_index(first, count, batches):
    """int64[count]: the batch of the samples of an add whose first sample is ray `first`."""
    rays = np.uint64(first) + np.arange(count, dtype=np.uint64)
    return ((rays >> np.uint64(6)) % np.uint64(batches)).astype(np.int64)


def batch_rays(first, count, batches):
    return np.bincount(batch_index(first, count, batches), minlength=batches).astype(np.int64)


def exact_standard_error(sums, total, rays, count):
    """(means, stderrs, used) of one cell's planted data, lists over nothing: sums[g] and total are doubles taken as the
    exact numbers they are, rays[g] and count integers.  mean a Fraction; stderr a Decimal of DIGITS digits, the square
    root taken last, or None with fewer than two batches that have rays."""
    pairs = [(Fraction(float(s)), int(n)) for s, n in zip(sums, rays) if int(n) > 0]
    mean = Fraction(float(total))/int(count)
    if len(pairs) < 2:
        return mean, None, len(pairs)
    variance = sum(n*(s/n - mean)**2 for s, n in pairs)/((len(pairs) - 1)*int(count))
    context = decimal.Context(prec=DIGITS + 10)
    root = context.sqrt(context.divide(decimal.Decimal(variance.numerator), decimal.Decimal(variance.denominator)))
    return mean, root, len(pairs)


def error_bound(sums, total, rays, count):
    """The bound on |fp64 stderr - exact stderr| of batches.standard_error_of for one cell, as a Fraction, from the
    roundings of its numpy expression (u = 2^-53, m batches with rays):
        p_g = S_g/n_g and P = S/N one rounding each, their difference a third: the computed deviation is off by at most
            delta_g = u (1 + u)(|p_g| + |P|) + u |d_g|;
        n d d two roundings, the sum of m terms of one sign at most m - 1 on any of them, (m - 1) N one, the quotient
            one: the radicand is sum n (d + eta)^2 times (1 + u)^(m + 3) at most; the root halves that and rounds once.
    With the triangle inequality of the n-weighted norm,
        |got - exact| <= gamma exact + (1 + gamma) sqrt(sum n delta_g^2/((m - 1) N)),  gamma = (1 + u)^((m + 5)/2) - 1,
    gamma and delta taken 1.0001 times their first order to cover the higher ones.  Roundings only: no operation
    under- or overflows."""
    u = Fraction(1, 2**53)
    slack = Fraction(10001, 10000)
    pairs = [(Fraction(float(s)), int(n)) for s, n in zip(sums, rays) if int(n) > 0]
    m = len(pairs)
    mean, exact, _ = exact_standard_error(sums, total, rays, count)
    deltas = [slack*u*(abs(s/n) + abs(mean) + abs(s/n - mean)) for s, n in pairs]
    carried = sum(n*d*d for (_, n), d in zip(pairs, deltas))/((m - 1)*int(count))
    context = decimal.Context(prec=DIGITS + 10)
    carried = context.sqrt(context.divide(decimal.Decimal(carried.numerator), decimal.Decimal(carried.denominator)))
    gamma = slack*u*Fraction(m + 5, 2)
    gamma = context.divide(decimal.Decimal(gamma.numerator), decimal.Decimal(gamma.denominator))
    return context.add(context.multiply(gamma, exact), context.multiply(context.add(decimal.Decimal(1), gamma), carried))


def tally(cell, value, cells, first, batches):
    """(batch sums (batches, cells), total (cells,)) of rays that put value[r] into cell[r], in fp64."""
    sums = np.zeros((batches, cells))
    np.add.at(sums, (batch_index(first, len(cell), batches), cell), value)
    return sums, np.bincount(cell, weights=value, minlength=cells)
