"""The model of the batches of particles (graph_framework_amd/batches.py, csrc/ray_batches.hpp with a particle's index in
place of a ray's): batch g's particles are selected in numpy and fed to the existing models of tests/moments_model.py and
tests/phase_model.py, one plain model per batch; the jackknife error of a ratio in rational arithmetic with the square
root taken last, and its rounding bound.  Nothing here is shared with the code under test but batches.batch_of."""
import decimal
from fractions import Fraction

import numpy as np

from graph_framework_amd import batches

import moments_model
import phase_model
from test_deposition import LIMBS, canonical_limbs, rounded

DIGITS = 50


def batch_index(first, count, batch_count):
    """int64[count]: the batch of the particles of an add whose first particle is `first`."""
    return batches.batch_of(int(first) + np.arange(int(count), dtype=np.int64), int(batch_count))


class Batched:
    """`batch_count` plain models, model g fed batch g's particles alone; the counters are those of all particles."""

    def __init__(self, make, batch_count):
        self.models = [make() for _ in range(batch_count)]
        self.batch_count = batch_count

    def add(self, columns, first, weight=None):
        batch = batch_index(first, len(columns[0]), self.batch_count)
        for g, model in enumerate(self.models):
            chosen = batch == g
            if chosen.any():
                model.add(*[np.asarray(c)[chosen] for c in columns], weight=None if weight is None else np.asarray(weight)[chosen])
        return self

    @property
    def counts(self):
        return {name: sum(model.counts[name] for model in self.models) for name in ("samples", "outside", "skipped")}

    def deposited(self):
        """int[batch_count]: the particles of every batch that deposited."""
        return np.array([m.counts["samples"] - m.counts["outside"] - m.counts["skipped"] for m in self.models])

    def state(self):
        return np.stack([model.state() for model in self.models])

    def bins(self):
        return np.stack([model.bins() for model in self.models])

    def total_units(self):
        return [sum(units) for units in zip(*[model.units for model in self.models])]

    def total_state(self):
        shape = self.models[0].shape
        return np.array([canonical_limbs(total) for total in self.total_units()], dtype=np.int64).reshape(shape + (LIMBS,))

    def total_bins(self):
        return np.array([rounded(total) for total in self.total_units()]).reshape(self.models[0].shape)


def moments(tables, sedges, batch_count, **options):
    return Batched(lambda: moments_model.Moments(tables, sedges, **options), batch_count)


def phase(tables, sedges, pedges, gedges, batch_count, **options):
    return Batched(lambda: phase_model.Phase(tables, sedges, pedges, gedges, **options), batch_count)


def merged_limbs(limbs):
    """The slabs of a batched state (G, ..., 67) added limb by limb as integers, then made canonical as the models do:
    (..., 67) int64."""
    limbs = np.asarray(limbs)
    flat = limbs.reshape(limbs.shape[0], -1, LIMBS)
    out = []
    for cell in range(flat.shape[1]):
        total = sum(int(limb) << (32*k) for slab in flat[:, cell] for k, limb in enumerate(slab))
        out.append(canonical_limbs(total))
    return np.array(out, dtype=np.int64).reshape(limbs.shape[1:])


def _root(value, context):
    return context.sqrt(context.divide(decimal.Decimal(value.numerator), decimal.Decimal(value.denominator)))


def exact_ratio_error(num, den):
    """The jackknife error of one cell's planted sums, doubles taken as the exact numbers they are: a Decimal of DIGITS
    digits, the root taken last; None with fewer than two batches with particles (either sum non-zero) or a zero
    denominator."""
    pairs = [(Fraction(float(a)), Fraction(float(b))) for a, b in zip(num, den) if float(a) != 0.0 or float(b) != 0.0]
    m = len(pairs)
    if m < 2:
        return None
    s1, s0 = sum(a for a, _ in pairs), sum(b for _, b in pairs)
    if any(s0 - b == 0 for _, b in pairs):
        return None
    replicates = [(s1 - a)/(s0 - b) for a, b in pairs]
    mean = sum(replicates)/m
    variance = Fraction(m - 1, m)*sum((r - mean)**2 for r in replicates)
    return _root(variance, decimal.Context(prec=DIGITS + 10))


def ratio_error_bound(num, den):
    """The bound on |fp64 ratio_error_of - exact| for one cell, a Decimal, from the roundings of its numpy expression
    (u = 2^-53, m batches with particles; roundings only, no operation under- or overflows).

    S1 and S0 are sums of m terms, in any order: |S~ - S| <= (m - 1) u A with A the sum of the absolute values.  S1 - S1_g
    and S0 - S0_g round once more.  With N_g = S1 - S1_g, D_g = S0 - S0_g exact, A1 = sum |S1_g|, A0 = sum |S0_g|:
        |N~_g - N_g| <= e1 = (m - 1) u A1 + u (A1 + |S1_g|) (1 + m u),   |D~_g - D_g| <= e0 likewise;
    the quotient rounds once: |R~_g - R_g| <= rho_g = (e1 + |R_g| e0)/(|D_g| - e0) + u (|R_g| + that).
    Rbar: a sum of m terms and a division, |Rbar~ - Rbar| <= max rho + (m) u max|R~|.  Each deviation d_g = R_g - Rbar is
    off by at most delta_g = rho_g + (max rho + m u B) + u (|d_g| + those), B = max |R_g| + max rho.  The radicand
    (m - 1)/m sum d^2 passes two roundings per term (square, the factor applied at the end counts two: the quotient and
    the product), m - 1 in the sum; the root halves them and rounds once.  With the triangle inequality of the 2-norm
        |got - exact| <= gamma exact + (1 + gamma) sqrt((m - 1)/m sum delta_g^2),   gamma = (1 + u)^((m + 5)/2) - 1,
    every first-order term taken 1.0001 times to cover the higher orders."""
    u = Fraction(1, 2**53)
    slack = Fraction(10001, 10000)
    pairs = [(Fraction(float(a)), Fraction(float(b))) for a, b in zip(num, den) if float(a) != 0.0 or float(b) != 0.0]
    m = len(pairs)
    s1, s0 = sum(a for a, _ in pairs), sum(b for _, b in pairs)
    a1, a0 = sum(abs(a) for a, _ in pairs), sum(abs(b) for _, b in pairs)
    replicates = [(s1 - a)/(s0 - b) for a, b in pairs]
    rho = []
    for (a, b), r in zip(pairs, replicates):
        e1 = slack*u*((m - 1)*a1 + (a1 + abs(a)))
        e0 = slack*u*((m - 1)*a0 + (a0 + abs(b)))
        assert abs(s0 - b) > e0
        first = (e1 + abs(r)*e0)/(abs(s0 - b) - e0)
        rho.append(slack*(first + u*(abs(r) + first)))
    top = max(abs(r) for r in replicates) + max(rho)
    mean = sum(replicates)/m
    shift = max(rho) + slack*m*u*top
    deltas = [p + shift + slack*u*(abs(r - mean) + p + shift) for p, r in zip(rho, replicates)]
    context = decimal.Context(prec=DIGITS + 10)
    carried = _root(Fraction(m - 1, m)*sum(d*d for d in deltas), context)
    gamma = slack*u*Fraction(m + 5, 2)
    gamma = context.divide(decimal.Decimal(gamma.numerator), decimal.Decimal(gamma.denominator))
    exact = exact_ratio_error(num, den)
    return context.add(context.multiply(gamma, exact), context.multiply(context.add(decimal.Decimal(1), gamma), carried))
