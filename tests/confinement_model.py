"""The first-exit rule of csrc/confinement.hip in numpy, and the tracker model the tests compare against.

The label is flux_model.label's, line for line the header's; columns of an fp32 state are widened first, which is exact,
so one model serves both types.  The footprint's cells are in rational arithmetic, as phase_model.Phase's."""
import numpy as np

import flux_model
from phase_model import LIMBS, canonical_limbs, rounded, units

CONFINED = 0xFFFFFFFF


def canonical(values):
    """Every NaN as the quiet NaN without payload."""
    values = np.array(values, dtype=np.float64)
    values[np.isnan(values)] = np.nan
    return values


def radius(x, y):
    x, y = (np.asarray(v).astype(np.float64) for v in (x, y))
    with np.errstate(invalid="ignore", over="ignore"):
        xx = x*x
        yy = y*y
        return np.sqrt(xx + yy)


class Confinement:
    """What a Confinement must hold after its checks: lost_step, alive, the exit arrays, per check its step and the
    number newly lost, per cell (ir, iz, ig) the exact sum as an integer count of 2^-1074, and the counters."""

    def __init__(self, tables, redges, zedges, gedges, count, limit=1.0, **options):
        self.tables = tables
        self.edges = [np.asarray(e, dtype=np.float64) for e in (redges, zedges, gedges)]
        self.options = options
        self.limit = np.float64(limit)
        self.shape = tuple(e.size - 1 for e in self.edges)
        self.units = [0]*int(np.prod(self.shape))
        self.counts = dict(samples=0, outside=0, skipped=0)
        self.lost_step = np.full(count, CONFINED, dtype=np.uint32)
        self.alive = np.ones(count)
        self.exit_r = np.full(count, np.nan)
        self.exit_z = np.full(count, np.nan)
        self.steps, self.newly_lost = [], []
        self.deposits = np.zeros(count, dtype=np.int64)      # how often each particle has reached the cells' rule

    def labels(self, x, y, z):
        return canonical(flux_model.label(self.tables, *(np.asarray(v).astype(np.float64) for v in (x, y, z)), **self.options))

    def check(self, x, y, z, ux, uy, uz, gamma, step, weight=None):
        z, gamma = (np.asarray(v).astype(np.float64) for v in (z, gamma))
        with np.errstate(invalid="ignore"):
            lost = (self.lost_step == CONFINED) & ~(self.labels(x, y, z) < self.limit)
        r = radius(x, y)
        self.lost_step[lost] = step
        self.alive[lost] = 0.0
        self.exit_r[lost] = canonical(r[lost])
        self.exit_z[lost] = canonical(z[lost])
        self.deposits[lost] += 1
        self.steps.append(int(step))
        self.newly_lost.append(int(lost.sum()))
        value = (np.ones(gamma.size) if weight is None else np.asarray(weight).astype(np.float64))[lost]
        cr, cz, cg = (flux_model.cells_of(e, v[lost]) for e, v in zip(self.edges, (r, z, gamma)))
        inside = (cr >= 0) & (cz >= 0) & (cg >= 0)
        cell = np.where(inside, (cr*self.shape[1] + cz)*self.shape[2] + cg, -1)
        finite = np.isfinite(value)
        self.counts["samples"] += int(lost.sum())
        self.counts["outside"] += int((~inside).sum())
        self.counts["skipped"] += int((inside & ~finite).sum())
        take = inside & finite
        pairs, number = np.unique(np.stack([cell[take].astype(np.uint64), value[take].view(np.uint64)]), axis=1, return_counts=True)
        for c, bits, k in zip(pairs[0], pairs[1], number):
            self.units[int(c)] += int(k)*units(np.uint64(bits).view(np.float64))
        return self

    def confined(self):
        return self.lost_step.size - np.cumsum(np.array(self.newly_lost, dtype=np.int64))

    def state(self):
        return np.array([canonical_limbs(total) for total in self.units], dtype=np.int64).reshape(self.shape + (LIMBS,))

    def bins(self, divisor=1.0):
        out = np.array([rounded(total) for total in self.units]).reshape(self.shape)
        with np.errstate(over="ignore", invalid="ignore"):
            return out/np.float64(divisor)
