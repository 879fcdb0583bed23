"""The pitch cosine of csrc/flux_label.hpp in numpy, line for line, and the distribution model the GPU tests compare
against.

As in spectrum_model.py every numpy operation below is one IEEE fp64 operation and numpy.sqrt is correctly rounded: the
arrays hold the bits the header must produce.  Columns of an fp32 state are widened first, which is exact, so one model
serves both types.  With dtype=numpy.longdouble the same lines are the 80-bit evaluation."""
import numpy as np

from test_deposition import LIMBS, canonical_limbs, rounded, units

import flux_model
import spectrum_model


def cosine_from(x, y, r, ux, uy, uz, gr, gz, f, dtype=np.float64):
    """num/den of flux_label.hpp's cosine_of with u in place of k."""
    x, y, r, ux, uy, uz, gr, gz, f = (v.astype(dtype) for v in (x, y, r, ux, uy, uz, gr, gz, f))
    uxx = ux*x
    uyy = uy*y
    a = uxx + uyy
    uyx = uy*x
    uxy = ux*y
    b = uyx - uxy
    agz = a*gz
    bf = b*f
    along = (agz + bf)/r
    uzgr = uz*gr
    num = along - uzgr
    gzgz = gz*gz
    ff = f*f
    grgr = gr*gr
    den = np.sqrt((gzgz + ff) + grgr)
    return num/den


def quotient_from(cosine, ux, uy, uz, dtype=np.float64):
    """cosine/p, not yet clamped."""
    ux, uy, uz = (v.astype(dtype) for v in (ux, uy, uz))
    uxux = ux*ux
    uyuy = uy*uy
    uzuz = uz*uz
    uu = (uxux + uyuy) + uzuz
    p = np.sqrt(uu)
    return cosine/p


def clamped(xi):
    """if (xi > 1) xi = 1; if (xi < -1) xi = -1: comparisons, a NaN stays."""
    xi = xi.copy()
    xi[xi > 1.0] = 1.0
    xi[xi < -1.0] = -1.0
    return xi


def field_at(tables, x, y, z, dtype=np.float64):
    """(inside, r, gR, gZ, fpol, psi) with the last four at the points inside the map only."""
    x, y, z = (np.asarray(v, dtype=np.float64) for v in (x, y, z))
    numr, numz = np.asarray(tables["psi_c00"]).shape
    xx = x*x
    yy = y*y
    r = np.sqrt(xx + yy)
    tr, tz = flux_model.normalised(tables, r, z)
    inside = (tr >= 0.0) & (tr < np.float64(numr)) & (tz >= 0.0) & (tz < np.float64(numz))
    psi, gr, gz, f, _, _ = spectrum_model.field_rz(tables, r[inside], tr[inside], tz[inside], dtype)
    return inside, r, gr, gz, f, psi


def label_pitch(tables, x, y, z, ux, uy, uz, psi0=None, span=None, sqrt_label=False, unclamped=False):
    """(label, xi) of every particle, both NaN outside the map; with unclamped=True also the quotient before the clamp."""
    x, y, z, ux, uy, uz = (np.asarray(v).astype(np.float64) for v in (x, y, z, ux, uy, uz))
    if psi0 is None or span is None:
        low, width = flux_model.default_range(tables)
        psi0 = low if psi0 is None else psi0
        span = width if span is None else span
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        inside, r, gr, gz, f, psi = field_at(tables, x, y, z)
        label = np.full(x.shape, np.nan)
        raw = np.full(x.shape, np.nan)
        s = (psi - np.float64(psi0))/np.float64(span)
        label[inside] = np.sqrt(s) if sqrt_label else s
        cosine = cosine_from(x[inside], y[inside], r[inside], ux[inside], uy[inside], uz[inside], gr, gz, f)
        raw[inside] = quotient_from(cosine, ux[inside], uy[inside], uz[inside])
        xi = clamped(raw)
    label[np.isnan(label)] = np.nan                                        # canonical(): one NaN, whatever the processor's
    xi[np.isnan(xi)] = np.nan
    return (label, xi, raw) if unclamped else (label, xi)


class Phase:
    """What a PhaseDistribution must hold: per cell (is, ip, ig) the exact sum as an integer count of 2^-1074, and the
    counters."""

    def __init__(self, tables, sedges, pedges, gedges, **options):
        self.tables = tables
        self.edges = [np.asarray(e, dtype=np.float64) for e in (sedges, pedges, gedges)]
        self.options = options
        self.shape = tuple(e.size - 1 for e in self.edges)
        self.units = [0]*int(np.prod(self.shape))
        self.counts = dict(samples=0, outside=0, skipped=0)

    def add(self, x, y, z, ux, uy, uz, gamma, weight=None):
        label, xi = label_pitch(self.tables, x, y, z, ux, uy, uz, **self.options)
        gamma = np.asarray(gamma).astype(np.float64)
        cs, cp, cg = (flux_model.cells_of(e, v) for e, v in zip(self.edges, (label, xi, gamma)))
        value = np.ones(gamma.size) if weight is None else np.asarray(weight).astype(np.float64)
        inside = (cs >= 0) & (cp >= 0) & (cg >= 0)
        cell = np.where(inside, (cs*self.shape[1] + cp)*self.shape[2] + cg, -1)
        finite = np.isfinite(value)
        self.counts["samples"] += value.size
        self.counts["outside"] += int((~inside).sum())
        self.counts["skipped"] += int((inside & ~finite).sum())
        take = inside & finite
        pairs, number = np.unique(np.stack([cell[take].astype(np.uint64), value[take].view(np.uint64)]), axis=1, return_counts=True)
        for c, bits, k in zip(pairs[0], pairs[1], number):
            self.units[int(c)] += int(k)*units(np.uint64(bits).view(np.float64))
        return self

    def state(self):
        return np.array([canonical_limbs(total) for total in self.units], dtype=np.int64).reshape(self.shape + (LIMBS,))

    def bins(self, divisor=1.0):
        out = np.array([rounded(total) for total in self.units]).reshape(self.shape)
        with np.errstate(over="ignore", invalid="ignore"):
            return out/np.float64(divisor)
