"""The moments of csrc/flux_label.hpp's moments_of in numpy, line for line, and the model the GPU tests compare a
FluxMoments against.

As in phase_model.py every numpy operation below is one IEEE fp64 operation: the arrays hold the bits the header must
produce.  Columns of an fp32 state are widened first, which is exact, so one model serves both types.  With
dtype=numpy.longdouble the same lines are the 80-bit evaluation."""
import numpy as np

from test_deposition import LIMBS, canonical_limbs, rounded, units

import flux_model
import phase_model

MOMENTS = ("density", "current", "energy", "radiation")


def moments_from(x, y, r, ux, uy, uz, gamma, gr, gz, f, dtype=np.float64, parts=False):
    """(n, 4): m = {1, vpar, kin, rad} of moments_of; with parts=True also a dict of uu, upup, the unclamped perp and bsq."""
    upar = phase_model.cosine_from(x, y, r, ux, uy, uz, gr, gz, f, dtype)
    r, ux, uy, uz, gamma, gr, gz, f = (v.astype(dtype) for v in (r, ux, uy, uz, gamma, gr, gz, f))
    vpar = upar/gamma
    kin = gamma - dtype(1.0)
    uxux = ux*ux
    uyuy = uy*uy
    uzuz = uz*uz
    uu = (uxux + uyuy) + uzuz
    upup = upar*upar
    raw = uu - upup
    perp = raw.copy()
    perp[perp < 0.0] = 0.0                                                 # a comparison: a NaN stays one
    gzgz = gz*gz
    ff = f*f
    grgr = gr*gr
    bsum = (gzgz + ff) + grgr
    rr = r*r
    bsq = bsum/rr
    rad = perp*bsq
    out = np.stack([np.ones(vpar.shape, dtype=dtype), vpar, kin, rad], axis=1)
    return (out, dict(upar=upar, uu=uu, upup=upup, raw=raw, bsq=bsq)) if parts else out


def label_values(tables, x, y, z, ux, uy, uz, gamma, psi0=None, span=None, sqrt_label=False, parts=False):
    """(label (n,), values (n, 4)) of every particle, all NaN outside the map; with parts=True also (inside, the parts of
    the particles inside)."""
    x, y, z, ux, uy, uz, gamma = (np.asarray(v).astype(np.float64) for v in (x, y, z, ux, uy, uz, gamma))
    if psi0 is None or span is None:
        low, width = flux_model.default_range(tables)
        psi0 = low if psi0 is None else psi0
        span = width if span is None else span
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        inside, r, gr, gz, f, psi = phase_model.field_at(tables, x, y, z)
        label = np.full(x.shape, np.nan)
        values = np.full(x.shape + (4,), np.nan)
        s = (psi - np.float64(psi0))/np.float64(span)
        label[inside] = np.sqrt(s) if sqrt_label else s
        values[inside], pieces = moments_from(x[inside], y[inside], r[inside], ux[inside], uy[inside], uz[inside], gamma[inside],
                                              gr, gz, f, parts=True)
    label[np.isnan(label)] = np.nan                                        # canonical(): one NaN, whatever the processor's
    values[np.isnan(values)] = np.nan
    return (label, values, inside, pieces) if parts else (label, values)


class Moments:
    """What a FluxMoments must hold: per cell (is, k) the exact sum as an integer count of 2^-1074, and the counters,
    which count particles.  A particle of which any v[k] is NaN or infinite deposits none of the four."""

    def __init__(self, tables, sedges, **options):
        self.tables = tables
        self.sedges = np.asarray(sedges, dtype=np.float64)
        self.options = options
        self.shape = (self.sedges.size - 1, 4)
        self.units = [0]*(self.shape[0]*4)
        self.counts = dict(samples=0, outside=0, skipped=0)

    def weighted(self, x, y, z, ux, uy, uz, gamma, weight=None):
        """(surface (n,), v (n, 4), takes (n,)): the cell of the label, v[0] = w and v[k] = w*m[k], and who deposits."""
        label, m = label_values(self.tables, x, y, z, ux, uy, uz, gamma, **self.options)
        surface = flux_model.cells_of(self.sedges, label)
        w = np.ones(label.size) if weight is None else np.asarray(weight).astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            v = np.stack([w, w*m[:, 1], w*m[:, 2], w*m[:, 3]], axis=1)
        inside = surface >= 0
        finite = np.isfinite(v).all(axis=1)
        return surface, v, inside, finite

    def add(self, x, y, z, ux, uy, uz, gamma, weight=None):
        surface, v, inside, finite = self.weighted(x, y, z, ux, uy, uz, gamma, weight)
        self.counts["samples"] += surface.size
        self.counts["outside"] += int((~inside).sum())
        self.counts["skipped"] += int((inside & ~finite).sum())
        take = inside & finite
        for k in range(4):
            cell = surface[take]*4 + k
            pairs, number = np.unique(np.stack([cell.astype(np.uint64), v[take, k].copy().view(np.uint64)]), axis=1, return_counts=True)
            for c, bits, n in zip(pairs[0], pairs[1], number):
                self.units[int(c)] += int(n)*units(np.uint64(bits).view(np.float64))
        return self

    def state(self):
        return np.array([canonical_limbs(total) for total in self.units], dtype=np.int64).reshape(self.shape + (LIMBS,))

    def bins(self, divisor=1.0):
        out = np.array([rounded(total) for total in self.units]).reshape(self.shape)
        with np.errstate(over="ignore", invalid="ignore"):
            return out/np.float64(divisor)

    def totals(self):
        """(4,): the exact sums over the surfaces, rounded once."""
        return np.array([rounded(sum(self.units[k::4])) for k in range(4)])
