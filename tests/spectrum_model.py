"""The field direction and the parallel refractive index of csrc/flux_label.hpp in numpy, line for line, and the spectrum
model the GPU tests compare against.

As in flux_model.py every numpy operation below is one IEEE fp64 operation and numpy.sqrt is correctly rounded: the arrays
hold the bits the header must produce.  With dtype=numpy.longdouble the same lines are the 80-bit evaluation."""
import numpy as np

from test_deposition import LIMBS, canonical_limbs, rounded, units

import flux_model

C = 1.0/np.sqrt(8.8541878138E-12*(np.pi*4.0E-7))                             # dispersion.hpp:494-502
FPOL_NAMES = tuple("fpol_c%d" % k for k in range(4))


def columns_of(tables, i, j, tz, dtype):
    """col_a and dcol_a, a = 0..3."""
    column, slope = [], []
    for a in range(4):
        c = [np.asarray(tables["psi_c%d%d" % (a, b)])[i, j].astype(dtype) for b in range(4)]
        t = c[3]*tz
        t = t + c[2]
        t = t*tz
        t = t + c[1]
        t = t*tz
        column.append(t + c[0])
        t = c[3]*dtype(3.0)
        t = t*tz
        u = c[2]*dtype(2.0)
        t = t + u
        t = t*tz
        slope.append(t + c[1])
    return column, slope


def horner(c, t):
    p = c[3]*t
    p = p + c[2]
    p = p*t
    p = p + c[1]
    p = p*t
    return p + c[0]


def field_rz(tables, r, tr, tz, dtype=np.float64):
    """(psi, gR, gZ, fpol, tp, q) at points inside the map, in `dtype` arithmetic; R B = (gZ, fpol, -gR)."""
    i = tr.astype(np.int64)
    j = tz.astype(np.int64)
    tr = tr.astype(dtype)
    tz = tz.astype(dtype)
    column, slope = columns_of(tables, i, j, tz, dtype)
    psi_tz = horner(slope, tr)
    t = column[3]*dtype(3.0)
    t = t*tr
    u = column[2]*dtype(2.0)
    t = t + u
    t = t*tr
    psi_tr = t + column[1]
    psi = horner(column, tr)
    gr = psi_tr/dtype(tables["dr"])
    gz = psi_tz/dtype(tables["dz"])
    tp = (psi - dtype(tables["psimin"]))/dtype(tables["dpsi"])
    numpsi = np.asarray(tables["fpol_c0"]).size
    q = np.zeros(tp.shape, dtype=np.int64)                                  # 0 unless tp >= 0: a NaN gives 0
    above = tp >= dtype(numpsi)
    between = (tp >= 0) & ~above
    q[above] = numpsi - 1
    q[between] = tp[between].astype(np.int64)
    f = horner([np.asarray(tables[name]).reshape(-1)[q].astype(dtype) for name in FPOL_NAMES], tp)
    return psi, gr, gz, f, tp, q


def npar_from(x, y, r, kx, ky, kz, w, gr, gz, f, c, dtype=np.float64):
    x, y, r, kx, ky, kz, w, gr, gz, f = (v.astype(dtype) for v in (x, y, r, kx, ky, kz, w, gr, gz, f))
    kxx = kx*x
    kyy = ky*y
    a = kxx + kyy
    kyx = ky*x
    kxy = kx*y
    b = kyx - kxy
    agz = a*gz
    bf = b*f
    along = (agz + bf)/r
    kzgr = kz*gr
    num = along - kzgr
    den = np.sqrt((gz*gz + f*f) + gr*gr)
    cosine = num/den
    return (dtype(c)*cosine)/w


def label_npar(tables, x, y, z, kx, ky, kz, w, psi0=None, span=None, sqrt_label=False, c=C):
    """(label, npar) of every sample, both NaN outside the map."""
    x, y, z, kx, ky, kz, w = (np.asarray(v, dtype=np.float64) for v in (x, y, z, kx, ky, kz, w))
    if psi0 is None or span is None:
        low, width = flux_model.default_range(tables)
        psi0 = low if psi0 is None else psi0
        span = width if span is None else span
    numr, numz = np.asarray(tables["psi_c00"]).shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        xx = x*x
        yy = y*y
        r = np.sqrt(xx + yy)
        tr, tz = flux_model.normalised(tables, r, z)
        inside = (tr >= 0.0) & (tr < np.float64(numr)) & (tz >= 0.0) & (tz < np.float64(numz))
        label = np.full(x.shape, np.nan)
        npar = np.full(x.shape, np.nan)
        psi, gr, gz, f, _, _ = field_rz(tables, r[inside], tr[inside], tz[inside])
        s = (psi - np.float64(psi0))/np.float64(span)
        label[inside] = np.sqrt(s) if sqrt_label else s
        npar[inside] = npar_from(x[inside], y[inside], r[inside], kx[inside], ky[inside], kz[inside], w[inside], gr, gz, f, c)
    label[np.isnan(label)] = np.nan                                        # canonical(): one NaN, whatever the processor's
    npar[np.isnan(npar)] = np.nan
    return label, npar


class Spectrum:
    """What a FluxSpectrum must hold: per cell (is, in) the exact sum as an integer count of 2^-1074, and the counters."""

    def __init__(self, tables, sedges, nedges, **options):
        self.tables = tables
        self.sedges = np.asarray(sedges, dtype=np.float64)
        self.nedges = np.asarray(nedges, dtype=np.float64)
        self.options = options
        self.shape = (self.sedges.size - 1, self.nedges.size - 1)
        self.units = [0]*(self.shape[0]*self.shape[1])
        self.counts = dict(samples=0, outside=0, skipped=0)

    def add(self, x, y, z, kx, ky, kz, w, value):
        label, npar = label_npar(self.tables, x, y, z, kx, ky, kz, w, **self.options)
        cs = flux_model.cells_of(self.sedges, label)
        cn = flux_model.cells_of(self.nedges, npar)
        value = np.asarray(value, dtype=np.float64)
        inside = (cs >= 0) & (cn >= 0)
        cell = np.where(inside, cs*self.shape[1] + cn, -1)
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
