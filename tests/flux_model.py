"""The flux label of csrc/flux_label.hpp in numpy, line for line, and the profile model the GPU tests compare against.

numpy's elementwise fp64 operations are single IEEE operations (no fusing), numpy.sqrt is the correctly rounded square
root: the arrays below hold the bits the header must produce."""
import numpy as np

from test_deposition import LIMBS, canonical_limbs, rounded, units

TABLE_NAMES = tuple("psi_c%d%d" % (a, b) for a in range(4) for b in range(4))


def default_range(tables):
    """psi0 = psimin, span = dpsi*(numpsi - 1): the axis-to-edge range of the reference's profile tables."""
    return float(tables["psimin"]), float(tables["dpsi"])*(tables["fpol_c0"].size - 1)


def psi_rz(tables, tr, tz, dtype=np.float64):
    """psi at normalised coordinates inside the map, in `dtype` arithmetic (float64: the contract; longdouble: the
    80-bit evaluation of the same polynomial)."""
    i = tr.astype(np.int64)
    j = tz.astype(np.int64)
    tr = tr.astype(dtype)
    tz = tz.astype(dtype)
    column = []
    for a in range(4):
        c = [np.asarray(tables["psi_c%d%d" % (a, b)])[i, j].astype(dtype) for b in range(4)]
        t = c[3]*tz
        t = t + c[2]
        t = t*tz
        t = t + c[1]
        t = t*tz
        column.append(t + c[0])
    p = column[3]*tr
    p = p + column[2]
    p = p*tr
    p = p + column[1]
    p = p*tr
    return p + column[0]


def normalised(tables, r, z):
    tr = (r - np.float64(tables["rmin"]))/np.float64(tables["dr"])
    tz = (z - np.float64(tables["zmin"]))/np.float64(tables["dz"])
    return tr, tz


def label(tables, x, y, z, psi0=None, span=None, sqrt_label=False):
    """The label of every point, NaN outside the map."""
    x, y, z = (np.asarray(c, dtype=np.float64) for c in (x, y, z))
    if psi0 is None or span is None:
        low, width = default_range(tables)
        psi0 = low if psi0 is None else psi0
        span = width if span is None else span
    numr, numz = np.asarray(tables["psi_c00"]).shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xx = x*x
        yy = y*y
        r = np.sqrt(xx + yy)
        tr, tz = normalised(tables, r, z)
        inside = (tr >= 0.0) & (tr < np.float64(numr)) & (tz >= 0.0) & (tz < np.float64(numz))
        out = np.full(x.shape, np.nan)
        psi = psi_rz(tables, tr[inside], tz[inside])
        s = (psi - np.float64(psi0))/np.float64(span)
        out[inside] = np.sqrt(s) if sqrt_label else s
    return out


def cells_of(edges, labels):
    """The cell of every label by edge[i] <= label < edge[i+1], -1 outside the edges or NaN."""
    edges = np.asarray(edges, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = (labels >= edges[0]) & (labels < edges[-1])
    cell = np.searchsorted(edges, np.where(inside, labels, edges[0]), side="right") - 1
    return np.where(inside, cell, -1)


class Profile:
    """What a FluxProfile must hold: per cell the exact sum as an integer count of 2^-1074, and the three counters."""

    def __init__(self, tables, edges, **options):
        self.tables = tables
        self.edges = np.asarray(edges, dtype=np.float64)
        self.options = options
        self.units = [0]*(self.edges.size - 1)
        self.counts = dict(samples=0, outside=0, skipped=0)

    def add(self, x, y, z, value):
        cell = cells_of(self.edges, label(self.tables, x, y, z, **self.options))
        value = np.asarray(value, dtype=np.float64)
        inside = cell >= 0
        finite = np.isfinite(value)
        self.counts["samples"] += value.size
        self.counts["outside"] += int((~inside).sum())
        self.counts["skipped"] += int((inside & ~finite).sum())
        take = inside & finite
#  equal (cell, value) pairs once, times their number: long adds of tiled samples stay cheap and exact
        pairs, number = np.unique(np.stack([cell[take].astype(np.uint64), value[take].view(np.uint64)]), axis=1, return_counts=True)
        for c, bits, k in zip(pairs[0], pairs[1], number):
            self.units[int(c)] += int(k)*units(np.uint64(bits).view(np.float64))
        return self

    def state(self):
        return np.array([canonical_limbs(total) for total in self.units], dtype=np.int64).reshape(-1, LIMBS)

    def bins(self, divisor=1.0):
        out = np.array([rounded(total) for total in self.units])
        with np.errstate(over="ignore", invalid="ignore"):
            return out/np.float64(divisor)
