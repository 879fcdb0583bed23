"""The volume quadrature of include/gf_hip.h in numpy, line for line, fed to the profile model of tests/flux_model.py, and
the planted map of the analytic solid.  numpy's elementwise fp64 operations are single IEEE operations: the arrays below
hold the bits the host and the device must produce."""
import numpy as np

import flux_model

WHOLE = (-np.inf, np.inf, -np.inf, np.inf)


def total_points(tables, sub):
    numr, numz = np.asarray(tables["psi_c00"]).shape
    return numr*sub*numz*sub


def points(tables, sub, first=0, count=None):
    """(gr, gz, R, z, w) of the points first .. first + count."""
    numz = np.asarray(tables["psi_c00"]).shape[1]
    row = numz*sub
    count = total_points(tables, sub) - first if count is None else count
    t = np.arange(first, first + count, dtype=np.int64)
    gr, gz = t//row, t % row
    rmin, dr, zmin, dz = (np.float64(tables[k]) for k in ("rmin", "dr", "zmin", "dz"))
    twice = np.float64(2*sub)
    fr = (2*gr + 1).astype(np.float64)/twice
    fz = (2*gz + 1).astype(np.float64)/twice
    r = rmin + dr*fr
    z = zmin + dz*fz
    area = (dr/np.float64(sub))*(dz/np.float64(sub))
    return gr, gz, r, z, r*area


def in_window(window, r, z):
    rlo, rhi, zlo, zhi = (np.float64(v) for v in window)
    return (rlo <= r) & (r < rhi) & (zlo <= z) & (z < zhi)


def deposit(profile, tables, sub, window=None, first=0, count=None):
    """The points into a flux_model.Profile: those in the window through add(R, 0, z, w), the others seen and outside."""
    _, _, r, z, w = points(tables, sub, first, count)
    take = in_window(WHOLE if window is None else window, r, z)
    profile.add(r[take], np.zeros(int(take.sum())), z[take], w[take])
    left_out = int((~take).sum())
    profile.counts["samples"] += left_out
    profile.counts["outside"] += left_out
    return profile


def model(tables, edges, sub, window=None, first=0, count=None, **options):
    return deposit(flux_model.Profile(tables, edges, **options), tables, sub, window, first, count)


#  psi = (R - 2)^2 + z^2 on 1 <= R < 3, -1 <= z < 1, 8 x 8 cells: with R = 1 + tr/4 and z = -1 + tz/4 that is
#  2 - tr/2 + tr^2/16 - tz/2 + tz^2/16 in the global normalised coordinates, the same 16 coefficients in every cell.
#  psi0 = 0, span = 1: the label is the squared distance from the circle R = 2, z = 0, and a cell of the label a torus
#  shell of volume 2 pi * 2 * pi * (edge[i+1] - edge[i]) (Pappus).
SOLID_EDGES = np.array([0.04, 0.25, 0.64])
SOLID_RANGE = dict(psi0=0.0, span=1.0)


def solid_tables():
    tables = {name: np.zeros((8, 8)) for name in flux_model.TABLE_NAMES}
    for name, value in (("psi_c00", 2.0), ("psi_c10", -0.5), ("psi_c20", 0.0625), ("psi_c01", -0.5), ("psi_c02", 0.0625)):
        tables[name][:] = value
    tables.update(rmin=np.float64(1.0), dr=np.float64(0.25), zmin=np.float64(-1.0), dz=np.float64(0.25))
    return tables


def solid_exact():
    return 2.0*np.pi*2.0*np.pi*np.diff(SOLID_EDGES)


def solid_bound(sub):
    """Per cell the most the quadrature can miss the shell's volume by.  A sub-cell's weight is the exact integral of R
    over it (the midpoint rule is exact for a linear integrand), so only the sub-cells that one of the cell's two
    bounding circles cuts contribute an error, each at most its own weight: those whose centre's distance rho from the
    circle R = 2, z = 0 lies within half a sub-cell diagonal of sqrt(edge)."""
    tables = solid_tables()
    _, _, r, z, w = points(tables, sub)
    rho = np.hypot(r - 2.0, z)
    reach = 0.5*np.hypot(0.25/sub, 0.25/sub)
    cut = [np.abs(rho - np.sqrt(edge)) <= reach for edge in SOLID_EDGES]
    return np.array([2.0*np.pi*w[cut[i] | cut[i + 1]].sum() for i in range(SOLID_EDGES.size - 1)])
