#!/usr/bin/env python3
"""Generate tests/golden/flux_golden.npz: the reference graph layer's psi on points of the EFIT table.

psi comes from oracle/_ref/gf_ref (`psi2`: equilibrium.hpp's build_psi evaluated by the reference's own graph,
strict IEEE fp64), through oracle.ref.Reference._run.  The file holds DATA only:

    r, z            4096 points uniform over the table, 200 of them on cell boundaries of each axis
    psi             the reference's psi there
    noise           the largest distance of the reference's psi from an 80-bit (numpy.longdouble) evaluation of the
                    same polynomial: what an fp64 evaluation of this ill-conditioned form is worth
    model_distance  the largest distance of tests/flux_model.py's psi from the reference's
    model_long      ... and from the 80-bit evaluation
    band_cells, band_dropped
                    for 7, 64 and 256 uniform cells on [0, 1]: the points whose reference label lies within 1e-6 of
                    an edge, which the cell-agreement test leaves out

Run:  python tests/golden/make_flux_golden.py        (needs make -C oracle ref)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref  # noqa: E402
import flux_model  # noqa: E402

POINTS, ON_EDGES, SEED, BAND = 4096, 200, 7, 1.0e-6


def points(tables):
    rng = np.random.default_rng(SEED)
    numr, numz = tables["psi_c00"].shape
    rmin, dr, zmin, dz = (float(tables[k]) for k in ("rmin", "dr", "zmin", "dz"))
    tr = rng.uniform(0.0, numr, POINTS)
    tz = rng.uniform(0.0, numz, POINTS)
    tr[:ON_EDGES] = rng.integers(0, numr, ON_EDGES)                        # on cell boundaries in r
    tz[ON_EDGES:2*ON_EDGES] = rng.integers(0, numz, ON_EDGES)              # ... and in z
    r, z = rmin + tr*dr, zmin + tz*dz
    qr, qz = flux_model.normalised(tables, r, z)
    keep = (qr >= 0.0) & (qr < numr) & (qz >= 0.0) & (qz < numz)           # the quotient decides, as in the label
    assert keep.sum() >= POINTS - 8, keep.sum()
    r[~keep], z[~keep] = rmin + 0.5*dr, zmin + 0.5*dz
    order = rng.permutation(POINTS)
    return r[order], z[order]


def long_psi(tables, r, z):
    """The same polynomial in 80-bit arithmetic, in the cell the fp64 quotients choose."""
    qr, qz = flux_model.normalised(tables, r, z)
    i, j = qr.astype(np.int64), qz.astype(np.int64)
    long = np.longdouble
    tr = (r.astype(long) - long(tables["rmin"]))/long(tables["dr"])
    tz = (z.astype(long) - long(tables["zmin"]))/long(tables["dz"])
    column = []
    for a in range(4):
        c = [tables["psi_c%d%d" % (a, b)][i, j].astype(long) for b in range(4)]
        column.append(((c[3]*tz + c[2])*tz + c[1])*tz + c[0])
    return ((column[3]*tr + column[2])*tr + column[1])*tr + column[0]


def measure(tables, r, z, psi):
    """(noise, model against reference, model against 80 bits, dropped per cell count)."""
    exact = long_psi(tables, r, z)
    model = flux_model.psi_rz(tables, *flux_model.normalised(tables, r, z))
    noise = float(np.abs(psi.astype(np.longdouble) - exact).max())
    psi0, span = flux_model.default_range(tables)
    label = (psi - psi0)/span
    cells = np.array([7, 64, 256])
    dropped = [int((np.abs(label[:, None] - np.linspace(0.0, 1.0, n + 1)[None, :]).min(axis=1) < BAND).sum()) for n in cells]
    return noise, float(np.abs(model - psi).max()), float(np.abs(model.astype(np.longdouble) - exact).max()), cells, np.array(dropped)


def main():
    tables = np.load(os.path.join(HERE, "efit_tables.npz"))
    r, z = points(tables)
    out, _ = ref.Reference(tables)._run("f64", "psi2", [r, z])
    psi = out[0]
    noise, distance, against_long, cells, dropped = measure(tables, r, z, psi)
    span = flux_model.default_range(tables)[1]
    print("noise %.3e (%.2e of the span); model against reference %.3e = %.2f x noise; model against 80 bits %.3e; "
          "dropped %r of %d" % (noise, noise/span, distance, distance/noise, against_long, dropped.tolist(), POINTS))
    np.savez(os.path.join(HERE, "flux_golden.npz"), r=r, z=z, psi=psi, noise=np.float64(noise),
             model_distance=np.float64(distance), model_long=np.float64(against_long), band_cells=cells, band_dropped=dropped)


if __name__ == "__main__":
    main()
