"""Deposition profiles: what utilities/bin.py computes from result<n>.nc, on the device and exact.

bin.py sums `d_power` over nx*ny*nz boolean masks of every sample (TensorFlow) and divides by the number of
rays.  Here every cell of the grid is an integer superaccumulator (csrc/superacc.hpp) fed by the deposit
kernel of csrc/deposition.hip: a cell holds the exact sum of its samples, rounded once when it is read, so
the profile does not depend on the order of the samples, on the split into records, files or ranks, or on
the run.  The cell rule is bin.py's: edge[i] <= c < edge[i+1] on each axis, against the edges that are
written to bins.nc.
"""
import os

import numpy as np

from .exact_cells import LIMBS, ExactCells, bin_files
from .output import write_bins


class Deposition(ExactCells):
    """A 3-D grid of exact sums on a context's device (gfhip_bins_*, include/gf_hip.h); state() is (nx, ny, nz, 67)."""
    prefix = "bins"

    def __init__(self, context, xedges, yedges, zedges):
        self.edges = [np.ascontiguousarray(e, dtype=np.float64).reshape(-1) for e in (xedges, yedges, zedges)]
        if any(e.size < 2 for e in self.edges):
            raise ValueError("an axis needs at least two edges")
        arguments = []
        for e in self.edges:
            arguments += [e.ctypes.data, e.size - 1]
        self._created(context, [e.size - 1 for e in self.edges], *arguments)

    def like(self, context):
        """An empty grid with this one's edges on another context."""
        return Deposition(context, *self.edges)

    def merge(self, limbs, samples=0, outside=0, skipped=0):
        """Add another grid's state() and counts() (same edges)."""
        limbs = np.ascontiguousarray(limbs, dtype=np.int64)
        if limbs.shape != self.shape + (LIMBS,):
            raise ValueError("merge: limbs of shape %r for a grid of %r" % (limbs.shape, self.shape))
        self.context._check(self.lib.gfhip_bins_merge(self.handle, limbs.ctypes.data, int(samples), int(outside), int(skipped)))


def bin_deposition(directory, num_files, num_x, min_x, max_x, num_y, min_y, max_y, num_z, min_z, max_z, index=0):
    """utilities/bin.py's main(): d_power of result0.nc .. result<num_files - 1>.nc binned on the grid, divided by the
    total number of rays, written to <directory>/bins.nc.  Returns (bins, counts)."""
    from .backend import Context
    edges = [np.linspace(low, high, n + 1) for low, high, n in ((min_x, max_x, num_x), (min_y, max_y, num_y), (min_z, max_z, num_z))]
    context = Context(index)
    deposition = Deposition(context, *edges)
    bins, counts, _ = bin_files(deposition, directory, num_files, "deposition")
    deposition.close()
    context.close()
    write_bins(os.path.join(directory, "bins.nc"), bins, *edges, **counts)
    return bins, counts
