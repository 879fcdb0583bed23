"""Deposition profiles: what utilities/bin.py computes from result<n>.nc, on the device and exact.

bin.py sums `d_power` over nx*ny*nz boolean masks of every sample (TensorFlow) and divides by the number of
rays.  Here every cell of the grid is an integer superaccumulator (csrc/superacc.hpp) fed by the deposit
kernel of csrc/deposition.hip: a cell holds the exact sum of its samples, rounded once when it is read, so
the profile does not depend on the order of the samples, on the split into records, files or ranks, or on
the run.  The cell rule is bin.py's: edge[i] <= c < edge[i+1] on each axis, against the edges that are
written to bins.nc.
"""
import ctypes
import os

import numpy as np

from .backend import GfHipError, key_of
from .output import ResultFile, write_bins

LIMBS = 67


class Deposition:
    """A 3-D grid of exact sums on a context's device (gfhip_bins_*, include/gf_hip.h)."""

    def __init__(self, context, xedges, yedges, zedges):
        self.context = context
        self.lib = context.lib
        self.edges = [np.ascontiguousarray(e, dtype=np.float64).reshape(-1) for e in (xedges, yedges, zedges)]
        if any(e.size < 2 for e in self.edges):
            raise ValueError("an axis needs at least two edges")
        self.shape = tuple(e.size - 1 for e in self.edges)
        arguments = []
        for e in self.edges:
            arguments += [e.ctypes.data, e.size - 1]
        self.handle = self.lib.gfhip_bins_create(context.handle, *arguments)
        if not self.handle:
            raise GfHipError(self.lib.gfhip_last_error(context.handle).decode())

    def add(self, x_key, y_key, z_key, value_key, count):
        """Bin `count` samples of four fp64 context buffers; asynchronous on the context's stream."""
        self.context._check(self.lib.gfhip_bins_add(self.handle, key_of(x_key), key_of(y_key), key_of(z_key),
                                                    key_of(value_key), int(count)))

    def counts(self):
        """{samples, outside, skipped}: the samples seen, those that fell outside the grid (or had a NaN coordinate)
        and those inside whose value was NaN or infinite."""
        values = [ctypes.c_uint64() for _ in range(3)]
        self.context._check(self.lib.gfhip_bins_counts(self.handle, *[ctypes.byref(v) for v in values]))
        return dict(zip(("samples", "outside", "skipped"), (v.value for v in values)))

    def state(self):
        """The canonical limbs, shape (nx, ny, nz, 67): identical bytes for the same samples in any order."""
        limbs = np.empty(self.shape + (LIMBS,), dtype=np.int64)
        self.context._check(self.lib.gfhip_bins_state(self.handle, limbs.ctypes.data))
        return limbs

    def merge(self, limbs, samples=0, outside=0, skipped=0):
        """Add another grid's state() and counts() (same edges)."""
        limbs = np.ascontiguousarray(limbs, dtype=np.int64)
        if limbs.shape != self.shape + (LIMBS,):
            raise ValueError("merge: limbs of shape %r for a grid of %r" % (limbs.shape, self.shape))
        self.context._check(self.lib.gfhip_bins_merge(self.handle, limbs.ctypes.data, int(samples), int(outside), int(skipped)))

    def read(self, divisor=1.0):
        """(nx, ny, nz): the correctly rounded exact sum of each cell, divided by `divisor`."""
        bins = np.empty(self.shape, dtype=np.float64)
        self.context._check(self.lib.gfhip_bins_read(self.handle, float(divisor), bins.ctypes.data))
        return bins

    def close(self):
        if self.handle and self.context.handle:              # a closed context has freed its grids
            self.lib.gfhip_bins_destroy(self.handle)
        self.handle = None


def bin_deposition(directory, num_files, num_x, min_x, max_x, num_y, min_y, max_y, num_z, min_z, max_z, index=0):
    """utilities/bin.py's main(): d_power of result0.nc .. result<num_files - 1>.nc binned on the grid, divided by the
    total number of rays, written to <directory>/bins.nc.  Returns (bins, counts)."""
    from .backend import Context
    from . import _lib
    edges = [np.linspace(low, high, n + 1) for low, high, n in ((min_x, max_x, num_x), (min_y, max_y, num_y), (min_z, max_z, num_z))]
    context = Context(index)
    deposition = Deposition(context, *edges)
    names = ("x", "y", "z", "d_power")
    total = 0
    for number in range(num_files):
        file = ResultFile(os.path.join(directory, "result%d.nc" % number))
        n = file.num_rays
        total += n                                           # bin.py:104
        keys = ["deposition_%s_%d" % (name, n) for name in names]      # one set of buffers per ensemble size
        for key in keys:
            context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), n, _lib.GFIR_F64))
        for record in range(file.records):
            for name, key in zip(names, keys):
                context.copy_to_device(key, file.read(name, record))
            deposition.add(*keys, n)
        file.close()
    bins = deposition.read(total)
    counts = deposition.counts()
    deposition.close()
    context.close()
    write_bins(os.path.join(directory, "bins.nc"), bins, *edges, **counts)
    return bins, counts
