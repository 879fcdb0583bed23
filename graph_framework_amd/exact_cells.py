"""What a deposition grid (deposition.py), a flux profile (flux.py) and a spectrum (spectrum.py) share: a store of exact
sums on a context's device, cells x 67 limbs of csrc/superacc.hpp and three counters, behind gfhip_bins_*, gfhip_flux_*
or gfhip_spectrum_* (include/gf_hip.h).
They differ in how a sample finds its cell, which is the constructor's business."""
import ctypes
import os

import numpy as np

from .backend import GfHipError, key_of
from .output import ResultFile

LIMBS = 67


class ExactCells:
    """add, counts, state, read and close of a handle made by gfhip_<prefix>_create.  A subclass sets `prefix` and, in its
    constructor, `context`, `shape` (of the cells) and `handle` (through `_created`)."""
    prefix = None

    def _call(self, name):
        return getattr(self.context.lib, "gfhip_%s_%s" % (self.prefix, name))

    def _created(self, context, shape, *arguments):
        self.context = context
        self.lib = context.lib
        self.shape = tuple(shape)
        self.handle = self._call("create")(context.handle, *arguments)
        if not self.handle:
            raise GfHipError(self.lib.gfhip_last_error(context.handle).decode())

    def add(self, x_key, y_key, z_key, value_key, count):
        """Bin `count` samples of four fp64 context buffers; asynchronous on the context's stream."""
        self.context._check(self._call("add")(self.handle, key_of(x_key), key_of(y_key), key_of(z_key), key_of(value_key),
                                              int(count)))

    def counts(self):
        """{samples, outside, skipped}: the samples seen, those that fell in no cell (off the grid, off the map, a NaN
        coordinate or label) and those inside whose value was NaN or infinite."""
        values = [ctypes.c_uint64() for _ in range(3)]
        self.context._check(self._call("counts")(self.handle, *[ctypes.byref(v) for v in values]))
        return dict(zip(("samples", "outside", "skipped"), (v.value for v in values)))

    def state(self):
        """The canonical limbs, shape + (67,): identical bytes for the same samples in any order and by any route."""
        limbs = np.empty(self.shape + (LIMBS,), dtype=np.int64)
        self.context._check(self._call("state")(self.handle, limbs.ctypes.data))
        return limbs

    def read(self, divisor=1.0):
        """shape: the correctly rounded exact sum of each cell, divided by `divisor`."""
        bins = np.empty(self.shape, dtype=np.float64)
        self.context._check(self._call("read")(self.handle, float(divisor), bins.ctypes.data))
        return bins

    def close(self):
        if self.handle and self.context.handle:              # a closed context has freed its grids and profiles
            self._call("destroy")(self.handle)
        self.handle = None


def bin_files(grid, directory, num_files, tag, names=("x", "y", "z", "d_power")):
    """d_power of <directory>/result0.nc .. result<num_files - 1>.nc binned into `grid` (an ExactCells) through buffers
    `<tag>_<name>_<rays>` of its context: (bins divided by the total number of rays, counts, that total).  names: the
    file's variables that grid.add takes, in its order."""
    from . import _lib
    context = grid.context
    total = 0
    for number in range(num_files):
        file = ResultFile(os.path.join(directory, "result%d.nc" % number))
        n = file.num_rays
        total += n                                           # bin.py:104
        keys = ["%s_%s_%d" % (tag, name, n) for name in names]          # one set of buffers per ensemble size
        for key in keys:
            context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), n, _lib.GFIR_F64))
        for record in range(file.records):
            for name, key in zip(names, keys):
                context.copy_to_device(key, file.read(name, record))
            grid.add(*keys, n)
        file.close()
    return grid.read(total), grid.counts(), total
