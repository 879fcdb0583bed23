"""What a deposition grid (deposition.py), a flux profile (flux.py) and a spectrum (spectrum.py) share: a store of exact
sums on a context's device, cells x 67 limbs of csrc/superacc.hpp and three counters, behind gfhip_bins_*, gfhip_flux_*
or gfhip_spectrum_* (include/gf_hip.h).
They differ in how a sample finds its cell, which is the constructor's business."""
import contextlib
import ctypes
import os

import numpy as np

from .backend import GfHipError, key_of
from .batches import batch_rays, standard_error_of
from .output import ResultFile

LIMBS = 67


class ExactCells:
    """add, counts, state, read and close of a handle made by gfhip_<prefix>_create.  A subclass sets `prefix` and, in its
    constructor, `context`, `shape` (of the cells) and `handle` (through `_created`)."""
    prefix = None

    def _call(self, name):
        return getattr(self.context.lib, "gfhip_%s_%s" % (self.prefix, name))

    def _created(self, context, shape, *arguments, create="create"):
        self.context = context
        self.lib = context.lib
        self.shape = tuple(shape)
        self.handle = self._call(create)(context.handle, *arguments)
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


class RayBatches(ExactCells):
    """What a flux profile and a spectrum with batches=G add to ExactCells (batches.py, csrc/ray_batches.hpp): the state
    is batch-major, shape (G,) + the cells', slab g that of the samples of batch g's rays.  A subclass sets `batches`
    (None: no batches) and `cell_shape` before `_created`, and has `_twin(context, batches)`.  A distribution and a
    moment profile of particles (distribution.py, moments.py) keep batches of particles the same way: read `particle`
    for `ray` below, the particle's index in the whole ensemble."""
    batches = None

    def _created_cells(self, context, batches, cell_shape, *arguments):
        """`_created` of a plain object, or of a batched one: gfhip_<prefix>_create_batched with the batches last."""
        self.batches = None if batches is None else int(batches)
        self.cell_shape = tuple(cell_shape)
        if self.batches is None:
            self._created(context, self.cell_shape, *arguments)
        else:
            self._created(context, (self.batches,) + self.cell_shape, *arguments, self.batches, create="create_batched")

    def like(self, context):
        """An empty twin with this one's map, edges, options and batches on another context."""
        return self._twin(context, self.batches)

    def _batched(self, what):
        if self.batches is None:
            raise ValueError("%s needs an object made with batches" % what)

    def merge(self, limbs, samples=0, outside=0, skipped=0):
        """Add another object's state() and counts() (same map and edges: the caller's business); another shape, the
        number of batches included, is refused."""
        limbs = np.ascontiguousarray(limbs, dtype=np.int64)
        if limbs.ndim != len(self.shape) + 1 or limbs.shape[-1] != LIMBS:
            raise ValueError("merge: limbs of shape %r are no %r state" % (limbs.shape, self.shape + (LIMBS,)))
        name = "merge" if self.batches is None else "merge_batches"
        self.context._check(self._call(name)(self.handle, limbs.ctypes.data, *limbs.shape[:-1], int(samples), int(outside),
                                             int(skipped)))

    def total(self, context=None):
        """A twin without batches (on `context`, this object's by default) that holds the marginal over the batches: the
        G slabs merged into it, which is exact.  Its state and counts are those of a plain object fed every sample."""
        self._batched("total()")
        marginal = self._twin(context or self.context, None)
        state = self.state()
        counts = self.counts()
        for g in range(self.batches):
            marginal.merge(state[g], **(counts if g == 0 else {}))
        return marginal

    @contextlib.contextmanager
    def _plain(self):
        """This object, or, of one with batches, its total() for the length of the block."""
        marginal = self if self.batches is None else self.total()
        try:
            yield marginal
        finally:
            if marginal is not self:
                marginal.close()

    def batch_rays(self, first, count):
        """int64[batches]: the rays of [first, first + count) in every batch."""
        self._batched("batch_rays()")
        return batch_rays(first, count, self.batches)

    def standard_error(self, first, count):
        """(mean, stderr, used) of the cells over the rays [first, first + count) that were fed: the mean per ray, its
        standard error from the spread of the batch means (batches.standard_error_of) and the number of batches with
        rays; stderr is NaN with fewer than two."""
        self._batched("standard_error()")
        marginal = self.total()
        try:
            total = marginal.read()
        finally:
            marginal.close()
        return standard_error_of(self.read(), total, self.batch_rays(first, count), count)

    def batch_means(self, first, count):
        """(batches,) + cells: every batch's sum per ray of the batch, NaN for a batch without rays."""
        rays = self.batch_rays(first, count).astype(np.float64).reshape((-1,) + (1,)*len(self.cell_shape))
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(rays > 0.0, self.read()/rays, np.nan)

    def error_variables(self, first, count):
        """The keywords of write_flux_bins and write_spectrum_bins for the batch statistics of the rays [first, first +
        count): stderr, batch_bins (the batch means) and batch_rays."""
        _, stderr, _ = self.standard_error(first, count)
        return dict(stderr=stderr, batch_bins=self.batch_means(first, count), batch_rays=self.batch_rays(first, count))


    def sum_error_variables(self, first, count):
        """The keywords of write_phase_bins and write_moment_bins for the batch statistics of the particles [first,
        first + count), for files whose bins are sums over the particles, not means: stderr, `count` times the standard
        error of the mean per particle; batch_bins, the batch means; batch_particles."""
        _, stderr, _ = self.standard_error(first, count)
        return dict(stderr=float(count)*stderr, batch_bins=self.batch_means(first, count),
                    batch_particles=self.batch_rays(first, count))


def bin_files(grid, directory, num_files, tag, names=("x", "y", "z", "d_power"), first_ray=0):
    """d_power of <directory>/result0.nc .. result<num_files - 1>.nc binned into `grid` (an ExactCells) through buffers
    `<tag>_<name>_<rays>` of its context: (bins divided by the total number of rays, counts, that total).  names: the
    file's variables that grid.add takes, in its order.  A grid with batches takes every record through add_rays: the
    rays of result0.nc are first_ray .., those of the next file follow on, and the bins keep the batch axis."""
    from . import _lib
    batched = getattr(grid, "batches", None) is not None
    context = grid.context
    total = 0
    for number in range(num_files):
        file = ResultFile(os.path.join(directory, "result%d.nc" % number))
        n = file.num_rays
        first = first_ray + total                            # the file's first ray in the ensemble
        total += n                                           # bin.py:104
        keys = ["%s_%s_%d" % (tag, name, n) for name in names]          # one set of buffers per ensemble size
        for key in keys:
            context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), n, _lib.GFIR_F64))
        for record in range(file.records):
            for name, key in zip(names, keys):
                context.copy_to_device(key, file.read(name, record))
            if batched:
                grid.add_rays(*keys, n, first)
            else:
                grid.add(*keys, n)
        file.close()
    return grid.read(total), grid.counts(), total
