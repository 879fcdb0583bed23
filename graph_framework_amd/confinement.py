"""First-exit tracking of the particles of a push, on the device: the confined fraction over time, the energy spectrum of
the lost particles and the footprint of the losses in the poloidal plane.

A Confinement belongs to one push (korc.py) and lives on its context and stream.  It keeps, per particle, the step at
which the particle was first found outside (lost_steps(), 0xFFFFFFFF while confined) and `alive`, a context buffer of the
push's type under the key `alive_key` that is 1 while the particle is confined and 0 afterwards: a weight column for
Korc.bin, so that lost particles drop out of the snapshots.  check() examines the particles that are still confined:

    label = the flux label of (x, y, z) in the fixed arithmetic of csrc/flux_label.hpp, NaN off the map
    lost  iff  not (label < limit)        off the map, a NaN position and label == limit are all lost

A particle found lost is settled once and never looked at again, even if a later step carries it back inside.  It
leaves its weight (1 without a weight column) in the exact cell (ir, iz, ig) of (R, z, gamma) (csrc/confinement.hip), and
R and z in the exit buffers where the caller gave them.  The state, shape (nr, nz, ng, 67), is the same bytes for fp32 and
fp64 columns of equal values and for any order of particles or shards.  A cell holds edge[i] <= c < edge[i+1].
"""
import ctypes

import numpy as np

from .backend import GfHipError, key_of
from .exact_cells import LIMBS, ExactCells
from .flux import _Info, flux_map
from .spectrum import _keys

CONFINED = 0xFFFFFFFF
_DTYPES = {"f32": np.float32, "f64": np.float64}


def _dtype_of(dtype):
    dtype = _DTYPES.get(dtype, dtype)
    if np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("a confinement tracker follows fp32 or fp64 particles")
    return np.dtype(dtype)


def check_host(tables, columns, step, lost_step, alive, limit=1.0, weight=None, exit=None, edges=None, limbs=None,
               counters=None, psi0=None, span=None, sqrt_label=False):
    """One check on the CPU (gfhip_confine_check_host), the bits of Confinement.check: `lost_step` (uint32) and `alive` (the
    columns' type) are updated in place, as are exit = (exit_r, exit_z) (float64), and, given edges = (redges, zedges,
    gedges), limbs (nr, nz, ng, 67) (int64) and counters (3, uint64).  columns: x, y, z, ux, uy, uz, gamma, all float32 or
    all float64.  Returns the number of particles found lost."""
    from . import _lib
    lib = _lib.load()
    given, keep = flux_map(tables, psi0, span, sqrt_label)
    if len(columns) != 7:
        raise ValueError("%d columns where 7 are needed" % len(columns))
    dtype = alive.dtype
    for name, array, kind in (("lost_step", lost_step, np.uint32), ("alive", alive, dtype)) + \
            ((("exit_r", exit[0], np.float64), ("exit_z", exit[1], np.float64)) if exit is not None else ()) + \
            ((("limbs", limbs, np.int64), ("counters", counters, np.uint64)) if limbs is not None else ()):
        if not isinstance(array, np.ndarray) or array.dtype != kind or not array.flags["C_CONTIGUOUS"]:
            raise ValueError("%s must be a contiguous %s array: it is updated in place" % (name, np.dtype(kind).name))
    if dtype not in (np.float32, np.float64):
        raise ValueError("alive must be float32 or float64, the columns' type")
    columns = [np.ascontiguousarray(column, dtype=dtype).reshape(-1) for column in columns]
    if weight is not None:
        columns.append(np.ascontiguousarray(weight, dtype=dtype).reshape(-1))
    count = columns[0].size
    sizes = {column.size for column in columns} | {lost_step.size, alive.size} | ({exit[0].size, exit[1].size} if exit is not None else set())
    if sizes != {count}:
        raise ValueError("the columns, lost_step, alive and the exit arrays differ in length")
    pointers = (ctypes.c_void_p*8)(*[column.ctypes.data for column in columns])
    axes = [None, 0, None, 0, None, 0]
    if limbs is not None:
        edges = [np.ascontiguousarray(e, dtype=np.float64).reshape(-1) for e in edges]
        if limbs.shape != tuple(e.size - 1 for e in edges) + (LIMBS,) or counters.size != 3:
            raise ValueError("limbs of shape %r and %d counters for these edges" % (limbs.shape, counters.size))
        axes = [v for e in edges for v in (e.ctypes.data, e.size - 1)]
    newly = ctypes.c_uint64(0)
    if lib.gfhip_confine_check_host(ctypes.byref(given), float(limit), *axes, pointers, int(dtype == np.float32), count, int(step),
                                    lost_step.ctypes.data, alive.ctypes.data, *([a.ctypes.data for a in exit] if exit is not None else [None, None]),
                                    ctypes.byref(newly), limbs.ctypes.data if limbs is not None else None,
                                    counters.ctypes.data if limbs is not None else None):
        raise GfHipError(lib.gfhip_last_error(None).decode())
    del keep
    return newly.value


class Confinement(ExactCells):
    """A first-exit tracker of `count` particles on a context's device (gfhip_confine_*, include/gf_hip.h); state() is
    the loss footprint, (nr, nz, ng, 67)."""
    prefix = "confine"

    def __init__(self, context, tables, redges, zedges, gedges, count, dtype, limit=1.0, psi0=None, span=None, sqrt_label=False,
                 alive="alive", capacity=4096):
        self.tables = tables
        self.redges, self.zedges, self.gedges = (np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
                                                 for edges in (redges, zedges, gedges))
        if min(self.redges.size, self.zedges.size, self.gedges.size) < 2:
            raise ValueError("a loss footprint needs at least two edges per axis")
        self.count = int(count)
        self.dtype = _dtype_of(dtype)
        self.limit = float(limit)
        self.sqrt_label = bool(sqrt_label)
        self.alive_key = alive
        self.capacity = int(capacity)
        given, keep = flux_map(tables, psi0, span, sqrt_label)
        self.psi0, self.span = given.psi0, given.span
        self._created(context, (self.redges.size - 1, self.zedges.size - 1, self.gedges.size - 1), ctypes.byref(given), self.limit,
                      self.redges.ctypes.data, self.redges.size - 1, self.zedges.ctypes.data, self.zedges.size - 1,
                      self.gedges.ctypes.data, self.gedges.size - 1, self.count, int(self.dtype == np.float32), key_of(alive),
                      self.capacity)
        del keep                                             # the library has copied the tables

    def like(self, context, alive=None, count=None, capacity=None):
        """An empty twin with this one's map, edges, limit and type on another context, or on this one under another
        `alive` key."""
        return Confinement(context, self.tables, self.redges, self.zedges, self.gedges, self.count if count is None else count,
                           self.dtype, self.limit, self.psi0, self.span, self.sqrt_label, self.alive_key if alive is None else alive,
                           self.capacity if capacity is None else capacity)

    @property
    def label_kind(self):
        return "sqrt_s" if self.sqrt_label else "s"

    def check(self, x, y, z, ux, uy, uz, gamma, step, weight=None, exit=None):
        """Examine the confined particles of seven context buffers of the tracker's type at step number `step` (not below
        the previous check's); weight: an eighth buffer of the same type; exit: the keys of two fp64 buffers (exit_r,
        exit_z).  Asynchronous on the context's stream."""
        keys = _keys((x, y, z, ux, uy, uz, gamma), 7)
        step = int(step)
        if not 0 <= step <= CONFINED:
            raise ValueError("a step number is a uint32")
        exit_r, exit_z = (0, 0) if exit is None else (key_of(key) for key in exit)
        self.context._check(self.lib.gfhip_confine_check(self.handle, keys, 0 if weight is None else key_of(weight),
                                                         int(weight is not None), exit_r, exit_z, int(exit is not None), step))

    def add(self, *arguments, **keywords):
        raise TypeError("a confinement tracker takes its particles through check()")

    def lost_steps(self):
        """uint32[count]: the step of the check that found each particle lost, CONFINED (0xFFFFFFFF) while confined."""
        out = np.empty(self.count, dtype=np.uint32)
        self.context._check(self.lib.gfhip_confine_lost_steps(self.handle, out.ctypes.data))
        return out

    def history(self):
        """{steps, newly_lost, confined}: per check its step, the particles it found lost and those confined after it."""
        steps = np.empty(self.capacity, dtype=np.uint32)
        newly = np.empty(self.capacity, dtype=np.uint64)
        checks = ctypes.c_size_t()
        self.context._check(self.lib.gfhip_confine_history(self.handle, steps.ctypes.data, newly.ctypes.data, ctypes.byref(checks)))
        steps, newly = steps[:checks.value].copy(), newly[:checks.value].astype(np.int64)
        return dict(steps=steps, newly_lost=newly, confined=self.count - np.cumsum(newly))

    def confined(self):
        """The number of particles still confined after the last check."""
        return self.count - int(self.history()["newly_lost"].sum())

    def merge(self, limbs, samples=0, outside=0, skipped=0):
        """Add another tracker's state() and counts() (same map and edges: the caller's business); another shape is
        refused.  The per-particle arrays and the history are not merged: they belong to a tracker's own particles."""
        limbs = np.ascontiguousarray(limbs, dtype=np.int64)
        if limbs.ndim != 4 or limbs.shape[-1] != LIMBS:
            raise ValueError("merge: limbs of shape %r are no %r state" % (limbs.shape, self.shape + (LIMBS,)))
        self.context._check(self.lib.gfhip_confine_merge(self.handle, limbs.ctypes.data, *limbs.shape[:-1], int(samples),
                                                         int(outside), int(skipped)))

    def _marginal(self, axes, slices):
        """read() of a one-particle twin on the edges `axes` into which `slices` of the state were merged, which is
        exact."""
        twin = Confinement(self.context, self.tables, *axes, 1, self.dtype, self.limit, self.psi0, self.span, self.sqrt_label,
                           "%s_marginal" % (self.alive_key,), 1)
        try:
            for part in slices:
                twin.merge(part)
            return twin.read()
        finally:
            twin.close()

    def footprint(self):
        """(nr, nz): the exact marginal over gamma, the ng slices state()[:, :, g] merged and rounded once."""
        state = self.state()
        ends = self.gedges[[0, -1]]
        return self._marginal((self.redges, self.zedges, ends), (state[:, :, g:g + 1] for g in range(self.shape[2])))[:, :, 0]

    def spectrum(self):
        """(ng,): the exact marginal over R and z, the nr*nz slices state()[r, z] merged and rounded once."""
        state = self.state()
        axes = (self.redges[[0, -1]], self.zedges[[0, -1]], self.gedges)
        return self._marginal(axes, (state[r:r + 1, z:z + 1] for r in range(self.shape[0]) for z in range(self.shape[1])))[0, 0]

    def info(self):
        """How checks are launched: {private_sums (always False), workgroup_size, cap_cells, max_workgroups, lds_bytes}."""
        info = _Info()
        self.context._check(self.lib.gfhip_confine_info(self.handle, ctypes.byref(info)))
        out = {name: int(getattr(info, name)) for name, _ in _Info._fields_}
        out["private_sums"] = bool(out["private_sums"])
        return out
