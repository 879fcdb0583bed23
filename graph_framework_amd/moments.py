"""Moments of the particles of a push per flux surface, on the device and exact: the density, the parallel current
j_par(s), the kinetic energy and the synchrotron-radiated power, the profiles a runaway-electron run is reported by.

A FluxMoments labels every particle with flux.py's label, evaluates the EFIT field B = (psi_z/R, fpol/R, -psi_R/R) once,
in the fixed arithmetic of csrc/flux_label.hpp, and forms

    m = (1, v_par/c = ((u.B)/|B|)/gamma, gamma - 1, |B|^2 u_perp^2)            MOMENTS

It adds w*m[k] (w: the particle's weight, 1 without one) to the superaccumulator of cell (is, k) of the particle's flux
surface `is` (csrc/moment_bins.hip), all four or, where one of them is NaN or infinite, none: the four moments are
always sums over the same particles, and `skipped` counts the others.  The particles stay where the push keeps them, fp32
or fp64: Korc.bin(moments) bins them on the push's own stream, Korc.bin(moments, weight=confinement.alive_key) the confined
ones only.  The state, shape (ns, 4, 67), is the same bytes with and without the workgroup-private sums, for fp32 and fp64
columns of equal values and for any order of particles or shards.

The moments are in the push's normalised units (u = gamma*beta, energies in m c^2, B as the tables hold it): no physical
constants are applied.  A cell holds edge[i] <= label < edge[i+1].
"""
import ctypes

import numpy as np

from .backend import GfHipError, key_of
from .batches import ratio_error_of
from .exact_cells import LIMBS, RayBatches
from .flux import FluxProfile, _Info, flux_map
from .spectrum import _keys, spectrum_field

MOMENTS = ("density", "current", "energy", "radiation")


def _host_columns(columns, weight=None):
    """The seven columns (and the weight) as contiguous arrays of one type, float32 only if all of them are."""
    columns = [np.asarray(column) for column in columns]
    if len(columns) != 7:
        raise ValueError("%d columns where 7 are needed" % len(columns))
    if weight is not None:
        columns.append(np.asarray(weight))
    is_f32 = all(column.dtype == np.float32 for column in columns)
    columns = [np.ascontiguousarray(column, dtype=np.float32 if is_f32 else np.float64).reshape(-1) for column in columns]
    if len({column.size for column in columns}) != 1:
        raise ValueError("the columns differ in length")
    return columns, is_f32


def values_host(tables, columns, psi0=None, span=None, sqrt_label=False):
    """(label (n,), values (n, 4)) of particles on the CPU (gfhip_moments_values_host): the bits of FluxMoments.values,
    NaN off the map.  columns: x, y, z, ux, uy, uz, gamma, all float32 or all float64 (anything else is taken as
    float64)."""
    from . import _lib
    lib = _lib.load()
    given, keep = flux_map(tables, psi0, span, sqrt_label)
    field, keep_field = spectrum_field(tables)
    columns, is_f32 = _host_columns(columns)
    pointers = (ctypes.c_void_p*7)(*[column.ctypes.data for column in columns])
    label = np.empty(columns[0].size, dtype=np.float64)
    values = np.empty((columns[0].size, len(MOMENTS)), dtype=np.float64)
    if lib.gfhip_moments_values_host(ctypes.byref(given), ctypes.byref(field), pointers, int(is_f32), label.size,
                                     label.ctypes.data, values.ctypes.data):
        raise GfHipError(lib.gfhip_last_error(None).decode())
    del keep, keep_field
    return label, values


def add_host(tables, sedges, columns, weight=None, limbs=None, counters=None, psi0=None, span=None, sqrt_label=False):
    """The exact deposit on the CPU (gfhip_moments_add_host), the bytes and numbers of FluxMoments.state() and counts()
    after the same particles: (limbs (ns, 4, 67) int64, counters (3,) uint64: samples, outside, skipped).  Given `limbs`
    and `counters` (contiguous, of those types) the particles are added to them in place."""
    from . import _lib
    lib = _lib.load()
    given, keep = flux_map(tables, psi0, span, sqrt_label)
    field, keep_field = spectrum_field(tables)
    sedges = np.ascontiguousarray(sedges, dtype=np.float64).reshape(-1)
    if sedges.size < 2:
        raise ValueError("a moment profile needs at least two edges")
    shape = (sedges.size - 1, len(MOMENTS), LIMBS)
    if limbs is None:
        limbs, counters = np.zeros(shape, dtype=np.int64), np.zeros(3, dtype=np.uint64)
    for name, array, kind, want in (("limbs", limbs, np.int64, shape), ("counters", counters, np.uint64, (3,))):
        if not isinstance(array, np.ndarray) or array.dtype != kind or array.shape != want or not array.flags["C_CONTIGUOUS"]:
            raise ValueError("%s must be a contiguous %s array of shape %r: it is updated in place" % (name, np.dtype(kind).name, want))
    columns, is_f32 = _host_columns(columns, weight)
    pointers = (ctypes.c_void_p*8)(*[column.ctypes.data for column in columns])
    if lib.gfhip_moments_add_host(ctypes.byref(given), ctypes.byref(field), sedges.ctypes.data, sedges.size - 1, pointers,
                                  int(is_f32), columns[0].size, limbs.ctypes.data, counters.ctypes.data):
        raise GfHipError(lib.gfhip_last_error(None).decode())
    del keep, keep_field
    return limbs, counters


def add_particles_host(tables, sedges, batches, columns, first, weight=None, limbs=None, counters=None, psi0=None, span=None,
                       sqrt_label=False):
    """add_host per batch of particles (gfhip_moments_add_particles_host): particle i of the columns is particle first + i
    of the ensemble.  (limbs (batches, ns, 4, 67) int64, counters (3,) uint64), the bytes and numbers of a FluxMoments
    with batches after the same add_particles; given `limbs` and `counters`, added to in place."""
    from . import _lib
    lib = _lib.load()
    given, keep = flux_map(tables, psi0, span, sqrt_label)
    field, keep_field = spectrum_field(tables)
    sedges = np.ascontiguousarray(sedges, dtype=np.float64).reshape(-1)
    if sedges.size < 2:
        raise ValueError("a moment profile needs at least two edges")
    shape = (int(batches), sedges.size - 1, len(MOMENTS), LIMBS)
    if limbs is None:
        limbs, counters = np.zeros(shape, dtype=np.int64), np.zeros(3, dtype=np.uint64)
    for name, array, kind, want in (("limbs", limbs, np.int64, shape), ("counters", counters, np.uint64, (3,))):
        if not isinstance(array, np.ndarray) or array.dtype != kind or array.shape != want or not array.flags["C_CONTIGUOUS"]:
            raise ValueError("%s must be a contiguous %s array of shape %r: it is updated in place" % (name, np.dtype(kind).name, want))
    columns, is_f32 = _host_columns(columns, weight)
    pointers = (ctypes.c_void_p*8)(*[column.ctypes.data for column in columns])
    if lib.gfhip_moments_add_particles_host(ctypes.byref(given), ctypes.byref(field), sedges.ctypes.data, sedges.size - 1,
                                            int(batches), pointers, int(is_f32), columns[0].size, int(first), limbs.ctypes.data,
                                            counters.ctypes.data):
        raise GfHipError(lib.gfhip_last_error(None).decode())
    del keep, keep_field
    return limbs, counters


class FluxMoments(RayBatches):
    """Exact sums of the four MOMENTS per flux surface on a context's device (gfhip_moments_*, include/gf_hip.h); state()
    is (ns, 4, 67), read() (ns, 4).  batches=G: the same sums per batch of particles (batches.py, the particle's index in
    the ensemble in place of a ray's), state() (G, ns, 4, 67), fed with add_particles; total() is the plain profile,
    standard_error() the error bar of its cells and means_error() that of means()."""
    prefix = "moments"

    def __init__(self, context, tables, sedges, psi0=None, span=None, sqrt_label=False, private=True, batches=None):
        self.tables = tables
        self.sedges = np.ascontiguousarray(sedges, dtype=np.float64).reshape(-1)
        if self.sedges.size < 2:
            raise ValueError("a moment profile needs at least two edges")
        self.sqrt_label = bool(sqrt_label)
        self.private = bool(private)
        given, keep = flux_map(tables, psi0, span, sqrt_label, private)
        field, keep_field = spectrum_field(tables)
        self.psi0, self.span = given.psi0, given.span
        self._created_cells(context, batches, (self.sedges.size - 1, len(MOMENTS)), ctypes.byref(given), ctypes.byref(field),
                            self.sedges.ctypes.data, self.sedges.size - 1)
        del keep, keep_field                                 # the library has copied the tables

    def _twin(self, context, batches, sedges=None):
        return FluxMoments(context, self.tables, self.sedges if sedges is None else sedges, self.psi0, self.span,
                           self.sqrt_label, self.private, batches)

    def like(self, context, sedges=None):
        """An empty twin with this one's map, options and batches on another context (or on other label edges)."""
        return self._twin(context, self.batches, sedges)

    @property
    def label_kind(self):
        return "sqrt_s" if self.sqrt_label else "s"

    def add(self, x, y, z, ux, uy, uz, gamma, count, weight=None):
        """Bin `count` particles of seven context buffers, all fp32 or all fp64, each with the weight of an eighth buffer
        of the same type or with 1.0; asynchronous on the context's stream.  The signature is PhaseDistribution.add's, so
        Korc.bin(moments, weight=...) bins the push's particles where they lie."""
        keys = _keys((x, y, z, ux, uy, uz, gamma), 7)
        self.context._check(self.lib.gfhip_moments_add(self.handle, keys, 0 if weight is None else key_of(weight),
                                                       int(weight is not None), int(count)))

    def add_particles(self, x, y, z, ux, uy, uz, gamma, count, first, weight=None):
        """add() for a profile with batches: particle i of the buffers is particle first + i of the whole ensemble."""
        keys = _keys((x, y, z, ux, uy, uz, gamma), 7)
        self.context._check(self.lib.gfhip_moments_add_particles(self.handle, keys, 0 if weight is None else key_of(weight),
                                                                 int(weight is not None), int(count), int(first)))

    def values(self, x, y, z, ux, uy, uz, gamma, label_key, values_key, count):
        """The labels of `count` particles into the fp64 buffer `label_key` and their four moments into the fp64 buffer
        `values_key` (4*count, [particle][k]), NaN off the map; asynchronous."""
        keys = _keys((x, y, z, ux, uy, uz, gamma), 7)
        self.context._check(self.lib.gfhip_moments_values(self.handle, keys, key_of(label_key), key_of(values_key), int(count)))

    def totals(self):
        """(4,): the exact marginal over the surfaces, the ns slices state()[s] merged into a one-surface twin on the
        first and the last edge and rounded once."""
        with self._plain() as plain:
            state = plain.state()
        twin = self._twin(self.context, None, self.sedges[[0, -1]])
        try:
            for s in range(state.shape[0]):
                twin.merge(state[s:s + 1])
            return twin.read()[0]
        finally:
            twin.close()

    def profile(self, context=None):
        """A FluxProfile on the label edges (on `context`, this object's by default) that holds moment 0, the weight per
        surface, with this object's counts: with skipped == 0 the bytes of a FluxProfile fed the same particles and
        weights."""
        marginal = FluxProfile(context or self.context, self.tables, self.sedges, self.psi0, self.span, self.sqrt_label,
                               self.private)
        with self._plain() as plain:
            marginal.merge(plain.state()[:, 0, :], **plain.counts())
        return marginal

    def means(self):
        """(ns, 3): current, energy and radiation per unit of weight, read()[:, 1:]/read()[:, :1]; NaN where empty."""
        with self._plain() as plain:
            bins = plain.read()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(bins[:, :1] == 0.0, np.nan, bins[:, 1:]/bins[:, :1])

    def means_error(self):
        """(ns, 3): the standard error of means() of a profile with batches, the delete-one-batch jackknife of the ratio
        of current, energy and radiation to the density (batches.ratio_error_of); NaN with fewer than two batches that
        reached the surface."""
        self._batched("means_error()")
        sums = self.read()
        return np.stack([ratio_error_of(sums[:, :, k], sums[:, :, 0]) for k in (1, 2, 3)], axis=1)

    def volumes(self, sub=16):
        """The volumes in m^3 of a FluxProfile on the same edges (FluxProfile.volumes)."""
        shells = FluxProfile(self.context, self.tables, self.sedges, self.psi0, self.span, self.sqrt_label, self.private)
        try:
            return shells.volumes(sub)[0]
        finally:
            shells.close()

    def densities(self, sub=16):
        """(ns, 4): read()/volume per surface, the number density, j_par(s), the energy density and the radiated power
        density; NaN where no quadrature point reached the cell."""
        volume = self.volumes(sub)[:, None]
        with self._plain() as plain:
            bins = plain.read()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(volume == 0.0, np.nan, bins/volume)

    def info(self):
        """How deposits are launched: {private_sums, workgroup_size, cap_cells, max_workgroups, lds_bytes}."""
        info = _Info()
        self.context._check(self.lib.gfhip_moments_info(self.handle, ctypes.byref(info)))
        out = {name: int(getattr(info, name)) for name, _ in _Info._fields_}
        out["private_sums"] = bool(out["private_sums"])
        return out
