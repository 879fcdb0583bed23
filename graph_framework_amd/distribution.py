"""Particle distributions over the flux label, the pitch cosine and gamma, f(psi, xi, gamma), on the device and exact.

A runaway-electron push (korc.py) is read through its distribution function: how many particles sit on which flux
surface, at which pitch to the field and at which energy.  A PhaseDistribution labels every particle with flux.py's
label and with xi = (u.B)/(|u||B|) from the EFIT field direction B = (psi_z/R, fpol/R, -psi_R/R), in the fixed arithmetic
of csrc/flux_label.hpp, takes gamma as it is, finds the three cells by the rule of the 3-D grid and adds the particle's
weight (1 without one) to the superaccumulator of cell (is, ip, ig) (csrc/phase_bins.hip).  The particles stay where the
push keeps them, fp32 or fp64: Korc.bin(distribution) bins them on the push's own stream.  The state, shape
(ns, np, ng, 67), is the same bytes with and without the workgroup-private sums, for fp32 and fp64 columns of equal
values and for any order of particles or shards; summed over pitch and gamma it is the flux profile's.

A cell holds edge[i] <= c < edge[i+1], so the last edge of an axis is outside it.  xi = 1 is a value particles have (the
quotient is clamped to [-1, 1]): pitch_edges(n) therefore ends just above 1.  Edges of the caller's own are taken as
they are.
"""
import ctypes

import numpy as np

from .backend import GfHipError, key_of
from .exact_cells import LIMBS, RayBatches
from .flux import FluxProfile, _Info, flux_map
from .spectrum import _keys, spectrum_field

PARTICLE_NAMES = ("x", "y", "z", "ux", "uy", "uz", "gamma")


def pitch_edges(n):
    """n uniform cells of the pitch cosine that hold every xi in [-1, 1]: linspace(-1, 1, n + 1) with the last edge
    replaced by nextafter(1, 2), since a value equal to an axis' last edge is outside it."""
    edges = np.linspace(-1.0, 1.0, int(n) + 1)
    edges[-1] = np.nextafter(1.0, 2.0)
    return edges


def coordinates_host(tables, columns, psi0=None, span=None, sqrt_label=False):
    """(label, xi) of particles on the CPU (gfhip_phase_coordinates_host): the bits of PhaseDistribution.coordinates,
    NaN off the map.  columns: x, y, z, ux, uy, uz, gamma, all float32 or all float64 (anything else is taken as
    float64)."""
    from . import _lib
    lib = _lib.load()
    given, keep = flux_map(tables, psi0, span, sqrt_label)
    field, keep_field = spectrum_field(tables)
    columns = [np.asarray(column) for column in columns]
    if len(columns) != 7:
        raise ValueError("%d columns where 7 are needed" % len(columns))
    is_f32 = all(column.dtype == np.float32 for column in columns)
    columns = [np.ascontiguousarray(column, dtype=np.float32 if is_f32 else np.float64).reshape(-1) for column in columns]
    if len({column.size for column in columns}) != 1:
        raise ValueError("the seven columns differ in length")
    pointers = (ctypes.c_void_p*7)(*[column.ctypes.data for column in columns])
    label = np.empty(columns[0].size, dtype=np.float64)
    pitch = np.empty(columns[0].size, dtype=np.float64)
    if lib.gfhip_phase_coordinates_host(ctypes.byref(given), ctypes.byref(field), pointers, int(is_f32), label.size,
                                        label.ctypes.data, pitch.ctypes.data):
        raise GfHipError(lib.gfhip_last_error(None).decode())
    del keep, keep_field
    return label, pitch


def add_particles_host(tables, sedges, pedges, gedges, batches, columns, first, weight=None, limbs=None, counters=None,
                       psi0=None, span=None, sqrt_label=False):
    """The exact deposit of a PhaseDistribution with batches on the CPU (gfhip_phase_add_particles_host): particle i of
    the columns is particle first + i of the ensemble.  (limbs (batches, ns, np, ng, 67) int64, counters (3,) uint64), the
    bytes and numbers of state() and counts() after the same add_particles; given `limbs` and `counters`, added to in
    place."""
    from . import _lib
    from .moments import _host_columns
    lib = _lib.load()
    given, keep = flux_map(tables, psi0, span, sqrt_label)
    field, keep_field = spectrum_field(tables)
    edges = [np.ascontiguousarray(e, dtype=np.float64).reshape(-1) for e in (sedges, pedges, gedges)]
    if min(e.size for e in edges) < 2:
        raise ValueError("a distribution needs at least two edges per axis")
    shape = (int(batches),) + tuple(e.size - 1 for e in edges) + (LIMBS,)
    if limbs is None:
        limbs, counters = np.zeros(shape, dtype=np.int64), np.zeros(3, dtype=np.uint64)
    for name, array, kind, want in (("limbs", limbs, np.int64, shape), ("counters", counters, np.uint64, (3,))):
        if not isinstance(array, np.ndarray) or array.dtype != kind or array.shape != want or not array.flags["C_CONTIGUOUS"]:
            raise ValueError("%s must be a contiguous %s array of shape %r: it is updated in place" % (name, np.dtype(kind).name, want))
    columns, is_f32 = _host_columns(columns, weight)
    pointers = (ctypes.c_void_p*8)(*[column.ctypes.data for column in columns])
    axes = [value for e in edges for value in (e.ctypes.data, e.size - 1)]
    if lib.gfhip_phase_add_particles_host(ctypes.byref(given), ctypes.byref(field), *axes, int(batches), pointers, int(is_f32),
                                          columns[0].size, int(first), limbs.ctypes.data, counters.ctypes.data):
        raise GfHipError(lib.gfhip_last_error(None).decode())
    del keep, keep_field
    return limbs, counters


class PhaseDistribution(RayBatches):
    """A grid of exact sums over (label, xi, gamma) on a context's device (gfhip_phase_*, include/gf_hip.h); state() is
    (ns, np, ng, 67).  batches=G: the same sums per batch of particles (batches.py, the particle's index in the ensemble
    in place of a ray's), state() (G, ns, np, ng, 67), fed with add_particles; total() is the plain distribution and
    standard_error() the error bar of its cells."""
    prefix = "phase"

    def __init__(self, context, tables, sedges, pedges, gedges, psi0=None, span=None, sqrt_label=False, private=True,
                 batches=None):
        self.tables = tables
        self.sedges, self.pedges, self.gedges = (np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
                                                 for edges in (sedges, pedges, gedges))
        if min(self.sedges.size, self.pedges.size, self.gedges.size) < 2:
            raise ValueError("a distribution needs at least two edges per axis")
        self.sqrt_label = bool(sqrt_label)
        self.private = bool(private)
        given, keep = flux_map(tables, psi0, span, sqrt_label, private)
        field, keep_field = spectrum_field(tables)
        self.psi0, self.span = given.psi0, given.span
        self._created_cells(context, batches, (self.sedges.size - 1, self.pedges.size - 1, self.gedges.size - 1),
                            ctypes.byref(given), ctypes.byref(field), self.sedges.ctypes.data, self.sedges.size - 1,
                            self.pedges.ctypes.data, self.pedges.size - 1, self.gedges.ctypes.data, self.gedges.size - 1)
        del keep, keep_field                                 # the library has copied the tables

    def _twin(self, context, batches):
        return PhaseDistribution(context, self.tables, self.sedges, self.pedges, self.gedges, self.psi0, self.span,
                                 self.sqrt_label, self.private, batches)

    @property
    def label_kind(self):
        return "sqrt_s" if self.sqrt_label else "s"

    def add(self, x, y, z, ux, uy, uz, gamma, count, weight=None):
        """Bin `count` particles of seven context buffers, all fp32 or all fp64, each with the weight of an eighth buffer
        of the same type or with 1.0; asynchronous on the context's stream."""
        keys = _keys((x, y, z, ux, uy, uz, gamma), 7)
        self.context._check(self.lib.gfhip_phase_add(self.handle, keys, 0 if weight is None else key_of(weight),
                                                     int(weight is not None), int(count)))

    def add_particles(self, x, y, z, ux, uy, uz, gamma, count, first, weight=None):
        """add() for a distribution with batches: particle i of the buffers is particle first + i of the whole ensemble."""
        keys = _keys((x, y, z, ux, uy, uz, gamma), 7)
        self.context._check(self.lib.gfhip_phase_add_particles(self.handle, keys, 0 if weight is None else key_of(weight),
                                                               int(weight is not None), int(count), int(first)))

    def coordinates(self, x, y, z, ux, uy, uz, gamma, label_key, pitch_key, count):
        """The labels and pitch cosines of `count` particles into the fp64 buffers `label_key` and `pitch_key` (NaN off
        the map); asynchronous."""
        keys = _keys((x, y, z, ux, uy, uz, gamma), 7)
        self.context._check(self.lib.gfhip_phase_coordinates(self.handle, keys, key_of(label_key), key_of(pitch_key), int(count)))

    def profile(self, context=None):
        """A FluxProfile on the label edges (on `context`, this distribution's by default) that holds the marginal over
        pitch and gamma: the np*ng slices state()[:, p, g, :] merged into it, which is exact.  Its counts are this
        distribution's: a particle that fell off the pitch or the gamma axis is among `outside`."""
        marginal = FluxProfile(context or self.context, self.tables, self.sedges, self.psi0, self.span, self.sqrt_label,
                               self.private)
        with self._plain() as plain:
            state = plain.state()
        counts = self.counts()
        for p in range(state.shape[1]):
            for g in range(state.shape[2]):
                marginal.merge(state[:, p, g, :], **(counts if p == 0 and g == 0 else {}))
        return marginal

    def info(self):
        """How deposits are launched: {private_sums, workgroup_size, cap_cells, max_workgroups, lds_bytes}."""
        info = _Info()
        self.context._check(self.lib.gfhip_phase_info(self.handle, ctypes.byref(info)))
        out = {name: int(getattr(info, name)) for name, _ in _Info._fields_}
        out["private_sums"] = bool(out["private_sums"])
        return out
