"""Flux-surface profiles: absorbed power per flux surface, P(psi), on the device and exact.

The 3-D grid of deposition.py is bin.py's picture; for a tokamak the result of a ray-tracing run is drawn over the flux
label.  A FluxProfile labels every sample with s = (psi(R, z) - psi0)/span (or its square root) from the EFIT psi spline,
in the fixed arithmetic of csrc/flux_label.hpp, finds the label's cell among the edges by the rule of the 3-D grid
(edge[i] <= label < edge[i+1]) and adds the value to that cell's superaccumulator (csrc/superacc.hpp).  A profile is small
enough for every workgroup to sum its deposits in LDS before they reach memory (csrc/flux_profile.hip); the state is the
same bytes with and without that, and for any order of samples, records, files or shards.

The volume between a cell's two flux surfaces is one more deposit into the same cells, of quadrature points that the
device generates itself (FluxProfile.add_volumes, the contract in include/gf_hip.h); volumes() and density() turn power
per cell into power per cubic metre.
"""
import ctypes
import os

import numpy as np

from .backend import GfHipError, key_of
from .exact_cells import LIMBS, RayBatches, bin_files
from .output import write_flux_bins

SQRT_LABEL = 1
NO_PRIVATE_SUMS = 2
TABLE_NAMES = tuple("psi_c%d%d" % (a, b) for a in range(4) for b in range(4))


class _Map(ctypes.Structure):
    _fields_ = [("rmin", ctypes.c_double), ("dr", ctypes.c_double), ("zmin", ctypes.c_double), ("dz", ctypes.c_double),
                ("numr", ctypes.c_uint64), ("numz", ctypes.c_uint64), ("coefficients", ctypes.c_void_p),
                ("psi0", ctypes.c_double), ("span", ctypes.c_double), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class _Info(ctypes.Structure):
    _fields_ = [("private_sums", ctypes.c_uint32), ("workgroup_size", ctypes.c_uint32), ("cap_cells", ctypes.c_uint64),
                ("max_workgroups", ctypes.c_uint64), ("lds_bytes", ctypes.c_uint64)]


def default_range(tables):
    """(psi0, span) of the reference's profile tables: the axis value psimin and dpsi*(numpsi - 1), axis to edge."""
    return float(tables["psimin"]), float(tables["dpsi"])*(np.asarray(tables["fpol_c0"]).size - 1)


def flux_map(tables, psi0=None, span=None, sqrt_label=False, private=True, flags=None):
    """(gfhip_flux_map, the array its pointer refers to) from a mapping with efit.nc's dataset names."""
    first = np.asarray(tables[TABLE_NAMES[0]])
    if first.ndim != 2:
        raise ValueError("psi_c00 must be a numr x numz table")
    coefficients = np.empty((16,) + first.shape, dtype=np.float64)
    for k, name in enumerate(TABLE_NAMES):
        table = np.asarray(tables[name], dtype=np.float64)
        if table.shape != first.shape:
            raise ValueError("%s has shape %r, psi_c00 %r" % (name, table.shape, first.shape))
        coefficients[k] = table
    if psi0 is None or span is None:
        low, width = default_range(tables)
        psi0 = low if psi0 is None else psi0
        span = width if span is None else span
    if flags is None:
        flags = (SQRT_LABEL if sqrt_label else 0) | (0 if private else NO_PRIVATE_SUMS)
    return _Map(float(tables["rmin"]), float(tables["dr"]), float(tables["zmin"]), float(tables["dz"]), first.shape[0],
                first.shape[1], coefficients.ctypes.data, float(psi0), float(span), int(flags), 0), coefficients


def label_host(tables, x, y, z, psi0=None, span=None, sqrt_label=False):
    """The labels of points on the CPU (gfhip_flux_label_host): the bits of FluxProfile.label, NaN outside the map."""
    from . import _lib
    lib = _lib.load()
    given, keep = flux_map(tables, psi0, span, sqrt_label)
    columns = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in (x, y, z)]
    if len({c.size for c in columns}) != 1:
        raise ValueError("x, y and z differ in length")
    label = np.empty(columns[0].size, dtype=np.float64)
    if lib.gfhip_flux_label_host(ctypes.byref(given), *[c.ctypes.data for c in columns], label.size, label.ctypes.data):
        raise GfHipError(lib.gfhip_last_error(None).decode())
    del keep
    return label


class _Window(ctypes.Structure):
    _fields_ = [("rlo", ctypes.c_double), ("rhi", ctypes.c_double), ("zlo", ctypes.c_double), ("zhi", ctypes.c_double)]


def _window(window):
    """(the pointer gfhip_flux_add_volumes takes, the structure behind it): None is the whole map."""
    if window is None:
        return None, None
    given = _Window(*(float(v) for v in window))
    return ctypes.byref(given), given


def _point_count(tables, sub, first, count):
    numr, numz = np.asarray(tables[TABLE_NAMES[0]]).shape
    return numr*int(sub)*numz*int(sub) - int(first) if count is None else int(count)


def volumes_host(tables, edges, sub, window=None, psi0=None, span=None, sqrt_label=False, first=0, count=None):
    """The quadrature of FluxProfile.add_volumes on the CPU (gfhip_flux_volumes_host): (limbs (cells, 67), counts), the
    bytes and numbers of a profile's state() and counts() after the same points."""
    from . import _lib
    lib = _lib.load()
    given, keep = flux_map(tables, psi0, span, sqrt_label)
    edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    if edges.size < 2:
        raise ValueError("a profile needs at least two edges")
    limbs = np.zeros((edges.size - 1, LIMBS), dtype=np.int64)
    counters = np.zeros(3, dtype=np.uint64)
    pointer, keep_window = _window(window)
    if lib.gfhip_flux_volumes_host(ctypes.byref(given), edges.ctypes.data, edges.size - 1, int(sub), pointer, int(first),
                                   _point_count(tables, sub, first, count), limbs.ctypes.data, counters.ctypes.data):
        raise GfHipError(lib.gfhip_last_error(None).decode())
    del keep, keep_window
    return limbs, dict(zip(("samples", "outside", "skipped"), (int(c) for c in counters)))


class FluxProfile(RayBatches):
    """A radial profile of exact sums on a context's device (gfhip_flux_*, include/gf_hip.h); state() is (cells, 67).
    batches=G: the same sums per batch of rays (batches.py), state() (G, cells, 67), fed with add_rays; total() is the
    plain profile and standard_error() the error bar of its cells."""
    prefix = "flux"

    def __init__(self, context, tables, edges, psi0=None, span=None, sqrt_label=False, private=True, batches=None):
        self.tables = tables
        self.edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        if self.edges.size < 2:
            raise ValueError("a profile needs at least two edges")
        self.cells = self.edges.size - 1
        self.sqrt_label = bool(sqrt_label)
        self.private = bool(private)
        given, keep = flux_map(tables, psi0, span, sqrt_label, private)
        self.psi0, self.span = given.psi0, given.span
        self._created_cells(context, batches, (self.cells,), ctypes.byref(given), self.edges.ctypes.data, self.cells)
        del keep                                             # the library has copied the tables

    def _twin(self, context, batches):
        return FluxProfile(context, self.tables, self.edges, self.psi0, self.span, self.sqrt_label, self.private, batches)

    def add_rays(self, x_key, y_key, z_key, value_key, count, first_ray):
        """add() for a profile with batches: sample i is ray first_ray + i of the whole ensemble."""
        self.context._check(self.lib.gfhip_flux_add_rays(self.handle, key_of(x_key), key_of(y_key), key_of(z_key),
                                                         key_of(value_key), int(count), int(first_ray)))

    @property
    def label_kind(self):
        return "sqrt_s" if self.sqrt_label else "s"

    def label(self, x_key, y_key, z_key, label_key, count):
        """The labels of `count` points into the fp64 buffer `label_key` (NaN outside the map); asynchronous."""
        self.context._check(self.lib.gfhip_flux_label(self.handle, key_of(x_key), key_of(y_key), key_of(z_key),
                                                      key_of(label_key), int(count)))

    def add_volumes(self, sub=16, window=None, first=0, count=None):
        """Deposit the quadrature points first .. first + count (default: to the last) of include/gf_hip.h's flux
        volumes into this profile: every table cell cut into sub x sub, weight R x area, window = (rlo, rhi, zlo, zhi) or
        the whole map.  Asynchronous.  For callers that shard the point range over devices and merge()."""
        pointer, keep = _window(window)
        self.context._check(self.lib.gfhip_flux_add_volumes(self.handle, int(sub), pointer, int(first),
                                                            _point_count(self.tables, sub, first, count)))
        del keep

    def volumes(self, sub=16, window=None, first=0, count=None):
        """(volume[cells] in m^3, counts): 2 pi times the exact sum of R dR dz over the part of the map (or window)
        whose label lies in each cell, on a twin of this profile.  Between closed surfaces that is the shell's volume."""
        twin = self._twin(self.context, None)
        try:
            twin.add_volumes(sub, window, first, count)
            return twin.read()*(2.0*np.pi), twin.counts()
        finally:
            twin.close()

    def density(self, divisor=1.0, sub=16, window=None):
        """read(divisor)/volume per cell, dP/dV; NaN where no quadrature point reached the cell."""
        return density_variables(self, self.read(divisor), sub, window)["density"]

    def info(self):
        """How deposits are launched: {private_sums, workgroup_size, cap_cells, max_workgroups, lds_bytes}."""
        info = _Info()
        self.context._check(self.lib.gfhip_flux_info(self.handle, ctypes.byref(info)))
        out = {name: int(getattr(info, name)) for name, _ in _Info._fields_}
        out["private_sums"] = bool(out["private_sums"])
        return out


def flux_deposition(directory, num_files, tables, cells, low, high, psi0=None, span=None, sqrt_label=False, private=True,
                    index=0, profile=None, density=False, sub=16, window=None, batches=None, first_ray=0):
    """bin_deposition's counterpart on flux surfaces: d_power of result0.nc .. result<num_files - 1>.nc binned on
    `cells` uniform cells of the label between `low` and `high`, divided by the total number of rays, written to
    <directory>/flux_bins.nc.  Returns (bins, counts).  profile: a FluxProfile that receives the exact state as well.
    density: the file also gets the cells' volumes (FluxProfile.volumes(sub, window)) and bins/volume.
    batches: the sums are kept per batch of rays (`profile`, if given, has the same batches), the rays counted on from
    first_ray across the files, and the file also gets stderr, batch_bins and batch_rays (write_flux_bins)."""
    from .backend import Context
    edges = np.linspace(low, high, cells + 1)
    context = Context(index)
    local = FluxProfile(context, tables, edges, psi0, span, sqrt_label, private, batches)
    bins, counts, total = bin_files(local, directory, num_files, "flux", first_ray=first_ray)
    if profile is not None:
        profile.merge(local.state(), **counts)
    psi0, span, kind = local.psi0, local.span, local.label_kind
    extra = {}
    if batches is not None:
        bins, extra = marginal_bins(local, total), local.error_variables(first_ray, total)
    if density:
        extra.update(density_variables(local, bins, sub, window))
    local.close()
    context.close()
    write_flux_bins(os.path.join(directory, "flux_bins.nc"), bins, edges, psi0, span, kind, **counts, **extra)
    return bins, counts


def marginal_bins(batched, divisor=1.0):
    """total().read(divisor) of a profile or a spectrum with batches: the bins of the plain object."""
    marginal = batched.total()
    try:
        return marginal.read(divisor)
    finally:
        marginal.close()


def density_variables(profile, bins, sub, window=None):
    """write_flux_bins' keywords for the power density: the volumes of `profile`'s cells and `bins` divided by them."""
    volume, _ = profile.volumes(sub, window)
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(volume=volume, density=np.where(volume == 0.0, np.nan, bins/volume), sub=sub, window=window)
