"""Power spectra over the flux label and the parallel refractive index, P(psi, N), on the device and exact.

A flux profile (flux.py) says on which flux surface the power was absorbed; current drive, Fokker-Planck and quasilinear
diffusion codes also need at which N = c (k.B)/(|B| w) it was.  A FluxSpectrum labels every sample with flux.py's label
and with N from the EFIT field direction B = (psi_z/R, fpol/R, -psi_R/R), in the fixed arithmetic of
csrc/flux_label.hpp, finds both cells by the rule of the 3-D grid and adds the value to the superaccumulator of cell
(is, in) (csrc/flux_spectrum.hip).  The state, shape (ns, nn, 67), is the same bytes with and without the
workgroup-private sums and for any order of samples, records, files or shards; summed over N it is the flux profile's.
"""
import ctypes
import os

import numpy as np

from .backend import GfHipError, key_of
from .exact_cells import RayBatches, bin_files
from .flux import FluxProfile, _Info, flux_map, marginal_bins
from .output import write_spectrum_bins

#  dispersion.hpp:494-502: the speed of light the dispersion relations use, 1/sqrt(epsilon0 mu0)
C = 1.0/np.sqrt(8.8541878138E-12*(np.pi*4.0E-7))
FPOL_NAMES = tuple("fpol_c%d" % k for k in range(4))
SAMPLE_NAMES = ("x", "y", "z", "kx", "ky", "kz", "w")


class _Field(ctypes.Structure):
    _fields_ = [("psimin", ctypes.c_double), ("dpsi", ctypes.c_double), ("numpsi", ctypes.c_uint64),
                ("fpol", ctypes.c_void_p*4), ("c", ctypes.c_double), ("reserved", ctypes.c_uint64)]


def spectrum_field(tables, c=None):
    """(gfhip_spectrum_field, the arrays its pointers refer to) from a mapping with efit.nc's dataset names."""
    fpol = [np.ascontiguousarray(tables[name], dtype=np.float64).reshape(-1) for name in FPOL_NAMES]
    if len({table.size for table in fpol}) != 1:
        raise ValueError("fpol_c0 .. fpol_c3 differ in length")
    pointers = (ctypes.c_void_p*4)(*[table.ctypes.data for table in fpol])
    return _Field(float(tables["psimin"]), float(tables["dpsi"]), fpol[0].size, pointers, float(C if c is None else c), 0), fpol


def _keys(keys, number):
    keys = [key_of(key) for key in keys]
    if len(keys) != number:
        raise ValueError("%d keys where %d are needed" % (len(keys), number))
    return (ctypes.c_uint64*number)(*keys)


def npar_host(tables, x, y, z, kx, ky, kz, w, psi0=None, span=None, sqrt_label=False, c=None):
    """(label, npar) of samples on the CPU (gfhip_spectrum_npar_host): the bits of FluxSpectrum.npar, NaN off the map."""
    from . import _lib
    lib = _lib.load()
    given, keep = flux_map(tables, psi0, span, sqrt_label)
    field, keep_field = spectrum_field(tables, c)
    columns = [np.ascontiguousarray(column, dtype=np.float64).reshape(-1) for column in (x, y, z, kx, ky, kz, w)]
    if len({column.size for column in columns}) != 1:
        raise ValueError("the seven columns differ in length")
    pointers = (ctypes.c_void_p*7)(*[column.ctypes.data for column in columns])
    label = np.empty(columns[0].size, dtype=np.float64)
    npar = np.empty(columns[0].size, dtype=np.float64)
    if lib.gfhip_spectrum_npar_host(ctypes.byref(given), ctypes.byref(field), pointers, label.size, label.ctypes.data,
                                    npar.ctypes.data):
        raise GfHipError(lib.gfhip_last_error(None).decode())
    del keep, keep_field
    return label, npar


class FluxSpectrum(RayBatches):
    """A grid of exact sums over (label, N) on a context's device (gfhip_spectrum_*, include/gf_hip.h); state() is
    (ns, nn, 67).  batches=G: the same sums per batch of rays (batches.py), state() (G, ns, nn, 67), fed with add_rays."""
    prefix = "spectrum"

    def __init__(self, context, tables, sedges, nedges, psi0=None, span=None, sqrt_label=False, private=True, c=None,
                 batches=None):
        self.tables = tables
        self.sedges = np.ascontiguousarray(sedges, dtype=np.float64).reshape(-1)
        self.nedges = np.ascontiguousarray(nedges, dtype=np.float64).reshape(-1)
        if self.sedges.size < 2 or self.nedges.size < 2:
            raise ValueError("a spectrum needs at least two edges per axis")
        self.sqrt_label = bool(sqrt_label)
        self.private = bool(private)
        given, keep = flux_map(tables, psi0, span, sqrt_label, private)
        field, keep_field = spectrum_field(tables, c)
        self.psi0, self.span, self.c = given.psi0, given.span, field.c
        self._created_cells(context, batches, (self.sedges.size - 1, self.nedges.size - 1), ctypes.byref(given),
                            ctypes.byref(field), self.sedges.ctypes.data, self.sedges.size - 1, self.nedges.ctypes.data,
                            self.nedges.size - 1)
        del keep, keep_field                                 # the library has copied the tables

    def _twin(self, context, batches):
        return FluxSpectrum(context, self.tables, self.sedges, self.nedges, self.psi0, self.span, self.sqrt_label, self.private,
                            self.c, batches)

    def add_rays(self, x_key, y_key, z_key, kx_key, ky_key, kz_key, w_key, value_key, count, first_ray):
        """add() for a spectrum with batches: sample i is ray first_ray + i of the whole ensemble."""
        keys = _keys((x_key, y_key, z_key, kx_key, ky_key, kz_key, w_key, value_key), 8)
        self.context._check(self.lib.gfhip_spectrum_add_rays(self.handle, keys, int(count), int(first_ray)))

    @property
    def label_kind(self):
        return "sqrt_s" if self.sqrt_label else "s"

    def add(self, x_key, y_key, z_key, kx_key, ky_key, kz_key, w_key, value_key, count):
        """Bin `count` samples of eight fp64 context buffers; asynchronous on the context's stream."""
        keys = _keys((x_key, y_key, z_key, kx_key, ky_key, kz_key, w_key, value_key), 8)
        self.context._check(self.lib.gfhip_spectrum_add(self.handle, keys, int(count)))

    def npar(self, x_key, y_key, z_key, kx_key, ky_key, kz_key, w_key, label_key, npar_key, count):
        """The labels and N of `count` samples into the fp64 buffers `label_key` and `npar_key` (NaN off the map);
        asynchronous."""
        keys = _keys((x_key, y_key, z_key, kx_key, ky_key, kz_key, w_key), 7)
        self.context._check(self.lib.gfhip_spectrum_npar(self.handle, keys, key_of(label_key), key_of(npar_key), int(count)))

    def profile(self, context=None):
        """A FluxProfile on the label edges (on `context`, this spectrum's by default) that holds the marginal over N:
        the nn slices state()[..., n, :] merged into it, which is exact.  Its counts are this spectrum's: a sample that
        fell off the N axis is among `outside`.  A spectrum with batches gives a profile with the same batches."""
        marginal = FluxProfile(context or self.context, self.tables, self.sedges, self.psi0, self.span, self.sqrt_label,
                               self.private, self.batches)
        state = self.state()
        counts = self.counts()
        for n in range(self.cell_shape[1]):
            marginal.merge(state[..., n, :], **(counts if n == 0 else {}))
        return marginal

    def info(self):
        """How deposits are launched: {private_sums, workgroup_size, cap_cells, max_workgroups, lds_bytes}."""
        info = _Info()
        self.context._check(self.lib.gfhip_spectrum_info(self.handle, ctypes.byref(info)))
        out = {name: int(getattr(info, name)) for name, _ in _Info._fields_}
        out["private_sums"] = bool(out["private_sums"])
        return out


def spectrum_deposition(directory, num_files, tables, cells, low, high, npar_cells, npar_low, npar_high, psi0=None, span=None,
                        sqrt_label=False, private=True, c=None, index=0, spectrum=None, batches=None, first_ray=0):
    """flux_deposition's counterpart over (label, N): d_power of result0.nc .. result<num_files - 1>.nc binned on
    `cells` uniform cells of the label between `low` and `high` times `npar_cells` of N between `npar_low` and
    `npar_high`, from x, y, z, kx, ky, kz, w of every record, divided by the total number of rays, written to
    <directory>/spectrum_bins.nc.  Returns (bins, counts).  spectrum: a FluxSpectrum that receives the exact state too.
    batches, first_ray: as in flux_deposition."""
    from .backend import Context
    sedges = np.linspace(low, high, cells + 1)
    nedges = np.linspace(npar_low, npar_high, npar_cells + 1)
    context = Context(index)
    local = FluxSpectrum(context, tables, sedges, nedges, psi0, span, sqrt_label, private, c, batches)
    bins, counts, total = bin_files(local, directory, num_files, "spectrum", SAMPLE_NAMES + ("d_power",), first_ray)
    if spectrum is not None:
        spectrum.merge(local.state(), **counts)
    psi0, span, kind, c = local.psi0, local.span, local.label_kind, local.c
    extra = {}
    if batches is not None:
        bins, extra = marginal_bins(local, total), local.error_variables(first_ray, total)
    local.close()
    context.close()
    write_spectrum_bins(os.path.join(directory, "spectrum_bins.nc"), bins, sedges, nedges, psi0, span, kind, c, **counts, **extra)
    return bins, counts
