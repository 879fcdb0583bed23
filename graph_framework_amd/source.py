"""A particle source: the seven columns of a push (korc.py) filled where they lie on the device, from a stated distribution.

A ParticleSource places particles uniformly in volume inside a box of the poloidal plane and between two flux surfaces
(slo <= label < shi, flux.py's label), optionally thinned by a radial profile of acceptance probabilities, and gives each a
speed |v|/c and a pitch cosine to the LOCAL field direction, both uniform in their ranges, at a uniform gyrophase.  The
columns receive the components of beta = v/c and gamma = 0: the push's own pre-item initialize_gamma turns them into
gamma and gamma*beta, exactly as it does for particles that came from the host.

Particle p, its index in the WHOLE ensemble, is drawn from a counter-based generator (Philox4x32-10) keyed by p and the
seed, in the fixed fp64 arithmetic of csrc/particle_draw.hpp: it is the same particle, to the last bit, on any device, for
any split into shards (fill(..., first_particle=)), launch shape or route, and on the host (fill_host).  Candidate
positions are rounded to the columns' type before their label is tested, so every placed particle passes the same test
when a diagnostic reads the column back.  A particle that finds no position in `attempts` candidates is unplaced: NaN in
all seven columns and 0 in `placed`, a column that is a weight for every diagnostic.
"""
import ctypes

import numpy as np

from .backend import GfHipError, key_of
from .flux import _Info, flux_map
from .spectrum import _keys, spectrum_field

PLAIN = 1
REFILL = 2
COUNTERS = ("placed", "unplaced", "position_tries", "gyro_tries")
_DTYPES = {"f32": np.float32, "f64": np.float64}


def _dtype_of(dtype):
    dtype = _DTYPES.get(dtype, dtype)
    if np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("a particle source fills fp32 or fp64 columns")
    return np.dtype(dtype)


def _parameters(box, label_range, speed_range, pitch_range, profile, seed, attempts):
    """The arguments of gfhip_source_create between the field and is_f32, and what their pointers refer to."""
    box = np.ascontiguousarray(box, dtype=np.float64).reshape(-1)
    if box.size != 4:
        raise ValueError("box is (rlo, rhi, zlo, zhi)")
    ranges = [float(v) for pair in (label_range, speed_range, pitch_range) for v in pair]
    if len(ranges) != 6:
        raise ValueError("label_range, speed_range and pitch_range are pairs (low, high)")
    sedges = accept = None
    if profile is not None:
        sedges, accept = (np.ascontiguousarray(values, dtype=np.float64).reshape(-1) for values in profile)
        if sedges.size != accept.size + 1 or accept.size < 1:
            raise ValueError("profile is (sedges, accept) with one edge more than probabilities")
    if not 0 <= int(seed) < 1 << 64 or not 0 <= int(attempts) < 1 << 32:
        raise ValueError("the seed is a uint64 and attempts a uint32")
    arguments = [box.ctypes.data] + ranges + [None if sedges is None else sedges.ctypes.data,
                                              None if accept is None else accept.ctypes.data,
                                              0 if accept is None else accept.size, int(seed), int(attempts)]
    return arguments, (box, sedges, accept)


def block_host(counter, key):
    """One Philox4x32-10 block (gfhip_source_block_host): uint32[4] from a counter of four words and a key of two."""
    from . import _lib
    lib = _lib.load()
    counter = np.ascontiguousarray(counter, dtype=np.uint32).reshape(4)
    key = np.ascontiguousarray(key, dtype=np.uint32).reshape(2)
    out = np.empty(4, dtype=np.uint32)
    lib.gfhip_source_block_host(counter.ctypes.data, key.ctypes.data, out.ctypes.data)
    return out


def fill_host(tables, box, label_range, speed_range, count, pitch_range=(-1.0, 1.0), profile=None, seed=0, attempts=64,
              dtype=np.float64, sqrt_label=False, first_particle=0, placed=True, psi0=None, span=None, flags=0):
    """ParticleSource.fill on the CPU (gfhip_source_fill_host), its bits: (columns, placed, counters) with columns the seven
    arrays x, y, z, ux, uy, uz, gamma of `dtype`, placed an eighth (None with placed=False) and counters a dict."""
    from . import _lib
    lib = _lib.load()
    dtype = _dtype_of(dtype)
    given, keep = flux_map(tables, psi0, span, sqrt_label)
    field, keep_field = spectrum_field(tables)
    arguments, keep_arguments = _parameters(box, label_range, speed_range, pitch_range, profile, seed, attempts)
    count = int(count)
    columns = [np.zeros(count, dtype=dtype) for _ in range(7)]
    mark = np.zeros(count, dtype=dtype) if placed else None
    pointers = (ctypes.c_void_p*8)(*([column.ctypes.data for column in columns] + [None if mark is None else mark.ctypes.data]))
    counters = np.zeros(4, dtype=np.uint64)
    if lib.gfhip_source_fill_host(ctypes.byref(given), ctypes.byref(field), *arguments, int(flags), pointers,
                                  int(dtype == np.float32), int(first_particle), count, counters.ctypes.data):
        raise GfHipError(lib.gfhip_last_error(None).decode())
    del keep, keep_field, keep_arguments
    return columns, mark, dict(zip(COUNTERS, (int(c) for c in counters)))


class ParticleSource:
    """A source of particles on a context's device (gfhip_source_*, include/gf_hip.h).  plain / refill: the route of
    csrc/particle_source.hip, the library's choice with neither; the bytes are the same."""

    def __init__(self, context, tables, box, label_range, speed_range, pitch_range=(-1.0, 1.0), profile=None, seed=0,
                 attempts=64, dtype=np.float64, sqrt_label=False, plain=False, refill=False, max_workgroups=0, psi0=None,
                 span=None):
        self.context = context
        self.lib = context.lib
        self.dtype = _dtype_of(dtype)
        self.sqrt_label = bool(sqrt_label)
        given, keep = flux_map(tables, psi0, span, sqrt_label)
        field, keep_field = spectrum_field(tables)
        arguments, keep_arguments = _parameters(box, label_range, speed_range, pitch_range, profile, seed, attempts)
        flags = (PLAIN if plain else 0) | (REFILL if refill else 0)
        self.handle = self.lib.gfhip_source_create(context.handle, ctypes.byref(given), ctypes.byref(field), *arguments,
                                                   int(self.dtype == np.float32), flags, int(max_workgroups))
        if not self.handle:
            raise GfHipError(self.lib.gfhip_last_error(context.handle).decode())
        del keep, keep_field, keep_arguments                 # the library has copied the tables

    def fill(self, x, y, z, ux, uy, uz, gamma, count, first_particle=0, placed=None):
        """Particles first_particle .. first_particle + count of the ensemble into elements 0 .. count of seven context
        buffers of the source's type (allocated where absent); placed: the key of an eighth that receives 1 or 0.
        Asynchronous on the context's stream."""
        keys = _keys((x, y, z, ux, uy, uz, gamma), 7)
        self.context._check(self.lib.gfhip_source_fill(self.handle, keys, 0 if placed is None else key_of(placed),
                                                       int(placed is not None), int(first_particle), int(count)))

    def counts(self):
        """{placed, unplaced, position_tries, gyro_tries} of all fills so far."""
        counters = np.zeros(4, dtype=np.uint64)
        self.context._check(self.lib.gfhip_source_counts(self.handle, counters.ctypes.data))
        return dict(zip(COUNTERS, (int(c) for c in counters)))

    def info(self):
        """How fills are launched: {refill, workgroup_size, max_workgroups, lds_bytes}."""
        info = _Info()
        self.context._check(self.lib.gfhip_source_info(self.handle, ctypes.byref(info)))
        return dict(refill=bool(info.private_sums), workgroup_size=int(info.workgroup_size),
                    max_workgroups=int(info.max_workgroups), lds_bytes=int(info.lds_bytes))

    def close(self):
        if self.handle and self.context.handle:              # a closed context has freed its sources
            self.lib.gfhip_source_destroy(self.handle)
        self.handle = None
