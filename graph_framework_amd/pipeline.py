"""The three stages of graph_driver/xrays.cpp:1100-1105 in one pass over the rays.

The reference, and absorption.run_absorption / absorption.bin_power after it, run `trace_ray`, `calculate_power` and
`bin_power` as three passes over result<n>.nc: the second re-reads every stored record to compute kamp, the third
re-reads it again to integrate the power.  Every value those two read was in device memory when the trace stored the
record.  `OnePass.record()` runs the SAME work items on the same values, in the same order, right there: the stages keep
a context each (x is fp64 in `power` and complex in the absorption items), gfhip_hand_over (include/gf_hip.h) carries the
arrays from one context's buffers to the next one's on the device, and the record is written to the file once, with all
twelve variables.

The bits are those of the three stages because nothing that computes has changed: the items, their input order and their
initial values come from absorption.absorption_work / absorption.power_work, which the three-stage path uses too; a file
stores a record bit for bit, so what a later stage reads back from it is what the hand-over delivers; a real variable
read into a complex data_set gets +0.0 imaginary parts (output.hpp:305, :425-428), which is the widening hand-over.
"""
from .absorption import WAVE_NAMES, _Writer, absorption_work, allocate_wave_buffers, feed_cells, power_work
from .backend import Context, key_of
from .output import RAY_VARIABLES, ResultFile
from . import _lib

#  the absorption items' real inputs under the file's names: what WeakDamping.run reads per record
_ABSORPTION_READS = (("w", "w"), ("kx", "kx"), ("ky", "ky"), ("kz", "kz"), ("x", "x"), ("y", "y"), ("z", "z"), ("t", "time"))
_POSITION = ("x", "y", "z")


class OnePass:
    """kamp, power, d_power (and the deposition grid) of the state a context holds NOW, appended to `path` with it.

    source: the Context that holds the nine trajectory arrays of `num_rays` fp64 elements.
    keys: {file variable (output.RAY_VARIABLES): buffer key in `source`}; the solver's names by default.
    model: "weak_damping" or "root_find" (run_absorption's).  items: GFIR replacing exported workloads, {"weak_damping",
    "init", "loss", "final", "power"}.  deposition, flux, spectrum, first_ray: as in absorption.bin_power.
    stream: the stream `source` launches on, when the caller knows it: the stage contexts then share it and nothing but
    stream order is needed between the stages; otherwise they get private streams and gfhip_hand_over orders them.

    record() with weak_damping returns when its work is queued.  It waits for one thing, the writer thread of the
    previous record (TrajectoryWriter.write_step's discipline): the record is gathered on the device into a context of
    its own, copied to pinned host memory on that context's stream and written by a thread, while `source` moves on.
    root_find synchronises per record in its converge loop, as RootFinder does."""

    def __init__(self, source, num_rays, path, model="weak_damping", index=0, stream=None, keys=None, deposition=None,
                 items=None, flux=None, spectrum=None, first_ray=0):
        items = items or {}
        self.source = source
        self.num_rays = n = int(num_rays)
        self.first_ray = int(first_ray)
        self.keys = dict(RAY_VARIABLES)
        self.keys.update(keys or {})
        self.absorption, _, self.newton = absorption_work(n, model, index, stream, items)
        self.power, _, _ = power_work(n, index, stream, items.get("power"))
        self.absorption.compile()
        self.power.compile()
        self.iterations = []
        self.records = 0
        self.deposition = deposition
        self.flux = flux
#  (the caller's, its local twin on the power stage's context), as in absorption.bin_power
        self.grids = [(target, target.like(self.power.context)) for target in (deposition, flux) if target is not None]
        self.spectrum = spectrum
        self.spectra = [(spectrum, spectrum.like(self.power.context))] if spectrum is not None else []
        if self.spectra:
            allocate_wave_buffers(self.power.context, n)
#  The record as the file takes it, on a stream of its own: the copies to the host overlap what `source` does next.
        self.gather = Context(index)
        self.file = ResultFile(path, n)
        self.mirrors = {}
        for name, dtype in [(name, _lib.GFIR_F64) for name, _ in RAY_VARIABLES] + [("kamp", _lib.GFIR_C64), ("power", _lib.GFIR_F64),
                                                                                   ("d_power", _lib.GFIR_F64)]:
            self.file.create_variable(name, parts=2 if dtype == _lib.GFIR_C64 else 1)
            self.gather._check(self.gather.lib.gfhip_allocate_buffer(self.gather.handle, self._gathered(name), n, dtype))
            self.mirrors[name] = self.gather.get_host_buffer(self._gathered(name))
        self.sync = _Writer()

    @staticmethod
    def _gathered(name):
        return key_of("record_" + name)

    def record(self):
        """Record j = the number of calls so far: exactly what the three stages do for it."""
        j = self.records
        self.sync.join()                                                    # the mirrors are free; a failed write surfaces
        absorption, power, keys = self.absorption.context, self.power.context, self.keys
        absorption.hand_over(self.source, [(name, keys[stored]) for name, stored in _ABSORPTION_READS])
        self.absorption.run()
        if self.newton is not None:
            self.iterations.append(self.newton.iterations)
        if j == 0:                                                          # dataset.read(file, 0), xrays.cpp:767-771
            power.hand_over(self.source, [(name, keys[name]) for name in _POSITION]
                            + [(name + "_last", keys[name]) for name in _POSITION])
        else:
            power.hand_over(self.source, [(name, keys[name]) for name in _POSITION])
            power.hand_over(absorption, [("kamp", "kamp", 1)])              # reference_imag_variable
            self.power.run()
        for _, local in self.grids:
            feed_cells(local, ("x", "y", "z", "d_power"), self.num_rays, self.first_ray)
        for _, local in self.spectra:
            power.hand_over(self.source, [(name, keys[name]) for name in WAVE_NAMES])
            feed_cells(local, ("x", "y", "z") + WAVE_NAMES + ("d_power",), self.num_rays, self.first_ray)
        gather = self.gather
        gather.hand_over(self.source, [(self._gathered(name), keys[name]) for name, _ in RAY_VARIABLES])
        gather.hand_over(absorption, [(self._gathered("kamp"), "kamp")])
        gather.hand_over(power, [(self._gathered(name), name) for name in ("power", "d_power")])
        self.records = j + 1

        def write():
            gather.wait()                                                   # the mirrors hold the record
            self.file.write(self.mirrors, index=j)
        self.sync.start(write)

    def close(self):
        """Join the writer (its error surfaces here), merge the deposition grid, the flux profile and the spectrum and
        free the stage contexts."""
        try:
            self.sync.join()
        finally:
            self.file.close()
            self.grids += self.spectra
            self.spectra = []
            while self.grids:
                target, local = self.grids.pop(0)
                target.merge(local.state(), **local.counts())
                local.close()
            for context in (self.absorption.context, self.power.context, self.gather):
                context.close()
