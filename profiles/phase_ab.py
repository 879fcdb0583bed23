#!/usr/bin/env python3
"""A/B of the particle distribution's deposit kernel (csrc/phase_bins.hip) against the spectrum's (csrc/flux_spectrum.hip,
the yardstick) on the same particles in the same process: alternating rounds, HIP events around adds that end in a stream
synchronise.  One JSON line per measurement, then one summary line per mode with the median of the rounds and their range;
a run writes its output file anew.

    python profiles/phase_ab.py [--rounds 3] [--adds 5] [--out profiles/phase_ab.jsonl]

The particles, 1e7: the example's ensemble (examples/push_particles.py) with gamma = sqrt(1 + u.u).  Modes:
  spectrum_f64   FluxSpectrum.add at 16 x 16 cells on (x, y, z, ux, uy, uz, gamma, ones), c = 1: N is the parallel velocity
  phase_f64      PhaseDistribution.add at 8 x 8 x 4 cells (the private path's cap), no weight, fp64 columns
  phase_f32      the same on the fp32 roundings of the columns
  phase_f32_global   16 x 16 x 8 cells, above the cap: the global path behind the wave pre-sum
After the rounds the marginal of phase_f64 over pitch and gamma is compared with a flux profile fed the same positions.
For scale, last: one step of the fp32 push on 1e7 particles next to one snapshot (Korc.bin) of its arrays.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

PEAK = 8.0e12                                                # HBM bytes per second
READ = {"spectrum_f64": 64, "phase_f64": 56, "phase_f32": 28, "phase_f32_global": 28}       # bytes per particle


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--adds", type=int, default=5, help="adds of all particles per measurement")
    parser.add_argument("--particles", type=int, default=10000000)
    parser.add_argument("--push-steps", type=int, default=20)
    parser.add_argument("--tables", default=os.path.join(ROOT, "tests", "golden", "efit_tables.npz"))
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase_ab.jsonl"))
    args = parser.parse_args()

    import numpy as np
    import torch
    from graph_framework_amd import Context, _lib, key_of, korc
    from graph_framework_amd.distribution import PhaseDistribution, coordinates_host, pitch_edges
    from graph_framework_amd.flux import FluxProfile
    from graph_framework_amd.spectrum import FluxSpectrum
    from push_particles import ensemble

    tables = dict(np.load(args.tables))
    count = args.particles
    start = ensemble(count, 0)
    start["gamma"] = np.sqrt(1.0 + start["ux"]**2 + start["uy"]**2 + start["uz"]**2)
    columns = [start[name] for name in korc.PARTICLE]
    stream = torch.cuda.Stream()
    context = Context(0, stream.cuda_stream)
    keys = {}
    for kind, dtype, code in (("f64", np.float64, _lib.GFIR_F64), ("f32", np.float32, _lib.GFIR_F32)):
        keys[kind] = []
        for name, column in zip(korc.PARTICLE + ("one",), columns + [np.ones(count)]):
            key = "%s_%s" % (name, kind)
            context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), count, code))
            context.copy_to_device(key, column.astype(dtype))
            keys[kind].append(key)
    label, _ = coordinates_host(tables, [c[:200000] for c in columns])
    low, high = float(np.nanmin(label)), float(np.nextafter(np.nanmax(label), np.inf))
    gamma_high = float(np.nextafter(columns[6].max(), np.inf))

    def edges(ns, cells, ng):
        return np.linspace(low, high, ns + 1), pitch_edges(cells), np.linspace(1.0, gamma_high, ng + 1)

    made = {"spectrum_f64": lambda: FluxSpectrum(context, tables, np.linspace(low, high, 17), pitch_edges(16), c=1.0),
            "phase_f64": lambda: PhaseDistribution(context, tables, *edges(8, 8, 4)),
            "phase_f32": lambda: PhaseDistribution(context, tables, *edges(8, 8, 4)),
            "phase_f32_global": lambda: PhaseDistribution(context, tables, *edges(16, 16, 8))}
    added = {"spectrum_f64": keys["f64"], "phase_f64": keys["f64"][:7], "phase_f32": keys["f32"][:7], "phase_f32_global": keys["f32"][:7]}
    open(args.out, "w").close()                              # a run's lines replace the file's

    def record(line):
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    times = {mode: [] for mode in made}
    marginal_state = None
    for round_number in range(args.rounds):
        for mode in made:
            grid = made[mode]()
            info = grid.info()
            grid.add(*added[mode], count)                    # warm: code object, tables in cache
            context.wait()
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record(stream)
            for _ in range(args.adds):
                grid.add(*added[mode], count)
            end.record(stream)
            stream.synchronize()
            ms = begin.elapsed_time(end)/args.adds
            counts = grid.counts()
            if mode == "phase_f64" and marginal_state is None:
                marginal = grid.profile()
                marginal_state = marginal.state().tobytes()
                marginal.close()
            grid.close()
            times[mode].append(ms)
            record(dict(mode=mode, shape=list(grid.shape), round=round_number, ms_per_add=round(ms, 4), particles_per_add=count,
                        particles_per_s=count/(ms*1.0e-3), share_of_read_floor=round(count*READ[mode]/PEAK/(ms*1.0e-3), 4),
                        private_sums=info["private_sums"], workgroup_size=info["workgroup_size"],
                        max_workgroups=info["max_workgroups"], lds_bytes=info["lds_bytes"], outside=counts["outside"],
                        samples=counts["samples"]))
    reference = FluxProfile(context, tables, np.linspace(low, high, 9))
    for _ in range(args.adds + 1):
        reference.add(*keys["f64"][:3], keys["f64"][7], count)
    same = reference.state().tobytes() == marginal_state
    reference.close()
    if not same:
        sys.exit("the distribution's marginal over pitch and gamma and the flux profile disagree")
    for mode, values in times.items():
        record(dict(summary=mode, median_ms=round(statistics.median(values), 4), min_ms=round(min(values), 4),
                    max_ms=round(max(values), 4), rounds=len(values)))
    context.close()

    push = korc.Korc(ensemble(count, 0), "f32")
    push.compile()
    push.pre_run()
#  initialize_gamma turns the start velocities into momenta: gamma reaches 1/sqrt(1 - 0.81) = 2.3
    snapshot = PhaseDistribution(push.work.context, tables, np.linspace(low, high, 9), pitch_edges(8), np.linspace(1.0, 3.0, 5))
    push.run(args.push_steps)                                # warm
    push.bin(snapshot)
    push.wait()
    clock = time.perf_counter()
    push.run(args.push_steps)
    push.wait()
    step_ms = (time.perf_counter() - clock)*1.0e3/args.push_steps
    clock = time.perf_counter()
    for _ in range(args.adds):
        push.bin(snapshot)
    push.wait()
    snapshot_ms = (time.perf_counter() - clock)*1.0e3/args.adds
    counts = snapshot.counts()
    record(dict(scale="korc_step_f32", particles=count, step_ms=round(step_ms, 4), snapshot_ms=round(snapshot_ms, 4),
                snapshot_in_steps=round(snapshot_ms/step_ms, 3), outside=counts["outside"], samples=counts["samples"]))
    snapshot.close()
    push.work.context.close()


if __name__ == "__main__":
    main()
