#!/usr/bin/env python3
"""A/B of the batched particle deposits (moment_deposit_particles_kernel, phase_deposit_particles_kernel) against the
plain ones (FluxMoments.add at 16 and at 64 surfaces, PhaseDistribution.add at 4 x 4 x 4: the yardsticks) on the same
particles in the same process, after the method of profiles/moments_ab.py: every mode warmed, alternating rounds, HIP
events around adds that end in a stream synchronise.  One JSON line per measurement with the ratio to its yardstick of
the same round, then one summary line per mode with the median of the rounds and their range; a run writes its output
file anew.  The script stops unless the total() of every batched object has the bytes of its plain twin's state.

    python profiles/particle_batches_ab.py [--rounds 3] [--adds 5] [--out profiles/particle_batches_ab.jsonl]

The particles, 1e7 fp32: the example's ensemble (examples/push_particles.py) with gamma = sqrt(1 + u.u).  Modes:
  moments_16, moments_64, phase_64       the plain adds (yardsticks)
  moments_16_g16, moments_16_g64         add_particles at 16 surfaces with 16 and 64 batches, private
  moments_64_g16, moments_64_g64         at 64 surfaces (256 cells, the cap: a drain of 137 KB per unit)
  phase_64_g16, phase_64_g64             add_particles at 4 x 4 x 4 cells
  moments_65_g16_global                  65 surfaces: the global path, the batch as part of the cell (once, for the record;
                                         its yardstick is moments_64)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

PEAK = 8.0e12                                                # HBM bytes per second
READ = 28                                                    # bytes per fp32 particle


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--adds", type=int, default=5, help="adds of all particles per measurement")
    parser.add_argument("--particles", type=int, default=10000000)
    parser.add_argument("--tables", default=os.path.join(ROOT, "tests", "golden", "efit_tables.npz"))
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "particle_batches_ab.jsonl"))
    args = parser.parse_args()

    import numpy as np
    import torch
    from graph_framework_amd import Context, _lib, key_of, korc
    from graph_framework_amd.distribution import PhaseDistribution, coordinates_host, pitch_edges
    from graph_framework_amd.moments import FluxMoments
    from push_particles import ensemble

    tables = dict(np.load(args.tables))
    count = args.particles
    start = ensemble(count, 0)
    start["gamma"] = np.sqrt(1.0 + start["ux"]**2 + start["uy"]**2 + start["uz"]**2)
    columns = [start[name].astype(np.float32) for name in korc.PARTICLE]
    stream = torch.cuda.Stream()
    context = Context(0, stream.cuda_stream)
    keys = []
    for name, column in zip(korc.PARTICLE, columns):
        context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(name + "_f32"), count, _lib.GFIR_F32))
        context.copy_to_device(name + "_f32", column)
        keys.append(name + "_f32")
    label, _ = coordinates_host(tables, [c[:200000] for c in columns])
    low, high = float(np.nanmin(label)), float(np.nextafter(np.nanmax(label), np.inf))
    gamma_high = float(np.nextafter(columns[6].max(), np.float32(np.inf)))

    def moments(ns, batches=None):
        return lambda: FluxMoments(context, tables, np.linspace(low, high, ns + 1), batches=batches)

    def phase(batches=None):
        return lambda: PhaseDistribution(context, tables, np.linspace(low, high, 5), pitch_edges(4),
                                         np.linspace(1.0, gamma_high, 5), batches=batches)

    #  mode: (maker, yardstick, rounds it is measured in)
    modes = {"moments_16": (moments(16), None, args.rounds), "moments_64": (moments(64), None, args.rounds),
             "phase_64": (phase(), None, args.rounds),
             "moments_16_g16": (moments(16, 16), "moments_16", args.rounds), "moments_16_g64": (moments(16, 64), "moments_16", args.rounds),
             "moments_64_g16": (moments(64, 16), "moments_64", args.rounds), "moments_64_g64": (moments(64, 64), "moments_64", args.rounds),
             "phase_64_g16": (phase(16), "phase_64", args.rounds), "phase_64_g64": (phase(64), "phase_64", args.rounds),
             "moments_65_g16_global": (moments(65, 16), "moments_64", 1)}
    open(args.out, "w").close()                              # a run's lines replace the file's

    def record(line):
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    def feed(grid):
        if grid.batches is None:
            grid.add(*keys, count)
        else:
            grid.add_particles(*keys, count, 0)

    times = {mode: [] for mode in modes}
    ratios = {mode: [] for mode in modes}
    states = {}
    for mode, (make, _, _) in modes.items():                 # every mode warmed before the first round, and its bytes kept
        grid = make()
        feed(grid)
        context.wait()
        if grid.batches is None:
            states[mode] = (grid.state().tobytes(), grid.counts())
        else:
            total = grid.total()
            states[mode] = (total.state().tobytes(), total.counts())
            total.close()
        grid.close()
    for mode, (_, yardstick, _) in modes.items():
        if yardstick is not None and mode != "moments_65_g16_global" and states[mode] != states[yardstick]:
            sys.exit("the total() of %s does not have the bytes of %s" % (mode, yardstick))
    for round_number in range(args.rounds):
        for mode, (make, yardstick, rounds) in modes.items():
            if round_number >= rounds:
                continue
            grid = make()
            info = grid.info()
            feed(grid)                                       # warm: this object's tables in cache
            context.wait()
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record(stream)
            for _ in range(args.adds):
                feed(grid)
            end.record(stream)
            stream.synchronize()
            ms = begin.elapsed_time(end)/args.adds
            counts = grid.counts()
            grid.close()
            times[mode].append(ms)
            if yardstick is not None:
                ratios[mode].append(ms/times[yardstick][round_number])
            record(dict(mode=mode, shape=list(grid.shape), round=round_number, ms_per_add=round(ms, 4), particles_per_add=count,
                        particles_per_s=count/(ms*1.0e-3), share_of_read_floor=round(count*READ/PEAK/(ms*1.0e-3), 4),
                        yardstick=yardstick, ratio_to_yardstick=round(ratios[mode][-1], 4) if yardstick else None,
                        private_sums=info["private_sums"], workgroup_size=info["workgroup_size"],
                        max_workgroups=info["max_workgroups"], lds_bytes=info["lds_bytes"], outside=counts["outside"],
                        skipped=counts["skipped"], samples=counts["samples"]))
    for mode, values in times.items():
        record(dict(summary=mode, median_ms=round(statistics.median(values), 4), min_ms=round(min(values), 4),
                    max_ms=round(max(values), 4), yardstick=modes[mode][1], ratios_to_yardstick=[round(r, 4) for r in ratios[mode]],
                    rounds=len(values)))
    context.close()


if __name__ == "__main__":
    main()
