#!/usr/bin/env python3
"""A/B of the first-exit check (csrc/confinement.hip) against the particle distribution's deposit kernel
(csrc/phase_bins.hip at 4 x 4 x 4 private, fp32: the yardstick) on the same particles in the same process, after the method
of profiles/phase_ab.py: alternating rounds, HIP events around calls that end in a stream synchronise.  One JSON line per
measurement, then one summary line per mode with the median of the rounds and their range; a run writes its output file
anew.

    python profiles/confinement_ab.py [--rounds 3] [--calls 5] [--out profiles/confinement_ab.jsonl]

The particles, 1e7, fp32: the example's ensemble (examples/push_particles.py) with gamma = sqrt(1 + u.u).  Modes:
  phase_f32          PhaseDistribution.add at 4 x 4 x 4 cells (private sums), no weight
  check_confined     Confinement.check with a limit above every label: every lane reads x, y, z and the 16 coefficients,
                     nobody is lost, nothing is written
  check_settled      the same tracker after one check with a limit below every label: every lane reads lost_step alone
A check of a mixed ensemble lies between the two.  The first check of check_settled's tracker, in which all 1e7 particles
are lost at once and deposit, is timed once per round as check_all_lost: the worst case, which a run meets at most once.
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
READ = {"phase_f32": 28, "check_confined": 16, "check_settled": 4, "check_all_lost": 24}     # bytes per particle


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--calls", type=int, default=5, help="calls on all particles per measurement")
    parser.add_argument("--particles", type=int, default=10000000)
    parser.add_argument("--tables", default=os.path.join(ROOT, "tests", "golden", "efit_tables.npz"))
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "confinement_ab.jsonl"))
    args = parser.parse_args()

    import numpy as np
    import torch
    from graph_framework_amd import Context, _lib, key_of, korc
    from graph_framework_amd.confinement import Confinement
    from graph_framework_amd.distribution import PhaseDistribution, coordinates_host, pitch_edges
    from push_particles import ensemble

    tables = dict(np.load(args.tables))
    count = args.particles
    start = ensemble(count, 0)
    start["gamma"] = np.sqrt(1.0 + start["ux"]**2 + start["uy"]**2 + start["uz"]**2)
    columns = [start[name] for name in korc.PARTICLE]
    stream = torch.cuda.Stream()
    context = Context(0, stream.cuda_stream)
    keys = []
    for name, column in zip(korc.PARTICLE, columns):
        context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(name), count, _lib.GFIR_F32))
        context.copy_to_device(name, column.astype(np.float32))
        keys.append(name)
    label, _ = coordinates_host(tables, [c[:200000].astype(np.float32) for c in columns])
    low, high = float(np.nanmin(label)), float(np.nextafter(np.nanmax(label), np.inf))
    gamma_high = float(np.nextafter(columns[6].max(), np.inf))
    numr, numz = tables["psi_c00"].shape
    rmin, dr, zmin, dz = (float(tables[k]) for k in ("rmin", "dr", "zmin", "dz"))
    box = (np.linspace(rmin, rmin + numr*dr, 17), np.linspace(zmin, zmin + numz*dz, 17), np.linspace(1.0, gamma_high, 9))
    open(args.out, "w").close()                              # a run's lines replace the file's

    def record(line):
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    def timed(call, calls):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(stream)
        for number in range(calls):
            call(number)
        end.record(stream)
        stream.synchronize()
        return begin.elapsed_time(end)/calls

    modes = ("phase_f32", "check_confined", "check_settled")
    times = {mode: [] for mode in modes + ("check_all_lost",)}
    for round_number in range(args.rounds):
        for mode in modes:
            if mode == "phase_f32":
                grid = PhaseDistribution(context, tables, np.linspace(low, high, 5), pitch_edges(4), np.linspace(1.0, gamma_high, 5))
                grid.add(*keys, count)                       # warm: code object, tables in cache
                context.wait()
                ms = timed(lambda number: grid.add(*keys, count), args.calls)
                seen = grid.counts()["samples"]
            else:
                settled = mode == "check_settled"
                grid = Confinement(context, tables, *box, count, "f32", limit=-np.inf if settled else np.inf,
                                   alive="alive_" + mode, capacity=args.calls + 1)
                context.wait()
                first = timed(lambda number: grid.check(*keys, 0), 1)                     # warm; of check_settled: everybody leaves
                if settled:
                    times["check_all_lost"].append(first)
                    record(dict(mode="check_all_lost", round=round_number, ms_per_call=round(first, 4), particles_per_call=count,
                                share_of_read_floor=round(count*READ["check_all_lost"]/PEAK/(first*1.0e-3), 4)))
                ms = timed(lambda number: grid.check(*keys, 1 + number), args.calls)
                seen = grid.counts()["samples"]
                if seen != (count if settled else 0) or grid.confined() != (0 if settled else count):
                    sys.exit("%s: %d lost, %d confined" % (mode, seen, grid.confined()))
            info = grid.info()
            grid.close()
            times[mode].append(ms)
            record(dict(mode=mode, shape=list(grid.shape), round=round_number, ms_per_call=round(ms, 4), particles_per_call=count,
                        particles_per_s=count/(ms*1.0e-3), share_of_read_floor=round(count*READ[mode]/PEAK/(ms*1.0e-3), 4),
                        private_sums=info["private_sums"], workgroup_size=info["workgroup_size"],
                        max_workgroups=info["max_workgroups"], lds_bytes=info["lds_bytes"], samples=seen))
    for mode, values in times.items():
        record(dict(summary=mode, median_ms=round(statistics.median(values), 4), min_ms=round(min(values), 4),
                    max_ms=round(max(values), 4), rounds=len(values)))
    context.close()


if __name__ == "__main__":
    main()
