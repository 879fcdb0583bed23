#!/usr/bin/env python3
"""A/B of the moment profile's deposit kernel (csrc/moment_bins.hip) against the particle distribution's
(csrc/phase_bins.hip at 4 x 4 x 4 private, fp32: the yardstick) on the same particles in the same process, after the
method of profiles/phase_ab.py: every mode warmed, alternating rounds, HIP events around adds that end in a stream
synchronise.  One JSON line per measurement with the ratio to the round's yardstick, then one summary line per mode with
the median of the rounds and their range; a run writes its output file anew.

    python profiles/moments_ab.py [--rounds 3] [--adds 5] [--out profiles/moments_ab.jsonl]

The particles, 1e7 fp32: the example's ensemble (examples/push_particles.py) with gamma = sqrt(1 + u.u).  Modes:
  phase_f32             PhaseDistribution.add at 4 x 4 x 4 cells, private, no weight
  moments_f32_16        FluxMoments.add at 16 surfaces (64 cells), private
  moments_f32_64        64 surfaces (256 cells, the private path's cap)
  moments_f32_65_global 65 surfaces (260 cells): the global path behind the wave pre-sum
After the rounds moment 0 of moments_f32_16 is compared with a flux profile fed the same positions.
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
READ = 28                                                    # bytes per fp32 particle
YARDSTICK = "phase_f32"


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--adds", type=int, default=5, help="adds of all particles per measurement")
    parser.add_argument("--particles", type=int, default=10000000)
    parser.add_argument("--push-steps", type=int, default=20)
    parser.add_argument("--tables", default=os.path.join(ROOT, "tests", "golden", "efit_tables.npz"))
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_ab.jsonl"))
    args = parser.parse_args()

    import numpy as np
    import torch
    from graph_framework_amd import Context, _lib, key_of, korc
    from graph_framework_amd.distribution import PhaseDistribution, coordinates_host, pitch_edges
    from graph_framework_amd.flux import FluxProfile
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
    wide = ["%s_f64" % name for name in ("x", "y", "z", "one")]     # the comparison's flux profile takes fp64
    for key, column in zip(wide, columns[:3] + [np.ones(count)]):
        context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), count, _lib.GFIR_F64))
        context.copy_to_device(key, column.astype(np.float64))
    label, _ = coordinates_host(tables, [c[:200000] for c in columns])
    low, high = float(np.nanmin(label)), float(np.nextafter(np.nanmax(label), np.inf))
    gamma_high = float(np.nextafter(columns[6].max(), np.float32(np.inf)))

    made = {YARDSTICK: lambda: PhaseDistribution(context, tables, np.linspace(low, high, 5), pitch_edges(4),
                                                 np.linspace(1.0, gamma_high, 5)),
            "moments_f32_16": lambda: FluxMoments(context, tables, np.linspace(low, high, 17)),
            "moments_f32_64": lambda: FluxMoments(context, tables, np.linspace(low, high, 65)),
            "moments_f32_65_global": lambda: FluxMoments(context, tables, np.linspace(low, high, 66))}
    open(args.out, "w").close()                              # a run's lines replace the file's

    def record(line):
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    times = {mode: [] for mode in made}
    ratios = {mode: [] for mode in made}
    first_state = None
    for mode in made:                                        # every mode warmed before the first round
        grid = made[mode]()
        grid.add(*keys, count)
        context.wait()
        grid.close()
    for round_number in range(args.rounds):
        for mode in made:
            grid = made[mode]()
            info = grid.info()
            grid.add(*keys, count)                           # warm: this object's tables in cache
            context.wait()
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record(stream)
            for _ in range(args.adds):
                grid.add(*keys, count)
            end.record(stream)
            stream.synchronize()
            ms = begin.elapsed_time(end)/args.adds
            counts = grid.counts()
            if mode == "moments_f32_16" and first_state is None:
                marginal = grid.profile()
                first_state = marginal.state().tobytes()
                marginal.close()
            grid.close()
            times[mode].append(ms)
            ratios[mode].append(ms/times[YARDSTICK][round_number])
            record(dict(mode=mode, shape=list(grid.shape), round=round_number, ms_per_add=round(ms, 4), particles_per_add=count,
                        particles_per_s=count/(ms*1.0e-3), share_of_read_floor=round(count*READ/PEAK/(ms*1.0e-3), 4),
                        ratio_to_yardstick=round(ratios[mode][-1], 4), private_sums=info["private_sums"],
                        workgroup_size=info["workgroup_size"], max_workgroups=info["max_workgroups"], lds_bytes=info["lds_bytes"],
                        outside=counts["outside"], skipped=counts["skipped"], samples=counts["samples"]))
    reference = FluxProfile(context, tables, np.linspace(low, high, 17))
    for _ in range(args.adds + 1):
        reference.add(*wide, count)
    same = reference.state().tobytes() == first_state
    reference.close()
    if not same:
        sys.exit("moment 0 of the moment profile and the flux profile disagree")
    for mode, values in times.items():
        record(dict(summary=mode, median_ms=round(statistics.median(values), 4), min_ms=round(min(values), 4),
                    max_ms=round(max(values), 4), ratios_to_yardstick=[round(r, 4) for r in ratios[mode]], rounds=len(values)))
    context.close()

    push = korc.Korc(ensemble(count, 0), "f32")
    push.compile()
    push.pre_run()
    snapshot = FluxMoments(push.work.context, tables, np.linspace(low, high, 17))
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
                snapshot_in_steps=round(snapshot_ms/step_ms, 3), outside=counts["outside"], skipped=counts["skipped"],
                samples=counts["samples"]))
    snapshot.close()
    push.work.context.close()


if __name__ == "__main__":
    main()
