#!/usr/bin/env python3
"""A/B of the particle source's two routes (csrc/particle_source.hip), after the method of profiles/moments_ab.py: every
mode warmed, alternating rounds, HIP events around fills that end in a stream synchronise.  One JSON line per measurement,
then one summary line per mode with the median of the rounds and their range; a run writes its output file anew.

    python profiles/particle_source_ab.py [--rounds 3] [--fills 3] [--out profiles/particle_source_ab.jsonl]

1e7 fp32 particles in the box (1.2, 2.3, -1, 1) of the fixture, 4096 attempts (nobody stays unplaced), at three label ranges
whose acceptance per attempt is about 0.5, 0.2 and 0.04: [0, 0.4), [0, 0.2) and [0, 0.045).  Modes: plain_<level> and
refill_<level>; every line carries the counters, the acceptance they give and the time per attempt.
Then, for scale, on the particles of the middle level as they lie on the device:
  phase_f32    PhaseDistribution.add at 4 x 4 x 4 cells, private, no weight (one field evaluation per particle)
  label_f64    FluxProfile.label of the same positions widened to fp64 (one label per particle, nothing else)
and the whole start of a run, each once after a warm-up of its own:
  start_host   the example's ensemble() on the host, Korc(...) with the copy to the device, compile(), pre_run()
  start_load   Korc(blank), compile(), load(), pre_run()
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

BOX = (1.2, 2.3, -1.0, 1.0)
LEVELS = (("0.5", (0.0, 0.4)), ("0.2", (0.0, 0.2)), ("0.04", (0.0, 0.045)))
SPEED = (0.3, 0.9)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--fills", type=int, default=3, help="fills of all particles per measurement")
    parser.add_argument("--particles", type=int, default=10000000)
    parser.add_argument("--attempts", type=int, default=4096)
    parser.add_argument("--tables", default=os.path.join(ROOT, "tests", "golden", "efit_tables.npz"))
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "particle_source_ab.jsonl"))
    args = parser.parse_args()

    import numpy as np
    import torch
    from graph_framework_amd import Context, _lib, key_of, korc
    from graph_framework_amd.distribution import PhaseDistribution, pitch_edges
    from graph_framework_amd.flux import FluxProfile
    from graph_framework_amd.source import ParticleSource
    from push_particles import ensemble

    tables = dict(np.load(args.tables))
    count = args.particles
    stream = torch.cuda.Stream()
    context = Context(0, stream.cuda_stream)
    keys = list(korc.PARTICLE)
    open(args.out, "w").close()                              # a run's lines replace the file's

    def record(line):
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    def timed(enqueue, repeats):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(stream)
        for _ in range(repeats):
            enqueue()
        end.record(stream)
        stream.synchronize()
        return begin.elapsed_time(end)/repeats

    modes = [("%s_%s" % (route, level), route, label_range) for level, label_range in LEVELS for route in ("plain", "refill")]

    def made(route, label_range):
        return ParticleSource(context, tables, BOX, label_range, SPEED, seed=1, attempts=args.attempts, dtype=np.float32,
                              **{route: True})

    times = {mode: [] for mode, _, _ in modes}
    for mode, route, label_range in modes:                   # every mode warmed before the first round
        source = made(route, label_range)
        source.fill(*keys, count)
        context.wait()
        source.close()
    for round_number in range(args.rounds):
        for mode, route, label_range in modes:
            source = made(route, label_range)
            info = source.info()
            source.fill(*keys, count)                        # warm: this object's tables in cache
            context.wait()
            ms = timed(lambda: source.fill(*keys, count), args.fills)
            counters = source.counts()
            source.close()
            tries = counters["position_tries"]/(args.fills + 1)
            times[mode].append(ms)
            record(dict(mode=mode, round=round_number, ms_per_fill=round(ms, 4), particles=count,
                        particles_per_s=count/(ms*1.0e-3), attempts_per_particle=round(tries/count, 4),
                        acceptance=round(counters["placed"]/counters["position_tries"], 4), ns_per_attempt=round(ms*1.0e6/tries, 5),
                        refill=info["refill"], workgroup_size=info["workgroup_size"], max_workgroups=info["max_workgroups"],
                        **counters))
    for mode, values in times.items():
        record(dict(summary=mode, median_ms=round(statistics.median(values), 4), min_ms=round(min(values), 4),
                    max_ms=round(max(values), 4), rounds=len(values)))

#  For scale: the middle level's particles through a distribution and through a label-only pass.
    source = made("plain", LEVELS[1][1])
    source.fill(*keys, count)
    tries = source.counts()["position_tries"]
    source.close()
    phase = PhaseDistribution(context, tables, np.linspace(0.0, 0.2, 5), pitch_edges(4), np.linspace(-0.5, 0.5, 5))
    phase.add(*keys, count)
    context.wait()
    phase_ms = timed(lambda: phase.add(*keys, count), args.fills)
    counts = phase.counts()
    phase.close()
    wide = ["x_f64", "y_f64", "z_f64", "label_f64"]
    for key, name in zip(wide, ("x", "y", "z", "x")):
        context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), count, _lib.GFIR_F64))
        context.copy_to_device(key, context.copy_to_host(name, np.empty(count, dtype=np.float32)).astype(np.float64))
    profile = FluxProfile(context, tables, np.linspace(0.0, 0.2, 5))
    profile.label(*wide, count)
    context.wait()
    label_ms = timed(lambda: profile.label(*wide, count), args.fills)
    profile.close()
    middle = {route: statistics.median(times["%s_%s" % (route, LEVELS[1][0])]) for route in ("plain", "refill")}
    record(dict(scale="phase_f32", particles=count, ms_per_add=round(phase_ms, 4), ns_per_particle=round(phase_ms*1.0e6/count, 5),
                outside=counts["outside"], samples=counts["samples"]))
    record(dict(scale="label_f64", particles=count, ms_per_pass=round(label_ms, 4), ns_per_label=round(label_ms*1.0e6/count, 5)))
    for route, ms in middle.items():
        record(dict(scale="fill_%s_%s" % (route, LEVELS[1][0]), ms_per_fill=round(ms, 4), attempts=tries,
                    ns_per_attempt=round(ms*1.0e6/tries, 5), attempt_in_phase_particles=round(ms/tries/(phase_ms/count), 4),
                    attempt_in_labels=round(ms/tries/(label_ms/count), 4), fill_in_phase_adds=round(ms/phase_ms, 3)))
    context.close()

#  The whole start of a run.
    def start_host():
        clock = time.perf_counter()
        particles = ensemble(count, 0)
        generated = time.perf_counter()
        push = korc.Korc(particles, "f32")
        push.compile()
        compiled = time.perf_counter()
        push.pre_run()
        push.wait()
        done = time.perf_counter()
        push.work.context.close()
        return dict(generate_s=generated - clock, construct_compile_s=compiled - generated, pre_run_s=done - compiled, total_s=done - clock)

    def start_load():
        clock = time.perf_counter()
        push = korc.Korc(korc.blank(count), "f32")
        push.compile()
        compiled = time.perf_counter()
        source = ParticleSource(push.work.context, tables, BOX, LEVELS[1][1], SPEED, seed=1, attempts=args.attempts, dtype=np.float32)
        push.load(source, placed="placed")
        push.wait()
        loaded = time.perf_counter()
        push.pre_run()
        push.wait()
        done = time.perf_counter()
        push.work.context.close()
        return dict(construct_compile_s=compiled - clock, load_s=loaded - compiled, pre_run_s=done - loaded, total_s=done - clock)

    for name, start in (("start_host", start_host), ("start_load", start_load)):
        start()                                              # warm: code objects loaded, pages touched
        record(dict(scale=name, particles=count, **{k: round(v, 4) for k, v in start().items()}))


if __name__ == "__main__":
    main()
