#!/usr/bin/env python3
"""A/B of the flux volumes' generator kernel (flux_volume_kernel of csrc/flux_profile.hip) against the route that was
there before it: the same quadrature points and weights generated in numpy, uploaded once and deposited with
FluxProfile.add (flux_deposit_kernel).  Same tree, alternating pairs in one process, HIP events around deposits that end
in a stream synchronise; the states of a pair must be the same bytes.  One JSON line per measurement; a run writes its
output file anew.

    python profiles/flux_volumes_ab.py [--pairs 3] [--calls 5] [--sub 64] [--out profiles/flux_volumes_ab.jsonl]
    rocprofv3 --kernel-trace --stats -d /tmp/volume_trace -- python profiles/flux_volumes_ab.py --only generator --cells 64 --out /dev/null

Workload: tests/golden/efit_tables.npz (64 x 64 table cells) at sub = 64, 1.68e7 points, on 64 and 256 uniform cells of
the label between 0 and 1.  The generator reads nothing per point where `add` reads 32 B; for `add` the time to generate
the points in numpy and to upload them is reported as well, once (`generate_ms`, `upload_ms`).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGIN = 0.02


def quadrature(tables, sub):
    """(R, 0, z, w) of every point by the contract of include/gf_hip.h, one numpy operation per line of it."""
    import numpy as np
    numr, numz = tables["psi_c00"].shape
    row = numz*sub
    t = np.arange(numr*sub*row, dtype=np.int64)
    rmin, dr, zmin, dz = (np.float64(tables[k]) for k in ("rmin", "dr", "zmin", "dz"))
    twice = np.float64(2*sub)
    r = rmin + dr*((2*(t//row) + 1).astype(np.float64)/twice)
    z = zmin + dz*((2*(t % row) + 1).astype(np.float64)/twice)
    area = (dr/np.float64(sub))*(dz/np.float64(sub))
    return [r, np.zeros(t.size), z, r*area]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--pairs", type=int, default=None, help="default: 3, or 1 with --only")
    parser.add_argument("--calls", type=int, default=5, help="deposits of all points per measurement")
    parser.add_argument("--sub", type=int, default=64)
    parser.add_argument("--only", choices=["generator", "add"], default=None, help="one route (one pair unless --pairs is given): for a profiler run")
    parser.add_argument("--cells", type=int, default=None)
    parser.add_argument("--tables", default=os.path.join(ROOT, "tests", "golden", "efit_tables.npz"))
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "flux_volumes_ab.jsonl"))
    args = parser.parse_args()

    import numpy as np
    import torch
    from graph_framework_amd import Context, _lib, key_of
    from graph_framework_amd.flux import FluxProfile

    tables = dict(np.load(args.tables))
    routes = [args.only] if args.only else ["generator", "add"]
    pairs = args.pairs if args.pairs else (1 if args.only else 3)
    stream = torch.cuda.Stream()
    context = Context(0, stream.cuda_stream)
    open(args.out, "w").close()                              # a run's lines replace the file's

    keys, generate_ms, upload_ms, count = [], None, None, None
    if "add" in routes:
        start = time.perf_counter()
        columns = quadrature(tables, args.sub)
        generate_ms = (time.perf_counter() - start)*1.0e3
        count = columns[0].size
        start = time.perf_counter()
        for name, column in zip(("x", "y", "z", "value"), columns):
            key = "volume_%s" % name
            context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), count, _lib.GFIR_F64))
            context.copy_to_device(key, column)
            keys.append(key)
        context.wait()
        upload_ms = (time.perf_counter() - start)*1.0e3
        del columns

    for cells in ([args.cells] if args.cells else [64, 256]):
        edges = np.linspace(0.0, 1.0, cells + 1)
        timings = {}
        for pair in range(pairs):
            states = {}
            for route in routes:
                profile = FluxProfile(context, tables, edges)
                info = profile.info()

                def deposit():
                    if route == "generator":
                        profile.add_volumes(args.sub)
                    else:
                        profile.add(*keys, count)

                deposit()                                    # warm: code object, tables in cache
                context.wait()
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(stream)
                for _ in range(args.calls):
                    deposit()
                stop.record(stream)
                stream.synchronize()
                ms = start.elapsed_time(stop)/args.calls
                counts = profile.counts()
                states[route] = (profile.state().tobytes(), counts)
                profile.close()
                points = counts["samples"]//(args.calls + 1)
                line = dict(sub=args.sub, cells=cells, route=route, pair=pair, ms_per_call=round(ms, 4), points_per_call=points,
                            points_per_s=points/(ms*1.0e-3), private_sums=info["private_sums"],
                            workgroup_size=info["workgroup_size"], max_workgroups=info["max_workgroups"],
                            lds_bytes=info["lds_bytes"], outside=counts["outside"], samples=counts["samples"])
                if route == "add":
                    line.update(generate_ms=round(generate_ms, 1), upload_ms=round(upload_ms, 1),
                                ms_per_call_with_generation=round(ms + generate_ms + upload_ms, 1))
                print(json.dumps(line), flush=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
                timings.setdefault(route, []).append(ms)
            if len(states) == 2 and states["generator"] != states["add"]:
                sys.exit("the two routes disagree on %d cells, pair %d" % (cells, pair))
        if len(timings) == 2:
#  The expectation: the generator's device time does not exceed add's; MARGIN is the pair-to-pair spread the flux
#  profile's A/B recorded.
            ratio = float(np.median(timings["generator"])/np.median(timings["add"]))
            line = dict(sub=args.sub, cells=cells, generator_over_add=round(ratio, 4), margin=MARGIN, expectation_held=ratio <= 1.0 + MARGIN)
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
    context.close()


if __name__ == "__main__":
    main()
