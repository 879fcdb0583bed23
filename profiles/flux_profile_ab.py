#!/usr/bin/env python3
"""A/B of the flux profile's deposit kernel (csrc/flux_profile.hip): workgroup-private sums in LDS against deposits
straight to the global state (private=False), in the same tree, alternating pairs in one process, HIP events around
adds that end in a stream synchronise.  One JSON line per measurement; a run writes its output file anew.

    python profiles/flux_profile_ab.py [--pairs 3] [--adds 5] [--out profiles/flux_profile_ab.jsonl]
    rocprofv3 --kernel-trace --stats -d /tmp/flux_trace -- python profiles/flux_profile_ab.py --only private --input cli_beam --cells 64 --out /dev/null
    rocprofv3 --pmc TCC_EA0_ATOMIC_sum -d /tmp/flux_pmc -- python profiles/flux_profile_ab.py --only private --input cli_beam --cells 64 --out /dev/null

Inputs, 1e7 samples each (100 records of 1e5 rays, as bench_extra.py's deposition): `identical` (every ray at one point
per record: the wave-uniform pre-sum) and `cli_beam` (the CLI example's beam, walked inwards from x = 2.5 to 1.5).
Cells: 64 and the private path's cap, uniform on the label range the samples cover.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOOR_BYTES, PEAK = 32, 8.0e12                               # read per sample; HBM bytes per second


def inputs(rays, records):
    import numpy as np
    from graph_framework_amd.xrays import cli_distribution
    beam = cli_distribution(rays, seed=0)
    rng = np.random.default_rng(0)
    out = {"identical": [[] for _ in range(4)], "cli_beam": [[] for _ in range(4)]}
    for r in range(records):
        inward = 1.0 - 0.4*(r % 20)/20                       # x from 2.5 towards 1.5
        for column, piece in zip(out["identical"], (np.full(rays, 2.5*inward), np.zeros(rays), np.zeros(rays), np.full(rays, 1.0e-3*inward))):
            column.append(piece)
        for column, piece in zip(out["cli_beam"], (beam["x"]*inward, beam["y"]*inward, beam["z"].copy(), rng.uniform(0.0, 1.0e-3, rays))):
            column.append(piece)
    return {name: [np.concatenate(column) for column in columns] for name, columns in out.items()}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--pairs", type=int, default=None, help="default: 3, or 1 with --only")
    parser.add_argument("--adds", type=int, default=5, help="adds of 1e7 samples per measurement")
    parser.add_argument("--rays", type=int, default=100000)
    parser.add_argument("--records", type=int, default=100)
    parser.add_argument("--only", choices=["private", "global"], default=None, help="one mode (one pair unless --pairs is given): for a profiler run")
    parser.add_argument("--input", choices=["identical", "cli_beam"], default=None)
    parser.add_argument("--cells", type=int, default=None)
    parser.add_argument("--tables", default=os.path.join(ROOT, "tests", "golden", "efit_tables.npz"))
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "flux_profile_ab.jsonl"))
    args = parser.parse_args()

    import numpy as np
    import torch
    from graph_framework_amd import Context, _lib, key_of
    from graph_framework_amd.flux import FluxProfile, label_host

    tables = dict(np.load(args.tables))
    data = inputs(args.rays, args.records)
    count = args.rays*args.records
    stream = torch.cuda.Stream()
    context = Context(0, stream.cuda_stream)
    probe = FluxProfile(context, tables, [0.0, 1.0])
    cap = probe.info()["cap_cells"]
    probe.close()
    modes = [args.only] if args.only else ["private", "global"]
    pairs = args.pairs if args.pairs else (1 if args.only else 3)
    open(args.out, "w").close()                              # a run's lines replace the file's
    for name in ([args.input] if args.input else ["cli_beam", "identical"]):
        columns = data[name]
        keys = []
        for column_name, column in zip(("x", "y", "z", "value"), columns):
            key = "%s_%s" % (name, column_name)
            context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), count, _lib.GFIR_F64))
            context.copy_to_device(key, column)
            keys.append(key)
        labels = label_host(tables, *columns[:3])
        low, high = float(np.nanmin(labels)), float(np.nextafter(np.nanmax(labels), np.inf))
        if not high > low:
            high = low + 1.0
        for cells in ([args.cells] if args.cells else [64, cap]):
            edges = np.linspace(low, high, cells + 1)
            occupied = int(np.unique(np.searchsorted(edges, labels[np.isfinite(labels)], side="right")).size)
            states = {}
            for pair in range(pairs):
                for mode in modes:
                    profile = FluxProfile(context, tables, edges, private=mode == "private")
                    info = profile.info()
                    profile.add(*keys, count)                # warm: code object, tables in cache
                    context.wait()
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record(stream)
                    for _ in range(args.adds):
                        profile.add(*keys, count)
                    stop.record(stream)
                    stream.synchronize()
                    ms = start.elapsed_time(stop)/args.adds
                    counts = profile.counts()
                    states[mode] = profile.state().tobytes()
                    profile.close()
                    line = dict(input=name, cells=cells, mode=mode, pair=pair, ms_per_add=round(ms, 4), samples_per_add=count,
                                samples_per_s=count/(ms*1.0e-3), share_of_read_floor=round(count*FLOOR_BYTES/PEAK/(ms*1.0e-3), 4),
                                private_sums=info["private_sums"], workgroup_size=info["workgroup_size"],
                                max_workgroups=info["max_workgroups"], lds_bytes=info["lds_bytes"], occupied_cells=occupied,
                                outside=counts["outside"], samples=counts["samples"])
                    print(json.dumps(line), flush=True)
                    with open(args.out, "a") as f:
                        f.write(json.dumps(line) + "\n")
            if len(states) == 2 and states["private"] != states["global"]:
                sys.exit("the two paths disagree on %s, %d cells" % (name, cells))
    context.close()


if __name__ == "__main__":
    main()
