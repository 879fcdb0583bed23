#!/usr/bin/env python3
"""A/B of the batched flux deposit (flux_deposit_rays_kernel, csrc/flux_profile.hip) against the plain one on the same
samples in the same tree, by the method of profiles/spectrum_ab.py: alternating rounds in one process, HIP events around
adds that end in a stream synchronise.  After every round the batched profile's total() is compared with the plain
profile's state.  One JSON line per measurement; a run writes its output file anew.

    python profiles/flux_batches_ab.py [--pairs 3] [--adds 5] [--out profiles/flux_batches_ab.jsonl]
    rocprofv3 --kernel-trace --stats -d /tmp/batches_trace -- python profiles/flux_batches_ab.py --input cli_beam --pairs 1 --out /dev/null

Inputs, 1e7 samples each, those of profiles/spectrum_ab.py: `identical` and `cli_beam`; the samples are the rays 0 .. 1e7
of an ensemble.  Modes, 64 label cells each, uniform on the range the samples cover:
    batched         16 batches, a workgroup sums one batch at a time in LDS (64 cells of it)
    profile         FluxProfile.add, no batches: the yardstick
    batched_global  16 batches without private sums: the batch as part of the cell, 1024 superaccumulators in memory
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

FLOOR_BYTES, PEAK = 32, 8.0e12                               # read per sample; HBM bytes per second
CELLS, BATCHES = 64, 16
MODES = ("batched", "profile", "batched_global")


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--pairs", type=int, default=3)
    parser.add_argument("--adds", type=int, default=5, help="adds of 1e7 samples per measurement")
    parser.add_argument("--rays", type=int, default=100000)
    parser.add_argument("--records", type=int, default=100)
    parser.add_argument("--input", choices=["identical", "cli_beam"], default=None)
    parser.add_argument("--tables", default=os.path.join(ROOT, "tests", "golden", "efit_tables.npz"))
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "flux_batches_ab.jsonl"))
    args = parser.parse_args()

    import numpy as np
    import torch
    from graph_framework_amd import Context, _lib, key_of
    from graph_framework_amd.flux import FluxProfile, label_host
    from spectrum_ab import inputs

    tables = dict(np.load(args.tables))
    data = inputs(args.rays, args.records)
    count = args.rays*args.records
    stream = torch.cuda.Stream()
    context = Context(0, stream.cuda_stream)
    open(args.out, "w").close()                              # a run's lines replace the file's
    for name in ([args.input] if args.input else ["cli_beam", "identical"]):
        columns = [data[name][k] for k in (0, 1, 2, 7)]
        keys = []
        for column_name, column in zip(("x", "y", "z", "value"), columns):
            key = "%s_%s" % (name, column_name)
            context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), count, _lib.GFIR_F64))
            context.copy_to_device(key, column)
            keys.append(key)
        labels = label_host(tables, *columns[:3])
        finite = labels[np.isfinite(labels)]
        low, high = float(finite.min()), float(np.nextafter(finite.max(), np.inf))
        edges = np.linspace(low, high if high > low else low + 1.0, CELLS + 1)
        made = {"batched": lambda: FluxProfile(context, tables, edges, batches=BATCHES),
                "profile": lambda: FluxProfile(context, tables, edges),
                "batched_global": lambda: FluxProfile(context, tables, edges, batches=BATCHES, private=False)}

        def add(grid):
            if grid.batches is None:
                grid.add(*keys, count)
            else:
                grid.add_rays(*keys, count, 0)

        for pair in range(args.pairs):
            states = {}
            for mode in MODES:
                grid = made[mode]()
                info = grid.info()
                add(grid)                                    # warm: code object, tables in cache
                context.wait()
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(stream)
                for _ in range(args.adds):
                    add(grid)
                stop.record(stream)
                stream.synchronize()
                ms = start.elapsed_time(stop)/args.adds
                counts = grid.counts()
                if grid.batches is None:
                    states[mode] = (grid.state().tobytes(), counts)
                else:
                    total = grid.total()
                    states[mode] = (total.state().tobytes(), total.counts())
                    total.close()
                grid.close()
                line = dict(input=name, mode=mode, shape=list(grid.shape), pair=pair, ms_per_add=round(ms, 4),
                            samples_per_add=count, samples_per_s=count/(ms*1.0e-3),
                            share_of_read_floor=round(count*FLOOR_BYTES/PEAK/(ms*1.0e-3), 4),
                            private_sums=info["private_sums"], workgroup_size=info["workgroup_size"],
                            max_workgroups=info["max_workgroups"], lds_bytes=info["lds_bytes"],
                            outside=counts["outside"], samples=counts["samples"])
                print(json.dumps(line), flush=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            if not states["batched"] == states["profile"] == states["batched_global"]:
                sys.exit("the batched profiles' totals and the plain profile disagree on %s" % name)
    context.close()


if __name__ == "__main__":
    main()
