#!/usr/bin/env python3
"""A/B of the spectrum's deposit kernel (csrc/flux_spectrum.hip) against the flux profile's (csrc/flux_profile.hip) on the
same samples in the same tree: alternating pairs in one process, HIP events around adds that end in a stream synchronise.
After every pair the spectrum's marginal over N is compared with the profile's state.  One JSON line per measurement; a run
writes its output file anew.

    python profiles/spectrum_ab.py [--pairs 3] [--adds 5] [--out profiles/spectrum_ab.jsonl]
    rocprofv3 --kernel-trace --stats -d /tmp/spectrum_trace -- python profiles/spectrum_ab.py --input cli_beam --case private --pairs 1 --out /dev/null

Inputs, 1e7 samples each (100 records of 1e5 rays): `identical` (every ray at one point with one wave vector per record)
and `cli_beam` (the CLI example's beam, walked inwards from x = 2.5 to 1.5, with its own wave vectors).  Cases: `private`,
16 x 16 cells against a profile of 256; `global`, 64 x 32 cells against a profile of 64 without private sums.  The label
cells are uniform on the range the samples cover, the cells of N on the range of their finite N.  w is the tracer's
(in units of c), so c = 1.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOOR_BYTES, PEAK = 64, 8.0e12                               # read per sample; HBM bytes per second
CASES = {"private": (16, 16, 256, True), "global": (64, 32, 64, False)}    # ns, nn, the profile's cells, its private flag


def inputs(rays, records):
    import numpy as np
    from graph_framework_amd.xrays import cli_distribution
    beam = cli_distribution(rays, seed=0)
    rng = np.random.default_rng(0)
    out = {"identical": [[] for _ in range(8)], "cli_beam": [[] for _ in range(8)]}
    for r in range(records):
        inward = 1.0 - 0.4*(r % 20)/20                       # x from 2.5 towards 1.5
        same = (2.5*inward, 0.0, 0.0, -600.0*inward, 50.0, 20.0, 700.0, 1.0e-3*inward)
        for column, value in zip(out["identical"], same):
            column.append(np.full(rays, value))
        pieces = (beam["x"]*inward, beam["y"]*inward, beam["z"].copy(), beam["kx"]*inward, beam["ky"].copy(), beam["kz"].copy(),
                  beam["w"].copy(), rng.uniform(0.0, 1.0e-3, rays))
        for column, piece in zip(out["cli_beam"], pieces):
            column.append(piece)
    return {name: [np.concatenate(column) for column in columns] for name, columns in out.items()}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--pairs", type=int, default=3)
    parser.add_argument("--adds", type=int, default=5, help="adds of 1e7 samples per measurement")
    parser.add_argument("--rays", type=int, default=100000)
    parser.add_argument("--records", type=int, default=100)
    parser.add_argument("--input", choices=["identical", "cli_beam"], default=None)
    parser.add_argument("--case", choices=sorted(CASES), default=None)
    parser.add_argument("--tables", default=os.path.join(ROOT, "tests", "golden", "efit_tables.npz"))
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_ab.jsonl"))
    args = parser.parse_args()

    import numpy as np
    import torch
    from graph_framework_amd import Context, _lib, key_of
    from graph_framework_amd.flux import FluxProfile
    from graph_framework_amd.spectrum import FluxSpectrum, npar_host

    tables = dict(np.load(args.tables))
    data = inputs(args.rays, args.records)
    count = args.rays*args.records
    stream = torch.cuda.Stream()
    context = Context(0, stream.cuda_stream)
    open(args.out, "w").close()                              # a run's lines replace the file's
    for name in ([args.input] if args.input else ["cli_beam", "identical"]):
        columns = data[name]
        keys = []
        for column_name, column in zip(("x", "y", "z", "kx", "ky", "kz", "w", "value"), columns):
            key = "%s_%s" % (name, column_name)
            context._check(context.lib.gfhip_allocate_buffer(context.handle, key_of(key), count, _lib.GFIR_F64))
            context.copy_to_device(key, column)
            keys.append(key)
        labels, npar = npar_host(tables, *columns[:7], c=1.0)
        ranges = []
        for values in (labels, npar):
            finite = values[np.isfinite(values)]
            low, high = float(finite.min()), float(np.nextafter(finite.max(), np.inf))
            ranges.append((low, high if high > low else low + 1.0))
        for case in ([args.case] if args.case else ["private", "global"]):
            ns, nn, cells, private = CASES[case]
            sedges, nedges = np.linspace(*ranges[0], ns + 1), np.linspace(*ranges[1], nn + 1)
            made = {"spectrum": lambda: FluxSpectrum(context, tables, sedges, nedges, c=1.0, private=private),
                    "profile": lambda: FluxProfile(context, tables, np.linspace(*ranges[0], cells + 1), private=private),
                    "marginal": lambda: FluxProfile(context, tables, sedges, private=private)}
            added = {"spectrum": keys, "profile": keys[:3] + keys[7:], "marginal": keys[:3] + keys[7:]}
            for pair in range(args.pairs):
                states = {}
                for mode in ("spectrum", "profile"):
                    grid = made[mode]()
                    info = grid.info()
                    grid.add(*added[mode], count)            # warm: code object, tables in cache
                    context.wait()
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record(stream)
                    for _ in range(args.adds):
                        grid.add(*added[mode], count)
                    stop.record(stream)
                    stream.synchronize()
                    ms = start.elapsed_time(stop)/args.adds
                    counts = grid.counts()
                    if mode == "spectrum":
                        marginal = grid.profile()
                        states[mode] = marginal.state().tobytes()
                        marginal.close()
                    grid.close()
                    line = dict(input=name, case=case, mode=mode, shape=list(grid.shape), pair=pair, ms_per_add=round(ms, 4),
                                samples_per_add=count, samples_per_s=count/(ms*1.0e-3),
                                share_of_read_floor=round(count*(FLOOR_BYTES if mode == "spectrum" else 32)/PEAK/(ms*1.0e-3), 4),
                                private_sums=info["private_sums"], workgroup_size=info["workgroup_size"],
                                max_workgroups=info["max_workgroups"], lds_bytes=info["lds_bytes"],
                                outside=counts["outside"], samples=counts["samples"])
                    print(json.dumps(line), flush=True)
                    with open(args.out, "a") as f:
                        f.write(json.dumps(line) + "\n")
                reference = made["marginal"]()               # the profile's kernel on the spectrum's label edges
                for _ in range(args.adds + 1):
                    reference.add(*added["marginal"], count)
                same = reference.state().tobytes() == states["spectrum"]
                reference.close()
                if not same:
                    sys.exit("the spectrum's marginal and the profile disagree on %s, %s" % (name, case))
    context.close()


if __name__ == "__main__":
    main()
