#!/usr/bin/env python3
"""A/B of examples/trace_rays.py with and without --one-pass: alternating pairs in child processes, one JSON line per
run (the wall clock of the trace loop, of everything after it, and of the process) appended to the output file.

    python profiles/one_pass_ab.py [--pairs 3] [--out profiles/one_pass_ab.jsonl] [--prefix /tmp/one_pass_ab]
"""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGUMENTS = ["--rays", "100000", "--dispersion", "ordinary_wave", "--steps", "20000", "--sub-steps", "100",
             "--absorption-model", "weak_damping", "--bins", "32,32,32", "--bin-box", "1.0,2.6,-0.4,0.4,-0.4,0.4"]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--pairs", type=int, default=3)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "one_pass_ab.jsonl"))
    parser.add_argument("--prefix", default="/tmp/one_pass_ab")
    parser.add_argument("--timeout", type=float, default=300.0)
    args = parser.parse_args()
    for pair in range(args.pairs):
        for mode, flag in (("three_stages", []), ("one_pass", ["--one-pass"])):
            start = time.perf_counter()
            out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "trace_rays.py")] + ARGUMENTS
                                 + ["--output", "%s_%s_" % (args.prefix, mode)] + flag,
                                 capture_output=True, text=True, timeout=args.timeout)
            wall = time.perf_counter() - start
            if out.returncode != 0:                      # nothing more is started behind a run that failed
                sys.stderr.write(out.stdout + out.stderr)
                sys.exit(out.returncode)
            trace = float(re.search(r"steps in ([0-9.]+) s", out.stdout).group(1))
            after = float(re.search(r"records in ([0-9.]+) s", out.stdout).group(1))
            line = dict(mode=mode, pair=pair, trace_s=trace, after_s=after, total_s=round(trace + after, 3),
                        process_s=round(wall, 3), transmitted=float(re.search(r"transmitted power ([0-9.naninf]+)", out.stdout).group(1)),
                        sum_of_bins=float(re.search(r"sum of bins ([0-9.e+-]+)", out.stdout).group(1)), arguments=" ".join(ARGUMENTS + flag))
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            for left in glob.glob("%s_%s_*.nc" % (args.prefix, mode)):     # 2 GB per trajectory file at this size
                os.remove(left)


if __name__ == "__main__":
    main()
