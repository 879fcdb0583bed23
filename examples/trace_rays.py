#!/usr/bin/env python3
"""Trace a beam through the EFIT equilibrium and write the trajectories — the flow of
graph_driver/xrays.cpp:419-461 (per device: initial distribution, Newton solve for kx, RK4 steps
with a record every `sub_steps`, result<rank>.nc) on the MI355X backend.

    python examples/trace_rays.py --rays 100000 --steps 1000 --sub-steps 100 [--output /tmp/rays]
    python examples/trace_rays.py --rays 10000 --dispersion ordinary_wave --steps 20000 --sub-steps 1000 --output /tmp/rays --absorption-model weak_damping
    python examples/trace_rays.py --rays 10000 --dispersion ordinary_wave --steps 20000 --sub-steps 1000 --output /tmp/rays --absorption-model weak_damping --bins 32,32,32 --bin-box 1.0,2.6,-0.4,0.4,-0.4,0.4
    python examples/trace_rays.py --rays 10000 --dispersion ordinary_wave --steps 20000 --sub-steps 1000 --output /tmp/rays --absorption-model weak_damping --bins 32,32,32 --bin-box 1.0,2.6,-0.4,0.4,-0.4,0.4 --one-pass
    python examples/trace_rays.py --rays 10000 --dispersion ordinary_wave --steps 20000 --sub-steps 1000 --output /tmp/rays --absorption-model weak_damping --flux-bins 64 --flux-tables tests/golden/efit_tables.npz --one-pass
    python examples/trace_rays.py --rays 10000 --dispersion ordinary_wave --steps 20000 --sub-steps 1000 --output /tmp/rays --absorption-model weak_damping --flux-bins 64 --flux-tables tests/golden/efit_tables.npz --flux-density 16 --flux-window 1.0,2.4,-1.0,1.0
    python examples/trace_rays.py --rays 10000 --dispersion ordinary_wave --steps 20000 --sub-steps 1000 --output /tmp/rays --absorption-model weak_damping --flux-bins 16 --flux-tables tests/golden/efit_tables.npz --npar-bins 16 --npar-range -1,1 --one-pass
    python examples/trace_rays.py --rays 10000 --dispersion ordinary_wave --steps 20000 --sub-steps 1000 --output /tmp/rays --absorption-model weak_damping --flux-bins 64 --flux-tables tests/golden/efit_tables.npz --flux-batches 16 --one-pass
    python examples/trace_rays.py --equilibrium vmec --rays 20000 --steps 10 --sub-steps 2 --output /tmp/vmec_rays
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/trace_rays.py ...

One process per GPU; the ensemble is split as the reference splits it over device threads; every rank
writes its own file (as the reference does).  The exported work items fix dt = 1e-3.
With --absorption-model the two stages that follow the trace in graph_driver/xrays.cpp:1100-1105 run on
the same file: calculate_power (kamp per stored record) and bin_power (power, d_power).  With --bins and
--bin-box as well, bin_power also bins d_power on that grid as it goes (utilities/bin.py's profile, exact sums)
and the rank writes <output>_bins<rank>.nc: its own rays' sums divided by its own ray count.
With --flux-bins and --flux-tables (alone or next to --bins) d_power is also binned on flux surfaces
(graph_framework_amd/flux.py) and the rank writes <output>_flux<rank>.nc; with --flux-density [SUB] (and --flux-window)
the file also holds the cells' volumes and the power density, bins/volume.
With --npar-bins N (and --npar-range) next to --flux-bins d_power is also binned over the flux label and the parallel
refractive index N = c (k.B)/(|B| w) (graph_framework_amd/spectrum.py) and the rank writes <output>_spectrum<rank>.nc.
With --flux-batches G the profile and the spectrum are also summed per batch of rays (graph_framework_amd/batches.py: ray r
of the whole ensemble belongs to batch (r >> 6) % G) and their files get stderr, the standard error of bins from the
spread of the batch means, with batch_bins and batch_rays.
With --one-pass as well the same work items run on every record while the trace holds it in device memory
(graph_framework_amd/pipeline.py): same file, same bits, written once, and no pass over the file afterwards.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def vmec_beam(count, seed, device):
    """A beam in the flux coordinates of the VMEC equilibrium: omega = 400, starting surfaces s in [0.3, 0.8], random
    poloidal and toroidal angles, k pointing inwards (k_s = -40: |k| ~ 0.9 omega on these surfaces, then the Newton solve),
    small random k_u, k_v — the ensemble of tests/golden/make_vmec_trace_golden.py at any size."""
    import numpy as np
    from graph_framework_amd.xrays import RaySolver
    rng = np.random.default_rng(seed)
    state = dict(t=np.zeros(count), w=np.full(count, 400.0), x=rng.uniform(0.3, 0.8, count), y=rng.uniform(0.0, 2.0*np.pi, count),
                 z=rng.uniform(0.0, 2.0*np.pi, count), kx=np.full(count, -40.0), ky=rng.uniform(-2.0, 2.0, count),
                 kz=rng.uniform(-20.0, 20.0, count))
    return RaySolver(state, index=device, device_state=True, workload_prefix="vmec86_")


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rays", type=int, default=100000, help="ensemble size over all ranks")
    parser.add_argument("--steps", type=int, default=1000)
    parser.add_argument("--sub-steps", type=int, default=100, help="steps between trajectory records")
    parser.add_argument("--output", default=None, help="prefix of the result files (default: no output)")
    parser.add_argument("--dispersion", choices=["cold_plasma", "ordinary_wave"], default="cold_plasma",
                        help="exported combinations: cold_plasma (dt = 1e-3, xrays_bench) and ordinary_wave (dt = 1e-4, the CLI example's)")
    parser.add_argument("--equilibrium", choices=["efit", "vmec"], default="efit",
                        help="efit: graph_tests/efit.nc, Cartesian rays (the benchmark's); vmec: graph_tests/vmec.nc, all 86 Fourier modes, "
                             "rays in flux coordinates (x, y, z = s, u, v; graph_driver/xrays.cpp:382), cold_plasma, dt = 1e-3 — the RK4 step "
                             "is a 54 k-record item that runs as 10 segment kernels")
    parser.add_argument("--absorption-model", choices=["weak_damping", "root_find"], default=None,
                        help="after the trace: kamp and power into the result file (needs --output)")
    parser.add_argument("--bins", default=None, metavar="NX,NY,NZ",
                        help="with --absorption-model and --bin-box: the deposition profile of utilities/bin.py on this grid")
    parser.add_argument("--bin-box", default=None, metavar="X0,X1,Y0,Y1,Z0,Z1", help="the box the grid divides")
    parser.add_argument("--flux-bins", type=int, default=None, metavar="N",
                        help="with --absorption-model and --flux-tables: absorbed power on N uniform cells of the flux label")
    parser.add_argument("--flux-tables", default=None, metavar="FILE.npz",
                        help="the EFIT tables under efit.nc's dataset names (psi_c00 .. psi_c33, rmin, dr, zmin, dz, psimin, dpsi)")
    parser.add_argument("--flux-range", default="0,1", metavar="LOW,HIGH", help="the label range the cells divide")
    parser.add_argument("--flux-sqrt", action="store_true", help="label sqrt((psi - psimin)/span) instead of (psi - psimin)/span")
    parser.add_argument("--flux-density", type=int, nargs="?", const=16, default=None, metavar="SUB",
                        help="with --flux-bins: also the cells' volumes (every table cell cut into SUB x SUB, default 16) and "
                             "the power density bins/volume, as volume and density in <output>_flux<rank>.nc")
    parser.add_argument("--flux-window", default=None, metavar="RLO,RHI,ZLO,ZHI",
                        help="with --flux-density: only the part of the map with RLO <= R < RHI and ZLO <= z < ZHI counts as volume")
    parser.add_argument("--flux-batches", type=int, default=None, metavar="G",
                        help="with --flux-bins: the sums of the flux profile (and of the spectrum) also per batch of rays, G "
                             "batches of the whole ensemble (1 to 256), and their standard error as stderr next to bins")
    parser.add_argument("--npar-bins", type=int, default=None, metavar="N",
                        help="with --flux-bins and --flux-tables: absorbed power also over N uniform cells of the parallel "
                             "refractive index, as <output>_spectrum<rank>.nc")
    parser.add_argument("--npar-range", default="-1,1", metavar="LOW,HIGH", help="the range of N the cells divide")
    parser.add_argument("--one-pass", action="store_true",
                        help="with --output and --absorption-model: kamp, power and the bins of every record while the rays are "
                             "traced, instead of two more passes over the file")
#  "--npar-range -1,1": a range that begins with a minus sign is no option; hand it over as --npar-range=-1,1
    argv = sys.argv[1:]
    for at in range(len(argv) - 1):
        if argv[at] == "--npar-range":
            argv[at:at + 2] = ["--npar-range=" + argv[at + 1]]
            break
    args = parser.parse_args(argv)
    if (args.bins is None) != (args.bin_box is None):
        parser.error("--bins and --bin-box go together")
    if (args.flux_bins is None) != (args.flux_tables is None):
        parser.error("--flux-bins and --flux-tables go together")
    if args.flux_bins is not None and not (args.output and args.absorption_model):
        parser.error("--flux-bins needs --output and --absorption-model")
    if args.flux_density is not None and args.flux_bins is None:
        parser.error("--flux-density needs --flux-bins")
    if args.flux_window is not None and args.flux_density is None:
        parser.error("--flux-window needs --flux-density")
    if args.flux_batches is not None and args.flux_bins is None:
        parser.error("--flux-batches needs --flux-bins")
    if args.npar_bins is not None and args.flux_bins is None:
        parser.error("--npar-bins needs --flux-bins and --flux-tables")
    if args.npar_range != "-1,1" and args.npar_bins is None:
        parser.error("--npar-range needs --npar-bins")
    if args.one_pass and not (args.output and args.absorption_model):
        parser.error("--one-pass needs --output and --absorption-model")

    import numpy as np
    import torch
    from graph_framework_amd import distributed
    from graph_framework_amd.output import TrajectoryWriter
    from graph_framework_amd.xrays import Rk4ColdPlasmaEfit, cli_distribution, shard_bounds

    rank, world, local_rank = distributed.init()
    torch.cuda.set_device(local_rank)
    begin, end = shard_bounds(args.rays, world, rank)
    if args.equilibrium == "vmec":
        solve = vmec_beam(end - begin, rank, local_rank)
    else:
        solve = Rk4ColdPlasmaEfit(cli_distribution(end - begin, seed=rank), index=local_rank, device_state=True,
                                  dispersion=args.dispersion)
    residual = solve.init("kx")
    solve.compile()
    path = "%s%d.nc" % (args.output, rank) if args.output else None

    def deposition_grid():
        """(context, grid, cells, edges) of --bins/--bin-box."""
        from graph_framework_amd import Context
        from graph_framework_amd.deposition import Deposition
        cells = [int(v) for v in args.bins.split(",")]
        box = [float(v) for v in args.bin_box.split(",")]
        edges = [np.linspace(box[2*a], box[2*a + 1], cells[a] + 1) for a in range(3)]
        context = Context(local_rank)
        return context, Deposition(context, *edges), cells, edges

    def write_deposition(context, deposition, cells, edges):
        from graph_framework_amd.output import write_bins
        counts = deposition.counts()
        bins = deposition.read(end - begin)
        deposition.close()
        context.close()
        write_bins("%s_bins%d.nc" % (args.output, rank), bins, *edges, **counts)
        print("rank %d: deposition on %s cells: %d samples, %d outside, %d skipped; sum of bins %.6e"
              % (rank, "x".join(str(c) for c in cells), counts["samples"], counts["outside"], counts["skipped"],
                 float(bins.sum())))

    def flux_profile():
        """(context, profile) of --flux-bins/--flux-tables/--flux-range/--flux-sqrt."""
        from graph_framework_amd import Context
        from graph_framework_amd.flux import FluxProfile
        low, high = (float(v) for v in args.flux_range.split(","))
        tables = dict(np.load(args.flux_tables))
        context = Context(local_rank)
        return context, FluxProfile(context, tables, np.linspace(low, high, args.flux_bins + 1), sqrt_label=args.flux_sqrt,
                                    batches=args.flux_batches)

    def batch_statistics(cells, what):
        """(bins, the writer's keywords) of a profile or spectrum with --flux-batches: this rank's rays are begin .. end
        of the ensemble."""
        from graph_framework_amd.batches import largest_relative_error
        from graph_framework_amd.flux import marginal_bins
        bins = marginal_bins(cells, end - begin)
        extra = cells.error_variables(begin, end - begin)
        print("rank %d: %s in %d batches of rays: largest relative standard error %.3e among the cells above 1 %% of the peak"
              % (rank, what, args.flux_batches, largest_relative_error(bins, extra["stderr"])))
        return bins, extra

    def write_flux(context, profile):
        from graph_framework_amd.output import write_flux_bins
        counts = profile.counts()
        extra = {}
        if args.flux_batches is not None:
            bins, extra = batch_statistics(profile, "flux profile")
        else:
            bins = profile.read(end - begin)
        edges, psi0, span, kind = profile.edges, profile.psi0, profile.span, profile.label_kind
        if args.flux_density is not None:
            from graph_framework_amd.flux import density_variables
            window = [float(v) for v in args.flux_window.split(",")] if args.flux_window else None
            extra.update(density_variables(profile, bins, args.flux_density, window))
        profile.close()
        context.close()
        write_flux_bins("%s_flux%d.nc" % (args.output, rank), bins, edges, psi0, span, kind, **counts, **extra)
        print("rank %d: flux profile on %d cells of %s: %d samples, %d outside, %d skipped; sum of bins %.6e"
              % (rank, bins.size, kind, counts["samples"], counts["outside"], counts["skipped"], float(bins.sum())))

    def flux_spectrum():
        """(context, spectrum) of --npar-bins/--npar-range on the label cells of --flux-bins."""
        from graph_framework_amd import Context
        from graph_framework_amd.spectrum import FluxSpectrum
        low, high = (float(v) for v in args.flux_range.split(","))
        npar_low, npar_high = (float(v) for v in args.npar_range.split(","))
        tables = dict(np.load(args.flux_tables))
        context = Context(local_rank)
#  The tracer's w is omega/c (its dispersion relations read wpe2 + k.k - w*w), so N = k.B/(|B| w): c = 1.
        return context, FluxSpectrum(context, tables, np.linspace(low, high, args.flux_bins + 1),
                                     np.linspace(npar_low, npar_high, args.npar_bins + 1), sqrt_label=args.flux_sqrt, c=1.0,
                                     batches=args.flux_batches)

    def write_spectrum(context, spectrum):
        from graph_framework_amd.output import write_spectrum_bins
        counts = spectrum.counts()
        extra = {}
        if args.flux_batches is not None:
            bins, extra = batch_statistics(spectrum, "spectrum")
        else:
            bins = spectrum.read(end - begin)
        kind = spectrum.label_kind
        write_spectrum_bins("%s_spectrum%d.nc" % (args.output, rank), bins, spectrum.sedges, spectrum.nedges, spectrum.psi0,
                            spectrum.span, kind, spectrum.c, **counts, **extra)
        spectrum.close()
        context.close()
        print("rank %d: spectrum on %dx%d cells of %s and N: %d samples, %d outside, %d skipped; sum of bins %.6e"
              % (rank, bins.shape[0], bins.shape[1], kind, counts["samples"], counts["outside"], counts["skipped"],
                 float(bins.sum())))

    grid = None
    surfaces = None
    waves = None
    if args.one_pass:
        from graph_framework_amd.pipeline import OnePass
        grid = deposition_grid() if args.bins else None
        surfaces = flux_profile() if args.flux_bins else None
        waves = flux_spectrum() if args.npar_bins else None
        writer = OnePass(solve.work.context, end - begin, path, model=args.absorption_model, index=local_rank,
                         stream=solve.torch_stream.cuda_stream, deposition=grid[1] if grid else None,
                         flux=surfaces[1] if surfaces else None, spectrum=waves[1] if waves else None, first_ray=begin)
        write_step = writer.record
    else:
        writer = TrajectoryWriter(solve, path) if args.output else None
        write_step = writer.write_step if writer else None
    if writer:
        write_step()

    start = time.perf_counter()
    for step in range(args.steps):
        solve.step()
        if writer and (step + 1) % args.sub_steps == 0:
            write_step()
    host = solve.sync_host()
    elapsed = time.perf_counter() - start
    after = time.perf_counter()
    if writer:
        writer.close()
    lost = int((~np.isfinite(host["x"])).sum())          # rays the reference graph itself drives to NaN
    print("rank %d: %d rays, Newton %d iterations (max residual %.3e), %d steps in %.3f s = %.3e ray-steps/s; "
          "x in [%.4f, %.4f], %d rays non-finite, status flags %d"
          % (rank, end - begin, solve.newton_iterations, residual, args.steps, elapsed,
             (end - begin)*args.steps/elapsed, np.nanmin(host["x"]), np.nanmax(host["x"]), lost,
             solve.work.context.flags()))
    if writer and args.absorption_model:
        from graph_framework_amd.output import ResultFile
        solve.work.context.close()
        records = args.steps//args.sub_steps
        if args.one_pass:
            start = after                                        # what is left after the trace: the last writes, the grid
            if grid:
                write_deposition(*grid)
            if surfaces:
                write_flux(*surfaces)
            if waves:
                write_spectrum(*waves)
        else:
            from graph_framework_amd.absorption import bin_power, run_absorption
            start = time.perf_counter()
            run_absorption(path, records, index=local_rank, model=args.absorption_model)
            grid = deposition_grid() if args.bins else None
            surfaces = flux_profile() if args.flux_bins else None
            waves = flux_spectrum() if args.npar_bins else None
            bin_power(path, records, index=local_rank, deposition=grid[1] if grid else None,
                      flux=surfaces[1] if surfaces else None, spectrum=waves[1] if waves else None, first_ray=begin)
            if grid:
                write_deposition(*grid)
            if surfaces:
                write_flux(*surfaces)
            if waves:
                write_spectrum(*waves)
        elapsed = time.perf_counter() - start
        result = ResultFile(path)
        power = result.read("power", records)
        result.close()
        kept = power[np.isfinite(power) & (power <= 1.0)]
        print("rank %d: absorption (%s) + power over %d records in %.3f s; transmitted power %.4f (mean over %d of %d rays "
              "with a power in [0, 1])" % (rank, args.absorption_model, records + 1, elapsed,
                                          float(kept.mean()) if kept.size else float("nan"), kept.size, power.size))


if __name__ == "__main__":
    main()
