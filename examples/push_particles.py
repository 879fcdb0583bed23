#!/usr/bin/env python3
"""Push an ensemble of runaway electrons through the EFIT equilibrium (graph_korc/xkorc.cpp's workflow,
graph_framework_amd/korc.py) and follow its distribution over the flux label, the pitch cosine and gamma
(graph_framework_amd/distribution.py): every `--every` steps the particles are binned where they lie on the device, on the
push's own stream, into a fresh exact distribution, and the snapshots are written to <output>_phase_bins.nc
(output.write_phase_bins).  With --loss-limit the particles are also tracked for their first exit through the flux surface
of that label (graph_framework_amd/confinement.py) at every snapshot: the snapshots then hold the confined particles
only, the confined fraction is printed per snapshot, and the losses over R, z and gamma go to <output>_loss_bins.nc.
With --moments NS every snapshot also gets the exact density, parallel current, kinetic energy and radiated power on NS
flux surfaces of the label range (graph_framework_amd/moments.py), under the same weights; the total current and energy
are printed per snapshot and the profiles go to <output>_moment_bins.nc, with --moments-density SUB also per volume.
With --particle-batches G the distribution and the moments are kept per batch of particles (graph_framework_amd/batches.py):
the totals are printed with their standard error, and the files also get stderr, batch_bins and batch_particles (the
moments' file means_stderr as well, the error of the moments per unit of density).

    python examples/push_particles.py --particles 1000000 --steps 200 --every 50 --flux-tables tests/golden/efit_tables.npz --output /tmp/korc
    python examples/push_particles.py --particles 100000 --dtype f64 --label-bins 16 --label-range 0,0.4 --pitch-bins 8 --gamma-bins 8 --gamma-range 1,3 --flux-tables tests/golden/efit_tables.npz
    python examples/push_particles.py --particles 1000000 --loss-limit 0.06 --loss-bins 32,32,8 --flux-tables tests/golden/efit_tables.npz --output /tmp/korc
    python examples/push_particles.py --particles 1000000 --moments 32 --moments-density 8 --flux-tables tests/golden/efit_tables.npz --output /tmp/korc
    python examples/push_particles.py --particles 1000000 --moments 32 --particle-batches 64 --loss-limit 0.06 --flux-tables tests/golden/efit_tables.npz --output /tmp/korc
    python examples/push_particles.py --particles 1000000 --load-label-range 0,0.3 --load-box 1.2,2.3,-1,1 --load-speed 0.3,0.9 --flux-tables tests/golden/efit_tables.npz

The start positions are spread around the axis and the start momenta in size and pitch, seeded.  The push conserves gamma
in a static field: the largest change of the gamma marginal between the first and the last snapshot is printed, the first
thing to check after a run.  The pitch axis is pitch_edges(--pitch-bins): uniform on [-1, 1], its last edge just above 1.
With --load-label-range LOW,HIGH the ensemble comes from a particle source instead (graph_framework_amd/source.py): drawn
on the device, uniform in volume between the two flux surfaces inside --load-box, speeds of --load-speed and pitches of
--load-pitch against the local field.  A particle that found no position in --load-attempts candidates is unplaced and
takes no part: its `placed` column is the weight of every snapshot (a tracker counts it lost at the first check).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ensemble(count, seed):
    """Seeded start values: positions in a box around the axis, momenta of 0.3 to 0.9 c at pitch angles all round."""
    import numpy as np
    rng = np.random.default_rng(seed)
    size = rng.uniform(0.3, 0.9, count)
    cosine = rng.uniform(-1.0, 1.0, count)
    turn = rng.uniform(0.0, 2.0*np.pi, count)
    across = size*np.sqrt(1.0 - cosine*cosine)
    return dict(x=rng.uniform(1.5, 1.9, count), y=rng.uniform(-0.2, 0.2, count), z=rng.uniform(-0.3, 0.3, count),
                ux=across*np.cos(turn), uy=size*cosine, uz=across*np.sin(turn), gamma=np.zeros(count))


def pair(text):
    low, high = (float(v) for v in text.split(","))
    return low, high


def triple(text):
    nr, nz, ng = (int(v) for v in text.split(","))
    return nr, nz, ng


def box(text):
    rlo, rhi, zlo, zhi = (float(v) for v in text.split(","))
    return rlo, rhi, zlo, zhi


def stacked(per_snapshot):
    """The snapshots' dictionaries of arrays as one dictionary of arrays with the time axis first."""
    import numpy as np
    return {name: np.stack([each[name] for each in per_snapshot]) for name in per_snapshot[0]}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--particles", type=int, default=100000)
    parser.add_argument("--steps", type=int, default=200)
    parser.add_argument("--every", type=int, default=50, help="steps between two snapshots of the distribution")
    parser.add_argument("--dtype", choices=["f32", "f64"], default="f32", help="the push's state (the benchmark's is f32)")
    parser.add_argument("--label-bins", type=int, default=16)
    parser.add_argument("--label-range", type=pair, default=(0.0, 0.4), metavar="LOW,HIGH")
    parser.add_argument("--pitch-bins", type=int, default=8)
    parser.add_argument("--gamma-bins", type=int, default=8)
    parser.add_argument("--gamma-range", type=pair, default=(1.0, 3.0), metavar="LOW,HIGH")
    parser.add_argument("--sqrt-label", action="store_true", help="label = sqrt((psi - psi0)/span)")
    parser.add_argument("--loss-limit", type=float, default=None, metavar="L",
                        help="track first exits: a particle is lost once its label is not below L")
    parser.add_argument("--loss-bins", type=triple, default=(16, 16, 8), metavar="NR,NZ,NG", help="cells of the loss footprint")
    parser.add_argument("--loss-box", type=box, default=None, metavar="RLO,RHI,ZLO,ZHI",
                        help="the footprint's extent in R and z (default: the map's)")
    parser.add_argument("--moments", type=int, default=None, metavar="NS",
                        help="also bin density, current, energy and radiated power on NS surfaces of --label-range")
    parser.add_argument("--moments-density", type=int, default=None, metavar="SUB",
                        help="with --moments: the file also gets the surfaces' volumes (quadrature SUB) and the moments per volume")
    parser.add_argument("--particle-batches", type=int, default=None, metavar="G",
                        help="keep the distribution and the moments per batch of particles, 1 to 256: error bars")
    parser.add_argument("--load-label-range", type=pair, default=None, metavar="LOW,HIGH",
                        help="draw the ensemble on the device, uniform in volume between these two flux labels")
    parser.add_argument("--load-box", type=box, default=None, metavar="RLO,RHI,ZLO,ZHI",
                        help="with --load-label-range: where positions are tried (default: the map)")
    parser.add_argument("--load-speed", type=pair, default=(0.3, 0.9), metavar="LOW,HIGH", help="|v|/c of the loaded particles")
    parser.add_argument("--load-pitch", type=pair, default=(-1.0, 1.0), metavar="LOW,HIGH", help="their pitch cosine to the local field")
    parser.add_argument("--load-attempts", type=int, default=64, help="positions tried per particle before it stays unplaced")
    parser.add_argument("--flux-tables", required=True, help="an .npz with efit.nc's psi and fpol tables (tests/golden/efit_tables.npz)")
    parser.add_argument("--output", default=None, help="prefix of <output>_phase_bins.nc (default: no file)")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--device", type=int, default=0)
    args = parser.parse_args()
    if args.every < 1 or args.steps < args.every:
        parser.error("--every needs 1 <= every <= steps")
    if args.moments is not None and args.moments < 1 or args.moments is None and args.moments_density is not None:
        parser.error("--moments needs NS >= 1, and --moments-density needs --moments")
    if args.particle_batches is not None and not 1 <= args.particle_batches <= 256:
        parser.error("--particle-batches needs 1 <= G <= 256")

    import numpy as np
    from graph_framework_amd import korc
    from graph_framework_amd.distribution import PhaseDistribution, pitch_edges
    from graph_framework_amd.output import write_loss_bins, write_phase_bins

    tables = dict(np.load(args.flux_tables))
    sedges = np.linspace(*args.label_range, args.label_bins + 1)
    pedges = pitch_edges(args.pitch_bins)
    gedges = np.linspace(*args.gamma_range, args.gamma_bins + 1)
    loaded = args.load_label_range is not None
    push = korc.Korc(korc.blank(args.particles) if loaded else ensemble(args.particles, args.seed), args.dtype, index=args.device)
    push.compile()
    placed_key = None
    if loaded:
        from graph_framework_amd.source import ParticleSource
        numr, numz = tables["psi_c00"].shape
        rmin, dr, zmin, dz = (float(tables[k]) for k in ("rmin", "dr", "zmin", "dz"))
        source = ParticleSource(push.work.context, tables, args.load_box or (rmin, rmin + numr*dr, zmin, zmin + numz*dz),
                                args.load_label_range, args.load_speed, args.load_pitch, seed=args.seed,
                                attempts=args.load_attempts, dtype=args.dtype, sqrt_label=args.sqrt_label)
        placed_key = "placed"
        push.load(source, placed=placed_key)
        load_counts = source.counts()
        source.close()
    push.pre_run()
    tracker = None
    if args.loss_limit is not None:
        from graph_framework_amd.confinement import Confinement
        numr, numz = tables["psi_c00"].shape
        rmin, dr, zmin, dz = (float(tables[k]) for k in ("rmin", "dr", "zmin", "dz"))
        rlo, rhi, zlo, zhi = args.loss_box or (rmin, rmin + numr*dr, zmin, zmin + numz*dz)
        nr, nz, ng = args.loss_bins
        tracker = Confinement(push.work.context, tables, np.linspace(rlo, rhi, nr + 1), np.linspace(zlo, zhi, nz + 1),
                              np.linspace(*args.gamma_range, ng + 1), args.particles, args.dtype, limit=args.loss_limit,
                              sqrt_label=args.sqrt_label, capacity=args.steps//args.every)

    profiles = []
    if args.moments is not None:
        from graph_framework_amd.moments import MOMENTS, FluxMoments
        from graph_framework_amd.output import write_moment_bins
        medges = np.linspace(*args.label_range, args.moments + 1)
    snapshots, steps, done = [], [], 0
    while done + args.every <= args.steps:
        push.run(args.every)
        done += args.every
        snapshot = PhaseDistribution(push.work.context, tables, sedges, pedges, gedges, sqrt_label=args.sqrt_label,
                                     batches=args.particle_batches)
        if tracker is not None:
            push.track(tracker)                              # settles the particles that have left since the last snapshot
        weight = tracker.alive_key if tracker is not None else placed_key
        push.bin(snapshot, weight=weight)                    # behind the steps on the push's stream; the particles stay put
        snapshots.append(snapshot)
        steps.append(done)
        if args.moments is not None:
            profiles.append(FluxMoments(push.work.context, tables, medges, sqrt_label=args.sqrt_label, batches=args.particle_batches))
            push.bin(profiles[-1], weight=weight)
    batched = args.particle_batches is not None
    errors, moment_errors = {}, {}
    if batched:
        from graph_framework_amd.batches import standard_error_of
        from graph_framework_amd.flux import marginal_bins
        bins = np.stack([marginal_bins(snapshot) for snapshot in snapshots])
        errors = stacked([snapshot.sum_error_variables(push.first_particle, args.particles) for snapshot in snapshots])
    else:
        bins = np.stack([snapshot.read() for snapshot in snapshots])
    counts = [snapshot.counts() for snapshot in snapshots]
    kind, psi0, span = snapshots[0].label_kind, snapshots[0].psi0, snapshots[0].span
    for snapshot in snapshots:
        snapshot.close()
    if profiles:
        moment_bins = np.stack([marginal_bins(profile) if batched else profile.read() for profile in profiles])
        moment_totals = np.stack([profile.totals() for profile in profiles])
        if batched:
            moment_errors = stacked([profile.sum_error_variables(push.first_particle, args.particles) for profile in profiles])
            moment_errors["means_stderr"] = np.stack([profile.means_error() for profile in profiles])
#  The totals' error: N times the standard error of the per-particle mean, from the batches' sums over the surfaces.
            total_errors = np.stack([args.particles*standard_error_of(profile.read().sum(axis=1), total,
                                                                      profile.batch_rays(push.first_particle, args.particles),
                                                                      args.particles)[1]
                                     for profile, total in zip(profiles, moment_totals)])
        moment_counts = [profile.counts() for profile in profiles]
        volume = profiles[0].volumes(args.moments_density) if args.moments_density is not None else None
        for profile in profiles:
            profile.close()
    if tracker is not None:
        history, lost, loss_counts = tracker.history(), tracker.read(), tracker.counts()
        tracker.close()
    push.work.context.close()

    print("%d particles (%s), %d steps, %d snapshots on %dx%dx%d cells of %s, xi and gamma"
          % (args.particles, args.dtype, done, len(steps), args.label_bins, args.pitch_bins, args.gamma_bins, kind))
    if loaded:
        print("loaded between %s = %g and %g: %d placed, %d unplaced, %.3f position attempts per particle"
              % ((kind,) + tuple(args.load_label_range) + (load_counts["placed"], load_counts["unplaced"],
                                                           load_counts["position_tries"]/args.particles)))
    for step, count, snapshot in zip(steps, counts, bins):
        print("  step %6d: %d in a cell, %d outside, %d skipped" % (step, int(snapshot.sum()), count["outside"], count["skipped"]))
    marginal = bins.sum(axis=(1, 2))                         # (time, ng): small integers, exact in fp64
    print("largest change of the gamma marginal between the first and the last snapshot: %d particles of %d"
          % (int(np.abs(marginal[-1] - marginal[0]).max()), args.particles))
    if tracker is not None:
        print("first exits through %s = %g, on %dx%dx%d cells of R, z and gamma:" % ((kind, args.loss_limit) + tracker.shape))
        for step, newly, confined in zip(history["steps"], history["newly_lost"], history["confined"]):
            print("  step %6d: %d newly lost, confined fraction %.6f" % (step, newly, confined/args.particles))
        print("  %d lost in all, %d of them outside the footprint's cells" % (loss_counts["samples"], loss_counts["outside"]))
        if args.output:
            path = args.output + "_loss_bins.nc"
            write_loss_bins(path, lost, tracker.redges, tracker.zedges, tracker.gedges, tracker.limit, tracker.psi0, tracker.span,
                            kind, **history, **loss_counts)
            print("wrote %s" % path)
    if profiles:
        print("moments on %d surfaces of %s (normalised units%s):" % (args.moments, kind, ", confined particles" if tracker is not None else ""))
        current, energy = MOMENTS.index("current"), MOMENTS.index("energy")
        for at, (step, total, count) in enumerate(zip(steps, moment_totals, moment_counts)):
            if batched:
                print("  step %6d: total current %.9e +- %.3e, total energy %.9e +- %.3e, %d outside, %d skipped"
                      % (step, total[current], total_errors[at][current], total[energy], total_errors[at][energy],
                         count["outside"], count["skipped"]))
            else:
                print("  step %6d: total current %.9e, total energy %.9e, %d outside, %d skipped"
                      % (step, total[current], total[energy], count["outside"], count["skipped"]))
        if args.output:
            path = args.output + "_moment_bins.nc"
            extra = {}
            if volume is not None:
                with np.errstate(divide="ignore", invalid="ignore"):
                    extra = dict(volume=volume, sub=args.moments_density,
                                 density=np.where(volume[None, :, None] == 0.0, np.nan, moment_bins/volume[None, :, None]))
            write_moment_bins(path, moment_bins, medges, psi0, span, kind, totals=moment_totals, steps=steps,
                              **{name: [count[name] for count in moment_counts] for name in ("samples", "outside", "skipped")}, **extra,
                              **moment_errors)
            print("wrote %s" % path)
    if args.output:
        path = args.output + "_phase_bins.nc"
        write_phase_bins(path, bins, sedges, pedges, gedges, psi0, span, kind, steps=steps,
                         **{name: [count[name] for count in counts] for name in ("samples", "outside", "skipped")}, **errors)
        print("wrote %s" % path)


if __name__ == "__main__":
    main()
