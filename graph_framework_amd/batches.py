"""Batches of rays: the rule of csrc/ray_batches.hpp on the host, and the batch statistics of a tally.

A cell of a flux profile or a spectrum is a Monte-Carlo estimate, the mean over rays of what each ray left in it.  The
rays are divided into G fixed batches, ray r (its index in the whole ensemble over all ranks and files) into batch
(r >> 6) % G, and the same tally is kept per batch (flux.FluxProfile and spectrum.FluxSpectrum with batches=G); the
spread of the batch means is the standard error of the whole.  The particles of a push are batched by the same rule,
particle p of the whole ensemble over all ranks and shards in place of the ray (distribution.PhaseDistribution and
moments.FluxMoments with batches=G); ratio_error_of is the error of a ratio of two such tallies.  No device, no library:
integers and fp64 numpy.
"""
import numpy as np

CHUNK_SHIFT = 6
CHUNK_RAYS = 1 << CHUNK_SHIFT
MAX_BATCHES = 256


def batch_of(ray, batches):
    """The batch of ray `ray` (an integer or an integer array)."""
    return (ray >> CHUNK_SHIFT) % batches


def _chunks_below(chunk, batches, g):
    return chunk//batches + (1 if chunk % batches > g else 0)


def batch_rays(first, count, batches):
    """int64[batches]: the rays of [first, first + count) in every batch, in closed form (ray_batches.hpp's batch_rays)."""
    first, count, batches = int(first), int(count), int(batches)
    rays = np.zeros(batches, dtype=np.int64)
    if count <= 0:
        return rays
    last = first + count - 1
    low, high = first >> CHUNK_SHIFT, last >> CHUNK_SHIFT
    for g in range(batches):
        n = (_chunks_below(high + 1, batches, g) - _chunks_below(low, batches, g)) << CHUNK_SHIFT
        if low % batches == g:
            n -= first & (CHUNK_RAYS - 1)
        if high % batches == g:
            n -= (CHUNK_RAYS - 1) - (last & (CHUNK_RAYS - 1))
        rays[g] = n
    return rays


def standard_error_of(batch_sums, total, rays, count):
    """(mean, stderr, used) of a batched tally, in fp64: batch_sums (G, ...) the batches' rounded exact sums S_g, total
    (...) the rounded exact sum S of all, rays (G,) the rays n_g of every batch, count their number N.
        P = S/N;  p_g = S_g/n_g;  stderr = sqrt(sum_g n_g (p_g - P)^2 / ((G' - 1) N))
    over the G' = used batches that have rays; NaN with fewer than two of them."""
    sums = np.asarray(batch_sums, dtype=np.float64)
    rays = np.asarray(rays, dtype=np.float64).reshape(-1)
    if sums.shape[0] != rays.size:
        raise ValueError("%d batches of sums, %d of rays" % (sums.shape[0], rays.size))
    mean = np.asarray(total, dtype=np.float64)/float(count)
    occupied = rays > 0.0
    used = int(occupied.sum())
    if used < 2:
        return mean, np.full(sums.shape[1:], np.nan), used
    n = rays[occupied].reshape((-1,) + (1,)*(sums.ndim - 1))
    with np.errstate(invalid="ignore", over="ignore"):
        deviation = sums[occupied]/n - mean
        stderr = np.sqrt((n*deviation*deviation).sum(axis=0)/((used - 1)*float(count)))
    return mean, stderr, used


def ratio_error_of(batch_sums_num, batch_sums_den):
    """The delete-one-batch jackknife standard error of the ratio of two tallied sums, in fp64 from the batches' rounded
    exact sums: batch_sums_num and batch_sums_den (G, ...), S1_g and S0_g.  Over the m batches with particles (those
    where S1_g or S0_g is not zero), with S1 and S0 their sums:
        R_(g) = (S1 - S1_g)/(S0 - S0_g);  Rbar = sum_g R_(g)/m;  se = sqrt((m - 1)/m sum_g (R_(g) - Rbar)^2)
    NaN with fewer than two such batches or where a denominator S0 - S0_g is zero."""
    num = np.asarray(batch_sums_num, dtype=np.float64)
    den = np.asarray(batch_sums_den, dtype=np.float64)
    if num.shape != den.shape or num.ndim < 1:
        raise ValueError("numerator sums of shape %r, denominator sums of shape %r" % (num.shape, den.shape))
    used = (num != 0.0) | (den != 0.0)
    m = used.sum(axis=0).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        num, den = np.where(used, num, 0.0), np.where(used, den, 0.0)
        rest = den.sum(axis=0) - den
        replicate = np.where(used, (num.sum(axis=0) - num)/rest, 0.0)
        mean = replicate.sum(axis=0)/m
        deviation = np.where(used, replicate - mean, 0.0)
        error = np.sqrt((m - 1.0)/m*(deviation*deviation).sum(axis=0))
    broken = (m < 2.0) | (used & (rest == 0.0)).any(axis=0)
    return np.where(broken, np.nan, error)


def largest_relative_error(mean, stderr, threshold=0.01):
    """The largest stderr/|mean| among the cells whose |mean| is above `threshold` of the largest; NaN if there is none."""
    mean, stderr = np.abs(np.asarray(mean, dtype=np.float64)), np.asarray(stderr, dtype=np.float64)
    peak = mean.max() if mean.size else 0.0
    chosen = (mean > threshold*peak) & np.isfinite(stderr)
    return float((stderr[chosen]/mean[chosen]).max()) if chosen.any() else float("nan")
