//------------------------------------------------------------------------------
///  @file cell_deposit.hpp
///  @brief The pieces of a deposit that every deposit kernel shares (device side): deposition.hip and, through
///  flux_sums.hpp, flux_profile.hip, flux_spectrum.hip, phase_bins.hip, moment_bins.hip and confinement.hip.
///
///  A store of exact sums is cells x 67 limbs of superacc.hpp, [cell][limb], and three counters (samples, outside,
///  skipped).  The deposit kernels differ in how a sample finds its cell and in where the limbs live (global
///  memory, or a workgroup's LDS); what a sample adds, how the counters are kept and how the limbs are added to is
///  written here, once.
//------------------------------------------------------------------------------
#ifndef GFHIP_CELL_DEPOSIT_HPP
#define GFHIP_CELL_DEPOSIT_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "superacc.hpp"

namespace gfhip {
namespace deposit {

//  The cell of `c` among the n + 1 increasing edges `e` (LDS), or -1: outside [e[0], e[n]) or NaN.
//  The guess from the uniform spacing is right or off by one for linspace edges; the stored edges decide.
__device__ __forceinline__ int find_cell(const double *e, const int n, const double scale, const double c) {
    if (!(c >= e[0] && c < e[n])) return -1;
    const double t = (c - e[0])*scale;
    int g = t >= 0.0 && t < static_cast<double> (n) ? static_cast<int> (t) : 0;
    if (c >= e[g] && c < e[g + 1]) return g;
    if (g + 1 < n && c >= e[g + 1] && c < e[g + 2]) return g + 1;
    if (g > 0 && c >= e[g - 1] && c < e[g]) return g - 1;
    int low = 0, high = n;                             // e[low] <= c < e[high]
    while (high - low > 1) {
        const int middle = (low + high)/2;
        if (c >= e[middle]) {
            low = middle;
        } else {
            high = middle;
        }
    }
    return low;
}

__device__ __forceinline__ long long wave_sum(long long v) {
    for (int offset = 32; offset > 0; offset >>= 1) v += __shfl_xor(v, offset, 64);
    return v;
}

//  What one sample adds: `c0`, `c1`, `c2` to the limbs `key & 63` and the two after it of cell `key >> 6`.
//  All zero when the sample is outside (`cell` is then ignored) or its value is NaN or infinite; a zero value adds nothing either.
struct contribution {
    bool inside, finite;
    unsigned int key;                                  // cell*64 + first limb
    long long c0, c1, c2;
};

__device__ __forceinline__ contribution contribution_of(const bool inside, const unsigned int cell, const double value) {
    contribution a = {inside, superacc::is_finite(value), 0u, 0, 0, 0};
    if (a.inside && a.finite) {
        const superacc::pieces p = superacc::split(value);
        a.key = cell*64u + static_cast<unsigned int> (p.first);
        a.c0 = p.negative ? -static_cast<long long> (p.chunk[0]) : static_cast<long long> (p.chunk[0]);
        a.c1 = p.negative ? -static_cast<long long> (p.chunk[1]) : static_cast<long long> (p.chunk[1]);
        a.c2 = p.negative ? -static_cast<long long> (p.chunk[2]) : static_cast<long long> (p.chunk[2]);
    }
    return a;
}

//  The three counters of a launch as a wave keeps them (wave-uniform).
struct tallies {
    unsigned long long seen = 0, outside = 0, skipped = 0;
};

//  Executed by whole waves, `present` false in the lanes past the end.
__device__ __forceinline__ void count(tallies &t, const bool present, const contribution &a) {
    t.seen += __popcll(__ballot(present));
    t.outside += __popcll(__ballot(present && !a.inside));
    t.skipped += __popcll(__ballot(present && a.inside && !a.finite));
}

//  counters: samples, outside, skipped.  Lane 0 of each wave adds its wave's.
__device__ __forceinline__ void flush(const tallies &t, unsigned long long *counters) {
    if ((threadIdx.x & 63u) == 0) {
        if (t.seen) atomicAdd(counters, t.seen);
        if (t.outside) atomicAdd(counters + 1, t.outside);
        if (t.skipped) atomicAdd(counters + 2, t.skipped);
    }
}

//  At most three 64-bit integer atomic adds on adjacent limbs of `base` ([cell][limb]; global memory or LDS: the
//  function is inlined and the address space is the caller's).  The results are unused: no-return atomics,
//  global_atomic_add_x2 or ds_add_u64.  A zero chunk adds nothing.
__device__ __forceinline__ void add_limbs(unsigned long long *base, const unsigned int key,
                                          const long long c0, const long long c1, const long long c2) {
    unsigned long long *limb = base + static_cast<size_t> (key >> 6)*superacc::limbs + (key & 63u);
    if (c0) atomicAdd(limb, static_cast<unsigned long long> (c0));
    if (c1) atomicAdd(limb + 1, static_cast<unsigned long long> (c1));
    if (c2) atomicAdd(limb + 2, static_cast<unsigned long long> (c2));
}

//  add_limbs behind the wave-uniform pre-sum, executed by whole waves: when every adding lane has the same cell and the
//  same first limb (identical rays: every wave, every record), the chunks are summed over the wave and lane 0 adds for
//  all, three atomics per wave.  Exact: the limbs are integers.
__device__ __forceinline__ void add_limbs_presummed(unsigned long long *base, const contribution &a) {
    const bool adds = (a.c0 | a.c1 | a.c2) != 0;
    const unsigned long long adders = __ballot(adds);
    if (adders == 0) return;                           // wave-uniform
    const unsigned int first = __builtin_amdgcn_readlane(a.key, __ffsll(static_cast<long long> (adders)) - 1);
    if (__ballot(adds && a.key != first) == 0) {
        const long long c0 = wave_sum(a.c0), c1 = wave_sum(a.c1), c2 = wave_sum(a.c2);
        if ((threadIdx.x & 63u) == 0) add_limbs(base, first, c0, c1, c2);
    } else {
        add_limbs(base, a.key, a.c0, a.c1, a.c2);
    }
}

}  // namespace deposit
}  // namespace gfhip

#endif
