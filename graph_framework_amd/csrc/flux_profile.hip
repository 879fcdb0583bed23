//------------------------------------------------------------------------------
///  @file flux_profile.hip
///  @brief Binning of per-sample values on flux surfaces with exact, workgroup-private sums (hand-written, gfx950).
///
///  A sample (x, y, z, value) gets the flux label of flux_label.hpp from the repacked psi tables ([cell][16]: a
///  lane's 16 coefficients are one 128-byte line, read with 16-byte loads) and belongs to profile cell i iff
///  edge[i] <= label < edge[i+1] (deposition.hip's rule).  Every profile cell is the superaccumulator of
///  superacc.hpp, 67 limbs of 64 bits.
///
///  Private path: every workgroup owns a grid of cells x 67 limbs in LDS (536 B per cell: 256 cells are 134 KiB of the
///  160 KiB a gfx950 workgroup may declare), zeroed at entry.  A deposit is at most three 64-bit integer LDS atomic
///  adds; after the grid-stride loop the workgroup adds its non-zero limbs to the global state with no-return 64-bit
///  global atomics.  Integer addition is associative and wraps, so the global limbs are those of the global path: the
///  state does not depend on the route, the launch shape or the order of the samples.  A LDS limb sees a subset of the
///  deposits of one launch, so the 2^30 rule of superacc.hpp holds as the host applies it to whole launches.
///
///  Global path (more cells than the cap, or flag bit 1 of the map): deposits go to the global state as in
///  deposition.hip's deposit_kernel.
//------------------------------------------------------------------------------
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flux_label.hpp"
#include "superacc.hpp"

namespace gfhip {

namespace {

constexpr unsigned int private_block = 1024;           // 16 waves: one workgroup per CU at the cap still has 4 waves per SIMD
constexpr unsigned int global_block = 256;
constexpr size_t lds_per_workgroup = 160u*1024u;
constexpr size_t private_cap = 256;                    // cells: 256*536 + 257*8 = 139,272 B of the 163,840 a workgroup may declare
constexpr size_t private_cap_bytes = private_cap*superacc::limbs*sizeof(unsigned long long) + (private_cap + 1)*sizeof(double);
static_assert(private_cap_bytes <= lds_per_workgroup, "the cap fits one workgroup's LDS");

//  The cell of `c` among the n + 1 increasing edges `e` (LDS), or -1: outside [e[0], e[n]) or NaN.  deposition.hip's
//  find_cell: the guess from the uniform spacing is right or off by one for linspace edges; the stored edges decide.
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

//  The label of one point, NaN outside the map.  `packed`: [table cell][16], 16-byte aligned.
__device__ __forceinline__ double label_at(const flux::map &m, const double *__restrict__ packed,
                                           const double x, const double y, const double z) {
    double tr, tz;
    const long long at = flux::locate(m, x, y, z, tr, tz);
    if (at < 0) return __builtin_nan("");
    const double2 *line = reinterpret_cast<const double2 *> (packed) + at*8;
    double c[16];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const double2 pair = line[k];
        c[2*k] = pair.x;
        c[2*k + 1] = pair.y;
    }
    return flux::label_of(m, flux::psi_of(c, tr, tz));
}

}  // namespace

//  PRIVATE: dynamic LDS = cells*67 limbs, then the cells + 1 edges; else the edges alone.
//  counters: samples, outside, skipped.
template<bool PRIVATE>
__global__ void __launch_bounds__(private_block)
flux_deposit_kernel(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                    const double *__restrict__ value, const unsigned long long count,
                    const flux::map m, const double *__restrict__ packed,
                    const double *__restrict__ edges, const int cells, const double scale,
                    unsigned long long *__restrict__ state, unsigned long long *__restrict__ counters) {
    extern __shared__ unsigned long long shared[];
    const unsigned int words = PRIVATE ? static_cast<unsigned int> (cells)*superacc::limbs : 0u;
    double *staged = reinterpret_cast<double *> (shared + words);
    for (unsigned int i = threadIdx.x; i < words; i += blockDim.x) shared[i] = 0ull;
    for (int i = threadIdx.x; i <= cells; i += blockDim.x) staged[i] = edges[i];
    __syncthreads();

    unsigned long long seen = 0, outside = 0, skipped = 0;                      // wave-uniform
    const unsigned long long stride = static_cast<unsigned long long> (gridDim.x)*blockDim.x;
//  `base` is the same for every lane of the workgroup: the ballots and shuffles below are executed by whole waves, and
//  every wave of the workgroup arrives at the barrier before the flush.
    for (unsigned long long base = static_cast<unsigned long long> (blockIdx.x)*blockDim.x; base < count; base += stride) {
        const unsigned long long at = base + threadIdx.x;
        const bool present = at < count;
        bool inside = false, finite = false;
        unsigned int key = 0;                          // cell*64 + first limb
        long long c0 = 0, c1 = 0, c2 = 0;
        if (present) {
            const double v = value[at];
            const int cell = find_cell(staged, cells, scale, label_at(m, packed, x[at], y[at], z[at]));
            inside = cell >= 0;
            finite = superacc::is_finite(v);
            if (inside && finite) {
                const superacc::pieces p = superacc::split(v);
                key = static_cast<unsigned int> (cell)*64u + static_cast<unsigned int> (p.first);
                c0 = p.negative ? -static_cast<long long> (p.chunk[0]) : static_cast<long long> (p.chunk[0]);
                c1 = p.negative ? -static_cast<long long> (p.chunk[1]) : static_cast<long long> (p.chunk[1]);
                c2 = p.negative ? -static_cast<long long> (p.chunk[2]) : static_cast<long long> (p.chunk[2]);
            }
        }
        seen += __popcll(__ballot(present));
        outside += __popcll(__ballot(present && !inside));
        skipped += __popcll(__ballot(present && inside && !finite));

        bool adds = (c0 | c1 | c2) != 0;               // a zero adds nothing
        if constexpr (!PRIVATE) {
//  Global path, as deposit_kernel: when every adding lane has the same cell and the same first limb (identical rays), sum
//  the chunks over the wave, three atomics from one lane.  Exact: the limbs are integers.  The private path does without:
//  measured with and without it, it made no difference there.
            const unsigned long long adders = __ballot(adds);
            if (adders == 0) continue;                 // wave-uniform
            const unsigned int first = __builtin_amdgcn_readlane(key, __ffsll(static_cast<long long> (adders)) - 1);
            if (__ballot(adds && key != first) == 0) {
                c0 = wave_sum(c0);
                c1 = wave_sum(c1);
                c2 = wave_sum(c2);
                key = first;
                adds = (threadIdx.x & 63u) == 0;
            }
        }
        if (adds) {
            const size_t limb = static_cast<size_t> (key >> 6)*superacc::limbs + (key & 63u);
//  The results are unused: no-return atomics, ds_add_u64 on the private grid and global_atomic_add_x2 on the state.
            if constexpr (PRIVATE) {
                if (c0) atomicAdd(&shared[limb], static_cast<unsigned long long> (c0));
                if (c1) atomicAdd(&shared[limb + 1], static_cast<unsigned long long> (c1));
                if (c2) atomicAdd(&shared[limb + 2], static_cast<unsigned long long> (c2));
            } else {
                if (c0) atomicAdd(state + limb, static_cast<unsigned long long> (c0));
                if (c1) atomicAdd(state + limb + 1, static_cast<unsigned long long> (c1));
                if (c2) atomicAdd(state + limb + 2, static_cast<unsigned long long> (c2));
            }
        }
    }
    if constexpr (PRIVATE) {
        __syncthreads();
        for (unsigned int i = threadIdx.x; i < words; i += blockDim.x) {
            const unsigned long long sum = shared[i];
            if (sum) atomicAdd(state + i, sum);
        }
    }
    if ((threadIdx.x & 63u) == 0) {
        if (seen) atomicAdd(counters, seen);
        if (outside) atomicAdd(counters + 1, outside);
        if (skipped) atomicAdd(counters + 2, skipped);
    }
}

//  One lane per point: its label, NaN outside the map.
__global__ void __launch_bounds__(256)
flux_label_kernel(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                  const unsigned long long count, const flux::map m, const double *__restrict__ packed,
                  double *__restrict__ label) {
    const unsigned long long at = static_cast<unsigned long long> (blockIdx.x)*blockDim.x + threadIdx.x;
    if (at < count) label[at] = label_at(m, packed, x[at], y[at], z[at]);
}

//  The shape of a profile's deposit launches.  The private path is taken when the grid and the edges fit the LDS of
//  one workgroup and the caller has not switched it off; `cap` is the most cells it takes.
void flux_launch_shape(const size_t cells, const bool allow_private, const unsigned int num_cus,
                       bool *is_private, size_t *cap, unsigned int *block, size_t *max_workgroups, size_t *lds_bytes) {
    const size_t per_cell = superacc::limbs*sizeof(unsigned long long);
    *cap = private_cap;
    const size_t edge_bytes = (cells + 1)*sizeof(double);
    *is_private = allow_private && cells <= *cap;
    if (*is_private) {
        *lds_bytes = cells*per_cell + edge_bytes;
        *block = private_block;
//  Two workgroups of 1024 are all the waves a CU holds; large grids leave room for one.
        const size_t per_cu = lds_per_workgroup/(*lds_bytes) >= 2 ? 2 : 1;
        *max_workgroups = static_cast<size_t> (num_cus)*per_cu;
    } else {
        *lds_bytes = edge_bytes;
        *block = global_block;
        *max_workgroups = static_cast<size_t> (num_cus)*8u;
    }
}

//  Dynamic LDS above 64 KiB has to be asked for.  The setting belongs to the function on the current device, not to a
//  profile: always the cap's size, so that no profile lowers what another one needs.
hipError_t flux_prepare() {
    return hipFuncSetAttribute(reinterpret_cast<const void *> (&flux_deposit_kernel<true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int> (private_cap_bytes));
}

void launch_flux_deposit(const double *x, const double *y, const double *z, const double *value, const size_t count,
                         const flux::map &m, const double *packed, const double *edges, const size_t cells, const double scale,
                         const bool is_private, const unsigned int block, const size_t max_workgroups, const size_t lds_bytes,
                         void *state, unsigned long long *counters, hipStream_t stream) {
    if (count == 0) return;
    const size_t want = (count + block - 1)/block;
    const unsigned int grid = static_cast<unsigned int> (want < max_workgroups ? want : max_workgroups);
    if (is_private) {
        hipLaunchKernelGGL(flux_deposit_kernel<true>, dim3(grid), dim3(block), lds_bytes, stream, x, y, z, value,
                           static_cast<unsigned long long> (count), m, packed, edges, static_cast<int> (cells), scale,
                           static_cast<unsigned long long *> (state), counters);
    } else {
        hipLaunchKernelGGL(flux_deposit_kernel<false>, dim3(grid), dim3(block), lds_bytes, stream, x, y, z, value,
                           static_cast<unsigned long long> (count), m, packed, edges, static_cast<int> (cells), scale,
                           static_cast<unsigned long long *> (state), counters);
    }
}

void launch_flux_label(const double *x, const double *y, const double *z, const size_t count, const flux::map &m,
                       const double *packed, double *label, hipStream_t stream) {
    if (count == 0) return;
    hipLaunchKernelGGL(flux_label_kernel, dim3(static_cast<unsigned int> ((count + 255)/256)), dim3(256), 0, stream, x, y, z,
                       static_cast<unsigned long long> (count), m, packed, label);
}

}  // namespace gfhip
