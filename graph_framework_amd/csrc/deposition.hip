//------------------------------------------------------------------------------
///  @file deposition.hip
///  @brief Binning of per-sample values on a 3-D grid with exact sums (hand-written, gfx950).
///
///  The device side of utilities/bin.py: a sample (x, y, z, value) belongs to cell (i, j, k) iff
///  edge[i] <= c && c < edge[i+1] on each axis (bin.py's `mask`), and every cell holds the exact sum
///  of its values on the integer superaccumulator of superacc.hpp: 67 limbs of 64 bits per cell,
///  [cell][limb].  A deposit is at most three 64-bit integer atomic adds on adjacent limbs
///  (no-return vector global atomics); integer addition is associative, so the state does not depend
///  on the order in which samples, records, files or ranks arrive.  One sample per lane, 32 B read
///  per sample.
//------------------------------------------------------------------------------
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "superacc.hpp"

namespace gfhip {

namespace {

constexpr unsigned int deposit_block = 256;

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

__device__ __forceinline__ void add_limb(unsigned long long *limb, const long long amount) {
    if (amount) atomicAdd(limb, static_cast<unsigned long long> (amount));     // result unused: no-return atomic
}

}  // namespace

//  edges: the nx + 1, ny + 1 and nz + 1 edges one after the other; scale: n/(e[n] - e[0]) per axis;
//  counters: samples, outside, skipped.
__global__ void __launch_bounds__(deposit_block)
deposit_kernel(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
               const double *__restrict__ value, const unsigned long long count,
               const double *__restrict__ edges, const int nx, const int ny, const int nz,
               const double scale_x, const double scale_y, const double scale_z,
               unsigned long long *__restrict__ state, unsigned long long *__restrict__ counters) {
    extern __shared__ double staged[];
    const int total_edges = nx + ny + nz + 3;
    for (int i = threadIdx.x; i < total_edges; i += blockDim.x) staged[i] = edges[i];
    __syncthreads();
    const double *ex = staged, *ey = staged + nx + 1, *ez = staged + nx + ny + 2;

    unsigned long long seen = 0, outside = 0, skipped = 0;                      // wave-uniform
    const unsigned long long stride = static_cast<unsigned long long> (gridDim.x)*blockDim.x;
//  `base` is the same for every lane of the workgroup: the shuffles below are executed by whole waves.
    for (unsigned long long base = static_cast<unsigned long long> (blockIdx.x)*blockDim.x; base < count; base += stride) {
        const unsigned long long at = base + threadIdx.x;
        const bool present = at < count;
        bool inside = false, finite = false;
        unsigned int key = 0;                          // cell*64 + first limb
        long long c0 = 0, c1 = 0, c2 = 0;
        if (present) {
            const double px = x[at], py = y[at], pz = z[at], v = value[at];
            const int i = find_cell(ex, nx, scale_x, px);
            const int j = find_cell(ey, ny, scale_y, py);
            const int k = find_cell(ez, nz, scale_z, pz);
            inside = i >= 0 && j >= 0 && k >= 0;
            finite = superacc::is_finite(v);
            if (inside && finite) {
                const superacc::pieces p = superacc::split(v);
                const unsigned int cell = (static_cast<unsigned int> (i)*ny + j)*nz + k;
                key = cell*64u + static_cast<unsigned int> (p.first);
                c0 = p.negative ? -static_cast<long long> (p.chunk[0]) : static_cast<long long> (p.chunk[0]);
                c1 = p.negative ? -static_cast<long long> (p.chunk[1]) : static_cast<long long> (p.chunk[1]);
                c2 = p.negative ? -static_cast<long long> (p.chunk[2]) : static_cast<long long> (p.chunk[2]);
            }
        }
        seen += __popcll(__ballot(present));
        outside += __popcll(__ballot(present && !inside));
        skipped += __popcll(__ballot(present && inside && !finite));

        const bool adds = (c0 | c1 | c2) != 0;         // a zero adds nothing
        const unsigned long long adders = __ballot(adds);
        if (adders == 0) continue;                     // wave-uniform
        const unsigned int first = __builtin_amdgcn_readlane(key, __ffsll(static_cast<long long> (adders)) - 1);
        if (__ballot(adds && key != first) == 0) {
//  Every adding lane has the same cell and the same first limb (identical rays: every wave, every record): sum the
//  chunks over the wave, three atomics from one lane.  Exact: the limbs are integers.
            c0 = wave_sum(c0);
            c1 = wave_sum(c1);
            c2 = wave_sum(c2);
            if ((threadIdx.x & 63u) == 0) {
                unsigned long long *limb = state + static_cast<size_t> (first >> 6)*superacc::limbs + (first & 63u);
                add_limb(limb, c0);
                add_limb(limb + 1, c1);
                add_limb(limb + 2, c2);
            }
        } else if (adds) {
            unsigned long long *limb = state + static_cast<size_t> (key >> 6)*superacc::limbs + (key & 63u);
            add_limb(limb, c0);
            add_limb(limb + 1, c1);
            add_limb(limb + 2, c2);
        }
    }
    if ((threadIdx.x & 63u) == 0) {
        if (seen) atomicAdd(counters, seen);
        if (outside) atomicAdd(counters + 1, outside);
        if (skipped) atomicAdd(counters + 2, skipped);
    }
}

//  One lane per cell: the state canonical in place.
__global__ void __launch_bounds__(256)
normalise_kernel(long long *__restrict__ state, const unsigned long long cells) {
    const unsigned long long cell = static_cast<unsigned long long> (blockIdx.x)*blockDim.x + threadIdx.x;
    if (cell < cells) superacc::normalise(reinterpret_cast<int64_t *> (state) + cell*superacc::limbs);
}

//  One lane per cell of a canonical state: the rounded exact sum, then the compiler's IEEE division: two
//  roundings, as bin.py's power_bins/total.
__global__ void __launch_bounds__(256)
round_kernel(const long long *__restrict__ state, const unsigned long long cells, const double divisor, double *__restrict__ bins) {
    const unsigned long long cell = static_cast<unsigned long long> (blockIdx.x)*blockDim.x + threadIdx.x;
    if (cell < cells) bins[cell] = superacc::round(reinterpret_cast<const int64_t *> (state) + cell*superacc::limbs)/divisor;
}

//  One lane per limb: another state added in, carry-save.
__global__ void __launch_bounds__(256)
merge_kernel(long long *__restrict__ state, const long long *__restrict__ other, const unsigned long long words) {
    const unsigned long long word = static_cast<unsigned long long> (blockIdx.x)*blockDim.x + threadIdx.x;
    if (word < words) state[word] += other[word];
}

void launch_deposit(const double *x, const double *y, const double *z, const double *value, const size_t count,
                    const double *edges, const int nx, const int ny, const int nz, const double *scale,
                    void *state, unsigned long long *counters, const unsigned int num_cus, hipStream_t stream) {
    if (count == 0) return;
    const size_t want = (count + deposit_block - 1)/deposit_block;
//  A few workgroups per CU, the lanes stride: the edges are staged once per workgroup.
    const size_t cap = static_cast<size_t> (num_cus)*8u;
    const unsigned int grid = static_cast<unsigned int> (want < cap ? want : cap);
    const size_t lds = static_cast<size_t> (nx + ny + nz + 3)*sizeof(double);
    hipLaunchKernelGGL(deposit_kernel, dim3(grid), dim3(deposit_block), lds, stream, x, y, z, value,
                       static_cast<unsigned long long> (count), edges, nx, ny, nz, scale[0], scale[1], scale[2],
                       static_cast<unsigned long long *> (state), counters);
}

static unsigned int blocks_for(const size_t lanes) {
    return static_cast<unsigned int> ((lanes + 255)/256);
}

void launch_bins_normalise(void *state, const size_t cells, hipStream_t stream) {
    hipLaunchKernelGGL(normalise_kernel, dim3(blocks_for(cells)), dim3(256), 0, stream, static_cast<long long *> (state),
                       static_cast<unsigned long long> (cells));
}

void launch_bins_round(const void *state, const size_t cells, const double divisor, double *bins, hipStream_t stream) {
    hipLaunchKernelGGL(round_kernel, dim3(blocks_for(cells)), dim3(256), 0, stream, static_cast<const long long *> (state),
                       static_cast<unsigned long long> (cells), divisor, bins);
}

void launch_bins_merge(void *state, const void *other, const size_t words, hipStream_t stream) {
    hipLaunchKernelGGL(merge_kernel, dim3(blocks_for(words)), dim3(256), 0, stream, static_cast<long long *> (state),
                       static_cast<const long long *> (other), static_cast<unsigned long long> (words));
}

}  // namespace gfhip
