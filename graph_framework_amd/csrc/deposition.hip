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
///  per sample.  The pieces of a deposit are cell_deposit.hpp's, shared with flux_profile.hip; the
///  normalise, round and merge kernels at the end serve every store of exact sums (cell_launch.hpp).
//------------------------------------------------------------------------------
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cell_deposit.hpp"
#include "cell_launch.hpp"
#include "superacc.hpp"

namespace gfhip {

constexpr unsigned int deposit_block = 256;

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

    deposit::tallies tally;
    const unsigned long long stride = static_cast<unsigned long long> (gridDim.x)*blockDim.x;
//  `base` is the same for every lane of the workgroup: the ballots and shuffles below are executed by whole waves.
    for (unsigned long long base = static_cast<unsigned long long> (blockIdx.x)*blockDim.x; base < count; base += stride) {
        const unsigned long long at = base + threadIdx.x;
        const bool present = at < count;
        bool inside = false;
        unsigned int cell = 0;
        double v = 0.0;
        if (present) {
            const double px = x[at], py = y[at], pz = z[at];
            v = value[at];
            const int i = deposit::find_cell(ex, nx, scale_x, px);
            const int j = deposit::find_cell(ey, ny, scale_y, py);
            const int k = deposit::find_cell(ez, nz, scale_z, pz);
            inside = i >= 0 && j >= 0 && k >= 0;
            cell = (static_cast<unsigned int> (i)*ny + j)*nz + k;
        }
        const deposit::contribution a = deposit::contribution_of(inside, cell, v);
        deposit::count(tally, present, a);
        deposit::add_limbs_presummed(state, a);
    }
    deposit::flush(tally, counters);
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
round_kernel(const long long *__restrict__ state, const unsigned long long cells, const double divisor, double *__restrict__ values) {
    const unsigned long long cell = static_cast<unsigned long long> (blockIdx.x)*blockDim.x + threadIdx.x;
    if (cell < cells) values[cell] = superacc::round(reinterpret_cast<const int64_t *> (state) + cell*superacc::limbs)/divisor;
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

void launch_cells_normalise(void *state, const size_t cells, hipStream_t stream) {
    hipLaunchKernelGGL(normalise_kernel, dim3(blocks_for(cells)), dim3(256), 0, stream, static_cast<long long *> (state),
                       static_cast<unsigned long long> (cells));
}

void launch_cells_round(const void *state, const size_t cells, const double divisor, double *values, hipStream_t stream) {
    hipLaunchKernelGGL(round_kernel, dim3(blocks_for(cells)), dim3(256), 0, stream, static_cast<const long long *> (state),
                       static_cast<unsigned long long> (cells), divisor, values);
}

void launch_cells_merge(void *state, const void *other, const size_t words, hipStream_t stream) {
    hipLaunchKernelGGL(merge_kernel, dim3(blocks_for(words)), dim3(256), 0, stream, static_cast<long long *> (state),
                       static_cast<const long long *> (other), static_cast<unsigned long long> (words));
}

}  // namespace gfhip
