//------------------------------------------------------------------------------
///  @file flux_profile.hip
///  @brief Binning of per-sample values on flux surfaces with exact, workgroup-private sums (hand-written, gfx950).
///
///  A sample (x, y, z, value) gets the flux label of flux_label.hpp from the repacked psi tables ([cell][16]: a
///  lane's 16 coefficients are one 128-byte line, read with 16-byte loads) and belongs to profile cell i iff
///  edge[i] <= label < edge[i+1] (cell_deposit.hpp's find_cell, deposition.hip's rule).  Every profile cell is the superaccumulator of
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
///  deposition.hip's deposit_kernel.  What a sample adds, the counters, the wave-level pre-sum and the atomic adds are
///  the functions of cell_deposit.hpp in both kernels; this one has the label and the private grid of its own.
///
///  flux_deposit_rays_kernel keeps the same sums per batch of rays (ray_batches.hpp), state [batch][cell][limb]: a
///  workgroup works on one batch at a time, so the private grid is still `cells` wide whatever the number of batches.
///
///  flux_volume_kernel deposits the same way, but what it deposits it generates itself: the quadrature points of
///  flux_label.hpp, weight R x area each, so that a cell's sum is the volume/2 pi of the part of the map whose label
///  lies in the cell.  It reads no sample arrays.
//------------------------------------------------------------------------------
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cell_deposit.hpp"
#include "cell_launch.hpp"
#include "flux_label.hpp"
#include "flux_sums.hpp"
#include "superacc.hpp"

namespace gfhip {

using namespace sums;                                  // flux_sums.hpp: label_at, workgroup_sums, the blocks and the cap

namespace {

constexpr size_t private_cap_bytes = private_cap*bytes_per_cell + (private_cap + 1)*sizeof(double);
static_assert(private_cap_bytes <= lds_per_workgroup, "the cap fits one workgroup's LDS");

}  // namespace

//  counters: samples, outside, skipped.
template<bool PRIVATE>
__global__ void __launch_bounds__(private_block)
flux_deposit_kernel(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                    const double *__restrict__ value, const unsigned long long count,
                    const flux::map m, const double *__restrict__ packed,
                    const double *__restrict__ edges, const int cells, const double scale,
                    unsigned long long *__restrict__ state, unsigned long long *__restrict__ counters) {
    extern __shared__ unsigned long long shared[];
    workgroup_sums<PRIVATE> sums;
    sums.open(shared, edges, cells);

    deposit::tallies tally;
    const unsigned long long stride = static_cast<unsigned long long> (gridDim.x)*blockDim.x;
//  `base` is the same for every lane of the workgroup: the ballots and shuffles below are executed by whole waves, and
//  every wave of the workgroup arrives at the barrier before the flush.
    for (unsigned long long base = static_cast<unsigned long long> (blockIdx.x)*blockDim.x; base < count; base += stride) {
        const unsigned long long at = base + threadIdx.x;
        const bool present = at < count;
        int cell = -1;                                 // outside, as in the lanes past the end
        double v = 0.0;
        if (present) {
            v = value[at];
            cell = deposit::find_cell(sums.staged, cells, scale, label_at(m, packed, x[at], y[at], z[at]));
        }
        const deposit::contribution a = deposit::contribution_of(cell >= 0, static_cast<unsigned int> (cell), v);
        deposit::count(tally, present, a);
        sums.add(state, a);
    }
    sums.close(state);
    deposit::flush(tally, counters);
}

//  flux_deposit_kernel with the samples' rays: sample i is ray first_ray + i, and the state is [batch][cell][limb]
//  (flux_sums.hpp's deposit_batched).
template<bool PRIVATE>
__global__ void __launch_bounds__(private_block)
flux_deposit_rays_kernel(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                         const double *__restrict__ value, const unsigned long long count, const unsigned long long first_ray,
                         const unsigned int batch_count, const flux::map m, const double *__restrict__ packed,
                         const double *__restrict__ edges, const int cells, const double scale,
                         unsigned long long *__restrict__ state, unsigned long long *__restrict__ counters) {
    extern __shared__ unsigned long long shared[];
    workgroup_sums<PRIVATE> sums;
    sums.open(shared, edges, cells);
    deposit_batched(sums, first_ray, count, batch_count, cells, state, counters, [&](const uint64_t at, double &v) {
        v = value[at];
        return deposit::find_cell(sums.staged, cells, scale, label_at(m, packed, x[at], y[at], z[at]));
    });
}

//  The volume quadrature of flux_label.hpp: the points first .. first + count of the flat index t = gr*row + gz
//  (row = numz*sub sub-cells along z), generated here; nothing is read but the coefficient lines and the edges.  A lane
//  divides once, to find the (gr, gz) of its first point, and then advances by the launch's stride, which is split
//  into rows and a remainder once as well.  Consecutive lanes are consecutive in gz: `sub` neighbours share a
//  coefficient line.  The shape, the counters and the sums are flux_deposit_kernel's.
template<bool PRIVATE>
__global__ void __launch_bounds__(private_block)
flux_volume_kernel(const unsigned long long first, const unsigned long long count, const unsigned long long row,
                   const double twice_sub, const double area, const flux::window window,
                   const flux::map m, const double *__restrict__ packed,
                   const double *__restrict__ edges, const int cells, const double scale,
                   unsigned long long *__restrict__ state, unsigned long long *__restrict__ counters) {
    extern __shared__ unsigned long long shared[];
    workgroup_sums<PRIVATE> sums;
    sums.open(shared, edges, cells);

    deposit::tallies tally;
    const unsigned long long stride = static_cast<unsigned long long> (gridDim.x)*blockDim.x;
    const unsigned long long stride_rows = stride/row, stride_rest = stride%row;
    const unsigned long long mine = first + static_cast<unsigned long long> (blockIdx.x)*blockDim.x + threadIdx.x;
    unsigned long long gr = mine/row, gz = mine%row;
    for (unsigned long long base = static_cast<unsigned long long> (blockIdx.x)*blockDim.x; base < count; base += stride) {
        const bool present = base + threadIdx.x < count;
        int cell = -1;
        double w = 0.0;
        if (present) {
            const double r = flux::sub_centre(m.rmin, m.dr, gr, twice_sub);
            const double z = flux::sub_centre(m.zmin, m.dz, gz, twice_sub);
            w = flux::sub_weight(r, area);
            if (flux::in_window(window, r, z)) cell = deposit::find_cell(sums.staged, cells, scale, label_at(m, packed, r, 0.0, z));
        }
        const deposit::contribution a = deposit::contribution_of(cell >= 0, static_cast<unsigned int> (cell), w);
        deposit::count(tally, present, a);
        sums.add(state, a);
        gr += stride_rows;
        gz += stride_rest;
        if (gz >= row) {
            gz -= row;
            gr++;
        }
    }
    sums.close(state);
    deposit::flush(tally, counters);
}

//  One lane per point: its label, NaN outside the map.
__global__ void __launch_bounds__(256)
flux_label_kernel(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                  const unsigned long long count, const flux::map m, const double *__restrict__ packed,
                  double *__restrict__ label) {
    const unsigned long long at = static_cast<unsigned long long> (blockIdx.x)*blockDim.x + threadIdx.x;
    if (at < count) label[at] = label_at(m, packed, x[at], y[at], z[at]);
}

//  The shape of the deposit launches of a profile (cells + 1 edges) or a spectrum (its two axes' edges).  The private
//  path is taken when the grid and the edges fit the LDS of one workgroup and the caller has not switched it off; `cap`
//  is the most cells it takes.
launch_shape flux_launch_shape(const size_t cells, const size_t edge_count, const bool allow_private, const unsigned int num_cus) {
    launch_shape shape = {};
    shape.cap = private_cap;
    const size_t edge_bytes = edge_count*sizeof(double);
    shape.is_private = allow_private && cells <= shape.cap && cells*bytes_per_cell + edge_bytes <= lds_per_workgroup;
    if (shape.is_private) {
        shape.lds_bytes = cells*bytes_per_cell + edge_bytes;
        shape.block = private_block;
//  Two workgroups of 1024 are all the waves a CU holds; large grids leave room for one.
        const size_t per_cu = lds_per_workgroup/shape.lds_bytes >= 2 ? 2 : 1;
        shape.max_workgroups = static_cast<size_t> (num_cus)*per_cu;
    } else {
        shape.lds_bytes = edge_bytes;
        shape.block = global_block;
        shape.max_workgroups = static_cast<size_t> (num_cus)*8u;
    }
    return shape;
}

hipError_t flux_prepare() {
    return prepare_private({reinterpret_cast<const void *> (&flux_deposit_kernel<true>),
                            reinterpret_cast<const void *> (&flux_deposit_rays_kernel<true>),
                            reinterpret_cast<const void *> (&flux_volume_kernel<true>)}, private_cap_bytes);
}

void launch_flux_deposit(const double *x, const double *y, const double *z, const double *value, const size_t count,
                         const cell_tables &t, const double *edges, const size_t cells, const double scale,
                         const launch_shape &shape, const cell_target &to) {
    if (count == 0) return;
    launch_on_route(flux_deposit_kernel<true>, flux_deposit_kernel<false>, shape, grid_of(count, shape.block, shape.max_workgroups),
                    to.stream, x, y, z, value, static_cast<unsigned long long> (count), t.map, t.packed, edges,
                    static_cast<int> (cells), scale, static_cast<unsigned long long *> (to.state), to.counters);
}

void launch_flux_deposit_rays(const double *x, const double *y, const double *z, const double *value, const size_t count,
                              const unsigned long long first_ray, const size_t batch_count, const cell_tables &t,
                              const double *edges, const size_t cells, const double scale, const launch_shape &shape,
                              const cell_target &to) {
    if (count == 0) return;
    launch_on_route(flux_deposit_rays_kernel<true>, flux_deposit_rays_kernel<false>, shape,
                    batched_grid_of(count, shape.block, shape.max_workgroups, batch_count), to.stream, x, y, z, value,
                    static_cast<unsigned long long> (count), first_ray, static_cast<unsigned int> (batch_count), t.map, t.packed,
                    edges, static_cast<int> (cells), scale, static_cast<unsigned long long *> (to.state), to.counters);
}

void launch_flux_volumes(const unsigned long long first, const size_t count, const unsigned long long row, const double twice_sub,
                         const double area, const flux::window &window, const cell_tables &t, const double *edges,
                         const size_t cells, const double scale, const launch_shape &shape, const cell_target &to) {
    if (count == 0) return;
    launch_on_route(flux_volume_kernel<true>, flux_volume_kernel<false>, shape, grid_of(count, shape.block, shape.max_workgroups),
                    to.stream, first, static_cast<unsigned long long> (count), row, twice_sub, area, window, t.map, t.packed,
                    edges, static_cast<int> (cells), scale, static_cast<unsigned long long *> (to.state), to.counters);
}

void launch_flux_label(const double *x, const double *y, const double *z, const size_t count, const cell_tables &t,
                       double *label, hipStream_t stream) {
    if (count == 0) return;
    hipLaunchKernelGGL(flux_label_kernel, dim3(static_cast<unsigned int> ((count + 255)/256)), dim3(256), 0, stream, x, y, z,
                       static_cast<unsigned long long> (count), t.map, t.packed, label);
}

}  // namespace gfhip
