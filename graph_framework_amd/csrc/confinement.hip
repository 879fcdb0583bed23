//------------------------------------------------------------------------------
///  @file confinement.hip
///  @brief First-exit tracking of the particles of a push: who has left the plasma, when, where and at what energy
///  (hand-written, gfx950).
///
///  Per particle the tracker keeps lost_step (uint32, 0xFFFFFFFF: confined) and alive (1 or 0 in the push's type).  A
///  check with step number `step` looks at the confined particles only: x, y, z are widened to fp64, which is exact,
///  and get the label of flux_label.hpp from the cell's 16 coefficients, as label_at reads them; the particle is lost
///  iff !(label < limit), so that a particle off the map, a NaN position and label == limit are all lost.  A lost
///  particle is settled once: lost_step = step, alive = 0, exit_r = R and exit_z = z where the caller gave exit buffers,
///  and its weight (1.0 without a weight column) goes to the exact cell (ir, iz, ig) of (R, z, gamma as stored) by
///  cell_deposit.hpp's find_cell, flat index (ir*nz + iz)*ng + ig.  It is never looked at again.
///
///  A lane reads lost_step first and nothing else when its particle is settled; a confined lane reads x, y, z and the 16
///  coefficients, and gamma and the weight only on loss.  Deposits go to the global state behind the wave pre-sum: over
///  a whole run a particle deposits at most once, so a workgroup-private grid would buy nothing.  The three counters
///  count the particles lost in the check (samples), those of them in no footprint cell (outside) and those with a
///  non-finite weight (skipped); newly_lost, the check's own entry, goes up by `samples`, one atomic per wave.
//------------------------------------------------------------------------------
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cell_deposit.hpp"
#include "cell_launch.hpp"
#include "flux_label.hpp"
#include "flux_sums.hpp"
#include "superacc.hpp"

namespace gfhip {

using namespace sums;

namespace {

constexpr unsigned int confined = 0xffffffffu;

}  // namespace

template<typename T>
struct confine_columns {
    const T *x, *y, *z, *gamma, *weight;               // weight: null when every particle deposits 1.0
    T *alive;
};

//  counters: samples, outside, skipped.  edges: the nr + 1 of R, the nz + 1 of z, the ng + 1 of gamma.  exit_r and
//  exit_z: both null without exit buffers.  newly_lost: the entry of this check.
template<typename T>
__global__ void __launch_bounds__(global_block)
confinement_check_kernel(const confine_columns<T> in, const unsigned long long count, const flux::map m,
                         const double *__restrict__ packed, const double limit, const double *__restrict__ edges,
                         const int nr, const int nz, const int ng, const double rscale, const double zscale, const double gscale,
                         const unsigned int step, unsigned int *__restrict__ lost_step, double *__restrict__ exit_r,
                         double *__restrict__ exit_z, unsigned long long *__restrict__ newly_lost,
                         unsigned long long *__restrict__ state, unsigned long long *__restrict__ counters) {
    extern __shared__ unsigned long long shared[];
    workgroup_sums<false> sums;
    sums.open(shared, edges, nr*nz*ng, nr + nz + ng + 3);
    const double *redge = sums.staged, *zedge = redge + nr + 1, *gedge = zedge + nz + 1;

    deposit::tallies tally;
    const unsigned long long stride = static_cast<unsigned long long> (gridDim.x)*blockDim.x;
//  `base` is the same for every lane of the workgroup: the ballots and shuffles below are executed by whole waves.
    for (unsigned long long base = static_cast<unsigned long long> (blockIdx.x)*blockDim.x; base < count; base += stride) {
        const unsigned long long at = base + threadIdx.x;
        bool lost = false;
        int cell = -1;
        double v = 0.0;
        if (at < count && lost_step[at] == confined) {
            const double x = static_cast<double> (in.x[at]), y = static_cast<double> (in.y[at]), z = static_cast<double> (in.z[at]);
            const double label = flux::canonical(label_at(m, packed, x, y, z));
            if (!(label < limit)) {
                lost = true;
                v = in.weight ? static_cast<double> (in.weight[at]) : 1.0;        // read before alive is written: it may be the weight
                const double r = flux::radius_of(x, y);
                const int ir = deposit::find_cell(redge, nr, rscale, r);
                const int iz = deposit::find_cell(zedge, nz, zscale, z);
                const int ig = deposit::find_cell(gedge, ng, gscale, static_cast<double> (in.gamma[at]));
                if (ir >= 0 && iz >= 0 && ig >= 0) cell = (ir*nz + iz)*ng + ig;
                lost_step[at] = step;
                in.alive[at] = static_cast<T> (0);
                if (exit_r) {
                    exit_r[at] = flux::canonical(r);
                    exit_z[at] = flux::canonical(z);
                }
            }
        }
        const deposit::contribution a = deposit::contribution_of(cell >= 0, static_cast<unsigned int> (cell), v);
        deposit::count(tally, lost, a);
        sums.add(state, a);
    }
    sums.close(state);
    deposit::flush(tally, counters);
    if ((threadIdx.x & 63u) == 0 && tally.seen) atomicAdd(newly_lost, tally.seen);
}

//  One lane per particle: the sentinel and alive = 1 (both null when only exit buffers are prepared), the quiet NaN
//  without payload into the exit buffers (both null without them).
template<typename T>
__global__ void __launch_bounds__(256)
confinement_reset_kernel(const unsigned long long count, unsigned int *__restrict__ lost_step, T *__restrict__ alive,
                         double *__restrict__ exit_r, double *__restrict__ exit_z) {
    const unsigned long long at = static_cast<unsigned long long> (blockIdx.x)*blockDim.x + threadIdx.x;
    if (at < count) {
        if (lost_step) {
            lost_step[at] = confined;
            alive[at] = static_cast<T> (1);
        }
        if (exit_r) {
            exit_r[at] = __builtin_nan("");
            exit_z[at] = __builtin_nan("");
        }
    }
}

void launch_confinement_check(const void *const *columns, void *alive, const bool is_f32, const size_t first, const size_t count,
                              const cell_tables &t, const double limit, const double *edges, const size_t *n,
                              const double *scale, const uint32_t step, uint32_t *lost_step, double *exit_r, double *exit_z,
                              unsigned long long *newly_lost, const launch_shape &shape, const cell_target &to) {
    if (count == 0) return;
    with_particle_type(is_f32, [&](auto type) {
        using T = decltype(type);
        const T *const *typed = reinterpret_cast<const T *const *> (columns);
        const confine_columns<T> in = {typed[0] + first, typed[1] + first, typed[2] + first, typed[6] + first,
                                       typed[7] ? typed[7] + first : nullptr, static_cast<T *> (alive) + first};
        hipLaunchKernelGGL(confinement_check_kernel<T>, dim3(grid_of(count, shape.block, shape.max_workgroups)), dim3(shape.block),
                           shape.lds_bytes, to.stream, in, static_cast<unsigned long long> (count), t.map, t.packed, limit, edges,
                           static_cast<int> (n[0]), static_cast<int> (n[1]), static_cast<int> (n[2]), scale[0], scale[1], scale[2],
                           step, lost_step + first, exit_r ? exit_r + first : nullptr, exit_z ? exit_z + first : nullptr,
                           newly_lost, static_cast<unsigned long long *> (to.state), to.counters);
    });
}

void launch_confinement_reset(const size_t count, uint32_t *lost_step, void *alive, const bool is_f32, double *exit_r,
                              double *exit_z, hipStream_t stream) {
    if (count == 0) return;
    with_particle_type(is_f32, [&](auto type) {
        using T = decltype(type);
        hipLaunchKernelGGL(confinement_reset_kernel<T>, dim3(static_cast<unsigned int> ((count + 255)/256)), dim3(256), 0, stream,
                           static_cast<unsigned long long> (count), lost_step, static_cast<T *> (alive), exit_r, exit_z);
    });
}

}  // namespace gfhip
