//------------------------------------------------------------------------------
///  @file moment_bins.hip
///  @brief Density, parallel current, kinetic energy and radiated power of particles per flux surface, exact sums
///  (hand-written, gfx950).
///
///  A particle (x, y, z, ux, uy, uz, gamma), seven reads of fp32 or fp64 (the push's state as it lies on the device), is
///  widened to fp64, which is exact, and gets the label and the four moments m = {1, v_par/c, gamma - 1, |B|^2 u_perp^2} of
///  flux_label.hpp: psi and its two derivatives from the cell's 16 coefficients, fpol from the interval's four, as
///  phase_bins.hip reads them, ONE evaluation of the field per particle.  The particle belongs to surface `is` iff its
///  label lies in [sedge[is], sedge[is+1]) by cell_deposit.hpp's find_cell; the cells are ns*4 superaccumulators, flat
///  index is*4 + k.  It deposits v[k] = w*m[k] (v[0] = w) with w its weight, an eighth column of the same type, or 1.0
///  where there is none: all four, or, when one of them is NaN or infinite, none (the particle is `skipped`).
///
///  The sums are flux_sums.hpp's: up to 256 cells (64 surfaces) every workgroup owns the grid in LDS, the label edges
///  staged behind it; above that, or with the map's no-private flag, deposits go to the global state behind the wave
///  pre-sum (particles without a weight on one surface share the limbs of moment 0: three atomics per wave for it).
///  The state does not depend on the route, the launch shape, the order of the particles or their type.
///
///  moment_deposit_particles_kernel keeps the same sums per batch of particles (ray_batches.hpp, the particle's index in
///  the ensemble in place of a ray's), state [batch][surface][moment][limb]: a workgroup works on one batch at a time, so
///  the private grid is still ns*4 cells whatever the number of batches.
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

constexpr int moment_count = 4;

//  The private path holds ns*4 <= 256 cells, so at most 64 surfaces and 65 edges.
constexpr size_t moment_cap_bytes = private_cap*bytes_per_cell + (private_cap/moment_count + 1)*sizeof(double);
static_assert(moment_cap_bytes <= lds_per_workgroup, "the cap fits one workgroup's LDS");

//  The label and the four moments of one particle, all NaN outside the map.  `fpol`: [interval][4], 32-byte aligned.
__device__ __forceinline__ double moments_at(const flux::map &m, const flux::field &f, const double *__restrict__ packed,
                                             const double *__restrict__ fpol, const double x, const double y, const double z,
                                             const double ux, const double uy, const double uz, const double gamma,
                                             double *moments) {
    double tr, tz;
    const long long at = flux::locate(m, x, y, z, tr, tz);
    if (at < 0) {
#pragma unroll
        for (int k = 0; k < moment_count; k++) moments[k] = __builtin_nan("");
        return __builtin_nan("");
    }
    double c[16];
    coefficients_at(packed, at, c);
    double gr, gz, tp;
    const double psi = flux::psi_gradient(m, c, tr, tz, gr, gz);
    const int q = flux::fpol_interval(f, psi, tp);
    const double2 *line = reinterpret_cast<const double2 *> (fpol) + static_cast<size_t> (q)*2;
    const double2 low = line[0], high = line[1];
    const double cubic[4] = {low.x, low.y, high.x, high.y};
    flux::moments_of(x, y, flux::radius_of(x, y), ux, uy, uz, gamma, gr, gz, flux::fpol_of(cubic, tp), moments);
    return flux::canonical(flux::label_of(m, psi));
}

}  // namespace

template<typename T>
struct moment_columns {
    const T *x, *y, *z, *ux, *uy, *uz, *gamma, *weight;    // weight: null when every particle has weight 1.0
};

//  counters: samples, outside, skipped, counted per particle.  edges: the ns + 1 of the label.
template<bool PRIVATE, typename T>
__global__ void __launch_bounds__(private_block)
moment_deposit_kernel(const moment_columns<T> in, const unsigned long long count,
                      const flux::map m, const flux::field f, const double *__restrict__ packed,
                      const double *__restrict__ fpol, const double *__restrict__ edges, const int ns, const double sscale,
                      unsigned long long *__restrict__ state, unsigned long long *__restrict__ counters) {
    extern __shared__ unsigned long long shared[];
    workgroup_sums<PRIVATE> sums;
    sums.open(shared, edges, ns*moment_count, ns + 1);
    const double *sedge = sums.staged;

    deposit::tallies tally;
    const unsigned long long stride = static_cast<unsigned long long> (gridDim.x)*blockDim.x;
//  `base` is the same for every lane of the workgroup: the ballots and shuffles below are executed by whole waves, and
//  every wave of the workgroup arrives at the barrier before the flush.
    for (unsigned long long base = static_cast<unsigned long long> (blockIdx.x)*blockDim.x; base < count; base += stride) {
        const unsigned long long at = base + threadIdx.x;
        const bool present = at < count;
        int is = -1;                                   // outside, as in the lanes past the end
        double v[moment_count] = {0.0, 0.0, 0.0, 0.0};
        if (present) {
            const double w = in.weight ? static_cast<double> (in.weight[at]) : 1.0;
            double moments[moment_count];
            const double label = moments_at(m, f, packed, fpol, static_cast<double> (in.x[at]), static_cast<double> (in.y[at]),
                                            static_cast<double> (in.z[at]), static_cast<double> (in.ux[at]),
                                            static_cast<double> (in.uy[at]), static_cast<double> (in.uz[at]),
                                            static_cast<double> (in.gamma[at]), moments);
            is = deposit::find_cell(sedge, ns, sscale, label);
            flux::weighted_moments(w, moments, v);
        }
//  Decided once per particle: inside, and all four finite or none deposited.
        const deposit::contribution particle = {is >= 0, flux::moments_finite(v), 0u, 0, 0, 0};
        deposit::count(tally, present, particle);
        const bool deposits = particle.inside && particle.finite;
        const unsigned int first = static_cast<unsigned int> (is)*moment_count;
#pragma unroll
        for (int k = 0; k < moment_count; k++) sums.add(state, deposit::contribution_of(deposits, first + k, v[k]));
    }
    sums.close(state);
    deposit::flush(tally, counters);
}

//  moment_deposit_kernel with the particles' indices in the ensemble: sample i is particle first_particle + i, and the
//  state is [batch][surface][moment][limb] (flux_sums.hpp's deposit_batched_many).  A workgroup holds the ns*4 cells of
//  ONE batch of particles (ray_batches.hpp's rule, a particle in place of a ray) whatever the number of batches.
template<bool PRIVATE, typename T>
__global__ void __launch_bounds__(private_block)
moment_deposit_particles_kernel(const moment_columns<T> in, const unsigned long long count, const unsigned long long first_particle,
                                const unsigned int batch_count, const flux::map m, const flux::field f,
                                const double *__restrict__ packed, const double *__restrict__ fpol,
                                const double *__restrict__ edges, const int ns, const double sscale,
                                unsigned long long *__restrict__ state, unsigned long long *__restrict__ counters) {
    extern __shared__ unsigned long long shared[];
    workgroup_sums<PRIVATE> sums;
    sums.open(shared, edges, ns*moment_count, ns + 1);
    const double *sedge = sums.staged;
    deposit_batched_many<PRIVATE, moment_count> (sums, first_particle, count, batch_count, ns, state, counters,
                                                 [&](const uint64_t at, double *v, bool &finite) {
        const double w = in.weight ? static_cast<double> (in.weight[at]) : 1.0;
        double moments[moment_count];
        const double label = moments_at(m, f, packed, fpol, static_cast<double> (in.x[at]), static_cast<double> (in.y[at]),
                                        static_cast<double> (in.z[at]), static_cast<double> (in.ux[at]),
                                        static_cast<double> (in.uy[at]), static_cast<double> (in.uz[at]),
                                        static_cast<double> (in.gamma[at]), moments);
        flux::weighted_moments(w, moments, v);
        finite = flux::moments_finite(v);
        return deposit::find_cell(sedge, ns, sscale, label);
    });
}

//  One lane per particle: its label and its four moments, values[at*4 + k], NaN outside the map.
template<typename T>
__global__ void __launch_bounds__(256)
moment_values_kernel(const moment_columns<T> in, const unsigned long long count, const flux::map m, const flux::field f,
                     const double *__restrict__ packed, const double *__restrict__ fpol,
                     double *__restrict__ label, double *__restrict__ values) {
    const unsigned long long at = static_cast<unsigned long long> (blockIdx.x)*blockDim.x + threadIdx.x;
    if (at < count) {
        double moments[moment_count];
        label[at] = moments_at(m, f, packed, fpol, static_cast<double> (in.x[at]), static_cast<double> (in.y[at]),
                               static_cast<double> (in.z[at]), static_cast<double> (in.ux[at]), static_cast<double> (in.uy[at]),
                               static_cast<double> (in.uz[at]), static_cast<double> (in.gamma[at]), moments);
#pragma unroll
        for (int k = 0; k < moment_count; k++) values[at*moment_count + k] = moments[k];
    }
}

//  Dynamic LDS above 64 KiB has to be asked for: always the cap's size, as flux_prepare does.
hipError_t moments_prepare() {
    for (const void *kernel : {reinterpret_cast<const void *> (&moment_deposit_kernel<true, float>),
                               reinterpret_cast<const void *> (&moment_deposit_kernel<true, double>),
                               reinterpret_cast<const void *> (&moment_deposit_particles_kernel<true, float>),
                               reinterpret_cast<const void *> (&moment_deposit_particles_kernel<true, double>)}) {
        const hipError_t status = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                      static_cast<int> (moment_cap_bytes));
        if (status != hipSuccess) return status;
    }
    return hipSuccess;
}

namespace {

template<typename T>
moment_columns<T> columns_from(const void *const *columns, const size_t first, const bool with_weight) {
    const T *const *typed = reinterpret_cast<const T *const *> (columns);
    return {typed[0] + first, typed[1] + first, typed[2] + first, typed[3] + first, typed[4] + first, typed[5] + first,
            typed[6] + first, with_weight ? typed[7] + first : nullptr};
}

template<typename T>
void deposit_as(const void *const *columns, const size_t first, const size_t count, const flux::map &m, const flux::field &f,
                const double *packed, const double *fpol, const double *edges, const size_t ns, const double sscale,
                const bool is_private, const unsigned int block, const size_t max_workgroups, const size_t lds_bytes,
                void *state, unsigned long long *counters, hipStream_t stream) {
    const moment_columns<T> in = columns_from<T> (columns, first, columns[7] != nullptr);
    const unsigned int grid = grid_of(count, block, max_workgroups);
    if (is_private) {
        hipLaunchKernelGGL((moment_deposit_kernel<true, T>), dim3(grid), dim3(block), lds_bytes, stream, in,
                           static_cast<unsigned long long> (count), m, f, packed, fpol, edges, static_cast<int> (ns), sscale,
                           static_cast<unsigned long long *> (state), counters);
    } else {
        hipLaunchKernelGGL((moment_deposit_kernel<false, T>), dim3(grid), dim3(block), lds_bytes, stream, in,
                           static_cast<unsigned long long> (count), m, f, packed, fpol, edges, static_cast<int> (ns), sscale,
                           static_cast<unsigned long long *> (state), counters);
    }
}

template<typename T>
void deposit_particles_as(const void *const *columns, const size_t first, const size_t count, const unsigned long long first_particle,
                          const size_t batch_count, const flux::map &m, const flux::field &f, const double *packed,
                          const double *fpol, const double *edges, const size_t ns, const double sscale, const bool is_private,
                          const unsigned int block, const size_t max_workgroups, const size_t lds_bytes, void *state,
                          unsigned long long *counters, hipStream_t stream) {
    const moment_columns<T> in = columns_from<T> (columns, first, columns[7] != nullptr);
    const unsigned int grid = batched_grid_of(count, block, max_workgroups, batch_count);
    if (is_private) {
        hipLaunchKernelGGL((moment_deposit_particles_kernel<true, T>), dim3(grid), dim3(block), lds_bytes, stream, in,
                           static_cast<unsigned long long> (count), first_particle, static_cast<unsigned int> (batch_count), m, f,
                           packed, fpol, edges, static_cast<int> (ns), sscale, static_cast<unsigned long long *> (state), counters);
    } else {
        hipLaunchKernelGGL((moment_deposit_particles_kernel<false, T>), dim3(grid), dim3(block), lds_bytes, stream, in,
                           static_cast<unsigned long long> (count), first_particle, static_cast<unsigned int> (batch_count), m, f,
                           packed, fpol, edges, static_cast<int> (ns), sscale, static_cast<unsigned long long *> (state), counters);
    }
}

}  // namespace

void launch_moment_deposit(const void *const *columns, const bool is_f32, const size_t first, const size_t count,
                           const flux::map &m, const flux::field &f, const double *packed, const double *fpol,
                           const double *edges, const size_t ns, const double sscale, const bool is_private,
                           const unsigned int block, const size_t max_workgroups, const size_t lds_bytes,
                           void *state, unsigned long long *counters, hipStream_t stream) {
    if (count == 0) return;
    if (is_f32) {
        deposit_as<float> (columns, first, count, m, f, packed, fpol, edges, ns, sscale, is_private, block, max_workgroups,
                           lds_bytes, state, counters, stream);
    } else {
        deposit_as<double> (columns, first, count, m, f, packed, fpol, edges, ns, sscale, is_private, block, max_workgroups,
                            lds_bytes, state, counters, stream);
    }
}

void launch_moment_deposit_particles(const void *const *columns, const bool is_f32, const size_t first, const size_t count,
                                     const unsigned long long first_particle, const size_t batch_count, const flux::map &m,
                                     const flux::field &f, const double *packed, const double *fpol, const double *edges,
                                     const size_t ns, const double sscale, const bool is_private, const unsigned int block,
                                     const size_t max_workgroups, const size_t lds_bytes, void *state,
                                     unsigned long long *counters, hipStream_t stream) {
    if (count == 0) return;
    if (is_f32) {
        deposit_particles_as<float> (columns, first, count, first_particle, batch_count, m, f, packed, fpol, edges, ns, sscale,
                                     is_private, block, max_workgroups, lds_bytes, state, counters, stream);
    } else {
        deposit_particles_as<double> (columns, first, count, first_particle, batch_count, m, f, packed, fpol, edges, ns, sscale,
                                      is_private, block, max_workgroups, lds_bytes, state, counters, stream);
    }
}

void launch_moment_values(const void *const *columns, const bool is_f32, const size_t count, const flux::map &m,
                          const flux::field &f, const double *packed, const double *fpol, double *label, double *values,
                          hipStream_t stream) {
    if (count == 0) return;
    const dim3 grid(static_cast<unsigned int> ((count + 255)/256));
    if (is_f32) {
        hipLaunchKernelGGL(moment_values_kernel<float>, grid, dim3(256), 0, stream, columns_from<float> (columns, 0, false),
                           static_cast<unsigned long long> (count), m, f, packed, fpol, label, values);
    } else {
        hipLaunchKernelGGL(moment_values_kernel<double>, grid, dim3(256), 0, stream, columns_from<double> (columns, 0, false),
                           static_cast<unsigned long long> (count), m, f, packed, fpol, label, values);
    }
}

}  // namespace gfhip
