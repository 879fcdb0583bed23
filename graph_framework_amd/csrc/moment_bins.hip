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

//  The label and the four moments of one particle, all NaN outside the map.
__device__ __forceinline__ double moments_at(const flux::map &m, const flux::field &f, const double *__restrict__ packed,
                                             const double *__restrict__ fpol, const double x, const double y, const double z,
                                             const double ux, const double uy, const double uz, const double gamma,
                                             double *moments) {
    field_point p;
    if (!point_at(m, f, packed, fpol, x, y, z, p)) {
#pragma unroll
        for (int k = 0; k < moment_count; k++) moments[k] = __builtin_nan("");
        return __builtin_nan("");
    }
    flux::moments_of(x, y, flux::radius_of(x, y), ux, uy, uz, gamma, p.gr, p.gz, p.fpol, moments);
//  Not p.label: formed here, after the moments, the label is not held in registers across them (the kernels below need
//  up to 12 fewer, one to two waves per SIMD more).
    return flux::canonical(flux::label_of(m, p.psi));
}

//  The same of particle `at` of the columns, widened to fp64.
template<typename T>
__device__ __forceinline__ double moments_at(const flux::map &m, const flux::field &f, const double *__restrict__ packed,
                                             const double *__restrict__ fpol, const particle_columns<T> &in,
                                             const unsigned long long at, double *moments) {
    return moments_at(m, f, packed, fpol, static_cast<double> (in.x[at]), static_cast<double> (in.y[at]),
                      static_cast<double> (in.z[at]), static_cast<double> (in.ux[at]), static_cast<double> (in.uy[at]),
                      static_cast<double> (in.uz[at]), static_cast<double> (in.gamma[at]), moments);
}

}  // namespace

//  counters: samples, outside, skipped, counted per particle.  edges: the ns + 1 of the label.  The loop is written out
//  here: behind a shared loop function the four variants of this kernel need 2 to 10 registers more and lose a wave
//  per SIMD each.
template<bool PRIVATE, typename T>
__global__ void __launch_bounds__(private_block)
moment_deposit_kernel(const particle_columns<T> in, const unsigned long long count,
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
            const double w = in.weight_of(at);
            double moments[moment_count];
            const double label = moments_at(m, f, packed, fpol, in, at, moments);
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
moment_deposit_particles_kernel(const particle_columns<T> in, const unsigned long long count, const unsigned long long first_particle,
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
        const double w = in.weight_of(at);
        double moments[moment_count];
        const double label = moments_at(m, f, packed, fpol, in, at, moments);
        flux::weighted_moments(w, moments, v);
        finite = flux::moments_finite(v);
        return deposit::find_cell(sedge, ns, sscale, label);
    });
}

//  One lane per particle: its label and its four moments, values[at*4 + k], NaN outside the map.
template<typename T>
__global__ void __launch_bounds__(256)
moment_values_kernel(const particle_columns<T> in, const unsigned long long count, const flux::map m, const flux::field f,
                     const double *__restrict__ packed, const double *__restrict__ fpol,
                     double *__restrict__ label, double *__restrict__ values) {
    const unsigned long long at = static_cast<unsigned long long> (blockIdx.x)*blockDim.x + threadIdx.x;
    if (at < count) {
        double moments[moment_count];
        label[at] = moments_at(m, f, packed, fpol, in, at, moments);
#pragma unroll
        for (int k = 0; k < moment_count; k++) values[at*moment_count + k] = moments[k];
    }
}

hipError_t moments_prepare() {
    return prepare_private({reinterpret_cast<const void *> (&moment_deposit_kernel<true, float>),
                            reinterpret_cast<const void *> (&moment_deposit_kernel<true, double>),
                            reinterpret_cast<const void *> (&moment_deposit_particles_kernel<true, float>),
                            reinterpret_cast<const void *> (&moment_deposit_particles_kernel<true, double>)}, moment_cap_bytes);
}

void launch_moment_deposit(const void *const *columns, const bool is_f32, const size_t first, const size_t count,
                           const cell_tables &t, const double *edges, const size_t ns, const double sscale,
                           const launch_shape &shape, const cell_target &to) {
    if (count == 0) return;
    with_particle_type(is_f32, [&](auto type) {
        using T = decltype(type);
        launch_on_route(moment_deposit_kernel<true, T>, moment_deposit_kernel<false, T>, shape,
                        grid_of(count, shape.block, shape.max_workgroups), to.stream,
                        columns_from<T> (columns, first, columns[7] != nullptr), static_cast<unsigned long long> (count), t.map,
                        t.field, t.packed, t.fpol, edges, static_cast<int> (ns), sscale,
                        static_cast<unsigned long long *> (to.state), to.counters);
    });
}

void launch_moment_deposit_particles(const void *const *columns, const bool is_f32, const size_t first, const size_t count,
                                     const unsigned long long first_particle, const size_t batch_count, const cell_tables &t,
                                     const double *edges, const size_t ns, const double sscale, const launch_shape &shape,
                                     const cell_target &to) {
    if (count == 0) return;
    with_particle_type(is_f32, [&](auto type) {
        using T = decltype(type);
        launch_on_route(moment_deposit_particles_kernel<true, T>, moment_deposit_particles_kernel<false, T>, shape,
                        batched_grid_of(count, shape.block, shape.max_workgroups, batch_count), to.stream,
                        columns_from<T> (columns, first, columns[7] != nullptr), static_cast<unsigned long long> (count),
                        first_particle, static_cast<unsigned int> (batch_count), t.map, t.field, t.packed, t.fpol, edges,
                        static_cast<int> (ns), sscale, static_cast<unsigned long long *> (to.state), to.counters);
    });
}

void launch_moment_values(const void *const *columns, const bool is_f32, const size_t count, const cell_tables &t,
                          double *label, double *values, hipStream_t stream) {
    if (count == 0) return;
    with_particle_type(is_f32, [&](auto type) {
        using T = decltype(type);
        hipLaunchKernelGGL(moment_values_kernel<T>, dim3(static_cast<unsigned int> ((count + 255)/256)), dim3(256), 0, stream,
                           columns_from<T> (columns, 0, false), static_cast<unsigned long long> (count), t.map, t.field, t.packed,
                           t.fpol, label, values);
    });
}

}  // namespace gfhip
