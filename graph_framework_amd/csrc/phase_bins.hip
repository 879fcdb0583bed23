//------------------------------------------------------------------------------
///  @file phase_bins.hip
///  @brief The distribution of particles over the flux label, the pitch cosine and gamma, exact sums (hand-written,
///  gfx950).
///
///  A particle (x, y, z, ux, uy, uz, gamma), seven reads of fp32 or fp64 (the push's state as it lies on the device), is
///  widened to fp64, which is exact, and gets the label and xi = (u.B)/(|u||B|) of flux_label.hpp: psi and its two
///  derivatives from the cell's 16 coefficients, fpol from the interval's four, as flux_spectrum.hip reads them.  gamma is
///  taken as it is.  The particle belongs to cell (is, ip, ig) iff each of the three lies in [edge[i], edge[i+1]) of its
///  axis by cell_deposit.hpp's find_cell; the cells are ns*np*ng superaccumulators, flat index (is*np + ip)*ng + ig.  It
///  deposits its weight, an eighth column of the same type, or 1.0 where there is none.
///
///  The sums are flux_sums.hpp's: up to 256 cells every workgroup owns the grid in LDS, the three axes' edges staged
///  behind it; above that, or with the map's no-private flag, deposits go to the global state behind the wave pre-sum
///  (particles without a weight that share a cell share the limbs too: three atomics per wave).  The state does not
///  depend on the route, the launch shape, the order of the particles or their type.
///
///  phase_deposit_particles_kernel keeps the same sums per batch of particles (ray_batches.hpp, the particle's index in
///  the ensemble in place of a ray's), state [batch][is][ip][ig][limb], one batch at a time in a workgroup's LDS.
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

//  The most edges of the private path's three axes: ns*np*ng <= 256 gives ns + np + ng <= 258, three more edges than cells.
constexpr size_t phase_cap_bytes = private_cap*bytes_per_cell + (private_cap + 5)*sizeof(double);
static_assert(phase_cap_bytes <= lds_per_workgroup, "the cap fits one workgroup's LDS");

//  The label and xi of one particle, both NaN outside the map.
__device__ __forceinline__ double pitch_at(const flux::map &m, const flux::field &f, const double *__restrict__ packed,
                                           const double *__restrict__ fpol, const double x, const double y, const double z,
                                           const double ux, const double uy, const double uz, double &label) {
    field_point p;
    if (!point_at(m, f, packed, fpol, x, y, z, p)) {
        label = __builtin_nan("");
        return __builtin_nan("");
    }
    label = p.label;
    return flux::pitch_of(x, y, flux::radius_of(x, y), ux, uy, uz, p.gr, p.gz, p.fpol);
}

//  The same of particle `at` of the columns, widened to fp64.
template<typename T>
__device__ __forceinline__ double pitch_at(const flux::map &m, const flux::field &f, const double *__restrict__ packed,
                                           const double *__restrict__ fpol, const particle_columns<T> &in,
                                           const unsigned long long at, double &label) {
    return pitch_at(m, f, packed, fpol, static_cast<double> (in.x[at]), static_cast<double> (in.y[at]),
                    static_cast<double> (in.z[at]), static_cast<double> (in.ux[at]), static_cast<double> (in.uy[at]),
                    static_cast<double> (in.uz[at]), label);
}

}  // namespace

//  counters: samples, outside, skipped.  edges: the ns + 1 of the label, the np + 1 of xi, the ng + 1 of gamma.  The loop
//  stays written out: behind a shared loop function this kernel's <true, float> needs 85 registers where it has 79
//  here, one wave per SIMD fewer.
template<bool PRIVATE, typename T>
__global__ void __launch_bounds__(private_block)
phase_deposit_kernel(const particle_columns<T> in, const unsigned long long count,
                     const flux::map m, const flux::field f, const double *__restrict__ packed,
                     const double *__restrict__ fpol, const double *__restrict__ edges, const int ns, const int np, const int ng,
                     const double sscale, const double pscale, const double gscale,
                     unsigned long long *__restrict__ state, unsigned long long *__restrict__ counters) {
    extern __shared__ unsigned long long shared[];
    workgroup_sums<PRIVATE> sums;
    sums.open(shared, edges, ns*np*ng, ns + np + ng + 3);
    const double *sedge = sums.staged, *pedge = sedge + ns + 1, *gedge = pedge + np + 1;
    deposit::tallies tally;
    const unsigned long long stride = static_cast<unsigned long long> (gridDim.x)*blockDim.x;
    for (unsigned long long base = static_cast<unsigned long long> (blockIdx.x)*blockDim.x; base < count; base += stride) {
        const unsigned long long at = base + threadIdx.x;
        const bool present = at < count;
        int cell = -1;                                 // outside, as in the lanes past the end
        double v = 0.0;
        if (present) {
            v = in.weight_of(at);
            double label;
            const double xi = pitch_at(m, f, packed, fpol, in, at, label);
            const int is = deposit::find_cell(sedge, ns, sscale, label);
            const int ip = deposit::find_cell(pedge, np, pscale, xi);
            const int ig = deposit::find_cell(gedge, ng, gscale, static_cast<double> (in.gamma[at]));
            if (is >= 0 && ip >= 0 && ig >= 0) cell = (is*np + ip)*ng + ig;
        }
        const deposit::contribution a = deposit::contribution_of(cell >= 0, static_cast<unsigned int> (cell), v);
        deposit::count(tally, present, a);
        sums.add(state, a);
    }
    sums.close(state);
    deposit::flush(tally, counters);
}

//  phase_deposit_kernel with the particles' indices in the ensemble: sample i is particle first_particle + i, and the
//  state is [batch][is][ip][ig][limb] (flux_sums.hpp's deposit_batched, a particle in place of a ray).
template<bool PRIVATE, typename T>
__global__ void __launch_bounds__(private_block)
phase_deposit_particles_kernel(const particle_columns<T> in, const unsigned long long count, const unsigned long long first_particle,
                               const unsigned int batch_count, const flux::map m, const flux::field f,
                               const double *__restrict__ packed, const double *__restrict__ fpol,
                               const double *__restrict__ edges, const int ns, const int np, const int ng,
                               const double sscale, const double pscale, const double gscale,
                               unsigned long long *__restrict__ state, unsigned long long *__restrict__ counters) {
    extern __shared__ unsigned long long shared[];
    workgroup_sums<PRIVATE> sums;
    sums.open(shared, edges, ns*np*ng, ns + np + ng + 3);
    const double *sedge = sums.staged, *pedge = sedge + ns + 1, *gedge = pedge + np + 1;
    deposit_batched(sums, first_particle, count, batch_count, ns*np*ng, state, counters, [&](const uint64_t at, double &v) {
        v = in.weight_of(at);
        double label;
        const double xi = pitch_at(m, f, packed, fpol, in, at, label);
        const int is = deposit::find_cell(sedge, ns, sscale, label);
        const int ip = deposit::find_cell(pedge, np, pscale, xi);
        const int ig = deposit::find_cell(gedge, ng, gscale, static_cast<double> (in.gamma[at]));
        return is >= 0 && ip >= 0 && ig >= 0 ? (is*np + ip)*ng + ig : -1;
    });
}

//  One lane per particle: its label and its xi, NaN outside the map.
template<typename T>
__global__ void __launch_bounds__(256)
phase_coordinates_kernel(const particle_columns<T> in, const unsigned long long count, const flux::map m, const flux::field f,
                         const double *__restrict__ packed, const double *__restrict__ fpol,
                         double *__restrict__ label, double *__restrict__ pitch) {
    const unsigned long long at = static_cast<unsigned long long> (blockIdx.x)*blockDim.x + threadIdx.x;
    if (at < count) {
        double s;
        pitch[at] = pitch_at(m, f, packed, fpol, in, at, s);
        label[at] = s;
    }
}

hipError_t phase_prepare() {
    return prepare_private({reinterpret_cast<const void *> (&phase_deposit_kernel<true, float>),
                            reinterpret_cast<const void *> (&phase_deposit_kernel<true, double>),
                            reinterpret_cast<const void *> (&phase_deposit_particles_kernel<true, float>),
                            reinterpret_cast<const void *> (&phase_deposit_particles_kernel<true, double>)}, phase_cap_bytes);
}

void launch_phase_deposit(const void *const *columns, const bool is_f32, const size_t first, const size_t count,
                          const cell_tables &t, const double *edges, const size_t *n, const double *scale,
                          const launch_shape &shape, const cell_target &to) {
    if (count == 0) return;
    with_particle_type(is_f32, [&](auto type) {
        using T = decltype(type);
        launch_on_route(phase_deposit_kernel<true, T>, phase_deposit_kernel<false, T>, shape,
                        grid_of(count, shape.block, shape.max_workgroups), to.stream,
                        columns_from<T> (columns, first, columns[7] != nullptr), static_cast<unsigned long long> (count), t.map,
                        t.field, t.packed, t.fpol, edges, static_cast<int> (n[0]), static_cast<int> (n[1]), static_cast<int> (n[2]),
                        scale[0], scale[1], scale[2], static_cast<unsigned long long *> (to.state), to.counters);
    });
}

void launch_phase_deposit_particles(const void *const *columns, const bool is_f32, const size_t first, const size_t count,
                                    const unsigned long long first_particle, const size_t batch_count, const cell_tables &t,
                                    const double *edges, const size_t *n, const double *scale, const launch_shape &shape,
                                    const cell_target &to) {
    if (count == 0) return;
    with_particle_type(is_f32, [&](auto type) {
        using T = decltype(type);
        launch_on_route(phase_deposit_particles_kernel<true, T>, phase_deposit_particles_kernel<false, T>, shape,
                        batched_grid_of(count, shape.block, shape.max_workgroups, batch_count), to.stream,
                        columns_from<T> (columns, first, columns[7] != nullptr), static_cast<unsigned long long> (count),
                        first_particle, static_cast<unsigned int> (batch_count), t.map, t.field, t.packed, t.fpol, edges,
                        static_cast<int> (n[0]), static_cast<int> (n[1]), static_cast<int> (n[2]), scale[0], scale[1], scale[2],
                        static_cast<unsigned long long *> (to.state), to.counters);
    });
}

void launch_phase_coordinates(const void *const *columns, const bool is_f32, const size_t count, const cell_tables &t,
                              double *label, double *pitch, hipStream_t stream) {
    if (count == 0) return;
    with_particle_type(is_f32, [&](auto type) {
        using T = decltype(type);
        hipLaunchKernelGGL(phase_coordinates_kernel<T>, dim3(static_cast<unsigned int> ((count + 255)/256)), dim3(256), 0, stream,
                           columns_from<T> (columns, 0, false), static_cast<unsigned long long> (count), t.map, t.field, t.packed,
                           t.fpol, label, pitch);
    });
}

}  // namespace gfhip
