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

//  The label and xi of one particle, both NaN outside the map.  `fpol`: [interval][4], 32-byte aligned.
__device__ __forceinline__ double pitch_at(const flux::map &m, const flux::field &f, const double *__restrict__ packed,
                                           const double *__restrict__ fpol, const double x, const double y, const double z,
                                           const double ux, const double uy, const double uz, double &label) {
    double tr, tz;
    const long long at = flux::locate(m, x, y, z, tr, tz);
    if (at < 0) {
        label = __builtin_nan("");
        return __builtin_nan("");
    }
    double c[16];
    coefficients_at(packed, at, c);
    double gr, gz, tp;
    const double psi = flux::psi_gradient(m, c, tr, tz, gr, gz);
    label = flux::canonical(flux::label_of(m, psi));
    const int q = flux::fpol_interval(f, psi, tp);
    const double2 *line = reinterpret_cast<const double2 *> (fpol) + static_cast<size_t> (q)*2;
    const double2 low = line[0], high = line[1];
    const double cubic[4] = {low.x, low.y, high.x, high.y};
    return flux::pitch_of(x, y, flux::radius_of(x, y), ux, uy, uz, gr, gz, flux::fpol_of(cubic, tp));
}

}  // namespace

template<typename T>
struct phase_columns {
    const T *x, *y, *z, *ux, *uy, *uz, *gamma, *weight;    // weight: null when every particle deposits 1.0
};

//  counters: samples, outside, skipped.  edges: the ns + 1 of the label, the np + 1 of xi, the ng + 1 of gamma.
template<bool PRIVATE, typename T>
__global__ void __launch_bounds__(private_block)
phase_deposit_kernel(const phase_columns<T> in, const unsigned long long count,
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
//  `base` is the same for every lane of the workgroup: the ballots and shuffles below are executed by whole waves, and
//  every wave of the workgroup arrives at the barrier before the flush.
    for (unsigned long long base = static_cast<unsigned long long> (blockIdx.x)*blockDim.x; base < count; base += stride) {
        const unsigned long long at = base + threadIdx.x;
        const bool present = at < count;
        int cell = -1;                                 // outside, as in the lanes past the end
        double v = 0.0;
        if (present) {
            v = in.weight ? static_cast<double> (in.weight[at]) : 1.0;
            double label;
            const double xi = pitch_at(m, f, packed, fpol, static_cast<double> (in.x[at]), static_cast<double> (in.y[at]),
                                       static_cast<double> (in.z[at]), static_cast<double> (in.ux[at]),
                                       static_cast<double> (in.uy[at]), static_cast<double> (in.uz[at]), label);
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
phase_deposit_particles_kernel(const phase_columns<T> in, const unsigned long long count, const unsigned long long first_particle,
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
        v = in.weight ? static_cast<double> (in.weight[at]) : 1.0;
        double label;
        const double xi = pitch_at(m, f, packed, fpol, static_cast<double> (in.x[at]), static_cast<double> (in.y[at]),
                                   static_cast<double> (in.z[at]), static_cast<double> (in.ux[at]),
                                   static_cast<double> (in.uy[at]), static_cast<double> (in.uz[at]), label);
        const int is = deposit::find_cell(sedge, ns, sscale, label);
        const int ip = deposit::find_cell(pedge, np, pscale, xi);
        const int ig = deposit::find_cell(gedge, ng, gscale, static_cast<double> (in.gamma[at]));
        return is >= 0 && ip >= 0 && ig >= 0 ? (is*np + ip)*ng + ig : -1;
    });
}

//  One lane per particle: its label and its xi, NaN outside the map.
template<typename T>
__global__ void __launch_bounds__(256)
phase_coordinates_kernel(const phase_columns<T> in, const unsigned long long count, const flux::map m, const flux::field f,
                         const double *__restrict__ packed, const double *__restrict__ fpol,
                         double *__restrict__ label, double *__restrict__ pitch) {
    const unsigned long long at = static_cast<unsigned long long> (blockIdx.x)*blockDim.x + threadIdx.x;
    if (at < count) {
        double s;
        pitch[at] = pitch_at(m, f, packed, fpol, static_cast<double> (in.x[at]), static_cast<double> (in.y[at]),
                             static_cast<double> (in.z[at]), static_cast<double> (in.ux[at]), static_cast<double> (in.uy[at]),
                             static_cast<double> (in.uz[at]), s);
        label[at] = s;
    }
}

//  Dynamic LDS above 64 KiB has to be asked for: always the cap's size, as flux_prepare does.
hipError_t phase_prepare() {
    for (const void *kernel : {reinterpret_cast<const void *> (&phase_deposit_kernel<true, float>),
                               reinterpret_cast<const void *> (&phase_deposit_kernel<true, double>),
                               reinterpret_cast<const void *> (&phase_deposit_particles_kernel<true, float>),
                               reinterpret_cast<const void *> (&phase_deposit_particles_kernel<true, double>)}) {
        const hipError_t status = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                      static_cast<int> (phase_cap_bytes));
        if (status != hipSuccess) return status;
    }
    return hipSuccess;
}

namespace {

template<typename T>
phase_columns<T> columns_from(const void *const *columns, const size_t first, const bool with_weight) {
    const T *const *typed = reinterpret_cast<const T *const *> (columns);
    return {typed[0] + first, typed[1] + first, typed[2] + first, typed[3] + first, typed[4] + first, typed[5] + first,
            typed[6] + first, with_weight ? typed[7] + first : nullptr};
}

template<typename T>
void deposit_as(const void *const *columns, const size_t first, const size_t count, const flux::map &m, const flux::field &f,
                const double *packed, const double *fpol, const double *edges, const size_t *n, const double *scale,
                const bool is_private, const unsigned int block, const size_t max_workgroups, const size_t lds_bytes,
                void *state, unsigned long long *counters, hipStream_t stream) {
    const phase_columns<T> in = columns_from<T> (columns, first, columns[7] != nullptr);
    const unsigned int grid = grid_of(count, block, max_workgroups);
    if (is_private) {
        hipLaunchKernelGGL((phase_deposit_kernel<true, T>), dim3(grid), dim3(block), lds_bytes, stream, in,
                           static_cast<unsigned long long> (count), m, f, packed, fpol, edges, static_cast<int> (n[0]),
                           static_cast<int> (n[1]), static_cast<int> (n[2]), scale[0], scale[1], scale[2],
                           static_cast<unsigned long long *> (state), counters);
    } else {
        hipLaunchKernelGGL((phase_deposit_kernel<false, T>), dim3(grid), dim3(block), lds_bytes, stream, in,
                           static_cast<unsigned long long> (count), m, f, packed, fpol, edges, static_cast<int> (n[0]),
                           static_cast<int> (n[1]), static_cast<int> (n[2]), scale[0], scale[1], scale[2],
                           static_cast<unsigned long long *> (state), counters);
    }
}

template<typename T>
void deposit_particles_as(const void *const *columns, const size_t first, const size_t count, const unsigned long long first_particle,
                          const size_t batch_count, const flux::map &m, const flux::field &f, const double *packed,
                          const double *fpol, const double *edges, const size_t *n, const double *scale, const bool is_private,
                          const unsigned int block, const size_t max_workgroups, const size_t lds_bytes, void *state,
                          unsigned long long *counters, hipStream_t stream) {
    const phase_columns<T> in = columns_from<T> (columns, first, columns[7] != nullptr);
    const unsigned int grid = batched_grid_of(count, block, max_workgroups, batch_count);
    if (is_private) {
        hipLaunchKernelGGL((phase_deposit_particles_kernel<true, T>), dim3(grid), dim3(block), lds_bytes, stream, in,
                           static_cast<unsigned long long> (count), first_particle, static_cast<unsigned int> (batch_count), m, f,
                           packed, fpol, edges, static_cast<int> (n[0]), static_cast<int> (n[1]), static_cast<int> (n[2]),
                           scale[0], scale[1], scale[2], static_cast<unsigned long long *> (state), counters);
    } else {
        hipLaunchKernelGGL((phase_deposit_particles_kernel<false, T>), dim3(grid), dim3(block), lds_bytes, stream, in,
                           static_cast<unsigned long long> (count), first_particle, static_cast<unsigned int> (batch_count), m, f,
                           packed, fpol, edges, static_cast<int> (n[0]), static_cast<int> (n[1]), static_cast<int> (n[2]),
                           scale[0], scale[1], scale[2], static_cast<unsigned long long *> (state), counters);
    }
}

}  // namespace

void launch_phase_deposit(const void *const *columns, const bool is_f32, const size_t first, const size_t count,
                          const flux::map &m, const flux::field &f, const double *packed, const double *fpol,
                          const double *edges, const size_t *n, const double *scale, const bool is_private,
                          const unsigned int block, const size_t max_workgroups, const size_t lds_bytes,
                          void *state, unsigned long long *counters, hipStream_t stream) {
    if (count == 0) return;
    if (is_f32) {
        deposit_as<float> (columns, first, count, m, f, packed, fpol, edges, n, scale, is_private, block, max_workgroups,
                           lds_bytes, state, counters, stream);
    } else {
        deposit_as<double> (columns, first, count, m, f, packed, fpol, edges, n, scale, is_private, block, max_workgroups,
                            lds_bytes, state, counters, stream);
    }
}

void launch_phase_deposit_particles(const void *const *columns, const bool is_f32, const size_t first, const size_t count,
                                    const unsigned long long first_particle, const size_t batch_count, const flux::map &m,
                                    const flux::field &f, const double *packed, const double *fpol, const double *edges,
                                    const size_t *n, const double *scale, const bool is_private, const unsigned int block,
                                    const size_t max_workgroups, const size_t lds_bytes, void *state,
                                    unsigned long long *counters, hipStream_t stream) {
    if (count == 0) return;
    if (is_f32) {
        deposit_particles_as<float> (columns, first, count, first_particle, batch_count, m, f, packed, fpol, edges, n, scale,
                                     is_private, block, max_workgroups, lds_bytes, state, counters, stream);
    } else {
        deposit_particles_as<double> (columns, first, count, first_particle, batch_count, m, f, packed, fpol, edges, n, scale,
                                      is_private, block, max_workgroups, lds_bytes, state, counters, stream);
    }
}

void launch_phase_coordinates(const void *const *columns, const bool is_f32, const size_t count, const flux::map &m,
                              const flux::field &f, const double *packed, const double *fpol, double *label, double *pitch,
                              hipStream_t stream) {
    if (count == 0) return;
    const dim3 grid(static_cast<unsigned int> ((count + 255)/256));
    if (is_f32) {
        hipLaunchKernelGGL(phase_coordinates_kernel<float>, grid, dim3(256), 0, stream, columns_from<float> (columns, 0, false),
                           static_cast<unsigned long long> (count), m, f, packed, fpol, label, pitch);
    } else {
        hipLaunchKernelGGL(phase_coordinates_kernel<double>, grid, dim3(256), 0, stream, columns_from<double> (columns, 0, false),
                           static_cast<unsigned long long> (count), m, f, packed, fpol, label, pitch);
    }
}

}  // namespace gfhip
