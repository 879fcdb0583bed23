//------------------------------------------------------------------------------
///  @file flux_spectrum.hip
///  @brief Binning of per-sample values over the flux label and the parallel refractive index, exact sums (hand-written,
///  gfx950).
///
///  A sample (x, y, z, kx, ky, kz, w, value), eight fp64 reads, gets the label and N = c (k.B)/(|B| w) of
///  flux_label.hpp: psi and its two derivatives from the cell's 16 coefficients (the [cell][16] line of
///  flux_profile.hip), fpol from the interval's four ([q][4], one 32-byte line).  It belongs to cell (is, in) iff
///  sedge[is] <= label < sedge[is+1] and nedge[in] <= N < nedge[in+1], both by cell_deposit.hpp's find_cell; the cells
///  are ns*nn superaccumulators, flat index is*nn + in.
///
///  The sums are flux_sums.hpp's: up to 256 cells every workgroup owns the grid in LDS, the two axes' edges staged
///  behind it; above that, or with the map's no-private flag, deposits go to the global state behind the wave pre-sum.
///  The state does not depend on the route, the launch shape or the order of the samples.
///
///  spectrum_deposit_rays_kernel keeps the same sums per batch of rays (ray_batches.hpp), state [batch][is][in][limb],
///  one batch at a time in a workgroup's LDS.
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

//  The most edges of the private path's two axes: ns*nn <= 256 gives ns + nn <= 257.
constexpr size_t private_cap_bytes = private_cap*bytes_per_cell + (private_cap + 3)*sizeof(double);
static_assert(private_cap_bytes <= lds_per_workgroup, "the cap fits one workgroup's LDS");

//  The label and N of one sample, both NaN outside the map.
__device__ __forceinline__ double npar_at(const flux::map &m, const flux::field &f, const double *__restrict__ packed,
                                          const double *__restrict__ fpol, const double x, const double y, const double z,
                                          const double kx, const double ky, const double kz, const double w, double &label) {
    field_point p;
    if (!point_at(m, f, packed, fpol, x, y, z, p)) {
        label = __builtin_nan("");
        return __builtin_nan("");
    }
    label = p.label;
    return flux::npar_of(f, x, y, flux::radius_of(x, y), kx, ky, kz, w, p.gr, p.gz, p.fpol);
}

}  // namespace

struct spectrum_columns {
    const double *x, *y, *z, *kx, *ky, *kz, *w, *value;
};

//  counters: samples, outside, skipped.  edges: the ns + 1 of the label, then the nn + 1 of N.
template<bool PRIVATE>
__global__ void __launch_bounds__(private_block)
spectrum_deposit_kernel(const spectrum_columns in, const unsigned long long count,
                        const flux::map m, const flux::field f, const double *__restrict__ packed,
                        const double *__restrict__ fpol, const double *__restrict__ edges, const int ns, const int nn,
                        const double sscale, const double nscale,
                        unsigned long long *__restrict__ state, unsigned long long *__restrict__ counters) {
    extern __shared__ unsigned long long shared[];
    workgroup_sums<PRIVATE> sums;
    sums.open(shared, edges, ns*nn, ns + nn + 2);
    const double *sedge = sums.staged, *nedge = sums.staged + ns + 1;

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
            v = in.value[at];
            double label;
            const double npar = npar_at(m, f, packed, fpol, in.x[at], in.y[at], in.z[at], in.kx[at], in.ky[at], in.kz[at],
                                        in.w[at], label);
            const int is = deposit::find_cell(sedge, ns, sscale, label);
            const int in_n = deposit::find_cell(nedge, nn, nscale, npar);
            if (is >= 0 && in_n >= 0) cell = is*nn + in_n;
        }
        const deposit::contribution a = deposit::contribution_of(cell >= 0, static_cast<unsigned int> (cell), v);
        deposit::count(tally, present, a);
        sums.add(state, a);
    }
    sums.close(state);
    deposit::flush(tally, counters);
}

//  spectrum_deposit_kernel with the samples' rays: sample i is ray first_ray + i, and the state is
//  [batch][is][in][limb] (flux_sums.hpp's deposit_batched).
template<bool PRIVATE>
__global__ void __launch_bounds__(private_block)
spectrum_deposit_rays_kernel(const spectrum_columns in, const unsigned long long count, const unsigned long long first_ray,
                             const unsigned int batch_count, const flux::map m, const flux::field f,
                             const double *__restrict__ packed, const double *__restrict__ fpol,
                             const double *__restrict__ edges, const int ns, const int nn, const double sscale,
                             const double nscale, unsigned long long *__restrict__ state,
                             unsigned long long *__restrict__ counters) {
    extern __shared__ unsigned long long shared[];
    workgroup_sums<PRIVATE> sums;
    sums.open(shared, edges, ns*nn, ns + nn + 2);
    const double *sedge = sums.staged, *nedge = sums.staged + ns + 1;
    deposit_batched(sums, first_ray, count, batch_count, ns*nn, state, counters, [&](const uint64_t at, double &v) {
        v = in.value[at];
        double label;
        const double npar = npar_at(m, f, packed, fpol, in.x[at], in.y[at], in.z[at], in.kx[at], in.ky[at], in.kz[at],
                                    in.w[at], label);
        const int is = deposit::find_cell(sedge, ns, sscale, label);
        const int in_n = deposit::find_cell(nedge, nn, nscale, npar);
        return is >= 0 && in_n >= 0 ? is*nn + in_n : -1;
    });
}

//  One lane per point: its label and its N, NaN outside the map.
__global__ void __launch_bounds__(256)
spectrum_npar_kernel(const spectrum_columns in, const unsigned long long count, const flux::map m, const flux::field f,
                     const double *__restrict__ packed, const double *__restrict__ fpol,
                     double *__restrict__ label, double *__restrict__ npar) {
    const unsigned long long at = static_cast<unsigned long long> (blockIdx.x)*blockDim.x + threadIdx.x;
    if (at < count) {
        double s;
        npar[at] = npar_at(m, f, packed, fpol, in.x[at], in.y[at], in.z[at], in.kx[at], in.ky[at], in.kz[at], in.w[at], s);
        label[at] = s;
    }
}

hipError_t spectrum_prepare() {
    return prepare_private({reinterpret_cast<const void *> (&spectrum_deposit_kernel<true>),
                            reinterpret_cast<const void *> (&spectrum_deposit_rays_kernel<true>)}, private_cap_bytes);
}

namespace {

//  The first `used` columns from sample `first` on.
spectrum_columns columns_at(const double *const *columns, const size_t first, const bool with_value) {
    return {columns[0] + first, columns[1] + first, columns[2] + first, columns[3] + first, columns[4] + first,
            columns[5] + first, columns[6] + first, with_value ? columns[7] + first : nullptr};
}

}  // namespace

void launch_spectrum_deposit(const double *const *columns, const size_t first, const size_t count, const cell_tables &t,
                             const double *edges, const size_t *n, const double *scale, const launch_shape &shape,
                             const cell_target &to) {
    if (count == 0) return;
    launch_on_route(spectrum_deposit_kernel<true>, spectrum_deposit_kernel<false>, shape,
                    grid_of(count, shape.block, shape.max_workgroups), to.stream, columns_at(columns, first, true),
                    static_cast<unsigned long long> (count), t.map, t.field, t.packed, t.fpol, edges, static_cast<int> (n[0]),
                    static_cast<int> (n[1]), scale[0], scale[1], static_cast<unsigned long long *> (to.state), to.counters);
}

void launch_spectrum_deposit_rays(const double *const *columns, const size_t first, const size_t count,
                                  const unsigned long long first_ray, const size_t batch_count, const cell_tables &t,
                                  const double *edges, const size_t *n, const double *scale, const launch_shape &shape,
                                  const cell_target &to) {
    if (count == 0) return;
    launch_on_route(spectrum_deposit_rays_kernel<true>, spectrum_deposit_rays_kernel<false>, shape,
                    batched_grid_of(count, shape.block, shape.max_workgroups, batch_count), to.stream,
                    columns_at(columns, first, true), static_cast<unsigned long long> (count), first_ray,
                    static_cast<unsigned int> (batch_count), t.map, t.field, t.packed, t.fpol, edges, static_cast<int> (n[0]),
                    static_cast<int> (n[1]), scale[0], scale[1], static_cast<unsigned long long *> (to.state), to.counters);
}

void launch_spectrum_npar(const double *const *columns, const size_t count, const cell_tables &t, double *label, double *npar,
                          hipStream_t stream) {
    if (count == 0) return;
    hipLaunchKernelGGL(spectrum_npar_kernel, dim3(static_cast<unsigned int> ((count + 255)/256)), dim3(256), 0, stream,
                       columns_at(columns, 0, false), static_cast<unsigned long long> (count), t.map, t.field, t.packed, t.fpol,
                       label, npar);
}

}  // namespace gfhip
