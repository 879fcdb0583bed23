//------------------------------------------------------------------------------
///  @file flux_sums.hpp
///  @brief What the deposit kernels of flux_profile.hip, flux_spectrum.hip, phase_bins.hip, moment_bins.hip and
///  confinement.hip share.  Device side: the label of a point from the repacked psi tables and the point with its field
///  (point_at), a workgroup's sums, private in LDS or global, and the deposit of the batched variants, one batch of rays
///  or particles (ray_batches.hpp) at a time, with one value per sample or several.  The plain kernels keep their
///  grid-stride loop written out: behind a shared loop function they need more registers or run slower (DESIGN.md
///  section 19).  Launch side: the particles' columns, the grid of a launch and the helpers that choose a kernel's route
///  and type.
//------------------------------------------------------------------------------
#ifndef GFHIP_FLUX_SUMS_HPP
#define GFHIP_FLUX_SUMS_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "cell_deposit.hpp"
#include "cell_launch.hpp"
#include "flux_label.hpp"
#include "ray_batches.hpp"
#include "superacc.hpp"

namespace gfhip {
namespace sums {

constexpr unsigned int private_block = 1024;           // 16 waves: one workgroup per CU at the cap still has 4 waves per SIMD
constexpr unsigned int global_block = 256;
constexpr size_t lds_per_workgroup = 160u*1024u;
constexpr size_t private_cap = 256;                    // cells: 256*536 + 257*8 = 139,272 B of the 163,840 a workgroup may declare
constexpr size_t bytes_per_cell = superacc::limbs*sizeof(unsigned long long);

//  A cell's 16 coefficients.  `packed`: [table cell][16], 16-byte aligned.
__device__ __forceinline__ void coefficients_at(const double *__restrict__ packed, const long long at, double *c) {
    const double2 *line = reinterpret_cast<const double2 *> (packed) + at*8;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const double2 pair = line[k];
        c[2*k] = pair.x;
        c[2*k + 1] = pair.y;
    }
}

//  The label of one point, NaN outside the map.
__device__ __forceinline__ double label_at(const flux::map &m, const double *__restrict__ packed,
                                           const double x, const double y, const double z) {
    double tr, tz;
    const long long at = flux::locate(m, x, y, z, tr, tz);
    if (at < 0) return __builtin_nan("");
    double c[16];
    coefficients_at(packed, at, c);
    return flux::label_of(m, flux::psi_of(c, tr, tz));
}

//  A point inside the map as the spectrum, the distribution and the moments need it: psi, its derivatives along R and
//  z, the canonical label and fpol.
struct field_point {
    double psi, gr, gz, label, fpol;
};

//  The field_point of (x, y, z), or false outside the map (`p` is then left alone).  `fpol`: [interval][4], 32-byte
//  aligned.  Only calls of flux_label.hpp's functions: no arithmetic of its own.
__device__ __forceinline__ bool point_at(const flux::map &m, const flux::field &f, const double *__restrict__ packed,
                                         const double *__restrict__ fpol, const double x, const double y, const double z,
                                         field_point &p) {
    double tr, tz;
    const long long at = flux::locate(m, x, y, z, tr, tz);
    if (at < 0) return false;
    double c[16];
    coefficients_at(packed, at, c);
    double tp;
    p.psi = flux::psi_gradient(m, c, tr, tz, p.gr, p.gz);
    const int q = flux::fpol_interval(f, p.psi, tp);
    const double2 *line = reinterpret_cast<const double2 *> (fpol) + static_cast<size_t> (q)*2;
    const double2 low = line[0], high = line[1];
    const double cubic[4] = {low.x, low.y, high.x, high.y};
    p.fpol = flux::fpol_of(cubic, tp);
    p.label = flux::canonical(flux::label_of(m, p.psi));
    return true;
}

//  What the deposit kernels share.  PRIVATE: dynamic LDS = cells*67 limbs, then the staged edges; else the edges
//  alone.  open(): the limbs zeroed and the edges staged; add(): one lane's contribution, executed by whole waves;
//  close(): the workgroup's non-zero limbs to the global state.
template<bool PRIVATE>
struct workgroup_sums {
    unsigned long long *shared;
    unsigned int words;
    double *staged;

//  `edge_count` edges behind the limbs: a profile's cells + 1, or a spectrum's two axes one after the other.
    __device__ __forceinline__ void open(unsigned long long *lds, const double *__restrict__ edges, const int cells,
                                         const int edge_count) {
        shared = lds;
        words = PRIVATE ? static_cast<unsigned int> (cells)*superacc::limbs : 0u;
        staged = reinterpret_cast<double *> (shared + words);
        for (unsigned int i = threadIdx.x; i < words; i += blockDim.x) shared[i] = 0ull;
        for (int i = threadIdx.x; i < edge_count; i += blockDim.x) staged[i] = edges[i];
        __syncthreads();
    }

    __device__ __forceinline__ void open(unsigned long long *lds, const double *__restrict__ edges, const int cells) {
        open(lds, edges, cells, cells + 1);
    }

//  The private grid takes every lane's chunks as they are (ds_add_u64): the pre-sum of the global path, measured with
//  and without it, made no difference there.
    __device__ __forceinline__ void add(unsigned long long *__restrict__ state, const deposit::contribution &a) const {
        if constexpr (PRIVATE) {
            deposit::add_limbs(shared, a.key, a.c0, a.c1, a.c2);
        } else {
            deposit::add_limbs_presummed(state, a);
        }
    }

    __device__ __forceinline__ void close(unsigned long long *__restrict__ state) const {
        if constexpr (PRIVATE) {
            __syncthreads();
            for (unsigned int i = threadIdx.x; i < words; i += blockDim.x) {
                const unsigned long long sum = shared[i];
                if (sum) atomicAdd(state + i, sum);
            }
        }
    }

//  Between two barriers: no wave adds to a limb that another one has yet to hand over.
    __device__ __forceinline__ void drain(unsigned long long *__restrict__ state) const {
        if constexpr (PRIVATE) {
            __syncthreads();
            for (unsigned int i = threadIdx.x; i < words; i += blockDim.x) {
                const unsigned long long sum = shared[i];
                if (sum) {
                    atomicAdd(state + i, sum);
                    shared[i] = 0ull;
                }
            }
            __syncthreads();
        }
    }
};

//  The body of the batched deposit kernels.  The state is batch-major, [batch][cell][limb]: slab g is the state of the
//  samples whose ray, first_ray + the sample's index, belongs to batch g.  The workgroup follows ray_batches.hpp's
//  walk: it holds the sums of ONE batch at a time (`cells` of them, whatever the number of batches), its waves take
//  that batch's chunks of 64 rays, and it drains into the batch's slab before it goes on.  On the global path the
//  batch is part of the cell, g*cells + cell, and a wave still has one batch: the pre-sum keeps working.
//  sample(at, value): the cell of sample `at`, or -1, and its value.  counters: samples, outside, skipped.
template<bool PRIVATE, typename SAMPLE>
__device__ __forceinline__ void deposit_batched(const workgroup_sums<PRIVATE> &sums, const unsigned long long first_ray,
                                                const unsigned long long count, const unsigned int batch_count, const int cells,
                                                unsigned long long *__restrict__ state,
                                                unsigned long long *__restrict__ counters, SAMPLE sample) {
    deposit::tallies tally;
    const unsigned int lane = threadIdx.x & 63u;
    const unsigned int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    batches::walk(first_ray, count, batch_count, gridDim.x, blockDim.x >> 6, blockIdx.x, wave,
                  [&](const unsigned int g, const uint64_t chunk_ray) {
                      uint64_t at;
                      const bool present = batches::sample_of(first_ray, count, chunk_ray, lane, at);
                      int cell = -1;                   // outside, as in the lanes that hold no sample
                      double v = 0.0;
                      if (present) cell = sample(at, v);
                      const unsigned int slab = PRIVATE ? 0u : g*static_cast<unsigned int> (cells);
                      const deposit::contribution a = deposit::contribution_of(cell >= 0, slab + static_cast<unsigned int> (cell), v);
                      deposit::count(tally, present, a);
                      sums.add(state, a);
                  },
                  [&](const unsigned int g) {
                      sums.drain(state + static_cast<size_t> (g)*static_cast<size_t> (cells)*superacc::limbs);
                  });
    deposit::flush(tally, counters);
}

//  deposit_batched for samples that deposit K values each, all of them or none (moment_bins.hip: a particle and its four
//  moments).  The cells are `groups` x K, cell group*K + k; the walk, the slabs and the drains are deposit_batched's.
//  sample(at, v, finite): the group of sample `at`, or -1, its K values, and whether all of them are finite.  The
//  sample is counted once, then the whole wave makes K adds.  counters: samples, outside, skipped, per sample.
template<bool PRIVATE, int K, typename SAMPLE>
__device__ __forceinline__ void deposit_batched_many(const workgroup_sums<PRIVATE> &sums, const unsigned long long first_ray,
                                                     const unsigned long long count, const unsigned int batch_count,
                                                     const int groups, unsigned long long *__restrict__ state,
                                                     unsigned long long *__restrict__ counters, SAMPLE sample) {
    deposit::tallies tally;
    const unsigned int lane = threadIdx.x & 63u;
    const unsigned int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t slab_words = static_cast<size_t> (groups)*K*superacc::limbs;
    batches::walk(first_ray, count, batch_count, gridDim.x, blockDim.x >> 6, blockIdx.x, wave,
                  [&](const unsigned int g, const uint64_t chunk_ray) {
                      uint64_t at;
                      const bool present = batches::sample_of(first_ray, count, chunk_ray, lane, at);
                      int group = -1;                  // outside, as in the lanes that hold no sample
                      double v[K];
#pragma unroll
                      for (int k = 0; k < K; k++) v[k] = 0.0;
                      bool finite = true;
                      if (present) group = sample(at, v, finite);
//  Decided once per sample: inside, and all K finite or none deposited.
                      const deposit::contribution whole = {group >= 0, finite, 0u, 0, 0, 0};
                      deposit::count(tally, present, whole);
                      const bool deposits = whole.inside && whole.finite;
                      const unsigned int slab = PRIVATE ? 0u : g*static_cast<unsigned int> (groups);
                      const unsigned int first = (slab + static_cast<unsigned int> (group))*K;
#pragma unroll
                      for (int k = 0; k < K; k++) sums.add(state, deposit::contribution_of(deposits, first + k, v[k]));
                  },
                  [&](const unsigned int g) {
                      sums.drain(state + static_cast<size_t> (g)*slab_words);
                  });
    deposit::flush(tally, counters);
}

//  A particle's columns as the push holds them, all of T; weight: null when every particle has weight 1.0.
template<typename T>
struct particle_columns {
    const T *x, *y, *z, *ux, *uy, *uz, *gamma, *weight;

    __device__ __forceinline__ double weight_of(const unsigned long long at) const {
        return weight ? static_cast<double> (weight[at]) : 1.0;
    }
};

//  Those of a launch that begins at particle `first` of the caller's eight (the eighth null without weights).
template<typename T>
particle_columns<T> columns_from(const void *const *columns, const size_t first, const bool with_weight) {
    const T *const *typed = reinterpret_cast<const T *const *> (columns);
    return {typed[0] + first, typed[1] + first, typed[2] + first, typed[3] + first, typed[4] + first, typed[5] + first,
            typed[6] + first, with_weight ? typed[7] + first : nullptr};
}

//  The workgroups of a launch of `count` samples.
inline unsigned int grid_of(const size_t count, const unsigned int block, const size_t max_workgroups) {
    const size_t want = (count + block - 1)/block;
    return static_cast<unsigned int> (want < max_workgroups ? want : max_workgroups);
}

//  Those of a batched launch: with more than one per batch, a whole number per batch (ray_batches.hpp).
inline unsigned int batched_grid_of(const size_t count, const unsigned int block, const size_t max_workgroups, const size_t batch_count) {
    return batches::whole_teams(grid_of(count, block, max_workgroups), static_cast<unsigned int> (batch_count));
}

//  A deposit launch on the route the shape was decided for: the kernel's <true> or its <false>.
template<typename... PARAMETERS, typename... ARGUMENTS>
void launch_on_route(void (*private_kernel)(PARAMETERS...), void (*global_kernel)(PARAMETERS...), const launch_shape &shape,
                     const unsigned int grid, hipStream_t stream, ARGUMENTS... arguments) {
    hipLaunchKernelGGL(shape.is_private ? private_kernel : global_kernel, dim3(grid), dim3(shape.block), shape.lds_bytes,
                       stream, arguments...);
}

//  with(float()) or with(double()): the particles' type, chosen once per launch.
template<typename WITH>
void with_particle_type(const bool is_f32, WITH with) {
    if (is_f32) {
        with(float());
    } else {
        with(double());
    }
}

//  Dynamic LDS above 64 KiB has to be asked for.  The setting belongs to the function on the current device, not to an
//  object: always the cap's size (`bytes`), so that no object lowers what another one needs.
inline hipError_t prepare_private(const std::initializer_list<const void *> kernels, const size_t bytes) {
    for (const void *kernel : kernels) {
        const hipError_t status = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int> (bytes));
        if (status != hipSuccess) return status;
    }
    return hipSuccess;
}

}  // namespace sums
}  // namespace gfhip

#endif
