//------------------------------------------------------------------------------
///  @file particle_source.hip
///  @brief The particle source: the seven columns of a push filled where they lie on the device (hand-written, gfx950).
///
///  Particle first_particle + i of the ensemble goes to element i of the columns by the rule of particle_draw.hpp, from
///  the [cell][16] psi pack and the [q][4] fpol pack the other kernels read; a profile's ns + 1 edges and ns
///  probabilities are staged in LDS.  What a particle becomes depends on its index alone, so the bytes are the same for
///  any launch shape, and for both routes:
///
///  plain   One lane, one particle, its own loops; a workgroup walks tiles of blockDim.x particles grid-stride.  A wave
///          stays in the position loop (16 coefficient loads and about 60 fp64 operations per attempt) until its slowest
///          lane is done.
///  refill  A wave owns tiles of 64 consecutive particles, grid-stride.  In every trip each lane evaluates one attempt
///          (p, a) of the position loop; a lane whose particle is settled (its position stored, or out of attempts) takes
///          the wave's next unstarted particle by a ballot and a lane-prefix count, from the next tile when this one is
///          used up, until the wave's tiles are exhausted.  Positions go to index p - first_particle, scattered within
///          the tile.  The momentum, one field evaluation per placed particle and the same work in every lane, is a
///          second launch over the stored positions (x is NaN where the first found no position), which repeats the
///          toroidal draw.
///
///  counters: placed, unplaced, position_tries, gyro_tries; every lane keeps its own, a wave adds its sums with one
///  integer atomic each.  No scratch.
//------------------------------------------------------------------------------
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cell_deposit.hpp"
#include "cell_launch.hpp"
#include "flux_label.hpp"
#include "flux_sums.hpp"
#include "particle_draw.hpp"

namespace gfhip {

using namespace sums;

namespace {

//  The packs in global memory and the profile in LDS.
struct device_tables {
    const double *__restrict__ packed, *__restrict__ fpol;
    const double *sedge, *accept;                      // LDS
    int ns;
    double scale;

    __device__ __forceinline__ void coefficients(const long long at, double *c) const {
        coefficients_at(packed, at, c);
    }
    __device__ __forceinline__ void cubic(const int q, double *c) const {
        const double2 *line = reinterpret_cast<const double2 *> (fpol) + static_cast<size_t> (q)*2;
        const double2 low = line[0], high = line[1];
        c[0] = low.x;
        c[1] = low.y;
        c[2] = high.x;
        c[3] = high.y;
    }
    __device__ __forceinline__ double accept_of(const double label) const {
        const int is = deposit::find_cell(sedge, ns, scale, label);
        return is >= 0 ? accept[is] : -1.0;
    }
};

//  profile: the ns + 1 edges, then the ns probabilities (global memory; unread when ns = 0), copied to `lds`.
__device__ __forceinline__ device_tables stage(double *lds, const double *__restrict__ packed, const double *__restrict__ fpol,
                                               const double *__restrict__ profile, const int ns, const double scale) {
    if (ns > 0) {
        for (int k = threadIdx.x; k < 2*ns + 1; k += blockDim.x) lds[k] = profile[k];
    }
    __syncthreads();
    return device_tables{packed, fpol, lds, lds + ns + 1, ns, scale};
}

struct tallies {
    unsigned long long placed = 0, unplaced = 0, position_tries = 0, gyro_tries = 0;
};

//  Executed by whole waves.
__device__ __forceinline__ void flush(const tallies &t, unsigned long long *__restrict__ counters) {
    const unsigned long long sum[4] = {static_cast<unsigned long long> (deposit::wave_sum(static_cast<long long> (t.placed))),
                                       static_cast<unsigned long long> (deposit::wave_sum(static_cast<long long> (t.unplaced))),
                                       static_cast<unsigned long long> (deposit::wave_sum(static_cast<long long> (t.position_tries))),
                                       static_cast<unsigned long long> (deposit::wave_sum(static_cast<long long> (t.gyro_tries)))};
    if ((threadIdx.x & 63u) == 0) {
        for (int k = 0; k < 4; k++) {
            if (sum[k]) atomicAdd(counters + k, sum[k]);
        }
    }
}

}  // namespace

template<typename T>
struct source_columns {
    T *column[7];                                      // x, y, z, ux, uy, uz, gamma
    T *placed;                                         // null: none
};

//  The plain route.
template<typename T>
__global__ void __launch_bounds__(global_block)
source_plain_kernel(const source_columns<T> out, const unsigned long long count, const unsigned long long first_particle,
                    const flux::map m, const flux::field f, const draw::parameters par, const double *__restrict__ packed,
                    const double *__restrict__ fpol, const double *__restrict__ profile, const double scale,
                    unsigned long long *__restrict__ counters) {
    extern __shared__ double staged[];
    const device_tables tables = stage(staged, packed, fpol, profile, par.ns, scale);
    tallies tally;
    const unsigned long long stride = static_cast<unsigned long long> (gridDim.x)*blockDim.x;
    for (unsigned long long base = static_cast<unsigned long long> (blockIdx.x)*blockDim.x; base < count; base += stride) {
        const unsigned long long at = base + threadIdx.x;
        if (at < count) {
            double values[6];
            uint32_t tries[2];
            const bool is_placed = draw::particle<T> (m, f, par, tables, first_particle + at, values, tries);
            draw::store<T> (out.column, out.placed, at, is_placed, values);
            tally.placed += is_placed ? 1u : 0u;
            tally.unplaced += is_placed ? 0u : 1u;
            tally.position_tries += tries[0];
            tally.gyro_tries += tries[1];
        }
    }
    flush(tally, counters);
}

//  The refill route's first launch: x, y, z of the particles that found a position, NaN into x of those that did not;
//  counters[2].  blockDim.x is a multiple of 64.
template<typename T>
__global__ void __launch_bounds__(global_block)
source_position_kernel(T *__restrict__ x, T *__restrict__ y, T *__restrict__ z, const unsigned long long count,
                       const unsigned long long first_particle, const flux::map m, const draw::parameters par,
                       const double *__restrict__ packed, const double *__restrict__ profile, const double scale,
                       unsigned long long *__restrict__ counters) {
    extern __shared__ double staged[];
    const device_tables tables = stage(staged, packed, nullptr, profile, par.ns, scale);
    const unsigned int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned long long stride = static_cast<unsigned long long> (gridDim.x)*blockDim.x;
//  Wave-uniform: the wave's current tile and how many of its 64 particles have been started.
    unsigned long long tile = static_cast<unsigned long long> (blockIdx.x)*blockDim.x + wave*64u;
    unsigned int started = 0;
//  The lane's particle: its index in the columns, the next attempt and its toroidal direction.
    bool active = false;
    unsigned long long at = 0;
    uint32_t a = 0;
    draw::direction phi = {0.0, 0.0};
    unsigned long long position_tries = 0;
    for (;;) {
        unsigned long long idle = __ballot(!active);
        while (idle != 0 && tile < count) {            // wave-uniform
            const unsigned long long left = count - tile - started;        // > 0
            const unsigned int room = 64u - started;
            const unsigned int available = left < room ? static_cast<unsigned int> (left) : room;
            const unsigned int rank = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned int> (idle >> 32),
                                                                __builtin_amdgcn_mbcnt_lo(static_cast<unsigned int> (idle), 0u));
            if (!active && rank < available) {
                at = tile + started + rank;                                 // < count
                a = 0;
                uint32_t used;
                active = draw::circle_loop(par, first_particle + at, draw::purpose_toroidal, phi, used);
                if (!active) x[at] = static_cast<T> (__builtin_nanf(""));  // unplaced by loop 1: settled at once
            }
            const unsigned int wanted = static_cast<unsigned int> (__popcll(idle));
            started += wanted < available ? wanted : available;
            if (started == 64u || tile + started >= count) {
                tile += stride;
                started = 0;
            }
            idle = __ballot(!active);
        }
        if (__ballot(active) == 0) break;              // nothing in flight and, after the loop above, nothing left to take
        if (active) {
            double xyz[3];
            const bool found = draw::position_attempt<T> (m, par, tables, first_particle + at, a, phi, xyz);
            a++;
            if (found || a == par.attempts) {
                position_tries += a;
                if (found) {
                    x[at] = static_cast<T> (xyz[0]);
                    y[at] = static_cast<T> (xyz[1]);
                    z[at] = static_cast<T> (xyz[2]);
                } else {
                    x[at] = static_cast<T> (__builtin_nanf(""));
                }
                active = false;
            }
        }
    }
    const unsigned long long sum = static_cast<unsigned long long> (deposit::wave_sum(static_cast<long long> (position_tries)));
    if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(counters + 2, sum);
}

//  The refill route's second launch, one lane per particle: steps 3 to 6 from the stored position; counters[0], [1], [3].
template<typename T>
__global__ void __launch_bounds__(global_block)
source_momentum_kernel(const source_columns<T> out, const unsigned long long count, const unsigned long long first_particle,
                       const flux::map m, const flux::field f, const draw::parameters par, const double *__restrict__ packed,
                       const double *__restrict__ fpol, unsigned long long *__restrict__ counters) {
    const device_tables tables = {packed, fpol, nullptr, nullptr, 0, 0.0};
    tallies tally;
    const unsigned long long stride = static_cast<unsigned long long> (gridDim.x)*blockDim.x;
    for (unsigned long long base = static_cast<unsigned long long> (blockIdx.x)*blockDim.x; base < count; base += stride) {
        const unsigned long long at = base + threadIdx.x;
        if (at < count) {
            double values[6] = {static_cast<double> (out.column[0][at]), 0.0, 0.0, 0.0, 0.0, 0.0};
            bool is_placed = values[0] == values[0];
            if (is_placed) {
                values[1] = static_cast<double> (out.column[1][at]);
                values[2] = static_cast<double> (out.column[2][at]);
                draw::direction phi;
                uint32_t used, gyro_tries = 0;
                is_placed = draw::circle_loop(par, first_particle + at, draw::purpose_toroidal, phi, used) &&
                            draw::momentum_of(m, f, par, tables, first_particle + at, phi, values, values + 3, gyro_tries);
                tally.gyro_tries += gyro_tries;
            }
            draw::store<T> (out.column, out.placed, at, is_placed, values);
            tally.placed += is_placed ? 1u : 0u;
            tally.unplaced += is_placed ? 0u : 1u;
        }
    }
    flush(tally, counters);
}

namespace {

template<typename T>
void fill_as(void *const *columns, void *placed, const size_t count, const unsigned long long first_particle, const flux::map &m,
             const flux::field &f, const draw::parameters &par, const double *packed, const double *fpol, const double *profile,
             const double scale, const bool refill, const size_t max_workgroups, unsigned long long *counters,
             hipStream_t stream) {
    source_columns<T> out;
    for (int k = 0; k < 7; k++) out.column[k] = static_cast<T *> (columns[k]);
    out.placed = static_cast<T *> (placed);
    const dim3 grid(grid_of(count, global_block, max_workgroups)), block(global_block);
    const size_t lds_bytes = par.ns ? (2*static_cast<size_t> (par.ns) + 1)*sizeof(double) : 0;
    const unsigned long long particles = count;
    if (refill) {
        hipLaunchKernelGGL(source_position_kernel<T>, grid, block, lds_bytes, stream, out.column[0], out.column[1], out.column[2],
                           particles, first_particle, m, par, packed, profile, scale, counters);
        hipLaunchKernelGGL(source_momentum_kernel<T>, grid, block, 0, stream, out, particles, first_particle, m, f, par, packed,
                           fpol, counters);
    } else {
        hipLaunchKernelGGL(source_plain_kernel<T>, grid, block, lds_bytes, stream, out, particles, first_particle, m, f, par,
                           packed, fpol, profile, scale, counters);
    }
}

}  // namespace

void launch_particle_source(void *const *columns, void *placed, const bool is_f32, const size_t count,
                            const unsigned long long first_particle, const flux::map &m, const flux::field &f,
                            const draw::parameters &par, const double *packed, const double *fpol, const double *profile,
                            const double scale, const bool refill, const size_t max_workgroups, unsigned long long *counters,
                            hipStream_t stream) {
    if (count == 0) return;
    if (is_f32) {
        fill_as<float> (columns, placed, count, first_particle, m, f, par, packed, fpol, profile, scale, refill, max_workgroups,
                        counters, stream);
    } else {
        fill_as<double> (columns, placed, count, first_particle, m, f, par, packed, fpol, profile, scale, refill, max_workgroups,
                         counters, stream);
    }
}

}  // namespace gfhip
