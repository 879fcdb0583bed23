//------------------------------------------------------------------------------
///  @file phase_host.hpp
///  @brief The batched deposit of phase_bins.hip on the CPU, particle by particle (gfhip_phase_add_particles_host).
///
///  The same lines as the kernel's on the caller's arrays: the label and xi from flux_label.hpp on the 16 coefficient
///  tables and the four fpol tables as the caller holds them (moments_host.hpp's host_tables), the three cells by
///  cell_deposit.hpp's rule, the batch by ray_batches.hpp's, the deposit by superacc.hpp.  Plain C++, no device, no
///  library: tests/particle_batches_check.cpp builds it under the sanitizers.
//------------------------------------------------------------------------------
#ifndef GFHIP_PHASE_HOST_HPP
#define GFHIP_PHASE_HOST_HPP

#include <stddef.h>
#include <stdint.h>

#include <limits>

#include "flux_label.hpp"
#include "moments_host.hpp"
#include "ray_batches.hpp"
#include "superacc.hpp"

namespace gfhip {
namespace phase {

//  The label and the pitch cosine of one particle, both the quiet NaN off the map.
inline void host_point(const flux::map &m, const flux::field &f, const moments::host_tables &t, const double x, const double y,
                       const double z, const double ux, const double uy, const double uz, double &label, double &pitch) {
    flux::host_point_values p;
    if (!flux::host_point(m, f, t, x, y, z, p)) {
        label = pitch = std::numeric_limits<double>::quiet_NaN();
        return;
    }
    label = p.label;
    pitch = flux::pitch_of(x, y, flux::radius_of(x, y), ux, uy, uz, p.gr, p.gz, p.fpol);
}

//  The deposit of `particles` particles, particle s of the columns being particle first_particle + s of the ensemble.
//  columns: the seven and the weight or null, all of T.  edges: the n[a] + 1 of the label, of xi and of gamma.  limbs:
//  [batch][n[0]*n[1]*n[2] cells][67], canonical on return, slab g the sums of batch g's particles; counters: samples,
//  outside, skipped of all of them.
template<typename T>
void add_particles_host(const flux::map &m, const flux::field &f, const moments::host_tables &t, const double *const *edges,
                        const size_t *n, const unsigned int batch_count, const uint64_t first_particle,
                        const void *const *columns, const size_t particles, int64_t *limbs, uint64_t *counters) {
    const T *const *in = reinterpret_cast<const T *const *> (columns);
    const size_t cells = n[0]*n[1]*n[2];
    const auto normalise_all = [&]() {
        for (size_t cell = 0; cell < batch_count*cells; cell++) superacc::normalise(limbs + cell*superacc::limbs);
    };
    uint64_t pending = 0, outside = 0, skipped = 0;
    for (size_t s = 0; s < particles; s++) {
        double label, xi;
        host_point(m, f, t, static_cast<double> (in[0][s]), static_cast<double> (in[1][s]), static_cast<double> (in[2][s]),
                   static_cast<double> (in[3][s]), static_cast<double> (in[4][s]), static_cast<double> (in[5][s]), label, xi);
        const long long is = moments::host_cell(edges[0], n[0], label);
        const long long ip = moments::host_cell(edges[1], n[1], xi);
        const long long ig = moments::host_cell(edges[2], n[2], static_cast<double> (in[6][s]));
        if (is < 0 || ip < 0 || ig < 0) {
            outside++;
            continue;
        }
        const double w = in[7] ? static_cast<double> (in[7][s]) : 1.0;
        if (!superacc::is_finite(w)) {
            skipped++;
            continue;
        }
        if (++pending > superacc::deposits_per_normalise) {    // a cell takes at most one deposit per particle
            normalise_all();
            pending = 1;
        }
        const size_t cell = (static_cast<size_t> (is)*n[1] + static_cast<size_t> (ip))*n[2] + static_cast<size_t> (ig);
        superacc::deposit(limbs + (batches::batch_of(first_particle + s, batch_count)*cells + cell)*superacc::limbs, w);
    }
    if (pending) normalise_all();
    counters[0] += particles;
    counters[1] += outside;
    counters[2] += skipped;
}

}  // namespace phase
}  // namespace gfhip

#endif
