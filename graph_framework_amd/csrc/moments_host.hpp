//------------------------------------------------------------------------------
///  @file moments_host.hpp
///  @brief The moment deposit of moment_bins.hip on the CPU, particle by particle (gfhip_moments_values_host,
///  gfhip_moments_add_host, and per batch of particles gfhip_moments_add_particles_host).
///
///  The same lines as the kernel's on the caller's arrays: the label and the four moments from flux_label.hpp on the 16
///  coefficient tables and the four fpol tables as the caller holds them ([k][table cell], [k][interval]), the surface by
///  cell_deposit.hpp's rule, the deposit by superacc.hpp.  Plain C++, no device, no library: tests/moments_host_check.cpp
///  builds it under the sanitizers.
//------------------------------------------------------------------------------
#ifndef GFHIP_MOMENTS_HOST_HPP
#define GFHIP_MOMENTS_HOST_HPP

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <limits>

#include "flux_label.hpp"
#include "point_host.hpp"
#include "ray_batches.hpp"
#include "superacc.hpp"

namespace gfhip {
namespace moments {

constexpr size_t count = 4;                            // density, current, energy, radiation

//  The caller's tables: coefficients [16][table], fpol [4][intervals] (point_host.hpp).
using host_tables = flux::host_tables;

//  The surface of `label` among the ns + 1 increasing edges, edge[i] <= label < edge[i+1], or -1: outside or NaN.
inline long long host_cell(const double *edges, const size_t ns, const double label) {
    if (!(label >= edges[0] && label < edges[ns])) return -1;
    return static_cast<long long> (std::upper_bound(edges, edges + ns + 1, label) - edges) - 1;
}

//  The label and the four moments of one particle, all the quiet NaN off the map.
inline double host_point(const flux::map &m, const flux::field &f, const host_tables &t, const double x, const double y,
                         const double z, const double ux, const double uy, const double uz, const double gamma, double *values) {
    flux::host_point_values p;
    if (!flux::host_point(m, f, t, x, y, z, p)) {
        for (size_t k = 0; k < count; k++) values[k] = std::numeric_limits<double>::quiet_NaN();
        return std::numeric_limits<double>::quiet_NaN();
    }
    flux::moments_of(x, y, flux::radius_of(x, y), ux, uy, uz, gamma, p.gr, p.gz, p.fpol, values);
    return p.label;
}

//  label[s] and values[s*4 + k] of `particles` particles.  columns: x, y, z, ux, uy, uz, gamma, all of T.
template<typename T>
void values_host(const flux::map &m, const flux::field &f, const host_tables &t, const void *const *columns,
                 const size_t particles, double *label, double *values) {
    const T *const *in = reinterpret_cast<const T *const *> (columns);
    for (size_t s = 0; s < particles; s++) {
        label[s] = host_point(m, f, t, static_cast<double> (in[0][s]), static_cast<double> (in[1][s]),
                              static_cast<double> (in[2][s]), static_cast<double> (in[3][s]), static_cast<double> (in[4][s]),
                              static_cast<double> (in[5][s]), static_cast<double> (in[6][s]), values + s*count);
    }
}

//  The deposit of `particles` particles.  columns: the seven and the weight or null, all of T.  limbs: ns*4 cells of 67,
//  canonical on return; counters: samples, outside, skipped, per particle.
template<typename T>
void add_host(const flux::map &m, const flux::field &f, const host_tables &t, const double *sedges, const size_t ns,
              const void *const *columns, const size_t particles, int64_t *limbs, uint64_t *counters) {
    const T *const *in = reinterpret_cast<const T *const *> (columns);
    const size_t cells = ns*count;
    const auto normalise_all = [&]() {
        for (size_t cell = 0; cell < cells; cell++) superacc::normalise(limbs + cell*superacc::limbs);
    };
    uint64_t pending = 0, outside = 0, skipped = 0;
    for (size_t s = 0; s < particles; s++) {
        double moments[count], v[count];
        const double label = host_point(m, f, t, static_cast<double> (in[0][s]), static_cast<double> (in[1][s]),
                                        static_cast<double> (in[2][s]), static_cast<double> (in[3][s]),
                                        static_cast<double> (in[4][s]), static_cast<double> (in[5][s]),
                                        static_cast<double> (in[6][s]), moments);
        const long long is = host_cell(sedges, ns, label);
        if (is < 0) {
            outside++;
            continue;
        }
        flux::weighted_moments(in[7] ? static_cast<double> (in[7][s]) : 1.0, moments, v);
        if (!flux::moments_finite(v)) {                // all four or none
            skipped++;
            continue;
        }
        if (++pending > superacc::deposits_per_normalise) {    // a cell takes at most one deposit per particle
            normalise_all();
            pending = 1;
        }
        for (size_t k = 0; k < count; k++) superacc::deposit(limbs + (static_cast<size_t> (is)*count + k)*superacc::limbs, v[k]);
    }
    if (pending) normalise_all();
    counters[0] += particles;
    counters[1] += outside;
    counters[2] += skipped;
}

//  add_host per batch of particles (ray_batches.hpp's rule, a particle's index in the ensemble in place of a ray's):
//  particle s of the columns is particle first_particle + s.  limbs: [batch][ns*4 cells][67], slab g what add_host makes
//  of batch g's particles alone; counters: samples, outside, skipped of all of them, per particle.
template<typename T>
void add_particles_host(const flux::map &m, const flux::field &f, const host_tables &t, const double *sedges, const size_t ns,
                        const unsigned int batch_count, const uint64_t first_particle, const void *const *columns,
                        const size_t particles, int64_t *limbs, uint64_t *counters) {
    const T *const *in = reinterpret_cast<const T *const *> (columns);
    const size_t cells = ns*count;
    const auto normalise_all = [&]() {
        for (size_t cell = 0; cell < batch_count*cells; cell++) superacc::normalise(limbs + cell*superacc::limbs);
    };
    uint64_t pending = 0, outside = 0, skipped = 0;
    for (size_t s = 0; s < particles; s++) {
        double moments[count], v[count];
        const double label = host_point(m, f, t, static_cast<double> (in[0][s]), static_cast<double> (in[1][s]),
                                        static_cast<double> (in[2][s]), static_cast<double> (in[3][s]),
                                        static_cast<double> (in[4][s]), static_cast<double> (in[5][s]),
                                        static_cast<double> (in[6][s]), moments);
        const long long is = host_cell(sedges, ns, label);
        if (is < 0) {
            outside++;
            continue;
        }
        flux::weighted_moments(in[7] ? static_cast<double> (in[7][s]) : 1.0, moments, v);
        if (!flux::moments_finite(v)) {                // all four or none
            skipped++;
            continue;
        }
        if (++pending > superacc::deposits_per_normalise) {    // a cell takes at most one deposit per particle
            normalise_all();
            pending = 1;
        }
        int64_t *slab = limbs + batches::batch_of(first_particle + s, batch_count)*cells*superacc::limbs;
        for (size_t k = 0; k < count; k++) superacc::deposit(slab + (static_cast<size_t> (is)*count + k)*superacc::limbs, v[k]);
    }
    if (pending) normalise_all();
    counters[0] += particles;
    counters[1] += outside;
    counters[2] += skipped;
}

}  // namespace moments
}  // namespace gfhip

#endif
