//------------------------------------------------------------------------------
///  @file source_host.hpp
///  @brief The particle source of particle_source.hip on the CPU, particle by particle (gfhip_source_fill_host).
///
///  The same lines as the kernel's on the caller's arrays: the rule of particle_draw.hpp on the 16 coefficient tables and
///  the four fpol tables as the caller holds them ([k][table cell], [k][interval]), the profile's cell by
///  cell_deposit.hpp's rule.  Plain C++, no device, no library: tests/particle_source_check.cpp builds it under the
///  sanitizers.
//------------------------------------------------------------------------------
#ifndef GFHIP_SOURCE_HOST_HPP
#define GFHIP_SOURCE_HOST_HPP

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "flux_label.hpp"
#include "particle_draw.hpp"

namespace gfhip {
namespace draw {

//  The caller's tables: coefficients [16][table], fpol [4][intervals]; the profile's ns + 1 edges and ns probabilities
//  (both null without one).
struct host_tables {
    const double *packed;
    size_t table;
    const double *fpol[4];
    const double *sedges, *accept;
    size_t ns;

    void coefficients(const long long at, double *c) const {
        for (size_t k = 0; k < 16; k++) c[k] = packed[k*table + static_cast<size_t> (at)];
    }
    void cubic(const int q, double *c) const {
        for (size_t k = 0; k < 4; k++) c[k] = fpol[k][q];
    }
    double accept_of(const double label) const {
        if (!(label >= sedges[0] && label < sedges[ns])) return -1.0;
        return accept[(std::upper_bound(sedges, sedges + ns + 1, label) - sedges) - 1];
    }
};

//  Particles first_particle .. first_particle + count into element 0 .. count of the seven columns of T and of `placed`
//  (null: none).  counters: placed, unplaced, position_tries, gyro_tries, added to.
template<typename T>
void fill_host(const flux::map &m, const flux::field &f, const parameters &par, const host_tables &tables, void *const *columns,
               void *placed, const uint64_t first_particle, const size_t count, uint64_t *counters) {
    T *const *out = reinterpret_cast<T *const *> (columns);
    for (size_t s = 0; s < count; s++) {
        double values[6];
        uint32_t tries[2];
        const bool is_placed = particle<T> (m, f, par, tables, first_particle + s, values, tries);
        store<T> (out, static_cast<T *> (placed), s, is_placed, values);
        counters[is_placed ? 0 : 1]++;
        counters[2] += tries[0];
        counters[3] += tries[1];
    }
}

}  // namespace draw
}  // namespace gfhip

#endif
