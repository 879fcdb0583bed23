//------------------------------------------------------------------------------
///  @file confinement_host.hpp
///  @brief The first-exit check of confinement.hip on the CPU, particle by particle (gfhip_confine_check_host).
///
///  The same lines as the kernel's on the caller's arrays: the label from flux_label.hpp on the 16 coefficient tables as
///  the caller holds them ([k][table cell]), the cell by cell_deposit.hpp's rule, the deposit by superacc.hpp.  Plain
///  C++, no device, no library: tests/confinement_host_check.cpp builds it under the sanitizers.
//------------------------------------------------------------------------------
#ifndef GFHIP_CONFINEMENT_HOST_HPP
#define GFHIP_CONFINEMENT_HOST_HPP

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <limits>

#include "flux_label.hpp"
#include "superacc.hpp"

namespace gfhip {
namespace confine {

constexpr uint32_t confined = 0xffffffffu;             // lost_step of a particle that has not left

//  The cell of `v` among the n + 1 increasing edges of an axis, edge[i] <= v < edge[i+1], or -1: outside or NaN.
inline long long host_cell(const double *edges, const size_t n, const double v) {
    if (!(v >= edges[0] && v < edges[n])) return -1;
    return static_cast<long long> (std::upper_bound(edges, edges + n + 1, v) - edges) - 1;
}

//  The label of (x, y, z), a NaN as the quiet NaN; NaN off the map.  coefficients: [k][table cell], `table` cells.
inline double host_label(const flux::map &m, const double *coefficients, const size_t table, const double x, const double y,
                         const double z) {
    double tr, tz, c[16];
    const long long at = flux::locate(m, x, y, z, tr, tz);
    if (at < 0) return std::numeric_limits<double>::quiet_NaN();
    for (size_t k = 0; k < 16; k++) c[k] = coefficients[k*table + static_cast<size_t> (at)];
    return flux::canonical(flux::label_of(m, flux::psi_of(c, tr, tz)));
}

//  One check of `count` particles at step number `step`.  columns: x, y, z, (three unread), gamma, the weight or null,
//  all of T.  exit_r and exit_z: both null, or both arrays.  limbs: null (then axes, n and counters are not looked at),
//  or n[0]*n[1]*n[2] cells of 67, canonical on return; counters: samples, outside, skipped.
template<typename T>
void check_host(const flux::map &m, const double *coefficients, const size_t table, const double limit, const double *const *axes,
                const size_t *n, const void *const *columns, const size_t count, const uint32_t step, uint32_t *lost_step,
                T *alive, double *exit_r, double *exit_z, uint64_t *newly_lost, int64_t *limbs, uint64_t *counters) {
    const T *const *in = reinterpret_cast<const T *const *> (columns);
    const size_t cells = limbs ? n[0]*n[1]*n[2] : 0;
    const auto normalise_all = [&]() {
        for (size_t cell = 0; cell < cells; cell++) superacc::normalise(limbs + cell*superacc::limbs);
    };
    uint64_t pending = 0, lost = 0, outside = 0, skipped = 0;
    for (size_t s = 0; s < count; s++) {
        if (lost_step[s] != confined) continue;        // settled: never looked at again
        const double x = static_cast<double> (in[0][s]), y = static_cast<double> (in[1][s]), z = static_cast<double> (in[2][s]);
        const double label = host_label(m, coefficients, table, x, y, z);
        if (label < limit) continue;
        lost++;
        const double v = in[7] ? static_cast<double> (in[7][s]) : 1.0;
        const double r = flux::radius_of(x, y);
        lost_step[s] = step;
        alive[s] = static_cast<T> (0);
        if (exit_r) {
            exit_r[s] = flux::canonical(r);
            exit_z[s] = flux::canonical(z);
        }
        if (!limbs) continue;
        const long long ir = host_cell(axes[0], n[0], r), iz = host_cell(axes[1], n[1], z),
                        ig = host_cell(axes[2], n[2], static_cast<double> (in[6][s]));
        if (ir < 0 || iz < 0 || ig < 0) {
            outside++;
            continue;
        }
        if (!superacc::is_finite(v)) {
            skipped++;
            continue;
        }
        if (++pending > superacc::deposits_per_normalise) {
            normalise_all();
            pending = 1;
        }
        const size_t cell = (static_cast<size_t> (ir)*n[1] + static_cast<size_t> (iz))*n[2] + static_cast<size_t> (ig);
        superacc::deposit(limbs + cell*superacc::limbs, v);
    }
    if (pending) normalise_all();
    *newly_lost += lost;
    if (limbs) {
        counters[0] += lost;
        counters[1] += outside;
        counters[2] += skipped;
    }
}

}  // namespace confine
}  // namespace gfhip

#endif
