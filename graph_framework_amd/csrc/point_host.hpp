//------------------------------------------------------------------------------
///  @file point_host.hpp
///  @brief A point of the map on the CPU from the caller's tables: flux_sums.hpp's label_at and point_at on the 16
///  coefficient tables and the four fpol tables as the caller holds them ([k][table cell], [k][interval]).
///
///  Only calls of flux_label.hpp's functions, in the kernels' order: nothing is computed here.  Plain C++, no device, no
///  library: the host entry points and the drivers under tests/ share it.
//------------------------------------------------------------------------------
#ifndef GFHIP_POINT_HOST_HPP
#define GFHIP_POINT_HOST_HPP

#include <stddef.h>

#include <limits>

#include "flux_label.hpp"

namespace gfhip {
namespace flux {

//  The caller's tables: coefficients [16][table], fpol [4][intervals] (null where only the label is asked for).
struct host_tables {
    const double *coefficients;
    size_t table;
    const double *fpol[4];
};

//  psi, its derivatives along R and z, the canonical label and fpol of a point inside the map.
struct host_point_values {
    double psi, gr, gz, label, fpol;
};

//  The table cell of (x, y, z) with its 16 coefficients and the normalised coordinates, or -1 outside the map.
inline long long host_coefficients(const map &m, const host_tables &t, const double x, const double y, const double z,
                                   double &tr, double &tz, double *c) {
    const long long at = locate(m, x, y, z, tr, tz);
    if (at < 0) return at;
    for (size_t k = 0; k < 16; k++) c[k] = t.coefficients[k*t.table + static_cast<size_t> (at)];
    return at;
}

//  The label of one point as label_at forms it (not canonical), the quiet NaN outside the map.
inline double host_label(const map &m, const host_tables &t, const double x, const double y, const double z) {
    double tr, tz, c[16];
    if (host_coefficients(m, t, x, y, z, tr, tz, c) < 0) return std::numeric_limits<double>::quiet_NaN();
    return label_of(m, psi_of(c, tr, tz));
}

//  The values of (x, y, z), or false outside the map (`p` is then left alone).
inline bool host_point(const map &m, const field &f, const host_tables &t, const double x, const double y, const double z,
                       host_point_values &p) {
    double tr, tz, tp, c[16], cubic[4];
    if (host_coefficients(m, t, x, y, z, tr, tz, c) < 0) return false;
    p.psi = psi_gradient(m, c, tr, tz, p.gr, p.gz);
    const int q = fpol_interval(f, p.psi, tp);
    for (size_t k = 0; k < 4; k++) cubic[k] = t.fpol[k][q];
    p.fpol = fpol_of(cubic, tp);
    p.label = canonical(label_of(m, p.psi));
    return true;
}

}  // namespace flux
}  // namespace gfhip

#endif
