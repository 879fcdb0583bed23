//------------------------------------------------------------------------------
///  @file flux_label.hpp
///  @brief The flux label of a point (x, y, z) from the EFIT psi spline, host and device.
///
///  The spline is evaluated in the representation the tracer itself uses: in every cell of the (R, Z) table a
///  bicubic polynomial in the GLOBAL normalised coordinates tr = (R - rmin)/dr, tz = (z - zmin)/dz, whose integer
///  parts are also the cell's indices.  The arithmetic is fixed: every operation below is one IEEE fp64 operation,
///  in this order, nothing fused (contraction is switched off here, whatever the translation unit's flags say), so
///  the host, the device and the numpy model of the tests give the same bits:
///
///      R   = sqrt(x*x + y*y)
///      tr  = (R - rmin)/dr          tz = (z - zmin)/dz
///      inside the map  iff  tr >= 0 && tr < numr && tz >= 0 && tz < numz      (a NaN is outside)
///      i = (int)tr, j = (int)tz, c[a][b] = psi_c<a><b>[i][j]
///      col_a = ((c[a][3]*tz + c[a][2])*tz + c[a][1])*tz + c[a][0]             a = 0..3
///      psi   = ((col_3*tr + col_2)*tr + col_1)*tr + col_0
///      s     = (psi - psi0)/span
///      label = s, or sqrt(s) when flag bit 0 is set (s < 0 gives NaN)
///
///  Unlike the tracer's gather the map does not clamp: a point off the table has no label (NaN).  Plain C++.
///
///  The field direction and the parallel refractive index N = c (k.B)/(|B| w) of a sample (x, y, z, kx, ky, kz, w),
///  by the same rules, for flux_spectrum.hip.  B = (psi_z/R, fpol/R, -psi_R/R) in (R, phi, z), the common 1/R dropped;
///  fpol is a cubic in the GLOBAL normalised tp per interval of the psi table, the interval clamped as the tracer's
///  1-D gather clamps it (labels a little above 1 occur inside the map); c[a][b], col_a and psi are those above:
///
///      dcol_a = ((c[a][3]*3.0)*tz + c[a][2]*2.0)*tz + c[a][1]                 a = 0..3
///      psi_tz = ((dcol_3*tr + dcol_2)*tr + dcol_1)*tr + dcol_0
///      psi_tr = ((col_3*3.0)*tr + col_2*2.0)*tr + col_1
///      gR = psi_tr/dr                 gZ = psi_tz/dz
///      tp = (psi - psimin)/dpsi
///      q  = 0 unless tp >= 0 (a NaN gives 0);  numpsi - 1 if tp >= numpsi;  else (int)tp
///      f  = ((fpol_c3[q]*tp + fpol_c2[q])*tp + fpol_c1[q])*tp + fpol_c0[q]
///      a  = kx*x + ky*y               b = ky*x - kx*y
///      num  = (a*gZ + b*f)/R - kz*gR
///      den  = sqrt((gZ*gZ + f*f) + gR*gR)
///      npar = (c*(num/den))/w
///
///  The pitch cosine of a particle (x, y, z, ux, uy, uz), for phase_bins.hip: num and den as above with u in place of k,
///
///      cosine = num/den
///      uu = (ux*ux + uy*uy) + uz*uz
///      p  = sqrt(uu)
///      xi = cosine/p;   if (xi > 1) xi = 1;   if (xi < -1) xi = -1        (comparisons: a NaN, as of u = 0, stays one)
///
///  No integer conversion of a NaN or of a value out of range is reached.  Which NaN an operation gives is not IEEE's
///  business and differs between processors: the label and npar of a sample leave as canonical(), so that the bits are
///  the same everywhere.
//------------------------------------------------------------------------------
#ifndef GFHIP_FLUX_LABEL_HPP
#define GFHIP_FLUX_LABEL_HPP

#include <math.h>
#include <stdint.h>

#include "superacc.hpp"                                // GFHIP_HD

namespace gfhip {
namespace flux {

constexpr uint32_t flag_sqrt_label = 1u;               // label = sqrt(s)
constexpr uint32_t flag_no_private_sums = 2u;          // flux_profile.hip: deposits go to the global state
constexpr uint32_t known_flags = flag_sqrt_label | flag_no_private_sums;

//  The scalars of a map; the coefficients travel separately (16 tables on the host, [cell][16] on the device).
struct map {
    double rmin, dr, zmin, dz;
    double numr, numz;                                 // the table's extents as doubles: what tr and tz are compared with
    unsigned long long columns;                        // numz: cell = i*columns + j
    double psi0, span;
    uint32_t flags;
};

//  R of (x, y).
GFHIP_HD double radius_of(const double x, const double y) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double xx = x*x;
    const double yy = y*y;
    return sqrt(xx + yy);
}

//  The table cell of (x, y, z), i*numz + j, with the normalised coordinates it was found from; -1 outside the map.
GFHIP_HD long long locate(const map &m, const double x, const double y, const double z, double &tr, double &tz) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double r = radius_of(x, y);
    tr = (r - m.rmin)/m.dr;
    tz = (z - m.zmin)/m.dz;
    if (!(tr >= 0.0 && tr < m.numr && tz >= 0.0 && tz < m.numz)) return -1;
    return static_cast<long long> (static_cast<int> (tr))*static_cast<long long> (m.columns) + static_cast<int> (tz);
}

//  col_a from a cell's 16 coefficients, c[a*4 + b].
GFHIP_HD void columns_of(const double *c, const double tz, double *column) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    for (int a = 0; a < 4; a++) {
        double t = c[4*a + 3]*tz;
        t = t + c[4*a + 2];
        t = t*tz;
        t = t + c[4*a + 1];
        t = t*tz;
        column[a] = t + c[4*a];
    }
}

//  psi from the four col_a.
GFHIP_HD double psi_from(const double *column, const double tr) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double p = column[3]*tr;
    p = p + column[2];
    p = p*tr;
    p = p + column[1];
    p = p*tr;
    return p + column[0];
}

//  psi from a cell's 16 coefficients, c[a*4 + b].
GFHIP_HD double psi_of(const double *c, const double tr, const double tz) {
    double column[4];
    columns_of(c, tz, column);
    return psi_from(column, tr);
}

GFHIP_HD double label_of(const map &m, const double psi) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double s = (psi - m.psi0)/m.span;
    return (m.flags & flag_sqrt_label) ? sqrt(s) : s;
}

//  What N needs beside the map; the fpol coefficients travel separately (four tables on the host, [q][4] on the device).
struct field {
    double psimin, dpsi;
    double numpsi;                                     // the table's extent as a double: what tp is compared with
    int last;                                          // numpsi - 1
    double c;
};

//  psi and its derivatives along R and z at a point inside the map, from the cell's 16 coefficients.
GFHIP_HD double psi_gradient(const map &m, const double *c, const double tr, const double tz, double &gr, double &gz) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double column[4], slope[4];
    columns_of(c, tz, column);
    for (int a = 0; a < 4; a++) {
        double t = c[4*a + 3]*3.0;
        t = t*tz;
        const double u = c[4*a + 2]*2.0;
        t = t + u;
        t = t*tz;
        slope[a] = t + c[4*a + 1];
    }
    const double psi_tz = psi_from(slope, tr);
    double t = column[3]*3.0;
    t = t*tr;
    const double u = column[2]*2.0;
    t = t + u;
    t = t*tr;
    const double psi_tr = t + column[1];
    gr = psi_tr/m.dr;
    gz = psi_tz/m.dz;
    return psi_from(column, tr);
}

//  The interval q of the fpol table and the coordinate tp it is evaluated at.
GFHIP_HD int fpol_interval(const field &f, const double psi, double &tp) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    tp = (psi - f.psimin)/f.dpsi;
    if (!(tp >= 0.0)) return 0;
    if (tp >= f.numpsi) return f.last;
    return static_cast<int> (tp);
}

//  fpol from an interval's four coefficients, c0 .. c3.
GFHIP_HD double fpol_of(const double *c, const double tp) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double f = c[3]*tp;
    f = f + c[2];
    f = f*tp;
    f = f + c[1];
    f = f*tp;
    return f + c[0];
}

//  A NaN as the quiet NaN with no payload, 0x7ff8000000000000; every other value as it is.
GFHIP_HD double canonical(const double v) {
    return v == v ? v : __builtin_nan("");
}

//  cosine = num/den of the lines above: (k.B)/|B|, the component of (kx, ky, kz) along the field.
GFHIP_HD double cosine_of(const double x, const double y, const double r, const double kx, const double ky, const double kz,
                          const double gr, const double gz, const double fpol) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double kxx = kx*x;
    const double kyy = ky*y;
    const double a = kxx + kyy;
    const double kyx = ky*x;
    const double kxy = kx*y;
    const double b = kyx - kxy;
    const double agz = a*gz;
    const double bf = b*fpol;
    const double along = (agz + bf)/r;
    const double kzgr = kz*gr;
    const double num = along - kzgr;
    const double gzgz = gz*gz;
    const double ff = fpol*fpol;
    const double grgr = gr*gr;
    const double den = sqrt((gzgz + ff) + grgr);
    return num/den;
}

//  N from the pieces above.
GFHIP_HD double npar_of(const field &f, const double x, const double y, const double r, const double kx, const double ky,
                        const double kz, const double w, const double gr, const double gz, const double fpol) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double cosine = cosine_of(x, y, r, kx, ky, kz, gr, gz, fpol);
    return canonical((f.c*cosine)/w);
}

//  The pitch cosine xi = (u.B)/(|u||B|) of a particle with momentum (ux, uy, uz), for phase_bins.hip.  The quotient of
//  a parallel u comes out a few 1e-16 above 1 in a third of the cases: it is clamped, by comparisons, so that a NaN
//  (u = 0: 0/0) stays one.
GFHIP_HD double pitch_of(const double x, const double y, const double r, const double ux, const double uy, const double uz,
                         const double gr, const double gz, const double fpol) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double cosine = cosine_of(x, y, r, ux, uy, uz, gr, gz, fpol);
    const double uxux = ux*ux;
    const double uyuy = uy*uy;
    const double uzuz = uz*uz;
    const double uu = (uxux + uyuy) + uzuz;
    const double p = sqrt(uu);
    double xi = cosine/p;
    if (xi > 1.0) xi = 1.0;
    if (xi < -1.0) xi = -1.0;
    return canonical(xi);
}

//  The moments of a particle (x, y, z, ux, uy, uz, gamma), for moment_bins.hip: m = {1, v_par/c, gamma - 1, |B|^2 u_perp^2},
//  the particle's share of the density, the parallel current, the kinetic energy (in m c^2) and the synchrotron power (up
//  to constants), in the push's normalised units.  r, gr, gz and fpol as pitch_of takes them; every line one operation:
//
//      upar = cosine                  (u.B)/|B|, the value pitch_of divides by p
//      vpar = upar/gamma              kin = gamma - 1.0
//      uu   = (ux*ux + uy*uy) + uz*uz                 upup = upar*upar
//      perp = uu - upup;   if (perp < 0) perp = 0     (a comparison: a NaN stays one; u along B cancels to a few ulp of uu)
//      bsum = (gz*gz + f*f) + gr*gr                   rr = r*r          bsq = bsum/rr          (|B|^2)
//      rad  = perp*bsq
//
//  u = 0 gives upar = 0 and rad = 0; gamma = 0 gives vpar = 0/0.  The four leave as canonical().
GFHIP_HD void moments_of(const double x, const double y, const double r, const double ux, const double uy, const double uz,
                         const double gamma, const double gr, const double gz, const double fpol, double *m) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double upar = cosine_of(x, y, r, ux, uy, uz, gr, gz, fpol);
    const double vpar = upar/gamma;
    const double kin = gamma - 1.0;
    const double uxux = ux*ux;
    const double uyuy = uy*uy;
    const double uzuz = uz*uz;
    const double uu = (uxux + uyuy) + uzuz;
    const double upup = upar*upar;
    double perp = uu - upup;
    if (perp < 0.0) perp = 0.0;
    const double gzgz = gz*gz;
    const double ff = fpol*fpol;
    const double grgr = gr*gr;
    const double bsum = (gzgz + ff) + grgr;
    const double rr = r*r;
    const double bsq = bsum/rr;
    const double rad = perp*bsq;
    m[0] = 1.0;
    m[1] = canonical(vpar);
    m[2] = canonical(kin);
    m[3] = canonical(rad);
}

//  What a particle of weight w deposits: v[0] = w, v[k] = w*m[k].
GFHIP_HD void weighted_moments(const double w, const double *m, double *v) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    v[0] = w;
    v[1] = w*m[1];
    v[2] = w*m[2];
    v[3] = w*m[3];
}

//  Whether a particle deposits at all: all four values finite, so that the four moments are sums over the same particles.
GFHIP_HD bool moments_finite(const double *v) {
    return superacc::is_finite(v[0]) && superacc::is_finite(v[1]) && superacc::is_finite(v[2]) && superacc::is_finite(v[3]);
}

//  The quadrature of the flux volumes (include/gf_hip.h): every table cell cut into sub x sub sub-cells, point
//  (gr, gz) at the centre of sub-cell gr of numr*sub along R and gz of numz*sub along z, weighted with R times the
//  sub-cell's area.  As above every line is one IEEE fp64 operation:
//
//      R = rmin + dr*((double)(2*gr + 1)/(double)(2*sub))        z = zmin + dz*((double)(2*gz + 1)/(double)(2*sub))
//      area = (dr/sub)*(dz/sub)                                   w = R*area
//      takes part  iff  rlo <= R && R < rhi && zlo <= z && z < zhi
//
//  and the label is that of (x = R, y = 0, z) by the functions above.
struct window {
    double rlo, rhi, zlo, zhi;
};

//  The centre of sub-cell `g` of an axis that starts at `low` with table cells of `step`; twice_sub = (double)(2*sub).
GFHIP_HD double sub_centre(const double low, const double step, const unsigned long long g, const double twice_sub) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double fraction = static_cast<double> (2ull*g + 1ull)/twice_sub;
    const double offset = step*fraction;
    return low + offset;
}

GFHIP_HD double sub_area(const map &m, const uint32_t sub) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double width = m.dr/static_cast<double> (sub);
    const double height = m.dz/static_cast<double> (sub);
    return width*height;
}

GFHIP_HD double sub_weight(const double r, const double area) {
    return r*area;
}

GFHIP_HD bool in_window(const window &w, const double r, const double z) {
    return w.rlo <= r && r < w.rhi && w.zlo <= z && z < w.zhi;
}

}  // namespace flux
}  // namespace gfhip

#endif
