//------------------------------------------------------------------------------
///  @file particle_draw.hpp
///  @brief The rule by which a particle source places particle `p` of an ensemble, host and device.
///
///  Particle p (uint64, its index in the WHOLE ensemble) is drawn from a counter-based generator keyed by p, so that it
///  is the same particle, to the last bit, whoever draws it: any device, shard split, launch shape or route, and the
///  host.  The arithmetic is fixed as in flux_label.hpp: every line below is one IEEE fp64 operation, in this order,
///  nothing fused (contraction is switched off here), only + - * / sqrt and comparisons, so the host, the device and the
///  numpy model of the tests give the same bits.  Plain C++.
///
///  Generator: Philox4x32, 10 rounds, M0 = 0xD2511F53, M1 = 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85,
///      round:  c' = (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)),  then k0 += W0, k1 += W1
///  Block (p, a, d) of seed: counter = (lo32(p), hi32(p), a, d), key = (lo32(seed), hi32(seed)); a: the attempt, d: the
///  purpose (0 position, 1 toroidal direction, 2 gyrophase, 3 speed and pitch, 4 profile).  Its four words w0..w3 give
///      u1 = U(w0, w1)    u2 = U(w2, w3)    U(hi, lo) = (double)(((uint64)hi << 21) | (lo >> 11)) * 2^-53    (both exact)
///
///  A unit vector on the circle from a block (circle):
///      t1 = 2.0*u1    v1 = t1 - 1.0    t2 = 2.0*u2    v2 = t2 - 1.0
///      a = v1*v1      b = v2*v2        q = a + b
///      accepted  iff  q < 1.0 && q > 0.0
///      d = a - b      c = d/q          m = 2.0*v1     n = m*v2      s = n/q            (the doubled angle)
///
///  Every loop below runs a = 0 .. attempts - 1 and stops at the first accepted attempt; a particle for which a loop runs
///  out, or the basis fails, is UNPLACED.  From the caller's box, ranges and seed (parameters_of):
///      rlo2 = rlo*rlo    rhi2 = rhi*rhi    dr2 = rhi2 - rlo2    dz = zhi - zlo    db = bhi - blo    dx = xhi - xlo
///
///  1. (cf, sf): circle on blocks d = 1.
///  2. Position, blocks d = 0 (position_attempt):
///      t = dr2*u1     R2 = rlo2 + t    R = sqrt(R2)
///      t = dz*u2      z = zlo + t
///      x = R*cf       y = R*sf
///      x, y, z rounded to the columns' type T and widened again: what follows sees what is STORED
///      label = canonical(label of (x, y, z)) by flux_label.hpp's locate, psi_of and label_of; NaN off the map
///      accepted  iff  slo <= label && label < shi
///      with a profile: is = the cell of label among sedges (no cell: rejected); u = u1 of block (p, a, 4);
///                      accepted  iff also  u < accept[is]
///  3. The field at the stored position (basis_at), psi_gradient, fpol_interval and fpol_of giving gR, gZ, f:
///      gzgz = gZ*gZ   ff = f*f   grgr = gR*gR   hh = gzgz + ff   dd = hh + grgr   den = sqrt(dd)   h = sqrt(hh)
///      fails  unless  h > 0.0 && den < infinity         (a NaN fails)
///      bR = gZ/den    bP = f/den    bZ = (-gR)/den                                      b, in (R, phi, z)
///      e1R = (-f)/h   e1P = gZ/h                                                        e1 (its z component is 0)
///      dh = den*h     t = gR*gZ   e2R = t/dh     t = gR*f   e2P = t/dh     e2Z = h/den  e2
///  4. (cg, sg): circle on blocks d = 2.
///  5. Speed and pitch, block (p, 0, 3) (velocity_of):
///      t = db*u1      beta = blo + t
///      t = dx*u2      xi = xlo + t
///      par = beta*xi
///      xx = xi*xi     om = 1.0 - xx;   if (om < 0.0) om = 0.0       sq = sqrt(om)     perp = beta*sq
///      p1 = cg*e1R    p2 = sg*e2R      wR = p1 + p2
///      p1 = cg*e1P    p2 = sg*e2P      wP = p1 + p2
///      wZ = sg*e2Z
///      p1 = par*bR    p2 = perp*wR     vR = p1 + p2           likewise vP and vZ
///      p1 = vR*cf     p2 = vP*sf       ux = p1 - p2
///      p1 = vR*sf     p2 = vP*cf       uy = p1 + p2           uz = vZ
///  6. The columns receive x, y, z as stored, ux, uy, uz rounded to T (components of beta: the push's initialize_gamma
///     makes gamma and gamma*beta of them) and gamma = 0; `placed`, where there is one, 1.  An unplaced particle gets the
///     quiet NaN without payload in all seven and placed = 0.
///
///  tries[0] counts the attempts loop 2 used (a + 1 of the accepted one, `attempts` when it ran out, 0 when loop 1
///  did), tries[1] those of loop 4.
//------------------------------------------------------------------------------
#ifndef GFHIP_PARTICLE_DRAW_HPP
#define GFHIP_PARTICLE_DRAW_HPP

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "flux_label.hpp"
#include "superacc.hpp"                                // GFHIP_HD

namespace gfhip {
namespace draw {

constexpr uint32_t flag_plain = 1u;                    // particle_source.hip: one lane, one particle
constexpr uint32_t flag_refill = 2u;                   // a settled lane takes the wave's next particle
constexpr uint32_t known_flags = flag_plain | flag_refill;
constexpr uint32_t max_attempts = 4096;
constexpr int max_profile_cells = 256;

constexpr uint32_t purpose_position = 0, purpose_toroidal = 1, purpose_gyrophase = 2, purpose_speed = 3, purpose_profile = 4;

//  What the rule needs beside the map and the field; ns = 0 without a profile.
struct parameters {
    double rlo2, dr2, zlo, dz, slo, shi, blo, db, xlo, dx;
    uint32_t key[2];
    uint32_t attempts;
    int ns;
};

//  box: rlo, rhi, zlo, zhi.
GFHIP_HD parameters parameters_of(const double *box, const double slo, const double shi, const double blo, const double bhi,
                                  const double xlo, const double xhi, const uint64_t seed, const uint32_t attempts, const int ns) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    parameters p;
    p.rlo2 = box[0]*box[0];
    const double rhi2 = box[1]*box[1];
    p.dr2 = rhi2 - p.rlo2;
    p.zlo = box[2];
    p.dz = box[3] - box[2];
    p.slo = slo;
    p.shi = shi;
    p.blo = blo;
    p.db = bhi - blo;
    p.xlo = xlo;
    p.dx = xhi - xlo;
    p.key[0] = static_cast<uint32_t> (seed);
    p.key[1] = static_cast<uint32_t> (seed >> 32);
    p.attempts = attempts;
    p.ns = ns;
    return p;
}

//  Philox4x32-10.
GFHIP_HD void philox(const uint32_t *counter, const uint32_t *key, uint32_t *out) {
    uint32_t c0 = counter[0], c1 = counter[1], c2 = counter[2], c3 = counter[3], k0 = key[0], k1 = key[1];
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = static_cast<uint64_t> (0xD2511F53u)*c0;
        const uint64_t p1 = static_cast<uint64_t> (0xCD9E8D57u)*c2;
        const uint32_t n0 = static_cast<uint32_t> (p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = static_cast<uint32_t> (p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = static_cast<uint32_t> (p1);
        c2 = n2;
        c3 = static_cast<uint32_t> (p0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

GFHIP_HD double uniform_of(const uint32_t hi, const uint32_t lo) {
    const uint64_t bits = (static_cast<uint64_t> (hi) << 21) | (lo >> 11);
    return static_cast<double> (bits)*0x1.0p-53;
}

//  u1 and u2 of block (p, a, d).
GFHIP_HD void uniforms_of(const parameters &par, const uint64_t p, const uint32_t a, const uint32_t d, double &u1, double &u2) {
    const uint32_t counter[4] = {static_cast<uint32_t> (p), static_cast<uint32_t> (p >> 32), a, d};
    uint32_t w[4];
    philox(counter, par.key, w);
    u1 = uniform_of(w[0], w[1]);
    u2 = uniform_of(w[2], w[3]);
}

struct direction {
    double c, s;
};

//  The unit vector of block (p, a, d); false: rejected.
GFHIP_HD bool circle(const parameters &par, const uint64_t p, const uint32_t a, const uint32_t d, direction &out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double u1, u2;
    uniforms_of(par, p, a, d, u1, u2);
    const double t1 = 2.0*u1;
    const double v1 = t1 - 1.0;
    const double t2 = 2.0*u2;
    const double v2 = t2 - 1.0;
    const double aa = v1*v1;
    const double bb = v2*v2;
    const double q = aa + bb;
    if (!(q < 1.0 && q > 0.0)) return false;
    const double dd = aa - bb;
    out.c = dd/q;
    const double m = 2.0*v1;
    const double n = m*v2;
    out.s = n/q;
    return true;
}

//  Loops 1 and 4: the first accepted attempt, `tries` the attempts used; false: none of par.attempts.
GFHIP_HD bool circle_loop(const parameters &par, const uint64_t p, const uint32_t d, direction &out, uint32_t &tries) {
    for (uint32_t a = 0; a < par.attempts; a++) {
        if (circle(par, p, a, d, out)) {
            tries = a + 1;
            return true;
        }
    }
    tries = par.attempts;
    return false;
}

//  TABLES, the caller's tables, has
//      void coefficients(long long at, double *c) const      the 16 of table cell `at`
//      void cubic(int q, double *c) const                    the 4 of fpol interval q
//      double accept_of(double label) const                  the profile's probability in label's cell, -1.0 in none

//  Attempt a of loop 2; xyz: the candidate as stored in T, widened.
template<typename T, typename TABLES>
GFHIP_HD bool position_attempt(const flux::map &m, const parameters &par, const TABLES &tables, const uint64_t p, const uint32_t a,
                               const direction &phi, double *xyz) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double u1, u2;
    uniforms_of(par, p, a, purpose_position, u1, u2);
    double t = par.dr2*u1;
    const double r2 = par.rlo2 + t;
    const double r = sqrt(r2);
    t = par.dz*u2;
    const double z = par.zlo + t;
    const double x = r*phi.c;
    const double y = r*phi.s;
    xyz[0] = static_cast<double> (static_cast<T> (x));
    xyz[1] = static_cast<double> (static_cast<T> (y));
    xyz[2] = static_cast<double> (static_cast<T> (z));
    double tr, tz, c[16];
    const long long at = flux::locate(m, xyz[0], xyz[1], xyz[2], tr, tz);
    if (at < 0) return false;
    tables.coefficients(at, c);
    const double label = flux::canonical(flux::label_of(m, flux::psi_of(c, tr, tz)));
    if (!(par.slo <= label && label < par.shi)) return false;
    if (par.ns == 0) return true;
    const double chance = tables.accept_of(label);
    if (chance < 0.0) return false;
    double v1, v2;
    uniforms_of(par, p, a, purpose_profile, v1, v2);
    return v1 < chance;
}

struct frame {
    double br, bp, bz, e1r, e1p, e2r, e2p, e2z;
};

//  Step 3; false: the particle stays unplaced.
template<typename TABLES>
GFHIP_HD bool basis_at(const flux::map &m, const flux::field &f, const TABLES &tables, const double *xyz, frame &out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double tr, tz, tp, gr, gz, c[16], cubic[4];
    const long long at = flux::locate(m, xyz[0], xyz[1], xyz[2], tr, tz);
    if (at < 0) return false;
    tables.coefficients(at, c);
    const double psi = flux::psi_gradient(m, c, tr, tz, gr, gz);
    const int q = flux::fpol_interval(f, psi, tp);
    tables.cubic(q, cubic);
    const double fp = flux::fpol_of(cubic, tp);
    const double gzgz = gz*gz;
    const double ff = fp*fp;
    const double grgr = gr*gr;
    const double hh = gzgz + ff;
    const double dd = hh + grgr;
    const double den = sqrt(dd);
    const double h = sqrt(hh);
    if (!(h > 0.0 && den < __builtin_inf())) return false;
    out.br = gz/den;
    out.bp = fp/den;
    out.bz = (-gr)/den;
    out.e1r = (-fp)/h;
    out.e1p = gz/h;
    const double dh = den*h;
    double t = gr*gz;
    out.e2r = t/dh;
    t = gr*fp;
    out.e2p = t/dh;
    out.e2z = h/den;
    return true;
}

//  Step 5: the Cartesian components of beta.
GFHIP_HD void velocity_of(const parameters &par, const uint64_t p, const direction &phi, const direction &gyro, const frame &e,
                          double *u) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double u1, u2;
    uniforms_of(par, p, 0, purpose_speed, u1, u2);
    double t = par.db*u1;
    const double beta = par.blo + t;
    t = par.dx*u2;
    const double xi = par.xlo + t;
    const double along = beta*xi;
    const double xx = xi*xi;
    double om = 1.0 - xx;
    if (om < 0.0) om = 0.0;
    const double sq = sqrt(om);
    const double perp = beta*sq;
    double p1 = gyro.c*e.e1r;
    double p2 = gyro.s*e.e2r;
    const double wr = p1 + p2;
    p1 = gyro.c*e.e1p;
    p2 = gyro.s*e.e2p;
    const double wp = p1 + p2;
    const double wz = gyro.s*e.e2z;
    p1 = along*e.br;
    p2 = perp*wr;
    const double vr = p1 + p2;
    p1 = along*e.bp;
    p2 = perp*wp;
    const double vp = p1 + p2;
    p1 = along*e.bz;
    p2 = perp*wz;
    const double vz = p1 + p2;
    p1 = vr*phi.c;
    p2 = vp*phi.s;
    u[0] = p1 - p2;
    p1 = vr*phi.s;
    p2 = vp*phi.c;
    u[1] = p1 + p2;
    u[2] = vz;
}

//  Steps 3 to 5 of a particle whose position was accepted: out[3..5], and tries[1]; false: unplaced.
template<typename TABLES>
GFHIP_HD bool momentum_of(const flux::map &m, const flux::field &f, const parameters &par, const TABLES &tables, const uint64_t p,
                          const direction &phi, const double *xyz, double *u, uint32_t &gyro_tries) {
    frame e;
    gyro_tries = 0;
    if (!basis_at(m, f, tables, xyz, e)) return false;
    direction gyro;
    if (!circle_loop(par, p, purpose_gyrophase, gyro, gyro_tries)) return false;
    velocity_of(par, p, phi, gyro, e, u);
    return true;
}

//  The whole of particle p: out = x, y, z, ux, uy, uz (fp64, x, y, z already as stored); tries: loops 2 and 4.
template<typename T, typename TABLES>
GFHIP_HD bool particle(const flux::map &m, const flux::field &f, const parameters &par, const TABLES &tables, const uint64_t p,
                       double *out, uint32_t *tries) {
    tries[0] = tries[1] = 0;
    direction phi;
    uint32_t used;
    if (!circle_loop(par, p, purpose_toroidal, phi, used)) return false;
    bool found = false;
    for (uint32_t a = 0; a < par.attempts && !found; a++) {
        found = position_attempt<T> (m, par, tables, p, a, phi, out);
        tries[0] = a + 1;
    }
    if (!found) return false;
    return momentum_of(m, f, par, tables, p, phi, out, out + 3, tries[1]);
}

//  Step 6 for one particle: columns x, y, z, ux, uy, uz, gamma at index `at`, and `placed` where there is one.
template<typename T>
GFHIP_HD void store(T *const *columns, T *placed, const size_t at, const bool is_placed, const double *out) {
    if (is_placed) {
        for (int k = 0; k < 6; k++) columns[k][at] = static_cast<T> (out[k]);
        columns[6][at] = static_cast<T> (0);
    } else {
        for (int k = 0; k < 7; k++) columns[k][at] = static_cast<T> (__builtin_nanf(""));
    }
    if (placed) placed[at] = static_cast<T> (is_placed ? 1 : 0);
}

}  // namespace draw
}  // namespace gfhip

#endif
