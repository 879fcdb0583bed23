"""The particle source of csrc/particle_draw.hpp in numpy, line for line: what gfhip_source_fill_host and the device fill
must give, byte for byte.

Philox4x32-10 in uint64 arithmetic (a 32 x 32 bit product fits), the draws in float64, one numpy operation per line of
the header, the labels and the field through flux_model.py and phase_model.py.  numpy's elementwise fp64 operations are
single IEEE operations and numpy.sqrt is correctly rounded."""
import numpy as np

import flux_model
import phase_model

MASK = np.uint64(0xFFFFFFFF)
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
POSITION, TOROIDAL, GYROPHASE, SPEED, PROFILE = range(5)
COUNTERS = ("placed", "unplaced", "position_tries", "gyro_tries")


def philox(counter, key):
    """The block of counter (four words) and key (two): arrays of words, or scalars; returns four uint64 arrays < 2^32."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) for k in key)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = M0*c0
        p1 = M1*c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & MASK, (p0 >> s32) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + W0) & MASK
        k1 = (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform_of(hi, lo):
    bits = (hi << np.uint64(21)) | (lo >> np.uint64(11))
    return bits.astype(np.float64)*np.float64(2.0**-53)


def uniforms(p, a, d, seed):
    """u1, u2 of block (p, a, d)."""
    p = np.asarray(p, dtype=np.uint64)
    a = np.broadcast_to(np.asarray(a, dtype=np.uint64), p.shape)
    d = np.full(p.shape, d, dtype=np.uint64)
    seed = np.uint64(seed)
    w = philox((p & MASK, p >> np.uint64(32), a, d), (seed & MASK, seed >> np.uint64(32)))
    return uniform_of(w[0], w[1]), uniform_of(w[2], w[3])


def circle(p, a, d, seed):
    """(accepted, c, s) of block (p, a, d)."""
    u1, u2 = uniforms(p, a, d, seed)
    t1 = 2.0*u1
    v1 = t1 - 1.0
    t2 = 2.0*u2
    v2 = t2 - 1.0
    aa = v1*v1
    bb = v2*v2
    q = aa + bb
    accepted = (q < 1.0) & (q > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        dd = aa - bb
        c = dd/q
        m = 2.0*v1
        n = m*v2
        s = n/q
    return accepted, c, s


def circle_loop(p, d, seed, attempts):
    """(found, c, s, tries) per particle."""
    found = np.zeros(p.size, dtype=bool)
    c, s = np.zeros(p.size), np.zeros(p.size)
    tries = np.full(p.size, attempts, dtype=np.int64)
    for a in range(attempts):
        todo = np.flatnonzero(~found)
        if todo.size == 0:
            break
        ok, ca, sa = circle(p[todo], a, d, seed)
        hit = todo[ok]
        found[hit], c[hit], s[hit], tries[hit] = True, ca[ok], sa[ok], a + 1
    return found, c, s, tries


def fill(tables, box, label_range, speed_range, count, pitch_range=(-1.0, 1.0), profile=None, seed=0, attempts=64,
         dtype=np.float64, sqrt_label=False, first_particle=0, psi0=None, span=None, details=False):
    """(columns, placed, counters) as source.fill_host returns them; with details=True also {beta, xi}, the drawn speed
    and pitch of every placed particle (NaN for the others)."""
    rlo, rhi, zlo, zhi = (np.float64(v) for v in box)
    slo, shi = (np.float64(v) for v in label_range)
    blo, bhi = (np.float64(v) for v in speed_range)
    xlo, xhi = (np.float64(v) for v in pitch_range)
    rlo2 = rlo*rlo
    rhi2 = rhi*rhi
    dr2 = rhi2 - rlo2
    dz = zhi - zlo
    db = bhi - blo
    dx = xhi - xlo
    options = dict(psi0=psi0, span=span, sqrt_label=sqrt_label)
    n = int(count)
    p = np.uint64(first_particle) + np.arange(n, dtype=np.uint64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        alive, cf, sf, _ = circle_loop(p, TOROIDAL, seed, attempts)
#  loop 2
        x, y, z = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
        found = np.zeros(n, dtype=bool)
        position_tries = np.where(alive, attempts, 0).astype(np.int64)
        for a in range(attempts):
            todo = np.flatnonzero(alive & ~found)
            if todo.size == 0:
                break
            u1, u2 = uniforms(p[todo], a, POSITION, seed)
            t = dr2*u1
            r2 = rlo2 + t
            r = np.sqrt(r2)
            t = dz*u2
            za = zlo + t
            xa = r*cf[todo]
            ya = r*sf[todo]
            xa, ya, za = (v.astype(dtype).astype(np.float64) for v in (xa, ya, za))
            label = flux_model.label(tables, xa, ya, za, **options)
            ok = (slo <= label) & (label < shi)
            if profile is not None:
                sedges, accept = (np.asarray(v, dtype=np.float64) for v in profile)
                cell = flux_model.cells_of(sedges, label)
                v1, _ = uniforms(p[todo], a, PROFILE, seed)
                ok &= (cell >= 0) & (v1 < accept[np.maximum(cell, 0)])
            hit = todo[ok]
            found[hit], x[hit], y[hit], z[hit], position_tries[hit] = True, xa[ok], ya[ok], za[ok], a + 1
        alive &= found
#  step 3
        at = np.flatnonzero(alive)
        inside, _, gr, gz, f, _ = phase_model.field_at(tables, x[at], y[at], z[at])
        assert inside.all()
        gzgz = gz*gz
        ff = f*f
        grgr = gr*gr
        hh = gzgz + ff
        dd = hh + grgr
        den = np.sqrt(dd)
        h = np.sqrt(hh)
        good = (h > 0.0) & (den < np.inf)
        br = gz/den
        bp = f/den
        bz = (-gr)/den
        e1r = (-f)/h
        e1p = gz/h
        dh = den*h
        t = gr*gz
        e2r = t/dh
        t = gr*f
        e2p = t/dh
        e2z = h/den
#  loop 4, for those with a basis
        turned, cg, sg, tries = circle_loop(p[at], GYROPHASE, seed, attempts)
        gyro_tries = np.zeros(n, dtype=np.int64)
        gyro_tries[at] = np.where(good, tries, 0)
        keep = good & turned
#  step 5
        u1, u2 = uniforms(p[at], 0, SPEED, seed)
        t = db*u1
        beta = blo + t
        t = dx*u2
        xi = xlo + t
        along = beta*xi
        xx = xi*xi
        om = 1.0 - xx
        om[om < 0.0] = 0.0
        sq = np.sqrt(om)
        perp = beta*sq
        p1 = cg*e1r
        p2 = sg*e2r
        wr = p1 + p2
        p1 = cg*e1p
        p2 = sg*e2p
        wp = p1 + p2
        wz = sg*e2z
        p1 = along*br
        p2 = perp*wr
        vr = p1 + p2
        p1 = along*bp
        p2 = perp*wp
        vp = p1 + p2
        p1 = along*bz
        p2 = perp*wz
        vz = p1 + p2
        p1 = vr*cf[at]
        p2 = vp*sf[at]
        ux = p1 - p2
        p1 = vr*sf[at]
        p2 = vp*cf[at]
        uy = p1 + p2
        uz = vz
    placed = np.zeros(n, dtype=bool)
    placed[at[keep]] = True
    columns = [np.full(n, np.nan, dtype=dtype) for _ in range(7)]
    final = at[keep]
    for column, values in zip(columns, (x[final], y[final], z[final], ux[keep], uy[keep], uz[keep], np.zeros(final.size))):
        column[final] = values.astype(dtype)
    counters = dict(placed=int(placed.sum()), unplaced=int(n - placed.sum()), position_tries=int(position_tries.sum()),
                    gyro_tries=int(gyro_tries.sum()))
    if not details:
        return columns, placed.astype(dtype), counters
    drawn = dict(beta=np.full(n, np.nan), xi=np.full(n, np.nan))
    drawn["beta"][final], drawn["xi"][final] = beta[keep], xi[keep]
    return columns, placed.astype(dtype), counters, drawn
