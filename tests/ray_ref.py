"""Reference for the searches along straight rays (test infrastructure, no GPU): the iterations of vi_eval_ray_peak_f64 and
vi_eval_ray_level_f64 (include/vinterp.h) in NumPy, statement by statement, on the oracle's basis and gradient basis
(oracle.SphHarmLagOracle.basis / grad_basis) and the Hessian restatement of tests/hessian_ref.py.  The point at the distance s
of a ray goes through geodesy.ecef2geodetic to the oracle, which takes geodetic points; w, the ray's unit direction in the
model's orthonormal frame (r', theta', phi') at the point, is formed as in the kernel: the direction turned by the model's
Rodrigues rotation and met with the three unit vectors of the rotated spherical coordinates (hessian_ref.model_axes holds
both).  All rays advance together; a ray that has stopped is left alone.  tests/test_ray_host.py holds the searches against
scipy.optimize.brentq on their own value and slope and, on vertical rays, against tests/peak_ref.py and tests/level_ref.py."""
import numpy as np

import hessian_ref as hr
from volumetricinterp_amd import geodesy


def lines(a, b):
    """(u, length): unit directions (P, 3) and lengths (P,) of the rays from a to b, (P, 3) each in ECEF metres."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    d = b - a
    length = np.sqrt(d[:, 0]**2 + d[:, 1]**2 + d[:, 2]**2)
    with np.errstate(all='ignore'):
        return d / length[:, None], length


def points(a, u, s):
    """(lat, lon, alt) of the points a + s u."""
    X = np.asarray(a, dtype=np.float64) + np.asarray(s, dtype=np.float64)[:, None] * u
    return geodesy.ecef2geodetic(X[:, 0], X[:, 1], X[:, 2])


def frame(o, u, lat, lon, alt):
    """w (P, 3): the components of the ECEF unit vectors u in the model's orthonormal frame at the points."""
    return np.einsum('pci,pi->pc', hr.model_axes(o, lat, lon, alt), u)


def walk(o, C, a, u, s, hess=True):
    """(f, d1, d2, terms, vterms) at the points a + s u, 1-D: the value, the slope w . grad f and the curvature w^T H w along the
    ray (NaN without `hess`), terms = |w . G| @ |C|, the size of the slope's summands, and vterms = |B| @ |C|, the size of the
    value's.  C: (N,) or a row per point, (P, N)."""
    s = np.asarray(s, dtype=np.float64).ravel()
    a, u = np.broadcast_to(a, (s.size, 3)), np.broadcast_to(u, (s.size, 3))
    C = np.broadcast_to(np.asarray(C, dtype=np.float64), (s.size, o.nbasis))
    with np.errstate(all='ignore'):
        lat, lon, alt = points(a, u, s)
        B = o.basis(lat, lon, alt)                                   # (P, N)
        G = o.grad_basis(lat, lon, alt)                              # (P, 3, N)
        w = frame(o, u, lat, lon, alt)                               # (P, 3)
        f = np.einsum('pn,pn->p', B, C)
        wG = np.einsum('pc,pcn->pn', w, G)
        d1 = np.einsum('pn,pn->p', wG, C)
        d2 = np.full_like(f, np.nan)
        if hess:
            Hc = np.einsum('pkn,pn->pk', hr.hess_basis(o, lat, lon, alt), C)
            d2 = np.zeros_like(f)
            for k, (c, d) in enumerate(hr.PAIRS):
                d2 += (1. if c == d else 2.) * w[:, c] * w[:, d] * Hc[:, k]
        terms = np.einsum('pn,pn->p', np.abs(wG), np.abs(C))
        vterms = np.einsum('pn,pn->p', np.abs(B), np.abs(C))
    return f, d1, d2, terms, vterms


def _ok_lines(a, length):
    with np.errstate(invalid='ignore'):
        return np.isfinite(a).all(axis=1) & np.isfinite(length) & (length > 0.)


def peak_search(o, C, a, b, s0, lo, hi, kind=1, tol=1e-3, max_iter=48):
    """The search of vi_eval_ray_peak_f64 on the rays a -> b, (P, 3) each, from s0 in [lo, hi]: a dict of arrays s, f, d1, d2
    (NaN with status 3), status, it, and terms, vterms (walk's, at the returned s).  C: (N,) or (P, N).  No hull."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    u, length = lines(a, b)
    P = a.shape[0]
    s, lb, ub = (np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), (P,))) for v in (s0, lo, hi))
    lo, hi = lb.copy(), ub.copy()
    C = np.broadcast_to(np.asarray(C, dtype=np.float64), (P, o.nbasis))
    sg = float(kind)
    with np.errstate(invalid='ignore'):
        ok = _ok_lines(a, length) & np.isfinite(s) & np.isfinite(lb) & np.isfinite(ub) & (lb <= s) & (s <= ub)
    out = {k: np.full(P, np.nan) for k in ('s', 'f', 'd1', 'd2', 'terms', 'vterms')}
    status, it, done = np.full(P, 3, dtype=np.int32), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=bool)
    margin, short = np.full(P, np.inf), np.zeros(P, dtype=bool)
    active = ok.copy()
    while active.any():
        i = np.flatnonzero(active)
        f, d1, d2, terms, vterms = walk(o, C[i], a[i], u[i], s[i])
        fin = np.isfinite(f) & np.isfinite(d1) & np.isfinite(d2)
        stop = ~fin | done[i] | (it[i] == max_iter)
        for k in np.flatnonzero(stop & fin):
            j = i[k]
            out['s'][j], out['f'][j], out['d1'][j], out['d2'][j] = s[j], f[k], d1[k], d2[k]
            out['terms'][j], out['vterms'][j] = terms[k], vterms[k]
            status[j] = 2 if not done[j] else 0 if (sg * d2[k] < 0. and abs(s[j] - lo[j]) > tol and abs(s[j] - hi[j]) > tol) else 1
        active[i[stop]] = False
        go = ~stop
        j = i[go]
        it[j] += 1
        up = sg * d1[go] > 0.
        lb[j[up]] = s[j[up]]
        ub[j[~up]] = s[j[~up]]
        with np.errstate(all='ignore'):
            sn = np.where(sg * d2[go] < 0., s[j] - d1[go] / d2[go], np.nan)
            inside = (lb[j] < sn) & (sn < ub[j])
            short[j] |= np.abs(sn - s[j]) < 4. * np.spacing(s[j])
        sn = np.where(inside, sn, 0.5 * (lb[j] + ub[j]))
        done[j] = np.abs(sn - s[j]) <= tol
        margin[j] = np.minimum(margin[j], np.abs(np.abs(sn - s[j]) - tol))
        s[j] = sn
    out.update(status=status, it=it, margin=margin, short=short)
    return out


def steady(r, o, peak):
    """Where the iteration count of a search result r (peak_search's or level_search's) is a reference: not `short`, and the
    stopping test |step| <= tol never came closer to flipping than twice the distance by which rounding can move an iterate -
    the bound N eps sum|terms| of a sum of N terms in any order (N the number of basis functions, eps 2^-52), turned into a
    distance by the derivative that Newton divides by: terms / |d2| for the peak, vterms / |d1| for the level.  Elsewhere two
    correct evaluations of the same iteration may count differently, the mirror in a batch and alone among them."""
    with np.errstate(all='ignore'):
        moved = o.nbasis * np.finfo(np.float64).eps * (r['terms'] / np.abs(r['d2']) if peak else r['vterms'] / np.abs(r['d1']))
        return ~r['short'] & ~(r['margin'] <= 2. * moved)


def level_search(o, C, a, b, level, lo, hi, tol=1e-3, max_iter=48):
    """The search of vi_eval_ray_level_f64 on the rays a -> b for `level` in (lo, hi): a dict of arrays s, f, d1 (NaN with
    status 1 and 3), status, it, and terms, vterms (walk's, at the returned s).  C: (N,) or (P, N).  No hull."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    u, length = lines(a, b)
    P = a.shape[0]
    Lv, lb, ub = (np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), (P,))) for v in (level, lo, hi))
    C = np.broadcast_to(np.asarray(C, dtype=np.float64), (P, o.nbasis))
    out = {k: np.full(P, np.nan) for k in ('s', 'f', 'd1', 'terms', 'vterms')}
    status, it, done = np.full(P, 3, dtype=np.int32), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=bool)
    s, sa = np.full(P, np.nan), np.zeros(P, dtype=bool)
    margin, short = np.full(P, np.inf), np.zeros(P, dtype=bool)

    def report(j, st, ss, w, k):
        out['s'][j], out['f'][j], out['d1'][j], out['terms'][j], out['vterms'][j] = ss, w[0][k], w[1][k], w[3][k], w[4][k]
        status[j] = st

    with np.errstate(invalid='ignore'):
        ok = _ok_lines(a, length) & np.isfinite(lb) & np.isfinite(ub) & np.isfinite(Lv) & (lb < ub)
    i = np.flatnonzero(ok)
    active = np.zeros(P, dtype=bool)
    if i.size:
        wa, wb = walk(o, C[i], a[i], u[i], lb[i], hess=False), walk(o, C[i], a[i], u[i], ub[i], hess=False)
        for k, j in enumerate(i):
            fa, fb = wa[0][k] - Lv[j], wb[0][k] - Lv[j]
            if not (np.isfinite(fa) and np.isfinite(fb)):
                continue                                              # status 3
            if fa == 0.:
                report(j, 0, lb[j], wa, k)
            elif fb == 0.:
                report(j, 0, ub[j], wb, k)
            elif (fa > 0.) == (fb > 0.):
                status[j] = 1
            else:
                sa[j] = fa > 0.
                s[j] = lb[j] - fa * (ub[j] - lb[j]) / (fb - fa)
                if not (lb[j] < s[j] < ub[j]):
                    s[j] = 0.5 * (lb[j] + ub[j])
                active[j] = True
    while active.any():
        i = np.flatnonzero(active)
        w = walk(o, C[i], a[i], u[i], s[i], hess=False)
        for k, j in enumerate(i):
            phi, d1 = w[0][k] - Lv[j], w[1][k]
            if not (np.isfinite(phi) and np.isfinite(d1)):
                status[j], active[j] = 3, False
            elif phi == 0. or done[j] or it[j] == max_iter:
                report(j, 0 if (phi == 0. or done[j]) else 2, s[j], w, k)
                active[j] = False
            else:
                it[j] += 1
                if (phi > 0.) == sa[j]:
                    lb[j] = s[j]
                else:
                    ub[j] = s[j]
                with np.errstate(all='ignore'):
                    sn = s[j] - phi / d1 if d1 != 0. else np.nan
                short[j] |= bool(abs(sn - s[j]) < 4. * np.spacing(s[j]))
                if not (lb[j] < sn < ub[j]):
                    sn = 0.5 * (lb[j] + ub[j])
                done[j] = abs(sn - s[j]) <= tol
                margin[j] = min(margin[j], abs(abs(sn - s[j]) - tol))
                s[j] = sn
    out.update(status=status, it=it, margin=margin, short=short)
    return out
