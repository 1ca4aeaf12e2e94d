"""Reference for the level-crossing search and the crossing maps (test infrastructure, no GPU): the iteration of
vi_eval_level_f64 (include/vinterp.h) in NumPy, statement by statement, on the oracle's basis and gradient basis
(oracle.SphHarmLagOracle.basis / grad_basis) and row 2 - `up` - of tests/hessian_ref.py's enu_frame; and crossing_index, the map
of vi_eval_resident_cross_f64 by a plain loop.  All columns advance together; a column that has stopped is left alone.
tests/test_level_host.py holds the search against scipy.optimize.brentq on its own value."""
import numpy as np

import hessian_ref as hr


def walk(o, C, lat, lon, h):
    """(f, d1, terms, vterms) at the points (lat, lon, h), 1-D: the value, the slope u . grad f along the geodetic normal u,
    terms = |u . G| @ |C|, the size of the slope's summands, and vterms = |B| @ |C|, the size of the value's.  C: (N,) or a row
    per point, (P, N)."""
    lat, lon, h = (np.asarray(a, dtype=np.float64).ravel() for a in (lat, lon, h))
    C = np.broadcast_to(np.asarray(C, dtype=np.float64), (lat.size, o.nbasis))
    with np.errstate(all='ignore'):
        B = o.basis(lat, lon, h)                                     # (P, N)
        G = o.grad_basis(lat, lon, h)                                # (P, 3, N)
        u = hr.enu_frame(o, lat, lon, h)[:, 2, :]                    # (P, 3)
        f = np.einsum('pn,pn->p', B, C)
        uG = np.einsum('pc,pcn->pn', u, G)
        d1 = np.einsum('pn,pn->p', uG, C)
        terms = np.einsum('pn,pn->p', np.abs(uG), np.abs(C))
        vterms = np.einsum('pn,pn->p', np.abs(B), np.abs(C))
    return f, d1, terms, vterms


def level_search(o, C, lat, lon, level, lo, hi, tol=1e-3, max_iter=48):
    """The search of vi_eval_level_f64 at the columns (lat, lon), 1-D, for `level` in (lo, hi): a dict of arrays h, f, d1 (NaN
    with status 1 and 3), status, it, and terms, vterms (walk's, at the returned h).  C: (N,) or (P, N).  No hull."""
    lat, lon = (np.asarray(a, dtype=np.float64).ravel() for a in (lat, lon))
    P = lat.size
    Lv, a, b = (np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), (P,))) for v in (level, lo, hi))
    C = np.broadcast_to(np.asarray(C, dtype=np.float64), (P, o.nbasis))
    out = {k: np.full(P, np.nan) for k in ('h', 'f', 'd1', 'terms', 'vterms')}
    status, it, done = np.full(P, 3, dtype=np.int32), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=bool)
    h, sa = np.full(P, np.nan), np.zeros(P, dtype=bool)

    def report(j, st, hh, w, k):
        out['h'][j], out['f'][j], out['d1'][j], out['terms'][j], out['vterms'][j] = hh, w[0][k], w[1][k], w[2][k], w[3][k]
        status[j] = st

    with np.errstate(invalid='ignore'):
        ok = np.isfinite(lat) & np.isfinite(lon) & np.isfinite(a) & np.isfinite(b) & np.isfinite(Lv) & (a < b)
    i = np.flatnonzero(ok)
    active = np.zeros(P, dtype=bool)
    if i.size:
        wa, wb = walk(o, C[i], lat[i], lon[i], a[i]), walk(o, C[i], lat[i], lon[i], b[i])
        for k, j in enumerate(i):
            fa, fb = wa[0][k] - Lv[j], wb[0][k] - Lv[j]
            if not (np.isfinite(fa) and np.isfinite(fb)):
                continue                                              # status 3
            if fa == 0.:
                report(j, 0, a[j], wa, k)
            elif fb == 0.:
                report(j, 0, b[j], wb, k)
            elif (fa > 0.) == (fb > 0.):
                status[j] = 1
            else:
                sa[j] = fa > 0.
                h[j] = a[j] - fa * (b[j] - a[j]) / (fb - fa)
                if not (a[j] < h[j] < b[j]):
                    h[j] = 0.5 * (a[j] + b[j])
                active[j] = True
    while active.any():
        i = np.flatnonzero(active)
        w = walk(o, C[i], lat[i], lon[i], h[i])
        for k, j in enumerate(i):
            phi, d1 = w[0][k] - Lv[j], w[1][k]
            if not (np.isfinite(phi) and np.isfinite(d1)):
                status[j], active[j] = 3, False
            elif phi == 0. or done[j] or it[j] == max_iter:
                report(j, 0 if (phi == 0. or done[j]) else 2, h[j], w, k)
                active[j] = False
            else:
                it[j] += 1
                if (phi > 0.) == sa[j]:
                    a[j] = h[j]
                else:
                    b[j] = h[j]
                with np.errstate(all='ignore'):
                    hn = h[j] - phi / d1 if d1 != 0. else np.nan
                if not (a[j] < hn < b[j]):
                    hn = 0.5 * (a[j] + b[j])
                done[j] = abs(hn - h[j]) <= tol
                h[j] = hn
    out.update(status=status, it=it)
    return out


def crossing_index(volume, level, axis=-1, which='first', direction='any'):
    """The map of ResidentGrid.crossing by a plain loop: volume (T,) + grid shape, `axis` an axis of the grid (counted without
    the leading T), level a scalar or anything that broadcasts to the map; int32 (T,) + grid shape without the axis."""
    volume = np.asarray(volume, dtype=np.float64)
    nd = volume.ndim - 1
    v = np.moveaxis(volume, 1 + axis % nd, -1)
    shape, L = v.shape[:-1], v.shape[-1]
    v = v.reshape(-1, L)
    lev = np.broadcast_to(np.asarray(level, dtype=np.float64), shape).ravel()
    idx = np.full(v.shape[0], -1, dtype=np.int32)
    for c in range(v.shape[0]):
        for l in (range(L - 1) if which == 'first' else range(L - 2, -1, -1)):
            f0, f1, lv = v[c, l], v[c, l + 1], lev[c]
            up, down = f0 <= lv <= f1, f0 >= lv >= f1
            if {'up': up, 'down': down, 'any': up or down}[direction]:
                idx[c] = l
                break
    return idx.reshape(shape)
