"""Reference for the sub-grid peak search (test infrastructure, no GPU): the iteration of vi_eval_peak_f64 (include/vinterp.h)
in NumPy, statement by statement, on the oracle's basis and gradient basis (oracle.SphHarmLagOracle.basis / grad_basis) and
the Hessian restatement of tests/hessian_ref.py (hess_basis, and row 2 - `up` - of enu_frame).  All columns advance together;
a column that has stopped is left alone.  tests/test_peak_host.py holds it against scipy.optimize.brentq on its own slope."""
import numpy as np

import hessian_ref as hr


def layer_fit(o, geom, seed=0):
    """synth's Chapman-like record on the beam geometry `geom` fitted with the oracle's basis by the weighted least squares of
    test_gpu_hessian._layer (minimum norm below 1e-10 of the largest singular value): the coefficient vector."""
    from volumetricinterp_amd import synth
    lat, lon, alt = synth.beams(*geom, seed=seed)
    value, error = synth.chapman_record(alt)
    A = o.basis(lat, lon, alt)
    return np.linalg.lstsq(A / error[:, None], value / error, rcond=1e-10)[0]


def walk(o, C, lat, lon, h):
    """(f, d1, d2, terms) at the points (lat, lon, h), 1-D: the value, the slope u . grad f and the curvature u^T H u along
    the geodetic normal u, and terms = |u . G| @ |C|, the size of the slope's summands.  C: (N,) or a row per point, (P, N)."""
    lat, lon, h = (np.asarray(a, dtype=np.float64).ravel() for a in (lat, lon, h))
    C = np.broadcast_to(np.asarray(C, dtype=np.float64), (lat.size, o.nbasis))
    with np.errstate(all='ignore'):
        B = o.basis(lat, lon, h)                                     # (P, N)
        G = o.grad_basis(lat, lon, h)                                # (P, 3, N)
        H = hr.hess_basis(o, lat, lon, h)                            # (P, 6, N), model frame
        u = hr.enu_frame(o, lat, lon, h)[:, 2, :]                    # (P, 3)
        f = np.einsum('pn,pn->p', B, C)
        uG = np.einsum('pc,pcn->pn', u, G)
        d1 = np.einsum('pn,pn->p', uG, C)
        Hc = np.einsum('pkn,pn->pk', H, C)
        d2 = np.zeros_like(f)
        for k, (c, d) in enumerate(hr.PAIRS):
            d2 += (1. if c == d else 2.) * u[:, c] * u[:, d] * Hc[:, k]
        terms = np.einsum('pn,pn->p', np.abs(uG), np.abs(C))
    return f, d1, d2, terms


def peak_search(o, C, lat, lon, h0, lo, hi, kind=1, tol=1e-3, max_iter=48):
    """The search of vi_eval_peak_f64 at the columns (lat, lon), 1-D, from h0 in [lo, hi]: a dict of arrays h, f, d1, d2 (NaN
    with status 3), status, it, and terms (walk's, at the returned h).  C: (N,) or (P, N)."""
    lat, lon = (np.asarray(a, dtype=np.float64).ravel() for a in (lat, lon))
    P = lat.size
    h, a, b = (np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), (P,))) for v in (h0, lo, hi))
    lo, hi = a.copy(), b.copy()
    C = np.broadcast_to(np.asarray(C, dtype=np.float64), (P, o.nbasis))
    s = float(kind)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(lat) & np.isfinite(lon) & np.isfinite(h) & np.isfinite(a) & np.isfinite(b) & (a <= h) & (h <= b)
    out = {k: np.full(P, np.nan) for k in ('h', 'f', 'd1', 'd2', 'terms')}
    status, it, done = np.full(P, 3, dtype=np.int32), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=bool)
    active = ok.copy()
    while active.any():
        i = np.flatnonzero(active)
        f, d1, d2, terms = walk(o, C[i], lat[i], lon[i], h[i])
        fin = np.isfinite(f) & np.isfinite(d1) & np.isfinite(d2)
        stop = ~fin | done[i] | (it[i] == max_iter)
        for j in i[stop & fin]:
            k = int(np.flatnonzero(i == j)[0])
            out['h'][j], out['f'][j], out['d1'][j], out['d2'][j], out['terms'][j] = h[j], f[k], d1[k], d2[k], terms[k]
            status[j] = 2 if not done[j] else 0 if (s * d2[k] < 0. and abs(h[j] - lo[j]) > tol and abs(h[j] - hi[j]) > tol) else 1
        active[i[stop]] = False
        go = ~stop
        j = i[go]
        it[j] += 1
        up = s * d1[go] > 0.
        a[j[up]] = h[j[up]]
        b[j[~up]] = h[j[~up]]
        with np.errstate(all='ignore'):
            hn = np.where(s * d2[go] < 0., h[j] - d1[go] / d2[go], np.nan)
            inside = (a[j] < hn) & (hn < b[j])
        hn = np.where(inside, hn, 0.5 * (a[j] + b[j]))
        done[j] = np.abs(hn - h[j]) <= tol
        h[j] = hn
    out.update(status=status, it=it)
    return out
