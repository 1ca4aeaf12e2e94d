"""Reference for the search of maxima and minima in three dimensions (test infrastructure, no GPU): the iteration of
vi_eval_extremum_f64 (include/vinterp.h) in NumPy, statement by statement, on the oracle's basis and gradient basis
(oracle.SphHarmLagOracle.basis / grad_basis) and the Hessian restatement of tests/hessian_ref.py.  An iterate x (ECEF metres)
goes through geodesy.ecef2geodetic to the oracle, which takes geodetic points; gradient and Hessian come in the model's
orthonormal frame (r', theta', phi') and are turned into ECEF with the unit vectors of that frame at the point
(hessian_ref.model_axes): g = E^T g_model, H = E^T H_model E - the Hessian is a tensor there, so H is the plain Cartesian matrix
of second derivatives and Newton's iteration in R^3 has no connection terms.  All searches advance together - one walk of all
that are still running per pass -; a search that has stopped is left alone.  tests/test_extremum_host.py holds it against
scipy.optimize.minimize(method='trust-exact') on its own value, gradient and Hessian and against tests/peak_ref.py."""
import numpy as np

import hessian_ref as hr
from volumetricinterp_amd import geodesy


def walk(o, C, x):
    """(f (P,), g (P, 3), H (P, 3, 3), terms (P,)) at the ECEF points x (P, 3): value, gradient and Hessian in ECEF, and
    terms = the largest component of |E^T G| @ |C|, the size of the gradient's summands.  C: (N,) or a row per point, (P, N)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    C = np.broadcast_to(np.asarray(C, dtype=np.float64), (x.shape[0], o.nbasis))
    with np.errstate(all='ignore'):
        lat, lon, alt = geodesy.ecef2geodetic(x[:, 0], x[:, 1], x[:, 2])
        B = o.basis(lat, lon, alt)                                       # (P, N)
        G = o.grad_basis(lat, lon, alt)                                  # (P, 3, N), model frame
        Hm = np.einsum('pkn,pn->pk', hr.hess_basis(o, lat, lon, alt), C)  # (P, 6), model frame
        E = hr.model_axes(o, lat, lon, alt)                              # (P, 3, 3): row c = unit vector c in ECEF
        f = np.einsum('pn,pn->p', B, C)
        EG = np.einsum('pci,pcn->pin', E, G)                             # the gradient basis in ECEF
        g = np.einsum('pin,pn->pi', EG, C)
        S = np.empty((x.shape[0], 3, 3))
        for k, (c, d) in enumerate(hr.PAIRS):
            S[:, c, d] = S[:, d, c] = Hm[:, k]
        H = np.einsum('pci,pcd,pdj->pij', E, S, E)
        H = 0.5 * (H + H.transpose(0, 2, 1))
        terms = np.einsum('pin,pn->pi', np.abs(EG), np.abs(C)).max(axis=1)
    return f, g, H, terms


def inside(x, eq, htol):
    """Whether the ECEF point x is inside every half-space of eq (F, 4): K2l's criterion, n . x + off <= htol.  None: no hull."""
    if eq is None or len(eq) == 0:
        return True
    with np.errstate(invalid='ignore'):
        return bool((eq[:, :3] @ x + eq[:, 3] <= htol).all())


def norm3(v):
    return float(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))


def pivots(A):
    """The three pivots of the LDL^T factorisation of the symmetric 3 x 3 matrix A in the order 1, 2, 3, nothing replaced."""
    with np.errstate(all='ignore'):
        p1 = A[0, 0]
        l21, l31 = A[1, 0] / p1, A[2, 0] / p1
        p2 = A[1, 1] - l21 * A[1, 0]
        t32 = A[2, 1] - l31 * A[1, 0]
        l32 = t32 / p2
        p3 = A[2, 2] - l31 * A[2, 0] - l32 * t32
    return p1, p2, p3


def definite(A):
    """All three pivots of A positive, by comparisons that a NaN fails."""
    p1, p2, p3 = pivots(A)
    return bool(p1 > 0. and p2 > 0. and p3 > 0.)


def newton_step(A, b, mu):
    """(d, mod): the solution of A d = b by LDL^T in the order 1, 2, 3 with every pivot that is not > mu replaced by mu, and
    whether one was."""
    mod = False
    p1 = A[0, 0]
    if not p1 > mu:
        p1, mod = mu, True
    l21, l31 = A[1, 0] / p1, A[2, 0] / p1
    p2 = A[1, 1] - l21 * A[1, 0]
    if not p2 > mu:
        p2, mod = mu, True
    t32 = A[2, 1] - l31 * A[1, 0]
    l32 = t32 / p2
    p3 = A[2, 2] - l31 * A[2, 0] - l32 * t32
    if not p3 > mu:
        p3, mod = mu, True
    y1 = b[0]
    y2 = b[1] - l21 * y1
    y3 = b[2] - l31 * y1 - l32 * y2
    d3 = y3 / p3
    d2 = y2 / p2 - l32 * d3
    d1 = y1 / p1 - l21 * d2 - l31 * d3
    return np.array([d1, d2, d3]), mod


def extremum_search(o, C, x0, radius, kind=1, max_step=None, tol=1e-3, max_iter=48, eq=None, htol=0.):
    """The search of vi_eval_extremum_f64 from the starts x0 (P, 3) in ECEF metres inside the balls of `radius` (P,) and the
    half-spaces eq (F, 4; None: no hull): a dict of arrays x (P, 3), f, g (P, 3), H (P, 3, 3) - NaN with status 3 -, status,
    it, rejects (the backtracking passes), terms (walk's, at the returned point) and lam, the smallest |eigenvalue| of H there.
    C: (N,) or (P, N).  max_step: a number for all (None: radius / 8 each)."""
    x0 = np.array(np.asarray(x0, dtype=np.float64).reshape(-1, 3))
    P = x0.shape[0]
    radius = np.array(np.broadcast_to(np.asarray(radius, dtype=np.float64), (P,)))
    mstep = radius / 8. if max_step is None else np.array(np.broadcast_to(np.asarray(max_step, dtype=np.float64), (P,)))
    C = np.broadcast_to(np.asarray(C, dtype=np.float64), (P, o.nbasis))
    sg = float(kind)
    out = dict(x=np.full((P, 3), np.nan), f=np.full(P, np.nan), g=np.full((P, 3), np.nan), H=np.full((P, 3, 3), np.nan),
               terms=np.full(P, np.nan), lam=np.full(P, np.nan))
    status, it, rejects = np.full(P, 3, dtype=np.int32), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(x0).all(axis=1) & np.isfinite(radius) & (radius > 0.) & np.isfinite(mstep) & (mstep > 0.)
    x, xb, d = x0.copy(), x0.copy(), np.zeros((P, 3))
    fb, gb, delta = np.zeros(P), np.zeros(P), mstep.copy()
    have, done, full = np.zeros(P, dtype=bool), np.zeros(P, dtype=bool), np.zeros(P, dtype=bool)
    active = ok.copy()
    while active.any():
        idx = np.flatnonzero(active)
        F, G, HH, terms = walk(o, C[idx], x[idx])
        for k, j in enumerate(idx):
            f, g, H = F[k], G[k], HH[k]
            dx = x[j] - x0[j]
            ins = inside(x[j], eq, htol) and norm3(dx) <= radius[j]
            fin = np.isfinite(f) and np.isfinite(g).all() and np.isfinite(H).all()
            if not fin or (not have[j] and not ins):
                active[j] = False                                        # status 3
                continue
            if done[j] or it[j] == max_iter:
                out['x'][j], out['f'][j], out['g'][j], out['H'][j], out['terms'][j] = x[j], f, g, H, terms[k]
                out['lam'][j] = np.abs(np.linalg.eigvalsh(H)).min()
                status[j] = 2 if not done[j] else 0 if (full[j] and ins and definite(-sg * H)) else 1
                active[j] = False
                continue
            it[j] += 1
            gn = norm3(g)
            if have[j] and (not ins or not (sg * f >= sg * fb[j] or (full[j] and gn < gb[j]))):
                rejects[j] += 1
                full[j] = False
                dl = norm3(d[j])
                if dl <= tol:                                            # the rejected step was within tol of the best point
                    x[j], done[j] = xb[j], True
                else:
                    d[j] = 0.25 * d[j]
                    delta[j] = 0.25 * dl
                    x[j] = xb[j] + d[j]
                continue
            if have[j]:
                delta[j] = min(2. * delta[j], mstep[j])
            xb[j], fb[j], gb[j], have[j] = x[j], f, gn, True
            if gn == 0.:
                step, mod = np.zeros(3), False                           # a zero gradient is a step of zero length
            else:
                step, mod = newton_step(-sg * H, sg * g, gn / delta[j])
            full[j] = not mod
            dn = norm3(step)
            if dn > delta[j]:
                step = step * (delta[j] / dn)
                full[j] = False
                dn = delta[j]
            d[j] = step
            done[j] = dn <= tol
            x[j] = x[j] + step
    out.update(status=status, it=it, rejects=rejects)
    return out
