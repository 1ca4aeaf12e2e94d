"""Reference for the Hessian basis (test infrastructure, no GPU): a float64 NumPy/SciPy restatement of the closed-form second
derivatives of the Laguerre x spherical-cap-harmonic basis, written on top of the oracle's own pieces (oracle.SphHarmLagOracle:
transform_coord, Kvm, Az, dAz, the signed order into scipy.special.lpmv) with one special-function evaluation per basis index,
as the oracle's grad_basis is.  The reference project has no Hessian; tests/test_hessian_host.py holds this file against
50-digit arithmetic and against second differences of the oracle's basis.

A basis function is f = g(r) T(theta') A(phi') with r = RE (z/100 + 1), a = 100/RE, x = cos theta', y = sin theta':
  g0 = e^(-z/2) L_k,  g1 = dg/dr = -1/2 e^(-z/2) (L_k + 2 L1_(k-1)) a,  g2 = d2g/dr2 = e^(-z/2) (L_k/4 + L1_(k-1) + L2_(k-2)) a^2
  T  = lpmv(m, nu, x),  T' = (-(nu+1) x T + (nu-m+1) lpmv(m, nu+1, x)) / y,  T'' = -(x/y) T' - (nu(nu+1) - m^2/y^2) T
  A  = Az,  A' = dAz,  A'' = -m^2 A
and its Hessian - the second covariant derivatives, a tensor in 1/m^2 - in the orthonormal frame (r', theta', phi'):
  H_rr = g2 T A                                  H_rt = (g1/r - g0/r^2) T' A
  H_tt = g0 T'' A / r^2 + g1 T A / r             H_rp = (g1/r - g0/r^2) T A' / y
  H_pp = g0 T A''/(r^2 y^2) + g1 T A / r + x g0 T' A / (y r^2)      H_tp = g0 A' (T'/y - x T/y^2) / r^2
  trace = (g2 + 2 g1/r - nu(nu+1) g0/r^2) T A   (the Laplacian)
packed in the order PAIRS = (0,0) (1,1) (2,2) (0,1) (0,2) (1,2)."""
import numpy as np
import scipy.special as sp

from oracle.geodesy import geodetic2ecef
from oracle.sphharmlag import RE

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def rotation(o):
    """The Rodrigues matrix of the oracle's transform_coord (+theta0 about k, sphharmlag.py:345-353): R' = Rot @ R."""
    x0, y0, z0 = geodetic2ecef(o.latcp, o.loncp, 0.0)
    theta0 = np.arccos(z0 / np.sqrt(x0**2 + y0**2 + z0**2))
    phi0 = np.arctan2(y0, x0)
    k = np.array([np.cos(phi0 + np.pi / 2.0), np.sin(phi0 + np.pi / 2.0), 0.0])
    Kx = np.array([[0., -k[2], k[1]], [k[2], 0., -k[0]], [-k[1], k[0], 0.]])
    return np.cos(theta0) * np.eye(3) + np.sin(theta0) * Kx + (1. - np.cos(theta0)) * np.outer(k, k)


def model_axes(o, lat, lon, alt):
    """(P, 3, 3): row c = the unit vector r', theta', phi' of the rotated spherical coordinates at the point, in ECEF."""
    _, th, ph = o.transform_coord(np.ravel(lat), np.ravel(lon), np.ravel(alt))
    st, ct, sp_, cp = np.sin(th), np.cos(th), np.sin(ph), np.cos(ph)
    E = np.stack([np.stack([st * cp, st * sp_, ct], axis=1),
                  np.stack([ct * cp, ct * sp_, -st], axis=1),
                  np.stack([-sp_, cp, np.zeros_like(ct)], axis=1)], axis=1)         # in the rotated frame
    return E @ rotation(o)                                                           # rows times Rot = Rot^T applied


def enu_axes(lat, lon):
    """(P, 3, 3): row i = the geodetic unit vector east, north, up (the ellipsoid's normal) at the point, in ECEF."""
    la, lo = np.radians(np.ravel(lat)), np.radians(np.ravel(lon))
    sl, cl, so, co = np.sin(la), np.cos(la), np.sin(lo), np.cos(lo)
    zero = np.zeros_like(sl)
    return np.stack([np.stack([-so, co, zero], axis=1),
                     np.stack([-sl * co, -sl * so, cl], axis=1),
                     np.stack([cl * co, cl * so, sl], axis=1)], axis=1)


def enu_frame(o, lat, lon, alt):
    """(P, 3, 3) matrices F with v_enu = F v_model: what Model.gradient_frame gives."""
    return enu_axes(lat, lon) @ model_axes(o, lat, lon, alt).transpose(0, 2, 1)


def turn(packed, F):
    """F H F^T of packed Hessians: packed (P, 6, N), F (P, 3, 3) -> (P, 6, N)."""
    H = np.empty((packed.shape[0], 3, 3, packed.shape[2]))
    for k, (c, d) in enumerate(PAIRS):
        H[:, c, d] = H[:, d, c] = packed[:, k]
    Ht = np.einsum('pic,pcdn,pjd->pijn', F, H, F)
    return np.stack([Ht[:, c, d] for c, d in PAIRS], axis=1)


def _factors(o, n, z, x, y, phi):
    """(g0, g1, g2, T, T', T'', A, A', A'', nu) of basis function n at the points."""
    k, l, m = o.basis_numbers(n)
    v = o.nu(n)
    a = 100. / RE
    e = np.exp(-0.5 * z)
    L0 = sp.eval_laguerre(k, z)
    L1 = sp.eval_genlaguerre(k - 1, 1, z) if k >= 1 else np.zeros_like(z)
    L2 = sp.eval_genlaguerre(k - 2, 2, z) if k >= 2 else np.zeros_like(z)
    g0 = e * L0
    g1 = -0.5 * e * (L0 + 2. * L1) * a
    g2 = e * (0.25 * L0 + L1 + L2) * a * a
    T = sp.lpmv(m, v, x)
    T1 = sp.lpmv(m, v + 1, x)
    Tp = (-(v + 1) * x * T + (v - m + 1) * T1) / y
    Tpp = -(x / y) * Tp - (v * (v + 1) - m * m / y**2) * T
    A = o.Az(v, m, phi)
    return g0, g1, g2, T, Tp, Tpp, A, o.dAz(v, m, phi), -m * m * A, v


def hess_basis(o, lat, lon, alt, frame='model'):
    """The Hessian basis of the oracle's model at 1-D points: (P, 6, N), packed in PAIRS order, frame 'model' or 'enu'."""
    lat, lon, alt = (np.asarray(a, dtype=np.float64).ravel() for a in (lat, lon, alt))
    z, theta, phi = o.transform_coord(lat, lon, alt)
    x, y = np.cos(theta), np.sin(theta)
    r = RE * (z / 100. + 1.)
    out = np.empty((lat.size, 6, o.nbasis))
    with np.errstate(all='ignore'):
        for n in range(o.nbasis):
            g0, g1, g2, T, Tp, Tpp, A, Ap, App, v = _factors(o, n, z, x, y, phi)
            gd = g1 / r - g0 / r**2
            out[:, 0, n] = g2 * T * A
            out[:, 1, n] = g0 * Tpp * A / r**2 + g1 * T * A / r
            out[:, 2, n] = g0 * T * App / (r**2 * y**2) + g1 * T * A / r + x * g0 * Tp * A / (y * r**2)
            out[:, 3, n] = gd * Tp * A
            out[:, 4, n] = gd * T * Ap / y
            out[:, 5, n] = g0 * Ap * (Tp / y - x * T / y**2) / r**2
    if frame == 'enu':
        return turn(out, enu_frame(o, lat, lon, alt))
    if frame != 'model':
        raise ValueError(frame)
    return out


def laplacian_basis(o, lat, lon, alt):
    """The Laplacian of every basis function in closed form, (g2 + 2 g1/r - nu(nu+1) g0/r^2) T A: (P, N)."""
    lat, lon, alt = (np.asarray(a, dtype=np.float64).ravel() for a in (lat, lon, alt))
    z, theta, phi = o.transform_coord(lat, lon, alt)
    x, y = np.cos(theta), np.sin(theta)
    r = RE * (z / 100. + 1.)
    out = np.empty((lat.size, o.nbasis))
    with np.errstate(all='ignore'):
        for n in range(o.nbasis):
            g0, g1, g2, T, _, _, A, _, _, v = _factors(o, n, z, x, y, phi)
            out[:, n] = (g2 + 2. * g1 / r - v * (v + 1) * g0 / r**2) * T * A
    return out


def colnorm_err6(H, Href):
    """Per basis function, the largest |H - Href| over points and entries relative to the largest |Href|: (N,)."""
    scale = np.max(np.abs(Href), axis=(0, 1))
    scale[scale == 0] = 1.
    return np.max(np.abs(H - Href), axis=(0, 1)) / scale
