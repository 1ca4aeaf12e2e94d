"""The reference of the Hessian tests (tests/hessian_ref.py) held against exact arithmetic and against the oracle.  No GPU.

The reference project has no second derivatives, so the yardsticks are (1) the same closed forms in 50-digit mpmath arithmetic
- legenp at real degree, the generalised laguerre, the coordinate transform and the frame in mpmath too - which bounds the
rounding error E_REF of the float64 restatement, and (2) second central differences of the oracle's own basis along straight
lines, which know nothing of the formulas."""
import io

import numpy as np
import pytest

import hessian_ref as hr
from conftest import load_golden

CONFIGS = ['default', 'k3l4cap15', 'k2l5cap12p7']       # the configurations of tests/golden/grad_sph.npz

# Largest column-norm relative error of hessian_ref.hess_basis against the 50-digit evaluation over the points of
# test_restatement_vs_mpmath, as measured when the test was written (model frame / enu frame):
#   default 2.20e-13 / 2.20e-13, k3l4cap15 1.49e-13 / 1.49e-13, k2l5cap12p7 7.11e-14 / 7.25e-14
# (SciPy's lpmv series at nu = 94 is the largest part).  E_REF is the largest of them rounded up to the next digit, so that the
# last digits of another SciPy build do not fail the test; tests/test_gpu_hessian.py takes its device bound,
# max(1e-11, 8 E_REF) = 1e-11, from it.
E_REF = 3e-13


def _oracle(cfg):
    import oracle
    return oracle.SphHarmLagOracle(maxk=int(cfg[0]), maxl=int(cfg[1]), cap_lim_deg=float(cfg[2]))


def _points(tag, theta_min):
    """The points of the golden file whose rotated colatitude is at least theta_min (rad)."""
    g = load_golden('grad_sph')
    o = _oracle(g[tag + '_cfg'])
    lat, lon, alt = g[tag + '_lat'], g[tag + '_lon'], g[tag + '_alt']
    _, th, _ = o.transform_coord(lat, lon, alt)
    ok = th >= theta_min
    return o, lat[ok], lon[ok], alt[ok]


def mp_hess_basis(o, lat, lon, alt):
    """hessian_ref's formulas in 50-digit arithmetic from the float64 coordinates on: (P, 6, N) in both frames, as float64."""
    import mpmath as mp
    from oracle.geodesy import WGS84_A, WGS84_B
    from oracle.sphharmlag import RE
    mp.mp.dps = 50
    A_, B_, RE_ = mp.mpf(WGS84_A), mp.mpf(WGS84_B), mp.mpf(RE)

    def ecef(la, lo, al):
        la, lo = mp.radians(mp.mpf(float(la))), mp.radians(mp.mpf(float(lo)))
        al = mp.mpf(float(al))
        N = A_**2 / mp.sqrt(A_**2 * mp.cos(la)**2 + B_**2 * mp.sin(la)**2)
        return mp.matrix([(N + al) * mp.cos(la) * mp.cos(lo), (N + al) * mp.cos(la) * mp.sin(lo), (N * (B_ / A_)**2 + al) * mp.sin(la)])

    c0 = ecef(o.latcp, o.loncp, 0.)
    theta0 = mp.acos(c0[2] / mp.norm(c0))
    phi0 = mp.atan2(c0[1], c0[0])
    k = mp.matrix([mp.cos(phi0 + mp.pi / 2), mp.sin(phi0 + mp.pi / 2), 0])
    Kx = mp.matrix([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Rot = mp.cos(theta0) * mp.eye(3) + mp.sin(theta0) * Kx + (1 - mp.cos(theta0)) * (k * k.T)
    a = 100 / RE_
    N = o.nbasis
    out = {f: np.empty((len(lat), 6, N)) for f in ('model', 'enu')}
    for p in range(len(lat)):
        R = Rot * ecef(lat[p], lon[p], alt[p])
        r = mp.norm(R)
        x = R[2] / r
        y = mp.sqrt(R[0]**2 + R[1]**2) / r
        phi = mp.atan2(R[1], R[0])
        z = 100 * (r / RE_ - 1)
        e = mp.exp(-z / 2)
        la, lo = mp.radians(mp.mpf(float(lat[p]))), mp.radians(mp.mpf(float(lon[p])))
        enu = mp.matrix([[-mp.sin(lo), mp.cos(lo), 0], [-mp.sin(la) * mp.cos(lo), -mp.sin(la) * mp.sin(lo), mp.cos(la)],
                         [mp.cos(la) * mp.cos(lo), mp.cos(la) * mp.sin(lo), mp.sin(la)]])
        cp, sp_ = mp.cos(phi), mp.sin(phi)
        E = mp.matrix([[y * cp, y * sp_, x], [x * cp, x * sp_, -y], [-sp_, cp, 0]]) * Rot
        F = enu * E.T
        leg = {}
        for n in range(N):
            kk, l, m = o.basis_numbers(n)
            kk, l, m = int(kk), int(l), int(m)
            v = mp.mpf(float(o.nu(n)))           # the oracle's float64 degree, exact from here on
            if (l, m) not in leg:
                leg[l, m] = (mp.legenp(v, m, x, type=2), mp.legenp(v + 1, m, x, type=2))
            T, T1 = leg[l, m]
            am = abs(m)
            K = mp.sqrt((2 * v + 1) / (4 * mp.pi) * mp.gamma(v - am + 1) / mp.gamma(v + am + 1)) * (mp.sqrt(2) if m else 1)
            Az = K * (mp.sin(am * phi) if m < 0 else mp.cos(am * phi))
            dAz = am * K * mp.cos(am * phi) if m < 0 else -m * K * mp.sin(am * phi)
            L0 = mp.laguerre(kk, 0, z)
            L1 = mp.laguerre(kk - 1, 1, z) if kk >= 1 else mp.mpf(0)
            L2 = mp.laguerre(kk - 2, 2, z) if kk >= 2 else mp.mpf(0)
            g0, g1, g2 = e * L0, -e * (L0 + 2 * L1) * a / 2, e * (L0 / 4 + L1 + L2) * a * a
            Tp = (-(v + 1) * x * T + (v - m + 1) * T1) / y
            Tpp = -(x / y) * Tp - (v * (v + 1) - m * m / y**2) * T
            gd = g1 / r - g0 / r**2
            h = [g2 * T * Az, g0 * Tpp * Az / r**2 + g1 * T * Az / r,
                 -g0 * T * m * m * Az / (r * y)**2 + g1 * T * Az / r + x * g0 * Tp * Az / (y * r**2),
                 gd * Tp * Az, gd * T * dAz / y, g0 * dAz * (Tp / y - x * T / y**2) / r**2]
            H = mp.matrix([[h[0], h[3], h[4]], [h[3], h[1], h[5]], [h[4], h[5], h[2]]])
            He = F * H * F.T
            for q, (c, d) in enumerate(hr.PAIRS):
                out['model'][p, q, n] = float(H[c, d])
                out['enu'][p, q, n] = float(He[c, d])
    return out


@pytest.mark.parametrize('tag', CONFIGS)
def test_restatement_vs_mpmath(tag):
    """hessian_ref.hess_basis against the same closed forms in 50-digit mpmath arithmetic (legenp at real degree with the
    signed order, laguerre, the transform and the frame) at 30 points of the golden file, every basis function, both frames:
    the largest column-norm relative error, E_REF, is the rounding error of the float64 restatement - the reference error the
    device's bound in tests/test_gpu_hessian.py is built on.  Measured: the table at E_REF above."""
    o, lat, lon, alt = _points(tag, np.radians(0.5))
    lat, lon, alt = lat[:30], lon[:30], alt[:30]
    assert lat.size == 30
    exact = mp_hess_basis(o, lat, lon, alt)
    for frame in ('model', 'enu'):
        H = hr.hess_basis(o, lat, lon, alt, frame)
        assert np.isfinite(H).all() and np.isfinite(exact[frame]).all()
        err = hr.colnorm_err6(H, exact[frame])
        print('%s %s: E_ref %.2e (function %d)' % (tag, frame, float(err.max()), int(err.argmax())))
        assert err.max() <= E_REF, (tag, frame, float(err.max()), int(err.argmax()))


def second_differences(o, C, X0, u, h):
    """Second central differences of the oracle's basis @ C along the straight lines X0 + s u (ECEF metres, unit u): (P,)."""
    from volumetricinterp_amd.geodesy import ecef2geodetic
    f = [o.basis(*ecef2geodetic(*(X0 + s * u).T)) @ C for s in (-h, 0., h)]
    return (f[0] - 2. * f[1] + f[2]) / (h * h)


@pytest.mark.parametrize('tag', CONFIGS)
def test_restatement_vs_finite_differences(tag):
    """u^T H u of the restatement, contracted with random coefficients, against second central differences of the oracle's
    own basis along straight ECEF lines, three random directions per point, points with theta' >= 0.01 rad, both frames
    (directions expressed along the model axes and along east, north, up).  The scheme is of second order: halving the step
    from 2 km to 1 km divides the error by 4 (ratio within [3.9, 4.1]), and at 1 km the error is at most 1e-3 of the largest
    entry - the truncation error (h nu_max / r)^2 / 12 is about 2e-5 of it at nu = 94.  Measured: ratios 3.9997 to 4.0003,
    at 1 km at most 5.2e-5 of the largest entry (default configuration, model frame)."""
    from oracle.geodesy import geodetic2ecef
    o, lat, lon, alt = _points(tag, 0.01)
    assert lat.size >= 30
    rng = np.random.default_rng(11)
    A = o.basis(lat, lon, alt)
    C = rng.standard_normal(o.nbasis) / np.max(np.abs(A), axis=0)            # every function contributes alike
    X0 = np.stack(geodetic2ecef(lat, lon, alt), axis=1)
    axes = {'model': hr.model_axes(o, lat, lon, alt), 'enu': hr.enu_axes(lat, lon)}
    for frame in ('model', 'enu'):
        packed = hr.hess_basis(o, lat, lon, alt, frame) @ C                      # (P, 6)
        H = np.empty((lat.size, 3, 3))
        for k, (c, d) in enumerate(hr.PAIRS):
            H[:, c, d] = H[:, d, c] = packed[:, k]
        big = float(np.max(np.abs(H)))
        for _ in range(3):
            w = rng.standard_normal((lat.size, 3))
            w /= np.linalg.norm(w, axis=1)[:, None]                              # components in the frame
            u = np.einsum('pc,pcx->px', w, axes[frame])                          # the same direction in ECEF
            exact = np.einsum('pc,pcd,pd->p', w, H, w)
            e2 = float(np.max(np.abs(second_differences(o, C, X0, u, 2000.) - exact)))
            e1 = float(np.max(np.abs(second_differences(o, C, X0, u, 1000.) - exact)))
            print('%s %s: error at 2 km %.3e, at 1 km %.3e of the largest entry, ratio %.4f' % (tag, frame, e2 / big, e1 / big, e2 / e1))
            assert 3.9 <= e2 / e1 <= 4.1, (tag, frame, e2 / e1)
            assert e1 <= 1e-3 * big, (tag, frame, e1 / big)


@pytest.mark.parametrize('tag', CONFIGS)
def test_trace_is_the_laplacian(tag):
    """The first three packed entries add up to the closed-form Laplacian (g2 + 2 g1/r - nu(nu+1) g0/r^2) T A, and the two
    frames have equal traces: to 1e-14 of the function's largest Hessian entry over the points."""
    o, lat, lon, alt = _points(tag, np.radians(0.5))
    Hm = hr.hess_basis(o, lat, lon, alt, 'model')
    He = hr.hess_basis(o, lat, lon, alt, 'enu')
    lap = hr.laplacian_basis(o, lat, lon, alt)
    scale = np.max(np.abs(Hm), axis=(0, 1))
    assert np.all(scale > 0)
    assert np.max(np.abs(Hm[:, :3].sum(axis=1) - lap) / scale) <= 1e-14
    assert np.max(np.abs(He[:, :3].sum(axis=1) - Hm[:, :3].sum(axis=1)) / scale) <= 1e-14


def test_frame_is_the_models():
    """hessian_ref.enu_frame restates Model.gradient_frame (pure NumPy there too)."""
    from volumetricinterp_amd.models.sphharmlag import Model
    o, lat, lon, alt = _points('default', 0.)
    m = Model(io.StringIO('[DEFAULT]\n[MODEL]\nNAME = sphharmlag\nMAXK = 4\nMAXL = 6\nCAP_LIM = 10\nMAX_Z_INT = INF\n'
                          'LATCP = 78\nLONCP = 262\n'))
    assert np.max(np.abs(hr.enu_frame(o, lat, lon, alt) - m.gradient_frame(lat, lon, alt))) <= 1e-14


def test_packed_order_and_symmetry():
    """gradcov_matrix of a packed Hessian: symmetric, entry (c, d) from plane GRADCOV_PAIRS.index((c, d)) - the order of
    hessian_ref.PAIRS and of the library."""
    from volumetricinterp_amd.estimate import GRADCOV_PAIRS, gradcov_matrix
    assert tuple(GRADCOV_PAIRS) == hr.PAIRS
    packed = np.arange(2 * 6 * 5, dtype=np.float64).reshape(2, 6, 5)
    H = gradcov_matrix(packed)
    assert H.shape == (2, 5, 3, 3) and np.array_equal(H, H.transpose(0, 1, 3, 2))
    for k, (c, d) in enumerate(GRADCOV_PAIRS):
        assert np.array_equal(H[..., c, d], packed[:, k])
    o, lat, lon, alt = _points('k3l4cap15', np.radians(0.5))
    Hb = gradcov_matrix(hr.hess_basis(o, lat[:4], lon[:4], alt[:4]).transpose(1, 0, 2).reshape(6, -1))
    assert np.array_equal(Hb, Hb.transpose(0, 2, 1))
