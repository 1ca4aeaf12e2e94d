"""Model.gradient_frame (models/sphharmlag.py): the per-point 3 x 3 matrices that turn a gradient along the model coordinates
(z, theta, phi of the rotated cap, what grad_basis and Estimate.gradient give) into local east, north, up.  No GPU.

The check is independent of the frame mathematics: the oracle's gradient, rotated by the matrices, against central finite
differences of the oracle's own density along geodetic east, north and up at a 10 m step.  The oracle alone meets 1.03e-9
(MAXK 8 x MAXL 2) and 1.11e-9 (default order) norm-wise - the truncation error of the differences, which converges as h^2
(2.6e-8 / 2.7e-8 at 50 m) and is deterministic, so the 1e-8 gate is nine times that and no more: a swapped or sign-flipped
axis is off by O(1), a radial `up` in place of the geodetic normal by 1e-3."""
import io

import numpy as np
import pytest

from conftest import load_golden, rel

WGS84_A = 6378137.0
WGS84_B = 6356752.31424518
FD_STEP = 10.                   # metres
FD_TOL = 1e-8


def frame_points():
    """The 60 points of the check: latitude, longitude, altitude drawn in that order."""
    rng = np.random.default_rng(5)
    return rng.uniform(75, 81, 60), rng.uniform(250, 274, 60), rng.uniform(150e3, 600e3, 60)


def enu_finite_differences(o, C, lat, lon, alt, h=FD_STEP):
    """(P, 3) central differences of the oracle's density along east, north and up, per metre."""
    import oracle
    e2 = 1. - (WGS84_B / WGS84_A)**2
    s2 = np.sin(np.radians(lat))**2
    Mphi = WGS84_A * (1. - e2) / (1. - e2 * s2)**1.5                    # meridional radius of curvature
    Nphi = WGS84_A / np.sqrt(1. - e2 * s2)                              # prime-vertical radius
    dlat = np.degrees(h / (Mphi + alt))
    dlon = np.degrees(h / ((Nphi + alt) * np.cos(np.radians(lat))))
    f = lambda a, b, c: oracle.evaluate(o, C, a, b, c)
    return np.stack([(f(lat, lon + dlon, alt) - f(lat, lon - dlon, alt)) / (2. * h),
                     (f(lat + dlat, lon, alt) - f(lat - dlat, lon, alt)) / (2. * h),
                     (f(lat, lon, alt + h) - f(lat, lon, alt - h)) / (2. * h)], axis=1)


def _model_and_oracle(tag):
    import oracle
    from volumetricinterp_amd.models.sphharmlag import Model
    f = load_golden('fit_' + tag)
    m = Model(io.StringIO(str(f['cfg'])))
    o = oracle.SphHarmLagOracle(maxk=m.maxk, maxl=m.maxl)
    return m, o, np.nan_to_num(f['Coeffs'])[0]


@pytest.mark.parametrize('tag', ['k8l2', 'default'])
def test_gradient_frame_orthonormal_and_physical(tag):
    import oracle
    m, o, C = _model_and_oracle(tag)
    lat, lon, alt = frame_points()
    M = m.gradient_frame(lat, lon, alt)
    assert M.shape == (60, 3, 3)
    orth = float(np.max(np.abs(M @ M.transpose(0, 2, 1) - np.eye(3))))
    g = np.einsum('pic,pc->pi', M, oracle.evaluate_gradient(o, C, lat, lon, alt))
    fd = enu_finite_differences(o, C, lat, lon, alt)
    err = rel(g, fd)
    print('%s: |M M^T - I| %.1e, rotated gradient against finite differences %.2e' % (tag, orth, err))
    assert orth <= 1e-14
    assert np.all(np.linalg.det(M) > 0.)                                # a rotation, not a reflection
    assert err <= FD_TOL


def test_gradient_frame_shapes():
    m, _, _ = _model_and_oracle('k8l2')
    assert m.gradient_frame(np.zeros(0), np.zeros(0), np.zeros(0)).shape == (0, 3, 3)
    lat, lon, alt = frame_points()
    M = m.gradient_frame(lat.reshape(6, 10), lon.reshape(6, 10), alt.reshape(6, 10))     # inputs of any shape, raveled
    assert np.array_equal(M, m.gradient_frame(lat, lon, alt))
