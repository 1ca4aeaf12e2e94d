"""The host side of Estimate.slant (line integrals along straight rays), no GPU: geodesy.ecef2geodetic, estimate.hull_chords - the
host statement of the clip kernel K2l makes (vi_eval_slant_f64) - and the argument errors slant raises before it touches a device."""
import functools

import numpy as np
import pytest

from conftest import load_golden

EPS = np.finfo(np.float64).eps


def test_ecef2geodetic_round_trip():
    """2e6 points from 10 km below the ellipsoid to 30 000 km above it, the poles, the equator and lon = +-180 among them:
    geodetic2ecef(ecef2geodetic(x)) is within 8 eps |x| of x for every point (a Bowring start with two fixed-point iterations
    measures 3.3 eps |x| on this set; the factor 8 leaves a sound alternative algorithm a couple of ulps), and the latitude comes
    back within 1e-12 degrees away from the poles."""
    from volumetricinterp_amd import geodesy
    rng = np.random.default_rng(0)
    n = 2_000_000
    lat, lon, alt = rng.uniform(-90, 90, n), rng.uniform(-180, 180, n), rng.uniform(-1e4, 3e7, n)
    special = [(90, 0, 0), (-90, 10, 0), (90, 77, -1e4), (-90, -77, -1e4), (90, 180, 3e7), (-90, -180, 3e7), (0, 0, 0), (0, 180, 0),
               (0, -180, 0), (0, 90, -1e4), (0, -90, 3e7), (45, 180, 1e6), (-45, -180, 1e6), (89.999999, 5, 3e5), (-89.999999, 5, 3e5)]
    for i, (la, lo, al) in enumerate(special):
        lat[i], lon[i], alt[i] = la, lo, al
    x = np.array(geodesy.geodetic2ecef(lat, lon, alt))
    la, lo, al = geodesy.ecef2geodetic(*x)
    assert la.shape == lo.shape == al.shape == (n,)
    y = np.array(geodesy.geodetic2ecef(la, lo, al))
    err = np.linalg.norm(y - x, axis=0) / np.linalg.norm(x, axis=0) / EPS
    print('round trip: max %.2f eps |x|' % err.max())
    assert err.max() <= 8., err.max()
    away = np.abs(lat) < 89.9
    assert np.abs(la - lat)[away].max() <= 1e-12
    assert np.all(np.abs(la) <= 90.) and np.all(np.abs(lo) <= 180.)
    # the shape is kept, scalars included
    g = geodesy.ecef2geodetic(x[0][:24].reshape(2, 3, 4), x[1][:24].reshape(2, 3, 4), x[2][:24].reshape(2, 3, 4))
    assert all(v.shape == (2, 3, 4) for v in g) and np.array_equal(g[0].ravel(), la[:24])
    assert all(np.shape(v) == () for v in geodesy.ecef2geodetic(x[0][20], x[1][20], x[2][20]))


@functools.lru_cache(maxsize=None)
def _hull():
    from volumetricinterp_amd.estimate import hull_equations
    eq, tol = hull_equations(load_golden('fit_k8l2')['hull_vert'])
    assert eq.shape == (460, 4)
    return eq, tol


def _segments(rng, P):
    """Random segments about the hull of the fixtures: from the ground below it to 1000 km above it (two thirds enter it)."""
    from volumetricinterp_amd import geodesy
    a = np.array(geodesy.geodetic2ecef(rng.uniform(75, 81, P), rng.uniform(250, 274, P), np.zeros(P))).T
    b = np.array(geodesy.geodetic2ecef(rng.uniform(72, 84, P), rng.uniform(240, 284, P), np.full(P, 1000e3))).T
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def _inside(eq, tol, x):
    return np.all(x @ eq[:, :3].T + eq[:, 3] <= tol, axis=-1)


def test_hull_chords_against_the_point_test():
    """1000 random segments, 200 samples of [0, 1] on each: a sample is inside the hull - by the point test of hull_equations -
    exactly when s0 <= s <= s1 (samples within 1e-9 of s0 or s1 excluded); a miss returns NaNs."""
    from volumetricinterp_amd.estimate import hull_chords
    eq, tol = _hull()
    rng = np.random.default_rng(5)
    a, b = _segments(rng, 1000)
    s0, s1 = hull_chords(eq, tol, a, b)
    assert s0.shape == s1.shape == (1000,)
    hit = ~np.isnan(s0)
    assert np.array_equal(np.isnan(s1), ~hit) and 0 < hit.sum() < 1000
    assert np.all((0. <= s0[hit]) & (s0[hit] < s1[hit]) & (s1[hit] <= 1.))
    s = np.sort(rng.uniform(0., 1., (1000, 200)), axis=1)
    s[:, 0], s[:, -1] = 0., 1.
    x = a[:, None, :] + s[:, :, None] * (b - a)[:, None, :]
    inside = _inside(eq, tol, x)
    with np.errstate(invalid='ignore'):
        expected = (s >= s0[:, None]) & (s <= s1[:, None])                  # all False for a miss
        judged = ~((np.abs(s - s0[:, None]) < 1e-9) | (np.abs(s - s1[:, None]) < 1e-9))
    assert judged.sum() > 0.99 * judged.size
    assert np.array_equal(inside[judged], expected[judged])
    assert not inside[~hit].any() and inside[hit].any(axis=1).sum() > 0.9 * hit.sum()      # (a short chord may hold no sample)


def test_hull_chords_inside_outside_and_non_finite():
    from volumetricinterp_amd.estimate import hull_chords
    eq, tol = _hull()
    rng = np.random.default_rng(6)
    a, b = _segments(rng, 400)
    s0, s1 = hull_chords(eq, tol, a, b)
    hit = ~np.isnan(s0)
    # two points inside: the interior points of chords
    u, v = rng.uniform(0.05, 0.95, (2, hit.sum()))
    pa = a[hit] + (s0[hit] + (s1[hit] - s0[hit]) * u)[:, None] * (b - a)[hit]
    pb = np.roll(a[hit] + (s0[hit] + (s1[hit] - s0[hit]) * v)[:, None] * (b - a)[hit], 1, axis=0)
    both = _inside(eq, tol, pa) & _inside(eq, tol, pb)
    assert both.sum() > 100
    t0, t1 = hull_chords(eq, tol, pa[both], pb[both])
    assert np.array_equal(t0, np.zeros(both.sum())) and np.array_equal(t1, np.ones(both.sum()))
    # a segment of length zero inside is a chord (0, 1); outside it is a miss
    z0, z1 = hull_chords(eq, tol, pa[both][:3], pa[both][:3])
    assert np.array_equal(z0, np.zeros(3)) and np.array_equal(z1, np.ones(3))
    assert np.isnan(hull_chords(eq, tol, a[:3], a[:3])[0]).all()             # (the ground is below the hull)
    # non-finite end points
    for bad in (np.nan, np.inf, -np.inf):
        for side in (0, 1):
            for comp in range(3):
                ends = [pa[both][:2].copy(), pb[both][:2].copy()]
                ends[side][0, comp] = bad
                n0, n1 = hull_chords(eq, tol, *ends)
                assert np.isnan(n0[0]) and np.isnan(n1[0]) and (n0[1], n1[1]) == (0., 1.)
    # no facet: the whole segment; no segment: nothing
    e0, e1 = hull_chords(np.zeros((0, 4)), 0., a[:5], b[:5])
    assert np.array_equal(e0, np.zeros(5)) and np.array_equal(e1, np.ones(5))
    assert hull_chords(eq, tol, np.zeros((0, 3)), np.zeros((0, 3)))[0].shape == (0,)
    with pytest.raises(ValueError, match='shape'):
        hull_chords(eq, tol, a[:5], b[:4])


def _estimate():
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_k8l2')
    return Estimate.from_arrays(f['Coeffs'], f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))


def test_slant_argument_errors_need_no_device():
    """Every ValueError of Estimate.slant is raised before a device is asked for (Estimate.from_arrays builds without one)."""
    es = _estimate()
    t = float(np.mean(es.time[0]))
    a, b = (78., 262., 0.), (78., 262., 1000e3)
    with pytest.raises(ValueError, match='coords must be'):
        es.slant(t, a, b, coords='enu')
    for nodes in (0, 257, -1, 2.5, True, None):
        with pytest.raises(ValueError, match='nodes must be'):
            es.slant(t, a, b, nodes=nodes)
    for rule in (([0., 1.], [1.]), ([], []), (np.zeros((2, 2)), np.zeros((2, 2))), (np.zeros(65537), np.zeros(65537)), 3., ([0.],),
                 (['a'], ['b'])):
        with pytest.raises(ValueError, match='rule must be a pair'):
            es.slant(t, a, b, rule=rule)
    for rule in (([np.nan], [2.]), ([0.], [np.inf])):
        with pytest.raises(ValueError, match='rule must be finite'):
            es.slant(t, a, b, rule=rule)
    with pytest.raises(ValueError, match='do not broadcast'):
        es.slant(t, (np.zeros(3), 262., 0.), (np.zeros(4), 262., 1e6))
    for start in ((78., 262.), 78., None):
        with pytest.raises(ValueError, match='triple'):
            es.slant(t, start, b)
    with pytest.raises(ValueError, match='times must be'):
        es.slant(np.full(3, t), (np.full(4, 78.), 262., 0.), b)
    with pytest.raises(ValueError, match='out must be'):
        es.slant(t, (np.full(4, 78.), 262., 0.), b, out=np.empty(5))
    with pytest.raises(ValueError, match='outside must be'):
        es.slant(t, a, b, outside='zero')
    with pytest.raises(ValueError) as e:
        es.slant(t + 1e9, a, b)
    assert str(e.value) == 'Requested time out of range of data file.'
    # no ray: nothing to compute, no device
    assert es.slant(t, (np.zeros((0, 2)), 262., 0.), b).shape == (0, 2)
    out = es.slant(np.zeros(0), (np.zeros(0), 262., 0.), b, chord=True)
    assert len(out) == 3 and all(v.shape == (0,) and v.dtype == np.float64 for v in out)


def test_slant_rule():
    from volumetricinterp_amd.estimate import slant_rule
    x, w = slant_rule(64)
    gx, gw = np.polynomial.legendre.leggauss(64)
    assert np.array_equal(x, gx) and np.array_equal(w, gw) and x.flags.c_contiguous
    x, w = slant_rule(7, rule=([0.], [2.]))             # nodes is ignored
    assert x.tolist() == [0.] and w.tolist() == [2.] and x.dtype == np.float64
    assert slant_rule(1)[0].shape == (1,) and slant_rule(256)[0].shape == (256,)
