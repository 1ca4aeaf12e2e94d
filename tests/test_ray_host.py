"""Host tests of the searches along straight rays (no GPU): the NumPy mirror of the two device iterations (tests/ray_ref.py)
against scipy.optimize.brentq on the mirror's own slope and value, on vertical rays against the column mirrors
(tests/peak_ref.py, tests/level_ref.py), its slope and curvature against central differences of the oracle's value along the
line; and the host helpers of estimate.py: ray_points, ray_samples, ray_peak_brackets, ray_level_brackets.

The rays of the layer tests (shared with tests/test_gpu_ray.py): sixteen beams from a ground site at (77.0, 262.0) - 111 km
south of the pole of the cap, where the beams of the fitted geometry start -, elevations 30 to 85 degrees in equal steps, the
azimuths 300, 330, 30 and 60 degrees in turn; ray k runs from the range 150 km / sin(el) to the range 450 km / sin(el), about
150 to 450 km of altitude."""
import functools

import numpy as np
import pytest
from scipy.optimize import brentq

import ray_ref as rr
from test_level_host import level_searches
from test_peak_host import HI, LO, TOL, layer, layer_searches

SITE = (77.0, 262.0)
ELEVATIONS = np.linspace(30., 85., 16)
AZIMUTHS = np.tile([300., 330., 30., 60.], 4)
FRACTIONS = (0.5, 0.8)
NEAR = 1000.        # brentq's bracket about a returned distance, metres


def beam_ends(site, el, az, r0, r1):
    """(a, b), (P, 3) each in ECEF metres: the points at the ranges r0 and r1 of the beams of elevation el and azimuth az
    (degrees, east of north) from the ground site (gdlat, gdlon) at altitude 0."""
    from volumetricinterp_amd import geodesy
    import hessian_ref as hr
    el, az = np.radians(np.atleast_1d(el)), np.radians(np.atleast_1d(az))
    enu = np.stack([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)], axis=1)
    d = enu @ hr.enu_axes([site[0]], [site[1]])[0]                      # rows east, north, up in ECEF
    X0 = np.array(geodesy.geodetic2ecef(site[0], site[1], 0.)).reshape(1, 3)
    return X0 + np.asarray(r0)[:, None] * d, X0 + np.asarray(r1)[:, None] * d


@functools.lru_cache(maxsize=None)
def rays():
    """(a, b, length) of the sixteen rays."""
    sn = np.sin(np.radians(ELEVATIONS))
    a, b = beam_ends(SITE, ELEVATIONS, AZIMUTHS, 150e3 / sn, 450e3 / sn)
    length = rr.lines(a, b)[1]
    for v in (a, b, length):
        v.setflags(write=False)
    return a, b, length


@functools.lru_cache(maxsize=None)
def ray_searches(case):
    """The mirror's searches on the sixteen rays: (peak arguments (start, lo, hi), peak result, level arguments (ray index,
    level, lo, hi), level result).  The peak search starts from the middle of the ray, in the bracket [0, length]; the level
    searches are those of every ray with an interior peak (status 0), at 0.5 and 0.8 of the peak value, before the peak
    (0, s_peak) and behind it (s_peak, length) - four per ray, ray-major, then fraction, then side.
    (A start from which Newton's last step falls below one ulp of the distance is no reference for the iteration count: the
    step lands on the iterate itself, not strictly inside the bracket, and whether the search then bisects depends on the sign
    of the rounding noise of a slope that is zero to rounding.  From the largest of 13 samples ray 12 at MAXK 8 x MAXL 2 is
    such a case - the mirror itself counts 7 iterations with the sixteen rays in one batch and 4 with the ray alone;
    test_mirror_counts_do_not_depend_on_the_batch holds the cases used here free of it.)"""
    o, C = layer(case)
    a, b, length = rays()
    start = 0.5 * length
    lo, hi = np.zeros(16), length.copy()
    peak = rr.peak_search(o, C, a, b, start, lo, hi, 1, TOL, 48)
    k = np.flatnonzero(peak['status'] == 0)
    ray = np.repeat(k, 4)
    level = (peak['f'][k][:, None, None] * np.array(FRACTIONS)[None, :, None] * np.ones((1, 1, 2))).ravel()
    l_lo = np.stack((np.zeros(k.size), peak['s'][k]), axis=1)[:, None, :].repeat(2, axis=1).ravel()
    l_hi = np.stack((peak['s'][k], length[k]), axis=1)[:, None, :].repeat(2, axis=1).ravel()
    lev = rr.level_search(o, C, a[ray], b[ray], level, l_lo, l_hi, TOL, 48)
    out = (start, lo, hi), peak, (ray, level, l_lo, l_hi), lev
    for v in (start, lo, hi, ray, level, l_lo, l_hi) + tuple(peak.values()) + tuple(lev.values()):
        v.setflags(write=False)
    return out


@pytest.mark.parametrize('case', ['k8l2', 'default'])
def test_mirror_finds_the_roots_of_its_own_slope_and_value(case):
    """Both mirrors on the sixteen rays, held to the bound of tests/test_peak_host.py and tests/test_level_host.py - tol: the
    search stops after a step of at most tol, and a Newton step next to a simple zero is as long as the distance it leaves to
    first order.  Every peak with status 0 lies within tol of the zero scipy.optimize.brentq (xtol 1e-9) finds of the mirror's
    own slope within 1 km of it, where the slope falls through zero; a level search has status 0 exactly where the value minus
    the level changes sign over its bracket and 1 elsewhere, and every crossing lies within tol of brentq's zero of the mirror's
    own value within 1 km of it.  At least 8 peaks and 8 crossings per fit are found: the cases tests/test_gpu_ray.py compares.
    Measured: k8l2 16 peaks in 4 iterations each at 172.0 to 292.7 km from the start of the ray, within 3.3e-9 m of brentq, and
    64 crossings within 3.6e-9 m; default 12 peaks in 4 to 7 iterations (the four lowest beams run onto the start of the ray in
    28 or 29 steps, status 1) within 6.9e-5 m and 41 of 48 crossings within 2.5e-4 m."""
    o, C = layer(case)
    a, b, length = rays()
    u = rr.lines(a, b)[0]
    (start, lo, hi), peak, (ray, level, l_lo, l_hi), lev = ray_searches(case)
    print(case, 'peak status', peak['status'], 'iterations', peak['it'])
    print(case, 'level status', lev['status'], 'iterations', lev['it'])
    found = np.flatnonzero(peak['status'] == 0)
    assert found.size >= 8 and (peak['status'] != 3).all()
    worst = 0.
    for k in found:
        slope = lambda s: float(rr.walk(o, C, a[k], u[k], [s], hess=False)[1][0])
        s = peak['s'][k]
        assert 0. < s < length[k] and peak['d2'][k] < 0.
        lo_k, hi_k = max(0., s - NEAR), min(length[k], s + NEAR)
        assert slope(lo_k) > 0. > slope(hi_k), (case, k)
        root = brentq(slope, lo_k, hi_k, xtol=1e-9, rtol=1e-15)
        worst = max(worst, abs(s - root))
        print('%s ray %2d (el %.1f az %.0f): peak at %.6f m of %.1f km, %.1e m from brentq, %d iterations, curvature %.3e'
              % (case, k, ELEVATIONS[k], AZIMUTHS[k], s, length[k] / 1e3, abs(s - root), peak['it'][k], peak['d2'][k]))
        assert abs(s - root) <= TOL, (case, k, s, root)
    print('%s: peaks within %.1e m of brentq' % (case, worst))
    worst, crossings = 0., 0
    for j in range(ray.size):
        k = ray[j]
        g = lambda s: float(rr.walk(o, C, a[k], u[k], [s], hess=False)[0][0]) - level[j]
        ga, gb = g(l_lo[j]), g(l_hi[j])
        change = (ga > 0.) != (gb > 0.) and ga != 0. and gb != 0.
        assert lev['status'][j] == (0 if change else 1), (case, j, ga, gb, lev['status'][j])
        if change:
            s = lev['s'][j]
            lo_j, hi_j = max(l_lo[j], s - NEAR), min(l_hi[j], s + NEAR)
            assert (g(lo_j) > 0.) != (g(hi_j) > 0.), (case, j)
            root = brentq(g, lo_j, hi_j, xtol=1e-9, rtol=1e-15)
            worst, crossings = max(worst, abs(s - root)), crossings + 1
            assert abs(s - root) <= TOL, (case, j, s, root)
            assert abs(lev['f'][j] - level[j]) <= abs(lev['d1'][j]) * TOL + 1e-12 * lev['vterms'][j]
    print('%s: %d of %d crossings, within %.1e m of brentq' % (case, crossings, ray.size, worst))
    assert crossings >= 8


@pytest.mark.parametrize('case', ['k8l2', 'default'])
def test_mirror_counts_do_not_depend_on_the_batch(case):
    """Every search of ray_searches run alone gives the status it has in the batch of all of them, and - where ray_ref.steady
    calls the count a reference - the iteration count: NumPy sums a batch in another order than a single row, and a count that
    hangs on the rounding of a sum is no yardstick for the device.  At MAXK 8 x MAXL 2 the counts of all 16 peaks and of 62 of
    the 64 levels are steady (rounding moves an iterate by 1e-7 m at most); at the default order, whose unregularised fit
    cancels heavily, rounding can move an iterate by 1e-3 to 1e-2 m - more than tol - and no count of a converged search is
    (the 7 steady ones are brackets without a crossing, no iteration): search 31 of the levels stops after a step of 9.4e-4 m,
    6e-5 m under tol, and counts 5 iterations in the batch and 4 alone."""
    o, C = layer(case)
    a, b, length = rays()
    (start, lo, hi), peak, (ray, level, l_lo, l_hi), lev = ray_searches(case)
    sp, sl = rr.steady(peak, o, True), rr.steady(lev, o, False)
    print('%s: steady counts: %d of 16 peaks, %d of %d levels' % (case, sp.sum(), sl.sum(), ray.size))
    if case == 'k8l2':
        assert sp.all() and sl.sum() >= 60
    for k in range(16):
        one = rr.peak_search(o, C, a[k:k + 1], b[k:k + 1], start[k], lo[k], hi[k], 1, TOL, 48)
        assert one['status'][0] == peak['status'][k] and (one['it'][0] == peak['it'][k] or not sp[k]), (case, k)
    for j in range(ray.size):
        k = ray[j]
        one = rr.level_search(o, C, a[k:k + 1], b[k:k + 1], level[j], l_lo[j], l_hi[j], TOL, 48)
        assert one['status'][0] == lev['status'][j] and (one['it'][0] == lev['it'][j] or not sl[j]), (case, j)


def test_vertical_rays_reproduce_the_column_mirrors():
    """Rays along the geodetic normal of the four columns of tests/test_peak_host.py, from 150 to 450 km: the distance plus
    150 km is the height.  The ray mirror reproduces peak_ref.peak_search (three starts per column) and level_ref.level_search
    (the 16 searches of tests/test_level_host.py) - statuses, iteration counts, and heights to 1e-6 m: the same iteration on the
    same function, the point going through ECEF and back (1e-9 m) and w = the `up` row of the frame to rounding."""
    from volumetricinterp_amd import geodesy
    o, C = layer('k8l2')
    lat, lon, start, ref = layer_searches('k8l2')
    a = np.stack(geodesy.geodetic2ecef(lat, lon, np.full(lat.size, LO)), axis=1)
    b = np.stack(geodesy.geodetic2ecef(lat, lon, np.full(lat.size, HI)), axis=1)
    length = rr.lines(a, b)[1]
    assert np.abs(length - (HI - LO)).max() <= 1e-6
    r = rr.peak_search(o, C, a, b, start - LO, 0., HI - LO, 1, TOL, 48)
    assert np.array_equal(r['status'], ref['status']) and np.array_equal(r['it'], ref['it'])
    print('peaks: distance + 150 km off the column mirror by', np.abs(r['s'] + LO - ref['h']))
    assert np.abs(r['s'] + LO - ref['h']).max() <= 1e-6
    assert np.abs(r['d2'] - ref['d2']).max() <= 1e-9 * np.abs(ref['d2']).max()
    lat, lon, level, lo, hi, ref = level_searches('k8l2')
    a = np.stack(geodesy.geodetic2ecef(lat, lon, np.full(lat.size, LO)), axis=1)
    b = np.stack(geodesy.geodetic2ecef(lat, lon, np.full(lat.size, HI)), axis=1)
    r = rr.level_search(o, C, a, b, level, lo - LO, hi - LO, TOL, 48)
    assert np.array_equal(r['status'], ref['status']) and np.array_equal(r['it'], ref['it'])
    print('levels: distance + 150 km off the column mirror by', np.abs(r['s'] + LO - ref['h']))
    assert np.abs(r['s'] + LO - ref['h']).max() <= 1e-6


def test_slope_and_curvature_against_differences_along_the_line():
    """w . grad f and w^T H w of the mirror at the middle of the sixteen rays, random coefficients at the default order (every
    function contributing alike), against first and second central differences of the oracle's value along the line: both
    schemes are of second order, so halving the step from 2 km to 1 km divides the error by 4 (ratio within [3.9, 4.1], as
    tests/test_hessian_host.py has it) - w^T H w is the second derivative along a straight line with no term in the gradient.
    Measured: both ratios 3.9999; at 1 km 2.7e-5 of the largest slope and 7.7e-6 of the largest curvature."""
    import oracle
    o = oracle.SphHarmLagOracle()
    a, b, length = rays()
    u = rr.lines(a, b)[0]
    s = 0.5 * length
    A = o.basis(*rr.points(a, u, s))
    C = np.random.default_rng(11).standard_normal(o.nbasis) / np.max(np.abs(A), axis=0)
    f0, d1, d2 = rr.walk(o, C, a, u, s)[:3]
    value = lambda t: rr.walk(o, C, a, u, s + t, hess=False)[0]
    err = {}
    for h in (2000., 1000.):
        fm, fp = value(-h), value(h)
        err[h] = (np.abs((fp - fm) / (2. * h) - d1).max(), np.abs((fm - 2. * f0 + fp) / (h * h) - d2).max())
    for k, (name, big) in enumerate((('slope', np.abs(d1).max()), ('curvature', np.abs(d2).max()))):
        ratio = err[2000.][k] / err[1000.][k]
        print('%s: error at 2 km %.3e, at 1 km %.3e of the largest, ratio %.4f' % (name, err[2000.][k] / big, err[1000.][k] / big, ratio))
        assert 3.9 <= ratio <= 4.1, (name, ratio)
        assert err[1000.][k] <= 1e-3 * big


def rays_into_hull(hull_vert, n, seed, site=(78., 262.)):
    """(a, b), (n, 3) each in ECEF metres: rays from the ground site through n points inside the hull of the vertices - random
    convex combinations of them - and as far again behind each."""
    from volumetricinterp_amd import geodesy
    hull_vert = np.asarray(hull_vert, dtype=np.float64)
    w = np.random.default_rng(seed).dirichlet(np.ones(hull_vert.shape[0]), n)
    a = np.tile(np.array(geodesy.geodetic2ecef(site[0], site[1], 0.)).reshape(1, 3), (n, 1))
    return a, a + 2. * (w @ hull_vert - a)


def _hull():
    from conftest import load_golden
    from volumetricinterp_amd.estimate import hull_equations
    v = load_golden('fit_k8l2')['hull_vert']
    return v, hull_equations(v)


def test_ray_samples_and_ray_points():
    """ray_samples on rays from a ground site into the k8l2 fixture's hull and on one that misses it: the first and the
    last distance are the chord of hull_chords pulled inside by 1e-6 of its length, the samples are equispaced, every finite
    sample passes check_hull's criterion (eq[:, :3] @ x + eq[:, 3] <= tol at the ECEF point of its geodetic coordinates), the
    missing ray is NaN throughout; ray_points gives the same geodetic points from the distances, keeps leading axes and NaN;
    coords='ecef' takes the end points as they are."""
    from volumetricinterp_amd import geodesy
    from volumetricinterp_amd.estimate import hull_chords, ray_points, ray_samples
    vert, (eq, tol) = _hull()
    a, b = rays_into_hull(vert, 35, 35)
    b[3] = a[3] + (a[3] - b[3])                                           # into the ground: a miss
    start, end = tuple(a.T.reshape(3, 5, 7)), tuple(b.T.reshape(3, 5, 7))
    dist, lat, lon, alt = ray_samples(eq, tol, start, end, 32, coords='ecef')
    assert all(v.shape == (5, 7, 32) for v in (dist, lat, lon, alt))
    s0, s1 = hull_chords(eq, tol, a, b)
    miss = np.isnan(s0).reshape(5, 7)
    assert miss[0, 3] and miss.sum() == 1
    assert all(np.isnan(v[miss]).all() and np.isfinite(v[~miss]).all() for v in (dist, lat, lon, alt))
    length = rr.lines(a, b)[1]
    c0, c1 = (s0 * length).reshape(5, 7)[~miss], (s1 * length).reshape(5, 7)[~miss]
    d = dist[~miss]
    assert np.allclose(d[:, 0], c0 + 1e-6 * (c1 - c0), rtol=1e-12, atol=1e-6)
    assert np.allclose(d[:, -1], c1 - 1e-6 * (c1 - c0), rtol=1e-12, atol=1e-6)
    assert (np.diff(d, axis=1) > 0.).all()
    assert np.allclose(d[:, 1:-1], c0[:, None] + (c1 - c0)[:, None] * np.linspace(0., 1., 32)[None, 1:-1], rtol=1e-12, atol=1e-6)
    X = np.stack(geodesy.geodetic2ecef(lat[~miss], lon[~miss], alt[~miss]), axis=-1)
    assert (X @ eq[:, :3].T + eq[:, 3] <= tol).all()
    p = ray_points(start, end, np.moveaxis(dist, -1, 0), coords='ecef')           # the samples as a leading axis
    for got, want in zip(p, (lat, lon, alt)):
        got = np.moveaxis(got, 0, -1)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.allclose(got[~miss], want[~miss], rtol=0., atol=1e-6)
    lead = ray_points(start, end, np.stack((dist[..., 5], dist[..., 9])), coords='ecef')
    assert lead[0].shape == (2, 5, 7) and np.allclose(lead[2][1][~miss], alt[..., 9][~miss], rtol=0., atol=1e-6)
    # geodetic end points give the same rays
    g0, g1 = geodesy.ecef2geodetic(*a.T), geodesy.ecef2geodetic(*b.T)
    again = ray_samples(eq, tol, tuple(v.reshape(5, 7) for v in g0), tuple(v.reshape(5, 7) for v in g1), 32)
    assert np.allclose(again[0][~miss], d, rtol=0., atol=1e-3)
    # no hull: the whole segment
    free = ray_samples(None, 0., start, end, 4, coords='ecef')[0]
    assert np.allclose(free[..., 0].ravel(), 1e-6 * length) and np.allclose(free[..., -1].ravel(), (1. - 1e-6) * length)
    with pytest.raises(ValueError, match='n must be'):
        ray_samples(eq, tol, start, end, 1, coords='ecef')
    with pytest.raises(ValueError, match='coords'):
        ray_samples(eq, tol, start, end, 8, coords='enu')
    with pytest.raises(ValueError, match='ray shape'):
        ray_points(start, end, np.zeros((5, 6)), coords='ecef')


def test_ray_brackets():
    """ray_peak_brackets: the distance at the index and those of its two neighbours on the ray, the sample itself at either
    end; ray_level_brackets: the distances at the index and the one after it.  NaN for -1 and for a ray without samples; the
    index map may carry a leading axis of times over the rays of dist; the index is checked."""
    from volumetricinterp_amd.estimate import ray_level_brackets, ray_peak_brackets
    nan = np.nan
    dist = np.array([[10., 20., 35., 50.], [5., 6., 7., 8.], [nan] * 4])
    idx = np.array([[2, 0, 1], [3, -1, -1]], dtype=np.int32)                   # (T = 2, 3 rays)
    s, lo, hi = ray_peak_brackets(dist, idx)
    assert s.shape == lo.shape == hi.shape == (2, 3) and s.dtype == np.float64
    assert np.array_equal(s, [[35., 5., nan], [50., nan, nan]], equal_nan=True)
    assert np.array_equal(lo, [[20., 5., nan], [35., nan, nan]], equal_nan=True)
    assert np.array_equal(hi, [[50., 6., nan], [50., nan, nan]], equal_nan=True)
    lo, hi = ray_level_brackets(dist, np.array([[2, 0, 1], [0, -1, -1]]))
    assert np.array_equal(lo, [[35., 5., nan], [10., nan, nan]], equal_nan=True)
    assert np.array_equal(hi, [[50., 6., nan], [20., nan, nan]], equal_nan=True)
    one = ray_peak_brackets(dist[0], np.zeros((), dtype=np.int64))
    assert all(v.shape == () for v in one) and (one[0], one[1], one[2]) == (10., 10., 20.)
    for f, bad in ((ray_peak_brackets, 4), (ray_peak_brackets, -2), (ray_level_brackets, 3), (ray_level_brackets, -2)):
        with pytest.raises(ValueError, match='index must lie'):
            f(dist, np.full((2, 3), bad))
    with pytest.raises(ValueError, match='integer'):
        ray_peak_brackets(dist, np.zeros((2, 3)))
    with pytest.raises(ValueError, match='broadcast'):
        ray_level_brackets(dist, np.zeros((2, 4), dtype=np.int64))
