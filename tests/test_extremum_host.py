"""Host tests of the search for maxima in three dimensions (no GPU): the NumPy mirror of the device iteration
(tests/extremum_ref.py) against scipy.optimize.minimize(method='trust-exact') on the mirror's own value, gradient and Hessian
and against the column search of tests/peak_ref.py; the host helpers estimate.local_maxima and synth.patch_record; and the set
of ROBUST starts that tests/test_gpu_extremum.py holds the device to.

The cases (shared with tests/test_gpu_extremum.py): synth.patch_record - a Chapman layer with a Gaussian enhancement centred at
(78.5, 263.0) - on the 26 x 100 beams of synth.GEOM_C2, fitted as peak_ref.layer_fit fits (lstsq, rcond 1e-10) at MAXK 4 x MAXL 4,
MAXK 6 x MAXL 3, the default order and MAXK 8 x MAXL 2; the hull is that of the beam points; 27 starts, lat {77.5, 78.5, 79.5} x
lon {258, 263, 268} x alt {220, 300, 400} km, radius 400 km, max_step 50 km, tol 1e-3 m, 48 iterations.

Measured (the mirror): k4l4 25 of 27 status 0 in 5 to 10 iterations without a reject, all at 79.1733, 264.2823, 315.177 km; k6l3
25 of 27 in 5 to 9 iterations at 78.6370, 263.0800, 324.812 km; default 14 of 27 at three maxima in 6 to 9 iterations with at
most one reject, 11 onto the hull's boundary (status 1, or 2 at 48 iterations); starts 18 and 24 are outside the hull (status
3) at every order; k8l2 has no maximum in three dimensions inside the hull for this patch - every search runs onto the hull's
boundary -: no status 0."""
import functools

import numpy as np
import pytest

import extremum_ref as er
import peak_ref as pk

TOL = 1e-3
RADIUS, MAX_STEP, MAX_ITER = 400e3, 50e3, 48
OFFSET = np.array([1., -1., 1.])        # metres: where trust-exact starts, from a result of the mirror
EPS = np.finfo(np.float64).eps
G_SLOPE = 1e-10         # tests/test_gpu_peak.py: a peak within tol + 1e-10 terms / |curvature| of the mirror's
CASES = {'k4l4': (4, 4), 'k6l3': (6, 3), 'default': (4, 6), 'k8l2': (8, 2)}       # (MAXK, MAXL)
ORDERS = ('k4l4', 'k6l3', 'default')
FLOORS = {'k4l4': 20, 'k6l3': 20, 'default': 10}
# The robust starts: the mirror reaches the same status for C, C (1 + 2^-48) and C (1 - 2^-48), and with status 0 the same point
# within the gate.  test_robust_starts recomputes them and holds this list to the result.
ROBUST = {
    'k4l4': (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26),
    'k6l3': (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26),
    'default': (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26),
}
ROBUST_FOUND = {
    'k4l4': (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 19, 20, 21, 22, 23, 25, 26),
    'k6l3': (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 19, 20, 21, 22, 23, 25, 26),
    'default': (9, 10, 11, 12, 13, 14, 16, 17, 19, 20, 21, 22, 23, 26),
}


def oracle_of(case):
    import oracle
    maxk, maxl = CASES[case]
    return oracle.SphHarmLagOracle(maxk=maxk, maxl=maxl)


@functools.lru_cache(maxsize=None)
def beam_points():
    """(lat, lon, alt, X): the beam points of GEOM_C2 and their ECEF coordinates (Q, 3), the vertices the hull is made of."""
    from volumetricinterp_amd import geodesy, synth
    lat, lon, alt = synth.beams(*synth.GEOM_C2, seed=0)
    X = np.stack(geodesy.geodetic2ecef(lat, lon, alt), axis=1)
    for v in (lat, lon, alt, X):
        v.setflags(write=False)
    return lat, lon, alt, X


@functools.lru_cache(maxsize=None)
def hull():
    """(eq, tol) of the beam points, as Estimate._hull makes them of the same vertices."""
    from volumetricinterp_amd.estimate import hull_equations
    eq, tol = hull_equations(beam_points()[3])
    eq.setflags(write=False)
    return eq, tol


@functools.lru_cache(maxsize=None)
def patch(case):
    """(oracle, coefficients) of the patch fitted at the order of `case`."""
    from volumetricinterp_amd import synth
    o = oracle_of(case)
    lat, lon, alt, _ = beam_points()
    value, error = synth.patch_record(lat, lon, alt)
    C = np.linalg.lstsq(o.basis(lat, lon, alt) / error[:, None], value / error, rcond=1e-10)[0]
    C.setflags(write=False)
    return o, C


@functools.lru_cache(maxsize=None)
def starts():
    """(lat, lon, alt, x0 (27, 3)) of the 27 starts, lat-major."""
    from volumetricinterp_amd import geodesy
    g = np.meshgrid([77.5, 78.5, 79.5], [258., 263., 268.], [220e3, 300e3, 400e3], indexing='ij')
    lat, lon, alt = (v.ravel() for v in g)
    x0 = np.stack(geodesy.geodetic2ecef(lat, lon, alt), axis=1)
    x0.setflags(write=False)
    return lat, lon, alt, x0


def search(case, scale=1., **kw):
    o, C = patch(case)
    eq, htol = hull()
    args = dict(kind=1, max_step=MAX_STEP, tol=TOL, max_iter=MAX_ITER, eq=eq, htol=htol)
    args.update(kw)
    return er.extremum_search(o, C * scale, starts()[3], RADIUS, **args)


@functools.lru_cache(maxsize=None)
def searches(case):
    """The mirror's 27 searches on the fit of `case` (arrays read-only): the reference of tests/test_gpu_extremum.py."""
    r = search(case)
    for v in r.values():
        v.setflags(write=False)
    return r


def gate(r):
    """tol + 1e-10 terms / lam: the project's G_SLOPE gate with the smallest curvature of the Hessian in place of the one
    curvature of a search along a line."""
    with np.errstate(all='ignore'):
        return TOL + G_SLOPE * r['terms'] / r['lam']


@functools.lru_cache(maxsize=None)
def robust(case):
    """(mask of the robust starts, mask of the robust starts with status 0), computed: see ROBUST."""
    r = searches(case)
    ok = np.ones(27, dtype=bool)
    for scale in (1. + 2.**-48, 1. - 2.**-48):
        s = search(case, scale)
        ok &= s['status'] == r['status']
        found = (r['status'] == 0) & (s['status'] == 0)
        dist = np.sqrt(((s['x'] - r['x'])**2).sum(axis=1))
        print('%s, C * %r: statuses %s, status-0 results within %.2e m' % (case, scale, s['status'], np.nanmax(dist[found])))
        with np.errstate(invalid='ignore'):
            ok &= ~found | (dist <= gate(r))
    return ok, ok & (r['status'] == 0)


# ==== (a), (b): the mirror ===================================================================================================
@pytest.mark.parametrize('case', ORDERS)
def test_mirror_against_trust_exact_and_the_column_search(case):
    """From a point one metre off every status-0 result of the mirror (1, -1, 1 m in ECEF) scipy.optimize.minimize(method=
    'trust-exact') on the mirror's own -f, -g and -H (gtol 4 N eps terms, four times the rounding bound of the gradient's sum)
    comes back to within tol + 1e-10 terms / lam of the result - the search stops after an unmodified Newton step of at most
    tol, which next to a simple zero is as long as the distance it leaves -, at the two low orders to within tol itself; and
    peak_ref.peak_search on the result's column from the result's height (bracket +-50 km) returns the same height within that
    gate: a maximum in three dimensions is a maximum along the vertical.  Starts 18 and 24 are outside the hull; at least 25, 25
    and 14 searches have status 0, in 5 to 10 iterations, with a reject at the default order only.
    Measured: k4l4 1.4e-6 m from trust-exact and 1.9e-8 m from the column search (gate 0.127 m); k6l3 1.7e-6 m and 7.5e-9 m (gate
    0.080 m); default 2.5e-5 to 1.73 m and 3.8e-5 m (gate 3.8 to 14.4 m) - there trust-exact, which accepts a step by the value
    alone, stops where the gain falls below the rounding of f (5e11 with terms of 2e12), for some results without having moved
    from its start one metre off: the case the acceptance by gradient norm is in the iteration for."""
    from scipy.optimize import minimize
    from volumetricinterp_amd import geodesy
    o, C = patch(case)
    r = searches(case)
    print(case, 'status', r['status'])
    print(case, 'iterations', r['it'], 'rejects', r['rejects'])
    found = np.flatnonzero(r['status'] == 0)
    assert list(np.flatnonzero(r['status'] == 3)) == [18, 24]
    assert found.size >= (14 if case == 'default' else 25) and r['it'][found].min() >= 5 and r['it'][found].max() <= 10
    assert r['rejects'][found].max() <= (1 if case == 'default' else 0)
    g = gate(r)
    one = lambda x, k: tuple(v[0] for v in er.walk(o, C, x[None, :])[:3])[k]
    worst = 0.
    for j in found:
        x = r['x'][j]
        assert er.definite(-r['H'][j]) and er.inside(x, *hull()) and er.norm3(x - starts()[3][j]) <= RADIUS
        res = minimize(lambda y: -one(y, 0), x + OFFSET, jac=lambda y: -one(y, 1), hess=lambda y: -one(y, 2),
                       method='trust-exact', options=dict(gtol=4. * o.nbasis * EPS * r['terms'][j], initial_trust_radius=1.,
                                                          max_trust_radius=100., maxiter=50))
        dist = er.norm3(res.x - x)
        worst = max(worst, dist)
        print('%s start %2d: %d iterations, %.3e m from trust-exact (%d iterations, |g| %.2e), gate %.2e m'
              % (case, j, r['it'][j], dist, res.nit, er.norm3(res.jac), g[j]))
        assert dist <= g[j] and (case == 'default' or dist <= TOL), (case, j, dist, g[j])
    lat, lon, alt = geodesy.ecef2geodetic(*r['x'][found].T)
    col = pk.peak_search(o, C, lat, lon, alt, alt - 50e3, alt + 50e3, 1, TOL, 48)
    diff = np.abs(col['h'] - alt)
    print('%s: within %.2e m of trust-exact; column search from the result: statuses %s, heights within %.2e m (gate %.2e m)'
          % (case, worst, col['status'], diff.max(), g[found].min()))
    assert (col['status'] == 0).all() and (diff <= g[found]).all()


def slack(x, x0, radius):
    """(hull, ball): how far the points x (P, 3) are inside the nearest facet of the hull and inside the ball about x0, metres
    (negative: outside)."""
    eq, _ = hull()
    return -(x @ eq[:, :3].T + eq[:, 3]).max(axis=1), radius - np.sqrt(((x - x0)**2).sum(axis=1))


def test_the_k8l2_fit_has_no_maximum():
    """MAXK 8 x MAXL 2: no start returns status 0; every search runs onto the boundary of the hull and ends there (status 1:
    within tol of a facet) or uses up its iterations on the way (2)."""
    r = searches('k8l2')
    print('k8l2 status', r['status'], 'iterations', r['it'])
    assert list(np.flatnonzero(r['status'] == 3)) == [18, 24] and not (r['status'] == 0).any()
    one = r['status'] == 1
    h, b = slack(r['x'][one], starts()[3][one], RADIUS)
    print('k8l2 status 1: %d results, %.2e to %.2e m inside the nearest facet, at least %.0f m inside the ball'
          % (one.sum(), h.min(), h.max(), b.min()))
    assert one.sum() >= 10 and ((h <= TOL) | (b <= TOL) | ~np.array([er.definite(-H) for H in r['H'][one]])).all()


def test_mirror_statuses_by_construction():
    """max_iter = 0 evaluates the start (status 2); a NaN start, a radius that is NaN, zero or negative and a start outside the
    hull give status 3 and NaN; a ball of 1 km around a start far from the maximum ends on the ball (status 1, within tol);
    kind = -1 on the negated coefficients walks the same points."""
    o, C = patch('k4l4')
    eq, htol = hull()
    x0 = starts()[3]
    kw = dict(max_step=MAX_STEP, tol=TOL, eq=eq, htol=htol)
    r = er.extremum_search(o, C, x0[[4, 4, 4, 4, 4, 18]] * np.array([1., np.nan, 1., 1., 1., 1.])[:, None],
                           [RADIUS, RADIUS, np.nan, 0., -1., RADIUS], max_iter=0, **kw)
    assert list(r['status']) == [2, 3, 3, 3, 3, 3] and list(r['it']) == [0] * 6
    assert np.array_equal(r['x'][0], x0[4]) and np.isnan(r['x'][1:]).all() and np.isnan(r['f'][1:]).all()
    f, g, H, _ = er.walk(o, C, x0[4:5])
    assert np.allclose(r['f'][0], f[0], rtol=1e-12) and np.allclose(r['g'][0], g[0], rtol=1e-9) and np.allclose(r['H'][0], H[0], rtol=1e-9)
    kw['max_step'] = None
    ball = er.extremum_search(o, C, x0[[4, 13]], 1e3, max_iter=MAX_ITER, **kw)
    dist = np.sqrt(((ball['x'] - x0[[4, 13]])**2).sum(axis=1))
    print('ball of 1 km: statuses %s, iterations %s, |x - x0| - radius %s' % (ball['status'], ball['it'], dist - 1e3))
    assert (ball['status'] == 1).all() and (np.abs(dist - 1e3) <= TOL).all()
    a = er.extremum_search(o, C, x0[:6], RADIUS, kind=1, max_iter=MAX_ITER, **kw)
    b = er.extremum_search(o, -C, x0[:6], RADIUS, kind=-1, max_iter=MAX_ITER, **kw)
    assert np.array_equal(a['x'], b['x']) and np.array_equal(a['f'], -b['f']) and np.array_equal(a['it'], b['it'])
    assert np.array_equal(a['status'], b['status'])


# ==== (c) local_maxima =======================================================================================================
def test_local_maxima():
    """Hand-made maps: a peak is strictly above its eight neighbours that are numbers; NaN neighbours and the edges do not count
    against it; a tie is no maximum; a column with index -1 is none and counts as NaN for its neighbours; kind='min'; the
    altitude is alt_axis[index]; the positions come in C order with their time."""
    from volumetricinterp_amd.estimate import local_maxima
    nan = np.nan
    alt = np.array([100e3, 200e3, 300e3, 400e3])
    v = np.array([[[1., 2., 1., 0.],
                   [2., 5., 2., 0.],
                   [1., 2., nan, 7.],
                   [9., 1., 7., 0.]],
                  [[3., 3., 0., 0.],
                   [0., 0., 0., 4.],
                   [0., 6., 0., nan],
                   [0., 0., 0., 8.]]])
    idx = np.full(v.shape, 2, dtype=np.int32)
    idx[0, 1, 1], idx[0, 3, 0], idx[1, 3, 3] = 1, 3, 0
    idx[np.isnan(v)] = -1
    t, i, j, a = local_maxima(v, idx, alt)
    got = list(zip(t.tolist(), i.tolist(), j.tolist(), a.tolist()))
    # record 0: (1,1) interior; (3,0) a corner; the two 7s at (2,3) and (3,2) are diagonal neighbours and tie: neither.
    # record 1: the 3s at (0,0), (0,1) tie; (1,3) 4 an edge next to a NaN; (2,1) interior; (3,3) a corner next to a NaN.
    assert got == [(0, 1, 1, 200e3), (0, 3, 0, 400e3), (1, 1, 3, 300e3), (1, 2, 1, 300e3), (1, 3, 3, 100e3)], got
    assert a.dtype == np.float64 and t.dtype.kind == 'i'
    # a -1 index blanks the column whatever its value holds: the 5 goes, and its neighbours (2s, tied in a ring) gain nothing
    idx2 = idx.copy()
    idx2[0, 1, 1] = -1
    t2, i2, j2, _ = local_maxima(v, idx2, alt)
    assert (0, 1, 1) not in list(zip(t2, i2, j2)) and len(t2) == len(t) - 1
    # kind='min' is the maxima of the negated maps
    tm, im, jm, am = local_maxima(-v, idx, alt, kind='min')
    assert np.array_equal(tm, t) and np.array_equal(im, i) and np.array_equal(jm, j) and np.array_equal(am, a)
    # a map of one column, a map without numbers, an empty list of records
    assert [x.tolist() for x in local_maxima([[[2.]]], np.array([[[3]]]), alt)] == [[0], [0], [0], [400e3]]
    assert all(x.size == 0 for x in local_maxima(np.full((1, 2, 2), nan), np.full((1, 2, 2), -1), alt))
    assert all(x.size == 0 for x in local_maxima(np.zeros((0, 2, 2)), np.zeros((0, 2, 2), dtype=np.int64), alt))
    with pytest.raises(ValueError, match='integer'):
        local_maxima(v, idx.astype(np.float64), alt)
    with pytest.raises(ValueError, match='one shape'):
        local_maxima(v, idx[0], alt)
    with pytest.raises(ValueError, match='index must lie'):
        local_maxima(v, np.full(v.shape, 4), alt)
    with pytest.raises(ValueError, match='kind must be'):
        local_maxima(v, idx, alt, kind='saddle')
    with pytest.raises(ValueError, match='alt_axis'):
        local_maxima(v, idx, np.zeros((2, 2)))


# ==== (d) patch_record =======================================================================================================
def test_patch_record():
    """Shapes follow the broadcast of the arguments; amp=0 is chapman_record bit for bit; at the centre the layer is doubled
    (amp=1), one sigma away along the 300 km shell it is the layer times 1 + exp(-1/2); the errors are 5 % + 1e10 of the value;
    the Chapman arguments pass through."""
    from volumetricinterp_amd import geodesy, synth
    lat, lon, alt = synth.beams(3, 7, seed=1)
    v, e = synth.patch_record(lat, lon, alt)
    assert v.shape == e.shape == (21,) and np.array_equal(e, 0.05 * v + 1e10)
    v0, e0 = synth.patch_record(lat, lon, alt, amp=0.)
    c, ce = synth.chapman_record(alt)
    assert np.array_equal(v0, c) and np.array_equal(e0, ce)
    assert (v >= c).all() and (v <= 2. * c).all()
    g = synth.patch_record(78.5, 263.0, np.array([[250e3, 300e3], [350e3, 500e3]]))[0]
    assert g.shape == (2, 2) and np.array_equal(g, 2. * synth.chapman_record([[250e3, 300e3], [350e3, 500e3]])[0])
    grid = synth.patch_record(np.array([77., 78., 79.])[:, None], np.array([260., 265.])[None, :], 300e3)[0]
    assert grid.shape == (3, 2)
    # a point at the ECEF distance sigma from the centre on the 300 km shell: move north until the chord is sigma
    X0 = np.array(geodesy.geodetic2ecef(78.5, 263.0, 300e3))
    lo, hi = 78.5, 81.
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if np.linalg.norm(np.array(geodesy.geodetic2ecef(mid, 263.0, 300e3)) - X0) < 120e3:
            lo = mid
        else:
            hi = mid
    one = synth.patch_record(lo, 263.0, 700e3)[0] / synth.chapman_record(700e3)[0]        # the altitude does not enter d
    assert abs(one - (1. + np.exp(-0.5))) <= 1e-9
    w = synth.patch_record(78.5, 263.0, 300e3, lat0=70., sigma=50e3, amp=-0.5, nmax=1e11, hm=300e3)[0]
    assert abs(w - 1e11) <= 1e-3                                                          # far from the depletion
    assert synth.patch_record(70., 263.0, 300e3, lat0=70., sigma=50e3, amp=-0.5, nmax=1e11)[0] == 0.5e11


# ==== (e) the robust starts ==================================================================================================
@pytest.mark.parametrize('case', ORDERS)
def test_robust_starts(case):
    """The starts whose mirror search reaches the same status for C, C (1 + 2^-48) and C (1 - 2^-48) and, with status 0, the
    same point within tol + 1e-10 terms / lam: a perturbation of the record by 16 ulps, which moves every sum as rounding in
    another order may.  They are the reference of tests/test_gpu_extremum.py; ROBUST and ROBUST_FOUND hold them, this test
    recomputes both.  At least 20, 20 and 10 of them have status 0."""
    ok, found = robust(case)
    print('%s: robust %s' % (case, np.flatnonzero(ok).tolist()))
    print('%s: robust with status 0 %s' % (case, np.flatnonzero(found).tolist()))
    assert found.sum() >= FLOORS[case]
    assert tuple(np.flatnonzero(ok)) == ROBUST[case] and tuple(np.flatnonzero(found)) == ROBUST_FOUND[case]
