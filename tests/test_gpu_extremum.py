"""GPU tests of the search for maxima and minima in three dimensions: Estimate.extremum (vi_eval_extremum_f64, kernel
k_extremum_sph of csrc/vi_extremum.hip: a lane per search, value, gradient and Hessian from one walk at the ECEF point, turned
into ECEF with the model's unit vectors there, a safeguarded Newton iteration in R^3 with the hull test of every iterate in the
kernel).

The reference project has no counterpart.  The yardstick of the positions is tests/extremum_ref.py, the device iteration in
NumPy on the oracle's basis, gradient basis and the Hessian restatement, which tests/test_extremum_host.py holds against
scipy's trust-exact and the column mirror; its robust starts (ROBUST there) are the reference.  Gates: a position within
tol + 1e-10 terms / lam of the mirror's (the gate of tests/test_gpu_peak.py with the smallest curvature of the Hessian in place
of the one curvature); value, gradient and Hessian within 1e-12 of the size of their terms of Estimate.__call__, gradient and
hessian at the returned point (the gate of tests/test_gpu_ray.py); bit for bit wherever the launch geometry changes."""
import functools

import numpy as np
import pytest

import extremum_ref as er
import hessian_ref as hr
import test_gpu_hessian as th
from test_extremum_host import (CASES, MAX_ITER, MAX_STEP, ORDERS, RADIUS, ROBUST, ROBUST_FOUND, TOL, beam_points, gate, hull,
                                patch, searches, slack, starts)
from test_gpu_hessian import T_MID
from test_gpu_level import _bits, _same_bits

pytestmark = pytest.mark.gpu

FIELDS = ('gdlat', 'gdlon', 'gdalt', 'value', 'gradient', 'hessian', 'status', 'iterations')
CFG = th.SPH_CFG


@functools.lru_cache(maxsize=None)
def _es(case, negate=False):
    """The patch fitted at the order of `case` as an Estimate of one record with the hull of the beam points: the coefficients
    and the facets the mirror ran on."""
    from volumetricinterp_amd.estimate import Estimate
    maxk, maxl = CASES[case]
    C = patch(case)[1]
    return Estimate.from_arrays((-C if negate else C)[None, :], np.zeros((1, C.size, C.size)), [[0., 60.]], beam_points()[3],
                                CFG % (maxk, maxl, 10.))


def _raw(es, C, x0, radius, kind=1, max_step=MAX_STEP, max_iter=MAX_ITER, tol=TOL, hull=True, guard=0):
    """vi_eval_extremum_f64 itself on the rows C (T, N) and the starts x0 (P, 3) or (T, P, 3): (out (13, T, P), status,
    iterations) as the library leaves them.  guard > 0: the three outputs sit between `guard` cells of a sentinel each, and
    the sentinels are checked."""
    from volumetricinterp_amd import _lib
    C = np.atleast_2d(np.asarray(C, dtype=np.float64))
    T = C.shape[0]
    x0 = np.asarray(x0, dtype=np.float64)
    x0 = np.broadcast_to(x0.reshape((-1,) + x0.shape[-2:]) if x0.ndim == 3 else x0[None], (T,) + x0.shape[-2:])
    P = x0.shape[1]
    xp = np.ascontiguousarray(np.moveaxis(x0, -1, 0))                       # (3, T, P) planar
    rad = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float64), (T, P)))
    eq, F, htol = es._hull_args(hull)
    with es.model.ctx.scope() as dev:
        dx, dr, dC = dev.up(xp), dev.up(rad), dev.up(C)
        dO = dev.up(np.full(13 * T * P + 2 * guard, 7.))
        dS, dI = (dev.up(np.full(T * P + 2 * guard, 7, dtype=np.int32)) for _ in range(2))
        _lib.check(_lib.lib.vi_eval_extremum_f64(es.model.handle(), T, P, dx.ptr, dr.ptr, dC.ptr,
                                                 None if eq is None else dev.up(eq).ptr, F, htol, kind,
                                                 0. if max_step is None else max_step, max_iter, tol, dO.offset_ptr(guard),
                                                 dS.offset_ptr(guard), dI.offset_ptr(guard)), 'vi_eval_extremum_f64')
        out, status, it = dO.download(), dS.download(), dI.download()
    for v in (out, status, it):
        assert (v[:guard] == 7).all() and (v[v.size - guard:] == 7).all()
    cut = lambda v: v[guard:v.size - guard]
    return cut(out).reshape(13, T, P), cut(status).reshape(T, P), cut(it).reshape(T, P)


def _take(full, rows, cols):
    out, status, it = full
    return out[:, rows][:, :, cols], status[rows][:, cols], it[rows][:, cols]


def _enu(out):
    """(lat, lon, alt, gradient (P, 3), hessian (P, 3, 3)) of raw results out (13, P): the geodetic points and the ECEF gradient
    and Hessian turned into east, north, up there with the geodetic axes of tests/hessian_ref.py."""
    from volumetricinterp_amd import geodesy
    from volumetricinterp_amd.estimate import gradcov_matrix
    lat, lon, alt = geodesy.ecef2geodetic(out[0], out[1], out[2])
    A = hr.enu_axes(lat, lon)
    return lat, lon, alt, np.einsum('pic,cp->pi', A, out[4:7]), np.einsum('pic,pcd,pjd->pij', A, gradcov_matrix(out[7:13]), A)


# ==== 1. against the mirror ==================================================================================================
@pytest.mark.parametrize('case', ORDERS)
def test_positions_against_the_mirror(case):
    """The patch at MAXK 4 x MAXL 4, MAXK 6 x MAXL 3 and the default order, the 27 starts of tests/test_extremum_host.py with
    the hull of the beam points: every robust start has the mirror's status, every robust status-0 position is within
    tol + 1e-10 terms / lam of the mirror's, the iteration counts are the mirror's at the two low orders and within one at the
    default order (whose fit cancels heavily: rounding moves an iterate by more than tol, the experience of ray_ref.steady);
    starts that are not robust are printed and held to a status in {0, 1, 2, 3} and a result inside the hull and the ball
    (to tol: the last Newton step is not tested).  Estimate.extremum gives the same results as geodetic points.
    Measured on the MI355X: all 27 starts are robust at every order and have the mirror's status and iteration count; the
    status-0 positions are 5.9e-9 to 8.0e-8 m from the mirror at k4l4 (25 searches, gate 0.127 m), 3.5e-9 to 2.5e-8 m at k6l3 (25,
    gate 0.080 m) and 1.3e-6 to 5.6e-5 m at the default order (14, gates 3.8 to 14.4 m)."""
    from volumetricinterp_amd import geodesy
    es = _es(case)
    r = searches(case)
    lat, lon, alt, x0 = starts()
    out, status, it = _raw(es, es.Coeffs, x0, RADIUS)
    rob = np.isin(np.arange(27), ROBUST[case])
    found = np.isin(np.arange(27), ROBUST_FOUND[case])
    assert found.sum() >= {'k4l4': 20, 'k6l3': 20, 'default': 10}[case] and (r['status'][found] == 0).all()
    dist = np.sqrt(((out[:3, 0].T - r['x'])**2).sum(axis=1))
    g = gate(r)
    for k in range(27):
        print('%s start %2d%s: status %d / mirror %d, %2d / %2d iterations, %.2e m from the mirror, gate %.2e m'
              % (case, k, ' ' if rob[k] else '*', status[0, k], r['status'][k], it[0, k], r['it'][k], dist[k], g[k]))
    assert np.array_equal(status[0][rob], r['status'][rob])
    assert (dist[found] <= g[found]).all(), (dist[found], g[found])
    print('%s: %d robust status-0 positions %.2e to %.2e m from the mirror (gate %.2e to %.2e m)'
          % (case, found.sum(), dist[found].min(), dist[found].max(), g[found].min(), g[found].max()))
    ran = rob & (r['status'] != 3)
    diff = np.abs(it[0] - r['it'])[ran]
    print('%s: iteration counts differ from the mirror\'s at %d of %d robust starts, by up to %d' % (case, (diff > 0).sum(),
                                                                                                   ran.sum(), diff.max()))
    assert diff.max() <= (1 if case == 'default' else 0)
    loose = ~rob
    assert np.isin(status[0][loose], (0, 1, 2, 3)).all()
    ok = loose & (status[0] != 3)
    if ok.any():
        h, b = slack(out[:3, 0].T[ok], x0[ok], RADIUS)
        assert (h >= -TOL).all() and (b >= -TOL).all()
    # the public method: the same searches as geodetic points, position and value blanked where the status is not 0
    p = es.extremum(T_MID, lat, lon, alt, RADIUS, max_step=MAX_STEP)
    assert p._fields == FIELDS and p.gdlat.shape == (27,) and p.gradient.shape == (27, 3) and p.hessian.shape == (27, 3, 3)
    assert np.array_equal(p.status, status[0]) and np.array_equal(p.iterations, it[0]) and p.status.dtype == np.int32
    glat, glon, galt, grad, hess = _enu(out[:, 0])
    z = status[0] == 0
    for got, want in ((p.gdlat, glat), (p.gdlon, glon), (p.gdalt, galt), (p.value, out[3, 0])):
        assert np.array_equal(_bits(got[z]), _bits(want[z])) and np.isnan(got[~z]).all()
    n3 = status[0] != 3
    assert np.allclose(p.gradient[n3], grad[n3], rtol=1e-12, atol=0.) and np.isnan(p.gradient[~n3]).all()
    assert np.allclose(p.hessian[n3], hess[n3], rtol=1e-9, atol=1e-12 * np.abs(hess[n3]).max()) and np.isnan(p.hessian[~n3]).all()
    X = np.stack(geodesy.geodetic2ecef(p.gdlat[z], p.gdlon[z], p.gdalt[z]), axis=1)
    assert np.abs(X - out[:3, 0].T[z]).max() <= 1e-6


# ==== 2. no maximum ==========================================================================================================
def test_the_k8l2_fit_has_no_maximum():
    """MAXK 8 x MAXL 2 (the (12, 8) kernel order) has no maximum in three dimensions for this patch: no start returns status 0,
    and every status-1 result lies within tol of a facet of the hull or of the ball, or has a Hessian that is not negative
    definite."""
    es = _es('k8l2')
    x0 = starts()[3]
    out, status, it = _raw(es, es.Coeffs, x0, RADIUS)
    print('k8l2 statuses', status[0], 'iterations', it[0], 'the mirror\'s', searches('k8l2')['status'])
    assert not (status[0] == 0).any() and list(np.flatnonzero(status[0] == 3)) == [18, 24]
    one = status[0] == 1
    h, b = slack(out[:3, 0].T[one], x0[one], RADIUS)
    from volumetricinterp_amd.estimate import gradcov_matrix
    H = gradcov_matrix(out[7:13, 0])[one]
    print('k8l2: %d status-1 results %.2e to %.2e m inside the nearest facet' % (one.sum(), h.min(), h.max()))
    assert one.sum() >= 10
    assert ((np.abs(h) <= TOL) | (np.abs(b) <= TOL) | ~np.array([er.definite(-m) for m in H])).all()


# ==== 3. consistency with the existing entries ===============================================================================
@pytest.mark.parametrize('which', ['k3l4cap15', 'k5l8cap15', 'k12l2'])
def test_values_at_the_returned_points(which):
    """At every kernel order - (6, 4) with the series seeds of k3l4cap15, (12, 8) with k5l8cap15, (2, 12) with k12l2 - and random
    coefficients, at the geodetic points of what the searches return from 27 starts with max_iter 48 and 1 (every search with
    status 0, 1 or 2; no hull): value against Estimate.__call__, gradient against gradient(frame='enu'), Hessian against
    hessian(frame='enu'), each within 1e-12 of the size of its terms at that point - two device summation orders of one
    quantity, and the frame turned on the host.  The public method's gradient and hessian are the same."""
    from test_gpu_ray import _random_case
    es, o, C = _random_case(which)
    m = es.model
    lat0, lon0, alt0, x0 = starts()
    for max_iter in (48, 1):
        out, status, it = _raw(es, C, x0, 100e3, max_step=None, max_iter=max_iter, hull=False)
        ran = status[0] != 3
        print('%s max_iter %d: statuses %s' % (which, max_iter, np.bincount(status[0], minlength=4)))
        assert ran.sum() >= 20 and np.isfinite(out[:, 0][:, ran]).all()
        lat, lon, alt, grad, hess = (v[ran] for v in _enu(out[:, 0]))
        pts = lat, lon, alt
        F = m.gradient_frame(*pts)
        t_value = np.abs(m.basis(*pts)) @ np.abs(C)
        t_grad = (np.abs(np.einsum('pic,pcn->pin', F, m.grad_basis(*pts))) @ np.abs(C)).max(axis=1)
        t_hess = (np.abs(m.hess_basis(*pts, frame='enu')) @ np.abs(C)).max(axis=1)
        e_value = np.abs(out[3, 0][ran] - es(T_MID, *pts, check_hull=False)) / t_value
        e_grad = np.abs(grad - es.gradient(T_MID, *pts, check_hull=False, frame='enu')).max(axis=1) / t_grad
        e_hess = np.abs(hess - es.hessian(T_MID, *pts, check_hull=False, frame='enu')).max(axis=(1, 2)) / t_hess
        print('%s max_iter %d: value %.2e, gradient %.2e, Hessian %.2e of their terms' % (which, max_iter, e_value.max(),
                                                                                         e_grad.max(), e_hess.max()))
        assert e_value.max() <= 1e-12 and e_grad.max() <= 1e-12 and e_hess.max() <= 1e-12
        p = es.extremum(T_MID, lat0, lon0, alt0, 100e3, max_iter=max_iter, check_hull=False)
        assert np.array_equal(p.status, status[0])
        assert (np.abs(p.gradient[ran] - grad).max(axis=1) <= 1e-12 * t_grad).all()
        assert (np.abs(p.hessian[ran] - hess).max(axis=(1, 2)) <= 1e-12 * t_hess).all()


# ==== 4. launch geometry =====================================================================================================
GEOMETRY_P = 257


@functools.lru_cache(maxsize=None)
def _geometry():
    """(estimate, C (3, N), x0 (3, 257, 3), radius (3, 257), the raw result of the one call with all of them): the k4l4 patch,
    its coefficients times 1.1 and 0.9; starts drawn over the field of view (some outside the hull: status 3 at the first walk),
    every 17th NaN (status 3, no walk), radii from 5 to 400 km (small balls: status 1)."""
    from volumetricinterp_amd import geodesy
    es = _es('k4l4')
    rng = np.random.default_rng(257)
    P = GEOMETRY_P
    pts = rng.uniform(77., 80., (3, P)), rng.uniform(256., 270., (3, P)), rng.uniform(200e3, 450e3, (3, P))
    x0 = np.stack(geodesy.geodetic2ecef(*pts), axis=-1)
    x0[:, ::17] = np.nan
    radius = rng.choice([5e3, 50e3, 400e3], (3, P))
    C = np.stack((es.Coeffs[0], 1.1 * es.Coeffs[0], 0.9 * es.Coeffs[0]))
    return es, C, x0, radius, _raw(es, C, x0, radius, max_step=None)


def test_every_search_has_the_bits_of_its_search_alone():
    """The call with 3 x 257 searches against calls with P = 1, T = 1 for the 64 lanes of the second wave of every row: the same
    bits.  In those waves lanes that never walk (NaN start), lanes outside the hull, lanes that stop early and lanes that go on
    sit next to each other: a stopped lane is frozen while the wave goes on."""
    es, C, x0, radius, full = _geometry()
    print('statuses %s, iterations up to %d' % (np.bincount(full[1].ravel(), minlength=4), full[2].max()))
    wave = slice(64, 128)
    for t in range(3):
        st = full[1][t, wave]
        assert (st == 3).sum() >= 3 and (st == 0).sum() >= 10 and (st == 1).sum() >= 3 and np.ptp(full[2][t, wave][st == 0]) >= 2
        for q in range(64, 128):
            one = _raw(es, C[t], x0[t, q][None], radius[t, q], max_step=None)
            _same_bits(one, _take(full, slice(t, t + 1), slice(q, q + 1)), (t, q))


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('P', [1, 63, 64, 65, 257])
def test_launch_geometry(P, T):
    """A block is 256 lanes, a wave 64: the fields of a search are the same bits whatever P and T are and wherever the search
    sits - the first P, the last P and a random draw of P of the 257 searches in a random order, the first T and the last T of
    the three rows, against the call with all of them.  Lanes past P write nothing: the outputs sit between guard cells."""
    es, C, x0, radius, full = _geometry()
    rng = np.random.default_rng(1000 * T + P)
    for rows in (slice(0, T), slice(3 - T, 3)):
        for cols in (np.arange(P), np.arange(GEOMETRY_P - P, GEOMETRY_P), rng.permutation(GEOMETRY_P)[:P]):
            r = _raw(es, C[rows], x0[rows][:, cols], radius[rows][:, cols], max_step=None, guard=300)
            assert r[0].shape == (13, T, P)
            _same_bits(r, _take(full, rows, cols), (P, T))


def test_more_rows_than_a_grid_holds():
    """T = 65 537 rows - one more than two slices of 65 535 hold, the third slice a single row -, one search, the same
    coefficient row in every row: rows 0, 65 534, 65 535 and 65 536 - the ends of the slices - and every other row have the
    bits of row 0, which are those of the search alone."""
    es = _es('k4l4')
    x0 = starts()[3][13]
    T = 65537
    out, status, it = _raw(es, np.tile(es.Coeffs[0], (T, 1)), x0[None], RADIUS, guard=8)
    one = _raw(es, es.Coeffs, x0[None], RADIUS)
    assert status[0, 0] == 0 and it[0, 0] == searches('k4l4')['it'][13]
    for t in (0, 65534, 65535, 65536):
        _same_bits(_take((out, status, it), slice(t, t + 1), slice(None)), one, t)
    assert (status == 0).all() and (it == it[0, 0]).all() and (_bits(out) == _bits(out[:, :1])).all()


# ==== 5. statuses ============================================================================================================
def test_every_status():
    """By construction, on the k4l4 patch.  A NaN start, a start outside the hull (start 18), a radius that is NaN, zero or
    negative: status 3, NaN, no iteration.  max_iter = 0: status 2 with the start itself and its own values.  A ball of 1 km
    around a start far from the maximum: status 1 with the result on the ball within tol.  The public method blanks position
    and value where the status is not 0 and keeps gradient and Hessian."""
    es = _es('k4l4')
    lat, lon, alt, x0 = starts()
    nan = np.nan
    xs = x0[[4, 4, 18, 4, 4, 4]].copy()
    xs[1, 1] = nan
    out, status, it = _raw(es, es.Coeffs, xs, [RADIUS, RADIUS, RADIUS, nan, 0., -1.])
    assert list(status[0]) == [0, 3, 3, 3, 3, 3] and (it[0, 1:] == 0).all()
    assert np.isnan(out[:, 0, 1:]).all() and np.isfinite(out[:, 0, 0]).all()
    free = _raw(es, es.Coeffs, xs[2:3], RADIUS, hull=False)
    assert free[1][0, 0] != 3                                               # outside the hull, not outside the model's domain
    out, status, it = _raw(es, es.Coeffs, x0[4:5], RADIUS, max_iter=0)
    assert status[0, 0] == 2 and it[0, 0] == 0 and np.array_equal(out[:3, 0, 0], x0[4]) and np.isfinite(out[:, 0, 0]).all()
    pts = lat[4:5], lon[4:5], alt[4:5]
    t_value = np.abs(es.model.basis(*pts)) @ np.abs(es.Coeffs[0])
    assert abs(out[3, 0, 0] - es(T_MID, *pts, check_hull=False)[0]) <= 1e-12 * t_value[0]
    p = es.extremum(T_MID, *pts, RADIUS, max_iter=0)
    assert p.status[0] == 2 and np.isnan([p.gdlat[0], p.gdlon[0], p.gdalt[0], p.value[0]]).all()
    assert np.isfinite(p.gradient).all() and np.isfinite(p.hessian).all()
    out, status, it = _raw(es, es.Coeffs, x0[[4, 13]], 1e3, max_step=None)
    dist = np.sqrt(((out[:3, 0].T - x0[[4, 13]])**2).sum(axis=1))
    print('ball of 1 km: statuses %s, iterations %s, |x - x0| - radius %s m' % (status[0], it[0], dist - 1e3))
    assert (status[0] == 1).all() and (np.abs(dist - 1e3) <= TOL).all()
    p = es.extremum(T_MID, lat[[4, 13]], lon[[4, 13]], alt[[4, 13]], 1e3)
    assert (p.status == 1).all() and np.isnan(p.value).all() and np.isfinite(p.gradient).all()


def test_a_nan_record_reaches_only_itself():
    """Three records, one NaN in the second: that record is status 3 and NaN at every start, the other two keep the bits they
    have without it."""
    es = _es('k4l4')
    x0 = starts()[3]
    C = np.stack((es.Coeffs[0], 1.1 * es.Coeffs[0], 0.9 * es.Coeffs[0]))
    Cn = C.copy()
    Cn[1, 5] = np.nan
    good, r = _raw(es, C, x0, RADIUS), _raw(es, Cn, x0, RADIUS)
    assert (r[1][1] == 3).all() and np.isnan(r[0][:, 1]).all() and (r[2][1] == 0).all()
    for i in (0, 2):
        _same_bits(_take(r, slice(i, i + 1), slice(None)), _take(good, slice(i, i + 1), slice(None)), i)


def test_min_of_the_negated_coefficients():
    """kind='min' on -C walks the points of kind='max' on C bit for bit - every comparison of the iteration carries the sign -
    with value, gradient and Hessian negated; statuses and iterations the same."""
    es, neg = _es('k4l4'), _es('k4l4', True)
    lat, lon, alt, x0 = starts()
    x = _raw(es, es.Coeffs, x0, RADIUS, kind=1)
    y = _raw(neg, neg.Coeffs, x0, RADIUS, kind=-1)
    assert np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) and (x[1] == 0).sum() >= 20
    ran = x[1][0] != 3
    assert np.isnan(x[0][:, 0, ~ran]).all() and np.isnan(y[0][:, 0, ~ran]).all()
    x0_, y0_ = x[0][:, 0, ran], y[0][:, 0, ran]
    assert np.array_equal(_bits(x0_[:3]), _bits(y0_[:3])) and np.array_equal(_bits(x0_[3:]), _bits(-y0_[3:]))
    px = es.extremum(T_MID, lat, lon, alt, RADIUS, kind='max', max_step=MAX_STEP)
    py = neg.extremum(T_MID, lat, lon, alt, RADIUS, kind='min', max_step=MAX_STEP)
    z = px.status == 0
    assert np.array_equal(_bits(px.gdalt[z]), _bits(py.gdalt[z])) and np.array_equal(_bits(px.value[z]), _bits(-py.value[z]))
    assert np.array_equal(_bits(px.hessian[ran]), _bits(-py.hessian[ran])) and np.array_equal(px.status, py.status)


def test_public_method_shapes_and_records():
    """extremum with a list of three datetimes gives (3,) + S, with one datetime S; record t of the batch has the bits of the
    same record alone, with its own altitude and radius; S may have any rank."""
    import datetime as dt
    from volumetricinterp_amd.estimate import Estimate
    maxk, maxl = CASES['k4l4']
    C0 = patch('k4l4')[1]
    C = np.stack((C0, 1.1 * C0, 0.9 * C0))
    es = Estimate.from_arrays(C, np.zeros((3, C0.size, C0.size)), [[60. * t, 60. * t + 60.] for t in range(3)], beam_points()[3],
                              CFG % (maxk, maxl, 10.))
    times = [dt.datetime(1970, 1, 1) + dt.timedelta(seconds=60. * t + 30.) for t in range(3)]
    rng = np.random.default_rng(35)
    lat, lon = rng.uniform(78., 79.5, (5, 7)), rng.uniform(260., 267., (5, 7))
    alt, radius = rng.uniform(250e3, 380e3, (3, 5, 7)), rng.choice([100e3, 400e3], (3, 5, 7))
    batch = es.extremum(times, lat, lon, alt, radius)
    assert batch.gdlat.shape == (3, 5, 7) and batch.hessian.shape == (3, 5, 7, 3, 3) and (batch.status == 0).sum() >= 50
    for i in range(3):
        one = es.extremum(times[i], lat, lon, alt[i], radius[i])
        assert one.gdlat.shape == (5, 7) and one.gradient.shape == (5, 7, 3)
        _same_bits(one, tuple(f[i] for f in batch), i)
    empty = es.extremum([], lat, lon, 300e3, 1e5)
    assert empty.gdlat.shape == (0, 5, 7) and empty.hessian.shape == (0, 5, 7, 3, 3) and empty.status.dtype == np.int32


# ==== 6. errors ==============================================================================================================
def test_error_bars():
    """error=True on the k4l4 patch with a positive definite coefficient covariance: position_covariance is H^-1 S H^-1
    recomputed here from gradient_covariance(frame='enu') at the returned points and the returned Hessian, symmetric and
    positive semi-definite where the status is 0 and NaN elsewhere; value_error is error() there bit for bit; the fields before
    them are those of error=False.  Without a covariance it raises, as the error entries do."""
    from volumetricinterp_amd.estimate import Estimate
    maxk, maxl = CASES['k4l4']
    C = patch('k4l4')[1]
    rng = np.random.default_rng(64)
    B = rng.standard_normal((C.size, C.size)) * (1e-3 * np.abs(C))[:, None]
    es = Estimate.from_arrays(C[None, :], (B @ B.T / C.size)[None], [[0., 60.]], beam_points()[3], CFG % (maxk, maxl, 10.))
    lat, lon, alt, x0 = starts()
    r = es.extremum(T_MID, lat, lon, alt, RADIUS, max_step=MAX_STEP, error=True)
    assert r._fields == FIELDS + ('position_covariance', 'value_error') and r.position_covariance.shape == (27, 3, 3)
    _same_bits(r[:8], es.extremum(T_MID, lat, lon, alt, RADIUS, max_step=MAX_STEP))
    ok = r.status == 0
    assert ok.sum() >= 20 and (r.status[[18, 24]] == 3).all()
    assert np.isnan(r.position_covariance[~ok]).all() and np.isnan(r.value_error[~ok]).all()
    pts = r.gdlat[ok], r.gdlon[ok], r.gdalt[ok]
    S = es.gradient_covariance(T_MID, *pts, frame='enu')
    Hi = np.linalg.inv(r.hessian[ok])
    want = np.einsum('pij,pjk,plk->pil', Hi, S, Hi)
    pc = r.position_covariance[ok]
    assert np.allclose(pc, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())
    assert np.abs(pc - pc.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(pc).max()
    eig = np.linalg.eigvalsh(0.5 * (pc + pc.transpose(0, 2, 1)))
    print('position errors (m, east north up) %s, value error %.3e' % (np.sqrt(np.diagonal(pc[0])), r.value_error[ok][0]))
    assert (eig[:, 0] >= -1e-12 * eig[:, 2]).all() and (eig[:, 2] > 0.).all()
    assert np.array_equal(r.value_error[ok], es.error(T_MID, *pts))
    bare = Estimate.from_arrays(C[None, :], None, [[0., 60.]], beam_points()[3], CFG % (maxk, maxl, 10.))
    with pytest.raises(ValueError, match='no covariance'):
        bare.extremum(T_MID, lat, lon, alt, RADIUS, error=True)


# ==== 7. refusals ============================================================================================================
def test_refusals():
    """The radial-basis model and an order beyond the gradient's (MAXL 13): VI_ERR_UNSUPPORTED (-6) from the library,
    VinterpError from Python.  max_iter above 10 000 or negative, tol <= 0 or not finite, a bad kind, a max_step that is
    negative or not finite, a null pointer, a negative size and facets counted but not given: VI_ERR_INVALID (-1), ValueError
    from Python.  Nothing was launched by any of them: the output buffers are untouched, and with the context's timing on, the
    kernel time it reports is still that of the call before.  T = 0 and P = 0 are no-ops; a null d_iter is allowed."""
    from conftest import load_golden
    from volumetricinterp_amd import _lib
    from volumetricinterp_amd.estimate import Estimate
    lat, lon, alt, x0 = starts()
    P = 27
    th.BASIS_CASES['k2l13'] = (2, 13, 10.)
    try:
        big = th._bare('k2l13')
    finally:
        del th.BASIS_CASES['k2l13']
    fr = load_golden('fit_rbf')
    rbf = Estimate.from_arrays(fr['Coeffs'], fr['Covariance'], fr['utime'], fr['hull_vert'], str(fr['cfg']))
    ok = th._bare('default', np.ones(144))
    xp = np.ascontiguousarray(x0.T)

    def call(es, dev, T=1, np_=P, kind=1, max_step=MAX_STEP, max_iter=48, tol=TOL, F=0, null=None):
        d = [dev.up(v) for v in (xp, np.full(P, RADIUS), np.ones(es.model.nbasis))]
        dO, dS, dI = dev.up(np.full(13 * P, 7.)), dev.up(np.full(P, 7, dtype=np.int32)), dev.up(np.full(P, 7, dtype=np.int32))
        p = [v.ptr for v in d] + [None, F, 0., kind, max_step, max_iter, tol, dO.ptr, dS.ptr, dI.ptr]
        if null is not None:
            p[null] = None
        rc = _lib.lib.vi_eval_extremum_f64(es.model.handle(), T, np_, *p)
        es.model.ctx.sync()
        assert np.array_equal(dO.download(), np.full(13 * P, 7.))
        assert np.array_equal(dS.download(), np.full(P, 7)) and np.array_equal(dI.download(), np.full(P, 7))
        return rc

    kw = dict(check_hull=False)
    ctx = ok.model.ctx
    ctx.eval_timing(True)
    try:
        ok.extremum(T_MID, lat, lon, alt, RADIUS, **kw)
        before = ctx.eval_kernel_ms()
        assert 0. < before < 1000.
        for es, what in ((big, 'beyond the compiled limits'), (rbf, 'only the sphharmlag model')):
            with es.model.ctx.scope() as dev:
                assert call(es, dev) == -6 and what in _lib.lib.vi_last_error().decode()
        with ctx.scope() as dev:
            bads = [dict(tol=0.), dict(tol=-1.), dict(tol=np.nan), dict(tol=np.inf), dict(max_iter=-1), dict(max_iter=10001),
                    dict(max_step=-1.), dict(max_step=np.nan), dict(max_step=np.inf), dict(kind=0), dict(kind=2), dict(F=3),
                    dict(T=-1), dict(np_=-1)] + [dict(null=i) for i in (0, 1, 2, 10, 11)]
            for bad in bads:
                assert call(ok, dev, **bad) == -1, bad
            assert call(ok, dev, T=0) == 0 and call(ok, dev, np_=0) == 0
        for es, what, t in ((big, 'beyond the compiled limits', T_MID), (rbf, 'only the sphharmlag model', th._t_rec(fr))):
            with pytest.raises(_lib.VinterpError, match=what):
                es.extremum(t, lat, lon, alt, RADIUS, **kw)
        for bad in (dict(tol=0.), dict(tol=np.nan), dict(max_iter=-1), dict(max_iter=1.5), dict(max_iter=10001),
                    dict(max_iter=True), dict(max_step=0.), dict(max_step=np.inf)):
            with pytest.raises(ValueError, match='tol must be|max_iter must be|max_step must be'):
                ok.extremum(T_MID, lat, lon, alt, RADIUS, **kw, **bad)
        with pytest.raises(ValueError, match='kind must be'):
            ok.extremum(T_MID, lat, lon, alt, RADIUS, kind='saddle', **kw)
        with pytest.raises(ValueError, match='broadcast'):
            ok.extremum(T_MID, lat, lon, alt, np.zeros(P + 1), **kw)
        assert ctx.eval_kernel_ms() == before                                 # nothing was launched since
        ok.extremum(T_MID, lat, lon, alt, RADIUS, **kw)
        assert 0. < ctx.eval_kernel_ms() < 1000.
    finally:
        ctx.eval_timing(False)
    with ctx.scope() as dev:
        d = [dev.up(v) for v in (xp, np.full(P, RADIUS), np.ones(144))]
        dO, dS = dev.empty((13, P)), dev.empty(P, np.int32)
        assert _lib.lib.vi_eval_extremum_f64(ok.model.handle(), 1, P, *(v.ptr for v in d), None, 0, 0., 1, 0., 48, TOL, dO.ptr,
                                             dS.ptr, None) == 0
        assert np.isin(dS.download(), (0, 1, 2, 3)).all()


# ==== 8. the recipe ==========================================================================================================
def test_from_column_maps_to_the_patch_centre():
    """The README's recipe end to end on the k4l4 patch: a resident grid of 9 x 9 x 13 points -> g.peak along altitude ->
    local_maxima -> extremum from the grid points it names, within a ball of two grid cells.  The map has one local maximum
    inside the hull, and the search from it ends at the maximum the 27 starts of the mirror find, to 2 tol."""
    from volumetricinterp_amd import geodesy
    from volumetricinterp_amd.estimate import local_maxima
    es = _es('k4l4')
    lat, lon, alt = np.linspace(77.5, 80., 9), np.linspace(258., 270., 9), np.linspace(200e3, 440e3, 13)
    glat, glon, galt = np.meshgrid(lat, lon, alt, indexing='ij')
    with es.resident_grid(glat, glon, galt) as g:
        value, index = g.peak([T_MID])
    t, i, j, a = local_maxima(value, index, alt)
    print('local maxima of the column map: %s' % list(zip(t.tolist(), i.tolist(), j.tolist(), a.tolist())))
    assert t.size >= 1
    r = es.extremum(T_MID, lat[i], lon[j], a, 120e3)
    print('statuses %s, iterations %s' % (r.status, r.iterations))
    ok = r.status == 0
    assert ok.sum() >= 1
    ref = searches('k4l4')
    X = np.stack(geodesy.geodetic2ecef(r.gdlat[ok], r.gdlon[ok], r.gdalt[ok]), axis=1)
    assert np.sqrt(((X - ref['x'][0])**2).sum(axis=1)).min() <= 2. * TOL + 1e-6
    assert (r.value[ok] >= value[t[ok], i[ok], j[ok]] * (1. - 1e-9)).all()
