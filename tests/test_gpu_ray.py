"""GPU tests of the searches along straight rays: Estimate.ray_peak and Estimate.ray_level (vi_eval_ray_peak_f64 and
vi_eval_ray_level_f64, kernels k_line_peak_sph and k_line_level_sph of csrc/vi_line.hip: a lane per ray, the point at the
distance s evaluated from ECEF, slope w . grad f and curvature w^T H w with the ray's direction w in the model's orthonormal
frame, both ends of a bracket tested against the hull in the kernel).

The reference project has neither.  The yardstick of the distances is tests/ray_ref.py, the device iterations in NumPy on the
oracle's basis, gradient basis and the Hessian restatement, which tests/test_ray_host.py holds against scipy.optimize.brentq
and, on vertical rays, against the column mirrors.  Gates, those of tests/test_gpu_peak.py and tests/test_gpu_level.py with the
distance in place of the height: a peak within tol + 1e-10 terms / |curvature| of the mirror's, a crossing within
tol + G_VALUE vterms / |slope|; value, slope and curvature within 1e-12 of the size of their terms of Estimate.__call__,
gradient and hessian at the returned point; bit for bit wherever the launch geometry changes."""
import functools

import numpy as np
import pytest

import hessian_ref as hr
import ray_ref as rr
import test_gpu_hessian as th
from conftest import load_golden
from test_gpu_hessian import T_MID, _bare, _estimate, _t_rec
from test_gpu_level import G_VALUE, TOL, _bits, _records, _same_bits
from test_peak_host import HI, LO, layer
from test_ray_host import SITE, beam_ends, ray_searches, rays, rays_into_hull

pytestmark = pytest.mark.gpu

PEAK_FIELDS = ('distance', 'value', 'slope', 'curvature', 'status', 'iterations')
LEVEL_FIELDS = ('distance', 'value', 'slope', 'status', 'iterations')
G_SLOPE = 1e-10         # tests/test_gpu_peak.py: a height within tol + 1e-10 terms / |curvature| of the mirror's


def _ends(a, b):
    """(start, end) for the public methods with coords='ecef' from (P, 3) end points."""
    return tuple(np.asarray(a).T), tuple(np.asarray(b).T)


def _raw_peak(es, C, a, b, start, lo, hi, kind=1, max_iter=48, tol=TOL, hull=False):
    """vi_eval_ray_peak_f64 itself on the rows C (T, N) and the rays a -> b (P, 3): (out (4, T, P), status, iterations) as the
    library leaves them - Estimate.ray_peak blanks the distance and the value where the status is not 0."""
    from volumetricinterp_amd import _lib
    C = np.atleast_2d(np.asarray(C, dtype=np.float64))
    a, b = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1, 3).T) for v in (a, b))
    T, P = C.shape[0], a.shape[1]
    per = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (T, P))) for v in (start, lo, hi)]
    eq, F, htol = es._hull_args(hull)
    with es.model.ctx.scope() as dev:
        d = [dev.up(v) for v in [a, b] + per + [C]]
        dO, dS, dI = dev.empty((4, T, P)), dev.empty((T, P), np.int32), dev.empty((T, P), np.int32)
        _lib.check(_lib.lib.vi_eval_ray_peak_f64(es.model.handle(), T, P, *(v.ptr for v in d),
                                                 None if eq is None else dev.up(eq).ptr, F, htol, kind, max_iter, tol, dO.ptr,
                                                 dS.ptr, dI.ptr), 'vi_eval_ray_peak_f64')
        return dO.download(), dS.download(), dI.download()


def _raw_level(es, C, a, b, level, lo, hi, max_iter=48, tol=TOL, hull=False):
    """vi_eval_ray_level_f64 itself: (out (3, T, P), status, iterations)."""
    from volumetricinterp_amd import _lib
    C = np.atleast_2d(np.asarray(C, dtype=np.float64))
    a, b = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1, 3).T) for v in (a, b))
    T, P = C.shape[0], a.shape[1]
    lev, lo, hi = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (T, P))) for v in (level, lo, hi))
    eq, F, htol = es._hull_args(hull)
    with es.model.ctx.scope() as dev:
        d = [dev.up(v) for v in (a, b, np.stack((lo, hi)), lev, C)]
        dO, dS, dI = dev.empty((3, T, P)), dev.empty((T, P), np.int32), dev.empty((T, P), np.int32)
        _lib.check(_lib.lib.vi_eval_ray_level_f64(es.model.handle(), T, P, *(v.ptr for v in d),
                                                  None if eq is None else dev.up(eq).ptr, F, htol, max_iter, tol, dO.ptr, dS.ptr,
                                                  dI.ptr), 'vi_eval_ray_level_f64')
        return dO.download(), dS.download(), dI.download()


def _take(full, rows, cols):
    out, status, it = full
    return out[:, rows][:, :, cols], status[rows][:, cols], it[rows][:, cols]


@functools.lru_cache(maxsize=None)
def _layer_es(case):
    """The Chapman layer of tests/test_peak_host.py as an Estimate of one record, no hull: the coefficients the mirror ran on."""
    return _bare(case, layer(case)[1])


def _direction(o, a, b, pts):
    """w (P, 3): the unit directions of the rays in the model's orthonormal frame at the geodetic points pts."""
    return rr.frame(o, rr.lines(a, b)[0], *pts)


def _sym(packed):
    """(P, 3, 3) from packed (P, 6) or (P, 6, N) in hessian_ref.PAIRS order."""
    H = np.empty((packed.shape[0], 3, 3) + packed.shape[2:])
    for k, (c, d) in enumerate(hr.PAIRS):
        H[:, c, d] = H[:, d, c] = packed[:, k]
    return H


# ==== 1. against the mirror ==================================================================================================
@pytest.mark.parametrize('case', ['k8l2', 'default'])
def test_distances_against_the_mirror(case):
    """The layer at MAXK 8 x MAXL 2 and at the default order on the sixteen oblique rays of tests/test_ray_host.py (elevations
    30 to 85 degrees, four azimuths, no hull): the peak of every ray from its middle, and the levels 0.5 and 0.8 of
    every found peak before and behind it.  Statuses are the mirror's, and iteration counts wherever the mirror's count is a
    reference (ray_ref.steady: the stopping test stayed farther from flipping than rounding can move an iterate - every peak
    and 62 of 64 levels at k8l2, none of the converged searches at the default order, where a flipped stopping test may cost or
    save one step; tests/test_ray_host.py shows the mirror disagreeing with itself there); every peak is within
    tol + 1e-10 terms / |d2| of the mirror's distance, terms = |w . G| @ |C| the size of the slope's summands, and every crossing
    within tol + G_VALUE vterms / |d1|, vterms = |B| @ |C| - the mirror's figures at its distance; at least 8 peaks and 8
    crossings per fit have status 0 in the mirror.
    Measured in the mirror (tests/test_ray_host.py): k8l2 16 peaks at 172.0 to 292.7 km along the ray and 64 crossings; default
    12 peaks and 41 of 48 crossings.  Measured on the MI355X: k8l2 peaks 0 to 2.0e-9 m from the mirror (gate 1.27e-3 to 1.68e-3 m),
    crossings 0 to 3.0e-9 m (gate 1.36e-3 to 2.92e-3 m); default peaks 2.3e-7 to 6.4e-5 m (gate 1.9 to 17.6 m), crossings 5.9e-7
    to 1.5e-4 m (gate 4.5 to 67 m); every status the mirror's, and - steady or not - every iteration count but one: level search
    31 at the default order takes 4 steps where the mirror counts 5 in the batch and 4 with the search alone."""
    es = _layer_es(case)
    a, b, length = rays()
    (start, lo, hi), peak, (ray, level, l_lo, l_hi), lev = ray_searches(case)
    r = es.ray_peak(T_MID, *_ends(a, b), start, lo, hi, coords='ecef', check_hull=False)
    out, status, it = _raw_peak(es, es.Coeffs, a, b, start, lo, hi)
    assert r._fields == PEAK_FIELDS and r.distance.shape == (16,) and r.status.dtype == np.int32
    ran = peak['status'] != 3
    found = peak['status'] == 0
    gate = TOL + G_SLOPE * peak['terms'] / np.abs(peak['d2'])
    dist = np.abs(out[0, 0] - peak['s'])
    for k in range(16):
        print('%s ray %2d peak: status %d / mirror %d, %2d / %2d iterations, distance %.6f m, %.2e m from the mirror, gate %.2e m'
              % (case, k, status[0, k], peak['status'][k], it[0, k], peak['it'][k], out[0, 0, k], dist[k], gate[k]))
    assert np.array_equal(status[0], peak['status']) and np.array_equal(r.status, peak['status'])
    steady = rr.steady(peak, layer(case)[0], True)
    print('%s peaks: %d steady counts; iterations %s, the mirror\'s %s' % (case, steady.sum(), it[0], peak['it']))
    assert np.array_equal(it[0][steady], peak['it'][steady]) and np.array_equal(r.iterations, it[0])
    assert (steady.all() if case == 'k8l2' else True) and np.abs(it[0] - peak['it'])[~peak['short']].max() <= 1
    assert ran.all() and found.sum() >= 8 and (dist <= gate).all(), (dist, gate)
    print('%s peaks: %.2e to %.2e m from the mirror (gate %.2e to %.2e m)' % (case, dist[found].min(), dist[found].max(),
                                                                           gate[found].min(), gate[found].max()))
    assert np.array_equal(_bits(r.distance[found]), _bits(out[0, 0][found])) and np.isnan(r.distance[~found]).all()
    assert np.array_equal(_bits(r.slope), _bits(out[2, 0])) and np.array_equal(_bits(r.curvature), _bits(out[3, 0]))
    # the levels: one ray per search, the rays repeated
    rl = es.ray_level(T_MID, *_ends(a[ray], b[ray]), level, l_lo, l_hi, coords='ecef', check_hull=False)
    out, status, it = _raw_level(es, es.Coeffs, a[ray], b[ray], level, l_lo, l_hi)
    assert rl._fields == LEVEL_FIELDS and rl.distance.shape == ray.shape
    found = lev['status'] == 0
    gate = TOL + G_VALUE * lev['vterms'] / np.abs(lev['d1'])
    dist = np.abs(out[0, 0] - lev['s'])
    print(case, 'level statuses', status[0], 'mirror', lev['status'])
    print(case, 'level iterations', it[0], 'mirror', lev['it'])
    assert np.array_equal(status[0], lev['status']) and np.array_equal(rl.status, lev['status'])
    steady = rr.steady(lev, layer(case)[0], False)
    print('%s levels: %d of %d counts steady' % (case, steady.sum(), ray.size))
    assert np.array_equal(it[0][steady], lev['it'][steady]) and np.array_equal(rl.iterations, it[0])
    assert (steady.sum() >= 60 if case == 'k8l2' else True) and np.abs(it[0] - lev['it'])[~lev['short']].max() <= 1
    assert found.sum() >= 8 and (dist[found] <= gate[found]).all(), (dist, gate)
    print('%s crossings: %d found, %.2e to %.2e m from the mirror (gate %.2e to %.2e m)'
          % (case, found.sum(), dist[found].min(), dist[found].max(), gate[found].min(), gate[found].max()))
    assert np.array_equal(_bits(rl.distance[found]), _bits(out[0, 0][found])) and np.isnan(rl.distance[~found]).all()
    assert np.isnan(out[:, 0][:, ~found]).all()
    if case == 'k8l2':
        assert found.all() and ((rl.slope > 0.) == (np.arange(ray.size) % 2 == 0)).all()      # rising before the peak


# ==== 2. vertical rays =======================================================================================================
def test_vertical_rays_against_the_column_searches():
    """Rays along the geodetic normal of 40 columns from 150 to 450 km, two records of the k8l2 layer: ray_peak and ray_level
    against Estimate.peak_height and Estimate.level_height on the same columns and records - equal statuses, and the distance
    plus 150 km within 2 tol plus the two gates of the height (1e-10 terms / |curvature|, G_VALUE vterms / |slope|, each at its
    own point: twice the larger) of the height."""
    es0 = _layer_es('k8l2')
    es, times = _records('k8l2', np.stack((es0.Coeffs[0], 1.1 * es0.Coeffs[0])))
    rng = np.random.default_rng(40)
    lat, lon = rng.uniform(77., 79., 40), rng.uniform(258., 266., 40)
    start, end = (lat, lon, np.full(40, LO)), (lat, lon, np.full(40, HI))
    h0 = rng.uniform(250e3, 400e3, (2, 40))
    col = es.peak_height(times, lat, lon, h0, LO, HI, check_hull=False)
    ray = es.ray_peak(times, start, end, h0 - LO, 0., HI - LO, check_hull=False)
    assert ray.distance.shape == (2, 40) and np.array_equal(ray.status, col.status) and (col.status == 0).all()
    m = es.model
    for t in range(2):
        pts = lat, lon, col.height[t]
        uG = np.einsum('pc,pcn->pn', m.gradient_frame(*pts)[:, 2, :], m.grad_basis(*pts))
        gate = 2. * TOL + 2. * G_SLOPE * (np.abs(uG) @ np.abs(es.Coeffs[t])) / np.abs(col.curvature[t])
        diff = np.abs(ray.distance[t] + LO - col.height[t])
        print('record %d peaks: distance + 150 km within %.2e m of the height (gate %.2e m)' % (t, diff.max(), gate.min()))
        assert (diff <= gate).all()
        assert np.abs(ray.curvature[t] - col.curvature[t]).max() <= 1e-6 * np.abs(col.curvature[t]).max()
    level = 0.5 * col.value
    for lo, hi in ((np.full((2, 40), LO), col.height), (col.height, np.full((2, 40), HI))):
        cl = es.level_height(times, lat, lon, level, lo, hi, check_hull=False)
        rl = es.ray_level(times, start, end, level, lo - LO, hi - LO, check_hull=False)
        assert np.array_equal(rl.status, cl.status) and (cl.status == 0).all()
        for t in range(2):
            pts = lat, lon, cl.height[t]
            gate = 2. * TOL + 2. * G_VALUE * (np.abs(m.basis(*pts)) @ np.abs(es.Coeffs[t])) / np.abs(cl.slope[t])
            diff = np.abs(rl.distance[t] + LO - cl.height[t])
            print('record %d levels: distance + 150 km within %.2e m of the height (gate %.2e m)' % (t, diff.max(), gate.min()))
            assert (diff <= gate).all()


# ==== 3. consistency with the existing entries ===============================================================================
@functools.lru_cache(maxsize=None)
def _random_case(which):
    """(estimate, oracle, C): random coefficients at the order of `which`, scaled by the largest value of their basis function
    at the middles of the sixteen rays."""
    a, b, length = rays()
    u = rr.lines(a, b)[0]
    pts = rr.points(a, u, 0.5 * length)
    A = _bare(which).model.basis(*pts)
    C = np.random.default_rng(7).standard_normal(A.shape[1]) / np.max(np.abs(A), axis=0)
    return _bare(which, C), th._oracle(which), C


@pytest.mark.parametrize('which', ['k3l4cap15', 'k5l8cap15', 'k12l2'])
def test_values_at_the_returned_distance(which):
    """At every kernel order - (6, 4) with the series seeds of k3l4cap15, (12, 8) with k5l8cap15, (2, 12) with k12l2 - and random
    coefficients, at the points ray_points gives for the distances the searches return (every ray with status 0, 1 or 2, with
    max_iter 48 and 1): value against Estimate.__call__, slope against gradient(frame='model') . w, curvature against
    w^T hessian(frame='model') w, each within 1e-12 of the size of its terms at that point: two device summation orders of one
    quantity.  The level of a ray is the mean of the device's values at its two ends, so every bracket holds a change of sign.
    Measured on the MI355X, the largest over the twelve runs: value 2.9e-14 (k12l2), slope 2.7e-14 (k12l2), curvature 2.1e-14
    (k3l4cap15) of their terms."""
    from volumetricinterp_amd.estimate import ray_points
    es, o, C = _random_case(which)
    a, b, length = rays()
    m = es.model
    start, end = _ends(a, b)
    ends = [es(T_MID, *ray_points(start, end, s, coords='ecef'), check_hull=False) for s in (np.zeros(16), length)]
    level = 0.5 * (ends[0] + ends[1])
    for max_iter in (48, 1):
        for name, (out, status, it) in (('peak', _raw_peak(es, C, a, b, 0.5 * length, 0., length, max_iter=max_iter)),
                                        ('level', _raw_level(es, C, a, b, level, 0., length, max_iter=max_iter))):
            ran = status[0] != 3 if name == 'peak' else (status[0] == 0) | (status[0] == 2)
            print('%s %s max_iter %d: statuses %s' % (which, name, max_iter, np.bincount(status[0], minlength=4)))
            assert ran.sum() >= 8 and np.isfinite(out[:, 0][:, ran]).all()
            if name == 'level' and max_iter == 48:
                assert (status[0] == 0).all()
            s = out[0, 0]
            assert ((s[ran] >= 0.) & (s[ran] <= length[ran])).all()
            pts = tuple(v[ran] for v in ray_points(start, end, s, coords='ecef'))
            w = _direction(o, a[ran], b[ran], pts)
            t_value = np.abs(m.basis(*pts)) @ np.abs(C)
            t_slope = np.abs(np.einsum('pc,pcn->pn', w, m.grad_basis(*pts))) @ np.abs(C)
            e_value = np.abs(out[1, 0][ran] - es(T_MID, *pts, check_hull=False)) / t_value
            e_slope = np.abs(out[2, 0][ran] - np.einsum('pc,pc->p', es.gradient(T_MID, *pts, check_hull=False), w)) / t_slope
            print('%s %s max_iter %d: value %.2e, slope %.2e of their terms' % (which, name, max_iter, e_value.max(), e_slope.max()))
            assert e_value.max() <= 1e-12 and e_slope.max() <= 1e-12
            if name == 'peak':
                t_curv = np.abs(np.einsum('pc,pcdn,pd->pn', w, _sym(m.hess_basis(*pts)), w)) @ np.abs(C)
                want = np.einsum('pc,pcd,pd->p', w, es.hessian(T_MID, *pts, check_hull=False), w)
                e_curv = np.abs(out[3, 0][ran] - want) / t_curv
                print('%s peak max_iter %d: curvature %.2e of its terms' % (which, max_iter, e_curv.max()))
                assert e_curv.max() <= 1e-12


# ==== 4. launch geometry =====================================================================================================
GEOMETRY_P = 513


@functools.lru_cache(maxsize=None)
def _geometry(max_iter):
    """(estimate, C (3, N), (a, b) of 513 rays, peak arguments, level arguments, the raw results of the one call each with all
    of them): the k8l2 layer, its coefficients times 1.1 and a row of zeros; beams from the site of tests/test_ray_host.py at
    random elevations (35 to 88 degrees) and azimuths from 150 to 450 km of altitude.  Peaks: the start anywhere in the bracket,
    every 17th start NaN (status 3, no walk).  Levels: 0.2 to 1.3 of the layer's peak before the middle of the ray - a level
    above the peak has no crossing (status 1 after the two walks of the ends, next to lanes that iterate) -, every 17th NaN; row
    2: the level 0 of an all-zero record is hit exactly at lo."""
    es = _layer_es('k8l2')
    rng = np.random.default_rng(513)
    P = GEOMETRY_P
    el, az = rng.uniform(35., 88., P), rng.uniform(0., 360., P)
    sn = np.sin(np.radians(el))
    a, b = beam_ends(SITE, el, az, 150e3 / sn, 450e3 / sn)
    length = rr.lines(a, b)[1]
    C = np.stack((es.Coeffs[0], 1.1 * es.Coeffs[0], np.zeros_like(es.Coeffs[0])))
    lo = rng.uniform(0., 0.1, (3, P)) * length
    hi = np.broadcast_to(length, (3, P)).copy()
    start = lo + rng.uniform(0., 1., (3, P)) * (hi - lo)
    start[:, ::17] = np.nan
    level = rng.uniform(0.2, 1.3, (3, P)) * 2.8e11
    level[:2, ::17] = np.nan
    level[2] = 0.
    l_hi = 0.55 * hi
    peak = _raw_peak(es, C, a, b, start, lo, hi, max_iter=max_iter)
    lev = _raw_level(es, C, a, b, level, lo, l_hi, max_iter=max_iter)
    return es, C, (a, b), (start, lo, hi), (level, lo, l_hi), peak, lev


@pytest.mark.parametrize('max_iter', [48, 1, 0])
def test_every_ray_has_the_bits_of_its_search_alone(max_iter):
    """The calls with 3 x 513 points against calls with P = 1, T = 1 for the 64 lanes of the second wave of every row: the same
    bits.  In those waves lanes that never walk (status 3), lanes that stop early and lanes that use up max_iter sit next to
    each other: a stopped lane is frozen while the wave goes on."""
    es, C, (a, b), pk_args, lv_args, peak, lev = _geometry(max_iter)
    for name, full in (('peak', peak), ('level', lev)):
        print('%s max_iter %d: statuses %s, iterations up to %d' % (name, max_iter, np.bincount(full[1].ravel(), minlength=4),
                                                                     full[2].max()))
    wave = slice(64, 128)
    for t in range(2):
        assert (peak[1][t, wave] == 3).sum() >= 3 and (lev[1][t, wave] == 3).sum() >= 3 and (lev[1][t, wave] == 1).sum() >= 5
        if max_iter == 48:
            assert (peak[1][t, wave] == 0).sum() >= 20 and (lev[1][t, wave] == 0).sum() >= 20 and peak[2][t, wave].max() >= 3
        else:
            assert (peak[1][t, wave] == 2).sum() >= 20 and (peak[2][t, wave][peak[1][t, wave] == 2] == max_iter).all()
            assert (lev[1][t, wave] == 2).sum() >= 20
    assert (lev[1][2] == 0).all() and (lev[2][2] == 0).all() and np.array_equal(lev[0][0, 2], lv_args[1][2])
    for t in range(3):
        for q in range(64, 128):
            one = _raw_peak(es, C[t], a[q], b[q], *(v[t, q] for v in pk_args), max_iter=max_iter)
            _same_bits(one, _take(peak, slice(t, t + 1), slice(q, q + 1)), ('peak', t, q))
            one = _raw_level(es, C[t], a[q], b[q], *(v[t, q] for v in lv_args), max_iter=max_iter)
            _same_bits(one, _take(lev, slice(t, t + 1), slice(q, q + 1)), ('level', t, q))


@pytest.mark.parametrize('T', [1, 2, 3])
@pytest.mark.parametrize('P', [1, 63, 64, 65, 255, 256, 257, 513])
def test_launch_geometry(P, T):
    """A block is 256 lanes, a wave 64: the fields of a point are the same bits whatever P and T are and wherever the ray sits
    - the first P, the last P and a random draw of P of the 513 rays in a random order, the first T and the last T of the three
    rows, against the call with all of them; max_iter = 48, 1 and 0."""
    rng = np.random.default_rng(1000 * T + P)
    for max_iter in (48, 1, 0):
        es, C, (a, b), pk_args, lv_args, peak, lev = _geometry(max_iter)
        for rows in (slice(0, T), slice(3 - T, 3)):
            for cols in (np.arange(P), np.arange(GEOMETRY_P - P, GEOMETRY_P), rng.permutation(GEOMETRY_P)[:P]):
                r = _raw_peak(es, C[rows], a[cols], b[cols], *(v[rows][:, cols] for v in pk_args), max_iter=max_iter)
                assert r[0].shape == (4, T, P)
                _same_bits(r, _take(peak, rows, cols), ('peak', P, T, max_iter))
                r = _raw_level(es, C[rows], a[cols], b[cols], *(v[rows][:, cols] for v in lv_args), max_iter=max_iter)
                assert r[0].shape == (3, T, P)
                _same_bits(r, _take(lev, rows, cols), ('level', P, T, max_iter))


def test_more_rows_than_a_grid_holds():
    """T = 65 537 rows - one more than two slices of 65 535 hold, the third slice a single row -, one ray, the same coefficient
    row, start, bracket and level in every row: every result has the bits of the first."""
    es = _layer_es('k8l2')
    a, b, length = rays()
    (start, lo, hi), peak, (ray, level, l_lo, l_hi), lev = ray_searches('k8l2')
    T = 65537
    C = np.tile(es.Coeffs[0], (T, 1))
    out, status, it = _raw_peak(es, C, a[5], b[5], start[5], lo[5], hi[5])
    assert status[0, 0] == 0 and it[0, 0] == peak['it'][5]
    assert (status == status[0, 0]).all() and (it == it[0, 0]).all() and (_bits(out) == _bits(out[:, :1])).all()
    j = int(np.flatnonzero(ray == 5)[0])
    out, status, it = _raw_level(es, C, a[5], b[5], level[j], l_lo[j], l_hi[j])
    assert status[0, 0] == 0 and it[0, 0] == lev['it'][j]
    assert (status == status[0, 0]).all() and (it == it[0, 0]).all() and (_bits(out) == _bits(out[:, :1])).all()


def test_public_method_shapes_and_records():
    """ray_peak and ray_level with a list of three datetimes give (3,) + S, with one datetime S; record t of the batch has the
    bits of the same record alone, with its own start, level and brackets; S may have any rank; geodetic end points."""
    from volumetricinterp_amd import geodesy
    es0 = _layer_es('k8l2')
    C = np.stack((es0.Coeffs[0], 1.1 * es0.Coeffs[0], 0.9 * es0.Coeffs[0]))
    es, times = _records('k8l2', C)
    rng = np.random.default_rng(70)
    el, az = rng.uniform(40., 85., 70), rng.uniform(0., 360., 70)
    sn = np.sin(np.radians(el))
    a, b = beam_ends(SITE, el, az, 150e3 / sn, 450e3 / sn)
    length = rr.lines(a, b)[1].reshape(7, 10)
    start, end = (tuple(v.reshape(7, 10) for v in geodesy.ecef2geodetic(*x.T)) for x in (a, b))
    s0 = rng.uniform(0.3, 0.7, (3, 7, 10)) * length
    level = rng.uniform(0.3, 0.9, (3, 7, 10)) * 2.8e11
    batch = es.ray_peak(times, start, end, s0, 0., length, check_hull=False)
    lbatch = es.ray_level(times, start, end, level, 0., 0.5 * length, check_hull=False)
    assert batch.distance.shape == (3, 7, 10) and (batch.status == 0).sum() >= 150
    assert lbatch.distance.shape == (3, 7, 10) and (lbatch.status == 0).sum() >= 100
    for i in range(3):
        one = es.ray_peak(times[i], start, end, s0[i], 0., length, check_hull=False)
        assert one.distance.shape == (7, 10)
        _same_bits(one, tuple(f[i] for f in batch), i)
        one = es.ray_level(times[i], start, end, level[i], 0., 0.5 * length, check_hull=False)
        _same_bits(one, tuple(f[i] for f in lbatch), i)


# ==== 5. kind and direction ==================================================================================================
def test_min_of_the_negated_coefficients():
    """kind='min' on -C walks the distances of kind='max' on C bit for bit - every comparison of the iteration carries the sign
    - with value, slope and curvature negated; statuses and iterations the same."""
    es = _layer_es('k8l2')
    a, b, length = rays()
    (start, lo, hi), peak, _, _ = ray_searches('k8l2')
    neg = _bare('k8l2', -es.Coeffs[0])
    x = _raw_peak(es, es.Coeffs, a, b, start, lo, hi, kind=1)
    y = _raw_peak(neg, neg.Coeffs, a, b, start, lo, hi, kind=-1)
    assert np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) and (x[1] == 0).all()
    assert np.array_equal(_bits(x[0][0]), _bits(y[0][0])) and np.array_equal(_bits(x[0][1:]), _bits(-y[0][1:]))
    rx = es.ray_peak(T_MID, *_ends(a, b), start, lo, hi, kind='max', coords='ecef', check_hull=False)
    ry = neg.ray_peak(T_MID, *_ends(a, b), start, lo, hi, kind='min', coords='ecef', check_hull=False)
    assert np.array_equal(_bits(rx.distance), _bits(ry.distance)) and np.array_equal(_bits(rx.value), _bits(-ry.value))


def test_reversed_rays():
    """The ray from b to a with the mirrored start and bracket: the peak and the crossings lie at len - distance within 2 tol
    (each search is within tol of the same zero), with the same statuses.  At one point seen from both ends - max_iter = 0
    evaluates the start, len - s of the reversed ray is the same point to rounding - the slope has the opposite sign and the
    curvature the same, within the sum of the two term gates (1e-12 of the size of the terms, once per evaluation)."""
    es = _layer_es('k8l2')
    o, C = layer('k8l2')
    a, b, length = rays()
    (start, lo, hi), peak, (ray, level, l_lo, l_hi), lev = ray_searches('k8l2')
    fwd = es.ray_peak(T_MID, *_ends(a, b), start, lo, hi, coords='ecef', check_hull=False)
    rev = es.ray_peak(T_MID, *_ends(b, a), length - start, length - hi, length - lo, coords='ecef', check_hull=False)
    assert (fwd.status == 0).all() and (rev.status == 0).all()
    print('peaks: len - distance of the reversed ray within %.2e m' % np.abs(length - rev.distance - fwd.distance).max())
    assert np.abs(length - rev.distance - fwd.distance).max() <= 2. * TOL
    lf = es.ray_level(T_MID, *_ends(a[ray], b[ray]), level, l_lo, l_hi, coords='ecef', check_hull=False)
    lr = es.ray_level(T_MID, *_ends(b[ray], a[ray]), level, length[ray] - l_hi, length[ray] - l_lo, coords='ecef',
                      check_hull=False)
    assert (lf.status == 0).all() and (lr.status == 0).all()
    assert np.abs(length[ray] - lr.distance - lf.distance).max() <= 2. * TOL
    assert ((lf.slope > 0.) == (lr.slope < 0.)).all()
    s = peak['s'] + 10e3                                                    # off the peak: a slope to compare
    f = _raw_peak(es, C, a, b, s, 0., length, max_iter=0)[0][:, 0]
    r = _raw_peak(es, C, b, a, length - s, 0., length, max_iter=0)[0][:, 0]
    m = es.model
    pts = rr.points(a, rr.lines(a, b)[0], s)
    w = _direction(o, a, b, pts)
    t_slope = np.abs(np.einsum('pc,pcn->pn', w, m.grad_basis(*pts))) @ np.abs(C)
    t_curv = np.abs(np.einsum('pc,pcdn,pd->pn', w, _sym(m.hess_basis(*pts)), w)) @ np.abs(C)
    t_value = np.abs(m.basis(*pts)) @ np.abs(C)
    print('one point from both ends: value %.2e, slope %.2e, curvature %.2e of their terms'
          % ((np.abs(f[1] - r[1]) / t_value).max(), (np.abs(f[2] + r[2]) / t_slope).max(), (np.abs(f[3] - r[3]) / t_curv).max()))
    assert (np.abs(f[1] - r[1]) <= 2e-12 * t_value).all()
    assert (np.abs(f[2] + r[2]) <= 2e-12 * t_slope).all() and (f[2] != 0.).all()
    assert (np.abs(f[3] - r[3]) <= 2e-12 * t_curv).all()


# ==== 6. statuses ============================================================================================================
def test_every_status():
    """By construction, on ray 8 of the k8l2 layer.  Peak: a bracket that ends before the peak has no interior peak (1: the
    search runs onto its upper end); max_iter 0 and 2 (2; the raw output holds the last iterate, the public method blanks
    distance and value); a NaN start, a NaN bound, lo > hi, a start outside the bracket, a NaN end point and a ray of length
    zero (3).  Level: a level above the peak (1, no iteration); max_iter 0 and 1 (2); a NaN level, a NaN bound, lo >= hi, a ray
    of length zero (3); an all-zero record and the level 0: an exact hit at lo (0 with no iteration, slope 0)."""
    es = _layer_es('k8l2')
    a, b, length = rays()
    (start, lo, hi), peak, (ray, level, l_lo, l_hi), lev = ray_searches('k8l2')
    k = 8
    A, B, L, sp = a[k:k + 1], b[k:k + 1], length[k], peak['s'][k]
    ends = _ends(A, B)
    kw = dict(coords='ecef', check_hull=False)
    r = es.ray_peak(T_MID, *ends, 0.3 * sp, 0., 0.6 * sp, **kw)
    assert r.status[0] == 1 and np.isnan(r.distance[0]) and np.isnan(r.value[0]) and r.slope[0] > 0.
    out = _raw_peak(es, es.Coeffs, A, B, 0.3 * sp, 0., 0.6 * sp)[0]
    assert abs(out[0, 0, 0] - 0.6 * sp) <= 2. * TOL
    for max_iter in (0, 2):
        out, status, it = _raw_peak(es, es.Coeffs, A, B, start[k], 0., L, max_iter=max_iter)
        assert status[0, 0] == 2 and it[0, 0] == max_iter and np.isfinite(out[:, 0, 0]).all()
        if max_iter == 0:
            assert out[0, 0, 0] == start[k]
        r = es.ray_peak(T_MID, *ends, start[k], 0., L, max_iter=max_iter, **kw)
        assert r.status[0] == 2 and r.iterations[0] == max_iter and np.isnan(r.distance[0]) and np.isnan(r.value[0])
        assert r.slope[0] == out[2, 0, 0] and r.curvature[0] == out[3, 0, 0]
    nan = np.nan
    A8, B8 = np.repeat(A, 8, axis=0), np.repeat(B, 8, axis=0)
    A8[6, 1] = nan
    B8[7] = A8[7]
    s0 = np.array([sp, nan, sp, sp, sp, 1.1 * L, sp, 0.])
    lo8 = np.array([0., 0., nan, 0., L, 0., 0., 0.])
    hi8 = np.array([L, L, L, nan, 0., L, L, 0.])
    bad = es.ray_peak(T_MID, *_ends(A8, B8), s0, lo8, hi8, **kw)
    assert list(bad.status) == [0] + [3] * 7 and (bad.iterations[1:] == 0).all()
    assert all(np.isnan(v[1:]).all() for v in bad[:4]) and np.isfinite(bad.distance[0])
    # the level search
    j = int(np.flatnonzero(ray == k)[0])
    r = es.ray_level(T_MID, *ends, 10. * level[j], l_lo[j], l_hi[j], **kw)
    assert r.status[0] == 1 and r.iterations[0] == 0 and all(np.isnan(v[0]) for v in r[:3])
    for max_iter in (0, 1):
        out, status, it = _raw_level(es, es.Coeffs, A, B, level[j], l_lo[j], l_hi[j], max_iter=max_iter)
        mirror = rr.level_search(layer('k8l2')[0], es.Coeffs[0], A, B, level[j], l_lo[j], l_hi[j], TOL, max_iter)
        assert status[0, 0] == 2 and it[0, 0] == max_iter and mirror['status'][0] == 2 and mirror['it'][0] == max_iter
        assert l_lo[j] < out[0, 0, 0] < l_hi[j] and abs(out[0, 0, 0] - mirror['s'][0]) <= 1e-6 * (l_hi[j] - l_lo[j])
        r = es.ray_level(T_MID, *ends, level[j], l_lo[j], l_hi[j], max_iter=max_iter, **kw)
        assert r.status[0] == 2 and r.iterations[0] == max_iter and np.isnan(r.distance[0]) and r.slope[0] == out[2, 0, 0]
    A6, B6 = np.repeat(A, 6, axis=0), np.repeat(B, 6, axis=0)
    B6[5] = A6[5]
    bad = es.ray_level(T_MID, *_ends(A6, B6), [level[j], nan, level[j], level[j], level[j], level[j]],
                       [l_lo[j], l_lo[j], nan, l_hi[j], l_hi[j], l_lo[j]], [l_hi[j], l_hi[j], l_hi[j], l_hi[j], l_lo[j], l_hi[j]],
                       **kw)
    assert list(bad.status) == [0] + [3] * 5 and (bad.iterations[1:] == 0).all()
    assert all(np.isnan(v[1:]).all() for v in bad[:3]) and np.isfinite(bad.distance[0])
    zero = _bare('k8l2')
    out, status, it = _raw_level(zero, zero.Coeffs, a, b, 0., 0.1 * length, length)
    assert (status == 0).all() and (it == 0).all() and np.array_equal(out[0, 0], 0.1 * length) and (out[1:] == 0.).all()
    z = zero.ray_level(T_MID, *_ends(a, b), 0., 0.1 * length, length, **kw)
    assert (z.status == 0).all() and np.array_equal(z.distance, 0.1 * length) and (z.slope == 0.).all()


def test_a_nan_record_reaches_only_itself():
    """Three records, one NaN in the second: that record is status 3 and NaN on every ray, the other two keep the bits they
    have without it - both searches."""
    es0 = _layer_es('k8l2')
    C = np.stack((es0.Coeffs[0], 1.1 * es0.Coeffs[0], 0.9 * es0.Coeffs[0]))
    Cn = C.copy()
    Cn[1, 5] = np.nan
    a, b, length = rays()
    for good, r in ((_raw_peak(es0, C, a, b, 0.5 * length, 0., length), _raw_peak(es0, Cn, a, b, 0.5 * length, 0., length)),
                    (_raw_level(es0, C, a, b, 1.4e11, 0., 0.5 * length), _raw_level(es0, Cn, a, b, 1.4e11, 0., 0.5 * length))):
        assert (good[1] == 0).all()
        assert (r[1][1] == 3).all() and np.isnan(r[0][:, 1]).all() and (r[2][1] == 0).all()
        for i in (0, 2):
            _same_bits(_take(r, slice(i, i + 1), slice(None)), _take(good, slice(i, i + 1), slice(None)), i)
    bad, times = _records('k8l2', Cn)
    pub = bad.ray_peak(times, *_ends(a, b), 0.5 * length, 0., length, coords='ecef', check_hull=False)
    assert (pub.status[1] == 3).all() and (pub.status[[0, 2]] == 0).all()


# ==== 7. the hull ============================================================================================================
def test_both_ends_go_through_the_hull():
    """192 rays from a ground site through the Qhull hull of the default fixture, brackets drawn on the chord of each ray so that
    either end is inside or outside, never closer than 1 m to a facet (the largest plane distance of every end is at most -1 m
    or at least +1 m, so the fp64 criterion of the kernel and est.check_hull's mask pass cannot disagree): status 3 and NaN
    exactly where the lower or the upper end is outside - one end outside is enough, the first wave has no lower end inside and
    leaves before any walk -, the brackets with both ends inside are searched and keep the bits they have without the hull
    test, and every returned point passes est.check_hull."""
    from volumetricinterp_amd.estimate import ray_points, ray_samples
    f, es, _ = _estimate('default')
    eq, tol = es._hull()
    a, b = rays_into_hull(f['hull_vert'], 192, 192)
    start, end = _ends(a, b)
    u, length = rr.lines(a, b)
    dist = ray_samples(eq, tol, start, end, 2, coords='ecef')[0]
    c0, c1 = dist[:, 0], dist[:, 1]
    assert np.isfinite(c0).all() and (c0 > 0.).all() and (c1 < length).all()      # the site and the far end are outside
    rng = np.random.default_rng(192)
    lo = c0 + rng.uniform(0.05, 0.3, 192) * (c1 - c0)
    hi = c0 + rng.uniform(0.6, 0.95, 192) * (c1 - c0)
    hi[::3] = c1[::3] + rng.uniform(0.05, 0.3, 64) * (c1 - c0)[::3]
    lo[:64] = c0[:64] * rng.uniform(0.3, 0.9, 64)
    plane = lambda s: ((a + s[:, None] * u) @ eq[:, :3].T + eq[:, 3]).max(axis=1)
    g_lo, g_hi = plane(lo), plane(hi)
    assert (np.abs(g_lo) >= 1.).all() and (np.abs(g_hi) >= 1.).all()
    in_lo, in_hi = g_lo < 0., g_hi < 0.
    inside = in_lo & in_hi
    assert inside.sum() >= 10 and (in_lo & ~in_hi).sum() >= 5 and (~in_lo & in_hi).sum() >= 5 and not in_lo[:64].any()
    for s, ok in ((lo, in_lo), (hi, in_hi)):
        assert np.array_equal(es.check_hull(*ray_points(start, end, s, coords='ecef')), ok)
    t = _t_rec(f)
    s0 = 0.5 * (lo + hi)
    r = es.ray_peak(t, start, end, s0, lo, hi, coords='ecef')
    free = es.ray_peak(t, start, end, s0, lo, hi, coords='ecef', check_hull=False)
    assert np.array_equal(r.status == 3, ~inside) and (free.status != 3).all()
    assert all(np.isnan(v[~inside]).all() for v in r[:4]) and (r.iterations[~inside] == 0).all()
    _same_bits(tuple(v[inside] for v in r), tuple(v[inside] for v in free))
    ok = r.status == 0
    print('peaks: statuses %s' % np.bincount(r.status, minlength=4))
    assert es.check_hull(*(v[ok] for v in ray_points(start, end, r.distance, coords='ecef'))).all()
    ends = [es(t, *ray_points(start, end, s, coords='ecef'), check_hull=False) for s in (lo, hi)]
    level = 0.5 * (ends[0] + ends[1])
    r = es.ray_level(t, start, end, level, lo, hi, coords='ecef')
    free = es.ray_level(t, start, end, level, lo, hi, coords='ecef', check_hull=False)
    assert np.array_equal(r.status == 3, ~inside) and (free.status != 3).all()
    assert all(np.isnan(v[~inside]).all() for v in r[:3]) and (r.iterations[~inside] == 0).all()
    _same_bits(tuple(v[inside] for v in r), tuple(v[inside] for v in free))
    ok = r.status == 0
    print('levels: statuses %s' % np.bincount(r.status, minlength=4))
    assert ok.sum() >= 5 and es.check_hull(*(v[ok] for v in ray_points(start, end, r.distance, coords='ecef'))).all()


# ==== 8. errors ==============================================================================================================
def test_error_bars():
    """error=True on the layer with the covariance of the k8l2 fixture's first record, against the composed formula on the
    public methods at ray_points(distance): distance_error = sqrt(w^T cov w) / |curvature| with gradient_covariance(frame=
    'model') and value_error = error() for the peak, distance_error = error() / |slope| for the level - w formed here from the
    oracle's axes, so to rounding (1e-9), the value errors bit for bit; the fields before them are those of error=False; NaN
    where the status is not 0.  Without a covariance it raises, as the error entries do."""
    from volumetricinterp_amd.estimate import Estimate, ray_points
    f = load_golden('fit_k8l2')
    layer_es = _layer_es('k8l2')
    o = layer('k8l2')[0]
    es = Estimate.from_arrays(layer_es.Coeffs, f['Covariance'][:1], [[0., 60.]], np.zeros((4, 3)), layer_es.config_file_text)
    a, b, length = rays()
    (start, lo, hi), peak, (ray, level, l_lo, l_hi), lev = ray_searches('k8l2')
    nan = np.nan
    a17, b17 = np.vstack((a, a[:1])), np.vstack((b, b[:1]))
    args = tuple(np.append(v, x) for v, x in ((start, nan), (lo, 0.), (hi, length[0])))
    kw = dict(coords='ecef', check_hull=False)
    r = es.ray_peak(T_MID, *_ends(a17, b17), *args, error=True, **kw)
    assert r._fields == PEAK_FIELDS + ('distance_error', 'value_error') and r.distance_error.shape == (17,)
    _same_bits(r[:6], es.ray_peak(T_MID, *_ends(a17, b17), *args, **kw))
    ok = r.status == 0
    assert ok[:16].all() and r.status[16] == 3 and np.isnan(r.distance_error[16]) and np.isnan(r.value_error[16])
    pts = tuple(v[ok] for v in ray_points(*_ends(a17, b17), r.distance, coords='ecef'))
    w = _direction(o, a17[ok], b17[ok], pts)
    cov = np.einsum('pc,pcd,pd->p', w, es.gradient_covariance(T_MID, *pts, check_hull=False, frame='model'), w)
    assert (cov > 0.).all()
    assert np.allclose(r.distance_error[ok], np.sqrt(cov) / np.abs(r.curvature[ok]), rtol=1e-9, atol=0.)
    assert np.array_equal(r.value_error[ok], es.error(T_MID, *pts, check_hull=False))
    print('distance errors %s m, value errors %s' % (r.distance_error[:16:5], r.value_error[:16:5]))
    ends = _ends(np.vstack((a[ray], a[:1])), np.vstack((b[ray], b[:1])))
    largs = tuple(np.append(v, x) for v, x in ((level, nan), (l_lo, 0.), (l_hi, length[0])))
    rl = es.ray_level(T_MID, *ends, *largs, error=True, **kw)
    assert rl._fields == LEVEL_FIELDS + ('distance_error',)
    _same_bits(rl[:5], es.ray_level(T_MID, *ends, *largs, **kw))
    ok = rl.status == 0
    assert ok[:-1].all() and rl.status[-1] == 3 and np.isnan(rl.distance_error[-1])
    pts = tuple(v[ok] for v in ray_points(*ends, rl.distance, coords='ecef'))
    err = es.error(T_MID, *pts, check_hull=False)
    assert (err > 0.).all() and np.array_equal(rl.distance_error[ok], err / np.abs(rl.slope[ok]))
    bare = Estimate.from_arrays(layer_es.Coeffs, None, [[0., 60.]], np.zeros((4, 3)), layer_es.config_file_text)
    for call in (lambda: bare.ray_peak(T_MID, *_ends(a, b), start, lo, hi, error=True, **kw),
                 lambda: bare.ray_level(T_MID, *_ends(a[ray], b[ray]), level, l_lo, l_hi, error=True, **kw)):
        with pytest.raises(ValueError, match='no covariance'):
            call()


# ==== 9. refusals and timing =================================================================================================
def test_refusals():
    """An order beyond the gradient's (MAXL 13) and the radial-basis model: VI_ERR_UNSUPPORTED (-6) from the library,
    VinterpError from Python.  A bad kind, tol or max_iter (above 10 000 too), a null pointer, a negative size and facets
    counted but not given: VI_ERR_INVALID (-1), ValueError from Python; so are arguments that do not broadcast and bad coords.
    Nothing was launched by any of them: the output buffers are untouched, and with the context's timing on, the kernel time it
    reports is still that of the call before - the events of a launch were not recorded again.  T = 0 and P = 0 are no-ops."""
    from volumetricinterp_amd import _lib
    from volumetricinterp_amd.estimate import Estimate
    a, b, length = rays()
    P = 16
    th.BASIS_CASES['k2l13'] = (2, 13, 10.)
    try:
        big = _bare('k2l13')
    finally:
        del th.BASIS_CASES['k2l13']
    fr = load_golden('fit_rbf')
    rbf = Estimate.from_arrays(fr['Coeffs'], fr['Covariance'], fr['utime'], fr['hull_vert'], str(fr['cfg']))
    ok = _bare('default', np.ones(144))
    aT, bT = np.ascontiguousarray(a.T), np.ascontiguousarray(b.T)

    def call(entry, es, dev, T=1, np_=P, kind=1, max_iter=48, tol=TOL, F=0, null=None):
        N = es.model.nbasis
        peak = entry == 'vi_eval_ray_peak_f64'
        per = [0.5 * length, np.zeros(P), length] if peak else [np.stack((np.zeros(P), length)), np.full(P, 1.)]
        d = [dev.up(v) for v in [aT, bT] + per + [np.ones(N)]]
        rows = 4 if peak else 3
        dO, dS, dI = dev.up(np.full(rows * P, 7.)), dev.up(np.full(P, 7, dtype=np.int32)), dev.up(np.full(P, 7, dtype=np.int32))
        p = [v.ptr for v in d] + [None, F, 0.] + ([kind] if peak else []) + [max_iter, tol, dO.ptr, dS.ptr, dI.ptr]
        if null is not None:
            p[null] = None
        rc = getattr(_lib.lib, entry)(es.model.handle(), T, np_, *p)
        es.model.ctx.sync()
        assert np.array_equal(dO.download(), np.full(rows * P, 7.))
        assert np.array_equal(dS.download(), np.full(P, 7)) and np.array_equal(dI.download(), np.full(P, 7))
        return rc

    kw = dict(coords='ecef', check_hull=False)
    ctx = ok.model.ctx
    ctx.eval_timing(True)
    try:
        ok.ray_peak(T_MID, *_ends(a, b), 0.5 * length, 0., length, **kw)
        before = ctx.eval_kernel_ms()
        assert 0. < before < 1000.
        for entry, nptr in (('vi_eval_ray_peak_f64', 6), ('vi_eval_ray_level_f64', 5)):
            for es, what in ((big, 'beyond the compiled limits'), (rbf, 'only the sphharmlag model')):
                with es.model.ctx.scope() as dev:
                    assert call(entry, es, dev) == -6 and what in _lib.lib.vi_last_error().decode()
            with ctx.scope() as dev:
                bads = [dict(tol=0.), dict(tol=-1.), dict(tol=np.nan), dict(tol=np.inf), dict(max_iter=-1), dict(max_iter=10001),
                        dict(F=3), dict(T=-1), dict(np_=-1)] + [dict(null=i) for i in range(nptr)]
                out0 = nptr + 3 + (3 if entry == 'vi_eval_ray_peak_f64' else 2)
                bads += [dict(null=out0), dict(null=out0 + 1)]
                if entry == 'vi_eval_ray_peak_f64':
                    bads += [dict(kind=0), dict(kind=2)]
                for bad in bads:
                    assert call(entry, ok, dev, **bad) == -1, (entry, bad)
                assert call(entry, ok, dev, T=0) == 0 and call(entry, ok, dev, np_=0) == 0
        for es, what, t in ((big, 'beyond the compiled limits', T_MID), (rbf, 'only the sphharmlag model', _t_rec(fr))):
            with pytest.raises(_lib.VinterpError, match=what):
                es.ray_peak(t, *_ends(a, b), 0.5 * length, 0., length, **kw)
            with pytest.raises(_lib.VinterpError, match=what):
                es.ray_level(t, *_ends(a, b), 1., 0., length, **kw)
        for bad in (dict(tol=0.), dict(tol=np.nan), dict(max_iter=-1), dict(max_iter=1.5), dict(max_iter=10001), dict(max_iter=True)):
            with pytest.raises(ValueError, match='tol must be|max_iter must be'):
                ok.ray_peak(T_MID, *_ends(a, b), 0.5 * length, 0., length, **kw, **bad)
            with pytest.raises(ValueError, match='tol must be|max_iter must be'):
                ok.ray_level(T_MID, *_ends(a, b), 1., 0., length, **kw, **bad)
        with pytest.raises(ValueError, match='kind must be'):
            ok.ray_peak(T_MID, *_ends(a, b), 0.5 * length, 0., length, kind='saddle', **kw)
        with pytest.raises(ValueError, match='broadcast'):
            ok.ray_peak(T_MID, *_ends(a, b), np.zeros(P + 1), 0., length, **kw)
        with pytest.raises(ValueError, match='broadcast'):
            ok.ray_level(T_MID, *_ends(a, b), 1., 0., np.zeros(P + 1), **kw)
        with pytest.raises(ValueError, match='do not broadcast'):
            ok.ray_peak(T_MID, _ends(a, b)[0], _ends(a[:5], b[:5])[1], 0.5, 0., 1., **kw)
        for method, args in ((ok.ray_peak, (0.5 * length, 0., length)), (ok.ray_level, (1., 0., length))):
            with pytest.raises(ValueError, match='coords must be'):
                method(T_MID, *_ends(a, b), *args, coords='enu', check_hull=False)
        assert ctx.eval_kernel_ms() == before                                 # nothing was launched since
        ok.ray_level(T_MID, *_ends(a, b), 1., 0., length, **kw)
        assert 0. < ctx.eval_kernel_ms() < 1000.
    finally:
        ctx.eval_timing(False)
    empty = ok.ray_peak([], *_ends(a, b), 0.5 * length, 0., length, **kw)
    assert all(v.shape == (0, P) for v in empty)
    empty = ok.ray_level(T_MID, *_ends(a[:0], b[:0]), 1., 0., 1., **kw)
    assert all(v.shape == (0,) for v in empty) and empty.status.dtype == np.int32
    # the null d_iter is allowed
    with ctx.scope() as dev:
        d = [dev.up(v) for v in (aT, bT, 0.5 * length, np.zeros(P), length, np.ones(144))]
        dO, dS = dev.empty((4, P)), dev.empty(P, np.int32)
        assert _lib.lib.vi_eval_ray_peak_f64(ok.model.handle(), 1, P, *(v.ptr for v in d), None, 0, 0., 1, 48, TOL, dO.ptr, dS.ptr,
                                             None) == 0
        assert np.isin(dS.download(), (0, 1, 2, 3)).all()


# ==== 10. the recipe =========================================================================================================
def test_from_samples_to_the_refined_peak_and_crossing():
    """The README's recipe end to end at S = (5, 7), n = 32, T = 3 on three records of the k8l2 layer with the hull of the k8l2
    fixture (the layer was fitted on the fixture's beams): ray_samples ->
    resident_grid on the samples -> peak / crossing along the last axis -> ray_peak_brackets / ray_level_brackets -> ray_peak /
    ray_level.  One of the 35 rays misses the hull: NaN samples, index -1, status 3.  Every status-0 result lies inside its
    bracket; every status-0 peak is at least as high as the best sample of its ray (to the 1e-10 of the terms between the
    grid's product and the walk), and every bracketed crossing is found."""
    from volumetricinterp_amd.estimate import ray_level_brackets, ray_peak_brackets, ray_samples
    import datetime as dt
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_k8l2')
    es0 = _layer_es('k8l2')
    C = np.stack((es0.Coeffs[0], 1.1 * es0.Coeffs[0], 0.9 * es0.Coeffs[0]))
    es = Estimate.from_arrays(C, np.zeros((3,) + 2 * C.shape[1:]), [[60. * t, 60. * t + 60.] for t in range(3)], f['hull_vert'],
                              es0.config_file_text)
    times = [dt.datetime(1970, 1, 1) + dt.timedelta(seconds=60. * t + 30.) for t in range(3)]
    eq, tol = es._hull()
    a, b = rays_into_hull(f['hull_vert'], 35, 35)
    b[3] = a[3] + (a[3] - b[3])                                             # into the ground: a miss
    start, end = tuple(a.T.reshape(3, 5, 7)), tuple(b.T.reshape(3, 5, 7))
    dist, lat, lon, alt = ray_samples(eq, tol, start, end, 32, coords='ecef')
    miss = np.isnan(dist[..., 0])
    assert miss.sum() == 1 and miss[0, 3]
    with es.resident_grid(lat, lon, alt) as g:
        vol = g(times)
        value, index = g.peak(times)
        level = 0.5 * value
        cross = g.crossing(times, level, which='first', direction='up')
    assert index.shape == (3, 5, 7) and (index[:, miss] == -1).all() and (index[:, ~miss] >= 0).all()
    s0, lo, hi = ray_peak_brackets(dist, index)
    r = es.ray_peak(times, start, end, s0, lo, hi, coords='ecef')
    assert r.distance.shape == (3, 5, 7) and (r.status[:, miss] == 3).all() and (r.status[:, ~miss] != 3).all()
    ok = r.status == 0
    print('peaks: statuses %s, iterations up to %d' % (np.bincount(r.status.ravel(), minlength=4), r.iterations.max()))
    assert ok.sum() >= 20
    assert ((r.distance[ok] >= lo[ok]) & (r.distance[ok] <= hi[ok])).all()
    C = np.array([es.get_C(t)[0] for t in times])
    terms = np.einsum('tn,pn->tp', np.abs(C), np.abs(es.model.basis(*(v[~miss].ravel() for v in (lat, lon, alt))))).max()
    assert (r.value[ok] >= value[ok] - 1e-10 * terms).all()
    has = cross >= 0
    l_lo, l_hi = ray_level_brackets(dist, cross)
    rl = es.ray_level(times, start, end, level, l_lo, l_hi, coords='ecef')
    print('crossings: %d bracketed, statuses %s' % (has.sum(), np.bincount(rl.status.ravel(), minlength=4)))
    assert has.sum() >= 20 and (rl.status[~has] == 3).all()
    found = rl.status == 0
    # (status 1: a sample within rounding of the level, whose change of sign the walk does not see)
    assert np.isin(rl.status[has], (0, 1)).all() and found.sum() >= 20
    assert ((rl.distance[found] >= l_lo[found]) & (rl.distance[found] <= l_hi[found])).all() and (rl.slope[found] > 0.).all()
    assert (np.abs(rl.value[found] - level[found]) <= np.abs(rl.slope[found]) * TOL + 1e-10 * terms).all()
