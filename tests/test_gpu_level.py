"""GPU tests of the level crossings: Estimate.level_height (vi_eval_level_f64, kernel k_level_sph: a lane per column, one
gradient walk of the chains per iteration for the value and the slope along the geodetic normal) and the crossing maps of a
resident grid (ResidentGrid.crossing, vi_eval_resident_cross_f64).

The reference project has neither.  The yardstick of the heights is tests/level_ref.py, the device iteration in NumPy on the
oracle's basis and gradient basis, which tests/test_level_host.py holds against scipy.optimize.brentq; the yardstick of the maps
is level_ref.crossing_index, a plain loop over the downloaded volume.  Gates: a height within tol + 1e-10 terms / |slope| of the
mirror's - tol is what the search promises, 1e-10 of the value's terms the project's gate of the device's value against the
oracle's basis (test_gpu_basis_eval.py::test_eval_many_timesteps_and_ragged_sizes), divided by the slope to make it a height -;
value and slope within 1e-12 of the size of their terms of Estimate.__call__ and gradient at the returned height, the gate
between two device summation orders (tests/test_gpu_peak.py); bit for bit wherever the launch geometry changes; the maps
exactly."""
import datetime as dt
import functools
import warnings

import numpy as np
import pytest

import level_ref as lv
import test_gpu_hessian as th
from conftest import load_golden
from test_gpu_hessian import SPH_CFG, T_MID, _bare, _estimate, _t_rec
from test_level_host import level_searches
from test_peak_host import HI, LO, TOL, layer

pytestmark = pytest.mark.gpu

FIELDS = ('height', 'value', 'slope', 'status', 'iterations')
G_VALUE = 1e-10         # test_gpu_basis_eval.py::test_eval_many_timesteps_and_ragged_sizes: rel(out[t], A @ C[t]) <= 1e-10


def _raw(es, C, lat, lon, level, lo, hi, max_iter=48, tol=TOL, hull=False):
    """vi_eval_level_f64 itself on the rows C (T, N) and the columns (lat, lon): (out (3, T, Q), status (T, Q), iterations
    (T, Q)) as the library leaves them - Estimate.level_height blanks the height and the value where the status is not 0."""
    from volumetricinterp_amd import _lib
    C = np.atleast_2d(np.asarray(C, dtype=np.float64))
    lat, lon = np.ravel(lat).astype(np.float64), np.ravel(lon).astype(np.float64)
    T, Q = C.shape[0], lat.size
    lev, a, b = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (T, Q))) for v in (level, lo, hi))
    eq, F, htol = es._hull_args(hull)
    with es.model.ctx.scope() as dev:
        d = [dev.up(v) for v in (np.tile(lat, 2 * T), np.tile(lon, 2 * T), np.stack((a, b)), lev, C)]
        dO, dS, dI = dev.empty((3, T, Q)), dev.empty((T, Q), np.int32), dev.empty((T, Q), np.int32)
        _lib.check(_lib.lib.vi_eval_level_f64(es.model.handle(), T, Q, *(v.ptr for v in d), None if eq is None else dev.up(eq).ptr,
                                              F, htol, max_iter, tol, dO.ptr, dS.ptr, dI.ptr), 'vi_eval_level_f64')
        return dO.download(), dS.download(), dI.download()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b, what=''):
    """two results (tuples of arrays): every field the same bits"""
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.shape(x) == np.shape(y) and np.array_equal(_bits(x), _bits(y)), (what, k)


@functools.lru_cache(maxsize=None)
def _layer_es(case):
    """The Chapman layer of tests/test_peak_host.py (fitted on the oracle's basis) as an Estimate of one record, no hull: the
    coefficients the mirror's searches of tests/test_level_host.py ran on."""
    return _bare(case, layer(case)[1])


def _records(case, Cs, covariance=None):
    """(estimate, times): an Estimate of the order of `case` with the rows of Cs as its records, a minute each, no hull."""
    from volumetricinterp_amd.estimate import Estimate
    maxk, maxl, cap = th.BASIS_CASES[case]
    Cs = np.atleast_2d(Cs)
    T, N = Cs.shape
    cov = np.zeros((T, N, N)) if covariance is None else covariance
    es = Estimate.from_arrays(Cs, cov, [[60. * t, 60. * t + 60.] for t in range(T)], np.zeros((4, 3)), SPH_CFG % (maxk, maxl, cap))
    return es, [dt.datetime(1970, 1, 1) + dt.timedelta(seconds=60. * t + 30.) for t in range(T)]


# ==== 1. against the mirror ==================================================================================================
@pytest.mark.parametrize('case', ['k8l2', 'default'])
def test_heights_against_the_mirror(case):
    """The layer at MAXK 8 x MAXL 2 and at the default order, the 16 searches of tests/test_level_host.py - four columns, 0.5
    and 0.8 of the peak, below and above it - and the same levels over the whole bracket 150 to 450 km: statuses and iteration
    counts are the mirror's, and every height is within tol + 1e-10 vterms / |d1| of the mirror's, vterms = |B| @ |C| the size
    of the value's summands and d1 the slope, both the mirror's at its height.  The second term computes to 4e-4 to 9e-4 m
    at k8l2 and to 8.6 to 39 m at the default order, whose unregularised fit cancels heavily.
    Measured on the MI355X: k8l2 1.2e-10 to 1.5e-9 m from the mirror (gate 1.38e-3 to 1.85e-3 m), all 16 status 0 in 3 to 5
    iterations; default 1.4e-6 to 1.4e-4 m (gate 8.6 to 39 m) at the 8 crossings that exist, 4 to 7 iterations, the other 8
    status 1; statuses and iteration counts the mirror's throughout."""
    es = _layer_es(case)
    lat, lon, level, lo, hi, ref = level_searches(case)
    r = es.level_height(T_MID, lat, lon, level, lo, hi, check_hull=False)
    out, status, it = _raw(es, es.Coeffs, lat, lon, level, lo, hi)
    assert r.height.shape == (16,) and r.status.dtype == np.int32 and r._fields == FIELDS
    found = ref['status'] == 0
    gate = TOL + G_VALUE * ref['vterms'] / np.abs(ref['d1'])
    dist = np.abs(out[0, 0] - ref['h'])
    for c in range(16):
        print('%s (%.1f, %.1f) level %.4e in (%.1f, %.1f) km: status %d / mirror %d, %2d / %2d iterations, height %.6f m, %.2e m '
              'from the mirror, gate %.2e m' % (case, lat[c], lon[c], level[c], lo[c] / 1e3, hi[c] / 1e3, status[0, c],
                                                ref['status'][c], it[0, c], ref['it'][c], out[0, 0, c], dist[c], gate[c]))
    assert np.array_equal(status[0], ref['status']) and np.array_equal(r.status, ref['status'])
    assert np.array_equal(it[0], ref['it']) and np.array_equal(r.iterations, ref['it'])
    assert found.sum() >= 8 and (dist[found] <= gate[found]).all(), (dist, gate)
    assert np.array_equal(_bits(r.height[found]), _bits(out[0, 0][found])) and np.isnan(r.height[~found]).all()
    assert np.array_equal(_bits(r.value[found]), _bits(out[1, 0][found])) and np.isnan(r.value[~found]).all()
    assert np.array_equal(_bits(r.slope), _bits(out[2, 0])) and np.isnan(out[:, 0][:, ~found]).all()
    if case == 'k8l2':
        assert found.all() and ((r.slope > 0.) == (np.arange(16) % 2 == 0)).all()       # bottomside up, topside down
    whole = es.level_height(T_MID, lat, lon, level, LO, HI, check_hull=False)
    mirror = lv.level_search(layer(case)[0], es.Coeffs[0], lat, lon, level, LO, HI, TOL, 48)
    assert np.array_equal(whole.status, mirror['status']) and np.array_equal(whole.iterations, mirror['it'])
    if case == 'k8l2':
        assert (whole.status == 1).all() and (whole.iterations == 0).all()
        assert all(np.isnan(v).all() for v in whole[:3])


# ==== 2. consistency with the existing entries ===============================================================================
@functools.lru_cache(maxsize=None)
def _consistency_case(which):
    """(estimate, lat, lon, level, lo, hi): a layer with its sixteen searches, or random coefficients - scaled by the largest
    value of their basis function on the columns - on 4 x 4 columns in 150 to 600 km, the level of a column the mean of the
    device's values at the two ends, so that every bracket holds a change of sign: the series seeds of k3l4cap15, the (12, 8)
    order with k5l8cap15, the (2, 12) order with k12l2."""
    if which.startswith('layer_'):
        return (_layer_es(which[6:]),) + level_searches(which[6:])[:5]
    lat, lon = (a.ravel() for a in np.meshgrid(np.linspace(76.5, 79.5, 4), np.linspace(256., 268., 4), indexing='ij'))
    A = _bare(which).model.basis(np.repeat(lat, 4), np.repeat(lon, 4), np.tile(np.linspace(150e3, 600e3, 4), 16))
    C = np.random.default_rng(7).standard_normal(A.shape[1]) / np.max(np.abs(A), axis=0)
    es = _bare(which, C)
    ends = [es(T_MID, lat, lon, np.full(16, h), check_hull=False) for h in (150e3, 600e3)]
    return es, lat, lon, 0.5 * (ends[0] + ends[1]), np.full(16, 150e3), np.full(16, 600e3)


@pytest.mark.parametrize('which', ['layer_k8l2', 'layer_default', 'k3l4cap15', 'k5l8cap15', 'k12l2'])
def test_values_are_those_of_the_existing_entries(which):
    """At the heights the search returns - every column with status 0 or 2 -: value against Estimate.__call__, slope against
    gradient(frame='enu')[..., 2], each within 1e-12 of the size of its terms at that point (|basis| @ |C|,
    |u . grad basis| @ |C|): two device summation orders of one quantity.  Measured on the MI355X, the largest over the ten
    runs: value 1.2e-14 (k12l2), slope 7.9e-15 (k5l8cap15) of their terms."""
    es, lat, lon, level, lo, hi = _consistency_case(which)
    C = es.Coeffs[0]
    for max_iter in (48, 1):
        out, status, it = _raw(es, C, lat, lon, level, lo, hi, max_iter=max_iter)
        h, value, slope = out[:, 0]
        ran = (status[0] == 0) | (status[0] == 2)
        print('%s max_iter %d: statuses %s' % (which, max_iter, np.bincount(status[0], minlength=4)))
        assert ran.sum() >= 8 and np.isfinite(out[:, 0][:, ran]).all()
        if max_iter == 48 and not which.startswith('layer_'):
            assert (status[0] == 0).all()
        pts = lat[ran], lon[ran], h[ran]
        m = es.model
        t_value = np.abs(m.basis(*pts)) @ np.abs(C)
        uG = np.einsum('pc,pcn->pn', m.gradient_frame(*pts)[:, 2, :], m.grad_basis(*pts))
        t_slope = np.abs(uG) @ np.abs(C)
        e_value = np.abs(value[ran] - es(T_MID, *pts, check_hull=False)) / t_value
        e_slope = np.abs(slope[ran] - es.gradient(T_MID, *pts, check_hull=False, frame='enu')[:, 2]) / t_slope
        print('%s max_iter %d: value %.2e, slope %.2e of their terms' % (which, max_iter, e_value.max(), e_slope.max()))
        assert e_value.max() <= 1e-12 and e_slope.max() <= 1e-12
        assert ((h[ran] >= lo[ran]) & (h[ran] <= hi[ran])).all()


# ==== 3. launch geometry =====================================================================================================
GEOMETRY_Q = 513


@functools.lru_cache(maxsize=None)
def _geometry(max_iter):
    """(estimate, C (3, N), (lat, lon) of 513 columns, (level, lo, hi) (3, 513), the raw result of the one call with all of
    them): the k8l2 layer, its coefficients times 1.1 and a row of zeros.  Rows 0 and 1: levels from 0.2 to 1.3 of the layer's
    peak in (150, 320) km - a level above the peak has no crossing and stops after the two walks of the ends, status 1, no
    iteration, next to lanes that iterate -, every 17th level NaN (status 3, no walk).  Row 2: the level 0 of an all-zero
    record is hit exactly at lo, no iteration."""
    es = _layer_es('k8l2')
    rng = np.random.default_rng(513)
    Q = GEOMETRY_Q
    lat, lon = rng.uniform(77., 79., Q), rng.uniform(258., 266., Q)
    C = np.stack((es.Coeffs[0], 1.1 * es.Coeffs[0], np.zeros_like(es.Coeffs[0])))
    level = rng.uniform(0.2, 1.3, (3, Q)) * 2.8e11
    level[:2, ::17] = np.nan
    level[2] = 0.
    lo, hi = np.full((3, Q), 150e3) + rng.uniform(0., 30e3, (3, Q)), np.full((3, Q), 320e3)
    full = _raw(es, C, lat, lon, level, lo, hi, max_iter=max_iter)
    return es, C, (lat, lon), (level, lo, hi), full


def _take(full, rows, cols):
    out, status, it = full
    return out[:, rows][:, :, cols], status[rows][:, cols], it[rows][:, cols]


@pytest.mark.parametrize('max_iter', [48, 2])
def test_every_column_has_the_bits_of_its_search_alone(max_iter):
    """The call with 3 x 513 points against calls with Q = 1, T = 1 for the 64 lanes of the second wave of every row: the same
    bits.  In those waves lanes that stop after the two walks of the ends (status 1), lanes that never walk (status 3), and -
    with max_iter = 2 - lanes that use up max_iter (status 2) sit next to each other: a stopped lane is frozen while the wave
    goes on."""
    es, C, (lat, lon), (level, lo, hi), full = _geometry(max_iter)
    out, status, it = full
    print('max_iter %d: statuses %s, iterations up to %d' % (max_iter, np.bincount(status.ravel(), minlength=4), it.max()))
    wave = slice(64, 128)
    for t in range(2):
        st = status[t, wave]
        assert (st == 1).sum() >= 5 and (st == 3).sum() >= 3 and (it[t, wave] == 0).sum() >= 8
        if max_iter == 2:
            assert (st == 2).sum() >= 20 and (it[t, wave][st == 2] == 2).all()
        else:
            assert (st == 0).sum() >= 20 and it[t, wave].max() >= 3
    assert (status[2] == 0).all() and (it[2] == 0).all() and np.array_equal(out[0, 2], lo[2]) and (out[1:, 2] == 0.).all()
    for t in range(3):
        for q in range(64, 128):
            one = _raw(es, C[t], lat[q], lon[q], level[t, q], lo[t, q], hi[t, q], max_iter=max_iter)
            _same_bits(one, _take(full, slice(t, t + 1), slice(q, q + 1)), (t, q))


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('Q', [1, 63, 64, 65, 255, 256, 257, 513])
def test_launch_geometry(Q, T):
    """A block is 256 lanes, a wave 64: the fields of a point are the same bits whatever Q and T are and wherever the point
    sits - the first Q, the last Q and a random draw of Q of the 513 columns in a random order, the first T and the last T of
    the three rows, against the call with all of them; max_iter = 48 and 2."""
    rng = np.random.default_rng(1000 * T + Q)
    for max_iter in (48, 2):
        es, C, (lat, lon), (level, lo, hi), full = _geometry(max_iter)
        for rows in (slice(0, T), slice(3 - T, 3)):
            for cols in (np.arange(Q), np.arange(GEOMETRY_Q - Q, GEOMETRY_Q), rng.permutation(GEOMETRY_Q)[:Q]):
                r = _raw(es, C[rows], lat[cols], lon[cols], level[rows][:, cols], lo[rows][:, cols], hi[rows][:, cols],
                         max_iter=max_iter)
                assert r[0].shape == (3, T, Q)
                _same_bits(r, _take(full, rows, cols), (Q, T, max_iter))


def test_public_method_shapes_and_records():
    """level_height with a list of three datetimes gives (3,) + S, with one datetime S; record t of the batch has the bits of
    the same record alone, with its own levels and brackets; S may have any rank."""
    es0 = _layer_es('k8l2')
    C = np.stack((es0.Coeffs[0], 1.1 * es0.Coeffs[0], 0.9 * es0.Coeffs[0]))
    es, times = _records('k8l2', C)
    rng = np.random.default_rng(70)
    lat, lon = rng.uniform(77., 79., (7, 10)), rng.uniform(258, 266, (7, 10))
    level = rng.uniform(0.3, 0.9, (3, 7, 10)) * 2.8e11
    batch = es.level_height(times, lat, lon, level, 150e3, 320e3, check_hull=False)
    assert batch.height.shape == (3, 7, 10) and (batch.status == 0).sum() >= 150
    raw = _raw(es, C, lat, lon, level.reshape(3, 70), 150e3, 320e3)
    assert np.array_equal(batch.status.reshape(3, 70), raw[1]) and np.array_equal(_bits(batch.slope.reshape(3, 70)), _bits(raw[0][2]))
    for i in range(3):
        one = es.level_height(times[i], lat, lon, level[i], 150e3, 320e3, check_hull=False)
        assert one.height.shape == (7, 10)
        _same_bits(one, tuple(f[i] for f in batch), i)


# ==== 4. statuses ============================================================================================================
def test_statuses_of_the_search():
    """Status 1: no change of sign.  Status 2 with max_iter = 0 and 1: the raw output holds the last iterate with its value and
    slope (max_iter = 0: the secant point of the ends), the public method blanks height and value.  Status 3: a NaN in any
    input, lo >= hi.  Status 0 by an exact hit: an all-zero record and level 0 give h = lo, no iteration, slope 0."""
    es = _layer_es('k8l2')
    lat, lon, level, lo, hi, ref = level_searches('k8l2')
    C = es.Coeffs[0]
    col = lat[:1], lon[:1]
    r = es.level_height(T_MID, *col, 10. * level[0], lo[0], hi[0], check_hull=False)
    assert r.status[0] == 1 and r.iterations[0] == 0 and all(np.isnan(v[0]) for v in r[:3])
    for max_iter in (0, 1):
        out, status, it = _raw(es, C, *col, level[0], lo[0], hi[0], max_iter=max_iter)
        mirror = lv.level_search(layer('k8l2')[0], C, *col, level[0], lo[0], hi[0], TOL, max_iter)
        assert status[0, 0] == 2 and it[0, 0] == max_iter and mirror['status'][0] == 2 and mirror['it'][0] == max_iter
        h = out[0, 0, 0]
        assert lo[0] < h < hi[0] and abs(h - mirror['h'][0]) <= 1e-6 * (hi[0] - lo[0])
        pt = col + (np.array([h]),)
        for got, want, basis in ((out[1, 0, 0], es(T_MID, *pt, check_hull=False)[0], es.model.basis(*pt)[0]),
                                 (out[2, 0, 0], es.gradient(T_MID, *pt, check_hull=False, frame='enu')[0, 2],
                                  np.einsum('c,cn->n', es.model.gradient_frame(*pt)[0, 2], es.model.grad_basis(*pt)[0]))):
            assert abs(got - want) <= 1e-12 * (np.abs(basis) @ np.abs(C))
        r = es.level_height(T_MID, *col, level[0], lo[0], hi[0], max_iter=max_iter, check_hull=False)
        assert r.status[0] == 2 and r.iterations[0] == max_iter and np.isnan(r.height[0]) and np.isnan(r.value[0])
        assert r.slope[0] == out[2, 0, 0]
    nan = np.nan
    bad = es.level_height(T_MID, [lat[0], nan, lat[0], lat[0], lat[0], lat[0], lat[0], lat[0]],
                          [lon[0], lon[0], nan, lon[0], lon[0], lon[0], lon[0], lon[0]],
                          [level[0], level[0], level[0], nan, level[0], level[0], level[0], level[0]],
                          [lo[0], lo[0], lo[0], lo[0], nan, lo[0], hi[0], hi[0]],
                          [hi[0], hi[0], hi[0], hi[0], hi[0], nan, hi[0], lo[0]], check_hull=False)
    assert list(bad.status) == [0] + [3] * 7 and (bad.iterations[1:] == 0).all()
    assert all(np.isnan(v[1:]).all() for v in bad[:3]) and np.isfinite(bad.height[0])
    zero = _bare('k8l2')
    out, status, it = _raw(zero, zero.Coeffs, lat, lon, 0., lo, hi)
    assert (status == 0).all() and (it == 0).all() and np.array_equal(out[0, 0], lo) and (out[1:] == 0.).all()
    z = zero.level_height(T_MID, lat, lon, 0., lo, hi, check_hull=False)
    assert (z.status == 0).all() and np.array_equal(z.height, lo) and (z.slope == 0.).all() and (z.value == 0.).all()


def test_a_nan_record_reaches_only_itself():
    """Three records, one NaN in the second: that record is status 3 and NaN in every column, the other two keep the bits they
    have without it."""
    es0 = _layer_es('k8l2')
    C = np.stack((es0.Coeffs[0], 1.1 * es0.Coeffs[0], 0.9 * es0.Coeffs[0]))
    Cn = C.copy()
    Cn[1, 5] = np.nan
    rng = np.random.default_rng(66)
    lat, lon = rng.uniform(77., 79., 66), rng.uniform(258, 266, 66)
    good = _raw(es0, C, lat, lon, 1.4e11, 150e3, 320e3)
    r = _raw(es0, Cn, lat, lon, 1.4e11, 150e3, 320e3)
    assert (good[1] == 0).all()
    assert (r[1][1] == 3).all() and np.isnan(r[0][:, 1]).all() and (r[2][1] == 0).all()
    for i in (0, 2):
        _same_bits(_take(r, slice(i, i + 1), slice(None)), _take(good, slice(i, i + 1), slice(None)), i)
    bad, times = _records('k8l2', Cn)
    pub = bad.level_height(times, lat, lon, 1.4e11, 150e3, 320e3, check_hull=False)
    assert (pub.status[1] == 3).all() and (pub.status[[0, 2]] == 0).all()


def test_both_ends_go_through_the_hull():
    """192 columns of the default fit with its hull, brackets drawn so that either end may be inside or outside: status 3 and
    NaN exactly where est.check_hull refuses the lower or the upper end - one end outside is enough -, and the brackets with
    both ends inside keep the bits they have without the hull test."""
    f, es, _ = _estimate('default')
    rng = np.random.default_rng(192)
    lat, lon = rng.uniform(77., 79., 192), rng.uniform(258, 266, 192)
    lo = rng.uniform(150e3, 350e3, 192)
    hi = lo + rng.uniform(20e3, 300e3, 192)
    hi[::3] = rng.uniform(1500e3, 3000e3, 64)
    lo[:64] = rng.uniform(-500e3, -100e3, 64)           # the first wave: no lower end inside, it leaves before any walk
    t = _t_rec(f)
    C = es.get_C(t)[0]
    ends = [es(t, lat, lon, h, check_hull=False) for h in (lo, hi)]
    level = 0.5 * (ends[0] + ends[1])
    in_lo, in_hi = es.check_hull(lat, lon, lo), es.check_hull(lat, lon, hi)
    inside = in_lo & in_hi
    assert inside.sum() >= 10 and (in_lo & ~in_hi).sum() >= 5 and (~in_lo & in_hi).sum() >= 1 and not in_lo[:64].any()
    r = es.level_height(t, lat, lon, level, lo, hi)
    free = es.level_height(t, lat, lon, level, lo, hi, check_hull=False)
    assert np.array_equal(r.status == 3, ~inside) and (free.status != 3).all()
    assert all(np.isnan(v[~inside]).all() for v in r[:3]) and (r.iterations[~inside] == 0).all()
    _same_bits(tuple(v[inside] for v in r), tuple(v[inside] for v in free))
    assert (r.status[inside] == 0).sum() >= 5
    ok = r.status == 0
    assert es.check_hull(lat[ok], lon[ok], r.height[ok]).all()          # between two points inside: inside


# ==== 5. errors ==============================================================================================================
def test_error_bars():
    """error=True on the layer with the covariance of the k8l2 fixture's first record: height_error is error() / |slope| at
    the returned heights, bit for bit; the five fields before it are those of error=False; NaN where the status is not 0.
    Without a covariance it raises, as the error entries do."""
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_k8l2')
    layer_es = _layer_es('k8l2')
    es = Estimate.from_arrays(layer_es.Coeffs, f['Covariance'][:1], [[0., 60.]], np.zeros((4, 3)), layer_es.config_file_text)
    lat, lon, level, lo, hi, _ = level_searches('k8l2')
    lat, lon, level, lo, hi = (np.append(a, v) for a, v in ((lat, 78.), (lon, 262.), (level, np.nan), (lo, LO), (hi, HI)))
    r = es.level_height(T_MID, lat, lon, level, lo, hi, check_hull=False, error=True)
    assert r._fields == FIELDS + ('height_error',) and r.height_error.shape == (17,)
    _same_bits(r[:5], es.level_height(T_MID, lat, lon, level, lo, hi, check_hull=False))
    ok = r.status == 0
    assert ok[:16].all() and r.status[16] == 3 and np.isnan(r.height_error[16])
    pts = lat[ok], lon[ok], r.height[ok]
    err = es.error(T_MID, *pts, check_hull=False)
    assert (err > 0.).all() and np.array_equal(r.height_error[ok], err / np.abs(r.slope[ok]))
    print('height errors %s m' % r.height_error[:16:4])
    bare = Estimate.from_arrays(layer_es.Coeffs, None, [[0., 60.]], np.zeros((4, 3)), layer_es.config_file_text)
    with pytest.raises(ValueError, match='no covariance'):
        bare.level_height(T_MID, lat, lon, level, lo, hi, check_hull=False, error=True)


# ==== 6. refusals and timing =================================================================================================
def test_refusals():
    """An order beyond the compiled ones (MAXL 13) and the radial-basis model: VI_ERR_UNSUPPORTED (-6) from the library with
    the output buffers untouched - nothing was launched -, VinterpError from Python.  A bad tol or max_iter, a null pointer
    and facets counted but not given: VI_ERR_INVALID (-1), ValueError from Python.  T = 0 and Q = 0 are no-ops."""
    from volumetricinterp_amd import _lib
    from volumetricinterp_amd.estimate import Estimate
    lat, lon, _ = th._basis_points('default')
    Q = lat.size
    th.BASIS_CASES['k2l13'] = (2, 13, 10.)
    try:
        big = _bare('k2l13')
    finally:
        del th.BASIS_CASES['k2l13']
    fr = load_golden('fit_rbf')
    rbf = Estimate.from_arrays(fr['Coeffs'], fr['Covariance'], fr['utime'], fr['hull_vert'], str(fr['cfg']))
    ok = _bare('default', np.ones(144))

    def call(es, dev, T=1, nq=Q, max_iter=48, tol=TOL, F=0, null=None):
        N = es.model.nbasis
        d = [dev.up(v) for v in (np.tile(lat, 2), np.tile(lon, 2), np.concatenate((np.full(Q, LO), np.full(Q, HI))),
                                 np.full(Q, 1.), np.ones(N))]
        dO, dS, dI = dev.up(np.full(3 * Q, 7.)), dev.up(np.full(Q, 7, dtype=np.int32)), dev.up(np.full(Q, 7, dtype=np.int32))
        p = [v.ptr for v in d] + [None, F, 0., max_iter, tol, dO.ptr, dS.ptr, dI.ptr]
        if null is not None:
            p[null] = None
        rc = _lib.lib.vi_eval_level_f64(es.model.handle(), T, nq, *p)
        es.model.ctx.sync()
        assert np.array_equal(dO.download(), np.full(3 * Q, 7.))
        assert np.array_equal(dS.download(), np.full(Q, 7)) and np.array_equal(dI.download(), np.full(Q, 7))
        return rc

    for es, what in ((big, 'beyond the compiled limits'), (rbf, 'only the sphharmlag model')):
        with es.model.ctx.scope() as dev:
            assert call(es, dev) == -6 and what in _lib.lib.vi_last_error().decode()
        with pytest.raises(_lib.VinterpError, match=what):
            es.level_height(_t_rec(fr) if es is rbf else T_MID, lat, lon, 1., LO, HI, check_hull=False)
    with ok.model.ctx.scope() as dev:
        for bad in (dict(tol=0.), dict(tol=-1.), dict(tol=np.nan), dict(tol=np.inf), dict(max_iter=-1), dict(max_iter=10001),
                    dict(F=3), dict(T=-1), dict(nq=-1), dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(null=4),
                    dict(null=10), dict(null=11)):
            assert call(ok, dev, **bad) == -1, bad
        assert call(ok, dev, T=0) == 0 and call(ok, dev, nq=0) == 0
    for bad in (dict(tol=0.), dict(tol=np.nan), dict(max_iter=-1), dict(max_iter=1.5), dict(max_iter=10001), dict(max_iter=True)):
        with pytest.raises(ValueError, match='tol must be|max_iter must be'):
            ok.level_height(T_MID, lat, lon, 1., LO, HI, check_hull=False, **bad)
    with pytest.raises(ValueError, match='broadcast'):
        ok.level_height(T_MID, lat, lon, np.zeros(Q + 1), LO, HI, check_hull=False)
    with pytest.raises(ValueError, match='one shape'):
        ok.level_height(T_MID, lat, lon[:-1], 1., LO, HI, check_hull=False)
    empty = ok.level_height([], lat, lon, 1., LO, HI, check_hull=False)
    assert all(v.shape == (0, Q) for v in empty)
    empty = ok.level_height(T_MID, lat[:0], lon[:0], 1., LO, HI, check_hull=False)
    assert all(v.shape == (0,) for v in empty) and empty.status.dtype == np.int32
    # the null d_iter is allowed
    with ok.model.ctx.scope() as dev:
        d = [dev.up(v) for v in (np.tile(lat, 2), np.tile(lon, 2), np.concatenate((np.full(Q, LO), np.full(Q, HI))),
                                 np.full(Q, 1.), np.ones(144))]
        dO, dS = dev.empty((3, Q)), dev.empty(Q, np.int32)
        assert _lib.lib.vi_eval_level_f64(ok.model.handle(), 1, Q, *(v.ptr for v in d), None, 0, 0., 48, TOL, dO.ptr, dS.ptr,
                                          None) == 0
        assert np.isin(dS.download(), (0, 1, 2, 3)).all()


def test_calls_are_timed():
    """Both entries record their kernels for vi_eval_kernel_ms, as their siblings do."""
    es = _layer_es('k8l2')
    lat, lon, level, lo, hi, _ = level_searches('k8l2')
    ctx = es.model.ctx
    ctx.eval_timing(True)
    try:
        es.level_height(T_MID, lat, lon, level, lo, hi, check_hull=False)
        assert 0. < ctx.eval_kernel_ms() < 1000.
    finally:
        ctx.eval_timing(False)


# ==== 7. crossing maps =======================================================================================================
COMBOS = [(w, d) for w in ('first', 'last') for d in ('any', 'up', 'down')]


def _grid(axis, L, n1=3, n2=4, top=450e3):
    """A 3-D grid of points with L altitudes from 150 km to `top` along `axis` and n1 x n2 columns over the other two."""
    shape = [n1, n2]
    shape.insert(axis, L)
    alt = np.linspace(150e3, top, L) if L > 1 else np.array([300e3])
    ix = np.indices(shape)
    others = [k for k in range(3) if k != axis]
    lat = 77.5 + ix[others[0]] / max(n1 - 1, 1)
    lon = 259. + 6. * ix[others[1]] / max(n2 - 1, 1)
    return lat, lon, alt[ix[axis]], alt


@pytest.mark.parametrize('L', [1, 2, 3, 5, 64, 65])
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_crossing_maps(axis, L):
    """The maps of two records of the k8l2 layer on a grid with the reduced axis first (inner > 1), in the middle and last
    (inner = 1, the lanes of a column side by side), L samples along it: every which and direction, a scalar level at 0.5 of the
    peak and a level per column and record, exactly the plain loop over the downloaded volume."""
    es0 = _layer_es('k8l2')
    es, times = _records('k8l2', np.stack((es0.Coeffs[0], 0.8 * es0.Coeffs[0])))
    lat, lon, alt, _ = _grid(axis, L)
    rng = np.random.default_rng(10 * L + axis)
    with es.resident_grid(lat, lon, alt, check_hull=False) as g:
        vol = g(times)
        rest = vol.shape[:1 + axis] + vol.shape[2 + axis:]
        per_column = rng.uniform(0.1, 1.1, rest) * 2.8e11
        per_column[0, 0, 0] = np.nan
        found = 0
        for level in (1.4e11, per_column):
            for which, direction in COMBOS:
                idx = g.crossing(times, level, axis=axis, which=which, direction=direction)
                want = lv.crossing_index(vol, level, axis, which, direction)
                assert idx.shape == rest and idx.dtype == np.int32
                assert np.array_equal(idx, want), (which, direction, idx, want)
                found += (idx >= 0).sum()
        assert (found > 0) == (L > 1)
        assert g.crossing(times, per_column, axis=axis)[0, 0, 0] == -1


def test_crossing_maps_hull_nan_record_and_slabs(monkeypatch):
    """The k8l2 fit with its hull on a grid that reaches above the beams (columns partly and wholly outside: NaN samples), four
    records with a NaN in the coefficients of the third (its map is -1 throughout), the level of a column midway between its
    smallest and its largest sample, run in one slab and - the slab size
    reported so - in slabs of three timesteps and of one: the same maps, those of the plain loop."""
    from volumetricinterp_amd.estimate import Estimate
    f, es, _ = _estimate('k8l2')
    Cs = np.array(es.Coeffs[:4])
    assert Cs.shape[0] == 4
    Cs[2, 7] = np.nan
    es5 = Estimate.from_arrays(Cs, f['Covariance'][:4], f['utime'][:4], f['hull_vert'], str(f['cfg']))
    times = [_t_rec(f, i) for i in range(4)]
    for axis in (0, 2):
        lat, lon, alt, _ = _grid(axis, 24, n1=4, n2=5, top=900e3)
        lat = lat + 2. * (lat - 77.5)                                      # 77.5 to 80.5: the outer columns leave the hull
        with es5.resident_grid(lat, lon, alt) as g:
            vol = g(times)
            assert np.isnan(vol[2]).all() and 0 < np.isnan(vol[0]).sum() < vol[0].size
            with warnings.catch_warnings():                                # (all-NaN columns: their level is NaN)
                warnings.simplefilter('ignore', RuntimeWarning)
                level = 0.5 * (np.nanmin(vol, axis=1 + axis) + np.nanmax(vol, axis=1 + axis))
            maps = {}
            for which, direction in COMBOS:
                idx = g.crossing(times, level, axis=axis, which=which, direction=direction)
                assert np.array_equal(idx, lv.crossing_index(vol, level, axis, which, direction)), (axis, which, direction)
                assert (idx[2] == -1).all()
                maps[which, direction] = idx
            assert (maps['first', 'any'][[0, 1, 3]] >= 0).sum() >= 5 and (maps['first', 'any'][[0, 1, 3]] < 0).any()
            calls = []
            monkeypatch.setattr(g, '_slab', lambda T, nbytes: calls.append(T) or (3 if axis else 1))
            for which, direction in COMBOS:
                assert np.array_equal(g.crossing(times, level, axis=axis, which=which, direction=direction), maps[which, direction])
            assert len(calls) == len(COMBOS)
            monkeypatch.undo()


def test_crossing_arguments():
    """which, direction, axis and the shape of the level are checked on the host; a closed grid refuses."""
    es = _layer_es('k8l2')
    lat, lon, alt, _ = _grid(2, 5)
    g = es.resident_grid(lat, lon, alt, check_hull=False)
    with g:
        for bad, what in ((dict(which='middle'), 'which must be'), (dict(direction='sideways'), 'direction must be'),
                          (dict(axis=3), 'axis must be')):
            with pytest.raises(ValueError, match=what):
                g.crossing([T_MID], 1e11, **bad)
        with pytest.raises(ValueError, match='level must be'):
            g.crossing([T_MID], np.zeros((1, 3, 5)))
        assert g.crossing([], 1e11).shape == (0, 3, 4)
        out = np.empty((1, 12), dtype=np.int32)
        assert g.evaluate_crossings(es.Coeffs, 1.4e11, out=out) is out
        assert np.array_equal(out.reshape(1, 3, 4), g.crossing([T_MID], 1.4e11))
    with pytest.raises(ValueError, match='closed'):
        g.crossing([T_MID], 1e11)


def test_from_a_grid_crossing_to_the_height():
    """The use the entries are made for, on a 6 x 5 x 16 grid of the k8l2 layer: crossing -> level_brackets -> level_height, for
    the bottomside ('up', first) and the topside ('down', last) crossing of 0.5 and 0.8 of 2.8e11.  No grid sample lies within
    1e-9 of the size of its terms of the level - closer, the rounding of the product and of the walk could disagree about a
    sign -, so wherever the map has a pair the search has a bracket with a change of sign: status 0, the height inside the
    pair, the slope of the asked sign, and the value within |slope| tol of the level."""
    from volumetricinterp_amd.estimate import level_brackets
    es = _layer_es('k8l2')
    alt = np.linspace(150e3, 450e3, 16)
    lat2, lon2 = np.meshgrid(np.linspace(77.2, 79., 6), np.linspace(255., 266., 5), indexing='ij')
    grid = [np.broadcast_to(a[..., None], lat2.shape + alt.shape) for a in (lat2, lon2)] + \
           [np.broadcast_to(alt, lat2.shape + alt.shape)]
    terms = (np.abs(es.model.basis(*(a.ravel() for a in grid))) @ np.abs(es.Coeffs[0])).reshape(grid[0].shape)
    with es.resident_grid(*grid, check_hull=False) as g:
        vol = g([T_MID])[0]
        for frac in (0.5, 0.8):
            level = frac * 2.8e11
            assert (np.abs(vol - level) > 1e-9 * terms).all()
            for which, direction, sign in (('first', 'up', 1.), ('last', 'down', -1.)):
                i = g.crossing([T_MID], level, which=which, direction=direction)
                assert i.shape == (1, 6, 5) and (i >= 0).sum() >= 20
                lo, hi = level_brackets(alt, i)
                r = es.level_height([T_MID], lat2, lon2, level, lo, hi, check_hull=False)
                has = i >= 0
                assert r.height.shape == (1, 6, 5) and (r.status[has] == 0).all() and (r.status[~has] == 3).all()
                assert ((r.height[has] >= lo[has]) & (r.height[has] <= hi[has])).all() and (sign * r.slope[has] > 0.).all()
                assert (np.abs(r.value[has] - level) <= np.abs(r.slope[has]) * TOL).all()
                print('level %.2e %s %s: heights %.1f to %.1f km, %d to %d iterations'
                      % (level, which, direction, r.height[has].min() / 1e3, r.height[has].max() / 1e3,
                         r.iterations[has].min(), r.iterations[has].max()))
