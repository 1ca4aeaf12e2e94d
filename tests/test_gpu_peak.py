"""GPU tests of the sub-grid peak search: Estimate.peak_height (vi_eval_peak_f64, kernel k_peak_sph: a lane per column, one walk
of the chains per iteration for the value, the slope and the curvature along the geodetic normal).

The reference project has no peak search.  The yardstick of the heights is tests/peak_ref.py, the device iteration in NumPy on
the oracle's basis and gradient basis and the Hessian restatement, which tests/test_peak_host.py holds against
scipy.optimize.brentq.  Gates: a height within tol + 1e-10 terms / |curvature| of the mirror's - tol is what the search
promises, 1e-10 of the slope's terms the project's gate of Estimate.gradient against the oracle, divided by the curvature to make
it a height -; value, slope and curvature within 1e-12 of the size of their terms of Estimate.__call__, gradient and hessian at
the returned height, the gate between two device summation orders; bit for bit wherever the launch geometry changes."""
import functools

import numpy as np
import pytest

import peak_ref as pk
import test_gpu_hessian as th
from conftest import load_golden
from test_gpu_hessian import T_MID, _bare, _estimate, _t_rec
from test_peak_host import COLUMNS, HI, LO, TOL, grid_start, layer_oracle

pytestmark = pytest.mark.gpu

FIELDS = ('height', 'value', 'slope', 'curvature', 'status', 'iterations')


def _raw(es, C, lat, lon, start, lo, hi, kind=1, max_iter=48, tol=TOL, hull=False):
    """vi_eval_peak_f64 itself on the rows C (T, N) and the columns (lat, lon): (out (4, T, Q), status (T, Q), iterations
    (T, Q)) as the library leaves them - Estimate.peak_height blanks the height and the value where the status is not 0."""
    from volumetricinterp_amd import _lib
    C = np.atleast_2d(np.asarray(C, dtype=np.float64))
    lat, lon = np.ravel(lat).astype(np.float64), np.ravel(lon).astype(np.float64)
    T, Q = C.shape[0], lat.size
    h0, a, b = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (T, Q))) for v in (start, lo, hi))
    eq, F, htol = es._hull_args(hull)
    with es.model.ctx.scope() as dev:
        d = [dev.up(v) for v in (np.tile(lat, T), np.tile(lon, T), h0, a, b, C)]
        dO, dS, dI = dev.empty((4, T, Q)), dev.empty((T, Q), np.int32), dev.empty((T, Q), np.int32)
        _lib.check(_lib.lib.vi_eval_peak_f64(es.model.handle(), T, Q, *(v.ptr for v in d), None if eq is None else dev.up(eq).ptr,
                                             F, htol, kind, max_iter, tol, dO.ptr, dS.ptr, dI.ptr), 'vi_eval_peak_f64')
        return dO.download(), dS.download(), dI.download()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b, what=''):
    """two results of peak_height (or tuples of arrays): every field the same bits"""
    assert len(a) == len(b)
    for name, x, y in zip(FIELDS + ('height_error', 'value_error'), a, b):
        assert np.shape(x) == np.shape(y) and np.array_equal(_bits(x), _bits(y)), (what, name)


def _cut(r, sl):
    return tuple(f[sl] for f in r)


@functools.lru_cache(maxsize=None)
def _layer_es(case):
    """The Chapman layer fitted on the device's own basis: th._layer() at MAXK 8 x MAXL 2 on the 11 x 50 beams, the same
    recipe at the default order on the 26 x 100 beams."""
    if case == 'k8l2':
        return th._layer()
    from volumetricinterp_amd import synth
    lat, lon, alt = synth.beams(*synth.GEOM_C2, seed=0)
    value, error = synth.chapman_record(alt)
    A = _bare('default').model.basis(lat, lon, alt)
    return _bare('default', np.linalg.lstsq(A / error[:, None], value / error, rcond=1e-10)[0])


@functools.lru_cache(maxsize=None)
def _layer_columns(case):
    """The four columns from 200 km, 440 km and the maximum of a 25 km grid, and the mirror's search of them with the
    estimate's coefficients: (lat, lon, start, mirror's result)."""
    C = _layer_es(case).Coeffs[0]
    o = layer_oracle(case)
    lat = np.repeat([c[0] for c in COLUMNS], 3)
    lon = np.repeat([c[1] for c in COLUMNS], 3)
    start = np.concatenate([[200e3, 440e3, grid_start(o, C, *c)] for c in COLUMNS])
    ref = pk.peak_search(o, C, lat, lon, start, LO, HI, 1, TOL, 48)
    for v in (lat, lon, start) + tuple(ref.values()):
        v.setflags(write=False)
    return lat, lon, start, ref


# ==== 1. against the mirror ==================================================================================================
@pytest.mark.parametrize('case', ['k8l2', 'default'])
def test_heights_against_the_mirror(case):
    """The layer at MAXK 8 x MAXL 2 and at the default order, four columns from three starts each, bracket 150 to 450 km:
    the statuses are the mirror's, and every height is within tol + 1e-10 terms / |d2| of the mirror's, terms = |u . G| @ |C|
    the size of the slope's summands and d2 the curvature, both the mirror's at its height.  The second term computes to
    2.8e-4 to 4.2e-4 m at k8l2 and to metres at the default order, whose unregularised fit cancels heavily.
    Measured on the MI355X: k8l2 5.8e-11 to 2.5e-9 m from the mirror (gate 1.28e-3 to 1.42e-3 m), default 1.1e-5 to 3.7e-5 m
    (gate 0.81 to 15 m; the two columns that end on the bracket's lower end 0 m); statuses and iteration counts the mirror's."""
    es = _layer_es(case)
    lat, lon, start, ref = _layer_columns(case)
    r = es.peak_height(T_MID, lat, lon, start, LO, HI, check_hull=False)
    out, status, it = _raw(es, es.Coeffs, lat, lon, start, LO, HI)
    assert r.height.shape == (12,) and r.status.dtype == np.int32
    gate = TOL + 1e-10 * ref['terms'] / np.abs(ref['d2'])
    dist = np.abs(out[0, 0] - ref['h'])
    for c in range(12):
        print('%s (%.1f, %.1f) from %6.1f km: status %d / mirror %d, %2d / %2d iterations, height %.6f m, %.2e m from the '
              'mirror, gate %.2e m' % (case, lat[c], lon[c], start[c] / 1e3, r.status[c], ref['status'][c], r.iterations[c],
                                       ref['it'][c], out[0, 0, c], dist[c], gate[c]))
    assert np.array_equal(r.status, ref['status']) and np.array_equal(status[0], ref['status'])
    assert (ref['status'] != 3).all() and (dist <= gate).all(), (dist, gate)
    ok = r.status == 0
    assert ok.sum() >= 6 and np.array_equal(_bits(r.height[ok]), _bits(out[0, 0][ok])) and np.isnan(r.height[~ok]).all()
    assert np.array_equal(_bits(r.value[ok]), _bits(out[1, 0][ok])) and np.isnan(r.value[~ok]).all()
    assert np.array_equal(_bits(r.slope), _bits(out[2, 0])) and np.array_equal(_bits(r.curvature), _bits(out[3, 0]))
    assert np.array_equal(r.iterations, it[0])


# ==== 2. consistency with the existing entries ===============================================================================
@functools.lru_cache(maxsize=None)
def _consistency_case(which):
    """(estimate, lat, lon, start, lo, hi): a layer fit on its twelve columns, or random coefficients - scaled by the largest
    value of their basis function on the columns - on 4 x 4 columns from 350 km in 150 to 600 km: the series seeds of
    k3l4cap15, the (12, 8) order with k5l8cap15, the (2, 12) order with k12l2."""
    if which.startswith('layer_'):
        lat, lon, start, _ = _layer_columns(which[6:])
        return _layer_es(which[6:]), lat, lon, start, LO, HI
    lat, lon = (a.ravel() for a in np.meshgrid(np.linspace(76.5, 79.5, 4), np.linspace(256., 268., 4), indexing='ij'))
    A = _bare(which).model.basis(np.repeat(lat, 4), np.repeat(lon, 4), np.tile(np.linspace(150e3, 600e3, 4), 16))
    C = np.random.default_rng(7).standard_normal(A.shape[1]) / np.max(np.abs(A), axis=0)
    return _bare(which, C), lat, lon, 350e3, 150e3, 600e3


@pytest.mark.parametrize('kind', ['max', 'min'])
@pytest.mark.parametrize('which', ['layer_k8l2', 'layer_default', 'k3l4cap15', 'k5l8cap15', 'k12l2'])
def test_values_are_those_of_the_existing_entries(which, kind):
    """At the heights the search returns - every column that ran, whatever its status -: value against Estimate.__call__,
    slope against gradient(frame='enu')[..., 2], curvature against hessian(frame='enu')[..., 2, 2], each within 1e-12 of the
    size of its terms at that point (|basis| @ |C|, |u . grad basis| @ |C|, |up-up Hessian basis| @ |C|): two device summation
    orders of one quantity.  Where the status is 0 the slope is that of a converged search,
    |slope| <= |curvature| tol + 1e-12 terms.  Measured on the MI355X, the largest over the ten cases: value 2.7e-15, slope
    1.3e-14 (k12l2), curvature 8.1e-15 of their terms."""
    es, lat, lon, start, lo, hi = _consistency_case(which)
    C = es.Coeffs[0]
    out, status, it = _raw(es, C, lat, lon, start, lo, hi, kind={'max': 1, 'min': -1}[kind])
    h, value, slope, curv = out[:, 0]
    ran = status[0] != 3
    print('%s %s: statuses %s' % (which, kind, np.bincount(status[0], minlength=4)))
    assert ran.sum() >= lat.size // 2
    if not which.startswith('layer_'):
        assert (status[0] == 0).sum() >= 4
    pts = lat[ran], lon[ran], h[ran]
    m = es.model
    t_value = np.abs(m.basis(*pts)) @ np.abs(C)
    uG = np.einsum('pc,pcn->pn', m.gradient_frame(*pts)[:, 2, :], m.grad_basis(*pts))
    t_slope = np.abs(uG) @ np.abs(C)
    t_curv = np.abs(m.hess_basis(*pts, frame='enu')[:, 2, :]) @ np.abs(C)
    e_value = np.abs(value[ran] - es(T_MID, *pts, check_hull=False)) / t_value
    e_slope = np.abs(slope[ran] - es.gradient(T_MID, *pts, check_hull=False, frame='enu')[:, 2]) / t_slope
    e_curv = np.abs(curv[ran] - es.hessian(T_MID, *pts, check_hull=False, frame='enu')[:, 2, 2]) / t_curv
    print('%s %s: value %.2e, slope %.2e, curvature %.2e of their terms' % (which, kind, e_value.max(), e_slope.max(), e_curv.max()))
    assert e_value.max() <= 1e-12 and e_slope.max() <= 1e-12 and e_curv.max() <= 1e-12
    ok = status[0][ran] == 0
    assert (np.abs(slope[ran][ok]) <= np.abs(curv[ran][ok]) * TOL + 1e-12 * t_slope[ok]).all()
    s = {'max': 1., 'min': -1.}[kind]
    assert (s * curv[ran][ok] < 0.).all() and (h[ran][ok] > lo).all() and (h[ran][ok] < hi).all()


# ==== 3. launch geometry =====================================================================================================
@functools.lru_cache(maxsize=None)
def _geometry(which):
    """(estimate, time, hull, (lat, lon, start) of 300 columns, their result): the default fit with its hull (integer degrees:
    the closed-form seeds) or the fractional degrees of k3l4cap15 (the seed series, whose exit test is wave-uniform)."""
    rng = np.random.default_rng(300)
    cols = rng.uniform(75, 81, 300), rng.uniform(250, 274, 300), rng.uniform(250e3, 400e3, 300)
    if which == 'fit':
        f, es, _ = _estimate('default')
        t, hull = _t_rec(f), True
    else:
        es, t, hull = _bare('k3l4cap15', rng.standard_normal(48)), T_MID, False
    return es, t, hull, cols, es.peak_height(t, *cols, 150e3, 600e3, check_hull=hull)


@pytest.mark.parametrize('Q', [0, 1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize('which', ['fit', 'series'])
def test_launch_geometry(which, Q):
    """A block is 256 lanes, a wave 64: the six results of a column are the same bits whatever Q is and wherever the column
    sits in the array - the first Q and the last Q of 300 columns against the call with all of them."""
    es, t, hull, cols, full = _geometry(which)
    print('%s: statuses %s' % (which, np.bincount(full.status, minlength=5)))
    assert (full.iterations > 1).sum() >= 10                            # columns that searched
    if which == 'fit':
        assert 0 < (full.status == 3).sum() < 300
    for sl in (slice(0, Q), slice(300 - Q, 300)):
        r = es.peak_height(t, *(a[sl] for a in cols), 150e3, 600e3, check_hull=hull)
        assert r.height.shape == (Q,)
        _same_bits(r, _cut(full, sl), (which, Q))


@pytest.mark.parametrize('T', [1, 3])
def test_records_in_a_batch(T):
    """The grid's second dimension is the record: record t inside a batch of T gives the bits of the same record alone, with
    its own starts and brackets.  The k8l2 fit with its hull, 70 columns."""
    f, es, _ = _estimate('k8l2')
    rng = np.random.default_rng(70)
    lat, lon = rng.uniform(77., 79., 70), rng.uniform(258, 266, 70)
    start = rng.uniform(200e3, 400e3, (T, 70))
    lo, hi = start - rng.uniform(0., 100e3, (T, 70)), start + rng.uniform(0., 300e3, (T, 70))
    times = [_t_rec(f, i) for i in range(T)]
    batch = es.peak_height(times, lat, lon, start, lo, hi)
    assert batch.height.shape == (T, 70) and (batch.status != 3).sum() >= 20
    for i in range(T):
        one = es.peak_height(times[i], lat, lon, start[i], lo[i], hi[i])
        assert one.height.shape == (70,)
        _same_bits(one, _cut(batch, i), i)
        _same_bits(es.peak_height(times[i:i + 1], lat, lon, start[i], lo[i], hi[i]), _cut(batch, slice(i, i + 1)), i)


def test_fast_and_slow_columns_in_one_wave():
    """One wave of 64 lanes: the even ones converge on the layer's peak in a few Newton steps from the grid maximum, the odd
    ones have a bracket below the layer's inflection - no interior peak, the curvature has the wrong sign, so the steps
    bisect towards the upper end: 40 km down to 1e-3 m is 26 halvings, status 1.  Finished lanes are frozen while
    the wave goes on: every lane has the bits of its column searched alone (Q = 1)."""
    es = _layer_es('k8l2')
    lat, lon, start, ref = _layer_columns('k8l2')
    fast = (lat[8], lon[8], start[8], LO, HI)
    slow = (78.5, 255., 170e3, 150e3, 210e3)
    cols = [np.array([fast[k] if q % 2 == 0 else slow[k] for q in range(64)]) for k in range(5)]
    r = es.peak_height(T_MID, *cols, check_hull=False)
    assert (r.status[0::2] == 0).all() and (r.iterations[0::2] <= 8).all(), (r.status, r.iterations)
    assert (r.status[1::2] == 1).all() and (r.iterations[1::2] >= 20).all(), (r.status, r.iterations)
    for q, col in ((0, fast), (1, slow)):
        one = es.peak_height(T_MID, *(np.array([v]) for v in col), check_hull=False)
        for lane in range(q, 64, 2):
            _same_bits(_cut(r, slice(lane, lane + 1)), one, lane)


# ==== 4. hull and NaN ========================================================================================================
def test_hull_and_nan_starts():
    """192 columns of the default fit: a wave whose starts are all far above every beam (it leaves before any walk), a wave
    with every other start there, a wave as drawn with two NaN starts: status 3 and four NaNs for all of these, numbers for
    others.  Without the hull test the columns that started inside keep their bits."""
    f, es, _ = _estimate('default')
    rng = np.random.default_rng(192)
    lat, lon, start = rng.uniform(77., 79., 192), rng.uniform(258, 266, 192), rng.uniform(250e3, 350e3, 192)
    start[:64] = rng.uniform(2000e3, 3000e3, 64)
    start[64:128:2] = rng.uniform(2000e3, 3000e3, 32)
    start[[130, 191]] = np.nan
    lo, hi = start - 100e3, start + 100e3
    t = _t_rec(f)
    r = es.peak_height(t, lat, lon, start, lo, hi)
    out3 = np.zeros(192, dtype=bool)
    out3[:64] = out3[64:128:2] = out3[[130, 191]] = True
    assert (r.status[out3] == 3).all() and (r.iterations[out3] == 0).all()
    for v in r[:4]:
        assert np.isnan(v[out3]).all()
    inside = es.check_hull(lat, lon, np.nan_to_num(start))
    assert np.array_equal(r.status == 3, ~inside) and 30 < inside.sum() < 128
    stayed = inside & (r.status != 4)                                    # (a search that left the hull is blanked on the host)
    assert stayed.sum() >= 20 and np.isfinite(r.slope[stayed]).all() and np.isfinite(r.curvature[stayed]).all()
    free = es.peak_height(t, lat, lon, start, lo, hi, check_hull=False)
    assert (free.status[[130, 191]] == 3).all() and (free.status[:128] != 3).all()
    kept = r.status != 4
    _same_bits(_cut(free, inside & kept), _cut(r, inside & kept))


def test_a_nan_record_reaches_only_itself():
    """Three records of the k8l2 fit, one NaN in the second: that record is status 3 and NaN in every column, the other two
    keep the bits they have without it."""
    from volumetricinterp_amd.estimate import Estimate
    f, es, _ = _estimate('k8l2')
    Cn = np.array(f['Coeffs'])
    Cn[1, 5] = np.nan
    bad = Estimate.from_arrays(Cn, f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))
    rng = np.random.default_rng(66)
    lat, lon = rng.uniform(77., 79., 66), rng.uniform(258, 266, 66)
    times = [_t_rec(f, i) for i in range(3)]
    good = es.peak_height(times, lat, lon, 300e3, 200e3, 500e3)
    r = bad.peak_height(times, lat, lon, 300e3, 200e3, 500e3)
    assert (good.status != 3).sum() >= 3 * 33
    assert (r.status[1] == 3).all() and all(np.isnan(v[1]).all() for v in r[:4])
    for i in (0, 2):
        _same_bits(_cut(r, i), _cut(good, i), i)


def test_a_search_that_leaves_the_hull():
    """The hull is tested on the device at the start only; the end point is tested on the host.  Minima of the default fit
    searched upwards from 300 km in a bracket that reaches 1500 km end far above the beams: status 4 and NaN exactly where
    the height found without the hull test is outside the hull, the other columns keep their bits."""
    f, es, _ = _estimate('default')
    rng = np.random.default_rng(64)
    lat, lon = rng.uniform(77, 79, 8), rng.uniform(258, 266, 8)
    t = _t_rec(f)
    started = es.check_hull(lat, lon, np.full(8, 300e3))
    assert started.sum() >= 4
    out, status, it = _raw(es, es.get_C(t)[0], lat, lon, 300e3, 300e3, 1500e3, kind=-1, hull=True)
    ended = es.check_hull(lat, lon, np.nan_to_num(out[0, 0]))
    left = started & ~ended
    assert np.array_equal(status[0] == 3, ~started) and left.sum() >= 2
    r = es.peak_height(t, lat, lon, 300e3, 300e3, 1500e3, kind='min')
    assert np.array_equal(r.status == 4, left) and np.array_equal(r.status == 3, ~started)
    for v in r[:4]:
        assert np.isnan(v[left]).all()
    assert np.array_equal(r.iterations, it[0])
    stay = started & ended
    assert np.array_equal(r.status[stay], status[0][stay]) and np.array_equal(_bits(r.slope[stay]), _bits(out[2, 0][stay]))


# ==== 5. statuses and kind ===================================================================================================
def test_statuses():
    """Column (79, 266) of the default-order layer from 200 km has no interior maximum below it and walks to the lower end of
    the bracket: status 1 at max_iter = 48, status 2 at max_iter = 20 (the mirror's, tests/test_peak_host.py).  max_iter = 0
    returns the start with its value, slope and curvature and status 2; lo > start is status 3."""
    es = _layer_es('default')
    col = np.array([79.]), np.array([266.])
    r = es.peak_height(T_MID, *col, 200e3, LO, HI, check_hull=False)
    assert r.status[0] == 1 and np.isnan(r.height[0]) and np.isnan(r.value[0]) and r.slope[0] < 0. and r.iterations[0] > 20
    out, status, it = _raw(es, es.Coeffs, *col, 200e3, LO, HI)
    assert status[0, 0] == 1 and abs(out[0, 0, 0] - LO) <= 2. * TOL
    r = es.peak_height(T_MID, *col, 200e3, LO, HI, max_iter=20, check_hull=False)
    assert r.status[0] == 2 and r.iterations[0] == 20 and np.isnan(r.height[0]) and np.isfinite(r.slope[0])
    r = es.peak_height(T_MID, *col, 200e3, LO, HI, max_iter=0, check_hull=False)
    out, status, it = _raw(es, es.Coeffs, *col, 200e3, LO, HI, max_iter=0)
    assert r.status[0] == 2 and r.iterations[0] == 0 and status[0, 0] == 2 and it[0, 0] == 0 and out[0, 0, 0] == 200e3
    pt = col + (np.array([200e3]),)
    C = es.Coeffs[0]
    for k, (got, want, basis) in enumerate((
            (out[1, 0, 0], es(T_MID, *pt, check_hull=False)[0], es.model.basis(*pt)[0]),
            (out[2, 0, 0], es.gradient(T_MID, *pt, check_hull=False, frame='enu')[0, 2],
             np.einsum('c,cn->n', es.model.gradient_frame(*pt)[0, 2], es.model.grad_basis(*pt)[0])),
            (out[3, 0, 0], es.hessian(T_MID, *pt, check_hull=False, frame='enu')[0, 2, 2],
             es.model.hess_basis(*pt, frame='enu')[0, 2]))):
        assert abs(got - want) <= 1e-12 * (np.abs(basis) @ np.abs(C)), k
    assert out[2, 0, 0] == r.slope[0] and out[3, 0, 0] == r.curvature[0]
    r = es.peak_height(T_MID, *col, 200e3, 210e3, HI, check_hull=False)
    assert r.status[0] == 3 and r.iterations[0] == 0 and all(np.isnan(v[0]) for v in r[:4])
    r = es.peak_height(T_MID, *col, 460e3, LO, HI, check_hull=False)
    assert r.status[0] == 3


def test_min_of_the_negated_coefficients():
    """kind='min' on -C walks the heights of kind='max' on C bit for bit - every comparison of the iteration carries the sign
    - with value, slope and curvature negated; statuses and iterations the same."""
    es = _layer_es('k8l2')
    lat, lon, start, _ = _layer_columns('k8l2')
    neg = _bare('k8l2', -es.Coeffs[0])
    a = _raw(es, es.Coeffs, lat, lon, start, LO, HI, kind=1)
    b = _raw(neg, neg.Coeffs, lat, lon, start, LO, HI, kind=-1)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and (a[1] == 0).all()
    assert np.array_equal(_bits(a[0][0]), _bits(b[0][0]))
    assert np.array_equal(_bits(a[0][1:]), _bits(-b[0][1:]))
    ra = es.peak_height(T_MID, lat, lon, start, LO, HI, kind='max', check_hull=False)
    rb = neg.peak_height(T_MID, lat, lon, start, LO, HI, kind='min', check_hull=False)
    assert np.array_equal(_bits(ra.height), _bits(rb.height)) and np.array_equal(_bits(ra.value), _bits(-rb.value))


# ==== 6. errors ==============================================================================================================
def test_error_bars():
    """error=True on the layer with the covariance of the k8l2 fixture's first record: height_error is
    sqrt(gradient_covariance(frame='enu')[..., 2, 2]) / |curvature| and value_error is error(), both at the returned
    heights; the six fields before them are those of error=False.  Without a covariance it raises, as the error entries do."""
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_k8l2')
    layer = _layer_es('k8l2')
    es = Estimate.from_arrays(layer.Coeffs, f['Covariance'][:1], [[0., 60.]], np.zeros((4, 3)), layer.config_file_text)
    lat, lon, start, _ = _layer_columns('k8l2')
    lat, lon, start = (np.append(a, v) for a, v in ((lat, 78.), (lon, 262.), (start, np.nan)))
    r = es.peak_height(T_MID, lat, lon, start, LO, HI, check_hull=False, error=True)
    assert r._fields == FIELDS + ('height_error', 'value_error') and r.height_error.shape == (13,)
    _same_bits(r[:6], es.peak_height(T_MID, lat, lon, start, LO, HI, check_hull=False))
    ok = r.status == 0
    assert ok[:12].all() and r.status[12] == 3 and np.isnan(r.height_error[12]) and np.isnan(r.value_error[12])
    pts = lat[ok], lon[ok], r.height[ok]
    cov = es.gradient_covariance(T_MID, *pts, check_hull=False, frame='enu')[:, 2, 2]
    assert (cov > 0.).all()
    assert np.array_equal(r.height_error[ok], np.sqrt(cov) / np.abs(r.curvature[ok]))
    assert np.array_equal(r.value_error[ok], es.error(T_MID, *pts, check_hull=False))
    print('height errors %s m, value errors %s' % (r.height_error[:12:3], r.value_error[:12:3]))
    bare = Estimate.from_arrays(layer.Coeffs, None, [[0., 60.]], np.zeros((4, 3)), layer.config_file_text)
    with pytest.raises(ValueError, match='no covariance'):
        bare.peak_height(T_MID, lat, lon, start, LO, HI, check_hull=False, error=True)


# ==== 7. refusals and timing =================================================================================================
def test_refusals():
    """An order beyond the compiled ones (MAXL 13) and the radial-basis model: VI_ERR_UNSUPPORTED (-6) from the library with
    the output buffers untouched - nothing was launched -, VinterpError from Python.  A bad kind, tol or max_iter, a null
    pointer and facets counted but not given: VI_ERR_INVALID (-1), ValueError from Python.  T = 0 and Q = 0 are no-ops."""
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

    def call(es, dev, T=1, nq=Q, kind=1, max_iter=48, tol=TOL, F=0, out=True):
        N = es.model.nbasis
        d = [dev.up(v) for v in (lat, lon, np.full(Q, 300e3), np.full(Q, LO), np.full(Q, HI), np.ones(N))]
        dO, dS, dI = dev.up(np.full(4 * Q, 7.)), dev.up(np.full(Q, 7, dtype=np.int32)), dev.up(np.full(Q, 7, dtype=np.int32))
        rc = _lib.lib.vi_eval_peak_f64(es.model.handle(), T, nq, *(v.ptr for v in d), None, F, 0., kind, max_iter, tol,
                                       dO.ptr if out else None, dS.ptr, dI.ptr)
        es.model.ctx.sync()
        assert np.array_equal(dO.download(), np.full(4 * Q, 7.))
        assert np.array_equal(dS.download(), np.full(Q, 7)) and np.array_equal(dI.download(), np.full(Q, 7))
        return rc

    for es, what in ((big, 'beyond the compiled limits'), (rbf, 'only the sphharmlag model')):
        with es.model.ctx.scope() as dev:
            assert call(es, dev) == -6 and what in _lib.lib.vi_last_error().decode()
        with pytest.raises(_lib.VinterpError, match=what):
            es.peak_height(_t_rec(fr) if es is rbf else T_MID, lat, lon, 300e3, LO, HI, check_hull=False)
    with ok.model.ctx.scope() as dev:
        for bad in (dict(kind=0), dict(kind=2), dict(tol=0.), dict(tol=-1.), dict(tol=np.nan), dict(tol=np.inf),
                    dict(max_iter=-1), dict(F=3), dict(out=False), dict(T=-1), dict(nq=-1)):
            assert call(ok, dev, **bad) == -1, bad
        assert call(ok, dev, T=0) == 0 and call(ok, dev, nq=0) == 0
    for bad in (dict(kind='xyz'), dict(kind=1), dict(tol=0.), dict(tol=np.nan), dict(max_iter=-1), dict(max_iter=1.5)):
        with pytest.raises(ValueError, match='kind must be|tol must be|max_iter must be'):
            ok.peak_height(T_MID, lat, lon, 300e3, LO, HI, check_hull=False, **bad)
    with pytest.raises(ValueError, match='broadcast'):
        ok.peak_height(T_MID, lat, lon, np.zeros(Q + 1), LO, HI, check_hull=False)
    with pytest.raises(ValueError, match='one shape'):
        ok.peak_height(T_MID, lat, lon[:-1], 300e3, LO, HI, check_hull=False)
    empty = ok.peak_height([], lat, lon, 300e3, LO, HI, check_hull=False)
    assert all(v.shape == (0, Q) for v in empty)
    empty = ok.peak_height(T_MID, lat[:0], lon[:0], 300e3, LO, HI, check_hull=False)
    assert all(v.shape == (0,) for v in empty) and empty.status.dtype == np.int32


def test_calls_are_timed():
    """The entry records its kernel for vi_eval_kernel_ms, as its siblings do."""
    es = _layer_es('k8l2')
    lat, lon, start, _ = _layer_columns('k8l2')
    ctx = es.model.ctx
    ctx.eval_timing(True)
    try:
        es.peak_height(T_MID, lat, lon, start, LO, HI, check_hull=False)
        assert 0. < ctx.eval_kernel_ms() < 1000.
    finally:
        ctx.eval_timing(False)


# ==== 8. from a grid peak ====================================================================================================
def test_refining_a_grid_peak():
    """The use the entry is made for: ResidentGrid.peak on a 25 km grid, peak_brackets, peak_height.  On the layer every
    column refines to an interior maximum inside the two grid cells around the grid peak, and the refined value is at least
    the grid's - up to 1e-12 of the size of its terms, the two being different device summations."""
    from volumetricinterp_amd.estimate import peak_brackets
    es = _layer_es('k8l2')
    alt = np.arange(150e3, 450e3 + 1., 25e3)
    lat2, lon2 = np.meshgrid(np.linspace(77.5, 78.5, 3), np.linspace(259., 265., 4), indexing='ij')
    grid = [np.broadcast_to(a[..., None], lat2.shape + alt.shape) for a in (lat2, lon2)] + \
           [np.broadcast_to(alt, lat2.shape + alt.shape)]
    with es.resident_grid(*grid, check_hull=False) as g:
        v, i = g.peak([T_MID])
    assert v.shape == (1, 3, 4) and (i > 0).all() and (i < alt.size - 1).all()
    start, lo, hi = peak_brackets(alt, i)
    r = es.peak_height([T_MID], lat2, lon2, start, lo, hi, check_hull=False)
    assert r.height.shape == (1, 3, 4) and (r.status == 0).all()
    assert (r.height > lo).all() and (r.height < hi).all()
    terms = (np.abs(es.model.basis(lat2.ravel(), lon2.ravel(), r.height.ravel())) @ np.abs(es.Coeffs[0])).reshape(v.shape)
    assert (r.value >= v - 1e-12 * terms).all()
    print('refined - grid height: %s km' % np.round((r.height - start)[0] / 1e3, 2))
