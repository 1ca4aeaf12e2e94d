"""Host tests of the level-crossing search (no GPU): estimate.level_brackets, level_ref.crossing_index on hand-made columns,
and the NumPy mirror of the device iteration (tests/level_ref.py) against scipy.optimize.brentq on the mirror's own value -
the layers of tests/test_peak_host.py, at 0.5 and 0.8 of each column's peak value, below and above the peak."""
import functools

import numpy as np
import pytest
from scipy.optimize import brentq

import level_ref as lv
from test_peak_host import COLUMNS, HI, LO, TOL, layer, layer_searches

FRACTIONS = (0.5, 0.8)


@functools.lru_cache(maxsize=None)
def level_searches(case):
    """The mirror's searches of the four columns at 0.5 and 0.8 of the column's peak value (the mirror peak searches of
    tests/test_peak_host.py), on the bottomside (150 km, peak height) and on the topside (peak height, 450 km):
    (lat, lon, level, lo, hi, result dict), 16 searches - column-major, then fraction, then side."""
    o, C = layer(case)
    peaks = layer_searches(case)[3]
    lat, lon, level, lo, hi = [], [], [], [], []
    for c, (la, lg) in enumerate(COLUMNS):
        # the interior peak (status 0) of the column's three searches with the largest value: at the default order the grid
        # maximum of column (79, 266) sits on the lower end of the bracket and only the search from 440 km finds a peak
        ok = [k for k in range(3 * c, 3 * c + 3) if peaks['status'][k] == 0]
        assert ok, (case, c)
        k = max(ok, key=lambda k: peaks['f'][k])
        hp, fp = peaks['h'][k], peaks['f'][k]
        assert np.isfinite(hp) and LO < hp < HI and fp > 0., (case, c, hp, fp)
        for frac in FRACTIONS:
            for a, b in ((LO, hp), (hp, HI)):
                lat.append(la), lon.append(lg), level.append(frac * fp), lo.append(a), hi.append(b)
    args = tuple(np.array(v) for v in (lat, lon, level, lo, hi))
    r = lv.level_search(o, C, *args, TOL, 48)
    for v in args + tuple(r.values()):
        v.setflags(write=False)
    return args + (r,)


def _value(o, C, la, lg, L):
    return lambda h: float(lv.walk(o, C, [la], [lg], [h])[0][0]) - L


def test_level_brackets():
    """The grid altitudes at the index and the one after it, the lower first on a descending axis too; NaN for -1; the shape
    of the index; the index lies in [-1, len - 1)."""
    from volumetricinterp_amd.estimate import level_brackets
    alt = np.array([100e3, 150e3, 225e3, 300e3, 500e3])
    idx = np.array([[2, 0, 3], [-1, 1, 3]], dtype=np.int32)
    lo, hi = level_brackets(alt, idx)
    assert lo.shape == hi.shape == (2, 3) and lo.dtype == hi.dtype == np.float64
    assert np.array_equal(lo, [[225e3, 100e3, 300e3], [np.nan, 150e3, 300e3]], equal_nan=True)
    assert np.array_equal(hi, [[300e3, 150e3, 500e3], [np.nan, 225e3, 500e3]], equal_nan=True)
    l2, h2 = level_brackets(alt[::-1], np.where(idx < 0, -1, 3 - idx))      # pair (l, l + 1) is pair (3 - l, 4 - l) reversed
    assert np.array_equal(l2, lo, equal_nan=True) and np.array_equal(h2, hi, equal_nan=True)
    assert (l2[idx >= 0] < h2[idx >= 0]).all()
    one = level_brackets(alt, np.zeros((), dtype=np.int64))
    assert all(v.shape == () for v in one) and one[0] == 100e3 and one[1] == 150e3
    assert all(v.shape == (0,) for v in level_brackets(alt, np.zeros(0, dtype=np.int64)))
    single = level_brackets([250e3], np.array([-1]))
    assert all(np.isnan(v).all() for v in single)
    for bad_axis in (np.zeros((2, 2)), [], [1., np.nan]):
        with pytest.raises(ValueError, match='alt_axis'):
            level_brackets(bad_axis, idx)
    for bad_idx in (np.array([4]), np.array([-2])):
        with pytest.raises(ValueError, match='index must lie'):
            level_brackets(alt, bad_idx)
    with pytest.raises(ValueError, match='index must lie'):
        level_brackets([250e3], np.array([0]))
    with pytest.raises(ValueError, match='integer'):
        level_brackets(alt, np.array([1.]))


def test_crossing_index_on_hand_made_columns():
    """Columns written by hand: NaN samples break a pair, a sample equal to the level crosses in both directions with both
    neighbours, an axis of one sample has no pair and one of two samples has one; every which and direction; a NaN level."""
    nan = np.nan
    cols = np.array([[1., 2., 4., 3., 1., 5.],        # level 2.5: up at 1, down at 3, up at 4
                     [1., nan, 4., 2., nan, 1.],      # NaN breaks (0,1), (1,2), (3,4), (4,5): only the pair (2,3) is left
                     [0., 2.5, 5., 2.5, 0., 0.],      # samples equal to the level
                     [5., 4., 3., 3., 3., 3.],        # never reaches 2.5
                     [nan] * 6])[None]                # (T = 1, 5, 6)
    want = {('first', 'any'): [1, 2, 0, -1, -1], ('last', 'any'): [4, 2, 3, -1, -1],
            ('first', 'up'): [1, -1, 0, -1, -1], ('last', 'up'): [4, -1, 1, -1, -1],
            ('first', 'down'): [3, 2, 2, -1, -1], ('last', 'down'): [3, 2, 3, -1, -1]}
    for (which, direction), idx in want.items():
        got = lv.crossing_index(cols, 2.5, -1, which, direction)
        assert got.shape == (1, 5) and got.dtype == np.int32 and list(got[0]) == idx, (which, direction, got)
        # the same columns along the other axis of the grid
        assert np.array_equal(lv.crossing_index(np.swapaxes(cols, 1, 2), 2.5, 0, which, direction), got)
    # a level per column, one of them NaN
    got = lv.crossing_index(cols, np.array([[2.5, 3.5, nan, 4.5, 0.]]), -1, 'first', 'any')
    assert list(got[0]) == [1, 2, -1, 0, -1]
    # L = 1: no pair; L = 2: one
    assert list(lv.crossing_index(np.array([[[2.5], [1.]]]), 2.5)[0]) == [-1, -1]
    two = np.array([[[1., 3.], [3., 1.], [2., 2.], [nan, 3.]]])
    assert list(lv.crossing_index(two, 2., -1, 'first', 'up')[0]) == [0, -1, 0, -1]
    assert list(lv.crossing_index(two, 2., -1, 'last', 'down')[0]) == [-1, 0, 0, -1]


def test_mirror_finds_the_root_of_its_own_value_k8l2():
    """MAXK 8 x MAXL 2: all 16 searches - four columns, 0.5 and 0.8 of the peak, bottomside and topside - end with status 0
    within 12 iterations, within tol of the root scipy.optimize.brentq (xtol 1e-9) finds of the mirror's own value in the same
    bracket.  The search stops after a step of at most tol or on an exact zero, and a Newton step next to a simple root is as
    long as the distance it leaves to first order.  Prototype: 3 to 5 iterations, heights 234.3 to 270.7 km below and 379.7 to
    438.2 km above the peak, within 4e-9 m of brentq."""
    o, C = layer('k8l2')
    lat, lon, level, lo, hi, r = level_searches('k8l2')
    assert np.array_equal(r['status'], np.zeros(16, dtype=np.int32)), r['status']
    assert (r['it'] <= 12).all(), r['it']
    for k in range(16):
        root = brentq(_value(o, C, lat[k], lon[k], level[k]), lo[k], hi[k], xtol=1e-9, rtol=1e-15)
        dist = abs(r['h'][k] - root)
        print('column (%.1f, %.1f) level %.4e in (%.1f, %.1f) km: brentq %.6f m, mirror off by %.1e m in %d iterations, slope %.3e'
              % (lat[k], lon[k], level[k], lo[k] / 1e3, hi[k] / 1e3, root, dist, r['it'][k], r['d1'][k]))
        assert dist <= TOL, (k, dist)
        assert lo[k] < r['h'][k] < hi[k] and (r['d1'][k] > 0.) == (k % 2 == 0)        # bottomside up, topside down
        assert abs(r['f'][k] - level[k]) <= abs(r['d1'][k]) * TOL + 1e-12 * r['vterms'][k]


def test_mirror_reports_a_bracket_without_a_sign_change():
    """The whole bracket 150 to 450 km at those levels: the value is below the level at both ends (prototype: f(150 km) -5.8e9
    to -1.0e10, f(450 km) 1.07e11 to 1.13e11, both below half the peak), so status 1 after the two walks of the ends, no
    iteration, NaN."""
    o, C = layer('k8l2')
    lat, lon, level, lo, hi, _ = level_searches('k8l2')
    r = lv.level_search(o, C, lat, lon, level, LO, HI, TOL, 48)
    assert (r['status'] == 1).all() and (r['it'] == 0).all(), (r['status'], r['it'])
    for k in ('h', 'f', 'd1'):
        assert np.isnan(r[k]).all()


def test_mirror_at_the_default_order():
    """The same layer at the default order (MAXK 4 x MAXL 6), whose unregularised fit cancels heavily: not every column has
    every crossing.  The mirror's status is 0 exactly where the value minus the level changes sign over the bracket - what
    brentq asks for - and 1 elsewhere, and where it is 0 the height is within tol of brentq's root (prototype: 1.4e-4 m)."""
    o, C = layer('default')
    lat, lon, level, lo, hi, r = level_searches('default')
    print('status', r['status'], 'iterations', r['it'])
    print('heights', r['h'])
    for k in range(16):
        g = _value(o, C, lat[k], lon[k], level[k])
        ga, gb = g(lo[k]), g(hi[k])
        change = (ga > 0.) != (gb > 0.) and ga != 0. and gb != 0.
        assert r['status'][k] == (0 if change else 1), (k, ga, gb, r['status'][k])
        if change:
            root = brentq(g, lo[k], hi[k], xtol=1e-9, rtol=1e-15)
            print('search %d: brentq %.6f m, mirror off by %.1e m in %d iterations' % (k, root, abs(r['h'][k] - root), r['it'][k]))
            assert abs(r['h'][k] - root) <= TOL, (k, r['h'][k], root)
    assert (r['status'] == 0).sum() >= 4 and (r['status'] == 1).sum() >= 1


def test_mirror_statuses_of_bad_input():
    """max_iter = 0 returns the secant point of the two ends with status 2; a NaN level, a NaN end, a non-finite column and
    lo >= hi give status 3 and NaN; an all-zero coefficient row with level 0 is an exact hit at lo: status 0, no iteration."""
    o, C = layer('k8l2')
    lat, lon, level, lo, hi, ref = level_searches('k8l2')
    r = lv.level_search(o, C, [lat[0]] * 6, [lon[0], lon[0], lon[0], np.nan, lon[0], lon[0]],
                        [level[0], np.nan, level[0], level[0], level[0], level[0]],
                        [lo[0], lo[0], np.nan, lo[0], hi[0], hi[0]], [hi[0], hi[0], hi[0], hi[0], hi[0], lo[0]], TOL, 0)
    assert list(r['status']) == [2, 3, 3, 3, 3, 3] and list(r['it']) == [0] * 6
    assert lo[0] < r['h'][0] < hi[0] and np.isfinite([r['f'][0], r['d1'][0]]).all()
    for k in ('h', 'f', 'd1'):
        assert np.isnan(r[k][1:]).all()
    one = lv.level_search(o, C, [lat[0]], [lon[0]], level[0], lo[0], hi[0], TOL, 1)
    assert one['status'][0] == 2 and one['it'][0] == 1
    z = lv.level_search(o, np.zeros_like(C), [lat[0]], [lon[0]], 0., lo[0], hi[0], TOL, 48)
    assert z['status'][0] == 0 and z['it'][0] == 0 and z['h'][0] == lo[0] and z['f'][0] == 0. and z['d1'][0] == 0.
