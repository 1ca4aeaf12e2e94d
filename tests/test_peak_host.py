"""Host tests of the sub-grid peak search (no GPU): estimate.peak_brackets, and the NumPy mirror of the device iteration
(tests/peak_ref.py) against scipy.optimize.brentq on the mirror's own slope - the Chapman layer of synth.chapman_record fitted
at MAXK 8 x MAXL 2 on the 11 x 50 beams and at the default order on the 26 x 100 beams."""
import functools

import numpy as np
import pytest
from scipy.optimize import brentq

import peak_ref as pk

# the columns of the layer tests (gdlat, gdlon) and their bracket, metres
COLUMNS = ((78., 262.), (77.2, 258.), (79., 266.), (78.5, 255.))
LO, HI = 150e3, 450e3
TOL = 1e-3


def layer_oracle(case):
    import oracle
    return oracle.SphHarmLagOracle(maxk=8, maxl=2) if case == 'k8l2' else oracle.SphHarmLagOracle()


@functools.lru_cache(maxsize=None)
def layer(case):
    """(oracle, coefficients) of the layer fit: 'k8l2' on GEOM_C1, 'default' (MAXK 4 x MAXL 6) on GEOM_C2."""
    from volumetricinterp_amd import synth
    o = layer_oracle(case)
    C = pk.layer_fit(o, synth.GEOM_C1 if case == 'k8l2' else synth.GEOM_C2)
    C.setflags(write=False)
    return o, C


def grid_start(o, C, lat, lon):
    """The altitude of the largest sample of the column on a 25 km grid over the bracket."""
    alt = np.arange(LO, HI + 1., 25e3)
    f = pk.walk(o, C, np.full(alt.size, lat), np.full(alt.size, lon), alt)[0]
    return float(alt[int(np.argmax(f))])


@functools.lru_cache(maxsize=None)
def layer_searches(case):
    """The mirror's searches of the four columns from 200 km, 440 km and the grid maximum: (lat, lon, start, result dict)."""
    o, C = layer(case)
    lat = np.repeat([c[0] for c in COLUMNS], 3)
    lon = np.repeat([c[1] for c in COLUMNS], 3)
    start = np.concatenate([[200e3, 440e3, grid_start(o, C, *c)] for c in COLUMNS])
    return lat, lon, start, pk.peak_search(o, C, lat, lon, start, LO, HI, 1, TOL, 48)


def test_peak_brackets():
    """The grid altitude at the index and its two neighbours; the sample itself at the ends of the axis; NaN for -1; the
    shape of the index; a descending axis gives lo <= start <= hi all the same."""
    from volumetricinterp_amd.estimate import peak_brackets
    alt = np.array([100e3, 150e3, 225e3, 300e3, 500e3])
    idx = np.array([[2, 0, 4], [-1, 1, 3]], dtype=np.int32)
    start, lo, hi = peak_brackets(alt, idx)
    assert start.shape == lo.shape == hi.shape == (2, 3) and start.dtype == np.float64
    assert np.array_equal(start, [[225e3, 100e3, 500e3], [np.nan, 150e3, 300e3]], equal_nan=True)
    assert np.array_equal(lo, [[150e3, 100e3, 300e3], [np.nan, 100e3, 225e3]], equal_nan=True)
    assert np.array_equal(hi, [[300e3, 150e3, 500e3], [np.nan, 225e3, 500e3]], equal_nan=True)
    s2, l2, h2 = peak_brackets(alt[::-1], 4 - np.where(idx < 0, 5, idx))
    for a, b in ((s2, start), (l2, lo), (h2, hi)):
        assert np.array_equal(a, b, equal_nan=True)
    one = peak_brackets([250e3], np.zeros((), dtype=np.int64))
    assert all(v.shape == () and v == 250e3 for v in one)
    assert all(v.shape == (0,) for v in peak_brackets(alt, np.zeros(0, dtype=np.int64)))
    for bad_axis in (np.zeros((2, 2)), [], [1., np.nan]):
        with pytest.raises(ValueError, match='alt_axis'):
            peak_brackets(bad_axis, idx)
    for bad_idx in (np.array([5]), np.array([-2])):
        with pytest.raises(ValueError, match='index must lie'):
            peak_brackets(alt, bad_idx)
    with pytest.raises(ValueError, match='integer'):
        peak_brackets(alt, np.array([1.]))


def test_mirror_finds_the_root_of_its_own_slope_k8l2():
    """MAXK 8 x MAXL 2: every column from every start converges (status 0) to the zero of the mirror's own slope that
    scipy.optimize.brentq finds between 200 km and the top of the bracket (the slope of column (77.2, 258) is negative again at
    150 km: brentq wants a change of sign).  Bound: tol.  The search stops after a step of at most tol, and a Newton step
    on a slope with negative curvature next to a simple zero is at least as long as the distance it leaves, so the returned
    height is within tol of the zero (prototype: 2e-9 m, 3 to 5 iterations, heights 320.9 to 326.8 km, curvature -33 to -41)."""
    o, C = layer('k8l2')
    lat, lon, start, r = layer_searches('k8l2')
    assert np.array_equal(r['status'], np.zeros(12, dtype=np.int32)), r['status']
    assert (r['it'] >= 1).all() and (r['it'] <= 12).all(), r['it']
    assert (r['d2'] < 0.).all() and (r['h'] > 300e3).all() and (r['h'] < 350e3).all()
    for c, (la, lg) in enumerate(COLUMNS):
        root = brentq(lambda h: float(pk.walk(o, C, [la], [lg], [h])[1][0]), 200e3, HI, xtol=1e-9, rtol=1e-15)
        dist = np.abs(r['h'][3 * c:3 * c + 3] - root)
        print('column %r: brentq %.6f m, mirror from 200 km / 440 km / grid maximum off by %s m in %s iterations, curvature %.2f'
              % ((la, lg), root, ' / '.join('%.1e' % d for d in dist), r['it'][3 * c:3 * c + 3], r['d2'][3 * c]))
        assert (dist <= TOL).all(), (la, lg, dist)


def test_mirror_at_the_default_order():
    """The same layer at the default order (MAXK 4 x MAXL 6) on the 26 x 100 beams: where the three starts of a column all
    converge they agree within 2 tol (each is within tol of one zero of the slope), and column (79, 266) from 200 km, which
    has no interior maximum below it, walks to the lower end of the bracket: status 1 at max_iter = 48, status 2 at 20."""
    o, C = layer('default')
    lat, lon, start, r = layer_searches('default')
    print('status', r['status'], 'iterations', r['it'])
    print('heights', r['h'])
    agree = 0
    for c in range(len(COLUMNS)):
        sl = slice(3 * c, 3 * c + 3)
        if (r['status'][sl] == 0).all():
            agree += 1
            assert np.ptp(r['h'][sl]) <= 2. * TOL, (COLUMNS[c], r['h'][sl])
    assert agree >= 3
    edge = pk.peak_search(o, C, [79.], [266.], 200e3, LO, HI, 1, TOL, 48)
    assert edge['status'][0] == 1 and abs(edge['h'][0] - LO) <= 2. * TOL, edge
    short = pk.peak_search(o, C, [79.], [266.], 200e3, LO, HI, 1, TOL, 20)
    assert short['status'][0] == 2 and short['it'][0] == 20 and np.isfinite(short['h'][0]), short


def test_mirror_statuses_of_bad_input():
    """max_iter = 0 evaluates the start (status 2); a NaN start, a non-finite column and lo > start give status 3 and NaN."""
    o, C = layer('k8l2')
    r = pk.peak_search(o, C, [78., 78., np.nan, 78.], [262.] * 4, [300e3, np.nan, 300e3, 300e3], [LO, LO, LO, 310e3], HI,
                       1, TOL, 0)
    assert list(r['status']) == [2, 3, 3, 3] and list(r['it']) == [0] * 4
    assert r['h'][0] == 300e3 and np.isfinite([r['f'][0], r['d1'][0], r['d2'][0]]).all()
    for k in ('h', 'f', 'd1', 'd2'):
        assert np.isnan(r[k][1:]).all()
    f = pk.walk(o, C, [78.], [262.], [300e3])
    assert r['f'][0] == f[0][0] and r['d1'][0] == f[1][0] and r['d2'][0] == f[2][0]
