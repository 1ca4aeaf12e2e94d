"""tests/hull_ref.py on the host, no GPU: the constructions lose no point to their margins, the by-construction plane distances
agree with the longdouble evaluation, the classification of the inputs is what each case is meant to exercise, and
estimate.hull_chords agrees with the longdouble restatement of the clip on the ray sets the device is tested with."""
import numpy as np
import pytest

import hull_ref as hr


@pytest.mark.parametrize('group', ['slots', 'places', 'dilated'])
def test_no_point_is_left_out_and_the_distances_are_the_constructed_ones(group):
    """Every case of the list: dropped == 0; a point's own facet is at tol + sigma delta within 1e-6 m, every other facet at
    (rho + tol)(n_g . n_f - 1) + sigma delta n_g . n_f + tol, also within 1e-6 m - the construction's formula against the
    longdouble planes through the rounded geodetic coordinates - and at least 1e-3 m inside."""
    cases = {'slots': hr.slot_cases(), 'places': hr.place_cases(), 'dilated': [c for c in hr.all_cases() if c.tol]}[group]
    assert cases
    for c in cases:
        b = hr.build(c)
        assert len(b.lat) == 2 * len(hr.STEPS) * c.F
        assert b.dropped == 0, (hr.case_name(c), b.dropped)
        sd = b.sigma * b.delta
        assert np.all(b.delta > 0) and np.all(b.delta <= np.array(hr.STEPS)[b.step])
        assert float(np.abs(b.own - (c.tol + sd)).max()) <= hr.OWN_MARGIN
        n = b.eq[:, :3]
        G = n @ n.T
        np.fill_diagonal(G, -1.)
        g = G[b.facet]                                                   # (point, other facet)
        formula = ((c.rho + c.tol) * (g - 1.) + sd[:, None] * g + c.tol).max(axis=1)
        assert float(np.abs(b.other - formula).max()) <= hr.OWN_MARGIN, hr.case_name(c)
        assert float((b.other - c.tol).max()) <= -hr.OTHER_MARGIN
        assert np.array_equal(b.expect, b.sigma < 0)
        assert np.all(np.isfinite(b.lat)) and np.all(np.abs(b.lat) <= 90.) and np.all(np.isfinite(b.alt))
        if c.lon == 'wrap':                                              # (5 km about 0.2 E does not reach the meridian)
            assert b.lon.min() >= 0. and (b.lon.max() > 180. or c.rho < 1e5)
        elif c.centre == 'equator':
            assert b.lon.min() < 0. or c.rho < 1e5
        # the paths of the prefilter: the smallest step is inside every band; an uncapped 300 m step outside the largest
        # band a judged point can have; the centre at 20 200 km switches the prefilter off for every point
        assert hr.BAND_MAX < hr.STEPS[-1] and hr.STEPS[0] < hr.BAND_ABS
        assert b.off.sum() + b.inband.sum() + b.outband.sum() == len(b.lat)
        if c.centre == 'gnss':
            assert b.off.all()
        else:
            assert not b.off.any() and b.inband.sum() >= 2 * c.F
            assert np.all(b.inband[b.step == 0])
            if np.all(b.delta[b.step == 3] == hr.STEPS[3]):
                assert np.all(b.outband[b.step == 3])
        print('%s: %d points, off %d, in band %d, outside band %d' % (hr.case_name(c), len(b.lat), b.off.sum(), b.inband.sum(),
                                                                      b.outband.sum()))


def test_facet_zero_puts_the_reference_point_where_the_case_wants_it():
    """'radial': c0, the foot of the origin's perpendicular on facet 0, is the tangent point of facet 0 - on the hull;
    'horizontal': the plane passes rho from the Earth's centre and c0 lies about |c| from the hull."""
    for c in (hr.Case(33, 2e5, 'north', 'radial'), hr.Case(33, 2e5, 'north', 'horizontal'), hr.Case(257, 2e6, 'south', 'horizontal')):
        b = hr.build(c)
        cen = hr.centre_ecef(c.centre)
        c0 = -b.eq[0, 3] * b.eq[0, :3]
        dist = np.linalg.norm(c0 - cen)
        if c.facet0 == 'radial':
            assert abs(dist - c.rho) < 1e-6
        else:
            assert abs(np.linalg.norm(c0) - c.rho) < 1e-6 and dist > 6.0e6


def test_far_and_deep_points():
    c = hr.Case(257, 2e6, 'north', 'radial')
    assert len(hr.far_outside(c)) == 3 and len(hr.deep_inside(c)) == 3


@pytest.mark.parametrize('name', hr.QHULL_NAMES)
def test_qhull_cases_leave_no_point_out(name):
    q = hr.qhull_case(*hr.qhull_input(name))
    assert q.dropped == 0 and len(q.lat) == 8 * len(q.eq)
    if name == 'box':
        assert len(q.eq) == 12 and len(np.unique(q.group)) == 6
    else:
        assert len(np.unique(q.group)) == len(q.eq) and len(q.eq) > 32


@pytest.mark.parametrize('F', hr.F_LIST)
def test_hull_chords_against_the_longdouble_clip(F):
    """estimate.hull_chords on the ray set of F facets: the same NaN pattern as the longdouble clip, the ends that are 0 and 1 by
    construction exactly so, a clipped end within 64 eps (|a| + |b|) metres of the longdouble one (these rays meet their
    binding facet at a right angle: the bound on a plane distance is the bound on the end)."""
    from volumetricinterp_amd.estimate import hull_chords
    r = hr.ray_set(F)
    assert r.dropped == 0 and len(r.a) == (2 + 2 * len(hr.STEPS)) * F
    s0, s1 = hull_chords(r.eq, r.tol, r.a, r.b)
    ratio = hr.check_chords(r, s0, s1)
    print('F = %d: %d rays, largest |end - longdouble end| / (64 eps (|a| + |b|)) = %.3g' % (F, len(r.a), ratio))
