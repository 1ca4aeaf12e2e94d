"""The host side of Estimate.resident_rays (the ray-integrated basis of fixed rays), no GPU: its argument errors are those of
Estimate.slant, raised by the helper both share (estimate.slant_rays) before a device is asked for - and slant still raises them."""
import numpy as np
import pytest

from conftest import load_golden


def _estimate():
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_k8l2')
    return Estimate.from_arrays(f['Coeffs'], f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))


A, B = (78., 262., 0.), (78., 262., 1000e3)
BAD = [('coords must be', dict(coords='enu')),
       ('nodes must be', dict(nodes=0)), ('nodes must be', dict(nodes=257)), ('nodes must be', dict(nodes=2.5)),
       ('nodes must be', dict(nodes=True)), ('nodes must be', dict(nodes=None)),
       ('rule must be a pair', dict(rule=([0., 1.], [1.]))), ('rule must be a pair', dict(rule=([], []))),
       ('rule must be a pair', dict(rule=3.)), ('rule must be a pair', dict(rule=(np.zeros(65537), np.zeros(65537)))),
       ('rule must be finite', dict(rule=([np.nan], [2.]))), ('rule must be finite', dict(rule=([0.], [np.inf]))),
       ('do not broadcast', dict(start=(np.zeros(3), 262., 0.), end=(np.zeros(4), 262., 1e6))),
       ('triple', dict(start=(78., 262.))), ('triple', dict(start=78.)), ('triple', dict(start=None)), ('triple', dict(end=(1., 2., 3., 4.)))]


def _message(call, kw):
    args = dict(start=A, end=B)
    args.update(kw)
    with pytest.raises(ValueError) as e:
        call(**args)
    return str(e.value)


@pytest.mark.parametrize('match,kw', BAD)
def test_resident_rays_and_slant_raise_the_same_argument_errors(match, kw):
    """Bad coords, a bad triple, ends that do not broadcast, nodes out of range, a malformed and a non-finite rule: one message,
    from both entries, and no device needed (Estimate.from_arrays builds without one)."""
    es = _estimate()
    t = float(np.mean(es.time[0]))
    rays = _message(es.resident_rays, kw)
    slant = _message(lambda **k: es.slant(t, **k), kw)
    assert match in rays and rays == slant


def test_the_first_error_is_the_same_one():
    """Several bad arguments at once: both entries report coords first, then the rule, then the triple."""
    es = _estimate()
    t = float(np.mean(es.time[0]))
    for kw, match in ((dict(coords='enu', nodes=0, start=None), 'coords must be'), (dict(nodes=0, start=None), 'nodes must be'),
                      (dict(rule=([np.nan], [1.]), start=(1., 2.)), 'rule must be finite')):
        assert match in _message(es.resident_rays, kw)
        assert match in _message(lambda **k: es.slant(t, **k), kw)


def test_slant_rays_shapes():
    from volumetricinterp_amd import geodesy
    from volumetricinterp_amd.estimate import slant_rays
    end = (np.full((4, 5), 80.), np.linspace(250., 270., 5), 1000e3)
    x, w, shape, a, b = slant_rays(A, end, nodes=3)
    assert shape == (4, 5) and a.shape == (3, 20) and b.shape == (3, 20) and x.shape == (3,) and w.shape == (3,)
    assert a.flags.c_contiguous and b.flags.c_contiguous and a.dtype == np.float64
    assert np.array_equal(a, np.repeat(np.array(geodesy.geodetic2ecef(*A))[:, None], 20, axis=1))
    assert np.array_equal(b, np.array(geodesy.geodetic2ecef(*(np.broadcast_to(v, (4, 5)).ravel() for v in end))))
    _, _, shape, a2, b2 = slant_rays(a.reshape(3, 4, 5), b.reshape(3, 4, 5), coords='ecef')
    assert shape == (4, 5) and np.array_equal(a2, a) and np.array_equal(b2, b)
    _, _, shape, a0, b0 = slant_rays((np.zeros((0, 2)), 262., 0.), B)
    assert shape == (0, 2) and a0.shape == (3, 0) and b0.shape == (3, 0)
