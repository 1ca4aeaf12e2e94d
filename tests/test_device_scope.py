"""The host idioms every evaluation entry shares, no GPU: _lib.DeviceScope (`with ctx.scope() as dev:` - the device temporaries of
one call, freed whatever happens) on a stub context that counts, estimate._check_out (the one statement of the `out=` check), and
the argument errors Estimate.evaluate_coeffs, track and slant raise through them before a device is asked for."""
import re

import numpy as np
import pytest

from conftest import load_golden


class StubArray(object):
    def __init__(self, log, fail_free=False):
        self.log, self.fail_free, self.frees = log, fail_free, 0
        log.append(self)

    def free(self):
        self.frees += 1
        if self.fail_free:
            raise RuntimeError('free failed')


class StubContext(object):
    """empty / to_device as the scope calls them; allocation number `fail_at` raises, array number `bad_free` cannot be freed."""

    def __init__(self, fail_at=None, bad_free=None):
        self.fail_at, self.bad_free, self.arrays, self.calls = fail_at, bad_free, [], []

    def _new(self, *call):
        if len(self.calls) == self.fail_at:
            raise MemoryError('allocation %d' % self.fail_at)
        self.calls.append(call)
        return StubArray(self.arrays, fail_free=len(self.arrays) == self.bad_free)

    def empty(self, shape, dtype=np.float64):
        return self._new('empty', shape, dtype)

    def to_device(self, host, dtype=None):
        return self._new('to_device', host, dtype)


def _scope(ctx):
    from volumetricinterp_amd import _lib
    dev = _lib.Context.scope(ctx)                   # what ctx.scope() is on a Context
    assert isinstance(dev, _lib.DeviceScope)
    return dev


def test_scope_frees_all_on_normal_exit_and_allocates_through_the_context():
    ctx = StubContext()
    host = np.arange(3.)
    with _scope(ctx) as dev:
        a, b, c, d = dev.up(host), dev.up(host, np.int32), dev.empty((2, 3)), dev.empty(5, np.uint8)
        assert [x.frees for x in ctx.arrays] == [0, 0, 0, 0]
    assert ctx.arrays == [a, b, c, d] and [x.frees for x in ctx.arrays] == [1, 1, 1, 1]
    assert ctx.calls == [('to_device', host, None), ('to_device', host, np.int32), ('empty', (2, 3), np.float64),
                         ('empty', 5, np.uint8)]


def test_scope_frees_all_when_the_body_raises_and_raises_the_same_exception():
    ctx = StubContext()
    boom = KeyError('the body')
    with pytest.raises(KeyError) as e:
        with _scope(ctx) as dev:
            dev.up([1.]), dev.empty(2), dev.empty(3)
            raise boom
    assert e.value is boom
    assert [x.frees for x in ctx.arrays] == [1, 1, 1]


def test_scope_frees_the_first_two_when_the_third_allocation_raises():
    ctx = StubContext(fail_at=2)
    with pytest.raises(MemoryError, match='allocation 2'):
        with _scope(ctx) as dev:
            dev.up([1.]), dev.empty(2)
            dev.empty(3)
            raise AssertionError('not reached')
    assert [x.frees for x in ctx.arrays] == [1, 1]


@pytest.mark.parametrize('fails', [False, True])
def test_a_detached_array_is_not_freed_while_the_others_are(fails):
    ctx = StubContext()
    try:
        with _scope(ctx) as dev:
            a, b, c = dev.empty(1), dev.empty(2), dev.up([3.])
            assert dev.detach(b) is b
            if fails:
                raise KeyError
    except KeyError:
        assert fails
    assert (a.frees, b.frees, c.frees) == (1, 0, 1)


def test_a_failing_free_does_not_keep_the_rest_from_being_freed():
    ctx = StubContext(bad_free=1)
    boom = KeyError('the body')
    with pytest.raises(KeyError) as e:              # the body's own exception is the one that propagates
        with _scope(ctx) as dev:
            dev.empty(1), dev.empty(2), dev.empty(3)
            raise boom
    assert e.value is boom and [x.frees for x in ctx.arrays] == [1, 1, 1]
    ctx = StubContext(bad_free=1)
    with pytest.raises(RuntimeError, match='free failed'):          # without one, the failure is not lost
        with _scope(ctx) as dev:
            dev.empty(1), dev.empty(2), dev.empty(3)
    assert [x.frees for x in ctx.arrays] == [1, 1, 1]


# ---- the out check ----------------------------------------------------------------------------------------------------------
def _bad_outs(shape, dtype=np.float64):
    """Bad `out` values for an entry that writes `dtype` of `shape` (2-D): a list, a wrong shape, a wrong dtype, a transposed -
    not C-contiguous - view of the right shape."""
    other = np.float32 if dtype == np.float64 else np.int64
    return [('list', np.zeros(shape, dtype).tolist()), ('shape', np.empty(shape[::-1], dtype)),
            ('dtype', np.empty(shape, other)), ('transposed', np.empty(shape[::-1], dtype).T)]


@pytest.mark.parametrize('dtype', [np.float64, np.int32])
def test_check_out(dtype):
    from volumetricinterp_amd.estimate import _check_out
    shape = (2, 3)
    for name, bad in _bad_outs(shape, dtype):
        assert np.shape(bad) == shape or name == 'shape'
        with pytest.raises(ValueError, match='out must be') as e:
            _check_out(bad, shape, dtype)
        assert str(e.value) == 'out must be a C-contiguous %s array of shape (2, 3)' % np.dtype(dtype).name, name
    good = np.empty(shape, dtype)
    assert _check_out(good, shape, dtype) is good
    new = _check_out(None, shape, dtype)
    assert new.shape == shape and new.dtype == dtype and new.flags.c_contiguous
    assert _check_out(None, shape).dtype == np.float64
    with pytest.raises(ValueError, match=r'float64 array of shape \(5\)$'):
        _check_out(np.empty(4), (5,))
    with pytest.raises(ValueError, match=r'float64 array of shape \(\)$'):
        _check_out(np.empty(1), ())


class NoDevice(object):
    """A context that must not be asked for anything."""

    def __getattr__(self, name):
        raise AssertionError('the device was asked for %r' % name)


def _estimate():
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_k8l2')
    return Estimate.from_arrays(f['Coeffs'], f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']), ctx=NoDevice())


LAT, LON, ALT = np.full((2, 3), 78.), np.full((2, 3), 262.), np.full((2, 3), 300e3)


def _entries(es):
    """Three entries that write a (2, 3) array."""
    t = float(np.mean(es.time[0]))
    return [('evaluate_coeffs', lambda out: es.evaluate_coeffs(es.Coeffs[:2], LAT[0], LON[0], ALT[0], out=out)),
            ('track', lambda out: es.track(t, LAT, LON, ALT, out=out)),
            ('slant', lambda out: es.slant(t, (LAT, LON, 0.), (LAT, LON, ALT), nodes=3, out=out))]


@pytest.mark.parametrize('name,bad', _bad_outs((2, 3)))
def test_the_entries_refuse_a_bad_out_alike_and_before_any_device_call(name, bad):
    es = _estimate()
    messages = []
    for entry, call in _entries(es):
        with pytest.raises(ValueError, match='out must be') as e:
            call(bad)
        messages.append(re.sub(r'\([^()]*\)$', '(shape)', str(e.value)))
    assert messages == ['out must be a C-contiguous float64 array of shape (shape)'] * 3


def test_the_times_shape_errors_keep_their_texts():
    es = _estimate()
    t = np.full(5, float(np.mean(es.time[0])))
    with pytest.raises(ValueError) as e:
        es.track(t, LAT, LON, ALT)
    assert str(e.value) == 'times must be one value or have the shape of gdlat'
    with pytest.raises(ValueError) as e:
        es.slant(t, (LAT, LON, 0.), (LAT, LON, ALT))
    assert str(e.value) == 'times must be one value or have the shape of the rays'
    with pytest.raises(ValueError) as e:            # the times are judged before `out`, as they were
        es.track(t, LAT, LON, ALT, out=np.empty(5))
    assert str(e.value) == 'times must be one value or have the shape of gdlat'
