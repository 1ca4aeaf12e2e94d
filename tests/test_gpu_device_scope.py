"""A failed call leaves the device as it found it: every evaluation entry that keeps its device temporaries in a scope
(_lib.DeviceScope) is run with each of its allocations failing in turn - Context.empty and Context.to_device wrapped on the context
instance so that allocation number k of the call raises a host MemoryError; no kernel is touched - and after each failure the free
device memory is, to the byte, what it was before the call (the check of test_unsupported_model_frees_everything, at every
site).  Fixture k8l2 (N = 32) on synth.query_grid(4) (64 points), 8 rays of 3 nodes, 3 records."""
import contextlib
import datetime as dt

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


class Allocations(object):
    """Counts the allocations made through a context while it is `wrapped`; number `fail_at` raises instead."""

    def __init__(self, ctx, fail_at=None):
        self.ctx, self.fail_at, self.count = ctx, fail_at, 0

    def _wrap(self, name):
        inner = getattr(self.ctx, name)

        def counted(*args, **kw):
            k = self.count
            self.count += 1
            if k == self.fail_at:
                raise MemoryError('injected')
            return inner(*args, **kw)
        return counted

    @contextlib.contextmanager
    def wrapped(self):
        for name in ('empty', 'to_device'):
            setattr(self.ctx, name, self._wrap(name))       # on the instance: the scope looks them up there at call time
        try:
            yield self
        finally:
            for name in ('empty', 'to_device'):
                delattr(self.ctx, name)


def _bits(r):
    return [np.ascontiguousarray(a).view(np.uint8).tobytes() for a in (r if isinstance(r, tuple) else (r,))]


def _fail_every_allocation(ctx, call):
    """call() once as it is - the code objects, the model tables and the context's work space exist from here on - then with each
    of its allocations failing in turn, then as it is again: the same bits."""
    with Allocations(ctx).wrapped() as counted:
        first = _bits(call())
    n = counted.count
    assert n >= 2, n
    for k in range(n):
        before = ctx.mem_info()[0]
        with Allocations(ctx, fail_at=k).wrapped() as a:
            with pytest.raises(MemoryError, match='injected'):
                call()
        assert a.count == k + 1
        assert ctx.mem_info()[0] == before, (k, n)
    assert _bits(call()) == first
    return n


def _estimates():
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_k8l2')
    args = (np.nan_to_num(f['Coeffs']), f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))
    return f, Estimate.from_arrays(*args), Estimate.from_arrays(*args, timeinterp=True)


def test_a_failed_estimate_call_frees_everything():
    from volumetricinterp_amd import synth
    f, es, esi = _estimates()
    ctx = es.model.ctx
    assert esi.model.ctx is ctx
    grid = synth.query_grid(4)
    mt = np.mean(f['utime'], axis=1)
    t = dt.datetime(1970, 1, 1) + dt.timedelta(seconds=float(mt[0]))
    times = np.resize(mt[:3], 64).reshape(4, 4, 4)                       # 3 records, every point at one of them
    between = np.linspace(mt[0], mt[2], 64, endpoint=False).reshape(4, 4, 4)
    lat = np.linspace(76., 80., 8)
    rays = dict(start=(lat, 262., 0.), end=(lat, 266., 1000e3), nodes=3)
    counts = {
        'gradient': _fail_every_allocation(ctx, lambda: es.gradient(t, *grid)),
        'error': _fail_every_allocation(ctx, lambda: es.error(t, *grid)),
        'track': _fail_every_allocation(ctx, lambda: es.track(times, *grid)),
        'track, timeinterp': _fail_every_allocation(ctx, lambda: esi.track(between, *grid)),
        'slant': _fail_every_allocation(ctx, lambda: es.slant(np.resize(mt[:3], 8), chord=True, **rays)),
    }

    def grid_maps():
        with es.resident_grid(*grid, gradient='model') as g:
            return g.evaluate_coeffs(es.Coeffs[:3]), g.evaluate_gradients(es.Coeffs[:3])

    def ray_maps():
        with es.resident_rays(**rays) as r:
            return (r.evaluate_coeffs(es.Coeffs[:3]),) + r.chords
    counts['resident_grid'] = _fail_every_allocation(ctx, grid_maps)
    counts['resident_rays'] = _fail_every_allocation(ctx, ray_maps)
    print(counts)
    # lat, lon, alt, the matrix, the output; + rec, Coeffs, hull (+ w); a, b, rec, Coeffs, hull, x, w, out, chords;
    # dY, dG, hull, lat, lon, alt + 2 x (C, out); dY, hull, a, b, x, w, chords + (C, out)
    assert counts == {'gradient': 5, 'error': 5, 'track': 7, 'track, timeinterp': 8, 'slant': 9, 'resident_grid': 10,
                      'resident_rays': 9}


def test_a_failed_call_on_a_live_grid_frees_everything():
    from volumetricinterp_amd import synth
    f, es, _ = _estimates()
    ctx = es.model.ctx
    C, dC = es.Coeffs[:3], es.Covariance[:3]
    w = np.linspace(1., 2., 4)

    def integrals():
        """Fresh weights at every call: the reduced basis a call builds is the grid's and outlives a product that fails after it,
        so it is given back here - every call builds it anew, and the free memory of before and after compares."""
        try:
            return g.evaluate_integrals(C, weights=w)
        finally:
            while g._reduced:
                g._reduced.popitem()[1].free()
    with es.resident_grid(*synth.query_grid(4)) as g:
        counts = {'evaluate_coeffs': _fail_every_allocation(ctx, lambda: g.evaluate_coeffs(C)),
                  'evaluate_errors': _fail_every_allocation(ctx, lambda: g.evaluate_errors(dC)),
                  'evaluate_peaks': _fail_every_allocation(ctx, lambda: g.evaluate_peaks(C)),
                  'evaluate_integrals': _fail_every_allocation(ctx, integrals)}
        print(counts)
        # the input and the output; + the index map and the work space; the reduced basis and the weights + (C, out)
        assert counts == {'evaluate_coeffs': 2, 'evaluate_errors': 2, 'evaluate_peaks': 4, 'evaluate_integrals': 4}


def test_a_failed_model_call_frees_everything():
    from volumetricinterp_amd import synth
    f, es, _ = _estimates()
    m = es.model
    lat, lon, alt = (a.ravel() for a in synth.query_grid(4))
    counts = {'basis': _fail_every_allocation(m.ctx, lambda: m.basis(lat, lon, alt)),
              'transform_coord': _fail_every_allocation(m.ctx, lambda: m.transform_coord(lat, lon, alt)),
              'grad_basis': _fail_every_allocation(m.ctx, lambda: m.grad_basis(lat, lon, alt))}
    print(counts)
    assert counts == {'basis': 4, 'transform_coord': 6, 'grad_basis': 4}


def test_the_unsupported_gradient_frees_everything_on_the_small_grid():
    """The library's own refusal (the radial-basis model has no gradient basis) in place of an injected failure."""
    from volumetricinterp_amd import _lib, synth
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_rbf')
    es = Estimate.from_arrays(f['Coeffs'], f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))
    grid = synth.query_grid(4)
    es.resident_grid(*grid).close()
    ctx = es.model.ctx
    before = ctx.mem_info()[0]
    with pytest.raises(_lib.VinterpError, match='only the sphharmlag model'):
        es.resident_grid(*grid, gradient='model')
    assert ctx.mem_info()[0] == before
