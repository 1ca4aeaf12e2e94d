"""GPU tests of the ray-integrated basis of fixed rays (Estimate.resident_rays, ResidentRays, vi_eval_slant_basis_f64 - kernel K1l: a
wave per ray, K2l's clip, a lane per node, every basis function summed over the lanes through an LDS tile) and of what the
resident-grid products make of it.

The matrix is checked against a different route through code that has its own tests: the chords of estimate.hull_chords on the
host, the node positions in NumPy, geodesy.ecef2geodetic, Model.basis at the nodes (K1) and the weighted sum on the host,

  ref[n, p] = sum_i W[p, i] A[p, i, n],    W[p, i] = wq[i] (s1 - s0)_p / 2 |b - a|_p.

Gate, per entry: |Y - ref| <= 1e-10 * sum_i |W[p, i] A[p, i, n]| - 1e-10 is the project's gate for one quantity by two routes
(ORACLE_TOL of the track tests, TOL of the slant tests: the reference's nodes pass through a geodetic round trip of about 4e-9 m);
the scale is the entry's own absolute sum, so that no large basis function hides a small one.  Whole columns are NaN, and the NaN
pattern is the host's exactly; every parity case asserts that each hit ray's chord is longer than 1 m, which keeps that pattern
off the decision boundary of the clip.

The rays and records are those of tests/test_gpu_slant.py and tests/test_gpu_track.py, the covariances those of
tests/test_gpu_resident_error.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_resident_error as re_
import test_gpu_resident_geometry as geo
import test_gpu_track as tt
from test_gpu_slant import TOL, _chords, _gauss, _length, _nodes, _rays, _reference

pytestmark = pytest.mark.gpu

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS = np.uint64(0x7FF8000000000000)            # the NaN vi_eval_basis_f64 writes
P = 260


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _same_bits(x, y):
    return x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


def _estimate(tag, timeinterp=False):
    """The estimate of the track tests (40 records) with a covariance for get_C to select: ResidentRays.__call__ goes through it."""
    es = tt._estimate(tag, timeinterp)
    es.Covariance = np.zeros((tt.R, 1, 1))
    return es


def _hit_first(name, n):
    """(a, b): n rays of a set, (n, 3) ECEF each, a ray that enters the hull first - one ray is then a number."""
    _, _, a, b = _rays(name, P)
    first = int(np.flatnonzero(~np.isnan(_chords(a, b, True)[0]))[0])
    order = np.r_[first, np.delete(np.arange(P), first)][:n]
    return np.ascontiguousarray(a[order]), np.ascontiguousarray(b[order])


def _host_basis(es, a, b, x, wq, check_hull):
    """(ref, scale, s0, s1): the matrix by the other route, (N, rays), and the absolute sums; NaN columns for the rays that miss."""
    s0, s1 = _chords(a, b, check_hull)
    hit = ~np.isnan(s0)
    N = es.model.nbasis
    ref, scale = np.full((N, len(a)), np.nan), np.full((N, len(a)), np.nan)
    if hit.any():
        lat, lon, alt = _nodes(a[hit], b[hit], s0[hit], s1[hit], x)
        A = es.model.basis(lat.ravel(), lon.ravel(), alt.ravel()).reshape(lat.shape + (N,))
        W = wq[None, :] * ((s1 - s0)[hit] / 2. * _length(a, b)[hit])[:, None]
        WA = W[:, :, None] * A
        ref[:, hit] = WA.sum(axis=1).T
        scale[:, hit] = np.abs(WA).sum(axis=1).T
    return ref, scale, s0, s1


def _gate(Y, ref, scale, what):
    """The gate of the module's docstring on every entry; returns the worst ratio |Y - ref| / (TOL scale)."""
    assert Y.shape == ref.shape
    assert np.array_equal(np.isnan(Y), np.isnan(ref)), (what, np.flatnonzero(np.isnan(Y).any(axis=0) != np.isnan(ref).any(axis=0))[:10])
    dead = np.isnan(ref).any(axis=0)
    assert np.all(np.isnan(ref[:, dead]))                                   # whole columns
    ok = ~np.isnan(ref)
    worst = 0.
    if ok.any():
        err, bound = np.abs(Y[ok] - ref[ok]), TOL * scale[ok]
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = np.where(err == 0., 0., err / bound)
        worst = float(ratio.max())
        print('%s: worst |Y - ref| / (1e-10 sum |W A|) = %.3e on %d finite columns of %d' % (what, worst, (~dead).sum(), dead.size))
        assert np.all(err <= bound), (what, worst)
    return worst


def _check_chords(r, a, b, s0, s1):
    d0, d1 = r.chords
    hit = ~np.isnan(s0)
    assert np.array_equal(np.isnan(d0.ravel()), ~hit) and np.array_equal(np.isnan(d1.ravel()), ~hit)
    length = _length(a, b)
    assert np.allclose(d0.ravel()[hit], (s0 * length)[hit], rtol=0., atol=1e-3)
    assert np.allclose(d1.ravel()[hit], (s1 * length)[hit], rtol=0., atol=1e-3)


# ---- 1. matrix parity --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['vertical', 'gnss'])
@pytest.mark.parametrize('check_hull', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'default', 'scr_k12l2', 'rbf'])
def test_matrix_parity(tag, check_hull, name):
    """260 rays, 64 Gauss-Legendre nodes: default (6, 4), k8l2 (2, 8) and scr_k12l2 (2, 12) at the compiled caps (6, 4), (12, 8)
    and (24, 16) of the sphharmlag kernel, rbf on the RBF form; vertical rays through the box of the tests and receiver-to-GNSS
    rays, clipped by the hull and whole."""
    es = _estimate(tag)
    start, end, a, b = _rays(name, P)
    x, wq = _gauss()
    with es.resident_rays(start, end, check_hull=check_hull) as r:
        assert r.shape == (P,) and r.Q == P and r.dG is None and r.frame is None
        Y = r.basis()
        ref, scale, s0, s1 = _host_basis(es, a, b, x, wq, check_hull)
        hit = ~np.isnan(s0)
        assert hit.sum() >= 50 and (check_hull or hit.all())
        assert np.all(((s1 - s0) * _length(a, b))[hit] > 1.)                # off the decision boundary
        assert Y.shape == (es.model.nbasis, P)
        _gate(Y, ref, scale, '%s %s hull=%s' % (tag, name, check_hull))
        assert np.all(_bits(Y[:, ~hit]) == NAN_BITS)
        _check_chords(r, a, b, s0, s1)
        if not check_hull:
            d0, d1 = r.chords
            assert np.array_equal(d0, np.zeros(P)) and np.array_equal(d1, _length(a, b))


# ---- 2. product parity -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'default'])
def test_product_parity(tag, timeinterp):
    """r(times)[t] against Estimate.slant at times[t] on the same rays: three times spread over the records."""
    es = _estimate(tag, timeinterp)
    start, end, a, b = _rays('gnss', P)
    mt = tt._mid(es.time)
    t0 = [mt[3], mt[20], mt[37]] if not timeinterp else [mt[3] + 17.25, mt[20] + 30., mt[36] + 59.5]
    times = [tt._datetime(t) for t in t0]
    x, wq = _gauss()
    with es.resident_rays(start, end) as r:
        out = r(times)
    assert out.shape == (3, P)
    for k, t in enumerate(times):
        got = es.slant(t, start, end)
        assert np.array_equal(np.isnan(out[k]), np.isnan(got))
        _, scale, s0, _ = _reference(es, t0[k], a, b, x, wq, True)
        ok = ~np.isnan(s0)
        assert ok.sum() >= 50 and np.array_equal(ok, ~np.isnan(got))
        err = np.abs(out[k][ok] - got[ok]) / scale[ok]
        print('%s interp=%s time %d: max |resident - slant| / sum |W f| = %.2e' % (tag, timeinterp, k, err.max()))
        assert np.all(np.abs(out[k][ok] - got[ok]) <= TOL * scale[ok]), err.max()


# ---- the error gate (tests 3 and 7) ------------------------------------------------------------------------------------------

def _check_errors(out, Y, dC, what):
    """out = sqrt(b^T dC b) per column of Y (N, rays) against the host form on the device's own bits:
    |out^2 - form| <= 1e-10 sum_ik |Y_i dC_ik Y_k| - the N^2 roundings of fp64 are 2.3e-12 of that sum at N = 144; against the
    absolute sum because the form cancels.  NaN exactly for the dead columns and where the form is negative, wherever |form|
    exceeds the bound."""
    dead = np.isnan(Y[0])
    assert np.array_equal(dead, np.isnan(Y).any(axis=0))
    Yl = Y[:, ~dead]
    form = np.einsum('ip,ip->p', Yl, dC @ Yl)
    bound = 1e-10 * np.einsum('ip,ip->p', np.abs(Yl), np.abs(dC) @ np.abs(Yl))
    assert np.all(np.isnan(out[dead]))
    o = out[~dead]
    sure = np.abs(form) > bound
    assert np.array_equal(np.isnan(o[sure]), form[sure] < 0.), what
    fin = ~np.isnan(o)
    err = np.abs(o[fin] ** 2 - form[fin])
    if fin.any():
        print('%s: worst |out^2 - form| / (1e-10 sum |Y dC Y|) = %.3e on %d columns' % (what, (err / bound[fin]).max(), fin.sum()))
    assert np.all(err <= bound[fin]), what
    return fin.sum()


# ---- 3. ray counts -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _count_reference():
    f, es = re_._estimate('default')
    a, b = _hit_first('oblique', P)
    ref, scale, s0, s1 = _host_basis(es, a, b, *_gauss(), True)
    for v in (ref, scale, s0, s1):
        v.setflags(write=False)
    return a, b, ref, scale, s0, s1


@pytest.mark.parametrize('n', [1, 3, 4, 5, 255, 256, 257, 260])
def test_ray_counts(n):
    """The default order with the hull at ray counts about the boundary of a workgroup of four rays and about the conditions of
    the products (K2r: Q >= 256 and a multiple of 4, K2e: Q even; the library's products elsewhere): the matrix at the gate of
    test 1, the product against the host product of the device's own bits, the errors at the gate of test 7."""
    f, es = re_._estimate('default')
    a, b, ref, scale, s0, s1 = _count_reference()
    N = es.model.nbasis
    C = np.nan_to_num(f['Coeffs'])[np.arange(3) % len(f['Coeffs'])] * np.array([1., -0.5, 3.])[:, None]
    dC = f['Covariance'][np.arange(2) % len(f['Covariance'])]
    with es.resident_rays(a[:n].T, b[:n].T, coords='ecef') as r:
        Y = r.basis()
        assert Y.shape == (N, n)
        _gate(Y, ref[:, :n], scale[:, :n], 'P=%d' % n)
        _check_chords(r, a[:n], b[:n], s0[:n], s1[:n])
        out = r.evaluate_coeffs(C)
        err = r.evaluate_errors(dC)
    assert not np.isnan(Y[0, 0])
    live = ~np.isnan(Y[0])
    assert out.shape == (3, n) and np.array_equal(np.isnan(out), np.broadcast_to(~live, (3, n)))
    host = C @ Y[:, live]
    mag = np.abs(C) @ np.abs(Y[:, live])
    assert np.all(np.abs(out[:, live] - host) <= 2. * geo.gamma(N + 2) * mag)
    for t in range(2):
        _check_errors(err[t], Y, dC[t], 'P=%d covariance %d' % (n, t))


# ---- 4. node counts ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nodes', [1, 2, 63, 64, 65, 128, 129, 256, 'composite'])
@pytest.mark.parametrize('tag', ['k8l2', 'scr_k12l2'])
def test_node_counts(tag, nodes):
    """Node counts about the boundaries of a pass of 64 nodes (idle lanes in the last pass, up to four passes) and a caller's
    composite midpoint rule of 1000 nodes (16 passes), five rays with the hull."""
    es = _estimate(tag)
    a, b = _hit_first('oblique', 5)
    if nodes == 'composite':
        x, wq = (np.arange(1000) + 0.5) / 500. - 1., np.full(1000, 2. / 1000)
        kw = dict(rule=(x, wq))
    else:
        x, wq = _gauss(nodes)
        kw = dict(nodes=nodes)
    with es.resident_rays(a.T, b.T, coords='ecef', **kw) as r:
        Y = r.basis()
    ref, scale, s0, _ = _host_basis(es, a, b, x, wq, True)
    assert not np.isnan(s0[0])
    _gate(Y, ref, scale, '%s nodes=%s' % (tag, nodes))


# ---- 5. independence ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', ['k8l2', 'default', 'rbf'])
def test_columns_are_independent(tag):
    """A ray's column and chord have the same bits in a batch of 260 rays, in the shuffled batch and alone."""
    es = _estimate(tag)
    _, _, a, b = _rays('oblique', P)

    def run(a, b):
        with es.resident_rays(a.T, b.T, coords='ecef') as r:
            return (r.basis(),) + tuple(v[None, :] for v in r.chords)
    batch = run(a, b)
    live = ~np.isnan(batch[0][0])
    assert 50 <= live.sum() < P
    order = np.random.default_rng(15).permutation(P)
    for x, y in zip(run(a[order], b[order]), batch):
        assert _same_bits(x, y[:, order])
    for p in (int(np.flatnonzero(live)[7]), int(np.flatnonzero(~live)[0]), P - 1):
        for x, y in zip(run(a[p:p + 1], b[p:p + 1]), batch):
            assert _same_bits(x, y[:, p:p + 1])


# ---- 6. dead and degenerate rays ---------------------------------------------------------------------------------------------

def _odd_rays(es):
    """(a, b) in ECEF, five rays: one that hits, one that misses, a NaN and an inf end point, a segment of length zero inside."""
    from volumetricinterp_amd import geodesy
    _, _, a, b = _rays('oblique', P)
    hit = ~np.isnan(_chords(a, b, True)[0])
    i, j = int(np.flatnonzero(hit)[0]), int(np.flatnonzero(~hit)[0])
    inside = np.array(geodesy.geodetic2ecef(78., 262., 300e3))
    assert es.check_hull(78., 262., 300e3)
    a5 = np.array([a[i], a[j], a[i], a[i], inside])
    b5 = np.array([b[i], b[j], b[i], b[i], inside])
    a5[2, 1] = np.nan
    b5[3, 2] = np.inf
    return a5, b5


@pytest.mark.parametrize('tag', ['k8l2', 'default', 'rbf'])
def test_dead_and_degenerate_rays(tag):
    es = _estimate(tag)
    a, b = _odd_rays(es)
    times = [tt._datetime(tt._mid(es.time)[5])]
    with es.resident_rays(a.T, b.T, coords='ecef') as r:
        Y = r.basis()
        d0, d1 = r.chords
        out = r(times)
    assert np.isfinite(Y[:, 0]).all() and np.any(Y[:, 0] != 0.)
    assert np.all(_bits(Y[:, 1:4]) == NAN_BITS)                             # every row of a miss, a NaN and an inf end point
    assert np.all(np.isnan(d0[1:4])) and np.all(np.isnan(d1[1:4]))
    assert np.all(Y[:, 4] == 0.) and d0[4] == 0. and d1[4] == 0.            # a live column of zeros
    assert np.isfinite(out[0, 0]) and np.all(np.isnan(out[0, 1:4])) and out[0, 4] == 0.
    got = es.slant(times[0], a.T, b.T, coords='ecef')
    assert np.array_equal(np.isnan(got), np.isnan(out[0])) and got[4] == 0.
    _, scale, _, _ = _reference(es, tt._mid(es.time)[5], a[:1], b[:1], *_gauss(), True)
    assert abs(out[0, 0] - got[0]) <= TOL * scale[0]


def _live_case():
    """evaluate_coeffs of 260 oblique rays (a third of them dead) at the default order: K2r's shape."""
    f, es = re_._estimate('default')
    _, _, a, b = _rays('oblique', P)
    C = np.nan_to_num(f['Coeffs'])[np.arange(20) % len(f['Coeffs'])] * np.linspace(-2., 2., 20)[:, None]
    C[7] = np.nan
    with es.resident_rays(a.T, b.T, coords='ecef') as r:
        return r.evaluate_coeffs(C)


CHILD = '''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import test_gpu_resident_rays as rr
np.save(sys.argv[1], rr._live_case())
'''


def test_product_without_the_live_list_in_a_child_process(tmp_path):
    """VINTERP_K2R_LIVE=0 (read once per process: a fresh child) - K2r's plain loop over every piece, which relies on the NaN of
    ALL rows of a dead column - gives the bits of the live list, which reads row 0."""
    assert os.environ.get('VINTERP_K2R_LIVE') != '0' and os.environ.get('VINTERP_EVAL_RESIDENT') != 'blas'
    own = _live_case()
    dead = np.isnan(own[0])
    assert 0 < dead.sum() < P and np.all(np.isnan(own[7])) and np.isfinite(own[0, ~dead]).all()
    script = tmp_path / 'child.py'
    script.write_text(CHILD % (REPO_ROOT, os.path.join(REPO_ROOT, 'tests')))
    env = dict(os.environ)
    for k in ('VINTERP_EVAL_RESIDENT', 'VINTERP_K2R_GROUPS'):
        env.pop(k, None)
    env['VINTERP_K2R_LIVE'] = '0'
    o = str(tmp_path / 'plain.npy')
    res = subprocess.run([sys.executable, str(script), o], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, 'VINTERP_K2R_LIVE=0 child: exit %d\n%s\n%s' % (res.returncode, res.stdout[-3000:], res.stderr[-3000:])
    plain = np.load(o)
    assert np.array_equal(np.isnan(plain), np.isnan(own))
    assert _same_bits(plain[~np.isnan(own)], own[~np.isnan(own)])


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', ['k8l2', 'default'])
def test_errors(tag):
    """Standard errors of the line integrals, 260 oblique rays: r.error([t]) against the host form on the device's own bits."""
    f, es = re_._estimate(tag)
    _, _, a, b = _rays('oblique', P)
    t = re_._t_mid(f)
    dC = np.asarray(es.get_C(t)[1], dtype=np.float64)
    with es.resident_rays(a.T, b.T, coords='ecef') as r:
        out = r.error([t])
        Y = r.basis()
    assert out.shape == (1, P)
    dead = np.isnan(Y[0])
    assert 50 <= (~dead).sum() < P
    assert _check_errors(out[0], Y, dC, tag) >= 50


def test_errors_time_interpolation():
    """timeinterp=True: the covariance is get_C's blend of two records."""
    from conftest import load_golden
    f, es = re_._estimate('default', timeinterp=True)
    _, _, a, b = _rays('oblique', P)
    t = tt.EPOCH + tt.dt.timedelta(seconds=float(load_golden('eval')['default_t_int']))
    dC = np.asarray(es.get_C(t)[1], dtype=np.float64)
    assert not any(np.array_equal(dC, c) for c in f['Covariance'])          # a blend, not a record
    with es.resident_rays(a.T, b.T, coords='ecef') as r:
        out = r.error([t])
        Y = r.basis()
    assert _check_errors(out[0], Y, dC, 'default interp') >= 50


# ---- 8. inherited maps -------------------------------------------------------------------------------------------------------

def test_inherited_maps():
    """Rays of shape (8, 64): peak and integrate along the last axis (K2p's and K2r's shapes) and along the first."""
    es = _estimate('default')
    rng = np.random.default_rng(8)
    start = (rng.uniform(75, 81, (8, 1)), rng.uniform(250, 274, (8, 1)), 0.)
    end = (rng.uniform(72, 84, (8, 64)), rng.uniform(240, 284, (8, 64)), 1000e3)
    mt = tt._mid(es.time)
    times = [tt._datetime(mt[k]) for k in (2, 11, 30)]
    N = es.model.nbasis
    with es.resident_rays(start, end) as r:
        assert r.shape == (8, 64)
        dens = r(times)
        assert dens.shape == (3, 8, 64)
        dead = np.isnan(dens[0])
        assert 0 < dead.sum() < dead.size
        Y = r.basis()
        for axis in (-1, 0):
            val, idx = r.peak(times, axis=axis)
            tot = r.integrate(times, axis=axis)
            ax = axis % 2 + 1
            none = np.all(np.isnan(dens), axis=ax)
            assert val.shape == none.shape and idx.shape == none.shape and tot.shape == none.shape
            assert np.array_equal(np.isnan(val), none) and np.array_equal(idx == -1, none) and np.array_equal(np.isnan(tot), none)
            filled = np.where(np.isnan(dens), -np.inf, dens)
            assert _same_bits(val[~none], filled.max(axis=ax)[~none])
            assert np.array_equal(idx[~none], filled.argmax(axis=ax)[~none])
            # the gate of tests/test_gpu_resident_integrate.py: gamma_{N + L + 2} of the sum of the magnitudes, once for the
            # reduced basis and once for the host's sum of the densities
            C = np.array([es.get_C(t)[0] for t in times])
            mag = np.where(np.isnan(Y[0])[None], 0., np.einsum('tn,n...->t...', np.abs(C), np.abs(np.nan_to_num(Y)))).sum(axis=ax)
            ref = np.where(np.isnan(dens), 0., dens).sum(axis=ax)
            L = dens.shape[ax]
            assert np.all(np.abs(tot - ref)[~none] <= 2. * geo.gamma(N + L + 2) * mag[~none])
        with pytest.raises(ValueError, match='holds no gradient basis'):
            r.gradient(times)
        with pytest.raises(ValueError, match='holds no gradient basis'):
            r.evaluate_gradients(np.zeros((1, N)))


# ---- 9. the C entry itself and the life of the object --------------------------------------------------------------------------

def _raw(es, a, b, eq, tol, rule=None, chord=True, null_out=False):
    """vi_eval_slant_basis_f64 on (P, 3) end points with the facet equations eq (None: F = 0): (rc, Y (N, P), chord or None)."""
    from volumetricinterp_amd import _lib
    ctx = es.model.ctx
    x, wq = _gauss() if rule is None else rule
    n, N = len(a), es.model.nbasis
    bufs = []
    try:
        up = lambda v, dtype=np.float64: bufs.append(ctx.to_device(np.ascontiguousarray(v), dtype)) or bufs[-1]
        da, db = up(a.T if n else np.zeros((3, 1))), up(b.T if n else np.zeros((3, 1)))
        dh = up(eq) if eq is not None else None
        dx, dq = up(x), up(wq)
        dY = up(np.full((N, max(n, 1)), 7.))
        dS = up(np.full((2, max(n, 1)), 7.)) if chord else None
        ptr = lambda d: d.ptr if d is not None else None
        rc = _lib.lib.vi_eval_slant_basis_f64(es.model.handle(), n, da.ptr, db.ptr, ptr(dh), 0 if eq is None else eq.shape[0], tol,
                                              len(x), dx.ptr, dq.ptr, None if null_out else dY.ptr, ptr(dS))
        ctx.sync()
        return rc, dY.download(), (dS.download() if chord else None)
    finally:
        for v in bufs:
            v.free()


@pytest.mark.parametrize('tag', ['k8l2', 'default', 'rbf'])
def test_raw_abi(tag):
    from volumetricinterp_amd import _lib
    es = _estimate(tag)
    eq, tol = es._hull()
    _, _, a, b = _rays('oblique', P)
    rc, Y, chord = _raw(es, a, b, eq, tol)
    assert rc == 0
    dead = np.isnan(chord[0])
    assert 0 < dead.sum() < P and np.array_equal(np.isnan(Y), np.broadcast_to(dead, Y.shape))
    # d_chord = NULL
    rc, Yn, none = _raw(es, a, b, eq, tol, chord=False)
    assert rc == 0 and none is None and _same_bits(Yn, Y)
    # F = 0: every ray whole
    rc, Yw, cw = _raw(es, a, b, None, 0.)
    assert rc == 0 and np.isfinite(Yw).all() and np.all(cw[0] == 0.) and np.all(cw[1] == 1.)
    # P = 0: VI_OK, nothing written
    rc, Y0, c0 = _raw(es, a[:0], b[:0], eq, tol)
    assert rc == 0 and np.all(Y0 == 7.) and np.all(c0 == 7.)
    # a null d_Y
    rc, Yx, _ = _raw(es, a, b, eq, tol, null_out=True)
    assert rc == -1 and np.all(Yx == 7.)                                    # VI_ERR_INVALID
    assert 'null argument' in _lib.lib.vi_last_error().decode()
    # two different P in a row on one handle against fresh models
    for n in (7, 133):
        rc, Yn, cn = _raw(es, a[:n], b[:n], eq, tol)
        rcf, Yf, cf = _raw(_estimate(tag), a[:n], b[:n], eq, tol)
        assert rc == 0 and rcf == 0 and _same_bits(Yn, Yf) and _same_bits(cn, cf) and _same_bits(Yn, Y[:, :n])


def test_close_and_use_after_close():
    es = _estimate('k8l2')
    _, _, a, b = _rays('oblique', 8)
    r = es.resident_rays(a.T, b.T, coords='ecef')
    assert r.basis().shape == (es.model.nbasis, 8)
    r.close()
    r.close()
    chords = r.chords                                                       # host data: kept
    assert chords[0].shape == (8,)
    for call in (lambda: r.basis(), lambda: r.evaluate_coeffs(es.Coeffs[:2]), lambda: r([tt._datetime(tt._mid(es.time)[0])]),
                 lambda: r.evaluate_errors(np.zeros((1, 32, 32))), lambda: r.evaluate_peaks(es.Coeffs[:2]),
                 lambda: r.evaluate_integrals(es.Coeffs[:2])):
        with pytest.raises(ValueError, match='has been closed'):
            call()
    # no ray: nothing to compute
    with es.resident_rays((np.zeros((0, 3)), 262., 0.), (80., 262., 1e6)) as r0:
        assert r0.shape == (0, 3) and r0.basis().shape == (es.model.nbasis, 0, 3) and r0(
            [tt._datetime(tt._mid(es.time)[0])]).shape == (1, 0, 3)
        assert r0.chords[0].shape == (0, 3)
