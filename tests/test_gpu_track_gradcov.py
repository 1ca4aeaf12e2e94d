"""GPU tests of the gradient covariances with one covariance per point: vi_eval_records_gradcov_f64 (kernel K2tc: K2c's body
with the covariance chosen per run of points; the library's product run by run for N > 144 and VINTERP_EVAL_RESIDENT=blas),
vi_eval_track_grad_cov_f64 and Estimate.track_gradient_covariance / track_gradient_error.

  U_r(q)[k] = entry GRADCOV_PAIRS[k] of g_c^T 1/2 (dC_r + dC_r^T) g_d at point q
  nearest: out[k, q] = U_rec[q](q)[k]        blend: out[k, q] = (1 - w[q]) U_rec[q](q)[k] + w[q] U_(rec[q]+1)(q)[k]

The reference never computes this quantity (its graderr code is dead); the yardsticks are exact arithmetic on the host and
the merged K2c.

1. integer G and dC small enough that forms, half-sums and blends with w in {0, 1/4, 1/2, 1} are exact (asserted on the host):
   NumPy's bits, sentinels around the output unchanged; every N and record pattern of tests/test_track_gradcov_host.py, both
   modes, once more with three blocks per workgroup.
2. nearest mode on real gradient bases with the fits' own covariances: bit for bit vi_eval_resident_gradcov_f64 (K2c) on the
   same device basis with the covariance of the point's record.
3. blend mode on the same data against error-free products and exact summation, within
   gamma_{2N+8} 1/2 sum ((1 - w)(|g_c| |dC_r| |g_d| + |g_d| |dC_r| |g_c|) + w (... dC_(r+1) ...)): the bound of the gradcov
   suite with the roundings of the blend (1 - w, two products, one sum) added; w = 0, w = 1, random w; the bound rejects one
   triangle of dC used for both.
4. missing and NaN records.  5. permutation.  6. the library routes.  7. the Python API."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_track as tt
import test_gpu_track_error as te
from test_gpu_resident_geometry import GUARD, SENTINEL, _handle, fsum2, gamma, mismatch, two_prod, two_sum
from test_gpu_resident_gradcov import PAIRS, gradcov_reference, host_gradcov
from test_track_gradcov_host import K2TC_NS, LIB_N, RAW_R, k2tc_geometry, patterns

pytestmark = pytest.mark.gpu

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QMAX = max(r.size for r in patterns().values())
WEIGHTS = np.array([0.0, 0.25, 0.5, 1.0])


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _same_bits(x, y):
    return x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


def _ptr(a):
    return None if a is None else a.ptr


def raw(h, ctx, G, rec, w, dC, resident=False):
    """vi_eval_records_gradcov_f64 on device copies of G (N, 3, Q), the (6, Q) output between GUARD sentinel doubles on either
    side.  Returns (out, whether every sentinel is unchanged) and, with `resident`, E (R, 6, Q) of
    vi_eval_resident_gradcov_f64 on the same device basis."""
    from volumetricinterp_amd import _lib
    N, _, Q = G.shape
    R = len(dC)
    with ctx.scope() as dev:
        dG = dev.up(np.ascontiguousarray(G, dtype=np.float64))
        dr = dev.up(np.ascontiguousarray(rec), np.int32)
        dw = None if w is None else dev.up(np.ascontiguousarray(w, dtype=np.float64))
        dD = dev.up(np.ascontiguousarray(dC, dtype=np.float64)) if R else None
        dO = dev.up(np.full(2 * GUARD + 6 * Q, SENTINEL))
        _lib.check(_lib.lib.vi_eval_records_gradcov_f64(h, Q, dG.ptr, dr.ptr, _ptr(dw), R, _ptr(dD), dO.offset_ptr(GUARD)),
                   'vi_eval_records_gradcov_f64')
        res = dO.download()
        E = None
        if resident:
            dE = dev.empty((R, 6, Q))
            _lib.check(_lib.lib.vi_eval_resident_gradcov_f64(h, Q, R, dG.ptr, dD.ptr, dE.ptr), 'vi_eval_resident_gradcov_f64')
            E = dE.download()
    sb = np.array([SENTINEL]).view(np.uint64)[0]
    b = res.view(np.uint64)
    guards = bool(np.all(b[:GUARD] == sb) and np.all(b[GUARD + 6 * Q:] == sb))
    out = res[GUARD:GUARD + 6 * Q].reshape(6, Q)
    return (out, guards, E) if resident else (out, guards)


# ==== 1. exact by construction ===============================================================================================
_INT = {}


def integer_stack(N):
    """(dC (RAW_R, N, N), G (N, 3, QMAX), U (RAW_R, 6, QMAX)) as integer_inputs of tests/test_gpu_resident_gradcov.py: |g|,
    |dC| <= 2^e with N^2 2^(3e + 1) <= 2^46, so every form is an integer below 2^45 in any order of summation and every packed
    entry a multiple of 1/2 below 2^46.  Covariances by r % 5: diagonally dominant asymmetric, its negation (negative diagonal
    entries), antisymmetric (everything exactly 0), random signs (not symmetric), a larger skew part."""
    if N not in _INT:
        rng = np.random.default_rng(2000 + N)
        e = int((45 - 2 * np.log2(N)) // 3)
        G = rng.integers(-2 ** e, 2 ** e + 1, (N, 3, QMAX)).astype(np.float64)
        dC = np.empty((RAW_R, N, N))
        for r in range(RAW_R):
            k = r % 5
            if k in (0, 1, 4):
                A = rng.integers(-2 ** (e - 3), 2 ** (e - 3) + 1, (N, N)).astype(np.float64)
                if k == 4:
                    A += np.triu(rng.integers(-2 ** (e - 3), 2 ** (e - 3) + 1, (N, N)), 1)
                A[np.diag_indices(N)] = rng.integers(2 ** (e - 1), 2 ** e + 1, N)
                dC[r] = -A if k == 1 else A
            elif k == 2:
                A = np.triu(rng.integers(-2 ** (e - 1), 2 ** (e - 1) + 1, (N, N)), 1).astype(np.float64)
                dC[r] = A - A.T
            else:
                dC[r] = rng.integers(-2 ** (e - 1), 2 ** (e - 1) + 1, (N, N))
        U = np.array([host_gradcov(G, d) for d in dC])
        assert np.all(2 * U == np.rint(2 * U)) and np.abs(U).max() < 2.0 ** 46
        assert not np.array_equal(dC[3], dC[3].T) and np.array_equal(dC[2], -dC[2].T) and not U[2].any()
        for a in (dC, G, U):
            a.setflags(write=False)
        _INT[N] = (dC, G, U)
    return _INT[N]


def exact_expected(U, rec, w):
    """The exact result of the pattern on the first rec.size points.  Blend: 8 times the value in 64-bit integers, (4 - 4 w)
    (2 U_r) + (4 w)(2 U_(r+1)), below 2^50 - asserted equal to what float64 gives for (1 - w) U_r + w U_(r+1), whose two
    products and sum are therefore exact, fused or not."""
    Q = rec.size
    q = np.arange(Q)
    a = U[rec, :, q].T
    if w is None:
        return a.copy()
    b = U[rec + 1, :, q].T
    w4 = np.rint(4 * w).astype(np.int64)
    assert np.array_equal(w4 / 4.0, w) and set(w4) <= {0, 1, 2, 4}
    v8 = (4 - w4) * np.rint(2 * a).astype(np.int64) + w4 * np.rint(2 * b).astype(np.int64)
    assert np.abs(v8).max() < 2 ** 50
    out = (1.0 - w) * a + w * b
    assert np.array_equal(out, v8 / 8.0)
    return out


def exact_suite(N, interp, tag=''):
    """Failures of every pattern at order N in one mode: NumPy's bits with the NaN columns of two masked points, untouched
    sentinels, exact zeros from the antisymmetric covariance."""
    from volumetricinterp_amd import _lib
    fails = []
    dC, G, U = integer_stack(N)
    h, ctx = _handle(N), _lib.get_context()
    for name, rec in sorted(patterns().items()):
        Q = rec.size
        what = 'K2tc N %d NB %d %s %s%s' % (N, -(-N // 16), name, 'blend' if interp else 'nearest', tag)
        w = WEIGHTS[(5 * np.arange(Q) + Q) % 7 % 4] if interp else None
        g = G[:, :, :Q].copy()
        ref = exact_expected(U, rec, w)
        if Q >= 4:
            for q in (1, Q - 2):
                g[:, :, q] = np.nan
                ref[:, q] = np.nan
        out, guards = raw(h, ctx, g, rec, w, dC)
        if not guards:
            fails.append(what + ': a store outside the output')
        m = mismatch(out, ref, what)
        if m:
            fails.append(m)
        if not interp and name == 'runs' and out[:, 0].any():
            fails.append(what + ': the antisymmetric covariance of the first run does not give exact zeros')
    return fails


def _report(fails):
    for f in fails:
        print('FAIL ' + f)
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('interp', [False, True])
@pytest.mark.parametrize('N', K2TC_NS)
def test_exact_at_every_order_and_pattern(N, interp, monkeypatch):
    monkeypatch.delenv('VINTERP_K2TC_GROUPS', raising=False)
    assert k2tc_geometry(N, QMAX)['path'] == 'kernel'
    _report(exact_suite(N, interp))


@pytest.mark.parametrize('interp', [False, True])
@pytest.mark.parametrize('N', [27, 144])
def test_exact_with_three_blocks_per_workgroup(N, interp, monkeypatch):
    """VINTERP_K2TC_GROUPS=3 (read at every launch): runs that go on across a block border inside a workgroup are not staged
    again, in blend mode the staged record's pass goes first; workgroups whose last blocks are empty."""
    monkeypatch.setenv('VINTERP_K2TC_GROUPS', '3')
    _report(exact_suite(N, interp, ' [groups 3]'))


# ==== 2. K2c's bits, 3. the blend against an exact reference =================================================================
REAL_TAGS = {'k8l2': 32, 'scr_k12l2': 48, 'default': 144}
REAL_Q = 600


@functools.lru_cache(maxsize=None)
def real_case(tag):
    """(es, G (N, 3, REAL_Q) as the device built it, dC, rec): 600 points of the box with the hull's NaN columns, in the model
    frame; dC the 12 records the track-error suite synthesises from the fit's own finite covariances (each once as it is, then
    scaled by powers of 4); rec sorted on the first 400 points, random after."""
    es = te._estimate(tag, 12)
    dC = te._records(tag, 12)[1]
    with es.resident_grid(*te._box(REAL_Q, seed=41), check_hull=True, gradient='model') as g:
        G = g.dG.download()
    assert G.shape == (REAL_TAGS[tag], 3, REAL_Q) and 0 < np.isnan(G[0, 0]).sum() < REAL_Q
    rng = np.random.default_rng(REAL_TAGS[tag])
    rec = rng.integers(0, len(dC) - 1, REAL_Q).astype(np.int32)
    rec[:400] = np.sort(rec[:400])
    for a in (G, rec):
        a.setflags(write=False)
    return es, G, dC, rec


@pytest.mark.parametrize('tag', sorted(REAL_TAGS))
def test_nearest_mode_has_k2c_bits(tag):
    es, G, dC, rec = real_case(tag)
    out, guards, E = raw(es.model.handle(), es.model.ctx, G, rec, None, dC, resident=True)
    assert guards
    want = E[rec, :, np.arange(REAL_Q)].T
    live = ~np.isnan(G[0, 0])
    assert np.array_equal(np.isnan(out), np.broadcast_to(~live, out.shape)) and np.isfinite(want[:, live]).all()
    assert not mismatch(out, want, '%s against K2c' % tag)
    assert np.abs(out[:, live]).max() > 0


@functools.lru_cache(maxsize=None)
def blend_references(tag):
    """Samples (q, pair k) of real_case(tag) at live points and, for the records r = rec[q] and r + 1 and for one triangle of
    dC mirrored, the exact forms as hi + lo with the bound's sums (gradcov_reference)."""
    es, G, dC, rec = real_case(tag)
    rng = np.random.default_rng(7)
    pool = np.nonzero(np.isfinite(G).all(axis=(0, 1)))[0]
    n = 96
    qs = pool[rng.integers(0, len(pool), n)]
    ks = np.concatenate([rng.integers(0, 6, n - 12), np.tile(np.arange(6), 2)])
    r0 = rec[qs].astype(np.int64)
    tri = np.array([np.triu(d) + np.triu(d, 1).T for d in dC])
    return qs, ks, [gradcov_reference(dC, G, r0 + i, qs, ks) for i in (0, 1)], [gradcov_reference(tri, G, r0 + i, qs, ks)[0]
                                                                               for i in (0, 1)]


def blend_exact(w, f0, f1):
    """(1 - w) U0 + w U1 of exact forms hi + lo as hi + lo, and the bound's sum (1 - w) B0 + w B1."""
    (h0, l0, b0), (h1, l1, b1) = f0, f1
    s, t = two_sum(np.ones_like(w), -w)                              # 1 - w = s + t exactly
    p0, e0 = two_prod(s, h0)
    p1, e1 = two_prod(w, h1)
    hi, lo = fsum2(np.array([p0, e0, t * h0, s * l0, p1, e1, w * l1]).T.tolist())
    return hi, lo, (1.0 - w) * b0 + w * b1


@pytest.mark.parametrize('wkind', ['w=0', 'w=1', 'random'])
@pytest.mark.parametrize('tag', sorted(REAL_TAGS))
def test_blend_mode_against_exact_reference(tag, wkind):
    es, G, dC, rec = real_case(tag)
    N = REAL_TAGS[tag]
    w = {'w=0': np.zeros(REAL_Q), 'w=1': np.ones(REAL_Q), 'random': np.random.default_rng(5).random(REAL_Q)}[wkind]
    out, guards = raw(es.model.handle(), es.model.ctx, G, rec, w, dC)
    assert guards
    live = ~np.isnan(G[0, 0])
    assert np.array_equal(np.isnan(out), np.broadcast_to(~live, out.shape))
    qs, ks, forms, wrong = blend_references(tag)
    hi, lo, B = blend_exact(w[qs], *forms)
    x = out[ks, qs]
    err = np.abs((x - hi) - lo)
    bound = gamma(2 * N + 8) * B
    assert np.all(B > 0)
    print('%s %s: %d samples, worst |x - exact| / bound %.3g' % (tag, wkind, len(qs), np.max(err / bound)))
    assert np.all(err <= bound), (tag, wkind, int(np.argmax(err - bound)))
    # the bound sees one triangle of dC used for both (at N = 32 the fit's covariances are too close to symmetric for any
    # bound of this kind to tell, as in the gradcov suite)
    if N >= 48:
        bad = (1.0 - w[qs]) * wrong[0] + w[qs] * wrong[1]
        assert not np.all(np.abs((bad - hi) - lo) <= bound)


# ==== 4. missing and NaN records =============================================================================================
@functools.lru_cache(maxsize=None)
def _grad_basis(tag, Q=520):
    """The device's own gradient basis (N, 3, Q) of Q points of the box with the hull's NaN columns, on the host."""
    es = te._estimate(tag, 2)
    with es.resident_grid(*te._box(Q), check_hull=True, gradient='model') as g:
        G = g.dG.download()
    dead = np.isnan(G[0, 0])
    assert 0 < dead[:300].sum() < 300 and np.array_equal(np.isnan(G), np.broadcast_to(dead, G.shape))
    G.setflags(write=False)
    return G


@pytest.mark.parametrize('interp', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'scr_k12l2'])
def test_missing_rows_and_nan_records(tag, interp):
    """rec = -1, rec >= R, rec = R - 1 with a weight (needs row R), scr_k12l2's NaN record between two good ones: six NaNs at
    exactly the points that need what is missing or lie outside the hull, six numbers everywhere else."""
    dC, rec, w, k = te._missing_case(tag, interp)
    assert (k is not None) == (tag == 'scr_k12l2')
    R = len(dC)
    es = te._estimate(tag, R)
    G = np.ascontiguousarray(_grad_basis(tag)[:, :, :rec.size])
    out, guards = raw(es.model.handle(), es.model.ctx, G, rec, w, dC)
    assert guards
    nan = np.isnan(G[0, 0]) | (rec < 0) | (rec >= R) | (interp & (rec == R - 1))
    if k is not None:
        nan |= (rec == k) | (interp & (rec == k - 1))
    assert 0 < nan.sum() < rec.size and (~nan & (rec == R - 1)).any() != interp
    assert np.array_equal(np.isnan(out), np.broadcast_to(nan, out.shape))
    assert np.isfinite(out[:, ~nan]).all()
    # no record at all: every point is NaN and no covariance is read
    none, guards = raw(es.model.handle(), es.model.ctx, G, rec, w, dC[:0])
    assert guards and np.all(np.isnan(none))


# ==== 5. permutation =========================================================================================================
@pytest.mark.parametrize('interp', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'default'])
def test_permutation(tag, interp):
    """A point's bits depend on its three columns, its record(s) and its weight alone: permuting the points permutes the bits,
    and so does cutting the points off after 300."""
    f, dC, _, _, _ = te._records(tag, te.RAW_R)
    es = te._estimate(tag, te.RAW_R)
    Q = 514
    rng = np.random.default_rng(9)
    rec = np.sort(rng.integers(0, te.RAW_R - 1, Q)).astype(np.int32)
    w = rng.random(Q) if interp else None
    G = np.ascontiguousarray(_grad_basis(tag)[:, :, :Q])
    h, ctx = es.model.handle(), es.model.ctx
    out, guards = raw(h, ctx, G, rec, w, dC)
    perm = rng.permutation(Q)
    got, guards2 = raw(h, ctx, np.ascontiguousarray(G[:, :, perm]), rec[perm], None if w is None else w[perm], dC)
    assert guards and guards2 and np.isfinite(out).sum() > 600
    assert _same_bits(got, out[:, perm])
    part, _ = raw(h, ctx, np.ascontiguousarray(G[:, :, :300]), rec[:300], None if w is None else w[:300], dC)
    assert _same_bits(part, np.ascontiguousarray(out[:, :300]))


# ==== 6. the other routes ====================================================================================================
@pytest.mark.parametrize('interp', [False, True])
def test_exact_above_the_kernels_orders(interp):
    """N = 160: run by run through the library - the same exact results."""
    assert k2tc_geometry(LIB_N, QMAX)['path'] == 'library'
    _report(exact_suite(LIB_N, interp, ' [library]'))


CHILD = '''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_track_gradcov as g
fails = g.child_suite(sys.argv[1])
for f in fails:
    print('FAIL ' + f)
sys.exit(1 if fails else 0)
'''


def child_suite(which):
    assert which == 'blas' and os.environ.get('VINTERP_EVAL_RESIDENT') == 'blas'
    fails = []
    for N in (27, 144):
        for interp in (False, True):
            fails += exact_suite(N, interp, ' [blas]')
    return fails


def _child(tmp_path, args, env_set, script_text):
    script = tmp_path / 'child.py'
    script.write_text(script_text % (REPO_ROOT, os.path.join(REPO_ROOT, 'tests')))
    env = dict(os.environ)
    for k in ('VINTERP_K2TC_GROUPS', 'VINTERP_EVAL_RESIDENT', 'VINTERP_TRACK_GRADCOV_CHUNK'):
        env.pop(k, None)
    env.update(env_set)
    r = subprocess.run([sys.executable, str(script)] + args, env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, 'child %r: exit %d\n%s\n%s' % (args, r.returncode, r.stdout[-4000:], r.stderr[-3000:])


def test_exact_suite_on_the_library_route(tmp_path):
    """The whole exact suite at N = 27 and 144 with VINTERP_EVAL_RESIDENT=blas (read once per process: a fresh child)."""
    _child(tmp_path, ['blas'], {'VINTERP_EVAL_RESIDENT': 'blas'}, CHILD)


# ==== 7. the Python API ======================================================================================================
def _bound_sums(G, dC, rec, w):
    """1/2 sum ((1 - w)(|g_c| |dC_r| |g_d| + |g_d| |dC_r| |g_c|) + w (... dC_(r+1) ...)) for every point and pair, (Q, 6)."""
    Q = G.shape[2]
    B = np.zeros((Q, 6))
    aG = np.abs(np.nan_to_num(G))
    for i in (0, 1):
        wt = (1.0 - w) if i == 0 else w
        for r in np.unique(rec):
            m = np.nonzero(rec == r)[0]
            Z = np.einsum('ik,kdq->idq', np.abs(dC[r + i]), aG[:, :, m])
            M = np.einsum('icq,idq->cdq', aG[:, :, m], Z)
            for k, (c, d) in enumerate(PAIRS):
                B[m, k] += wt[m] * 0.5 * (M[c, d] + M[d, c])
    return B


@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('frame', ['model', 'enu'])
@pytest.mark.parametrize('check_hull', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'default'])
def test_track_gradient_covariance_api(tag, check_hull, frame, timeinterp, monkeypatch):
    monkeypatch.delenv('VINTERP_TRACK_GRADCOV_CHUNK', raising=False)
    es = te._estimate(tag, 12, timeinterp)
    N = es.Covariance.shape[1]
    Q = 300
    lat, lon, alt = te._box(Q, seed=31)
    t0 = te._record_times(es, Q)
    rec, w = es.select_records(t0)
    assert len(np.unique(rec)) == (11 if timeinterp else 12) and np.any(np.diff(rec) < 0)       # about 10 records, unsorted
    cov = es.track_gradient_covariance(t0, lat, lon, alt, check_hull=check_hull, frame=frame)
    assert cov.shape == (Q, 3, 3) and cov.dtype == np.float64
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2), equal_nan=True)
    grad = es.track_gradient(t0, lat, lon, alt, check_hull=check_hull, frame=frame)
    assert np.array_equal(np.isnan(cov), np.broadcast_to(np.isnan(grad[:, 0])[:, None, None], cov.shape))
    outside = np.isnan(cov[:, 0, 0]).sum()
    assert (0 < outside < Q) if check_hull else outside == 0
    err = es.track_gradient_error(t0, lat, lon, alt, check_hull=check_hull, frame=frame)
    assert err.shape == (Q, 3)
    diag = np.einsum('qcc->qc', cov)
    with np.errstate(invalid='ignore'):
        assert np.array_equal(err, np.sqrt(diag), equal_nan=True)
    ok = np.isfinite(err)
    assert np.all(np.abs(err[ok] ** 2 - diag[ok]) <= 4 * np.finfo(float).eps * np.abs(diag[ok]))
    # element q is Estimate.gradient_covariance at the point's time
    ref = np.full((Q, 3, 3), np.nan)
    for t in np.unique(t0):
        m = t0 == t
        ref[m] = es.gradient_covariance(tt._datetime(t), lat[m], lon[m], alt[m], check_hull=check_hull, frame=frame)
    assert np.array_equal(np.isnan(cov), np.isnan(ref))
    if not timeinterp:
        assert _same_bits(cov, ref)
        return
    # the per-call method blends dC before the form, this one after it: within the bound of part 3
    with es.resident_grid(lat, lon, alt, check_hull=check_hull, gradient=frame) as g:
        G = g.dG.download()
    B = _bound_sums(G, es.Covariance, rec, w)
    live = np.isfinite(cov[:, 0, 0])
    for k, (c, d) in enumerate(PAIRS):
        diff = np.abs(cov[live, c, d] - ref[live, c, d])
        assert np.all(diff <= gamma(2 * N + 8) * B[live, k]), (c, d, float(np.max(diff / B[live, k])))


def test_track_gradient_covariance_interface():
    es = te._estimate('k8l2', 12)
    Q = 200
    lat, lon, alt = te._box(Q, seed=32)
    mt = tt._mid(es.time)
    times = (mt[:-1] + 12.5)[np.random.default_rng(2).integers(0, 11, Q)]
    got = es.track_gradient_covariance(times, lat, lon, alt)
    gerr = es.track_gradient_error(times, lat, lon, alt)
    assert 0 < np.isnan(got[:, 0, 0]).sum() < Q
    # one time for all points: a scalar, as a datetime and as seconds
    one = es.track_gradient_covariance(tt._datetime(mt[4] + 17.25), lat, lon, alt)
    assert _same_bits(one, es.gradient_covariance(tt._datetime(mt[4] + 17.25), lat, lon, alt))
    assert _same_bits(es.track_gradient_covariance(mt[4] + 17.25, lat, lon, alt), one)
    # out=, a (3, 5) shape
    buf = np.empty((Q, 3, 3))
    assert es.track_gradient_covariance(times, lat, lon, alt, out=buf) is buf and _same_bits(buf, got)
    ebuf = np.empty((Q, 3))
    assert es.track_gradient_error(times, lat, lon, alt, out=ebuf) is ebuf and _same_bits(ebuf, gerr)
    sh = es.track_gradient_covariance(*(a[:15].reshape(3, 5) for a in (times, lat, lon, alt)))
    assert sh.shape == (3, 5, 3, 3) and _same_bits(sh.reshape(15, 3, 3), got[:15])
    assert es.track_gradient_error(*(a[:15].reshape(3, 5) for a in (times, lat, lon, alt))).shape == (3, 5, 3)
    for call, bad in ((es.track_gradient_covariance, np.empty((Q, 3))), (es.track_gradient_error, np.empty((Q, 3, 3)))):
        with pytest.raises(ValueError, match='out must be'):
            call(times, lat, lon, alt, out=bad)
        with pytest.raises(ValueError, match='times must be'):
            call(times[:7], lat, lon, alt)
        with pytest.raises(ValueError, match="frame must be 'model' or 'enu'"):
            call(times, lat, lon, alt, frame='ecef')
    # times outside the file
    late = times.copy()
    late[:10] = mt[-1] + 4000.
    for call, full in ((es.track_gradient_covariance, got), (es.track_gradient_error, gerr)):
        with pytest.raises(ValueError) as e:
            call(late, lat, lon, alt)
        assert str(e.value) == tt.MESSAGE
        part = call(late, lat, lon, alt, outside='nan')
        assert np.all(np.isnan(part[:10])) and _same_bits(part[10:], full[10:])
    # nothing to compute; no covariance
    assert es.track_gradient_covariance(times[:0], lat[:0], lon[:0], alt[:0]).shape == (0, 3, 3)
    assert es.track_gradient_error(times[:0], lat[:0], lon[:0], alt[:0]).shape == (0, 3)
    nocov = te._estimate('k8l2', 12)
    nocov.Covariance = None
    for call in (nocov.track_gradient_covariance, nocov.track_gradient_error):
        with pytest.raises(ValueError, match='no covariance'):
            call(times, lat, lon, alt)


def _chunk_case():
    """track_gradient_covariance of 200 points whose runs of records straddle the chunk borders at 50, 100 and 150, in both
    modes and both frames: what the chunked child and the unchunked parent both compute."""
    lat, lon, alt = te._box(200, seed=33)
    out = []
    for timeinterp in (False, True):
        es = te._estimate('default', 12, timeinterp)
        mt = tt._mid(es.time)
        rec = te._run_records((40, 30, 50, 60, 20), 1, 2)       # runs [0, 40) [40, 70) [70, 120) [120, 180) [180, 200)
        for frame in ('model', 'enu'):
            out.append(es.track_gradient_covariance(mt[rec] + 7.5, lat, lon, alt, frame=frame))
    return np.array(out)


CHUNK_CHILD = '''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import test_gpu_track_gradcov as g
np.save(sys.argv[1], g._chunk_case())
'''


def test_chunks_in_a_child_process(tmp_path):
    """VINTERP_TRACK_GRADCOV_CHUNK=50 in a fresh child: four chunks, runs of records across the borders - the bits of the
    unchunked call."""
    assert 'VINTERP_TRACK_GRADCOV_CHUNK' not in os.environ
    own = _chunk_case()
    assert own.shape == (4, 200, 3, 3) and 0 < np.isnan(own[0, :, 0, 0]).sum() < 200
    o = str(tmp_path / 'chunked.npy')
    _child(tmp_path, [o], {'VINTERP_TRACK_GRADCOV_CHUNK': '50'}, CHUNK_CHILD)
    assert _same_bits(np.load(o), own)
