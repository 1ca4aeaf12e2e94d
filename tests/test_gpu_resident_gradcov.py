"""Gradient-covariance maps and gradient standard errors (vi_eval_resident_gradcov_f64: K2c on the matrix cores, the library's
product for N > 144; vi_eval_grad_cov_f64; ResidentGrid.gradient_covariance / gradient_error / evaluate_gradient_*;
Estimate.gradient_covariance / gradient_error).

  cov[c][d] = g_c^T 1/2 (dC + dC^T) g_d,  packed in the order of GRADCOV_PAIRS,  err[c] = sqrt(g_c^T dC g_c)

1. integer inputs small enough that every order of summation is exact: NumPy's bits at every launch geometry
   (tests/test_gradcov_host.py restates the launch and lists the cases), one-hot covariances per 16 x 16 block, dC = I, NaN
   and infinite inputs, sentinels around the output; once more in child processes with VINTERP_K2C_GROUPS=3 and with
   VINTERP_EVAL_RESIDENT=blas (the library path).
2. scaling the covariances by powers of 4 scales the maps by them bit for bit, the errors by powers of 2.
3. the fits' own covariances on real gradient bases against error-free products and exact summation, within
   gamma_{2N+4} 1/2 sum (|g_c| |dC| |g_d| + |g_d| |dC| |g_c|); the bound rejects one triangle of dC used for both.
4. the Python API: shapes, symmetry, NaN pattern, K2c's diagonal against K2e's on the same bits, Estimate.gradient_covariance
   against the map, chunked builds, time interpolation.
5. the oracle's gradient basis.  6. the errors raised."""
import datetime as dt
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden, rel
from test_gpu_resident_geometry import (GUARD, SENTINEL, _handle, form_reference, fsum2, gamma, map_gate, mismatch, sum2,
                                        two_prod)
from test_gpu_resident_error import BITS_TOL, BITS_WORST
from test_gradcov_host import K2C_QS, K2C_TS, case_line, k2c_cases, k2c_geometry

gpu = pytest.mark.gpu
pytestmark = gpu

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
QMAX, TMAX = max(K2C_QS), max(K2C_TS)


def _t_mid(f):
    return dt.datetime(1970, 1, 1) + dt.timedelta(seconds=float(np.mean(f['utime'][0])))


def _estimate(tag, timeinterp=False, cov=True):
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_' + tag)
    return f, Estimate.from_arrays(np.nan_to_num(f['Coeffs']), f['Covariance'] if cov else None, f['utime'], f['hull_vert'],
                                   str(f['cfg']), timeinterp=timeinterp)


def host_gradcov(G, dC):
    """The definition on the host: (6, Q) packed, for a gradient basis G (N, 3, Q) and one covariance."""
    N, _, Q = G.shape
    with np.errstate(invalid='ignore', over='ignore'):
        Z = (dC @ G.reshape(N, 3 * Q)).reshape(N, 3, Q)
        M = np.einsum('icq,idq->cdq', G, Z)
        return np.array([M[c, c] if c == d else 0.5 * (M[c, d] + M[d, c]) for c, d in PAIRS])


def _same_bits(x, ref, worst=True):
    """NaN pattern identical; finite values within the same-bits gate of test_gpu_resident_error.py: norm-wise and, for a
    quantity that does not change sign (worst), at the worst point."""
    assert np.array_equal(np.isnan(x), np.isnan(ref))
    ok = np.isfinite(ref)
    assert ok.any()
    assert rel(x[ok], ref[ok]) <= BITS_TOL
    if worst:
        assert np.max(np.abs(x[ok] - ref[ok]) / np.abs(ref[ok])) <= BITS_WORST


def _same_bits_packed(x, ref):
    """_same_bits per plane of a packed (6, Q) result: the diagonal entries also at the worst point, the cross terms (which
    pass through zero) norm-wise."""
    for k, (c, d) in enumerate(PAIRS):
        _same_bits(x[k], ref[k], worst=c == d)


# ==== 1. exact by construction ===============================================================================================
def run(N, Q, T, G, dC, h=None):
    """vi_eval_resident_gradcov_f64 on device copies, the output between GUARD sentinel doubles on either side.  Returns
    (out (T, 6, Q), whether every sentinel is unchanged)."""
    from volumetricinterp_amd import _lib
    ctx = _lib.get_context()
    h = _handle(N) if h is None else h
    G = np.ascontiguousarray(G, dtype=np.float64)
    dC = np.ascontiguousarray(dC, dtype=np.float64)
    assert G.shape == (N, 3, Q) and dC.shape == (T, N, N)
    bufs = []
    try:
        bufs.append(ctx.to_device(G) if G.size else ctx.empty(1))
        bufs.append(ctx.to_device(dC) if dC.size else ctx.empty(1))
        dO = ctx.to_device(np.full(2 * GUARD + T * 6 * Q, SENTINEL))
        bufs.append(dO)
        _lib.check(_lib.lib.vi_eval_resident_gradcov_f64(h, Q, T, bufs[0].ptr, bufs[1].ptr, dO.offset_ptr(GUARD)),
                   'vi_eval_resident_gradcov_f64')
        res = dO.download()
    finally:
        for b in bufs:
            b.free()
    sb = np.array([SENTINEL]).view(np.uint64)[0]
    bits = res.view(np.uint64)
    guards = bool(np.all(bits[:GUARD] == sb) and np.all(bits[GUARD + T * 6 * Q:] == sb))
    return res[GUARD:GUARD + T * 6 * Q].reshape(T, 6, Q), guards


def diff(out, ref, what):
    return mismatch(out.reshape(out.shape[0], -1), ref.reshape(ref.shape[0], -1), what)


_INT = {}


def integer_inputs(N):
    """|g|, |dC| <= 2^e with N^2 2^(3e + 1) <= 2^46: every form is an integer below 2^45 in any order of summation (K2c's
    dC_IJ + dC_JI^T and the half-sum of two forms included), so the result is exact and must have NumPy's bits.  TMAX
    covariances by t % 5 as in the K2e suite - diagonally dominant asymmetric, its negation (negative diagonal entries,
    returned as they are), antisymmetric (everything exactly 0), random signs, a larger skew part - on QMAX points; computed
    once per N, every case takes its first T covariances and Q points.  Returns (dC, G, ref (TMAX, 6, QMAX))."""
    if N not in _INT:
        rng = np.random.default_rng(1000 + N)
        e = int((45 - 2 * math.log2(N)) // 3)
        G = rng.integers(-2 ** e, 2 ** e + 1, (N, 3, QMAX)).astype(np.float64)
        dC = np.empty((TMAX, N, N))
        for t in range(TMAX):
            k = t % 5
            if k in (0, 1, 4):
                A = rng.integers(-2 ** (e - 3), 2 ** (e - 3) + 1, (N, N)).astype(np.float64)
                if k == 4:
                    A += np.triu(rng.integers(-2 ** (e - 3), 2 ** (e - 3) + 1, (N, N)), 1)
                A[np.diag_indices(N)] = rng.integers(2 ** (e - 1), 2 ** e + 1, N)
                dC[t] = -A if k == 1 else A
            elif k == 2:
                A = np.triu(rng.integers(-2 ** (e - 1), 2 ** (e - 1) + 1, (N, N)), 1).astype(np.float64)
                dC[t] = A - A.T
            else:
                dC[t] = rng.integers(-2 ** (e - 1), 2 ** (e - 1) + 1, (N, N))
        ref = np.array([host_gradcov(G, d) for d in dC])
        assert np.all(2 * ref == np.rint(2 * ref)) and np.abs(ref).max() < 2.0 ** 46
        for a in (dC, G, ref):
            a.setflags(write=False)
        _INT[N] = (dC, G, ref)
    return _INT[N]


def integer_case(N, Q, T):
    """The first T covariances and Q points of integer_inputs(N) with the special values of the case: NaN point columns
    (hull-masked points: all three components) and, from T = 3 on, one NaN covariance entry."""
    dC, G, ref = integer_inputs(N)
    dC, G, ref = dC[:T].copy(), G[:, :, :Q].copy(), ref[:T, :, :Q].copy()
    if Q >= 4:
        for q in (1, Q - 2):
            G[:, :, q] = np.nan
            ref[:, :, q] = np.nan
    if T >= 3:
        dC[2, N // 2, N - 1] = np.nan
        ref[2] = np.nan
    return dC, G, ref


def integer_suite(cases, tag=''):
    """Failures of the integer cases (N, Q, T): NumPy's bits, untouched sentinels, exact zeros for antisymmetric
    covariances, negative diagonal entries returned."""
    fails = []
    for N, Q, T in cases:
        line = case_line(N, Q, T, int(tag[9:-1]) if tag.startswith(' [groups') else None, blas='blas' in tag) + tag
        print(line)
        dC, G, ref = integer_case(N, Q, T)
        out, guards = run(N, Q, T, G, dC)
        if not guards:
            fails.append(line + ': a store outside the output')
        m = diff(out, ref, line + ' integer')
        if m:
            fails.append(m)
        if T >= 2 and not (ref[1, :3, 0] < 0).all():
            fails.append(line + ': no negative diagonal entry in the reference')
    return fails


def one_hot_suite(tag=''):
    """N = 144 and N = 50, Q = 65: one covariance e_i e_k^T per 16 x 16 block (I, J), i and k at varying places inside their
    blocks (i != k: asymmetric), expected 1/2 (G[i, c] G[k, d] + G[k, c] G[i, d]) with G[n, c, q] = 1 + (3 n + c) Q + q
    naming its element; then dC = I: the Gram matrix of the three columns."""
    fails = []
    for N in (144, 50):
        NB, Q = -(-N // 16), 65
        G = 1.0 + (3 * np.arange(N)[:, None, None] + np.arange(3)[None, :, None]) * Q + np.arange(Q)[None, None, :]
        ik = [(min(16 * I + (5 * I + 3 * J + 1) % 16, N - 1 - (I == J)), min(16 * J + (7 * J + I + 2) % 16, N - 1))
              for I in range(NB) for J in range(NB)]
        ik = [(i, k if k != i else k - 1) for i, k in ik]
        T = len(ik) + 1
        dC = np.zeros((T, N, N))
        ref = np.empty((T, 6, Q))
        for t, (i, k) in enumerate(ik):
            assert i != k and 0 <= i < N and 0 <= k < N
            dC[t, i, k] = 1.0
            for p, (c, d) in enumerate(PAIRS):
                ref[t, p] = 0.5 * (G[i, c] * G[k, d] + G[k, c] * G[i, d])
        assert {(i // 16, k // 16) for i, k in ik} == {(I, J) for I in range(NB) for J in range(NB)}
        dC[T - 1] = np.eye(N)
        for p, (c, d) in enumerate(PAIRS):
            ref[T - 1, p] = (G[:, c] * G[:, d]).sum(0)
        assert np.abs(ref).max() < 2.0 ** 52
        what = 'K2c one-hot N %d Q %d T %d%s' % (N, Q, T, tag)
        print(what)
        out, guards = run(N, Q, T, G, dC)
        if not guards:
            fails.append(what + ': a store outside the output')
        m = diff(out, ref, what)
        if m:
            t = int(np.argwhere(~(out == ref))[0][0])
            fails.append(m + (' (covariance e_%d e_%d^T)' % ik[t] if t < len(ik) else ' (dC = I)'))
    return fails


def special_suite(tag=''):
    """A NaN column gives six NaNs at that point only, a NaN in one covariance NaN in that timestep only (both in every integer
    case); here an infinite entry in row 0 of component 0 at N = 18 and N = 50 (padded rows in the last block column): the
    entries of the pairs without component 0 keep NumPy's bits everywhere, the others everywhere but at those points, where
    they are not finite."""
    fails = []
    for N in (18, 50):
        Q, T = 260, 3
        dC, G, ref = integer_inputs(N)
        dC, G, ref = dC[:T].copy(), G[:, :, :Q].copy(), ref[:T, :, :Q].copy()
        hit = np.array([0, 5, 17, Q // 3, Q - 1])
        G[0, 0, hit] = [np.inf, -np.inf, np.inf, -np.inf, np.inf]
        what = 'K2c N %d Q %d T %d inf in row 0%s' % (N, Q, T, tag)
        print(what)
        out, guards = run(N, Q, T, G, dC)
        if not guards:
            fails.append(what + ': a store outside the output')
        with0 = np.array([0 in p for p in PAIRS])
        if np.isfinite(out[:, with0][:, :, hit]).any():
            fails.append(what + ': a finite entry of component 0 at a point with an infinite basis value')
        chk, want = out.copy(), ref.copy()
        for a in (chk, want):
            a[:, :, hit] = np.where(with0[None, :, None], 0.0, a[:, :, hit])
        m = diff(chk, want, what)
        if m:
            fails.append(m + ' (leaked into another point or component)')
    for Q, T in ((260, 0), (0, 3)):                        # T = 0 and Q = 0 write nothing
        out, guards = run(32, Q, T, np.ones((32, 3, Q)), np.ones((T, 32, 32)))
        if not guards or out.size:
            fails.append('K2c N 32 Q %d T %d: not a no-op%s' % (Q, T, tag))
    return fails


def _cases(groups, Ns=None):
    return [(N, Q, T) for N, Q, T, g in k2c_cases() if g == groups and (Ns is None or N in Ns)]


def _report(fails):
    for f in fails:
        print('FAIL ' + f)
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('N', sorted({c[0] for c in k2c_cases()}))
def test_integer_inputs_exact_at_every_geometry(N, monkeypatch):
    """Every case of k2c_cases at the default groups: NumPy's bits, nothing touched outside the output."""
    monkeypatch.delenv('VINTERP_K2C_GROUPS', raising=False)
    assert k2c_geometry(N, 260, 1)['path'] == ('kernel' if N <= 144 else 'library')
    _report(integer_suite(_cases(None, (N,))))


def test_one_hot_identity_and_special_values(monkeypatch):
    monkeypatch.delenv('VINTERP_K2C_GROUPS', raising=False)
    _report(one_hot_suite() + special_suite())


CHILD = '''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_resident_gradcov as g
fails = g.child_suite(sys.argv[1])
for f in fails:
    print('FAIL ' + f)
sys.exit(1 if fails else 0)
'''


def child_suite(which):
    """What a child process runs: 'groups<n>' the cases of k2c_cases with that VINTERP_K2C_GROUPS (set by the parent), 'blas'
    the whole integer suite and the real-magnitude suite on the library path."""
    if which.startswith('groups'):
        n = int(which[6:])
        assert os.environ.get('VINTERP_K2C_GROUPS') == str(n)
        fails = integer_suite(_cases(n), ' [groups %d]' % n)
        return fails + (one_hot_suite(' [groups %d]' % n) if n > 1 else [])
    assert which == 'blas' and os.environ.get('VINTERP_EVAL_RESIDENT') == 'blas'
    fails = integer_suite(_cases(None), ' [blas]') + one_hot_suite(' [blas]') + special_suite(' [blas]')
    for tag in sorted(REAL_N):
        fails += real_suite(tag, ' [blas]')
    return fails


def _child(tmp_path, which, env_set):
    script = tmp_path / 'child.py'
    script.write_text(CHILD % (REPO_ROOT, os.path.join(REPO_ROOT, 'tests')))
    env = dict(os.environ)
    for k in ('VINTERP_K2C_GROUPS', 'VINTERP_EVAL_RESIDENT', 'VINTERP_GRADCOV_CHUNK'):
        env.pop(k, None)
    env.update(env_set)
    r = subprocess.run([sys.executable, str(script), which], env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, '%s child: exit %d\n%s\n%s' % (which, r.returncode, r.stdout[-4000:], r.stderr[-3000:])


@pytest.mark.parametrize('groups', [1, 3])
def test_integer_suite_with_several_groups(tmp_path, groups):
    """VINTERP_K2C_GROUPS = 1 and 3 in a fresh child process each: several passes over points per workgroup, passes that end
    early and workgroups whose last passes are empty."""
    _child(tmp_path, 'groups%d' % groups, {'VINTERP_K2C_GROUPS': str(groups)})


def test_suites_on_the_library_path(tmp_path):
    """The whole integer suite and the real-magnitude suite once more with VINTERP_EVAL_RESIDENT=blas (read once per
    process: a fresh child process): the library path gives the same exact bits and meets the same bound."""
    _child(tmp_path, 'blas', {'VINTERP_EVAL_RESIDENT': 'blas'})


# ==== 2. exact scaling =======================================================================================================
def test_scaling_by_powers_of_four_is_exact():
    """Covariances scaled by 4^j, j in [-4, 4]: the maps scale by 4^j and evaluate_gradient_errors by 2^j, bit for bit (a
    power of two changes no rounding).  Q = 2052, T = 40, the k8l2 fixture, random points, some outside the hull."""
    f, es = _estimate('k8l2')
    rng = np.random.default_rng(40)
    Q, T = 2052, 40
    lat, lon, alt = rng.uniform(74, 82, Q), rng.uniform(248, 276, Q), rng.uniform(90e3, 750e3, Q)
    cov = np.nan_to_num(f['Covariance'])
    dC = cov[rng.integers(0, len(cov), T)] * rng.uniform(0.5, 2.0, (T, 1, 1))
    j = (np.arange(T) % 9) - 4
    assert set(j) == set(range(-4, 5))
    with es.resident_grid(lat, lon, alt, gradient='model') as g:
        base = g.evaluate_gradient_covariances(dC)
        scaled = g.evaluate_gradient_covariances(dC * (4.0 ** j)[:, None, None])
        ebase = g.evaluate_gradient_errors(dC)
        escaled = g.evaluate_gradient_errors(dC * (4.0 ** j)[:, None, None])
    outside = np.isnan(base[0, 0])
    assert 0 < outside.sum() < Q
    assert np.array_equal(np.isnan(base), np.broadcast_to(outside, base.shape))
    assert not diff(scaled, base * (4.0 ** j)[:, None, None], 'maps scaled by 4^j')
    assert not diff(escaled, ebase * (2.0 ** j)[:, None, None], 'errors scaled by 2^j')
    assert np.isfinite(ebase[:, :, ~outside]).any()


# ==== 3. real magnitudes against an exact reference ==========================================================================
REAL_N = {'default': 144, 'scr_k12l2': 48, 'k8l2': 32}


def bilinear_reference(dC, A, B, ts, qs):
    """sum_ik A[i, q] dC[t, i, k] B[k, q] at the samples as hi + lo, and sum_ik |a_i| |dC_ik| |b_k|: z = dC b from the exact
    products summed by sum2, then a . z by math.fsum over exact products - form_reference with two vectors."""
    N = A.shape[0]
    hi, lo, B0 = np.empty(len(ts)), np.empty(len(ts)), np.empty(len(ts))
    step = max(1, 2 ** 21 // (N * N))
    for t in np.unique(ts):
        idx = np.nonzero(ts == t)[0]
        D = dC[t]
        for s in range(0, len(idx), step):
            j = idx[s:s + step]
            a, b = A[:, qs[j]].T, B[:, qs[j]].T
            p, e = two_prod(D[None, :, :], b[:, None, :])
            zh, zl = sum2(p)
            zl = zl + e.sum(-1)
            p2, e2 = two_prod(a, zh)
            hi[j], lo[j] = fsum2(np.concatenate([p2, e2, a * zl], axis=1).tolist())
            B0[j] = ((np.abs(b) @ np.abs(D).T) * np.abs(a)).sum(1)
    return hi, lo, B0


def gradcov_reference(dC, G, ts, qs, ks):
    """g_c^T 1/2 (dC + dC^T) g_d at the samples (t, q, pair k) as hi + lo, and the bound's sum
    1/2 sum_ik (|g_c,i| |dC_ik| |g_d,k| + |g_d,i| |dC_ik| |g_c,k|)."""
    hi, lo, B0 = np.empty(len(ts)), np.empty(len(ts)), np.empty(len(ts))
    for k, (c, d) in enumerate(PAIRS):
        w = np.nonzero(ks == k)[0]
        if not len(w):
            continue
        h1, l1, b1 = bilinear_reference(dC, G[:, c], G[:, d], ts[w], qs[w])
        h2, l2, b2 = (h1, l1, b1) if c == d else bilinear_reference(dC, G[:, d], G[:, c], ts[w], qs[w])
        hi[w], lo[w] = fsum2((0.5 * np.array([h1, l1, h2, l2]).T).tolist())          # halving is exact
        B0[w] = 0.5 * (b1 + b2)
    return hi, lo, B0


def gradcov_gate(x, hi, lo, B0, N):
    """Per sample: |x - exact| <= gamma_{2N+4} B0: form_gate's bound with one more rounding for the symmetrising sum."""
    return np.abs((x - hi) - lo) <= gamma(2 * N + 4) * B0


def real_suite(tag, note=''):
    """The fixture `tag` (N = 144, 48, 32) with the fit's own covariances: synth.query_grid(6) with the hull in the model frame
    and 2052 random points, some outside the hull, in east-north-up, through evaluate_gradient_covariances and
    evaluate_gradient_errors; samples (t, q, pair) against the exact reference on the downloaded dG bits."""
    from volumetricinterp_amd import synth
    fails = []
    N = REAL_N[tag]
    f, es = _estimate(tag)
    dC = np.nan_to_num(f['Covariance'])
    T = len(dC)
    rng = np.random.default_rng(N)
    sets = (('grid 6^3 model', tuple(np.asarray(a).ravel() for a in synth.query_grid(6)), 'model'),
            ('2052 random enu', (rng.uniform(74, 82, 2052), rng.uniform(248, 276, 2052), rng.uniform(90e3, 750e3, 2052)), 'enu'))
    for name, pts, frame in sets:
        what = 'K2c real %s N %d %s%s' % (tag, N, name, note)
        with es.resident_grid(*pts, check_hull=True, gradient=frame) as g:
            G = g.dG.download()
            out = g.evaluate_gradient_covariances(dC)
            err = g.evaluate_gradient_errors(dC)
        Q = G.shape[2]
        inside = np.isfinite(G[0, 0])
        pool = np.nonzero(np.isfinite(G).all(axis=(0, 1)))[0]
        if not (20 <= inside.sum() < Q and len(pool) >= 20):
            fails.append(what + ': %d points inside the hull of %d' % (inside.sum(), Q))
            continue
        if not np.array_equal(np.isnan(out), np.broadcast_to(~inside, out.shape)):
            fails.append(what + ': the NaN pattern is not the hull\'s')
        n = 240
        ts = np.concatenate([rng.integers(0, T, n), np.repeat(np.arange(min(T, 2)), 12)])
        qs = np.concatenate([pool[rng.integers(0, len(pool), n)], np.tile(np.repeat(pool[[0, -1]], 6), min(T, 2))])
        ks = np.concatenate([rng.integers(0, 6, n), np.tile(np.arange(6), 2 * min(T, 2))])
        hi, lo, B0 = gradcov_reference(dC, G, ts, qs, ks)
        x = out[ts, ks, qs]
        ok = gradcov_gate(x, hi, lo, B0, N)
        live = B0 > 0                                    # (a failed record's covariance is stored as zeros here: 0 <= 0)
        if live.sum() < 100:
            fails.append('%s: only %d samples with a covariance that is not zero' % (what, live.sum()))
            continue
        worst = np.max(np.abs((x - hi) - lo)[live] / (gamma(2 * N + 4) * B0[live]))
        print('%s: %d samples, worst |x - exact| / bound %.3g' % (what, len(ts), worst))
        if not ok.all():
            i = np.nonzero(~ok)[0][0]
            fails.append('%s: %d of %d samples outside the bound, first t %d q %d pair %d: %r, exact %r, bound %r' % (
                what, (~ok).sum(), len(ok), ts[i], qs[i], ks[i], x[i], hi[i], gamma(2 * N + 4) * B0[i]))
        # the bound sees one triangle of dC used for both (an answer that takes dC for symmetric)
        if N >= 48:
            tri = np.array([np.triu(d) + np.triu(d, 1).T for d in dC])
            wrong = gradcov_reference(tri, G, ts, qs, ks)[0]
            if gradcov_gate(wrong, hi, lo, B0, N).all():
                fails.append(what + ': the bound accepts one triangle of dC mirrored')
        # the standard errors: K2e on the 3Q columns, against the diagonal
        dg = ks < 3
        eh, el, eb = form_reference(dC, G.reshape(G.shape[0], 3 * Q), ts[dg], ks[dg] * Q + qs[dg])
        okm = map_gate(err[ts[dg], ks[dg], qs[dg]], eh, el, eb, N)
        if not okm.all():
            fails.append('%s: %d of %d gradient errors outside the bound' % (what, (~okm).sum(), len(okm)))
        if not np.isnan(err[:, :, ~inside]).all():
            fails.append(what + ': a gradient error outside the hull is not NaN')
    return fails


@pytest.mark.parametrize('tag', sorted(REAL_N))
def test_real_magnitudes_against_exact_reference(tag):
    _report(real_suite(tag))


# ==== 4. the Python API ======================================================================================================
@pytest.mark.parametrize('frame', ['model', 'enu'])
@pytest.mark.parametrize('check_hull', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'default'])
def test_maps_through_the_python_api(tag, check_hull, frame, monkeypatch):
    from volumetricinterp_amd import synth
    monkeypatch.delenv('VINTERP_GRADCOV_CHUNK', raising=False)
    f, es = _estimate(tag)
    grid = synth.query_grid(6)
    t = _t_mid(f)
    with es.resident_grid(*grid, check_hull=check_hull, gradient=frame) as g:
        cov = g.gradient_covariance([t])
        assert cov.shape == (1, 3, 3, 6, 6, 6)
        assert np.array_equal(cov, np.swapaxes(cov, 1, 2), equal_nan=True)
        dens = g([t])
        assert np.isfinite(dens[0]).sum() > 20
        for c in range(3):
            for d in range(3):
                assert np.array_equal(np.isnan(cov[0, c, d]), np.isnan(dens[0])), (c, d)
        err = g.gradient_error([t])
        assert err.shape == (1, 3, 6, 6, 6)
        for c in range(3):                              # the same quantity from K2c and from K2e on the same bits
            _same_bits(cov[0, c, c].ravel(), err[0, c].ravel() ** 2)
        packed = g.evaluate_gradient_covariances(es.get_C(t)[1][None])
        _same_bits_packed(packed[0], host_gradcov(g.dG.download(), es.get_C(t)[1]))
    pt = es.gradient_covariance(t, *grid, check_hull=check_hull, frame=frame)
    assert pt.shape == (6, 6, 6, 3, 3)
    assert np.array_equal(pt, np.swapaxes(pt, -1, -2), equal_nan=True)
    for c, d in PAIRS:
        _same_bits(pt[..., c, d].ravel(), cov[0, c, d].ravel())
    pe = es.gradient_error(t, *grid, check_hull=check_hull, frame=frame)
    assert pe.shape == (6, 6, 6, 3)
    with np.errstate(invalid='ignore'):
        assert np.array_equal(pe, np.sqrt(np.einsum('...cc->...c', pt)), equal_nan=True)
    # the basis built in chunks: Q = 216 in three chunks, the last one ragged - the same bits
    monkeypatch.setenv('VINTERP_GRADCOV_CHUNK', '100')
    chunked = es.gradient_covariance(t, *grid, check_hull=check_hull, frame=frame)
    assert np.array_equal(chunked.view(np.uint64), pt.view(np.uint64))


@pytest.mark.parametrize('tag', ['k8l2', 'default'])
def test_time_interpolation(tag):
    """timeinterp=True: the covariance the reference's own get_C interpolated (tests/golden/eval.npz), on the grid's own
    gradient bits, and the reference's error text for a time outside the records."""
    from volumetricinterp_amd import synth
    e = load_golden('eval')
    f, es = _estimate(tag, timeinterp=True)
    grid = synth.query_grid(6)
    t = dt.datetime(1970, 1, 1) + dt.timedelta(seconds=float(e[tag + '_t_int']))
    with es.resident_grid(*grid, gradient='model') as g:
        cov = g.gradient_covariance([t])
        ref = host_gradcov(g.dG.download(), e[tag + '_tinterp_dC'])
        assert np.isfinite(ref[0]).sum() > 20
        _same_bits_packed(np.array([cov[0, c, d].ravel() for c, d in PAIRS]), ref)
        pt = es.gradient_covariance(t, *grid)
        _same_bits_packed(np.array([pt[..., c, d].ravel() for c, d in PAIRS]), ref)
        for call in (g.gradient_covariance, g.gradient_error):
            with pytest.raises(ValueError, match=re.escape(str(e[tag + '_oor']))):
                call([t - dt.timedelta(days=30)])
    with pytest.raises(ValueError, match=re.escape(str(e[tag + '_oor']))):
        es.gradient_covariance(t - dt.timedelta(days=30), *grid)


# ==== 5. against the oracle ==================================================================================================
@pytest.mark.parametrize('tag', ['k8l2', 'default'])
def test_against_the_oracle_gradient_basis(tag):
    """The oracle's grad_basis with the fixture's covariance gives the host form F_or; the host form on the device's own dG
    bits is F_dev.  The device result x may add only the same-bits gate to the difference of the two bases, which is
    existing code's and measured here: rel(x, F_or) <= rel(F_dev, F_or) + BITS_TOL.  Model frame (the oracle has no other)."""
    import oracle
    from volumetricinterp_amd import synth
    f, es = _estimate(tag)
    o = {'k8l2': lambda: oracle.SphHarmLagOracle(maxk=8, maxl=2), 'default': lambda: oracle.SphHarmLagOracle()}[tag]()
    grid = synth.query_grid(6)
    t = _t_mid(f)
    _, dC = oracle.get_C(t, f['utime'], f['Coeffs'], f['Covariance'])
    lat, lon, alt = (np.asarray(a, dtype=np.float64).ravel() for a in grid)
    Gor = np.ascontiguousarray(np.transpose(o.grad_basis(lat, lon, alt), (2, 1, 0)))         # (P, 3, N) -> (N, 3, P)
    F_or = host_gradcov(Gor, dC)
    with es.resident_grid(*grid, check_hull=False, gradient='model') as g:
        x = g.evaluate_gradient_covariances(dC[None])[0]
        F_dev = host_gradcov(g.dG.download(), dC)
    pt = np.stack([es.gradient_covariance(t, *grid, check_hull=False)[..., c, d].ravel() for c, d in PAIRS])
    ok = np.isfinite(F_or) & np.isfinite(F_dev)
    assert ok.sum() > 6 * 20 and np.array_equal(np.isfinite(x), np.isfinite(F_dev))
    base = rel(F_dev[ok], F_or[ok])
    for name, v in (('map', x), ('points', pt)):
        got = rel(v[ok], F_or[ok])
        print('%s %s: rel(x, F_or) %.3g, rel(F_dev, F_or) %.3g' % (tag, name, got, base))
        assert got <= base + BITS_TOL


# ==== 6. errors ==============================================================================================================
def test_errors_raised():
    from volumetricinterp_amd import _lib, synth
    from volumetricinterp_amd.estimate import Estimate
    f, es = _estimate('k8l2')
    grid = synth.query_grid(4)
    Q, t = 64, _t_mid(f)
    dC = f['Covariance'][:3]
    with es.resident_grid(*grid) as plain:                        # no gradient basis
        for call, arg in ((plain.gradient_covariance, [t]), (plain.gradient_error, [t]),
                          (plain.evaluate_gradient_covariances, dC), (plain.evaluate_gradient_errors, dC)):
            with pytest.raises(ValueError, match='holds no gradient basis'):
                call(arg)
    with es.resident_rays((grid[0].ravel()[:4], grid[1].ravel()[:4], grid[2].ravel()[:4]),
                          (grid[0].ravel()[4:8], grid[1].ravel()[4:8], grid[2].ravel()[4:8]), nodes=4) as rays:
        with pytest.raises(ValueError, match='holds no gradient basis'):
            rays.gradient_covariance([t])
    _, nocov = _estimate('k8l2', cov=False)
    with nocov.resident_grid(*grid, gradient='model') as gn:
        for call in (gn.gradient_covariance, gn.gradient_error):
            with pytest.raises(ValueError, match='no covariance'):
                call([t])
    for call in (nocov.gradient_covariance, nocov.gradient_error):
        with pytest.raises(ValueError, match='no covariance'):
            call(t, *grid)
    with es.resident_grid(*grid, gradient='enu') as g:
        for call, width in ((g.evaluate_gradient_covariances, 6), (g.evaluate_gradient_errors, 3)):
            with pytest.raises(ValueError, match='covariances must have shape'):
                call(np.zeros((3, 31, 31)))
            with pytest.raises(ValueError, match='covariances must have shape'):
                call(np.zeros((32, 32)))
            for bad in (np.empty((2, width, Q)), np.empty((3, width, Q), dtype=np.float32), np.empty((3, Q, width)),
                        np.empty((3, width + 1, Q))):
                with pytest.raises(ValueError, match='out must be'):
                    call(dC, out=bad)
            out = _lib.pinned_empty((3, width, Q))
            assert call(dC, out=out) is out
            assert np.array_equal(out, call(dC), equal_nan=True)
            assert call(dC[:0]).shape == (0, width, Q)
        assert g.gradient_covariance([]).shape == (0, 3, 3, 4, 4, 4) and g.gradient_error([]).shape == (0, 3, 4, 4, 4)
    with pytest.raises(ValueError, match='closed'):
        g.evaluate_gradient_covariances(dC)
    with pytest.raises(ValueError, match="frame must be 'model' or 'enu'"):
        es.gradient_covariance(t, *grid, frame='ecef')
    assert es.gradient_covariance(t, grid[0][:0], grid[1][:0], grid[2][:0]).shape == grid[0][:0].shape + (3, 3)
    # the RBF model has no gradient basis: the library's refusal surfaces, as it does for Estimate.gradient
    fr = load_golden('fit_rbf')
    rbf = Estimate.from_arrays(fr['Coeffs'], fr['Covariance'], fr['utime'], fr['hull_vert'], str(fr['cfg']))
    with pytest.raises(_lib.VinterpError, match='only the sphharmlag model provides a gradient basis'):
        rbf.gradient_covariance(_t_mid(fr), *grid)
    with pytest.raises(_lib.VinterpError, match='only the sphharmlag model provides a gradient basis'):
        rbf.gradient_error(_t_mid(fr), *grid)
