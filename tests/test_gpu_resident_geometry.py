"""Resident-grid evaluation (vi_eval_resident_f64) and standard-error maps (vi_eval_resident_err_f64) at every launch geometry,
against answers known by construction and against a high-precision reference.

The launch of both calls is chosen from (N, Q, T, alignment) alone (csrc/vi_eval_resident.hip, csrc/vi_resident.hip);
k2r_geometry and k2e_geometry below restate it:

  K2r  k_eval_resident       KS = ceil(N / 4) k-steps, padded to KSp (a multiple of PF = 4); coefficient tile KSp x 2 KB of
                             LDS, <= 150 KB (N <= 288); Q % 4 == 0, Q >= 256, Y and out 32-byte aligned.  groups =
                             clamp(Q >> 16, 1, 32) (VINTERP_K2R_GROUPS: 1 .. 256), npg = ceil(Q / (256 groups)) groups of
                             points, ntt = ceil(T / 64) timestep tiles, blocks in XCD order (npg rounded up to 8).
                             Anything else: the library's product.
  K2e  k_eval_resident_err   NB = ceil(N / 16) = 1 .. 9 (N <= 144); Q even, Y and out 16-byte aligned.  groups =
       <NB>                  clamp(Q >> 16, 1, 8) (VINTERP_K2E_GROUPS), npg = ceil(Q / (256 groups)), one timestep per
                             block.  Anything else: the library's product plus a row dot, in chunks of 2^25 / N points.

Part 1 (no GPU) asserts that the case lists reach every class of these formulas.  Part 2 uses integer inputs small enough
that every summation order gives the exact result, so every geometry must give NumPy's bits: one-hot inputs pin the index
maps, sentinel rows around the output catch stray stores, and NaN / infinite / negative / zero cases must come out as IEEE
evaluation gives them.  The whole integer suite runs a second time in a child process with VINTERP_EVAL_RESIDENT=blas (the
setting is read once per process).  Part 3 checks real basis matrices with fixture and synthetic coefficients and
covariances pointwise against error bounds around a reference built from error-free products and exact summation, and shows
on the host that each bound rejects an emulated wrong answer.  Part 4 covers the slab loops of ResidentGrid and the
fused-evaluation dispatch entries that no other test reaches.

Finding: K2r read basis row 0 for the padded rows of its last k-steps and multiplied it by a zero coefficient, so an infinite
value in row 0 gave NaN at every order with N % 16 != 0 (test_k2r_infinite_basis_row).  The padded rows are now zero."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden, rel

gpu = pytest.mark.gpu                # every test but test_geometry_list_covers_every_class

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LDS_LIMIT = 150 * 1024
GUARD = 64                                          # sentinel doubles before and after every output (512 bytes)
SENTINEL = np.array([0xFFF0DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]
GROUP_ENV = ('VINTERP_K2R_GROUPS', 'VINTERP_K2E_GROUPS')


# ==== 1. launch geometry ====================================================================================================
def _groups(Q, cap, env):
    g = min(max(Q >> 16, 1), cap)
    if env is not None and 1 <= env <= 256:
        g = env
    return g


def k2r_geometry(N, Q, T, groups=None, off=0):
    """The launch vi_eval_resident_f64 chooses (vi_eval_resident_mfma); off: Y and out this many doubles past an aligned
    base; groups: VINTERP_K2R_GROUPS."""
    KS = (N + 3) // 4
    KSp = (KS + 3) // 4 * 4
    shm = KSp * 4 * 64 * 8
    g = _groups(Q, 32, groups)
    npg = -(-Q // (256 * g))
    ntt = -(-T // 64)
    kernel = Q % 4 == 0 and (8 * off) % 32 == 0 and shm <= LDS_LIMIT and Q >= 256 and (npg + 7) // 8 * 8 * ntt < 2 ** 31
    return dict(path='kernel' if kernel else 'library', KS=KS, KSp=KSp, pad=KSp - KS, shm=shm, groups=g, npg=npg, ntt=ntt,
                cls='KSp %2d (KS %2d +%d, KSp/4 %s, N%%4 %d)' % (KSp, KS, KSp - KS, 'odd' if (KSp // 4) % 2 else 'even', N % 4))


def k2e_geometry(N, Q, T, groups=None, off=0):
    """The launch vi_eval_resident_err_f64 chooses (vi_eval_resident_err_mfma, else the library in chunks of 2^25 / N)."""
    NB = -(-N // 16)
    g = _groups(Q, 8, groups)
    npg = -(-Q // (256 * g))
    kernel = 1 <= N <= 144 and Q % 2 == 0 and (8 * off) % 16 == 0 and (npg + 7) // 8 * 8 * T < 2 ** 31
    chunk = min(2 ** 25 // N, max(Q, 1))
    return dict(path='kernel' if kernel else 'library', NB=NB, shm=NB * (NB + 1) // 2 * 2048, groups=g, npg=npg,
                chunks=-(-Q // chunk) if Q else 0, cls='NB %d%s' % (NB, ' (N%%16 %d)' % (N % 16) if N % 16 else ''))


def case_line(kind, N, Q, T, groups, off):
    """One line of the case table: N, class, Q, T, groups and path."""
    if kind == 'r':
        g = k2r_geometry(N, Q, T, groups, off)
        extra = 'groups %3d npg %5d ntt %d' % (g['groups'], g['npg'], g['ntt'])
    else:
        g = k2e_geometry(N, Q, T, groups, off)
        extra = 'groups %3d npg %5d' % (g['groups'], g['npg']) if g['path'] == 'kernel' else 'chunks %d' % g['chunks']
    return '%s N %3d  %-38s Q %7d T %3d off %d  %-26s %s' % ('K2r' if kind == 'r' else 'K2e', N, g['cls'], Q, T, off, extra,
                                                            g['path'])


K2R_NS = [4, 12, 16, 18, 27, 32, 36, 50, 75, 81, 100, 125, 128, 144, 147, 150, 180, 196, 216, 256, 288, 289, 300]
K2E_NS = [12, 16, 18, 32, 36, 48, 50, 64, 75, 80, 81, 96, 100, 112, 125, 128, 144, 147, 288]
BIG = 2 ** 17 + 4


def k2r_cases():
    """(N, Q, T, groups, off) of the integer suite for K2r."""
    c = [(N, 260, 65, None, 0) for N in K2R_NS] + [(N, 1028, 17, None, 0) for N in K2R_NS]
    c += [(N, 256, T, None, 0) for N in (18, 147) for T in (1, 15, 16, 17, 63, 64, 65, 129, 300)]
    c += [(27, 256, 3, None, 0), (288, 256, 3, None, 0), (36, 8196, 5, None, 0), (144, 8196, 5, None, 0),
          (216, 8196, 5, None, 0), (81, BIG, 3, None, 0), (288, BIG, 2, None, 0), (50, 2 ** 21, 2, None, 0)]
    c += [(27, 257, 5, None, 0), (27, 258, 5, None, 0), (27, 252, 5, None, 0), (144, 1029, 70, None, 0),    # library shapes
          (144, 1028, 17, None, 1), (18, 1028, 17, None, 1), (144, 1028, 17, None, 4), (18, 1028, 17, None, 4),
          (300, 1028, 65, None, 4)]
    c += [(18, 8196, 17, g, 0) for g in (1, 2, 3, 7, 256)] + [(144, 8196, 65, g, 0) for g in (3, 256)]
    return c


def k2e_cases():
    """(N, Q, T, groups, off) of the integer suite for K2e."""
    c = [(N, 1028, 2, None, 0) for N in K2E_NS] + [(N, 260, 9, None, 0) for N in K2E_NS]
    c += [(50, 258, T, None, 0) for T in (1, 2, 9, 70)]
    c += [(16, 256, 1, None, 0), (144, 8196, 2, None, 0), (36, BIG, 2, None, 0), (288, BIG, 2, None, 0),
          (36, 2 ** 21, 2, None, 0)]
    c += [(32, 1027, 2, None, 0), (32, 1030, 2, None, 0), (32, 250, 3, None, 0), (32, 255, 3, None, 0),
          (48, 1028, 2, None, 1), (48, 1028, 2, None, 2), (147, 1028, 2, None, 2)]
    c += [(81, 8196, 2, g, 0) for g in (1, 2, 3, 7, 256)] + [(144, 8196, 3, g, 0) for g in (2, 8)]
    return c


def test_geometry_list_covers_every_class():
    """The case lists reach every class of the restated launch formulas (no GPU needed)."""
    r = [(N, Q, T, g, o, k2r_geometry(N, Q, T, g, o)) for N, Q, T, g, o in k2r_cases()]
    kr = [x for x in r if x[5]['path'] == 'kernel']
    assert {x[5]['pad'] for x in kr} == {0, 1, 2, 3}                      # padded k-steps
    assert {x[5]['KSp'] // 4 % 2 for x in kr} == {0, 1}                   # the loop's trailing stage or none
    assert {x[0] % 4 for x in kr} == {0, 1, 2, 3}
    assert {x[0] for x in kr} == {N for N in K2R_NS if N <= 288}
    assert k2r_geometry(288, 1028, 1)['shm'] == 144 * 1024 and k2r_geometry(288, 1028, 1)['path'] == 'kernel'
    assert k2r_geometry(289, 1028, 1)['path'] == 'library' and k2r_geometry(300, 1028, 1)['path'] == 'library'
    assert all(k2r_geometry(N, 1028, 1)['path'] == 'kernel' for N in range(1, 289))
    assert {x[5]['groups'] for x in kr} >= {1, 2, 3, 7, 32, 256}
    assert any(x[5]['npg'] % 8 for x in kr if x[5]['groups'] > 1)        # blocks that return at once
    # a last workgroup whose second group of points is empty: Q = 2^17 + 4, groups 2
    assert any(x[1] == BIG and x[5]['groups'] == 2 and (x[1] - 1) % 512 < 256 for x in kr)
    assert {x[2] for x in kr} >= {1, 15, 16, 17, 63, 64, 65, 129, 300}
    assert {x[1] for x in kr} >= {256, 260, 1028, 8196, BIG, 2 ** 21}
    assert all(x[0] <= 144 for x in r if x[1] > BIG)
    lib = [x for x in r if x[5]['path'] == 'library']
    assert any(x[1] % 2 for x in lib) and any(x[1] % 4 == 2 for x in lib) and any(x[1] < 256 for x in lib)
    assert any(x[4] == 1 for x in lib) and any(x[4] == 4 for x in kr) and any(x[0] > 288 for x in lib)
    e = [(N, Q, T, g, o, k2e_geometry(N, Q, T, g, o)) for N, Q, T, g, o in k2e_cases()]
    ke = [x for x in e if x[5]['path'] == 'kernel']
    for NB in range(1, 10):
        ns = {x[0] for x in ke if x[5]['NB'] == NB}
        assert 16 * NB in ns, NB
        if NB < 9:
            assert any(n % 16 for n in ns), NB
    assert {x[5]['groups'] for x in ke} >= {1, 2, 3, 7, 8, 256}
    assert {x[5]['groups'] for x in ke if x[0] == 144} >= {2, 8}             # the setting of tools/perf_eval_resident_err.py
    assert {x[2] for x in ke} >= {1, 2, 9, 70}
    assert any(x[1] % 4 == 2 for x in ke) and any(x[1] < 256 for x in ke) and any(x[4] == 2 for x in ke)
    assert all(x[0] <= 144 for x in e if x[1] > BIG)
    le = [x for x in e if x[5]['path'] == 'library']
    assert any(x[1] % 2 for x in le) and any(x[4] == 1 for x in le) and {147, 288} <= {x[0] for x in le}
    assert any(x[0] == 288 and x[5]['chunks'] == 2 for x in le)               # past the first chunk of 116 508 points
    assert 2 ** 25 // 288 == 116508


# ==== device calls ==========================================================================================================
_MODELS = {}


def _handle(N):
    """A model handle with nbasis N (radial basis functions on a line): the resident calls use only N; Y is uploaded."""
    from volumetricinterp_amd import _lib
    if N not in _MODELS:
        ctx = _lib.get_context()
        cen = np.zeros((N, 3))
        cen[:, 0] = np.arange(N)
        d = _lib.ModelDesc()
        d.kind = _lib.VI_MODEL_RADBASFUN
        d.nbasis = N
        d.centers = cen.ctypes.data_as(_lib.c_double_p)
        d.eps = 1.0
        h = _lib.VOIDP()
        _lib.check(_lib.lib.vi_model_create(ctx.handle, ctypes.byref(d), ctypes.byref(h)), 'vi_model_create')
        _MODELS[N] = (h, cen)
    return _MODELS[N][0]


def run(kind, N, Q, T, Y, M, off=0, h=None):
    """vi_eval_resident_f64 (kind 'r', M = C (T, N)) or vi_eval_resident_err_f64 (kind 'e', M = dC (T, N, N)) on device
    copies: Y and the output `off` doubles past 256-byte aligned bases, the output between GUARD sentinel doubles on either
    side.  Returns (out (T, Q), whether every sentinel is unchanged)."""
    from volumetricinterp_amd import _lib
    ctx = _lib.get_context()
    h = _handle(N) if h is None else h
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    M = np.ascontiguousarray(M, dtype=np.float64)
    bufs = []
    try:
        dY = ctx.empty(max(1, off + N * Q))
        bufs.append(dY)
        if Y.size:
            _lib.check(_lib.lib.vi_h2d(ctx.handle, dY.offset_ptr(off), Y.ctypes.data_as(_lib.VOIDP), Y.nbytes), 'h2d')
        bufs.append(ctx.to_device(M) if M.size else ctx.empty(1))
        dO = ctx.to_device(np.full(2 * GUARD + off + T * Q, SENTINEL))
        bufs.append(dO)
        fn = _lib.lib.vi_eval_resident_f64 if kind == 'r' else _lib.lib.vi_eval_resident_err_f64
        _lib.check(fn(h, Q, T, dY.offset_ptr(off), bufs[1].ptr, dO.offset_ptr(GUARD + off)), 'resident call')
        res = dO.download()
    finally:
        for b in bufs:
            b.free()
    lo, hi = GUARD + off, GUARD + off + T * Q
    sb = np.array([SENTINEL]).view(np.uint64)[0]
    bits = res.view(np.uint64)
    guards = bool(np.all(bits[:lo] == sb) and np.all(bits[hi:] == sb))
    return res[lo:hi].reshape(T, Q), guards


def mismatch(out, ref, what):
    """'' when out equals ref bit for bit (any NaN matches any NaN), else a description of the first difference."""
    same = (out.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(out) & np.isnan(ref))
    if same.all():
        return ''
    bad = np.argwhere(~same)
    t, q = bad[0]
    return '%s: %d of %d differ, first (t %d, q %d): got %r, want %r' % (what, len(bad), same.size, t, q, out[t, q], ref[t, q])


# ==== 2. exact by construction ===============================================================================================
def k2r_integer_inputs(rng, N, Q, T, special=True):
    """|C|, |Y| <= 2^b with N 2^(2b) <= 2^50, mixed signs: every partial sum is an integer below 2^50, exact in any order.
    special: NaN in two point columns of Y (hull-masked points), in one coefficient row and in one single coefficient.
    Returns C, Y and the exact result with its NaNs."""
    b = int((50 - math.log2(N)) // 2)
    C = rng.integers(-2 ** b, 2 ** b + 1, (T, N)).astype(np.float64)
    Y = rng.integers(-2 ** b, 2 ** b + 1, (N, Q), dtype=np.int32).astype(np.float64)
    ref = C @ Y
    if special and Q >= 2 and T >= 2:
        for q in (Q // 2, Q - 1):
            Y[:, q] = np.nan
            ref[:, q] = np.nan
        C[T - 1, N - 1] = np.nan
        ref[T - 1] = np.nan
        if T >= 3:
            C[T // 2] = np.nan
            ref[T // 2] = np.nan
    return C, Y, ref


def k2e_integer_inputs(rng, N, Q, T, special=True):
    """|y|, |dC| <= 2^e with N^2 2^(3e + 1) <= 2^46: the form is exact in any order (K2e's dC_IJ + dC_JI^T included), and a
    change of 1 in it moves the map by at least 2^6 ulp.  Covariances by t % 5: diagonally dominant and asymmetric (positive
    forms), its negation (negative forms: NaN), antisymmetric (forms exactly 0: +0.0), random signs (mixed), asymmetric with a
    larger skew part.  special: NaN point columns of Y and one NaN covariance entry.  Returns dC, Y and the exact map, np.sqrt
    of the exact form: the device's square root is correctly rounded, so no ulp of slack is needed."""
    e = int((45 - 2 * math.log2(N)) // 3)
    Y = rng.integers(-2 ** e, 2 ** e + 1, (N, Q)).astype(np.float64)
    dC = np.empty((T, N, N))
    for t in range(T):
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
    F = np.empty((T, Q))
    for t in range(T):
        F[t] = ((dC[t] @ Y) * Y).sum(0)
    with np.errstate(invalid='ignore'):
        ref = np.sqrt(F)
    if special and Q >= 4:
        for q in (1, Q - 2):
            Y[:, q] = np.nan
            ref[:, q] = np.nan
        if T >= 4:
            dC[3, N // 2, N - 1] = np.nan
            ref[3] = np.nan
    return dC, Y, ref


def integer_suite(setenv, delenv, tag=''):
    """Every case of k2r_cases / k2e_cases with integer inputs, one-hot inputs on the smaller ones, T = 0 and Q = 0: a list of
    failures, empty when every result has NumPy's bits and every sentinel is untouched."""
    fails = []
    rng = np.random.default_rng(2026)
    for kind, cases in (('r', k2r_cases()), ('e', k2e_cases())):
        for N, Q, T, groups, off in cases:
            for n in GROUP_ENV:
                delenv(n)
            if groups is not None:
                setenv(GROUP_ENV[0] if kind == 'r' else GROUP_ENV[1], str(groups))
            line = case_line(kind, N, Q, T, groups, off) + tag
            print(line)
            M, Y, ref = (k2r_integer_inputs if kind == 'r' else k2e_integer_inputs)(rng, N, Q, T)
            out, guards = run(kind, N, Q, T, Y, M, off)
            if not guards:
                fails.append(line + ': a store outside the output')
            m = mismatch(out, ref, line + ' integer')
            if m:
                fails.append(m)
            if kind == 'e':
                z = ref == 0
                if np.any(np.signbit(out[z])):
                    fails.append(line + ': a zero form gives -0.0')
                if not (z.any() or T < 3):
                    fails.append(line + ': no zero form')
            del M, Y, ref, out
            if Q * N <= 300 * 1100:                       # one-hot: each output is one element (or product) of Y
                m = one_hot(kind, N, Q, T, off)
                if m:
                    fails.append(m + tag)
    for n in GROUP_ENV:
        delenv(n)
    for kind in ('r', 'e'):                                # T = 0 and Q = 0 write nothing
        for Q, T in ((1028, 0), (0, 5)):
            M = np.ones((T, 36)) if kind == 'r' else np.ones((T, 36, 36))
            out, guards = run(kind, 36, Q, T, np.ones((36, Q)), M)
            if not guards or out.size:
                fails.append('%s N 36 Q %d T %d: not a no-op%s' % (kind, Q, T, tag))
    return fails


def one_hot(kind, N, Q, T, off):
    """K2r: C[t] = e_n(t), so out[t] = Y[n(t)], with Y[n, q] = 1 + n Q + q naming its element.  K2e: dC[t] = e_i(t) e_k(t)^T,
    so out[t] = sqrt(Y[i(t)] Y[k(t)]).  Returns '' or a readable description of the first wrong element."""
    n_t = (7 * np.arange(T) + 3) % N
    k_t = (5 * np.arange(T) + 1) % N
    Y = 1.0 + np.arange(N)[:, None] * Q + np.arange(Q)[None, :]
    if kind == 'r':
        C = np.zeros((T, N))
        C[np.arange(T), n_t] = 1.0
        out, guards = run('r', N, Q, T, Y, C, off)
        ref = Y[n_t]
    else:
        dC = np.zeros((T, N, N))
        dC[np.arange(T), n_t, k_t] = 1.0
        out, guards = run('e', N, Q, T, Y, dC, off)
        ref = np.sqrt(Y[n_t] * Y[k_t])
    what = '%s one-hot N %d Q %d T %d off %d' % ('K2r' if kind == 'r' else 'K2e', N, Q, T, off)
    if not guards:
        return what + ': a store outside the output'
    m = mismatch(out, ref, what)
    if m:
        t, q = np.argwhere(~(out == ref))[0]
        v = out[t, q] - 1.0
        if kind == 'r':
            m += (' (row %d point %d of Y; wanted row %d point %d)' % (v // Q, v % Q, n_t[t], q)
                  if v == int(v) and 0 <= v < N * Q else ' (not an element of Y)')
        else:
            m += ' (wanted rows %d and %d of Y at point %d)' % (n_t[t], k_t[t], q)
    return m


@gpu
def test_integer_inputs_exact_at_every_geometry(monkeypatch):
    """Every geometry of k2r_cases / k2e_cases gives NumPy's bits on exact integer inputs and touches nothing outside its
    output; NaN point columns, coefficient rows and covariances give NaN exactly there, negative forms NaN, zero forms +0.0."""
    fails = integer_suite(monkeypatch.setenv, lambda n: monkeypatch.delenv(n, raising=False))
    for f in fails:
        print('FAIL ' + f)
    assert not fails, '\n'.join(fails)


def inf_row_cases():
    return ([(N, 1028, 17, 0) for N in K2R_NS] + [(18, 260, 65, 0), (147, 8196, 5, 0), (18, 1028, 17, 1), (50, 1028, 17, 4)])


def infinite_row_suite(tag=''):
    """+-inf in basis row 0: out[t, q] = C[t, 0] Y[0, q] + (a finite sum) is +-inf, or NaN where C[t, 0] == 0, as IEEE
    evaluation of the sum gives it."""
    fails = []
    rng = np.random.default_rng(77)
    for N, Q, T, off in inf_row_cases():
        line = case_line('r', N, Q, T, None, off) + tag
        print(line + '  inf in row 0')
        C, Y, _ = k2r_integer_inputs(rng, N, Q, T, special=False)
        C[1, 0] = 0.0
        Y[0, [0, 5, Q // 3, Q - 1]] = [np.inf, -np.inf, np.inf, -np.inf]
        with np.errstate(invalid='ignore'):
            ref = C[:, 1:] @ Y[1:] + C[:, :1] * Y[:1]
        out, guards = run('r', N, Q, T, Y, C, off)
        m = mismatch(out, ref, line + ' inf in row 0')
        if m or not guards:
            fails.append(m or line + ': a store outside the output')
    return fails


@gpu
def test_k2r_infinite_basis_row():
    """An infinite basis value in row 0 gives +-inf, or NaN against a zero coefficient, at every geometry.  K2r gave NaN at
    every order with padded rows before they were zeroed."""
    fails = infinite_row_suite()
    for f in fails:
        print('FAIL ' + f)
    assert not fails, '\n'.join(fails)


CHILD = '''
import os
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_resident_geometry as g
fails = g.integer_suite(lambda n, v: os.environ.__setitem__(n, v), lambda n: os.environ.pop(n, None), ' [blas]')
fails += g.infinite_row_suite(' [blas]')
for f in fails:
    print('FAIL ' + f)
sys.exit(1 if fails else 0)
'''


@gpu
def test_integer_suite_on_the_library_path(tmp_path):
    """The whole integer suite once more with VINTERP_EVAL_RESIDENT=blas (read once per process: a child process): the
    library's path gives the same exact bits at every shape."""
    script = tmp_path / 'child.py'
    script.write_text(CHILD % (REPO_ROOT, os.path.join(REPO_ROOT, 'tests')))
    env = dict(os.environ)
    for k in GROUP_ENV:
        env.pop(k, None)
    env['VINTERP_EVAL_RESIDENT'] = 'blas'
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, 'blas child: exit %d\n%s\n%s' % (r.returncode, r.stdout[-4000:], r.stderr[-3000:])


# ==== 3. real magnitudes against a high-precision reference ==================================================================
def gamma(n):
    return n * U / (1 - n * U)


def _split(a):
    c = 134217729.0 * a                              # Veltkamp: a = hi + lo with 26 and 27 significant bits
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """p + e == a * b exactly (no overflow or underflow in these data)."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def sum2(x):
    """Sum along the last axis as hi + lo, to within about n u^2 sum |x|: a pairwise tree of error-free additions whose
    errors are summed in floating point."""
    lo = np.zeros(x.shape[:-1])
    while x.shape[-1] > 1:
        if x.shape[-1] % 2:
            x = np.concatenate([x, np.zeros(x.shape[:-1] + (1,))], axis=-1)
        x, e = two_sum(x[..., 0::2], x[..., 1::2])
        lo += e.sum(-1)
    return x[..., 0], lo


def fsum2(rows):
    """The exact sum of each row (math.fsum) as hi + lo."""
    hi = [math.fsum(r) for r in rows]
    lo = [math.fsum(r + [-h]) for r, h in zip(rows, hi)]
    return np.array(hi), np.array(lo)


def eval_reference(C, Y, ts, qs):
    """sum_n C[t, n] Y[n, q] at the samples: math.fsum over the exact products (two_prod) as hi + lo, and sum_n |C Y|."""
    a, b = C[ts], Y[:, qs].T
    p, e = two_prod(a, b)
    hi, lo = fsum2(np.concatenate([p, e], axis=1).tolist())
    return hi, lo, np.abs(a * b).sum(1)


def form_reference(dC, Y, ts, qs):
    """sum_ik Y[i, q] dC[t, i, k] Y[k, q] at the samples as hi + lo, and B0 = sum_ik |y_i| |dC_ik| |y_k|: z = dC y from the
    exact products dC_ik y_k summed by sum2, then y . z by math.fsum over exact products.  Error below 4 N u^2 B0."""
    N = Y.shape[0]
    hi, lo, B0 = np.empty(len(ts)), np.empty(len(ts)), np.empty(len(ts))
    step = max(1, 2 ** 21 // (N * N))
    for t in np.unique(ts):
        idx = np.nonzero(ts == t)[0]
        D = dC[t]
        for s in range(0, len(idx), step):
            j = idx[s:s + step]
            y = Y[:, qs[j]].T                                          # (samples, N)
            p, e = two_prod(D[None, :, :], y[:, None, :])              # dC_ik y_k
            zh, zl = sum2(p)
            zl = zl + e.sum(-1)
            p2, e2 = two_prod(y, zh)
            hi[j], lo[j] = fsum2(np.concatenate([p2, e2, y * zl], axis=1).tolist())
            B0[j] = ((np.abs(y) @ np.abs(D).T) * np.abs(y)).sum(1)
    return hi, lo, B0


def eval_gate(out, hi, lo, absum, N):
    """Per sample: |out - exact| <= gamma_{N+1} sum_n |C_tn Y_nq|."""
    with np.errstate(invalid='ignore'):
        return np.isfinite(out) & (np.abs((out - hi) - lo) <= gamma(N + 1) * absum)


def form_gate(form, hi, lo, B0, N):
    """Per sample: |form - exact| <= gamma_{2N+3} sum_ik |y_i| |dC_ik| |y_k| =: B."""
    return np.abs((form - hi) - lo) <= gamma(2 * N + 3) * B0


def map_gate(m, hi, lo, B0, N):
    """Per sample: where exact > B the map is finite and |map^2 - exact| <= B + 3 u map^2 (map^2 exact on the host); where
    exact < -B it is NaN; in between either."""
    B = gamma(2 * N + 3) * B0
    ok = np.ones(m.shape, dtype=bool)
    pos, neg = hi > B, hi < -B
    ok[neg] = np.isnan(m[neg])
    fin = np.isfinite(m)
    ok[pos & ~fin] = False
    w = np.nonzero(pos & fin)[0]
    if len(w):
        p, e = two_prod(m[w], m[w])
        d = np.array([abs(math.fsum([a, b, -c, -f])) for a, b, c, f in zip(p.tolist(), e.tolist(), hi[w].tolist(),
                                                                           lo[w].tolist())])
        ok[w] = d <= B[w] + 3 * U * p
    return ok


def samples(rng, T, Q, pool, n=2000, edges_q=()):
    """n random (t, q) with q in pool, and every pair of a tile / group / chunk edge of t and one of q (those in pool)."""
    et = sorted({t for t in (0, 1, 15, 16, 63, 64, T - 1) if 0 <= t < T})
    inpool = np.zeros(Q, bool)
    inpool[pool] = True
    eq = sorted({q for q in (0, 1, 2, 3, 4, 5, 31, 32, 255, 256, 257, 511, 512, Q - 5, Q - 4, Q - 3, Q - 2, Q - 1)
                 + tuple(edges_q) if 0 <= q < Q and inpool[q]})
    ts = np.concatenate([rng.integers(0, T, n), np.repeat(et, len(eq))])
    qs = np.concatenate([pool[rng.integers(0, len(pool), n)], np.tile(eq, len(et))]).astype(np.int64)
    return ts, qs


SPH_CFG = ('[DEFAULT]\n[MODEL]\nNAME = sphharmlag\nMAXK = %d\nMAXL = %d\nCAP_LIM = 10\nMAX_Z_INT = INF\nLATCP = 78\n'
           'LONCP = 262\n')
RBF_CFG = ('[DEFAULT]\n[MODEL]\nNAME = radbasfun\nLATCP = 78\nLONCP = 262\nEPS = 100000.0\nLATRANGE = 74,80\n'
           'LONRANGE = 260,285\nALTRANGE = 100,600\nNUMGRIDPNT = %d\n')
REAL = {16: ('sph', 4, 2), 27: 'rbf', 32: 'k8l2', 48: 'scr_k12l2', 125: ('rbf', 5), 144: 'default', 180: ('sph', 5, 6),
        196: ('sph', 4, 7), 288: ('sph', 8, 6)}


def real_estimate(N):
    """An Estimate of order N with the default fixture's hull, and its fixture's (Coeffs, Covariance) or None."""
    from volumetricinterp_amd import synth
    from volumetricinterp_amd.estimate import Estimate
    spec = REAL[N]
    hull = load_golden('fit_default')['hull_vert']
    if isinstance(spec, str):
        f = load_golden('fit_' + spec)
        es = Estimate.from_arrays(f['Coeffs'], f['Covariance'], f['utime'], hull, str(f['cfg']))
        fx = (f['Coeffs'], f['Covariance'])
    else:
        cfg = SPH_CFG % (spec[1], spec[2]) if spec[0] == 'sph' else RBF_CFG % spec[1]
        es = Estimate.from_arrays(np.zeros((1, N)), None, [[0., 60.]], hull, cfg)
        fx = None
    assert es.model.nbasis == N
    return es, fx


def _points(rng, Q):
    return rng.uniform(74, 82, Q), rng.uniform(248, 276, Q), rng.uniform(90e3, 750e3, Q)


def _row_scale(Y):
    s = np.nanmax(np.abs(Y), axis=1)
    s[~(s > 0)] = 1.0
    return s


def real_coeffs(rng, N, Y, fx, T=70):
    """T coefficient rows: the fixture's (to 1e20, heavy cancellation) times random factors, and column-normalised random
    rows, C_tn = r / max_q |Y[n, q]|."""
    C = rng.standard_normal((T, N)) / _row_scale(Y)
    if fx is not None:
        base = np.nan_to_num(fx[0])
        C[:T // 2] = base[rng.integers(0, len(base), T // 2)] * rng.uniform(-3, 3, (T // 2, 1))
    return C


def real_covariances(rng, N, Y, fx):
    """The fixture's covariances (asymmetric, cancelling by six decades) where there are any, then synthetic positive
    definite and indefinite ones with a 10 % skew part, scaled by the basis rows."""
    s = _row_scale(Y)
    out = [np.nan_to_num(c) for c in fx[1]] if fx is not None else []
    for k in range(4):
        R = rng.standard_normal((N, N))
        d = np.ones(N) if k % 2 == 0 else np.where(rng.random(N) < 0.3, -1.0, 1.0)
        M = (R * d) @ R.T / N + 0.1 * rng.standard_normal((N, N)) / math.sqrt(N)
        out.append(M / np.outer(s, s))
    return np.array(out)


def blocks_transposed(dC):
    """Every 16 x 16 block of dC transposed in place: a staging lane map with i and k swapped (transposing the whole of dC
    leaves the form unchanged)."""
    out = dC.copy()
    N = dC.shape[1]
    for I in range(0, N, 16):
        for J in range(0, N, 16):
            n = min(16, N - I, N - J)
            out[:, I:I + n, J:J + n] = np.swapaxes(dC[:, I:I + n, J:J + n], 1, 2)
    return out


@gpu
@pytest.mark.parametrize('N', sorted(REAL))
def test_real_basis_against_exact_reference(N):
    """Real basis matrices (vi_eval_basis_f64, some points outside the hull): K2r and the library's product, K2e and the
    library's form, at >= 2000 samples each against the reference, pointwise, with the hull's NaN pattern.  On the host the
    gates reject the last real k-step dropped and points rotated by one inside a group of 4 (K2r), and one triangle of dC
    mirrored, every 16 x 16 block of dC transposed and rotated points (K2e)."""
    rng = np.random.default_rng(N)
    es, fx = real_estimate(N)
    Q = 4100
    lat, lon, alt = _points(rng, Q)
    h = es.model.handle()
    with es.resident_grid(lat, lon, alt, check_hull=True) as g:
        Y = g.dY.download()
    inside = np.isfinite(Y[0])
    assert 0 < inside.sum() < Q and np.array_equal(np.isfinite(Y), np.broadcast_to(inside, Y.shape))
    pool = np.nonzero(inside)[0]
    C = real_coeffs(rng, N, Y, fx)
    T = C.shape[0]
    ts, qs = samples(rng, T, Q, pool)
    hi, lo, ab = eval_reference(C, Y, ts, qs)
    for off in (0, 1):
        print(case_line('r', N, Q, T, None, off) + '  real, %d samples' % len(ts))
        out, guards = run('r', N, Q, T, Y, C, off, h=h)
        assert guards
        assert np.array_equal(np.isnan(out), np.broadcast_to(~inside, out.shape))
        ok = eval_gate(out[ts, qs], hi, lo, ab, N)
        assert ok.all(), 'K2r off %d: %d samples outside the bound' % (off, (~ok).sum())
    KS = (N + 3) // 4
    Cd = C.copy()
    Cd[:, 4 * (KS - 1):] = 0.0
    assert not eval_gate(eval_reference(Cd, Y, ts, qs)[0], hi, lo, ab, N).all()
    rot = 4 * (qs // 4) + (qs + 1) % 4
    keep = inside[rot]
    assert not eval_gate(out[ts[keep], rot[keep]], hi[keep], lo[keep], ab[keep], N).all()
    # the forms
    dC = real_covariances(rng, N, Y, fx)
    T = len(dC)
    ts, qs = samples(rng, T, Q, pool)
    hi, lo, B0 = form_reference(dC, Y, ts, qs)
    B = gamma(2 * N + 3) * B0
    for off in (0, 1):
        print(case_line('e', N, Q, T, None, off) + '  real, %d samples: %d positive, %d negative beyond the bound' % (
            len(ts), (hi > B).sum(), (hi < -B).sum()))
        out, guards = run('e', N, Q, T, Y, dC, off, h=h)
        assert guards
        assert np.isnan(out[:, ~inside]).all()
        ok = map_gate(out[ts, qs], hi, lo, B0, N)
        assert ok.all(), 'K2e off %d: %d samples outside the bound, first t %d q %d: %r, exact %r, B %r' % (
            off, (~ok).sum(), ts[~ok][0], qs[~ok][0], out[ts, qs][~ok][0], hi[~ok][0], B[~ok][0])
    rot = 4 * (qs // 4) + (qs + 1) % 4
    keep = inside[rot]
    assert not map_gate(out[ts[keep], rot[keep]], hi[keep], lo[keep], B0[keep], N).all()
    if N in (48, 144, 180):
        for name, bad in (('mirrored', np.array([np.triu(d) + np.triu(d, 1).T for d in dC])),
                          ('blocks transposed', blocks_transposed(dC))):
            wh = form_reference(bad, Y, ts, qs)[0]
            assert not form_gate(wh, hi, lo, B0, N).all(), name
            with np.errstate(invalid='ignore'):
                assert not map_gate(np.sqrt(wh), hi, lo, B0, N).all(), name


@gpu
@pytest.mark.parametrize('N', [180, 288])
def test_device_error_over_two_chunks(N):
    """Estimate.error's device call (vi_eval_err_f64) at 65 536 + 1001 points, two chunks of its basis tile: its basis (the
    same vi_basis_f64 in the point-major layout) is the resident basis bit for bit, and its maps and those of the resident
    library path meet the map gate."""
    from volumetricinterp_amd import _lib
    rng = np.random.default_rng(100 + N)
    es, _ = real_estimate(N)
    Q = 65536 + 1001
    lat, lon, alt = _points(rng, Q)
    with es.resident_grid(lat, lon, alt, check_hull=False) as g:
        Y = g.dY.download()
    assert np.array_equal(np.ascontiguousarray(es.model.basis(lat, lon, alt).T).view(np.uint64), Y.view(np.uint64))
    dC = real_covariances(rng, N, Y, None)[:2]
    ts, qs = samples(rng, 2, Q, np.arange(Q), edges_q=(65534, 65535, 65536, 65537))
    hi, lo, B0 = form_reference(dC, Y, ts, qs)
    print(case_line('e', N, Q, 2, None, 0) + '  real, and vi_eval_err_f64')
    res, guards = run('e', N, Q, 2, Y, dC, 0, h=es.model.handle())
    assert guards
    ctx = es.model.ctx
    dev = np.empty((2, Q))
    bufs = [ctx.to_device(a) for a in (lat, lon, alt)]
    try:
        for t in range(2):
            dD, dO = ctx.to_device(dC[t]), ctx.empty(Q)
            _lib.check(_lib.lib.vi_eval_err_f64(es.model.handle(), Q, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, dD.ptr, dO.ptr),
                       'vi_eval_err_f64')
            dev[t] = dO.download()
            dD.free()
            dO.free()
    finally:
        for b in bufs:
            b.free()
    for name, out in (('vi_eval_err_f64', dev), ('vi_eval_resident_err_f64', res)):
        ok = map_gate(out[ts, qs], hi, lo, B0, N)
        assert ok.all(), '%s: %d samples outside the bound' % (name, (~ok).sum())


# ==== 4. slab loops and fused-evaluation dispatch ==========================================================================
@gpu
def test_resident_grid_slab_loops(monkeypatch):
    """evaluate_coeffs / evaluate_errors with the free memory reported so that each call runs in slabs of 7 timesteps (30 =
    4 x 7 + 2): the same bits as in one slab."""
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_k8l2')
    es = Estimate.from_arrays(f['Coeffs'], f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))
    rng = np.random.default_rng(3)
    Q, T, N = 2052, 30, 32
    lat, lon, alt = rng.uniform(75, 81, Q), rng.uniform(250, 274, Q), rng.uniform(100e3, 700e3, Q)
    C = f['Coeffs'][rng.integers(0, len(f['Coeffs']), T)] * rng.uniform(-2, 2, (T, 1))
    dC = f['Covariance'][rng.integers(0, len(f['Covariance']), T)] * rng.uniform(0.5, 2, (T, 1, 1))
    with es.resident_grid(lat, lon, alt) as g:
        one_c, one_e = g.evaluate_coeffs(C), g.evaluate_errors(dC)
        ctx = es.model.ctx
        total = ctx.mem_info()[1]
        monkeypatch.setattr(ctx, 'mem_info', lambda: (4 * 7 * Q * 8 + 100, total))
        sl_c = g.evaluate_coeffs(C)
        monkeypatch.setattr(ctx, 'mem_info', lambda: (4 * 7 * (Q + N * N) * 8 + 100, total))
        sl_e = g.evaluate_errors(dC)
    assert (4 * 7 * Q * 8 + 100) // 4 // (Q * 8) == 7 and (4 * 7 * (Q + N * N) * 8 + 100) // 4 // ((Q + N * N) * 8) == 7
    assert np.isnan(one_c).any() and np.isfinite(one_c).any() and np.isfinite(one_e).any()
    assert np.array_equal(sl_c.view(np.uint64), one_c.view(np.uint64))
    assert np.array_equal(sl_e.view(np.uint64), one_e.view(np.uint64))


@gpu
@pytest.mark.parametrize('maxk,maxl', [(3, 4), (2, 3)])
def test_fast_kernel_orders_vs_oracle(maxk, maxl):
    """VI_FAST(4, 3) (MAXK 3 x MAXL 4) and VI_FAST(3, 2) (MAXK 2 x MAXL 3) at CAP_LIM 10, one degree group: the oracle at
    1e-10 per row, as test_eval_matrix_core_other_orders_vs_oracle requires of the other orders."""
    import oracle
    from volumetricinterp_amd.estimate import Estimate
    N = maxk * maxl * maxl
    rng = np.random.default_rng(11)
    Q, T = 333, 40
    lat, lon, alt = rng.uniform(75, 81, Q), rng.uniform(250, 274, Q), rng.uniform(100e3, 700e3, Q)
    A = oracle.SphHarmLagOracle(maxk=maxk, maxl=maxl, cap_lim_deg=10.).basis(lat, lon, alt)
    assert np.all(np.isfinite(A))
    C = rng.standard_normal((T, N)) / np.maximum(np.abs(A).max(axis=0), 1e-300)
    es = Estimate.from_arrays(C, None, [[0., 60.]] * T, np.zeros((4, 3)), SPH_CFG % (maxk, maxl))
    assert len(es.model.device_tables()['groups']) == 1
    out = es.evaluate_coeffs(C, lat, lon, alt, check_hull=False)
    for t in range(T):
        assert rel(out[t], A @ C[t]) <= 1e-10, t


DISPATCH_ORDERS = {'k8l12': (8, 12, 15.), 'k2l12': (2, 12, 15.), 'k4l6': (4, 6, 10.), 'k8l2': (8, 2, 10.),
                   'k4l3': (4, 3, 10.), 'k3l4': (3, 4, 10.)}
DISPATCH_CHILD = '''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import test_gpu_resident_geometry as g
np.savez(sys.argv[1], **{tag: g.dispatch_eval(tag) for tag in sys.argv[2].split(",")})
'''


def dispatch_eval(tag):
    """Densities of 40 timesteps (two tiles of 16 for the matrix-core kernel, 8 for the VALU kernels) at 1003 points, some
    outside the default fixture's hull, at order `tag` of DISPATCH_ORDERS."""
    from volumetricinterp_amd.estimate import Estimate
    maxk, maxl, cap = DISPATCH_ORDERS[tag]
    N = maxk * maxl * maxl
    cfg = ('[DEFAULT]\n[MODEL]\nNAME = sphharmlag\nMAXK = %d\nMAXL = %d\nCAP_LIM = %g\nMAX_Z_INT = INF\nLATCP = 78\n'
           'LONCP = 262\n' % (maxk, maxl, cap))
    rng = np.random.default_rng(N)
    Q, T = 1003, 40
    lat, lon, alt = _points(rng, Q)
    es = Estimate.from_arrays(np.zeros((1, N)), None, [[0., 60.]], load_golden('fit_default')['hull_vert'], cfg)
    C = rng.standard_normal((T, N)) / _row_scale(es.model.basis(lat, lon, alt).T)
    return es.evaluate_coeffs(C, lat, lon, alt, check_hull=True)


def _dispatch_child(tmp_path, name, env_set, tags):
    script = tmp_path / 'dispatch_child.py'
    script.write_text(DISPATCH_CHILD % (REPO_ROOT, os.path.join(REPO_ROOT, 'tests')))
    env = dict(os.environ)
    for k in ('VINTERP_SPLIT_NH', 'VINTERP_EVAL_SPLIT', 'VINTERP_EVAL_MFMA', 'VINTERP_EVAL'):
        env.pop(k, None)
    env.update(env_set)
    o = str(tmp_path / ('%s.npz' % name))
    r = subprocess.run([sys.executable, str(script), o, ','.join(tags)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, '%s child: exit %d\n%s' % (name, r.returncode, r.stderr[-3000:])
    return dict(np.load(o))


@gpu
def test_dispatch_switches_in_child_processes(tmp_path):
    """VINTERP_SPLIT_NH=2 / 4 (the high-order kernel with its chains in two / four groups), VINTERP_EVAL_SPLIT=0
    (k_eval_sph_fast at MAXL 12) and VINTERP_EVAL_MFMA=0 (the VALU kernels for the matrix-core orders), each against the
    default dispatch of the same order: NaN masks identical, every row within 1e-12."""
    runs = {'default': ({}, list(DISPATCH_ORDERS)),
            'nh2': ({'VINTERP_SPLIT_NH': '2'}, ['k8l12']),
            'nh4': ({'VINTERP_SPLIT_NH': '4'}, ['k8l12']),
            'split0': ({'VINTERP_EVAL_SPLIT': '0'}, ['k8l12', 'k2l12']),
            'mfma0': ({'VINTERP_EVAL_MFMA': '0'}, ['k4l6', 'k8l2', 'k4l3'])}
    res = {name: _dispatch_child(tmp_path, name, env, tags) for name, (env, tags) in runs.items()}
    fails = []
    for name, (env, tags) in runs.items():
        for tag in tags if name != 'default' else ():
            a, b = res[name][tag], res['default'][tag]
            ok = np.isfinite(b)
            worst = max(rel(a[t][ok[t]], b[t][ok[t]]) for t in range(len(b)))
            print('%-7s %-6s worst row rel %.1e, %d of %d points inside' % (name, tag, worst, ok[0].sum(), ok.shape[1]))
            if not np.array_equal(np.isnan(a), np.isnan(b)):
                fails.append('%s %s: NaN masks differ' % (name, tag))
            if not 0 < ok[0].sum() < ok.shape[1]:
                fails.append('%s %s: no point or every point inside the hull' % (name, tag))
            if not worst <= 1e-12:
                fails.append('%s %s: row rel %.1e' % (name, tag, worst))
    assert not fails, '\n'.join(fails)
