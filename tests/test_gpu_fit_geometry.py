"""The stage entries of the fit (csrc/vi_fit.hip, csrc/vi_gemm_device.h) at every launch shape, against answers known by
construction and against error-free references: vi_normal_eq_f64, vi_form_system_f64, vi_chi2_f64, vi_cov_f64,
vi_warm_solve_f64, vi_warm_prepare_f64 / vi_warm_finish_f64, vi_warm_rebase_f64, vi_warm_chi2_one_f64, vi_gcv_terms_f64.
(The two entries of the root finder, vi_brent_warm_f64 and vi_brent_host_one_f64, live in tests/test_gpu_brent_geometry.py,
the forming step of vi_basis_solve_f64, vi_walk_form_f64, in tests/test_gpu_walk_geometry.py.)

The launches are chosen from the sizes alone; the *_geometry functions below restate them:

  normal equations  chunks of Tc = min(2^30 / (8 N P), 65 504) records; k_scale_rows (ceil(P / 256), N, tc) blocks; products in
                    groups of GEMM_GROUP = 32 with the last group padded by repeats of its last entry, whose results go to a
                    scratch area; k_atwb one block per (n, 8 records), 256 threads striding over P, slices of 8 x 65 535 records.
  chi^2             k_chi2_part<256, S>: S = 8 from B = 2048 on (8 N + 256 doubles within 48 KB), 2 from B = 256 on, else 1;
                    ceil(B / S) x nb blocks, nb = ceil(P / 256); k_chi2_sum adds the nb partial sums in order.
  form pair         X = f (D1 + alpha D2): fused in registers while N^2 <= 24 x 1024 (N <= 156), else k_form_pair +
                    k_scale_system<256>.
  wg_gemm           count x 4 <= n_cu and N > 24: "tiled", ceil(ceil(N / 3) / 8)^2 workgroups of 64 threads with 3 x 3 tiles
                    per product; else "whole", one workgroup of min(640, ceil(N / 6)^2 rounded up to 64) threads with 6 x 6
                    tiles, which takes a second pass of its tile loop from N = 151 on.  k panels of 16, LDS panels with the
                    leading dimension N rounded up to 8.
  gcv               k_form_loo one block per left-out point, k_loo_resid four points per block of 256 threads.

Part 1 (no GPU) asserts that the case lists reach every class of these formulas and prints the case table, and shows on
the host that every derived bound of part 3 rejects an emulated wrong answer.  Part 2 uses integer inputs small enough that
every summation order is exact (the bound is stated and asserted per entry), so every result must have NumPy's bits;
one-hot inputs pin the index maps and every output lies between GUARD sentinel doubles.  Part 3 checks real bases with
weights of 1e-22 against references made of error-free products and exact sums (or 80-bit arithmetic where the operation
is a matrix chain), pointwise within derived bounds, and the bits of a record across batch sizes and launch shapes.
Part 4 is the grid limit.

Finding: vi_normal_eq_f64 launched k_scale_rows with gridDim.z = the records of a chunk, and a chunk was bounded by bytes
only (1 GiB of scaled copies): with N P <= 2048 and more than 65 535 records gridDim.z exceeds what a launch takes, and the
call returns the launch error (test_normal_equations_of_70000_small_records; N = 8, P = 64, T = 70 000).  The chunk is now
capped at 65 504 records (whole groups of 32), and k_atwb, whose gridDim.y = ceil(T / 8) has the same limit at T > 524 280,
is launched in slices.  A record's numbers do not depend on the chunk it falls in: the batch-independence tests here and in
test_gpu_configs.py say so."""
import ctypes
import math

import numpy as np
import pytest

from conftest import load_golden
from test_gpu_resident_geometry import GUARD, SENTINEL, U, fsum2, gamma, mismatch, sum2, two_prod, two_sum
from test_gpu_solver_geometry import _n_cu, jacobi_class

gpu = pytest.mark.gpu
EPS = np.finfo(float).eps
LD = np.longdouble

NS = [8, 9, 24, 25, 27, 33, 50, 64, 65, 96, 100, 144, 150, 151, 156, 157, 180, 196]
PS = [40, 255, 256, 257, 550, 2600]
TS = [1, 7, 8, 9, 31, 32, 33, 65, 255, 256, 257, 2047, 2048, 2051]
GEMM_GROUP = 32
GRID_YZ_MAX = 65535
N_CU_REF = 256                       # the CU count the case table is printed for; the GPU tests ask the device


# ==== 1. launch geometry ====================================================================================================
def normal_eq_geometry(N, P, T):
    """vi_normal_eq_f64: the chunk loop, k_scale_rows' grid, the product groups, k_atwb's groups of 8."""
    Tc = min(max(2 ** 30 // (8 * N * P), 1), T, GRID_YZ_MAX // GEMM_GROUP * GEMM_GROUP)
    last = T - (T - 1) // Tc * Tc                        # records of the last chunk
    pcls = '<64' if P < 64 else '<256' if P < 256 else '256k' if P % 256 == 0 else '256k+r'
    return dict(Tc=Tc, chunks=-(-T // Tc), pcls=pcls, t8=T % 8, t32=T % 32, pad=-last % GEMM_GROUP, grid_z=Tc,
                atwb_y=-(-min(T, 8 * GRID_YZ_MAX) // 8),
                cls='P %-6s T%%8 %d T%%32 %2d pad %2d chunks %d' % (pcls, T % 8, T % 32, -last % GEMM_GROUP, -(-T // Tc)))


def chi2_geometry(N, P, B, rec=True):
    """vi_chi2_f64: systems per block S, blocks of 256 points nb, the ragged last block of either kind."""
    S = 8 if B >= 2048 and (8 * N + 256) * 8 <= 48 * 1024 else 2 if B >= 256 else 1
    nb = -(-P // 256)
    return dict(S=S, nb=nb, full_b=B % S == 0, full_p=P % 256 == 0, rec=rec, grid=(-(-B // S), nb),
                cls='S %d %s nb %2d %s rec %s' % (S, 'full  ' if B % S == 0 else 'ragged', nb, 'full  ' if P % 256 == 0 else 'ragged',
                                                 'given' if rec else 'NULL'))


def form_pair_geometry(N):
    """form_pair_scaled: one fused pass while the system fits 24 registers of 1024 threads."""
    NN = N * N
    fused = NN <= 24 * 1024
    return dict(fused=fused, NN=NN, rem=NN % 1024, cls=('fused NN%%1024 %4d' % (NN % 1024)) if fused else 'two kernels')


def wg_gemm_geometry(N, count, n_cu):
    """wg_gemm_batched: the tiled or the whole shape of k_wg_gemm, with the classes of N that its loops distinguish."""
    rems = 'N%%3 %d N%%6 %d N%%8 %d N%%16 %2d' % (N % 3, N % 6, N % 8, N % 16)
    if count * 4 <= n_cu and N > 24:
        nt = (N + 2) // 3
        nb = -(-nt // 8)
        return dict(shape='tiled', nb=nb, grid=(count, nb * nb), threads=64, dead=nt % 8 != 0, part=N % 3 != 0, passes=1,
                    cls='tiled nb %d%s%s  %s' % (nb, ' dead-tiles' if nt % 8 else '', ' part-tile' if N % 3 else '', rems))
    nt = (N + 5) // 6
    threads = min(640, (nt * nt + 63) // 64 * 64)
    passes = -(-nt * nt // threads)
    return dict(shape='whole', nb=0, grid=(count, 1), threads=threads, dead=(nt * nt) % threads != 0, part=N % 6 != 0,
                passes=passes, cls='whole %3d thr %d pass%s  %s' % (threads, passes, 'es' if passes > 1 else '  ', rems))


def gcv_geometry(N, npnt):
    """vi_gcv_terms_f64: k_loo_resid puts four points into a block."""
    return dict(blocks=-(-npnt // 4), rem=npnt % 4, cls='np %d: %d block%s, np%%4 %d' % (npnt, -(-npnt // 4), 's' if npnt > 4 else '',
                                                                                       npnt % 4))


def supported_orders():
    """The orders of the list that the in-LDS solver serves (restated in test_gpu_solver_geometry.jacobi_class and compared
    with the library's own answer by test_library_serves_the_listed_orders)."""
    return [N for N in NS if jacobi_class(N) != 'library']


def normal_eq_cases():
    """(N, P, T): large T only with small N and P."""
    c = [(8, 40, T) for T in TS]
    c += [(9, 255, 33), (24, 256, 31), (25, 257, 65), (33, 550, 9), (64, 40, 32), (65, 256, 7), (96, 255, 8), (100, 257, 1),
          (150, 40, 257), (157, 550, 1), (196, 255, 33), (144, 2600, 7), (144, 2600, 400)]
    return c


def chi2_cases():
    """(N, P, B, rec given)."""
    c = [(9, 40, B, i % 2 == 0) for i, B in enumerate(TS)]
    c += [(8, 256, 256, True), (8, 256, 257, False), (24, 255, 2047, True), (25, 256, 2048, False), (27, 256, 2051, True),
          (33, 257, 2048, True), (50, 550, 1, False), (50, 550, 33, True), (50, 550, 257, False), (50, 550, 2051, False),
          (64, 256, 7, True), (65, 257, 2047, True), (96, 40, 256, True), (100, 255, 9, False), (144, 2600, 7, True),
          (144, 2600, 256, False), (150, 256, 31, False), (151, 257, 8, True), (156, 40, 2048, True), (157, 257, 9, True),
          (180, 255, 65, True), (196, 256, 2048, True), (196, 550, 32, False)]
    return c


def gcv_cases():
    return [(N, k) for N in (27, 50, 144) for k in (1, 2, 3, 4, 5, 9)]


def rebase_counts(n_cu):
    """The two batch sizes of the re-basing tests: 3 products (tiled where N > 24) and the first count past n_cu / 4."""
    return 3, n_cu // 4 + 1


def case_table():
    """One line per case: entry, N, class, sizes, shape."""
    lines = []
    for N, P, T in normal_eq_cases():
        g = normal_eq_geometry(N, P, T)
        lines.append('normal_eq  N %3d  %-44s P %4d T %5d  scale_rows grid (%d, %d, %d), atwb grid (%d, %d)'
                     % (N, g['cls'], P, T, -(-P // 256), N, g['grid_z'], N, g['atwb_y']))
    for N, P, B, rec in chi2_cases():
        g = chi2_geometry(N, P, B, rec)
        lines.append('chi2       N %3d  %-44s P %4d B %5d  grid %r' % (N, g['cls'], P, B, g['grid']))
    for N in supported_orders():
        g = form_pair_geometry(N)
        lines.append('form_pair  N %3d  %-44s NN %5d          %s' % (N, g['cls'], g['NN'], '1024 thr' if g['fused'] else '256 + 256 thr'))
    for N in supported_orders():
        for count in rebase_counts(N_CU_REF):
            g = wg_gemm_geometry(N, count, N_CU_REF)
            lines.append('wg_gemm    N %3d  %-62s count %3d  grid %r x %d thr' % (N, g['cls'], count, g['grid'], g['threads']))
    for N, k in gcv_cases():
        lines.append('gcv        N %3d  %-44s' % (N, gcv_geometry(N, k)['cls']))
    return lines


def test_geometry_list_covers_every_class():
    """The case lists reach every class of the restated launch formulas (no GPU needed); prints the case table."""
    print('\n'.join(case_table()))
    sup = supported_orders()
    assert set(sup) <= set(NS) and {8, 156, 157, 196} <= set(sup)
    # ---- normal equations
    ne = [(N, P, T, normal_eq_geometry(N, P, T)) for N, P, T in normal_eq_cases()]
    assert all(N in NS and P in PS and (T in TS or (N, P, T) == (144, 2600, 400)) for N, P, T, _ in ne)
    assert {g['pcls'] for *_, g in ne} == {'<64', '<256', '256k', '256k+r'}
    assert 0 in {g['t8'] for *_, g in ne} and len({g['t8'] for *_, g in ne}) > 3
    assert {g['t32'] for *_, g in ne} >= {0, 1, 31}
    assert any(T == 1 for _, _, T, _ in ne)
    two = [x for x in ne if x[3]['chunks'] == 2]
    assert two and two[0][:3] == (144, 2600, 400) and two[0][3]['Tc'] == 358 and 2 ** 30 // (144 * 2600 * 8) == 358
    assert all(N * P * T * 8 <= 2 ** 31 for N, P, T, _ in ne)                       # large T only with small N and P
    assert all(g['grid_z'] <= GRID_YZ_MAX and g['atwb_y'] <= GRID_YZ_MAX for *_, g in ne)
    g7 = normal_eq_geometry(8, 64, 70000)                                          # part 4
    assert g7['chunks'] == 2 and g7['Tc'] == 65504 and 70000 * 8 * 64 * 8 < 2 ** 30 and g7['Tc'] % GEMM_GROUP == 0
    assert normal_eq_geometry(8, 64, 600000)['atwb_y'] == GRID_YZ_MAX
    # ---- chi^2
    ch = [(N, P, B, chi2_geometry(N, P, B, r)) for N, P, B, r in chi2_cases()]
    assert all(N in NS and P in PS and B in TS for N, P, B, _ in ch)
    for S in (1, 2, 8):
        mine = [g for *_, g in ch if g['S'] == S]
        assert {g['full_p'] for g in mine} == {True, False}, S
        assert {g['full_b'] for g in mine} == ({True} if S == 1 else {True, False}), S
        assert {g['rec'] for g in mine} == {True, False}, S
        assert {min(g['nb'], 3) for g in mine} == {1, 2, 3}, S
    assert all(N * B <= 2 ** 19 for N, P, B, _ in ch)
    assert chi2_geometry(737, 40, 2048)['S'] == 2 and chi2_geometry(736, 40, 2048)['S'] == 8
    # ---- form pair
    fp = {N: form_pair_geometry(N) for N in sup}
    assert fp[156]['fused'] and fp[156]['NN'] == 24336 and not fp[157]['fused']
    assert not fp[180]['fused'] and not fp[196]['fused']
    assert {g['rem'] == 0 for g in fp.values() if g['fused']} == {True, False}
    assert all(form_pair_geometry(N)['fused'] == (N <= 156) for N in range(1, 300))
    # ---- wg_gemm
    few, many = rebase_counts(N_CU_REF)
    wt = {N: wg_gemm_geometry(N, few, N_CU_REF) for N in sup}
    ww = {N: wg_gemm_geometry(N, many, N_CU_REF) for N in sup}
    assert all(g['shape'] == 'whole' for g in ww.values())
    assert all((g['shape'] == 'tiled') == (N > 24) for N, g in wt.items())
    assert {g['passes'] for g in ww.values()} == {1, 2} and ww[150]['passes'] == 1 and ww[151]['passes'] == 2
    tiled = {N: g for N, g in wt.items() if g['shape'] == 'tiled'}
    assert {g['nb'] for g in tiled.values()} == set(range(2, 10))
    assert {g['dead'] for g in tiled.values()} == {True, False} and {g['part'] for g in tiled.values()} == {True, False}
    for shape in (tiled, ww):
        for m in (3, 6, 8, 16):
            assert {N % m == 0 for N in shape} == {True, False}, m
    assert wg_gemm_geometry(25, N_CU_REF // 4, N_CU_REF)['shape'] == 'tiled' and wg_gemm_geometry(24, 1, N_CU_REF)['shape'] == 'whole'
    # ---- gcv
    gc = [gcv_geometry(N, k) for N, k in gcv_cases()]
    assert {g['rem'] for g in gc} == {0, 1, 2, 3} and any(k == 1 for _, k in gcv_cases()) and {g['blocks'] for g in gc} == {1, 2, 3}


# ==== device calls ==========================================================================================================
def _L():
    from volumetricinterp_amd import _lib, fitengine  # noqa: F401 (registers the signatures of the fit entries)
    return _lib


def _ctx():
    return _L().get_context()


def dev(x, dtype=None):
    return _ctx().to_device(np.ascontiguousarray(x, dtype=dtype))


class Out:
    """A device output of the given shape between GUARD sentinel doubles on either side (init: its first contents)."""

    def __init__(self, shape, init=None):
        self.shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
        self.n = int(np.prod(self.shape))
        host = np.full(2 * GUARD + self.n, SENTINEL)
        if init is not None:
            host[GUARD:GUARD + self.n] = np.asarray(init, np.float64).ravel()
        self.d = dev(host)
        self.ptr = self.d.offset_ptr(GUARD)

    def get(self):
        """The contents; asserts that every sentinel survived."""
        res = self.d.download()
        sb = np.array([SENTINEL]).view(np.uint64)[0]
        bits = res.view(np.uint64)
        assert np.all(bits[:GUARD] == sb) and np.all(bits[GUARD + self.n:] == sb), 'a store outside the output'
        return res[GUARD:GUARD + self.n].reshape(self.shape).copy()


def same(out, ref, what):
    """'' when out has ref's bits, else a description of the first difference (mismatch() wants two dimensions)."""
    out, ref = np.ascontiguousarray(out, np.float64) + 0.0, np.ascontiguousarray(ref, np.float64) + 0.0      # (-0.0 is 0.0 here)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    k = out.shape[-1] if out.ndim > 1 else 1
    return mismatch(out.reshape(-1, k), ref.reshape(-1, k), what)


def call(name, *args):
    """A library entry on the process-wide context; device arrays and Out objects are passed as such (and so stay alive for
    the duration of the call), None is a null pointer."""
    _lib = _L()
    _lib.check(getattr(_lib.lib, name)(_ctx().handle, *[a.ptr if hasattr(a, 'ptr') else a for a in args]), name)


_N_CU = []


def n_cu_of_device():
    """_n_cu() starts a child process: ask once per session."""
    if not _N_CU:
        _N_CU.append(_n_cu())
    return _N_CU[0]


def normal_eq(At, W, b):
    """vi_normal_eq_f64 of a basis At (N, P) and records W, b (T, P): AWA (T, N, N), y (T, N)."""
    N, P = At.shape
    T = W.shape[0]
    dAt, dW, db = dev(At), dev(W), dev(b)
    oA, oy = Out((T, N, N)), Out((T, N))
    call('vi_normal_eq_f64', T, P, N, dAt, dW, db, oA, oy)
    return oA.get(), oy.get()


def chi2(At, C, rec, W, b):
    N, P = At.shape
    B = C.shape[0]
    o = Out((B,))
    drec = dev(rec, np.int32) if rec is not None else None
    call('vi_chi2_f64', B, P, N, dev(At), dev(C), drec, dev(W), dev(b), o)
    return o.get()


def warm_solve(D1, D2, yt, V, slot, alpha):
    """vi_warm_solve_f64: C (B, N) and rank (B,)."""
    N = D1.shape[-1]
    B = len(slot)
    oC, drk = Out((B, N)), _ctx().empty((B,), np.int32)
    call('vi_warm_solve_f64', B, N, dev(D1), dev(D2), dev(yt), dev(V), dev(slot, np.int32), dev(alpha), EPS,
         oC, drk, None)
    return oC.get(), drk.download()


def warm_rebase(AWA, R, y, rec, slot, alpha, V, D1, D2, yt, nplain=0):
    """vi_warm_rebase_f64 on device copies of the slots: C, rank and the slots V, D1, D2, yt as the call leaves them."""
    N = V.shape[-1]
    B = len(slot)
    o = [Out(x.shape, x) for x in (V, D1, D2, yt)]
    oC, drk = Out((B, N)), _ctx().empty((B,), np.int32)
    call('vi_warm_rebase_f64', B, nplain, N, dev(AWA), dev(R), dev(y), dev(rec, np.int32), dev(slot, np.int32),
         dev(alpha), EPS, o[0], o[1], o[2], o[3], oC, drk, None)
    return (oC.get(), drk.download()) + tuple(x.get() for x in o)


def warm_prepare(AWA, R, y, rec, alpha0):
    """vi_warm_prepare_f64: C, rank, V, D1, D2, yt."""
    N = AWA.shape[-1]
    B = len(rec)
    o = [Out((B, N)), Out((B, N, N)), Out((B, N, N)), Out((B, N, N)), Out((B, N))]
    drk = _ctx().empty((B,), np.int32)
    call('vi_warm_prepare_f64', B, N, dev(AWA), dev(rec, np.int32), dev(alpha0), dev(R), dev(y), EPS, o[0],
         drk, o[1], o[2], o[3], o[4])
    return (o[0].get(), drk.download()) + tuple(x.get() for x in o[1:])


@gpu
def test_library_serves_the_listed_orders():
    """Ask the library which orders the in-LDS solver serves: vi_warm_solve_f64 refuses the others before it touches the
    device.  Every order of the list is served, and the restated range is the library's."""
    _lib = _L()
    ctx = _ctx()
    for N in NS + [7, 197]:
        z, zi = ctx.zeros((N * N,)), ctx.zeros((1,), np.int32)
        one, C = dev(np.ones(1)), ctx.empty((N,))
        rc = _lib.lib.vi_warm_solve_f64(ctx.handle, 1, N, z.ptr, z.ptr, z.ptr, z.ptr, zi.ptr, one.ptr, EPS, C.ptr, None, None)
        assert (rc == 0) == (jacobi_class(N) != 'library'), (N, rc)
        ctx.sync()
    assert supported_orders() == NS


# ==== 2. exact by construction ===============================================================================================
def normal_eq_integer_inputs(rng, N, P, T):
    """At in -2..2, W in 0..3 with whole points of weight zero in every record (dropped data), b in -3..3: every term of AWA is
    at most 12 and of y at most 18 in magnitude, so every partial sum in any order is an integer below 18 P < 2^53."""
    At = rng.integers(-2, 3, (N, P)).astype(np.float64)
    W = rng.integers(0, 4, (T, P)).astype(np.float64)
    W[:, rng.integers(0, P, max(1, P // 7))] = 0.0
    if T > 2:
        W[1] = 0.0                                       # a record without data
    b = rng.integers(-3, 4, (T, P)).astype(np.float64)
    assert 18 * P < 2 ** 53
    return At, W, b


def normal_eq_exact(At, W, b, ts=None):
    """AWA of the records ts (all by default) and y of all records: float64 products of integers whose every partial sum is
    below 2^53, hence NumPy's integer arithmetic whatever order its library sums in."""
    ts = np.arange(W.shape[0]) if ts is None else np.asarray(ts)
    AWA = np.empty((len(ts), At.shape[0], At.shape[0]))
    for j, t in enumerate(ts):
        AWA[j] = (At * W[t]) @ At.T
    return AWA, (W * b) @ At.T


@gpu
def test_normal_equations_integer_at_every_shape():
    """AWA and y of integer records have NumPy's bits at every (N, P, T) of the list - ragged groups of 8 and 32, P below and
    across 256, two chunks - and one-hot weights pin the index maps: W[t] = e_p(t) gives AWA[t] = a_p a_p^T, y[t] = b a_p."""
    rng = np.random.default_rng(2027)
    fails = []
    for N, P, T in normal_eq_cases():
        g = normal_eq_geometry(N, P, T)
        line = 'normal_eq N %d P %d T %d (%s)' % (N, P, T, g['cls'])
        print(line)
        At, W, b = normal_eq_integer_inputs(rng, N, P, T)
        AWA, y = normal_eq(At, W, b)
        if g['chunks'] == 1 or T <= 64:
            ts = np.arange(T)
        else:                                            # the chunk edge in full, every record through a contraction
            ts = np.unique([0, 1, 31, 32, g['Tc'] - 1, g['Tc'], g['Tc'] + 1, g['Tc'] + 31, g['Tc'] + 32, T - 2, T - 1])
            u = rng.integers(-1, 2, N).astype(np.float64)
            q = np.einsum('n,tnm,m->t', u, AWA, u)                             # < 2^53: |entries| <= 12 P
            fails.append(same(q, ((u @ At) ** 2 * W).sum(1), line + ' u^T AWA u'))
        ra, ry = normal_eq_exact(At, W, b, ts)
        fails += [same(AWA[ts], ra, line + ' AWA'), same(y, ry, line + ' y')]
        if N * P * T <= 2 ** 22:                         # one-hot
            At1 = 1.0 + np.arange(N * P, dtype=np.float64).reshape(N, P)
            assert (N * P) ** 2 * 3 < 2 ** 53
            pt = (7 * np.arange(T) + 3) % P
            W1 = np.zeros((T, P))
            W1[np.arange(T), pt] = 1.0 + np.arange(T) % 3
            b1 = np.full((T, P), 2.0)
            AWA1, y1 = normal_eq(At1, W1, b1)
            a = At1[:, pt].T                                                   # (T, N)
            w = W1[np.arange(T), pt]
            fails += [same(AWA1, a[:, :, None] * a[:, None, :] * w[:, None, None], line + ' one-hot AWA'),
                      same(y1, 2.0 * w[:, None] * a, line + ' one-hot y')]
    fails = [f for f in fails if f]
    assert not fails, '\n'.join(fails)


def real_records(rng, N, P, T):
    """A basis with columns over six decades, weights around 1e-22 with dropped points, data around 1e11."""
    At = rng.standard_normal((N, P)) * 10.0 ** rng.uniform(-3, 3, (N, 1))
    W = (0.05 * rng.uniform(0.5, 50.0, (T, P)) * 1e11 + 1e10) ** -2.0
    W[:, rng.integers(0, P, max(1, P // 9))] = 0.0
    b = rng.standard_normal((T, P)) * 1e11
    return At, W, b


@gpu
@pytest.mark.parametrize('N,P', [(8, 40), (50, 257), (144, 2600), (157, 550)])
def test_normal_equations_do_not_depend_on_the_batch(N, P):
    """Record r's AWA[r] and y[r] are the same bits alone, as the last of 7, 33 and 65 records, and at positions 0 and 31 of
    a product group - for integer data (where anything else would be wrong arithmetic) and for real data, where it is the
    claim above GEMM_GROUP: the padded last group runs the kernel the full groups run."""
    rng = np.random.default_rng(N)
    for kind in ('integer', 'real'):
        At, W, b = (normal_eq_integer_inputs if kind == 'integer' else real_records)(rng, N, P, 65)
        A1, y1 = normal_eq(At, W[64:], b[64:])
        assert np.all(np.isfinite(A1)) and np.any(A1 != 0)
        for T, pos in ((7, 6), (33, 32), (65, 64), (32, 0), (32, 31), (65, 31), (65, 32)):
            Wt, bt = W[:T].copy(), b[:T].copy()
            Wt[pos], bt[pos] = W[64], b[64]
            At_, yt_ = normal_eq(At, Wt, bt)
            m = same(At_[pos], A1[0], '%s N %d P %d: AWA of a record at %d of %d' % (kind, N, P, pos, T)) or \
                same(yt_[pos], y1[0], '%s N %d P %d: y of a record at %d of %d' % (kind, N, P, pos, T))
            assert not m, m


@gpu
def test_form_system_integer():
    """vi_form_system_f64: X[i] = AWA[rec[i]] + alpha[i] R with rec NULL and a permutation with repeats, alpha a power of two
    times a small integer, a second penalty term accumulated (AWA NULL), and R NULL (a gather).  |AWA| <= 1000, |R| <= 8,
    alpha = k 2^e with k <= 5, -2 <= e <= 3: every result is a multiple of 1/4 below 2^11, so each fma is exact."""
    rng = np.random.default_rng(5)
    for N in (8, 9, 65, 157):
        T, B = 5, 9
        AWA = rng.integers(-1000, 1001, (T, N, N)).astype(np.float64)
        R = rng.integers(-8, 9, (N, N)).astype(np.float64)
        R2 = rng.integers(-8, 9, (N, N)).astype(np.float64)
        alpha = rng.integers(1, 6, B) * 2.0 ** rng.integers(-2, 4, B)
        alpha2 = rng.integers(1, 6, B) * 2.0 ** rng.integers(-2, 4, B)
        rec = np.array([4, 0, 0, 2, 3, 1, 4, 4, 2], np.int32)
        dA, dR, dR2, da, da2, drec = dev(AWA), dev(R), dev(R2), dev(alpha), dev(alpha2), dev(rec)
        assert 1000 + 2 * 40 * 8 < 2 ** 11
        o = Out((B, N, N))
        call('vi_form_system_f64', B, N, dA, drec, da, dR, o)
        ref = AWA[rec] + alpha[:, None, None] * R
        assert not same(o.get(), ref, 'form_system N %d rec' % N)
        call('vi_form_system_f64', B, N, None, None, da2, dR2, o)            # accumulate: rec is not used
        ref2 = ref + alpha2[:, None, None] * R2
        assert not same(o.get(), ref2, 'form_system N %d accumulate' % N)
        o = Out((T, N, N))
        call('vi_form_system_f64', T, N, dA, None, da, dR, o)
        assert not same(o.get(), AWA + alpha[:T, None, None] * R, 'form_system N %d rec NULL' % N)
        o = Out((B, N, N))
        call('vi_form_system_f64', B, N, dA, drec, None, None, o)
        assert not same(o.get(), AWA[rec], 'form_system N %d R NULL' % N)


def chi2_integer_inputs(rng, N, P, B, rec):
    """C, At in -2..2, b in -3..3, W in 0..3: a model value is at most 4 N, a term at most 3 (4 N + 3)^2 < 2^21, chi^2 below
    2^21 P < 2^53 in any order."""
    assert 3 * (4 * N + 3) ** 2 * P < 2 ** 53
    T = 5 if rec else B
    At = rng.integers(-2, 3, (N, P)).astype(np.float64)
    C = rng.integers(-2, 3, (B, N)).astype(np.float64)
    W = rng.integers(0, 4, (T, P)).astype(np.float64)
    b = rng.integers(-3, 4, (T, P)).astype(np.float64)
    r = rng.integers(0, T, B).astype(np.int32) if rec else None
    return At, C, r, W, b


@gpu
def test_chi2_integer_at_every_shape():
    """vi_chi2_f64 has NumPy's bits at every class of chi2_geometry: S = 1, 2, 8 with full and ragged last blocks of systems
    and of points, one, two and several blocks of points, records given and NULL; a one-hot coefficient vector names the basis
    row it reads."""
    rng = np.random.default_rng(11)
    fails = []
    for N, P, B, rec in chi2_cases():
        line = 'chi2 N %d P %d B %d (%s)' % (N, P, B, chi2_geometry(N, P, B, rec)['cls'])
        print(line)
        At, C, r, W, b = chi2_integer_inputs(rng, N, P, B, rec)
        rr = r if rec else np.arange(B)
        fails.append(same(chi2(At, C, r, W, b), (((C @ At) - b[rr]) ** 2 * W[rr]).sum(1), line))
        # one-hot: C[i] = e_n(i), W = e_p(i) per record, b = 0: chi^2 = At[n(i), p(i)]^2
        At1 = 1.0 + np.arange(N * P, dtype=np.float64).reshape(N, P)
        n_i, p_i = (7 * np.arange(B) + 3) % N, (5 * np.arange(B) + 1) % P
        C1 = np.zeros((B, N))
        C1[np.arange(B), n_i] = 1.0
        W1 = np.zeros((B, P))
        W1[np.arange(B), p_i] = 1.0
        perm = rng.permutation(B).astype(np.int32) if rec else None
        Wd = W1 if perm is None else W1[np.argsort(perm)]                 # record perm[i] holds system i's weights
        fails.append(same(chi2(At1, C1, perm, Wd, np.zeros((B, P))), At1[n_i, p_i] ** 2, line + ' one-hot'))
    fails = [f for f in fails if f]
    assert not fails, '\n'.join(fails)


@gpu
@pytest.mark.parametrize('N,P', [(9, 40), (50, 550), (157, 257), (196, 256)])
def test_chi2_of_a_system_is_the_same_bits_in_every_batch(N, P):
    """One system (real data) gives the same chi^2 through S = 1, 2 and 8, at the first and at the last position of the batch,
    last positions in ragged blocks included: the extension of test_chi2_kernel_has_one_summation_order to other shapes."""
    rng = np.random.default_rng(N + P)
    At, W, b = real_records(rng, N, P, 3)
    C0 = rng.standard_normal(N) * 1e11 / (np.abs(At).sum(1) + 1.0)
    vals = []
    for B in (1, 7, 256, 257, 2048, 2051):
        for pos in {0, B - 1}:
            C = rng.standard_normal((B, N)) * np.abs(C0)
            C[pos] = C0
            rec = rng.integers(0, 3, B).astype(np.int32)
            rec[pos] = 2
            out = chi2(At, C, rec, W, b)
            assert np.all(np.isfinite(out))
            vals.append(out[pos])
    assert all(v == vals[0] for v in vals), vals


@gpu
def test_covariance_integer():
    """vi_cov_f64: dC = H AWA H for integer symmetric H and AWA in -4..4 (entries of the result below 16 N^2 4 < 2^53) at
    T in {1, 3, 33} and N in {9, 50, 144}; H = I and AWA = I pin the index maps."""
    rng = np.random.default_rng(3)
    for N in (9, 50, 144):
        assert 64 * N * N < 2 ** 53
        for T in (1, 3, 33):
            H = rng.integers(-4, 5, (T, N, N))
            A = rng.integers(-4, 5, (T, N, N))
            H, A = (H + H.transpose(0, 2, 1)) // 2, (A + A.transpose(0, 2, 1)) // 2
            H[0], A[T - 1] = np.eye(N), np.eye(N)
            o = Out((T, N, N))
            call('vi_cov_f64', T, N, dev(H, np.float64), dev(A, np.float64), o)
            m = same(o.get(), (H @ A @ H).astype(np.float64), 'cov N %d T %d' % (N, T))
            assert not m, m


SCALES = [-70, -33, 0, 17, 40, None]                    # per-slot power of two (None: the all-zero system)


def diagonal_slots(rng, N, scales):
    """Rotated systems in which X(alpha) = D1 + alpha D2 is diagonal with powers of two (or zeros) on its diagonal, so that
    the solve makes no rotation and every division is exact.  Per slot s with scale 2^e and alpha_s in {1, 3}, element j has
    mu = +-2^(k + e), 0 <= k <= 30, and one of three kinds: d1 = d2 = mu (lambda = (1 + alpha) mu), d1 = mu and d2 = 0
    (lambda = mu), d1 = 3 mu and d2 = -mu (lambda = 2 mu at alpha = 1, exactly 0 at alpha = 3).  Element 0 is the largest
    (k = 30) and two elements have k = -40: they fall under the truncation cut eps max|lambda| by 2^-16 at least, every other
    non-zero one stays above it by 2^20.  yt: non-zero integers.  V: a signed permutation, row k = basis vector k = s_k e_pi(k).
    Returns D1, D2, yt, V, alpha_s, and per slot the exact solution C and rank."""
    ns = len(scales)
    D1, D2, V = np.zeros((ns, N, N)), np.zeros((ns, N, N)), np.zeros((ns, N, N))
    yt = (rng.integers(1, 9, (ns, N)) * rng.choice([-1, 1], (ns, N))).astype(np.float64)
    alpha = np.where(np.arange(ns) % 2 == 0, 1.0, 3.0)
    C, rank = np.zeros((ns, N)), np.zeros(ns, np.int32)
    j = np.arange(N)
    for s, e in enumerate(scales):
        k = rng.integers(0, 31, N)
        kind = rng.integers(0, 3, N)
        k[0], kind[0] = 30, 1
        k[[N // 2, N - 1]] = -40
        mu = rng.choice([-1.0, 1.0], N) * 2.0 ** (k + (0 if e is None else e)) * (0.0 if e is None else 1.0)
        d1 = np.where(kind == 2, 3.0 * mu, mu)
        d2 = np.where(kind == 0, mu, np.where(kind == 1, 0.0, -mu))
        D1[s, j, j], D2[s, j, j] = d1, d2
        lam = d1 + alpha[s] * d2
        assert np.all((lam == 0) | (np.frexp(lam)[0] == 0.5) | (np.frexp(lam)[0] == -0.5))          # powers of two
        keep = np.abs(lam) > EPS * np.abs(lam).max()
        assert not np.any(np.abs(np.abs(lam) / max(np.abs(lam).max(), 1e-300) - EPS) < EPS / 2)       # nothing at the cut
        cp = np.where(keep, yt[s] / np.where(keep, lam, 1.0), 0.0)
        pi, sg = rng.permutation(N), rng.choice([-1.0, 1.0], N)
        V[s, j, pi] = sg
        C[s, pi] = sg * cp
        rank[s] = keep.sum()
        assert (e is None) == (rank[s] == 0) and (e is None or 2 <= N - rank[s])
    return D1, D2, yt, V, alpha, C, rank


@gpu
@pytest.mark.parametrize('N', NS)
def test_warm_solve_of_diagonal_systems_is_exact(N):
    """vi_warm_solve_f64 through the fused forming pass (N <= 156) and the two-kernel one (N >= 157): diagonal systems with
    scales from 2^-70 to 2^40 and one all-zero system (f = 1) across the batch, slots listed with repeats and out of order.
    C = V (yt / diag) and rank must be exact: forming, the per-system power of two, the truncation cut and k_v_vec."""
    rng = np.random.default_rng(N)
    D1, D2, yt, V, al, C, rank = diagonal_slots(rng, N, SCALES)
    slot = np.array([2, 0, 5, 3, 1, 2, 4, 5, 0], np.int32)
    out, rk = warm_solve(D1, D2, yt, V, slot, al[slot])
    print('warm_solve N %d (%s)' % (N, form_pair_geometry(N)['cls']))
    m = same(out, C[slot], 'warm_solve N %d C' % N)
    assert not m, m
    assert np.array_equal(rk, rank[slot]), (N, rk, rank[slot])


def rebase_integer_case(N, count, nplain, seed):
    """Diagonal slots (no rotation: the log is empty and Vw = I) with integer bases V in -2..2, and integer AWA, R in -3..3
    (not symmetric: a transposed product would show) and y in -4..4: V_new = V, D1 = V AWA V^T, D2 = V R V^T (row k of V =
    basis vector k), yt = V y, every partial sum an integer below 12 N^2 < 2^53.  Returns a list of failures."""
    assert 12 * N * N < 2 ** 53
    rng = np.random.default_rng(seed)
    B = count + nplain
    ns, T = B + 2, 4
    D1, D2, yt, _, al, _, _ = diagonal_slots(rng, N, [SCALES[i % len(SCALES)] for i in range(ns)])
    V = rng.integers(-2, 3, (ns, N, N)).astype(np.float64)
    AWA = rng.integers(-3, 4, (T, N, N)).astype(np.float64)
    R = rng.integers(-3, 4, (N, N)).astype(np.float64)
    y = rng.integers(-4, 5, (T, N)).astype(np.float64)
    slot = rng.permutation(ns)[:B].astype(np.int32)
    rec = rng.integers(0, T, B).astype(np.int32)
    Cw, rkw = warm_solve(D1, D2, yt, V, slot, al[slot])
    C, rk, Vn, D1n, D2n, ytn = warm_rebase(AWA, R, y, rec, slot, al[slot], V, D1, D2, yt, nplain)
    tag = 'rebase N %d count %d nplain %d' % (N, count, nplain)
    eV, e1, e2, ey = V.copy(), D1.copy(), D2.copy(), yt.copy()
    for i in range(nplain, B):
        s, t = slot[i], rec[i]
        e1[s], e2[s], ey[s] = V[s] @ AWA[t] @ V[s].T, V[s] @ R @ V[s].T, V[s] @ y[t]
    fails = [same(C, Cw, tag + ' C against vi_warm_solve_f64'), same(Vn, eV, tag + ' V'), same(D1n, e1, tag + ' D1'),
             same(D2n, e2, tag + ' D2'), same(ytn, ey, tag + ' yt')]
    if not np.array_equal(rk, rkw):
        fails.append(tag + ' rank')
    return [f for f in fails if f]


@gpu
@pytest.mark.parametrize('N', NS)
def test_rebase_of_diagonal_systems_is_exact(N):
    """vi_warm_rebase_f64 where the rotation log is empty: the four wg_gemm products (V_old Vw, AWA V, V^T (AWA V), R V,
    V^T (R V): plain and transposed), k_scatter_mat, k_form_system without R and k_vt_vec_slot in the tiled shape (3 products)
    and the whole one (n_cu / 4 + 1 products), with and without a plain warm solve riding along, whose slot must stay as it
    is - as must every slot that is not listed.  If the solver rotated here, V would change and this test would say so."""
    n_cu = n_cu_of_device()
    fails = []
    for count in rebase_counts(n_cu):
        print('rebase N %d: %s' % (N, wg_gemm_geometry(N, count, n_cu)['cls']))
        assert wg_gemm_geometry(N, count, n_cu)['shape'] == ('tiled' if count == 3 and N > 24 else 'whole')
        for nplain in (0, 1):
            fails += rebase_integer_case(N, count, nplain, 100 * N + count + nplain)
    assert not fails, '\n'.join(fails)


# ==== 3. real data against error-free references ============================================================================
def awa_reference(At, W, b, t, pairs):
    """Record t at the element pairs (n, m): sum_p A_np W_p A_mp as hi + lo - the three-fold products are exact (two_prod
    twice: A_mp W_p = h + e, then A_np h and A_np e), the sum is math.fsum's - and sum_p |A_np W_p A_mp|."""
    n, m = pairs[:, 0], pairs[:, 1]
    h, e = two_prod(At[m], W[t][None, :])
    p1, e1 = two_prod(At[n], h)
    p2, e2 = two_prod(At[n], e)
    hi, lo = fsum2(np.concatenate([p1, e1, p2, e2], axis=1).tolist())
    return hi, lo, np.abs(At[n] * h).sum(1)


def y_reference(At, W, b, t):
    """y[t] = sum_p A_np W_p b_p for every n as hi + lo, and sum_p |A_np W_p b_p|."""
    h, e = two_prod(W[t], b[t])
    p1, e1 = two_prod(At, h[None, :])
    p2, e2 = two_prod(At, e[None, :])
    hi, lo = fsum2(np.concatenate([p1, e1, p2, e2], axis=1).tolist())
    return hi, lo, np.abs(At * h[None, :]).sum(1)


def sum_gate(out, hi, lo, absum, P):
    """|out - exact| <= gamma(P + 2) sum |terms|: one rounding of W a (or W b), then P terms summed in any order, fused
    or not (gamma(P + 1) covers it; P + 2 is the bound the suite was asked to hold)."""
    return np.isfinite(out) & (np.abs((out - hi) - lo) <= gamma(P + 2) * absum)


def sample_pairs(rng, N, n=300):
    edge = [(0, 0), (N - 1, N - 1), (0, N - 1), (N - 1, 0), (N // 2, N // 2), (1, 0)]
    return np.concatenate([np.array(edge), rng.integers(0, N, (n, 2))])


def chi2_reference(At, C, W, b):
    """chi^2 = sum_p W_p (sum_n A_np C_n - b_p)^2 of one system and the bound on what k_chi2_part + k_chi2_sum may return.
    The model value m_p is exact as hi + lo (two_prod, math.fsum), d_p = m_p - b_p by two_sum, and the sum of W d^2 runs in
    80-bit arithmetic (P positive terms: relative error below P 2^-63, 2^-10 of one ulp of the result).
    The kernel: m_p is ONE fma chain over n, |m^ - m| <= gamma(N) s_p with s_p = sum_n |A_np C_n|; d^ = fl(m^ - b), so
    |d^ - d| <= e_p = gamma(N) s_p (1 + u) + u |d_p|; |d^^2 - d^2| <= E_p = e_p (2 |d_p| + e_p); the term W d^ d^ takes two
    roundings, the tree over 256 points eight, k_chi2_sum nb - 1: |chi2^ - chi2| <= sum_p W_p (E_p + gamma(10 + nb) (d_p^2 +
    E_p))."""
    N, P = At.shape
    nb = -(-P // 256)
    p, e = two_prod(At.T, C[None, :])
    mh, ml = fsum2(np.concatenate([p, e], axis=1).tolist())
    dh, dl = two_sum(mh, -b)
    d = dh.astype(LD) + (dl.astype(LD) + ml.astype(LD))
    ref = np.sum(W.astype(LD) * d * d)
    s = np.abs(At.T * C[None, :]).sum(1)
    ad = np.abs(d).astype(np.float64)
    ep = gamma(N) * s * (1 + U) + U * ad
    E = ep * (2 * ad + ep)
    bound = float(np.sum(W * (E + gamma(10 + nb) * (ad * ad + E))))
    return ref, bound


def chi2_gate(out, ref, bound):
    return bool(np.isfinite(out) and abs(LD(out) - ref) <= LD(bound))


def chain_reference(V, M):
    """V M V^T (row k of V = basis vector k) in 80-bit arithmetic - its own error is 2^-11 of the bound - and the bound of
    the chain of two float64 products that forms it: T = fl(M V^T), |T - M V^T| <= gamma(N) |M| |V|^T, then fl(V T):
    (2 gamma(N) + gamma(N)^2) |V| |M| |V|^T, whatever the order of the sums."""
    N = V.shape[0]
    assert np.finfo(LD).eps <= 2.0 ** -63
    Vl = V.astype(LD)
    ref = Vl @ (M.astype(LD) @ Vl.T)
    g = gamma(N)
    return ref, (2 * g + g * g) * (np.abs(V) @ np.abs(M) @ np.abs(V).T)


def chain_gate(D, V, M):
    ref, bound = chain_reference(V, M)
    return np.isfinite(D) & (np.abs(D.astype(LD) - ref) <= bound.astype(LD))


def vec_gate(yt, V, y):
    """yt = V y, one dot product per element: |yt^ - yt| <= gamma(N) |V| |y|."""
    ref = V.astype(LD) @ y.astype(LD)
    return np.isfinite(yt) & (np.abs(yt.astype(LD) - ref) <= (gamma(V.shape[0]) * (np.abs(V) @ np.abs(y))).astype(LD))


def orth_defect(V):
    return float(np.max(np.abs(V @ V.T - np.eye(V.shape[0]))))


def test_bounds_reject_emulated_wrong_answers():
    """On the host, with the fixture basis of fit_k8l2 (550 points, N = 32) and synthetic records: NumPy's float64 results
    pass every gate of part 3, and each gate rejects an emulated fault - one term of a sum dropped, the result of the
    neighbouring record (a padded group's output stored in a real slot), the last block of points dropped from chi^2, one
    basis row skipped, one k panel of 16 skipped in a product of the chain, a transposed factor."""
    from volumetricinterp_amd import synth
    rng = np.random.default_rng(1)
    A = load_golden('fit_k8l2')['rec0_A']
    P, N = A.shape
    At = np.ascontiguousarray(A.T)
    b, err = synth.synth_records(A, 3, seed0=50)
    W = err ** -2.0
    assert 1e-24 < W.max() < 1e-19
    pairs = sample_pairs(rng, N)
    AWA = np.array([(At * W[t]) @ At.T for t in range(3)])
    y = (W * b) @ At.T
    hi, lo, ab = awa_reference(At, W, b, 1, pairs)
    out = AWA[1][pairs[:, 0], pairs[:, 1]]
    assert sum_gate(out, hi, lo, ab, P).all()
    p0 = int(np.argmax(W[1] > 0))                                         # one term dropped
    drop = out - At[pairs[:, 0], p0] * W[1, p0] * At[pairs[:, 1], p0]
    assert not sum_gate(drop, hi, lo, ab, P).all()
    assert not sum_gate(AWA[2][pairs[:, 0], pairs[:, 1]], hi, lo, ab, P).any()           # the next record's result
    yh, yl, yab = y_reference(At, W, b, 1)
    assert sum_gate(y[1], yh, yl, yab, P).all()
    assert not sum_gate(y[1] - At[:, p0] * W[1, p0] * b[1, p0], yh, yl, yab, P).all() and not sum_gate(y[2], yh, yl, yab, P).all()
    # chi^2
    C = np.linalg.lstsq(A * np.sqrt(W[1])[:, None], b[1] * np.sqrt(W[1]), rcond=None)[0]
    ref, bound = chi2_reference(At, C, W[1], b[1])
    d = A @ C - b[1]
    assert chi2_gate(float(np.sum(d * d * W[1])), ref, bound)
    assert bound < 1e-6 * float(ref)                                     # the gate is not vacuous
    assert not chi2_gate(float(np.sum((d * d * W[1])[:512])), ref, bound)               # the last block of points dropped
    d1 = A[:, :-1] @ C[:-1] - b[1]
    assert not chi2_gate(float(np.sum(d1 * d1 * W[1])), ref, bound)                     # the last basis row skipped
    # the chain V M V^T
    V = np.linalg.qr(rng.standard_normal((N, N)))[0]
    M = AWA[1]
    D = V @ (M @ V.T)
    assert chain_gate(D, V, M).all() and vec_gate(V @ y[1], V, y[1]).all()
    Vz = V.copy()
    Vz[:, 16:32] = 0.0                                                                  # k panel 16 .. 31 of the first product
    assert not chain_gate(V @ (M @ Vz.T), V, M).all()
    As = rng.standard_normal((N, N)) * np.abs(M)                                        # not symmetric: a transposed factor
    assert chain_gate(V @ (As @ V.T), V, As).all() and not chain_gate(V @ (As.T @ V.T), V, As).all()
    assert not vec_gate(V.T @ y[1], V, y[1]).all()


_PROBLEMS = {}


def _curvature_like(N, scale):
    """A symmetric positive semi-definite penalty for orders without a fixture: squared second differences."""
    D = np.zeros((N - 2, N))
    i = np.arange(N - 2)
    D[i, i], D[i, i + 1], D[i, i + 2] = 1.0, -2.0, 1.0
    return scale * (D.T @ D)


def problem(name):
    """Real fit problems: 'k8l2' (the fixture basis rec0_A, N = 32, P = 550), 'c144' (CFG144 on GEOM_C2, N = 144, P = 2600,
    the fixture's curvature matrix), 'n196' (MAXK 4 x MAXL 7 on GEOM_C2) and 'n196:N' (its first N columns).  33 synthetic
    records with weights around 1e-22; AWA and y by NumPy (they are inputs here).  alpha0 lies where both terms matter."""
    if name in _PROBLEMS:
        return _PROBLEMS[name]
    import io
    from volumetricinterp_amd import synth
    from test_gpu_configs import CFG144
    from test_gpu_resident_geometry import SPH_CFG
    if name == 'k8l2':
        f = load_golden('fit_k8l2')
        A, R, alpha0 = f['rec0_A'], f['R'], float(np.nan_to_num(f['alpha'][0], nan=1e-26))
    elif name.startswith('n196:'):
        A = problem('n196')['A'][:, :int(name[5:])]
        R = alpha0 = None
    else:
        from volumetricinterp_amd.models.sphharmlag import Model
        m = Model(io.StringIO(CFG144 if name == 'c144' else SPH_CFG % (4, 7)))
        lat, lon, alt = synth.beams(*synth.GEOM_C2, seed=0)
        ctx = m.ctx
        At = m.basis_device(ctx.to_device(lat), ctx.to_device(lon), ctx.to_device(alt), lat.size, transposed=True)
        A = At.download().T
        R, alpha0 = (load_golden('regmat')['default_curvature'], 10.0 ** -26.5) if name == 'c144' else (None, None)
    A = np.ascontiguousarray(A)
    P, N = A.shape
    T = 33
    b, err = synth.synth_records(A, T, seed0=7000)
    W = err ** -2.0
    At = np.ascontiguousarray(A.T)
    AWA = np.array([(At * W[t]) @ A for t in range(T)])
    y = (W * b) @ A
    if R is None:
        R, alpha0 = _curvature_like(N, float(np.mean(np.diag(AWA[0])))), 1e-3
    _PROBLEMS[name] = dict(A=A, At=At, P=P, N=N, T=T, W=W, b=b, AWA=AWA, y=y, R=np.ascontiguousarray(R), alpha0=alpha0)
    return _PROBLEMS[name]


@gpu
@pytest.mark.parametrize('name', ['k8l2', 'c144', 'n196'])
def test_normal_equations_of_real_records_within_the_bound(name):
    """AWA at 300 random element pairs and the corners, y at every n, of the first, the last-but-one and the last of 33 records
    (the last is the one the padded group repeats): |out - exact| <= gamma(P + 2) sum_p |A_np W_p A_mp|."""
    q = problem(name)
    rng = np.random.default_rng(q['N'])
    AWA, y = normal_eq(q['At'], q['W'], q['b'])
    pairs = sample_pairs(rng, q['N'])
    for t in (0, 31, 32):
        hi, lo, ab = awa_reference(q['At'], q['W'], q['b'], t, pairs)
        ok = sum_gate(AWA[t][pairs[:, 0], pairs[:, 1]], hi, lo, ab, q['P'])
        assert ok.all(), (name, t, pairs[~ok][:5])
        yh, yl, yab = y_reference(q['At'], q['W'], q['b'], t)
        ok = sum_gate(y[t], yh, yl, yab, q['P'])
        assert ok.all(), (name, t, np.nonzero(~ok)[0][:5])


@gpu
@pytest.mark.parametrize('name', ['k8l2', 'c144', 'n196'])
def test_chi2_of_real_records_within_the_bound(name):
    """chi^2 of least-squares coefficients (A C cancels by many digits) and of random ones, in batches of 9 and 257, against
    chi2_reference within its derived bound."""
    q = problem(name)
    rng = np.random.default_rng(q['N'] + 1)
    A, N = q['A'], q['N']
    Cs = []
    for t in (0, 32):
        sw = np.sqrt(q['W'][t])
        c = np.linalg.lstsq(A * sw[:, None], q['b'][t] * sw, rcond=None)[0]
        Cs += [c, c * (1.0 + 1e-3 * rng.standard_normal(N))]
    for B in (9, 257):
        C = rng.standard_normal((B, N)) * np.abs(Cs[0])
        rec = rng.integers(0, q['T'], B).astype(np.int32)
        for j, pos in enumerate((0, 3, B - 2, B - 1)):
            C[pos], rec[pos] = Cs[j], (0, 0, 32, 32)[j]
        out = chi2(q['At'], C, rec, q['W'], q['b'])
        for pos in (0, 1, 3, B - 2, B - 1):
            ref, bound = chi2_reference(q['At'], C[pos], q['W'][rec[pos]], q['b'][rec[pos]])
            assert chi2_gate(float(out[pos]), ref, bound), (name, B, pos, out[pos], float(ref), bound)


def rotated_system_gates(tag, V, D1, D2, yt, AWA, R, y, orth_gate):
    """V orthonormal to orth_gate (the gates of test_gpu_search_stages.py: 1e-13 after vi_warm_prepare_f64, 1e-12 after
    vi_warm_rebase_f64) and, given this V, D1 = V AWA V^T, D2 = V R V^T within chain_reference's bound and yt = V y within
    vec_gate's.  A list of failures."""
    fails = []
    if not orth_defect(V) <= orth_gate:
        fails.append('%s: V V^T - I = %.2e > %.0e' % (tag, orth_defect(V), orth_gate))
    for nm, D, M in (('D1', D1, AWA), ('D2', D2, R)):
        ok = chain_gate(D, V, M)
        if not ok.all():
            fails.append('%s: %s outside the bound at %d elements, first %r' % (tag, nm, (~ok).sum(), tuple(np.argwhere(~ok)[0])))
    ok = vec_gate(yt, V, y)
    if not ok.all():
        fails.append('%s: yt outside the bound at %r' % (tag, np.nonzero(~ok)[0][:5]))
    return fails


@gpu
@pytest.mark.parametrize('name', ['k8l2', 'c144', 'n196'])
def test_prepare_and_finish_in_batches_of_1_31_33(name):
    """vi_warm_prepare_f64 with 1, 31 and 33 systems (one padded group; a full group and a padded one): record 5 - first of
    1, last of 31, last of 33, the entry the padding repeats - gets the same C, rank, V, D1, D2, yt bit for bit, and so does
    record 6 at position 0 of the larger batches; vi_decompose_f64 + vi_warm_finish_f64 of the 33 leave the same bits; the
    rotated systems of records 5 and 6 pass rotated_system_gates at the prepare gate."""
    _lib = _L()
    q = problem(name)
    N = q['N']
    recs = {1: [5], 31: [6] + list(range(7, 36))[:29] + [5], 33: [6] + list(range(7, 38))[:31] + [5]}
    res = {}
    for B, rec in recs.items():
        rec = np.array(rec, np.int32) % q['T']
        rec[-1] = 5
        assert len(rec) == B
        res[B] = (rec, warm_prepare(q['AWA'], q['R'], q['y'], rec, np.full(B, q['alpha0'])))
    for B in (31, 33):
        for k, (a, c) in enumerate(zip(res[1][1], res[B][1])):
            assert np.array_equal(a[0], c[B - 1]), (name, B, 'record 5, output %d' % k)
    for k, (a, c) in enumerate(zip(res[31][1], res[33][1])):
        assert np.array_equal(a[0], c[0]), (name, 'record 6, output %d' % k)
    rec, (C, rk, V, D1, D2, yt) = res[33]
    fails = []
    for pos in (0, 32):
        t = rec[pos]
        fails += rotated_system_gates('%s prepare record %d' % (name, t), V[pos], D1[pos], D2[pos], yt[pos], q['AWA'][t], q['R'],
                                      q['y'][t], 1e-13)
    assert not fails, '\n'.join(fails)
    # the two phases as separate calls
    ctx = _ctx()
    B = 33
    logd = int(_lib.lib.vi_rotation_log_bytes(N)) // 8
    dlog, dnr = ctx.empty((B * logd,)), ctx.empty((B,), np.int32)
    dA, dR, dy, drec, dal = dev(q['AWA']), dev(q['R']), dev(q['y']), dev(rec), dev(np.full(B, q['alpha0']))
    oC, drk = Out((B, N)), ctx.empty((B,), np.int32)
    call('vi_decompose_f64', B, N, dA, drec, dal, dR, dy, EPS, oC, drk, dlog, dnr)
    assert np.array_equal(oC.get(), C) and np.array_equal(drk.download(), rk)
    o = [Out((B, N, N)), Out((B, N, N)), Out((B, N, N)), Out((B, N))]
    call('vi_warm_finish_f64', B, N, dlog, dnr, dA, drec, dR, dy, *o)
    for k, (a, c) in enumerate(zip(o, (V, D1, D2, yt))):
        assert np.array_equal(a.get(), c), (name, 'finish output %d' % k)


def prepared_slots(name, nrec=3):
    """Records 0 .. nrec - 1 of a problem set up at alpha0 (vi_warm_prepare_f64): V, D1, D2, yt."""
    q = problem(name)
    key = ('slots', nrec)
    if key not in q:
        rec = np.arange(nrec, dtype=np.int32)
        q[key] = warm_prepare(q['AWA'], q['R'], q['y'], rec, np.full(nrec, q['alpha0']))[2:]
    return q, q[key]


@gpu
@pytest.mark.parametrize('N', [50, 100, 151, 157, 180])
def test_rebase_with_real_rotations_tiled_against_whole(N):
    """vi_warm_rebase_f64 0.13 decades away from where the rotated systems were set up (the solve rotates: V changes), with 3
    systems (tiled products) and with n_cu / 4 + 1 (whole products, the shape inside k_brent_warm): every slot of the large
    batch holds a copy of one of the three systems and must come out with the bits that system gets in the batch of 3 - C,
    rank, V, D1, D2, yt.  The new V is orthonormal and diagonalises X(alpha) to the gates of test_gpu_search_stages.py (1e-12),
    and D1, D2, yt pass rotated_system_gates for it."""
    n_cu = n_cu_of_device()
    q, (V, D1, D2, yt) = prepared_slots('n196:%d' % N)
    few, many = rebase_counts(n_cu)
    assert wg_gemm_geometry(N, few, n_cu)['shape'] == 'tiled' and wg_gemm_geometry(N, many, n_cu)['shape'] == 'whole'
    a1 = q['alpha0'] * 10.0 ** 0.13
    res = {}
    for B in (few, many):
        src = np.arange(B) % 3
        res[B] = warm_rebase(q['AWA'], q['R'], q['y'], src, np.arange(B), np.full(B, a1), V[src], D1[src], D2[src], yt[src])
    for k, (a, c) in enumerate(zip(res[few], res[many])):
        for j in range(many):
            assert np.array_equal(a[j % 3], c[j]), (N, 'output %d of system %d: tiled and whole differ' % (k, j))
    C, rk, Vn, D1n, D2n, ytn = res[few]
    fails = []
    for i in range(3):
        assert not np.array_equal(Vn[i], V[i])                                     # the solve did rotate
        assert orth_defect(V[i]) <= 1e-13
        fails += rotated_system_gates('N %d rebase record %d' % (N, i), Vn[i], D1n[i], D2n[i], ytn[i], q['AWA'][i], q['R'], q['y'][i],
                                      1e-12)
        Vw = V[i] @ Vn[i].T                                                        # V_new = V_old Vw in the library's layout
        if not orth_defect(Vw) <= 1e-12 + 1e-13:                                  # (the defects of its two factors)
            fails.append('N %d record %d: Vw is not orthonormal, %.2e' % (N, i, orth_defect(Vw)))
        Xr = D1n[i] + a1 * D2n[i]
        off = Xr - np.diag(np.diag(Xr))
        if not np.max(np.abs(off)) <= 1e-12 * np.max(np.abs(np.diag(Xr))):
            fails.append('N %d record %d: X(alpha) is not diagonal in the new basis' % (N, i))
    assert not fails, '\n'.join(fails)


@gpu
@pytest.mark.parametrize('N', [50, 157])
def test_warm_chi2_one_is_warm_solve_plus_chi2(N):
    """vi_warm_chi2_one_f64 (fused forming at N = 50, the two-kernel one at N = 157): h_chi2[0] has the bits of
    vi_warm_solve_f64 followed by vi_chi2_f64 for that (slot, alpha, record)."""
    _lib = _L()
    ctx = _ctx()
    q, (V, D1, D2, yt) = prepared_slots('n196:%d' % N)
    dD1, dD2, dyt, dV, dAt, dW, db = dev(D1), dev(D2), dev(yt), dev(V), dev(q['At']), dev(q['W']), dev(q['b'])
    scratch = ctx.empty((N + 8,))
    for slot, dec in ((0, 0.0), (2, 0.07), (1, -0.2)):
        alpha = q['alpha0'] * 10.0 ** dec
        h = (ctypes.c_double * 3)()
        call('vi_warm_chi2_one_f64', N, q['P'], dD1, dD2, dyt, dV, slot, alpha, EPS, dAt, slot, dW, db,
             scratch, h)
        C, _ = warm_solve(D1, D2, yt, V, np.array([slot], np.int32), np.array([alpha]))
        want = chi2(q['At'], C, np.array([slot], np.int32), q['W'], q['b'])[0]
        assert np.isfinite(want) and want > 0
        assert h[0] == want, (N, slot, h[0], want)


# ---- generalised cross validation ------------------------------------------------------------------------------------------
GCV_C = 64.0


def gcv_problem(N, P=257, seed=0):
    """A well-conditioned record: Gaussian basis with columns graded over 2.2 decades (condition of the systems 2e4 .. 1e5),
    weights in 0.5 .. 1.5, R = I, alpha a thousandth of the smallest eigenvalue's scale."""
    rng = np.random.default_rng(1000 * N + seed)
    At = rng.standard_normal((N, P)) * 10.0 ** (-2.2 * np.arange(N) / N)[:, None]
    W = rng.uniform(0.5, 1.5, P)
    b = rng.standard_normal(P)
    AWA = (At * W) @ At.T
    AWA = 0.5 * (AWA + AWA.T)
    y = At @ (W * b)
    R = np.eye(N)
    alpha = 1e-3 * float(np.linalg.eigvalsh(AWA)[0])
    return At, W, b, AWA, y, R, alpha


def gcv_reference(At, W, b, AWA, y, R, alpha, p):
    """The leave-one-out term of point p: X = AWA - W_p a a^T + alpha R and y - W_p b_p a formed in 80-bit arithmetic, solved
    by float64 LU with iterative refinement on 80-bit residuals (three steps: the error falls by kappa u each step, to the
    80-bit level kappa N 2^-64), res = (a . C - b_p)^2 W_p.  Returns res, C, the condition number of X and its rank at the
    library's cut eps max|lambda|."""
    a = At[:, p].astype(LD)
    X = AWA.astype(LD) - LD(W[p]) * np.outer(a, a) + LD(alpha) * R.astype(LD)
    yl = y.astype(LD) - LD(W[p]) * LD(b[p]) * a
    X64 = X.astype(np.float64)
    lam = np.linalg.eigvalsh(X64)
    C = np.linalg.solve(X64, yl.astype(np.float64)).astype(LD)
    for _ in range(3):
        C = C + np.linalg.solve(X64, (yl - X @ C).astype(np.float64)).astype(LD)
    d = a @ C - LD(b[p])
    return d * d * LD(W[p]), C, float(np.abs(lam).max() / np.abs(lam).min()), int((np.abs(lam) > EPS * np.abs(lam).max()).sum())


def gcv_gate(out, At, W, b, p, res, C, kappa):
    """|out - res| <= W_p dm (2 |d| + dm) with dm = |a|_2 GCV_C kappa N u |C|_2 + gamma(N) sum_n |a_n C_n|: the solution of a
    system of condition kappa by a backward-stable eigen-solve moves by at most c kappa N u |C| - the constant c = 64 stands
    for the two fmas that form X (2 u |X| elementwise), ten Jacobi sweeps in which each element takes part in two rotations
    of error 3 u each, and the truncated solve's two products - and the residual's dot product adds its gamma(N) term."""
    N = At.shape[0]
    a = At[:, p]
    C64 = C.astype(np.float64)
    dm = np.linalg.norm(a) * GCV_C * kappa * N * U * np.linalg.norm(C64) + gamma(N) * np.abs(a * C64).sum()
    d = abs(float(a.astype(LD) @ C - LD(b[p])))
    return bool(np.isfinite(out) and abs(LD(out) - res) <= LD(W[p] * dm * (2 * d + dm)))


def test_gcv_gate_rejects_a_neighbouring_point():
    """Host: NumPy's float64 leave-one-out term passes gcv_gate; the term of another point, and the term with the down-date
    left out (the full fit's residual), do not."""
    At, W, b, AWA, y, R, alpha = gcv_problem(27)
    p = 5
    res, C, kappa, rank = gcv_reference(At, W, b, AWA, y, R, alpha, p)
    assert kappa <= 1e6 and rank == 27
    a = At[:, p]
    c64 = np.linalg.solve(AWA - W[p] * np.outer(a, a) + alpha * R, y - W[p] * b[p] * a)
    assert gcv_gate((a @ c64 - b[p]) ** 2 * W[p], At, W, b, p, res, C, kappa)
    cfull = np.linalg.solve(AWA + alpha * R, y)
    assert not gcv_gate((a @ cfull - b[p]) ** 2 * W[p], At, W, b, p, res, C, kappa)
    res6 = gcv_reference(At, W, b, AWA, y, R, alpha, 6)[0]
    assert not gcv_gate(float(res6), At, W, b, p, res, C, kappa)


@gpu
@pytest.mark.parametrize('N', [27, 50, 144])
def test_gcv_terms_against_a_leave_one_out_solve(N):
    """vi_gcv_terms_f64 with np in {1, 2, 3, 4, 5, 9} listed points, repeats among them (np % 4 = 0 .. 3, one to three blocks of
    k_loo_resid): every term against gcv_reference within gcv_gate; the systems have condition <= 1e6 and full rank at the
    library's cut (asserted on the reference), so the truncation keeps every eigenvalue; a repeated point gives the same
    bits."""
    At, W, b, AWA, y, R, alpha = gcv_problem(N)
    P = At.shape[1]
    dAt, dA, dy, dW, db, dR = dev(At), dev(AWA), dev(y), dev(W), dev(b), dev(R)
    base = np.array([3, P - 1, 3, 0, 200, 3, P - 1, 77, 256], np.int32)
    refs = {}
    for p in np.unique(base):
        refs[p] = gcv_reference(At, W, b, AWA, y, R, alpha, p)
        assert refs[p][2] <= 1e6 and refs[p][3] == N, (N, p, refs[p][2:])
    for _, k in [c for c in gcv_cases() if c[0] == N]:
        pidx = base[:k]
        o = Out((k,))
        call('vi_gcv_terms_f64', k, P, N, dAt, dev(pidx), dA, dy, dW, db, alpha, dR, EPS, o)
        out = o.get()
        for i, p in enumerate(pidx):
            res, C, kappa, _ = refs[p]
            assert gcv_gate(float(out[i]), At, W, b, p, res, C, kappa), (N, k, i, p, out[i], float(res))
            assert out[i] == out[list(pidx).index(p)], (N, k, i, p)


# ==== 4. the grid limit =====================================================================================================
@gpu
def test_normal_equations_of_70000_small_records():
    """N = 8, P = 64, T = 70 000 integer records: 287 MB of scaled copies, within the byte budget of one chunk, but more
    records than gridDim.z of k_scale_rows takes - the call failed until the chunk was capped at the grid limit.  AWA and y
    of the first, the 65 536th and the last record (and of every other one) have NumPy's bits."""
    N, P, T = 8, 64, 70000
    g = normal_eq_geometry(N, P, T)
    assert T * N * P * 8 < 2 ** 30 and T > GRID_YZ_MAX and g['chunks'] == 2
    rng = np.random.default_rng(70000)
    At, W, b = normal_eq_integer_inputs(rng, N, P, T)
    AWA, y = normal_eq(At, W, b)
    ref = np.matmul(At[None, :, :] * W[:, None, :], At.T)
    ry = (W * b) @ At.T
    for t in (0, 65535, T - 1):
        m = same(AWA[t], ref[t], 'record %d AWA' % t) or same(y[t], ry[t], 'record %d y' % t)
        assert not m, m
    m = same(AWA, ref, 'AWA') or same(y, ry, 'y')
    assert not m, m
