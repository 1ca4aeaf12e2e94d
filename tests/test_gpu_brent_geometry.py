"""The device-side root finder (csrc/vi_brent.hip: vi_brent_warm_f64 / k_brent_warm, vi_brent_host_one_f64,
vi_brent_warm_supported) at every launch geometry, against roots known by construction and against the host-driven loop
bit for bit.  These are the two stage entries that tests/test_gpu_fit_geometry.py does not hold.

k_brent_warm is one persistent workgroup per record; its shape follows from N alone (brent_geometry, brent_lds_bytes in
vi_brent.hip, restated below from vi_jacobi.hip and vi_gemm_device.h):

    N           Jacobi body inside the kernel        threads               chi^2 blocks per pass (nbp = threads >> 8)
    8 - 92      jacobi_system<1>                     512 (own kernel: 64 - 256)      2
    93 - 112    jacobi_system_v2                     512 (own kernel: 384 - 448)     2
    113 - 144   jacobi_system_v2                     512 - 704                       2
    145 - 152   jacobi_system_v2                     768                             3
    153 - 156   jacobi_system<1>                     768                             3
    157 - 180   jacobi_system<2>                     512                             2
    181 - 192   jacobi_system<3>                     512                             2
    193 - 196   none: the workgroup's LDS image exceeds 160 KB whatever P; vi_brent_warm_supported is 0
(M = 37 matches, N = 145 - 148, have 666 super-blocks: 704 update threads + the set-up wave = 768 already, so the three-block
chi^2 pass starts at 145, not at 149; both 144 / 145 and 148 / 149 are in the list.)
LDS: 256 static bytes + max(Jacobi image, wg_gemm panels) + (N rounded to even + 768 + npart + 16) doubles + the state + 64 bytes, npart = 64
partial sums up to 64 blocks of 256 points and nb rounded up to even beyond.  wg_gemm runs its tile loop ceil(ceil(N / 6)^2 /
threads) times with the Brent workgroup's thread count: twice from N = 157 to 192 (27^2 .. 32^2 tiles, 512 threads).

Part 1 (no GPU) prints the case table and asserts that it reaches every row above on both sides of every boundary, and shows
on the host that the gate of part 3 rejects emulated wrong roots.  Part 2 compares vi_brent_warm_supported with the
restatement for N = 1 .. 260 and checks that unsupported sizes are refused before anything is written.  Part 3 runs records
whose root is known by construction (chi^2 of a well-conditioned ridge problem is monotone in alpha; nu is chi^2 at a chosen
x0 in 80-bit arithmetic) within a derived gate.  Part 4 compares the kernel with vi_brent_host_one_f64 - the stand-alone
kernels of the host path - bit for bit on real graded problems under three re-basing rules, with task and slot indirection,
with more tasks than workgroups, under a sweep cap that makes records leave with status 2, and through FitEngine against
the NumPy iteration (alpha_search.BrentBatch).

Finding: k_brent_warm<3> (N = 181 ... 192) returned wrong roots.  It called the solver body through the out-of-line
jacobi_system_call, as the other variants do to keep the solver's register budget; with three super-blocks per thread that
copy returned solutions that changed from one function value to the next of the same record: Brent ended on its jump rule, or
at an end of the bracket, 3e-3 ... 0.47 decades from the known root (test_known_roots_at_every_order[181 ... 192]), and
after 4 iterations where the host loop takes 8 (test_device_brent_is_the_host_loop_bit_for_bit).  The stand-alone
k_jacobi_solve<3>, which inlines the same body, is right - the host loop and the bracket-end values use it.  The kernel now
inlines jacobi_system<3> as well; the variants for N <= 180 are unchanged.
Finding: FitEngine never launched that variant: FitEngine.warm_enabled() ended the rotated-system search at N = 180, the in-LDS
solver's range before its three-super-block kernel, so at N = 181 ... 192 every fit took cold solves and
device_brent_records grew by 0 of 12 (test_engine_with_device_and_with_numpy_brent[192]).  The search now runs up to N = 192,
the last order the kernel serves; 193 ... 196 keep the cold path.
Finding: brent_lds_bytes left out the 256 bytes of static LDS the compiler gives the kernel (the word behind
__syncthreads_or).  At N = 189 ... 192 records of more than 35 328 and up to 43 520 points passed vi_brent_warm_supported and
the launch then failed with "invalid argument" from hipFuncSetAttribute - and left that error behind for the next launch
(test_known_roots_at_the_top_of_lds).  The static part is now counted (BRENT_STATIC_LDS, checked against the kernel's own
attributes at the launch), so such records are refused as unsupported and the engine takes the host path."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_fit_geometry import (GCV_C, LD, U, Out, _L, _ctx, call, chi2, chi2_reference, dev, gamma, n_cu_of_device,
                                   prepared_slots, problem, same, warm_prepare, warm_solve, wg_gemm_geometry)
from test_gpu_solver_geometry import jacobi_class

gpu = pytest.mark.gpu
EPS = np.finfo(float).eps
REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024
STATE_BYTES = 104                    # sizeof(BrentState): nine doubles and seven ints, padded to the alignment of a double
STATIC_LDS = 256                     # the kernel's static LDS (the compiler's, for __syncthreads_or): BRENT_STATIC_LDS
N_CU_REF = 256                       # the CU count the case table is printed for; the GPU tests ask the device
XTOL, RTOL = 2e-12, 4 * EPS          # brentq's tolerances, as vi_brent_warm_f64 passes them
VI_ERR_UNSUPPORTED = -6


# ==== 1. restated geometry ==================================================================================================
def jacobi_own_geometry(N):
    """jacobi_geometry and vi_jacobi_use_v2 (vi_jacobi.hip): the K3 kernel's own super-blocks per thread, threads, v2."""
    M = (N + 3) // 4
    nsb = M * (M - 1) // 2
    if nsb <= 768:
        it, thr = 1, max(64, (nsb + 63) // 64 * 64)
    else:
        it, thr = (nsb + 511) // 512, 512
    return it, thr, it == 1 and 24 <= M <= 64 and thr + 64 <= 768


def jacobi_lds(N):
    """vi_jacobi_lds_bytes."""
    Np = (N + 3) // 4 * 4
    M = Np // 4
    b = (Np * (Np + 1) // 2 + 2 * Np) * 8 + 4 * M * 16 + 128
    if jacobi_own_geometry(N)[2]:
        b += 4 * M * 16 + 4 * M * 8 + 16 + 14 * M * 4
    return (b + 15) // 16 * 16


def brent_geometry(N):
    """brent_geometry (vi_brent.hip): body, threads of the workgroup, blocks of 256 points per chi^2 pass."""
    it, thr, v2 = jacobi_own_geometry(N)
    if v2:
        body, threads = 'v2', max(512, 64 + thr)
    elif it == 1:
        body, threads = 'v1 IT=1', max(512, thr)
    else:
        body, threads = 'v1 IT=%d' % it, 512
    return body, threads, threads >> 8


def brent_lds(N, P):
    """brent_lds_bytes: bytes of the workgroup's dynamic LDS and the length of part[]."""
    ldsj = jacobi_lds(N)
    ldsg = 2 * 16 * ((N + 7) // 8 * 8) * 8                       # wg_gemm_lds_doubles
    eff = ldsj if ldsj > ldsg else (ldsg + 15) // 16 * 16
    nb = -(-P // 256)
    npart = 64 if nb < 64 else (nb + 1) // 2 * 2
    return STATIC_LDS + eff + ((N + 1) // 2 * 2 + 768 + npart + 16) * 8 + STATE_BYTES + 64, npart


def brent_supported(N, P):
    return N >= 1 and P >= 1 and jacobi_class(N) != 'library' and brent_lds(N, P)[0] <= LDS_LIMIT


def largest_p(N, ok=None):
    """The largest P with ok(N, P) (the restatement by default), 0 when there is none: bisection, ok being monotone in P."""
    ok = ok or brent_supported
    if not ok(N, 1):
        return 0
    lo, hi = 1, 1 << 40
    assert not ok(N, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(N, mid) else (lo, mid)
    return lo


def gemm_passes(N):
    """Passes of wg_gemm's tile loop inside k_brent_warm: 6 x 6 tiles over the Brent workgroup's threads."""
    nt = -(-N // 6)
    return -(-nt * nt // brent_geometry(N)[1])


def row_of(N):
    """The row of the table at the top that N belongs to."""
    if not brent_supported(N, 1):
        return 'no device Brent' if jacobi_class(N) != 'library' else 'library'
    body, threads, nbp = brent_geometry(N)
    own = jacobi_own_geometry(N)[1] + (64 if body == 'v2' else 0)
    if body == 'v2':
        return 'v2 raised to 512' if own < 512 else 'v2 512-704' if threads < 768 else 'v2 768'
    if body == 'v1 IT=1':
        return 'v1 IT=1 raised to 512' if own < 512 else 'v1 IT=1 768'
    return body


ROWS = {'v1 IT=1 raised to 512': (8, 92), 'v2 raised to 512': (93, 112), 'v2 512-704': (113, 144), 'v2 768': (145, 152),
        'v1 IT=1 768': (153, 156), 'v1 IT=2': (157, 180), 'v1 IT=3': (181, 192), 'no device Brent': (193, 196)}
BOUNDARIES = [(92, 93), (112, 113), (144, 145), (148, 149), (152, 153), (156, 157), (180, 181), (192, 193)]
ORDERS = [8, 9, 10, 11, 32, 64, 92, 93, 94, 95, 100, 112, 113, 124, 144, 145, 148, 149, 152, 153, 156, 157, 159, 180, 181, 186,
          187, 191, 192, 193, 196]


def class_of(N):
    if row_of(N) in ('no device Brent', 'library'):
        return row_of(N)
    body, threads, nbp = brent_geometry(N)
    own = jacobi_own_geometry(N)[1]
    return '%-7s %3d thr (own kernel %s) nbp %d, wg_gemm %d pass%s, N%%4 %d' % (
        body, threads, '%d+64' % own if body == 'v2' else '%d' % own, nbp, gemm_passes(N), 'es' if gemm_passes(N) > 1 else '', N % 4)


CASES = {N: class_of(N) for N in ORDERS}
SUPPORTED = [N for N in ORDERS if brent_supported(N, 1)]
NB_ORDERS = (9, 100, 149, 153, 157)                  # the orders that take every P of PS_NB: nbp = 2 and 3, v1 and v2
PS_ALL, PS_NB = (40, 257), (255, 256, 550, 2600)
BIG_PS = (16384, 16500, 16700)                       # nb = 64, 65, 66 at N = 9
RULES = ('default', 'none', 'four')
NREC = 4                                             # records per bit-for-bit case
P_REAL = {32: 550}                                   # data points of the real problems of part 4 (2600 elsewhere)


def known_cases(n_cu=N_CU_REF):
    """(N, P, ntask) of part 3: roots known by construction.  P = 0 stands for the largest supported P of that order."""
    c = [(N, P, 3) for N in SUPPORTED for P in PS_ALL]
    c += [(N, P, 3) for N in NB_ORDERS for P in PS_NB]
    c += [(9, 1, 3), (9, 40, 1), (144, 257, 1)]
    c += [(9, P, 2) for P in BIG_PS]
    c += [(192, 0, 2)]
    c += [(9, 40, n_cu + 37), (100, 257, n_cu + 37)]
    return c


def case_list(n_cu=N_CU_REF):
    """(N, P, ntask, rule): part 3 under the engine's rule, part 4 under all three."""
    c = [(N, P or largest_p(N), n, 'default') for N, P, n in known_cases(n_cu)]
    c += [(N, P_REAL.get(N, 2600), NREC, r) for N in SUPPORTED for r in RULES]
    return c


def test_case_list_reaches_every_class():
    """Prints the case table; the lists reach every row of the table at the top on both sides of every boundary, every
    residue of N mod 4 where the padding differs, both chi^2 pass widths with every remainder of blocks, ragged and full
    blocks of points, part[] of 64 and of 66 entries, one and two passes of wg_gemm's tile loop, one task, a few, and more
    tasks than workgroups."""
    cl = case_list()
    for N in ORDERS:
        mine = [(P, n, r) for M, P, n, r in cl if M == N]
        print('N %3d  %-62s LDS %6d B at P <= 16384, largest P %8d | %s' % (
            N, CASES[N], brent_lds(N, 1)[0], largest_p(N),
            ' '.join('%dx%d%s' % (P, n, '' if r == 'default' else ':' + r) for P, n, r in mine) or 'refused'))
    # the restated ranges are the rows, and every row has an order on both sides of each of its ends
    rows = {}
    for N in range(8, 197):
        rows.setdefault(row_of(N), []).append(N)
    assert {k: (v[0], v[-1]) for k, v in rows.items()} == ROWS and all(v == list(range(v[0], v[-1] + 1)) for v in rows.values())
    assert row_of(7) == 'library' and row_of(197) == 'library'
    for name in ROWS:
        assert any(row_of(N) == name for N in ORDERS), 'no order left in row %r' % name
    for a, b in BOUNDARIES:
        assert a in ORDERS and b in ORDERS, (a, b)
        assert (row_of(a) != row_of(b)) == ((a, b) != (148, 149))
    assert 8 in ORDERS and min(ORDERS) == 8
    for name in ('v1 IT=1 raised to 512', 'v1 IT=3'):
        assert {N % 4 for N in ORDERS if row_of(N) == name} == {0, 1, 2, 3}, name
    assert {N % 4 for N in ORDERS if row_of(N).startswith('v2')} == {0, 1, 2, 3}
    assert set(SUPPORTED) == {N for N in ORDERS if N <= 192} and set(NB_ORDERS) <= set(SUPPORTED)
    # every supported order runs in part 3 (P = 40 and 257, three tasks) and in part 4 (three rules)
    for N in SUPPORTED:
        assert {(P, n) for M, P, n, r in cl if M == N and r == 'default'} >= {(40, 3), (257, 3)}, N
        assert {r for M, P, n, r in cl if M == N and n == NREC} == set(RULES), N
    # chi^2 passes: nbp = 2 and 3, the number of blocks leaving every remainder
    for nbp in (2, 3):
        mine = [(N, P) for N, P, n, r in cl if brent_geometry(N)[2] == nbp]
        assert {-(-P // 256) % nbp for N, P in mine} == set(range(nbp)), nbp
        assert {brent_geometry(N)[0][:2] for N, P in mine} == {'v1', 'v2'}
        assert {P % 256 == 0 for N, P in mine} == {True, False}
    assert {P for N, P, n, r in cl} >= {1, 40, 255, 256, 257, 550, 2600}
    assert [brent_lds(9, P)[1] for P in BIG_PS] == [64, 66, 66] and [-(-P // 256) for P in BIG_PS] == [64, 65, 66]
    assert all((9, P, 2, 'default') in cl for P in BIG_PS)
    assert all(N <= 32 or P <= 2600 or P == largest_p(N) for N, P, n, r in cl)               # big P goes with small N
    # the order next to the top of LDS, at its largest record
    top = largest_p(192)
    assert (192, top, 2, 'default') in cl and brent_lds(192, top)[0] <= LDS_LIMIT < brent_lds(192, top + 1)[0]
    assert brent_lds(192, 16384)[0] == 162984 + STATIC_LDS == brent_lds(191, 1)[0] and brent_lds(189, 1)[0] == 162968 + STATIC_LDS
    assert LDS_LIMIT - brent_lds(189, 1)[0] < 900 and top == 138 * 256 and brent_lds(192, top)[1] == 138
    assert all(brent_lds(N, 1)[0] > LDS_LIMIT for N in (193, 196)) and jacobi_class(196) != 'library'
    # wg_gemm: one and two passes of the tile loop; the host path's own one-workgroup shape differs (640 threads at most)
    assert {gemm_passes(N) for N in SUPPORTED} == {1, 2}
    assert gemm_passes(156) == 1 and gemm_passes(157) == 2 and gemm_passes(192) == 2 and gemm_passes(152) == 1
    assert wg_gemm_geometry(152, N_CU_REF, N_CU_REF)['passes'] == 2 and wg_gemm_geometry(157, N_CU_REF, N_CU_REF)['threads'] == 640
    # tasks
    assert {n for N, P, n, r in cl} >= {1, 2, 3, NREC, N_CU_REF + 37}
    assert {(N, P) for N, P, n, r in cl if n == N_CU_REF + 37} == {(9, 40), (100, 257)}


# ==== device calls ==========================================================================================================
I_SENTINEL = -559038737                                # 0xDEADBEEF as an int32
I_GUARD = 128


class IntOut:
    """An int32 device output of n entries between I_GUARD sentinel ints on either side."""

    def __init__(self, n, init=None):
        self.n = int(n)
        host = np.full(2 * I_GUARD + self.n, I_SENTINEL, np.int32)
        if init is not None:
            host[I_GUARD:I_GUARD + self.n] = init
        self.d = dev(host, np.int32)
        self.ptr = self.d.offset_ptr(I_GUARD)

    def get(self):
        res = self.d.download()
        assert np.all(res[:I_GUARD] == I_SENTINEL) and np.all(res[I_GUARD + self.n:] == I_SENTINEL), 'a store outside the output'
        return res[I_GUARD:I_GUARD + self.n].copy()


def vptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def exp10(x):
    """10^x by the library's routine (vi_exp10.h), the one the kernel and the host loop use."""
    a, o = np.array([float(x)]), np.empty(1)
    assert _L().lib.vi_exp10_f64(vptr(a), vptr(o), 1) == 0
    return float(o[0])


_RULES = {}


def rule(name):
    """h_rebase (10 doubles): 'default' is FitEngine._brent_rule() of an engine without environment overrides; 'none' the
    same with no re-basing (what VINTERP_REBASE=0 gives); 'four' moves the system at each of the first four iterates after
    the first (two consecutive abscissae are always closer than 10 decades)."""
    if not _RULES:
        from volumetricinterp_amd.fitengine import FitEngine
        assert not any(k in os.environ for k in ('VINTERP_REBASE', 'VINTERP_REBASE2', 'VINTERP_REBASE_SCHEDULE', 'VINTERP_JUMP_STOP'))
        eng = FitEngine.__new__(FitEngine)
        eng._subs, eng._bufs, eng.R = None, {}, {}
        d = eng._brent_rule()
        assert d.shape == (10,) and d[0] == 1 and d[1] == FitEngine.REBASE_WITHIN and d[7] == 1 and d[8] > 0
        none, four = d.copy(), d.copy()
        none[0], none[1:5], none[7] = 0, 0, 0
        four[0], four[1:5] = 4, 10.0
        _RULES.update(default=d, none=none, four=four)
    return _RULES[name]


def on_device(pb):
    """The inputs of a problem on the device, once: At (N, P), W, b (T, P), AWA (T, N, N), R (N, N), y (T, N)."""
    if 'brent_dev' not in pb:
        pb['brent_dev'] = {k: dev(pb[k]) for k in ('At', 'W', 'b', 'AWA', 'R', 'y')}
    return pb['brent_dev']


def warm_chi2_one(pb, dslots, slot, rec, alpha):
    """vi_warm_chi2_one_f64 on device slots (V, D1, D2, yt): chi^2 and the sweeps of its solve."""
    d = on_device(pb)
    N, P = pb['N'], pb['P']
    if 'brent_scratch' not in pb:
        pb['brent_scratch'] = _ctx().empty((N + 8,))
    h = (ctypes.c_double * 3)()
    call('vi_warm_chi2_one_f64', N, P, dslots[1], dslots[2], dslots[3], dslots[0], int(slot), float(alpha), EPS, d['At'],
         int(rec), d['W'], d['b'], pb['brent_scratch'], h)
    return h[0], int(np.array([h[2]]).view(np.int32)[0])


def brent_warm(pb, slots, rec, slot, xa, xb, fa, fb, nu, rl, raw=False):
    """vi_brent_warm_f64 on device copies of the slots (V, D1, D2, yt), every output and every slot array between sentinels.
    Returns a dict: root, other, iters, funcalls, status, rebased (ntask each) and the slots as the call leaves them."""
    d = on_device(pb)
    n = len(rec)
    o = [Out(x.shape, x) for x in slots]
    oroot, oother = Out((n,), np.full(n, 7.25)), Out((n,), np.full(n, 7.25))
    oit, ofc, ost = IntOut(n, -7), IntOut(n, -7), IntOut(n, -7)
    args = (n, pb['N'], pb['P'], o[1], o[2], o[3], o[0], d['AWA'], d['R'], d['y'], vptr(rl), d['At'], d['W'], d['b'],
            dev(rec, np.int32), dev(slot, np.int32), dev(xa, np.float64), dev(xb, np.float64), dev(fa, np.float64),
            dev(fb, np.float64), dev(nu, np.float64), EPS, oroot, oother, oit, ofc, ost)
    if raw:                                              # the return code instead of an exception
        lib = _L().lib
        rc = lib.vi_brent_warm_f64(_ctx().handle, *[a.ptr if hasattr(a, 'ptr') else a for a in args])
        _ctx().sync()
    else:
        call('vi_brent_warm_f64', *args)
        rc = 0
    st = ost.get()
    return dict(rc=rc, root=oroot.get(), other=oother.get(), iters=oit.get(), funcalls=ofc.get(), status=st & 0xff if rc == 0 else st,
                rebased=st >> 8, V=o[0].get(), D1=o[1].get(), D2=o[2].get(), yt=o[3].get())


def brent_host(pb, slots, rec, slot, xa, xb, fa, fb, nu, rl):
    """vi_brent_host_one_f64 record after record on device copies of the same slots: brent_warm's dict."""
    d = on_device(pb)
    n, N = len(rec), pb['N']
    o = [Out(x.shape, x) for x in slots]
    scratch = _ctx().empty((N + 8,))
    res = np.zeros((n, 6))
    for i in range(n):
        call('vi_brent_host_one_f64', N, pb['P'], o[1], o[2], o[3], o[0], d['AWA'], d['R'], d['y'], vptr(rl), d['At'], d['W'],
             d['b'], int(rec[i]), int(slot[i]), float(xa[i]), float(xb[i]), float(fa[i]), float(fb[i]), float(nu[i]), EPS,
             scratch, vptr(res[i]))
    return dict(rc=0, root=res[:, 0].copy(), other=res[:, 1].copy(), iters=res[:, 2].astype(np.int32),
                funcalls=res[:, 3].astype(np.int32), status=res[:, 4].astype(np.int32), rebased=res[:, 5].astype(np.int32),
                V=o[0].get(), D1=o[1].get(), D2=o[2].get(), yt=o[3].get())


def differences(a, b, tag, tasks=None):
    """Every field of two result dicts compared bit for bit (the records `tasks` of the per-task fields): the failures."""
    t = slice(None) if tasks is None else tasks
    fails = [same(a[k][t], b[k][t], '%s %s' % (tag, k)) for k in ('root', 'other')]
    for k in ('iters', 'funcalls', 'status', 'rebased'):
        if not np.array_equal(a[k][t], b[k][t]):
            fails.append('%s %s: %r against %r' % (tag, k, a[k][t], b[k][t]))
    fails += [same(a[k], b[k], '%s slots %s' % (tag, k)) for k in ('V', 'D1', 'D2', 'yt')]
    return [f for f in fails if f]


# ==== 2. the library agrees with the restatement ============================================================================
@gpu
def test_supported_sizes_are_the_restated_ones():
    """vi_brent_warm_supported(N, P) for N = 1 .. 260, at P = 1, at sizes around 64 blocks and on both sides of the largest P
    the restatement admits for that N, equals 'the Jacobi range and brent_lds(N, P) <= 160 KB'.  The largest supported P of
    N = 192 is found by bisection on the library's own answer and compared with the restated one (it depends on
    sizeof(BrentState), which the restatement takes as 104)."""
    lib = _L().lib
    bad = []
    for N in range(1, 261):
        top = largest_p(N)
        probe = {1, 255, 16384, 16385, 16641, 10 ** 7} | ({top - 256, top - 1, top, top + 1, top + 256, top + 513} if top else set())
        for P in sorted(p for p in probe if p > 0):
            if lib.vi_brent_warm_supported(N, P) != int(brent_supported(N, P)):
                bad.append((N, P, brent_lds(N, P)))
    assert not bad, bad[:10]
    assert lib.vi_brent_warm_supported(0, 40) == 0 and lib.vi_brent_warm_supported(144, 0) == 0
    top_lib = largest_p(192, lambda N, P: lib.vi_brent_warm_supported(N, P) == 1)
    print('N 192: the library takes up to %d data points per record (%d blocks); restated %d' % (top_lib, top_lib // 256, largest_p(192)))
    assert top_lib == largest_p(192) and top_lib % 256 == 0


@gpu
@pytest.mark.parametrize('N,P', [(193, 40), (196, 257), (192, 0)])
def test_unsupported_sizes_are_refused_before_anything_is_written(N, P):
    """vi_brent_warm_f64 at N = 193 and 196 (the in-LDS solver serves them, the Brent workgroup does not fit) and at N = 192
    one block of points past its limit: VI_ERR_UNSUPPORTED, and the outputs and the slots keep what they held."""
    lib = _L().lib
    P = P or largest_p(192, lambda n, p: lib.vi_brent_warm_supported(n, p) == 1) + 1
    assert lib.vi_brent_warm_supported(N, P) == 0 and jacobi_class(N) != 'library'
    rng = np.random.default_rng(N)
    n = 2
    pb = dict(N=N, P=P, At=np.zeros((N, P)), W=np.ones((1, P)), b=np.zeros((1, P)), AWA=np.ones((1, N, N)), R=np.eye(N),
              y=np.ones((1, N)))
    slots = [rng.standard_normal(s) for s in ((n, N, N), (n, N, N), (n, N, N), (n, N))]
    z = np.zeros(n)
    r = brent_warm(pb, slots, np.zeros(n, np.int32), np.arange(n, dtype=np.int32), z - 3.0, z - 2.0, z - 1.0, z + 1.0, z + 5.0,
                   rule('default'), raw=True)
    assert r['rc'] == VI_ERR_UNSUPPORTED, r['rc']
    assert np.all(r['root'] == 7.25) and np.all(r['other'] == 7.25)
    assert all(np.all(r[k] == -7) for k in ('iters', 'funcalls', 'status'))
    for k, s in zip(('V', 'D1', 'D2', 'yt'), slots):
        assert np.array_equal(r[k], s), k


# ==== 3. roots known by construction ========================================================================================
_KNOWN = {}


def ref_solve(AWA, y, alpha):
    """(AWA + alpha I) C = y in 80-bit arithmetic as gcv_reference does it: float64 LU, three steps of refinement on 80-bit
    residuals.  Returns C (80-bit), the condition number of the system and its rank at the library's cut eps max|lambda|."""
    N = AWA.shape[0]
    X = AWA.astype(LD) + LD(alpha) * np.eye(N, dtype=LD)
    X64 = X.astype(np.float64)
    lam = np.linalg.eigvalsh(X64)
    C = np.linalg.solve(X64, y).astype(LD)
    for _ in range(3):
        C = C + np.linalg.solve(X64, (y.astype(LD) - X @ C).astype(np.float64)).astype(LD)
    return C, float(np.abs(lam).max() / np.abs(lam).min()), int((np.abs(lam) > EPS * np.abs(lam).max()).sum())


def ref_chi2(A_ld, W, b, C):
    """sum_p W_p (a_p . C - b_p)^2 in 80-bit arithmetic; A_ld is the basis (P, N) in 80 bits.  Also the residuals."""
    d = A_ld @ C - b.astype(LD)
    return np.sum(W.astype(LD) * d * d), d


def root_gate(At, W, b, C, d, kappa, nu, fprime, x0):
    """|root - x0| <= 2e-12 + 4 eps |x0| + (E + u nu) / |f'(x0)|: brentq's own tolerance, and the distance by which an error of
    E in chi^2 (and the rounding of nu) moves the root of a function of slope f'.  E bounds the kernel's chi^2 at the reference
    coefficients: E = sum_p W_p dm_p (2 |d_p| + dm_p) + gamma(10 + nb) sum_p W_p d_p^2 with dm_p = |a_p|_2 GCV_C kappa N u |C|_2 +
    gamma(N) sum_n |a_pn C_n| - gcv_gate's bound on a model value after a backward-stable eigen-solve of condition kappa, and
    chi2_reference's bound on the sum in blocks of 256 points.  Returns the gate and E."""
    N, P = At.shape
    nb = -(-P // 256)
    C64 = C.astype(np.float64)
    dm = np.linalg.norm(At, axis=0) * GCV_C * kappa * N * U * np.linalg.norm(C64) + gamma(N) * (np.abs(At) * np.abs(C64)[:, None]).sum(0)
    ad = np.abs(d).astype(np.float64)
    E = float(np.sum(W * dm * (2 * ad + dm)) + gamma(10 + nb) * np.sum(W * ad * ad))
    return XTOL + RTOL * abs(x0) + (E + U * nu) / abs(fprime), E


def known_problem(N, P, T=3):
    """T well-conditioned records that share gcv_problem's kind of basis - Gaussian, columns graded over 2.2 decades - with
    weights in 0.5 .. 1.5 per record, R = I, b = A c + noise.  Per record: alpha in the middle of the spectrum, x0 =
    floor(log10 lambda_mid) + frac with a seeded frac in (0.05, 0.95) and lambda_mid the median of the eigenvalues of A^T W A
    above N eps max (lambda_{N/2} where the record has full rank; records with P < N have N - P zero eigenvalues), and
    nu = chi^2(10^x0) in 80-bit arithmetic.  chi^2 of a ridge problem rises monotonically with alpha, so chi^2 - nu has its
    one root on the unit bracket [floor(x0), floor(x0) + 1] at x0, up to the rounding of nu.  Also per record: the slope
    f'(x0) (central difference of the 80-bit function over 2e-4 decades), the gate and E of root_gate."""
    key = (N, P, T)
    if key in _KNOWN:
        return _KNOWN[key]
    rng = np.random.default_rng([N, P, 7])
    grade = 10.0 ** (-2.2 * np.arange(N) / N)
    At = rng.standard_normal((N, P)) * grade[:, None]
    W = rng.uniform(0.5, 1.5, (T, P))
    c = rng.standard_normal((T, N)) / grade
    b = c @ At + 0.1 * rng.standard_normal((T, P))
    AWA = np.array([(At * W[t]) @ At.T for t in range(T)])
    AWA = 0.5 * (AWA + AWA.transpose(0, 2, 1))
    y = (W * b) @ At.T
    A_ld = np.ascontiguousarray(At.T).astype(LD)
    pb = dict(N=N, P=P, T=T, At=At, W=W, b=b, AWA=AWA, y=y, R=np.eye(N), x0=np.empty(T), nu=np.empty(T), gate=np.empty(T),
              E=np.empty(T), fprime=np.empty(T), kappa=np.empty(T))
    h = 1e-4
    for t in range(T):
        lam = np.linalg.eigvalsh(AWA[t])
        nz = lam[lam > N * EPS * lam[-1]]
        assert len(nz) == min(N, P), (N, P, len(nz))
        x0 = math.floor(math.log10(nz[len(nz) // 2])) + float(rng.uniform(0.05, 0.95))
        C, kappa, rank = ref_solve(AWA[t], y[t], LD(10) ** LD(x0))
        assert rank == N and kappa <= 1e4, (N, P, t, rank, kappa)             # the truncation keeps every eigenvalue
        nu, d = ref_chi2(A_ld, W[t], b[t], C)
        f = [ref_chi2(A_ld, W[t], b[t], ref_solve(AWA[t], y[t], LD(10) ** LD(x))[0])[0] - nu for x in (x0 - h, x0 + h)]
        assert f[0] < 0 < f[1]
        fprime = float((f[1] - f[0]) / (2 * h))
        pb['x0'][t], pb['nu'][t], pb['fprime'][t], pb['kappa'][t] = x0, float(nu), fprime, kappa
        pb['gate'][t], pb['E'][t] = root_gate(At, W[t], b[t], C, d, kappa, float(nu), fprime, x0)
    _KNOWN[key] = pb
    return pb


def host_root(pb, t, W=None, b=None, At=None, Vswap=None):
    """The root of chi^2 - nu of record t by the float64 iteration on the host: brentq_gen on a plain eigen-solve of
    AWA + alpha I, chi^2 summed by NumPy.  W, b, At: other data for the normal equations and chi^2 (an emulated fault);
    Vswap: two coefficients whose columns of the eigenvector matrix are exchanged before C = V c'."""
    from volumetricinterp_amd.alpha_search import brentq_gen
    At = pb['At'] if At is None else At
    W = pb['W'][t] if W is None else W
    b = pb['b'][t] if b is None else b
    AWA = (At * W) @ At.T
    y = At @ (W * b)

    def f(x):
        lam, V = np.linalg.eigh(0.5 * (AWA + AWA.T) + 10.0 ** x * np.eye(pb['N']))
        cp = (V.T @ y) / lam
        if Vswap is not None:                            # C = V c' with the vectors of two coefficients exchanged
            V[:, list(Vswap)] = V[:, list(Vswap)[::-1]]
        d = (V @ cp) @ At - b
        return float(np.sum(W * d * d)) - pb['nu'][t]
    xa = math.floor(pb['x0'][t])
    xb = xa + 1.0
    fa, fb = f(xa), f(xb)
    if not fa * fb < 0:                                  # a wrong function may have its root outside the unit bracket
        xa, xb = xa - 3.0, xb + 3.0
        fa, fb = f(xa), f(xb)
        if not fa * fb < 0:
            return None
    g = brentq_gen(xa, xb, fa, fb)
    try:
        x = next(g)
        while True:
            x = g.send(f(x))
    except StopIteration as e:
        return e.value[0]


def test_root_gate_rejects_emulated_wrong_answers():
    """On the host, at (N, P) = (9, 40), (50, 257) and (144, 2600): the float64 iteration lands inside the gate with a factor of
    ten to spare at least, the gate is far below any effect of a wrong index (chi^2 moves by per cents over the bracket), and
    it rejects the root found with another record's weights, with one data point dropped, and with one coefficient's column
    of V exchanged with its neighbour's (that function need not change sign at all)."""
    for N, P in ((9, 40), (50, 257), (144, 2600)):
        pb = known_problem(N, P)
        for t in range(pb['T']):
            x0, gate = pb['x0'][t], pb['gate'][t]
            r = host_root(pb, t)
            print('N %3d P %4d record %d: x0 %.15f float64 brentq off by %.2e, gate %.2e (E / nu %.1e, kappa %.0f, f\' / nu %.2f)'
                  % (N, P, t, x0, abs(r - x0), gate, pb['E'][t] / pb['nu'][t], pb['kappa'][t], pb['fprime'][t] / pb['nu'][t]))
            assert abs(r - x0) <= 0.1 * gate
            assert 2e-12 < gate <= 1e-6
            keep = np.ones(P, bool)
            keep[P // 2] = False
            wrong = {'weights': host_root(pb, t, W=pb['W'][(t + 1) % pb['T']]),
                     'point': host_root(pb, t, W=pb['W'][t][keep], b=pb['b'][t][keep], At=pb['At'][:, keep]),
                     'column': host_root(pb, t, Vswap=(N // 2, N // 2 + 1))}
            for what, w in wrong.items():
                assert w is None or abs(w - x0) > gate, (N, P, t, what, w, x0, gate)
            assert wrong['point'] is not None and wrong['weights'] is not None


def bracket_of_known(pb, slots):
    """The unit bracket of every record and the kernel's own function values at its ends (vi_warm_chi2_one_f64 from the slot
    of the record, as the engine asks for them)."""
    T = pb['T']
    dsl = [dev(x) for x in slots]
    xa = np.floor(pb['x0'])
    xb = xa + 1.0
    fa = np.array([warm_chi2_one(pb, dsl, t, t, exp10(xa[t]))[0] for t in range(T)]) - pb['nu']
    fb = np.array([warm_chi2_one(pb, dsl, t, t, exp10(xb[t]))[0] for t in range(T)]) - pb['nu']
    return xa, xb, fa, fb


def run_known(N, P, ntask, copies=0):
    """One case of part 3: the records of known_problem(N, P) - ntask of them, or with copies > 0 that many copies of the three
    records' systems in distinct slots, listed against the slot order - through vi_brent_warm_f64 under the engine's rule.
    Returns the result dict, the record of every task and the lines to print; asserts the gate, the status, the counts and the
    width of the final bracket."""
    T = ntask if not copies else 3
    pb = known_problem(N, P, T)
    mid = np.power(10.0, np.floor(pb['x0']) + 0.5)
    key = 'brent_slots'
    if key not in pb:
        C, rk, V, D1, D2, yt = warm_prepare(pb['AWA'], pb['R'], pb['y'], np.arange(T, dtype=np.int32), mid)
        assert np.all(rk == N)
        pb[key] = (V, D1, D2, yt)
        pb['bracket'] = bracket_of_known(pb, pb[key])
    xa, xb, fa, fb = pb['bracket']
    assert np.all(fa < 0) and np.all(fb > 0), (N, P, fa, fb)
    n = copies or T
    rec = (np.arange(n) % T).astype(np.int32)[::-1].copy()              # task i: record rec[i] from slot n - 1 - i
    slot = np.arange(n, dtype=np.int32)[::-1].copy()
    src = np.arange(n) % T                                              # slot s holds a copy of record s % T
    assert np.array_equal(src[slot], rec)
    slots = [x[src] for x in pb[key]]
    r = brent_warm(pb, slots, rec, slot, xa[rec], xb[rec], fa[rec], fb[rec], pb['nu'][rec], rule('default'))
    lines, fails = [], []
    for i in range(n):
        t = rec[i]
        dist = abs(r['root'][i] - pb['x0'][t])
        if i < T or dist > pb['gate'][t]:
            lines.append('known root N %3d P %5d (%s, nb %% nbp %d, npart %d) task %d of %d: |root - x0| %.2e, gate %.2e, |f| / nu at the '
                         'ends %.1e %.1e, %d iterations, %d re-basings' % (N, P, brent_geometry(N)[0], -(-P // 256) % brent_geometry(N)[2],
                                                                          brent_lds(N, P)[1], i, n, dist, pb['gate'][t], abs(fa[t]) / pb['nu'][t],
                                                                          abs(fb[t]) / pb['nu'][t], r['iters'][i], r['rebased'][i]))
        if not dist <= pb['gate'][t]:
            fails.append('task %d: root %.15f, x0 %.15f, gate %.2e' % (i, r['root'][i], pb['x0'][t], pb['gate'][t]))
        if r['status'][i] != 0 or not 1 <= r['funcalls'][i] <= 20 or not 1 <= r['iters'][i] <= 20:
            fails.append('task %d: status %d, %d iterations, %d function values' % (i, r['status'][i], r['iters'][i], r['funcalls'][i]))
        if not abs(r['other'][i] - r['root'][i]) <= 2 * (XTOL + RTOL * abs(r['root'][i])):
            # brentq also ends on an exact zero: the function at the root, from the slot as the kernel left it
            sl = [r[k][slot[i]][None] for k in ('V', 'D1', 'D2', 'yt')]
            Cr, _ = warm_solve(sl[1], sl[2], sl[3], sl[0], np.zeros(1, np.int32), np.array([exp10(r['root'][i])]))
            if chi2(pb['At'], Cr, None, pb['W'][t][None], pb['b'][t][None])[0] - pb['nu'][t] != 0.0:
                fails.append('task %d: final bracket %.3e wide' % (i, abs(r['other'][i] - r['root'][i])))
    print('\n'.join(lines))
    assert not fails, '\n'.join(['N %d P %d' % (N, P)] + fails)
    return pb, r, rec, slot


def ps_of(N):
    return sorted({P for M, P, n in known_cases() if M == N and n == 3})


@gpu
@pytest.mark.parametrize('N', SUPPORTED)
def test_known_roots_at_every_order(N):
    """Three records of known root at P = 40 and 257 (and at 1 or 255, 256, 550, 2600 for the orders of the chi^2-pass
    classes): |root - x0| within root_gate, status 0, at most 20 iterations and function values, the final bracket within
    brentq's tolerance, sentinels around every output and slot array intact.  At the reference coefficients the library's own
    chi^2 (vi_chi2_f64) lies within chi2_reference's bound of the 80-bit nu."""
    print('N %d: %s' % (N, CASES[N]))
    for P in ps_of(N):
        pb, r, rec, slot = run_known(N, P, 3)
        t = 0
        C = ref_solve(pb['AWA'][t], pb['y'][t], LD(10) ** LD(pb['x0'][t]))[0].astype(np.float64)
        ref, bound = chi2_reference(pb['At'], C, pb['W'][t], pb['b'][t])
        out = chi2(pb['At'], C[None], None, pb['W'][t][None], pb['b'][t][None])[0]
        assert abs(LD(out) - ref) <= LD(bound) and abs(ref - LD(pb['nu'][t])) <= LD(bound), (N, P, out, float(ref), pb['nu'][t])


@gpu
@pytest.mark.parametrize('N,P', [(9, 40), (144, 257)])
def test_known_root_of_a_single_task(N, P):
    """One task, one workgroup."""
    run_known(N, P, 1)


@gpu
@pytest.mark.parametrize('P', BIG_PS)
def test_known_roots_with_64_65_66_blocks_of_points(P):
    """N = 9 with nb = 64, 65 and 66 blocks of 256 points: part[] has 64, 66 and 66 entries (the even rounding of npart)."""
    assert brent_lds(9, P)[1] == (64 if P == BIG_PS[0] else 66)
    run_known(9, P, 2)


@gpu
def test_known_roots_at_the_top_of_lds():
    """N = 192 at the largest record the library admits (found by bisection on its own answer; 35 328 points with a 104-byte
    state and 256 bytes of static LDS): the workgroup's LDS ends within 16 bytes of the 160 KB limit and part[] next to it."""
    lib = _L().lib
    P = largest_p(192, lambda n, p: lib.vi_brent_warm_supported(n, p) == 1)
    assert P == largest_p(192) and LDS_LIMIT - brent_lds(192, P)[0] < 16
    print('N 192 P %d: %d of %d bytes of LDS, part[%d]' % (P, brent_lds(192, P)[0], LDS_LIMIT, brent_lds(192, P)[1]))
    run_known(192, P, 2)
    _KNOWN.pop((192, P, 2))                                             # a 54 MB basis and its 80-bit copy


@gpu
@pytest.mark.parametrize('N,P', [(9, 40), (100, 257)])
def test_more_tasks_than_workgroups(N, P):
    """n_cu + 37 tasks: copies of three records' systems in distinct slots, tasks listed against the slot order.  Every copy
    must leave with the bits its record gets in a launch of three - root, other end, counts, status and the slot it moved -
    whichever workgroup served it and whatever that workgroup ran before; and the roots are the known ones."""
    n_cu = n_cu_of_device()
    n = n_cu + 37
    pb, alone, rec3, slot3 = run_known(N, P, 3)
    pb, r, rec, slot = run_known(N, P, 3, copies=n)
    first = {int(t): i for i, t in enumerate(rec3)}
    fails = []
    for i in range(n):
        j = first[int(rec[i])]
        for k in ('root', 'other', 'iters', 'funcalls', 'status', 'rebased'):
            if not np.array_equal(r[k][i:i + 1].view(np.uint8), alone[k][j:j + 1].view(np.uint8)):
                fails.append('task %d (record %d) %s: %r, alone %r' % (i, rec[i], k, r[k][i], alone[k][j]))
        for k in ('V', 'D1', 'D2', 'yt'):
            if not np.array_equal(r[k][slot[i]], alone[k][slot3[j]]):
                fails.append('task %d (record %d): slot array %s differs' % (i, rec[i], k))
    assert not fails, '\n'.join(fails[:20])
    assert alone['rebased'].max() >= 1                                   # the copies' slots did move


# ==== 4. the implementations agree bit for bit ==============================================================================
def real_name(N):
    return {32: 'k8l2', 144: 'c144'}.get(N, 'n196:%d' % N)


def real_brackets(name):
    """Per record 0 .. NREC - 1 of a real problem, the way the engine takes them: the unit bracket around alpha0 (where
    prepared_slots set the rotated systems up), nu = chi^2 at a seeded point inside it, the function values at the ends by
    vi_warm_chi2_one_f64.  keep: the ends differ in sign (chi^2 of the graded problems is not monotone where eigenvalues cross
    the truncation cut, so the seed of a record is the first of eight draws that leaves a sign change)."""
    q, slots = prepared_slots(name, NREC)
    if 'brent_brackets' not in q:
        rng = np.random.default_rng(q['N'])
        dsl = [dev(x) for x in slots]
        x0 = math.log10(q['alpha0'])
        xa, xb = np.full(NREC, x0 - 0.5), np.full(NREC, x0 + 0.5)
        val = np.empty((NREC, 3, 2))
        for t in range(NREC):
            val[t, 0], val[t, 1] = warm_chi2_one(q, dsl, t, t, exp10(xa[t])), warm_chi2_one(q, dsl, t, t, exp10(xb[t]))
            for _ in range(8):                           # the seed: the first of eight draws that leaves a sign change
                val[t, 2] = warm_chi2_one(q, dsl, t, t, exp10(xa[t] + rng.uniform(0.15, 0.85)))
                if (val[t, 0, 0] - val[t, 2, 0]) * (val[t, 1, 0] - val[t, 2, 0]) < 0:
                    break
        nu = val[:, 2, 0]
        fa, fb = val[:, 0, 0] - nu, val[:, 1, 0] - nu
        q['brent_brackets'] = dict(xa=xa, xb=xb, fa=fa, fb=fb, nu=nu, keep=(fa * fb < 0), sweeps=val[:, :, 1].astype(int))
    return q, slots, q['brent_brackets']


SLOT_OF_REC = np.array([4, 0, 5, 2], np.int32)          # six slots: 1 and 3 are not listed and hold a pattern
TASK_ORDER = [2, 0, 3, 1]
PATTERN = 12345.678


def real_tasks(name):
    """The slot arrays (6 slots) and the task arrays of a real problem: records listed in TASK_ORDER from the slots
    SLOT_OF_REC - rec and slot are different permutations, neither in order."""
    q, prep, br = real_brackets(name)
    assert (~br['keep']).sum() <= NREC // 4, (name, br['fa'], br['fb'])                 # the cap on dropped records
    slots = []
    for x in prep:
        s = np.full((6,) + x.shape[1:], PATTERN)
        s[SLOT_OF_REC] = x
        slots.append(s)
    rec = np.array([t for t in TASK_ORDER if br['keep'][t]], np.int32)
    return q, slots, rec, SLOT_OF_REC[rec], br


@gpu
@pytest.mark.parametrize('N', SUPPORTED)
def test_device_brent_is_the_host_loop_bit_for_bit(N):
    """vi_brent_warm_f64 against vi_brent_host_one_f64 on copies of the same slots, record by record: root, other end,
    iterations, function values, status, re-basings and the slots V, D1, D2, yt as either leaves them, bit for bit - under the
    engine's rule, without re-basing, and with a move at each of the first four iterates (rebase_call and its four wg_gemm
    products at every order).  The host loop runs the stand-alone kernels (k_jacobi_solve*, k_wg_gemm tiled, vi_chi2_f64):
    this pins the kernel's in-place copies of all of them.  Slots that no task lists keep their pattern."""
    name = real_name(N)
    q, slots, rec, slot, br = real_tasks(name)
    assert q['N'] == N and q['P'] == P_REAL.get(N, 2600) and len(rec) >= 3
    fails = []
    for rn in RULES:
        args = (q, slots, rec, slot, br['xa'][rec], br['xb'][rec], br['fa'][rec], br['fb'][rec], br['nu'][rec], rule(rn))
        d, h = brent_warm(*args), brent_host(*args)
        print('N %3d %-7s %-40s iterations %r re-basings %r status %r' % (N, rn, CASES[N][:40], list(d['iters']), list(d['rebased']), list(d['status'])))
        fails += differences(d, h, 'N %d rule %s: device against host loop,' % (N, rn))
        for res in (d, h):
            for k in ('V', 'D1', 'D2', 'yt'):
                if not np.all(res[k][[1, 3]] == PATTERN):
                    fails.append('N %d rule %s: an unlisted slot of %s was written' % (N, rn, k))
        assert np.all(d['status'] == 0) and np.all(d['funcalls'] >= 2), (N, rn, d['status'], d['funcalls'])
        if rn == 'none':
            assert np.all(d['rebased'] == 0) and all(np.array_equal(d[k], s) for k, s in zip(('V', 'D1', 'D2', 'yt'), slots))
        if rn == 'four':
            assert d['rebased'].max() >= 1 and not np.array_equal(d['V'], slots[0]), (N, d['rebased'])
    assert not fails, '\n'.join(fails)


SWEEP_CAP_CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import test_gpu_brent_geometry as g
z = dict(np.load(sys.argv[1]))
assert g._L().lib.vi_max_sweeps() == 4, g._L().lib.vi_max_sweeps()
out = {}
for N in (50, 144):
    pb = {k: z["%%d_%%s" %% (N, k)] for k in ("At", "W", "b", "AWA", "R", "y")}
    pb["N"], pb["P"] = pb["At"].shape
    slots = [z["%%d_%%s" %% (N, k)] for k in ("V", "D1", "D2", "yt")]
    t = [z["%%d_%%s" %% (N, k)] for k in ("rec", "slot", "xa", "xb", "fa", "fb", "nu")]
    for rn in ("default", "none"):
        d = g.brent_warm(pb, slots, *t, g.rule(rn))
        h = g.brent_host(pb, slots, *t, g.rule(rn))
        for k, v in d.items():
            out["%%d_%%s_dev_%%s" %% (N, rn, k)] = np.asarray(v)
        for k, v in h.items():
            out["%%d_%%s_host_%%s" %% (N, rn, k)] = np.asarray(v)
np.savez(sys.argv[2], **out)
'''


@gpu
def test_sweep_cap_sends_records_back_with_status_2(tmp_path):
    """With the solver's sweep cap at its lowest (VINTERP_MAX_SWEEPS=2 is clamped to 4; read once per process, hence one child
    process) a solve far from where the rotated system was set up does not converge and its record leaves with status 2 -
    a return code, after which the host iterates that record itself.  The rotated systems and the bracket-end values are made
    here, under the default cap (under a cap of 4 vi_warm_prepare_f64 itself would stop early); the child runs the kernel and
    the host loop on them at N = 50 and N = 144: same statuses, same counts, same bits for every record - those served after a
    record of status 2 in the same launch included - and at least one record of status 2."""
    data = {}
    for N in (50, 144):
        q, slots, rec, slot, br = real_tasks(real_name(N))
        for k in ('At', 'W', 'b', 'AWA', 'R', 'y'):
            data['%d_%s' % (N, k)] = q[k][:NREC] if k in ('W', 'b', 'AWA', 'y') else q[k]
        for k, v in zip(('V', 'D1', 'D2', 'yt'), slots):
            data['%d_%s' % (N, k)] = v
        for k, v in zip(('rec', 'slot', 'xa', 'xb', 'fa', 'fb', 'nu'),
                        (rec, slot, br['xa'][rec], br['xb'][rec], br['fa'][rec], br['fb'][rec], br['nu'][rec])):
            data['%d_%s' % (N, k)] = v
    np.savez(tmp_path / 'in.npz', **data)
    script = tmp_path / 'sweep_cap.py'
    script.write_text(SWEEP_CAP_CHILD % (REPO_ROOT, REPO_ROOT))
    env = dict(os.environ, VINTERP_MAX_SWEEPS='2')
    p = subprocess.run([sys.executable, str(script), str(tmp_path / 'in.npz'), str(tmp_path / 'out.npz')], env=env,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    z = np.load(tmp_path / 'out.npz')
    fails, n2, after = [], 0, 0
    for N in (50, 144):
        for rn in ('default', 'none'):
            d = {k: z['%d_%s_dev_%s' % (N, rn, k)] for k in ('root', 'other', 'iters', 'funcalls', 'status', 'rebased', 'V', 'D1', 'D2', 'yt')}
            h = {k: z['%d_%s_host_%s' % (N, rn, k)] for k in d}
            print('N %3d %-7s status %r function values %r (host loop %r %r)' % (N, rn, list(d['status']), list(d['funcalls']),
                                                                               list(h['status']), list(h['funcalls'])))
            fails += differences(d, h, 'N %d rule %s under the cap:' % (N, rn))
            assert set(d['status']) <= {0, 2}
            n2 += int((d['status'] == 2).sum())
            two = np.nonzero(d['status'] == 2)[0]
            after += int(len(two) and two[0] < len(d['status']) - 1)
    assert not fails, '\n'.join(fails)
    assert n2 >= 1 and after >= 1, (n2, after)


@gpu
@pytest.mark.parametrize('N', [32, 100, 157, 192, 193])
def test_engine_with_device_and_with_numpy_brent(N, monkeypatch):
    """A batch of 12 records through FitEngine.fit with VINTERP_DEVICE_BRENT=1 and =0 (the NumPy iteration,
    alpha_search.BrentBatch - the third implementation): alpha, chi^2, coefficients and iteration counts bit for bit, and
    device_brent_records grows by at least half the batch.  At N = 193 the engine reports the device path off and the fit
    gives the same answers as at =0."""
    from volumetricinterp_amd.fitengine import FitEngine
    q = problem(real_name(N))
    T, P = 12, q['P']
    eng = FitEngine(_ctx(), dev(q['At']), P, N, {'curvature': q['R']}, ['curvature'])
    W, b = q['W'][:T], q['b'][:T]
    try:
        monkeypatch.setenv('VINTERP_DEVICE_BRENT', '1')
        if N == 193:
            assert not eng.device_brent_enabled() and _L().lib.vi_brent_warm_supported(N, P) == 0
        n0 = eng.stats.get('device_brent_records', 0)
        d = eng.fit(W, b, [P] * T)
        grown = eng.stats.get('device_brent_records', 0) - n0
        monkeypatch.setenv('VINTERP_DEVICE_BRENT', '0')
        h = eng.fit(W, b, [P] * T)
        assert eng.stats.get('device_brent_records', 0) - n0 == grown
    finally:
        eng.close()
    print('N %d: %d of %d records through the device kernel, outcomes %r' % (N, grown, T, d['search']['curvature']['outcomes']))
    for t in range(T):
        a1, a2 = d['reg_params'][t]['curvature'], h['reg_params'][t]['curvature']
        i1, i2 = d['search']['curvature']['info'][t], h['search']['curvature']['info'][t]
        assert i1.get('iterations') == i2.get('iterations') and i1.get('other_end') == i2.get('other_end'), (N, t, i1, i2)
        assert a1 == a2 or (np.isnan(a1) and np.isnan(a2)), (N, t, a1, a2)
        assert np.array_equal(d['Coeffs'][t], h['Coeffs'][t], equal_nan=True), (N, t)
        assert d['chi_sq'][t] == h['chi_sq'][t] or np.isnan(a1), (N, t)
    assert (grown == 0) if N == 193 else (grown >= T // 2), (N, grown)


@gpu
@pytest.mark.parametrize('N', [187, 192])
def test_engine_search_at_the_orders_of_the_three_block_kernel(N, monkeypatch):
    """FitEngine at N = 187 and 192 (the rotated-system search used to end at 180; warm_enabled() now reaches the kernel's last
    order and stops there): a batch of 12 goes through the shared-basis walk (k_walk_rotate without padding at 192 = 16 x 12),
    the re-basing and the device kernel - the same bits with the walk solved cold, records 0 and 7 the same alone as in the
    batch, the same outcomes as the search on cold solves alone (VINTERP_WARM=0), and chi^2 on the search's target within 1e-4
    or flagged as a jump, the gate of test_largest_in_lds_order_goes_through_the_batched_search at N = 180."""
    from volumetricinterp_amd.fitengine import FitEngine
    q = problem(real_name(N))
    T, P = 12, q['P']
    W, b = q['W'][:T], q['b'][:T]
    eng = FitEngine(_ctx(), dev(q['At']), P, N, {'curvature': q['R']}, ['curvature'])
    try:
        assert eng.warm_enabled()
        eng.N = 193
        assert not eng.warm_enabled()
        eng.N = N
        full = eng.fit(W, b, [P] * T)
        assert eng.stats.get('shared_solves', 0) > 0 and eng.stats.get('device_brent_records', 0) >= T // 2
        monkeypatch.setenv('VINTERP_SHAREDWALK', '0')
        cold_walk = eng.fit(W, b, [P] * T)
        monkeypatch.delenv('VINTERP_SHAREDWALK')
        ones = {t: eng.fit(W[t:t + 1], b[t:t + 1], [P]) for t in (0, 7)}
        monkeypatch.setenv('VINTERP_WARM', '0')
        cold = eng.fit(W, b, [P] * T)
    finally:
        eng.close()
    assert np.array_equal(full['Coeffs'], cold_walk['Coeffs'], equal_nan=True)
    assert np.array_equal(full['chi_sq'], cold_walk['chi_sq'], equal_nan=True)
    for t, one in ones.items():
        assert np.array_equal(one['Coeffs'][0], full['Coeffs'][t], equal_nan=True), t
    inf = full['search']['curvature']
    assert inf['outcomes'] == cold['search']['curvature']['outcomes']
    nroot = 0
    for t in range(T):
        if inf['outcomes'][t] == 'root':
            nroot += 1
            nu = inf['info'][t]['sf'] * P
            print('N %d record %2d: chi^2 / nu - 1 = %.2e (cold solves alone %.2e), log10 alpha %.12f (%.12f)'
                  % (N, t, full['chi_sq'][t] / nu - 1, cold['chi_sq'][t] / nu - 1,
                     np.log10(full['reg_params'][t]['curvature']), np.log10(cold['reg_params'][t]['curvature'])))
            assert abs(full['chi_sq'][t] - nu) <= 1e-4 * nu or inf['info'][t].get('jump'), (t, full['chi_sq'][t], nu)
            assert abs(cold['chi_sq'][t] - nu) <= 1e-4 * nu or cold['search']['curvature']['info'][t].get('jump'), t
    assert nroot >= T // 2
