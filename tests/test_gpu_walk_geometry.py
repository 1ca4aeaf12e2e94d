"""The forming step of the shared-basis bracket walk (csrc/vi_walk.hip, kernel K_walk; or the library chain of csrc/vi_fit.hip
with VINTERP_WALK_FORM=blas) on its own, through the stage-test entry vi_walk_form_f64, at every launch shape and against
answers known by construction:

    X[i] = f (V A V^T + alpha D2),  scl[i] = 1 / f,  yt[i] = V y        A = AWA[rec[i]], V = V[basis[i]], D2 = D2[basis[i]]

with f the power of two that brings max|X| into [1, 2).  K_walk is chosen from N alone out of 25 template instantiations;
walk_geometry below restates the switch at the foot of vi_walk.hip:

  NT = ceil(N / 16) waves, one per block of 16 columns, NT = 1 .. 13; each NT has an exact variant (N = 16 NT) and a padded
  one (loads past N go to clamped addresses and are multiplied by zero).  Through NT = 8 the operands are held in registers
  (resident); at N = 144 the last KL = 16 k-steps of V are parked in LDS; at N = 129 .. 143 and from N = 145 on the operands are
  fetched at every use.  Of X only the lower block triangle (column < 16 (row / 16 + 1)) is written; the maximum is taken over
  it.  The library chain writes all of X and takes the maximum over all of it.

Part 1 (no GPU) asserts that the case list reaches every instantiation the switch can reach - both sides of every NT
boundary, all four residues of N mod 4 (how much of the last k-step of 4 is real) in a padded resident, a padded NT = 9 and a
padded non-resident variant - prints the case table, and shows on the host that every gate of parts 2 and 3 rejects emulated
wrong answers: a dropped k-step, a transposed tile, the neighbouring slot's D2, f off by 2, V transposed in yt, a stray store,
an unwritten element.  The issue's list of orders lacked N mod 4 = 2 in the padded resident and non-resident variants and
N mod 4 = 0 in the padded NT = 9 one; 30, 140 and 150 were added for them.
Part 2: integer inputs small enough that every summation order is exact (the bound is stated and asserted per N), so scl X,
scl and yt must have NumPy's bits; signed permutations and one-hot matrices pin the index maps at the corners and edges of
every 16-block; every output lies between GUARD sentinels and X starts as sentinels, so that an element above the block
diagonal is either untouched or right; IEEE cases (zero system, alpha = 0, f = 1 at max|X| >= 1.7e308, tiny systems, NaN and
Inf records); orders out of range.  Part 3: systems of real magnitudes (weights of 1e-22) pointwise against an 80-bit
reference within a derived bound, and the bits of one triple across batches.  Part 4: through vi_basis_solve_f64 at nine more
orders.  Parts 2 and 3 run a second time in a child process with VINTERP_WALK_FORM=blas (the setting is read once per
process), part 4 in a child with VINTERP_WALK_TOL=0: this file is also those children's script.

The bound of part 3.  Either way of forming computes d^ = fl(fl(V A) V^T) (or fl(V fl(A V^T))), two chained products whose
elements are sums of N terms in some order, fused or not: |fl(V A) - V A| <= gamma(N) |V||A|, and the second product adds
gamma(N) |fl(V A)||V|^T, so |d^ - d| <= (2 gamma(N) + gamma(N)^2) S <= gamma(2N) S with S = |V||A||V|^T (zeros of the padding
add nothing).  Then v = fma(alpha, D2, d^) = (alpha D2 + d^)(1 + delta), |delta| <= u: |v - E| <= gamma(2N) S + u (|E| +
gamma(2N) S) <= gamma(2N + 1) S + u |E|, and the scaling by f and back by scl is exact.  The gate is the slightly wider
gamma(2N + 2) S + 3u |E| that the suite was asked to hold.  yt[k] is one fma chain of ceil(N / 64) terms per lane and a tree
of six additions: gamma(N + 6) (|V||y|)_k covers it.  The reference runs in numpy.longdouble (64-bit significand, unit
roundoff 2^-64): its own error is below (2N + 2) 2^-64 S + 2^-63 (|alpha D2| + |E|), asserted to be under 1/100 of the gate at
every element.

Findings.
  * f = ldexp(1, 1 - ex) overflowed to infinity for a system with max|X| < 2^-1023 (k_walk_rotate, k_form_pair_scaled,
    k_scale_system alike): X came out as Inf / NaN and scl as 0 (test_tiny_systems; integer inputs times 2^-1040).  The exponent
    is now capped so that f <= 2^1023 in the three kernels; no system with max|X| >= 2^-1023 changes a bit
    (k_brent_warm in vi_brent.hip holds a fourth copy of the expression, which no entry tested here reaches; it is as it was).
  * The systems of a record with one Inf in A depended on who formed them: +-Inf at every element from the exact K_walk
    variants and from the library chain (IEEE arithmetic: V A V^T is +-Inf wherever both factors of V that meet the Inf are
    non-zero; N = 196: 62 256 Inf, 0 NaN), but NaN all over from a padded K_walk variant with the Inf in the last row or
    column, which its clamped loads multiply by zero (test_a_record_with_an_inf failed on all of them but the last).  The
    scaling pass of the three kernels now writes NaN all over a system whose maximum is infinite - the same answer as for a
    record with a NaN, at every order and either way of forming; scl stays 1 and no system with a finite maximum changes a
    bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_resident_geometry import GUARD, SENTINEL, U, gamma, two_prod, fsum2, mismatch  # noqa: F401
from test_gpu_solver_geometry import jacobi_class

gpu = pytest.mark.gpu
EPS = np.finfo(float).eps
LD = np.longdouble
SB = np.array([SENTINEL]).view(np.uint64)[0]
VI_ERR_UNSUPPORTED = -6

NS = [8, 9, 15, 16, 17, 30, 31, 32, 33, 47, 48, 49, 64, 65, 75, 80, 81, 96, 97, 111, 112, 113, 127, 128,
      129, 130, 135, 140, 143, 144,
      145, 147, 150, 159, 160, 161, 176, 177, 180, 191, 192, 193, 196]
ADDED = (30, 140, 150)                 # not in the issue's list: the residues of N mod 4 it lacked
KINDS = {'resident exact': 64, 'resident padded': 75, 'N = 144': 144, 'NT = 9 padded': 135, 'non-resident': 180}
SOLVE_NS = [16, 64, 128, 135, 147, 160, 176, 192, 196]
KS = np.array([0., -10., -22., -26., -30., -40.])


# ==== 1. launch geometry ====================================================================================================
def walk_geometry(N):
    """The switch of vi_walk_rotate: VI_W(NT, RES, KL, RESP) with RES / KL of the exact order 16 NT and RESP of the padded ones."""
    NT = (N + 15) // 16
    assert 1 <= NT <= 13
    pad = N != 16 * NT
    res = NT <= 8 or (NT == 9 and not pad)
    KL = 16 if (NT == 9 and not pad) else 0
    kind = ('N = 144' if KL else 'resident padded' if res and pad else 'resident exact' if res else
            'NT = 9 padded' if NT == 9 else 'non-resident')
    return dict(NT=NT, res=res, KL=KL, pad=pad, waves=NT, threads=64 * NT, m4=N % 4, m16=N % 16, kind=kind,
                inst=(NT, pad), cls='NT %2d %-8s %-6s KL %2d  %3d thr  N%%4 %d N%%16 %2d'
                % (NT, 'resident' if res else 'fetched', 'padded' if pad else 'exact', KL, 64 * NT, N % 4, N % 16))


def b_list(N):
    """Batch sizes of part 2: 300 is more than one round of the 256 CUs."""
    return [1, 5, 300] + ([3000] if N <= 32 else [])


def case_table():
    return ['walk N %3d  %s  %-15s B %s' % (N, walk_geometry(N)['cls'], walk_geometry(N)['kind'], b_list(N)) for N in NS]


def test_geometry_list_covers_every_instantiation():
    """The list reaches each of the 25 instantiations (NT = 1 .. 13, exact and padded, but for NT = 13 exact = 208, beyond
    K3), both sides of every NT boundary, every residue of N mod 4 in each padded kind; prints the case table."""
    print('\n'.join(case_table()))
    g = {N: walk_geometry(N) for N in NS}
    want = {(NT, pad) for NT in range(1, 14) for pad in (False, True)} - {(13, False)}
    assert {x['inst'] for x in g.values()} == want and len(want) == 25
    assert jacobi_class(208) == 'library' and jacobi_class(197) == 'library' and jacobi_class(7) == 'library'
    assert all(jacobi_class(N) != 'library' for N in NS) and min(NS) == 8 and max(NS) == 196
    for NT in range(1, 13):
        assert 16 * NT in NS and 16 * NT + 1 in NS, NT
        assert g[16 * NT]['NT'] == NT and g[16 * NT + 1]['NT'] == NT + 1
    for kind in ('resident padded', 'NT = 9 padded', 'non-resident'):
        assert {x['m4'] for x in g.values() if x['kind'] == kind} == {0, 1, 2, 3}, kind
    assert all(g[N]['kind'] == kind for kind, N in KINDS.items())
    assert {x['kind'] for x in g.values()} == set(KINDS)
    assert all(x['res'] for N, x in g.items() if N <= 128) and g[144]['res'] and g[144]['KL'] == 16
    assert not any(x['res'] for N, x in g.items() if 129 <= N <= 143 or N >= 145)
    assert {N for N in NS if g[N]['pad'] and g[N]['res']} >= {8, 9, 15, 127} and not g[192]['pad'] and g[196]['pad']
    assert set(SOLVE_NS) <= set(NS) and {walk_geometry(N)['kind'] for N in SOLVE_NS} >= {'resident exact', 'NT = 9 padded',
                                                                                         'non-resident'}
    assert set(NS) - set(ADDED) == {8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 75, 80, 81, 96, 97, 111, 112, 113, 127,
                                    128, 129, 130, 135, 143, 144, 145, 147, 159, 160, 161, 176, 177, 180, 191, 192, 193, 196}
    for N in NS:
        assert N * N * 2 ** (3 * bits_of(N)) < 2 ** 52


def lbt(N):
    """The lower block triangle: (row, column) with column < 16 (row / 16 + 1)."""
    r = np.arange(N)
    return r[None, :] < 16 * (r[:, None] // 16 + 1)


def corner_pairs(N):
    """(row, column) in X, row's block >= column's block: the four corners of every 16-block of the lower block triangle (the
    last valid row and column included) and, on the diagonal blocks and the last block row, two points on the edges."""
    NT = (N + 15) // 16
    out = []
    for I in range(NT):
        r0, r1 = 16 * I, min(16 * I + 15, N - 1)
        for J in range(I + 1):
            c0, c1 = 16 * J, min(16 * J + 15, N - 1)
            out += [(r0, c0), (r0, c1), (r1, c0), (r1, c1)]
            if I == J or I == NT - 1:
                out += [((r0 + r1) // 2, c0), (r1, (c0 + c1 + 1) // 2)]
    return sorted(set(out))


# ==== the gates =============================================================================================================
def expected_scl(mx):
    """scl = 1 / f of a system with maximum mx: f = 2^(1 - ex) for mx = m 2^ex, m in [0.5, 1), capped at 2^1023 (the largest
    power of two; only a system with mx < 2^-1023 meets the cap); f = 1 for the zero system, for mx >= 1.7e308 and for a system
    whose every element is NaN (the device's fmax skips NaN)."""
    mx = np.asarray(mx, np.float64)
    _, ex = np.frexp(mx)
    ok = (mx > 0) & (mx < 1.7e308)
    return np.where(ok, np.ldexp(1.0, np.maximum(ex - 1, -1023)), 1.0)


def name_first(bad, what, got, want):
    b = np.argwhere(bad)
    i = tuple(int(x) for x in b[0])
    return '%s: %d of %d wrong, first %r: got %r, want %r' % (what, len(b), bad.size, i, float(got[i]), float(want[i]))


def same_bits(a, b):
    a, b = a + 0.0, b + 0.0                                          # -0.0 is 0.0 here
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def check_exact(tag, X, scl, yt, E, Eyt):
    """Failures of a device result against the exact E = V A V^T + alpha D2 (B, N, N) and Eyt = V y, each naming its first
    element: scl is the power of two of max|E| over the lower block triangle; there scl X has E's bits and nothing is left
    unwritten; above it an element is the sentinel it was or has E's bits; yt has Eyt's bits."""
    B, N = Eyt.shape
    m = np.broadcast_to(lbt(N), (B, N, N))
    fails = []
    with np.errstate(all='ignore'):
        mx = np.fmax.reduce(np.where(m, np.abs(E), 0.0).reshape(B, -1), axis=1, initial=0.0)
        sref = expected_scl(mx)
        Xs = X * scl[:, None, None]
    if not same_bits(scl, sref).all():
        fails.append(name_first(~same_bits(scl, sref), tag + ' scl [system]', scl, sref))
    sent = X.view(np.uint64) == SB
    if (m & sent).any():
        fails.append(name_first(m & sent, tag + ' X not written in the lower block triangle [system, row, column]', X, E))
    ok = same_bits(Xs, E)
    if (m & ~ok & ~sent).any():
        fails.append(name_first(m & ~ok & ~sent, tag + ' scl X [system, row, column]', Xs, E))
    if (~m & ~ok & ~sent).any():
        fails.append(name_first(~m & ~ok & ~sent, tag + ' stray store above the block diagonal [system, row, column]', Xs, E))
    if not same_bits(yt, Eyt).all():
        fails.append(name_first(~same_bits(yt, Eyt), tag + ' yt [system, k]', yt, Eyt))
    return fails


def real_reference(AWA, V, D2, y, rec, bas, al):
    """E = V A V^T + alpha D2 and V y of the triples in 80-bit arithmetic, S = |V||A||V|^T, the gates' bounds, and the assertion
    that the reference's own error is under 1/100 of them."""
    assert np.finfo(LD).eps <= 2.0 ** -63
    B, N = len(rec), V.shape[-1]
    E, S, Ey, Sy = np.empty((B, N, N), LD), np.empty((B, N, N)), np.empty((B, N), LD), np.empty((B, N))
    memo = {}
    for i, (r, k, a) in enumerate(zip(rec, bas, al)):
        if (r, k) not in memo:
            Vl = V[k].astype(LD)
            memo[r, k] = (Vl @ (AWA[r].astype(LD) @ Vl.T), np.abs(V[k]) @ np.abs(AWA[r]) @ np.abs(V[k]).T,
                          Vl @ y[r].astype(LD), np.abs(V[k]) @ np.abs(y[r]))
        d, S[i], Ey[i], Sy[i] = memo[r, k]
        E[i] = d + LD(a) * D2[k].astype(LD)
    aE = np.abs(E).astype(np.float64)
    bound = gamma(2 * N + 2) * S + 3 * U * aE
    # 80-bit arithmetic rounds to 2^-64: the chain (2N + 1) 2^-64 S (as above), the product alpha D2 and the sum one rounding each
    own = (2 * N + 2) * 2.0 ** -64 * S + 2.0 ** -63 * (np.abs(al)[:, None, None] * np.abs(D2[bas]) + aE)
    assert np.all(own <= bound / 100), 'the reference is not 100 times better than the gate'
    return dict(E=E, S=S, bound=bound, Ey=Ey, ybound=gamma(N + 6) * Sy, aE=aE)


def scl_choices(ref):
    """Per system the powers of two that the gate allows for scl: those of the smallest and the largest value the computed
    maximum can take within the bound, over the lower block triangle (K_walk) and over the whole matrix (the library chain)."""
    B, N = ref['Ey'].shape
    out = []
    for region in (np.broadcast_to(lbt(N), (B, N, N)), np.ones((B, N, N), bool)):
        lo = np.where(region, ref['aE'] - ref['bound'], 0.0).reshape(B, -1).max(1)
        hi = np.where(region, ref['aE'] + ref['bound'], 0.0).reshape(B, -1).max(1)
        out += [expected_scl(lo), expected_scl(hi)]
    return np.array(out)                                             # (4, B)


def check_real(tag, X, scl, yt, ref):
    """(failures, per system the worst ratio error / bound over the lower block triangle, worst ratio of yt)."""
    B, N = yt.shape
    m = np.broadcast_to(lbt(N), (B, N, N))
    fails = []
    ch = scl_choices(ref)
    okS = (scl[None, :] == ch).any(0)
    if not okS.all():
        fails.append(name_first(~okS, tag + ' scl [system]', scl, ch[0]))
    sent = X.view(np.uint64) == SB
    if (m & sent).any():
        fails.append(name_first(m & sent, tag + ' X not written in the lower block triangle [system, row, column]', X, ref['E']))
    with np.errstate(all='ignore'):
        Xs = X * scl[:, None, None]                                  # exact: scl is a power of two
        err = np.abs(Xs.astype(LD) - ref['E']).astype(np.float64)
    bad = ~(np.isfinite(Xs) & (err <= ref['bound']))
    if (m & bad & ~sent).any():
        fails.append(name_first(m & bad & ~sent, tag + ' scl X outside the bound [system, row, column]', Xs, ref['E']))
    if (~m & bad & ~sent).any():
        fails.append(name_first(~m & bad & ~sent, tag + ' stray store above the block diagonal [system, row, column]', Xs, ref['E']))
    with np.errstate(all='ignore'):
        ratio = np.where(m & ~sent, err / ref['bound'], 0.0).reshape(B, -1).max(1)
        ey = np.abs(yt.astype(LD) - ref['Ey']).astype(np.float64)
    bady = ~(np.isfinite(yt) & (ey <= ref['ybound']))
    if bady.any():
        fails.append(name_first(bady, tag + ' yt outside the bound [system, k]', yt, ref['Ey']))
    return fails, ratio, float(np.max(ey / ref['ybound']))


# ==== inputs ================================================================================================================
def bits_of(N):
    """|A|, |V| <= 2^b with N^2 2^(3b) < 2^52 (b = 12 at N = 196): an element of V A V^T is a sum of N^2 integers of at most
    2^(3b), every partial sum in any order an integer below 2^52; alpha D2 below 2^7 is added exactly."""
    b = 12
    while N * N * 2 ** (3 * b) >= 2 ** 52:
        b -= 1
    return b


def integer_inputs(N, seed=0, T=4, K=3, amp=None):
    """Symmetric integer A (T records) and D2 (K slots, |D2| <= 8), integer V and y, mixed signs."""
    rng = np.random.default_rng(1000 * N + seed)
    a = 2 ** bits_of(N) if amp is None else amp
    A = rng.integers(-a, a + 1, (T, N, N))
    A = np.tril(A) + np.tril(A, -1).transpose(0, 2, 1)
    D2 = rng.integers(-8, 9, (K, N, N))
    D2 = np.tril(D2) + np.tril(D2, -1).transpose(0, 2, 1)
    V = rng.integers(-a, a + 1, (K, N, N))
    y = rng.integers(-a, a + 1, (T, N))
    assert N * N * a ** 3 < 2 ** 52 and N * a * a < 2 ** 52
    return dict(N=N, AWA=A.astype(np.float64), D2=D2.astype(np.float64), V=V.astype(np.float64), y=y.astype(np.float64))


def integer_triples(N, B, T=4, K=3, seed=0):
    """rec and basis non-monotone with repeats, alpha a small integer (0 included): alpha D2 <= 64, added exactly."""
    rng = np.random.default_rng(77 * N + B + seed)
    rec = rng.integers(0, T, B).astype(np.int32)
    bas = rng.integers(0, K, B).astype(np.int32)
    al = rng.choice([0.0, 1.0, 2.0, 3.0, 4.0, 8.0], B)
    if B >= 5:
        rec[:5], bas[:5] = [T - 1, 0, 0, T - 1, 1], [K - 1, K - 1, 0, 1, 0]
    return rec, bas, al


def exact_answers(inp, rec, bas, al):
    """V A V^T + alpha D2 and V y in float64: exact for integer_inputs whatever order NumPy's library sums in."""
    pair = {}
    B, N = len(rec), inp['N']
    E, Ey = np.empty((B, N, N)), np.empty((B, N))
    for i, (r, k, a) in enumerate(zip(rec, bas, al)):
        if (r, k) not in pair:
            pair[r, k] = (inp['V'][k] @ inp['AWA'][r] @ inp['V'][k].T, inp['V'][k] @ inp['y'][r])
        E[i] = pair[r, k][0] + a * inp['D2'][k]
        Ey[i] = pair[r, k][1]
    return E, Ey


def one_hot_case(N, K=5, pairs=None, w=None, d2=None):
    """V[k] signed permutations (row j of V[k] = s e_pi(j)); record t holds A = w (e_p e_q^T + e_q e_p^T) with (p, q) =
    (pi(i), pi(j)) for the t-th pair (i, j) of corner_pairs under the basis it is used with, D2[k] = e_a e_b^T + e_b e_a^T at
    pair 7k + 3 (d2 = (a, b, value): there, in every slot), y one-hot.  System t' (records in a scrambled order, ten of them
    twice) is then the two-element matrix s_i s_j w at (i, j) and (j, i) plus alpha D2, built here by index arithmetic alone."""
    rng = np.random.default_rng(N)
    pairs = np.array(corner_pairs(N) if pairs is None else pairs)
    T = len(pairs)
    pi = np.array([rng.permutation(N) for _ in range(K)])
    sg = rng.choice([-1.0, 1.0], (K, N))
    V = np.zeros((K, N, N))
    for k in range(K):
        V[k, np.arange(N), pi[k]] = sg[k]
    order = np.concatenate([rng.permutation(T), rng.integers(0, T, 10)]).astype(np.int32)
    kof = ((3 * np.arange(T) + 1) % K).astype(np.int32)              # record t is used with basis kof[t]
    w = 1.0 + np.arange(T) % 7 if w is None else np.asarray(w, np.float64)
    ii, jj = pairs[:, 0], pairs[:, 1]
    A = np.zeros((T, N, N))
    np.add.at(A, (np.arange(T), pi[kof, ii], pi[kof, jj]), w)
    np.add.at(A, (np.arange(T), pi[kof, jj], pi[kof, ii]), w)
    D2 = np.zeros((K, N, N))
    for k in range(K):
        a, b, v = tuple(pairs[(7 * k + 3) % T]) + (1.0,) if d2 is None else d2
        D2[k, a, b] += v
        if a != b:
            D2[k, b, a] += v
    ym = (5 * np.arange(T) + 3) % N
    yv = 1.0 + np.arange(T) % 5
    y = np.zeros((T, N))
    y[np.arange(T), ym] = yv
    rec, bas = order, kof[order]
    al = 2.0 ** (np.arange(len(rec)) % 3)
    B = len(rec)
    E = al[:, None, None] * D2[bas]
    val = sg[bas, ii[rec]] * sg[bas, jj[rec]] * w[rec]
    np.add.at(E, (np.arange(B), ii[rec], jj[rec]), val)
    np.add.at(E, (np.arange(B), jj[rec], ii[rec]), val)
    inv = np.argsort(pi, axis=1)                                     # row k of V[b] picks y[pi(k)]: non-zero at k = pi^-1(m)
    Ey = np.zeros((B, N))
    kk = inv[bas, ym[rec]]
    Ey[np.arange(B), kk] = sg[bas, kk] * yv[rec]
    return dict(N=N, AWA=A, D2=D2, V=V, y=y), rec, bas, al, E, Ey


_REAL = {}


def real_case(N, solve=False):
    """Part 3: A_r = G^T diag(w_r) G with Gaussian G (2N x N) and weights of 1e-22 spread over four decades, R symmetric
    positive definite with a spectrum graded over six decades, alpha_k = 10^(KS_k + 22) max|A| / max|R| (so that KS = -22 weighs
    the two terms alike), V_k the eigenvectors of the mean system at alpha_k (row k = vector k), D2_k = V_k R V_k^T rounded from
    80-bit arithmetic; 4 records x 6 bases.  solve (part 4): the spectra of A_r and R in [0.1, 1] x 1e-20 and [0.1, 1], so that
    every A_r + alpha R has a condition number of at most 10.  The seed is the first for which no system's maximum lies within
    the bound of a power of two (asserted: the scl gate then accepts one value per system)."""
    if (N, solve) in _REAL:
        return _REAL[N, solve]
    for seed in range(5):
        rng = np.random.default_rng(10000 * seed + 10 * N + solve)
        Q = np.linalg.qr(rng.standard_normal((N, N)))[0]
        if solve:
            A = np.empty((4, N, N))
            for r in range(4):
                Qr = np.linalg.qr(rng.standard_normal((N, N)))[0]
                A[r] = (Qr * (1e-20 * rng.uniform(0.1, 1.0, N))) @ Qr.T
            R = (Q * rng.uniform(0.1, 1.0, N)) @ Q.T
        else:
            G = rng.standard_normal((2 * N, N))
            w = 1e-22 * 10.0 ** rng.uniform(-2.0, 2.0, (4, 2 * N))
            A = np.array([(G.T * w[r]) @ G for r in range(4)])
            R = (Q * 10.0 ** np.linspace(0.0, -6.0, N)) @ Q.T
        A, R = (A + A.transpose(0, 2, 1)) / 2, (R + R.T) / 2
        y = rng.standard_normal((4, N)) * 1e-9
        alk = 10.0 ** (KS + 22.0) * np.abs(A).max() / np.abs(R).max()
        V = np.array([np.ascontiguousarray(np.linalg.eigh(A.mean(0) + a * R)[1].T) for a in alk])
        D2 = np.array([(v.astype(LD) @ R.astype(LD) @ v.astype(LD).T).astype(np.float64) for v in V])
        D2 = (D2 + D2.transpose(0, 2, 1)) / 2
        rec, bas = np.repeat(np.arange(4, dtype=np.int32), 6), np.tile(np.arange(6, dtype=np.int32), 4)
        al = alk[bas]
        ref = real_reference(A, V, D2, y, rec, bas, al)
        ch = scl_choices(ref)
        if np.all(ch == ch[0]):
            break
    assert np.all(ch == ch[0]), 'a maximum within the bound of a power of two'
    c = dict(inp=dict(N=N, AWA=A, D2=D2, V=V, y=y), R=R, alk=alk, rec=rec, bas=bas, al=al, ref=ref, seed=seed)
    _REAL[N, solve] = c
    return c


# ==== part 1, continued: the gates reject emulated wrong answers (no GPU) =====================================================
def emulate(inp, rec, bas, al, fault=None):
    """What a forming kernel with the given fault would return in float64: X with sentinels above the block diagonal, scl, yt."""
    N, B = inp['N'], len(rec)
    X, scl, yt = np.full((B, N, N), SENTINEL), np.empty(B), np.empty((B, N))
    m = lbt(N)
    for i, (r, k, a) in enumerate(zip(rec, bas, al)):
        V, A = inp['V'][k], inp['AWA'][r]
        V1 = V.copy()
        if fault == 'kstep':
            V1[:, 4 * ((N - 1) // 4):] = 0.0                         # the last k-step of W = V A
        v = (V1 @ A) @ V.T + a * inp['D2'][(k + 1) % len(inp['D2']) if fault == 'slot' else k]
        if fault == 'tile':
            v[16:32, 0:16] = v[16:32, 0:16].T.copy()
        s = float(expected_scl(np.abs(np.where(m, v, 0.0)).max()))
        with np.errstate(all='ignore'):
            X[i][m] = (v / s * (2.0 if fault in ('f', 'fx') else 1.0))[m]
        if fault == 'stray':
            X[i, 0, N - 1] = 1.0
        if fault == 'unwritten':
            X[i, N - 1, 0] = SENTINEL
        scl[i] = s / 2.0 if fault == 'f' else s
        yt[i] = (V.T if fault == 'vt' else V) @ inp['y'][r]
    return X, scl, yt


FAULTS = ('kstep', 'tile', 'slot', 'f', 'fx', 'vt', 'stray', 'unwritten')


def test_gates_reject_emulated_wrong_answers():
    """On the host at N = 33 (three blocks, padded): NumPy's own results pass the exact gate of part 2 and the derived bound of
    part 3, and each gate names the fault of: the last k-step of the first product dropped, one 16 x 16 tile of X transposed,
    D2 of the neighbouring slot, f off by a factor 2 (in X and scl, and in X alone), yt with V transposed, a store above the
    block diagonal, an element of the lower block triangle left as it was."""
    N = 33
    inp = integer_inputs(N)
    rec, bas, al = integer_triples(N, 5)
    al[al == 0] = 1.0
    E, Ey = exact_answers(inp, rec, bas, al)
    assert not check_exact('ok', *emulate(inp, rec, bas, al), E, Ey)
    where = {'kstep': ' scl X', 'tile': ' scl X', 'slot': ' scl X', 'f': ' scl [system]', 'fx': ' scl X', 'vt': ' yt',
             'stray': 'stray store', 'unwritten': 'not written'}
    for f in FAULTS:
        fails = check_exact(f, *emulate(inp, rec, bas, al, f), E, Ey)
        assert fails and any(where[f] in x for x in fails), (f, fails)
        if f == 'tile':                                              # the failure names the first element of the tile that moved
            assert 'first (0, 16, 1)' in fails[0], fails
    oh, rec1, bas1, al1, E1, Ey1 = one_hot_case(N)
    assert not check_exact('one-hot', *emulate(oh, rec1, bas1, al1), E1, Ey1)          # the index arithmetic is NumPy's product
    assert check_exact('one-hot', *emulate(oh, rec1, bas1, al1, 'vt'), E1, Ey1)
    # ---- the derived bound
    c = real_case(N)
    assert c['ref']['bound'].max() < 1e-12 * c['ref']['aE'].max()                      # the gate is not vacuous
    X, scl, yt = emulate(c['inp'], c['rec'], c['bas'], c['al'])
    fails, ratio, ry = check_real('ok', X, scl, yt, c['ref'])
    assert not fails and 0 < ratio.max() < 1 and 0 < ry < 1, (fails, ratio, ry)
    for f in FAULTS:
        fails = check_real(f, *emulate(c['inp'], c['rec'], c['bas'], c['al'], f), c['ref'])[0]
        assert fails and any(where[f] in x for x in fails), (f, fails)


# ==== device calls ==========================================================================================================
def _fg():
    import test_gpu_fit_geometry as fg
    return fg


class Device:
    """The five input arrays of a case on the device, uploaded once and used by every batch of the case."""

    def __init__(self, inp):
        fg = _fg()
        self.N = inp['N']
        self.a = [fg.dev(inp[k]) for k in ('AWA', 'V', 'D2', 'y')]

    def form(self, rec, bas, al, want=0):
        """vi_walk_form_f64 of the triples: X, scl, yt - each between guards, X starting as sentinels.  want: the status."""
        fg = _fg()
        lib, ctx = fg._L(), fg._ctx()
        B, N = len(rec), self.N
        oX, oS, oY = fg.Out((max(B, 1), N, N)), fg.Out((max(B, 1),)), fg.Out((max(B, 1), N))
        ins = [fg.dev(rec, np.int32), fg.dev(bas, np.int32), fg.dev(al)] if B else [fg.dev(np.zeros(1, np.int32))] * 2 + [fg.dev(np.zeros(1))]
        AWA, V, D2, y = self.a
        rc = lib.lib.vi_walk_form_f64(ctx.handle, B, N, AWA.ptr, ins[0].ptr, V.ptr, D2.ptr, ins[1].ptr, y.ptr, ins[2].ptr,
                                      oX.ptr, oS.ptr, oY.ptr)
        ctx.sync()
        assert rc == want, (rc, want, lib.lib.vi_last_error())
        return oX.get()[:max(B, 1)], oS.get(), oY.get()


def untouched(*arrays):
    return all(np.all(a.view(np.uint64) == SB) for a in arrays)


def basis_solve(inp, rec, bas, al):
    fg = _fg()
    lib, ctx = fg._L(), fg._ctx()
    B, N = len(rec), inp['N']
    oC, drk, dsw = fg.Out((B, N)), ctx.empty((B,), np.int32), ctx.empty((B,), np.int32)
    a = [fg.dev(inp[k]) for k in ('AWA', 'y')] + [fg.dev(rec, np.int32), fg.dev(bas, np.int32), fg.dev(al), fg.dev(inp['V']),
                                                  fg.dev(inp['D2'])]
    lib.check(lib.lib.vi_basis_solve_f64(ctx.handle, B, N, *[x.ptr for x in a], EPS, oC.ptr, drk.ptr, dsw.ptr), 'basis_solve')
    return oC.get(), drk.download(), dsw.download()


# ==== 2. exact by construction ===============================================================================================
def exact_suite(N, tag=''):
    """Integer inputs at B = 1, 5, 300 (3000 for N <= 32) and the one-hot index maps; returns the failures."""
    g = walk_geometry(N)
    print('walk N %d (%s)%s' % (N, g['cls'], tag))
    inp = integer_inputs(N)
    d = Device(inp)
    fails = []
    for B in b_list(N):
        rec, bas, al = integer_triples(N, B)
        E, Ey = exact_answers(inp, rec, bas, al)
        fails += check_exact('N %d B %d%s' % (N, B, tag), *d.form(rec, bas, al), E, Ey)
    oh, rec, bas, al, E, Ey = one_hot_case(N)
    fails += check_exact('N %d one-hot%s' % (N, tag), *Device(oh).form(rec, bas, al), E, Ey)
    return fails


def ieee_suite(N, tag=''):
    """The zero system (f = scl = 1, X = 0) in a batch with others; alpha = 0; systems whose maximum is 1.75e308 (f = 1) and
    1.6e308 (f = 2^-1023); B = 0."""
    inp = integer_inputs(N, seed=1)
    inp['AWA'][2] = 0.0
    rec = np.array([2, 0, 2, 1, 3, 2], np.int32)
    bas = np.array([1, 0, 2, 2, 1, 0], np.int32)
    al = np.array([0.0, 0.0, 0.0, 4.0, 0.0, 1.0])
    E, Ey = exact_answers(inp, rec, bas, al)
    assert not E[0].any() and not E[2].any() and E[5].any()
    d = Device(inp)
    X, scl, yt = d.form(rec, bas, al)
    fails = check_exact('N %d zero system and alpha = 0%s' % (N, tag), X, scl, yt, E, Ey)
    m = lbt(N)
    if not (scl[0] == 1.0 and scl[2] == 1.0 and not X[0][m].any() and not X[2][m].any()):
        fails.append('N %d%s: the zero system is not X = 0, scl = 1' % (N, tag))
    out = d.form(rec[:0], bas[:0], al[:0])
    if not untouched(*out):
        fails.append('N %d%s: B = 0 wrote something' % (N, tag))
    # ---- huge: one-hot systems (every product is x 1 or x 0), off-diagonal elements of 1.75e308 and 1.6e308; D2 = 2^1000 at (5, 5)
    hp = [(N - 1, 0), (N // 2, 1), (3, 2), (N - 2, N - 3)]
    oh, rec, bas, al, E, Ey = one_hot_case(N, pairs=hp, w=[1.75e308, 1.6e308, 1.75e308, 1.6e308], d2=(5, 5, 2.0 ** 1000))
    assert np.isfinite(oh['AWA']).all() and np.isfinite(E).all() and all(i != j and (5, 5) != (i, j) for i, j in hp)
    X, scl, yt = Device(oh).form(rec, bas, al)
    fails += check_exact('N %d huge%s' % (N, tag), X, scl, yt, E, Ey)
    want = np.where(rec % 2 == 0, 1.0, 2.0 ** 1023)
    if not np.array_equal(scl, want):
        fails.append('N %d huge%s: scl %r, want %r' % (N, tag, scl, want))
    return fails


def tiny_suite(N, tag=''):
    """Integer inputs in -1 .. 1, A and D2 times 2^-1040: every sum is an integer below 2^17 times 2^-1040, a multiple of
    2^-1074 (nothing smaller is formed), so max|X| < 2^-1023 and 2^(1 - ex) would be 2^1024 and more.  f is capped at 2^1023:
    scl = 2^-1023, scl X exact."""
    inp = integer_inputs(N, seed=2, amp=1)
    assert N * N + 8 < 2 ** 17
    inp['D2'] = np.clip(inp['D2'], -1, 1)
    rec, bas, al = integer_triples(N, 5, seed=2)
    al = np.minimum(al, 1.0)
    E, Ey = exact_answers(inp, rec, bas, al)
    t = 2.0 ** -1040
    inp['AWA'], inp['D2'] = inp['AWA'] * t, inp['D2'] * t
    assert np.abs(E).max() * t < 2.0 ** -1023 and np.all(E * t / t == E)
    X, scl, yt = Device(inp).form(rec, bas, al)
    fails = check_exact('N %d tiny%s' % (N, tag), X, scl, yt, E * t, Ey)
    if not np.all(scl[np.abs(E).reshape(5, -1).max(1) > 0] == 2.0 ** -1023):
        fails.append('N %d tiny%s: scl %r, want 2^-1023' % (N, tag, scl))
    return fails


def nonfinite_suite(N, what, tag=''):
    """A batch of 9 triples of 4 records, and the same batch with triples of a fifth record - record 1 with one NaN (or Inf) -
    put in between.  Returns (failures of what must hold in any case, the counts of NaN / Inf / finite elements in the lower
    block triangle of the systems of the fifth record).  At a padded order a second batch has the NaN in row and column
    N - 1, the address that the padded loads clamp to."""
    fails, counts = [], []
    m = lbt(N)
    places = [(N // 3, N // 2)] + ([(N - 1, N - 1)] if N % 16 else [])
    for p, q in places:
        inp = integer_inputs(N, seed=3, T=5)
        inp['AWA'][4] = inp['AWA'][1]
        inp['y'][4] = inp['y'][1]
        rec, bas, al = integer_triples(N, 9, seed=3)
        al = np.maximum(al, 1.0)
        X0, s0, y0 = Device(inp).form(rec, bas, al)
        fails += check_exact('N %d %s base%s' % (N, what, tag), X0, s0, y0, *exact_answers(inp, rec, bas, al))
        inp['AWA'][4, p, q] = np.nan if what == 'nan' else np.inf
        at = [0, 4, 11]                                              # where the bad triples go: first, inside, last
        rec2, bas2, al2 = np.insert(rec, [0, 3, 9], 4), np.insert(bas, [0, 3, 9], [0, 2, 1]), np.insert(al, [0, 3, 9], [1.0, 2.0, 1.0])
        assert list(np.flatnonzero(rec2 == 4)) == at and len(rec2) == 12
        X, s, y = Device(inp).form(rec2, bas2, al2)
        good = np.flatnonzero(rec2 != 4)
        for name, a, b in (('X', X[good], X0), ('scl', s[good], s0), ('yt', y[good], y0)):
            if not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
                fails.append('N %d %s at (%d, %d)%s: %s of the other systems moved' % (N, what, p, q, tag, name))
        bad = X[at][:, m]
        if np.any(bad.view(np.uint64) == SB):
            fails.append('N %d %s at (%d, %d)%s: elements not written' % (N, what, p, q, tag))
        if np.isfinite(bad).any():
            fails.append('N %d %s at (%d, %d)%s: %d finite elements in a system of the bad record' % (N, what, p, q, tag, np.isfinite(bad).sum()))
        if not np.array_equal(y[at], np.einsum('bkn,n->bk', inp['V'][bas2[at]], inp['y'][4])) or not np.all(s[at] == 1.0):
            fails.append('N %d %s at (%d, %d)%s: yt or scl of the bad record, scl %r' % (N, what, p, q, tag, s[at]))
        counts.append(((p, q), int(np.isnan(bad).sum()), int(np.isinf(bad).sum()), int(np.isfinite(bad).sum()), s[at].tolist()))
    return fails, counts


def refusal_suite(tag=''):
    """N = 7 and N = 197: VI_ERR_UNSUPPORTED from the host, every sentinel in place."""
    fails = []
    for N in (7, 197):
        inp = dict(N=N, AWA=np.ones((1, N, N)), V=np.ones((1, N, N)), D2=np.ones((1, N, N)), y=np.ones((1, N)))
        out = Device(inp).form(np.zeros(2, np.int32), np.zeros(2, np.int32), np.ones(2), want=VI_ERR_UNSUPPORTED)
        if not untouched(*out):
            fails.append('N %d%s: a refused call wrote something' % (N, tag))
    return fails


@gpu
@pytest.mark.parametrize('N', NS)
def test_integer_inputs_exact_at_every_shape(N):
    """scl X, scl and yt have NumPy's bits at B = 1, 5, 300 (N <= 32: 3000) and for the one-hot index maps; nothing but the
    right value is stored above the block diagonal, nothing outside the outputs."""
    fails = exact_suite(N)
    assert not fails, '\n'.join(fails)


@gpu
@pytest.mark.parametrize('N', NS)
def test_zero_huge_and_empty_systems(N):
    fails = ieee_suite(N)
    assert not fails, '\n'.join(fails)


@gpu
@pytest.mark.parametrize('N', NS)
def test_tiny_systems(N):
    """max|X| < 2^-1023: before the cap on f (see Findings) this gave X = Inf / NaN and scl = 0 at every order, either way of
    forming."""
    fails = tiny_suite(N)
    assert not fails, '\n'.join(fails)


@gpu
@pytest.mark.parametrize('N', NS)
def test_a_record_with_a_nan(N):
    """The systems of a record with one NaN in A are NaN all over the lower block triangle, and every other system of the batch
    has the bits it has without that record - also where the NaN sits at (N - 1, N - 1) of a padded order."""
    fails, counts = nonfinite_suite(N, 'nan')
    for pq, nnan, ninf, nfin, _ in counts:
        if ninf or nfin:
            fails.append('N %d NaN at %r: %d NaN, %d Inf, %d finite' % (N, pq, nnan, ninf, nfin))
    assert not fails, '\n'.join(fails)


def all_nan(counts):
    return all(ninf == 0 and nfin == 0 for _, _, ninf, nfin, _ in counts)


@gpu
@pytest.mark.parametrize('N', NS)
def test_a_record_with_an_inf(N):
    """As test_a_record_with_a_nan with one Inf, at a place inside the matrix and, at a padded order, at (N - 1, N - 1): the
    systems of that record are NaN all over the lower block triangle (none unwritten), their scl is 1, their yt is right, and
    no other system of the batch moves.  Before the scaling pass poisoned a system with an infinite maximum (Findings at the
    head of the file) this failed with all +-Inf at every order but for the padded corner under K_walk."""
    fails, counts = nonfinite_suite(N, 'inf')
    assert not fails, '\n'.join(fails)
    print('N %d Inf record [(place), NaN, Inf, finite, scl]: %r' % (N, counts))
    assert all_nan(counts), counts


@gpu
def test_orders_out_of_range_are_refused():
    fails = refusal_suite()
    assert not fails, '\n'.join(fails)


# ==== 3. real magnitudes ====================================================================================================
def real_suite(N, tag=''):
    c = real_case(N)
    X, scl, yt = Device(c['inp']).form(c['rec'], c['bas'], c['al'])
    fails, ratio, ry = check_real('N %d real%s' % (N, tag), X, scl, yt, c['ref'])
    print('walk real N %3d%s: worst error / bound %.3f (X), %.3f (X at the smallest alpha: the products alone), %.3f (yt); seed %d'
          % (N, tag, ratio.max(), ratio[c['bas'] == 5].max(), ry, c['seed']))
    return fails


@gpu
@pytest.mark.parametrize('N', NS)
def test_real_magnitudes_within_the_derived_bound(N, capsys):
    """Pointwise over the lower block triangle: |scl X - E| <= gamma(2N + 2) |V||A||V|^T + 3u |E|, yt within gamma(N + 6) |V||y|,
    scl the power of two of the reference maximum (module docstring; the measured worst ratios are in DESIGN.md)."""
    with capsys.disabled():
        fails = real_suite(N)
    assert not fails, '\n'.join(fails)


def n144_suite(tag=''):
    """The real set-up of test_gpu_walk_rotate at N = 144: the device's own V and D2 (vi_warm_prepare_f64) of six decades."""
    import test_gpu_walk_rotate as wr
    s = wr._setup('n144')
    d = wr._bases(s)
    inp = dict(N=144, AWA=d['dAWA'].download(), V=d['dV'].download(), D2=d['dD2'].download(), y=d['dy'].download())
    rec, bas, al = wr._triples24()
    ref = real_reference(inp['AWA'], inp['V'], inp['D2'], inp['y'], rec, bas, al)
    ch = scl_choices(ref)
    assert np.all(ch == ch[0]), 'a maximum within the bound of a power of two'
    X, scl, yt = Device(inp).form(rec, bas, al)
    fails, ratio, ry = check_real('n144 set-up%s' % tag, X, scl, yt, ref)
    print('walk real n144 set-up%s: worst error / bound %.3f (X), %.3f (X at the smallest alpha), %.3f (yt)'
          % (tag, ratio.max(), ratio[bas == 5].max(), ry))
    return fails


@gpu
def test_the_n144_setup_within_the_derived_bound(capsys):
    with capsys.disabled():
        fails = n144_suite()
    assert not fails, '\n'.join(fails)


@gpu
@pytest.mark.parametrize('kind', list(KINDS))
def test_a_system_does_not_depend_on_the_batch(kind):
    """One (record, basis, alpha) triple alone, first, in the middle and last of a batch of 300, at place 4 of a batch of 7
    other triples, and with the call repeated: X (all of it, what lies above the block diagonal included), scl and yt bit
    for bit.  K_walk only - the claim at the head of vi_walk.hip; the library chain is free to choose its kernels by batch."""
    assert os.environ.get('VINTERP_WALK_FORM') != 'blas'
    N = KINDS[kind]
    assert walk_geometry(N)['kind'] == kind
    c = real_case(N)
    d = Device(c['inp'])
    probe = (2, 3, c['alk'][3] * 10.0 ** 0.2)
    X1, s1, y1 = d.form(np.array([probe[0]], np.int32), np.array([probe[1]], np.int32), np.array([probe[2]]))
    assert np.all(np.isfinite(X1[0][lbt(N)])) and np.isfinite(y1).all()
    rng = np.random.default_rng(N)

    def batch(B, at):
        rec, bas = rng.integers(0, 4, B).astype(np.int32), rng.integers(0, 6, B).astype(np.int32)
        al = c['alk'][bas] * 10.0 ** rng.uniform(-0.5, 0.5, B)
        for i in at:
            rec[i], bas[i], al[i] = probe
        return rec, bas, al
    b300 = batch(300, (0, 150, 299))
    for rep in range(2):
        X, s, y = d.form(*b300)
        for i in (0, 150, 299):
            assert np.array_equal(X[i].view(np.uint64), X1[0].view(np.uint64)) and s[i] == s1[0] and np.array_equal(y[i], y1[0]), (rep, i)
    X, s, y = d.form(*batch(7, (4,)))
    assert np.array_equal(X[4].view(np.uint64), X1[0].view(np.uint64)) and s[4] == s1[0] and np.array_equal(y[4], y1[0])


# ==== 4. through vi_basis_solve_f64 ==========================================================================================
def solve_suite():
    """C, rank, sweeps of the 24 triples of real_case(N, solve=True) at every N of SOLVE_NS."""
    out = {}
    for N in SOLVE_NS:
        c = real_case(N, solve=True)
        C, rk, sw = basis_solve(c['inp'], c['rec'], c['bas'], c['al'])
        out['C%d' % N], out['rank%d' % N], out['sweeps%d' % N] = C, rk, sw
    return out


def solve_reference(N):
    c = real_case(N, solve=True)
    A, R, y = c['inp']['AWA'], c['R'], c['inp']['y']
    return np.array([np.linalg.solve(A[r] + a * R, y[r]) for r, a in zip(c['rec'], c['al'])])


@gpu
def test_basis_solve_at_every_kind(tmp_path, capsys):
    """vi_basis_solve_f64 at N = 16, 64, 128, 135, 147, 160, 176, 192, 196 on systems of condition number <= 10.  With
    VINTERP_WALK_TOL=0 (a child process; the criterion of all other solves) C is within rel 1e-10 of numpy.linalg.solve - the F1
    gate of test_gpu_solver_geometry.py -, the rank is N and the sweeps stay under the cap; at the walk's own tolerance C is
    finite and the rank right (its accuracy is what test_gpu_walk_rotate.py gates through chi^2)."""
    from conftest import rel
    lib = _fg()._L()
    cap = int(lib.lib.vi_max_sweeps())
    here = solve_suite()
    tight = _child('solve', tmp_path, VINTERP_WALK_TOL='0')[0]
    fails = []
    for N in SOLVE_NS:
        ref = solve_reference(N)
        worst = max(rel(tight['C%d' % N][i], ref[i]) for i in range(len(ref)))
        with capsys.disabled():
            print('walk solve N %3d (%s): worst rel(C) %.2e, sweeps %s' % (N, walk_geometry(N)['kind'], worst,
                                                                          np.bincount(tight['sweeps%d' % N]).tolist()))
        if not worst <= 1e-10:
            fails.append('N %d: rel(C) %.3e' % (N, worst))
        if not np.all(tight['rank%d' % N] == N) or not np.all(here['rank%d' % N] == N):
            fails.append('N %d: rank' % N)
        if not np.max(tight['sweeps%d' % N]) < cap or not np.max(here['sweeps%d' % N]) < cap:
            fails.append('N %d: sweeps at the cap' % N)
        if not np.isfinite(here['C%d' % N]).all():
            fails.append('N %d: C at the default tolerance' % N)
    assert not fails, '\n'.join(fails)


# ==== the child processes ===================================================================================================
def _child(what, tmp_path, must_pass=True, **env):
    e = dict(os.environ)
    for k in ('VINTERP_WALK_FORM', 'VINTERP_WALK_TOL', 'VINTERP_WALK_CHUNK'):
        e.pop(k, None)
    e.update(env)
    out = str(tmp_path / (what + '.npz'))
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), what, out]
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=900)
    print(r.stdout[-6000:])
    if must_pass:
        assert r.returncode == 0, '%s child %r: exit %d\n%s\n%s' % (what, env, r.returncode, r.stdout[-6000:], r.stderr[-3000:])
    return (np.load(out, allow_pickle=False) if os.path.exists(out) else None), r


def blas_suite():
    """Parts 2 and 3 for the child (but for the batch independence, which is K_walk's claim): the failures, and the counts of
    the Inf records as rows (N, row, column, NaN, Inf, finite), which the parent judges in a test of their own."""
    tag = ' [blas]'
    fails = refusal_suite(tag) + n144_suite(tag)
    rows = []
    for N in NS:
        fails += exact_suite(N, tag) + ieee_suite(N, tag) + tiny_suite(N, tag) + real_suite(N, tag)
        f, counts = nonfinite_suite(N, 'nan', tag)
        fails += f + ['N %d NaN at %r%s: %d NaN, %d Inf, %d finite' % (N, pq, tag, a, b, c) for pq, a, b, c, _ in counts if b or c]
        f, counts = nonfinite_suite(N, 'inf', tag)
        fails += f
        rows += [(N, pq[0], pq[1], a, b, c) for pq, a, b, c, _ in counts]
    return fails, np.array(rows, np.int64)


_BLAS = []


def _blas_child(tmp_path_factory):
    """One child process with VINTERP_WALK_FORM=blas for the two tests below."""
    if not _BLAS:
        _BLAS.append(_child('blas', tmp_path_factory.mktemp('walk_blas'), must_pass=False, VINTERP_WALK_FORM='blas'))
    return _BLAS[0]


@gpu
def test_exact_and_real_suites_on_the_library_chain(tmp_path_factory, capsys):
    """Everything of parts 2 and 3 once more with VINTERP_WALK_FORM=blas, in one child process: the chain that K_walk replaced
    and that remains the fallback forms the same exact bits and stays within the same bound (its worst ratios are printed)."""
    _, r = _blas_child(tmp_path_factory)
    with capsys.disabled():
        print('\n'.join(x for x in r.stdout.splitlines() if x.startswith('walk real')))
    assert r.returncode == 0, 'blas child: exit %d\n%s\n%s' % (r.returncode, r.stdout[-6000:], r.stderr[-3000:])


@gpu
def test_a_record_with_an_inf_on_the_library_chain(tmp_path_factory):
    """The all-NaN requirement of test_a_record_with_an_inf for the library chain (the same child process as above)."""
    out, r = _blas_child(tmp_path_factory)
    assert out is not None, r.stderr[-3000:]
    rows = out['inf_counts']
    assert len(rows) >= len(NS)
    bad = rows[(rows[:, 4] != 0) | (rows[:, 5] != 0)]
    assert not len(bad), 'rows (N, row, column, NaN, Inf, finite): %r' % bad[:6].tolist()


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    what, out = sys.argv[1], sys.argv[2]
    if what == 'blas':
        assert os.environ.get('VINTERP_WALK_FORM') == 'blas'
        fails, rows = blas_suite()
        np.savez(out, inf_counts=rows)
        for f in fails:
            print('FAIL ' + f)
        sys.exit(1 if fails else 0)
    elif what == 'solve':
        np.savez(out, **solve_suite())
    else:
        raise SystemExit('unknown job %r' % what)
