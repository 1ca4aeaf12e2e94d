"""Reference and checks for K3p, the pivoted Householder pre-conditioner of the cold solves (csrc/vi_qr.hip).  No GPU.

Restatements.  qr_rt, hh_off, hh_doubles, the thread counts of the three launches and the EPL rule of k_qr_back_vec are
restated from the sizes alone; geometry(N) names the class an order falls in.

The reference does not run a QR of its own.  It takes the reflectors a kernel (or the emulation below) produced - v_k and
tau_k unpacked from the packed store - and applies H_k = I - tau_k v_k v_k^T in np.longdouble (64-bit mantissa).  The states
S_k = H_{k-1} ... H_0 X give the remaining norms at every step (the pivot rule), S_K = R P^T, and Q^T / Q applied to any
vector.  Every comparison is then a forward bound of applying KNOWN reflectors to a KNOWN input.

Bounds (u = 2^-53, gamma(n) = n u / (1 - n u), n = NR = 8 RT, the rows an octet holds; Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., Lemmas 19.2 - 19.3, with the kernels' own operation counts):

  reflector   The owner forms s2 = fl(sum x_i^2) = |x|^2 (1 + th), |th| <= gamma(n) (n fma / additions in any order, all terms
              of one sign); r = qr_rsqrt(s2) (relative error e_r), s = fl(s2 r) = |x| (1 + eta), |eta| <= gamma(n) / 2 + e_r + u;
              v_k = x_k + sign(x_k) s (one rounding, no cancellation); tau = fl(r qr_rcp(fl(s + |x_k|))) = (1 + e_t) /
              (s (s + |x_k|)), |e_t| <= 2 e_r + e_c + 3 u.  With v^T v = 2 s (s + |x_k|) - 2 eta s^2 + 2 u (s + |x_k|)^2:
                  |tau v^T v - 2| <= 2 |e_t| + 2 |eta| + 4 u <= gamma(n) + 6 e_r + 2 e_c + 12 u.
              qr_rsqrt is the hardware estimate (2^-23 or better) and one third-order step: the remainder is 2^-66, the
              roundings of the step are x y (u, carried into e), the inner fma pair (below u) and the last fma (u):
              e_r <= 4 u.  qr_rcp is two Newton steps, remainder 2^-90, two roundings in the last step: e_c <= 3 u.
                  REFL = gamma(n) + 42 u.
  one step    a' = a - tau (v^T a) v as d = fl(v^T a) (|d - v^T a| <= gamma(n) |v| |a|), w = fl(tau d), a'_i = fma(-w, v_i, a_i):
                  |fl(a') - a'| <= (1 + u) tau |v|^2 (gamma(n) (1 + u) + u) |a| + u |a'| <= (1 + REFL) (2 gamma(n) + 3 u) |a|
              so STEP = gamma(2 n + 4) times the growth (1 + REFL) that a reflector which is orthogonal only to REFL allows.
  K steps     b(K) = K STEP (1 + REFL)^K (1 + STEP)^K (1 + 2^-10): the inputs of the later steps are the computed ones, and the
              last factor covers the reference's own rounding (K n 2^-64 against K n 2^-53).
  triangle    In the reference the column a reflector was made from keeps, below the diagonal, x_i (1 - tau v^T x) with
              |1 - tau v^T x| <= |e_t| + 2 |eta| + u <= REFL; the later reflectors do not enlarge it beyond the growth, and
              the device is within b(K) of the reference: TRI = b(K) + REFL (1 + REFL)^K, times the norm of the input column.
  pivot       The kernel compares fl(|a_j|^2) of its own columns a_j, which are within b(k) |X_j| of S_k: choosing p over j
              means |a_p| (1 + gamma(n) / 2) >= |a_j| (1 - gamma(n) / 2), i.e. with the reference's norms n_j
                  n_p >= n_j - PIV(k) (|X_p| + |X_j|),   PIV(k) = b(k) + gamma(n + 2).
              A step is "discriminating" when this inequality would reject the runner-up, had it been chosen.

The float64 emulation follows the kernel's conventions (pivot by recomputed norms, ties to the lower index, alpha =
-copysign(|x|, x_k), tau = 1 / (|x| (|x| + |x_k|)), stop when the largest remaining squared norm is zero or below the normal
range) with NumPy's own summation orders; tests/test_qr_ref_host.py runs it and a list of wrong variants of it through
every check."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TINY = float(np.finfo(np.float64).tiny)

NS = [8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 143, 144]
RTS = (4, 6, 8, 12, 18)
BACK_VEC_THREADS = 256
LDS_LIMIT = 159 * 1024


# ==== restatements of csrc/vi_qr.hip ========================================================================================
def qr_rt(N):
    """Local rows per lane: the smallest instantiation that holds N rows; 0 where there is none."""
    need = (N + 7) // 8
    for o in RTS:
        if need <= o:
            return o
    return 0


def hh_off(k, NR):
    """Start of v_k in the packed store: stored from row 8 (k >> 3) to row NR - 1."""
    B = k >> 3
    return 8 * NR * B - 32 * B * (B - 1) + (k & 7) * (NR - 8 * B)


def hh_doubles(N):
    """Packed size of one system's reflector set (N vectors, then the N taus); 0 where K3p does not run."""
    if not supported(N):
        return 0
    return hh_off(N, 8 * qr_rt(N)) + N


def lds_bytes(N):
    NR = 8 * qr_rt(N)
    return 2 * NR * 8 + (hh_off(N, NR) + N + 16) * 8 + 16 * 4


def supported(N):
    return N >= 8 and qr_rt(N) > 0 and lds_bytes(N) <= LDS_LIMIT


def up16_doubles(N):
    """The stride the solves pass: the packed bytes rounded up to 16, in doubles."""
    return ((8 * hh_doubles(N) + 15) & ~15) // 8


def sim_threads(N):
    return (8 * ((N + 2) // 2) + 63) // 64 * 64          # an octet per pair of columns, y is column N


def back_mat_threads(N):
    return (8 * ((N + 1) // 2) + 63) // 64 * 64


def epl(N):
    return 1 if N <= 64 else 2 if N <= 128 else 3


def geometry(N):
    rt = qr_rt(N)
    th = sim_threads(N)
    return dict(rt=rt, NR=8 * rt, epl=epl(N), sim=th, back_mat=back_mat_threads(N), waves=th // 64, odd=N % 2 == 1,
                y_slot='c1 of a matrix octet' if N % 2 else 'c0 of its own octet', full_rows=N == 8 * rt,
                full_block=th == (320 if rt <= 8 else 640), hh=hh_doubles(N), stride16=up16_doubles(N),
                cls='RT %2d EPL %d %s' % (rt, epl(N), 'odd ' if N % 2 else 'even'))


def case_table():
    lines = []
    for N in NS:
        g = geometry(N)
        lines.append('N %3d  RT %2d (NR %3d%s)  EPL %d  k_qr_sim %3d thr%s  k_qr_back_mat %3d thr  y is %-20s  hh %5d doubles, '
                     'up16 stride %5d' % (N, g['rt'], g['NR'], ', no padding' if g['full_rows'] else '', g['epl'], g['sim'],
                                          ' = launch bound' if g['full_block'] else '', g['back_mat'], g['y_slot'], g['hh'],
                                          g['stride16']))
    return lines


# ==== bounds ================================================================================================================
def gamma(n):
    return n * U / (1.0 - n * U)


def refl_bound(NR):
    return gamma(NR) + 42.0 * U


def step_bound(NR):
    return gamma(2 * NR + 4)


def b_apply(K, NR):
    return K * step_bound(NR) * (1.0 + refl_bound(NR)) ** K * (1.0 + step_bound(NR)) ** K * (1.0 + 2.0 ** -10)


def tri_bound(K, NR):
    return b_apply(K, NR) + refl_bound(NR) * (1.0 + refl_bound(NR)) ** K


def pivot_bound(k, NR):
    return b_apply(k, NR) + gamma(NR + 2)


# ==== the packed store ======================================================================================================
def unpack(hh, N):
    """(V, tau, stored): V[k] = v_k over rows 0 .. NR - 1 (zero where nothing is stored), tau[k], and stored[k] = the first
    stored row of v_k, from one system's packed set."""
    NR = 8 * qr_rt(N)
    hh = np.asarray(hh)
    V = np.zeros((N, NR))
    stored = np.zeros(N, dtype=np.int64)
    for k in range(N):
        r0 = 8 * (k >> 3)
        V[k, r0:] = hh[hh_off(k, NR):hh_off(k, NR) + NR - r0]
        stored[k] = r0
    tau = np.array(hh[hh_off(N, NR):hh_off(N, NR) + N])
    return V, tau, stored


def pack(V, tau, N):
    NR = 8 * qr_rt(N)
    hh = np.zeros(hh_doubles(N))
    for k in range(N):
        r0 = 8 * (k >> 3)
        hh[hh_off(k, NR):hh_off(k, NR) + NR - r0] = V[k, r0:]
    hh[hh_off(N, NR):] = tau
    return hh


def split_sets(buf, B, N, stride=0):
    """The B packed sets of a buffer in which they lie `stride` doubles apart (0: packed)."""
    P = hh_doubles(N)
    stride = stride or P
    return [np.array(buf[i * stride:i * stride + P]) for i in range(B)]


def layout_problems(hh, N):
    """What of the packed layout does not hold, as a list of strings: exact zeros above row k and from row N on, the taken
    steps a prefix, untaken steps all zero (the last vector and tau always), everything finite."""
    V, tau, _ = unpack(hh, N)
    bad = []
    if not (np.all(np.isfinite(V)) and np.all(np.isfinite(tau))):
        return ['non-finite reflector data']
    taken = tau != 0.0
    K = int(np.argmin(taken)) if not taken.all() else N
    if taken[K:].any():
        bad.append('taus after the first zero tau: %r' % np.nonzero(taken)[0].tolist())
    if taken[N - 1]:
        bad.append('tau[N-1] = %r' % tau[N - 1])
    for k in range(N):
        if np.any(V[k, :k] != 0.0):
            bad.append('v_%d nonzero above row %d' % (k, k))
        if np.any(V[k, N:] != 0.0):
            bad.append('v_%d nonzero from row N on' % k)
        if not taken[k] and np.any(V[k] != 0.0):
            bad.append('v_%d nonzero with tau = 0' % k)
        if taken[k] and V[k, k] == 0.0:
            bad.append('v_%d has no diagonal entry' % k)
    if np.any(tau < 0.0):
        bad.append('negative tau')
    return bad


# ==== the reference =========================================================================================================
def symm(X):
    """The matrix the kernels read: the lower triangle mirrored."""
    return np.tril(X) + np.tril(X, -1).T


class Reference:
    """The device's reflectors applied in long double to X (N x N, symmetric)."""

    def __init__(self, X, hh):
        N = X.shape[0]
        self.N, self.NR = N, 8 * qr_rt(N)
        V, tau, _ = unpack(hh, N)
        self.V, self.tau = V[:, :N].astype(LD), tau.astype(LD)
        taken = tau != 0.0
        self.K = K = int(np.argmin(taken)) if not taken.all() else N
        S = X.astype(LD)
        self.colnorm = np.sqrt(np.sum(S * S, axis=0))
        self.fro = np.sqrt(np.sum(S * S))
        self.norms = np.zeros((K, N), dtype=LD)
        for k in range(K):
            self.norms[k] = np.sqrt(np.sum(S[k:] * S[k:], axis=0))
            v = self.V[k, k:]
            S[k:] -= np.outer(v, self.tau[k] * (v @ S[k:]))
        self.RPt = S
        self.delta = np.abs(self.tau[:K] * np.sum(self.V[:K] * self.V[:K], axis=1) - 2) if K else np.zeros(0, dtype=LD)

    def qt(self, A):
        """H_{K-1} ... H_0 A for the columns of A (N x m) or a vector."""
        A = np.array(A, dtype=LD)
        for k in range(self.K):
            v = self.V[k, k:]
            A[k:] -= np.multiply.outer(v, self.tau[k] * (v @ A[k:]))
        return A

    def q(self, A, skip_last=False):
        """H_0 ... H_{K-1} A."""
        A = np.array(A, dtype=LD)
        for k in range(self.K - 1 - (1 if skip_last else 0), -1, -1):
            v = self.V[k, k:]
            A[k:] -= np.multiply.outer(v, self.tau[k] * (v @ A[k:]))
        return A


def recover_pivots(RPt, K):
    """p_k = the not yet pivoted column of largest |RPt[k, .]| (the first one among equals), k < K; the rest in order."""
    N = RPt.shape[0]
    live = np.ones(N, dtype=bool)
    piv = []
    for k in range(K):
        row = np.where(live, np.abs(RPt[k]), -1)
        p = int(np.argmax(row))
        piv.append(p)
        live[p] = False
    return piv + [j for j in range(N) if live[j]]


def column_ratio(dev, ref, innorm, bound):
    """max over columns of |dev - ref| / (bound |input column|); a column of zero input must come out as the reference
    has it, exactly."""
    err = np.sqrt(np.sum((np.asarray(dev).astype(LD) - ref) ** 2, axis=0))
    innorm = np.atleast_1d(innorm)
    err = np.atleast_1d(err)
    if not np.all(np.isfinite(err)):
        return float('inf')
    worst = 0.0
    z = innorm == 0
    if np.any(err[z] != 0):
        return float('inf')
    if np.any(~z):
        worst = float(np.max(err[~z] / (bound * innorm[~z])))
    return worst


def pivot_steps(ref, piv):
    """Per taken step: (ratio of the pivot-rule inequality over the live columns, discriminating or not)."""
    N, K, NR = ref.N, ref.K, ref.NR
    live = np.ones(N, dtype=bool)
    cn = ref.colnorm
    ratios, disc = [], []
    for k in range(K):
        n = ref.norms[k]
        p = piv[k]
        pb = pivot_bound(k, NR)
        others = live.copy()
        others[p] = False
        if others.any():
            slack = pb * (cn[p] + cn[others])
            gap = n[others] - n[p]
            with np.errstate(divide='ignore', invalid='ignore'):
                r = np.where(gap > 0, gap / slack, 0)
            ratios.append(float(np.max(r)))
            # the two largest live norms: would the inequality reject the smaller, had it been pivoted?
            idx = np.nonzero(live)[0]
            order = idx[np.argsort(-n[idx], kind='stable')]
            a, b = order[0], order[1]
            disc.append(bool(n[a] - n[b] > pb * (cn[a] + cn[b])))
        else:
            ratios.append(0.0)
            disc.append(True)
        live[p] = False
    return ratios, disc


def discriminating_share(ref):
    """Share of the taken steps at which the pivot rule decides between the two largest remaining norms, from the reference
    alone (its own R P^T names the pivots)."""
    if ref.K == 0:
        return 1.0
    _, disc = pivot_steps(ref, recover_pivots(np.asarray(ref.RPt, dtype=np.float64), ref.K))
    return float(np.mean(disc))


CHECKS = ('layout', 'reflector', 'RPt', 'X1', 'y1', 'similarity', 'Qc', 'QV', 'vec_vs_mat', 'triangular', 'pivots_distinct',
          'pivot_rule')


def run_checks(X, y, out, C_in=None, V_in=None, skip=(), ref=None):
    """Every check on one system.  X: the symmetric input, y its right-hand side; out: dict with hh (packed), RPt, X1, y1 and,
    where C_in / V_in (V_in[j] = vector j) were given, C and V as the back-transformations left them.  Returns
    (ratios, info): ratios[name] = worst error / bound (<= 1 passes; exact checks give 0 or inf), info = K, pivots, share,
    the Reference (ref: one made before from the same X and out['hh'])."""
    N = X.shape[0]
    NR = 8 * qr_rt(N)
    r = {}
    bad = layout_problems(out['hh'], N)
    r['layout'] = float('inf') if bad else 0.0
    finite = all(np.all(np.isfinite(out[k])) for k in ('hh', 'RPt', 'X1', 'y1'))
    if not finite or (bad and bad[0].startswith('non-finite')):
        return dict.fromkeys(CHECKS, float('inf')), dict(K=-1, problems=bad or ['non-finite output'])
    ref = ref or Reference(X, out['hh'])
    K = ref.K
    bK = b_apply(K, NR)
    r['reflector'] = float(np.max(ref.delta) / refl_bound(NR)) if K else 0.0
    r['RPt'] = column_ratio(out['RPt'], ref.RPt, ref.colnorm, bK) if K else column_ratio(out['RPt'], ref.RPt, 0 * ref.colnorm, 1)
    Rd = np.asarray(out['RPt'])
    rown = np.sqrt(np.sum(Rd.astype(LD) ** 2, axis=1))
    # phase 2 on the device's own rows: X1[c, :] = Q^T (row c of R P^T)
    r['X1'] = column_ratio(np.asarray(out['X1']).T, ref.qt(Rd.T), rown if K else 0 * rown, bK if K else 1)
    yn = np.sqrt(np.sum(np.asarray(y).astype(LD) ** 2))
    r['y1'] = column_ratio(out['y1'], ref.qt(y), yn if K else 0 * yn, bK if K else 1)
    grow = (1.0 + refl_bound(NR)) ** K
    full = ref.qt(ref.RPt.T).T
    e = np.sqrt(np.sum((np.asarray(out['X1']).astype(LD) - full) ** 2))
    r['similarity'] = float(e / (bK * grow * (2 + bK) * ref.fro)) if K and ref.fro > 0 else (0.0 if e == 0 else float('inf'))
    qc = qv = None
    if C_in is not None:
        cn = np.sqrt(np.sum(np.asarray(C_in).astype(LD) ** 2))
        qc = ref.q(C_in)
        r['Qc'] = column_ratio(out['C'], qc, cn if K else 0 * cn, bK if K else 1)
    if V_in is not None:
        vn = np.sqrt(np.sum(np.asarray(V_in).astype(LD) ** 2, axis=1))
        qv = ref.q(np.asarray(V_in).T)
        r['QV'] = column_ratio(np.asarray(out['V']).T, qv, vn if K else 0 * vn, bK if K else 1)
    if 'C_as_column' in out:
        # the same vector through k_qr_back_vec and as a column of k_qr_back_mat: each within b(K) of the reference
        j, col = out['C_as_column']
        d = np.sqrt(np.sum((np.asarray(out['C']).astype(LD) - np.asarray(col).astype(LD)) ** 2))
        cn = np.sqrt(np.sum(np.asarray(C_in).astype(LD) ** 2))
        r['vec_vs_mat'] = float(d / (2 * bK * cn)) if K and cn > 0 else (0.0 if d == 0 else float('inf'))
    piv = recover_pivots(Rd, K)
    r['pivots_distinct'] = 0.0 if sorted(piv) == list(range(N)) else float('inf')
    info = dict(K=K, piv=piv, ref=ref, problems=bad)
    if 'triangular' not in skip:
        R = Rd[:, piv].astype(LD)
        below = np.sqrt(np.sum(np.tril(R, -1) ** 2, axis=0))
        r['triangular'] = column_ratio(below[None, :], np.zeros((1, N), dtype=LD), ref.colnorm[piv], tri_bound(K, NR)) if K else (
            0.0 if not np.any(below) else float('inf'))
    if 'pivot_rule' not in skip:
        ratios, _ = pivot_steps(ref, piv)
        r['pivot_rule'] = max(ratios) if ratios else 0.0
    return r, info


def worst(ratio_dicts):
    out = {}
    for r in ratio_dicts:
        for k, v in r.items():
            out[k] = max(out.get(k, 0.0), v)
    return out


def fmt(ratios):
    return '  '.join('%s %.3g' % (k, ratios[k]) for k in CHECKS if k in ratios)


# ==== inputs ================================================================================================================
def scale_to_one(X):
    """Times the power of two that brings max|x| into [1, 2), as the solves scale their systems."""
    m = np.max(np.abs(X))
    return X * 2.0 ** (1 - np.frexp(m)[1]) if m > 0 else X


def graded(rng, N, decades, factor=1.0):
    """Q diag(10^U(-decades, 0) * +-1) Q^T, symmetric in bits, scaled to max|x| in [1, 2), times `factor` (a power of two)."""
    Q, _ = np.linalg.qr(rng.standard_normal((N, N)))
    lam = 10.0 ** rng.uniform(-decades, 0, N) * rng.choice([-1.0, 1.0], N)
    M = (Q * lam) @ Q.T
    return scale_to_one(symm(M)) * factor


def golden_systems(e, count=3):
    """The first systems of tests/golden/exact_default_c2.npz, lower triangle mirrored, scaled."""
    return np.array([scale_to_one(symm(e['X'][i])) for i in range(count)]), np.array(e['y'][:count])


def tie_pairs(N):
    """(a, b), a < b, of the integer tie systems: one thread, two octets of one wave, two waves (N > 16), the last two."""
    pairs = [(2, 3), (1, 6)]
    if N > 16:
        pairs.append((5, 16 + (N - 16) // 2))
    pairs.append((N - 2, N - 1))
    return pairs


def tie_system(rng, N, a, b):
    """Integers in [-3, 3], symmetric, but columns (and rows) a and b: 64 on the diagonal alone.  Every squared norm is an
    exact integer, 4096 for a and b and at most 9 N < 4096 for the others: step 0 is an exact tie of a and b."""
    assert 9 * N < 4096 and 0 < a < b < N
    M = rng.integers(-3, 4, (N, N)).astype(np.float64)
    M = np.tril(M) + np.tril(M, -1).T
    for c in (a, b):
        M[c, :] = 0
        M[:, c] = 0
        M[c, c] = 64.0
    return M


def tie_problems(hh, N, a, b):
    """Step 0 of a tie system must pivot the lower column a: v_0 = 64 e_0 + 64 e_a, tau_0 = 1 / 4096."""
    V, tau, _ = unpack(hh, N)
    want = np.zeros(V.shape[1])
    want[0] = 64.0
    want[a] = 64.0
    bad = []
    if not np.array_equal(V[0], want):
        bad.append('v_0 has nonzeros on rows %r, wanted rows 0 and %d (column %d tied with column %d)'
                   % (np.nonzero(V[0])[0].tolist(), a, a, b))
    if tau[0] != 1.0 / 4096:
        bad.append('tau_0 = %r' % tau[0])
    return bad


def block_system(rng, N, r):
    """blockdiag(M_r, 0) under a symmetric permutation, M_r a full symmetric r x r block; returns (X, rows of the block)."""
    rows = np.sort(rng.permutation(N)[:r])
    M = rng.standard_normal((r, r))
    M = M + M.T + 4 * np.eye(r)
    X = np.zeros((N, N))
    X[np.ix_(rows, rows)] = M
    return scale_to_one(X), rows


def subnormal_system(rng, N):
    """blockdiag(M, 2^-520 M'), M' 3 x 3, max|x| in [1, 2): the last three columns have norms about 3e-157, whose squares
    are subnormal."""
    X = np.zeros((N, N))
    X[:N - 3, :N - 3] = graded(rng, N - 3, 2)
    Mp = rng.standard_normal((3, 3))
    X[N - 3:, N - 3:] = (Mp + Mp.T) * 2.0 ** -520
    return X


def identity_problems(out, N, m):
    """X = 2^m I: every step a tie, pivots 0, 1, 2, ...; v_k = 2^(m+1) e_k; R P^T = -2^m I but +2^m in the last row."""
    V, tau, _ = unpack(out['hh'], N)
    bad = []
    wantV = np.zeros_like(V)
    for k in range(N - 1):
        wantV[k, k] = 2.0 ** (m + 1)
    if not np.array_equal(V, wantV):
        bad.append('reflectors are not 2^(m+1) e_k: first difference at %r' % (np.argwhere(V != wantV)[0].tolist(),))
    wtau = np.full(N, 2.0 ** -(2 * m + 1))
    wtau[N - 1] = 0
    if not np.array_equal(tau, wtau):
        bad.append('taus are not 2^-(2m+1)')
    wantR = -(2.0 ** m) * np.eye(N)
    wantR[N - 1, N - 1] = 2.0 ** m
    if not np.array_equal(out['RPt'], wantR):
        bad.append('R P^T is not -2^m I (+2^m last)')
    if recover_pivots(np.asarray(out['RPt']), N - 1) != list(range(N)):
        bad.append('pivots are not 0, 1, 2, ...')
    if not np.max(np.abs(out['X1'] - 2.0 ** m * np.eye(N))) <= 4 * 2 * U * 2.0 ** m:
        bad.append('X1 is not X to 4 ulps')
    return bad


# ==== float64 emulation of the kernels' algorithm ===========================================================================
def emulate(X, y, tie='low', pivot='norm', runner_up_at=None):
    """k_qr_sim in float64 NumPy: returns dict(hh, RPt, X1, y1, piv, K).  pivot: 'norm' (the kernel's rule) or 'none';
    tie: 'low' or 'high'; runner_up_at: a step at which the second largest norm is pivoted."""
    N = X.shape[0]
    NR = 8 * qr_rt(N)
    A = np.concatenate([symm(X), np.asarray(y, dtype=np.float64)[:, None]], axis=1)
    live = np.ones(N, dtype=bool)
    V = np.zeros((N, NR))
    tau = np.zeros(N)
    RPt = np.zeros((N, N))
    piv = []
    K = 0
    for k in range(N - 1):
        n2 = np.where(live, np.sum(A[k:, :N] * A[k:, :N], axis=0), -1.0)
        if pivot == 'none':
            p = int(np.nonzero(live)[0][0])
        elif tie == 'high':
            p = N - 1 - int(np.argmax(n2[::-1]))
        else:
            p = int(np.argmax(n2))
        if runner_up_at == k:
            n2b = n2.copy()
            n2b[p] = -1.0
            p = int(np.argmax(n2b))
        pmax = n2[p]
        if not pmax >= TINY:                             # zero, or below the normal range: nothing left to reflect
            break
        x = A[k:, p].copy()
        xk = x[0]
        nx = np.sqrt(pmax)
        x[0] = xk + np.copysign(nx, xk)
        t = 1.0 / (nx * (nx + abs(xk)))
        V[k, k:N] = x
        tau[k] = t
        A[k:] -= np.outer(x, t * (x @ A[k:]))
        RPt[k] = A[k, :N]
        A[k] = 0.0
        live[p] = False
        piv.append(p)
        K = k + 1
    RPt[K:] = A[K:, :N]
    X1 = np.array(RPt)                                   # row c takes all reflectors
    y1 = np.array(y, dtype=np.float64)
    for k in range(K):
        v = V[k, k:N]
        X1[:, k:] -= np.outer(tau[k] * (X1[:, k:] @ v), v)
        y1[k:] -= tau[k] * (v @ y1[k:]) * v
    return dict(hh=pack(V, tau, N), RPt=RPt, X1=X1, y1=y1, piv=piv, K=K)


def emulate_back(hh, N, A, transpose=False, skip_last=False):
    """k_qr_back_vec / k_qr_back_mat in float64: H_0 ... H_{K-1} applied to the columns of A (or a vector); transpose: the
    wrong order H_{K-1} ... H_0; skip_last: without H_{K-1}."""
    V, tau, _ = unpack(hh, N)
    A = np.array(A, dtype=np.float64)
    ks = [k for k in range(N - 1) if tau[k] != 0.0]
    if skip_last:
        ks = ks[:-1]
    for k in (ks if transpose else ks[::-1]):
        v = V[k, k:N]
        A[k:] -= np.multiply.outer(v, tau[k] * (v @ A[k:]))
    return A
