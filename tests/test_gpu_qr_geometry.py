"""K3p (csrc/vi_qr.hip), the pivoted Householder pre-conditioner of the cold solves, reflector by reflector at every tile
size: k_qr_sim<RT>, k_qr_back_vec<EPL> and k_qr_back_mat<RT> through the stage entry vi_qr_stage_f64, which hands out the
packed reflectors and the rows of R P^T and calls the kernels the way the solves do (y through d_rec, X1 in place, a
reflector stride of its own).

The order list (tests/qr_ref.py NS; tests/test_qr_ref_host.py shows that it reaches every class) has both sides of every
RT boundary (32 | 33, 48 | 49, 64 | 65, 96 | 97) and of every EPL boundary (64 | 65, 128 | 129), the full 320- and
640-thread launches (N = 64, 144), odd and even orders in every class (y as column c1 of a matrix octet, or c0 of its own) and
the first octet-row boundary of the steps (k = 8).

Known by construction: X = 0 (no reflector, inputs back in their bits), X = 2^m I (every step an exact tie), integer systems
with an exact tie at step 0 between two columns of one thread, two octets, two waves and the last pair, and systems of rank
1 and 10 (the factorisation stops after exactly that many reflectors).  Real systems - graded over 2 to 30 decades, the same
times 2^-63, and at N = 144 the default-order systems of tests/golden/exact_default_c2.npz - go through every check of
tests/qr_ref.py: the reference applies the DEVICE's reflectors in long double, so each comparison is a forward bound of
known reflectors on a known input, and the pivot rule is held against the reference's remaining norms at every step.
One system keeps its bits alone and at the first, middle and last place of batches of 3 and 257, with y fetched through
d_rec, with X1 written over X, and with packed, packed + 2 and 16-byte rounded reflector strides; every output lies between
sentinel doubles and the stride gaps keep theirs.

Finding (test_subnormal_remaining_norm): a remaining column whose norm lies between about 1e-162 and 1e-154 while the matrix
maximum is about 1 has a squared norm below the normal range.  k_qr_sim took it as a pivot like any other: tau =
1 / (|x| (|x| + |x_k|)) is then about 1 / pmax > 1.8e308, which is inf in float64, and the update spread NaN.  On the
MI355X, blockdiag(M, 2^-520 M') in batches of three came back with one non-finite tau per system and, at N = 16 / 144, 144 /
1296 non-finite values in R P^T, 456 / 4680 in X1, 24 / 24 in y1, 48 / 432 in Q c and 768 / 62 208 in Q V.  Smaller columns
square to exactly zero and end the factorisation cleanly; larger ones are fine.  The systems of the fit are graded over some 50 decades only, so no solve of the suite comes near it.  k_qr_sim now
ends phase 1 when the largest remaining squared norm is below the smallest normal number, as it does for an exact zero:
what is left (at most 1.5e-154 of the matrix maximum) stays in the rows of R P^T as it is, so X1 = Q^T X Q still holds.  The
new exit is taken only where 0 < pmax < 2.2e-308: every other output of this file (all launches of the three other test groups
at the 22 orders) and every result of test_gpu_solver_geometry.run_geometry at the orders up to 144 kept its bits across the
change (471 digests compared), and the case now passes with K = N - 3 reflectors at ratios like those of the other systems."""
import numpy as np
import pytest

import qr_ref as q
from conftest import load_golden
from test_gpu_resident_geometry import GUARD, SENTINEL

pytestmark = pytest.mark.gpu
VI_ERR_UNSUPPORTED = -6
SB = np.array([SENTINEL]).view(np.uint64)[0]


def _L():
    from volumetricinterp_amd import _lib, fitengine  # noqa: F401 (registers the signatures of the fit entries)
    return _lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Guarded:
    """A device buffer of n doubles between GUARD sentinel doubles on either side, filled with sentinels or `init`."""

    def __init__(self, ctx, n, init=None):
        host = np.full(2 * GUARD + n, SENTINEL)
        if init is not None:
            host[GUARD:GUARD + n] = np.ravel(init)
        self.n, self.dev = n, ctx.to_device(host)
        self.ptr = self.dev.offset_ptr(GUARD)

    def fetch(self, what):
        host = self.dev.download()
        u = host.view(np.uint64)
        assert np.all(u[:GUARD] == SB) and np.all(u[GUARD + self.n:] == SB), 'sentinels around %s overwritten' % what
        return host[GUARD:GUARD + self.n]


def stage(X, y, C=None, V=None, rec=None, inplace=False, stride=0, expect=0):
    """vi_qr_stage_f64 on B systems.  X (B, N, N); y (T, N), row rec[i] for system i (row i without rec); C (B, N) and V (B, N, N;
    V[i, j] = vector j) are transformed in place, or left out.  Returns dict(hh (B packed sets), RPt, X1, y1, C, V); the
    inputs that are only read are compared with what was uploaded."""
    _lib = _L()
    ctx = _lib.get_context()
    B, N = X.shape[0], X.shape[1]
    P = int(_lib.lib.vi_qr_hh_doubles(N))
    assert P == q.hh_doubles(N)
    st = stride or P or 1
    dy = ctx.to_device(y)
    drec = ctx.to_device(np.asarray(rec, np.int32)) if rec is not None else None
    gX1 = Guarded(ctx, B * N * N, X if inplace else None)
    dX = None if inplace else ctx.to_device(X)
    gy1, ghh, gR = Guarded(ctx, B * N), Guarded(ctx, B * st), Guarded(ctx, B * N * N)
    gC = Guarded(ctx, B * N, C) if C is not None else None
    gV = Guarded(ctx, B * N * N, V) if V is not None else None
    rc = _lib.lib.vi_qr_stage_f64(ctx.handle, B, N, gX1.ptr if inplace else dX.ptr, dy.ptr, drec.ptr if drec is not None else None,
                                  gX1.ptr, gy1.ptr, ghh.ptr, stride, gR.ptr, gC.ptr if gC else None, gV.ptr if gV else None)
    assert rc == expect, (rc, _lib.lib.vi_last_error())
    ctx.sync()
    out = dict(X1=gX1.fetch('X1').reshape(B, N, N), y1=gy1.fetch('y1').reshape(B, N), RPt=gR.fetch('R P^T').reshape(B, N, N))
    hh = ghh.fetch('hh')
    out['hh_raw'] = hh
    if rc == 0:
        out['hh'] = np.array(q.split_sets(hh, B, N, st))
        gaps = hh.reshape(B, st)[:, P:]
        assert np.all(gaps.view(np.uint64) == SB), 'the stride gaps of hh were written'
    out['C'] = gC.fetch('C').reshape(B, N) if gC else None
    out['V'] = gV.fetch('V').reshape(B, N, N) if gV else None
    assert same_bits(dy.download(), np.ascontiguousarray(y, dtype=np.float64)), 'd_y was written'
    if dX is not None:
        assert same_bits(dX.download(), X), 'd_X was written'
    return out


def one(out, i, C_as_column=True):
    o = {k: out[k][i] for k in ('hh', 'RPt', 'X1', 'y1')}
    if out['C'] is not None:
        o['C'] = out['C'][i]
    if out['V'] is not None:
        o['V'] = out['V'][i]
        if C_as_column and out['C'] is not None:
            o['C_as_column'] = (0, out['V'][i][0])
    return o


def vectors(rng, B, N, T=None):
    """y, C and V (vector 0 of every V is that system's C, for the comparison of the two back kernels)."""
    y, C = rng.standard_normal((T or B, N)), rng.standard_normal((B, N))
    V = rng.standard_normal((B, N, N))
    V[:, 0] = C
    return y, C, V


OUTS = ('hh', 'RPt', 'X1', 'y1', 'C', 'V')


# ==== the entry itself ======================================================================================================
def test_packed_size_and_unsupported_orders():
    """vi_qr_hh_doubles is the restated packed size at every order, 0 outside 8 .. 144; there vi_qr_stage_f64 returns
    VI_ERR_UNSUPPORTED and writes nothing."""
    _lib = _L()
    for N in range(1, 200):
        assert int(_lib.lib.vi_qr_hh_doubles(N)) == q.hh_doubles(N), N
    rng = np.random.default_rng(1)
    for N in (7, 145):
        X = np.array([q.graded(rng, N, 2)])
        y, C, V = vectors(rng, 1, N)
        out = stage(X, y, C, V, stride=12000, expect=VI_ERR_UNSUPPORTED)
        for k in ('X1', 'y1', 'RPt', 'hh_raw'):
            assert np.all(bits(out[k]) == SB), (N, k)
        assert same_bits(out['C'], C) and same_bits(out['V'], V)


# ==== known by construction =================================================================================================
@pytest.mark.parametrize('N', q.NS)
def test_known_by_construction(N):
    rng = np.random.default_rng(100 + N)
    kinds, Xs = [], []
    kinds.append(('zero',))
    Xs.append(np.zeros((N, N)))
    for m in (0, -40):
        kinds.append(('identity', m))
        Xs.append(2.0 ** m * np.eye(N))
    for a, b in q.tie_pairs(N):
        kinds.append(('tie', a, b))
        Xs.append(q.tie_system(rng, N, a, b))
    for r in (1, 10):
        if r < N - 1:
            X, rows = q.block_system(rng, N, r)
            kinds.append(('block', r, rows))
            Xs.append(X)
    X = np.array(Xs)
    B = len(Xs)
    y, C, V = vectors(rng, B, N)
    out = stage(X, y, C, V)
    worst = []
    for i, kind in enumerate(kinds):
        o = one(out, i)
        r, info = q.run_checks(X[i], y[i], o, C[i], V[i])
        print('N %3d %-22s K %3d  %s' % (N, kind[:3] if kind[0] != 'block' else kind[:2], info['K'], q.fmt(r)))
        assert all(v <= 1.0 for v in r.values()), (N, kind, q.fmt(r), info.get('problems'))
        worst.append(r)
        if kind[0] == 'zero':
            assert info['K'] == 0 and not np.any(o['hh']) and not np.any(o['X1']) and not np.any(o['RPt'])
            assert same_bits(o['y1'], y[i]) and same_bits(o['C'], C[i]) and same_bits(o['V'], V[i])
        elif kind[0] == 'identity':
            assert q.identity_problems(o, N, kind[1]) == [], (N, kind)
        elif kind[0] == 'tie':
            assert q.tie_problems(o['hh'], N, kind[1], kind[2]) == [], (N, kind)
            assert info['K'] == N - 1 and info['piv'][0] == kind[1]
        else:
            assert info['K'] == kind[1] and sorted(info['piv'][:kind[1]]) == kind[2].tolist(), (N, kind, info['K'])
            assert not np.any(q.unpack(o['hh'], N)[1][kind[1]:])
    print('N %3d RT %2d worst  %s' % (N, q.qr_rt(N), q.fmt(q.worst(worst))))


# ==== real systems through every check ======================================================================================
CAPS = {2: 0.90, 6: 0.90, 9: 0.90, 12: 0.75, 'golden': 0.75}
PER_FAMILY = 3


def real_systems(rng, N):
    fams, Xs = [], []
    for d in (2, 6, 9, 12, 30):
        for factor in (1.0, 2.0 ** -63):
            for _ in range(PER_FAMILY):
                fams.append((d, factor))
                Xs.append(q.graded(rng, N, d, factor))
    return fams, np.array(Xs)


@pytest.mark.parametrize('N', q.NS)
def test_real_systems_through_every_check(N):
    rng = np.random.default_rng(200 + N)
    fams, X = real_systems(rng, N)
    B = len(fams)
    y, C, V = vectors(rng, B, N)
    if N == 144:
        gX, gy = q.golden_systems(load_golden('exact_default_c2'))
        fams += [('golden', 1.0)] * len(gX)
        X = np.concatenate([X, gX])
        y2, C2, V2 = vectors(rng, len(gX), N)
        y, C, V = np.concatenate([y, gy]), np.concatenate([C, C2]), np.concatenate([V, V2])
        B = len(fams)
    out = stage(X, y, C, V)
    eye = np.broadcast_to(np.eye(N), (B, N, N)).copy()
    out_eye = stage(X, y, None, eye)                           # the explicit Q
    for k in ('hh', 'RPt', 'X1', 'y1'):
        assert same_bits(out[k], out_eye[k]), k
    per = {}
    for i, (fam, factor) in enumerate(fams):
        o = one(out, i)
        assert q.layout_problems(o['hh'], N) == [], (N, fam, i)
        ref = q.Reference(X[i], o['hh'])
        assert ref.K == N - 1, (N, fam, i, ref.K)
        if fam != 30:                                          # a condition on the inputs, asserted before the device is compared
            share = q.discriminating_share(ref)
            assert share >= CAPS[fam], (N, fam, i, share)
            per.setdefault((fam, 'share'), []).append(share)
        r, info = q.run_checks(X[i], y[i], o, C[i], V[i], ref=ref)
        r['QV'] = max(r['QV'], q.column_ratio(out_eye['V'][i].T, ref.q(eye[i]), np.ones(N), q.b_apply(ref.K, ref.NR)))
        assert all(v <= 1.0 for v in r.values()), (N, fam, factor, i, q.fmt(r), info.get('problems'))
        per.setdefault(fam, []).append(r)
    for fam in (2, 6, 9, 12, 30, 'golden'):
        if fam in per:
            sh = per.get((fam, 'share'))
            print('N %3d RT %2d %-7s %s%s' % (N, q.qr_rt(N), fam if fam == 'golden' else '%d dec' % fam, q.fmt(q.worst(per[fam])),
                                            '  share >= %.2f' % min(sh) if sh else ''))
    print('N %3d RT %2d worst   %s' % (N, q.qr_rt(N), q.fmt(q.worst([r for k, v in per.items() if not isinstance(k, tuple) for r in v]))))


# ==== launch independence, bit for bit ======================================================================================
@pytest.mark.parametrize('N', q.NS)
def test_launch_independence(N):
    rng = np.random.default_rng(300 + N)
    probe = q.graded(rng, N, 9)
    fill = np.array([q.graded(rng, N, d) for d in (2, 12, 30)])
    py, pC, pV = vectors(rng, 1, N)
    fy, fC, fV = vectors(rng, 3, N)
    alone = stage(probe[None], py, pC, pV)
    for B in (3, 257) if N <= 33 else (3,):
        for place in (0, B // 2, B - 1):
            idx = np.arange(B) % 3
            X, y, C, V = fill[idx], fy[idx], fC[idx], fV[idx]
            X[place], y[place], C[place], V[place] = probe, py[0], pC[0], pV[0]
            out = stage(X, y, C, V)
            for k in OUTS:
                assert same_bits(out[k][place], alone[k][0]), (N, B, place, k)
    # a batch of three under every way of calling
    X = np.concatenate([probe[None], fill[:2]])
    y, C, V = np.concatenate([py, fy[:2]]), np.concatenate([pC, fC[:2]]), np.concatenate([pV, fV[:2]])
    base = stage(X, y, C, V)
    P = q.hh_doubles(N)
    rec = np.array([4, 0, 2], np.int32)
    yrec = rng.standard_normal((5, N))
    yrec[rec] = y
    variants = dict(rec=dict(y=yrec, rec=rec), inplace=dict(inplace=True), stride2=dict(stride=P + 2),
                    up16=dict(stride=q.up16_doubles(N)),
                    engine=dict(y=yrec, rec=rec, inplace=True, stride=q.up16_doubles(N)))
    for name, kw in variants.items():
        kw = dict(kw)
        out = stage(X, kw.pop('y', y), C, V, **kw)
        for k in OUTS:
            assert same_bits(out[k], base[k]), (N, name, k)


# ==== the subnormal-norm edge ===============================================================================================
@pytest.mark.parametrize('N', [16, 144])
def test_subnormal_remaining_norm(N):
    """blockdiag(M, 2^-520 M'), M' 3 x 3, max|x| about 1: the last three columns have squared norms below the normal range.
    Every output is finite and the reflector, application and similarity checks hold (see the finding above)."""
    rng = np.random.default_rng(400 + N)
    B = 3
    X = np.array([q.subnormal_system(rng, N) for _ in range(B)])
    y, C, V = vectors(rng, B, N)
    out = stage(X, y, C, V)
    for k in OUTS:
        print('N %3d %-3s non-finite values: %d' % (N, k, np.count_nonzero(~np.isfinite(out[k]))))
    for k in OUTS:
        assert np.all(np.isfinite(out[k])), (N, k, np.count_nonzero(~np.isfinite(out[k])))
    for i in range(B):
        r, info = q.run_checks(X[i], y[i], one(out, i), C[i], V[i], skip=('triangular', 'pivot_rule'))
        print('N %3d system %d K %3d  %s' % (N, i, info['K'], q.fmt(r)))
        assert all(v <= 1.0 for v in r.values()), (N, i, q.fmt(r), info.get('problems'))
