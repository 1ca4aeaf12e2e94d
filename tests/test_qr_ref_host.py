"""tests/qr_ref.py on the host: the N list of tests/test_gpu_qr_geometry.py reaches every launch class of K3p
(csrc/vi_qr.hip), the input families decide the pivot often enough to test the pivot rule, a float64 emulation of the
kernels' algorithm lies inside every derived bound (the worst error / bound ratios are printed), and every emulated
wrong answer of the list is rejected by at least one check.  No GPU."""
import numpy as np
import pytest

import qr_ref as q
from conftest import load_golden


def test_case_list_covers_every_class():
    """The restated formulas over N = 8 .. 144 and the classes the list reaches; prints the case table."""
    print('\n'.join(q.case_table()))
    G = {N: q.geometry(N) for N in q.NS}
    every = {N: q.geometry(N) for N in range(8, 145)}
    assert not q.supported(7) and not q.supported(145) and q.hh_doubles(7) == 0 and q.hh_doubles(145) == 0
    assert all(q.supported(N) for N in range(8, 145)) and q.lds_bytes(144) <= q.LDS_LIMIT
    # every (RT, EPL, parity) class that exists is in the list, and both sides of every boundary
    assert {(g['rt'], g['epl'], g['odd']) for g in G.values()} == {(g['rt'], g['epl'], g['odd']) for g in every.values()}
    assert {g['rt'] for g in G.values()} == set(q.RTS)
    for lo in (32, 48, 64, 96):
        assert lo in G and lo + 1 in G and G[lo]['rt'] < G[lo + 1]['rt'] and G[lo]['full_rows']
    assert 8 in G and 144 in G and G[144]['full_rows'] and not G[143]['full_rows']
    for lo in (64, 128):
        assert G[lo]['epl'] + 1 == G[lo + 1]['epl']
    assert (G[64]['rt'], G[65]['rt'], G[128]['rt'], G[129]['rt']) == (8, 12, 18, 18)      # the EPL switch is no RT boundary
    # the thread-count edges
    assert G[64]['sim'] == 320 and G[64]['full_block'] and G[144]['sim'] == 640 and G[144]['full_block']
    assert G[63]['sim'] == 256 and G[143]['sim'] == 576
    for N, g in every.items():
        assert g['sim'] <= (320 if g['rt'] <= 8 else 640) and g['back_mat'] <= (320 if g['rt'] <= 8 else 640)
        assert g['sim'] // 8 * 2 >= N + 1 and g['back_mat'] // 8 * 2 >= N and g['NR'] >= N and 64 * g['epl'] >= N
        assert g['sim'] % 64 == 0 and g['back_mat'] % 64 == 0
    assert {g['waves'] for g in G.values()} >= {1, 2, 3, 4, 5, 7, 9, 10}
    assert any(g['sim'] != g['back_mat'] for g in G.values())             # the y column opens a wave of its own (N = 16, ...)
    # the packed layout: consecutive, v_k stored from row 8 (k >> 3) on
    for N in q.NS:
        NR = G[N]['NR']
        assert q.hh_off(0, NR) == 0
        assert all(q.hh_off(k + 1, NR) - q.hh_off(k, NR) == NR - 8 * (k >> 3) for k in range(N))
        assert q.hh_doubles(N) == q.hh_off(N, NR) + N and 0 <= G[N]['stride16'] - G[N]['hh'] <= 1
    assert {G[N]['stride16'] - G[N]['hh'] for N in q.NS} == {0, 1}
    assert q.hh_doubles(144) == 10944 + 144
    # tie pairs: one thread, two octets of a wave, two waves, the last two columns
    for N in q.NS:
        pairs = q.tie_pairs(N)
        assert pairs[0][0] // 2 == pairs[0][1] // 2
        assert pairs[1][0] // 2 != pairs[1][1] // 2 and pairs[1][0] // 16 == pairs[1][1] // 16
        assert (N <= 16) or pairs[2][0] // 16 != pairs[2][1] // 16
        assert pairs[-1] == (N - 2, N - 1) and all(0 < a < b < N for a, b in pairs)


# ==== the emulation through every check =====================================================================================
def emulated(X, y, C, Vs, **kw):
    """The emulation's outputs in the form run_checks takes; Vs: V_in with V_in[j] = vector j, column 0 replaced by C."""
    N = X.shape[0]
    out = q.emulate(X, y, **kw)
    out['C'] = q.emulate_back(out['hh'], N, C)
    out['V'] = q.emulate_back(out['hh'], N, Vs.T).T
    out['C_as_column'] = (0, out['V'][0])
    return out


def inputs(rng, N):
    y, C = rng.standard_normal(N), rng.standard_normal(N)
    Vs = rng.standard_normal((N, N))
    Vs[0] = C
    return y, C, Vs


FAMILIES = [(N, d) for N in (8, 33, 64, 97, 144) for d in (2, 6, 9)] + [(N, 12) for N in (64, 97, 144)] + [(N, 30) for N in (33, 144)]
CAPS = {2: 0.90, 6: 0.90, 9: 0.90, 12: 0.75, 'golden': 0.75}


@pytest.fixture(scope='module')
def runs():
    """(name, family, N, X, y, C, Vs, out) of every emulated system, computed once."""
    rng = np.random.default_rng(20240607)
    rows = []
    for N, d in FAMILIES:
        for factor in (1.0, 2.0 ** -63):
            X = q.graded(rng, N, d, factor)
            y, C, Vs = inputs(rng, N)
            rows.append(('graded %2d decades%s' % (d, ' x 2^-63' if factor != 1.0 else ''), d, N, X, y, C, Vs, emulated(X, y, C, Vs)))
    gX, gy = q.golden_systems(load_golden('exact_default_c2'))
    for i in range(3):
        _, C, Vs = inputs(rng, 144)
        rows.append(('exact_default_c2[%d]' % i, 'golden', 144, gX[i], gy[i], C, Vs, emulated(gX[i], gy[i], C, Vs)))
    return rows


def test_inputs_decide_the_pivot_often_enough(runs):
    """From the reference alone: the share of steps at which the pivot inequality separates the two largest remaining norms is
    at least 90 % for the families of up to 9 decades, 75 % for the 12-decade family and the golden systems."""
    for name, fam, N, X, y, C, Vs, out in runs:
        if fam == 30:
            continue
        ref = q.Reference(X, out['hh'])
        share = q.discriminating_share(ref)
        print('N %3d  %-28s steps %3d  discriminating %5.1f %%' % (N, name, ref.K, 100 * share))
        assert ref.K == N - 1
        assert share >= CAPS[fam], (name, N, share)


def test_emulation_lies_inside_every_bound(runs):
    per_family = {}
    for name, fam, N, X, y, C, Vs, out in runs:
        r, info = q.run_checks(X, y, out, C, Vs)
        assert info['K'] == N - 1 and info['piv'][:N - 1] == out['piv'], (name, N)
        assert all(v <= 1.0 for v in r.values()), (name, N, q.fmt(r))
        per_family.setdefault((q.qr_rt(N), name), []).append(r)
    for (rt, name), rs in sorted(per_family.items()):
        print('RT %2d  %-28s %s' % (rt, name, q.fmt(q.worst(rs))))


def test_emulation_on_the_systems_known_by_construction():
    rng = np.random.default_rng(5)
    for N in (8, 17, 33, 144):
        y, C, Vs = inputs(rng, N)
        # zero: no reflector, everything comes back as it went in
        out = emulated(np.zeros((N, N)), y, C, Vs)
        r, info = q.run_checks(np.zeros((N, N)), y, out, C, Vs)
        assert info['K'] == 0 and all(v == 0.0 for v in r.values()), q.fmt(r)
        assert not np.any(out['hh']) and np.array_equal(out['y1'], y) and np.array_equal(out['C'], C)
        for m in (0, -40):
            X = 2.0 ** m * np.eye(N)
            out = emulated(X, y, C, Vs)
            assert q.identity_problems(out, N, m) == []
            r, _ = q.run_checks(X, y, out, C, Vs)
            assert all(v <= 1.0 for v in r.values()), q.fmt(r)
        for a, b in q.tie_pairs(N):
            X = q.tie_system(rng, N, a, b)
            out = emulated(X, y, C, Vs)
            assert q.tie_problems(out['hh'], N, a, b) == []
            r, _ = q.run_checks(X, y, out, C, Vs)
            assert all(v <= 1.0 for v in r.values()), q.fmt(r)
        for rank in (1, 10):
            if rank >= N:
                continue
            X, rows = q.block_system(rng, N, rank)
            out = emulated(X, y, C, Vs)
            r, info = q.run_checks(X, y, out, C, Vs)
            assert info['K'] == rank and sorted(info['piv'][:rank]) == rows.tolist()
            assert all(v <= 1.0 for v in r.values()), q.fmt(r)
    for N in (16, 144):
        X = q.subnormal_system(rng, N)
        y, C, Vs = inputs(rng, N)
        out = emulated(X, y, C, Vs)
        r, info = q.run_checks(X, y, out, C, Vs, skip=('triangular', 'pivot_rule'))
        assert info['K'] == N - 3 and all(v <= 1.0 for v in r.values()), q.fmt(r)
        print('subnormal edge N %3d  %s' % (N, q.fmt(r)))


# ==== wrong answers =========================================================================================================
def _base(N=33, decades=6, seed=11):
    rng = np.random.default_rng(seed)
    X = q.graded(rng, N, decades)
    y, C, Vs = inputs(rng, N)
    return rng, N, X, y, C, Vs, emulated(X, y, C, Vs)


def _rejected(r):
    return sorted(k for k, v in r.items() if v > 1.0)


def test_every_listed_wrong_answer_is_rejected():
    rng, N, X, y, C, Vs, good = _base()
    r0, info0 = q.run_checks(X, y, good, C, Vs)
    assert _rejected(r0) == []
    rep = {}

    def mutated(**changes):
        out = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        out.update(changes)
        return q.run_checks(X, y, out, C, Vs)[0]

    # the runner-up pivoted at a discriminating step
    _, disc = q.pivot_steps(info0['ref'], info0['piv'])
    k = [i for i, d in enumerate(disc) if d][len(disc) // 2]
    r = q.run_checks(X, y, emulated(X, y, C, Vs, runner_up_at=k), C, Vs)[0]
    rep['runner-up pivoted at step %d' % k] = _rejected(r)
    assert r['pivot_rule'] > 1.0
    # no pivoting at all
    r = q.run_checks(X, y, emulated(X, y, C, Vs, pivot='none'), C, Vs)[0]
    rep['no pivoting'] = _rejected(r)
    assert r['pivot_rule'] > 1.0
    # ties to the higher column: the systems with exact ties
    a, b = q.tie_pairs(N)[1]
    Xt = q.tie_system(rng, N, a, b)
    bad = q.tie_problems(emulated(Xt, y, C, Vs, tie='high')['hh'], N, a, b)
    rep['ties to the higher column (tie system)'] = bad
    assert bad and q.tie_problems(emulated(Xt, y, C, Vs)['hh'], N, a, b) == []
    bad = q.identity_problems(emulated(np.eye(N), y, C, Vs, tie='high'), N, 0)
    rep['ties to the higher column (identity)'] = bad
    assert bad
    # tau off by a relative 1e-12
    V, tau, _ = q.unpack(good['hh'], N)
    t2 = tau.copy()
    t2[5] *= 1 + 1e-12
    r = mutated(hh=q.pack(V, t2, N))
    rep['tau_5 off by 1e-12'] = _rejected(r)
    assert r['reflector'] > 1.0
    # one row of one stored reflector dropped
    V2 = V.copy()
    row = 4 + int(np.argmax(np.abs(V[3, 4:])))
    V2[3, row] = 0.0
    r = mutated(hh=q.pack(V2, tau, N))
    rep['row %d of v_3 dropped' % row] = _rejected(r)
    assert r['reflector'] > 1.0 and r['RPt'] > 1.0
    # a nonzero above row k in the packed store
    V2 = V.copy()
    V2[5, 2] = 1e-300
    r = mutated(hh=q.pack(V2, tau, N))
    rep['v_5 nonzero on row 2'] = _rejected(r)
    assert r['layout'] > 1.0
    # y left untransformed
    r = mutated(y1=np.array(y))
    rep['y1 = y'] = _rejected(r)
    assert r['y1'] > 1.0
    # Q^T where Q belongs
    r = mutated(C=q.emulate_back(good['hh'], N, C, transpose=True), V=q.emulate_back(good['hh'], N, Vs.T, transpose=True).T)
    rep['Q^T applied in the back-transformation'] = _rejected(r)
    assert r['Qc'] > 1.0 and r['QV'] > 1.0
    # the last reflector skipped in back_vec
    r = mutated(C=q.emulate_back(good['hh'], N, C, skip_last=True))
    rep['last reflector skipped in back_vec'] = _rejected(r)
    assert r['Qc'] > 1.0 and r['vec_vs_mat'] > 1.0
    # reflector sets of neighbouring systems overlapping by one double
    P = q.hh_doubles(N)
    buf = np.zeros(3 * P)
    for i in range(3):
        buf[i * (P - 1):i * (P - 1) + P] = good['hh']
    sets = q.split_sets(buf, 3, N, P - 1)
    bad = q.layout_problems(sets[0], N)
    rep['sets overlapping by one double'] = bad
    assert bad and q.layout_problems(sets[2], N) == []
    for k, v in rep.items():
        print('%-44s rejected by %s' % (k, v))
