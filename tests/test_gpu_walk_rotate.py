"""K_walk (csrc/vi_walk.hip): the rotated systems of the bracket walk in shared bases, formed in one fp64-MFMA kernel instead
of two batched rocBLAS products and two element-wise kernels - through vi_basis_solve_f64 and the engine only.

  * same answers as the library chain (VINTERP_WALK_FORM=blas, the path before K_walk) and as cold solves, at N = 144 (operands
    in registers and LDS), N = 180 (not a multiple of 16; operands fetched at every use), N = 75 (not a multiple of 16, 19
    matches: the v1 K3 kernel) and N = 32;
  * a system's bits do not depend on the batch, on its place in it or on the chunk;
  * nothing downstream of the walk moves: a fit of 300 records is bit-identical with either way of forming.

The switch is read once per process, so the other setting runs in a child process: this file is also that child's script
(`python test_gpu_walk_rotate.py <what> <out.npz>`).

Forming on its own (X scl against V AWA V^T + alpha D2 element by element, at every instantiation of the kernel, through the
stage-test entry vi_walk_form_f64) is tested in tests/test_gpu_walk_geometry.py."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden
from test_gpu_configs import _engine, CFG144, EPS

pytestmark = pytest.mark.gpu

CFGS = {
    'n144': CFG144,
    'n180': CFG144.replace('MAXK = 4', 'MAXK = 5'),
    'n75': CFG144.replace('MAXK = 4', 'MAXK = 3').replace('MAXL = 6', 'MAXL = 5'),
    'n32': CFG144.replace('MAXK = 4', 'MAXK = 8').replace('MAXL = 6', 'MAXL = 2'),
}
ORDER = {'n144': 144, 'n180': 180, 'n75': 75, 'n32': 32}
KS = np.array([0., -10., -22., -26., -30., -40.])


def _setup(name):
    from volumetricinterp_amd import synth
    from volumetricinterp_amd.models.sphharmlag import Model
    cfg = CFGS[name]
    R = load_golden('regmat')['default_curvature'] if name == 'n144' else Model(io.StringIO(cfg)).eval_reg_matricies['curvature']()
    m, ctx, eng, A, _ = _engine(cfg, synth.GEOM_C2, R=R)
    assert A.shape[1] == ORDER[name]
    value, error = synth.synth_records(A, 12, seed0=1000)
    W = error**-2.
    eng.load_records(W, value)
    AWA, y = eng.normal_equations()
    return dict(m=m, ctx=ctx, eng=eng, A=A, W=W, b=value, AWA=AWA, y=y, R=np.asarray(R, dtype=float), N=A.shape[1])


def _bases(s):
    """The set-up of test_basis_solve_equals_cold_solve_in_any_basis: reference = mean of the last 6 records, its eigenbases
    at six decades; device arrays of records 0..3 (+ the reference as record 4)."""
    from volumetricinterp_amd import _lib
    ctx, N = s['ctx'], s['N']
    K = len(KS)
    ref = np.mean(s['AWA'][6:], axis=0)
    d = dict(dAWA=ctx.to_device(np.concatenate([s['AWA'][:4], ref[None]])),
             dy=ctx.to_device(np.concatenate([s['y'][:4], s['y'][:1]])), dR=ctx.to_device(s['R']),
             dV=ctx.empty((K, N, N)), dD1=ctx.empty((K, N, N)), dD2=ctx.empty((K, N, N)), dyt=ctx.empty((K, N)))
    keep = [ctx.to_device(np.full(K, 4, np.int32)), ctx.to_device(10.**KS), ctx.empty((K, N)), ctx.empty((K,), np.int32)]
    _lib.check(_lib.lib.vi_warm_prepare_f64(ctx.handle, K, N, d['dAWA'].ptr, keep[0].ptr, keep[1].ptr, d['dR'].ptr, d['dy'].ptr,
                                            EPS, keep[2].ptr, keep[3].ptr, d['dV'].ptr, d['dD1'].ptr, d['dD2'].ptr,
                                            d['dyt'].ptr), 'prepare')
    return d


def _basis_solve(s, d, rec, bas, al, dV=None, dD2=None):
    from volumetricinterp_amd import _lib
    ctx, N = s['ctx'], s['N']
    B = len(rec)
    dC, drk, dsw = ctx.empty((B, N)), ctx.empty((B,), np.int32), ctx.empty((B,), np.int32)
    drec, dbas, dal = ctx.to_device(np.asarray(rec, np.int32)), ctx.to_device(np.asarray(bas, np.int32)), ctx.to_device(np.asarray(al, float))
    _lib.check(_lib.lib.vi_basis_solve_f64(ctx.handle, B, N, d['dAWA'].ptr, d['dy'].ptr, drec.ptr, dbas.ptr, dal.ptr,
                                           (dV or d['dV']).ptr, (dD2 or d['dD2']).ptr, EPS, dC.ptr, drk.ptr, dsw.ptr), 'basis_solve')
    return dC.download(), drk.download(), dsw.download()


def _triples24():
    K = len(KS)
    return np.repeat(np.arange(4, dtype=np.int32), K), np.tile(np.arange(K, dtype=np.int32), 4), np.tile(10.**KS, 4)


def _triples300():
    """300 (record, basis, alpha) triples: every combination of 4 records x 6 bases, alpha up to half a decade off the
    basis's own; the probe triple sits first, in the middle and last."""
    rng = np.random.default_rng(11)
    rec = rng.integers(0, 4, 300).astype(np.int32)
    bas = rng.integers(0, len(KS), 300).astype(np.int32)
    al = 10.**(KS[bas] + rng.uniform(-0.5, 0.5, 300))
    for i in (0, 150, 299):
        rec[i], bas[i], al[i] = PROBE
    return rec, bas, al


PROBE = (2, 3, 10.**-26.3)


def _chi2(s, C, t):
    return float(np.sum((s['A'] @ C - s['b'][t])**2 * s['W'][t]))


# ---- the child process ---------------------------------------------------------------------------------------------------
def _child_walk(name, out):
    s = _setup(name)
    d = _bases(s)
    C, rk, sw = _basis_solve(s, d, *_triples24())
    np.savez(out, C=C, rank=rk, sweeps=sw)


def _child_walk300(out):
    s = _setup('n144')
    d = _bases(s)
    C, rk, sw = _basis_solve(s, d, *_triples300())
    np.savez(out, C=C, rank=rk, sweeps=sw)


def _fit300():
    from volumetricinterp_amd import synth
    m, ctx, eng, A, _ = _engine(CFG144, synth.GEOM_C2)
    P, T = A.shape[0], 300
    value, error = synth.synth_records(A, T, seed0=9000)
    res = eng.fit(error**-2., value, [P] * T, calccov=True)
    inf = res['search']['curvature']
    out = dict(Coeffs=res['Coeffs'], chi_sq=res['chi_sq'], Covariance=res['Covariance'], ranks=res['ranks'],
               alpha=np.array([p['curvature'] for p in res['reg_params']], dtype=float),
               outcomes=np.array(inf['outcomes']),
               iterations=np.array([-1 if i.get('iterations') is None else i.get('iterations') for i in inf['info']]),
               polished_cold=np.array(sorted(inf.get('polished_cold', [])), dtype=np.int64),
               redone_cold=np.array(sorted(inf.get('redone_cold', [])), dtype=np.int64),
               shared_solves=np.array(eng.stats.get('shared_solves', 0)))
    eng.close()
    return out


def _child_fit(out):
    np.savez(out, **_fit300())


def _run_child(what, out, **env):
    e = dict(os.environ)
    e.update(env)
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), what, str(out)]
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (what, env, r.stdout[-2000:], r.stderr[-4000:])
    return np.load(str(out), allow_pickle=False)


# ---- tests -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['n144', 'n180', 'n75', 'n32'])
def test_walk_solutions_match_the_library_chain_and_the_cold_solve(name, tmp_path, capsys):
    """chi^2 of the walk solution: within 2e-4 of the cold solve's (the bound of test_basis_solve_equals_cold_solve_in_any_
    basis), and within 2e-4 of what the rocBLAS chain gives for the same call - 25 times under alpha_search.WALK_SIGN_MARGIN
    (5e-3), the only thing the walk's accuracy has to respect.  Both ways of forming carry N eps of rounding in different
    orders, which eigenvalues next to the truncation cut amplify (that is where the deviation from the cold solve comes
    from as well).  Measured on MI355X, worst of the 24 systems against the chain / against the cold solve: N = 144
    2.0e-6 / 1.7e-5, N = 180 4.3e-8 / 3.3e-5, N = 75 0 / 4.0e-7, N = 32 1.2e-14 / 2.7e-9 (the gate: 100 x the worst); the
    sweep counts are those of the chain system by system."""
    from volumetricinterp_amd import _lib
    from volumetricinterp_amd.alpha_search import WALK_SIGN_MARGIN
    assert os.environ.get('VINTERP_WALK_FORM') != 'blas'
    s = _setup(name)
    ctx, N = s['ctx'], s['N']
    d = _bases(s)
    V = d['dV'].download()
    for k in range(len(KS)):
        assert np.max(np.abs(V[k] @ V[k].T - np.eye(N))) <= 1e-13
    rec, bas, al = _triples24()
    Cs, rk, sw = _basis_solve(s, d, rec, bas, al)
    B = len(rec)
    dX = ctx.to_device(np.stack([s['AWA'][r] + a * s['R'] for r, a in zip(rec, al)]))
    dCc, drc = ctx.empty((B, N)), ctx.empty((B,), np.int32)
    drec = ctx.to_device(rec)
    _lib.check(_lib.lib.vi_solve_trunc_f64(ctx.handle, B, N, dX.ptr, d['dy'].ptr, drec.ptr, EPS, dCc.ptr, drc.ptr, N * EPS, None), 'cold')
    Cc = dCc.download()
    lib = _run_child('walk-' + name, tmp_path / 'blas.npz', VINTERP_WALK_FORM='blas')
    worst_cold = worst_blas = 0.
    for i in range(B):
        c_s, c_c, c_b = _chi2(s, Cs[i], rec[i]), _chi2(s, Cc[i], rec[i]), _chi2(s, lib['C'][i], rec[i])
        worst_cold = max(worst_cold, abs(c_s - c_c) / c_c)
        worst_blas = max(worst_blas, abs(c_s - c_b) / c_b)
    with capsys.disabled():
        print('\n[walk_rotate %s] worst |dchi2|/chi2: vs cold %.3e, vs rocBLAS chain %.3e; sweeps %s (chain %s)'
              % (name, worst_cold, worst_blas, np.bincount(sw).tolist(), np.bincount(lib['sweeps']).tolist()))
    assert np.all(np.isfinite(Cs))
    assert worst_cold <= 2e-4, worst_cold
    assert worst_blas <= 2e-4 < WALK_SIGN_MARGIN, worst_blas      # measured 2.0e-6 at the worst (N = 144)
    assert int(np.max(sw)) <= int(_lib.lib.vi_max_sweeps())                 # every system converged under the cap
    if name == 'n144':
        # a random orthogonal basis: same answer (D2 must then be formed for it)
        import scipy.linalg
        rng = np.random.default_rng(3)
        Q, _ = np.linalg.qr(rng.standard_normal((N, N)))
        dVr = ctx.to_device(np.ascontiguousarray(Q.T)[None])               # library layout: row k = basis vector k
        dD2r = ctx.to_device((Q.T @ s['R'] @ Q)[None])
        C1 = _basis_solve(s, d, [0], [0], [1e-12], dV=dVr, dD2=dD2r)[0]
        Cl = scipy.linalg.lstsq(s['AWA'][0] + 1e-12 * s['R'], s['y'][0])[0]
        assert abs(_chi2(s, C1[0], 0) / _chi2(s, Cl, 0) - 1.) <= 1e-6


def test_a_walk_system_does_not_depend_on_the_batch(tmp_path):
    """The same (record, basis, alpha) triple alone, first, in the middle and last in a batch of 300, and with the batch cut
    into two chunks (256 + 44, VINTERP_WALK_CHUNK): C, rank and sweep count identical bit for bit - and so is every other
    system of the batch between the one-chunk and the two-chunk call."""
    s = _setup('n144')
    d = _bases(s)
    rec, bas, al = _triples300()
    C, rk, sw = _basis_solve(s, d, rec, bas, al)
    C1, rk1, sw1 = _basis_solve(s, d, [PROBE[0]], [PROBE[1]], [PROBE[2]])
    assert np.all(np.isfinite(C1))
    for i in (0, 150, 299):
        assert np.array_equal(C[i], C1[0]) and rk[i] == rk1[0] and sw[i] == sw1[0], i
    two = _run_child('walk300', tmp_path / 'two.npz', VINTERP_WALK_CHUNK='256')
    assert np.array_equal(two['C'], C) and np.array_equal(two['rank'], rk) and np.array_equal(two['sweeps'], sw)


def test_fit_is_bit_identical_with_either_way_of_forming(tmp_path):
    """FitEngine.fit on 300 synthetic records of the bench geometry (N = 144, covariance on), as built and with VINTERP_
    WALK_FORM=blas, a process each: the walk's values only decide signs, and a value within WALK_SIGN_MARGIN of the target
    is asked for again from a cold solve, so coefficients, chi^2, alpha, ranks, covariances and the search bookkeeping must
    not move by a bit."""
    a = _run_child('fit', tmp_path / 'mfma.npz')
    b = _run_child('fit', tmp_path / 'blas.npz', VINTERP_WALK_FORM='blas')
    assert int(a['shared_solves']) > 0 and int(a['shared_solves']) == int(b['shared_solves'])
    for k in ('Coeffs', 'chi_sq', 'alpha', 'Covariance'):
        diff = np.flatnonzero(~np.all((a[k] == b[k]) | (np.isnan(a[k]) & np.isnan(b[k])), axis=tuple(range(1, a[k].ndim))))
        assert diff.size == 0, (k, diff[:10])
    for k in ('ranks', 'outcomes', 'iterations', 'polished_cold', 'redone_cold'):
        assert np.array_equal(a[k], b[k]), k
    assert np.sum(a['outcomes'] == 'root') > 0


if __name__ == '__main__':
    what, out = sys.argv[1], sys.argv[2]
    if what.startswith('walk-'):
        _child_walk(what[5:], out)
    elif what == 'walk300':
        _child_walk300(out)
    elif what == 'fit':
        _child_fit(out)
    else:
        raise SystemExit('unknown job %r' % what)
