"""The load and the replay of the role-separated Jacobi kernel (csrc/vi_jacobi_v2_device.h: v2_load_rows, v2_replay_ahead) in
batches around the CU count, against known answers and against the two-barrier kernel.

k_jacobi_solve_v2 (N = 93 ... 152) loads a system row by row - 16-byte loads where a row starts on a 16-byte boundary (every
row for even N, every other system's even or odd rows for odd N), zeros for the padding - and replays the rotation log with
eight rounds of it in flight, whatever the number of rounds (fewer than eight, not a multiple of eight, none).  VINTERP_K3=v1
runs the two-barrier kernel (k_jacobi_solve<1>), whose load and replay are the element-wise and batched ones: same bits.  The
switch is read once per process, so each setting runs in a child process of its own.

Orders: 93 (first order of the kernel, Np = 96, odd: rows on and off the 16-byte boundary), 144 (the benchmarked one), 149
(padded to Np = 152, odd).  Batches, from the CU count of the device: 1, 2, CUs (one workgroup each), CUs + 1 (one CU takes a
second workgroup), 2 CUs + 3.

Systems come from test_gpu_solver_geometry.make_systems - X = Q diag(l) Q^T of known spectrum - four seeds of F1 (full rank,
|l| in [0.1, 1]), F2 (graded over six decades, a block of eigenvalues below the cut, exact zeros: many sweeps) and F4_cluster
(equal eigenvalues) interleaved, and one F4_diag (nothing to rotate: few or no rounds to replay): 13 systems, so that
neighbouring systems differ in sweep count and rank and the pattern does not repeat with the CU count.  System i of a batch is
number i mod 13 with a right-hand side of its own.

Per batch, in the order given and in reversed order:
  vi_solve_trunc_f64     C, rank           - against the construction at that module's gates (F1, F4: 1e-10, F2: 1e-7, rank exact)
  vi_eigvals_f64         eigenvalues, sweeps - eigenvalues to 1e-12 max|l| as there, every solve converged
  vi_decompose_f64       C, rank, nround and the rotation log (X = AWA[rec] + 0 R, y[rec]: both through the record index; cap
                         24 sweeps at every order, which ends some F2 solves of N = 149: that path is compared as well)
and (a) the gates above, (b) every array equal by bytes to the VINTERP_K3=v1 child, (c) every system's bytes equal in the
reversed batch - where a system lies in the batch and in memory does not show, (d) right-hand sides picked through a permuted
record list equal by bytes to the gathered ones (at N = 149 the kernel itself does the picking, below that the pre-conditioner).
The log is 4.4 MB per system and C is its replay on the right-hand side, so all of C is compared and of the log itself the
first nround rounds of a sample of each batch: the first four systems, the last twelve and eight in between.

(The same batches and assertions served a kernel with persistent workgroups, compared with this one through a switch of its
own; it was measured slower and is kept as tools/experiments/k3_persistent_workgroups.patch.)"""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (93, 144, 149)
POOL_FAMILIES = ('F1', 'F2', 'F4_cluster')
POOL_SEEDS = 4


def batch_sizes(ncu):
    return [1, 2, ncu, ncu + 1, 2 * ncu + 3]


def pool(N):
    """The 13 systems of order N, interleaved by family."""
    import test_gpu_solver_geometry as g
    per_seed = [{s['fam']: s for s in g.make_systems(N, seed)} for seed in range(POOL_SEEDS)]
    out = [per_seed[seed][fam] for seed in range(POOL_SEEDS) for fam in POOL_FAMILIES]
    out.append(per_seed[0]['F4_diag'])
    return out


def batch_rhs(N, B):
    return np.random.default_rng(7919 * N + B).standard_normal((B, N))


def log_sample(B):
    """Positions (in the given order) of the systems whose rotation logs are compared."""
    s = set(range(min(B, 4))) | set(range(max(0, B - 12), B)) | set(int(v) for v in np.linspace(0, B - 1, 8))
    return sorted(s)


def device_cus():
    """multiProcessorCount of the context's device, asked of the HIP runtime the library is linked to (a symbol lookup in the
    library's handle reaches its dependencies; 63 = hipDeviceAttributeMultiprocessorCount)."""
    from volumetricinterp_amd import _lib
    v = C.c_int(0)
    rc = _lib.lib.hipDeviceGetAttribute(C.byref(v), 63, _lib.default_device())
    assert rc == 0 and 8 <= v.value <= 4096, (rc, v.value)
    return v.value


def run_all(out_path):
    """Child process: every order, batch and direction; one npz."""
    import test_gpu_solver_geometry as g
    from volumetricinterp_amd import _lib, fitengine  # noqa: F401 (registers the fit signatures)
    ctx = _lib.get_context()
    ncu = device_cus()
    out = {'ncu': np.array(ncu)}
    for N in NS:
        P = pool(N)
        Xp = np.array([s['X'] for s in P])
        Yp = np.array([s['y'] for s in P])
        M = (N + 3) // 4
        logd = int(_lib.lib.vi_rotation_log_bytes(N)) // 8            # doubles per log record
        dAWA, dYp, dR = ctx.to_device(Xp), ctx.to_device(Yp), ctx.zeros((N, N))
        for B in batch_sizes(ncu):
            idx = np.arange(B) % len(P)
            Y = batch_rhs(N, B)
            for tag in ('f', 'r'):
                ii, yy = (idx, Y) if tag == 'f' else (idx[::-1], Y[::-1])
                k = '%d_%d_%s_' % (N, B, tag)
                X = np.ascontiguousarray(Xp[ii])
                out[k + 'C'], out[k + 'rank'], _ = g.solve(X, np.ascontiguousarray(yy))
                out[k + 'lam'], out[k + 'sweeps'] = g.eigvals(X)
                drec, dal = ctx.to_device(ii.astype(np.int32)), ctx.zeros((B,))
                dC, drk, dnr = ctx.empty((B, N)), ctx.empty((B,), np.int32), ctx.empty((B,), np.int32)
                dlog = ctx.empty((B * logd,))
                _lib.check(_lib.lib.vi_decompose_f64(ctx.handle, B, N, dAWA.ptr, drec.ptr, dal.ptr, dR.ptr, dYp.ptr, g.EPS,
                                                     dC.ptr, drk.ptr, dlog.ptr, dnr.ptr), 'vi_decompose_f64')
                nr = dnr.download()
                out[k + 'C2'], out[k + 'rank2'], out[k + 'nround'] = dC.download(), drk.download(), nr
                pos = log_sample(B) if tag == 'f' else [B - 1 - p for p in log_sample(B)]
                assert int(nr.max()) * 4 * M * 2 <= logd, (N, B, int(nr.max()))
                out[k + 'logcrc'] = np.array([zlib.crc32(dlog.download(int(nr[p]) * 4 * M * 2, offset=p * logd).tobytes())
                                              for p in pos], np.int64)
                for a in (drec, dal, dC, drk, dnr, dlog):
                    a.free()
            if N == 149 or B == 2 * ncu + 3:
                # (d) six right-hand sides, every system picking one through a permuted list
                recs = batch_rhs(N, 6)
                rec = (np.arange(B) * 5 + 2) % 6
                X = np.ascontiguousarray(Xp[idx])
                out['%d_%d_recC' % (N, B)], out['%d_%d_recrank' % (N, B)], _ = g.solve(X, recs, rec=rec.astype(np.int32))
                out['%d_%d_gatC' % (N, B)], out['%d_%d_gatrank' % (N, B)], _ = g.solve(X.copy(), np.ascontiguousarray(recs[rec]))
    np.savez(out_path, **out)


CHILD = '''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_k3_batches as t
t.run_all(sys.argv[1])
'''


def _child(tmp_path, name, env_set):
    script = tmp_path / 'child.py'
    script.write_text(CHILD % (REPO_ROOT, os.path.join(REPO_ROOT, 'tests')))
    env = dict(os.environ)
    for k in ('VINTERP_K3', 'VINTERP_QRPRE', 'VINTERP_EIG', 'VINTERP_MAX_SWEEPS', 'VINTERP_K3_MINM'):
        env.pop(k, None)
    env.update(env_set)
    o = str(tmp_path / ('%s.npz' % name))
    r = subprocess.run([sys.executable, str(script), o], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, '%s child (%s): exit %d\n%s' % (name, env_set, r.returncode, r.stderr[-3000:])
    return dict(np.load(o))


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """The two children, run once for the whole module: the role-separated kernel (the default) and the two-barrier kernel."""
    d = tmp_path_factory.mktemp('k3b')
    return _child(d, 'default', {}), _child(d, 'v1', {'VINTERP_K3': 'v1'})


def _cases(r):
    ncu = int(r['ncu'])
    return [(N, B) for N in NS for B in batch_sizes(ncu)]


def test_known_spectra(runs):
    """(a) C, rank and the eigenvalues of every system of every batch against the construction."""
    import test_gpu_solver_geometry as g
    p, _ = runs
    fails = []
    for N in NS:
        P = pool(N)
        for B in batch_sizes(int(p['ncu'])):
            k = '%d_%d_f_' % (N, B)
            Y = batch_rhs(N, B)
            worst = {}
            for i in range(B):
                s = P[i % len(P)]
                eC = g.rel(p[k + 'C'][i], s['H_ref'] @ Y[i])
                mx = np.max(np.abs(s['lam']))
                el = float(np.max(np.abs(np.sort(p[k + 'lam'][i]) - np.sort(s['lam'])))) / mx
                sw = int(p[k + 'sweeps'][i])
                worst[s['fam']] = max(worst.get(s['fam'], 0.0), eC)
                if not (eC <= g.GATE[s['fam']] and int(p[k + 'rank'][i]) == s['rank_ref'] and el <= 1e-12 and sw <= g.sweep_cap(N)):
                    fails.append('N %d B %d system %d (%s): rel C %.1e rank %d (ref %d) eig %.1e sweeps %d'
                                 % (N, B, i, s['fam'], eC, p[k + 'rank'][i], s['rank_ref'], el, sw))
            print('N %d B %d: worst rel C %s, sweeps %d .. %d' % (N, B, {f: '%.1e' % v for f, v in worst.items()},
                                                                 p[k + 'sweeps'].min(), p[k + 'sweeps'].max()))
    assert not fails, '\n'.join(fails[:40])


def test_bytes_equal_the_two_barrier_kernel(runs):
    """(b) C, rank, eigenvalues, sweeps, nround and the sampled rotation logs: the bytes of VINTERP_K3=v1."""
    p, q = runs
    assert int(p['ncu']) == int(q['ncu'])
    bad = [k for k in p if k != 'ncu' and not (p[k].dtype == q[k].dtype and p[k].tobytes() == q[k].tobytes())]
    assert not bad, bad
    assert sum(k.endswith('logcrc') for k in p) == 2 * len(_cases(p))


def test_bytes_do_not_depend_on_the_order_of_the_batch(runs):
    """(c) A system gives the same bytes in the reversed batch, in both kernels: its place in the batch - and with it the
    alignment of its rows at odd N - does not show.  The sweep counts of neighbours differ, or the test is idle."""
    for r in runs:
        for N, B in _cases(r):
            f, b = '%d_%d_f_' % (N, B), '%d_%d_r_' % (N, B)
            for k in ('C', 'rank', 'lam', 'sweeps', 'C2', 'rank2', 'nround'):
                assert r[f + k].tobytes() == r[b + k][::-1].tobytes(), (N, B, k)
            assert r[f + 'logcrc'].tobytes() == r[b + 'logcrc'].tobytes(), (N, B)      # (sampled by system, not by position)
            if B > 2:
                assert len(set(r[f + 'sweeps'][:13].tolist())) >= 3 and len(set(r[f + 'rank'][:13].tolist())) >= 2, (N, B)


def test_right_hand_sides_through_the_record_list(runs):
    """(d) y[rec[i]] picked on the device equals the gathered right-hand sides by bytes, and is the right one."""
    import test_gpu_solver_geometry as g
    p, _ = runs
    ncu = int(p['ncu'])
    seen = 0
    for N, B in _cases(p):
        if not (N == 149 or B == 2 * ncu + 3):
            continue
        k = '%d_%d_' % (N, B)
        assert p[k + 'recC'].tobytes() == p[k + 'gatC'].tobytes() and p[k + 'recrank'].tobytes() == p[k + 'gatrank'].tobytes(), (N, B)
        P, recs = pool(N), batch_rhs(N, 6)
        for i in range(B):
            s = P[i % len(P)]
            assert g.rel(p[k + 'recC'][i], s['H_ref'] @ recs[(i * 5 + 2) % 6]) <= g.GATE[s['fam']], (N, B, i)
        seen += 1
    assert seen == 7
