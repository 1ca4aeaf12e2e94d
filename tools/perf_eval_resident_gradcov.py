"""Rate of the gradient-covariance maps on a resident grid (vi_eval_resident_gradcov_f64), kernel time per timestep of three
routes on the same gradient basis:

  k2c   K2c (csrc/vi_eval_resident.hip): the six entries of the 3 x 3 covariance of the gradient per point;
  k2e   K2e on the same dG (vi_eval_resident_err_f64 with 3Q columns, ResidentGrid.evaluate_gradient_errors): the three
        diagonal entries only - the floor, the same matrix-core work without the cross terms;
  blas  the library path of the same call as k2c (VINTERP_EVAL_RESIDENT=blas: per chunk of points the three components
        point-major, per timestep the library's product with dC_t and nine row dots).

Workload: the default order (N = 144, the config of tests/golden/fit_default.npz), an n^3 grid (default 128^3) with the hull
mask of that fixture, model frame, T covariances (default 16: the fixture's covariances times positive scales).  The switch is
read once per process, so every route runs in a fresh child process; the children alternate, `--reps` of each, every child
warms up before it times `--calls` calls (device time of the call's kernels from the context's event pair, and host time of
the call ending in a synchronise).

    python tools/perf_eval_resident_gradcov.py [--n 128] [--T 16] [--reps 3] [--calls 3] [--out FILE]
    python tools/perf_eval_resident_gradcov.py --child k2c [--n 128] [--T 16] [--calls 3]      # one route, this process
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PEAK_TF = 78.6                  # fp64 matrix peak of the MI355X
ROUTES = ('k2c', 'k2e', 'blas')


def child(route, n, T, calls):
    from volumetricinterp_amd import _lib, synth
    from volumetricinterp_amd.estimate import Estimate
    f = np.load(os.path.join(REPO, 'tests', 'golden', 'fit_default.npz'))
    es = Estimate.from_arrays(f['Coeffs'], f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))
    N = es.model.nbasis
    rng = np.random.default_rng(0)
    dC = f['Covariance'][np.arange(T) % len(f['Covariance'])] * rng.uniform(0.5, 2., T)[:, None, None]
    grid = synth.query_grid(n)
    ctx = es.model.ctx
    assert (os.environ.get('VINTERP_EVAL_RESIDENT') == 'blas') == (route == 'blas')
    with es.resident_grid(*grid, gradient='model') as g:
        Q = g.Q
        planes = 3 if route == 'k2e' else 6
        dD, dO = ctx.to_device(dC), ctx.empty((T, planes, Q))
        ctx.eval_timing(True)
        h = es.model.handle()

        def call():
            if route == 'k2e':
                _lib.check(_lib.lib.vi_eval_resident_err_f64(h, 3 * Q, T, g.dG.ptr, dD.ptr, dO.ptr), 'vi_eval_resident_err_f64')
            else:
                _lib.check(_lib.lib.vi_eval_resident_gradcov_f64(h, Q, T, g.dG.ptr, dD.ptr, dO.ptr),
                           'vi_eval_resident_gradcov_f64')
            ctx.sync()

        call()                                           # warm-up: code objects, the library's kernel choice, workspace
        kms, wms = [], []
        for _ in range(calls):
            t0 = time.perf_counter()
            call()
            wms.append((time.perf_counter() - t0) * 1e3)
            kms.append(ctx.eval_kernel_ms())
        out = dO.download()
        dD.free()
        dO.free()
    if route == 'k2e':
        out = out ** 2                                   # the diagonal of the other two routes
    inside = float(np.isfinite(out[0, 0]).mean())
    return dict(path=route, n=n, Q=Q, N=N, T=T, kernel_ms=kms, wall_ms=wms, inside=inside,
                checksum=float(np.nansum(out[::max(1, T // 4), :3])))


def report(r):
    N, Q, T = r['N'], r['Q'], r['T']
    Np = 16 * ((N + 15) // 16)
    ms = min(r['kernel_ms'])
    # matrix-core flop issued: K2c and K2e on 3Q columns the blocks of the upper triangle for three vectors; the library the
    # full product for three vectors
    issued = (3. * Np * (Np + 16) if r['path'] != 'blas' else 3. * 2. * N * N) * Q * T
    tf = issued / ms / 1e9
    return ('%-4s %d^3 x T %3d: kernel %9.3f ms (median %9.3f, wall %9.3f) = %7.4f ms/timestep, %.3e point-timesteps/s, '
            '%5.1f TF/s MFMA-issued = %4.1f %% of the %.1f TF fp64 matrix peak'
            % (r['path'], r['n'], T, ms, float(np.median(r['kernel_ms'])), min(r['wall_ms']), ms / T, Q * T / (ms * 1e-3), tf,
               100. * tf / PEAK_TF, PEAK_TF))


def run_child(route, n, T, calls):
    env = dict(os.environ)
    env.pop('VINTERP_EVAL_RESIDENT', None)
    env.pop('VINTERP_K2C_GROUPS', None)
    if route == 'blas':
        env['VINTERP_EVAL_RESIDENT'] = 'blas'
    p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', route, '--n', str(n), '--T', str(T), '--calls',
                        str(calls)], env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit('child (%s) failed with status %d' % (route, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', choices=ROUTES)
    ap.add_argument('--n', type=int, default=128)
    ap.add_argument('--T', type=int, default=16)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.n, a.T, a.calls)))
        return
    lines, res = [], {p: [] for p in ROUTES}

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                        # written as it goes: a run cut short keeps what it measured
            with open(a.out, 'w') as fh:
                fh.write('\n'.join(lines) + '\n')

    emit('vi_eval_resident_gradcov_f64, N = 144, %d^3 grid with the hull mask, model frame, T = %d; %d alternating children per '
         'route, %d timed calls each after a warm-up' % (a.n, a.T, a.reps, a.calls))
    for rep in range(a.reps):
        for route in ROUTES:
            r = run_child(route, a.n, a.T, a.calls)
            res[route].append(r)
            emit('rep %d %s' % (rep, report(r)))
    best = {p: min(res[p], key=lambda r: min(r['kernel_ms'])) for p in res}
    emit('best of each: ' + ' | '.join(report(best[p]) for p in ROUTES))
    ms = {p: min(best[p]['kernel_ms']) / a.T for p in ROUTES}
    emit('kernel time per timestep: (a) K2c %.4f ms, (b) K2e on the same dG %.4f ms, (c) library %.4f ms; K2c / K2e %.3f, K2c / '
         'library %.3f (library %.2fx the time of K2c); inside the hull %.1f %% of the points; checksums of the diagonal k2c '
         '%.9e k2e %.9e library %.9e' % (ms['k2c'], ms['k2e'], ms['blas'], ms['k2c'] / ms['k2e'], ms['k2c'] / ms['blas'],
                                         ms['blas'] / ms['k2c'], 100. * best['k2c']['inside'], best['k2c']['checksum'],
                                         best['k2e']['checksum'], best['blas']['checksum']))


if __name__ == '__main__':
    main()
