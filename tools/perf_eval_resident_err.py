"""Rate of the standard-error maps on a resident grid (vi_eval_resident_err_f64): K2e (csrc/vi_eval_resident.hip) against the
library path (VINTERP_EVAL_RESIDENT=blas: per timestep the library's product of the point-major basis with dC_t, then a row
dot, as Estimate.error computes one timestep).

Workload: the default order (N = 144, the config of tests/golden/fit_default.npz), an n^3 grid (default 128^3) with the hull
mask of that fixture, T covariances (default 64: the fixture's covariances times positive scales).  The switch is read once
per process, so each path runs in a fresh child process; the children alternate, `--reps` of each, every child warms up
before it times `--calls` calls (device time of the call's kernels from the context's event pair, and host time of the call
ending in a synchronise).  `--big` adds one pair at 256^3 x 16 timesteps (basis 19 GB).

    python tools/perf_eval_resident_err.py [--n 128] [--T 64] [--reps 3] [--calls 3] [--big] [--out FILE]
    python tools/perf_eval_resident_err.py --child [--n 128] [--T 64] [--calls 3]      # one path, this process (profiling)
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


def child(n, T, calls):
    from volumetricinterp_amd import _lib, synth
    from volumetricinterp_amd.estimate import Estimate
    f = np.load(os.path.join(REPO, 'tests', 'golden', 'fit_default.npz'))
    es = Estimate.from_arrays(f['Coeffs'], f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))
    N = es.model.nbasis
    rng = np.random.default_rng(0)
    dC = f['Covariance'][np.arange(T) % len(f['Covariance'])] * rng.uniform(0.5, 2., T)[:, None, None]
    grid = synth.query_grid(n)
    ctx = es.model.ctx
    with es.resident_grid(*grid) as g:
        Q = g.Q
        dD, dO = ctx.to_device(dC), ctx.empty((T, Q))
        ctx.eval_timing(True)
        h = es.model.handle()

        def call():
            _lib.check(_lib.lib.vi_eval_resident_err_f64(h, Q, T, g.dY.ptr, dD.ptr, dO.ptr), 'vi_eval_resident_err_f64')
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
    inside = float(np.isfinite(out[0]).mean())
    return dict(path=os.environ.get('VINTERP_EVAL_RESIDENT', 'k2e') or 'k2e', n=n, Q=Q, N=N, T=T, kernel_ms=kms, wall_ms=wms,
                inside=inside, checksum=float(np.nansum(out[::max(1, T // 4)])))


def report(r):
    N, Q, T = r['N'], r['Q'], r['T']
    Np = 16 * ((N + 15) // 16)
    ms = min(r['kernel_ms'])
    full = 2. * N * N * Q * T                            # the definition's 2 N^2 per point-timestep (plus 2N, not counted)
    issued = Np * (Np + 16) * Q * T if r['path'] == 'k2e' else full     # K2e: the blocks of the upper triangle
    tf_full, tf_issued = full / ms / 1e9, issued / ms / 1e9
    return ('%-4s %d^3 x T %3d: kernel %9.3f ms (median %9.3f, wall %9.3f) = %7.4f ms/timestep, %.3e point-timesteps/s, '
            '%5.1f TF/s full-form 2N^2Q, %5.1f TF/s MFMA-issued = %4.1f %% of the %.1f TF fp64 matrix peak'
            % (r['path'], r['n'], T, ms, float(np.median(r['kernel_ms'])), min(r['wall_ms']), ms / T, Q * T / (ms * 1e-3),
               tf_full, tf_issued, 100. * tf_issued / PEAK_TF, PEAK_TF))


def run_child(path, n, T, calls):
    env = dict(os.environ)
    env.pop('VINTERP_EVAL_RESIDENT', None)
    if path == 'blas':
        env['VINTERP_EVAL_RESIDENT'] = 'blas'
    p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--n', str(n), '--T', str(T), '--calls',
                        str(calls)], env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit('child (%s) failed with status %d' % (path, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--n', type=int, default=128)
    ap.add_argument('--T', type=int, default=64)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--big', action='store_true')
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.n, a.T, a.calls)))
        return
    lines, res = [], {'k2e': [], 'blas': []}

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit('vi_eval_resident_err_f64, N = 144, %d^3 grid with the hull mask, T = %d; %d alternating children per path, %d timed '
         'calls each after a warm-up' % (a.n, a.T, a.reps, a.calls))
    for rep in range(a.reps):
        for path in ('k2e', 'blas'):
            r = run_child(path, a.n, a.T, a.calls)
            res[path].append(r)
            emit('rep %d %s' % (rep, report(r)))
    best = {p: min(res[p], key=lambda r: min(r['kernel_ms'])) for p in res}
    emit('best of each: ' + ' | '.join(report(best[p]) for p in ('k2e', 'blas')))
    emit('K2e / library kernel time: %.3f (library %.2fx the time of K2e); inside the hull %.1f %% of the points; '
         'checksums k2e %.9e library %.9e' % (min(best['k2e']['kernel_ms']) / min(best['blas']['kernel_ms']),
                                              min(best['blas']['kernel_ms']) / min(best['k2e']['kernel_ms']),
                                              100. * best['k2e']['inside'], best['k2e']['checksum'], best['blas']['checksum']))
    if a.big:
        for path in ('k2e', 'blas'):
            emit('big  ' + report(run_child(path, 256, 16, 1)))
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
