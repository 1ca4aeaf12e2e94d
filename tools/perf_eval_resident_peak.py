"""Cost of the column maps of a resident grid (ResidentGrid.peak / integrate, vi_eval_resident_peak_f64) against the density
product they replace.

Workload: the default order (N = 144, the config of tests/golden/fit_default.npz), an n^3 grid with the hull mask of that
fixture, altitude last (L = n, M = n^2 columns), T timesteps of the fixture's coefficients.  Per path, in one process: a
warm-up call, then `--calls` calls; kernel time from the context's event pair (vi_eval_kernel_ms), wall time box to box
(host arrays in, host arrays out), medians.  The switches are read once per process, so the paths run in child processes:

  (a) volume   g.evaluate_coeffs, then np.nanmax / np.nanargmax on the host: what a user does without this call
  (b) twopass  g.evaluate_peaks under VINTERP_K2P=twopass: the density product into a device slab, then k_peak_columns
  (c) k2p      g.evaluate_peaks: K2p, the product with the reduction in place of the stores
  (d) integ    g.evaluate_integrals against np.nansum of (a)'s volume (the first call builds the reduced basis: timed apart)
  (e) k2r      vi_eval_resident_f64 alone on the same shape: the floor

    python tools/perf_eval_resident_peak.py [--n 128] [--T 64] [--calls 5] [--big] [--out FILE]
    python tools/perf_eval_resident_peak.py --child PATH [--n 128] [--T 64] [--calls 5]
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

PATHS = ('volume', 'twopass', 'k2p', 'integ', 'k2r')


def child(path, n, T, calls):
    from volumetricinterp_amd import _lib, synth
    from volumetricinterp_amd.estimate import Estimate
    f = np.load(os.path.join(REPO, 'tests', 'golden', 'fit_default.npz'))
    es = Estimate.from_arrays(f['Coeffs'], f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))
    N = es.model.nbasis
    rng = np.random.default_rng(0)
    base = np.nan_to_num(f['Coeffs'])
    C = base[np.arange(T) % len(base)] * rng.uniform(0.5, 2., T)[:, None]
    ctx = es.model.ctx
    res = dict(path=path, n=n, T=T, N=N, setup_ms=0.)
    with es.resident_grid(*synth.query_grid(n)) as g:
        Q, M = g.Q, g.Q // n
        ctx.eval_timing(True)
        if path == 'volume':
            out = _lib.pinned_empty((T, Q))

            def call():
                g.evaluate_coeffs(C, out=out)
                k = ctx.eval_kernel_ms()
                v = out.reshape(T, M, n)
                none = np.isnan(v).all(axis=2)
                val = np.nanmax(np.where(none[:, :, None], 0., v), axis=2)
                idx = np.nanargmax(np.where(none[:, :, None], 0., v), axis=2)
                return k, float(np.sum(np.where(none, 0., val))) + float(np.sum(np.where(none, 0, idx)))
        elif path in ('twopass', 'k2p'):
            o = (np.empty((T, M)), np.empty((T, M), np.int32))

            def call():
                val, idx = g.evaluate_peaks(C, out=o)
                return ctx.eval_kernel_ms(), float(np.nansum(val)) + float(np.sum(np.maximum(idx, 0)))
        elif path == 'integ':
            o = np.empty((T, M))
            t0 = time.perf_counter()
            g.evaluate_integrals(C[:1])
            res['setup_ms'] = (time.perf_counter() - t0) * 1e3             # k_reduce_basis, once per (axis, weights)

            def call():
                return ctx.eval_kernel_ms() if g.evaluate_integrals(C, out=o) is o else 0., float(np.nansum(o))
        else:
            dC, dO = ctx.to_device(C), ctx.empty((T, Q))
            h = es.model.handle()

            def call():
                _lib.check(_lib.lib.vi_eval_resident_f64(h, Q, T, g.dY.ptr, dC.ptr, dO.ptr), 'vi_eval_resident_f64')
                ctx.sync()
                return ctx.eval_kernel_ms(), 0.
        call()                                           # warm-up: code objects, allocations
        kms, wms = [], []
        for _ in range(calls):
            t0 = time.perf_counter()
            k, chk = call()
            wms.append((time.perf_counter() - t0) * 1e3)
            kms.append(k)
        res.update(Q=Q, kernel_ms=kms, wall_ms=wms, checksum=chk)
    return res


def report(r):
    T = r['T']
    k, w = float(np.median(r['kernel_ms'])), float(np.median(r['wall_ms']))
    return ('%-7s %d^3 x T %3d: kernel %9.3f ms = %8.4f ms/timestep, wall %10.3f ms = %9.4f ms/timestep%s'
            % (r['path'], r['n'], T, k, k / T, w, w / T, ', set-up %.1f ms' % r['setup_ms'] if r['setup_ms'] else ''))


def run_child(path, n, T, calls):
    env = dict(os.environ)
    env.pop('VINTERP_K2P', None)
    if path == 'twopass':
        env['VINTERP_K2P'] = 'twopass'
    p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', path, '--n', str(n), '--T', str(T), '--calls',
                        str(calls)], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit('child (%s) failed with status %d' % (path, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', choices=PATHS)
    ap.add_argument('--n', type=int, default=128)
    ap.add_argument('--T', type=int, default=64)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--big', action='store_true', help='also 256^3 x 512 timesteps (basis 19 GB; the volume path: 64)')
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.n, a.T, a.calls)))
        return
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit('column maps of a resident grid, N = 144, hull mask, altitude last; medians of %d calls after a warm-up' % a.calls)
    sizes = [(a.n, a.T, a.calls)] + ([(256, 512, 3)] if a.big else [])
    for n, T, calls in sizes:
        res = {}
        for path in PATHS:
            Tp = min(T, 64) if path == 'volume' else T          # the host reduction of 512 volumes of 256^3 takes minutes
            res[path] = run_child(path, n, Tp, calls)
            emit(report(res[path]))
        k = {p: float(np.median(res[p]['kernel_ms'])) / res[p]['T'] for p in PATHS}
        w = {p: float(np.median(res[p]['wall_ms'])) / res[p]['T'] for p in PATHS}
        emit('%d^3 kernel time per timestep: K2p %.3f x K2r, two-pass %.3f x K2r, K2p / two-pass %.3f; integrals %.4f x K2r'
             % (n, k['k2p'] / k['k2r'], k['twopass'] / k['k2r'], k['k2p'] / k['twopass'], k['integ'] / k['k2r']))
        emit('%d^3 wall time per timestep: volume + host reduction %.3f ms, two-pass %.3f ms, K2p %.3f ms (%.0f x), integrals '
             '%.3f ms' % (n, w['volume'], w['twopass'], w['k2p'], w['volume'] / w['k2p'], w['integ']))
        if res['k2p']['T'] == res['twopass']['T']:
            emit('checksums: K2p %.12e two-pass %.12e%s' % (res['k2p']['checksum'], res['twopass']['checksum'],
                                                           '' if res['volume']['T'] != T else ' volume %.12e'
                                                           % res['volume']['checksum']))
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
