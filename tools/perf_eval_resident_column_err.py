"""Cost of the standard errors of the column maps of a resident grid (ResidentGrid.peak_error / integrate_error) against the
error volume they replace.

Workload: the default order (N = 144, the config of tests/golden/fit_default.npz), an n^3 grid with the hull mask of that
fixture, altitude last (L = n, M = n^2 columns), T covariances of the fixture.  One process (no switch is involved): per path
a warm-up call, then `--calls` calls; kernel time from the context's event pair (vi_eval_kernel_ms), medians.

  (a) k2eg    vi_eval_resident_err_at_f64 at the index map of evaluate_peaks: K2e's form at M gathered points per timestep
  (b) volume  vi_eval_resident_err_f64 on the whole grid, K2e on M L points per timestep: the only route before K2eg - and, timed
              apart, what it needs besides: the (T, Q) download and np.take_along_axis on the host
  (c) integ   vi_eval_resident_err_f64 on the reduced basis of evaluate_integrals: K2e on M columns (integrate_error)
and the wall time, host arrays in and out, of g.evaluate_peak_errors against g.evaluate_peaks + route (b).

    python tools/perf_eval_resident_column_err.py [--n 128] [--T 64] [--calls 5] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def med(x):
    x = np.asarray(x)
    return '%9.3f ms (%.3f - %.3f)' % (np.median(x), x.min(), x.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=128)
    ap.add_argument('--T', type=int, default=64)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--out')
    a = ap.parse_args()
    from volumetricinterp_amd import _lib, synth
    from volumetricinterp_amd.estimate import Estimate, column_points
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    n, T = a.n, a.T
    f = np.load(os.path.join(REPO, 'tests', 'golden', 'fit_default.npz'))
    es = Estimate.from_arrays(f['Coeffs'], f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))
    N = es.model.nbasis
    rng = np.random.default_rng(0)
    k = np.arange(T) % len(f['Coeffs'])
    C = np.nan_to_num(f['Coeffs'])[k] * rng.uniform(0.5, 2., T)[:, None]
    dC = f['Covariance'][k] * rng.uniform(0.5, 2., T)[:, None, None]
    ctx, h = es.model.ctx, es.model.handle()
    emit('standard errors of the column maps of a resident grid, N = %d, %d^3 grid with the hull mask, altitude last '
         '(M = %d columns of L = %d), T = %d covariances; medians (min - max) of %d calls after a warm-up' % (N, n, n * n, n, T, a.calls))
    with es.resident_grid(*synth.query_grid(n)) as g:
        Q, M = g.Q, g.Q // n
        val, idx = g.evaluate_peaks(C)
        emit('columns with a peak: %d of %d per timestep' % ((idx[0] >= 0).sum(), M))
        ctx.eval_timing(True)
        with ctx.scope() as dev:
            dD, dI = dev.up(dC), dev.up(idx, np.int32)
            dE, dV = dev.empty((T, M)), dev.empty((T, Q))
            host = _lib.pinned_empty((T, Q))
            g.evaluate_integrals(C[:1])                  # builds the reduced basis of (altitude, ones)
            dYr = next(iter(g._reduced.values()))

            def k2eg():
                _lib.check(_lib.lib.vi_eval_resident_err_at_f64(h, M, n, 1, T, g.dY.ptr, dD.ptr, dI.ptr, dE.ptr),
                           'vi_eval_resident_err_at_f64')

            def volume():
                _lib.check(_lib.lib.vi_eval_resident_err_f64(h, Q, T, g.dY.ptr, dD.ptr, dV.ptr), 'vi_eval_resident_err_f64')

            def integ():
                _lib.check(_lib.lib.vi_eval_resident_err_f64(h, M, T, dYr.ptr, dD.ptr, dE.ptr), 'vi_eval_resident_err_f64')
            kms = {}
            for name, call in (('k2eg', k2eg), ('volume', volume), ('integ', integ)):
                call()
                ctx.sync()
                ms = []
                for _ in range(a.calls):
                    call()
                    ctx.sync()
                    ms.append(ctx.eval_kernel_ms())
                kms[name] = float(np.median(ms))
                emit('%-7s kernel %s = %8.4f ms/timestep' % (name, med(ms), kms[name] / T))
            k2eg()
            ctx.sync()
            at = dE.download()
            # what route (b) needs besides its kernel: the volume on the host and one value per column picked from it
            dl, pick = [], []
            q = np.maximum(column_points((n, n, n), 2, idx), 0)
            for _ in range(a.calls):
                t0 = time.perf_counter()
                dV.download(out=host)
                t1 = time.perf_counter()
                sel = np.take_along_axis(host, q, 1)
                t2 = time.perf_counter()
                dl.append((t1 - t0) * 1e3)
                pick.append((t2 - t1) * 1e3)
            sel[idx < 0] = np.nan
            emit('volume  download of (T, Q) to pinned memory %s, host gather %s' % (med(dl), med(pick)))
            emit('K2eg / K2e on the volume: %.4f of the kernel time (%.1f x less), for 1 / %d of the points; with the download '
                 'and the gather the volume route takes %.1f x K2eg' % (kms['k2eg'] / kms['volume'], kms['volume'] / kms['k2eg'], n,
                                                                       (kms['volume'] + np.median(dl) + np.median(pick))
                                                                       / kms['k2eg']))
            emit('K2eg per gathered point %.2f ns, K2e per point of the volume %.3f ns, K2e on the reduced basis per column %.3f ns'
                 % (kms['k2eg'] * 1e6 / (T * M), kms['volume'] * 1e6 / (T * Q), kms['integ'] * 1e6 / (T * M)))
            emit('bits: the gathered errors equal the picked ones: %s' % np.array_equal(at, sel, equal_nan=True))
        ctx.eval_timing(False)
        # box to box
        for name, call in (('evaluate_peak_errors', lambda: g.evaluate_peak_errors(C, dC)),
                           ('evaluate_peaks + evaluate_errors + host gather',
                            lambda: np.take_along_axis(g.evaluate_errors(dC), np.maximum(column_points((n, n, n), 2,
                                                                                                     g.evaluate_peaks(C)[1]), 0), 1)),
                           ('evaluate_integral_errors', lambda: g.evaluate_integral_errors(dC))):
            call()
            ws = []
            for _ in range(max(1, a.calls // 2)):
                t0 = time.perf_counter()
                call()
                ws.append((time.perf_counter() - t0) * 1e3)
            emit('wall, host arrays in and out: %-48s %s' % (name, med(ws)))
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
