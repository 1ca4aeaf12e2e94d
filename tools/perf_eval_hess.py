"""Cost of the second derivatives next to the first: the Hessian of the fitted parameter at points (vi_eval_hess_f64) next to its
gradient (vi_eval_grad_f64), and the set-up of the Hessian basis of a resident grid (vi_eval_hess_basis_f64, N x 6 x Q) next to
that of the gradient basis (vi_eval_grad_basis_f64, N x 3 x Q), on the same points.  Both Hessian kernels walk the gradient's
chains once per point (k_hess_sph, csrc/vi_hess.hip), so the ratios are the numbers to look at: six sums against three, and
twice the stores.

Workload: the default order (N = 144, the config of tests/golden/fit_default.npz) on an n^3 grid with the hull mask of that
fixture, east-north-up frame for the two entries that take one.  One process; every call is warmed up before anything is timed.
"call" is HIP events on the context's stream around the whole entry (hull pass included where the entry has one:
vi_eval_grad_f64 has none - Estimate.gradient masks on the host), "kernel" the context's own event pair around the evaluation
kernel (vi_eval_kernel_ms; the two gradient entries record none), best of --calls.

    python tools/perf_eval_hess.py [--n 128] [--calls 3] [--frame enu] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=128)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--frame', default='enu', choices=['model', 'enu'])
    ap.add_argument('--out')
    a = ap.parse_args()
    from volumetricinterp_amd import _lib, synth
    from volumetricinterp_amd.estimate import Estimate, GRADIENT_FRAMES
    f = np.load(os.path.join(REPO, 'tests', 'golden', 'fit_default.npz'))
    es = Estimate.from_arrays(np.nan_to_num(f['Coeffs']), f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))
    ctx, h, N = es.model.ctx, es.model.handle(), es.model.nbasis
    grid = synth.query_grid(a.n)
    Q = grid[0].size
    eq, tol = es._hull()
    F, frame = eq.shape[0], GRADIENT_FRAMES[a.frame]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, kernel):
        fn()                                                            # warm-up
        ctx.sync()
        call = kern = np.inf
        for _ in range(a.calls):
            ctx.timer_start()
            fn()
            call = min(call, ctx.timer_stop_ms())
            if kernel:
                kern = min(kern, ctx.eval_kernel_ms())
        return call, kern

    with ctx.scope() as dev:
        dlat, dlon, dalt = (dev.up(np.ascontiguousarray(x.ravel())) for x in grid)
        dE, dC = dev.up(eq), dev.up(np.nan_to_num(f['Coeffs'])[0])
        d3, d6 = dev.empty((Q, 3)), dev.empty((6, Q))
        dG = dev.empty((N, 3, Q))
        dH = dev.empty((N, 6, Q))
        pts = (h, Q, dlat.ptr, dlon.ptr, dalt.ptr)
        lib, check = _lib.lib, _lib.check
        ctx.eval_timing(True)
        g_call, _ = timed(lambda: check(lib.vi_eval_grad_f64(*pts, dC.ptr, d3.ptr), 'vi_eval_grad_f64'), False)
        h_call, h_kern = timed(lambda: check(lib.vi_eval_hess_f64(*pts, dC.ptr, dE.ptr, F, tol, frame, d6.ptr), 'vi_eval_hess_f64'),
                               True)
        n_call, n_kern = timed(lambda: check(lib.vi_eval_hess_f64(*pts, dC.ptr, None, 0, 0., frame, d6.ptr), 'vi_eval_hess_f64'),
                               True)
        gb_call, _ = timed(lambda: check(lib.vi_eval_grad_basis_f64(*pts, dE.ptr, F, tol, frame, dG.ptr), 'vi_eval_grad_basis_f64'),
                           False)
        hb_call, hb_kern = timed(lambda: check(lib.vi_eval_hess_basis_f64(*pts, dE.ptr, F, tol, frame, dH.ptr),
                                               'vi_eval_hess_basis_f64'), True)
        ctx.eval_timing(False)
        inside = float(np.isfinite(d6.download()[0]).mean())            # (the last vi_eval_hess_f64 call had no hull)
        inside_h = float(np.isfinite(dH.download(Q)).mean())
    emit('second derivatives, N = %d, %d^3 = %d points, %d hull facets (%.1f %% of the points inside), frame %s; best of %d timed '
         'calls after a warm-up' % (N, a.n, Q, F, 100. * inside_h, a.frame, a.calls))
    assert inside == 1.0
    emit('  at points, one coefficient vector:')
    emit('    vi_eval_grad_f64 (no hull, model frame)   call %9.3f ms = %6.2f ns/point' % (g_call, 1e6 * g_call / Q))
    emit('    vi_eval_hess_f64 without the hull         call %9.3f ms, kernel %9.3f ms = %6.2f ns/point; kernel / gradient call %.2f'
         % (n_call, n_kern, 1e6 * n_kern / Q, n_kern / g_call))
    emit('    vi_eval_hess_f64 with the hull            call %9.3f ms, kernel %9.3f ms = %6.2f ns/point' % (h_call, h_kern, 1e6 * h_kern / Q))
    emit('  set-up of a resident grid (hull pass included in the call):')
    emit('    vi_eval_grad_basis_f64  N x 3 x Q = %5.1f GB   call %9.3f ms = %6.1f GB/s of stores' % (N * 3 * Q * 8 / 1e9, gb_call, N * 3 * Q * 8 / gb_call / 1e6))
    emit('    vi_eval_hess_basis_f64  N x 6 x Q = %5.1f GB   call %9.3f ms = %6.1f GB/s of stores, kernel %9.3f ms; Hessian / gradient '
         'call %.2f (twice the stores)' % (N * 6 * Q * 8 / 1e9, hb_call, N * 6 * Q * 8 / hb_call / 1e6, hb_kern, hb_call / gb_call))
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
