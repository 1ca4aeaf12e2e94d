"""Rate of the gradient maps on a resident grid (Estimate.resident_grid(..., gradient=...)): the set-up of the gradient basis
G (vi_eval_grad_basis_f64) next to that of the basis matrix Y (vi_eval_basis_f64), the gradient product next to the density
product on the same grid (both vi_eval_resident_f64 - K2r, csrc/vi_eval_resident.hip - the gradient on three times the columns,
so their ratio is the number to look at), and the same timesteps as a loop of Estimate.gradient calls, the only way to get
gradient maps without the resident grid.

Workload: the default order (N = 144, the config of tests/golden/fit_default.npz), an n^3 grid with the hull mask of that
fixture, T coefficient rows (the fixture's, scaled).  Shapes: 128^3 x 64, 128^3 x 512, and with --big 256^3 x 64 (Y 19 GB,
G 57 GB, the gradient maps of the call 26 GB).  One process; every shape is warmed up before anything is timed.  Set-up times
are HIP events on the context's stream around the call, product times the context's own event pair around the evaluation
kernel (vi_eval_kernel_ms), best of --calls; the Estimate.gradient loop is host time per call (upload of the coordinates, the
fused kernel, the hull mask through a second evaluation, download), over --loop calls.

    python tools/perf_eval_resident_grad.py [--big] [--calls 3] [--loop 4] [--frame enu] [--out FILE]
"""
import argparse
import datetime as dt
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PEAK_TF = 78.6                  # fp64 matrix peak of the MI355X


def shape(es, f, n, T, frame, calls, loop, emit):
    from volumetricinterp_amd import _lib, synth
    from volumetricinterp_amd.estimate import GRADIENT_FRAMES
    ctx, h, N = es.model.ctx, es.model.handle(), es.model.nbasis
    rng = np.random.default_rng(0)
    C = np.nan_to_num(f['Coeffs'])[np.arange(T) % len(f['Coeffs'])] * rng.uniform(0.5, 2., T)[:, None]
    grid = synth.query_grid(n)
    with es.resident_grid(*grid, gradient=frame) as g:                  # (warm-up of both set-up calls)
        Q = g.Q
        eq, tol = es._hull()
        bufs = [ctx.to_device(np.ascontiguousarray(a.ravel())) for a in grid] + [ctx.to_device(eq), ctx.to_device(C)]
        dO = ctx.empty((T, 3, Q))
        try:
            def setup_y():
                _lib.check(_lib.lib.vi_eval_basis_f64(h, Q, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, eq.shape[0], tol,
                                                      g.dY.ptr), 'vi_eval_basis_f64')

            def setup_g():
                _lib.check(_lib.lib.vi_eval_grad_basis_f64(h, Q, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, eq.shape[0],
                                                           tol, GRADIENT_FRAMES[frame], g.dG.ptr), 'vi_eval_grad_basis_f64')

            def product(dM, cols):
                _lib.check(_lib.lib.vi_eval_resident_f64(h, cols, T, dM.ptr, bufs[4].ptr, dO.ptr), 'vi_eval_resident_f64')
                ctx.sync()
                return ctx.eval_kernel_ms()

            def timed(fn):
                best = np.inf
                for _ in range(calls):
                    ctx.timer_start()
                    fn()
                    best = min(best, ctx.timer_stop_ms())
                return best

            ms_y, ms_g = timed(setup_y), timed(setup_g)
            ctx.eval_timing(True)
            product(g.dY, Q), product(g.dG, 3 * Q)                      # warm-up of both shapes
            ms_d = min(product(g.dY, Q) for _ in range(calls))
            ms_v = min(product(g.dG, 3 * Q) for _ in range(calls))
            ctx.eval_timing(False)
            inside = float(np.isfinite(g.evaluate_coeffs(C[:1])[0]).mean())
        finally:
            for a in bufs + [dO]:
                a.free()
    emit('%d^3 x T %3d (%s, %.1f %% of the points inside the hull): set-up Y %8.2f ms, G %8.2f ms (%.2fx)'
         % (n, T, frame, 100. * inside, ms_y, ms_g, ms_g / ms_y))
    tf = lambda ms, cols: 2. * N * cols * T / ms / 1e9
    emit('    density product  %9.3f ms = %7.4f ms/timestep, %5.1f TF/s over all points = %4.1f %% of the %.1f TF fp64 matrix peak'
         % (ms_d, ms_d / T, tf(ms_d, Q), 100. * tf(ms_d, Q) / PEAK_TF, PEAK_TF))
    emit('    gradient product %9.3f ms = %7.4f ms/timestep, %5.1f TF/s over all points = %4.1f %% of peak; gradient / density '
         '%.3f (three times the columns)' % (ms_v, ms_v / T, tf(ms_v, 3 * Q), 100. * tf(ms_v, 3 * Q) / PEAK_TF, ms_v / ms_d))
    if loop:
        t = dt.datetime(1970, 1, 1) + dt.timedelta(seconds=float(np.mean(f['utime'][0])))
        es.gradient(t, *grid)                                           # warm-up
        t0 = time.perf_counter()
        for _ in range(loop):
            es.gradient(t, *grid)
        per = (time.perf_counter() - t0) * 1e3 / loop
        emit('    Estimate.gradient, one call per timestep: %9.2f ms/timestep host time (mean of %d calls) = %.0fx the resident '
             'product per timestep (device time; set-up of G and the download of the maps not counted)' % (per, loop, per / (ms_v / T)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--big', action='store_true')
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--loop', type=int, default=4)
    ap.add_argument('--frame', default='enu', choices=['model', 'enu'])
    ap.add_argument('--out')
    a = ap.parse_args()
    from volumetricinterp_amd.estimate import Estimate
    f = np.load(os.path.join(REPO, 'tests', 'golden', 'fit_default.npz'))
    es = Estimate.from_arrays(np.nan_to_num(f['Coeffs']), f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit('gradient maps on a resident grid, N = %d, hull mask of the default fixture; best of %d timed calls after a warm-up of '
         'every shape' % (es.model.nbasis, a.calls))
    for n, T, loop in [(128, 64, a.loop), (128, 512, 0)] + ([(256, 64, min(a.loop, 2))] if a.big else []):
        shape(es, f, n, T, a.frame, a.calls, loop, emit)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
