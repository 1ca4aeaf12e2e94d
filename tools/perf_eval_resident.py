"""Rate of the resident-basis evaluation (vi_eval_resident_f64) on a 256^3 grid at the default order, by timesteps per call:
K2r (csrc/vi_eval_resident.hip) and, with VINTERP_EVAL_RESIDENT=blas, the library's product.

python tools/perf_eval_resident.py [n] [--hull] [--timesteps T[,T...]] [--reps R]

--hull: Y through vi_eval_basis_f64 with the hull of bench.py (beams synth.beams(26, 100, seed=0)), the points outside it as NaN
columns, as workload c3 evaluates it; K2r then skips the 32-byte pieces whose four points are all outside (VINTERP_K2R_LIVE=0:
it does not), and the line carries the issued rate - 2 N x points of live pieces x timesteps / time, what the matrix cores
execute - next to the algorithmic one over all points.  --timesteps 512 --reps 1: one call, for a counter pass."""
import argparse
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from volumetricinterp_amd import _lib, synth                                  # noqa: E402
from volumetricinterp_amd.models.sphharmlag import Model                      # noqa: E402

CFG = '[DEFAULT]\n[MODEL]\nNAME = sphharmlag\nMAXK = 4\nMAXL = 6\nCAP_LIM = 10\nMAX_Z_INT = INF\nLATCP = 78\nLONCP = 262\n'
ap = argparse.ArgumentParser()
ap.add_argument('n', nargs='?', type=int, default=256)
ap.add_argument('--hull', action='store_true')
ap.add_argument('--timesteps', default='64,128,256,512')
ap.add_argument('--reps', type=int, default=3)
args = ap.parse_args()
n = args.n
Ts = [int(t) for t in args.timesteps.split(',')]
m = Model(io.StringIO(CFG))
ctx, h, N = m.ctx, m.handle(), m.nbasis
g = synth.query_grid(n)
Q = g[0].size
dq = [ctx.to_device(a.ravel()) for a in g]
dY = ctx.empty((N, Q))
dhull, F, tol = None, 0, 0.
if args.hull:
    from scipy.spatial import ConvexHull
    from volumetricinterp_amd.estimate import hull_equations
    from volumetricinterp_amd.geodesy import geodetic2ecef
    R = np.array(geodetic2ecef(*synth.beams(*synth.GEOM_C2, seed=0))).T
    eq, tol = hull_equations(R[ConvexHull(R).vertices])
    dhull, F = ctx.to_device(np.ascontiguousarray(eq)), eq.shape[0]
ctx.timer_start()
_lib.check(_lib.lib.vi_eval_basis_f64(h, Q, dq[0].ptr, dq[1].ptr, dq[2].ptr, dhull.ptr if dhull else None, F, tol, dY.ptr),
           'vi_eval_basis_f64')
print('basis of %d^3 points (%.1f GB)%s: %.1f ms' % (n, N * Q * 8 / 1e9, ', hull of %d facets' % F if F else '', ctx.timer_stop_ms()))
live = 1.
if args.hull:
    row0 = np.empty(Q)
    _lib.check(_lib.lib.vi_d2h(ctx.handle, row0.ctypes.data_as(_lib.VOIDP), dY.ptr, Q * 8), 'vi_d2h')
    inside = np.isfinite(row0)
    live = float(inside.reshape(-1, 4).any(axis=1).mean()) if Q % 4 == 0 else 1.
    print('%.1f %% of the points outside the hull; live share of the 4-point pieces %.3f' % (100. * (1. - inside.mean()), live))
rng = np.random.default_rng(0)
Tmax = max(Ts)
dC = ctx.to_device(rng.standard_normal((Tmax, N)))
dO = ctx.empty((Tmax, Q))
plain = os.environ.get('VINTERP_K2R_LIVE') == '0' or os.environ.get('VINTERP_EVAL_RESIDENT') == 'blas'
for T in Ts:
    best = 1e9
    for rep in range(args.reps):
        ctx.timer_start()
        _lib.check(_lib.lib.vi_eval_resident_f64(h, Q, T, dY.ptr, dC.ptr, dO.ptr), 'vi_eval_resident_f64')
        best = min(best, ctx.timer_stop_ms())
    alg = 2. * N * Q * T / best / 1e9
    print('%s T %4d: %8.3f ms  %.1f TFLOP/s  %.3e point-timesteps/s; algorithmic bytes (Y once + out) %.1f GB -> %.0f GB/s' % (
        os.environ.get('VINTERP_EVAL_RESIDENT', 'own'), T, best, alg, Q * T / (best * 1e-3),
        (N * Q * 8 + T * Q * 8) / 1e9, (N * Q * 8 + T * Q * 8) / 1e9 / (best * 1e-3))
        + ('; issued %.1f TFLOP/s (live share %.3f; Y of live pieces + out %.1f GB)'
           % (alg * live, live, (live * N * Q * 8 + T * Q * 8) / 1e9) if args.hull and not plain else ''))
