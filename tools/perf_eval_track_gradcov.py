"""Cost of the gradient covariances with a time per point (Estimate.track_gradient_covariance, vi_eval_track_grad_cov_f64 - the
gradient basis of a chunk, then K2tc, csrc/vi_eval_resident.hip), against
  (a) the library route of the same call (VINTERP_EVAL_RESIDENT=blas, read once per process: a child process),
  (b) the loop a user writes without it: one Estimate.gradient_covariance per distinct record on that record's points (each
      call uploads a covariance, evaluates the hull on the host side of the call and builds the gradient basis of its points),
  (c) the floor: the same points at ONE record through vi_eval_resident_gradcov_f64 - K2c on a resident gradient basis - and,
      on that same resident basis, K2tc alone through vi_eval_records_gradcov_f64: K2tc over K2c is what the staging per run
      costs; the same with VINTERP_K2TC_GROUPS = 1, 2, 4, 8, 16 blocks of 256 points per workgroup.

Workload: the default order (N = 144, tests/golden/fit_default.npz) with the hull of that fixture, R = 1000 records 60 s apart
(the fixture's covariances, scaled by powers of 4), Q = 1e5 and 1e6 random points in the box of the tests at times uniform over
the records' range, sorted by time.  One process per route; every shape is called once before anything is timed; --reps
repetitions, median and range reported.  Device time is the context's event pair (vi_eval_kernel_ms: for
track_gradient_covariance around the chunk loop, gradient basis included; for gradient_covariance around the form of its last
chunk, gradient basis excluded); wall time is the host clock around the Python call.

    python tools/perf_eval_track_gradcov.py [--reps 5] [--small] [--out FILE]
"""
import argparse
import datetime as dt
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))

from perf_eval_track_err import EPOCH, R, estimate, points, stats, timed      # noqa: E402  (the same records and points)

GROUPS = (1, 2, 4, 8, 16)


def track_shape(f, Q, reps, emit, rest=True):
    from volumetricinterp_amd import _lib
    from volumetricinterp_amd.estimate import used_records
    for timeinterp in (False, True):
        es = estimate(f, timeinterp)
        ctx = es.model.ctx
        ctx.eval_timing(True)
        t0, lat, lon, alt = points(es, Q, 'sorted')
        out = np.empty((Q, 3, 3))
        dev, wall = timed(ctx, lambda: es.track_gradient_covariance(t0, lat, lon, alt, out=out), reps)
        emit('  track_gradient_covariance, %-14s device %s = %.3e points/s; wall %s (%.1f %% of the points inside the hull)'
             % ('interpolation:' if timeinterp else 'nearest:', stats(dev), Q / np.median(dev) * 1e3, stats(wall),
                100. * np.isfinite(out[:, 0, 0]).mean()))
    if not rest:
        return
    # (b) the loop of the parent commit, nearest mode
    es = estimate(f)
    ctx = es.model.ctx
    t0, lat, lon, alt = points(es, Q, 'sorted')
    rec, _ = es.select_records(t0)
    by = np.argsort(rec, kind='stable')
    cut = np.searchsorted(rec[by], np.arange(R + 1))
    when = [EPOCH + dt.timedelta(seconds=float(m)) for m in np.mean(es.time, axis=1)]

    def loop():
        t = time.perf_counter()
        dev = 0.0
        for r in range(R):
            k = by[cut[r]:cut[r + 1]]
            if k.size:
                es.gradient_covariance(when[r], lat[k], lon[k], alt[k])
                dev += ctx.eval_kernel_ms()
        return dev, (time.perf_counter() - t) * 1e3

    loop()
    b = [loop() for _ in range(max(1, reps // 2))]
    emit('  (b) one Estimate.gradient_covariance per record (%d calls): device, the forms alone, %s; wall %s'
         % (R, stats([x[0] for x in b]), stats([x[1] for x in b])))
    # (c) the floor: one record for all points on a resident gradient basis (K2c), and K2tc alone on that basis
    h = es.model.handle()
    with es.resident_grid(lat, lon, alt, gradient='model') as g:
        rows, compact = used_records(np.sort(rec), None, R)
        with ctx.scope() as dev_:
            dD, dO = dev_.up(es.Covariance[rows]), dev_.empty((6, Q))
            dw = dev_.up(np.random.default_rng(3).random(Q))

            def k2c():
                _lib.check(_lib.lib.vi_eval_resident_gradcov_f64(h, Q, 1, g.dG.ptr, dD.ptr, dO.ptr), 'vi_eval_resident_gradcov_f64')
                ctx.sync()
            base = timed(ctx, k2c, reps)[0]
            emit('  (c) one record, resident gradient basis, K2c (vi_eval_resident_gradcov_f64): device %s = %.3e points/s'
                 % (stats(base), Q / np.median(base) * 1e3))
            dr = dev_.up(compact, np.int32)
            for groups in (None,) + GROUPS:
                if groups is None:
                    os.environ.pop('VINTERP_K2TC_GROUPS', None)
                else:
                    os.environ['VINTERP_K2TC_GROUPS'] = str(groups)
                line = '      K2tc alone (vi_eval_records_gradcov_f64), records sorted, %s:' % (
                    'default blocks per workgroup' if groups is None else '%2d blocks per workgroup' % groups)
                for name, w in (('nearest', None), ('blend', dw)):
                    def call():
                        _lib.check(_lib.lib.vi_eval_records_gradcov_f64(h, Q, g.dG.ptr, dr.ptr, None if w is None else w.ptr,
                                                                        len(rows), dD.ptr, dO.ptr), 'vi_eval_records_gradcov_f64')
                        ctx.sync()
                    d = timed(ctx, call, reps)[0]
                    line += ' %s device %s = %.2fx K2c;' % (name, stats(d), np.median(d) / np.median(base))
                emit(line)
            os.environ.pop('VINTERP_K2TC_GROUPS', None)
    ctx.eval_timing(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='Q = 1e5 only')
    ap.add_argument('--route-child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--out')
    a = ap.parse_args()
    f = np.load(os.path.join(REPO, 'tests', 'golden', 'fit_default.npz'))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    sizes = [100000] + ([] if a.small else [1000000])
    if a.route_child:       # the call alone, in whatever route the environment selects
        for Q in sizes:
            emit('Q = %d' % Q)
            track_shape(f, Q, a.reps, emit, rest=False)
        return
    emit('gradient covariances with a time per point, N = 144, hull of the default fixture, R = %d records, times sorted; median '
         '(min - max) of %d timed calls after a warm-up' % (R, a.reps))
    for Q in sizes:
        emit('Q = %d' % Q)
        track_shape(f, Q, a.reps, emit)
    emit('(a) the library route of the call (VINTERP_EVAL_RESIDENT=blas, a child process)')
    child = subprocess.run([sys.executable, os.path.abspath(__file__), '--route-child', '--reps', str(a.reps)]
                           + (['--small'] if a.small else []), env=dict(os.environ, VINTERP_EVAL_RESIDENT='blas'),
                           capture_output=True, text=True)
    for s in (child.stdout if child.returncode == 0 else 'child failed: ' + child.stderr[-2000:]).splitlines():
        emit(s)
    name = os.path.join('profiles', 'r18_perf_eval_track_gradcov.txt')
    emit('(output of tools/perf_eval_track_gradcov.py; kept as %s)' % name)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
