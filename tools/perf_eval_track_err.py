"""Cost of the standard errors with a time per point (Estimate.track_error, vi_eval_track_err_f64 - the basis of a chunk, then
K2te, csrc/vi_eval_resident.hip) and per ray (Estimate.slant_error, vi_eval_slant_err_f64 - K1l, then K2te), against
  (b) the loop a user writes without them: one Estimate.error per distinct record on that record's points (each call uploads
      a covariance, builds a basis, runs the library's product and evaluates the points again for the hull),
  (c) the floor: the same points at ONE record through resident_grid(...).error - K2e on a resident basis - and, on that same
      resident basis, K2te alone through vi_eval_records_err_f64: K2te over K2e is what the staging per run costs,
  (d) Estimate.slant on the same rays: the integral itself,
and against the library route of the same call (VINTERP_EVAL_RESIDENT=blas, read once per process: a child process).

Workload: the default order (N = 144, tests/golden/fit_default.npz) with the hull of that fixture, R = 1000 records 60 s apart
(the fixture's covariances, scaled by powers of 4), Q = 1e5 and 1e6 random points in the box of the tests at times uniform over
the records' range, sorted by time and in random order (track_error sorts by record on the host either way: the difference is
that sort); 1e5 receiver-to-GNSS rays.  One process per route; every shape is called once before anything is timed; --reps
repetitions, the versions alternating, median and range reported.  Device time is the context's event pair (vi_eval_kernel_ms:
for track_error and slant_error around the chunk loop, basis included); wall time is the host clock around the Python call.

    python tools/perf_eval_track_err.py [--reps 5] [--small] [--out FILE]
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

EPOCH = dt.datetime(1970, 1, 1)
R = 1000


def stats(x):
    x = np.sort(np.asarray(x, dtype=np.float64))
    return '%9.3f ms (%.3f - %.3f)' % (np.median(x), x[0], x[-1])


def estimate(f, timeinterp=False):
    from volumetricinterp_amd import synth
    from volumetricinterp_amd.estimate import Estimate
    rng = np.random.default_rng(0)
    base = f['Covariance']
    dC = base[np.arange(R) % len(base)] * (4.0 ** rng.integers(-4, 5, R))[:, None, None]
    C = np.zeros((R, base.shape[1]))
    return Estimate.from_arrays(C, dC, synth.unix_times(R), f['hull_vert'], str(f['cfg']), timeinterp=timeinterp)


def points(es, Q, order):
    rng = np.random.default_rng(1)
    mt = np.mean(es.time, axis=1)
    lat, lon, alt = rng.uniform(75, 81, Q), rng.uniform(250, 274, Q), rng.uniform(100e3, 700e3, Q)
    t0 = rng.uniform(mt[0], mt[-1], Q)
    return (np.sort(t0) if order == 'sorted' else t0), lat, lon, alt


def timed(ctx, call, reps):
    """(device ms, wall ms) lists of `reps` calls after one warm-up."""
    call()
    dev, wall = [], []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(ctx.eval_kernel_ms())
    return dev, wall


def track_shape(f, Q, order, reps, emit, loop=True):
    from volumetricinterp_amd import _lib
    from volumetricinterp_amd.estimate import used_records
    res = {}
    for timeinterp in (False, True):
        es = estimate(f, timeinterp)
        ctx = es.model.ctx
        ctx.eval_timing(True)
        t0, lat, lon, alt = points(es, Q, order)
        out = np.empty(Q)
        dev, wall = timed(ctx, lambda: es.track_error(t0, lat, lon, alt, out=out), reps)
        res[timeinterp] = (np.median(dev), np.median(wall))
        emit('  (a) track_error, %-14s device %s = %.3e points/s; wall %s (%.1f %% of the points inside the hull)'
             % ('interpolation:' if timeinterp else 'nearest:', stats(dev), Q / np.median(dev) * 1e3, stats(wall),
                100. * np.isfinite(out).mean()))
    if not loop:
        return res
    # (b) the loop of the parent commit, alternating with (a), nearest mode
    es = estimate(f)
    ctx = es.model.ctx
    t0, lat, lon, alt = points(es, Q, order)
    rec, _ = es.select_records(t0)
    by = np.argsort(rec, kind='stable')
    cut = np.searchsorted(rec[by], np.arange(R + 1))
    when = [EPOCH + dt.timedelta(seconds=float(m)) for m in np.mean(es.time, axis=1)]

    def loop_():
        t = time.perf_counter()
        for r in range(R):
            k = by[cut[r]:cut[r + 1]]
            if k.size:
                es.error(when[r], lat[k], lon[k], alt[k])
        return (time.perf_counter() - t) * 1e3

    loop_()
    a_wall, b_wall = [], []
    for _ in range(max(1, reps // 2)):
        t = time.perf_counter()
        es.track_error(t0, lat, lon, alt)
        a_wall.append((time.perf_counter() - t) * 1e3)
        b_wall.append(loop_())
    emit('  (b) one Estimate.error per record (%d calls; vi_eval_err_f64 has no event pair: device not measured): wall %s = %.1fx '
         'the nearest-mode track_error beside it (%s)' % (R, stats(b_wall), np.median(b_wall) / np.median(a_wall), stats(a_wall)))
    # (c) the floor: one record for all points on a resident basis (K2e), and K2te alone on that basis
    with es.resident_grid(lat, lon, alt) as g:
        dC1 = es.Covariance[:1]
        g.evaluate_errors(dC1)
        k2e = []
        for _ in range(reps):
            g.evaluate_errors(dC1)
            k2e.append(ctx.eval_kernel_ms())
        rows, compact = used_records(np.sort(rec), None, R)
        k2te = {}
        with ctx.scope() as dev_:
            dD, dO = dev_.up(es.Covariance[rows]), dev_.empty(Q)
            for name, rr, w in (('nearest', compact, None), ('one record', np.zeros(Q, np.int32), None)):
                dr = dev_.up(rr, np.int32)

                def call():
                    _lib.check(_lib.lib.vi_eval_records_err_f64(es.model.handle(), Q, g.dY.ptr, dr.ptr, None, len(rows), dD.ptr,
                                                                dO.ptr), 'vi_eval_records_err_f64')
                    ctx.sync()
                k2te[name] = timed(ctx, call, reps)[0]
    emit('  (c) one record, resident basis, K2e (ResidentGrid.evaluate_errors): device %s = %.3e points/s' % (stats(k2e),
                                                                                                              Q / np.median(k2e) * 1e3))
    emit('      the same basis through vi_eval_records_err_f64 (K2te alone), records sorted: device %s = %.2fx K2e; all points on '
         'one record: %s = %.2fx K2e' % (stats(k2te['nearest']), np.median(k2te['nearest']) / np.median(k2e),
                                         stats(k2te['one record']), np.median(k2te['one record']) / np.median(k2e)))
    ctx.eval_timing(False)
    return res


def slant_shape(f, P, reps, emit):
    es = estimate(f)
    ctx = es.model.ctx
    ctx.eval_timing(True)
    rng = np.random.default_rng(2)
    mt = np.mean(es.time, axis=1)
    start = (rng.uniform(75, 81, P), rng.uniform(250, 274, P), np.zeros(P))
    end = (rng.uniform(40, 89, P), rng.uniform(200, 320, P), np.full(P, 20200e3))
    t0 = np.sort(rng.uniform(mt[0], mt[-1], P))
    out = np.empty(P)
    e_dev, e_wall, s_dev, s_wall = [], [], [], []
    es.slant_error(t0, start, end, out=out)
    es.slant(t0, start, end)
    for _ in range(reps):
        for call, dev, wall in ((lambda: es.slant_error(t0, start, end, out=out), e_dev, e_wall),
                                (lambda: es.slant(t0, start, end), s_dev, s_wall)):
            t = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(ctx.eval_kernel_ms())
    ctx.eval_timing(False)
    emit('  (d) slant_error: device %s = %.3e rays/s; wall %s (%.1f %% of the rays enter the hull)'
         % (stats(e_dev), P / np.median(e_dev) * 1e3, stats(e_wall), 100. * np.isfinite(out).mean()))
    emit('      slant on the same rays: device %s; wall %s; slant_error / slant: device %.2f, wall %.2f'
         % (stats(s_dev), stats(s_wall), np.median(e_dev) / np.median(s_dev), np.median(e_wall) / np.median(s_wall)))


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

    if a.route_child:       # (a) alone at the largest shape, sorted, in whatever route the environment selects
        track_shape(f, 100000 if a.small else 1000000, 'sorted', a.reps, emit, loop=False)
        return
    emit('standard errors with a time per point or ray, N = 144, hull of the default fixture, R = %d records; median (min - max) '
         'of %d timed calls after a warm-up' % (R, a.reps))
    for Q in [100000] + ([] if a.small else [1000000]):
        for order in ('sorted', 'random'):
            emit('Q = %d, times %s' % (Q, order))
            track_shape(f, Q, order, a.reps, emit, loop=order == 'sorted')
    emit('P = 100000 rays, 64 nodes, times sorted')
    slant_shape(f, 100000, a.reps, emit)
    emit('the library route of (a) (VINTERP_EVAL_RESIDENT=blas, a child process), Q = %d, times sorted' % (100000 if a.small else 1000000))
    child = subprocess.run([sys.executable, os.path.abspath(__file__), '--route-child', '--reps', str(a.reps)]
                           + (['--small'] if a.small else []), env=dict(os.environ, VINTERP_EVAL_RESIDENT='blas'),
                           capture_output=True, text=True)
    for s in (child.stdout if child.returncode == 0 else 'child failed: ' + child.stderr[-2000:]).splitlines():
        emit(s)
    name = os.path.join('profiles', 'r17_perf_eval_track_err.txt')
    emit('(output of tools/perf_eval_track_err.py; kept as %s)' % name)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
