"""Rate of the evaluation along a trajectory (Estimate.track, vi_eval_track_f64 - K2t, csrc/vi_track.hip): every point at its
own time, one library call, in nearest and in interpolation mode, against
  (a) the floor: the same points at ONE time, one vi_eval_f64 call with a single coefficient row (what the points cost when
      they share a time; and with four rows: what the tile of four costs in k_eval_sph_fast's workgroups of 256), and
  (b) the loop a user writes without it: one Estimate.__call__ per record on that record's points.

Workload: the default order (N = 144, the config of tests/golden/fit_default.npz) with the hull mask of that fixture, R = 1000
records 60 s apart (the fixture's rows, scaled), Q = 1e6 and 1e7 random points in the box of the tests (some of it outside the
hull) at sorted times uniform over the records' range.  One process; every shape is warmed up before anything is timed; --reps
repetitions, median and range reported.  Device time is the context's event pair around the evaluation kernel
(vi_eval_kernel_ms: the hull pass and the coefficient preparation are outside it); wall time is the host clock around the
whole Python call (record selection, sort, uploads, kernel, download; for the loop: all R calls), which ends in a download.

    python tools/perf_eval_track.py [--reps 5] [--small] [--out FILE]
"""
import argparse
import datetime as dt
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

EPOCH = dt.datetime(1970, 1, 1)


def stats(x):
    x = np.sort(np.asarray(x, dtype=np.float64))
    return '%9.3f ms (%.3f - %.3f)' % (np.median(x), x[0], x[-1])


def shape(f, R, Q, reps, emit):
    from volumetricinterp_amd import _lib, synth
    from volumetricinterp_amd.estimate import Estimate
    rng = np.random.default_rng(0)
    rows = np.nan_to_num(f['Coeffs'])
    N = rows.shape[1]
    C = rows[np.arange(R) % len(rows)] * rng.uniform(0.5, 2., R)[:, None]
    time_ = synth.unix_times(R)
    mt = np.mean(time_, axis=1)
    cov = np.broadcast_to(np.zeros((1, N, N)), (R, N, N))              # get_C indexes it; nothing here evaluates it
    lat, lon, alt = rng.uniform(75, 81, Q), rng.uniform(250, 274, Q), rng.uniform(100e3, 700e3, Q)
    t0 = np.sort(rng.uniform(mt[0], mt[-1], Q))
    res = {}
    for timeinterp in (False, True):
        es = Estimate.from_arrays(C, cov, time_, f['hull_vert'], str(f['cfg']), timeinterp=timeinterp)
        ctx = es.model.ctx
        ctx.eval_timing(True)
        out = es.track(t0, lat, lon, alt)                               # warm-up
        dev, wall = [], []
        for _ in range(reps):
            t = time.perf_counter()
            es.track(t0, lat, lon, alt, out=out)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(ctx.eval_kernel_ms())
        res[timeinterp] = (np.median(dev), np.median(wall))
        inside = float(np.isfinite(out).mean())
        emit('  track, %-13s device %s = %.3e points/s; wall %s' % ('interpolation:' if timeinterp else 'nearest:', stats(dev),
                                                                   Q / np.median(dev) * 1e3, stats(wall)))
    # (a) the floor: all points at one time, device buffers, one row
    eq, tol = es._hull()
    bufs = [ctx.to_device(a) for a in (lat, lon, alt, C[:4], eq)] + [ctx.empty((4, Q))]
    try:
        def one(T=1):
            _lib.check(_lib.lib.vi_eval_f64(es.model.handle(), Q, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, T, bufs[3].ptr, bufs[4].ptr,
                                            eq.shape[0], tol, bufs[5].ptr), 'vi_eval_f64')
            ctx.sync()
            return ctx.eval_kernel_ms()
        one(), one(4)
        floor = [one() for _ in range(reps)]
        tile = [one(4) for _ in range(reps)]            # the same points against a tile of four rows in k_eval_sph_fast
    finally:
        for a in bufs:
            a.free()
    emit('  (a) one time, one row (vi_eval_f64, T = 1): device %s = %.3e points/s; track / floor: nearest %.2f, interpolation '
         '%.2f (%.1f %% of the points inside the hull)' % (stats(floor), Q / np.median(floor) * 1e3, res[False][0] / np.median(floor),
                                                           res[True][0] / np.median(floor), 100. * inside))
    emit('      four rows at one time (vi_eval_f64, T = 4: the tile of four in workgroups of 256): device %s; track / that: nearest '
         '%.2f, interpolation %.2f' % (stats(tile), res[False][0] / np.median(tile), res[True][0] / np.median(tile)))
    # (b) the loop: one __call__ per record on its points (nearest mode: the record's mid-time)
    es = Estimate.from_arrays(C, cov, time_, f['hull_vert'], str(f['cfg']))
    ctx = es.model.ctx
    rec, _ = es.select_records(t0)
    cut = np.searchsorted(rec, np.arange(R + 1))
    when = [EPOCH + dt.timedelta(seconds=float(m)) for m in mt]

    def loop():
        dev = 0.
        t = time.perf_counter()
        for r in range(R):
            a, b = cut[r], cut[r + 1]
            if b > a:
                es(when[r], lat[a:b], lon[a:b], alt[a:b])
                dev += ctx.eval_kernel_ms()
        return dev, (time.perf_counter() - t) * 1e3
    loop()
    runs = [loop() for _ in range(max(1, reps // 2))]
    ctx.eval_timing(False)
    ldev, lwall = np.median([r[0] for r in runs]), np.median([r[1] for r in runs])
    emit('  (b) one Estimate.__call__ per record (%d calls): device %s, wall %s = %.1fx / %.1fx the nearest-mode track'
         % (R, stats([r[0] for r in runs]), stats([r[1] for r in runs]), ldev / res[False][0], lwall / res[False][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='Q = 1e6 only')
    ap.add_argument('--out')
    a = ap.parse_args()
    f = np.load(os.path.join(REPO, 'tests', 'golden', 'fit_default.npz'))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit('evaluation along a trajectory, N = 144, hull mask of the default fixture, R = 1000 records, points sorted by time; '
         'median (min - max) of %d timed calls after a warm-up' % a.reps)
    for Q in [1000000] + ([] if a.small else [10000000]):
        emit('Q = %d' % Q)
        shape(f, 1000, Q, a.reps, emit)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
