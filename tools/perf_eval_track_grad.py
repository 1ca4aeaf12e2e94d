"""Rate of the gradient along a trajectory (Estimate.track_gradient, vi_eval_track_grad_f64 - K2tg, csrc/vi_track.hip): every
point at its own time, one library call, in nearest and in interpolation mode, in the model frame and in east-north-up, against
  (a) the floor: vi_eval_track_f64 (K2t, the density) on the same points, records and mode, and
  (b) the loop it replaces: one vi_eval_grad_f64 call per record on that record's points (nearest mode) - the summed kernel time
      of the calls on device copies, and the wall time of one Estimate.gradient per record, with the host hull mask it applies.

Workload: the default order (N = 144, the config of tests/golden/fit_default.npz) with the hull mask of that fixture, R = 1000
records 60 s apart (the fixture's rows, scaled), Q = 1e6 and 1e7 random points in the box of the tests (some of it outside the
hull) at sorted times uniform over the records' range.  One process; every shape is warmed up before anything is timed; --reps
repetitions, median and range reported.  Device time of (a) and of the new call is the context's event pair around the
evaluation kernel (vi_eval_kernel_ms: the hull pass and the coefficient preparation are outside it); vi_eval_grad_f64 is not
timed by that pair, so the loop's kernel time is the context's other event pair (vi_timer_start / vi_timer_stop_ms) around each
launch on the same stream, summed.  Wall time is the host clock around the whole Python call (record selection, sort, uploads, kernel, download;
for the loop: all R calls).

    python tools/perf_eval_track_grad.py [--reps 5] [--small] [--out FILE]
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
        mode = 'interpolation' if timeinterp else 'nearest'
        es = Estimate.from_arrays(C, cov, time_, f['hull_vert'], str(f['cfg']), timeinterp=timeinterp)
        ctx = es.model.ctx
        ctx.eval_timing(True)
        for frame in ('model', 'enu'):
            out = es.track_gradient(t0, lat, lon, alt, frame=frame)     # warm-up
            dev, wall = [], []
            for _ in range(reps):
                t = time.perf_counter()
                es.track_gradient(t0, lat, lon, alt, frame=frame, out=out)
                wall.append((time.perf_counter() - t) * 1e3)
                dev.append(ctx.eval_kernel_ms())
            res[timeinterp, frame] = (np.median(dev), np.median(wall))
            emit('  track_gradient, %-13s %-5s device %s = %.3e points/s; wall %s'
                 % (mode + ',', frame + ':', stats(dev), Q / np.median(dev) * 1e3, stats(wall)))
        # (a) the floor: the density on the same points
        den = es.track(t0, lat, lon, alt)
        dev, wall = [], []
        for _ in range(reps):
            t = time.perf_counter()
            es.track(t0, lat, lon, alt, out=den)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(ctx.eval_kernel_ms())
        emit('  (a) track (vi_eval_track_f64), %-13s device %s; wall %s; track_gradient / track, device: model %.2f, enu %.2f '
             '(%.1f %% of the points inside the hull)' % (mode + ':', stats(dev), stats(wall), res[timeinterp, 'model'][0] / np.median(dev),
                                                         res[timeinterp, 'enu'][0] / np.median(dev), 100. * np.isfinite(den).mean()))
        ctx.eval_timing(False)
    # (b) the loop: one gradient call per record on its points (nearest mode: the record's mid-time)
    es = Estimate.from_arrays(C, cov, time_, f['hull_vert'], str(f['cfg']))
    ctx = es.model.ctx
    rec, _ = es.select_records(t0)
    cut = np.searchsorted(rec, np.arange(R + 1))
    when = [EPOCH + dt.timedelta(seconds=float(m)) for m in mt]
    bufs = [ctx.to_device(a) for a in (lat, lon, alt, C)] + [ctx.empty((Q, 3))]
    try:
        def kernels():
            """the R launches alone, on device copies of the sorted points: summed stream time of the launches"""
            total = 0.
            ptr = [b.ptr.value for b in bufs]
            for r in range(R):
                a, b = int(cut[r]), int(cut[r + 1])
                if b > a:
                    ctx.timer_start()
                    _lib.check(_lib.lib.vi_eval_grad_f64(es.model.handle(), b - a, ptr[0] + 8 * a, ptr[1] + 8 * a, ptr[2] + 8 * a,
                                                         ptr[3] + 8 * N * r, ptr[4] + 24 * a), 'vi_eval_grad_f64')
                    total += ctx.timer_stop_ms()
            return total
        kernels()
        kdev = [kernels() for _ in range(reps)]
    finally:
        for a in bufs:
            a.free()

    def loop():
        t = time.perf_counter()
        for r in range(R):
            a, b = cut[r], cut[r + 1]
            if b > a:
                es.gradient(when[r], lat[a:b], lon[a:b], alt[a:b])
        return (time.perf_counter() - t) * 1e3
    loop()
    lwall = [loop() for _ in range(max(1, reps // 2))]
    one = res[False, 'model']
    emit('  (b) one vi_eval_grad_f64 per record (%d launches): summed kernel time %s = %.2fx the nearest-mode model-frame '
         'track_gradient; one Estimate.gradient per record, with its host hull mask: wall %s = %.1fx'
         % (R, stats(kdev), np.median(kdev) / one[0], stats(lwall), np.median(lwall) / one[1]))


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

    emit('gradient along a trajectory, N = 144, hull mask of the default fixture, R = 1000 records, points sorted by time; '
         'median (min - max) of %d timed calls after a warm-up' % a.reps)
    for Q in [1000000] + ([] if a.small else [10000000]):
        emit('Q = %d' % Q)
        shape(f, 1000, Q, a.reps, emit)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
