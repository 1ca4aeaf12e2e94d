"""Rate of the line integrals along straight rays (Estimate.slant, vi_eval_slant_f64 - K2l, csrc/vi_slant.hip): every ray at its own
time, one library call, in nearest and in interpolation mode, against
  (b) the floor: one vi_eval_f64 call with a single coefficient row and no hull on as many points as (a) has live nodes (what
      the nodes cost when they are plain points that share a time), and
  (c) what a user writes without it: the chords and the nodes on the host, geodesy.ecef2geodetic, Estimate.track at all nodes
      (no hull test: the nodes are inside by construction), and the weighted sum on the host.
Also the largest per-ray difference between 64 and 128 Gauss-Legendre nodes on the same rays, relative to the ray's absolute sum
sum_i |W_i f_i| at 128 nodes: how far the default rule is converged.

Workload: the default order (N = 144, the config of tests/golden/fit_default.npz) with the hull of that fixture, R = 1000 records
60 s apart (the fixture's rows, scaled), P = 1e5 and 1e6 rays from the ground below the hull to GNSS altitude (start lat 75-81,
lon 250-274, alt 0; end lat 40-89, lon 200-320, alt 20 200 km; about half of them enter the hull) at random times over the
records' range, 64 nodes.  One process; every shape is warmed up before anything is timed; --reps repetitions, median and range
reported.  Device time is the context's event pair around the evaluation kernel (vi_eval_kernel_ms: the coefficient preparation
and, for (c), the hull pass are outside it); wall time is the host clock around the whole Python call, which ends in a download.

    python tools/perf_eval_slant.py [--reps 5] [--small] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NODES = 64
USER_RAYS = 100000           # rays of the comparison with the user's path


def stats(x):
    x = np.sort(np.asarray(x, dtype=np.float64))
    return '%9.3f ms (%.3f - %.3f)' % (np.median(x), x[0], x[-1])


def user_path(es, t0, a, b, x, wq, chunk=1 << 16):
    """(c): host chords, host nodes, ecef2geodetic, Estimate.track, host sum - in chunks of rays, as the node arrays are 64 times
    the rays'.  Returns (values, absolute sums, device ms of the track calls)."""
    from volumetricinterp_amd import geodesy
    from volumetricinterp_amd.estimate import hull_chords
    eq, tol = es._hull()
    ctx = es.model.ctx
    P = len(a)
    out, scale, dev = np.full(P, np.nan), np.full(P, np.nan), 0.
    for i in range(0, P, chunk):
        k = slice(i, i + chunk)
        s0, s1 = hull_chords(eq, tol, a[k], b[k])
        hit = np.flatnonzero(~np.isnan(s0))
        if not hit.size:
            continue
        aa, d = a[k][hit], (b[k] - a[k])[hit]
        s = s0[hit, None] + (s1 - s0)[hit, None] * (1. + x[None, :]) / 2.
        pts = aa[:, None, :] + s[:, :, None] * d[:, None, :]
        lat, lon, alt = geodesy.ecef2geodetic(pts[..., 0], pts[..., 1], pts[..., 2])
        f = es.track(np.repeat(t0[k][hit], x.size).reshape(lat.shape), lat, lon, alt, check_hull=False)
        dev += ctx.eval_kernel_ms()
        W = wq[None, :] * ((s1 - s0)[hit] / 2. * np.linalg.norm(d, axis=1))[:, None]
        out[i + hit] = (W * f).sum(axis=1)
        scale[i + hit] = np.abs(W * f).sum(axis=1)
    return out, scale, dev


def shape(f, R, P, reps, emit):
    from volumetricinterp_amd import _lib, geodesy, synth
    from volumetricinterp_amd.estimate import Estimate
    rng = np.random.default_rng(0)
    rows = np.nan_to_num(f['Coeffs'])
    C = rows[np.arange(R) % len(rows)] * rng.uniform(0.5, 2., R)[:, None]
    time_ = synth.unix_times(R)
    mt = np.mean(time_, axis=1)
    start = (rng.uniform(75, 81, P), rng.uniform(250, 274, P), np.zeros(P))
    end = (rng.uniform(40, 89, P), rng.uniform(200, 320, P), np.full(P, 20200e3))
    a = np.ascontiguousarray(np.array(geodesy.geodetic2ecef(*start)).T)
    b = np.ascontiguousarray(np.array(geodesy.geodetic2ecef(*end)).T)
    t0 = rng.uniform(mt[0], mt[-1], P)
    x, wq = np.polynomial.legendre.leggauss(NODES)
    res = {}
    for timeinterp in (False, True):
        es = Estimate.from_arrays(C, None, time_, f['hull_vert'], str(f['cfg']), timeinterp=timeinterp)
        ctx = es.model.ctx
        ctx.eval_timing(True)
        out = es.slant(t0, start, end, nodes=NODES)                     # warm-up
        dev, wall = [], []
        for _ in range(reps):
            t = time.perf_counter()
            es.slant(t0, start, end, nodes=NODES, out=out)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(ctx.eval_kernel_ms())
        live = int(np.isfinite(out).sum())
        res[timeinterp] = (np.median(dev), np.median(wall), out.copy())
        emit('  (a) slant, %-13s device %s = %.3e live nodes/s (%d of %d rays enter the hull); wall %s'
             % ('interpolation:' if timeinterp else 'nearest:', stats(dev), live * NODES / np.median(dev) * 1e3, live, P, stats(wall)))
        # convergence of the default rule
        fine, scale, _ = user_path(es, t0[:20000], a[:20000], b[:20000], *np.polynomial.legendre.leggauss(128))
        ok = np.isfinite(fine)
        more = es.slant(t0[:20000], start_of(start, 20000), start_of(end, 20000), nodes=128)
        emit('      64 against 128 nodes on the first 20000 rays: max |difference| / sum |W f| = %.2e (slant at 128 nodes against '
             'the host sum at 128: %.2e)' % (np.max(np.abs(out[:20000][ok] - more[ok]) / scale[ok]),
                                            np.max(np.abs(fine[ok] - more[ok]) / scale[ok])))
    # (b) the floor: as many plain points as (a) has live nodes, one time, one row, no hull - device buffers
    Q = live * NODES
    lat, lon, alt = rng.uniform(75, 81, Q), rng.uniform(250, 274, Q), rng.uniform(100e3, 700e3, Q)
    bufs = [ctx.to_device(v) for v in (lat, lon, alt, C[:1])] + [ctx.empty((1, Q))]
    try:
        def one():
            _lib.check(_lib.lib.vi_eval_f64(es.model.handle(), Q, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, 1, bufs[3].ptr, None, 0, 0.,
                                            bufs[4].ptr), 'vi_eval_f64')
            ctx.sync()
            return ctx.eval_kernel_ms()
        one()
        floor = [one() for _ in range(reps)]
    finally:
        for v in bufs:
            v.free()
    emit('  (b) %d points at one time, one row (vi_eval_f64, T = 1, no hull): device %s = %.3e points/s; slant / floor: nearest '
         '%.2f, interpolation %.2f' % (Q, stats(floor), Q / np.median(floor) * 1e3, res[False][0] / np.median(floor),
                                       res[True][0] / np.median(floor)))
    # (c) the user's path (interpolation mode, the Estimate of the last round) on the first USER_RAYS rays - its host side takes a
    # minute per 1e6 rays -, against the slant of the same rays
    n = min(P, USER_RAYS)
    sub = es.slant(t0[:n], start_of(start, n), start_of(end, n), nodes=NODES)
    sdev, swall = [], []
    for _ in range(reps):
        t = time.perf_counter()
        es.slant(t0[:n], start_of(start, n), start_of(end, n), nodes=NODES, out=sub)
        swall.append((time.perf_counter() - t) * 1e3)
        sdev.append(ctx.eval_kernel_ms())
    user_path(es, t0[:n], a[:n], b[:n], x, wq)
    runs = []
    for _ in range(max(1, reps // 2)):
        t = time.perf_counter()
        val, scale, dev = user_path(es, t0[:n], a[:n], b[:n], x, wq)
        runs.append((dev, (time.perf_counter() - t) * 1e3))
    ctx.eval_timing(False)
    ok = np.isfinite(val)
    udev, uwall = np.median([r[0] for r in runs]), np.median([r[1] for r in runs])
    emit('  (c) host nodes, ecef2geodetic, Estimate.track, host sum (interpolation, the first %d rays): device %s, wall %s; the slant '
         'of the same rays: device %s, wall %s; (c) / slant: device %.2f, wall %.1f; max |slant - (c)| / sum |W f| = %.2e'
         % (n, stats([r[0] for r in runs]), stats([r[1] for r in runs]), stats(sdev), stats(swall), udev / np.median(sdev),
            uwall / np.median(swall), np.max(np.abs(val[ok] - sub[ok]) / scale[ok])))


def start_of(triple, n):
    return tuple(v[:n] for v in triple)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='P = 1e5 only')
    ap.add_argument('--out')
    a = ap.parse_args()
    f = np.load(os.path.join(REPO, 'tests', 'golden', 'fit_default.npz'))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit('line integrals along rays, N = 144, hull of the default fixture, R = 1000 records, %d Gauss-Legendre nodes, rays in random '
         'order; median (min - max) of %d timed calls after a warm-up' % (NODES, a.reps))
    for P in [100000] + ([] if a.small else [1000000]):
        emit('P = %d' % P)
        shape(f, 1000, P, a.reps, emit)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
