"""Cost of the ray-integrated basis of fixed rays (Estimate.resident_rays, vi_eval_slant_basis_f64 - K1l, csrc/vi_slant.hip) and of
the products on it, against what exists without it.

  set-up        kernel time of K1l for 65 536 and 262 144 rays, against the device route that exists today on 65 536 rays: the
                chords and the nodes on the host, geodesy.ecef2geodetic, vi_eval_basis_f64 at all nodes of the rays that enter the
                hull (N x nodes doubles: 4.8 GB if every ray did), vi_reduce_basis_f64 with the rule's weights along each ray, and
                the per-ray scale (s1 - s0) / 2 |b - a| on the host;
  per timestep  ResidentRays.evaluate_coeffs at T = 512 on 262 144 rays, against ONE Estimate.slant call on the same rays at one
                time, in kernel time and in wall time;
  errors        ResidentRays.evaluate_errors with 64 covariances on 262 144 rays (nothing to compare with: recorded only).

Workload: the default order (N = 144, the config of tests/golden/fit_default.npz) with the hull of that fixture, 64 Gauss-Legendre
nodes, rays from the ground below the hull to GNSS altitude (start lat 75-81, lon 250-274, alt 0; end lat 40-89, lon 200-320, alt
20 200 km; about half of them enter the hull).  One process; every shape is warmed up before anything is timed; --reps repetitions,
median and range reported.  Kernel time is the context's event pair around the evaluation kernels of the last library call
(vi_eval_kernel_ms); wall time is the host clock around the whole Python call, transfers included.

    python tools/perf_eval_resident_rays.py [--reps 5] [--small] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NODES = 64


def stats(x):
    x = np.sort(np.asarray(x, dtype=np.float64))
    return '%9.3f ms (%.3f - %.3f)' % (np.median(x), x[0], x[-1])


def rays(rng, P):
    start = (rng.uniform(75, 81, P), rng.uniform(250, 274, P), np.zeros(P))
    end = (rng.uniform(40, 89, P), rng.uniform(200, 320, P), np.full(P, 20200e3))
    return start, end


def timed(reps, call):
    """call() -> kernel ms or None, once as a warm-up and then `reps` times: (kernel times, wall times)."""
    call()
    dev, wall = [], []
    for _ in range(reps):
        t = time.perf_counter()
        d = call()
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(d)
    return dev, wall


def old_route(es, a, b, x, wq):
    """The ray basis of the rays that enter the hull without K1l.  Returns (B (N, hit rays), hit, host ms, device ms)."""
    from volumetricinterp_amd import _lib, geodesy
    from volumetricinterp_amd.estimate import hull_chords
    ctx, h, N = es.model.ctx, es.model.handle(), es.model.nbasis
    t = time.perf_counter()
    eq, tol = es._hull()
    s0, s1 = hull_chords(eq, tol, a, b)
    hit = np.flatnonzero(~np.isnan(s0))
    d = (b - a)[hit]
    s = s0[hit, None] + (s1 - s0)[hit, None] * (1. + x[None, :]) / 2.
    pts = a[hit][:, None, :] + s[:, :, None] * d[:, None, :]
    lat, lon, alt = geodesy.ecef2geodetic(pts[..., 0], pts[..., 1], pts[..., 2])
    scale = (s1 - s0)[hit] / 2. * np.linalg.norm(d, axis=1)
    host = (time.perf_counter() - t) * 1e3
    H, Q = hit.size, hit.size * x.size
    bufs = []
    try:
        t = time.perf_counter()
        for v in (lat, lon, alt, wq):
            bufs.append(ctx.to_device(v))
        bufs.append(ctx.empty((N, Q)))
        bufs.append(ctx.empty((N, H)))
        _lib.check(_lib.lib.vi_eval_basis_f64(h, Q, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None, 0, 0., bufs[4].ptr), 'vi_eval_basis_f64')
        _lib.check(_lib.lib.vi_reduce_basis_f64(h, H, x.size, 1, bufs[4].ptr, bufs[3].ptr, bufs[5].ptr), 'vi_reduce_basis_f64')
        B = bufs[5].download()
        dev = (time.perf_counter() - t) * 1e3
    finally:
        for v in bufs:
            v.free()
    t = time.perf_counter()
    B *= scale[None, :]
    host += (time.perf_counter() - t) * 1e3
    return B, hit, host, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='65 536 rays everywhere, T = 64, 8 covariances')
    ap.add_argument('--out')
    args = ap.parse_args()
    from volumetricinterp_amd import geodesy, synth
    from volumetricinterp_amd.estimate import Estimate
    f = np.load(os.path.join(REPO, 'tests', 'golden', 'fit_default.npz'))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    PS, PL = 65536, (65536 if args.small else 262144)
    T, E = (64, 8) if args.small else (512, 64)
    rng = np.random.default_rng(0)
    rows = np.nan_to_num(f['Coeffs'])
    C = rows[np.arange(T) % len(rows)] * rng.uniform(0.5, 2., T)[:, None]
    cov = f['Covariance'][np.all(np.isfinite(f['Covariance']), axis=(1, 2))]
    dC = cov[np.arange(E) % len(cov)] * rng.uniform(0.5, 2., E)[:, None, None]
    time_ = synth.unix_times(T)
    es = Estimate.from_arrays(C, None, time_, f['hull_vert'], str(f['cfg']))
    ctx = es.model.ctx
    ctx.eval_timing(True)
    N = es.model.nbasis
    x, wq = np.polynomial.legendre.leggauss(NODES)
    emit('ray-integrated basis of fixed rays, N = %d, hull of the default fixture, %d Gauss-Legendre nodes; median (min - max) of %d '
         'timed calls after a warm-up' % (N, NODES, args.reps))

    # ---- set-up
    emit('set-up')
    sets = {}
    for P in sorted({PS, PL}):
        sets[P] = rays(np.random.default_rng(P), P)
        live = [0]

        def build(P=P):
            with es.resident_rays(*sets[P], nodes=NODES) as r:
                k = ctx.eval_kernel_ms()
                live[0] = int((~np.isnan(r.chords[0])).sum())
            return k
        dev, wall = timed(args.reps, build)
        emit('  K1l, %7d rays (%d enter the hull): kernel %s = %.3e live nodes/s; resident_rays wall %s'
             % (P, live[0], stats(dev), live[0] * NODES / np.median(dev) * 1e3, stats(wall)))
    start, end = sets[PS]
    a = np.ascontiguousarray(np.array(geodesy.geodetic2ecef(*start)).T)
    b = np.ascontiguousarray(np.array(geodesy.geodetic2ecef(*end)).T)
    old_route(es, a, b, x, wq)
    runs = [old_route(es, a, b, x, wq) for _ in range(max(1, args.reps // 2))]
    B, hit = runs[-1][0], runs[-1][1]
    with es.resident_rays(*sets[PS], nodes=NODES) as r:
        Y = r.basis()[:, hit]
        dead = int(np.isnan(r.basis()[0]).sum())
    scale = np.abs(Y).max(axis=1, keepdims=True)
    emit('  without it, %d rays (%d enter the hull): host chords, nodes and ecef2geodetic %s; uploads, vi_eval_basis_f64 on %d points '
         '(%.1f GB), vi_reduce_basis_f64, download: wall %s; the two matrices differ by %.1e of the row maximum at most; the dead rays '
         'agree: %s' % (PS, hit.size, stats([q[2] for q in runs]), hit.size * NODES, N * hit.size * NODES * 8 / 1e9,
                        stats([q[3] for q in runs]), np.max(np.abs(Y - B) / scale), dead == PS - hit.size))

    # ---- per timestep and errors
    with es.resident_rays(*sets[PL], nodes=NODES) as r:
        out = np.empty((T, PL))

        def product():
            r.evaluate_coeffs(C, out=out)
            return ctx.eval_kernel_ms()
        dev, wall = timed(args.reps, product)
        emit('per timestep, %d rays' % PL)
        emit('  evaluate_coeffs, T = %d: kernel %s = %.3f us per timestep, %.3e ray-timesteps/s; wall %s = %.3f ms per timestep'
             % (T, stats(dev), np.median(dev) / T * 1e3, PL * T / np.median(dev) * 1e3, stats(wall), np.median(wall) / T))
        t0 = float(np.mean(time_[T // 2]))
        one = np.empty(PL)

        def slant():
            es.slant(t0, *sets[PL], nodes=NODES, out=one)
            return ctx.eval_kernel_ms()
        sdev, swall = timed(args.reps, slant)
        ok = np.isfinite(one)
        emit('  one slant call at one time: kernel %s, wall %s; slant / resident per timestep: kernel %.0f, wall %.1f; max |resident - '
             'slant| / |slant| at that time: %.1e' % (stats(sdev), stats(swall), np.median(sdev) / (np.median(dev) / T),
                                                      np.median(swall) / (np.median(wall) / T),
                                                      np.max(np.abs(out[T // 2][ok] - one[ok]) / np.abs(one[ok]))))
        eout = np.empty((E, PL))

        def errors():
            r.evaluate_errors(dC, out=eout)
            return ctx.eval_kernel_ms()
        edev, ewall = timed(args.reps, errors)
        emit('errors, %d rays' % PL)
        emit('  evaluate_errors, %d covariances: kernel %s = %.3f ms per covariance; wall %s'
             % (E, stats(edev), np.median(edev) / E, stats(ewall)))
    ctx.eval_timing(False)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
