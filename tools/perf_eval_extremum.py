"""Maxima in three dimensions in one call (Estimate.extremum: vi_eval_extremum_f64, kernel k_extremum_sph) against the only
route there was before it: a host loop of Estimate.__call__ + gradient(frame='enu') + hessian(frame='enu') per iteration and
record on the searches that are still running - three library calls and three walks of the chains per step, uploads every
time -, running the same safeguarded Newton iteration in NumPy; and against the searches along a direction, k_peak_sph
(vi_eval_peak_f64) and k_line_peak_sph (vi_eval_ray_peak_f64), measured in the same run on the columns of the same lattice - the
same walk of ten sums, a 3 x 3 solve and a facet loop per pass here.

Workload: that of tools/perf_eval_peak.py - the default order (N = 144) with the hull of tests/golden/fit_default.npz, T records
(default 64) fitted on the 26 x 100 beams by weighted least squares on the device's own basis - with synth.patch_record in place
of the Chapman record (the layer's peak at 280 km + 1 km per record).  Starts: (a) the recipe of the README - a resident grid of
g x g columns x 13 altitudes, ResidentGrid.peak, estimate.local_maxima - with a ball of 150 km, one call per record; (b) a regular
lattice of n x n columns (default 128 x 128) over 76.5-79.5 N, 255-269 E at 300 km with a ball of 400 km, every column at every
record in one call.  tol 1e-3 m, max_iter 48, max_step an eighth of the radius.  "kernel": the context's event pair around the
kernel (vi_eval_kernel_ms), best of --calls after a warm-up; "wall": the public method from host arrays to host arrays.  The host
loop runs the lattice for --host-records records (default 2) after a warm-up, and the same records go through Estimate.extremum
for the comparison.

    python tools/perf_eval_extremum.py [--n 128] [--grid 48] [--records 64] [--host-records 2] [--calls 3] [--out FILE]
"""
import argparse
import datetime as dt
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
LO, START, HI, TOL, MAX_ITER = 150e3, 300e3, 450e3, 1e-3, 48
RADIUS, RECIPE_RADIUS = 400e3, 150e3


def workload(n, T):
    """(estimate, times, lat, lon): T records of the patch at the default order, and the n x n columns of the lattice."""
    from volumetricinterp_amd import synth
    from volumetricinterp_amd.estimate import Estimate
    f = np.load(os.path.join(HERE, 'tests', 'golden', 'fit_default.npz'))
    cfg = str(f['cfg'])
    lat, lon, alt = synth.beams(*synth.GEOM_C2, seed=0)
    bare = Estimate.from_arrays(np.zeros((1, 144)), np.zeros((1, 1, 1)), [[0., 60.]], f['hull_vert'], cfg)
    A = bare.model.basis(lat, lon, alt)
    recs = [synth.patch_record(lat, lon, alt, hm=280e3 + 1e3 * t) for t in range(T)]
    C = np.stack([np.linalg.lstsq(A / r[1][:, None], r[0] / r[1], rcond=1e-10)[0] for r in recs])
    utime = np.stack([60. * np.arange(T), 60. * np.arange(T) + 60.], axis=1)
    es = Estimate.from_arrays(C, np.zeros((T, 1, 1)), utime, f['hull_vert'], cfg)
    times = [dt.datetime(1970, 1, 1) + dt.timedelta(seconds=60. * t + 30.) for t in range(T)]
    glat, glon = np.meshgrid(np.linspace(76.5, 79.5, n), np.linspace(255., 269., n), indexing='ij')
    return es, times, glat.ravel(), glon.ravel()


def enu_axes(lat, lon):
    """(P, 3, 3): rows east, north, up at the points, in ECEF."""
    sl, cl, so, co = (f(np.radians(v)) for v in (lat, lon) for f in (np.sin, np.cos))
    zero = np.zeros_like(sl)
    return np.stack([np.stack([-so, co, zero], axis=-1), np.stack([-sl * co, -sl * so, cl], axis=-1),
                     np.stack([cl * co, cl * so, sl], axis=-1)], axis=-2)


def newton_steps(A, b, mu):
    """(d (P, 3), mod (P,)): LDL^T solves of A d = b in the order 1, 2, 3 with pivots floored at mu, vectorised."""
    with np.errstate(all='ignore'):
        mod = np.zeros(mu.shape, dtype=bool)

        def floor(p):
            bad = ~(p > mu)
            mod[:] |= bad
            return np.where(bad, mu, p)

        p1 = floor(A[:, 0, 0])
        l21, l31 = A[:, 1, 0] / p1, A[:, 2, 0] / p1
        p2 = floor(A[:, 1, 1] - l21 * A[:, 1, 0])
        t32 = A[:, 2, 1] - l31 * A[:, 1, 0]
        l32 = t32 / p2
        p3 = floor(A[:, 2, 2] - l31 * A[:, 2, 0] - l32 * t32)
        y1 = b[:, 0]
        y2 = b[:, 1] - l21 * y1
        y3 = b[:, 2] - l31 * y1 - l32 * y2
        d3 = y3 / p3
        d2 = y2 / p2 - l32 * d3
        d1 = y1 / p1 - l21 * d2 - l31 * d3
    return np.stack([d1, d2, d3], axis=1), mod


def host_loop(es, times, lat, lon, alt, radius):
    """The iteration of vi_eval_extremum_f64 (kind +1) with the three existing entries and check_hull: (x (T, P, 3), status,
    iterations, rejects, library calls).  Every walk is __call__ + gradient(frame='enu') + hessian(frame='enu') at the geodetic
    points of the searches still running, turned into ECEF on the host."""
    from volumetricinterp_amd import geodesy
    T, P = len(times), lat.size
    x0 = np.stack(geodesy.geodetic2ecef(lat, lon, alt), axis=1)
    X, S = np.full((T, P, 3), np.nan), np.full((T, P), 3, dtype=np.int32)
    IT, RJ, calls = np.zeros((T, P), dtype=np.int32), np.zeros((T, P), dtype=np.int32), 0
    norm = lambda v: np.sqrt(v[:, 0]**2 + v[:, 1]**2 + v[:, 2]**2)
    for t, tm in enumerate(times):
        x, xb, d = x0.copy(), x0.copy(), np.zeros((P, 3))
        fb, gb, delta = np.zeros(P), np.zeros(P), np.full(P, radius / 8.)
        have, done, full = (np.zeros(P, dtype=bool) for _ in range(3))
        it, act = np.zeros(P, dtype=np.int32), np.arange(P)
        while act.size:
            pts = geodesy.ecef2geodetic(*x[act].T)
            A = enu_axes(pts[0], pts[1])
            f = es(tm, *pts, check_hull=False)
            g = np.einsum('pic,pi->pc', A, es.gradient(tm, *pts, check_hull=False, frame='enu'))
            H = np.einsum('pic,pij,pjd->pcd', A, es.hessian(tm, *pts, check_hull=False, frame='enu'), A)
            ins = es.check_hull(*pts) & (norm(x[act] - x0[act]) <= radius)
            calls += 4
            fin = np.isfinite(f) & np.isfinite(g).all(axis=1) & np.isfinite(H).all(axis=(1, 2))
            bad = ~fin | (~have[act] & ~ins)
            stop = ~bad & (done[act] | (it[act] == MAX_ITER))
            st = act[stop]
            X[t, st] = x[st]
            with np.errstate(all='ignore'):
                Hs = -H[stop]
                p1 = Hs[:, 0, 0]
                l21, l31 = Hs[:, 1, 0] / p1, Hs[:, 2, 0] / p1
                p2 = Hs[:, 1, 1] - l21 * Hs[:, 1, 0]
                t32 = Hs[:, 2, 1] - l31 * Hs[:, 1, 0]
                p3 = Hs[:, 2, 2] - l31 * Hs[:, 2, 0] - (t32 / p2) * t32
                definite = (p1 > 0.) & (p2 > 0.) & (p3 > 0.)
            S[t, st] = np.where(~done[st], 2, np.where(full[st] & ins[stop] & definite, 0, 1))
            go = ~bad & ~stop
            j = act[go]
            it[j] += 1
            gn = norm(g[go])
            rej = have[j] & (~ins[go] | ~((f[go] >= fb[j]) | (full[j] & (gn < gb[j]))))
            # reject: backtrack, or stop at the best point once the rejected step was within tol
            r = j[rej]
            RJ[t, r] += 1
            full[r] = False
            dl = norm(d[r])
            end = dl <= TOL
            done[r[end]] = True
            x[r[end]] = xb[r[end]]
            d[r[~end]] *= 0.25
            delta[r[~end]] = 0.25 * dl[~end]
            x[r[~end]] = xb[r[~end]] + d[r[~end]]
            # accept: a Newton step from here
            a = j[~rej]
            k = np.flatnonzero(go)[~rej]
            delta[a] = np.where(have[a], np.minimum(2. * delta[a], radius / 8.), delta[a])
            xb[a], fb[a], gb[a], have[a] = x[a], f[k], gn[~rej], True
            step, mod = newton_steps(-H[k], g[k], gn[~rej] / delta[a])
            zero = gn[~rej] == 0.
            step[zero], mod[zero] = 0., False
            dn = norm(step)
            clip = dn > delta[a]
            with np.errstate(all='ignore'):
                step[clip] *= (delta[a][clip] / dn[clip])[:, None]
            dn[clip] = delta[a][clip]
            full[a] = ~mod & ~clip
            d[a] = step
            done[a] = dn <= TOL
            x[a] = x[a] + step
            act = j
        IT[t] = it
    return X, S, IT, RJ, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=128)
    ap.add_argument('--grid', type=int, default=48)
    ap.add_argument('--records', type=int, default=64)
    ap.add_argument('--host-records', type=int, default=2)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--out')
    a_ = ap.parse_args()
    es, times, lat, lon = workload(a_.n, a_.records)
    from volumetricinterp_amd import _lib, geodesy
    from volumetricinterp_amd.estimate import local_maxima
    ctx, T, P = es.model.ctx, a_.records, lat.size
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    eq, tol = es._hull()
    F = eq.shape[0]
    emit('maxima in three dimensions, N = 144, %d hull facets, %d records of synth.patch_record, tol %g m, max_iter %d, max_step '
         'radius / 8; best of %d timed calls after a warm-up' % (F, T, TOL, MAX_ITER, a_.calls))
    # ---- (a) the recipe: column maps -> local_maxima -> extremum, a call per record
    ga = np.linspace(LO, HI, 13)
    glat, glon, galt = np.meshgrid(np.linspace(76.5, 79.5, a_.grid), np.linspace(255., 269., a_.grid), ga, indexing='ij')
    t0 = time.perf_counter()
    with es.resident_grid(glat, glon, galt) as g:
        ctx.sync()
        t_grid = time.perf_counter() - t0
        g.peak(times[:1])
        t0 = time.perf_counter()
        value, index = g.peak(times)
        t_maps = time.perf_counter() - t0
    t0 = time.perf_counter()
    tt, ii, jj, aa = local_maxima(value, index, ga)
    t_lm = time.perf_counter() - t0
    es.extremum(times[0], glat[ii[:1], jj[:1], 0], glon[ii[:1], jj[:1], 0], aa[:1], RECIPE_RADIUS)
    t0 = time.perf_counter()
    st_r, it_r = [], []
    for t in range(T):
        sel = tt == t
        r = es.extremum(times[t], glat[ii[sel], jj[sel], 0], glon[ii[sel], jj[sel], 0], aa[sel], RECIPE_RADIUS)
        st_r.append(r.status)
        it_r.append(r.iterations)
    t_rec = time.perf_counter() - t0
    st_r, it_r = np.concatenate(st_r), np.concatenate(it_r)
    emit('  recipe: resident grid of %d x %d x 13 points %.1f ms, peak maps of %d records %.1f ms, local_maxima %.1f ms: %d starts '
         '(%.2f per record); Estimate.extremum, a call per record, ball %g km: wall %.1f ms; statuses 0..3 %s; iterations mean '
         '%.2f, max %d' % (a_.grid, a_.grid, 1e3 * t_grid, T, 1e3 * t_maps, 1e3 * t_lm, tt.size, tt.size / T, RECIPE_RADIUS / 1e3,
                            1e3 * t_rec, np.bincount(st_r, minlength=4), it_r[st_r != 3].mean() if (st_r != 3).any() else np.nan,
                            it_r.max() if it_r.size else 0))
    # ---- (b) the lattice: the entry on device copies, and the searches along a direction on the same columns
    x0 = np.ascontiguousarray(np.tile(np.stack(geodesy.geodetic2ecef(lat, lon, np.full(P, START)))[:, None, :], (1, T, 1)))
    ra = np.stack(geodesy.geodetic2ecef(lat, lon, np.full(P, LO)))
    rb = np.stack(geodesy.geodetic2ecef(lat, lon, np.full(P, HI)))
    with ctx.scope() as dev:
        dx, dr, dC, dE = dev.up(x0), dev.up(np.full(T * P, RADIUS)), dev.up(es.Coeffs), dev.up(eq)
        dlat, dlon = dev.up(np.tile(lat, T)), dev.up(np.tile(lon, T))
        dcol = [dev.up(np.full(T * P, v)) for v in (START, LO, HI)]
        da, db = dev.up(np.ascontiguousarray(ra)), dev.up(np.ascontiguousarray(rb))
        dray = [dev.up(np.full(T * P, v)) for v in (START - LO, 0., HI - LO)]
        dO, dS, dI = dev.empty((13, T, P)), dev.empty((T, P), np.int32), dev.empty((T, P), np.int32)
        h, L = es.model.handle(), _lib.lib
        runs = (('extremum', lambda: L.vi_eval_extremum_f64(h, T, P, dx.ptr, dr.ptr, dC.ptr, dE.ptr, F, tol, 1, 0., MAX_ITER, TOL,
                                                            dO.ptr, dS.ptr, dI.ptr)),
                ('extremum, no hull', lambda: L.vi_eval_extremum_f64(h, T, P, dx.ptr, dr.ptr, dC.ptr, None, 0, 0., 1, 0., MAX_ITER,
                                                                     TOL, dO.ptr, dS.ptr, dI.ptr)),
                ('peak', lambda: L.vi_eval_peak_f64(h, T, P, dlat.ptr, dlon.ptr, *(v.ptr for v in dcol), dC.ptr, dE.ptr, F, tol, 1,
                                                    MAX_ITER, TOL, dO.ptr, dS.ptr, dI.ptr)),
                ('ray_peak', lambda: L.vi_eval_ray_peak_f64(h, T, P, da.ptr, db.ptr, *(v.ptr for v in dray), dC.ptr, dE.ptr, F, tol,
                                                            1, MAX_ITER, TOL, dO.ptr, dS.ptr, dI.ptr)))
        ctx.eval_timing(True)
        res = {}
        for name, run in runs:
            _lib.check(run(), name)
            ctx.sync()
            call = kern = np.inf
            for _ in range(a_.calls):
                ctx.timer_start()
                _lib.check(run(), name)
                call = min(call, ctx.timer_stop_ms())
                kern = min(kern, ctx.eval_kernel_ms())
            res[name] = call, kern, dS.download().ravel(), dI.download().ravel()
        ctx.eval_timing(False)
    emit('  lattice: %d x %d = %d columns at %g km x %d records in one call, ball %g km' % (a_.n, a_.n, P, START / 1e3, T,
                                                                                          RADIUS / 1e3))
    ns = {}
    for name, (call, kern, st, it) in res.items():
        ran = st != 3
        walks = (it + 1)[ran].sum()
        ns[name] = 1e6 * kern / walks
        emit('  %-18s call %9.3f ms, kernel %9.3f ms = %8.1f ns per search = %7.2f ns per search and walk; statuses 0..3 %s; '
             'iterations per search: mean %.2f, max %d' % (name, call, kern, 1e6 * kern / max(ran.sum(), 1), ns[name],
                                                           np.bincount(st, minlength=4), it[ran].mean(), it[ran].max()))
    emit('  a walk of k_extremum_sph / of k_line_peak_sph: %.3f;  / of k_peak_sph: %.3f;  without the facet loop / of '
         'k_line_peak_sph: %.3f' % (ns['extremum'] / ns['ray_peak'], ns['extremum'] / ns['peak'],
                                    ns['extremum, no hull'] / ns['ray_peak']))
    # ---- host to host, and the host loop it replaces, on the first records
    Th = min(a_.host_records, T)
    es.extremum(times[:1], lat, lon, START, RADIUS)
    t0 = time.perf_counter()
    full = es.extremum(times, lat, lon, START, RADIUS)
    wall = time.perf_counter() - t0
    t0 = time.perf_counter()
    r = es.extremum(times[:Th], lat, lon, START, RADIUS)
    wall_h = time.perf_counter() - t0
    assert np.array_equal(full.status.ravel(), res['extremum'][2])
    emit('  Estimate.extremum, host arrays in and out: wall %9.1f ms for %d records, %9.1f ms for %d' % (1e3 * wall, T, 1e3 * wall_h, Th))
    host_loop(es, times[:1], lat[:256], lon[:256], np.full(256, START), RADIUS)
    ctx.sync()
    t0 = time.perf_counter()
    X, S, IT, RJ, calls = host_loop(es, times[:Th], lat, lon, np.full(P, START), RADIUS)
    wall_l = time.perf_counter() - t0
    both = (S == 0) & (r.status == 0)
    Xd = np.stack(geodesy.geodetic2ecef(r.gdlat[both], r.gdlon[both], r.gdalt[both]), axis=1)
    dist = np.sqrt(((Xd - X[both])**2).sum(axis=1))
    ran = S != 3
    emit('  host loop of __call__ / gradient / hessian / check_hull, %d records: wall %9.1f ms in %d library calls; statuses 0..3 %s '
         '(Estimate.extremum: %s), the same status at %d of %d searches; status 0 in both: %d, positions within %.2e m (median '
         '%.2e m); rejects per search: mean %.2f, max %d; iterations mean %.2f'
         % (Th, 1e3 * wall_l, calls, np.bincount(S.ravel(), minlength=4), np.bincount(r.status.ravel(), minlength=4),
            (S == r.status).sum(), S.size, both.sum(), dist.max() if dist.size else np.nan,
            np.median(dist) if dist.size else np.nan, RJ[ran].mean(), RJ[ran].max(), IT[ran].mean()))
    emit('  host loop wall / Estimate.extremum wall, %d records: %.1f' % (Th, wall_l / wall_h))
    if a_.out:
        with open(a_.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
