"""Peaks and level crossings along straight rays in one call each (Estimate.ray_peak, Estimate.ray_level: vi_eval_ray_peak_f64
and vi_eval_ray_level_f64, kernels k_line_peak_sph and k_line_level_sph) against the only route there was before them: a host
loop of Estimate.__call__ + gradient (+ hessian) per iteration and record on the rays that are still searching, running the
same safeguarded Newton iterations in NumPy; and against the column kernels k_peak_sph and k_level_sph, measured in the same run
on vertical columns of the same count - the same walks, a geodetic step and a byte mask there, an ECEF point and a facet loop
per lane here.

Workload: the model and records of tools/perf_eval_peak.py - the default order (N = 144) with the hull of
tests/golden/fit_default.npz, T records (default 64) of synth's Chapman layer -, n x n rays (default 128 x 128) from the ground
site of synth.beams, (78, 262, 0), elevations 35 to 90 degrees x azimuths 0 to 360, each 1000 km long.  The brackets come from
the recipe of the README: ray_samples (64 samples on the chord inside the hull) -> resident_grid -> peak / crossing ->
ray_peak_brackets / ray_level_brackets; the level is half the sampled peak of the ray, its first rising crossing.  "kernel": the
context's event pair around the kernel (vi_eval_kernel_ms), best of --calls after a warm-up; "wall": the public method from
host arrays to host arrays.  The host loop runs once after a warm-up of one record.

    python tools/perf_eval_ray.py [--n 128] [--records 64] [--calls 3] [--samples 64] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from perf_eval_peak import HI, LO, MAX_ITER, START, TOL, workload      # noqa: E402

SITE = (78., 262.)
RANGE = 1000e3


def beams(n):
    """(a, b), (n * n, 3) each in ECEF metres: the rays from the site, elevations 35 to 90 degrees x n azimuths."""
    from volumetricinterp_amd import geodesy
    el, az = np.meshgrid(np.radians(np.linspace(35., 90., n)), np.radians(np.linspace(0., 360., n, endpoint=False)), indexing='ij')
    la, lo = np.radians(SITE)
    east = np.array([-np.sin(lo), np.cos(lo), 0.])
    north = np.array([-np.sin(la) * np.cos(lo), -np.sin(la) * np.sin(lo), np.cos(la)])
    up = np.array([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)])
    d = (np.cos(el) * np.sin(az)).reshape(-1, 1) * east + (np.cos(el) * np.cos(az)).reshape(-1, 1) * north + \
        np.sin(el).reshape(-1, 1) * up
    a = np.tile(np.array(geodesy.geodetic2ecef(SITE[0], SITE[1], 0.)).reshape(1, 3), (n * n, 1))
    return a, a + RANGE * d


def host_loop(es, times, a, b, peak_args, level_args):
    """Both iterations with the existing entries: (peak distances (T, P), peak status, level distances, level status, library
    calls).  Every walk is __call__ + gradient(frame='model') (+ hessian(frame='model') for the peak) at the geodetic points of
    the rays still searching, the direction turned into the model's frame on the host."""
    T, P = len(times), a.shape[0]
    q = dict(a=np.ascontiguousarray(a.T), b=np.ascontiguousarray(b.T))
    calls = 0

    def walk(tm, i, s, hess):
        ok = np.zeros(P, dtype=bool)
        ok[i] = True
        pts, w = es._ray_frame(q, ok, s)
        f = es(tm, *pts, check_hull=False)
        d1 = np.einsum('pc,pc->p', es.gradient(tm, *pts, check_hull=False), w)
        d2 = np.einsum('pc,pcd,pd->p', w, es.hessian(tm, *pts, check_hull=False), w) if hess else None
        return f, d1, d2, (4 if hess else 3)

    s0, plo, phi_ = peak_args
    lev, llo, lhi = level_args
    SP, StP = np.full((T, P), np.nan), np.full((T, P), 3, dtype=np.int32)
    SL, StL = np.full((T, P), np.nan), np.full((T, P), 3, dtype=np.int32)
    for t, tm in enumerate(times):
        # ---- the peak
        idx = np.flatnonzero(np.isfinite(s0[t]) & np.isfinite(plo[t]) & np.isfinite(phi_[t]))
        s, lb, ub = s0[t][idx].copy(), plo[t][idx].copy(), phi_[t][idx].copy()
        act, done, it = np.arange(idx.size), np.zeros(idx.size, dtype=bool), 0
        while act.size:
            f, d1, d2, n = walk(tm, idx[act], s[act], True)
            calls += n
            fin = np.isfinite(f) & np.isfinite(d1) & np.isfinite(d2)
            stop = ~fin | done[act] | (it == MAX_ITER)
            st = act[stop & fin]
            SP[t, idx[st]] = s[st]
            d2s = d2[stop & fin]
            StP[t, idx[st]] = np.where(~done[st], 2, np.where((d2s < 0.) & (np.abs(s[st] - plo[t][idx[st]]) > TOL)
                                                              & (np.abs(s[st] - phi_[t][idx[st]]) > TOL), 0, 1))
            go = ~stop
            j = act[go]
            it += 1
            up = d1[go] > 0.
            lb[j[up]], ub[j[~up]] = s[j[up]], s[j[~up]]
            with np.errstate(all='ignore'):
                sn = np.where(d2[go] < 0., s[j] - d1[go] / d2[go], np.nan)
                sn = np.where((lb[j] < sn) & (sn < ub[j]), sn, 0.5 * (lb[j] + ub[j]))
            done[j] = np.abs(sn - s[j]) <= TOL
            s[j] = sn
            act = j
        # ---- the level
        with np.errstate(invalid='ignore'):
            idx = np.flatnonzero(np.isfinite(lev[t]) & np.isfinite(llo[t]) & np.isfinite(lhi[t]) & (llo[t] < lhi[t]))
        if idx.size == 0:
            continue
        lb, ub, Lv = llo[t][idx].copy(), lhi[t][idx].copy(), lev[t][idx]
        wa, wb = walk(tm, idx, lb, False), walk(tm, idx, ub, False)
        calls += wa[3] + wb[3]
        fa, fb = wa[0] - Lv, wb[0] - Lv
        fin = np.isfinite(fa) & np.isfinite(fb)
        same = fin & ((fa > 0.) == (fb > 0.)) & (fa != 0.) & (fb != 0.)
        StL[t, idx[same]] = 1
        for end, f0 in ((lb, fa), (ub, fb)):
            hit = fin & (f0 == 0.) & (StL[t, idx] == 3)
            SL[t, idx[hit]], StL[t, idx[hit]] = end[hit], 0
        act = np.flatnonzero(fin & ~same & (fa != 0.) & (fb != 0.))
        sa = fa > 0.
        with np.errstate(all='ignore'):
            s = lb - fa * (ub - lb) / (fb - fa)
        s = np.where((lb < s) & (s < ub), s, 0.5 * (lb + ub))
        done, it = np.zeros(idx.size, dtype=bool), 0
        while act.size:
            f, d1, _, n = walk(tm, idx[act], s[act], False)
            calls += n
            ph = f - Lv[act]
            fin = np.isfinite(ph) & np.isfinite(d1)
            stop = ~fin | (ph == 0.) | done[act] | (it == MAX_ITER)
            st = act[stop & fin]
            SL[t, idx[st]] = s[st]
            StL[t, idx[st]] = np.where((ph[stop & fin] == 0.) | done[st], 0, 2)
            go = ~stop
            j = act[go]
            it += 1
            left = (ph[go] > 0.) == sa[j]
            lb[j[left]], ub[j[~left]] = s[j[left]], s[j[~left]]
            with np.errstate(all='ignore'):
                sn = np.where(d1[go] != 0., s[j] - ph[go] / d1[go], np.nan)
                sn = np.where((lb[j] < sn) & (sn < ub[j]), sn, 0.5 * (lb[j] + ub[j]))
            done[j] = np.abs(sn - s[j]) <= TOL
            s[j] = sn
            act = j
    return SP, StP, SL, StL, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=128)
    ap.add_argument('--records', type=int, default=64)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--samples', type=int, default=64)
    ap.add_argument('--out')
    a_ = ap.parse_args()
    es, times, lat, lon = workload(HERE, a_.n, a_.records)
    from volumetricinterp_amd import _lib
    from volumetricinterp_amd.estimate import ray_level_brackets, ray_peak_brackets, ray_samples
    ctx, T = es.model.ctx, a_.records
    a, b = beams(a_.n)
    P = a.shape[0]
    start, end = tuple(a.T), tuple(b.T)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    eq, tol = es._hull()
    F = eq.shape[0]
    # ---- the bracket stage: the recipe
    t0 = time.perf_counter()
    dist, slat, slon, salt = ray_samples(eq, tol, start, end, a_.samples, coords='ecef')
    t_samples = time.perf_counter() - t0
    t0 = time.perf_counter()
    with es.resident_grid(slat, slon, salt) as g:
        ctx.sync()
        t_grid = time.perf_counter() - t0
        g.peak(times[:1])
        t0 = time.perf_counter()
        value, index = g.peak(times)
        level = 0.5 * value
        cross = g.crossing(times, level, which='first', direction='up')
        t_maps = time.perf_counter() - t0
    s0, plo, phi_ = ray_peak_brackets(dist, index)
    llo, lhi = ray_level_brackets(dist, cross)
    # ---- the two entries on device copies, and the column kernels on as many vertical columns
    pk = es.peak_height(times, lat[:P], lon[:P], START, LO, HI)
    clevel, chi = 0.5 * pk.value, pk.height
    Q = min(P, lat.size)
    with ctx.scope() as dev:
        da, db, dC, dE = dev.up(np.ascontiguousarray(a.T)), dev.up(np.ascontiguousarray(b.T)), dev.up(es.Coeffs), dev.up(eq)
        dpk = [dev.up(np.ascontiguousarray(v)) for v in (s0, plo, phi_)]
        dends, dlev = dev.up(np.stack((llo, lhi))), dev.up(np.ascontiguousarray(level))
        dlat, dlon = dev.up(np.tile(lat[:Q], 2 * T)), dev.up(np.tile(lon[:Q], 2 * T))
        dcpk = [dev.up(np.full(T * Q, v)) for v in (START, LO, HI)]
        dcends, dclev = dev.up(np.stack((np.full((T, Q), LO), chi))), dev.up(clevel)
        dO, dS, dI = dev.empty((4, T, P)), dev.empty((T, P), np.int32), dev.empty((T, P), np.int32)
        h = es.model.handle()
        L = _lib.lib
        runs = (
            ('ray_peak', lambda: L.vi_eval_ray_peak_f64(h, T, P, da.ptr, db.ptr, *(v.ptr for v in dpk), dC.ptr, dE.ptr, F, tol, 1,
                                                        MAX_ITER, TOL, dO.ptr, dS.ptr, dI.ptr)),
            ('ray_level', lambda: L.vi_eval_ray_level_f64(h, T, P, da.ptr, db.ptr, dends.ptr, dlev.ptr, dC.ptr, dE.ptr, F, tol,
                                                          MAX_ITER, TOL, dO.ptr, dS.ptr, dI.ptr)),
            ('peak', lambda: L.vi_eval_peak_f64(h, T, Q, dlat.ptr, dlon.ptr, *(v.ptr for v in dcpk), dC.ptr, dE.ptr, F, tol, 1,
                                                MAX_ITER, TOL, dO.ptr, dS.ptr, dI.ptr)),
            ('level', lambda: L.vi_eval_level_f64(h, T, Q, dlat.ptr, dlon.ptr, dcends.ptr, dclev.ptr, dC.ptr, dE.ptr, F, tol,
                                                  MAX_ITER, TOL, dO.ptr, dS.ptr, dI.ptr)))
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
            res[name] = call, kern, dS.download(), dI.download()
        ctx.eval_timing(False)
    # ---- host to host
    es.ray_peak(times[:1], start, end, s0[:1], plo[:1], phi_[:1], coords='ecef')
    t0 = time.perf_counter()
    rp = es.ray_peak(times, start, end, s0, plo, phi_, coords='ecef')
    wall_p = time.perf_counter() - t0
    t0 = time.perf_counter()
    rl = es.ray_level(times, start, end, level, llo, lhi, coords='ecef')
    wall_l = time.perf_counter() - t0
    emit('peaks and half-peak crossings along rays, N = 144, %d x %d = %d rays x %d records, %d hull facets, rays of %g km from '
         '(%g, %g, 0), elevations 35 to 90 degrees, %d samples per ray, tol %g m; best of %d timed calls after a warm-up'
         % (a_.n, a_.n, P, T, F, RANGE / 1e3, SITE[0], SITE[1], a_.samples, TOL, a_.calls))
    emit('  bracket stage: ray_samples %.1f ms on the host, resident grid of %d points %.1f ms, peak and crossing maps of %d '
         'records %.1f ms' % (1e3 * t_samples, dist.size, 1e3 * t_grid, T, 1e3 * t_maps))
    ns = {}
    for name, extra, label in (('ray_peak', 1, 'ray'), ('ray_level', 3, 'ray'), ('peak', 1, 'column'), ('level', 3, 'column')):
        call, kern, st, it = res[name]
        st, it = st.ravel()[:T * (P if 'ray' in name else Q)], it.ravel()[:T * (P if 'ray' in name else Q)]
        ran = st != 3
        walks = (np.where(st == 1, 2, it + 3) if extra == 3 else it + 1)[ran].sum()
        ns[name] = 1e6 * kern / walks
        emit('  vi_eval_%-14s call %9.3f ms, kernel %9.3f ms = %7.2f ns per %s and walk; statuses 0..3 %s; iterations per searching '
             '%s: mean %.2f, max %d' % (name + '_f64', call, kern, ns[name], label, np.bincount(st, minlength=4), label,
                                        it[ran].mean(), it[ran].max()))
    assert np.array_equal(res['ray_peak'][2].ravel()[:T * P], rp.status.ravel())
    assert np.array_equal(res['ray_level'][2].ravel()[:T * P], rl.status.ravel())
    emit('  a walk of k_line_peak_sph / of k_peak_sph: %.3f;  of k_line_level_sph / of k_level_sph: %.3f'
         % (ns['ray_peak'] / ns['peak'], ns['ray_level'] / ns['level']))
    emit('  Estimate.ray_peak, host arrays in and out: wall %9.1f ms;  Estimate.ray_level: wall %9.1f ms' % (1e3 * wall_p, 1e3 * wall_l))
    host_loop(es, times[:1], a, b, (s0[:1], plo[:1], phi_[:1]), (level[:1], llo[:1], lhi[:1]))
    ctx.sync()
    t0 = time.perf_counter()
    SP, StP, SL, StL, calls = host_loop(es, times, a, b, (s0, plo, phi_), (level, llo, lhi))
    wall_h = time.perf_counter() - t0
    bp, bl = (StP == 0) & (rp.status.reshape(T, P) == 0), (StL == 0) & (rl.status.reshape(T, P) == 0)
    dp, dl = np.abs(SP[bp] - rp.distance.reshape(T, P)[bp]), np.abs(SL[bl] - rl.distance.reshape(T, P)[bl])
    emit('  host loop of __call__ / gradient / hessian (no hull test): wall %9.1f ms in %d library calls; status 0 in both: %d peaks '
         'within %.2e m, %d crossings within %.2e m' % (1e3 * wall_h, calls, bp.sum(), dp.max() if dp.size else np.nan, bl.sum(),
                                                        dl.max() if dl.size else np.nan))
    emit('  host loop wall / (ray_peak + ray_level wall): %.1f' % (wall_h / (wall_p + wall_l)))
    if a_.out:
        with open(a_.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
