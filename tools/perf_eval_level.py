"""Level crossings in one call (Estimate.level_height: vi_eval_level_f64, kernel k_level_sph) against the only route there was
before it: a host loop of Estimate.__call__ + gradient(frame='enu') per iteration and record - two library calls and two walks
of the chains per step, uploads every time - running the same safeguarded Newton iteration in NumPy on the columns that are
still searching; and against k_peak_sph, whose walk keeps ten sums where the gradient walk of k_level_sph keeps four.

Workload: that of tools/perf_eval_peak.py - the default order (N = 144) with the hull of tests/golden/fit_default.npz, n x n
columns (default 128 x 128), T records (default 64) of synth's Chapman layer -, and per column and record the bottomside
half-peak height: the level is half the value of the layer's peak (Estimate.peak_height, status 0), the bracket 150 km to the
peak's height, tol 1e-3 m, max_iter 48; a column without an interior peak has a NaN level and bracket (status 3).  One process
times the new entry - "kernel": the context's event pair around k_level_sph (vi_eval_kernel_ms), "call": events around the
whole entry with the hull pass of both ends, on device copies, best of --calls after a warm-up; "wall": Estimate.level_height
from host arrays to host arrays - and k_peak_sph on the same columns.  The host loop runs in a child process - with --parent
TREE on that tree's library, which need not have the new entry - once after a warm-up of one record, and hands its heights back
for comparison.

    python tools/perf_eval_level.py [--n 128] [--records 64] [--calls 3] [--parent TREE] [--out FILE]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from perf_eval_peak import HI, LO, MAX_ITER, START, TOL, workload      # noqa: E402


def host_loop(es, times, lat, lon, level, hi):
    """The iteration of vi_eval_level_f64 with the two existing entries: (heights (T, Q), status, library calls)."""
    T, Q = len(times), lat.size
    H, S, calls = np.full((T, Q), np.nan), np.full((T, Q), 3, dtype=np.int32), 0

    def walk(tm, i, h):
        pts = lat[i], lon[i], h
        return es(tm, *pts, check_hull=False), es.gradient(tm, *pts, check_hull=False, frame='enu')[:, 2]

    for t, tm in enumerate(times):
        with np.errstate(invalid='ignore'):
            ok = np.isfinite(level[t]) & np.isfinite(hi[t]) & (LO < hi[t])
        ok[ok] = es.check_hull(lat[ok], lon[ok], np.full(ok.sum(), LO)) & es.check_hull(lat[ok], lon[ok], hi[t][ok])
        calls += 2
        idx = np.flatnonzero(ok)
        if idx.size == 0:
            continue
        a, b, Lv = np.full(idx.size, LO), hi[t][idx].copy(), level[t][idx]
        fa, fb = walk(tm, idx, a)[0] - Lv, walk(tm, idx, b)[0] - Lv
        calls += 4
        fin = np.isfinite(fa) & np.isfinite(fb)
        same = fin & ((fa > 0.) == (fb > 0.)) & (fa != 0.) & (fb != 0.)
        S[t, idx[same]] = 1
        for end, f0 in ((a, fa), (b, fb)):
            hit = fin & (f0 == 0.) & (S[t, idx] == 3)
            H[t, idx[hit]], S[t, idx[hit]] = end[hit], 0
        act = np.flatnonzero(fin & ~same & (fa != 0.) & (fb != 0.))
        sa = fa > 0.
        with np.errstate(all='ignore'):
            h = a - fa * (b - a) / (fb - fa)
        h = np.where((a < h) & (h < b), h, 0.5 * (a + b))
        done, it = np.zeros(idx.size, dtype=bool), 0
        while act.size:
            f, d1 = walk(tm, idx[act], h[act])
            calls += 2
            phi = f - Lv[act]
            fin = np.isfinite(phi) & np.isfinite(d1)
            stop = ~fin | (phi == 0.) | done[act] | (it == MAX_ITER)
            st = act[stop & fin]
            H[t, idx[st]] = h[st]
            S[t, idx[st]] = np.where((phi[stop & fin] == 0.) | done[st], 0, 2)
            go = ~stop
            j = act[go]
            it += 1
            left = (phi[go] > 0.) == sa[j]
            a[j[left]], b[j[~left]] = h[j[left]], h[j[~left]]
            with np.errstate(all='ignore'):
                hn = np.where(d1[go] != 0., h[j] - phi[go] / d1[go], np.nan)
                hn = np.where((a[j] < hn) & (hn < b[j]), hn, 0.5 * (a[j] + b[j]))
            done[j] = np.abs(hn - h[j]) <= TOL
            h[j] = hn
            act = j
    return H, S, calls


def child(a):
    es, times, lat, lon = workload(a.child, a.n, a.records)
    w = np.load(a.load)
    host_loop(es, times[:1], lat, lon, w['level'], w['hi'])               # warm-up
    es.model.ctx.sync()
    t0 = time.perf_counter()
    H, S, calls = host_loop(es, times, lat, lon, w['level'], w['hi'])
    wall = time.perf_counter() - t0
    np.savez(a.save, H=H, S=S, calls=calls, wall=wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=128)
    ap.add_argument('--records', type=int, default=64)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--parent', help='source tree with a built library for the host loop (default: this tree)')
    ap.add_argument('--out')
    ap.add_argument('--child', help=argparse.SUPPRESS)
    ap.add_argument('--load', help=argparse.SUPPRESS)
    ap.add_argument('--save', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    es, times, lat, lon = workload(HERE, a.n, a.records)
    from volumetricinterp_amd import _lib
    ctx, T, Q = es.model.ctx, a.records, lat.size
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    pk = es.peak_height(times, lat, lon, START, LO, HI)
    level, hi = 0.5 * pk.value, pk.height                                  # NaN where there is no interior peak
    eq, tol = es._hull()
    F = eq.shape[0]
    with ctx.scope() as dev:
        dlat, dlon, dC = dev.up(np.tile(lat, 2 * T)), dev.up(np.tile(lon, 2 * T)), dev.up(es.Coeffs)
        dends, dlev = dev.up(np.stack((np.full((T, Q), LO), hi))), dev.up(level)
        dpk = [dev.up(np.full(T * Q, v)) for v in (START, LO, HI)]
        dE, dO, dS, dI = dev.up(eq), dev.empty((4, T, Q)), dev.empty((T, Q), np.int32), dev.empty((T, Q), np.int32)
        h = es.model.handle()

        def run_level():
            _lib.check(_lib.lib.vi_eval_level_f64(h, T, Q, dlat.ptr, dlon.ptr, dends.ptr, dlev.ptr, dC.ptr, dE.ptr, F, tol,
                                                  MAX_ITER, TOL, dO.ptr, dS.ptr, dI.ptr), 'vi_eval_level_f64')

        def run_peak():
            _lib.check(_lib.lib.vi_eval_peak_f64(h, T, Q, dlat.ptr, dlon.ptr, *(v.ptr for v in dpk), dC.ptr, dE.ptr, F, tol, 1,
                                                 MAX_ITER, TOL, dO.ptr, dS.ptr, dI.ptr), 'vi_eval_peak_f64')

        ctx.eval_timing(True)
        res = {}
        for name, run in (('level', run_level), ('peak', run_peak)):
            run()
            ctx.sync()
            call = kern = np.inf
            for _ in range(a.calls):
                ctx.timer_start()
                run()
                call = min(call, ctx.timer_stop_ms())
                kern = min(kern, ctx.eval_kernel_ms())
            res[name] = call, kern, dS.download(), dI.download()
        ctx.eval_timing(False)
    es.level_height(times[:1], lat, lon, level[:1], LO, hi[:1])
    t0 = time.perf_counter()
    r = es.level_height(times, lat, lon, level, LO, hi)
    wall = time.perf_counter() - t0
    call, kern, st, it = res['level']
    assert np.array_equal(st, r.status)
    ran = st != 3
    walks = np.where(st == 1, 2, it + 3)[ran].sum()
    emit('bottomside half-peak heights, N = 144, %d x %d = %d columns x %d records, %d hull facets (%.1f %% of the columns have an '
         'interior peak and both ends inside), level half the peak value in (%g km, peak height), tol %g m; best of %d timed calls '
         'after a warm-up' % (a.n, a.n, Q, T, F, 100. * ran.mean(), LO / 1e3, TOL, a.calls))
    emit('  statuses 0..3 of Estimate.level_height: %s; iterations of the columns that searched: mean %.2f, max %d'
         % (np.bincount(st.ravel(), minlength=4), it[ran].mean(), it[ran].max()))
    ns_level = 1e6 * kern / walks
    emit('  vi_eval_level_f64 with the hull    call %9.3f ms, kernel %9.3f ms = %7.2f ns per column and walk (it + 3 walks, 2 with '
         'status 1)' % (call, kern, ns_level))
    cp, kp, sp, ip = res['peak']
    ns_peak = 1e6 * kp / (ip[sp != 3] + 1).sum()
    emit('  vi_eval_peak_f64 with the hull     call %9.3f ms, kernel %9.3f ms = %7.2f ns per column and walk (it + 1 walks, mean '
         '%.2f iterations)' % (cp, kp, ns_peak, ip[sp != 3].mean()))
    emit('  a gradient walk of k_level_sph / a value-gradient-Hessian walk of k_peak_sph, per column: %.2f' % (ns_level / ns_peak))
    emit('  Estimate.level_height, host arrays in and out: wall %9.1f ms' % (1e3 * wall))
    tree = os.path.abspath(a.parent) if a.parent else HERE
    with tempfile.TemporaryDirectory() as tmp:
        load, save = os.path.join(tmp, 'workload.npz'), os.path.join(tmp, 'host_loop.npz')
        np.savez(load, level=level, hi=hi)
        subprocess.run([sys.executable, os.path.abspath(__file__), '--child', tree, '--load', load, '--save', save, '--n', str(a.n),
                        '--records', str(T)], check=True, cwd=tree, env=dict(os.environ, PYTHONPATH=tree))
        hl = np.load(save)
        both = (hl['S'] == 0) & (st == 0)
        diff = np.abs(hl['H'][both] - r.height[both])
        emit('  host loop of __call__ / gradient on %s library: wall %9.1f ms in %d library calls; %d columns with status 0 in '
             'both, heights differ by at most %.2e m'
             % ("the parent's" if a.parent else "this tree's", 1e3 * float(hl['wall']), int(hl['calls']), int(both.sum()),
                float(diff.max()) if diff.size else float('nan')))
        emit('  host loop wall / level_height wall: %.1f' % (float(hl['wall']) / wall))
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
