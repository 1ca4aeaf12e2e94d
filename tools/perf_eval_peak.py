"""Sub-grid layer peaks in one call (Estimate.peak_height: vi_eval_peak_f64, kernel k_peak_sph) against the only route there was
before it: a host loop of Estimate.__call__ + gradient(frame='enu') + hessian(frame='enu') per iteration and record - three
library calls and three walks of the chains per step, uploads every time - running the same safeguarded Newton iteration in
NumPy on the columns that are still searching.

Workload: the default order (N = 144) with the hull of tests/golden/fit_default.npz, n x n columns (default 128 x 128) over
76.5-79.5 N, 255-269 E, T records (default 64): synth's Chapman layer with its peak at 280 km + 1 km per record, fitted on the
26 x 100 beams by weighted least squares on the device's own basis.  Every column starts at 300 km in the bracket 150-450 km,
tol 1e-3 m, max_iter 48.  One process times the new entry - "kernel": the context's event pair around k_peak_sph
(vi_eval_kernel_ms), "call": events around the whole entry with the hull pass, on device copies, best of --calls after a
warm-up; "wall": Estimate.peak_height from host arrays to host arrays.  The host loop runs in a child process - with --parent
TREE in that tree, on its library, which need not have the new entry - once after a warm-up of one record, and hands its heights
back for comparison.

    python tools/perf_eval_peak.py [--n 128] [--records 64] [--calls 3] [--parent TREE] [--out FILE]
"""
import argparse
import datetime as dt
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, START, HI, TOL, MAX_ITER = 150e3, 300e3, 450e3, 1e-3, 48


def workload(repo, n, T):
    """(estimate, times, lat, lon): built with the package of the tree `repo` - the same numbers in either tree."""
    sys.path.insert(0, repo)
    from volumetricinterp_amd import synth
    from volumetricinterp_amd.estimate import Estimate
    f = np.load(os.path.join(repo, 'tests', 'golden', 'fit_default.npz'))
    cfg = str(f['cfg'])
    lat, lon, alt = synth.beams(*synth.GEOM_C2, seed=0)
    bare = Estimate.from_arrays(np.zeros((1, 144)), None, [[0., 60.]], f['hull_vert'], cfg)
    A = bare.model.basis(lat, lon, alt)
    recs = [synth.chapman_record(alt, hm=280e3 + 1e3 * t) for t in range(T)]
    C = np.stack([np.linalg.lstsq(A / r[1][:, None], r[0] / r[1], rcond=1e-10)[0] for r in recs])
    utime = np.stack([60. * np.arange(T), 60. * np.arange(T) + 60.], axis=1)
    es = Estimate.from_arrays(C, np.zeros((T, 1, 1)), utime, f['hull_vert'], cfg)
    times = [dt.datetime(1970, 1, 1) + dt.timedelta(seconds=60. * t + 30.) for t in range(T)]
    glat, glon = np.meshgrid(np.linspace(76.5, 79.5, n), np.linspace(255., 269., n), indexing='ij')
    return es, times, glat.ravel(), glon.ravel()


def host_loop(es, times, lat, lon):
    """The iteration of vi_eval_peak_f64 with the three existing entries: (heights (T, Q), status, library calls)."""
    T, Q = len(times), lat.size
    H, S, calls = np.full((T, Q), np.nan), np.full((T, Q), 3, dtype=np.int32), 0
    for t, tm in enumerate(times):
        inside = es.check_hull(lat, lon, np.full(Q, START))
        calls += 1
        idx = np.flatnonzero(inside)
        h, a, b = np.full(idx.size, START), np.full(idx.size, LO), np.full(idx.size, HI)
        done, it = np.zeros(idx.size, dtype=bool), 0
        act = np.arange(idx.size)
        while act.size:
            pts = lat[idx[act]], lon[idx[act]], h[act]
            f = es(tm, *pts, check_hull=False)
            d1 = es.gradient(tm, *pts, check_hull=False, frame='enu')[:, 2]
            d2 = es.hessian(tm, *pts, check_hull=False, frame='enu')[:, 2, 2]
            calls += 3
            fin = np.isfinite(f) & np.isfinite(d1) & np.isfinite(d2)
            stop = ~fin | done[act] | (it == MAX_ITER)
            st = act[stop & fin]
            H[t, idx[st]] = h[st]
            S[t, idx[st]] = np.where(~done[st], 2, np.where((d2[stop & fin] < 0.) & (np.abs(h[st] - LO) > TOL)
                                                             & (np.abs(h[st] - HI) > TOL), 0, 1))
            go = ~stop
            j = act[go]
            it += 1
            up = d1[go] > 0.
            a[j[up]], b[j[~up]] = h[j[up]], h[j[~up]]
            with np.errstate(all='ignore'):
                hn = np.where(d2[go] < 0., h[j] - d1[go] / d2[go], np.nan)
                hn = np.where((a[j] < hn) & (hn < b[j]), hn, 0.5 * (a[j] + b[j]))
            done[j] = np.abs(hn - h[j]) <= TOL
            h[j] = hn
            act = j
    return H, S, calls


def child(a):
    es, times, lat, lon = workload(a.child, a.n, a.records)
    host_loop(es, times[:1], lat, lon)                                  # warm-up
    es.model.ctx.sync()
    t0 = time.perf_counter()
    H, S, calls = host_loop(es, times, lat, lon)
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

    eq, tol = es._hull()
    with ctx.scope() as dev:
        d = [dev.up(v) for v in (np.tile(lat, T), np.tile(lon, T), np.full(T * Q, START), np.full(T * Q, LO), np.full(T * Q, HI),
                                 es.Coeffs)]
        dE, dO, dS, dI = dev.up(eq), dev.empty((4, T, Q)), dev.empty((T, Q), np.int32), dev.empty((T, Q), np.int32)

        def run(F):
            _lib.check(_lib.lib.vi_eval_peak_f64(es.model.handle(), T, Q, *(v.ptr for v in d), dE.ptr if F else None, F, tol, 1,
                                                 MAX_ITER, TOL, dO.ptr, dS.ptr, dI.ptr), 'vi_eval_peak_f64')

        ctx.eval_timing(True)
        res = {}
        for F in (eq.shape[0], 0):
            run(F)
            ctx.sync()
            call = kern = np.inf
            for _ in range(a.calls):
                ctx.timer_start()
                run(F)
                call = min(call, ctx.timer_stop_ms())
                kern = min(kern, ctx.eval_kernel_ms())
            res[F] = call, kern, dS.download(), dI.download()
        ctx.eval_timing(False)
    es.peak_height(times[:1], lat, lon, START, LO, HI)
    t0 = time.perf_counter()
    r = es.peak_height(times, lat, lon, START, LO, HI)
    wall = time.perf_counter() - t0
    F = eq.shape[0]
    call, kern, st, it = res[F]
    ran = st != 3
    emit('sub-grid peaks, N = 144, %d x %d = %d columns x %d records, %d hull facets (%.1f %% of the starts inside), start %g km in '
         '[%g, %g] km, tol %g m; best of %d timed calls after a warm-up'
         % (a.n, a.n, Q, T, F, 100. * ran.mean(), START / 1e3, LO / 1e3, HI / 1e3, TOL, a.calls))
    emit('  statuses 0..4 of Estimate.peak_height: %s; iterations of the columns that searched: mean %.2f, max %d'
         % (np.bincount(r.status.ravel(), minlength=5), it[ran].mean(), it[ran].max()))
    emit('  vi_eval_peak_f64 with the hull     call %9.3f ms, kernel %9.3f ms = %7.2f ns per column and walk'
         % (call, kern, 1e6 * kern / (it[ran] + 1).sum()))
    c0, k0, s0, i0 = res[0]
    emit('  vi_eval_peak_f64 without the hull  call %9.3f ms, kernel %9.3f ms = %7.2f ns per column and walk (mean %.2f iterations)'
         % (c0, k0, 1e6 * k0 / (i0[s0 != 3] + 1).sum(), i0[s0 != 3].mean()))
    emit('  Estimate.peak_height, host arrays in and out, hull test of the end points included: wall %9.1f ms' % (1e3 * wall))
    tree = os.path.abspath(a.parent) if a.parent else HERE
    with tempfile.TemporaryDirectory() as tmp:
        save = os.path.join(tmp, 'host_loop.npz')
        subprocess.run([sys.executable, os.path.abspath(__file__), '--child', tree, '--save', save, '--n', str(a.n), '--records',
                        str(T)], check=True, cwd=tree, env=dict(os.environ, PYTHONPATH=tree))
        hl = np.load(save)
        both = (hl['S'] == 0) & (r.status.reshape(T, Q) == 0)
        diff = np.abs(hl['H'][both] - r.height.reshape(T, Q)[both])
        emit('  host loop of __call__ / gradient / hessian on %s library: wall %9.1f ms in %d library calls; %d columns with '
             'status 0 in both, heights differ by at most %.2e m'
             % ("the parent's" if a.parent else "this tree's", 1e3 * float(hl['wall']), int(hl['calls']), int(both.sum()),
                float(diff.max()) if diff.size else float('nan')))
        emit('  host loop wall / peak_height wall: %.1f' % (float(hl['wall']) / wall))
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
