"""Share of a hull-masked grid that the live list of K2r (csrc/vi_eval_resident.hip) can skip, by run length: aligned runs of 4
(the 32-byte piece), 16, 64 (a wave's tile of a group) and 256 points (a group) in the raveled order K2r sees (altitude
fastest), all outside the hull / all inside / mixed.  CPU only: the hull of bench.py (beams synth.beams(26, 100, seed=0),
facets and tolerance from estimate.hull_equations) on synth.query_grid(n).

python tools/k2r_live_table.py [n ...]          (default: 128 256)"""
import os
import sys

import numpy as np
from scipy.spatial import ConvexHull

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from volumetricinterp_amd import synth                                         # noqa: E402
from volumetricinterp_amd.estimate import hull_equations                       # noqa: E402
from volumetricinterp_amd.geodesy import geodetic2ecef                         # noqa: E402


def bench_hull():
    lat, lon, alt = synth.beams(*synth.GEOM_C2, seed=0)
    R = np.array(geodetic2ecef(lat, lon, alt)).T
    return hull_equations(R[ConvexHull(R).vertices])


def inside_mask(n, eq, tol, chunk=1 << 18):
    g = [a.ravel() for a in synth.query_grid(n)]
    Q = g[0].size
    inside = np.empty(Q, dtype=bool)
    for s in range(0, Q, chunk):
        X = np.array(geodetic2ecef(*(a[s:s + chunk] for a in g))).T
        inside[s:s + chunk] = (X @ eq[:, :3].T + eq[:, 3]).max(axis=1) <= tol
    return inside


def run_shares(inside, run):
    """(all outside, all inside, mixed) shares of the aligned runs of `run` points."""
    k = inside[:inside.size // run * run].reshape(-1, run).sum(axis=1)
    return (k == 0).mean(), (k == run).mean(), ((k > 0) & (k < run)).mean()


def main():
    eq, tol = bench_hull()
    for n in [int(a) for a in sys.argv[1:]] or [128, 256]:
        inside = inside_mask(n, eq, tol)
        print('grid %d^3 = %d points, %d facets: %.1f %% of the points outside the hull, live share of the 4-point pieces %.3f'
              % (n, inside.size, len(eq), 100. * (1. - inside.mean()), 1. - run_shares(inside, 4)[0]))
        print('  %-22s %12s %12s %12s' % ('aligned run of points', 'all outside', 'all inside', 'mixed'))
        for run in (4, 16, 64, 256):
            o, i, m = run_shares(inside, run)
            print('  %-22d %10.1f %% %10.1f %% %10.1f %%' % (run, 100. * o, 100. * i, 100. * m))
        # chunks of 16 live pieces per workgroup of 32 groups (8192 points): the partly filled last chunk
        if inside.size % 8192 == 0:
            live = inside.reshape(-1, 4).any(axis=1).reshape(-1, 2048).sum(axis=1)
            chunks = -(-live // 16)
            print('  workgroups of 8192 points: live pieces %d .. %d of 2048 (mean %.0f), %d without any; chunks of 16 issued '
                  '%d for %d live pieces: issued share %.3f of all pieces'
                  % (live.min(), live.max(), live.mean(), (live == 0).sum(), chunks.sum(), live.sum(),
                     16. * chunks.sum() / (inside.size / 4)))


if __name__ == '__main__':
    main()
