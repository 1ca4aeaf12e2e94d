"""Measurement (GPU): one bracket-walk launch of the role-separated Jacobi kernel at the benchmarked geometry - T records x 49
decades in shared bases, N = 144, the walk's convergence tolerance - timed with the HIP events of vi_solve_timing, best of the four calls after the first:
microseconds per system chip-wide and sweeps per system.  VINTERP_K3_PERSIST=0 and VINTERP_LIB select what is measured.
With a stamped library (make STAMPS=1; VINTERP_LIB) it also prints where thread 0 of the workgroups spent its cycles, per phase
of a solve (vi_debug_jacobi_phases), for the walk's systems and for all others (the cold solves of the reference systems).
    python tools/perf_k3_walk.py [records]"""
import ctypes as C
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from volumetricinterp_amd import _lib, synth  # noqa: E402
from volumetricinterp_amd.fitengine import FitEngine  # noqa: E402
from volumetricinterp_amd.models.sphharmlag import Model  # noqa: E402

CFG = '[DEFAULT]\n[MODEL]\nNAME = sphharmlag\nMAXK = 4\nMAXL = 6\nCAP_LIM = 10\nMAX_Z_INT = INF\nLATCP = 78\nLONCP = 262\n'
T = int(sys.argv[1]) if len(sys.argv) > 1 else 100
PHASES = ('set-up', 'load', 'rounds', 'truncation + outputs', 'replay (| next load)', 'copy-out of C (| join)')

m = Model(io.StringIO(CFG))
ctx = m.ctx
lat, lon, alt = synth.beams(*synth.GEOM_C2, seed=0)
P, N = lat.size, m.nbasis
d = [ctx.to_device(a) for a in (lat, lon, alt)]
At = m.basis_device(d[0], d[1], d[2], P, transposed=True)
A = At.download().T
R = m.eval_reg_matricies['curvature']()
value, error = synth.synth_records(A, T, seed0=1000)
os.environ['VINTERP_PIPELINES'] = '1'
eng = FitEngine(ctx, At, P, N, {'curvature': R}, ['curvature'])
eng.upload_records(error**-2., value)
eng.form_normal_equations()
eng._warm_reset()
eng._find_same_below('curvature')
ks = np.arange(0., -49., -1.)
rec = np.repeat(np.arange(T, dtype=np.int32), len(ks))
la = np.tile(ks, T)
stamped = hasattr(_lib.lib, 'vi_debug_jacobi_phases')
ph = (C.c_double * 16)()
best = None
for rep in range(5):
    eng._walk_cache = {}
    ctx.solve_timing(1)
    if stamped:
        _lib.lib.vi_debug_jacobi_phases(ph, 1)
    t0 = time.perf_counter()
    eng.chi2_batch_search(rec, la, 'curvature')
    ctx.sync()
    t1 = time.perf_counter()
    st = ctx.solve_timing(1)
    print('rep %d: wall %.1f ms, %d eigen-solve launches, %d systems, launches %.2f ms in all, the largest %.2f ms, %.2f sweeps '
          'per system' % (rep, (t1 - t0) * 1e3, st['launches'], st['systems'], st['total_ms'], st['max_ms'],
                          st['rounds'] / (N / 2.) / max(1, st['systems'])))
    if rep > 0 and (best is None or st['total_ms'] < best['total_ms']):        # (the first call also decomposes the references)
        best = st
print('N %d, %d records x %d decades: the walk launches %.3f ms best of 4 for %d systems (chunks of the workspace budget, the '
      'largest %.3f ms) = %.3f us per system chip-wide' % (N, T, len(ks), best['total_ms'], best['systems'], best['max_ms'],
                                                           best['total_ms'] * 1e3 / best['systems']))
if stamped:
    _lib.lib.vi_debug_jacobi_phases(ph, 0)
    v = np.array(list(ph))
    for name, o in (('walk systems (conv_tol > 0)', 0), ('other systems (cold)', 8)):
        n = v[o + 7]
        if n == 0:
            continue
        tot = v[o:o + 6].sum()
        print('%s: %d solves in the last repetition, %.0f stamped cycles of thread 0 per solve' % (name, n, tot / n))
        for k, p in enumerate(PHASES):
            print('    %-26s %9.0f cycles  %5.1f %%' % (p, v[o + k] / n, 100. * v[o + k] / tot))
