"""Peak maps of a resident grid (ResidentGrid.peak / evaluate_peaks, vi_eval_resident_peak_f64): np.nanmax / np.nanmin of the
density map along one axis of the grid and the first position that attains it, computed on the device.

Two device paths (csrc/vi_eval_resident.hip, restated in peak_path below):

  fused     K2p, K2r with a reduction in place of the stores: reduced axis last (inner == 1), L % 4 == 0 and K2r's own shapes.
            Partials keyed by (timestep, chunk parity, column + 64-point block), one writer per slot, folded by k_peak_finish.
  two-pass  vi_eval_resident_f64 into the work space, then k_peak_columns (inner > 1) or k_peak_columns_last (inner == 1).

Part 1 (no GPU): the bindings, the path choice and the work-space arithmetic, the classes the constructed cases reach, the
LDS bound, the compiler's resource report of K2p.  Part 2: constructed integer inputs (every sum exact) through the C-ABI against
NumPy, bit for bit, with sentinels around both outputs - in this process and in child processes under VINTERP_K2P=twopass,
VINTERP_EVAL_RESIDENT=blas and VINTERP_K2R_LIVE=0 (each read once per process).  Part 3: real grids through the Python API
against np.nanmax / first argmax of ResidentGrid.__call__, every axis, in slabs, and once against the oracle.  Part 4: arguments.

-0 never leaves the product (the accumulators start at +0 and x + (-0) = x), so the +0 / -0 tie of the specification cannot be
planted through the C-ABI; the compares are plain IEEE (== and <=), for which the two zeros are equal, and columns of equal
zeros are among the planted ties."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden                                            # noqa: F401
import test_gpu_resident_geometry as geo
import test_gpu_resident_live as live

gpu = pytest.mark.gpu
REPO_ROOT = geo.REPO_ROOT
GROUPS_ENV = live.GROUPS_ENV
IDX_SENTINEL = np.int32(0x5EAD5EAD)
CU_LDS = 160 * 1024


# ==== 1. arithmetic ==========================================================================================================
def peak_path(N, outer, L, inner, twopass=False, blas=False):
    """The path vi_eval_resident_peak_f64 takes for a 32-byte aligned basis (vi_peak_fused_shape)."""
    Q = outer * L * inner
    g = geo.k2r_geometry(N, Q, 1)
    fused = (not twopass and not blas and inner == 1 and L % 4 == 0 and Q % 4 == 0 and Q >= 256 and g['shm'] <= geo.LDS_LIMIT
             and outer + -(-Q // 64) < 2 ** 31 - 1)
    return 'fused' if fused else 'twopass'


def peak_slots(outer, L):
    """Slots per timestep and parity: one per key = column + 64-point block of the grid."""
    return outer + -(-(outer * L) // 64)


def peak_work_bytes(N, outer, L, inner, T, **kw):
    if min(outer, L, inner, T) <= 0:
        return 0
    if peak_path(N, outer, L, inner, **kw) == 'fused':
        return T * 2 * peak_slots(outer, L) * 12
    return T * outer * L * inner * 8


def constructed_cases():
    """(N, outer, L, inner, T, groups)."""
    c = [(16, 65, 4, 1, 1, 1), (50, 33, 8, 1, 16, 1), (144, 5, 60, 1, 64, 1), (16, 5, 64, 1, 65, 1), (50, 3, 100, 1, 130, 1),
         (144, 2, 256, 1, 65, 1), (16, 3, 260, 1, 16, 1)]
    # every class of live list (one per workgroup in turn: 13 workgroups and 260 points), columns across tiles and workgroups
    c += [(16, 39, 92, 1, 65, 1), (144, 13, 276, 1, 16, 1), (50, 897, 4, 1, 64, 1)]
    # two groups per workgroup; 33: a second, partly filled batch per workgroup
    c += [(50, 65, 100, 1, 17, 2), (16, 391, 260, 1, 65, 33)]
    # two-pass: L not a multiple of 4, the reduced axis not last, Q < 256
    c += [(16, 50, 6, 1, 5, None), (50, 4, 10, 7, 16, None), (16, 2, 5, 64, 65, None), (144, 5, 8, 1, 3, None),
          (16, 3, 4, 7, 2, None), (50, 6, 66, 1, 2, None)]
    return c


def split_blocks(dead, Q, groups):
    """Number of 64-point blocks whose live pieces fall into two chunks of 16 of their batch's list."""
    P = Q // 4
    n = 0
    per_wg = 64 * groups
    for w0 in range(0, P, per_wg):
        for b0 in range(w0, min(w0 + per_wg, P), 64 * live.LIVE_BATCH):
            np_ = min(64 * live.LIVE_BATCH, w0 + per_wg - b0, P - b0)
            pieces = b0 + np.nonzero(~dead[b0:b0 + np_])[0]
            chunk = np.arange(len(pieces)) // 16
            blk = pieces // 16
            for b in np.unique(blk):
                k = np.unique(chunk[blk == b])
                assert len(k) <= 2 and (len(k) < 2 or k[1] == k[0] + 1)          # what gives every slot one writer
                n += len(k) == 2
    return n


def test_bindings():
    from volumetricinterp_amd import _lib
    for name in ('vi_eval_resident_peak_f64', 'vi_eval_resident_peak_work_bytes', 'vi_reduce_basis_f64'):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert _lib.ABI_VERSION == 2


def test_path_choice_and_case_classes():
    cs = constructed_cases()
    paths = {c: peak_path(*c[:4]) for c in cs}
    fused = [c for c in cs if paths[c] == 'fused']
    two = [c for c in cs if paths[c] == 'twopass']
    assert fused and two
    assert {c[2] for c in fused} >= {4, 8, 60, 64, 100, 256, 260} and {c[0] for c in fused} == {16, 50, 144}
    assert {c[4] for c in fused} >= {1, 16, 64, 65, 130}
    assert any(c[2] < 64 for c in fused) and any(c[2] == 64 for c in fused) and any(c[2] > 64 for c in fused)
    assert any(c[2] % 64 for c in fused if c[2] > 4)                               # columns straddling 64-point tiles
    assert any((256 * c[5]) % c[2] for c in fused)                                 # columns straddling workgroups
    assert all(c[1] * c[2] > 256 for c in fused)
    assert all((c[1] * c[2]) % (256 * c[5]) for c in fused if c[1] * c[2] != 512)  # ragged against 256 x groups, but for
    assert any(c[1] * c[2] == 512 and c[5] == 1 for c in fused)                    # ... two whole workgroups, one column each
    assert any(c[2] % 4 and c[3] == 1 for c in two) and {c[3] for c in two} >= {7, 64}
    assert any(c[1] * c[2] * c[3] < 256 for c in two) and any(c[2] % 4 == 2 and c[2] > 64 for c in two)
    rng = np.random.default_rng(11)
    seen, nsplit = set(), 0
    for c in fused:
        Q = c[1] * c[2]
        _, dead, s = live.constructed_row0(rng, Q, c[5])
        seen |= s
        nsplit += split_blocks(dead, Q, c[5])
    assert seen == set(live.CLASSES), set(live.CLASSES) - seen
    assert nsplit > 100
    # the path choice by its conditions, one at a time
    assert peak_path(144, 4096, 64, 1) == 'fused' and peak_path(144, 4096, 64, 1, twopass=True) == 'twopass'
    assert peak_path(144, 4096, 64, 1, blas=True) == 'twopass' and peak_path(144, 64, 64, 64) == 'twopass'
    assert peak_path(144, 4096, 62, 1) == 'twopass' and peak_path(144, 3, 84, 1) == 'twopass'
    assert peak_path(288, 4096, 64, 1) == 'fused' and peak_path(289, 4096, 64, 1) == 'twopass'
    # work space: the fused path holds partials only - on 256^3 with altitude last 1 / 17 of the volume
    assert peak_slots(65536, 256) == 65536 + 262144
    assert peak_work_bytes(144, 65536, 256, 1, 10) == 10 * 2 * 327680 * 12
    assert peak_work_bytes(144, 65536, 256, 1, 10, twopass=True) == 10 * 2 ** 24 * 8
    assert peak_work_bytes(144, 256, 256, 256, 3) == 3 * 2 ** 24 * 8 and peak_work_bytes(144, 0, 4, 1, 3) == 0
    # keys: column + block grows by at least one from one (column, block) pair to the next, and stays below the slot count
    for outer, L in ((65, 4), (5, 60), (3, 260), (2, 256), (39, 92)):
        q = np.arange(outer * L)
        pairs = np.unique(np.stack([q // L, q // 64], axis=1), axis=0)
        keys = pairs.sum(axis=1)
        assert len(np.unique(keys)) == len(pairs) and keys.max() < peak_slots(outer, L)


def test_lds_bound_two_workgroups_per_cu():
    """K2p allocates what K2r does: the coefficient tile, the live list and its counts; the cross-lane reduction uses none."""
    g = live.live_geometry(144, 256 ** 3, 512)
    assert 2 * g['lds'] <= CU_LDS and g['lds'] == 73728 + live.LIST_BYTES


K2P_VGPRS = {True: 217, False: 254}                 # by LIVE, as DESIGN.md states them


def test_k2p_instantiations_use_no_scratch(tmp_path):
    """hipcc's resource report of the device code: the four k_eval_resident_peak<PAD, LIVE> instantiations use no scratch, the
    VGPRs DESIGN.md states (two waves per SIMD: two workgroups per CU) and the list's 4112 bytes of static LDS or none."""
    import re
    import shutil
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc to ask')
    src = os.path.join(REPO_ROOT, 'volumetricinterp_amd', 'csrc', 'vi_eval_resident.hip')
    r = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I/opt/rocm/include', '--cuda-device-only',
                        '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', str(tmp_path / 'k2p.o')],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    use, inst = {}, None
    for l in r.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', l)
        if m:
            t = re.search(r'k_eval_resident_peakILb([01])ELb([01])E', m.group(1))          # <PAD, LIVE>
            inst = (t.group(1) == '1', t.group(2) == '1') if t else None
        m = re.search(r'remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)', l)
        if m and inst is not None:
            use.setdefault(inst, {})[m.group(1).split()[0]] = int(m.group(2))
    for k, u in sorted(use.items()):
        print('PAD %d LIVE %d' % k, u)
    assert sorted(use) == [(False, False), (False, True), (True, False), (True, True)], sorted(use)
    for (pad, lv), u in use.items():
        assert u['ScratchSize'] == 0 and u['VGPRs'] == K2P_VGPRS[lv], ((pad, lv), u)
        assert u['LDS'] == (live.LIST_BYTES if lv else 0), ((pad, lv), u)


# ==== 2. constructed inputs, exact ===========================================================================================
def ref_peak(vol, outer, L, inner, kind):
    """np.nanmax / np.nanmin along axis 2 of vol (T, outer * L * inner) seen as (T, outer, L, inner), the first position that
    attains it, (NaN, -1) where the column holds no number.  Returns (T, M) value and int32 index."""
    T = vol.shape[0]
    x = vol.reshape(T, outer, L, inner)
    key = -x if kind == 'min' else x
    num = ~np.isnan(key)
    with np.errstate(invalid='ignore'):
        mx = np.max(np.where(num, key, -np.inf), axis=2, keepdims=True)
        idx = np.argmax(num & (key == mx), axis=2)
    val = np.take_along_axis(x, idx[:, :, None, :], axis=2)[:, :, 0, :]
    none = ~num.any(axis=2)
    val = np.where(none, np.nan, val)
    idx = np.where(none, -1, idx).astype(np.int32)
    return val.reshape(T, outer * inner), idx.reshape(T, outer * inner)


def constructed_inputs(rng, N, outer, L, inner, T, groups):
    """live.constructed_inputs (integer C and Y, the NaN classes of row 0 per workgroup, NaN in another row, zero / infinite /
    NaN coefficients) plus, column by column in turn: a dead column, only the first / only the last point live, a dead
    64-point stretch inside a live column, ties - the whole column one value, two values alternating at distances 1, 4, 64
    and 256 x groups, a column of zeros - and an infinite basis value.  Returns C, Y and the IEEE result (T, Q)."""
    Q = outer * L * inner
    C, Y, _, nanpt = live.constructed_inputs(rng, N, Q, T, groups or 1)
    q = (np.arange(outer)[:, None, None] * L + np.arange(L)[None, :, None]) * inner + np.arange(inner)[None, None, :]
    cols = q.transpose(0, 2, 1).reshape(outer * inner, L)                     # points of column m, ascending l
    for m in range(0, len(cols), 2):                                          # every other column keeps the random pattern
        pts = cols[m]
        k = (m // 2 + 4) % 9
        if k == 0:
            Y[0, pts] = np.nan
        elif k == 1:
            Y[0, pts[1:]] = np.nan
            Y[0, pts[0]] = 1.0
        elif k == 2:
            Y[0, pts[:-1]] = np.nan
            Y[0, pts[-1]] = 1.0
        elif k == 3 and L > 64:
            Y[0, pts[L // 2 - 32:L // 2 + 32]] = np.nan
        elif k == 4:                                                          # one value all along the live points
            Y[1:, pts] = Y[1:, pts[1:2]]
            Y[0, pts] = np.where(np.isnan(Y[0, pts]), np.nan, 3.0)
        elif k == 5:                                                          # two values: equal maxima d apart
            d = max(1, min(L // 2, (1, 4, 64, 256 * (groups or 1))[(m // 18) % 4]))
            Y[:, pts] = Y[:, pts[(np.arange(L) // d) % 2 * d]]
        elif k == 6:
            Y[:, pts] = 0.0
        elif k == 7 and N > 2:
            Y[1, pts[L // 3]] = np.inf
            Y[2, pts[(2 * L) // 3]] = -np.inf
    with np.errstate(invalid='ignore', over='ignore'):
        ref = C[:, :1] * Y[:1]
        for n in range(1, N):                                                 # ascending n, as the device: inf - inf alike
            ref = ref + C[:, n:n + 1] * Y[n:n + 1]
    return C, Y, ref


def run_peak(N, outer, L, inner, T, Y, C, kind, work=None, h=None):
    """vi_eval_resident_peak_f64 on device copies, both outputs between sentinels.  Returns (val, idx, sentinels intact)."""
    from volumetricinterp_amd import _lib
    ctx = _lib.get_context()
    h = geo._handle(N) if h is None else h
    M = outer * inner
    G = geo.GUARD
    if work is None:
        work = int(_lib.lib.vi_eval_resident_peak_work_bytes(h, outer, L, inner, T))
    bufs = []
    try:
        dY = ctx.to_device(np.ascontiguousarray(Y, dtype=np.float64))
        bufs.append(dY)
        dC = ctx.to_device(np.ascontiguousarray(C, dtype=np.float64))
        bufs.append(dC)
        dV = ctx.to_device(np.full(2 * G + T * M, geo.SENTINEL))
        bufs.append(dV)
        dI = ctx.to_device(np.full(2 * G + T * M, IDX_SENTINEL, dtype=np.int32))
        bufs.append(dI)
        dW = ctx.empty(max(work, 8), np.uint8)
        bufs.append(dW)
        _lib.check(_lib.lib.vi_eval_resident_peak_f64(h, outer, L, inner, T, dY.ptr, dC.ptr, 0 if kind == 'max' else 1,
                                                      dV.offset_ptr(G), dI.offset_ptr(G), dW.ptr, work), 'peak call')
        v, i = dV.download(), dI.download()
    finally:
        for b in bufs:
            b.free()
    sb = np.array([geo.SENTINEL]).view(np.uint64)[0]
    vb = v.view(np.uint64)
    ok = bool(np.all(vb[:G] == sb) and np.all(vb[G + T * M:] == sb) and np.all(i[:G] == IDX_SENTINEL)
              and np.all(i[G + T * M:] == IDX_SENTINEL))
    return v[G:G + T * M].reshape(T, M), i[G:G + T * M].reshape(T, M), ok


def check_peak(val, idx, rv, ri, what):
    m = geo.mismatch(val, rv, what + ' value')
    if m:
        return m
    if not np.array_equal(idx, ri):
        t, c = np.argwhere(idx != ri)[0]
        return '%s index: %d of %d differ, first (t %d, column %d): got %d, want %d (value %r)' % (
            what, (idx != ri).sum(), idx.size, t, c, idx[t, c], ri[t, c], rv[t, c])
    return ''


def constructed_suite(setenv, delenv, tag='', **path):
    from volumetricinterp_amd import _lib
    fails = []
    rng = np.random.default_rng(2028)
    for case in constructed_cases():
        N, outer, L, inner, T, groups = case
        delenv(GROUPS_ENV)
        if groups is not None:
            setenv(GROUPS_ENV, str(groups))
        line = 'K2p N %3d (outer %3d, L %3d, inner %2d) T %3d groups %s: %s%s' % (N, outer, L, inner, T, groups,
                                                                              peak_path(N, outer, L, inner, **path), tag)
        print(line)
        wb = int(_lib.lib.vi_eval_resident_peak_work_bytes(geo._handle(N), outer, L, inner, T))
        if wb != peak_work_bytes(N, outer, L, inner, T, **path):
            fails.append(line + ': work bytes %d, restated %d' % (wb, peak_work_bytes(N, outer, L, inner, T, **path)))
            continue
        C, Y, ref = constructed_inputs(rng, N, outer, L, inner, T, groups)
        for kind in ('max', 'min'):
            rv, ri = ref_peak(ref, outer, L, inner, kind)
            assert (ri < 0).any() and (ri >= 0).any()
            val, idx, ok = run_peak(N, outer, L, inner, T, Y, C, kind)
            if not ok:
                fails.append(line + ' ' + kind + ': a store outside the outputs')
            m = check_peak(val, idx, rv, ri, line + ' ' + kind)
            if m:
                fails.append(m)
    delenv(GROUPS_ENV)
    # the two-pass path in slabs: a work space of two timesteps and a bit for five
    N, outer, L, inner, T = 16, 50, 6, 1, 5
    C, Y, ref = constructed_inputs(rng, N, outer, L, inner, T, None)
    rv, ri = ref_peak(ref, outer, L, inner, 'max')
    val, idx, ok = run_peak(N, outer, L, inner, T, Y, C, 'max', work=2 * 300 * 8 + 100)
    m = check_peak(val, idx, rv, ri, 'two timesteps per slab' + tag)
    if m or not ok:
        fails.append(m or 'two timesteps per slab: a store outside the outputs')
    return fails


@gpu
def test_constructed_peaks_exact(monkeypatch):
    """Every constructed case, both kinds: NumPy's bits and first positions, (NaN, -1) for the empty columns, nothing written
    outside the outputs; planted ties return the lowest index."""
    fails = constructed_suite(monkeypatch.setenv, lambda n: monkeypatch.delenv(n, raising=False))
    for f in fails:
        print('FAIL ' + f)
    assert not fails, '\n'.join(fails)


@gpu
def test_cut_of_timesteps_does_not_matter():
    """130 timesteps in one call and in calls of 1, 64 and 65: the same bits."""
    rng = np.random.default_rng(7)
    N, outer, L, inner, T = 16, 5, 64, 1, 130
    C, Y, ref = constructed_inputs(rng, N, outer, L, inner, T, 1)
    one_v, one_i, ok = run_peak(N, outer, L, inner, T, Y, C, 'max')
    assert ok
    parts = [run_peak(N, outer, L, inner, b - a, Y, C[a:b], 'max') for a, b in ((0, 1), (1, 65), (65, 130))]
    assert np.array_equal(np.concatenate([p[1] for p in parts]), one_i)
    assert not geo.mismatch(np.concatenate([p[0] for p in parts]), one_v, 'cut')


CHILD = '''
import os
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_resident_peak as pk
fails = pk.constructed_suite(lambda n, v: os.environ.__setitem__(n, v), lambda n: os.environ.pop(n, None), %r, **%r)
for f in fails:
    print('FAIL ' + f)
sys.exit(1 if fails else 0)
'''


@gpu
@pytest.mark.parametrize('name,value,path', [('VINTERP_K2P', 'twopass', {'twopass': True}),
                                             ('VINTERP_EVAL_RESIDENT', 'blas', {'blas': True}),
                                             ('VINTERP_K2R_LIVE', '0', {})])
def test_constructed_peaks_under_the_switches(tmp_path, name, value, path):
    """The same suite in a child process with one switch set (each is read once per process): NumPy's bits again."""
    script = tmp_path / 'child.py'
    script.write_text(CHILD % (REPO_ROOT, os.path.join(REPO_ROOT, 'tests'), ' [%s=%s]' % (name, value), path))
    env = dict(os.environ)
    env.pop(GROUPS_ENV, None)
    env[name] = value
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, '%s=%s child: exit %d\n%s\n%s' % (name, value, r.returncode, r.stdout[-4000:], r.stderr[-3000:])


# ==== 3. real grids through the Python API ===================================================================================
def _times(es, k):
    import datetime as dt
    return [dt.datetime(1970, 1, 1) + dt.timedelta(seconds=float(np.mean(u))) for u in es.time[:k]]


def _host_peaks(vol, axis, kind):
    """np.nanmax / np.nanmin and the first position along `axis` of vol (T,) + shape, as ref_peak."""
    T = vol.shape[0]
    shape = vol.shape[1:]
    outer = int(np.prod(shape[:axis], dtype=np.int64))
    inner = int(np.prod(shape[axis + 1:], dtype=np.int64))
    v, i = ref_peak(vol.reshape(T, -1), outer, shape[axis], inner, kind)
    rest = (T,) + shape[:axis] + shape[axis + 1:]
    return v.reshape(rest), i.reshape(rest)


def _grids():
    from volumetricinterp_amd import synth
    yield 'query_grid(8)', synth.query_grid(8)
    lat, lon, alt = np.meshgrid(np.linspace(75., 81., 4), np.linspace(250., 274., 4), np.linspace(100e3, 700e3, 64), indexing='ij')
    yield '(4, 4, 64)', (lat, lon, alt)


@gpu
@pytest.mark.parametrize('check_hull', [True, False])
@pytest.mark.parametrize('N', [144, 180])
def test_peak_equals_host_reduction_of_the_density(N, check_hull):
    """g.peak(times, axis, kind) is np.nanmax / np.nanmin and the first np.nanargmax of g(times), exactly, for every axis of a
    (8, 8, 8) and a (4, 4, 64) grid: the last axis through K2p, the others through the two-pass path."""
    es, fx = geo.real_estimate(N)
    rng = np.random.default_rng(N)
    base = rng.standard_normal((3, N)) if fx is None else np.nan_to_num(fx[0])[[0, -1, 0]] * np.array([[1.], [1.], [-0.5]])
    base[1] = np.nan                                                         # a failed fit: (NaN, -1) everywhere
    es.Coeffs, es.Covariance = base, np.zeros((3, N, N))
    es.time = np.array([[0., 60.], [60., 120.], [120., 180.]])
    times = _times(es, 3)
    for name, grid in _grids():
        shape = grid[0].shape
        with es.resident_grid(*grid, check_hull=check_hull) as g:
            vol = g(times)
            assert vol.shape == (3,) + shape
            assert np.isnan(vol[0]).any() == check_hull and np.isfinite(vol[0]).any()
            for axis in (-1, 0, 1, 2):
                L = shape[axis]
                outer, inner = int(np.prod(shape[:axis % 3])), int(np.prod(shape[axis % 3 + 1:]))
                assert peak_path(N, outer, L, inner) == ('fused' if axis in (-1, 2) else 'twopass')
                for kind in ('max', 'min'):
                    val, idx = g.peak(times, axis=axis, kind=kind)
                    rv, ri = _host_peaks(vol, axis % 3, kind)
                    assert val.shape == rv.shape and idx.dtype == np.int32 and val.dtype == np.float64
                    assert not geo.mismatch(val.reshape(3, -1), rv.reshape(3, -1), '%s axis %d %s' % (name, axis, kind))
                    assert np.array_equal(idx, ri), (name, axis, kind)
                    assert np.all(idx[1] == -1) and np.isnan(val[1]).all()


@gpu
def test_peaks_in_slabs_of_seven(monkeypatch):
    """30 timesteps with the free memory reported so that the call runs in slabs of 7 (4 x 7 + 2): the bits of one slab, on the
    fused path and on the two-pass path."""
    from volumetricinterp_amd import synth
    es, fx = geo.real_estimate(144)
    rng = np.random.default_rng(3)
    C = np.nan_to_num(fx[0])[rng.integers(0, len(fx[0]), 30)] * rng.uniform(-2, 2, (30, 1))
    with es.resident_grid(*synth.query_grid(8)) as g:
        ctx = es.model.ctx
        total = ctx.mem_info()[1]
        for axis, path in ((-1, 'fused'), (0, 'twopass')):
            assert peak_path(144, 64 if axis else 1, 8, 1 if axis else 64) == path
            one = g.evaluate_peaks(C, axis=axis)
            per = peak_work_bytes(144, 64 if axis else 1, 8, 1 if axis else 64, 1) + 64 * 12
            with monkeypatch.context() as mp:
                mp.setattr(ctx, 'mem_info', lambda: (4 * 7 * per + 100, total))
                assert (4 * 7 * per + 100) // 4 // per == 7
                sl = g.evaluate_peaks(C, axis=axis)
            assert np.isfinite(one[0]).any()
            assert np.array_equal(sl[0].view(np.uint64), one[0].view(np.uint64)) and np.array_equal(sl[1], one[1])


@gpu
def test_peak_value_vs_oracle():
    """The peak along altitude of the default fixture's fit on synth.query_grid(8) against the oracle's density map at the
    project's 1e-10 gate (relative to the largest density), and the oracle's position wherever its margin exceeds the gate."""
    import oracle
    from volumetricinterp_amd import synth
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_default')
    es = Estimate.from_arrays(np.nan_to_num(f['Coeffs']), f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))
    t = _times(es, 1)
    grid = synth.query_grid(8)
    C, _ = oracle.get_C(t[0], f['utime'], np.nan_to_num(f['Coeffs']), f['Covariance'])
    ref = oracle.evaluate(oracle.SphHarmLagOracle(), C, *grid, hull_vert=f['hull_vert'])
    rv, ri = _host_peaks(ref[None], 2, 'max')
    with es.resident_grid(*grid) as g:
        val, idx = g.peak(t)
    scale = np.nanmax(np.abs(ref))
    assert np.array_equal(np.isnan(val), np.isnan(rv)) and np.isfinite(rv).any() and np.isnan(rv).any()
    err = np.nanmax(np.abs(val - rv)) / scale
    print('peak value against the oracle: %.2e of the largest density' % err)
    assert err <= 1e-10
    with np.errstate(invalid='ignore'):
        second = np.sort(np.where(np.isnan(ref), -np.inf, ref), axis=2)[None, :, :, -2]
        clear = (rv - second) > 1e-9 * scale
    assert clear.any() and np.array_equal(idx[clear], ri[clear])
    assert np.array_equal(idx < 0, ri < 0)


# ==== 4. arguments ===========================================================================================================
@gpu
def test_peak_arguments():
    from volumetricinterp_amd import synth
    es, fx = geo.real_estimate(16)
    es.Covariance = np.zeros((1, 16, 16))
    grid = synth.query_grid(4)
    C = np.ones((2, 16))
    g = es.resident_grid(*grid, check_hull=False)
    for bad in (3, -4, 1.5, None, 'alt'):
        with pytest.raises(ValueError, match='axis'):
            g.evaluate_peaks(C, axis=bad)
    with pytest.raises(ValueError, match='kind'):
        g.evaluate_peaks(C, kind='median')
    with pytest.raises(ValueError, match='coefficients'):
        g.evaluate_peaks(np.ones((2, 15)))
    for out in ((np.empty((2, 16)), np.empty((2, 16))), (np.empty((2, 16)), np.empty((2, 15), np.int32)), np.empty((2, 16)),
                (np.empty((2, 16), np.float32), np.empty((2, 16), np.int32))):
        with pytest.raises(ValueError, match='out'):
            g.evaluate_peaks(C, out=out)
    v, i = g.evaluate_peaks(np.ones((0, 16)))
    assert v.shape == (0, 16) and i.shape == (0, 16) and i.dtype == np.int32
    out = (np.empty((2, 16)), np.empty((2, 16), np.int32))
    r = g.evaluate_peaks(C, out=out)
    assert r[0] is out[0] and r[1] is out[1]
    v2, i2 = g.evaluate_peaks(C)
    assert np.array_equal(v2, out[0]) and np.array_equal(i2, out[1]) and np.isfinite(v2).all()
    pv, pi = g.peak(_times(es, 1), axis=1)
    assert pv.shape == (1, 4, 4) and pi.shape == (1, 4, 4)
    g.close()
    with pytest.raises(ValueError, match='closed'):
        g.evaluate_peaks(C)
    with es.resident_grid(np.zeros((3, 0)), np.zeros((3, 0)), np.zeros((3, 0)), check_hull=False) as e:
        v, i = e.evaluate_peaks(C, axis=0)
        assert v.shape == (2, 0) and i.shape == (2, 0)
        v, i = e.evaluate_peaks(C, axis=1)                                   # columns of length zero: nothing to select
        assert v.shape == (2, 3) and np.isnan(v).all() and np.all(i == -1)
    with es.resident_grid(78., 262., 3e5, check_hull=False) as s:
        with pytest.raises(ValueError, match='0-d'):
            s.evaluate_peaks(C)
