"""The live list of K2r (k_eval_resident<PAD, true>, csrc/vi_eval_resident.hip): the product runs over the 32-byte pieces (four
consecutive points) that carry a point inside the hull; a piece whose four values of basis row 0 are all NaN gets its NaNs
stored directly.  live_geometry below restates the arithmetic on top of k2r_geometry (tests/test_gpu_resident_geometry.py):

  a workgroup owns 256 x groups points = 64 x groups pieces and goes through them in batches of at most 32 groups = 2048
  pieces; per batch the local indices (16 bit) of the live pieces are compacted into LDS in ascending order (4096 bytes + 16
  bytes of per-wave counts next to the coefficient tile) and the four waves take chunks of 16 of them round-robin.

Part 1 (no GPU) asserts the LDS bounds - two workgroups per CU at N = 144, one CU at N = 288 - and that the constructed cases
reach every class of list.  Part 2 runs constructed Y (integer values, every summation exact) with NaNs in row 0 against NumPy,
equal bits or both NaN, sentinels around the output.  Part 3 runs real hull-masked grids (vi_eval_basis_f64) with the live list
and, in a child process, with VINTERP_K2R_LIVE=0 (the setting is read once per process): the outputs must be equal bit for bit,
NaN bits included, and the NaN columns must be the mask.

The NaN a dead piece gets is the one the full product gives for a column of k_mask_basis NaNs (0x7FF8000000000000, the quiet NaN
of __builtin_nan("") carried through the chain); part 2 asserts those bits at every point of every dead piece and that nothing
of the output keeps its prefill, part 3 prints the bits it finds on either path.  Part 4 (no GPU, needs hipcc) compiles the
kernels and asserts that no instantiation of k_eval_resident uses scratch: the list path holds its registers with three empty
asm statements, and a compiler that spills after all must be noticed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden                                            # noqa: F401  (real_estimate's fixtures)
import test_gpu_resident_geometry as geo

gpu = pytest.mark.gpu

REPO_ROOT = geo.REPO_ROOT
LIVE_BATCH = 32                                     # groups per list
LIST_BYTES = 2 * LIVE_BATCH * 64 + 4 * 4            # 16-bit indices of 2048 pieces + one count per wave
CU_LDS = 160 * 1024
GROUPS_ENV = 'VINTERP_K2R_GROUPS'
DEAD_NAN = 0x7FF8000000000000                      # what the list stores to a dead piece
SENTINEL_BITS = int(np.array([geo.SENTINEL]).view(np.uint64)[0])


# ==== 1. arithmetic of the list ==============================================================================================
def live_geometry(N, Q, T, groups=None):
    """k2r_geometry plus the list: batches per workgroup, LDS bytes of a workgroup (tile + list + counts)."""
    g = geo.k2r_geometry(N, Q, T, groups)
    g['batches'] = -(-g['groups'] // LIVE_BATCH)
    g['lds'] = g['shm'] + LIST_BYTES
    return g


def batch_lists(dead, Q, groups):
    """What the kernel builds from `dead` (per piece: all four values of row 0 NaN): for every workgroup the list of
    (pieces of the batch, live count, chunks of 16) of its batches (those that begin before Q)."""
    P = Q // 4
    out = []
    per_wg = 64 * groups
    for w0 in range(0, P, per_wg):
        wg = []
        for b0 in range(w0, min(w0 + per_wg, P), 64 * LIVE_BATCH):
            np_ = min(64 * LIVE_BATCH, w0 + per_wg - b0, P - b0)
            nlive = int((~dead[b0:b0 + np_]).sum())
            wg.append((np_, nlive, -(-nlive // 16)))
        out.append(wg)
    return out


# classes of a workgroup's pieces, by workgroup index modulo len(CLASSES)
CLASSES = ('all live', 'none live', 'first live', 'last live', 'alternating', 'live 32', 'live 33', 'live 31', 'mixed pieces',
           'random', 'first batch dead', 'only first batch live')


def constructed_row0(rng, Q, groups):
    """NaN pattern of basis row 0, one class of CLASSES per workgroup in turn.  Returns (nan (Q,) bool, dead (Q / 4,) bool,
    classes present).  'mixed pieces': pieces with one, two and three NaN points (live) between dead ones."""
    P = Q // 4
    per_wg = 64 * groups
    nanpt = np.zeros(Q, bool)
    seen = set()
    for w, w0 in enumerate(range(0, P, per_wg)):
        n = min(per_wg, P - w0)
        cls = CLASSES[w % len(CLASSES)]
        d = np.zeros(n, bool)                          # dead pieces of the workgroup
        if cls == 'none live':
            d[:] = True
        elif cls == 'first live':
            d[1:] = True
        elif cls == 'last live':
            d[:-1] = True
        elif cls == 'alternating':
            d[1::2] = True
        elif cls in ('live 32', 'live 33', 'live 31'):
            k = int(cls.split()[1])
            if n < k:
                continue
            d[:] = True
            d[rng.choice(n, k, replace=False)] = False
        elif cls == 'mixed pieces':
            d[rng.random(n) < 0.4] = True
        elif cls == 'random':
            d[rng.random(n) < 0.5] = True
        elif cls == 'first batch dead':
            d[:64 * LIVE_BATCH] = True
            if n <= 64 * LIVE_BATCH:                   # one batch only: this is 'none live'
                cls = 'none live'
        elif cls == 'only first batch live':
            d[64 * LIVE_BATCH:] = True
            if n <= 64 * LIVE_BATCH:
                cls = 'all live'
        seen.add(cls)
        pts = np.repeat(d, 4)
        if cls == 'mixed pieces':                      # live pieces with 1, 2, 3 NaN points, at rotating positions
            livep = np.nonzero(~d)[0]
            for j, pc in enumerate(livep[:len(livep) // 2]):
                k = 1 + j % 3
                pts[4 * pc + (j + np.arange(k)) % 4] = True
        nanpt[4 * w0:4 * (w0 + n)] = pts
    dead = nanpt.reshape(-1, 4).all(axis=1)
    return nanpt, dead, seen


def constructed_cases():
    """(N, Q, T, groups): groups 1, 2, the default, 33 and 256 (one batch, a second partly filled batch, eight batches), T of 1,
    64, 65 and 512, N with and without padded k-steps and the largest tile.  Q = 12 or 13 workgroups and 260 points."""
    c = [(16, 13 * 256 + 260, T, 1) for T in (1, 64, 65, 512)]
    c += [(N, 13 * 256 + 260, 65, 1) for N in (18, 144, 288)]
    c += [(N, 12 * 512 + 260, 65, 2) for N in (18, 144)]
    c += [(16, 2 ** 17 + 4, 64, None)]                               # the default: 2 groups
    c += [(16, 12 * 33 * 256 + 260, 65, 33), (288, 2 * 33 * 256 + 260, 5, 33), (18, 12 * 33 * 256 + 260, 3, 33)]
    c += [(16, 12 * 65536 + 260, 65, 256)]
    # the shape the benchmark runs: N = 144, 32 groups, one full batch of 2048 pieces per workgroup; T = 1 and 512 beyond one batch
    c += [(144, 13 * 8192 + 260, 65, 32), (144, 4 * 8192 + 260, 512, 32), (18, 12 * 33 * 256 + 260, 1, 33),
          (16, 3 * 33 * 256 + 260, 512, 33)]
    return c


def test_list_arithmetic_and_case_classes():
    """Batches and chunks as the kernel forms them, the LDS bounds, and the classes the constructed cases reach (no GPU)."""
    g = live_geometry(144, 256 ** 3, 512)
    assert g['shm'] == 73728 and g['lds'] == 73728 + 4096 + 16 and 2 * g['lds'] <= CU_LDS       # two workgroups share a CU
    assert (g['groups'], g['batches'], g['npg'], g['ntt']) == (32, 1, 2048, 8)
    g = live_geometry(288, 1028, 1)
    assert g['shm'] == 147456 and g['lds'] <= CU_LDS and g['path'] == 'kernel'                  # the largest tile: one CU
    assert all(live_geometry(N, 1028, 1)['lds'] <= CU_LDS for N in range(1, 289))
    assert [live_geometry(16, 2 ** 20, 1, gr)['batches'] for gr in (1, 2, 32, 33, 64, 65, 256)] == [1, 1, 1, 2, 2, 3, 8]
    assert 64 * LIVE_BATCH - 1 < 2 ** 16                                                        # 16-bit local indices
    rng = np.random.default_rng(5)
    seen, live_mod, batches, points_nan = set(), set(), set(), set()
    empty_batch_in_live_wg = empty_wg = one_piece_wg = part_batch = False
    for N, Q, T, groups in constructed_cases():
        g = live_geometry(N, Q, T, groups)
        assert g['path'] == 'kernel' and Q % (256 * g['groups']) and Q % 4 == 0
        nanpt, dead, s = constructed_row0(rng, Q, g['groups'])
        seen |= s
        batches.add(g['batches'])
        for wg in batch_lists(dead, Q, g['groups']):
            tot = sum(b[1] for b in wg)
            empty_wg |= tot == 0
            empty_batch_in_live_wg |= tot > 0 and any(b[1] == 0 for b in wg)
            one_piece_wg |= sum(b[0] for b in wg) == 1
            part_batch |= len(wg) > 1 and wg[-1][0] < 64 * LIVE_BATCH
            for b in wg:
                assert b[2] * 16 >= b[1] > (b[2] - 1) * 16 or b[1] == b[2] == 0
                if b[1]:
                    live_mod.add(b[1] % 16)
        k = nanpt.reshape(-1, 4).sum(axis=1)
        points_nan |= set(np.unique(k).tolist())
    assert seen == set(CLASSES), set(CLASSES) - seen
    assert live_mod >= {0, 1, 15} and batches >= {1, 2, 8} and points_nan == {0, 1, 2, 3, 4}
    assert empty_wg and empty_batch_in_live_wg and one_piece_wg and part_batch
    cs = constructed_cases()
    assert {c[3] for c in cs} >= {1, 2, None, 33, 256} and {c[2] for c in cs} >= {1, 64, 65, 512}
    assert {c[0] for c in cs} >= {144, 288} and any(c[0] % 16 for c in cs)
    assert any(c[0] == 144 and c[3] == 32 and c[1] > 12 * 8192 for c in cs)                     # the benchmark's shape, every class
    assert {c[2] for c in cs if (c[3] or 0) >= 32} >= {1, 65, 512}                              # T beyond groups = 1
    # dead stores by every wave and every round of the scan, in batches after the first, in workgroups without a live piece
    dead_at = set()
    for N, Q, T, groups in cs:
        gr = live_geometry(N, Q, T, groups)['groups']
        _, dead, _ = constructed_row0(rng, Q, gr)
        loc = np.nonzero(dead)[0] % (64 * gr)                                                   # piece within its workgroup
        dead_at |= set(zip((loc // 2048 > 0).tolist(), (loc % 2048 // 512).tolist(), (loc % 512 // 64).tolist()))
    assert dead_at == {(b, w, it) for b in (False, True) for w in range(4) for it in range(8)}
    assert live_geometry(16, 2 ** 17 + 4, 64)['groups'] == 2


# ==== 2. constructed lists, exact ============================================================================================
def constructed_inputs(rng, N, Q, T, groups):
    """Integer C and Y (geo.k2r_integer_inputs: every partial sum exact) with the NaN pattern of constructed_row0 in row 0
    ONLY (the other rows of a dead piece stay finite: nothing but row 0 may decide), a NaN only in a row other than 0 at a few
    live points, and row 0 coefficients of zero, infinity and NaN.  Returns C, Y and the result IEEE evaluation gives."""
    C, Y, _ = geo.k2r_integer_inputs(rng, N, Q, T, special=False)
    nanpt, dead, _ = constructed_row0(rng, Q, groups)
    Y[0, nanpt] = np.nan
    if N > 1:
        livept = np.nonzero(~nanpt)[0]
        Y[N - 1, livept[::max(1, len(livept) // 7)]] = np.nan          # NaN in another row only: computed, NaN as before
    if T >= 2:
        C[1, 0] = 0.0
    if T >= 3:
        C[2, 0] = np.inf
    if T >= 4:
        C[3, 0] = np.nan
    with np.errstate(invalid='ignore'):
        ref = C[:, :1] * Y[:1]
        if N > 1:
            ref = ref + C[:, 1:] @ Y[1:]
    return C, Y, ref, nanpt


def constructed_suite(setenv, delenv, tag=''):
    fails = []
    rng = np.random.default_rng(2027)
    for N, Q, T, groups in constructed_cases():
        delenv(GROUPS_ENV)
        if groups is not None:
            setenv(GROUPS_ENV, str(groups))
        g = live_geometry(N, Q, T, groups)
        line = geo.case_line('r', N, Q, T, groups, 0) + ' batches %d%s' % (g['batches'], tag)
        print(line)
        C, Y, ref, nanpt = constructed_inputs(rng, N, Q, T, g['groups'])
        out, guards = geo.run('r', N, Q, T, Y, C, 0)
        if not guards:
            fails.append(line + ': a store outside the output')
        m = geo.mismatch(out, ref, line)
        if m:
            fails.append(m)
        if not np.isnan(out[:, nanpt]).all():
            fails.append(line + ': a point with NaN in row 0 is not NaN')
        # the stores of the dead pieces: the output is prefilled with the sentinel, itself a NaN, so NaN alone does not show
        # that a dead piece was written.  Every point of a dead piece holds exactly DEAD_NAN at every timestep, and no
        # element of the output still carries the sentinel.
        bits = out.view(np.uint64)
        deadpt = np.repeat(nanpt.reshape(-1, 4).all(axis=1), 4)
        assert deadpt.any()
        if not (bits[:, deadpt] == DEAD_NAN).all():
            t, q = np.argwhere(bits[:, deadpt] != DEAD_NAN)[0]
            fails.append(line + ': %d elements of dead pieces do not hold 0x%016X, first (t %d, dead point no. %d): 0x%016X'
                         % ((bits[:, deadpt] != DEAD_NAN).sum(), DEAD_NAN, t, q, bits[:, deadpt][t, q]))
        if (bits == SENTINEL_BITS).any():
            t, q = np.argwhere(bits == SENTINEL_BITS)[0]
            fails.append(line + ': %d elements were never written, first (t %d, q %d)' % ((bits == SENTINEL_BITS).sum(), t, q))
        del bits
        del C, Y, ref, out
    delenv(GROUPS_ENV)
    return fails


@gpu
def test_constructed_lists_exact(monkeypatch):
    """Every class of list - no live piece in a batch or a workgroup, all live, one live piece first / last, alternating, live
    counts of 16 k and 16 k +- 1, pieces with one to three NaN points, NaN only in another row, NaN in row 0 against zero,
    infinite and NaN coefficients - gives NumPy's bits (or NaN where NumPy has NaN) and touches nothing outside the output."""
    fails = constructed_suite(monkeypatch.setenv, lambda n: monkeypatch.delenv(n, raising=False))
    for f in fails:
        print('FAIL ' + f)
    assert not fails, '\n'.join(fails)


# ==== 3. real masked grids: the live list against the plain loop, bit for bit ================================================
REAL_NS = (144, 27, 180)                            # no padded k-steps; one and three padded k-steps (geo.REAL)
REAL_T = 70
REAL_OFF = 4                                        # doubles: Y and out 32 bytes into their buffers


def real_grid_points():
    """A 24^3 geodetic grid, altitude fastest as in bench.py, cut to 13 700 points (53 groups of 256 and 132 points)."""
    from volumetricinterp_amd import synth
    lat, lon, alt = (a.ravel()[:13700].copy() for a in synth.query_grid(24, lat=(74., 82.), lon=(248., 276.), alt=(90e3, 750e3)))
    return lat, lon, alt


def real_inputs(N):
    """(h, Y with the hull's NaN columns from vi_eval_basis_f64, C (70, N))."""
    rng = np.random.default_rng(1000 + N)
    es, fx = geo.real_estimate(N)
    lat, lon, alt = real_grid_points()
    with es.resident_grid(lat, lon, alt, check_hull=True) as g:
        Y = g.dY.download()
    return es, Y, geo.real_coeffs(rng, N, Y, fx, T=REAL_T)


def real_outputs():
    """out (70, Q) of every order of REAL_NS at the default groups and at VINTERP_K2R_GROUPS=3, with the guards' verdict."""
    res = {}
    for N in REAL_NS:
        es, Y, C = real_inputs(N)
        for groups in (None, 3):
            os.environ.pop(GROUPS_ENV, None)
            if groups is not None:
                os.environ[GROUPS_ENV] = str(groups)
            try:
                out, guards = geo.run('r', N, Y.shape[1], REAL_T, Y, C, REAL_OFF, h=es.model.handle())
            finally:
                os.environ.pop(GROUPS_ENV, None)
            res['out_%d_%s' % (N, groups)] = out
            res['guards_%d_%s' % (N, groups)] = np.array(guards)
    return res


CHILD = '''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import test_gpu_resident_live as live
np.savez(sys.argv[1], **live.real_outputs())
'''


@gpu
def test_real_masked_grids_bit_for_bit(tmp_path):
    """Real hull-masked basis matrices at N = 144, 27 and 180, Q = 13 700 (not a multiple of 256 x groups), T = 70, Y and out
    32 bytes into their buffers: the live list and VINTERP_K2R_LIVE=0 (child process) give the same bits, NaN bits included,
    and the NaN columns are the mask."""
    script = tmp_path / 'child.py'
    script.write_text(CHILD % (REPO_ROOT, os.path.join(REPO_ROOT, 'tests')))
    env = dict(os.environ)
    env.pop(GROUPS_ENV, None)
    env['VINTERP_K2R_LIVE'] = '0'
    o = str(tmp_path / 'plain.npz')
    r = subprocess.run([sys.executable, str(script), o], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, 'VINTERP_K2R_LIVE=0 child: exit %d\n%s\n%s' % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    plain = dict(np.load(o))
    assert os.environ.get('VINTERP_K2R_LIVE') != '0'
    mine = real_outputs()
    for N in REAL_NS:
        _, Y, _ = real_inputs(N)
        Q = Y.shape[1]
        inside = np.isfinite(Y[0])
        assert np.array_equal(np.isfinite(Y), np.broadcast_to(inside, Y.shape))
        k = inside.reshape(-1, 4).sum(axis=1)
        print('N %3d Q %d: %.1f %% of the points outside; pieces: %d dead, %d all inside, %d mixed'
              % (N, Q, 100. * (1. - inside.mean()), (k == 0).sum(), (k == 4).sum(), ((k > 0) & (k < 4)).sum()))
        assert (k == 0).sum() > Q // 40 and (k == 4).sum() > Q // 40 and ((k > 0) & (k < 4)).sum() > 0
        for groups in (None, 3):
            key = '%d_%s' % (N, groups)
            a, b = mine['out_' + key], plain['out_' + key]
            assert bool(mine['guards_' + key]) and bool(plain['guards_' + key]), key
            assert geo.k2r_geometry(N, Q, REAL_T, groups, REAL_OFF)['path'] == 'kernel' and Q % (256 * (groups or 1))
            nan_a = np.unique(a.view(np.uint64)[np.isnan(a)])
            nan_b = np.unique(b.view(np.uint64)[np.isnan(b)])
            print('  groups %s: NaN bits with the list %s, plain loop %s' % (groups, [hex(int(x)) for x in nan_a],
                                                                            [hex(int(x)) for x in nan_b]))
            assert np.array_equal(np.isnan(a), np.broadcast_to(~inside, a.shape)), key
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), '%s: %d elements differ in their bits' % (
                key, (a.view(np.uint64) != b.view(np.uint64)).sum())


# ==== 4. registers ===========================================================================================================
def test_k2r_instantiations_use_no_scratch(tmp_path):
    """hipcc's resource report of csrc/vi_eval_resident.hip with the Makefile's flags: the four k_eval_resident instantiations
    use no scratch, at most 256 VGPRs, and the list path 4112 bytes of static LDS (no GPU needed)."""
    import re
    import shutil
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(REPO_ROOT, 'volumetricinterp_amd', 'csrc', 'vi_eval_resident.hip')
    r = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I/opt/rocm/include',
                        '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', str(tmp_path / 'k2r.o')],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    use = {}
    name = None
    for l in r.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', l)
        if m:
            name = m.group(1)
        m = re.search(r'remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)', l)
        if m and name:
            use.setdefault(name, {})[m.group(1).split()[0]] = int(m.group(2))
    k2r = {n: u for n, u in use.items() if 'k_eval_residentILb' in n}
    for n, u in sorted(k2r.items()):
        print(n, u)
    assert len(k2r) == 4, sorted(use)
    for n, u in k2r.items():
        assert u['ScratchSize'] == 0 and u['VGPRs'] <= 256, (n, u)
        assert u['LDS'] == (LIST_BYTES if 'ELb1EEE' in n else 0), (n, u)
