"""The stores of K2r (csrc/vi_eval_resident.hip, store32 / store16): the densities leave a wave as 16-byte stores at two sites,
each with a cache policy fixed at compile time (VI_K2R_PRODUCT_STORE, VI_K2R_DEAD_STORE) - the product stores of tile_product,
a 32-byte piece per lane and timestep, and the NaN stores of the dead pieces of the live list, which a wave writes as the
16-byte chunks ln and 64 + ln of the 2048 bytes its round of 64 pieces covers in a row (whole lines per instruction wherever a
run of pieces is dead).  What ships: plain product stores, non-temporal (nt) dead stores.

Part 1 (no GPU, needs hipcc) compiles the unit to assembly and counts, in each of the four k_eval_resident bodies, the 16-byte
global stores by policy: what the source implies for the two sites with the shipped policies and none with another - a
non-temporal store that silently turned plain would show here and nowhere else.  (A build with one of the inline-asm policies
must close every asm store statement with its wait states; the check is there for the variant builds.)

Part 2 runs constructed inputs (integer C and Y: every sum exact) against NumPy, bit for bit, at the smallest shapes at which a
store can go wrong - Q = 256; a ragged tail whose last lanes hold no piece; T = 70, a full timestep tile and a ragged one; N = 50,
the padded instantiation - with liveness set per 32-byte piece so that 128-byte lines of the output are written in parts: by
the product and by the NaN stores, by two waves, by some lanes of a chunk store and not by others, or not at all by one of the
sites.  The output lies inside a larger buffer of sentinels: the row before it and the 64 rows after it must come back
untouched.  The same suite runs in a child process with VINTERP_K2R_LIVE=0 (the plain loop; the setting is read once per
process).

Part 3: a kernel that follows on the same stream sees the stores.  Under VINTERP_K2P=twopass (child process)
vi_eval_resident_peak_f64 runs K2r into its work space and k_peak_columns_last over it with no host synchronisation in between;
its maps must be NumPy's nanmax / nanmin and first positions."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_resident_geometry as geo
import test_gpu_resident_live as live

gpu = pytest.mark.gpu
REPO_ROOT = geo.REPO_ROOT
DEAD_NAN = live.DEAD_NAN
SENTINEL_BITS = live.SENTINEL_BITS

# ---- what ships (csrc/vi_eval_resident.hip: the defaults of VI_K2R_PRODUCT_STORE and VI_K2R_DEAD_STORE)
SHIPPED = {'product': 'plain', 'dead': 'nt'}
RT = 4                                               # row tiles of a wave: RT x 4 timesteps per lane
SCAN_ROUNDS = live.LIVE_BATCH * 64 // 256            # rounds of the row-0 scan (unrolled), two chunk stores each
PRODUCT_STORES = 2 * RT * 4                          # 16-byte stores of one tile_product: 16 pieces of 32 bytes
DEAD_STORES = 2 * SCAN_ROUNDS                        # ... of the dead stores of the LIVE branch: chunks ln and 64 + ln


# ==== 1. the policy in the instructions ======================================================================================
def store_policy(line):
    """'plain', 'sc1', 'sc0 sc1' or 'nt' of a global_store line."""
    bits = [b for b in ('sc0', 'sc1', 'nt') if re.search(r'\b%s\b' % b, line.split(';')[0])]
    return ' '.join(bits) or 'plain'


def expected_stores(is_live):
    """{policy: 16-byte stores} of a k_eval_resident body: one tile_product, and with the list the dead stores."""
    want = {}
    want[SHIPPED['product']] = PRODUCT_STORES
    if is_live:
        want[SHIPPED['dead']] = want.get(SHIPPED['dead'], 0) + DEAD_STORES
    return want


def test_store_policy_in_the_assembly(tmp_path):
    """The unit with the flags of test_k2r_instantiations_use_no_scratch, to assembly: per k_eval_resident instantiation the
    16-byte stores by policy are the two sites' with the shipped policies and nothing else, no other global store exists, and
    an asm store statement (the sc1 policies, variant builds only) ends with s_nop 1."""
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(REPO_ROOT, 'volumetricinterp_amd', 'csrc', 'vi_eval_resident.hip')
    asm = tmp_path / 'k2r.s'
    r = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I/opt/rocm/include',
                        '--cuda-device-only', '-S', src, '-o', str(asm)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    bodies, name = {}, None
    for l in asm.read_text().splitlines():
        m = re.match(r'^(_Z\w+):', l)
        if m:
            name = m.group(1)
            bodies[name] = []
        elif name is not None:
            bodies[name].append(l.strip())
            if l.strip().startswith('s_endpgm'):
                name = None
    k2r = {n: b for n, b in bodies.items() if 'k_eval_residentILb' in n}
    assert len(k2r) == 4, sorted(bodies)
    assert {('ELb1EEE' in n) for n in k2r} == {False, True}
    for n, body in sorted(k2r.items()):
        stores = [l for l in body if l.startswith('global_store_') or l.startswith('flat_store_') or l.startswith('buffer_store_')
                  or l.startswith('scratch_store_')]
        got = {}
        for l in stores:
            assert l.startswith('global_store_dwordx4 '), (n, l)                # nothing but 16-byte stores to `out`
            got[store_policy(l)] = got.get(store_policy(l), 0) + 1
        print(n, got)
        assert got == expected_stores('ELb1EEE' in n), (n, got)
        # asm statements, where a policy is one of the asm ones: one or two stores and their wait states, nothing else
        inside, block, blocks = False, [], []
        for l in body:
            if l.startswith(';;#ASMSTART'):
                inside, block = True, []
            elif l.startswith(';;#ASMEND'):
                inside = False
                if any(x.startswith('global_store') for x in block):
                    blocks.append(block)
            elif inside and l:
                block.append(l)
        n_asm = sum(c for p, c in got.items() if 'sc1' in p)
        assert sum(len(b) - 1 for b in blocks) == n_asm, (n, blocks, n_asm)
        for b in blocks:
            assert all(x.startswith('global_store_dwordx4') for x in b[:-1]) and b[-1].split(';')[0].split() == ['s_nop', '1'], (n, b)
            assert len({store_policy(x) for x in b[:-1]}) == 1 and len(b) in (2, 3), (n, b)


# ==== 2. exact against NumPy, partial lines ==================================================================================
SHAPES = ((144, 256, 1), (144, 256 * 3 + 4 * 5, 70), (50, 256 * 3 + 4 * 5, 70))      # (N, Q, T)
PATTERNS = ('alternating', 'three live one dead', 'one live three dead', 'run of 16 k + 2', 'no live piece', 'none dead')
ROWS_BEFORE, ROWS_AFTER = 1, 64                      # sentinel rows around the output: a whole timestep tile after it


def dead_pieces(pattern, Q):
    """(Q / 4,) bool: the 32-byte pieces whose four points are NaN in row 0.  A workgroup owns 64 pieces (groups = 1 at these
    sizes), a 128-byte line of the output four."""
    P = Q // 4
    i = np.arange(P)
    if pattern == 'alternating':
        return i % 2 == 1
    if pattern == 'three live one dead':
        return i % 4 == 3
    if pattern == 'one live three dead':
        return i % 4 != 0
    if pattern == 'run of 16 k + 2':                 # per workgroup one live run of 18 or 34 pieces, off the line grid: the
        d = np.ones(P, bool)                         # list's chunks of 16 cut it inside a line, two waves write that line
        for w0 in range(0, P, 64):
            k = 18 if (w0 // 64) % 2 == 0 else 34
            d[w0 + 3:min(w0 + 3 + k, w0 + 64, P)] = False
        return d
    if pattern == 'no live piece':
        return np.ones(P, bool)
    assert pattern == 'none dead'
    return np.zeros(P, bool)


def test_patterns_reach_what_they_aim_at():
    """The constructed liveness at the shapes of the suite (no GPU): lines written in parts by both sites, a live run that two
    waves share inside a line, a workgroup whose last lanes hold no piece."""
    assert all(geo.k2r_geometry(N, Q, T)['path'] == 'kernel' and geo.k2r_geometry(N, Q, T)['groups'] == 1 for N, Q, T in SHAPES)
    assert {geo.k2r_geometry(N, Q, T)['pad'] > 0 for N, Q, T in SHAPES} == {False, True}
    assert {geo.k2r_geometry(N, Q, T)['ntt'] for N, Q, T in SHAPES} == {1, 2} and any(T % 64 for _, _, T in SHAPES)
    assert any(Q == 256 for _, Q, _ in SHAPES) and any((Q // 4) % 64 % 16 for _, Q, _ in SHAPES)
    for _, Q, _ in SHAPES:
        per_line = {p: dead_pieces(p, Q)[:Q // 16 * 4].reshape(-1, 4).sum(axis=1) for p in PATTERNS}
        assert set(per_line['alternating']) == {2} and set(per_line['three live one dead']) == {1}
        assert set(per_line['one live three dead']) == {3}
        assert set(per_line['no live piece']) == {4} and set(per_line['none dead']) == {0}
        d = dead_pieces('run of 16 k + 2', Q)
        for w0 in range(0, Q // 4, 64):
            livep = np.nonzero(~d[w0:w0 + 64])[0]
            if len(livep) in (18, 34):
                cut = livep[16]                       # first piece of the second chunk, another wave's
                assert cut % 4 != 0 and not d[w0 + cut - 1]                    # ... inside a line the first chunk began
        assert any(len(np.nonzero(~d[w0:w0 + 64])[0]) in (18, 34) for w0 in range(0, Q // 4, 64))


def run_framed(N, Q, T, Y, C):
    """vi_eval_resident_f64 into rows [ROWS_BEFORE, ROWS_BEFORE + T) of a buffer of sentinel rows.  Returns (out (T, Q),
    whether every row around it still holds the sentinel)."""
    from volumetricinterp_amd import _lib
    ctx = _lib.get_context()
    h = geo._handle(N)
    rows = ROWS_BEFORE + T + ROWS_AFTER
    bufs = []
    try:
        dY = ctx.to_device(np.ascontiguousarray(Y, dtype=np.float64))
        bufs.append(dY)
        dC = ctx.to_device(np.ascontiguousarray(C, dtype=np.float64))
        bufs.append(dC)
        dO = ctx.to_device(np.full(rows * Q, geo.SENTINEL))
        bufs.append(dO)
        _lib.check(_lib.lib.vi_eval_resident_f64(h, Q, T, dY.ptr, dC.ptr, dO.offset_ptr(ROWS_BEFORE * Q)), 'vi_eval_resident_f64')
        res = dO.download().reshape(rows, Q)
    finally:
        for b in bufs:
            b.free()
    bits = res.view(np.uint64)
    framed = bool((bits[:ROWS_BEFORE] == SENTINEL_BITS).all() and (bits[ROWS_BEFORE + T:] == SENTINEL_BITS).all())
    return res[ROWS_BEFORE:ROWS_BEFORE + T], framed


_INPUTS = {}


def inputs(N, Q, T):
    """Integer C, Y and the exact product, once per shape."""
    if (N, Q, T) not in _INPUTS:
        C, Y, ref = geo.k2r_integer_inputs(np.random.default_rng(23 + N + Q + T), N, Q, T, special=False)
        for a in (C, Y, ref):
            a.setflags(write=False)
        _INPUTS[(N, Q, T)] = (C, Y, ref)
    return _INPUTS[(N, Q, T)]


def store_suite(tag=''):
    """Every shape with every pattern.  Returns the list of failures."""
    fails = []
    for N, Q, T in SHAPES:
        assert (Q * 8) % 32 == 0 and ROWS_BEFORE * Q * 8 % 32 == 0                # the kernel's alignment
        C, Y0, ref0 = inputs(N, Q, T)
        for pattern in PATTERNS:
            line = 'K2r stores N %3d Q %4d T %2d, %s%s' % (N, Q, T, pattern, tag)
            print(line)
            deadpt = np.repeat(dead_pieces(pattern, Q), 4)
            Y = Y0.copy()
            Y[0, deadpt] = np.nan
            ref = ref0.copy()
            ref[:, deadpt] = np.nan
            out, framed = run_framed(N, Q, T, Y, C)
            if not framed:
                fails.append(line + ': a store in the rows around the output')
            bits = out.view(np.uint64)
            if not np.array_equal(bits[:, ~deadpt], ref.view(np.uint64)[:, ~deadpt]):
                bad = np.argwhere(bits != ref.view(np.uint64))
                bad = bad[~deadpt[bad[:, 1]]]
                fails.append('%s: %d live elements differ in their bits, first (t %d, q %d): got %r, want %r'
                             % (line, len(bad), bad[0][0], bad[0][1], out[tuple(bad[0])], ref[tuple(bad[0])]))
            if not (bits[:, deadpt] == DEAD_NAN).all():
                t, q = np.argwhere(bits[:, deadpt] != DEAD_NAN)[0]
                fails.append('%s: %d elements of dead pieces do not hold 0x%016X, first (t %d, dead point no. %d): 0x%016X'
                             % (line, (bits[:, deadpt] != DEAD_NAN).sum(), DEAD_NAN, t, q, bits[:, deadpt][t, q]))
    return fails


@gpu
def test_stores_exact_with_partial_lines():
    """The live list: NumPy's bits at every live point, the canonical NaN at every point of a dead piece, the sentinel rows
    around the output untouched."""
    assert os.environ.get('VINTERP_K2R_LIVE') != '0'
    fails = store_suite()
    for f in fails:
        print('FAIL ' + f)
    assert not fails, '\n'.join(fails)


CHILD = '''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_resident_stores as st
fails = st.%s
for f in fails:
    print('FAIL ' + f)
sys.exit(1 if fails else 0)
'''


def _child(tmp_path, call, name, value):
    script = tmp_path / 'child.py'
    script.write_text(CHILD % (REPO_ROOT, os.path.join(REPO_ROOT, 'tests'), call))
    env = dict(os.environ)
    env.pop(live.GROUPS_ENV, None)
    env[name] = value
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, '%s=%s child: exit %d\n%s\n%s' % (name, value, r.returncode, r.stdout[-4000:], r.stderr[-3000:])


@gpu
def test_stores_exact_on_the_plain_loop(tmp_path):
    """The same suite with VINTERP_K2R_LIVE=0: every piece through the product and its stores, the NaN of a dead piece carried
    through the chain - the same bits."""
    _child(tmp_path, "store_suite(' [VINTERP_K2R_LIVE=0]')", 'VINTERP_K2R_LIVE', '0')


# ==== 3. the next kernel on the stream reads what was stored =================================================================
VIS_GRID = (4, 8, 64)                                # (lat, lon, alt), altitude last: 32 columns of 64 points
VIS_N, VIS_T = 144, 70


def visibility_suite():
    """K2r into the work space, k_peak_columns_last over it right behind, both kinds: NumPy's maps."""
    import test_gpu_resident_peak as pk
    outer, L = VIS_GRID[0] * VIS_GRID[1], VIS_GRID[2]
    assert pk.peak_path(VIS_N, outer, L, 1, twopass=True) == 'twopass' and pk.peak_path(VIS_N, outer, L, 1) == 'fused'
    assert geo.k2r_geometry(VIS_N, outer * L, VIS_T)['path'] == 'kernel'
    C, Y, ref = pk.constructed_inputs(np.random.default_rng(2029), VIS_N, outer, L, 1, VIS_T, None)
    fails = []
    for kind in ('max', 'min'):
        rv, ri = pk.ref_peak(ref, outer, L, 1, kind)
        assert (ri < 0).any() and (ri >= 0).any()
        val, idx, ok = pk.run_peak(VIS_N, outer, L, 1, VIS_T, Y, C, kind)
        if not ok:
            fails.append(kind + ': a store outside the outputs')
        m = pk.check_peak(val, idx, rv, ri, 'two-pass peak after K2r, ' + kind)
        if m:
            fails.append(m)
    return fails


@gpu
def test_following_kernel_sees_the_stores(tmp_path):
    """VINTERP_K2P=twopass on a 4 x 8 x 64 grid: the consumer of the density volume runs on the stream right after K2r."""
    _child(tmp_path, 'visibility_suite()', 'VINTERP_K2P', 'twopass')
