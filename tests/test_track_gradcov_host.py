"""Host half of the gradient covariances along a track (vi_eval_records_gradcov_f64, kernel K2tc; vi_eval_track_grad_cov_f64;
Estimate.track_gradient_covariance / track_gradient_error): the block / tile / run geometry of K2tc restated, the check that
the case list of tests/test_gpu_track_gradcov.py reaches every relation of a run to a tile and to a block at every NB, the
declarations and bindings of the two library entries, and the errors the two methods raise before anything is uploaded.
No GPU needed.

  K2tc  k_eval_records_gradcov   NB = ceil(N / 16) = 1 .. 9 (N <= 144), any Q, no alignment condition.  A workgroup of 4 waves
        <NB, INTERP>             takes `groups` blocks of 256 consecutive points one after the other, groups = clamp(Q >> 16, 1, 8)
                                 (VINTERP_K2TC_GROUPS: 1 .. 256); a block is 16 tiles of 16 points, tile t goes to wave t & 3.
                                 The runs of equal rec are cut at the block borders; per run and pass the record's S is staged
                                 unless it is the one staged last; every tile that meets the run is computed, a lane keeps
                                 its point if it lies in the run.  Anything else, and VINTERP_EVAL_RESIDENT=blas: run by run
                                 through the library."""
import os
import re

import numpy as np
import pytest

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, TILE, WAVES = 256, 16, 4

# the orders of the exact suite: the issue's list, NB = 1, 1, 2, 3, 7, 9, 9 with padded and exact last blocks, extended by
# N = 50, 80, 96, 113 so that every NB from 1 to 9 runs every pattern (NB = 4, 5, 6, 8)
K2TC_NS = [5, 16, 27, 48, 50, 80, 96, 100, 113, 129, 144]
LIB_N = 160                                                    # above K2tc's orders: the library route in-process
ONE_QS = (1, 15, 16, 17, 255, 256, 257, 513)
RUNS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1)
DESCENDING = 70                                                # every column its own record, 70 ... 1
RAW_R = 74                                                     # records of the exact suite: rows 0 ... 73


def run_records(lengths, first=0, step=1):
    """rec of consecutive runs of the given lengths, records first, first + step, ..."""
    return np.concatenate([np.full(n, first + k * step) for k, n in enumerate(lengths)]).astype(np.int32)


def patterns():
    """name -> rec of the exact suite.  The runs take records 2, 5, 8, ... (r + 1 is never the next run's record), the single
    records take 3."""
    p = {'one%d' % q: np.full(q, 3, dtype=np.int32) for q in ONE_QS}
    p['runs'] = run_records(RUNS, 2, 3)
    p['runs_reversed'] = run_records(RUNS, 2, 3)[::-1].copy()
    p['descending'] = np.arange(DESCENDING, 0, -1).astype(np.int32)
    return p


def k2tc_groups(Q, env=None):
    g = min(max(Q >> 16, 1), 8)
    if env is not None and 1 <= env <= 256:
        g = env
    return g


def k2tc_geometry(N, Q, groups=None, blas=False):
    NB = -(-N // 16)
    g = k2tc_groups(Q, groups)
    nblk = -(-Q // (BLOCK * g))
    kernel = not blas and 1 <= N <= 144 and nblk < 2 ** 31
    return dict(path='kernel' if kernel else 'library', NB=NB, groups=g, nblk=nblk,
                shm=NB * (NB + 1) // 2 * 2048 + 6 * BLOCK * 8 + BLOCK * 4 + BLOCK // 8)


def k2tc_walk(rec, groups=1, interp=False, R=RAW_R):
    """What the workgroups of K2tc do with rec: a list of dicts, one per run as a block sees it - block, [p, e) inside it, the
    record, the tiles computed (tile, wave, columns kept), the stagings done - in the order of the kernel."""
    rec = np.asarray(rec)
    Q = rec.size
    out = []
    for wg in range(-(-Q // (BLOCK * groups))):
        staged = None
        for grp in range(groups):
            q0 = (wg * groups + grp) * BLOCK
            if q0 >= Q:
                break
            nq = min(Q - q0, BLOCK)
            r_blk = rec[q0:q0 + nq]
            starts = [0] + [c for c in range(1, nq) if r_blk[c] != r_blk[c - 1]]
            for i, p in enumerate(starts):
                e = starts[i + 1] if i + 1 < len(starts) else nq
                r = int(r_blk[p])
                run = dict(block=q0 // BLOCK, q0=q0, p=p, e=e, rec=r, tiles=[], staged=[])
                out.append(run)
                if r < 0 or r + (1 if interp else 0) >= R:
                    continue
                first = 1 if interp and staged == r + 1 else 0
                for it in range(2 if interp else 1):
                    ps = it ^ first
                    if staged != r + ps:
                        run['staged'].append(r + ps)
                        staged = r + ps
                    if it == 0:
                        for t in range(p // TILE, (e - 1) // TILE + 1):
                            run['tiles'].append((t, t & (WAVES - 1), max(p, TILE * t), min(e, TILE * t + TILE)))
    return out


def relations(rec, groups=1):
    """The relations of runs to tiles and blocks that rec reaches."""
    rec = np.asarray(rec)
    Q = rec.size
    walk = k2tc_walk(rec, groups)
    got = set()
    kept = np.zeros(Q, dtype=int)
    per_tile = {}
    for run in walk:
        p, e, q0 = run['p'], run['e'], run['q0']
        if p % TILE:
            got.add('starts inside a tile')
        if e % TILE and q0 + e < Q:
            got.add('ends inside a tile')
        if p % TILE == 0 and e == p + TILE:
            got.add('covers a tile exactly')
        if p == 0 and q0 > 0 and rec[q0 - 1] == rec[q0]:
            got.add('spans a block border')
        if e - p >= TILE * WAVES:
            got.add('occupies all four waves')
        for t, wave, a, b in run['tiles']:
            assert wave == t % WAVES and a < b
            kept[q0 + a:q0 + b] += 1
            per_tile.setdefault((run['block'], t), []).append(run['rec'])
            if Q % TILE and q0 + TILE * t + TILE > Q:
                got.add('a run in the last partial tile')
    assert np.all(kept == 1)                                   # every column is kept by exactly one run and tile
    if any(len(v) > 1 for v in per_tile.values()):
        got.add('a tile shared by two runs')
    if any(len(v) > 2 for v in per_tile.values()):
        got.add('a tile shared by more than two runs')
    return got


ALL_RELATIONS = {'starts inside a tile', 'ends inside a tile', 'covers a tile exactly', 'spans a block border',
                 'occupies all four waves', 'a tile shared by two runs', 'a tile shared by more than two runs',
                 'a run in the last partial tile'}


def test_patterns_reach_every_relation_at_every_nb():
    pats = patterns()
    assert pats['runs'].size == sum(RUNS) == 1012 and pats['descending'].size == DESCENDING
    assert max(int(r.max()) for r in pats.values()) + 1 < RAW_R                       # r + 1 is a row of the stack
    got = set()
    for name, rec in pats.items():
        got |= relations(rec)
    assert got == ALL_RELATIONS, ALL_RELATIONS - got
    # ... the runs alone reach all but the exact tile, in either direction
    for name in ('runs', 'runs_reversed'):
        assert relations(pats[name]) >= ALL_RELATIONS - {'covers a tile exactly', 'a tile shared by more than two runs'}, name
    assert 'covers a tile exactly' in relations(pats['one16'])
    assert 'a tile shared by more than two runs' in relations(pats['descending'])
    # every pattern runs at every N of the list, and the list holds every NB, padded and exact last blocks among them
    nbs = {k2tc_geometry(N, 1012)['NB'] for N in K2TC_NS}
    assert nbs == set(range(1, 10))
    assert {5, 16, 27, 48, 100, 129, 144} <= set(K2TC_NS)
    assert any(N % 16 == 0 for N in K2TC_NS) and any(N % 16 for N in K2TC_NS)
    assert all(k2tc_geometry(N, 1012)['path'] == 'kernel' for N in K2TC_NS)
    assert k2tc_geometry(LIB_N, 1012)['path'] == 'library' and k2tc_geometry(144, 1012, blas=True)['path'] == 'library'
    assert k2tc_geometry(144, 1012)['shm'] == 92160 + 12288 + 1056
    assert k2tc_geometry(144, 1 << 20)['groups'] == 8 and k2tc_geometry(144, 1012)['groups'] == 1


def test_stagings_of_the_walk():
    """One staging per run in nearest mode, two in blend mode; with several blocks per workgroup a run that goes on across a
    block border is not staged again, and in blend mode the pass whose record is staged goes first."""
    rec = patterns()['runs']
    for groups in (1, 3):
        near = k2tc_walk(rec, groups)
        blend = k2tc_walk(rec, groups, interp=True)
        assert len(near) == len(blend)
        for a, b in zip(near, blend):
            cont = a['p'] == 0 and a['block'] % groups and rec[a['q0'] - 1] == a['rec']
            assert a['staged'] == ([] if cont else [a['rec']])
            assert len(b['staged']) == (1 if cont else 2) and set(b['staged']) <= {b['rec'], b['rec'] + 1}
        assert any(not a['staged'] for a in near) == (groups > 1)
    # rows the stack does not hold stage nothing
    for r in k2tc_walk(np.array([-1, -1, 3, RAW_R - 1, RAW_R]), interp=True):
        assert bool(r['staged']) == (r['rec'] == 3)


def test_header_declares_and_lib_binds_the_entries():
    from volumetricinterp_amd import _lib
    with open(os.path.join(REPO_ROOT, 'include', 'vinterp.h')) as fh:
        header = fh.read()
    for name in ('vi_eval_records_gradcov_f64', 'vi_eval_track_grad_cov_f64'):
        assert re.search(r'^int\s+%s\(vi_model\*' % name, header, re.M), name
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name).argtypes is not None
    assert len(_lib.lib.vi_eval_records_gradcov_f64.argtypes) == 8
    assert len(_lib.lib.vi_eval_track_grad_cov_f64.argtypes) == 14


def test_methods_raise_before_anything_is_uploaded():
    """A bad frame and an Estimate without covariances are refused on an object that has no model and no device."""
    from volumetricinterp_amd.estimate import Estimate
    es = Estimate.__new__(Estimate)
    es.Covariance = None
    for call in (es.track_gradient_covariance, es.track_gradient_error):
        with pytest.raises(ValueError, match="frame must be 'model' or 'enu'"):
            call(0., [78.], [262.], [300e3], frame='xyz')
        with pytest.raises(ValueError, match='no covariance'):
            call(0., [78.], [262.], [300e3])
        with pytest.raises(ValueError, match='no covariance'):
            call(0., [78.], [262.], [300e3], frame='enu')
    es.Covariance = np.zeros((1, 2, 2))
    with pytest.raises(ValueError, match="frame must be 'model' or 'enu'"):
        es.track_gradient_covariance(0., [78.], [262.], [300e3], frame='xyz')
