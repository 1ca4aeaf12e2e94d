"""GPU tests of the standard errors with one covariance per point or ray: vi_eval_records_err_f64 (kernel K2te: K2e's body with
the covariance chosen per run of columns; the library's product run by run for other shapes), Estimate.track_error
(vi_eval_track_err_f64) and Estimate.slant_error (vi_eval_slant_err_f64).

Records are synthesised as tests/test_gpu_resident_error.py does: the fixture's finite covariances, each once as it is and
then scaled by 4^j (exact in every operation), mid-times 60 s apart, built with Estimate.from_arrays.

Gates, all the project's own:
  G-bits    nearest mode, K2e's shapes: out[q] is bit for bit E[rec[q], q], E = vi_eval_resident_err_f64 of all R records on
            the same matrix; a record that is 4^j times another gives exactly 2^j times its values.
  G-form    _check_errors of tests/test_gpu_resident_rays.py with a covariance per point: on the device's own columns Y and
            the host blend S_q, |out^2 - y_q^T S_q y_q| <= 1e-10 |y_q|^T |S_q| |y_q|; NaN exactly at dead columns, missing
            records and NaN covariances; |form| > bound is asserted at EVERY live point, so NaN <=> form < 0 is decided
            everywhere (the points are drawn from the box lat 75-81, lon 250-274, alt 100-700 km, where the smallest
            form / bound of the fixtures is 161).
  G-oracle  ORACLE_TOL = 1e-8 norm-wise with equal NaN masks against oracle.get_C + oracle.evaluate_error, once per
            distinct time (tests/test_gpu_resident_error.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_resident_error as re_
import test_gpu_track as tt
from conftest import load_golden, rel
from test_gpu_slant import _rays

pytestmark = pytest.mark.gpu

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_TOL = re_.ORACLE_TOL
FORM_TOL = 1e-10
TAGS = ['rbf', 'k8l2', 'scr_k12l2', 'default']              # N = 27 (NB = 2, five padded rows), 32 (NB = 2 exact), 48, 144
RAW_R = 72                                                  # records of the raw tests: a column each at Q = 70
RUNS = (1, 2, 31, 32, 33, 255, 256, 257, 1)                 # odd starts, a run inside a lane pair, across a tile and a block


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _same_bits(x, y):
    return x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


# ---- records and bases -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _records(tag, nrec):
    """(fixture, dC (nrec, N, N), idx, j, time): record k is the finite fixture covariance idx[k] times 4^j[k]; the first
    records are the fixture's own (j = 0)."""
    from volumetricinterp_amd import synth
    f = load_golden('fit_' + tag)
    base = f['Covariance']
    good = np.flatnonzero(np.isfinite(base).all(axis=(1, 2)))
    rng = np.random.default_rng(23)
    idx, j = good[rng.integers(0, len(good), nrec)], rng.integers(-4, 5, nrec)
    n = min(len(good), nrec)
    idx[:n], j[:n] = good[:n], 0
    dC = base[idx] * (4.0 ** j)[:, None, None]
    dC.setflags(write=False)
    return f, dC, idx, j, synth.unix_times(nrec)


def _estimate(tag, nrec, timeinterp=False, Covariance=None):
    from volumetricinterp_amd.estimate import Estimate
    f, dC, _, _, time = _records(tag, nrec)
    N = dC.shape[1]
    return Estimate.from_arrays(np.zeros((nrec, N)), dC if Covariance is None else Covariance, time, f['hull_vert'], str(f['cfg']),
                                timeinterp=timeinterp)


def _box(Q, seed=23):
    rng = np.random.default_rng(seed)
    return rng.uniform(75, 81, Q), rng.uniform(250, 274, Q), rng.uniform(100e3, 700e3, Q)


@functools.lru_cache(maxsize=None)
def _basis(tag, Q=1026):
    """The device's own basis columns (N, Q) of Q points of the box with the hull's NaN columns, on the host."""
    es = _estimate(tag, 2)
    with es.resident_grid(*_box(Q), check_hull=True) as g:
        Y = g.dY.download()
    dead = np.isnan(Y[0])
    assert 0 < dead[:64].sum() < 64 and 0 < dead.sum() < Q
    Y.setflags(write=False)
    return Y


def _ptr(a):
    return None if a is None else a.ptr


def _raw(es, Y, rec, w, dC, offset=0, resident=False):
    """vi_eval_records_err_f64 on the columns Y (N, Q) - d_out `offset` doubles into its allocation - and, with `resident`, E
    (R, Q) of vi_eval_resident_err_f64 on the same device matrix."""
    from volumetricinterp_amd import _lib
    Q, R = Y.shape[1], len(dC)
    h = es.model.handle()
    with es.model.ctx.scope() as dev:
        dY, dr = dev.up(Y), dev.up(rec, np.int32)
        dw = None if w is None else dev.up(w)
        dD = dev.up(dC) if R else None
        dO = dev.empty(Q + 2)
        _lib.check(_lib.lib.vi_eval_records_err_f64(h, Q, dY.ptr, dr.ptr, _ptr(dw), R, _ptr(dD), dO.offset_ptr(offset)),
                   'vi_eval_records_err_f64')
        out = dO.download()[offset:offset + Q]
        if not resident:
            return out
        dE = dev.empty((R, Q))
        _lib.check(_lib.lib.vi_eval_resident_err_f64(h, Q, R, dY.ptr, dD.ptr, dE.ptr), 'vi_eval_resident_err_f64')
        return out, dE.download()


# ---- the gates ---------------------------------------------------------------------------------------------------------------

def _check_form(out, Y, dC, rec, w, what):
    """G-form with the covariance of every point; returns the number of finite results."""
    R = len(dC)
    out, rec = np.ravel(out), np.ravel(rec)
    w = None if w is None else np.ravel(w)
    dead = np.isnan(Y[0])
    assert np.array_equal(dead, np.isnan(Y).any(axis=0))
    pair = 0 if w is None else 1
    missing = (rec < 0) | (rec + pair >= R)
    nanrec = np.isnan(dC).any(axis=(1, 2)) if R else np.zeros(0, dtype=bool)
    r0 = np.clip(rec, 0, max(R - 1, 0))
    bad = np.zeros(rec.size, dtype=bool)
    if R:
        bad = nanrec[r0] | (nanrec[np.clip(rec + 1, 0, R - 1)] if pair else False)
    live = ~(dead | missing | bad)
    assert np.all(np.isnan(out[~live])), what
    q = np.flatnonzero(live)
    form, bound = np.empty(q.size), np.empty(q.size)
    for k, p in enumerate(q):
        S = dC[rec[p]] if w is None else (1 - w[p]) * dC[rec[p]] + w[p] * dC[rec[p] + 1]
        y = Y[:, p]
        form[k] = y @ S @ y
        bound[k] = FORM_TOL * (np.abs(y) @ np.abs(S) @ np.abs(y))
    assert np.all(np.abs(form) > bound), (what, float(np.min(np.abs(form) / bound)))      # decided at every live point
    o = out[q]
    assert np.array_equal(np.isnan(o), form < 0.), what
    fin = ~np.isnan(o)
    err = np.abs(o[fin] ** 2 - form[fin])
    if fin.any():
        print('%s: worst |out^2 - form| / (1e-10 |y| |S| |y|) = %.3e, least |form| / bound %.3g, on %d points'
              % (what, (err / bound[fin]).max(), np.min(np.abs(form) / bound), fin.sum()))
    assert np.all(err <= bound[fin]), what
    return int(fin.sum())


def _check_bits(out, E, rec, idx, j, what):
    """G-bits: nearest mode against the maps of all records, and the exact scaling between a record and its 4^j copy."""
    ok = (rec >= 0) & (rec < len(E))
    q = np.flatnonzero(ok)
    assert _same_bits(out[q], E[rec[q], q]), what
    assert np.all(np.isnan(out[~ok])), what
    for r in range(len(E)):
        assert np.array_equal(E[r], 2.0 ** j[r] * E[int(np.flatnonzero(idx == idx[r])[0])], equal_nan=True), (what, r)


def _run_records(lengths, first=0, step=1):
    """rec of consecutive runs of the given lengths, records first, first + step, ..."""
    return np.concatenate([np.full(n, first + k * step) for k, n in enumerate(lengths)]).astype(np.int32)


PATTERNS = {
    'one2': lambda: np.full(2, 3), 'one64': lambda: np.full(64, 3), 'one254': lambda: np.full(254, 3),
    'one256': lambda: np.full(256, 3), 'one258': lambda: np.full(258, 3), 'one514': lambda: np.full(514, 3),
    'runs': lambda: _run_records(RUNS, 2, 3),
    'runs_reversed': lambda: _run_records(RUNS, 2, 3)[::-1].copy(),
    'descending': lambda: np.arange(70, 0, -1),                              # every column its own record: 70 ... 1
}


# ---- 1. the raw entry --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pattern', sorted(PATTERNS))
@pytest.mark.parametrize('tag', TAGS)
def test_raw_runs(tag, pattern):
    """K2te's shapes (Q even, aligned): G-bits in nearest mode, G-form in nearest mode and with w = 0, 1 and random."""
    f, dC, idx, j, _ = _records(tag, RAW_R)
    es = _estimate(tag, RAW_R)
    rec = PATTERNS[pattern]().astype(np.int32)
    Q = rec.size
    assert Q % 2 == 0 and (pattern not in ('runs', 'runs_reversed') or Q == 868)
    first = int(np.flatnonzero(~np.isnan(_basis(tag)[0]))[0]) & ~1       # (Q = 2: a live column among the two)
    Y = np.ascontiguousarray(_basis(tag)[:, first:first + Q])
    out, E = _raw(es, Y, rec, None, dC, resident=True)
    _check_bits(out, E, rec, idx, j, '%s %s' % (tag, pattern))
    assert _check_form(out, Y, dC, rec, None, '%s %s nearest' % (tag, pattern)) > 0
    rng = np.random.default_rng(3)
    for name, w in (('w=0', np.zeros(Q)), ('w=1', np.ones(Q)), ('w random', rng.random(Q))):
        got = _raw(es, Y, rec, w, dC)
        assert _check_form(got, Y, dC, rec, w, '%s %s %s' % (tag, pattern, name)) > 0


def _missing_case(tag, interp):
    """(dC, rec, w, k): 12 records - for scr_k12l2 record k = 5 is the fixture's NaN record, between two good ones - and 300
    columns in runs that name -1, rows >= R, R - 1, the NaN record and both its neighbours."""
    R = 12
    f, dC, _, _, _ = _records(tag, R)
    dC = dC.copy()
    k = None
    if tag == 'scr_k12l2':
        k = 5
        nan = f['Covariance'][np.flatnonzero(np.isnan(f['Covariance']).any(axis=(1, 2)))[0]]
        assert np.isnan(nan).all()
        dC[k] = nan
    recs = [0, -1, 4, 5, 5, 6, R, 3, R - 1, R + 5, -1, 6, 5, 4, R - 2, 1]
    lengths = [7, 3, 30, 2, 41, 17, 5, 1, 33, 9, 2, 60, 1, 31, 40, 18]
    rec = np.concatenate([np.full(n, r) for r, n in zip(recs, lengths)]).astype(np.int32)
    assert rec.size == 300
    w = np.random.default_rng(4).random(rec.size) if interp else None
    return dC, rec, w, k


@pytest.mark.parametrize('interp', [False, True])
@pytest.mark.parametrize('tag', TAGS)
def test_raw_missing_rows_and_nan_records(tag, interp):
    """rec = -1, rec >= R, rec = R - 1 with a weight (needs row R), a NaN record between two good ones: NaN for exactly the
    points that need what is missing - the NaN record's own points, and with a weight the pairs of the record before it."""
    dC, rec, w, k = _missing_case(tag, interp)
    R = len(dC)
    es = _estimate(tag, R)
    Y = np.ascontiguousarray(_basis(tag)[:, :rec.size])
    out = _raw(es, Y, rec, w, dC)
    assert _check_form(out, Y, dC, rec, w, '%s interp=%s' % (tag, interp)) > 0
    livecol = ~np.isnan(Y[0])
    assert np.all(np.isnan(out[(rec < 0) | (rec >= R)]))
    assert np.all(np.isnan(out[rec == R - 1]) == (interp | ~livecol[rec == R - 1]))
    if k is not None:
        assert np.all(np.isnan(out[rec == k]))
        assert np.all(np.isnan(out[rec == k - 1]) == (interp | ~livecol[rec == k - 1]))
        assert np.array_equal(np.isnan(out[rec == k + 1]), ~livecol[rec == k + 1])
    # no record at all: every point is NaN and no covariance is read
    none = _raw(es, Y, rec, w, dC[:0])
    assert np.all(np.isnan(none))


@pytest.mark.parametrize('interp', [False, True])
@pytest.mark.parametrize('tag', TAGS)
def test_raw_permutation(tag, interp):
    """A point's bits depend on its column, its record(s) and its weight alone: permuting the columns permutes the bits."""
    f, dC, _, _, _ = _records(tag, RAW_R)
    es = _estimate(tag, RAW_R)
    Q = 514
    rng = np.random.default_rng(9)
    rec = np.sort(rng.integers(0, RAW_R - 1, Q)).astype(np.int32)
    w = rng.random(Q) if interp else None
    Y = np.ascontiguousarray(_basis(tag)[:, :Q])
    out = _raw(es, Y, rec, w, dC)
    perm = rng.permutation(Q)
    got = _raw(es, np.ascontiguousarray(Y[:, perm]), rec[perm], None if w is None else w[perm], dC)
    assert np.isfinite(out).sum() > 100
    assert _same_bits(got, out[perm])


@pytest.mark.parametrize('shape', ['Q1', 'Q255', 'Q257', 'misaligned'])
@pytest.mark.parametrize('tag', TAGS)
def test_raw_other_routes(tag, shape):
    """Odd Q and an output that is not 16-byte aligned go run by run through the library: G-form in both modes."""
    f, dC, _, _, _ = _records(tag, 12)
    es = _estimate(tag, 12)
    Q = {'Q1': 1, 'Q255': 255, 'Q257': 257, 'misaligned': 256}[shape]
    first = int(np.flatnonzero(~np.isnan(_basis(tag)[0]))[0])
    Y = np.ascontiguousarray(_basis(tag)[:, first:first + Q])
    rng = np.random.default_rng(6)
    rec = np.sort(rng.integers(-1, 12, Q)).astype(np.int32)
    rec[0] = 2                                              # (Q = 1: a live point with a record)
    for w in (None, rng.random(Q)):
        out = _raw(es, Y, rec, w, dC, offset=1 if shape == 'misaligned' else 0)
        assert _check_form(out, Y, dC, rec, w, '%s %s interp=%s' % (tag, shape, w is not None)) > 0


# ---- 2. track_error against the oracle and the form --------------------------------------------------------------------------

def _record_times(es, Q, seed=12):
    """Q times in random order, two distinct ones (datetimes hold them exactly) at every record - with timeinterp at every
    pair - of es."""
    mt = tt._mid(es.time)
    rng = np.random.default_rng(seed)
    r = rng.integers(0, len(mt) - (1 if es.timeinterp else 0), Q)
    return mt[r] + rng.choice([3.5, 20.25], Q)


@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('check_hull', [False, True])
@pytest.mark.parametrize('tag', TAGS)
def test_track_error_parity(tag, check_hull, timeinterp):
    """300 points over 12 synthetic records, every point at its own time: G-oracle once per distinct time, G-form on the
    basis columns resident_grid builds for the same points."""
    import oracle
    es = _estimate(tag, 12, timeinterp)
    f = _records(tag, 12)[0]
    Q = 300
    lat, lon, alt = _box(Q, seed=31)
    t0 = _record_times(es, Q)
    rec, w = es.select_records(t0)
    assert len(np.unique(rec)) == (11 if timeinterp else 12) and np.any(np.diff(rec) < 0)
    out = es.track_error(t0, lat, lon, alt, check_hull=check_hull)
    assert out.shape == (Q,) and out.dtype == np.float64
    o = re_._oracle(tag)
    ref = np.full(Q, np.nan)
    for t in np.unique(t0):
        m = t0 == t
        _, dC = oracle.get_C(tt._datetime(t), es.time, es.Coeffs, es.Covariance, timeinterp=timeinterp)
        ref[m] = oracle.evaluate_error(o, dC, lat[m], lon[m], alt[m], hull_vert=f['hull_vert'] if check_hull else None)
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    ok = np.isfinite(ref)
    err = rel(out[ok], ref[ok])
    print('%s hull=%s interp=%s against the oracle: rel %.2e on %d points' % (tag, check_hull, timeinterp, err, ok.sum()))
    assert err <= ORACLE_TOL, err
    outside = np.isnan(out).sum()
    assert (0 < outside < Q) if check_hull else outside == 0
    with es.resident_grid(lat, lon, alt, check_hull=check_hull) as g:
        Y = g.dY.download()
    _check_form(out, Y, es.Covariance, rec, w, '%s hull=%s interp=%s' % (tag, check_hull, timeinterp))


# ---- 3. track_error against Estimate.error, and its interface ----------------------------------------------------------------

@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'default'])
def test_track_error_vs_error(tag, timeinterp):
    es = _estimate(tag, 12, timeinterp)
    Q = 200
    lat, lon, alt = _box(Q, seed=32)
    mt = tt._mid(es.time)

    def gate(out, ref, what):
        assert np.array_equal(np.isnan(out), np.isnan(ref)), what
        ok = np.isfinite(ref)
        assert 0 < ok.sum() < ok.size and rel(out[ok], ref[ok]) <= ORACLE_TOL, (what, rel(out[ok], ref[ok]))

    # one time for all points: a scalar, as a datetime and as seconds
    t = tt._datetime(mt[4] + 17.25)
    one = es.error(t, lat, lon, alt)
    got = es.track_error(t, lat, lon, alt)
    gate(got, one, 'one time')
    assert _same_bits(es.track_error(mt[4] + 17.25, lat, lon, alt), got)
    assert _same_bits(es.track_error(np.full(Q, mt[4] + 17.25), lat, lon, alt), got)
    # a time per record, unsorted: Estimate.error once per distinct time
    times = (mt[:-1] + 12.5)[np.random.default_rng(2).integers(0, 11, Q)]
    ref = np.full(Q, np.nan)
    for v in np.unique(times):
        m = times == v
        ref[m] = es.error(tt._datetime(v), lat[m], lon[m], alt[m])
    got = es.track_error(times, lat, lon, alt)
    gate(got, ref, 'a time per record')
    # out=, a (3, 5) shape, datetimes
    buf = np.empty(Q)
    assert es.track_error(times, lat, lon, alt, out=buf) is buf and _same_bits(buf, got)
    sh = es.track_error(times[:15].reshape(3, 5), lat[:15].reshape(3, 5), lon[:15].reshape(3, 5), alt[:15].reshape(3, 5))
    assert sh.shape == (3, 5) and _same_bits(sh.ravel(), es.track_error(times[:15], lat[:15], lon[:15], alt[:15]))
    dts = np.array([tt._datetime(v) for v in times[:15]], dtype=object)
    assert _same_bits(es.track_error(dts, lat[:15], lon[:15], alt[:15]), sh.ravel())
    with pytest.raises(ValueError, match='out must be'):
        es.track_error(times, lat, lon, alt, out=np.empty(Q + 1))
    with pytest.raises(ValueError, match='times must be'):
        es.track_error(times[:7], lat, lon, alt)
    # times outside the file
    late = times.copy()
    late[:10] = mt[-1] + 4000.
    with pytest.raises(ValueError) as e:
        es.track_error(late, lat, lon, alt)
    assert str(e.value) == tt.MESSAGE
    part = es.track_error(late, lat, lon, alt, outside='nan')
    assert np.all(np.isnan(part[:10])) and _same_bits(part[10:], got[10:])
    # nothing to compute; no covariance
    assert es.track_error(times[:0], lat[:0], lon[:0], alt[:0]).shape == (0,)
    nocov = _estimate(tag, 12, timeinterp)
    nocov.Covariance = None
    with pytest.raises(ValueError, match='no covariance'):
        nocov.track_error(times, lat, lon, alt)
    with pytest.raises(ValueError, match='no covariance'):
        nocov.slant_error(times[0], (78., 262., 0.), (79., 262., 1e6))


# ---- 4. chunks ---------------------------------------------------------------------------------------------------------------

def _chunk_case():
    """track_error of 200 points whose runs of records straddle the borders at 64 and 128, in both modes, and slant_error of
    the 260 oblique rays with their chords: what the chunked child and the unchunked parent both compute."""
    lat, lon, alt = _box(200, seed=33)
    out = []
    for timeinterp in (False, True):
        es = _estimate('default', 12, timeinterp)
        mt = tt._mid(es.time)
        rec = _run_records((50, 30, 40, 60, 20), 1, 2)          # runs [0, 50) [50, 80) [80, 120) [120, 180) [180, 200)
        out.append(es.track_error(mt[rec] + 7.5, lat, lon, alt))
        start, end, _, _ = _rays('oblique', 260)
        rrec = np.sort(np.random.default_rng(5).integers(0, 11, 260))
        out.extend(es.slant_error(mt[rrec] + 7.5, start, end, chord=True))
    return np.array([np.pad(v, (0, 260 - v.size)) for v in out])


CHILD = '''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import test_gpu_track_error as te
np.save(sys.argv[1], te._chunk_case())
'''


def test_chunks_in_a_child_process(tmp_path):
    """VINTERP_TRACK_ERR_CHUNK=64 in a fresh child: four chunks of points, five of rays, runs of records across the borders -
    the bits of the unchunked call."""
    assert 'VINTERP_TRACK_ERR_CHUNK' not in os.environ
    own = _chunk_case()
    assert 0 < np.isnan(own[0]).sum() < 200 and 0 < np.isnan(own[1]).sum() < 260
    script = tmp_path / 'child.py'
    script.write_text(CHILD % (REPO_ROOT, os.path.join(REPO_ROOT, 'tests')))
    o = str(tmp_path / 'chunked.npy')
    res = subprocess.run([sys.executable, str(script), o], env=dict(os.environ, VINTERP_TRACK_ERR_CHUNK='64'),
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, 'chunked child: exit %d\n%s\n%s' % (res.returncode, res.stdout[-3000:], res.stderr[-3000:])
    assert _same_bits(np.load(o), own)


# ---- 5. slant_error ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'default'])
def test_slant_error(tag, timeinterp):
    """260 oblique rays over 8 synthetic records in random order: G-form on the matrix resident_rays builds for the same
    rays, and per distinct time ResidentRays.error of that time's rays at G-form's bound."""
    es = _estimate(tag, 8, timeinterp)
    P = 260
    start, end, a, b = _rays('oblique', P)
    t0 = _record_times(es, P, seed=14)
    rec, w = es.select_records(t0)
    assert len(np.unique(rec)) == (7 if timeinterp else 8) and np.any(np.diff(rec) < 0)
    out, d0, d1 = es.slant_error(t0, start, end, chord=True)
    assert out.shape == (P,)
    with es.resident_rays(start, end) as r:
        Y = r.basis()
    assert 0 < np.isnan(Y[0]).sum() < P
    assert _check_form(out, Y, es.Covariance, rec, w, '%s interp=%s' % (tag, timeinterp)) >= 50
    # the chord is slant's, bit for bit; the values do not depend on asking for it
    _, s0, s1 = es.slant(t0, start, end, chord=True)
    assert _same_bits(d0, s0) and _same_bits(d1, s1)
    assert _same_bits(es.slant_error(t0, start, end), out)
    for t in np.unique(t0):
        m = np.flatnonzero(t0 == t)
        sub = tuple(v[m] for v in start), tuple(v[m] for v in end)
        with es.resident_rays(*sub) as r:
            ref = r.error([tt._datetime(t)])[0]
        got = out[m]
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        S = es.get_C(tt._datetime(t))[1]
        Ym = Y[:, m]
        live = ~np.isnan(ref)
        bound = FORM_TOL * np.einsum('ip,ip->p', np.abs(Ym[:, live]), np.abs(S) @ np.abs(Ym[:, live]))
        assert np.all(np.abs(got[live] ** 2 - ref[live] ** 2) <= bound)


@pytest.mark.parametrize('timeinterp', [False, True])
def test_slant_error_edges(timeinterp):
    """The dead ray, the ray of length zero and chord=True as slant treats them; times outside the file; shapes."""
    es = _estimate('k8l2', 8, timeinterp)
    mt = tt._mid(es.time)
    t = mt[2] + 7.5
    inside = (78., 262., 300e3)
    assert es.check_hull(*inside)
    # a live ray, a miss, a NaN and an infinite start, a segment of length zero inside the hull
    # (the first is the vertical through `inside`)
    start = (np.array([78., 20., np.nan, 78., 78.]), 262., np.array([0., 0., 0., np.inf, 300e3]))
    end = (np.array([78., 21., 79., 79., 78.]), 262., np.array([1000e3, 1000e3, 1000e3, 1000e3, 300e3]))
    val, d0, d1 = es.slant_error(t, start, end, chord=True)
    ref = es.slant(t, start, end, chord=True)
    assert np.isfinite(val[0]) and val[0] > 0. and np.all(np.isnan(val[1:4])) and val[4] == 0.
    assert _same_bits(d0, ref[1]) and _same_bits(d1, ref[2])
    # a (4, 5) array of satellites from one receiver, out=
    rng = np.random.default_rng(30)
    sats = (rng.uniform(72, 84, (4, 5)), rng.uniform(240, 284, (4, 5)), 1000e3)
    t0 = np.round(rng.uniform(mt[0], mt[-1] - 1., (4, 5)) * 64.) / 64.
    buf = np.empty((4, 5))
    out = es.slant_error(t0, (78., 262., 0.), sats, out=buf)
    assert out is buf and 0 < np.isnan(out).sum() < 20
    flat = es.slant_error(t0.ravel(), (78., 262., 0.), tuple(np.ravel(np.broadcast_to(v, (4, 5))) for v in sats))
    assert _same_bits(flat, out.ravel())
    late = t0.copy()
    late[0, :] = mt[-1] + 4000.
    with pytest.raises(ValueError) as e:
        es.slant_error(late, (78., 262., 0.), sats)
    assert str(e.value) == tt.MESSAGE
    part = es.slant_error(late, (78., 262., 0.), sats, outside='nan')
    assert np.all(np.isnan(part[0])) and _same_bits(part[1:], out[1:])
    with pytest.raises(ValueError, match='times must be'):
        es.slant_error(t0.ravel()[:7], (78., 262., 0.), sats)
    assert es.slant_error(np.zeros((0, 3)), (np.zeros((0, 3)), 262., 0.), (80., 262., 1e6)).shape == (0, 3)


@pytest.mark.parametrize('n', [1, 3, 255, 256, 257])
def test_slant_error_ray_counts(n):
    """Ray counts about K2te's conditions (Q even) and the border of its block, at the default order: G-form on the matrix."""
    es = _estimate('default', 8)
    start, end, _, _ = _rays('oblique', 260)
    start, end = tuple(v[:n] for v in start), tuple(v[:n] for v in end)
    mt = tt._mid(es.time)
    t0 = (mt + 7.5)[np.random.default_rng(n).integers(0, 8, n)]
    rec, w = es.select_records(t0)
    out = es.slant_error(t0, start, end)
    with es.resident_rays(start, end) as r:
        Y = r.basis()
    fin = _check_form(out, Y, es.Covariance, rec, w, 'n = %d' % n)
    assert fin == (~np.isnan(Y[0])).sum()
