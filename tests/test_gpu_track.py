"""GPU parity of the evaluation along a trajectory (Estimate.track, vi_eval_track_f64: every point at its own time, one library
call) against an independent device path - Estimate.evaluate_coeffs of ALL records at the points, then the element (or the blend
of two) that Estimate.select_records names - and against the CPU oracle with oracle.get_C's row.

Gates: between the two device paths the NaN pattern is identical and the finite values agree to 1e-12 norm-wise (the gate of
tests/test_gpu_eval_resident.py between two device paths of one contraction); against the oracle 1e-10 (the project's gate L6)."""
import datetime as dt
import functools

import numpy as np
import pytest

from conftest import load_golden, rel

pytestmark = pytest.mark.gpu

EPOCH = dt.datetime(1970, 1, 1)
MESSAGE = 'Requested time out of range of data file.'
DEVICE_TOL = 1e-12
ORACLE_TOL = 1e-10
R = 40


def _oracle(tag):
    import oracle
    return {'k8l2': lambda: oracle.SphHarmLagOracle(maxk=8, maxl=2),
            'scr_k12l2': lambda: oracle.SphHarmLagOracle(maxk=12, maxl=2),
            'rbf': lambda: oracle.RadBasFunOracle(numgridpnt=3),
            'default': lambda: oracle.SphHarmLagOracle()}[tag]()


@functools.lru_cache(maxsize=None)
def _records(tag, nrec=R):
    """(fixture, Coeffs, time): nrec records, each a finite fixture coefficient row drawn at random times a power of two - the
    rows differ and keep their bits -, mid-times 60 s apart."""
    from volumetricinterp_amd import synth
    f = load_golden('fit_' + tag)
    rows = f['Coeffs'][np.all(np.isfinite(f['Coeffs']), axis=1)]
    rng = np.random.default_rng(40)
    C = rows[rng.integers(len(rows), size=nrec)] * 2. ** rng.integers(-3, 4, size=nrec)[:, None]
    C.setflags(write=False)
    return f, C, synth.unix_times(nrec)


def _estimate(tag, timeinterp, nrec=R, Coeffs=None):
    from volumetricinterp_amd.estimate import Estimate
    f, C, time = _records(tag, nrec)
    return Estimate.from_arrays(C if Coeffs is None else Coeffs, None, time, f['hull_vert'], str(f['cfg']), timeinterp=timeinterp)


def _box(rng, Q):
    """Random points in the box of the resident tests: some of it lies outside the hull."""
    return rng.uniform(75, 81, Q), rng.uniform(250, 274, Q), rng.uniform(100e3, 700e3, Q)


@functools.lru_cache(maxsize=None)
def _reference(tag, check_hull, Q=1000, nrec=R, seed=7):
    """(lat, lon, alt, E): Q points and the densities E (nrec, Q) of every record at them by Estimate.evaluate_coeffs."""
    lat, lon, alt = _box(np.random.default_rng(seed), Q)
    es = _estimate(tag, False, nrec)
    E = es.evaluate_coeffs(es.Coeffs, lat, lon, alt, check_hull=check_hull)
    for a in (lat, lon, alt, E):
        a.setflags(write=False)
    return lat, lon, alt, E


def _expected(E, rec, w):
    """The element of E the record selection names, or the blend of two as vi_eval_track_f64 defines it; NaN without a record."""
    q = np.arange(rec.size)
    r = np.maximum(rec, 0)
    out = E[r, q] if w is None else (1 - w) * E[r, q] + w * E[np.minimum(r + 1, E.shape[0] - 1), q]
    out[rec < 0] = np.nan
    return out


def _gate(out, exp, what=''):
    assert out.shape == exp.shape
    assert np.array_equal(np.isnan(out), np.isnan(exp)), what
    ok = np.isfinite(exp)
    assert ok.any(), what
    err = rel(out[ok], exp[ok])
    print('%s rel %.2e on %d finite of %d' % (what, err, ok.sum(), ok.size))
    assert err <= DEVICE_TOL, (what, err)


def _mid(time):
    return np.mean(time, axis=1)


def _datetime(t0):
    return EPOCH + dt.timedelta(seconds=float(t0))


@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('check_hull', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'default', 'scr_k12l2', 'rbf'])
def test_track_parity(tag, check_hull, timeinterp):
    """1000 random points at random times over the records' range, unsorted: k8l2 (2, 8) and default (6, 4) on the tiled
    kernel, scr_k12l2 (2, 12) on the per-lane sphharmlag kernel, rbf on the per-lane RBF kernel."""
    import oracle
    lat, lon, alt, E = _reference(tag, check_hull)
    es = _estimate(tag, timeinterp)
    mt = _mid(es.time)
    t0 = np.random.default_rng(12).uniform(mt[0], mt[-1], lat.size)
    rec, w = es.select_records(t0)
    assert len(np.unique(rec)) >= R - 2 and np.any(np.diff(rec) < 0)            # every record, and unsorted
    out = es.track(t0, lat, lon, alt, check_hull=check_hull)
    exp = _expected(E, rec, w)
    assert (0 < np.isnan(exp).sum() < lat.size) if check_hull else np.isfinite(exp).all()
    _gate(out, exp, '%s hull=%s interp=%s' % (tag, check_hull, timeinterp))
    if not check_hull:
        o = _oracle(tag)
        cov = np.zeros((R, 1, 1))
        # datetimes carry microseconds: the 50 points are evaluated again at times a datetime holds exactly
        t50 = np.array([(_datetime(t) - EPOCH).total_seconds() for t in t0[:50]])
        out50 = es.track(t50, lat[:50], lon[:50], alt[:50], check_hull=False)
        ref = np.array([oracle.evaluate(o, oracle.get_C(_datetime(t50[q]), es.time, es.Coeffs, cov, timeinterp=timeinterp)[0],
                                        lat[q:q + 1], lon[q:q + 1], alt[q:q + 1])[0] for q in range(50)])
        err = rel(out50, ref)
        print('%s interp=%s against the oracle: rel %.2e' % (tag, timeinterp, err))
        assert err <= ORACLE_TOL, err


# ---- geometry of the windows (k8l2, N = 32: the window logic does not depend on the order) ----------------------------------

def _runs(es, p, nrec):
    """Times that put p consecutive points on every record (in interpolation mode: on every pair, the last one ending on
    the last row), and the (rec, w) they must select."""
    mt = _mid(es.time)
    last = nrec - 1 if es.timeinterp else nrec              # rec = R - 2 is the last pair; nearest mode reaches the last row
    rec = np.repeat(np.arange(last, dtype=np.int32), p)
    frac = np.random.default_rng(p).uniform(0., 59., rec.size) if es.timeinterp else np.zeros(rec.size)
    t0 = mt[rec] + frac
    got, w = es.select_records(t0)
    assert np.array_equal(got, rec) and rec[-1] == last - 1
    return t0, rec, w


@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('p', [1, 2, 3, 5, 64, 100, 256, 700])
def test_track_runs_of_points_per_record(p, timeinterp):
    """p points on each of the 40 records (up to 28 000 points): every alignment of a window boundary against a group of 64
    points and a workgroup occurs, whatever the window width."""
    lat, lon, alt, E = _reference('k8l2', True, Q=R * 700, seed=8)
    es = _estimate('k8l2', timeinterp)
    t0, rec, w = _runs(es, p, R)
    Q = rec.size
    out = es.track(t0, lat[:Q], lon[:Q], alt[:Q])
    _gate(out, _expected(E[:, :Q], rec, w), 'p=%d interp=%s' % (p, timeinterp))


@pytest.mark.parametrize('timeinterp', [False, True])
def test_track_span_wider_than_a_workgroup(timeinterp):
    """300 records with one point each: a group of 64 points spans 64 records, many windows."""
    lat, lon, alt, E = _reference('k8l2', True, Q=300, nrec=300, seed=9)
    es = _estimate('k8l2', timeinterp, nrec=300)
    t0, rec, w = _runs(es, 1, 300)
    Q = rec.size
    out = es.track(t0, lat[:Q], lon[:Q], alt[:Q])
    _gate(out, _expected(E[:, :Q], rec, w), 'R=300 interp=%s' % timeinterp)


@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('Q', [1, 63, 257])
def test_track_small_and_odd_sizes(Q, timeinterp):
    lat, lon, alt, E = _reference('k8l2', False)
    es = _estimate('k8l2', timeinterp)
    mt = _mid(es.time)
    t0 = np.random.default_rng(Q).uniform(mt[0], mt[-1], Q)
    t0[-1] = mt[-1] if not timeinterp else mt[-1] - 1.          # the last row / the pair that ends on it
    rec, w = es.select_records(t0)
    assert rec[-1] == (R - 1 if not timeinterp else R - 2)
    out = es.track(t0, lat[:Q], lon[:Q], alt[:Q], check_hull=False)
    _gate(out, _expected(E[:, :Q], rec, w), 'Q=%d interp=%s' % (Q, timeinterp))


# ---- the C entry itself ----------------------------------------------------------------------------------------------------------

def _raw(es, lat, lon, alt, rec, w, check_hull=True):
    """vi_eval_track_f64 on the points as given (no sorting): (Q,) host array."""
    from volumetricinterp_amd import _lib
    ctx = es.model.ctx
    eq, tol = es._hull() if check_hull else (None, 0.)
    bufs = []
    try:
        for a in (lat, lon, alt):
            bufs.append(ctx.to_device(a))
        bufs.append(ctx.to_device(rec, np.int32))
        bufs.append(ctx.to_device(es.Coeffs))
        bufs.append(ctx.empty(lat.size))
        dw = dh = None
        if w is not None:
            dw = ctx.to_device(w)
            bufs.append(dw)
        if eq is not None:
            dh = ctx.to_device(eq)
            bufs.append(dh)
        _lib.check(_lib.lib.vi_eval_track_f64(es.model.handle(), lat.size, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr,
                                              dw.ptr if dw is not None else None, es.Coeffs.shape[0], bufs[4].ptr,
                                              dh.ptr if dh is not None else None, 0 if eq is None else eq.shape[0], tol,
                                              bufs[5].ptr), 'vi_eval_track_f64')
        return bufs[5].download()
    finally:
        for a in bufs:
            a.free()


def _same_bits(x, y):
    return np.array_equal(x.view(np.uint64), y.view(np.uint64))


@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'scr_k12l2'])
def test_raw_abi_point_order_and_rows_outside(tag, timeinterp):
    """The same points sorted by record and shuffled give the same bits per point; d_rec = -1, d_rec = R and - with d_w -
    d_rec = R - 1 give NaN and leave the points around them as they were."""
    lat, lon, alt, E = _reference(tag, True)
    es = _estimate(tag, timeinterp)
    mt = _mid(es.time)
    Q = lat.size
    rec, w = es.select_records(np.random.default_rng(21).uniform(mt[0], mt[-1], Q))
    order = np.argsort(rec, kind='stable')
    pick = lambda a, i: None if a is None else np.ascontiguousarray(a[i])
    srt = _raw(es, lat[order], lon[order], alt[order], rec[order], pick(w, order))
    shuffled = _raw(es, lat, lon, alt, rec, w)
    assert _same_bits(shuffled[order], srt)
    _gate(shuffled, _expected(E, rec, w), '%s raw interp=%s' % (tag, timeinterp))
    bad = rec[order].copy()
    where = {100: -1, 101: R, 500: -1, 777: R, Q - 1: R}
    if timeinterp:
        where.update({102: R - 1, 640: R - 1})
    for q, r in where.items():
        bad[q] = r
    out = _raw(es, lat[order], lon[order], alt[order], bad, pick(w, order))
    hit = np.zeros(Q, dtype=bool)
    hit[list(where)] = True
    assert np.all(np.isnan(out[hit]))
    assert _same_bits(out[~hit], srt[~hit])
    assert np.isfinite(srt[hit]).any()                  # (some of them were numbers before)


def _raw_eval(es, lat, lon, alt, C, eq, tol):
    """vi_eval_f64 of the rows C at the points, masked by the facet equations eq (None: no hull test): (T, Q) host array."""
    from volumetricinterp_amd import _lib
    ctx = es.model.ctx
    bufs = [ctx.to_device(a) for a in (lat, lon, alt, C)] + [ctx.empty((C.shape[0], lat.size))]
    try:
        dh = None
        if eq is not None:
            dh = ctx.to_device(eq)
            bufs.append(dh)
        _lib.check(_lib.lib.vi_eval_f64(es.model.handle(), lat.size, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, C.shape[0], bufs[3].ptr,
                                        dh.ptr if dh is not None else None, 0 if eq is None else eq.shape[0], tol, bufs[4].ptr),
                   'vi_eval_f64')
        return bufs[4].download()
    finally:
        for a in bufs:
            a.free()


@pytest.mark.parametrize('tag', ['default', 'k8l2'])
def test_raw_abi_buffers_regrow_on_one_handle(tag):
    """The model's grow-only buffers (hull, mask, prepared coefficients) through grow, shrink, grow on ONE handle: vi_eval_f64 at
    (Q, T, F) = (300, 3, all facets), (5000, 53, all facets) - the dispatch walks 53 as 32 + 16 + 4 + 1, every tile width on the
    freshly grown coefficient buffer; 300 is no multiple of 256 -, (300, 3, the first half of the facets: fewer facets bound a
    larger convex region), vi_eval_track_f64 with 257 points, 40 records, blending and the full hull, and vi_eval_f64 at
    (300, 3, no hull).  Every result has the NaNs and the bits of the same call on a fresh model."""
    eq, tol = _estimate(tag, True)._hull()
    F = eq.shape[0]
    C53 = _records(tag, 53)[1]
    one = _estimate(tag, True)
    mt = _mid(one.time)

    def evaluate(Q, T, eqs):
        lat, lon, alt = _box(np.random.default_rng(Q + T), Q)
        return lambda es: _raw_eval(es, lat, lon, alt, C53[:T], eqs, tol if eqs is not None else 0.)

    def track(Q):
        lat, lon, alt = _box(np.random.default_rng(Q), Q)
        rec, w = one.select_records(np.random.default_rng(Q + 1).uniform(mt[0], mt[-1], Q))
        assert w is not None and one.Coeffs.shape[0] == R
        return lambda es: _raw(es, lat, lon, alt, rec, w)

    steps = [('eval 300 x 3, all facets', evaluate(300, 3, eq)), ('eval 5000 x 53, all facets', evaluate(5000, 53, eq)),
             ('eval 300 x 3, half the facets', evaluate(300, 3, np.ascontiguousarray(eq[:F // 2]))),
             ('track 257, blending, all facets', track(257)), ('eval 300 x 3, no hull', evaluate(300, 3, None))]
    got = {}
    for what, call in steps:
        out, fresh = call(one), call(_estimate(tag, True))
        assert np.array_equal(np.isnan(out), np.isnan(fresh)), what
        ok = ~np.isnan(fresh)
        assert ok.any() and _same_bits(out[ok], fresh[ok]), what
        got[what] = ok
    full, half = got['eval 300 x 3, all facets'], got['eval 300 x 3, half the facets']
    assert 0 < full.sum() < full.size and np.all(half[full]) and got['eval 300 x 3, no hull'].all()
    assert 0 < got['eval 5000 x 53, all facets'].sum() < 5000 * 53


@pytest.mark.parametrize('timeinterp', [False, True])
def test_track_failed_fit(timeinterp):
    """Record 17 all NaN (a failed fit).  Nearest mode: exactly its points are NaN, and the points of records 16 and 18, which
    share a window with it, keep their bits.  Interpolation mode: exactly the points of the pairs that hold it, rec 16 and 17 -
    a point at w == 0 of rec 16 among them, as get_C forms 1 * C_16 + 0 * C_17."""
    lat, lon, alt, _ = _reference('k8l2', False)
    es = _estimate('k8l2', timeinterp)
    C = np.array(es.Coeffs)
    C[17] = np.nan
    broken = _estimate('k8l2', timeinterp, Coeffs=C)
    t0, rec, w = _runs(es, 5, R)
    mt = _mid(es.time)
    first16 = int(np.flatnonzero(rec == 16)[0])
    t0[first16] = mt[16]                                # exactly on the mid-time: w == 0 in interpolation mode
    rec, w = es.select_records(t0)
    assert rec[first16] == 16 and (w is None or w[first16] == 0.)
    Q = rec.size
    good = es.track(t0, lat[:Q], lon[:Q], alt[:Q], check_hull=False)
    out = broken.track(t0, lat[:Q], lon[:Q], alt[:Q], check_hull=False)
    assert np.isfinite(good).all()
    lost = np.isin(rec, [16, 17]) if timeinterp else rec == 17
    assert np.array_equal(np.isnan(out), lost)
    assert _same_bits(out[~lost], good[~lost])
    assert (~lost)[rec == 18].all() and (timeinterp or (~lost)[rec == 16].all())


# ---- the Python surface ----------------------------------------------------------------------------------------------------------

def _fixture_estimate(tag, timeinterp):
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_' + tag)
    return Estimate.from_arrays(f['Coeffs'], f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']), timeinterp=timeinterp)


@pytest.mark.parametrize('timeinterp', [False, True])
def test_track_api(timeinterp):
    from volumetricinterp_amd import synth
    es = _fixture_estimate('k8l2', timeinterp)
    mt = _mid(es.time)
    rng = np.random.default_rng(30)
    lat, lon, alt = (a[:4, :5, :6] for a in synth.query_grid(6))
    # times a datetime holds exactly, so that datetimes and float seconds are the same instants
    t0 = np.round(rng.uniform(mt[0], mt[-1] - 1., (4, 5, 6)) * 64.) / 64.
    times = np.array([_datetime(t) for t in t0.ravel()], dtype=object).reshape(t0.shape)
    out = es.track(t0, lat, lon, alt)
    assert out.shape == (4, 5, 6) and 0 < np.isnan(out).sum() < out.size
    assert _same_bits(es.track(times, lat, lon, alt), out)
    assert _same_bits(es.track(times.tolist(), lat, lon, alt), out)
    buf = np.empty((4, 5, 6))
    assert es.track(t0, lat, lon, alt, out=buf) is buf and _same_bits(buf, out)
    with pytest.raises(ValueError, match='out must be'):
        es.track(t0, lat, lon, alt, out=np.empty(120))
    with pytest.raises(ValueError, match='times must be'):
        es.track(t0.ravel()[:7], lat, lon, alt)
    # one scalar time is broadcast, and is what __call__ gives for that time
    t = _datetime(t0[1, 2, 3])
    one = es.track(t, lat, lon, alt)
    assert _same_bits(one, es.track(np.full((4, 5, 6), t0[1, 2, 3]), lat, lon, alt))
    call = es(t, lat, lon, alt)
    assert np.array_equal(np.isnan(one), np.isnan(call)) and 0 < np.isfinite(call).sum() < call.size
    ok = np.isfinite(call)
    assert rel(one[ok], call[ok]) <= DEVICE_TOL
    nohull = es.track(t, lat, lon, alt, check_hull=False)
    assert np.isfinite(nohull).all() and rel(nohull, es(t, lat, lon, alt, check_hull=False)) <= DEVICE_TOL
    # times outside the file
    late = t0.copy()
    late[0, 0, :] = mt[-1] + 4000.
    with pytest.raises(ValueError) as e:
        es.track(late, lat, lon, alt)
    assert str(e.value) == MESSAGE
    part = es.track(late, lat, lon, alt, outside='nan')
    assert np.all(np.isnan(part[0, 0])) and _same_bits(part[1:], out[1:])
    # no point: nothing to compute
    empty = es.track(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    assert empty.shape == (0, 3) and empty.dtype == np.float64
    assert es.track(t, [], [], []).shape == (0,)
