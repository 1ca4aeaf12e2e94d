"""GPU parity of the gradient along a trajectory (Estimate.track_gradient, vi_eval_track_grad_f64, kernel K2tg: every point at its
own time, one library call) against an independent device path - Estimate.gradient of EVERY record at all points (k_grad_sph, one
call per record, the frame as tested), then the element (or the blend of two) that Estimate.select_records names - and against
the CPU oracle's grad_basis contracted with oracle.get_C's row.

Gates, the project's own for the gradient: between the two device paths the NaN pattern is identical and the finite values agree
to 1e-12 norm-wise per component (tests/test_gpu_basis_eval.py, tests/test_gpu_resident_gradient.py: two device summation orders
of one contraction); against the oracle 1e-10 (gate L6, test_estimate_gradient_vs_oracle).  The helpers follow
tests/test_gpu_track.py: the same 40 records, the same box and seeds."""
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
FRAMES = ['model', 'enu']
ORDERS = {'default': dict(), 'k8l2': dict(maxk=8, maxl=2), 'scr_k12l2': dict(maxk=12, maxl=2)}


@functools.lru_cache(maxsize=None)
def _records(tag, nrec=R):
    """(fixture, Coeffs, time): nrec records, each a finite fixture coefficient row times a power of two - the rows differ and
    keep their bits -, mid-times 60 s apart."""
    from volumetricinterp_amd import synth
    f = load_golden('fit_' + tag)
    rows = f['Coeffs'][np.all(np.isfinite(f['Coeffs']), axis=1)]
    rng = np.random.default_rng(40)
    C = rows[rng.integers(len(rows), size=nrec)] * 2. ** rng.integers(-3, 4, size=nrec)[:, None]
    C.setflags(write=False)
    return f, C, synth.unix_times(nrec)


def _estimate(tag, timeinterp, nrec=R, Coeffs=None):
    """An Estimate of the nrec records.  get_C indexes the covariance, nothing here evaluates it: one zero matrix, broadcast."""
    from volumetricinterp_amd.estimate import Estimate
    f, C, time = _records(tag, nrec)
    C = C if Coeffs is None else Coeffs
    cov = np.broadcast_to(np.zeros((1, C.shape[1], C.shape[1])), (nrec, C.shape[1], C.shape[1]))
    return Estimate.from_arrays(C, cov, time, f['hull_vert'], str(f['cfg']), timeinterp=timeinterp)


def _box(rng, Q):
    """Random points in the box of the resident tests: some of it lies outside the hull."""
    return rng.uniform(75, 81, Q), rng.uniform(250, 274, Q), rng.uniform(100e3, 700e3, Q)


def _mid(time):
    return np.mean(time, axis=1)


def _datetime(t0):
    return EPOCH + dt.timedelta(seconds=float(t0))


@functools.lru_cache(maxsize=None)
def _reference(tag, check_hull, frame, Q=1000, nrec=R, seed=7):
    """(lat, lon, alt, E): Q points and the gradients E (nrec, Q, 3) of every record at them, one Estimate.gradient call per
    record at the record's mid-time (nearest mode: get_C gives the record's own row)."""
    lat, lon, alt = _box(np.random.default_rng(seed), Q)
    es = _estimate(tag, False, nrec)
    E = np.array([es.gradient(_datetime(m), lat, lon, alt, check_hull=check_hull, frame=frame) for m in _mid(es.time)])
    assert E.shape == (nrec, Q, 3)
    for a in (lat, lon, alt, E):
        a.setflags(write=False)
    return lat, lon, alt, E


def _expected(E, rec, w):
    """The triple of E the record selection names, or the blend of two as vi_eval_track_grad_f64 defines it; NaN without a
    record."""
    q = np.arange(rec.size)
    r = np.maximum(rec, 0)
    out = E[r, q] if w is None else (1 - w)[:, None] * E[r, q] + w[:, None] * E[np.minimum(r + 1, E.shape[0] - 1), q]
    out[rec < 0] = np.nan
    return out


def _gate(out, exp, what=''):
    """Identical NaN pattern, whole triples only, and every component within DEVICE_TOL norm-wise."""
    assert out.shape == exp.shape and out.shape[-1] == 3
    assert np.array_equal(np.isnan(out), np.isnan(exp)), what
    bad = np.isnan(exp).any(axis=-1)
    assert np.array_equal(np.isnan(exp).all(axis=-1), bad), what
    ok = ~bad
    assert ok.any(), what
    for c in range(3):
        err = rel(out[ok, c], exp[ok, c])
        print('%s component %d: rel %.2e on %d finite of %d' % (what, c, err, ok.sum(), ok.size))
        assert err <= DEVICE_TOL, (what, c, err)


def _same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('frame', FRAMES)
@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('check_hull', [False, True])
@pytest.mark.parametrize('tag', ['default', 'k8l2', 'scr_k12l2'])
def test_track_gradient_parity(tag, check_hull, timeinterp, frame):
    """1000 random points at random times over the records' range, unsorted, at the three compiled caps: default (6, 4), k8l2
    (2, 8) under the cap (12, 8), scr_k12l2 (2, 12)."""
    import oracle
    lat, lon, alt, E = _reference(tag, check_hull, frame)
    es = _estimate(tag, timeinterp)
    mt = _mid(es.time)
    t0 = np.random.default_rng(12).uniform(mt[0], mt[-1], lat.size)
    rec, w = es.select_records(t0)
    assert len(np.unique(rec)) == (R - 1 if timeinterp else R) and np.any(np.diff(rec) < 0)      # every record, and unsorted
    out = es.track_gradient(t0, lat, lon, alt, check_hull=check_hull, frame=frame)
    exp = _expected(E, rec, w)
    nans = int(np.isnan(exp).any(axis=-1).sum())
    assert (0 < nans < lat.size) if check_hull else np.isfinite(exp).all()
    _gate(out, exp, '%s hull=%s interp=%s %s' % (tag, check_hull, timeinterp, frame))
    if not check_hull and frame == 'model':
        o = oracle.SphHarmLagOracle(**ORDERS[tag])
        cov = np.zeros((R, 1, 1))
        # datetimes carry microseconds: the 50 points are evaluated again at times a datetime holds exactly
        t50 = np.array([(_datetime(t) - EPOCH).total_seconds() for t in t0[:50]])
        out50 = es.track_gradient(t50, lat[:50], lon[:50], alt[:50], check_hull=False)
        ref = np.array([oracle.evaluate_gradient(o, oracle.get_C(_datetime(t50[q]), es.time, es.Coeffs, cov,
                                                                 timeinterp=timeinterp)[0],
                                                 lat[q:q + 1], lon[q:q + 1], alt[q:q + 1])[0] for q in range(50)])
        for c in range(3):
            err = rel(out50[:, c], ref[:, c])
            print('%s interp=%s component %d against the oracle: rel %.2e' % (tag, timeinterp, c, err))
            assert err <= ORACLE_TOL, (c, err)


# ---- 2. definition -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('frame', FRAMES)
@pytest.mark.parametrize('timeinterp', [False, True])
def test_track_gradient_is_gradient_per_point(timeinterp, frame):
    """20 single points: track_gradient on the one point is Estimate.gradient at the point's time (in interpolation mode the
    gradient of get_C's blended row: the same number to rounding, the gradient being linear in the coefficients)."""
    lat, lon, alt = _box(np.random.default_rng(7), 1000)
    es = _estimate('default', timeinterp)
    mt = _mid(es.time)
    t0 = np.round(np.random.default_rng(3).uniform(mt[0], mt[-1] - 1., 20) * 64.) / 64.          # a datetime holds them exactly
    got = np.array([es.track_gradient(t0[q], lat[q], lon[q], alt[q], check_hull=False, frame=frame) for q in range(20)])
    exp = np.array([es.gradient(_datetime(t0[q]), lat[q], lon[q], alt[q], check_hull=False, frame=frame) for q in range(20)])
    assert got.shape == (20, 3) and np.isfinite(exp).all()
    _gate(got, exp, 'definition interp=%s %s' % (timeinterp, frame))
    hull = np.array([es.track_gradient(t0[q], lat[q], lon[q], alt[q], frame=frame) for q in range(20)])
    exph = np.array([es.gradient(_datetime(t0[q]), lat[q], lon[q], alt[q], frame=frame) for q in range(20)])
    assert np.array_equal(np.isnan(hull), np.isnan(exph))
    assert _same_bits(hull[np.isfinite(hull)], got[np.isfinite(hull)])


# ---- 3. geometry of the windows (k8l2, N = 32: the window logic does not depend on the order) -------------------------------------

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
@pytest.mark.parametrize('p', [1, 2, 3, 5, 64, 100])
def test_track_gradient_runs_of_points_per_record(p, timeinterp):
    """p points on each of the 40 records: every alignment of a window boundary against a wave of 64 points occurs, whatever
    the window width."""
    lat, lon, alt, E = _reference('k8l2', True, 'model', Q=R * 100, seed=8)
    es = _estimate('k8l2', timeinterp)
    t0, rec, w = _runs(es, p, R)
    Q = rec.size
    out = es.track_gradient(t0, lat[:Q], lon[:Q], alt[:Q])
    exp = _expected(E[:, :Q], rec, w)
    if p >= 5:
        assert 0 < np.isnan(exp).any(axis=-1).sum() < Q
    _gate(out, exp, 'p=%d interp=%s' % (p, timeinterp))


@pytest.mark.parametrize('timeinterp', [False, True])
def test_track_gradient_span_wider_than_a_wave(timeinterp):
    """300 records with one point each: a wave of 64 points spans 64 records, many windows."""
    lat, lon, alt, E = _reference('k8l2', False, 'model', Q=300, nrec=300, seed=9)
    es = _estimate('k8l2', timeinterp, nrec=300)
    t0, rec, w = _runs(es, 1, 300)
    Q = rec.size
    out = es.track_gradient(t0, lat[:Q], lon[:Q], alt[:Q], check_hull=False)
    assert np.isfinite(out).all()
    _gate(out, _expected(E[:, :Q], rec, w), 'R=300 interp=%s' % timeinterp)


@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('Q', [1, 63, 257])
def test_track_gradient_small_and_odd_sizes(Q, timeinterp):
    lat, lon, alt, E = _reference('k8l2', False, 'model')
    es = _estimate('k8l2', timeinterp)
    mt = _mid(es.time)
    t0 = np.random.default_rng(Q).uniform(mt[0], mt[-1], Q)
    t0[-1] = mt[-1] if not timeinterp else mt[-1] - 1.          # the last row / the pair that ends on it
    rec, w = es.select_records(t0)
    assert rec[-1] == (R - 1 if not timeinterp else R - 2)
    out = es.track_gradient(t0, lat[:Q], lon[:Q], alt[:Q], check_hull=False)
    assert np.isfinite(out).all()
    _gate(out, _expected(E[:, :Q], rec, w), 'Q=%d interp=%s' % (Q, timeinterp))


# ---- 4. the C entry itself ---------------------------------------------------------------------------------------------------------

def _raw(es, lat, lon, alt, rec, w, check_hull=True, frame=0, nrows=None, status=False):
    """vi_eval_track_grad_f64 on the points as given (no sorting): (Q, 3) host array; with status=True the call's return code
    instead.  nrows: the R handed to the call (default: all rows)."""
    from volumetricinterp_amd import _lib
    ctx = es.model.ctx
    eq, tol = es._hull() if check_hull else (None, 0.)
    bufs = []
    try:
        for a in (lat, lon, alt):
            bufs.append(ctx.to_device(a))
        bufs.append(ctx.to_device(rec, np.int32))
        bufs.append(ctx.to_device(es.Coeffs))
        bufs.append(ctx.empty((lat.size, 3)))
        dw = dh = None
        if w is not None:
            dw = ctx.to_device(w)
            bufs.append(dw)
        if eq is not None:
            dh = ctx.to_device(eq)
            bufs.append(dh)
        rc = _lib.lib.vi_eval_track_grad_f64(es.model.handle(), lat.size, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr,
                                             dw.ptr if dw is not None else None, es.Coeffs.shape[0] if nrows is None else nrows,
                                             bufs[4].ptr, dh.ptr if dh is not None else None, 0 if eq is None else eq.shape[0],
                                             tol, frame, bufs[5].ptr)
        if status:
            return rc
        _lib.check(rc, 'vi_eval_track_grad_f64')
        return bufs[5].download()
    finally:
        for a in bufs:
            a.free()


def _pick(a, i):
    return None if a is None else np.ascontiguousarray(a[i])


@pytest.mark.parametrize('frame', [0, 1])
@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('tag', ['default', 'k8l2'])
def test_raw_abi_point_order_and_rows_outside(tag, timeinterp, frame):
    """The same points sorted by record and shuffled give the same bits per point; d_rec = -1, d_rec = R and - with d_w -
    d_rec = R - 1 give NaN triples and leave the points around them, in the same wave, as they were; R = 0 gives all NaN."""
    lat, lon, alt, E = _reference(tag, True, FRAMES[frame])
    es = _estimate(tag, timeinterp)
    mt = _mid(es.time)
    Q = lat.size
    rec, w = es.select_records(np.random.default_rng(21).uniform(mt[0], mt[-1], Q))
    order = np.argsort(rec, kind='stable')
    srt = _raw(es, lat[order], lon[order], alt[order], rec[order], _pick(w, order), frame=frame)
    shuffled = _raw(es, lat, lon, alt, rec, w, frame=frame)
    assert _same_bits(shuffled[order], srt)
    _gate(shuffled, _expected(E, rec, w), '%s raw interp=%s frame=%d' % (tag, timeinterp, frame))
    bad = rec[order].copy()
    where = {100: -1, 101: R, 500: -1, 777: R, Q - 1: R}
    if timeinterp:
        where.update({102: R - 1, 640: R - 1})
    for q, r in where.items():
        bad[q] = r
    out = _raw(es, lat[order], lon[order], alt[order], bad, _pick(w, order), frame=frame)
    hit = np.zeros(Q, dtype=bool)
    hit[list(where)] = True
    assert np.all(np.isnan(out[hit]))
    assert _same_bits(out[~hit], srt[~hit])
    assert np.isfinite(srt[hit]).any()                  # (some of them were numbers before)
    assert np.all(np.isnan(_raw(es, lat, lon, alt, rec, w, frame=frame, nrows=0)))


@pytest.mark.parametrize('timeinterp', [False, True])
def test_raw_abi_hull_and_frame_argument(timeinterp):
    """F = 0 and F > 0 agree bit for bit on the points inside the hull; a frame that is neither value is an argument error."""
    lat, lon, alt, _ = _reference('default', True, 'model')
    es = _estimate('default', timeinterp)
    mt = _mid(es.time)
    rec, w = es.select_records(np.random.default_rng(22).uniform(mt[0], mt[-1], lat.size))
    masked = _raw(es, lat, lon, alt, rec, w, check_hull=True)
    free = _raw(es, lat, lon, alt, rec, w, check_hull=False)
    inside = np.isfinite(masked).all(axis=-1)
    assert 0 < inside.sum() < lat.size and np.all(np.isnan(masked[~inside])) and np.isfinite(free).all()
    assert _same_bits(masked[inside], free[inside])
    for frame in (2, -1):
        assert _raw(es, lat, lon, alt, rec, w, frame=frame, status=True) == -1            # VI_ERR_INVALID


# ---- 5. failed fits ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('timeinterp', [False, True])
def test_track_gradient_failed_fits(timeinterp):
    """Records 17 and 30 all NaN (failed fits).  Nearest mode: exactly their points are NaN.  Interpolation mode: exactly the
    points of the pairs that hold one of them, rec 16, 17, 29 and 30 - a point at w == 0 of rec 16 among them, as get_C forms
    1 * C_16 + 0 * C_17.  Every other point keeps its bits."""
    lat, lon, alt = _box(np.random.default_rng(7), 1000)
    es = _estimate('k8l2', timeinterp)
    C = np.array(es.Coeffs)
    C[[17, 30]] = np.nan
    broken = _estimate('k8l2', timeinterp, Coeffs=C)
    t0, rec, w = _runs(es, 5, R)
    mt = _mid(es.time)
    first16 = int(np.flatnonzero(rec == 16)[0])
    t0[first16] = mt[16]                                # exactly on the mid-time: w == 0 in interpolation mode
    rec, w = es.select_records(t0)
    assert rec[first16] == 16 and (w is None or w[first16] == 0.)
    Q = rec.size
    good = es.track_gradient(t0, lat[:Q], lon[:Q], alt[:Q], check_hull=False)
    out = broken.track_gradient(t0, lat[:Q], lon[:Q], alt[:Q], check_hull=False)
    assert np.isfinite(good).all()
    lost = np.isin(rec, [16, 17, 29, 30]) if timeinterp else np.isin(rec, [17, 30])
    assert np.array_equal(np.isnan(out), np.repeat(lost[:, None], 3, axis=1))
    assert _same_bits(out[~lost], good[~lost])
    assert (~lost)[np.isin(rec, [18, 31])].all() and (timeinterp or (~lost)[np.isin(rec, [16, 29])].all())


# ---- 6. the Python surface ---------------------------------------------------------------------------------------------------------

def _fixture_estimate(tag, timeinterp):
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_' + tag)
    return Estimate.from_arrays(f['Coeffs'], f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']), timeinterp=timeinterp)


@pytest.mark.parametrize('timeinterp', [False, True])
def test_track_gradient_api(timeinterp):
    from volumetricinterp_amd import synth
    es = _fixture_estimate('k8l2', timeinterp)
    mt = _mid(es.time)
    rng = np.random.default_rng(30)
    lat, lon, alt = (a[:4, :5, :6] for a in synth.query_grid(6))
    # times a datetime holds exactly, so that datetimes and float seconds are the same instants
    t0 = np.round(rng.uniform(mt[0], mt[-1] - 1., (4, 5, 6)) * 64.) / 64.
    times = np.array([_datetime(t) for t in t0.ravel()], dtype=object).reshape(t0.shape)
    out = es.track_gradient(t0, lat, lon, alt)
    assert out.shape == (4, 5, 6, 3) and 0 < np.isnan(out).sum() < out.size
    assert _same_bits(es.track_gradient(times, lat, lon, alt), out)
    assert _same_bits(es.track_gradient(times.tolist(), lat, lon, alt), out)
    buf = np.empty((4, 5, 6, 3))
    assert es.track_gradient(t0, lat, lon, alt, out=buf) is buf and _same_bits(buf, out)
    for wrong in (np.empty((4, 5, 6)), np.empty(360), np.empty((4, 5, 6, 3), dtype=np.float32)):
        with pytest.raises(ValueError, match='out must be'):
            es.track_gradient(t0, lat, lon, alt, out=wrong)
    with pytest.raises(ValueError, match='times must be'):
        es.track_gradient(t0.ravel()[:7], lat, lon, alt)
    with pytest.raises(ValueError, match="frame must be 'model' or 'enu'"):
        es.track_gradient(t0, lat, lon, alt, frame='xyz')
    # one scalar time is broadcast, and is what gradient gives for that time
    t = _datetime(t0[1, 2, 3])
    for frame in FRAMES:
        one = es.track_gradient(t, lat, lon, alt, frame=frame)
        assert _same_bits(one, es.track_gradient(np.full((4, 5, 6), t0[1, 2, 3]), lat, lon, alt, frame=frame))
        call = es.gradient(t, lat, lon, alt, frame=frame)
        assert 0 < np.isfinite(call).sum() < call.size
        _gate(one, call, 'scalar time interp=%s %s' % (timeinterp, frame))
    # times outside the file
    late = t0.copy()
    late[0, 0, :] = mt[-1] + 4000.
    with pytest.raises(ValueError) as e:
        es.track_gradient(late, lat, lon, alt)
    assert str(e.value) == MESSAGE
    part = es.track_gradient(late, lat, lon, alt, outside='nan')
    assert np.all(np.isnan(part[0, 0])) and _same_bits(part[1:], out[1:])
    # no point: nothing to compute
    empty = es.track_gradient(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    assert empty.shape == (0, 3, 3) and empty.dtype == np.float64
    assert es.track_gradient(t, [], [], []).shape == (0, 3)
    # the kernel's device time
    ctx = es.model.ctx
    ctx.eval_timing(True)
    try:
        es.track_gradient(t0, lat, lon, alt)
        assert ctx.eval_kernel_ms() > 0.
    finally:
        ctx.eval_timing(False)


def test_track_gradient_rbf_raises():
    """The RBF model has no gradient basis: what Estimate.gradient raises for it."""
    from volumetricinterp_amd import _lib
    es = _fixture_estimate('rbf', False)
    mt = _mid(es.time)
    lat, lon, alt = _box(np.random.default_rng(1), 10)
    with pytest.raises(_lib.VinterpError, match='only the sphharmlag model provides a gradient basis') as e:
        es.gradient(_datetime(mt[0]), lat, lon, alt)
    with pytest.raises(type(e.value), match='only the sphharmlag model provides a gradient basis'):
        es.track_gradient(np.full(10, mt[0]), lat, lon, alt)
