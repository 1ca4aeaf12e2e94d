"""select_records (volumetricinterp_amd/estimate.py): the record Estimate.get_C selects for a time, for many times at once, against
a Python loop over get_C itself (the package's and the oracle's, both restating estimate.py:180-221).  Host arithmetic only."""
import datetime as dt

import numpy as np
import pytest

import oracle
from volumetricinterp_amd.estimate import Estimate, select_records

EPOCH = dt.datetime(1970, 1, 1)
MESSAGE = 'Requested time out of range of data file.'
R, N = 7, 5
CFG = ('[DEFAULT]\n[MODEL]\nNAME = sphharmlag\nMAXK = 4\nMAXL = 6\nCAP_LIM = 10\nMAX_Z_INT = INF\nLATCP = 78\nLONCP = 262\n')


def _time(kind):
    """(R, 2) start / end times whose mid-times are 60 s apart: increasing, with one mid-time twice, or shuffled."""
    mt = 1480286730. + 60. * np.arange(R)
    if kind == 'repeated':
        mt[3] = mt[2]
    elif kind == 'shuffled':
        mt = mt[np.random.default_rng(3).permutation(R)]
        assert np.any(np.diff(mt) < 0)
    time = np.stack([mt - 30., mt + 30.], axis=1)
    assert np.array_equal(np.mean(time, axis=1), mt)
    return time, mt


def _queries(mt, timetol):
    """datetimes at the places where the selection can go wrong, and their unix seconds as get_C forms them."""
    s = np.unique(mt)
    t0 = np.concatenate([
        mt,                                             # exactly on a mid-time (mt[0] and mt[-1] among them)
        0.5 * (s[:-1] + s[1:]),                         # exactly half-way between two: the tie
        [s[0] - timetol, s[-1] + timetol],              # at timetol exactly
        [s[0] - timetol - 1e-3, s[-1] + timetol + 1e-3],        # just beyond
        [s[0] - 4000., s[-1] + 4000.],                  # before and after all records
        s[:-1] + 7.25, s[:-1] + 45.5, s[1:] - 1e-3])    # in between
    times = [EPOCH + dt.timedelta(seconds=float(x)) for x in t0]
    return times, np.array([(t - EPOCH).total_seconds() for t in times])


def _loop(get_C, times, Coeffs, timeinterp):
    """rows[q]: get_C's coefficient row for times[q], or None where it raises the reference's error."""
    rows = []
    for t in times:
        try:
            rows.append(np.array(get_C(t)[0]))
        except ValueError as e:
            assert str(e) == MESSAGE
            rows.append(None)
    return rows


@pytest.mark.parametrize('timetol', [60., 20.])
@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('kind', ['increasing', 'repeated', 'shuffled'])
def test_select_records_is_get_C_per_element(kind, timeinterp, timetol):
    time, mt = _time(kind)
    rng = np.random.default_rng(11)
    Coeffs, Cov = rng.standard_normal((R, N)), np.zeros((R, 1, 1))
    times, t0 = _queries(mt, timetol)
    rows = _loop(lambda t: oracle.get_C(t, time, Coeffs, Cov, timetol=timetol, timeinterp=timeinterp), times, Coeffs, timeinterp)
    inside = np.array([r is not None for r in rows])
    assert inside.any() and not inside.all()
    rec, w = select_records(time, t0, timetol=timetol, timeinterp=timeinterp, outside='nan')
    assert rec.dtype == np.int32 and rec.shape == t0.shape
    assert np.array_equal(rec >= 0, inside)                     # 'nan': -1 exactly where get_C raises
    if timeinterp:
        assert w.dtype == np.float64 and w.shape == t0.shape and np.all(w[~inside] == 0.)
        assert np.all(rec[t0 == mt.max()] == -1)                # the last mid-time itself is out of range, as in the reference
    else:
        assert w is None
    for q in np.flatnonzero(inside):
        if timeinterp:
            want = np.argwhere((t0[q] >= mt[:-1]) & (t0[q] < mt[1:])).flatten()[0]
            row = (1 - w[q]) * Coeffs[rec[q]] + w[q] * Coeffs[rec[q] + 1]
        else:
            want = np.argmin(np.abs(mt - t0[q]))
            row = Coeffs[rec[q]]
        assert rec[q] == want, (q, t0[q])
        assert row.tobytes() == rows[q].tobytes(), (q, t0[q])    # bit for bit get_C's row
    with pytest.raises(ValueError) as e:
        select_records(time, t0, timetol=timetol, timeinterp=timeinterp, outside='raise')
    assert str(e.value) == MESSAGE
    rec_in, w_in = select_records(time, t0[inside], timetol=timetol, timeinterp=timeinterp)       # 'raise' is the default
    assert np.array_equal(rec_in, rec[inside]) and (w is None or np.array_equal(w_in, w[inside]))


@pytest.mark.parametrize('timeinterp', [False, True])
def test_select_records_keeps_the_shape(timeinterp):
    time, mt = _time('increasing')
    t0 = np.random.default_rng(5).uniform(mt[0], mt[-1] - 1., (3, 5))
    rec, w = select_records(time, t0, timeinterp=timeinterp)
    flat, wf = select_records(time, t0.ravel(), timeinterp=timeinterp)
    assert rec.shape == (3, 5) and np.array_equal(rec.ravel(), flat)
    assert (w is None) if not timeinterp else (w.shape == (3, 5) and np.array_equal(w.ravel(), wf))
    rec0, w0 = select_records(time, np.float64(t0[1, 2]), timeinterp=timeinterp)
    assert rec0.shape == () and rec0 == rec[1, 2] and rec0.dtype == np.int32
    assert (w0 is None) if not timeinterp else (w0.shape == () and w0 == w[1, 2])
    with pytest.raises(ValueError, match='outside'):
        select_records(time, t0, outside='clip')


@pytest.mark.parametrize('timeinterp', [False, True])
def test_estimate_select_records_takes_datetimes(timeinterp):
    """The method over it: this Estimate's records, timetol and timeinterp; datetimes and float seconds alike."""
    time, mt = _time('increasing')
    rng = np.random.default_rng(2)
    Coeffs = rng.standard_normal((R, 144))
    es = Estimate.from_arrays(Coeffs, np.zeros((R, 1, 1)), time, np.zeros((4, 3)), CFG, timetol=20., timeinterp=timeinterp)
    times, t0 = _queries(mt, 20.)
    rows = _loop(es.get_C, times, Coeffs, timeinterp)
    inside = np.array([r is not None for r in rows])
    rec, w = es.select_records(times, outside='nan')
    rec_f, w_f = es.select_records(t0, outside='nan')
    assert np.array_equal(rec, rec_f) and (w is None or np.array_equal(w, w_f))
    assert np.array_equal(rec >= 0, inside)
    for q in np.flatnonzero(inside):
        row = Coeffs[rec[q]] if not timeinterp else (1 - w[q]) * Coeffs[rec[q]] + w[q] * Coeffs[rec[q] + 1]
        assert row.tobytes() == rows[q].tobytes()
    with pytest.raises(ValueError) as e:
        es.select_records(times)
    assert str(e.value) == MESSAGE
    assert es.select_records(times[0])[0].shape == ()
