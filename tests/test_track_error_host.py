"""Host half of Estimate.track_error / slant_error: estimate.used_records, which picks the covariances a call uploads and
re-indexes (rec, w) of select_records into them.  No GPU: the forms are NumPy's, on the full and on the compacted stack."""
import numpy as np
import pytest

from volumetricinterp_amd.estimate import used_records

N = 5


def _stack(R, seed=3):
    """R asymmetric N x N matrices and 40 columns."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((R, N, N)), rng.standard_normal((N, 40))


def _forms(dC, Y, rec, w):
    """What vi_eval_records_err_f64 defines before its square root, by NumPy: NaN without a record or with a row >= R."""
    R = len(dC)
    out = np.full(rec.size, np.nan)
    for q, r in enumerate(rec):
        if r < 0 or r + (w is not None) >= R:
            continue
        f0 = Y[:, q] @ dC[r] @ Y[:, q]
        out[q] = f0 if w is None else (1 - w[q]) * f0 + w[q] * (Y[:, q] @ dC[r + 1] @ Y[:, q])
    return out


def _check(rec, w, R):
    """The contract of used_records on one input; returns (rows, compact)."""
    rec = np.asarray(rec, dtype=np.int32)
    rows, compact = used_records(rec, w, R)
    assert compact.dtype == np.int32 and compact.shape == rec.shape
    assert np.all(np.diff(rows) > 0) and np.all((rows >= 0) & (rows < R))
    need = set()
    for r in rec.ravel():
        if r >= 0:
            need.update(x for x in ((r,) if w is None else (r, r + 1)) if x < R)
    assert set(rows.tolist()) == need                                         # what is needed and nothing else
    flat, cflat = rec.ravel(), compact.ravel()
    assert np.array_equal(cflat[flat < 0], np.full((flat < 0).sum(), -1))     # -1 is kept
    for r, c in zip(flat, cflat):
        if r < 0:
            continue
        if r < R:
            assert rows[c] == r
            if w is not None:                                                 # the pair stays adjacent, or runs off the end
                assert (rows[c + 1] == r + 1) if r + 1 < R else (c + 1 >= len(rows))
        else:
            assert c >= len(rows)                                             # a row >= R stays a row >= len(rows)
    return rows, compact


@pytest.mark.parametrize('interp', [False, True])
def test_used_records_cases(interp):
    R = 9
    rng = np.random.default_rng(1)
    w = (lambda n: rng.random(n)) if interp else (lambda n: None)
    _check([], w(0), R)                                                       # empty input
    rows, c = _check([4, 4, 4], w(3), R)                                      # one record
    assert rows.tolist() == ([4, 5] if interp else [4]) and c.tolist() == [0, 0, 0]
    rows, c = _check(np.arange(R), w(R), R)                                   # all records
    assert rows.tolist() == list(range(R)) and c.tolist() == list(range(R))
    _check([-1, -1], w(2), R)                                                 # no record at all
    rows, c = _check([7, -1, 2, 2, 8, 0, -1, 7], w(8), R)                     # unsorted, -1 between, the last row
    assert c[1] == -1 and c[6] == -1
    rows, c = _check([3, 9, 12, 8, -1], w(5), R)                              # rows >= R
    assert c[1] >= len(rows) and c[2] >= len(rows)
    if interp:
        assert c[3] + 1 >= len(rows)                                          # R - 1 with a weight needs row R
    _check(np.array([[0, 5, 5], [6, -1, 2]]), None if not interp else rng.random((2, 3)), R)   # the shape is kept
    _check([1, 2], w(2), 0)                                                   # R = 0: no row to upload
    assert used_records(np.array([1, 2]), w(2), 0)[0].size == 0


@pytest.mark.parametrize('interp', [False, True])
def test_forms_from_the_compacted_stack_are_the_same(interp):
    """The forms computed from Covariance[rows] with the compacted records equal those of the full stack exactly: the same
    matrices enter the same operations."""
    R = 12
    dC, Y = _stack(R)
    rng = np.random.default_rng(8)
    rec = rng.choice([-1, 0, 3, 4, 7, 10, 11, 12, 15], size=Y.shape[1]).astype(np.int32)
    w = rng.random(rec.size) if interp else None
    rows, compact = used_records(rec, w, R)
    assert 0 < len(rows) < R
    full = _forms(dC, Y, rec, w)
    small = _forms(dC[rows], Y, compact, w)
    assert 0 < np.isnan(full).sum() < full.size
    assert np.array_equal(full.view(np.uint64), small.view(np.uint64))


def test_methods_raise_without_a_covariance():
    """Both methods refuse an Estimate without covariances before anything reaches the device."""
    from volumetricinterp_amd.estimate import Estimate
    es = Estimate.__new__(Estimate)
    es.Covariance = None
    with pytest.raises(ValueError, match='no covariance'):
        es.track_error(0., [78.], [262.], [300e3])
    with pytest.raises(ValueError, match='no covariance'):
        es.slant_error(0., (78., 262., 0.), (79., 262., 1e6))
