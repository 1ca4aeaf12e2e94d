"""Host side of the column-map errors (ResidentGrid.errors_at / peak_error / integrate_error): column_points, the flat point
index of a position along one axis per column, and the binding of vi_eval_resident_err_at_f64.  No GPU."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 7, 6), (4,), (258, 2)]


def _cases():
    for shape in SHAPES:
        for axis in range(len(shape)):
            yield shape, axis


def _index(rng, shape, axis, T=3):
    """Random positions in [0, L) per (t, column), the ends forced: (T, M), and the same as (T,) + the shape without axis."""
    L = shape[axis]
    rest = shape[:axis] + shape[axis + 1:]
    M = int(np.prod(rest, dtype=np.int64))
    idx = rng.integers(0, L, (T, M)).astype(np.int32)
    idx[0, 0], idx[-1, -1] = 0, L - 1
    return idx, rest


@pytest.mark.parametrize('shape,axis', list(_cases()))
def test_column_points_is_ravel_multi_index(shape, axis):
    from volumetricinterp_amd.estimate import column_points
    rng = np.random.default_rng(len(shape) * 10 + axis)
    idx, rest = _index(rng, shape, axis)
    T, M = idx.shape
    # the multi-index of column m in C order of the remaining axes, with the position along `axis` put back in its place
    cols = np.unravel_index(np.arange(M), rest) if rest else ()
    for t in range(T):
        multi = list(cols[:axis]) + [idx[t]] + list(cols[axis:])
        ref = np.ravel_multi_index(multi, shape)
        q = column_points(shape, axis, idx[t:t + 1])
        assert q.shape == (1, M) and q.dtype == np.int64
        assert np.array_equal(q[0], ref)
        assert np.array_equal(column_points(shape, axis - len(shape), idx[t:t + 1]), q)     # the axis counted from the end
    # what it is for: picking one value per column out of a volume
    vol = rng.standard_normal((T,) + shape)
    picked = np.take_along_axis(vol.reshape(T, -1), column_points(shape, axis, idx), 1)
    ref = np.take_along_axis(vol, np.expand_dims(idx.reshape((T,) + rest), axis + 1), axis + 1)
    assert np.array_equal(picked, ref.reshape(T, M))


@pytest.mark.parametrize('shape,axis', list(_cases()))
def test_minus_one_passes_through(shape, axis):
    from volumetricinterp_amd.estimate import column_points
    rng = np.random.default_rng(5)
    idx, _ = _index(rng, shape, axis)
    full = column_points(shape, axis, idx)
    idx[1] = -1
    idx[0, -1] = -1
    q = column_points(shape, axis, idx)
    assert np.all(q[1] == -1) and q[0, -1] == -1
    keep = idx >= 0
    assert np.array_equal(q[keep], full[keep]) and np.all(q[keep] >= 0)
    assert column_points(shape, axis, idx.astype(np.int64)).tolist() == q.tolist()
    assert column_points(shape, axis, np.empty((0, idx.shape[1]), np.int32)).shape == (0, idx.shape[1])


def test_column_points_refuses():
    from volumetricinterp_amd.estimate import column_points
    shape, axis = (5, 7, 6), 1
    L, M = 7, 30
    ok = np.zeros((2, M), np.int32)
    for bad_value in (L, -2):
        idx = ok.copy()
        idx[1, 3] = bad_value
        with pytest.raises(ValueError, match='index must lie in'):
            column_points(shape, axis, idx)
    with pytest.raises(ValueError, match='integer'):
        column_points(shape, axis, ok.astype(np.float64))
    with pytest.raises(ValueError, match='integer'):
        column_points(shape, axis, ok.astype(bool))
    for bad_shape in ((2, M + 1), (M,), (2, 5, 6), (2, M, 1)):
        with pytest.raises(ValueError, match='index must have shape'):
            column_points(shape, axis, np.zeros(bad_shape, np.int32))
    for bad_axis in (3, -4, 1.0, None, True):
        with pytest.raises(ValueError, match='axis'):
            column_points(shape, bad_axis, ok)
    with pytest.raises(ValueError, match='0-d'):
        column_points((), 0, np.zeros((1, 1), np.int32))


def test_entry_is_declared_and_bound():
    """vi_eval_resident_err_at_f64 is declared in include/vinterp.h with the signature the issue of this feature fixes, has
    a ctypes signature and is listed among the exports; the ABI version is still 2."""
    from volumetricinterp_amd import _lib
    txt = open(os.path.join(REPO, 'include', 'vinterp.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    m = re.search(r'int\s+vi_eval_resident_err_at_f64\s*\(([^)]*)\)\s*;', code)
    assert m, 'not declared'
    args = [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]
    assert args == ['vi_model* model', 'int64_t outer', 'int64_t L', 'int64_t inner', 'int64_t T', 'const double* d_Y',
                    'const double* d_dC', 'const int32_t* d_idx', 'double* d_out']
    assert 'vi_eval_resident_err_at_f64' in _lib.EXPORTS
    f = _lib.lib.vi_eval_resident_err_at_f64
    assert len(f.argtypes) == 9 and f.argtypes[1:5] == [_lib.I64] * 4
    assert _lib.lib.vi_abi_version() == 2
    assert 'K2eg' in txt          # the header comment says which kernel serves the entry
