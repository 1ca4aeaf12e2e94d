"""GPU parity of the standard-error maps on a resident grid (ResidentGrid.error / evaluate_errors, vi_eval_resident_err_f64:
K2e on the matrix cores, the library's product for other shapes) against the CPU oracle, the one-timestep device path
(Estimate.error) and the host product on the same basis bits.

err[t, q] = sqrt(sum_ik Y[i, q] dC[t, i, k] Y[k, q]) with the full covariance as stored: the fits' covariances are not
symmetric and the form cancels by up to six decades, so the same-bits gate below (1e-10 norm-wise, 1e-6 at the worst point)
is one that evaluating only one triangle of dC fails on these fixtures."""
import datetime as dt
import re

import numpy as np
import pytest

from conftest import load_golden, rel

pytestmark = pytest.mark.gpu

ORACLE_TOL = 1e-8          # the gate Estimate.error meets against the oracle (its own basis, host einsum)
BITS_TOL = 1e-10           # same basis bits, another summation order: norm-wise
BITS_WORST = 1e-6          # ... and at the worst point


def _estimate(tag, timeinterp=False):
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_' + tag)
    return f, Estimate.from_arrays(f['Coeffs'], f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']),
                                   timeinterp=timeinterp)


def _oracle(tag):
    import oracle
    return {'k8l2': lambda: oracle.SphHarmLagOracle(maxk=8, maxl=2),
            'scr_k12l2': lambda: oracle.SphHarmLagOracle(maxk=12, maxl=2),
            'rbf': lambda: oracle.RadBasFunOracle(numgridpnt=3),
            'default': lambda: oracle.SphHarmLagOracle()}[tag]()


def _host_err(Y, dC):
    """The definition on the host, on the device's own basis matrix Y (N, Q): (Q,) for one covariance."""
    with np.errstate(invalid='ignore'):
        return np.sqrt(np.einsum('iq,iq->q', Y, dC @ Y))


def _same_bits(x, ref):
    """NaN pattern identical; finite values within the same-bits gate."""
    assert np.array_equal(np.isnan(x), np.isnan(ref))
    ok = np.isfinite(ref)
    assert ok.any()
    assert rel(x[ok], ref[ok]) <= BITS_TOL
    assert np.max(np.abs(x[ok] - ref[ok]) / np.abs(ref[ok])) <= BITS_WORST


def _t_mid(f):
    return dt.datetime(1970, 1, 1) + dt.timedelta(seconds=float(np.mean(f['utime'][0])))


@pytest.mark.parametrize('check_hull', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'scr_k12l2', 'rbf', 'default'])
def test_error_map_vs_oracle_and_device_paths(tag, check_hull):
    """Every fixture order (N = 32, 48, 27, 144) on the 6^3 grid: the oracle at its gate, Estimate.error (a basis built
    separately) at the same gate, and the host product on the grid's own basis bits at the same-bits gate."""
    import oracle
    from volumetricinterp_amd import synth
    f, es = _estimate(tag)
    o = _oracle(tag)
    grid = synth.query_grid(6)
    t = _t_mid(f)
    _, dC = oracle.get_C(t, f['utime'], f['Coeffs'], f['Covariance'])
    with es.resident_grid(*grid, check_hull=check_hull) as g:
        out = g.error([t])
        assert out.shape == (1, 6, 6, 6)
        ref = oracle.evaluate_error(o, dC, *grid, hull_vert=f['hull_vert'] if check_hull else None)
        ok = np.isfinite(ref)
        assert ok.sum() > 20 and np.array_equal(np.isfinite(out[0]), ok)
        assert rel(out[0][ok], ref[ok]) <= ORACLE_TOL
        dev = es.error(t, *grid, check_hull=check_hull)
        assert np.array_equal(np.isnan(out[0]), np.isnan(dev))
        assert rel(out[0][ok], dev[ok]) <= ORACLE_TOL
        _same_bits(out[0].ravel(), _host_err(g.dY.download(), dC))


@pytest.mark.parametrize('tag', ['k8l2', 'default'])
def test_error_map_time_interpolation(tag):
    """timeinterp=True: the covariance the reference's own get_C interpolated (tests/golden/eval.npz) through the oracle, and
    the reference's error for a time outside the records."""
    import oracle
    from volumetricinterp_amd import synth
    e = load_golden('eval')
    f, es = _estimate(tag, timeinterp=True)
    grid = synth.query_grid(6)
    t = dt.datetime(1970, 1, 1) + dt.timedelta(seconds=float(e[tag + '_t_int']))
    with es.resident_grid(*grid) as g:
        out = g.error([t])
        ref = oracle.evaluate_error(_oracle(tag), e[tag + '_tinterp_dC'], *grid, hull_vert=f['hull_vert'])
        assert np.array_equal(np.isnan(out[0]), np.isnan(ref))
        ok = np.isfinite(ref)
        assert ok.sum() > 20 and rel(out[0][ok], ref[ok]) <= ORACLE_TOL
        with pytest.raises(ValueError, match=re.escape(str(e[tag + '_oor']))):
            g.error([t - dt.timedelta(days=30)])


@pytest.mark.parametrize('Q', [1777, 2052, 8192 + 256])
def test_error_maps_many_timesteps(Q):
    """300 covariances (the fixture's four, each once as it is and then scaled by 4^j, j in [-4, 4]) with timestep 123 all
    NaN, on random points some outside the hull.  Q = 1777 (odd) goes through the library's product; 2052 through K2e with a
    ragged last group of points (nine workgroups per timestep), 8448 through K2e with 33 workgroups per timestep."""
    f, es = _estimate('k8l2')
    rng = np.random.default_rng(23)
    lat, lon, alt = rng.uniform(75, 81, Q), rng.uniform(250, 274, Q), rng.uniform(100e3, 700e3, Q)
    base = f['Covariance']
    idx = rng.integers(0, len(base), 300)
    j = rng.integers(-4, 5, 300)
    idx[:len(base)], j[:len(base)] = np.arange(len(base)), 0
    dC = base[idx] * (4.0 ** j)[:, None, None]
    dC[123] = np.nan
    with es.resident_grid(lat, lon, alt, check_hull=True) as g:
        out = g.evaluate_errors(dC)
        assert out.shape == (300, Q)
        Y = g.dY.download()
        for t in (0, 1, 127, 128, 255, 256, 299):
            _same_bits(out[t], _host_err(Y, dC[t]))
        # scaling by 4^j is exact in every operation: the maps scale by 2^j bit for bit
        for t in range(300):
            if t != 123:
                assert np.array_equal(out[t], 2.0 ** j[t] * out[idx[t]], equal_nan=True), t
        outside = np.isnan(g.evaluate_coeffs(f['Coeffs'][:1])[0])
        assert 0 < outside.sum() < Q
        nan = np.broadcast_to(outside, out.shape).copy()
        nan[123] = True
        assert np.array_equal(np.isnan(out), nan)


def test_error_maps_default_order_kernel_vs_library():
    """Default order (N = 144): 4096 points x 70 timesteps of the fit's own covariances (asymmetric, indefinite at rounding
    level), scaled: K2e against the library path on the same basis (the same call with an output that is not 16-byte
    aligned), at the same-bits gate, with identical NaN patterns."""
    from volumetricinterp_amd import _lib
    f, es = _estimate('default')
    rng = np.random.default_rng(5)
    Q, T = 4096, 70
    lat, lon, alt = rng.uniform(75, 81, Q), rng.uniform(250, 274, Q), rng.uniform(100e3, 700e3, Q)
    dC = f['Covariance'][np.arange(T) % 2] * (4.0 ** rng.integers(-4, 5, T))[:, None, None]
    with es.resident_grid(lat, lon, alt, check_hull=True) as g:
        own = g.evaluate_errors(dC)
        ctx = es.model.ctx
        dD, dO = ctx.to_device(dC), ctx.empty((T, Q + 1))
        try:
            _lib.check(_lib.lib.vi_eval_resident_err_f64(es.model.handle(), Q, T, g.dY.ptr, dD.ptr, dO.offset_ptr(1)),
                       'vi_eval_resident_err_f64')
            lib = dO.download().ravel()[1:1 + T * Q].reshape(T, Q)
        finally:
            dD.free()
            dO.free()
        ok = np.isfinite(lib)
        assert 0 < ok[0].sum() < Q
        _same_bits(own, lib)
        Y = g.dY.download()
        for t in (0, 69):
            _same_bits(own[t], _host_err(Y, dC[t]))


def test_error_maps_order_above_kernel_range():
    """MAXK 8 x MAXL 6 (N = 288, beyond K2e's N <= 144): the library path, against the host product on the same basis, for
    three synthetic positive definite covariances."""
    from volumetricinterp_amd import synth
    from volumetricinterp_amd.estimate import Estimate
    cfg = ('[DEFAULT]\n[MODEL]\nNAME = sphharmlag\nMAXK = 8\nMAXL = 6\nCAP_LIM = 10\nMAX_Z_INT = INF\n'
           'LATCP = 78\nLONCP = 262\n')
    N, Q, T = 288, 2048, 3
    rng = np.random.default_rng(7)
    R = rng.standard_normal((T, N, N))
    dC = R @ R.transpose(0, 2, 1) / N + np.eye(N)
    es = Estimate.from_arrays(np.zeros((T, N)), dC, synth.unix_times(T), np.zeros((4, 3)), cfg)
    assert es.model.nbasis == N
    lat, lon, alt = rng.uniform(75, 81, Q), rng.uniform(250, 274, Q), rng.uniform(100e3, 700e3, Q)
    with es.resident_grid(lat, lon, alt, check_hull=False) as g:
        out = g.evaluate_errors(dC)
        Y = g.dY.download()
        for t in range(T):
            ref = _host_err(Y, dC[t])
            assert np.isfinite(ref).all()
            _same_bits(out[t], ref)


def test_error_maps_api_edges():
    from volumetricinterp_amd import _lib, synth
    from volumetricinterp_amd.estimate import Estimate
    f, es = _estimate('k8l2')
    grid = synth.query_grid(4)
    Q = 64
    t = _t_mid(f)
    g = es.resident_grid(*grid)
    two = g.error([t, t])
    assert two.shape == (2, 4, 4, 4)
    assert np.array_equal(two[0], two[1], equal_nan=True)
    dC = f['Covariance'][:3]
    out = _lib.pinned_empty((3, Q))
    assert g.evaluate_errors(dC, out=out) is out
    assert np.array_equal(out, g.evaluate_errors(dC), equal_nan=True)
    for bad in (np.empty((2, Q)), np.empty((3, Q), dtype=np.float32), np.empty((Q, 3)).T):
        with pytest.raises(ValueError, match='out must be'):
            g.evaluate_errors(dC, out=bad)
    with pytest.raises(ValueError, match='covariances must have shape'):
        g.evaluate_errors(np.zeros((3, 31, 31)))
    with pytest.raises(ValueError, match='covariances must have shape'):
        g.evaluate_errors(np.zeros((32, 32)))
    assert g.evaluate_errors(dC[:0]).shape == (0, Q)
    assert g.error([]).shape == (0, 4, 4, 4)
    g.close()
    with pytest.raises(ValueError, match='closed'):
        g.evaluate_errors(dC)
    empty = es.resident_grid(grid[0][:0], grid[1][:0], grid[2][:0])
    assert empty.evaluate_errors(dC).shape == (3, 0)
    empty.close()
    nocov = Estimate.from_arrays(f['Coeffs'], None, f['utime'], f['hull_vert'], str(f['cfg']))
    with nocov.resident_grid(*grid) as gn:
        with pytest.raises(ValueError, match='no covariance'):
            gn.error([t])
