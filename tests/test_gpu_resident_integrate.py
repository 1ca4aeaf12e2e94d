"""Weighted column sums of a resident grid (ResidentGrid.integrate / evaluate_integrals, vi_reduce_basis_f64):

  out[t, m] = sum_l w[l] density[t, m, l]   over the points of column m inside the hull

The sum is linear in the coefficients, so the basis is summed along the axis once (k_reduce_basis, csrc/vi_eval_resident.hip:
sequentially in ascending l over the points whose ROW 0 of the basis is not NaN, NaN for a column without one) and every call
is vi_eval_resident_f64 on M = Q / L points.

Part 1: integer inputs and weights through the C-ABI - every sum exact - against the masked NumPy sum, bit for bit, for every
axis of two grids (M below and inside K2r's range), columns all dead, partly dead and all live.  Part 2: a real hull-masked basis
against the exact sum of the downloaded matrix, per sample

  |out - exact| <= gamma_{N+L+2} sum_n sum_l |C_n w_l Y_nl|

(one rounding for w Y, L - 1 additions along the column, one multiplication by C and N - 1 additions of the product: at most
N + L factors of (1 + delta), and two to spare; derived, not measured), and the NaN pattern against the density's.  Part 3: the
cache of reduced bases and the arguments."""
import math

import numpy as np
import pytest

from conftest import load_golden                                            # noqa: F401
import test_gpu_resident_geometry as geo

gpu = pytest.mark.gpu


def test_bindings():
    from volumetricinterp_amd import _lib
    from volumetricinterp_amd.estimate import ResidentGrid
    assert 'vi_reduce_basis_f64' in _lib.EXPORTS and hasattr(_lib.lib, 'vi_reduce_basis_f64')
    assert hasattr(ResidentGrid, 'integrate') and hasattr(ResidentGrid, 'evaluate_integrals')


# ==== 1. exact by construction ===============================================================================================
def run_reduce(N, outer, L, inner, Y, w):
    """vi_reduce_basis_f64 on device copies, the output between sentinels.  Returns (Yr (N, M), sentinels intact)."""
    from volumetricinterp_amd import _lib
    ctx = _lib.get_context()
    M = outer * inner
    G = geo.GUARD
    bufs = []
    try:
        dY = ctx.to_device(np.ascontiguousarray(Y, dtype=np.float64))
        bufs.append(dY)
        dw = ctx.to_device(np.ascontiguousarray(w, dtype=np.float64))
        bufs.append(dw)
        dR = ctx.to_device(np.full(2 * G + N * M, geo.SENTINEL))
        bufs.append(dR)
        _lib.check(_lib.lib.vi_reduce_basis_f64(geo._handle(N), outer, L, inner, dY.ptr, dw.ptr, dR.offset_ptr(G)), 'reduce')
        r = dR.download()
    finally:
        for b in bufs:
            b.free()
    sb = np.array([geo.SENTINEL]).view(np.uint64)[0]
    rb = r.view(np.uint64)
    return r[G:G + N * M].reshape(N, M), bool(np.all(rb[:G] == sb) and np.all(rb[G + N * M:] == sb))


def integer_inputs(rng, N, shape, axis, T):
    """Integer C, Y and weights with N L 7 2^(2b) <= 2^50: every sum exact in any order.  Row 0 of Y: NaN at 30 % of the points,
    along whole columns (every fifth) and nowhere in others (every fifth + 1); the other rows stay finite there - only row 0
    decides.  One coefficient row of NaN.  Returns C, Y, w and the masked sums (T, M)."""
    L = shape[axis]
    outer, inner = int(np.prod(shape[:axis])), int(np.prod(shape[axis + 1:]))
    Q = outer * L * inner
    b = int((50 - math.log2(N * L * 7)) // 2)
    C = rng.integers(-2 ** b, 2 ** b + 1, (T, N)).astype(np.float64)
    Y = rng.integers(-2 ** b, 2 ** b + 1, (N, Q)).astype(np.float64)
    w = rng.integers(1, 8, L).astype(np.float64)
    dead = (rng.random(Q) < 0.3).reshape(outer, L, inner)
    cols = np.arange(outer * inner).reshape(outer, 1, inner)
    dead = np.where(cols % 5 == 0, True, np.where(cols % 5 == 1, False, dead)).reshape(Q)
    Yr = (np.where(dead, 0.0, Y).reshape(N, outer, L, inner) * w[None, None, :, None]).sum(axis=2).reshape(N, outer * inner)
    none = dead.reshape(outer, L, inner).all(axis=1).reshape(-1)
    Yr[:, none] = np.nan
    ref = C @ np.where(np.isnan(Yr), 0.0, Yr)
    ref[:, none] = np.nan
    if T >= 2:
        C[1, N // 2] = np.nan
        ref[1] = np.nan
    Y[0, dead] = np.nan
    return C, Y, w, Yr, ref, (outer, L, inner)


@gpu
@pytest.mark.parametrize('N', [16, 50])
@pytest.mark.parametrize('shape', [(5, 6, 12), (8, 9, 40)])
def test_integer_integrals_exact(N, shape):
    """Every axis of a (5, 6, 12) grid (M = 72, 60, 30: the library's product) and of a (8, 9, 40) grid (M = 360, 320: K2r; 72):
    the reduced basis and the integrals have the bits of the masked NumPy sums, NaN where the column has no live point."""
    rng = np.random.default_rng(100 * N + shape[0])
    paths = set()
    for axis in range(3):
        C, Y, w, Yr_ref, ref, (outer, L, inner) = integer_inputs(rng, N, shape, axis, 5)
        M = outer * inner
        paths.add(geo.k2r_geometry(N, M, 5)['path'])
        Yr, ok = run_reduce(N, outer, L, inner, Y, w)
        assert ok, 'a store outside the reduced basis'
        assert not geo.mismatch(Yr, Yr_ref, 'reduced basis N %d shape %s axis %d' % (N, shape, axis))
        none = np.isnan(Yr_ref[0])
        assert none.any() and (~none).any() and np.array_equal(np.isnan(Yr), np.broadcast_to(none, Yr.shape))
        out, ok = geo.run('r', N, M, 5, Yr, C)
        assert ok
        assert not geo.mismatch(out, ref, 'integrals N %d shape %s axis %d' % (N, shape, axis))
    assert paths == ({'library'} if shape[0] == 5 else {'kernel', 'library'})


# ==== 2. a real basis against the exact sum ==================================================================================
def exact_integrals(C, w, Ycols):
    """sum_n sum_l C[n] w[l] Ycols[n, l] exactly (two_prod twice: every term a sum of four doubles; math.fsum) as hi + lo, and
    the sum of the magnitudes."""
    p, e = geo.two_prod(w[None, :], Ycols)
    a, b = geo.two_prod(C[:, None], p)
    c, d = geo.two_prod(C[:, None], e)
    hi, lo = geo.fsum2([np.concatenate([a.ravel(), b.ravel(), c.ravel(), d.ravel()]).tolist()])
    return hi[0], lo[0], float(np.abs(C[:, None] * w[None, :] * Ycols).sum())


@gpu
@pytest.mark.parametrize('N', [144, 180])
def test_real_basis_integrals_within_the_derived_bound(N):
    """synth.query_grid(8) with the hull, trapezoid weights in metres (axis 2) and unit weights (the others): every finite
    sample within gamma_{N+L+2} of the exact sum of the downloaded basis, NaN exactly where the density column is all NaN."""
    from volumetricinterp_amd import synth
    es, fx = geo.real_estimate(N)
    grid = synth.query_grid(8)
    alt = grid[2][0, 0]
    trap = np.empty(8)
    trap[1:-1] = 0.5 * (alt[2:] - alt[:-2])
    trap[0], trap[-1] = 0.5 * (alt[1] - alt[0]), 0.5 * (alt[-1] - alt[-2])
    rng = np.random.default_rng(N)
    with es.resident_grid(*grid) as g:
        Y = g.dY.download()
        C = geo.real_coeffs(rng, N, Y, fx, T=6)
        C[4] = np.nan
        dens = g.evaluate_coeffs(C).reshape(6, 8, 8, 8)
        worst = 0.
        for axis, w in ((2, trap), (-1, None), (0, None), (1, trap)):
            out = g.evaluate_integrals(C, weights=w, axis=axis)
            ax = axis % 3
            assert out.shape == (6, 64)
            nanref = np.all(np.isnan(dens), axis=ax + 1).reshape(6, 64)
            assert np.array_equal(np.isnan(out), nanref) and nanref[4].all() and not nanref[0].all() and nanref[0].any()
            wv = np.ones(8) if w is None else w
            Yc = np.moveaxis(Y.reshape(N, 8, 8, 8), ax + 1, -1).reshape(N, 64, 8)            # (n, column, l)
            for t in (0, 3, 5):
                for m in np.nonzero(~nanref[t])[0]:
                    livel = ~np.isnan(Yc[0, m])
                    hi, lo, mag = exact_integrals(C[t], wv[livel], Yc[:, m, livel])
                    err = abs((out[t, m] - hi) - lo)
                    worst = max(worst, err / (geo.gamma(N + 8 + 2) * mag))
                    assert err <= geo.gamma(N + 8 + 2) * mag, (axis, t, m, out[t, m], hi, err, mag)
        print('N %d: worst error %.3f of the bound' % (N, worst))
        # the same through the datetime interface
        import datetime as dt
        es.Coeffs, es.Covariance = C, np.zeros((6, N, N))
        es.time = np.stack([60. * np.arange(6), 60. * np.arange(6) + 60.], axis=1)
        times = [dt.datetime(1970, 1, 1) + dt.timedelta(seconds=60. * k + 30.) for k in (0, 3)]
        r = g.integrate(times, weights=trap)
        assert r.shape == (2, 8, 8)
        assert not geo.mismatch(r.reshape(2, 64), g.evaluate_integrals(C[[0, 3]], weights=trap), 'integrate')


# ==== 3. cache and arguments =================================================================================================
@gpu
def test_reduced_basis_cache_and_arguments():
    from volumetricinterp_amd import synth
    es, fx = geo.real_estimate(16)
    grid = synth.query_grid(4)
    C = np.ones((2, 16))
    g = es.resident_grid(*grid, check_hull=False)
    a = g.evaluate_integrals(C)
    assert a.shape == (2, 16) and np.isfinite(a).all() and len(g._reduced) == 1
    first = next(iter(g._reduced.values()))
    ptr = first.ptr.value
    b = g.evaluate_integrals(C, weights=np.ones(4))                          # the default weights by value: the same entry
    assert len(g._reduced) == 1 and next(iter(g._reduced.values())) is first and first.ptr.value == ptr
    assert np.array_equal(a, b)
    c = g.evaluate_integrals(C, weights=[1., 2., 3., 4.])
    assert len(g._reduced) == 2 and not np.array_equal(a, c)
    g.evaluate_integrals(C, axis=0)
    assert len(g._reduced) == 3
    # against the host sum of the density
    dens = g.evaluate_coeffs(C).reshape(2, 4, 4, 4)
    assert geo.rel(c, (dens * np.array([1., 2., 3., 4.])).sum(axis=3).reshape(2, 16)) <= 1e-13
    out = np.empty((2, 16))
    assert g.evaluate_integrals(C, out=out) is out and np.array_equal(out, a)
    assert g.evaluate_integrals(np.ones((0, 16))).shape == (0, 16)
    for bad in (np.ones(3), np.ones((4, 1)), [1., np.nan, 1., 1.], [1., np.inf, 1., 1.]):
        with pytest.raises(ValueError, match='weights'):
            g.evaluate_integrals(C, weights=bad)
    with pytest.raises(ValueError, match='axis'):
        g.evaluate_integrals(C, axis=3)
    with pytest.raises(ValueError, match='out'):
        g.evaluate_integrals(C, out=np.empty((2, 15)))
    with pytest.raises(ValueError, match='coefficients'):
        g.evaluate_integrals(np.ones((2, 15)))
    # weights that change with every call: the grid keeps the last REDUCED_BASES matrices and frees the others
    from volumetricinterp_amd.estimate import REDUCED_BASES
    for k in range(REDUCED_BASES + 2):
        g.evaluate_integrals(C, weights=[1., 2., 3., 5. + k])
    assert len(g._reduced) == REDUCED_BASES and first.ptr is None
    assert np.array_equal(g.evaluate_integrals(C), a)                         # rebuilt after it was dropped
    entries = list(g._reduced.values())
    g.close()
    assert not g._reduced and all(e.ptr is None for e in entries)
    with pytest.raises(ValueError, match='closed'):
        g.evaluate_integrals(C)
    g.close()                                                                 # idempotent
