"""GPU tests of the second derivatives: Model.hess_basis, Estimate.hessian / laplacian (vi_eval_hess_f64: kernel k_hess_sph
contracting against one coefficient vector) and the Hessian maps of a resident grid (vi_eval_hess_basis_f64, then the density's
product on 6Q columns).

The reference project has no Hessian.  The yardstick is tests/hessian_ref.py, a float64 restatement of the closed forms on the
oracle's pieces, which tests/test_hessian_host.py holds against 50-digit arithmetic (its rounding error there: E_REF) and
against second differences of the oracle's basis.  Gates: max(1e-11, 8 E_REF) per column for the basis - 1e-11 is the gate of
test_grad_basis_vs_reference, 8 E_REF covers the device's different chain (seeds and recurrence instead of SciPy's series) -,
1e-12 between two device summation orders of one quantity, 1e-10 against the restatement contracted with fitted coefficients,
as for the gradient."""
import datetime as dt
import functools
import io

import numpy as np
import pytest

import hessian_ref as hr
from conftest import load_golden, rel
from test_hessian_host import E_REF

pytestmark = pytest.mark.gpu

SPH_CFG = ('[DEFAULT]\n[MODEL]\nNAME = sphharmlag\nMAXK = %d\nMAXL = %d\nCAP_LIM = %r\nMAX_Z_INT = INF\nLATCP = 78\n'
           'LONCP = 262\n')
# (MAXK, MAXL, CAP_LIM): the three configurations of tests/golden/grad_sph.npz - all within the (6, 4) kernel order - then
# MAXL 2 with MAXK 8 and MAXL 8 with MAXK 5, both compiled at (12, 8), and MAXL 2 with MAXK 12, the (2, 12) order
BASIS_CASES = {'default': (4, 6, 10.), 'k3l4cap15': (3, 4, 15.), 'k2l5cap12p7': (2, 5, 12.7), 'k8l2': (8, 2, 10.),
               'k5l8cap15': (5, 8, 15.), 'k12l2': (12, 2, 10.)}
BASIS_TOL = max(1e-11, 8. * E_REF)
T_MID = dt.datetime(1970, 1, 1) + dt.timedelta(seconds=30)          # the one record of _bare's estimates


def _bare(case, C=None):
    """An Estimate of the order of `case` with one record of coefficients C (zeros), a zero covariance (get_C reads it) and
    no hull."""
    from volumetricinterp_amd.estimate import Estimate
    maxk, maxl, cap = BASIS_CASES[case]
    N = maxk * maxl**2
    return Estimate.from_arrays(np.zeros((1, N)) if C is None else np.asarray(C).reshape(1, N), np.zeros((1, N, N)),
                                [[0., 60.]], np.zeros((4, 3)), SPH_CFG % (maxk, maxl, cap))


def _oracle(case):
    import oracle
    maxk, maxl, cap = BASIS_CASES[case]
    return oracle.SphHarmLagOracle(maxk=maxk, maxl=maxl, cap_lim_deg=cap)


def _estimate(tag):
    """The fixture's fit with its NaN coefficients (failed records) zeroed, and the oracle of its configuration."""
    import oracle
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_' + tag)
    es = Estimate.from_arrays(np.nan_to_num(f['Coeffs']), f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))
    return f, es, oracle.SphHarmLagOracle.from_config(io.StringIO(str(f['cfg'])))


def _t_rec(f, i=0):
    return dt.datetime(1970, 1, 1) + dt.timedelta(seconds=float(np.mean(f['utime'][i])))


@functools.lru_cache(maxsize=None)
def _basis_points(case):
    """The 45 points of the golden file (the default configuration's for the cases it does not hold) at least 0.5 degrees of
    rotated colatitude from the pole of the cap."""
    g = load_golden('grad_sph')
    tag = case if case + '_lat' in g.files else 'default'
    lat, lon, alt = g[tag + '_lat'], g[tag + '_lon'], g[tag + '_alt']
    _, th, _ = _oracle(case).transform_coord(lat, lon, alt)
    ok = th >= np.radians(0.5)
    assert ok.sum() >= 30
    return lat[ok], lon[ok], alt[ok]


@functools.lru_cache(maxsize=None)
def _basis_ref(case, frame):
    H = hr.hess_basis(_oracle(case), *_basis_points(case), frame)
    H.setflags(write=False)
    return H


# ==== 1. the basis ===========================================================================================================
@pytest.mark.parametrize('frame', ['model', 'enu'])
@pytest.mark.parametrize('case', sorted(BASIS_CASES))
def test_hess_basis_vs_restatement(case, frame):
    """Model.hess_basis (P, 6, N) against tests/hessian_ref.py per basis function: the largest error over points and entries
    relative to the function's largest entry is within BASIS_TOL = max(1e-11, 8 E_REF) = 1e-11 (E_REF = 3e-13, the
    restatement's own error against 50-digit arithmetic), both frames, every kernel order: (6, 4) for the three golden
    configurations, (12, 8) for MAXL 2 x MAXK 8 and MAXL 8 x MAXK 5, (2, 12) for MAXL 2 x MAXK 12.  Points at least 0.5
    degrees from the pole.  Measured on the MI355X (model / enu frame): default 8.62e-14 / 8.62e-14, k3l4cap15 5.93e-14 /
    5.95e-14, k2l5cap12p7 2.95e-14 / 3.01e-14, k8l2 4.78e-14 / 4.78e-14, k5l8cap15 7.99e-14 / 7.96e-14, k12l2 4.78e-14 /
    4.80e-14 - below the restatement's own distance from exact arithmetic."""
    es = _bare(case)
    lat, lon, alt = _basis_points(case)
    H = es.model.hess_basis(lat, lon, alt, frame=frame)
    ref = _basis_ref(case, frame)
    assert H.shape == ref.shape and np.isfinite(H).all()
    err = hr.colnorm_err6(H, ref)
    print('%s %s: largest column error %.2e (function %d), bound %.1e' % (case, frame, float(err.max()), int(err.argmax()),
                                                                            BASIS_TOL))
    assert err.max() <= BASIS_TOL, (case, frame, float(err.max()), int(err.argmax()))
    assert es.model.hess_basis(lat[:0], lon[:0], alt[:0], frame=frame).shape == (0, 6, es.model.nbasis)


# ==== 2. the contraction =====================================================================================================
@pytest.mark.parametrize('frame', ['model', 'enu'])
@pytest.mark.parametrize('case', ['default', 'k5l8cap15', 'k12l2'])
def test_hessian_is_the_basis_times_the_coefficients(case, frame):
    """Estimate.hessian (six sums per lane in the kernel) against Model.hess_basis @ C on the host: two summation orders of
    one quantity, 1e-12 as the gradient's consistency check (test_estimate_gradient_vs_oracle)."""
    from volumetricinterp_amd.estimate import gradcov_matrix
    lat, lon, alt = _basis_points(case)
    rng = np.random.default_rng(7)
    B = _bare(case).model.hess_basis(lat, lon, alt, frame=frame)
    C = rng.standard_normal(B.shape[2]) / np.max(np.abs(B), axis=(0, 1))
    H = _bare(case, C).hessian(T_MID, lat, lon, alt, check_hull=False, frame=frame)
    assert H.shape == (lat.size, 3, 3)
    assert rel(H, gradcov_matrix((B @ C).T)) <= 1e-12


@pytest.mark.parametrize('frame', ['model', 'enu'])
@pytest.mark.parametrize('tag', ['default', 'k8l2'])
def test_hessian_vs_restatement_with_fitted_coefficients(tag, frame):
    """Estimate.hessian of the fixtures' fits on a 5^3 grid against the restatement contracted with the same coefficients,
    scaled by the size of the terms, |H| @ |C| (a fit's coefficients cancel heavily, as in test_rbf_estimate_vs_oracle): 1e-10,
    the gate of Estimate.gradient against the oracle."""
    from volumetricinterp_amd import synth
    from volumetricinterp_amd.estimate import gradcov_matrix
    f, es, o = _estimate(tag)
    grid = synth.query_grid(5)
    C = np.nan_to_num(f['Coeffs'])[0]
    H = es.hessian(_t_rec(f), *grid, check_hull=False, frame=frame)
    assert H.shape == (5, 5, 5, 3, 3)
    B = hr.hess_basis(o, *(a.ravel() for a in grid), frame)                      # (P, 6, N)
    ref = gradcov_matrix((B @ C).T)
    scale = np.linalg.norm(gradcov_matrix((np.abs(B) @ np.abs(C)).T))
    err = np.linalg.norm(H.reshape(-1, 3, 3) - ref) / scale
    print('%s %s: %.2e of the terms' % (tag, frame, err))
    assert err <= 1e-10


# ==== 3. launch geometry =====================================================================================================
@functools.lru_cache(maxsize=None)
def _geometry(which):
    """(estimate, time, 1000 points, their packed-as-(Q, 3, 3) Hessians): the default fit with its hull (integer degrees: the
    closed-form seeds) or the fractional degrees of k3l4cap15 (the seed series, whose exit test is wave-uniform), frame enu."""
    rng = np.random.default_rng(1000)
    pts = rng.uniform(75, 81, 1000), rng.uniform(250, 274, 1000), rng.uniform(100e3, 700e3, 1000)
    if which == 'fit':
        f, es, _ = _estimate('default')
        t, hull = _t_rec(f), True
    else:
        es, t, hull = _bare('k3l4cap15', rng.standard_normal(48)), T_MID, False
    return es, t, hull, pts, es.hessian(t, *pts, check_hull=hull, frame='enu')


@pytest.mark.parametrize('Q', [0, 1, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize('which', ['fit', 'series'])
def test_launch_geometry(which, Q):
    """A block is 256 lanes, a wave 64: the six values of a point are the same bits whatever Q is and wherever the point sits
    in the array - the first Q and the last Q of the 1000 points against the call with all of them."""
    es, t, hull, pts, full = _geometry(which)
    if which == 'fit':
        nan = np.isnan(full[:, 0, 0])
        assert 0 < nan.sum() < 1000
    for sl in (slice(0, Q), slice(1000 - Q, 1000)):
        H = es.hessian(t, *(a[sl] for a in pts), check_hull=hull, frame='enu')
        assert H.shape == (Q, 3, 3)
        assert np.array_equal(H.view(np.uint64), full[sl].view(np.uint64))


# ==== 4. hull ================================================================================================================
def test_hull_mask():
    """192 points: a wave wholly outside the hull (it leaves before the chains), a wave with lanes on both sides, a wave as
    drawn.  All six entries of a point are NaN or none is; the pattern is Estimate.gradient's on the same points; without the
    hull test nothing is NaN and the points inside keep their bits."""
    f, es, _ = _estimate('default')
    rng = np.random.default_rng(64)
    lat, lon, alt = rng.uniform(76.5, 79.5, 192), rng.uniform(255, 269, 192), rng.uniform(150e3, 500e3, 192)
    alt[:64] = rng.uniform(2000e3, 3000e3, 64)                                   # far above every beam
    alt[64:128:2] = rng.uniform(2000e3, 3000e3, 32)
    t = _t_rec(f)
    for frame in ('model', 'enu'):
        H = es.hessian(t, lat, lon, alt, frame=frame)
        nan = np.isnan(H)
        pt = nan[:, 0, 0]
        assert np.array_equal(nan, np.broadcast_to(pt[:, None, None], nan.shape))
        assert pt[:64].all() and pt[64:128:2].all() and not pt[64:128].all() and not pt.all()
        assert np.array_equal(pt, np.isnan(es.gradient(t, lat, lon, alt, frame=frame)).all(axis=-1))
        assert np.array_equal(pt, np.isnan(es.laplacian(t, lat, lon, alt)))
        free = es.hessian(t, lat, lon, alt, check_hull=False, frame=frame)
        assert np.isfinite(free).all()
        assert np.array_equal(free[~pt].view(np.uint64), H[~pt].view(np.uint64))


# ==== 5. symmetry and trace ==================================================================================================
@pytest.mark.parametrize('tag', ['default', 'k8l2'])
def test_symmetry_and_trace(tag):
    """hessian is symmetric, laplacian is its trace bit for bit, and the traces of the two frames - one tensor in two
    orthonormal frames - agree to 1e-12 of the diagonal's size."""
    from volumetricinterp_amd import synth
    f, es, _ = _estimate(tag)
    grid = synth.query_grid(6)
    t = _t_rec(f)
    Hm, He = es.hessian(t, *grid), es.hessian(t, *grid, frame='enu')
    lap = es.laplacian(t, *grid)
    assert Hm.shape == (6, 6, 6, 3, 3) and lap.shape == (6, 6, 6)
    ok = np.isfinite(lap)
    assert 20 < ok.sum() < ok.size
    for H in (Hm, He):
        assert np.array_equal(H, np.swapaxes(H, -1, -2), equal_nan=True)
    tr = (Hm[..., 0, 0] + Hm[..., 1, 1]) + Hm[..., 2, 2]
    assert np.array_equal(tr.view(np.uint64)[ok], lap.view(np.uint64)[ok]) and np.isnan(tr[~ok]).all()
    size = np.abs(Hm[..., 0, 0]) + np.abs(Hm[..., 1, 1]) + np.abs(Hm[..., 2, 2])
    tre = (He[..., 0, 0] + He[..., 1, 1]) + He[..., 2, 2]
    assert np.linalg.norm((tre - tr)[ok]) <= 1e-12 * np.linalg.norm(size[ok])


# ==== 6. resident grid =======================================================================================================
def _resident_grid_points():
    return np.meshgrid(np.linspace(75., 81., 6), np.linspace(250., 274., 5), np.linspace(100e3, 700e3, 8), indexing='ij')


@pytest.mark.parametrize('frame', ['model', 'enu'])
def test_resident_grid_hessians(frame):
    """A 6 x 5 x 8 grid with the hull: the Hessian maps of every record of the k8l2 fit (one product on 6Q columns) against
    Estimate.hessian record by record, 1e-12 (two summation orders); a NaN coefficient row gives a NaN map, columns outside the
    hull are NaN, laplacian is the sum of the first three planes."""
    f, es, _ = _estimate('k8l2')
    grid = _resident_grid_points()
    C = np.nan_to_num(f['Coeffs'])
    R, Q = C.shape[0], 240
    with es.resident_grid(*grid, hessian=frame) as g:
        assert g.dH.shape == (32, 6, Q) and g.dG is None
        maps = g.evaluate_hessians(np.concatenate([C, np.full((1, 32), np.nan)]))
        assert maps.shape == (R + 1, 6, Q)
        assert np.isnan(maps[R]).all()
        dens = g.evaluate_coeffs(C)
        outside = np.isnan(dens[0])
        assert 0 < outside.sum() < Q
        times = [_t_rec(f, i) for i in range(R)]
        Hm, lap = g.hessian(times), g.laplacian(times)
        assert Hm.shape == (R, 6, 6, 5, 8) and lap.shape == (R, 6, 5, 8)
        assert np.array_equal(Hm.reshape(R, 6, Q), maps[:R], equal_nan=True)
        assert np.array_equal(lap, (Hm[:, 0] + Hm[:, 1]) + Hm[:, 2], equal_nan=True)
    from volumetricinterp_amd.estimate import GRADCOV_PAIRS
    for i in range(R):
        assert np.array_equal(np.isnan(maps[i]), np.broadcast_to(outside, (6, Q))), i
        H = es.hessian(times[i], *grid, frame=frame).reshape(Q, 3, 3)
        assert np.array_equal(np.isnan(H[:, 0, 0]), outside)
        one = np.stack([H[:, c, d] for c, d in GRADCOV_PAIRS])
        assert rel(maps[i][:, ~outside], one[:, ~outside]) <= 1e-12, i


def test_resident_grid_api():
    """Gradient and Hessian basis together; a grid without hessian= refuses the three methods by name; after close() they say
    so; a bad frame is refused before anything is allocated."""
    f, es, _ = _estimate('k8l2')
    grid = _resident_grid_points()
    C = np.nan_to_num(f['Coeffs'])[:2]
    t = _t_rec(f)
    with es.resident_grid(*grid, gradient='enu', hessian='enu') as g:
        assert g.dG.shape == (32, 3, 240) and g.dH.shape == (32, 6, 240)
        assert g.evaluate_gradients(C).shape == (2, 3, 240) and g.evaluate_hessians(C).shape == (2, 6, 240)
        both = g.hessian([t])
    with es.resident_grid(*grid, hessian='enu') as g:
        assert np.array_equal(g.hessian([t]), both, equal_nan=True)
        assert g.evaluate_hessians(C[:0]).shape == (0, 6, 240) and g.hessian([]).shape == (0, 6, 6, 5, 8)
    with es.resident_grid(*grid, gradient='model') as g0:
        assert g0.dH is None
        for call in (lambda: g0.evaluate_hessians(C), lambda: g0.hessian([t]), lambda: g0.laplacian([t])):
            with pytest.raises(ValueError, match='hessian='):
                call()
    g = es.resident_grid(*grid, hessian='model')
    g.close()
    assert g.dY is None and g.dH is None
    for call in (lambda: g.evaluate_hessians(C), lambda: g.hessian([t]), lambda: g.laplacian([t])):
        with pytest.raises(ValueError, match='closed'):
            call()
    g.close()
    for bad in ('xyz', 'ENU', 0, True):
        with pytest.raises(ValueError, match='hessian must be'):
            es.resident_grid(*grid, hessian=bad)


# ==== 7. refusals ============================================================================================================
def test_refusals():
    """An order beyond the compiled ones (MAXL 13), the radial-basis model and a bad frame: VI_ERR_UNSUPPORTED (-6) or
    VI_ERR_INVALID (-1) from the library with the output buffer untouched - nothing was launched -, ValueError from Python."""
    from volumetricinterp_amd import _lib
    from volumetricinterp_amd.estimate import Estimate
    lat, lon, alt = _basis_points('default')
    Q = lat.size
    BASIS_CASES['k2l13'] = (2, 13, 10.)
    try:
        big = _bare('k2l13')
    finally:
        del BASIS_CASES['k2l13']
    fr = load_golden('fit_rbf')
    rbf = Estimate.from_arrays(fr['Coeffs'], fr['Covariance'], fr['utime'], fr['hull_vert'], str(fr['cfg']))
    for es, what in ((big, 'beyond the compiled limits'), (rbf, 'only the sphharmlag model')):
        ctx, N = es.model.ctx, es.model.nbasis
        with ctx.scope() as dev:
            dlat, dlon, dalt, dC = dev.up(lat), dev.up(lon), dev.up(alt), dev.up(np.ones(N))
            for entry, size in (('vi_eval_hess_f64', 6 * Q), ('vi_eval_hess_basis_f64', 6 * Q * N)):
                dO = dev.up(np.full(size, 7.))
                args = (es.model.handle(), Q, dlat.ptr, dlon.ptr, dalt.ptr) + ((dC.ptr,) if entry == 'vi_eval_hess_f64' else ())
                rc = getattr(_lib.lib, entry)(*args, None, 0, 0., _lib.VI_FRAME_MODEL, dO.ptr)
                assert rc == -6 and what in _lib.lib.vi_last_error().decode(), (entry, rc)
                ctx.sync()
                assert np.array_equal(dO.download(), np.full(size, 7.))
        with pytest.raises(_lib.VinterpError, match=what):
            es.hessian(_t_rec(fr) if es is rbf else T_MID, lat, lon, alt, check_hull=False)
        with pytest.raises(_lib.VinterpError, match=what):
            es.resident_grid(lat, lon, alt, check_hull=False, hessian='model')
    with pytest.raises(_lib.VinterpError, match='beyond the compiled limits'):
        big.model.hess_basis(lat, lon, alt)
    ok = _bare('default')
    for call in (lambda: ok.hessian(T_MID, lat, lon, alt, check_hull=False, frame='xyz'),
                 lambda: ok.model.hess_basis(lat, lon, alt, frame='ENU')):
        with pytest.raises(ValueError, match='frame must be'):
            call()
    ctx = ok.model.ctx
    with ctx.scope() as dev:
        dlat, dlon, dalt, dC, dO = dev.up(lat), dev.up(lon), dev.up(alt), dev.up(np.ones(144)), dev.up(np.full(6 * Q, 7.))
        h = ok.model.handle()
        assert _lib.lib.vi_eval_hess_f64(h, Q, dlat.ptr, dlon.ptr, dalt.ptr, dC.ptr, None, 0, 0., 7, dO.ptr) == -1
        assert _lib.lib.vi_eval_hess_f64(h, Q, dlat.ptr, dlon.ptr, dalt.ptr, dC.ptr, None, 3, 0., 0, dO.ptr) == -1   # F without facets
        assert _lib.lib.vi_eval_hess_basis_f64(h, Q, dlat.ptr, dlon.ptr, dalt.ptr, None, 0, 0., -1, dO.ptr) == -1
        assert _lib.lib.vi_eval_hess_f64(h, 0, dlat.ptr, dlon.ptr, dalt.ptr, dC.ptr, None, 0, 0., 0, dO.ptr) == 0      # Q = 0
        ctx.sync()
        assert np.array_equal(dO.download(), np.full(6 * Q, 7.))


# ==== 8. timing ==============================================================================================================
def test_calls_are_timed():
    """Both entries record their kernel for vi_eval_kernel_ms, as their siblings do."""
    es = _bare('default', np.ones(144))
    lat, lon, alt = _basis_points('default')
    ctx = es.model.ctx
    ctx.eval_timing(True)
    try:
        es.hessian(T_MID, lat, lon, alt, check_hull=False)
        assert 0. < ctx.eval_kernel_ms() < 1000.
        es.model.hess_basis(lat, lon, alt)
        assert 0. < ctx.eval_kernel_ms() < 1000.
    finally:
        ctx.eval_timing(False)


# ==== 9. a layer =============================================================================================================
@functools.lru_cache(maxsize=None)
def _layer():
    """synth's Chapman-like record on an 11 x 50 beam geometry, fitted once at MAXK 8 x MAXL 2: weighted least squares on the
    device's own basis (minimum norm below 1e-10 of the largest singular value)."""
    from volumetricinterp_amd import synth
    lat, lon, alt = synth.beams(*synth.GEOM_C1, seed=0)
    value, error = synth.chapman_record(alt)
    es = _bare('k8l2')
    A = es.model.basis(lat, lon, alt)
    C = np.linalg.lstsq(A / error[:, None], value / error, rcond=1e-10)[0]
    return _bare('k8l2', C)


def test_curvature_of_a_layer():
    """One column through the fitted layer, 150 to 450 km above the radar: hessian(frame='enu')[..., 2, 2] is the second
    derivative along the geodetic normal, so it agrees with second central differences of Estimate.__call__ along altitude,
    and the differences' error falls by 4 when the step is halved from 500 m to 250 m (ratio within [3.5, 4.5]; measured
    4.000).  At 250 m the differences are within 1e-4 of the largest curvature: their truncation error is h^2/12 f'''' =
    (250 m / 50 km)^2 / 12 = 2e-6 of f'' times the ratio f'''' H^4 / (f'' H^2), a few units for a Chapman layer of scale
    height H = 50 km - fifty would still pass (measured 4.8e-6)."""
    es = _layer()
    alt = np.linspace(150e3, 450e3, 31)
    lat, lon = np.full(31, 78.), np.full(31, 262.)
    curv = es.hessian(T_MID, lat, lon, alt, check_hull=False, frame='enu')[:, 2, 2]
    dens = es(T_MID, lat, lon, alt, check_hull=False)
    assert dens.max() > 1e11 and curv[np.argmax(dens)] < 0.                       # a layer, concave at its peak
    err = {}
    for h in (500., 250.):
        fd = (es(T_MID, lat, lon, alt - h, check_hull=False) - 2. * dens + es(T_MID, lat, lon, alt + h, check_hull=False)) / (h * h)
        err[h] = float(np.max(np.abs(fd - curv)))
    print('second differences along altitude: error %.3e at 500 m, %.3e at 250 m of a largest curvature %.3e, ratio %.3f'
          % (err[500.], err[250.], float(np.max(np.abs(curv))), err[500.] / err[250.]))
    assert err[250.] <= 1e-4 * np.max(np.abs(curv))
    assert 3.5 <= err[500.] / err[250.] <= 4.5
