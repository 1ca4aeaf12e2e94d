"""GPU parity of the gradient maps on a resident grid (Estimate.resident_grid(..., gradient='model' | 'enu'),
ResidentGrid.gradient / evaluate_gradients): the gradient basis G (N, 3, Q) assembled once by vi_eval_grad_basis_f64 - planar,
hull mask as NaN, the east-north-up rotation folded in - and multiplied with the coefficients of many timesteps by
vi_eval_resident_f64 on 3Q columns (K2r, or the library for the shapes K2r does not take).

Gates, the project's own: 1e-10 against the oracle (test_estimate_gradient_vs_oracle), 1e-11 per column against the reference's
gradient basis (test_grad_basis_vs_reference), 1e-12 between two device summation orders of the same quantity and 1e-13 for K2r
against the library on the same bits (test_gpu_eval_resident.py); 1e-8 for east-north-up against finite differences of the
oracle's density (test_gradient_frame.py, where the figure is derived)."""
import datetime as dt
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden, colnorm_err, rel
import test_gradient_frame as tf

pytestmark = pytest.mark.gpu

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPH_CFG = ('[DEFAULT]\n[MODEL]\nNAME = sphharmlag\nMAXK = %d\nMAXL = %d\nCAP_LIM = %r\nMAX_Z_INT = INF\nLATCP = 78\n'
           'LONCP = 262\n')
ORDERS = {'k8l2': (8, 2), 'scr_k12l2': (12, 2), 'default': (4, 6)}


def _estimate(tag):
    """The fixture's fit with its NaN coefficients (failed records) zeroed, as test_estimate_gradient_vs_oracle does."""
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_' + tag)
    return f, Estimate.from_arrays(np.nan_to_num(f['Coeffs']), f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))


def _t_mid(f):
    return dt.datetime(1970, 1, 1) + dt.timedelta(seconds=float(np.mean(f['utime'][0])))


def _host_product(G, C):
    """(3, Q) = sum_n G[n] C[n] on the host, on the device's own gradient basis G (N, 3, Q)."""
    with np.errstate(invalid='ignore'):
        return np.einsum('ncq,n->cq', G, C)


# ==== 1. the matrix itself ===================================================================================================
@pytest.mark.parametrize('tag', ['default', 'k3l4cap15', 'k2l5cap12p7'])
def test_gradient_basis_vs_reference(tag):
    """The three orders of tests/golden/grad_sph.npz (N = 144, 48, 50) on their 45 points, model frame, no hull: the
    reference's own grad_basis output per component, Model.grad_basis (the same code at other strides) and - 3Q = 135 is odd,
    so the product is the library's - the host product on the downloaded bits."""
    from volumetricinterp_amd.estimate import Estimate
    gs = load_golden('grad_sph')
    maxk, maxl, cap = gs[tag + '_cfg']
    N = int(maxk) * int(maxl)**2
    es = Estimate.from_arrays(np.zeros((1, N)), None, [[0., 60.]], np.zeros((4, 3)), SPH_CFG % (maxk, maxl, float(cap)))
    lat, lon, alt = gs[tag + '_lat'], gs[tag + '_lon'], gs[tag + '_alt']
    Gref = gs[tag + '_G']                                                # (P, 3, N)
    with es.resident_grid(lat, lon, alt, check_hull=False, gradient='model') as g:
        assert g.dG.shape == (N, 3, 45) and g.Q == 45
        G = g.dG.download()
        own = es.model.grad_basis(lat, lon, alt)
        for c in range(3):
            err = colnorm_err(G[:, c, :].T, Gref[:, c, :])
            assert np.max(err) <= 1e-11, (tag, c, float(np.max(err)), int(np.argmax(err)))
            assert rel(G[:, c, :].T, own[:, c, :]) <= 1e-13, (tag, c)
        rng = np.random.default_rng(45)
        C = rng.standard_normal((5, N)) / np.max(np.abs(G), axis=(1, 2))
        out = g.evaluate_gradients(C)
        assert out.shape == (5, 3, 45)
        for t in range(5):
            assert rel(out[t], _host_product(G, C[t])) <= 1e-12, t


# ==== 2. maps ================================================================================================================
@functools.lru_cache(maxsize=None)
def _oracle_map(tag, check_hull):
    """(6, 6, 6, 3) oracle gradient in the model frame on synth.query_grid(6), one Qhull per point with the hull: once per
    (fixture, hull) for both frames."""
    import oracle
    from volumetricinterp_amd import synth
    f = load_golden('fit_' + tag)
    o = oracle.SphHarmLagOracle(maxk=ORDERS[tag][0], maxl=ORDERS[tag][1])
    C, _ = oracle.get_C(_t_mid(f), f['utime'], np.nan_to_num(f['Coeffs']), f['Covariance'])
    ref = oracle.evaluate_gradient(o, C, *synth.query_grid(6), hull_vert=f['hull_vert'] if check_hull else None)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize('frame', ['model', 'enu'])
@pytest.mark.parametrize('check_hull', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'scr_k12l2', 'default'])
def test_gradient_map_vs_oracle_and_estimate_gradient(tag, check_hull, frame):
    """N = 32, 48, 144 on the 6^3 grid: Q = 216, 3Q = 648 - K2r with three ragged groups of columns."""
    from volumetricinterp_amd import synth
    f, es = _estimate(tag)
    grid = synth.query_grid(6)
    t = _t_mid(f)
    ref = _oracle_map(tag, check_hull)
    if frame == 'enu':
        M = es.model.gradient_frame(*grid).reshape(6, 6, 6, 3, 3)
        ref = np.einsum('...ic,...c->...i', M, ref)
    with es.resident_grid(*grid, check_hull=check_hull, gradient=frame) as g:
        out = g.gradient([t])
        assert out.shape == (1, 3, 6, 6, 6)
        dens = g([t])
        for c in range(3):
            assert np.array_equal(np.isnan(out[0, c]), np.isnan(dens[0])), c
        ok = np.isfinite(dens[0])
        assert ok.sum() > 20 and (check_hull or ok.all())
        dev = es.gradient(t, *grid, check_hull=check_hull, frame=frame)
        assert np.array_equal(np.isnan(np.moveaxis(out[0], 0, -1)), np.isnan(dev))
        for c in range(3):
            e_or, e_dev = rel(out[0, c][ok], ref[..., c][ok]), rel(out[0, c][ok], dev[..., c][ok])
            print('%s hull %d %s component %d: oracle %.1e, Estimate.gradient %.1e' % (tag, check_hull, frame, c, e_or, e_dev))
            assert e_or <= 1e-10, c
            assert e_dev <= 1e-12, c


# ==== 3. east-north-up against finite differences of the oracle density ======================================================
def test_enu_gradient_vs_finite_differences():
    """The device's east-north-up gradient (rotation folded into G by the kernel) at the 60 points of test_gradient_frame.py
    against central differences of the oracle's density at a 10 m step: independent of Model.gradient_frame."""
    import oracle
    f, es = _estimate('default')
    lat, lon, alt = tf.frame_points()
    C = np.nan_to_num(f['Coeffs'])[0]
    fd = tf.enu_finite_differences(oracle.SphHarmLagOracle(), C, lat, lon, alt)
    with es.resident_grid(lat, lon, alt, check_hull=False, gradient='enu') as g:
        out = g.evaluate_gradients(C[None, :])[0]                       # (3, 60)
    err = rel(out.T, fd)
    print('device east-north-up gradient against finite differences: %.2e' % err)
    assert err <= tf.FD_TOL


# ==== 4. many timesteps and dispatch =========================================================================================
MANY_T = 130
MANY_FRAME = {84: 'model', 1777: 'enu', 2052: 'enu', 8192 + 256: 'model'}


def many_timesteps(Q):
    """(C (130, 32), G (32, 3, Q), out (130, 3, Q)) of fixture k8l2 on Q random points, some outside the hull: the fixture's
    rows scaled by 4^j, row 77 all NaN; timestep tiles of 64 + 64 + 2."""
    f, es = _estimate('k8l2')
    rng = np.random.default_rng(23)
    lat, lon, alt = rng.uniform(75, 81, Q), rng.uniform(250, 274, Q), rng.uniform(100e3, 700e3, Q)
    base = np.nan_to_num(f['Coeffs'])
    C = base[rng.integers(0, len(base), MANY_T)] * (4.0 ** rng.integers(-4, 5, MANY_T))[:, None]
    C[77] = np.nan
    with es.resident_grid(lat, lon, alt, check_hull=True, gradient=MANY_FRAME[Q]) as g:
        return C, g.dG.download(), g.evaluate_gradients(C)


@pytest.mark.parametrize('Q', sorted(MANY_FRAME))
def test_gradient_maps_many_timesteps(Q):
    """Q = 84 (3Q = 252 < 256) and 1777 (odd) go through the library; 2052 through K2r with 25 groups of 256 columns, the last
    ragged, and the live list; 8448 through K2r with 99."""
    C, G, out = many_timesteps(Q)
    assert out.shape == (MANY_T, 3, Q)
    outside = np.isnan(G[0, 0])
    assert 0 < outside.sum() < Q
    assert np.array_equal(np.isnan(G), np.broadcast_to(outside, G.shape))
    for t in (0, 63, 64, 77, 128, 129):
        ref = _host_product(G, C[t])
        nan = np.isnan(out[t])
        assert np.array_equal(nan, np.isnan(ref)), t
        assert np.array_equal(nan, np.broadcast_to(nan[0], nan.shape)), t          # all three components of a point or none
        assert np.array_equal(nan[0], outside | (t == 77)), t
        if t != 77:
            assert rel(out[t][~nan], ref[~nan]) <= 1e-12, t


# ==== 5. slabs ===============================================================================================================
def test_gradient_maps_slab_loop(monkeypatch):
    """30 timesteps with the free memory reported so that the call runs in slabs of 7 (4 x 7 + 2): the bits of one slab."""
    f, es = _estimate('k8l2')
    rng = np.random.default_rng(3)
    Q, T = 2052, 30
    lat, lon, alt = rng.uniform(75, 81, Q), rng.uniform(250, 274, Q), rng.uniform(100e3, 700e3, Q)
    C = np.nan_to_num(f['Coeffs'])[rng.integers(0, len(f['Coeffs']), T)] * rng.uniform(-2, 2, (T, 1))
    with es.resident_grid(lat, lon, alt, gradient='enu') as g:
        one = g.evaluate_gradients(C)
        ctx = es.model.ctx
        total = ctx.mem_info()[1]
        free = 4 * 7 * 3 * Q * 8 + 100
        assert free // 4 // (3 * Q * 8) == 7
        monkeypatch.setattr(ctx, 'mem_info', lambda: (free, total))
        slabs = g.evaluate_gradients(C)
    assert np.isnan(one).any() and np.isfinite(one).any()
    assert np.array_equal(slabs.view(np.uint64), one.view(np.uint64))


# ==== 6. switches ============================================================================================================
CHILD = '''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import test_gpu_resident_gradient as rg
np.save(sys.argv[1], rg.many_timesteps(2052)[2])
'''


def test_gradient_product_switches_in_child_processes(tmp_path):
    """The switches of the density product apply to the gradient product (both are read once per process: one child each, one
    after the other).  VINTERP_K2R_LIVE=0, the plain loop over every piece: the default's bits, NaN-aware.
    VINTERP_EVAL_RESIDENT=blas, the library: 1e-13 on the same G bits, the same NaN pattern."""
    script = tmp_path / 'child.py'
    script.write_text(CHILD % (REPO_ROOT, os.path.join(REPO_ROOT, 'tests')))
    assert os.environ.get('VINTERP_K2R_LIVE') != '0' and os.environ.get('VINTERP_EVAL_RESIDENT') != 'blas'
    own = many_timesteps(2052)[2]
    res = {}
    for name, var in (('plain', 'VINTERP_K2R_LIVE'), ('blas', 'VINTERP_EVAL_RESIDENT')):
        env = dict(os.environ)
        for k in ('VINTERP_K2R_LIVE', 'VINTERP_EVAL_RESIDENT', 'VINTERP_K2R_GROUPS'):
            env.pop(k, None)
        env[var] = '0' if name == 'plain' else 'blas'
        o = str(tmp_path / (name + '.npy'))
        r = subprocess.run([sys.executable, str(script), o], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, '%s child: exit %d\n%s\n%s' % (name, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
        res[name] = np.load(o)
    assert np.array_equal(res['plain'], own, equal_nan=True)
    assert np.array_equal(np.isnan(res['blas']), np.isnan(own))
    ok = np.isfinite(own)
    assert ok.any() and rel(own[ok], res['blas'][ok]) <= 1e-13


# ==== 7. edges ===============================================================================================================
def test_gradient_maps_api_edges(monkeypatch):
    from volumetricinterp_amd import _lib, synth
    f, es = _estimate('k8l2')
    grid = synth.query_grid(4)
    Q, N = 64, 32
    t = _t_mid(f)
    C = np.nan_to_num(f['Coeffs'])[:3]
    # a grid without the keyword: the gradient is refused by name, density and error as before
    with es.resident_grid(*grid) as g0:
        assert g0.dG is None
        with pytest.raises(ValueError, match='gradient='):
            g0.gradient([t])
        with pytest.raises(ValueError, match='gradient='):
            g0.evaluate_gradients(C)
        assert g0([t]).shape == (1, 4, 4, 4) and g0.error([t]).shape == (1, 4, 4, 4)
        dens = g0([t])
    for bad in ('xyz', 'ENU', 0, True):
        with pytest.raises(ValueError, match='gradient must be'):
            es.resident_grid(*grid, gradient=bad)
    with pytest.raises(ValueError, match='frame must be'):
        es.gradient(t, *grid, frame='xyz')
    g = es.resident_grid(*grid, gradient='model')
    two = g.gradient([t, t])
    assert two.shape == (2, 3, 4, 4, 4)
    assert np.array_equal(two[0], two[1], equal_nan=True)
    assert np.array_equal(g([t]), dens, equal_nan=True)                  # the density of a grid that also keeps G
    out = _lib.pinned_empty((3, 3, Q))
    assert g.evaluate_gradients(C, out=out) is out
    assert np.array_equal(out, g.evaluate_gradients(C), equal_nan=True)
    for bad in (np.empty((3, Q, 3)), np.empty((3, 3, Q), dtype=np.float32), np.empty((3, Q)), np.empty((Q, 3, 3)).T):
        with pytest.raises(ValueError, match='out must be'):
            g.evaluate_gradients(C, out=bad)
    for bad in (np.zeros((3, 31)), np.zeros(32), np.zeros((3, 32, 1))):
        with pytest.raises(ValueError, match='coefficients must have shape'):
            g.evaluate_gradients(bad)
    assert g.evaluate_gradients(C[:0]).shape == (0, 3, Q)
    assert g.gradient([]).shape == (0, 3, 4, 4, 4)
    assert g([]).shape == (0, 4, 4, 4)                  # no times: the empty map, as every other map of the grid gives it
    g.close()
    assert g.dY is None and g.dG is None
    with pytest.raises(ValueError, match='closed'):
        g.evaluate_gradients(C)
    with pytest.raises(ValueError, match='closed'):
        g.gradient([t])
    g.close()                                                            # idempotent
    empty = es.resident_grid(grid[0][:0], grid[1][:0], grid[2][:0], gradient='enu')
    assert empty.evaluate_gradients(C).shape == (3, 3, 0)
    assert empty.gradient([t]).shape == (1, 3, 0, 4, 4)
    empty.close()
    # Estimate.gradient: 'enu' is the model-frame result times gradient_frame; the default is the model frame, unchanged
    gm = es.gradient(t, *grid)
    assert np.array_equal(gm, es.gradient(t, *grid, frame='model'), equal_nan=True)
    M = es.model.gradient_frame(*grid).reshape(4, 4, 4, 3, 3)
    assert np.array_equal(es.gradient(t, *grid, frame='enu'), np.einsum('...ic,...c->...i', M, gm), equal_nan=True)
    assert np.isnan(gm).any() and np.isfinite(gm).any()
    # the memory check counts both matrices: a device that admits Y but not Y + G
    ctx = es.model.ctx
    total = ctx.mem_info()[1]
    monkeypatch.setattr(ctx, 'mem_info', lambda: (int(2 * N * Q * 8 / 0.9), total))
    es.resident_grid(*grid).close()
    with pytest.raises(MemoryError, match='gradient basis'):
        es.resident_grid(*grid, gradient='model')


def test_default_frame_of_estimate_gradient_unchanged():
    """What test_estimate_gradient_vs_oracle pins, with the new keyword left at its default and given as 'model'."""
    import oracle
    from volumetricinterp_amd import synth
    f, es = _estimate('default')
    grid = synth.query_grid(5)
    t = _t_mid(f)
    C, _ = oracle.get_C(t, f['utime'], np.nan_to_num(f['Coeffs']), f['Covariance'])
    ref = oracle.evaluate_gradient(oracle.SphHarmLagOracle(), C, *grid)
    for kw in ({}, {'frame': 'model'}):
        g = es.gradient(t, *grid, check_hull=False, **kw)
        assert g.shape == (5, 5, 5, 3)
        for c in range(3):
            assert rel(g[..., c], ref[..., c]) <= 1e-10, c


def test_unsupported_model_frees_everything():
    """The radial-basis model has no gradient basis: the constructor raises and the device memory is what it was before."""
    from volumetricinterp_amd import _lib, synth
    from volumetricinterp_amd.estimate import Estimate
    f = load_golden('fit_rbf')
    es = Estimate.from_arrays(f['Coeffs'], f['Covariance'], f['utime'], f['hull_vert'], str(f['cfg']))
    grid = synth.query_grid(6)
    es.resident_grid(*grid).close()                                      # context, model tables, hull buffers, code objects
    ctx = es.model.ctx
    before = ctx.mem_info()[0]
    with pytest.raises(_lib.VinterpError, match='only the sphharmlag model'):
        es.resident_grid(*grid, gradient='model')
    assert ctx.mem_info()[0] == before
    es.resident_grid(*grid).close()                                      # and the grid without a gradient still builds
