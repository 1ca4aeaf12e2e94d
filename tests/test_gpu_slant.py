"""GPU parity of the line integrals along straight rays (Estimate.slant, vi_eval_slant_f64 - kernel K2l: a wave per ray, the ray
clipped against the hull's facets in the kernel, a quadrature rule on exactly the part inside, one coefficient row per ray)
against a different device route through code that has its own tests: the chords of estimate.hull_chords on the host, the node
positions in NumPy, geodesy.ecef2geodetic, Estimate.track at the nodes with the ray's time repeated per node and no hull test,
and the weighted sum on the host.

Gate, per ray: the NaN pattern is identical, and |out - ref| <= 1e-10 * sum_i |W_i f_i| for every finite ray - 1e-10 is the
project's gate L6 for one quantity by two routes (the reference's points pass through a geodetic round trip of about 4e-9 m and,
in interpolation mode, a blend of densities instead of coefficients); the scale is the ray's own absolute sum, so that no large
ray hides a small one.  Every parity test asserts that each hit ray's chord is longer than 1 m, which keeps the NaN pattern off
the decision boundary of the clip.

The records are those of tests/test_gpu_track.py: R = 40 rows of the fixtures, mid-times 60 s apart."""
import functools

import numpy as np
import pytest

import test_gpu_track as tt

pytestmark = pytest.mark.gpu

R = tt.R
TOL = 1e-10                 # the gate above (ORACLE_TOL of the track tests: the project's L6)
EPS = np.finfo(np.float64).eps
P = 1000


# ---- rays ------------------------------------------------------------------------------------------------------------------------

def _ecef(lat, lon, alt):
    from volumetricinterp_amd import geodesy
    return np.ascontiguousarray(np.array(geodesy.geodetic2ecef(lat, lon, alt)).T)


@functools.lru_cache(maxsize=None)
def _rays(name, n=P):
    """(start, end, a, b): geodetic triples and the (n, 3) ECEF end points of a ray set; 'inside': ECEF only (start, end None)."""
    rng = np.random.default_rng(5)
    if name == 'inside':
        lat, lon, alt = tt._box(rng, 8 * n)
        ok = tt._estimate('k8l2', False).check_hull(lat, lon, alt)
        assert ok.sum() >= 2 * n
        x = _ecef(lat[ok], lon[ok], alt[ok])
        out = (None, None, np.ascontiguousarray(x[:n]), np.ascontiguousarray(x[n:2 * n]))
    else:
        if name == 'vertical':
            lat, lon = rng.uniform(75, 81, n), rng.uniform(250, 274, n)
            start, end = (lat, lon, np.full(n, 100e3)), (lat, lon, np.full(n, 700e3))
        else:
            start = (rng.uniform(75, 81, n), rng.uniform(250, 274, n), np.zeros(n))
            if name == 'oblique':
                end = (rng.uniform(72, 84, n), rng.uniform(240, 284, n), np.full(n, 1000e3))
            else:
                assert name == 'gnss'
                end = (rng.uniform(40, 89, n), rng.uniform(200, 320, n), np.full(n, 20200e3))
        out = (start, end, _ecef(*start), _ecef(*end))
    for v in out[2:] + (out[0] or ()) + (out[1] or ()):
        v.setflags(write=False)
    return out


def _length(a, b):
    return np.linalg.norm(b - a, axis=1)


def _chords(a, b, check_hull):
    """Host chords (s0, s1) of the rays: hull_chords on the fixtures' hull, or the whole segment."""
    from volumetricinterp_amd.estimate import hull_chords
    if not check_hull:
        return np.zeros(len(a)), np.ones(len(a))
    eq, tol = tt._estimate('k8l2', False)._hull()
    return hull_chords(eq, tol, a, b)


def _nodes(a, b, s0, s1, x):
    """(lat, lon, alt), each (rays, nodes): the nodes of the rule on [s0, s1] of every ray (rays with a chord only)."""
    from volumetricinterp_amd import geodesy
    s = s0[:, None] + (s1 - s0)[:, None] * (1. + x[None, :]) / 2.
    pts = a[:, None, :] + s[:, :, None] * (b - a)[:, None, :]
    return geodesy.ecef2geodetic(pts[..., 0], pts[..., 1], pts[..., 2])


def _reference(es, t0, a, b, x, wq, check_hull):
    """(ref, scale, s0, s1): the integrals by the other route - host chords, Estimate.track at the nodes - and sum |W f|."""
    s0, s1 = _chords(a, b, check_hull)
    hit = ~np.isnan(s0)
    ref, scale = np.full(len(a), np.nan), np.full(len(a), np.nan)
    if hit.any():
        lat, lon, alt = _nodes(a[hit], b[hit], s0[hit], s1[hit], x)
        times = np.repeat(np.broadcast_to(t0, (len(a),))[hit], x.size).reshape(lat.shape)
        f = es.track(times, lat, lon, alt, check_hull=False, outside='nan')
        W = wq[None, :] * ((s1 - s0)[hit] / 2. * _length(a, b)[hit])[:, None]
        ref[hit] = (W * f).sum(axis=1)
        scale[hit] = np.abs(W * f).sum(axis=1)
    return ref, scale, s0, s1


def _gate(out, ref, scale, what=''):
    assert out.shape == ref.shape
    assert np.array_equal(np.isnan(out), np.isnan(ref)), (what, np.flatnonzero(np.isnan(out) != np.isnan(ref))[:10])
    ok = ~np.isnan(ref)
    if ok.any():
        err = np.abs(out[ok] - ref[ok]) / scale[ok]
        print('%s: max |out - ref| / sum |W f| = %.2e on %d finite rays of %d' % (what, err.max(), ok.sum(), ok.size))
        assert np.all(np.abs(out[ok] - ref[ok]) <= TOL * scale[ok]), (what, err.max())
    return ok


def _gauss(n=64):
    return np.polynomial.legendre.leggauss(n)


def _times(es, n, seed=12):
    mt = tt._mid(es.time)
    return np.random.default_rng(seed).uniform(mt[0], mt[-1], n)


def _same_bits(x, y):
    return np.array_equal(x.view(np.uint64), y.view(np.uint64))


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('check_hull', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'default', 'scr_k12l2', 'rbf'])
def test_slant_parity(tag, check_hull, timeinterp):
    """1000 rays at random times over the records' range, unsorted, 64 Gauss-Legendre nodes: k8l2 (2, 8) and default (6, 4) on
    the tiled kernel, scr_k12l2 (2, 12) on the per-lane sphharmlag kernel, rbf on the per-lane RBF kernel.  With the hull: the
    oblique set (a third of the rays miss); without: rays between two points inside the hull, the first 50 of them also against
    the CPU oracle at the nodes with oracle.get_C's row."""
    import oracle
    es = tt._estimate(tag, timeinterp)
    start, end, a, b = _rays('oblique' if check_hull else 'inside')
    t0 = _times(es, P)
    rec, w = es.select_records(t0)
    assert len(np.unique(rec)) >= R - 2 and np.any(np.diff(rec) < 0)            # every record, and unsorted
    x, wq = _gauss()
    if check_hull:
        out, d0, d1 = es.slant(t0, start, end, chord=True)
    else:
        out, d0, d1 = es.slant(t0, a.T, b.T, coords='ecef', check_hull=False, chord=True)
    ref, scale, s0, s1 = _reference(es, t0, a, b, x, wq, check_hull)
    hit = ~np.isnan(s0)
    assert (0 < hit.sum() < P) if check_hull else hit.all()
    assert np.all(((s1 - s0) * _length(a, b))[hit] > 1.)                        # off the decision boundary
    assert np.array_equal(np.isnan(d0), ~hit) and np.array_equal(np.isnan(d1), ~hit)
    ok = _gate(out, ref, scale, '%s hull=%s interp=%s' % (tag, check_hull, timeinterp))
    assert np.array_equal(ok, hit)
    if not check_hull:
        assert np.array_equal(d0, np.zeros(P)) and np.array_equal(d1, _length(a, b))
        o = tt._oracle(tag)
        cov = np.zeros((R, 1, 1))
        # datetimes carry microseconds: the 50 rays are integrated again at times a datetime holds exactly
        t50 = np.array([(tt._datetime(t) - tt.EPOCH).total_seconds() for t in t0[:50]])
        out50 = es.slant(t50, a[:50].T, b[:50].T, coords='ecef', check_hull=False)
        lat, lon, alt = _nodes(a[:50], b[:50], np.zeros(50), np.ones(50), x)
        W = wq[None, :] * (_length(a, b)[:50] / 2.)[:, None]
        f = np.array([oracle.evaluate(o, oracle.get_C(tt._datetime(t50[q]), es.time, es.Coeffs, cov, timeinterp=timeinterp)[0],
                                      lat[q], lon[q], alt[q]) for q in range(50)])
        _gate(out50, (W * f).sum(axis=1), np.abs(W * f).sum(axis=1), '%s interp=%s against the oracle' % (tag, timeinterp))


# ---- 2. midpoint rule ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'scr_k12l2', 'rbf'])
def test_slant_midpoint_rule(tag, timeinterp):
    """rule = ([0], [2]): one node, nothing to sum - the value is the length of the chord times the density Estimate.track gives
    at the chord's midpoint."""
    from volumetricinterp_amd import geodesy
    es = tt._estimate(tag, timeinterp)
    start, end, a, b = _rays('oblique')
    t0 = _times(es, P, seed=13)
    out, d0, d1 = es.slant(t0, start, end, rule=([0.], [2.]), chord=True)
    hit = ~np.isnan(d0)
    assert 0 < hit.sum() < P and np.array_equal(np.isnan(out), ~hit)
    u = (b - a) / _length(a, b)[:, None]
    mid = a[hit] + (0.5 * (d0 + d1)[hit])[:, None] * u[hit]
    f = es.track(t0[hit], *geodesy.ecef2geodetic(mid[:, 0], mid[:, 1], mid[:, 2]), check_hull=False)
    ref = (d1 - d0)[hit] * f
    err = np.abs(out[hit] - ref) / np.abs(ref)
    print('%s interp=%s midpoint: max rel %.2e' % (tag, timeinterp, err.max()))
    assert np.all(np.abs(out[hit] - ref) <= TOL * np.abs(ref)), err.max()


# ---- 3. the chord output ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['oblique', 'gnss'])
def test_slant_chords(name):
    """The chord ends the kernel returns lie ON the hull's surface: with x0, x1 the end points recomputed in NumPy,
    max_f (n_f . x + d_f) is within 64 eps (|a| + |b|) of tol at each clipped end - the round-off of a plane distance at those
    magnitudes (about 4e-7 m for a GNSS ray) times an order of magnitude for the division and this re-evaluation.  An end that is
    not clipped (d0 == 0 or d1 == |b - a|) is inside.  0 <= d0 < d1 <= |b - a|; NaNs exactly for the rays that miss."""
    es = tt._estimate('k8l2', False)
    eq, tol = es._hull()
    start, end, a, b = _rays(name)
    s0, s1 = _chords(a, b, True)
    hit = ~np.isnan(s0)
    assert 0 < hit.sum() < P
    assert np.all(((s1 - s0) * _length(a, b))[hit] > 1.)
    out, d0, d1 = es.slant(_times(es, P), start, end, chord=True)
    assert np.array_equal(np.isnan(d0), ~hit) and np.array_equal(np.isnan(d1), ~hit) and np.array_equal(np.isnan(out), ~hit)
    length = _length(a, b)[hit]
    d0, d1, a, b = d0[hit], d1[hit], a[hit], b[hit]
    assert np.all((0. <= d0) & (d0 < d1) & (d1 <= length))
    u = (b - a) / length[:, None]
    bound = 64. * EPS * (np.linalg.norm(a, axis=1) + np.linalg.norm(b, axis=1))
    clipped = 0
    for d, free in ((d0, d0 == 0.), (d1, d1 == length)):
        x = a + d[:, None] * u
        g = np.max(x @ eq[:, :3].T + eq[:, 3], axis=1) - tol
        print('%s: max |max_f g - tol| / bound at the clipped ends %.3f (%d of %d clipped)'
              % (name, np.max(np.abs(g[~free]) / bound[~free]), (~free).sum(), free.size))
        assert np.all(np.abs(g[~free]) <= bound[~free]), np.max(np.abs(g[~free]) / bound[~free])
        assert np.all(g[free] <= bound[free])
        clipped += (~free).sum()
    assert clipped > 1.5 * hit.sum()                    # these sets start below the hull and end above it
    # the distances are the host's chords (a millimetre: the rounding of a plane distance, 1e-9 m, over the sine of the angle
    # between ray and facet, which no ray of these sets has below 1e-6)
    assert np.allclose(d0, s0[hit] * length, rtol=0., atol=1e-3) and np.allclose(d1, s1[hit] * length, rtol=0., atol=1e-3)


def test_slant_chords_inside_and_vertical():
    """Rays between two points inside the hull: exactly (0, |b - a|).  Vertical rays through the box of the tests: clipped at both
    ends, at one, or missing the hull - the host's pattern."""
    es = tt._estimate('k8l2', False)
    _, _, a, b = _rays('inside')
    t0 = _times(es, P)
    out, d0, d1 = es.slant(t0, a.T, b.T, coords='ecef', chord=True)
    assert np.isfinite(out).all()
    assert np.array_equal(d0, np.zeros(P)) and np.array_equal(d1, _length(a, b))
    start, end, a, b = _rays('vertical')
    s0, s1 = _chords(a, b, True)
    hit = ~np.isnan(s0)
    both = hit & (s0 > 0.) & (s1 < 1.)
    assert 0 < both.sum() < hit.sum() < P
    out, d0, d1 = es.slant(t0, start, end, chord=True)
    assert np.array_equal(np.isnan(d0), ~hit) and np.array_equal(np.isnan(out), ~hit)
    assert np.array_equal(d0[hit] > 0., s0[hit] > 0.) and np.array_equal(d1[hit] < _length(a, b)[hit], s1[hit] < 1.)
    ref, scale, _, _ = _reference(es, t0, a, b, *_gauss(), True)
    _gate(out, ref, scale, 'vertical')


# ---- 4. geometry of the launch (k8l2, N = 32: the logic does not depend on the order) ----------------------------------------

def _geometry_rays(check_hull, n):
    """n rays: of the oblique set with the hull - a ray that hits first, so that one ray is a number -, of the inside set without."""
    if not check_hull:
        return _rays('inside')[2][:n], _rays('inside')[3][:n]
    _, _, a, b = _rays('oblique')
    first = int(np.flatnonzero(~np.isnan(_chords(a, b, True)[0]))[0])
    order = np.r_[first, np.delete(np.arange(P), first)][:n]
    return np.ascontiguousarray(a[order]), np.ascontiguousarray(b[order])


def _geometry_times(es, n):
    """n random times, the last ray on the last row (nearest mode) or on the pair that ends on it."""
    mt = tt._mid(es.time)
    t0 = _times(es, n, seed=n)
    t0[-1] = mt[-1] - 1. if es.timeinterp else mt[-1]
    assert es.select_records(t0)[0][-1] == (R - 2 if es.timeinterp else R - 1)
    return t0


@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('check_hull', [False, True])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 63, 257])
def test_slant_ray_counts(n, check_hull, timeinterp):
    """Ray counts about the boundaries of a wave and of a workgroup of four rays, F = 0 and all facets, both modes."""
    es = tt._estimate('k8l2', timeinterp)
    a, b = _geometry_rays(check_hull, n)
    t0 = _geometry_times(es, n)
    out = es.slant(t0, a.T, b.T, coords='ecef', check_hull=check_hull)
    ref, scale, _, _ = _reference(es, t0, a, b, *_gauss(), check_hull)
    ok = _gate(out, ref, scale, 'P=%d hull=%s interp=%s' % (n, check_hull, timeinterp))
    assert ok[0] and (check_hull or ok.all())


@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('check_hull', [False, True])
@pytest.mark.parametrize('nodes', [1, 2, 63, 64, 65, 128, 200])
def test_slant_node_counts(nodes, check_hull, timeinterp):
    """Node counts about the boundaries of a pass of 64 nodes (idle lanes in the last pass), five rays."""
    es = tt._estimate('k8l2', timeinterp)
    a, b = _geometry_rays(check_hull, 5)
    t0 = _geometry_times(es, 5)
    out = es.slant(t0, a.T, b.T, coords='ecef', nodes=nodes, check_hull=check_hull)
    ref, scale, _, _ = _reference(es, t0, a, b, *_gauss(nodes), check_hull)
    ok = _gate(out, ref, scale, 'nodes=%d hull=%s interp=%s' % (nodes, check_hull, timeinterp))
    assert ok[0]


# ---- 5. independence -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'scr_k12l2', 'rbf'])
def test_slant_rays_are_independent(tag, timeinterp):
    """The same 257 rays shuffled and in order give the same bits per ray, and ray 100 alone the bits it has in the batch."""
    es = tt._estimate(tag, timeinterp)
    _, _, a, b = _rays('oblique')
    a, b = a[:257], b[:257]
    t0 = _times(es, 257, seed=14)
    out, d0, d1 = es.slant(t0, a.T, b.T, coords='ecef', chord=True)
    assert 0 < np.isfinite(out).sum() < 257 and np.isfinite(out[100])
    order = np.random.default_rng(15).permutation(257)
    shuffled = es.slant(t0[order], a[order].T, b[order].T, coords='ecef', chord=True)
    for x, y in zip(shuffled, (out, d0, d1)):
        assert _same_bits(x, y[order])
    alone = es.slant(t0[100:101], a[100:101].T, b[100:101].T, coords='ecef', chord=True)
    for x, y in zip(alone, (out, d0, d1)):
        assert _same_bits(x, y[100:101])


# ---- the C entry itself ----------------------------------------------------------------------------------------------------------

def _raw(es, a, b, rec, w, eq, tol, rule=None, chord=True, Coeffs=None):
    """vi_eval_slant_f64 on (P, 3) end points with the facet equations eq (None: no hull): (out, chord (2, P) or None)."""
    from volumetricinterp_amd import _lib
    ctx = es.model.ctx
    C = es.Coeffs if Coeffs is None else Coeffs
    x, wq = _gauss() if rule is None else rule
    n = len(a)
    bufs = []
    try:
        up = lambda v, dtype=np.float64: bufs.append(ctx.to_device(np.ascontiguousarray(v), dtype)) or bufs[-1]
        da, db, dr = up(a.T), up(b.T), up(rec, np.int32)
        dw = up(w) if w is not None else None
        dC = up(C) if len(C) else None
        dh = up(eq) if eq is not None else None
        dx, dq = up(x), up(wq)
        bufs.append(ctx.empty(n))
        dO = bufs[-1]
        dS = None
        if chord:
            bufs.append(ctx.empty((2, n)))
            dS = bufs[-1]
        ptr = lambda d: d.ptr if d is not None else None
        _lib.check(_lib.lib.vi_eval_slant_f64(es.model.handle(), n, da.ptr, db.ptr, dr.ptr, ptr(dw), len(C), ptr(dC), ptr(dh),
                                              0 if eq is None else eq.shape[0], tol, len(x), dx.ptr, dq.ptr, dO.ptr, ptr(dS)),
                   'vi_eval_slant_f64')
        return dO.download(), (dS.download() if chord else None)
    finally:
        for v in bufs:
            v.free()


@pytest.mark.parametrize('timeinterp', [False, True])
@pytest.mark.parametrize('tag', ['k8l2', 'scr_k12l2', 'rbf'])
def test_raw_abi_rows_outside(tag, timeinterp):
    """d_rec = -1, d_rec = R and - with d_w - d_rec = R - 1 give NaN, every other ray keeps its bits, the chord of a ray without
    a record is still written, d_chord = NULL is accepted, and R = 0 makes every ray NaN."""
    es = tt._estimate(tag, timeinterp)
    eq, tol = es._hull()
    _, _, a, b = _rays('oblique')
    rec, w = es.select_records(_times(es, P, seed=21))
    out, chord = _raw(es, a, b, rec, w, eq, tol)
    hit = ~np.isnan(chord[0])
    assert 0 < hit.sum() < P and np.array_equal(np.isnan(out), ~hit) and np.array_equal(np.isnan(chord[1]), ~hit)
    nochord, none = _raw(es, a, b, rec, w, eq, tol, chord=False)
    assert none is None and _same_bits(nochord, out)
    where = np.flatnonzero(hit)[[0, 1, 100, 101, 102, 300, -2, -1]]
    bad = rec.copy()
    bad[where] = [-1, R, -1, R, R + 7, -5, -1, R]
    if timeinterp:
        bad[where[[4, 5]]] = R - 1
    got, gchord = _raw(es, a, b, bad, w, eq, tol)
    lost = np.zeros(P, dtype=bool)
    lost[where] = True
    assert np.all(np.isnan(got[lost])) and np.isfinite(out[lost]).all()
    assert _same_bits(got[~lost], out[~lost])
    assert _same_bits(gchord, chord)                    # geometry only: the rays without a record have theirs
    empty, echord = _raw(es, a, b, rec, w, eq, tol, Coeffs=np.zeros((0, es.Coeffs.shape[1])))
    assert np.all(np.isnan(empty)) and _same_bits(echord, chord)


@pytest.mark.parametrize('timeinterp', [False, True])
def test_slant_failed_fit(timeinterp):
    """Record 17 all NaN (a failed fit).  Nearest mode: exactly its rays are NaN.  Interpolation mode: exactly the rays of the
    pairs that hold it, rec 16 and 17 - a ray at w == 0 of rec 16 among them, as get_C forms 1 * C_16 + 0 * C_17.  All other
    rays keep the bits of the intact file."""
    es = tt._estimate('k8l2', timeinterp)
    C = np.array(es.Coeffs)
    C[17] = np.nan
    broken = tt._estimate('k8l2', timeinterp, Coeffs=C)
    t0, rec, w = tt._runs(es, 5, R)
    first16 = int(np.flatnonzero(rec == 16)[0])
    t0[first16] = tt._mid(es.time)[16]                  # exactly on the mid-time: w == 0 in interpolation mode
    rec, w = es.select_records(t0)
    assert rec[first16] == 16 and (w is None or w[first16] == 0.)
    _, _, a, b = _rays('inside')
    a, b = a[:rec.size], b[:rec.size]
    good = es.slant(t0, a.T, b.T, coords='ecef', check_hull=False)
    out = broken.slant(t0, a.T, b.T, coords='ecef', check_hull=False)
    assert np.isfinite(good).all()
    lost = np.isin(rec, [16, 17]) if timeinterp else rec == 17
    assert np.array_equal(np.isnan(out), lost) and lost[first16] == timeinterp
    assert _same_bits(out[~lost], good[~lost])


@pytest.mark.parametrize('tag', ['default', 'k8l2'])
def test_raw_abi_buffers_regrow_on_one_handle(tag):
    """The model's grow-only buffers on ONE handle through vi_eval_f64 (300 x 3, all facets), vi_eval_slant_f64 (257 rays,
    blending, all facets: 40 prepared rows), vi_eval_f64 (5000 x 53) and the slant again: each result has the bits of the same
    call on a fresh model."""
    eq, tol = tt._estimate(tag, True)._hull()
    C53 = tt._records(tag, 53)[1]
    one = tt._estimate(tag, True)
    _, _, a, b = _rays('oblique')
    a, b = a[:257], b[:257]
    rec, w = one.select_records(_times(one, 257, seed=22))

    def evaluate(Q, T):
        lat, lon, alt = tt._box(np.random.default_rng(Q + T), Q)
        return lambda es: tt._raw_eval(es, lat, lon, alt, C53[:T], eq, tol)

    def slant(es):
        out, chord = _raw(es, a, b, rec, w, eq, tol)
        return np.concatenate([out[None, :], chord])
    steps = [('eval 300 x 3', evaluate(300, 3)), ('slant 257', slant), ('eval 5000 x 53', evaluate(5000, 53)), ('slant 257 again', slant)]
    for what, call in steps:
        out, fresh = call(one), call(tt._estimate(tag, True))
        assert np.array_equal(np.isnan(out), np.isnan(fresh)), what
        ok = ~np.isnan(fresh)
        assert 0 < ok.sum() < ok.size and _same_bits(out[ok], fresh[ok]), what


# ---- 9. the Python surface -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('timeinterp', [False, True])
def test_slant_api(timeinterp):
    from volumetricinterp_amd import geodesy
    es = tt._fixture_estimate('k8l2', timeinterp)
    mt = tt._mid(es.time)
    rng = np.random.default_rng(30)
    # one receiver, a (4, 5) array of satellites: the ray shape comes from broadcasting
    start = (78., 262., 0.)
    end = (rng.uniform(72, 84, (4, 5)), rng.uniform(240, 284, (4, 5)), 1000e3)
    # times a datetime holds exactly, so that datetimes and float seconds are the same instants
    t0 = np.round(rng.uniform(mt[0], mt[-1] - 1., (4, 5)) * 64.) / 64.
    times = np.array([tt._datetime(t) for t in t0.ravel()], dtype=object).reshape(t0.shape)
    out = es.slant(t0, start, end)
    assert out.shape == (4, 5) and out.dtype == np.float64 and 0 < np.isnan(out).sum() < out.size
    assert _same_bits(es.slant(times, start, end), out)
    assert _same_bits(es.slant(times.tolist(), start, end), out)
    # the same rays in ECEF
    a = geodesy.geodetic2ecef(*(np.full((4, 5), v) for v in start))
    b = geodesy.geodetic2ecef(end[0], end[1], np.full((4, 5), end[2]))
    assert _same_bits(es.slant(t0, a, b, coords='ecef'), out)
    # Gauss-Legendre by number of nodes is the rule of numpy, and `rule` overrides `nodes`
    assert _same_bits(es.slant(t0, start, end, nodes=3, rule=np.polynomial.legendre.leggauss(64)), out)
    assert not _same_bits(es.slant(t0, start, end, nodes=3), out)
    # out=, chord=
    buf = np.empty((4, 5))
    assert es.slant(t0, start, end, out=buf) is buf and _same_bits(buf, out)
    three = es.slant(t0, start, end, chord=True, out=buf)
    assert len(three) == 3 and three[0] is buf and all(v.shape == (4, 5) and v.dtype == np.float64 for v in three)
    assert np.array_equal(np.isnan(three[1]), np.isnan(out)) and np.array_equal(np.isnan(three[2]), np.isnan(out))
    with pytest.raises(ValueError, match='out must be'):
        es.slant(t0, start, end, out=np.empty(20))
    with pytest.raises(ValueError, match='out must be'):
        es.slant(t0, start, end, out=np.empty((4, 5), dtype=np.float32))
    with pytest.raises(ValueError, match='times must be'):
        es.slant(t0.ravel()[:7], start, end)
    with pytest.raises(ValueError, match='do not broadcast'):
        es.slant(t0, (np.zeros(3), 262., 0.), end)
    with pytest.raises(ValueError, match='coords must be'):
        es.slant(t0, start, end, coords='enu')
    with pytest.raises(ValueError, match='nodes must be'):
        es.slant(t0, start, end, nodes=257)
    with pytest.raises(ValueError, match='rule must be'):
        es.slant(t0, start, end, rule=([0., 1.], [1.]))
    with pytest.raises(ValueError, match='rule must be finite'):
        es.slant(t0, start, end, rule=([0., np.nan], [1., 1.]))
    with pytest.raises(ValueError, match='outside must be'):
        es.slant(t0, start, end, outside='zero')
    # one scalar time is broadcast
    t = tt._datetime(t0[1, 2])
    assert _same_bits(es.slant(t, start, end), es.slant(np.full((4, 5), t0[1, 2]), start, end))
    # without the hull the whole segment is integrated: every ray is a number, and not the clipped one
    whole = es.slant(t0, start, end, check_hull=False)
    assert np.isfinite(whole).all() and not np.any(whole == out)
    # a caller's rule with more nodes than the kernel's Gauss-Legendre limit: composite midpoint on 1000 panels
    xm = (np.arange(1000) + 0.5) / 500. - 1.
    mid = es.slant(t0, start, end, rule=(xm, np.full(1000, 2. / 1000)))
    ok = np.isfinite(out)
    assert np.array_equal(np.isnan(mid), ~ok) and np.allclose(mid[ok], out[ok], rtol=1e-3, atol=0.)
    # times outside the file
    late = t0.copy()
    late[0, :] = mt[-1] + 4000.
    with pytest.raises(ValueError) as e:
        es.slant(late, start, end)
    assert str(e.value) == tt.MESSAGE
    part, d0, d1 = es.slant(late, start, end, outside='nan', chord=True)
    assert np.all(np.isnan(part[0])) and _same_bits(part[1:], out[1:])
    assert _same_bits(d0, three[1]) and _same_bits(d1, three[2])        # the chord of a ray without a record is still given
    # non-finite end points; a segment of length zero inside the hull
    inside = (78., 262., 300e3)
    assert es.check_hull(*inside)
    odd = es.slant(t0[0, 0], (np.array([78., np.nan, 78.]), 262., np.array([300e3, 300e3, np.inf])), inside, chord=True)
    assert odd[0][0] == 0. and odd[1][0] == 0. and odd[2][0] == 0.
    assert all(np.isnan(v[1:]).all() for v in odd)
    # no ray: nothing to compute
    assert es.slant(np.zeros((0, 3)), (np.zeros((0, 3)), 262., 0.), end=(80., 262., 1e6)).shape == (0, 3)
