"""Every copy of the Legendre start-up on the device - sph_point and grad_hess_point (Model.basis, grad_basis, hess_basis, the
per-lane evaluation, K2tg), fast_chains (K2t), k_eval_sph_fast, K2m and K2s - with both seed branches, over the whole model
domain, against 50 digits: the fixtures tests/golden/domain_<tag>.npz (tools/gen_domain.py) assembled in np.longdouble by
tests/domain_ref.py.  The points: the pole of the cap (theta' = 1e-9, 1e-6, 1e-3 rad), the cap up to its edge, the 18-30 deg
band of the older tests, 45 ... 135 deg, both sides of the atan2 cut of phi', z < 0 and 3000 km, longitudes given 360 deg
lower and higher, lat = 90 - and the class `beyond` (145 ... 179.5 deg), where a model with non-integer degrees has no
converged seed series: there every output is within the gate or NaN (tests/test_basis_domain_host.py has the limit).

Orders (tag: MAXK, MAXL, CAP_LIM): k4l6c10 (4, 6, 10: integer seeds; fast tiles, K2m, K2t, K2tg, grad, hess), k4l6c15 (series
seeds in every one of those), k3l4c15 (VI_FAST(4, 3) with series seeds, no K2m), k2l5c12p7 (five degree groups: per-lane
kernels), k8l12c15 (K2s with 2, 3 and 4 groups, and k_eval_sph_fast at MAXL 12).  T = 21 coefficient rows: tiles of 16 + 4 + 1.

Gates.  The reference is always the fixture; a gate is the larger of the project's (L2: 1e-11 of a column's maximum for a basis;
L6: 1e-10 for an evaluation) and 4 x the oracle's own error against the fixture on the same points (domain_ref.ORACLE_ERR,
measured by tests/test_basis_domain_host.py; the factor 4 for the kernels' summation order and fmas):

    tag         basis    grad     hess     eval     tgrad    | oracle, pole class: basis    eval    -> gates
    k4l6c10     3.7e-13  3.6e-13  3.8e-13  6.0e-14  1.4e-13  |                     7.0e-08  5.2e-08    2.8e-07  2.1e-07
    k4l6c15     6.9e-13  3.1e-13  5.9e-13  6.4e-14  1.5e-13  |                     5.0e-08  3.8e-08    2.0e-07  1.6e-07
    k3l4c15     1.3e-13  1.3e-13  2.2e-13  1.1e-13  1.6e-13  |                     2.3e-08  3.7e-08    9.2e-08  1.5e-07
    k2l5c12p7   2.0e-13  2.8e-13  2.4e-13  1.8e-13  2.0e-13  |                     6.8e-08  7.8e-08    2.8e-07  3.2e-07
    k8l12c15    1.1e-12  4.7e-13  6.9e-13  4.0e-14  1.1e-13  |                     2.5e-07  6.2e-08    1.0e-06  2.5e-07

Outside the pole class 4 x the oracle's figure is below the project's gate everywhere, so the gates there are 1e-11 (basis,
gradient basis, Hessian basis: column-norm error over the in-domain points) and 1e-10 (evaluation, track, track gradient: per
point, |out[t, p] - ref[t, p]| <= g sum_n |C[t, n] B[p, n]| - a norm over points would hide the far, high ones where exp(-z/2)
is small).  In the pole class sin theta' = sqrt(1 - x^2) loses digits by construction, in the oracle as in the kernels (g.s
mirrors scipy.special.lpmv): at theta' = 1e-6 the rounding of x alone is 1e-4 of 1 - x^2; the class has the gate of its own
oracle figure.  Gradient and Hessian are gated where sin theta' >= 1e-3 and must be finite at theta' = 1e-3 rad.  At the integer
tag the `beyond` class must hold the gates too - the basis the in-domain one; gradient and Hessian, which at 179.5 deg divide by
sin^2 theta' = 7.6e-5, 4 x the oracle's figure on that class (4.4e-7 and 1.8e-6: SciPy is far less accurate there than the
kernels; the kernels' own figures are printed).

Kernel variants are chosen by switches read once per process, so each runs in a child process, one after the other: the
default dispatch, VINTERP_EVAL_MFMA=0, VINTERP_EVAL=generic and, for k8l12c15, VINTERP_SPLIT_NH=2 / 4 and VINTERP_EVAL_SPLIT=0.
A child evaluates every entry in several arrangements of the same points - (a) shuffled, (b) 64 copies of one cap point (a wave
that leaves the seed series at its first test) before the points sorted by theta', (c) 63 cap points and one 135 deg point in
one wave (one far lane holds the others to its last term), (d) Q = 1, 63, 65, 193 (partial waves) - and reports (a) in the
fixture's order and, per arrangement, how far any point's result is from (a) in ulps: only the exit of the series depends on
the other lanes and the terms past convergence are below 1e-17 of the sum, so the bits should agree; the gate is 4 ulp.
Estimate.track sorts its points by record, so there the arrangements are regrouped by the record of each point.
Model.grad_basis has no frame argument; the east-north-up frame is covered through Estimate.track_gradient."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import domain_ref as dr

pytestmark = pytest.mark.gpu

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 21
ULP_GATE = 4
SWITCHES = ('VINTERP_SPLIT_NH', 'VINTERP_EVAL_SPLIT', 'VINTERP_EVAL_MFMA', 'VINTERP_EVAL')
ALL_ENTRIES = ('basis', 'grad', 'hess', 'eval', 'track', 'track_interp', 'tgrad_model', 'tgrad_enu')
EVAL_ENTRIES = ('eval', 'track', 'track_interp', 'tgrad_model')
#           name: (environment, tags, entries)
VARIANTS = {'default': ({}, tuple(dr.TAGS), ALL_ENTRIES),
            'mfma0': ({'VINTERP_EVAL_MFMA': '0'}, ('k4l6c10', 'k4l6c15', 'k3l4c15'), EVAL_ENTRIES),
            'generic': ({'VINTERP_EVAL': 'generic'}, ('k4l6c10', 'k4l6c15', 'k3l4c15', 'k8l12c15'), EVAL_ENTRIES),
            'nh2': ({'VINTERP_SPLIT_NH': '2'}, ('k8l12c15',), ('eval',)),
            'nh4': ({'VINTERP_SPLIT_NH': '4'}, ('k8l12c15',), ('eval',)),
            'split0': ({'VINTERP_EVAL_SPLIT': '0'}, ('k8l12c15',), ('eval',))}
CHILD = '''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import test_gpu_basis_domain as g
np.savez(sys.argv[1], **g.child_results(sys.argv[2].split(","), sys.argv[3].split(",")))
'''


# ---- what a child process computes ------------------------------------------------------------------------------------------
def arrangements(tag):
    """{name: indices into the fixture's points}: the arrangements (a) - (d) of the module docstring."""
    f = dr.fixture(tag)
    P = f['lat'].size
    th = np.arctan2(f['y'], f['x'])
    perm = np.random.default_rng(1234).permutation(P)
    cap = np.flatnonzero(dr.in_class(f, 'cap'))
    far = np.flatnonzero(dr.in_class(f, 'wide') & (np.abs(np.degrees(th) - 135.) < 1e-3))[0]
    out = {'a': perm,
           'b': np.concatenate([np.full(64, cap[len(cap) // 2]), np.argsort(th, kind='stable')]),
           'c': np.concatenate([np.resize(cap, 63), [far]])}
    for Q in (1, 63, 65, 193):
        out['d%d' % Q] = np.resize(perm, Q)
    return out


def point_records(tag, interp):
    """(times, rec, w) per fixture point: the record a point is evaluated at along a track is a property of the point, so that
    its result does not depend on the arrangement.  rec and w as Estimate.select_records returns them for those times."""
    from volumetricinterp_amd import synth
    from volumetricinterp_amd.estimate import select_records
    P = dr.fixture(tag)['lat'].size
    time = synth.unix_times(T)
    mid = np.mean(time, axis=1)
    p = np.arange(P)
    r = (7 * p) % (T - 1)
    t0 = mid[r] + (60. * ((0.37 * p + 0.11) % 1.) if interp else 0.)
    rec, w = select_records(time, t0, 60., interp)
    assert np.array_equal(rec, r)
    return t0, rec, w


def _ulps(a, b):
    """The largest distance in units of the last place between the finite elements of a and b; inf where one is NaN and the
    other is not."""
    a, b = np.ravel(a), np.ravel(b)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return np.inf
    ok = np.isfinite(a) & np.isfinite(b)
    if not np.array_equal(a[~ok].view(np.uint64), b[~ok].view(np.uint64)) and not np.all(np.isnan(a[~ok])):
        return np.inf
    ia, ib = a[ok].view(np.int64), b[ok].view(np.int64)
    ia = np.where(ia < 0, np.int64(-2**63) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2**63) - ib, ib)
    return float(np.max(np.abs(ia.astype(np.longdouble) - ib.astype(np.longdouble)))) if ok.any() else 0.


def _entries(tag):
    """{entry: function of (fixture point indices, lat, lon, alt) -> array with the points on axis 0}"""
    from volumetricinterp_amd import synth
    from volumetricinterp_amd.estimate import Estimate
    C = dr.coefficients(tag, T)[0]
    cfg = dr.config_text(tag)
    hull = np.zeros((4, 3))
    es = {i: Estimate.from_arrays(C, None, synth.unix_times(T), hull, cfg, timeinterp=i) for i in (False, True)}
    m = es[False].model
    times = {i: point_records(tag, i)[0] for i in (False, True)}
    return {'basis': lambda ix, *g: m.basis(*g),
            'grad': lambda ix, *g: m.grad_basis(*g),
            'hess': lambda ix, *g: m.hess_basis(*g),
            'eval': lambda ix, *g: np.ascontiguousarray(es[False].evaluate_coeffs(C, *g, check_hull=False).T),
            'track': lambda ix, *g: es[False].track(times[False][ix], *g, check_hull=False),
            'track_interp': lambda ix, *g: es[True].track(times[True][ix], *g, check_hull=False),
            'tgrad_model': lambda ix, *g: es[False].track_gradient(times[False][ix], *g, check_hull=False, frame='model'),
            'tgrad_enu': lambda ix, *g: es[False].track_gradient(times[False][ix], *g, check_hull=False, frame='enu')}


def child_results(tags, entries):
    """Per tag and entry: '<tag>/<entry>' - the result of arrangement (a) in the fixture's order; '<tag>/<entry>/ulps' - per
    arrangement (sorted by name) the largest distance of a point's result from that, in ulps; '<tag>/<entry>/nonfinite' - with a
    NaN latitude, a +Inf longitude and a -Inf altitude in three lanes of arrangement (a): [those rows all NaN, largest distance
    of every other row from the clean run in ulps]."""
    res = {}
    for tag in tags:
        f = dr.fixture(tag)
        arr = arrangements(tag)
        fun = _entries(tag)
        for e in entries:
            def run(ix, poke=None):
                g = [np.array(f[n][ix]) for n in ('lat', 'lon', 'alt')]
                for (which, lane, value) in poke or ():
                    g[which][lane] = value
                return np.asarray(fun[e](ix, *g))
            first = run(arr['a'])
            base = np.empty_like(first)
            base[arr['a']] = first
            res['%s/%s' % (tag, e)] = base
            res['%s/%s/ulps' % (tag, e)] = np.array([_ulps(run(arr[a]), base[arr[a]]) for a in sorted(arr)])
            lanes = (3, 70, 110)
            bad = run(arr['a'], ((0, lanes[0], np.nan), (1, lanes[1], np.inf), (2, lanes[2], -np.inf)))
            keep = np.setdiff1d(np.arange(len(first)), lanes)
            res['%s/%s/nonfinite' % (tag, e)] = np.array([float(np.all(np.isnan(bad[list(lanes)]))),
                                                          _ulps(bad[keep], first[keep])])
    return res


# ---- the parent: children and gates -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _child(name):
    import tempfile
    env_set, tags, entries = VARIANTS[name]
    with tempfile.TemporaryDirectory() as d:
        script = os.path.join(d, 'domain_child.py')
        with open(script, 'w') as fh:
            fh.write(CHILD % (REPO_ROOT, os.path.join(REPO_ROOT, 'tests')))
        env = dict(os.environ)
        for k in SWITCHES:
            env.pop(k, None)
        env.update(env_set)
        o = os.path.join(d, name + '.npz')
        r = subprocess.run([sys.executable, script, o, ','.join(tags), ','.join(entries)], env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, '%s child: exit %d\n%s' % (name, r.returncode, r.stderr[-3000:])
        return dict(np.load(o))


def _masks(tag):
    f = dr.fixture(tag)
    dom = dr.in_domain(f)
    return f, dom, dr.in_class(f, 'pole'), dom & (f['y'] >= 1e-3)


def _check_columns(name, tag, what, A, Aref, sel_sets, fails):
    """Column-norm gate of a basis-like array (points on axis 0, basis functions last): over the in-domain point sets sel_sets
    {label: (mask, gate)} finite and within the gate; on the `beyond` class within the gate of the first set or NaN."""
    f, dom, pole, away = _masks(tag)
    ax = tuple(range(Aref.ndim - 1))
    scale = np.max(np.abs(Aref[dom & ~pole if what != 'basis' else dom]), axis=ax)
    scale = np.where(scale == 0, 1, scale)
    for label, (sel, g) in sel_sets.items():
        finite = bool(np.all(np.isfinite(A[sel])))
        e = float(np.max(np.abs(A[sel].astype(dr.LD) - Aref[sel]) / scale)) if finite else np.nan
        print('%-8s %-10s %-12s %-9s colnorm err %.2e (gate %.1e)' % (name, tag, what, label, e, g))
        if not (finite and e <= g):
            fails.append('%s %s %s %s: %.2e > %.1e or not finite' % (name, tag, what, label, e, g))
    g0 = next(iter(sel_sets.values()))[1]
    if what + '_beyond' in dr.ORACLE_ERR[tag]:          # integer degrees: the oracle's own figure on this class (domain_ref.py)
        g0 = dr.gate(tag, what + '_beyond')
    with np.errstate(invalid='ignore'):
        worst = np.nanmax(np.abs(A[~dom].astype(dr.LD) - Aref[~dom]) / scale) if np.isfinite(A[~dom]).any() else 0.
        off = np.abs(A[~dom].astype(dr.LD) - Aref[~dom]) / scale > g0                 # False where A is NaN
    print('%-8s %-10s %-12s beyond    worst finite colnorm err %.2e (gate %.1e)' % (name, tag, what, float(worst), g0))
    nan_pts = int(np.sum(np.any(np.isnan(A[~dom].reshape((~dom).sum(), -1)), axis=1)))
    print('%-8s %-10s %-12s beyond    %d of %d points with NaN, %d finite values outside the gate' % (
        name, tag, what, nan_pts, (~dom).sum(), int(off.sum())))
    if off.any():
        fails.append('%s %s %s: %d finite values outside the gate beyond the domain' % (name, tag, what, int(off.sum())))
    if tag in dr.INTEGER_TAGS and nan_pts:
        fails.append('%s %s %s: NaN at integer degrees' % (name, tag, what))


def _check_points(name, tag, what, out, ref, S, sel, fails, kind='eval'):
    """Per-point gate of densities or gradient components: out, ref, S of one shape with the points on axis 0; finite and
    |out - ref| <= g S on the points `sel`, with the pole class at its own g; on the `beyond` class that or NaN."""
    f, dom, pole, away = _masks(tag)
    shape = (-1,) + (1,) * (ref.ndim - 1)
    g = (dr.point_gates(tag, kind) if kind == 'eval' else np.full(pole.size, dr.gate(tag, kind))).reshape(shape)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = (np.abs(out.astype(dr.LD) - ref) / S).astype(np.float64)
    for label, m in (('in domain', sel & ~pole), ('pole', sel & pole)):
        if not m.any():
            continue
        worst = float(np.max(ratio[m])) if np.all(np.isfinite(out[m])) else np.nan
        print('%-8s %-10s %-12s %-9s per-point err %.2e of sum |C B| (gate %.1e)' % (
            name, tag, what, label, worst, float(np.max(g[m]))))
        if not np.all(ratio[m] <= np.broadcast_to(g, ratio.shape)[m]):
            fails.append('%s %s %s %s: %.2e' % (name, tag, what, label, worst))
    off = ~(ratio[~dom] <= dr.gate(tag, kind)) & ~np.isnan(out[~dom])
    print('%-8s %-10s %-12s beyond    %d of %d values NaN, %d finite outside the gate' % (
        name, tag, what, int(np.isnan(out[~dom]).sum()), out[~dom].size, int(off.sum())))
    if off.any():
        fails.append('%s %s %s: %d finite values outside the gate beyond the domain' % (name, tag, what, int(off.sum())))
    if tag in dr.INTEGER_TAGS and np.isnan(out[~dom]).any():
        fails.append('%s %s %s: NaN at integer degrees' % (name, tag, what))


def _track_reference(tag, interp, M, Mabs):
    """Reference and scale of a track from per-record arrays M, Mabs (T, P, ...): the record of each point, or the blend."""
    _, rec, w = point_records(tag, interp)
    p = np.arange(rec.size)
    if w is None:
        return M[rec, p], Mabs[rec, p]
    w = w.astype(dr.LD).reshape((-1,) + (1,) * (M.ndim - 2))
    return (1 - w) * M[rec, p] + w * M[rec + 1, p], (1 - w) * Mabs[rec, p] + w * Mabs[rec + 1, p]


def _check_variant(name):
    import hessian_ref
    import oracle
    env, tags, entries = VARIANTS[name]
    res = _child(name)
    fails = []
    for tag in tags:
        f, dom, pole, away = _masks(tag)
        C, ref, S = dr.coefficients(tag, T)
        Cl = C.astype(dr.LD)
        for e in entries:
            out = res['%s/%s' % (tag, e)]
            if e == 'basis':
                _check_columns(name, tag, e, out, dr.basis(tag), {'in domain': (dom & ~pole, dr.gate(tag, 'basis')),
                                                                  'pole': (pole, dr.gate(tag, 'basis_pole'))}, fails)
            elif e in ('grad', 'hess'):
                Gr, Hr = dr.grad_hess(tag)
                _check_columns(name, tag, e, out, Gr if e == 'grad' else Hr, {'in domain': (away, dr.gate(tag, e))}, fails)
                if not np.all(np.isfinite(out[pole & (f['y'] > 5e-4)])):
                    fails.append('%s %s %s: not finite at theta\' = 1e-3 rad' % (name, tag, e))
            elif e == 'eval':
                _check_points(name, tag, e, out, ref.T, S.T, dom, fails)
            elif e in ('track', 'track_interp'):
                r, s = _track_reference(tag, e == 'track_interp', ref, S)
                _check_points(name, tag, e, out, r, s, dom, fails)
            else:
                Gr = dr.grad_hess(tag)[0]
                with np.errstate(invalid='ignore'):
                    M = np.einsum('tn,pcn->tpc', Cl, Gr)
                    Mabs = np.einsum('tn,pcn->tpc', np.abs(Cl), np.abs(Gr))
                if e == 'tgrad_enu':
                    maxk, maxl, cap = dr.TAGS[tag]
                    F = hessian_ref.enu_frame(oracle.SphHarmLagOracle(maxk=maxk, maxl=maxl, cap_lim_deg=cap), f['lat'], f['lon'],
                                              f['alt']).astype(dr.LD)
                    with np.errstate(invalid='ignore'):
                        M, Mabs = np.einsum('pic,tpc->tpi', F, M), np.einsum('pic,tpc->tpi', np.abs(F), Mabs)
                r, s = _track_reference(tag, False, M, Mabs)
                _check_points(name, tag, e, out, r, s, away, fails, kind='tgrad')
                if not np.all(np.isfinite(out[pole & (f['y'] > 5e-4)])):
                    fails.append('%s %s %s: not finite at theta\' = 1e-3 rad' % (name, tag, e))
            ulps = res['%s/%s/ulps' % (tag, e)]
            print('%-8s %-10s %-12s arrangements %s: ulps from (a) %s' % (name, tag, e, sorted(arrangements(tag)), ulps))
            if not np.all(ulps <= ULP_GATE):
                fails.append('%s %s %s: a point\'s result moves with the arrangement by %s ulps' % (name, tag, e, ulps))
            rows_nan, others = res['%s/%s/nonfinite' % (tag, e)]
            if not (rows_nan == 1. and others == 0.):
                fails.append('%s %s %s: non-finite inputs: rows NaN %s, other rows %s ulps from the clean run' % (
                    name, tag, e, rows_nan, others))
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('name', list(VARIANTS))
def test_domain_against_fixture(name):
    """One kernel variant (VARIANTS) in a child process: every entry at every tag of the variant within its gate on the in-domain
    points, within the gate or NaN beyond, identical between the arrangements, NaN rows for non-finite inputs."""
    _check_variant(name)


def test_variants_reach_their_kernels():
    """The switches do select other kernels: the evaluation of a variant differs from the default dispatch's in some bit at every
    tag it names (generic: the per-lane kernel in place of the tiles; mfma0: the VALU tiles in place of K2m; nh2, nh4, split0:
    another grouping of the chains) - except where the default already is the kernel the switch falls back to."""
    base = _child('default')
    same = []
    for name, (env, tags, entries) in VARIANTS.items():
        if name == 'default':
            continue
        res = _child(name)
        for tag in tags:
            a, b = res['%s/eval' % tag], base['%s/eval' % tag]
            ok = np.isfinite(a) & np.isfinite(b)
            if np.array_equal(a[ok], b[ok]):
                same.append((name, tag))
    print('bit-identical to the default dispatch:', same)
    # k3l4c15 has no K2m instantiation (mfma0 changes nothing there); every other pair is another kernel
    assert set(same) <= {('mfma0', 'k3l4c15')}, same
