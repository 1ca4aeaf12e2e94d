"""The whole-domain fixtures (tests/golden/domain_<tag>.npz, exact factors from tools/gen_domain.py) against the CPU
restatements, before anything touches a device: the oracle's basis and grad_basis, hessian_ref.hess_basis and
emulate.basis_from_tables (the NumPy restatement of sph_point on the device tables) are compared with the basis, gradient basis
and Hessian basis that tests/domain_ref.py assembles from the fixture in np.longdouble.  No GPU.

What this file establishes:
  * the oracle's own error against the exact values per tag and point class - the figures ORACLE_ERR of domain_ref.py, from which
    the gates of tests/test_gpu_basis_domain.py follow (gate = max(project gate, 4 x oracle error)), are upper bounds of what is
    measured here;
  * the device recurrence, restated on the host, holds the basis gate on every in-domain point;
  * the domain limit: on a theta' scan along one meridian, integer-degree models hold the gate up to 179.5 deg; models with
    non-integer degrees hold it up to DOMAIN_LIMIT_DEG, where the table of the seed series (HYP_TERMS) runs out, and return NaN -
    never a finite value outside the gate - beyond it.
Every test prints its figures (pytest -s)."""
import functools
import io

import numpy as np
import pytest

import domain_ref as dr
import hessian_ref
from emulate import basis_from_tables

TAGS = list(dr.TAGS)


def _oracle(tag):
    import oracle
    maxk, maxl, cap = dr.TAGS[tag]
    return oracle.SphHarmLagOracle(maxk=maxk, maxl=maxl, cap_lim_deg=cap)


def _tables(tag):
    from volumetricinterp_amd.models.sphharmlag import Model
    return Model(io.StringIO(dr.config_text(tag))).device_tables()


@functools.lru_cache(maxsize=None)
def _oracle_outputs(tag):
    f = dr.fixture(tag)
    o = _oracle(tag)
    A = o.basis(f['lat'], f['lon'], f['alt'])
    G = o.grad_basis(f['lat'], f['lon'], f['alt'])
    H = hessian_ref.hess_basis(o, f['lat'], f['lon'], f['alt'])
    return A, G, H


def _per_class(f, X, Xref, dom):
    return {c: dr.col_err(X, Xref, dom & dr.in_class(f, c), dom) for c in f['classes'] if c != 'beyond'}


def test_fixture_point_classes():
    """The point set is what the issue lists: every class present, the `beyond` class at most 15 %, the cap edge itself,
    both sides of the atan2 cut, z < 0, the same longitude given twice, lat = 90 exactly."""
    for tag in TAGS:
        f = dr.fixture(tag)
        n = {c: int(dr.in_class(f, c).sum()) for c in f['classes']}
        print(tag, n)
        assert all(v > 0 for v in n.values()), n
        assert n['beyond'] <= 0.15 * f['lat'].size
        th = np.degrees(np.arctan2(f['y'], f['x']))
        assert np.all(th[dr.in_class(f, 'beyond')] > 144.) and np.all(th[dr.in_domain(f)] < 135.001)
        assert np.min(np.abs(th[dr.in_class(f, 'cap')] - dr.TAGS[tag][2])) < 1e-6
        assert np.min(th) < 1e-7 and np.sum(f['y'] < 1e-3) >= 6
        cut = dr.in_class(f, 'azimuth') & (f['cphi'] < -0.999999)
        assert np.any(f['sphi'][cut] > 0) and np.any(f['sphi'][cut] < 0) and np.all(np.abs(f['sphi'][cut]) < 1e-11)
        assert np.any(f['z'] < 0) and np.max(f['z']) > 40.
        assert np.any(f['lon'] < 0) and np.any(f['lon'] > 360.) and np.any(f['lat'] == 90.)
        # unit vectors and sin^2 + cos^2 of the 50-digit geometry, to the rounding of the stored float64
        assert np.max(np.abs(f['x']**2 + f['y']**2 - 1)) < 5e-16 and np.max(np.abs(f['cphi']**2 + f['sphi']**2 - 1)) < 5e-16


@pytest.mark.parametrize('tag', TAGS)
def test_oracle_against_fixture(tag):
    """The oracle's basis and grad_basis and hessian_ref.hess_basis against the fixture on the in-domain points, per class: the
    recorded figures ORACLE_ERR[tag] (domain_ref.py), which set the gates of the GPU test, bound what is measured."""
    f = dr.fixture(tag)
    A, G, H = _oracle_outputs(tag)
    B = dr.basis(tag)
    Gr, Hr = dr.grad_hess(tag)
    dom = dr.in_domain(f)
    away = dom & (f['y'] >= 1e-3)                      # the gradient and the Hessian are exempt at the pole of the cap
    eb, eg, eh = _per_class(f, A, B, dom), _per_class(f, G, Gr, away), _per_class(f, H, Hr, away)
    for c in eb:
        print('%-10s %-14s basis %.1e  grad %.1e  hess %.1e' % (tag, c, eb[c], eg[c], eh[c]))
    C, ref, S = dr.coefficients(tag)
    pole = dr.in_class(f, 'pole')
    ep = np.max(np.abs((C @ A.T).astype(dr.LD) - ref) / S, axis=0).astype(np.float64)
    rest = lambda e: max(v for c, v in e.items() if c != 'pole')
    Cl = C.astype(dr.LD)
    M, Mabs = np.einsum('tn,pcn->tpc', Cl, Gr[away]), np.einsum('tn,pcn->tpc', np.abs(Cl), np.abs(Gr[away]))
    et = float(np.max(np.abs(np.einsum('tn,pcn->tpc', C, G[away]).astype(dr.LD) - M) / Mabs))
    got = dict(tgrad=et, basis=rest(eb), grad=rest(eg), hess=rest(eh), eval=float(np.max(ep[dom & ~pole])), basis_pole=eb['pole'],
               eval_pole=float(np.max(ep[pole])))
    if tag in dr.INTEGER_TAGS:                       # gradient and Hessian at integer degrees past 135 deg, up to 179.5 deg
        got.update(grad_beyond=dr.col_err(G, Gr, ~dom, away), hess_beyond=dr.col_err(H, Hr, ~dom, away))
    print('%-10s measured: ' % tag + '  '.join('%s %.2e' % kv for kv in got.items()))
    print('%-10s gates:    ' % tag + '  '.join('%s %.2e' % (w, dr.gate(tag, w)) for w in got))
    assert np.all(np.isfinite(A[dom])) and np.all(np.isfinite(G[away])) and np.all(np.isfinite(H[away]))
    for what, e in got.items():
        assert e <= dr.ORACLE_ERR[tag][what], (what, e, dr.ORACLE_ERR[tag][what])


@pytest.mark.parametrize('tag', TAGS)
def test_device_recurrence_against_fixture(tag):
    """emulate.basis_from_tables - the device's seeds and chains on the device's tables, in NumPy - against the fixture on the
    in-domain points at the basis gate; beyond, at a non-integer tag, within the gate or NaN."""
    f = dr.fixture(tag)
    maxk, maxl, _ = dr.TAGS[tag]
    A = basis_from_tables(_tables(tag), maxk, maxl, f['lat'], f['lon'], f['alt'])
    B = dr.basis(tag)
    dom = dr.in_domain(f)
    e = _per_class(f, A, B, dom)
    for c, v in e.items():
        print('%-10s %-14s emulated device basis %.1e' % (tag, c, v))
    assert np.all(np.isfinite(A[dom]))
    assert max(v for c, v in e.items() if c != 'pole') <= dr.gate(tag, 'basis') and e['pole'] <= dr.gate(tag, 'basis_pole'), e
    scale = np.max(np.abs(B[dom]), axis=0)
    bad = np.abs(A[~dom].astype(dr.LD) - B[~dom]) / scale > dr.gate(tag, 'basis')          # False where A is NaN
    assert not np.any(bad), 'finite values outside the gate beyond the domain: %d' % bad.sum()
    if tag in dr.INTEGER_TAGS:
        assert np.all(np.isfinite(A))


def _scan(tag):
    """(theta' in deg, error per scan point relative to the column maxima over theta' <= 135 deg, NaN where the emulation is)."""
    f = dr.fixture(tag)
    maxk, maxl, _ = dr.TAGS[tag]
    A = basis_from_tables(_tables(tag), maxk, maxl, f['scan_lat'], f['scan_lon'], f['scan_alt'])
    B = dr.basis(tag, scan=True)
    th = f['scan_theta']
    scale = np.max(np.abs(B[th <= 135.]), axis=0)
    with np.errstate(invalid='ignore'):
        return th, np.max(np.abs(A.astype(dr.LD) - B) / scale, axis=1).astype(np.float64)


def test_domain_limit_on_the_scan():
    """The theta' scan (0.25 deg steps between 136 and 152 deg): integer-degree tags hold the basis gate up to 179.5 deg;
    every non-integer tag holds it up to DOMAIN_LIMIT_DEG and gives NaN, or a value within the gate, past that - no finite
    value outside the gate anywhere."""
    limits = {}
    for tag in TAGS:
        th, err = _scan(tag)
        g = dr.gate(tag, 'basis')
        ok = err <= g                                                   # False where NaN
        first_bad = int(np.argmin(ok)) if not np.all(ok) else len(th)
        limits[tag] = float(th[first_bad - 1])
        print('%-10s holds %.1e up to %.2f deg; worst finite error %.1e; NaN from %s deg' % (
            tag, g, limits[tag], np.nanmax(err), th[np.isnan(err)][0] if np.isnan(err).any() else '-'))
        assert not np.any(np.isfinite(err) & ~ok), (tag, th[np.isfinite(err) & ~ok])
        if tag in dr.INTEGER_TAGS:
            assert limits[tag] == 179.5
        else:
            assert limits[tag] >= dr.DOMAIN_LIMIT_DEG, (tag, limits[tag])
    print('measured domain limit of the non-integer tags: %.2f deg' % min(v for t, v in limits.items() if t not in dr.INTEGER_TAGS))
    assert min(v for t, v in limits.items() if t not in dr.INTEGER_TAGS) == dr.DOMAIN_LIMIT_DEG
