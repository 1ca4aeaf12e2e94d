"""The hull mask of every masked call (prepare_call -> launch_hull_mask: k_hull_mask_mx on the matrix cores, k_hull_mask with
VINTERP_HULL=fp32, prep_hull_body; csrc/vi_basis.hip) and the ray clip (slant_clip, csrc/vi_slant.hip), facet by facet at every
list size, against answers that tests/hull_ref.py decides on the host in np.longdouble before the device sees a case: tangent
polytopes whose points are outside by ONE known facet or inside, so that a wrong slot in the last, partial tile, a facet dropped
at F % 32 == 1 or a half-maximum taken from the wrong lane group shows as a wrong bit.  tests/test_hull_ref_host.py checks the
constructions themselves (no point is left out, the margins hold, the paths of the prefilter each case takes).

The mask is read through the raw entry: vi_eval_f64 with T = 1 and zero coefficients on a MAXK 2 x MAXL 2 model whose basis is
finite everywhere (integer degrees: test_the_unmasked_output_is_finite_at_every_point), so the mask is isfinite of the output.
Every mask comparison is np.array_equal against the constructed answer; a failure prints case, F, facet, tile, slot, delta,
sigma and the position of the point in its workgroup.

Every mask call of the groups of GROUPS is recorded under a name; the last test repeats them all in ONE child process with
VINTERP_HULL=fp32 (the switch is read once per process) and asks for the same bits.  Run as a script, this file is that child."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import hull_ref as hr

pytestmark = pytest.mark.gpu

CFG = ('[DEFAULT]\n[MODEL]\nNAME = sphharmlag\nMAXK = 2\nMAXL = 2\nCAP_LIM = 10\nMAX_Z_INT = INF\nLATCP = 78\nLONCP = 262\n')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WG = 1024                    # points of a workgroup of k_hull_mask_mx: 256 threads x 4 points, point q0 + 256 u of thread q0
SEEN = {}                    # name of a recorded call -> its mask, for the comparison with the packed-fp32 pass


@functools.lru_cache(maxsize=None)
def _estimate(hull=None):
    from volumetricinterp_amd import synth
    from volumetricinterp_amd.estimate import Estimate
    hv = np.zeros((4, 3)) if hull is None else hr.qhull_input(hull)[0]
    return Estimate.from_arrays(np.zeros((1, 8)), None, synth.unix_times(1), hv, CFG)


def mask_of(eq, tol, lat, lon, alt):
    """The mask of one raw call: vi_eval_f64, T = 1, zero coefficients, the list eq (F, 4) and tol as given; F = 0 without eq."""
    from volumetricinterp_amd import _lib
    m = _estimate().model
    Q = len(lat)
    with m.ctx.scope() as dev:
        dq = [dev.up(np.ascontiguousarray(v, dtype=np.float64)) for v in (lat, lon, alt)]
        dC, dout = dev.up(np.zeros((1, m.nbasis))), dev.empty((1, Q))
        de = None if eq is None else dev.up(np.ascontiguousarray(eq, dtype=np.float64))
        _lib.check(_lib.lib.vi_eval_f64(m.handle(), Q, dq[0].ptr, dq[1].ptr, dq[2].ptr, 1, dC.ptr, None if de is None else de.ptr,
                                        0 if eq is None else len(eq), float(tol), dout.ptr), 'vi_eval_f64')
        out = dout.download()[0]
    if eq is not None:
        assert np.all(np.isnan(out) | (out == 0.))
    return np.isfinite(out)


# ---- the calls: (name, eq, tol, lat, lon, alt, expect, explain) with explain(wrong positions) -> text -------------------------------

def _orders(b, tag=None, eq=None, tol=None, orders=('facet', 'shuffled', 'alone')):
    """The points of the built case b in three orders: by facet; shuffled; each point alone in a wave of points far outside
    (point i at position 64 i + i % 64: every lane, and with the waves every one of the four points a thread carries)."""
    name = tag or hr.case_name(b.case)
    eq = b.eq if eq is None else eq
    tol = b.tol if tol is None else tol
    P = len(b.lat)
    for order in orders:
        if order == 'facet':
            idx = np.arange(P)
        else:
            idx = np.random.default_rng(P).permutation(P)
        if order == 'alone':
            pos = 64 * np.arange(P) + np.arange(P) % 64
            flat, flon, falt = hr.far_outside(b.case)
            lat, lon, alt = np.full(64 * P, flat), np.full(64 * P, flon), np.full(64 * P, falt)
            lat[pos], lon[pos], alt[pos] = b.lat[idx], b.lon[idx], b.alt[idx]
            expect = np.zeros(64 * P, dtype=bool)
            expect[pos] = b.expect[idx]
        else:
            pos = np.arange(P)
            lat, lon, alt, expect = b.lat[idx], b.lon[idx], b.alt[idx], b.expect[idx]
        yield name + '/' + order, eq, tol, lat, lon, alt, expect, _explainer(b, idx, pos)


def _explainer(b, idx, pos):
    def explain(wrong):
        at = {int(q): int(i) for i, q in zip(idx, pos)}
        known = [q for q in wrong if int(q) in at]
        text = hr.describe(b, [at[int(q)] for q in known], known)
        if len(known) < len(wrong):
            text += '\n  and %d filler points, first at %s' % (len(wrong) - len(known),
                                                                [int(q) for q in wrong if int(q) not in at][:8])
        return text
    return explain


def calls_slots():
    """Every facet slot - every F of the list at 200 km, facet 0 radial and horizontal, three orders."""
    for c in hr.slot_cases():
        yield from _orders(hr.build(c))


def calls_places():
    """The scales and places; the prefilter switched off at 20 200 km."""
    for c in hr.place_cases():
        yield from _orders(hr.build(c), 'places/' + hr.case_name(c))


def calls_invariances():
    """Permutations of the list, scaled lists, a dilated hull, one handle at F = 1025, 4, 1025."""
    for f0 in ('radial', 'horizontal'):
        b = hr.build(hr.Case(33, 2e5, 'north', f0))
        name = hr.case_name(b.case)
        for k in range(1, 33):                  # every rotation of the list: every facet is facet 0 - the reference point - once
            yield from _orders(b, '%s/rotated%d' % (name, k), eq=np.roll(b.eq, k, axis=0), orders=('shuffled',))
        yield from _orders(b, name + '/reversed', eq=b.eq[::-1], orders=('shuffled', 'alone'))
    for F in (257, 1025):
        b = hr.build(hr.Case(F, 2e5, 'north', 'radial'))
        name = hr.case_name(b.case)
        yield from _orders(b, name + '/reversed', eq=b.eq[::-1], orders=('facet', 'alone'))
        perm = np.random.default_rng(F).permutation(F)
        yield from _orders(b, name + '/permuted', eq=b.eq[perm], orders=('facet', 'alone'))
    dil = hr.build(hr.Case(257, 2e5, 'north', 'radial', 'neg', 500.))
    yield from _orders(dil)
    for b in (hr.build(hr.Case(257, 2e5, 'north', 'horizontal')), dil):
        for f in (3., 1e-3):
            yield from _orders(b, '%s/times%g' % (hr.case_name(b.case), f), eq=b.eq * f, tol=b.tol * f, orders=('shuffled', 'alone'))
    for i, F in enumerate((1025, 4, 1025)):
        yield from _orders(hr.build(hr.Case(F, 2e5, 'north', 'radial')), 'reuse%d-F%d' % (i, F), orders=('facet',))


LANES_CASE = hr.Case(257, 2e6, 'north', 'radial')


def calls_lanes():
    """Q = 1024 x 1024.  In workgroup b every point is far outside - decided by tile 0 - except point b, which is outside
    only by facet 256, the one facet of the last tile (F = 257), by 300 m (the fp16 products decide: outside the band) or by
    1e-2 m (the fp64 test decides); then the same with point b inside; then the complement: every point deep inside, point b
    outside by the last facet.  The late point sits on every lane of every one of the four points a thread carries."""
    b = hr.build(LANES_CASE)
    f = LANES_CASE.F - 1
    at = WG * np.arange(WG) + np.arange(WG)
    for step in (3, 0):
        out_p, in_p = 8 * f + 2 * step, 8 * f + 2 * step + 1
        assert b.facet[out_p] == f and b.step[out_p] == step and b.sigma[out_p] > 0 and b.sigma[in_p] < 0
        assert b.outband[out_p] and b.outband[in_p] if step == 3 else b.inband[out_p] and b.inband[in_p]
        for tag, fill, p in (('far+out', hr.far_outside(LANES_CASE), out_p), ('far+in', hr.far_outside(LANES_CASE), in_p),
                             ('deep+out', hr.deep_inside(LANES_CASE), out_p)):
            lat, lon, alt = (np.full(WG * WG, v) for v in fill)
            lat[at], lon[at], alt[at] = b.lat[p], b.lon[p], b.alt[p]
            expect = np.full(WG * WG, tag.startswith('deep'))
            expect[at] = b.expect[p]
            idx = np.full(WG, p)
            yield ('lanes/%s/delta%g' % (tag, b.delta[p]), b.eq, b.tol, lat, lon, alt, expect, _explainer(b, idx, at))


SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)


def calls_sizes():
    """Prefixes of the shuffled F = 33 set, repeated cyclically to 2049 points."""
    for f0 in ('radial', 'horizontal'):
        b = hr.build(hr.Case(33, 2e5, 'north', f0))
        P = len(b.lat)
        idx = np.resize(np.random.default_rng(33).permutation(P), max(SIZES))
        for Q in SIZES:
            i = idx[:Q]
            yield ('%s/Q%d' % (hr.case_name(b.case), Q), b.eq, b.tol, b.lat[i], b.lon[i], b.alt[i], b.expect[i],
                   _explainer(b, i, np.arange(Q)))


GROUPS = {'slots': calls_slots, 'places': calls_places, 'invariances': calls_invariances, 'lanes': calls_lanes,
          'sizes': calls_sizes}


def _run(group, check=True):
    """Runs the calls of a group, records the masks, and asserts each against its constructed answer."""
    t0 = time.perf_counter()
    n = q = 0
    failures = []
    for name, eq, tol, lat, lon, alt, expect, explain in GROUPS[group]():
        got = mask_of(eq, tol, lat, lon, alt)
        assert name not in SEEN or np.array_equal(SEEN[name], got), 'the call %s gave another mask the second time' % name
        SEEN[name] = got
        n, q = n + 1, q + len(lat)
        if check and not np.array_equal(got, expect):
            failures.append('%s: %s' % (name, explain(np.flatnonzero(got != expect))))
    print('%s: %d calls, %d points, %.2f s' % (group, n, q, time.perf_counter() - t0))
    assert not failures, '%d of %d calls wrong\n' % (len(failures), n) + '\n'.join(failures[:20])


# ---- the mask through the raw entry ---------------------------------------------------------------------------------------------------------------

def test_the_unmasked_output_is_finite_at_every_point():
    """What lets isfinite be the mask: without a hull the zero-coefficient output is finite (0) at every point the cases use,
    the fillers included - from 1700 km below the ellipsoid to 20 400 km above it, both poles' neighbourhoods."""
    pts = [np.array([hr.far_outside(c) for c in hr.all_cases()]).T, np.array([hr.deep_inside(c) for c in hr.all_cases()]).T]
    for c in hr.all_cases():
        b = hr.build(c)
        pts.append(np.array([b.lat, b.lon, b.alt]))
    lat, lon, alt = np.concatenate(pts, axis=1)
    out = mask_of(None, 0., lat, lon, alt)
    assert out.all(), np.flatnonzero(~out)[:10]


def test_every_facet_slot_in_three_orders():
    for c in hr.slot_cases():
        b = hr.build(c)
        assert b.dropped == 0
        print('%s: off %d, in band %d, outside band %d' % (hr.case_name(c), b.off.sum(), b.inband.sum(), b.outband.sum()))
    _run('slots')


def test_scales_places_and_the_prefilter_switched_off():
    for c in hr.place_cases():
        b = hr.build(c)
        assert b.dropped == 0 and (b.off.all() if c.centre == 'gnss' else not b.off.any())
        print('%s: off %d, in band %d, outside band %d' % (hr.case_name(c), b.off.sum(), b.inband.sum(), b.outband.sum()))
    _run('places')


def test_permuted_scaled_dilated_lists_and_a_reused_handle():
    _run('invariances')


def test_the_late_point_on_every_lane():
    _run('lanes')


def test_query_sizes():
    _run('sizes')


# ---- Qhull hulls through Estimate.check_hull ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', hr.QHULL_NAMES)
def test_qhull_hulls_through_check_hull(name):
    """Hulls as a fit stores them - synth.beams geometries of 44 and 460 facets, a box whose 12 triangles are coplanar pairs -
    through Estimate.check_hull (hull_equations, order_facets, vi_eval_f64_host): points +- delta off every facet's centroid,
    decided in longdouble with the margins of the tangent polytopes and none left out; and the hull's own vertices, which lie
    ON it: a vertex whose largest longdouble plane distance is at most tol - 8 eps max |x| must be inside - the device's ECEF
    is within a few ulps of a coordinate (eps |x| each) and its three FMAs add one more of the offset, so 8 eps max |x|
    (1.2e-8 m) bounds what it may add to a distance - and at least nine vertices in ten are that clear."""
    hv, tol = hr.qhull_input(name)
    q = hr.qhull_case(hv, tol)
    assert q.dropped == 0
    es = _estimate(name)
    assert es._hull()[1] == tol and len(es._hull()[0]) == len(q.eq)
    for order in ('facet', 'shuffled'):
        idx = np.arange(len(q.lat)) if order == 'facet' else np.random.default_rng(1).permutation(len(q.lat))
        got = es.check_hull(q.lat[idx], q.lon[idx], q.alt[idx])
        wrong = np.flatnonzero(got != q.expect[idx])
        assert wrong.size == 0, ['facet %d (group %d) delta %g sigma %+d at p = %d' % (q.facet[idx[w]], q.group[q.facet[idx[w]]],
                                                                                       q.delta[idx[w]], q.sigma[idx[w]], w)
                                 for w in wrong[:12]]
    clear = np.array(q.vdist <= hr.LD(tol) - hr.LD(8. * hr.EPS * np.abs(hv).max()))
    print('%s: %d facets, %d points off them, %d of %d vertices clear of tol' % (name, len(q.eq), len(q.lat), clear.sum(), len(hv)))
    assert clear.mean() >= 0.9
    on = es.check_hull(q.vlat, q.vlon, q.valt)
    assert np.all(on[clear]), np.flatnonzero(clear & ~on)


# ---- the ray clip ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('F', hr.F_LIST)
def test_ray_clip_facet_by_facet(F):
    """Estimate.slant (vi_eval_slant_f64) with coords='ecef', chord=True on the ray set of F facets: NaN chord and NaN integral
    exactly where the longdouble clip has none, 0 and |b - a| exactly where the construction puts an end inside, a clipped end
    within 64 eps (|a| + |b|) metres of the longdouble clip; at 1, 63 and 65 rays and the whole set."""
    from volumetricinterp_amd import synth
    from volumetricinterp_amd.estimate import Estimate, slant_rays
    r = hr.ray_set(F)
    assert r.dropped == 0
    es = Estimate.from_arrays(np.zeros((2, 8)), None, synth.unix_times(2), np.zeros((4, 3)), CFG)
    es._hull_eq = (r.eq, r.tol)                                   # the list of the case in place of a Qhull hull
    t0 = float(synth.unix_times(2)[0].mean())
    worst = 0.
    n = len(r.a)
    for P in sorted({min(p, n) for p in (1, 63, 65, n)}):
        rays = slice(0, n) if P == n else slice(n - P, n) if P == 65 else slice(min(7, n - P), min(7, n - P) + P)
        a, b = r.a[rays], r.b[rays]
        val, d0, d1 = es.slant(t0, tuple(a.T), tuple(b.T), nodes=4, coords='ecef', chord=True)
        pa, pb = slant_rays(tuple(a.T), tuple(b.T), 4, None, 'ecef')[3:]
        length = np.linalg.norm(pb - pa, axis=0)                  # the |b - a| slant multiplies the fractions with
        worst = max(worst, hr.check_chords(r, d0, d1, rays, length))
        assert np.array_equal(np.isnan(val), np.isnan(d0)) and np.all(val[~np.isnan(val)] == 0.)
    print('F = %d: %d rays, largest |end - longdouble end| / (64 eps (|a| + |b|)) = %.3g' % (F, len(r.a), worst))


# ---- the packed-fp32 pass ----------------------------------------------------------------------------------------------------------

def test_packed_fp32_pass_gives_the_same_bits(tmp_path):
    """Every recorded call once more in ONE child process with VINTERP_HULL=fp32 (k_hull_mask instead of k_hull_mask_mx): every call's
    mask equals this process's bit for bit."""
    for group in GROUPS:                                          # (only what an earlier test of this run has not recorded)
        if not any(True for name, *_ in GROUPS[group]() if name not in SEEN):
            continue
        _run(group, check=False)
    out = str(tmp_path / 'fp32_masks.npz')
    env = dict(os.environ, VINTERP_HULL='fp32')
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    print('child: %.2f s\n%s' % (time.perf_counter() - t0, r.stdout))
    child = np.load(out)
    names = [str(k) for k in child['names']]
    assert names == sorted(SEEN)
    differ = []
    for i, name in enumerate(names):
        mask = SEEN[name]
        got = np.unpackbits(child['m%d' % i])[:int(child['sizes'][i])].astype(bool)
        if not np.array_equal(got, mask):
            w = np.flatnonzero(got != mask)
            differ.append('%s: %d bits differ, first at p = %s (fp32 pass says %s)' % (name, w.size, w[:8], got[w[:8]]))
    assert not differ, '\n'.join(differ[:20])


def _child(out):
    sys.path.insert(0, REPO)
    for group in GROUPS:
        _run(group, check=False)
    names = sorted(SEEN)
    np.savez(out, names=np.array(names), sizes=np.array([SEEN[k].size for k in names]),
             **{'m%d' % i: np.packbits(SEEN[k]) for i, k in enumerate(names)})


if __name__ == '__main__':
    _child(sys.argv[1])
