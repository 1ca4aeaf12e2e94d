"""Hulls with answers known by construction, and np.longdouble references, for the hull mask (k_hull_mask_mx, k_hull_mask:
csrc/vi_basis.hip) and the ray clip (slant_clip: csrc/vi_slant.hip).  No GPU here: tests/test_hull_ref_host.py checks this file
on the host, tests/test_gpu_hull_geometry.py runs the device against it.

Tangent polytopes.  For a centre c (ECEF of a geodetic point), a radius rho and F unit normals n_f the list is
eq[f] = (n_f, -(n_f . c + rho)): every facet is tangent to the sphere of radius rho about c.  The normals are a Fibonacci sphere
under a fixed random rotation, turned once more so that facet 0 points where the case wants it: 'radial' (along c, so that the
reference point of the mask pass - the foot of the origin's perpendicular on facet 0 - is the tangent point of facet 0, a point
of the hull) or 'horizontal' (at a right angle to c: the plane passes rho from the Earth's centre and the reference point lies
|c| away from the hull, as with the side facets of a radar's beam fan).  The point c + (rho + tol + sigma delta) n_f has plane
distance tol + sigma delta from facet f and (rho + tol)(n_g . n_f - 1) + sigma delta n_g . n_f + tol from every other facet g,
so with gap_f = (rho + tol) min_g (1 - n_g . n_f) and delta <= gap_f / 4 it is outside by facet f alone (sigma = +1) or inside
(sigma = -1).  The steps are STEPS metres, each capped at that quarter: without the cap the 300 m step at rho = 5 km violates
the neighbouring facets from F = 129 on.

Reference.  The device takes geodetic inputs, so a point goes through geodesy.ecef2geodetic; its ECEF is then recomputed from
the ROUNDED float64 latitude, longitude and altitude in np.longdouble, and all F plane distances are evaluated in np.longdouble.
A point enters a test only if its own facet's distance is within OWN_MARGIN of the intended tol + sigma delta and every other
facet is at least OTHER_MARGIN inside.  OTHER_MARGIN = 1e-3 m is derived, not measured: the device's ECEF and its plane distance
differ from these by a few eps |x| ~ 1e-8 m at |x| <= 2.7e7 m, five decades below the margin (the smallest step, 1e-2 m, is six
decades above that error).  No case may lose a point to the margins: `dropped` is asserted to be 0 for every case of the list.

np.longdouble is the 80-bit format on x86 (eps 1.1e-19: 3e-12 m at 2.7e7 m); where it is only a double the margins still hold,
by four decades instead of nine."""
import collections
import functools

import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps
STEPS = (1e-2, 1., 30., 300.)       # metres off the facet, each capped at a quarter of the facet's gap
OWN_MARGIN = 1e-6                   # |own facet's distance - (tol + sigma delta)| at most
OTHER_MARGIN = 1e-3                 # every other facet at least this far inside

# partial and whole tiles of 32; tile counts 1, 2, 3, 4, 5, 8, 9, 15, 33 around the early-exit points after tiles 0, 1, 3, 7, ...;
# the fp32 list's padding to 16
F_LIST = (4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256, 257, 460, 1025)
RHOS = (5e3, 2e5, 2e6)
CENTRES = {'north': (78., 262., 350e3), 'equator': (0.3, 0.2, 400e3), 'south': (-89.6, 135., 300e3),
           'gnss': (78., 262., 20200e3)}

# the prefilter's constants, restated (csrc/vi_basis.hip: HULL_BAND, HULL_MX_REL, HULL_FAR, HULL_UNIT and the fp16 range)
BAND_ABS, BAND_REL, FAR, OFFMAX_LIMIT = 4., 4e-6, 1.6e7, 65000. * 256.
# |r| < FAR and offmax <= OFFMAX_LIMIT bound the band of a judged point: a step of 300 m is always outside it, 1e-2 m inside
BAND_MAX = BAND_ABS + BAND_REL * (FAR + OFFMAX_LIMIT)

Case = collections.namedtuple('Case', 'F rho centre facet0 lon tol')
Case.__new__.__defaults__ = ('north', 'radial', 'neg', 0.)


def case_name(c):
    return 'F%d-rho%gkm-%s-%s-lon_%s-tol%g' % (c.F, c.rho / 1e3, c.centre, c.facet0, c.lon, c.tol)


def slot_cases():
    """Every facet count, at 200 km about the northern centre, facet 0 radial and horizontal."""
    return [Case(F, 2e5, 'north', f0) for F in F_LIST for f0 in ('radial', 'horizontal')]


def place_cases():
    """Three radii, three centres (the one on the Greenwich meridian with its western longitudes once negative and once
    as 360 - x), facet 0 radial and horizontal, at F = 33 (two tiles, the second with ONE facet) and 257 (nine tiles, past
    the early-exit test after tile 7); and the centre at 20 200 km, where the prefilter is off for every point."""
    out = []
    for F in (33, 257):
        for rho in RHOS:
            for centre, lon in (('north', 'neg'), ('equator', 'neg'), ('equator', 'wrap'), ('south', 'neg')):
                for f0 in ('radial', 'horizontal'):
                    out.append(Case(F, rho, centre, f0, lon))
    out.append(Case(257, 2e5, 'gnss', 'horizontal'))
    return out


def all_cases():
    return slot_cases() + place_cases() + [Case(257, 2e5, 'north', 'radial', 'neg', 500.)]


# ---- geometry ---------------------------------------------------------------------------------------------------------------------

def ecef_ld(lat, lon, alt):
    """(P, 3) np.longdouble ECEF of float64 geodetic coordinates: geodesy.geodetic2ecef, every operation in longdouble."""
    from volumetricinterp_amd.geodesy import WGS84_A, WGS84_B
    pi = LD(4) * np.arctan(LD(1))
    la, lo, h = (np.asarray(v, dtype=np.float64).astype(LD) for v in (lat, lon, alt))
    la, lo = la * pi / LD(180), lo * pi / LD(180)
    a, b = LD(WGS84_A), LD(WGS84_B)
    sl, cl = np.sin(la), np.cos(la)
    N = a * a / np.sqrt(a * a * cl * cl + b * b * sl * sl)
    return np.stack([(N + h) * cl * np.cos(lo), (N + h) * cl * np.sin(lo), (N * (b / a) ** 2 + h) * sl], axis=-1)


def fibonacci(F):
    i = np.arange(F) + 0.5
    z = 1. - 2. * i / F
    phi = i * np.pi * (3. - np.sqrt(5.))
    r = np.sqrt(1. - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def _fixed_rotation():
    q, r = np.linalg.qr(np.random.default_rng(20240611).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def _rotation_onto(u, v):
    """The rotation that takes the unit vector u to the unit vector v (Rodrigues; a half turn when they are opposite)."""
    w, c = np.cross(u, v), float(u @ v)
    if c < -1. + 1e-12:
        t = np.cross(u, [1., 0., 0.] if abs(u[0]) < 0.9 else [0., 1., 0.])
        t /= np.linalg.norm(t)
        return 2. * np.outer(t, t) - np.eye(3)
    K = np.array([[0., -w[2], w[1]], [w[2], 0., -w[0]], [-w[1], w[0], 0.]])
    return np.eye(3) + K + K @ K / (1. + c)


def centre_ecef(name):
    return np.array(ecef_ld(*CENTRES[name]), dtype=np.float64)


def normals(F, centre, facet0):
    """(F, 3) unit normals (to a rounding), facet 0 along the centre ('radial') or at a right angle to it ('horizontal')."""
    n = fibonacci(F) @ _fixed_rotation().T
    up = centre / np.linalg.norm(centre)
    if facet0 == 'radial':
        want = up
    else:
        assert facet0 == 'horizontal'
        want = np.cross(up, [0., 0., 1.] if abs(up[2]) < 0.9 else [1., 0., 0.])
        want /= np.linalg.norm(want)
    n = n @ _rotation_onto(n[0], want).T
    n /= np.linalg.norm(n, axis=1)[:, None]
    assert abs(n[0] @ want - 1.) < 1e-12
    return np.ascontiguousarray(n)


def gaps(n, rho):
    """gap_f = rho min_{g != f} (1 - n_g . n_f), (F,)."""
    G = n @ n.T
    np.fill_diagonal(G, -1.)
    return rho * (1. - G.max(axis=1))


def equations(n, c, rho):
    """(F, 4) float64: eq[f] = (n_f, -(n_f . c + rho)), the offset formed in longdouble and rounded once."""
    d = -((n.astype(LD) * c.astype(LD)).sum(axis=1) + LD(rho))
    return np.ascontiguousarray(np.concatenate([n, np.array(d, dtype=np.float64)[:, None]], axis=1))


def distances_ld(eq, X, facet, group=None, chunk=1024):
    """(own, other), np.longdouble (P,): the plane distance of the longdouble points X (P, 3) from their own facet `facet[p]` of
    the float64 list eq - with `group` (F,): the largest and, as a third value, the smallest over the facets of its group - and
    the largest distance from every other facet (every facet outside the group); -inf where there is no other."""
    e = eq.astype(LD)
    F = len(eq)
    grp = np.arange(F) if group is None else np.asarray(group)
    own, low, other = np.empty(len(X), dtype=LD), np.empty(len(X), dtype=LD), np.empty(len(X), dtype=LD)
    for i in range(0, len(X), chunk):
        x = X[i:i + chunk]
        d = x[:, 0, None] * e[None, :, 0] + x[:, 1, None] * e[None, :, 1] + x[:, 2, None] * e[None, :, 2] + e[None, :, 3]
        mine = grp[None, :] == grp[facet[i:i + chunk]][:, None]
        own[i:i + chunk] = np.where(mine, d, -np.inf).max(axis=1)
        low[i:i + chunk] = np.where(mine, d, np.inf).min(axis=1)
        other[i:i + chunk] = np.where(mine, -np.inf, d).max(axis=1)
    return (own, other) if group is None else (own, other, low)


def classify(eq, tol, X, dmax):
    """The prefilter's view of the points, restated from its constants: (off, inband, outband) boolean (P,).  X: ECEF (P, 3),
    dmax: the largest plane distance of each point.  off: not judged by the fp16 products (list unusable - offset beyond the
    fp16 range - or the point further than FAR from the reference point c0); inband: judged and within the band
    s (4 + 4e-6 (r + offmax)) of tol, so that the fp64 test decides; outband: decided by the fp16 products alone.  A property
    of the inputs, used to show which path a case takes; the device's own fp32 arithmetic may differ in the last digits."""
    e = np.asarray(eq, dtype=np.float64)
    c0 = -e[0, 3] * e[0, :3]
    s = max(1., float(np.sqrt((e[:, :3] ** 2).sum(axis=1).max())))
    offmax = float(np.abs(e[:, :3] @ c0 + e[:, 3]).max()) / s
    r = np.linalg.norm(np.asarray(X, dtype=np.float64) - c0, axis=1)
    usable = np.isfinite(offmax) and offmax <= OFFMAX_LIMIT
    off = np.full(len(r), True) if not usable else ~(r < FAR)
    band = s * (BAND_ABS + BAND_REL * (r + (offmax if usable else 0.)))
    inband = ~off & (np.abs(np.asarray(dmax, dtype=np.float64) - tol) <= band)
    return off, inband, ~off & ~inband


# ---- the mask cases ---------------------------------------------------------------------------------------------------------------

Built = collections.namedtuple('Built', 'case eq tol lat lon alt expect facet step delta sigma own other dropped off inband outband')


@functools.lru_cache(maxsize=None)
def build(case):
    """The points of a case in facet order - p = 8 f + 2 k + i: facet f, step k of STEPS, sigma = (+1, -1)[i] - with the
    expected mask (sigma < 0) decided in longdouble.  Arrays are read-only: the cases are shared by the tests."""
    from volumetricinterp_amd import geodesy
    c = centre_ecef(case.centre)
    n = normals(case.F, c, case.facet0)
    eq = equations(n, c, case.rho)
    gap = gaps(n, case.rho + case.tol)
    K = len(STEPS)
    facet = np.repeat(np.arange(case.F), 2 * K)
    step = np.tile(np.repeat(np.arange(K), 2), case.F)
    sigma = np.tile(np.array([1., -1.]), K * case.F)
    delta = np.minimum(np.array(STEPS)[step], gap[facet] / 4.)
    X = c.astype(LD)[None, :] + (LD(case.rho + case.tol) + (sigma * delta).astype(LD))[:, None] * n[facet].astype(LD)
    lat, lon, alt = geodesy.ecef2geodetic(*(np.array(X[:, j], dtype=np.float64) for j in range(3)))
    if case.lon == 'wrap':
        lon = np.where(lon < 0., 360. - (-lon), lon)              # 360 - x for the western longitudes
    else:
        assert case.lon == 'neg'
    Xr = ecef_ld(lat, lon, alt)
    own, other = distances_ld(eq, Xr, facet)
    ok = (np.abs(own - (LD(case.tol) + (sigma * delta).astype(LD))) <= OWN_MARGIN) & (other <= LD(case.tol) - LD(OTHER_MARGIN))
    off, inband, outband = classify(eq, case.tol, np.array(Xr, dtype=np.float64), np.maximum(own, other))
    out = Built(case, eq, case.tol, lat, lon, alt, sigma < 0., facet, step, delta, sigma, own, other, int((~ok).sum()),
                off, inband, outband)
    for v in out:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def far_outside(case, factor=3.):
    """(lat, lon, alt) of one point far outside the hull of `case` by facet 0 - and so decided by tile 0 -: c + factor rho n_0;
    with its largest plane distance and the largest of the others, for the margins."""
    from volumetricinterp_amd import geodesy
    b = build(case)
    c = centre_ecef(case.centre)
    x = c + factor * (case.rho + case.tol) * b.eq[0, :3]
    lat, lon, alt = (np.atleast_1d(v) for v in geodesy.ecef2geodetic(*x))
    own, other = distances_ld(b.eq, ecef_ld(lat, lon, alt), np.zeros(1, dtype=np.int64))
    assert own[0] > case.tol + 0.5 * case.rho
    return float(lat[0]), float(lon[0]), float(alt[0])


def deep_inside(case):
    """(lat, lon, alt) of the centre of the hull of `case`: rho inside every facet."""
    from volumetricinterp_amd import geodesy
    c = centre_ecef(case.centre)
    lat, lon, alt = (np.atleast_1d(v) for v in geodesy.ecef2geodetic(*c))
    b = build(case)
    own, other = distances_ld(b.eq, ecef_ld(lat, lon, alt), np.zeros(1, dtype=np.int64))
    assert max(own[0], other[0]) < case.tol - 0.5 * case.rho
    return float(lat[0]), float(lon[0]), float(alt[0])


def describe(b, idx, pos, limit=12):
    """Failing points in the terms of the kernel: point idx[j] of the case sat at position pos[j] of the call - the facet, its
    tile and slot, the step, the side, and p // 256, p % 64 of the position."""
    lines = ['%s F=%d: %d wrong' % (case_name(b.case), b.case.F, len(idx))]
    for i, q in list(zip(idx, pos))[:limit]:
        lines.append('  facet %d (tile %d, slot %d) delta %g sigma %+d at p = %d (p // 256 = %d, p %% 64 = %d): expected %s'
                     % (b.facet[i], b.facet[i] // 32, b.facet[i] % 32, b.delta[i], b.sigma[i], q, q // 256, q % 64,
                        'inside' if b.expect[i] else 'outside'))
    return '\n'.join(lines)


# ---- Qhull hulls ------------------------------------------------------------------------------------------------------------------

Qh = collections.namedtuple('Qh', 'eq group lat lon alt expect facet delta sigma dropped vlat vlon valt vdist')


def qhull_case(hull_vert, tol):
    """Points off the facets of the convex hull of `hull_vert` (ECEF, (V, 3)): centroid of every triangle +- delta along its
    normal, delta of STEPS capped at a quarter of the centroid's depth below the nearest facet of another plane.  Coplanar
    triangles (a box's faces) form a group: a point off one of them is off its twin too, and 'alone' means the group.  Also the
    hull's own vertices in geodetic coordinates with their largest longdouble plane distance `vdist`."""
    from scipy.spatial import ConvexHull
    from volumetricinterp_amd import geodesy
    hv = np.ascontiguousarray(hull_vert, dtype=np.float64)
    h = ConvexHull(hv)
    eq = np.ascontiguousarray(h.equations, dtype=np.float64)
    F = len(eq)
    same = (eq[:, :3] @ eq[:, :3].T > 1. - 1e-12) & (np.abs(eq[:, None, 3] - eq[None, :, 3]) < 1e-6)
    group = np.array([int(np.flatnonzero(same[f])[0]) for f in range(F)])
    cen = hv[h.simplices].mean(axis=1)
    depth = -(cen @ eq[:, :3].T + eq[:, 3])                     # (facet's centroid, facet): positive inside
    depth[group[:, None] == group[None, :]] = np.inf
    gap = depth.min(axis=1)
    K = len(STEPS)
    facet = np.repeat(np.arange(F), 2 * K)
    sigma = np.tile(np.array([1., -1.]), K * F)
    delta = np.minimum(np.tile(np.repeat(np.array(STEPS), 2), F), gap[facet] / 4.)
    X = cen[facet].astype(LD) + (LD(tol) + (sigma * delta).astype(LD))[:, None] * eq[facet, :3].astype(LD)
    lat, lon, alt = geodesy.ecef2geodetic(*(np.array(X[:, j], dtype=np.float64) for j in range(3)))
    own, other, low = distances_ld(eq, ecef_ld(lat, lon, alt), facet, group)
    want = LD(tol) + (sigma * delta).astype(LD)
    ok = (np.abs(own - want) <= OWN_MARGIN) & (np.abs(low - want) <= OWN_MARGIN) & (other <= LD(tol) - LD(OTHER_MARGIN))
    vlat, vlon, valt = geodesy.ecef2geodetic(hv[:, 0], hv[:, 1], hv[:, 2])
    vo, vr = distances_ld(eq, ecef_ld(vlat, vlon, valt), np.zeros(len(hv), dtype=np.int64))
    return Qh(eq, group, lat, lon, alt, sigma < 0., facet, delta, sigma, int((~ok).sum()), vlat, vlon, valt,
              np.maximum(vo, vr))


def box_vertices():
    """The 8 corners of a box of 300 x 200 x 400 km at 350 km over 78 N 262 E, axes east, north, up there: Qhull makes 12
    triangles of it, coplanar in pairs."""
    c = centre_ecef('north')
    up = c / np.linalg.norm(c)
    east = np.cross([0., 0., 1.], up)
    east /= np.linalg.norm(east)
    north = np.cross(up, east)
    s = np.array([[i, j, k] for i in (-1., 1.) for j in (-1., 1.) for k in (-1., 1.)])
    return c + s[:, :1] * 150e3 * east + s[:, 1:2] * 100e3 * north + s[:, 2:] * 200e3 * up


# ---- rays -------------------------------------------------------------------------------------------------------------------------

def clip_ld(eq, tol, a, b, chunk=1024):
    """(s0, s1, lo_facet, hi_facet): the interval of s in [0, 1] on which every n_f . (a + s (b - a)) + d_f <= tol, in
    np.longdouble from the float64 list and end points - the definition, facet by facet: the distance is linear in s, g(s) =
    ga + s (gb - ga), so a rising facet allows s <= (tol - ga) / (gb - ga), a falling one s >= the same quotient, a level one
    every s or none.  (nan, nan) where fewer than two points remain (not s0 < s1) or an end point is not finite.  Also the
    facets that bind the two ends (-1: the end of the segment itself)."""
    e = np.asarray(eq, dtype=np.float64).astype(LD)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    P = len(a)
    s0, s1 = np.zeros(P, dtype=LD), np.ones(P, dtype=LD)
    f0, f1 = np.full(P, -1), np.full(P, -1)
    t = LD(tol)
    for i in range(0, P, chunk):
        al, bl = a[i:i + chunk].astype(LD), b[i:i + chunk].astype(LD)
        ga = al[:, 0, None] * e[None, :, 0] + al[:, 1, None] * e[None, :, 1] + al[:, 2, None] * e[None, :, 2] + e[None, :, 3]
        gb = bl[:, 0, None] * e[None, :, 0] + bl[:, 1, None] * e[None, :, 1] + bl[:, 2, None] * e[None, :, 2] + e[None, :, 3]
        m = gb - ga
        with np.errstate(divide='ignore', invalid='ignore'):
            q = (t - ga) / m
        upper = np.where(m > 0, q, np.where((m == 0) & (ga > t), -np.inf, np.inf))
        lower = np.where(m < 0, q, np.where((m == 0) & (ga > t), np.inf, -np.inf))
        hi, lo = upper.min(axis=1), lower.max(axis=1)
        k = slice(i, i + len(al))
        f1[k] = np.where(hi < 1, upper.argmin(axis=1), -1)
        f0[k] = np.where(lo > 0, lower.argmax(axis=1), -1)
        s1[k], s0[k] = np.minimum(hi, 1), np.maximum(lo, 0)
    bad = ~(s0 < s1) | ~(np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1))
    s0[bad] = np.nan
    s1[bad] = np.nan
    return s0, s1, f0, f1


Rays = collections.namedtuple('Rays', 'eq tol a b kind facet delta s0 s1 dropped')
OUTWARD, INWARD, OFF_PLANE, UNDER_PLANE = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def ray_set(F, rho=2e5, centre='north'):
    """Rays with known chords through the tangent polytope of F facets (facet 0 radial, tol = 0), ECEF end points.  Per facet f,
    in this order: OUTWARD c -> c + 2 rho n_f (s0 = 0 exactly, the upper end bound by f alone, met at a right angle); INWARD,
    its reverse (s1 = 1 exactly); then for each step delta (capped as for the mask): OFF_PLANE, a short ray in the plane at
    rho + delta from c, both ends outside by f alone (no chord); UNDER_PLANE, the same at rho - delta (the whole segment).
    The ends are decided in longdouble with the margins of the mask cases; s0, s1 are clip_ld's."""
    c = centre_ecef(centre)
    n = normals(F, c, 'radial')
    eq = equations(n, c, rho)
    gap = gaps(n, rho)
    a, b, kind, facet, delta = [], [], [], [], []
    for f in range(F):
        e = np.eye(3)[int(np.argmin(np.abs(n[f])))]
        t = np.cross(n[f], e)
        t /= np.linalg.norm(t)
        far = c + 2. * rho * n[f]
        rows = [(c, far, OUTWARD, 0.), (far, c, INWARD, 0.)]
        for st in STEPS:
            d = min(st, gap[f] / 4.)
            for sg, kd in ((1., OFF_PLANE), (-1., UNDER_PLANE)):
                mid = c + (rho + sg * d) * n[f]
                rows.append((mid - gap[f] / 4. * t, mid + gap[f] / 4. * t, kd, d))
        for r in rows:
            a.append(r[0]); b.append(r[1]); kind.append(r[2]); facet.append(f); delta.append(r[3])
    a, b = np.ascontiguousarray(np.array(a)), np.ascontiguousarray(np.array(b))
    kind, facet, delta = np.array(kind), np.array(facet), np.array(delta)
    s0, s1, f0, f1 = clip_ld(eq, 0., a, b)
    oa, xa = distances_ld(eq, a.astype(LD), facet)
    ob, xb = distances_ld(eq, b.astype(LD), facet)
    m = LD(OTHER_MARGIN)
    ok = np.zeros(len(a), dtype=bool)
    k = kind == OUTWARD
    ok[k] = (np.maximum(oa, xa)[k] <= -m) & (ob[k] >= m) & (s0[k] == 0) & (f1[k] == facet[k]) & (s1[k] < 1)
    k = kind == INWARD
    ok[k] = (np.maximum(ob, xb)[k] <= -m) & (oa[k] >= m) & (s1[k] == 1) & (f0[k] == facet[k]) & (s0[k] > 0)
    k = kind == OFF_PLANE
    ok[k] = ((np.abs(oa - delta)[k] <= OWN_MARGIN) & (np.abs(ob - delta)[k] <= OWN_MARGIN) & (np.maximum(xa, xb)[k] <= -m)
             & np.isnan(s0[k]))
    k = kind == UNDER_PLANE
    ok[k] = ((np.abs(oa + delta)[k] <= OWN_MARGIN) & (np.abs(ob + delta)[k] <= OWN_MARGIN) & (np.maximum(xa, xb)[k] <= -m)
             & (s0[k] == 0) & (s1[k] == 1))
    out = Rays(eq, 0., a, b, kind, facet, delta, s0, s1, int((~ok).sum()))
    for v in out:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def check_chords(r, e0, e1, rays=slice(None), length=None):
    """Asserts the chord ends (e0, e1) of the rays `rays` of the set r - fractions of the segment, or with `length` (the |b - a|
    they were multiplied with) metres from a: the NaN pattern is the longdouble clip's, the ends that are 0 and the whole
    segment by construction are exactly so, a clipped end is within 64 eps (|a| + |b|) metres of the longdouble one.  Returns
    the largest ratio of a clipped end's error to that bound."""
    a, b, kind = r.a[rays], r.b[rays], r.kind[rays]
    w0, w1 = r.s0[rays], r.s1[rays]
    nan = np.array(np.isnan(w0))
    assert np.array_equal(np.isnan(e0), nan) and np.array_equal(np.isnan(e1), nan), np.flatnonzero(np.isnan(e0) != nan)[:10]
    assert np.array_equal(nan, kind == OFF_PLANE)
    whole = np.ones(len(a)) if length is None else length
    metres = np.linalg.norm(b - a, axis=1) if length is None else np.ones(len(a))
    k = (kind == OUTWARD) | (kind == UNDER_PLANE)
    assert np.array_equal(e0[k], np.zeros(k.sum())), ('s0 != 0', np.flatnonzero(k)[e0[k] != 0][:10])
    k = (kind == INWARD) | (kind == UNDER_PLANE)
    assert np.array_equal(e1[k], whole[k]), ('s1 != 1', np.flatnonzero(k)[e1[k] != whole[k]][:10])
    bound = 64. * EPS * (np.linalg.norm(a, axis=1) + np.linalg.norm(b, axis=1))
    ratio = 0.
    for got, want, k in ((e1, w1, kind == OUTWARD), (e0, w0, kind == INWARD)):
        if k.any():
            err = np.abs(np.array(got[k].astype(LD) - want[k] * whole[k].astype(LD), dtype=np.float64)) * metres[k]
            ratio = max(ratio, float((err / bound[k]).max()))
            assert np.all(err <= bound[k]), ('facets', r.facet[rays][k][err > bound[k]][:10], float((err / bound[k]).max()))
    return ratio


QHULL_NAMES = ('box', 'beams_3x20', 'beams_11x50')


def qhull_input(name):
    """(hull vertices, tol) of a Qhull case: the box, or the hull of a synth.beams geometry as the fit stores it."""
    from scipy.spatial import ConvexHull
    from volumetricinterp_amd import synth
    from volumetricinterp_amd.estimate import hull_equations
    from volumetricinterp_amd.geodesy import geodetic2ecef
    if name == 'box':
        hv = box_vertices()
    else:
        nb, nr = {'beams_3x20': (3, 20), 'beams_11x50': synth.GEOM_C1}[name]
        R = np.array(geodetic2ecef(*synth.beams(nb, nr, seed=0))).T
        hv = R[ConvexHull(R).vertices]
    return hv, hull_equations(hv)[1]
