"""Evaluate a fitted model at arbitrary geodetic points on the MI355X.

Drop-in mirror of the reference class ``volumetricinterp/estimate.py:13-221``:
same constructor, same ``__call__`` signature and error behaviour, same
``get_C`` time selection.  ``__call__`` runs the fused HIP kernel
(``vi_eval_f64``: coordinates -> basis -> contraction with C -> hull mask)
instead of materialising ``A`` (1 152 B per point at N = 144) and calling
``einsum`` (estimate.py:113-115); the per-point Qhull of ``check_hull``
(estimate.py:153-178) becomes one host Qhull plus a half-space test fused in
the kernel.
"""
import collections
import configparser
import datetime as dt
import importlib
import io

import numpy as np
from scipy.spatial import ConvexHull

from . import _lib
from . import geodesy


def hull_equations(hull_vert):
    """Facet half-spaces (F, 4) of the data hull: inside <=> eq[:, :3] @ x + eq[:, 3] <= tol."""
    hull_vert = np.ascontiguousarray(hull_vert, dtype=np.float64)
    eq = np.ascontiguousarray(ConvexHull(hull_vert).equations, dtype=np.float64)
    # Qhull treats a point within its distance round-off of a facet as coplanar (not a new vertex),
    # which the reference's vertex-list comparison (estimate.py:174-176) then reports as inside.
    tol = 4. * np.finfo(np.float64).eps * 3. * float(np.max(np.abs(hull_vert)))
    return order_facets(eq, hull_vert), tol


def order_facets(eq, hull_vert, nsample=4096, nlead=32):
    """The same half-spaces, the most telling ones first.  The mask pass (k_hull_mask) takes the maximum over all facets - the
    order cannot change a result - but leaves as soon as every point of a wave has been found outside by SOME facet: with
    Qhull's order an outside point met its first violated facet late.  Greedy cover on a sample of the vertices' bounding
    box: the facet that rejects most sample points first, then the one that rejects most of the rest, ... (nlead of them);
    the others keep their order."""
    if len(eq) <= nlead:
        return eq
    lo, hi = hull_vert.min(axis=0), hull_vert.max(axis=0)
    pts = lo + (hi - lo) * np.random.default_rng(0).random((nsample, 3))
    out = (pts @ eq[:, :3].T + eq[:, 3]) > 0.                     # (sample, facet): the facet puts the point outside
    left = out.any(axis=1)
    lead = []
    for _ in range(nlead):
        if not left.any():
            break
        gain = out[left].sum(axis=0)
        gain[lead] = -1
        f = int(np.argmax(gain))
        if gain[f] <= 0:
            break
        lead.append(f)
        left &= ~out[:, f]
    rest = np.setdiff1d(np.arange(len(eq)), lead)
    return np.ascontiguousarray(eq[np.concatenate([np.array(lead, dtype=np.int64), rest])])


def ravel_points(gdlat, gdlon, gdalt):
    """The coordinates of the points as three contiguous 1-D float64 arrays of one size."""
    lat, lon, alt = (np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel()) for a in (gdlat, gdlon, gdalt))
    if not (lat.size == lon.size == alt.size):
        raise ValueError('gdlat, gdlon, gdalt must have the same shape')
    return lat, lon, alt


OUT_OF_RANGE = 'Requested time out of range of data file.'        # estimate.py:219


def unix_seconds(times):
    """float64 unix seconds of naive-UTC datetimes (the expression of get_C, estimate.py:196) or of numbers, shape kept."""
    a = np.asarray(times)
    if a.dtype != object:
        return a.astype(np.float64)
    epoch = dt.datetime(1970, 1, 1)
    flat = [(t - epoch).total_seconds() for t in a.ravel()]
    return np.array(flat, dtype=np.float64).reshape(a.shape)


def _select_literal(mt, t0, timetol, timeinterp, rec, ok, idx):
    """select_records for the elements idx of the raveled t0 by the literal rule of get_C, a slab of elements at a time."""
    slab = max(1, (1 << 20) // max(1, mt.size))
    for s in range(0, idx.size, slab):
        k = idx[s:s + slab]
        t = t0[k][:, None]
        if timeinterp:
            hit = (t >= mt[None, :-1]) & (t < mt[None, 1:])             # estimate.py:204
            rec[k] = np.argmax(hit, axis=1) if hit.shape[1] else 0      # the first i
            ok[k] = hit.any(axis=1)
        else:
            d = np.abs(mt[None, :] - t)                                 # estimate.py:212
            i = np.argmin(d, axis=1)                                    # the first minimum
            rec[k] = i
            ok[k] = ~(d[np.arange(k.size), i] > timetol)                # estimate.py:213


def select_records(time, t0, timetol=60., timeinterp=False, outside='raise'):
    """The record Estimate.get_C (estimate.py:180-221) selects, for every element of t0 at once.

    time: the (R, 2) /UnixTime array; t0: float64 unix seconds of any shape.  Returns (rec, w): rec int32 of the shape of t0 and
    w float64 of that shape, or None without timeinterp.  Nearest mode: rec = argmin |mt - t0| over the record mid-times mt
    (the first minimum), out of range where that distance exceeds timetol.  With timeinterp: rec = the first i with
    mt[i] <= t0 < mt[i+1] and w = (t0 - mt[i]) / (mt[i+1] - mt[i]), so that (1 - w) * Coeffs[rec] + w * Coeffs[rec + 1] is
    get_C's row bit for bit; out of range where no such i exists (t0 == mt[-1] included, as in the reference).  Any `time`
    array: mid-times that repeat or do not increase take the literal rule, strictly increasing ones a binary search.
    outside='raise': ValueError with the reference's message if any element is out of range; 'nan': rec = -1 (and w = 0) there."""
    if outside not in ('raise', 'nan'):
        raise ValueError("outside must be 'raise' or 'nan', not %r" % (outside,))
    mt = np.mean(np.asarray(time), axis=1)
    t0 = np.asarray(t0, dtype=np.float64)
    shape = t0.shape
    t0 = t0.ravel()
    R = mt.size
    rec = np.zeros(t0.size, dtype=np.int64)
    ok = np.zeros(t0.size, dtype=bool)
    if R == 0:
        pass                                            # no record: every time is out of range
    elif R > 1 and np.all(mt[1:] > mt[:-1]):
        hi = np.searchsorted(mt, t0, side='right')      # mt[hi - 1] <= t0 < mt[hi]; NaN sorts past the end
        if timeinterp:
            rec[:] = hi - 1
            ok[:] = (hi >= 1) & (hi <= R - 1)
            rec[~ok] = 0
        else:
            # the nearest of the two neighbours, the lower one on a tie; the distances |mt - t0| as get_C forms them do not
            # decrease away from t0, so that one is the first minimum unless the record below it ties with it in floating
            # point (or t0 is NaN): those elements take the literal rule
            a, b = np.clip(hi - 1, 0, R - 1), np.clip(hi, 0, R - 1)
            da, db = np.abs(mt[a] - t0), np.abs(mt[b] - t0)
            rec[:] = np.where(da <= db, a, b)
            d = np.abs(mt[rec] - t0)
            ok[:] = ~(d > timetol)
            below = np.abs(mt[np.maximum(rec - 1, 0)] - t0)
            sure = (d == d) & ((rec == 0) | (below > d))
            _select_literal(mt, t0, timetol, timeinterp, rec, ok, np.flatnonzero(~sure))
    else:
        _select_literal(mt, t0, timetol, timeinterp, rec, ok, np.arange(t0.size))
    if not ok.all():
        if outside == 'raise':
            raise ValueError(OUT_OF_RANGE)
        rec[~ok] = -1
    w = None
    if timeinterp:
        w = np.zeros(t0.size)
        i = rec[ok]
        w[ok] = (t0[ok] - mt[i]) / (mt[i + 1] - mt[i])                # estimate.py:206
        w = w.reshape(shape)
    return rec.astype(np.int32).reshape(shape), w


def used_records(rec, w, R):
    """(rows, rec_compact): the records a call of track_error / slant_error has to upload, and the (rec, w) of select_records
    re-indexed into them.  rows: the sorted distinct records below R that the elements need - rec itself, with `w` given rec + 1
    too.  rec_compact: int32 of the shape of rec, the position of rec in rows, -1 kept as -1; a pair (r, r + 1) stays adjacent,
    r + 1 being in rows whenever r is and directly after it, and a needed row >= R keeps pointing at a row >= len(rows), which
    the library answers with NaN as it does in the full stack."""
    rec = np.asarray(rec)
    r = rec.ravel().astype(np.int64)
    ok = r >= 0
    need = r[ok] if w is None else np.concatenate([r[ok], r[ok] + 1])
    rows = np.unique(need[need < R])
    compact = np.full(r.size, -1, dtype=np.int64)
    pos = np.searchsorted(rows, r[ok])
    pos[r[ok] >= R] = rows.size
    compact[ok] = pos
    return rows, compact.astype(np.int32).reshape(rec.shape)


def hull_chords(eq, tol, a, b):
    """(s0, s1), each (P,): the part [s0, s1] of [0, 1] on which the segment a + s (b - a) lies inside the hull of
    hull_equations - inside <=> eq[:, :3] @ x + eq[:, 3] <= tol - for (P, 3) end points in ECEF metres.  The hull is convex, so
    that part is one interval: with the plane distances ga, gb of the two ends, a facet with both ends inside does not bound
    the segment, one with both ends outside is missed by the whole segment, every other facet bounds s from below at
    (ga - tol) / (ga - gb) or from above at (tol - ga) / (gb - ga).  Two end points inside give (0, 1) exactly.  (NaN, NaN)
    for a miss (not s0 < s1) and for non-finite end points.  The host statement of the clip in K2l (vi_eval_slant_f64)."""
    eq = np.asarray(eq, dtype=np.float64).reshape(-1, 4)
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape != b.shape:
        raise ValueError('a and b must both have shape (P, 3)')
    P = a.shape[0]
    s0, s1 = np.zeros(P), np.ones(P)
    miss = ~(np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1))
    slab = max(1, (1 << 20) // max(1, eq.shape[0]))
    with np.errstate(invalid='ignore', divide='ignore'):
        for i in range(0, P if eq.shape[0] else 0, slab):
            k = slice(i, i + slab)
            ga = a[k] @ eq[:, :3].T + eq[:, 3]
            gb = b[k] @ eq[:, :3].T + eq[:, 3]
            ina, inb = ga <= tol, gb <= tol
            miss[k] |= (~ina & ~inb).any(axis=1)
            enter, leave = ~ina & inb, ina & ~inb
            s0[k] = np.maximum(s0[k], np.where(enter, (ga - tol) / (ga - gb), 0.).max(axis=1))
            s1[k] = np.minimum(s1[k], np.where(leave, (tol - ga) / (gb - ga), 1.).min(axis=1))
    miss |= ~(s0 < s1)
    s0[miss] = np.nan
    s1[miss] = np.nan
    return s0, s1


SLANT_COORDS = ('geodetic', 'ecef')
SLANT_MAX_NODES = 256                              # Gauss-Legendre nodes Estimate.slant makes itself
SLANT_MAX_RULE = 65536                             # nodes of a caller's rule


def slant_rule(nodes=64, rule=None):
    """(x, w), contiguous float64: the quadrature rule of Estimate.slant on [-1, 1] - the caller's `rule`, else Gauss-Legendre
    of `nodes` nodes."""
    if rule is None:
        if isinstance(nodes, bool) or not isinstance(nodes, (int, np.integer)) or not 1 <= nodes <= SLANT_MAX_NODES:
            raise ValueError('nodes must be an integer from 1 to %d, not %r' % (SLANT_MAX_NODES, nodes))
        x, w = np.polynomial.legendre.leggauss(int(nodes))
    else:
        try:
            x, w = rule
            x, w = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError('rule must be a pair (x, w) of 1-D arrays of numbers')
        if x.ndim != 1 or w.ndim != 1 or x.size != w.size or not 1 <= x.size <= SLANT_MAX_RULE:
            raise ValueError('rule must be a pair (x, w) of 1-D arrays of one length from 1 to %d' % SLANT_MAX_RULE)
        if not (np.isfinite(x).all() and np.isfinite(w).all()):
            raise ValueError('rule must be finite')
    return np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)


def slant_rays(start, end, nodes=64, rule=None, coords='geodetic'):
    """(x, w, shape, a, b): what Estimate.slant and Estimate.resident_rays make of their ray arguments - the rule of slant_rule,
    the ray shape (the broadcast shape of the six arrays of `start` and `end`) and the end points in ECEF metres, planar
    (3, P) each, P the number of rays."""
    if coords not in SLANT_COORDS:
        raise ValueError("coords must be 'geodetic' or 'ecef', not %r" % (coords,))
    x, wq = slant_rule(nodes, rule)
    try:
        if len(start) != 3 or len(end) != 3:
            raise TypeError
        ends = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in tuple(start) + tuple(end)))
    except TypeError:
        raise ValueError('start and end must each be a triple of arrays')
    except ValueError:
        raise ValueError('the arrays of start and end do not broadcast against each other')
    shape = ends[0].shape
    ends = [np.ascontiguousarray(v).ravel() for v in ends]
    if coords == 'geodetic':
        ends = geodesy.geodetic2ecef(*ends[:3]) + geodesy.geodetic2ecef(*ends[3:])
    a, b = np.array(ends[:3]), np.array(ends[3:])       # planar (3, P)
    return x, wq, shape, a, b


def _check_out(out, shape, dtype=np.float64):
    """`out`, checked, or a new array: what every entry with an `out` argument writes into."""
    if out is None:
        return np.empty(shape, dtype=dtype)
    if not isinstance(out, np.ndarray) or out.shape != tuple(shape) or out.dtype != dtype or not out.flags.c_contiguous:
        raise ValueError('out must be a C-contiguous %s array of shape (%s)'
                         % (np.dtype(dtype).name, ', '.join('%d' % n for n in shape)))
    return out


def _ptr(a):
    """The device pointer of an optional argument of a library call."""
    return None if a is None else a.ptr


GRADIENT_FRAMES = {'model': _lib.VI_FRAME_MODEL, 'enu': _lib.VI_FRAME_ENU}
PEAK_KINDS = {'max': 0, 'min': 1}                 # vi_eval_resident_peak_f64's kind
REDUCED_BASES = 8                                  # reduced bases a ResidentGrid keeps (evaluate_integrals), oldest out
# the six distinct entries (c, d) of a gradient covariance in the packed order of vi_eval_resident_gradcov_f64
GRADCOV_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def gradcov_matrix(packed):
    """The symmetric 3 x 3 matrices of packed gradient covariances: (..., 6, Q-like) - the six entries in the order of
    GRADCOV_PAIRS on axis -2 - to (...) + (Q-like) + (3, 3), on the host."""
    packed = np.asarray(packed, dtype=np.float64)
    if packed.ndim < 2 or packed.shape[-2] != 6:
        raise ValueError('packed gradient covariances must have shape (..., 6, Q), not %r' % (packed.shape,))
    cov = np.empty(packed.shape[:-2] + packed.shape[-1:] + (3, 3))
    for k, (c, d) in enumerate(GRADCOV_PAIRS):
        cov[..., c, d] = cov[..., d, c] = packed[..., k, :]
    return cov


def _grid_columns(shape, axis):
    """A C-ordered grid of `shape` as (outer, L, inner) about `axis`: point q = (o * L + l) * inner + i, column
    m = o * inner + i.  Returns (axis, outer, L, inner), the axis counted from the front."""
    nd = len(shape)
    if nd == 0:
        raise ValueError('a 0-d grid has no axis to reduce')
    if not isinstance(axis, (int, np.integer)) or isinstance(axis, bool) or not -nd <= axis < nd:
        raise ValueError('axis must be an integer in [%d, %d), not %r' % (-nd, nd, axis))
    axis = int(axis) % nd
    outer = int(np.prod(shape[:axis], dtype=np.int64))
    inner = int(np.prod(shape[axis + 1:], dtype=np.int64))
    return axis, outer, int(shape[axis]), inner


def column_points(shape, axis, index):
    """The flat index (C order) of the point at position index[t, m] along `axis` in column m of a grid of `shape`, the
    columns in C order of the remaining axes as ResidentGrid.peak numbers them: (T, M) int64, -1 where index is -1 (a column
    without a peak).  index: (T, M) integers in [-1, L), L the length of the axis; anything else raises ValueError.  On the
    host; np.take_along_axis(volume.reshape(T, -1), column_points(...), 1) picks the selected values where index >= 0."""
    shape = tuple(int(n) for n in shape)
    axis, outer, L, inner = _grid_columns(shape, axis)
    index = np.asarray(index)
    if index.dtype.kind not in 'iu':
        raise ValueError('index must be an integer array, not %s' % index.dtype)
    M = outer * inner
    if index.ndim != 2 or index.shape[1] != M:
        raise ValueError('index must have shape (T, %d), not %r' % (M, index.shape))
    index = index.astype(np.int64)
    if index.size and (index.min() < -1 or index.max() >= L):
        raise ValueError('index must lie in [-1, %d)' % L)
    o, i = np.divmod(np.arange(M, dtype=np.int64), max(inner, 1))
    return np.where(index < 0, -1, (o * L + index) * inner + i)


PEAK_HEIGHT_KINDS = {'max': 1, 'min': -1}         # vi_eval_peak_f64's kind
PEAK_HEIGHT_FIELDS = ('height', 'value', 'slope', 'curvature', 'status', 'iterations')
PeakHeight = collections.namedtuple('PeakHeight', PEAK_HEIGHT_FIELDS)
PeakHeightError = collections.namedtuple('PeakHeightError', PEAK_HEIGHT_FIELDS + ('height_error', 'value_error'))


def peak_brackets(alt_axis, index):
    """(start, lo, hi) for Estimate.peak_height from the altitude axis of a grid and the index map of ResidentGrid.peak: the
    grid altitude at `index` and the altitudes of its two neighbours on the axis - the lower and the higher of them, the sample
    itself where it is the first or the last of the axis -, NaN where index is -1 (a column without a peak; peak_height gives
    such a column status 3).  alt_axis: 1-D, finite, at least one sample; index: integers in [-1, len(alt_axis)) of any shape.
    Three float64 arrays of the shape of index.  On the host."""
    alt = np.asarray(alt_axis, dtype=np.float64)
    if alt.ndim != 1 or alt.size == 0 or not np.isfinite(alt).all():
        raise ValueError('alt_axis must be a 1-D array of finite altitudes with at least one sample')
    index = np.asarray(index)
    if index.dtype.kind not in 'iu':
        raise ValueError('index must be an integer array, not %s' % index.dtype)
    index = index.astype(np.int64)
    L = alt.size
    if index.size and (index.min() < -1 or index.max() >= L):
        raise ValueError('index must lie in [-1, %d)' % L)
    none = index < 0
    i = np.where(none, 0, index)
    below, above = alt[np.maximum(i - 1, 0)], alt[np.minimum(i + 1, L - 1)]
    start, lo, hi = alt[i], np.minimum(below, above), np.maximum(below, above)
    lo, hi = np.minimum(lo, start), np.maximum(hi, start)
    return tuple(np.where(none, np.nan, a) for a in (start, lo, hi))


LEVEL_HEIGHT_FIELDS = ('height', 'value', 'slope', 'status', 'iterations')
LevelHeight = collections.namedtuple('LevelHeight', LEVEL_HEIGHT_FIELDS)
LevelHeightError = collections.namedtuple('LevelHeightError', LEVEL_HEIGHT_FIELDS + ('height_error',))
CROSSING_WHICH = {'first': 0, 'last': 1}          # vi_eval_resident_cross_f64's which and direction
CROSSING_DIRECTIONS = {'any': 0, 'up': 1, 'down': 2}


def level_brackets(alt_axis, index):
    """(lo, hi) for Estimate.level_height from the altitude axis of a grid and the index map of ResidentGrid.crossing: the grid
    altitudes at `index` and at `index` + 1 - the pair of neighbours that holds the level between them -, the lower of the two
    as lo, so that lo < hi on a descending axis too; NaN where index is -1 (a column without a crossing; level_height gives
    such a column status 3).  alt_axis: 1-D, finite, at least one sample; index: integers in [-1, len(alt_axis) - 1) of any
    shape.  Two float64 arrays of the shape of index.  On the host."""
    alt = np.asarray(alt_axis, dtype=np.float64)
    if alt.ndim != 1 or alt.size == 0 or not np.isfinite(alt).all():
        raise ValueError('alt_axis must be a 1-D array of finite altitudes with at least one sample')
    index = np.asarray(index)
    if index.dtype.kind not in 'iu':
        raise ValueError('index must be an integer array, not %s' % index.dtype)
    index = index.astype(np.int64)
    L = alt.size
    if index.size and (index.min() < -1 or index.max() >= L - 1):
        raise ValueError('index must lie in [-1, %d)' % (L - 1))
    none = index < 0
    i = np.where(none, 0, index)
    below, above = alt[i], alt[np.minimum(i + 1, L - 1)]
    return tuple(np.where(none, np.nan, a) for a in (np.minimum(below, above), np.maximum(below, above)))


RAY_PEAK_FIELDS = ('distance', 'value', 'slope', 'curvature', 'status', 'iterations')
RayPeak = collections.namedtuple('RayPeak', RAY_PEAK_FIELDS)
RayPeakError = collections.namedtuple('RayPeakError', RAY_PEAK_FIELDS + ('distance_error', 'value_error'))
RAY_LEVEL_FIELDS = ('distance', 'value', 'slope', 'status', 'iterations')
RayLevel = collections.namedtuple('RayLevel', RAY_LEVEL_FIELDS)
RayLevelError = collections.namedtuple('RayLevelError', RAY_LEVEL_FIELDS + ('distance_error',))


def _ray_lines(start, end, coords):
    """(shape, a, b, u, length) of the rays of slant_rays: the ray shape S, the end points (P, 3) in ECEF metres, the unit
    directions (P, 3) and the lengths (P,) - NaN directions for a ray of length zero."""
    _, _, shape, a, b = slant_rays(start, end, 1, None, coords)
    a, b = a.T, b.T
    d = b - a
    length = np.sqrt(d[:, 0]**2 + d[:, 1]**2 + d[:, 2]**2)
    with np.errstate(invalid='ignore', divide='ignore'):
        u = d / length[:, None]
    return shape, a, b, u, length


def ray_points(start, end, distance, coords='geodetic'):
    """(gdlat, gdlon, gdalt) of the points at `distance` metres from `start` on the straight rays from `start` to `end`
    (triples of arrays, as Estimate.slant takes them): the points Estimate.ray_peak and ray_level report, for __call__, error
    and the other point entries.  distance: the ray shape S with any leading axes - (T,) + S as ray_peak returns it.  Three
    arrays of the shape of distance, NaN where distance is.  On the host, through geodesy.ecef2geodetic."""
    shape, a, _, u, _ = _ray_lines(start, end, coords)
    distance = np.asarray(distance, dtype=np.float64)
    nd = len(shape)
    if distance.ndim < nd or distance.shape[distance.ndim - nd:] != shape:
        raise ValueError('distance must have the ray shape %r as its last axes, not %r' % (shape, distance.shape))
    s = distance.reshape(-1, a.shape[0])
    with np.errstate(invalid='ignore'):
        X = a.T[:, None, :] + s[None] * u.T[:, None, :]                  # (3, lead, P)
        lat, lon, alt = geodesy.ecef2geodetic(X[0], X[1], X[2])
    return tuple(np.where(np.isfinite(s), v, np.nan).reshape(distance.shape) for v in (lat, lon, alt))


def ray_samples(eq, tol, start, end, n=64, coords='geodetic'):
    """(dist, gdlat, gdlon, gdalt), each S + (n,), S the ray shape: n equispaced samples on the part of every ray inside the
    hull (eq, tol) of hull_equations - the chord hull_chords gives -, as distances in metres from `start` and as geodetic points.
    The two end samples are pulled inside by one part in 10^6 of the chord, so that rounding does not put them outside.  A ray
    that misses the hull has NaN throughout.  est.resident_grid(gdlat, gdlon, gdalt) on these points gives the coarse stage of
    ray_peak and ray_level: g.peak(times) and g.crossing(times, level) along the last axis, ray_peak_brackets and
    ray_level_brackets turn their index maps into brackets.  On the host."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 2:
        raise ValueError('n must be an integer of at least 2, not %r' % (n,))
    shape, a, b, u, length = _ray_lines(start, end, coords)
    s0, s1 = hull_chords(np.zeros((0, 4)) if eq is None else eq, tol, a, b)
    frac = np.linspace(0., 1., int(n))
    frac[0], frac[-1] = 1e-6, 1. - 1e-6
    with np.errstate(invalid='ignore'):
        dist = length[:, None] * (s0[:, None] + (s1 - s0)[:, None] * frac[None, :])       # (P, n)
        X = a.T[:, :, None] + dist[None] * u.T[:, :, None]
        lat, lon, alt = geodesy.ecef2geodetic(X[0], X[1], X[2])
    ok = np.isfinite(dist)
    return tuple(np.where(ok, v, np.nan).reshape(shape + (int(n),)) for v in (dist, lat, lon, alt))


def _ray_index(dist, index, last):
    """(dist, index, none) of the two bracket makers below: dist broadcast to index.shape + (n,), the index checked against
    [-1, last) and with 0 in place of -1, and where it was -1."""
    dist = np.asarray(dist, dtype=np.float64)
    if dist.ndim < 1 or dist.shape[-1] < 1:
        raise ValueError('dist must have the samples of a ray on its last axis')
    index = np.asarray(index)
    if index.dtype.kind not in 'iu':
        raise ValueError('index must be an integer array, not %s' % index.dtype)
    index = index.astype(np.int64)
    n = dist.shape[-1]
    if index.size and (index.min() < -1 or index.max() >= n - last):
        raise ValueError('index must lie in [-1, %d)' % (n - last))
    try:
        dist = np.broadcast_to(dist, index.shape + (n,))
    except ValueError:
        raise ValueError('dist %r does not broadcast to the index map %r with the samples on a last axis'
                         % (dist.shape, index.shape))
    none = index < 0
    return dist, np.where(none, 0, index), none


def ray_peak_brackets(dist, index):
    """(s_start, s_lo, s_hi) for Estimate.ray_peak from the sample distances of ray_samples, S + (n,), and the index map
    (T,) + S (or S) that ResidentGrid.peak gives on those samples along their last axis: the distance of the sample at `index`
    and those of its two neighbours on the ray - the sample itself where it is the first or the last -, NaN where index is -1 (a
    ray without a peak; ray_peak gives it status 3) and where the ray has no samples.  Three float64 arrays of the shape of
    index.  The analogue of peak_brackets.  On the host."""
    dist, i, none = _ray_index(dist, index, 0)
    n = dist.shape[-1]
    pick = lambda j: np.take_along_axis(dist, j[..., None], axis=-1)[..., 0]
    start, below, above = pick(i), pick(np.maximum(i - 1, 0)), pick(np.minimum(i + 1, n - 1))
    with np.errstate(invalid='ignore'):
        lo, hi = np.minimum(np.minimum(below, above), start), np.maximum(np.maximum(below, above), start)
    return tuple(np.where(none, np.nan, a) for a in (start, lo, hi))


def ray_level_brackets(dist, index):
    """(s_lo, s_hi) for Estimate.ray_level from the sample distances of ray_samples and the index map that ResidentGrid.crossing
    gives on those samples along their last axis: the distances of the samples at `index` and at `index` + 1, the smaller first;
    NaN where index is -1 (a ray without a crossing; ray_level gives it status 3).  index: integers in [-1, n - 1).  Two float64
    arrays of the shape of index.  The analogue of level_brackets.  On the host."""
    dist, i, none = _ray_index(dist, index, 1)
    n = dist.shape[-1]
    pick = lambda j: np.take_along_axis(dist, j[..., None], axis=-1)[..., 0]
    below, above = pick(i), pick(np.minimum(i + 1, n - 1))
    with np.errstate(invalid='ignore'):
        return tuple(np.where(none, np.nan, a) for a in (np.minimum(below, above), np.maximum(below, above)))


EXTREMUM_FIELDS = ('gdlat', 'gdlon', 'gdalt', 'value', 'gradient', 'hessian', 'status', 'iterations')
Extremum = collections.namedtuple('Extremum', EXTREMUM_FIELDS)
ExtremumError = collections.namedtuple('ExtremumError', EXTREMUM_FIELDS + ('position_covariance', 'value_error'))


def local_maxima(value, index, alt_axis, kind='max'):
    """The starts of Estimate.extremum from the column maps of ResidentGrid.peak on a (lat, lon, alt) grid: value and index
    (T, nlat, nlon) - the peak of every column along altitude and its position on alt_axis, as g.peak(times, kind=kind) gives
    them -, alt_axis the grid's altitudes.  Returns (t, i, j, alt): the positions, in C order, whose column peak is a number
    (index >= 0) and strictly above (kind='min': below) those of its eight horizontal neighbours that are numbers - a tie with
    a neighbour is no maximum, a NaN neighbour or the edge of the map does not count against one -, and the grid altitude
    alt_axis[index] of that peak.  The coarse stage of a search in three dimensions: a maximum over altitude of every
    column that is also a maximum among the columns around it.  On the host."""
    if kind not in PEAK_HEIGHT_KINDS:
        raise ValueError("kind must be 'max' or 'min', not %r" % (kind,))
    alt = np.asarray(alt_axis, dtype=np.float64)
    if alt.ndim != 1 or alt.size == 0:
        raise ValueError('alt_axis must be a 1-D array with at least one sample')
    value, index = np.asarray(value, dtype=np.float64), np.asarray(index)
    if index.dtype.kind not in 'iu':
        raise ValueError('index must be an integer array, not %s' % index.dtype)
    if value.ndim != 3 or index.shape != value.shape:
        raise ValueError('value and index must have one shape (T, nlat, nlon), not %r and %r' % (value.shape, index.shape))
    index = index.astype(np.int64)
    if index.size and (index.min() < -1 or index.max() >= alt.size):
        raise ValueError('index must lie in [-1, %d)' % alt.size)
    T, n, m = value.shape
    v = PEAK_HEIGHT_KINDS[kind] * np.where(index >= 0, value, np.nan)
    pad = np.full((T, n + 2, m + 2), np.nan)
    pad[:, 1:-1, 1:-1] = v
    top = ~np.isnan(v)
    with np.errstate(invalid='ignore'):
        for di in (0, 1, 2):
            for dj in (0, 1, 2):
                if (di, dj) != (1, 1):
                    w = pad[:, di:di + n, dj:dj + m]
                    top &= (v > w) | np.isnan(w)
    t, i, j = np.nonzero(top)
    return t, i, j, alt[index[t, i, j]]


class Estimate(object):
    def __init__(self, coeff_filename, timetol=60., timeinterp=False, ctx=None):
        self.timetol = timetol
        self.timeinterp = timeinterp
        self._ctx = ctx
        self.loadh5(filename=coeff_filename)
        self._init_model()

    @classmethod
    def from_arrays(cls, Coeffs, Covariance, time, hull_vert, config_text, timetol=60., timeinterp=False, ctx=None):
        """Build an Estimate from in-memory fit results (what loadh5 would have read)."""
        self = cls.__new__(cls)
        self.timetol, self.timeinterp, self._ctx = timetol, timeinterp, ctx
        self.Coeffs = np.asarray(Coeffs, dtype=np.float64)
        self.Covariance = None if Covariance is None else np.asarray(Covariance, dtype=np.float64)
        self.time = np.asarray(time)
        self.hull_vert = np.asarray(hull_vert, dtype=np.float64)
        self.config_file_text = config_text.encode('utf-8') if isinstance(config_text, str) else config_text
        self._init_model()
        return self

    def _init_model(self):
        # estimate.py:41-50: the model is rebuilt from the config text embedded in the file
        config_file = io.StringIO(self.config_file_text.decode('utf-8'))
        config = configparser.ConfigParser()
        config.read_file(config_file)
        self.model_name = config.get('MODEL', 'NAME')
        config_file.seek(0)
        m = importlib.import_module('.models.' + self.model_name, package='volumetricinterp_amd')
        self.model = m.Model(config_file, ctx=self._ctx)
        self._hull_eq = None

    # estimate.py:53-70
    def loadh5(self, filename=None):
        from .h5io import read_coeff_file
        d = read_coeff_file(filename)
        self.Coeffs = d['Coeffs']
        self.Covariance = d['Covariance']
        self.time = d['time']
        self.hull_vert = d['hull_vert']
        self.config_file_text = d['config_file_text']

    def _hull(self):
        if self._hull_eq is None:
            self._hull_eq = hull_equations(self.hull_vert)
        return self._hull_eq

    def _hull_args(self, check_hull):
        """(eq, F, tol): the hull arguments of a library call - the half-spaces, their number, the tolerance - and
        (None, 0, 0.) without the hull test."""
        if not check_hull:
            return None, 0, 0.
        eq, tol = self._hull()
        return eq, eq.shape[0], tol

    # estimate.py:75-123
    def __call__(self, time, gdlat, gdlon, gdalt, calcgrad=False, calcerr=False, check_hull=True):
        # calcgrad / calcerr are accepted and ignored, exactly as in the reference (code after the
        # `return` at estimate.py:123 is dead)
        C, dC = self.get_C(time)
        gdlat = np.asarray(gdlat, dtype=np.float64)
        out = self.evaluate_coeffs(np.asarray(C, dtype=np.float64)[None, :], gdlat, gdlon, gdalt, check_hull)
        return out[0].reshape(gdlat.shape)

    def evaluate_coeffs(self, C, gdlat, gdlon, gdalt, check_hull=True, out=None):
        """out[t] = density of coefficient row C[t] at the points; (T, Q).  `out`: optional C-contiguous float64 (T, Q)
        array to write into (e.g. from _lib.pinned_empty, like the coordinate arrays, for full-rate transfers)."""
        C = np.ascontiguousarray(C, dtype=np.float64)
        lat, lon, alt = ravel_points(gdlat, gdlon, gdalt)
        T, Q = C.shape[0], lat.size
        if C.shape[1] != self.model.nbasis:
            raise ValueError('coefficient vector length %d != nbasis %d' % (C.shape[1], self.model.nbasis))
        out = _check_out(out, (T, Q))
        if Q == 0 or T == 0:
            return out
        h = self.model.handle()
        P = _lib.c_double_p
        eq, F, tol = self._hull_args(check_hull)
        _lib.check(_lib.lib.vi_eval_f64_host(h, Q, lat.ctypes.data_as(P), lon.ctypes.data_as(P),
                                             alt.ctypes.data_as(P), T, C.ctypes.data_as(P),
                                             None if eq is None else eq.ctypes.data_as(P), F, tol,
                                             out.ctypes.data_as(P)), 'vi_eval_f64_host')
        return out

    def resident_grid(self, gdlat, gdlon, gdalt, check_hull=True, gradient=None, hessian=None):
        """The points of a grid that MANY timesteps are going to be evaluated on (the reference calls Estimate.__call__ once
        per timestep and rebuilds the basis of the grid every time, estimate.py:110-115): their basis matrix is assembled once
        and stays in device memory (N x Q doubles - 19 GB at the default order on a 256^3 grid), and every batch of timesteps
        is one matrix product (ResidentGrid.evaluate_coeffs / ResidentGrid.__call__).  Same values as __call__ to rounding.

        `gradient`: None (no gradient maps, nothing more allocated), 'model' or 'enu' - the grid also keeps its gradient basis
        (N x 3 x Q doubles, three times the basis matrix: 57 GB of the 76 GB the two take at the default order on 256^3) and
        ResidentGrid.gradient / evaluate_gradients give the gradient maps of many timesteps as one product, with components
        along the model coordinates (z, theta, phi, as Estimate.gradient) or along local east, north, up.

        `hessian`: None, 'model' or 'enu' in the same way - the grid also keeps its Hessian basis (N x 6 x Q doubles, six times
        the basis matrix, counted in the free-memory check) and ResidentGrid.hessian / evaluate_hessians / laplacian give the
        maps of the second derivatives (Estimate.hessian's entries, packed in GRADCOV_PAIRS order) as one product."""
        return ResidentGrid(self, gdlat, gdlon, gdalt, check_hull, gradient, hessian)

    def resident_rays(self, start, end, nodes=64, rule=None, coords='geodetic', check_hull=True):
        """The rays of a fixed geometry that MANY timesteps are going to be integrated along (an all-sky imager's lines of
        sight, a receiver looking at geostationary satellites, a fixed optical column): Estimate.slant walks the chains of all
        nodes of every ray at every call, but the integral is linear in the coefficients, so the ray-integrated basis
        B[n, p] = (s1 - s0) / 2 |b - a| sum_i w_i basis_n(a_p + s_i (b_p - a_p)) is assembled once (vi_eval_slant_basis_f64,
        kernel K1l) and stays in device memory - N x P doubles, 0.3 GB for 512 x 512 rays at the default order - and every
        batch of timesteps is one matrix product.  start, end, nodes, rule, coords and check_hull as in slant: the same rays,
        the same clip against the data hull, the same rule on the part inside.  Returns a ResidentRays."""
        return ResidentRays(self, start, end, nodes, rule, coords, check_hull)

    def gradient(self, time, gdlat, gdlon, gdalt, check_hull=True, frame='model'):
        """Gradient of the fitted parameter at the points: array of shape gdlat.shape + (3,), components along the
        model coordinates z, theta, phi exactly as ``Model.grad_basis`` defines them (sphharmlag.py:148-184), NaN outside
        the hull.  This is the output the reference's ``__call__`` advertises as ``calcgrad`` but never computes (the
        code after its ``return`` is dead, estimate.py:125-147); ``__call__`` itself keeps ignoring the flag,
        as the reference does.  ``frame='enu'``: the same gradient along local east, north, up (the model-frame result
        rotated on the host by ``Model.gradient_frame``)."""
        if frame not in GRADIENT_FRAMES:
            raise ValueError("frame must be 'model' or 'enu', not %r" % (frame,))
        C, dC = self.get_C(time)
        out, lat, lon, alt = self._at_points('vi_eval_grad_f64', C, gdlat, gdlon, gdalt, (3,), check_hull)
        if frame == 'enu' and lat.size:
            out = np.einsum('pic,pc->pi', self.model.gradient_frame(lat, lon, alt), out)
        return out.reshape(np.shape(gdlat) + (3,))

    def error(self, time, gdlat, gdlon, gdalt, check_hull=True):
        """Standard error of the fitted parameter at the points, sqrt(a^T dC a) with a the basis row of the point and dC
        the coefficient covariance of the record (first-order error propagation): the ``calcerr`` output the reference
        advertises but never computes (estimate.py:139-145).  Same shape as gdlat, NaN outside the hull."""
        C, dC = self.get_C(time)
        return self._at_points('vi_eval_err_f64', dC, gdlat, gdlon, gdalt, (), check_hull)[0].reshape(np.shape(gdlat))

    def gradient_covariance(self, time, gdlat, gdlon, gdalt, check_hull=True, frame='model'):
        """Covariance of the gradient of the fitted parameter at the points: array of shape gdlat.shape + (3, 3), symmetric,
        cov[c][d] = g_c^T 1/2 (dC + dC^T) g_d with g_c the gradient basis of component c at the point and dC the coefficient
        covariance of the record (get_C: with timeinterp the blend of the two neighbours) - first-order error propagation, the
        ``graderr`` the reference advertises but never computes (estimate.py:125-147).  Components and frame as in gradient;
        NaN outside the hull.  The standard error of the gradient along a unit vector u is
        np.sqrt(np.einsum('...i,...ij,...j', u, cov, u)).  One library call (vi_eval_grad_cov_f64): hull test, frame and the
        form on the device, the (Q, 3, N) gradient basis never leaves it."""
        packed = self._gradient_covariance(time, gdlat, gdlon, gdalt, check_hull, frame)
        return gradcov_matrix(packed).reshape(np.shape(gdlat) + (3, 3))

    def gradient_error(self, time, gdlat, gdlon, gdalt, check_hull=True, frame='model'):
        """Standard errors of the three gradient components at the points, shape gdlat.shape + (3,): the square root of the
        diagonal of gradient_covariance (NaN where it is negative, as error gives it)."""
        packed = self._gradient_covariance(time, gdlat, gdlon, gdalt, check_hull, frame)
        with np.errstate(invalid='ignore'):
            return np.sqrt(packed[:3].T).reshape(np.shape(gdlat) + (3,))

    def hessian(self, time, gdlat, gdlon, gdalt, check_hull=True, frame='model'):
        """Hessian of the fitted parameter at the points: array of shape gdlat.shape + (3, 3), symmetric, in the parameter's
        unit per m^2 - the second covariant derivatives (a true tensor) in the orthonormal frame of gradient: (r', theta',
        phi') of the rotated cap, or with frame='enu' local east, north, up, H_enu = F H F^T with Model.gradient_frame's F.
        [..., 2, 2] of frame='enu' is exactly the second derivative along the geodetic normal - the curvature of a layer at
        its peak; the horizontal entries are second derivatives along straight tangent lines, not along curves of constant
        altitude (those differ by the first derivative along `up` over the radius of curvature).  Closed form, no differences:
        the reference has no counterpart.  NaN outside the hull; non-finite at the pole of the cap (sin theta' = 0), as
        gradient is there, and next to it the accuracy falls as eps / sin^2 theta'.  One library call (vi_eval_hess_f64):
        hull test, frame and the contraction with the coefficients on the device, the (Q, 6, N) basis is never formed.
        sphharmlag only, at the orders of gradient."""
        return gradcov_matrix(self._hessian(time, gdlat, gdlon, gdalt, check_hull, frame)).reshape(np.shape(gdlat) + (3, 3))

    def laplacian(self, time, gdlat, gdlon, gdalt, check_hull=True):
        """Laplacian of the fitted parameter at the points, shape of gdlat: the trace of hessian (the same in either frame)."""
        p = self._hessian(time, gdlat, gdlon, gdalt, check_hull, 'model')
        return (p[0] + p[1] + p[2]).reshape(np.shape(gdlat))

    def _hessian(self, time, gdlat, gdlon, gdalt, check_hull, frame):
        """What hessian and laplacian share: the packed (6, Q) result of vi_eval_hess_f64, entries in GRADCOV_PAIRS order."""
        if frame not in GRADIENT_FRAMES:
            raise ValueError("frame must be 'model' or 'enu', not %r" % (frame,))
        C, dC = self.get_C(time)
        C = np.ascontiguousarray(C, dtype=np.float64)
        if C.shape != (self.model.nbasis,):
            raise ValueError('coefficient vector length %d != nbasis %d' % (C.size, self.model.nbasis))
        lat, lon, alt = ravel_points(gdlat, gdlon, gdalt)
        Q = lat.size
        if Q == 0:
            return np.empty((6, 0))
        eq, F, tol = self._hull_args(check_hull)
        with self.model.ctx.scope() as dev:
            dlat, dlon, dalt, dC_ = dev.up(lat), dev.up(lon), dev.up(alt), dev.up(C)
            dO = dev.empty((6, Q))
            _lib.check(_lib.lib.vi_eval_hess_f64(self.model.handle(), Q, dlat.ptr, dlon.ptr, dalt.ptr, dC_.ptr,
                                                 _ptr(None if eq is None else dev.up(eq)), F, tol, GRADIENT_FRAMES[frame],
                                                 dO.ptr), 'vi_eval_hess_f64')
            return dO.download()

    def peak_height(self, times, gdlat, gdlon, start, lo, hi, kind='max', tol=1e-3, max_iter=48, check_hull=True, error=False):
        """Sub-grid layer peaks: per column (gdlat, gdlon) and time the height in [lo, hi] at which the fitted parameter has its
        maximum (kind='min': minimum) along the geodetic normal, and the parameter there - hmF2 and NmF2 of a fitted volume.
        A safeguarded Newton search from `start` on the analytic model itself, not on grid samples: value, slope df/dh and
        curvature d2f/dh2 (hessian(frame='enu')[..., 2, 2]) are closed-form and come from one walk of the basis per iteration;
        a step that leaves the bracket, or a curvature of the wrong sign, is replaced by a bisection of the bracket.  All
        columns and times in ONE library call (vi_eval_peak_f64, kernel k_peak_sph, include/vinterp.h has the iteration).

        times: one naive-UTC datetime or a sequence of T of them; the coefficients of get_C per time, as hessian takes them.
        gdlat, gdlon: the columns, of one shape S, degrees.  start, lo, hi: metres, broadcast to (T,) + S (to S for one time),
        lo <= start <= hi; peak_brackets makes them from the index map of ResidentGrid.peak.  tol: the search stops when a step
        is at most tol metres.  max_iter=48: bisecting 600 km down to 1e-3 m takes 30 steps, Newton on top a handful, the rest
        is slack.

        Returns the named tuple (height, value, slope, curvature, status, iterations), each of shape (T,) + S (S for one time):
        status 0  an interior peak: converged, the curvature has the sign of the kind, farther than tol from lo and hi
               1  converged, but onto an end of the bracket or with a curvature of the wrong sign: no interior peak
               2  not converged within max_iter; max_iter=0 evaluates the start
               3  nothing to report: the start is outside the hull (check_hull) or NaN - what peak_brackets makes of a column
                  without a grid peak -, not lo <= start <= hi, or the record or the basis is not finite there
               4  the search ended outside the hull (tested on the host, self.check_hull); all four values are NaN
        height and value are NaN wherever status is not 0; slope and curvature are those of the last iterate (NaN with status
        3 and 4), iterations the steps made.

        error=True: the named tuple grows by (height_error, value_error), first-order error propagation at the refined peaks,
        NaN where status is not 0: height_error = sqrt(cov_up,up) / |curvature| with the gradient covariance of
        gradient_covariance(frame='enu') - the peak is where the slope is zero, so its height moves by -(error of the slope) /
        curvature - and value_error = error() at the peak.  These are the existing entries called once per time at the refined
        points, not fused into the search.  Raises ValueError when the Estimate holds no covariance.
        sphharmlag only, at the orders of gradient."""
        if kind not in PEAK_HEIGHT_KINDS:
            raise ValueError("kind must be 'max' or 'min', not %r" % (kind,))
        tol = float(tol)
        if not (np.isfinite(tol) and tol > 0.):
            raise ValueError('tol must be finite and positive, not %r' % (tol,))
        if not isinstance(max_iter, (int, np.integer)) or isinstance(max_iter, bool) or max_iter < 0:
            raise ValueError('max_iter must be a non-negative integer, not %r' % (max_iter,))
        if error:
            self._need_covariance()
        single = isinstance(times, dt.datetime)
        times = [times] if single else list(times)
        lat, lon = np.asarray(gdlat, dtype=np.float64), np.asarray(gdlon, dtype=np.float64)
        if lat.shape != lon.shape:
            raise ValueError('gdlat and gdlon must have one shape, not %r and %r' % (lat.shape, lon.shape))
        T, Q, N = len(times), lat.size, self.model.nbasis
        full = (T,) + lat.shape
        try:
            h0, a, b = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), full)).reshape(T, Q)
                        for v in (start, lo, hi))
        except ValueError:
            raise ValueError('start, lo and hi must broadcast to the shape %r' % (full,))
        C = np.empty((T, N))
        for t, time in enumerate(times):
            C[t] = self.get_C(time)[0]
        shape = lat.shape if single else full
        res, status, iters = np.full((4, T, Q), np.nan), np.full((T, Q), 3, dtype=np.int32), np.zeros((T, Q), dtype=np.int32)
        if T and Q:
            latq, lonq = np.tile(lat.ravel(), T), np.tile(lon.ravel(), T)
            eq, F, htol = self._hull_args(check_hull)
            with self.model.ctx.scope() as dev:
                dlat, dlon, dh0, da, db, dC_ = (dev.up(v) for v in (latq, lonq, h0, a, b, C))
                dO, dS, dI = dev.empty((4, T, Q)), dev.empty((T, Q), np.int32), dev.empty((T, Q), np.int32)
                _lib.check(_lib.lib.vi_eval_peak_f64(self.model.handle(), T, Q, dlat.ptr, dlon.ptr, dh0.ptr, da.ptr, db.ptr,
                                                     dC_.ptr, _ptr(None if eq is None else dev.up(eq)), F, htol,
                                                     PEAK_HEIGHT_KINDS[kind], int(max_iter), tol, dO.ptr, dS.ptr, dI.ptr),
                           'vi_eval_peak_f64')
                res, status, iters = dO.download(), dS.download(), dI.download()
            if check_hull:
                ran = status != 3
                left = np.zeros((T, Q), dtype=bool)
                left[ran] = ~self.check_hull(latq.reshape(T, Q)[ran], lonq.reshape(T, Q)[ran], res[0][ran])
                status[left] = 4
                res[:, left] = np.nan
        res[:2, status != 0] = np.nan
        out = tuple(r.reshape(shape) for r in res) + (status.reshape(shape), iters.reshape(shape))
        if not error:
            return PeakHeight(*out)
        herr, verr = np.full((T, Q), np.nan), np.full((T, Q), np.nan)
        for t, time in enumerate(times):
            ok = status[t] == 0
            if ok.any():
                pts = lat.ravel()[ok], lon.ravel()[ok], res[0, t][ok]
                cov = self._gradient_covariance(time, *pts, check_hull, 'enu')
                with np.errstate(invalid='ignore', divide='ignore'):
                    herr[t, ok] = np.sqrt(cov[2]) / np.abs(res[3, t][ok])
                verr[t, ok] = self.error(time, *pts, check_hull)
        return PeakHeightError(*(out + (herr.reshape(shape), verr.reshape(shape))))

    def level_height(self, times, gdlat, gdlon, level, lo, hi, tol=1e-3, max_iter=48, check_hull=True, error=False):
        """Level crossings: per column (gdlat, gdlon) and time the height in [lo, hi] at which the fitted parameter crosses
        `level` along the geodetic normal - the reflection height of a sounding frequency (Ne = 1.24e10 f^2 m^-3, f in MHz),
        the half-peak heights of a layer, an isodensity surface.  A safeguarded Newton search on the analytic model itself, not
        on grid samples: value and slope df/dh are closed-form and come from one gradient walk of the basis per iteration; a
        step that leaves the bracket is replaced by a bisection of the bracket, which always holds a change of sign.  All
        columns and times in ONE library call (vi_eval_level_f64, kernel k_level_sph, include/vinterp.h has the iteration).

        times: one naive-UTC datetime or a sequence of T of them; the coefficients of get_C per time, as peak_height takes
        them.  gdlat, gdlon: the columns, of one shape S, degrees.  level (the parameter's unit), lo, hi (metres): broadcast to
        (T,) + S (to S for one time), lo < hi; level_brackets makes lo and hi from the index map of ResidentGrid.crossing.
        tol: the search stops when a step is at most tol metres.  max_iter: at most 10000.

        Returns the named tuple (height, value, slope, status, iterations), each of shape (T,) + S (S for one time):
        status 0  a crossing: the value is the level exactly, or the last step was at most tol
               1  the parameter minus the level has one sign at lo and at hi: no crossing is bracketed
               2  not converged within max_iter
               3  nothing to report: lo or hi is outside the hull (check_hull) or NaN - what level_brackets makes of a column
                  without a grid crossing -, not lo < hi, the level is NaN, or the record or the basis is not finite there
        height and value are NaN wherever status is not 0; slope is that of the last iterate (NaN with status 1 and 3) and its
        sign tells a bottomside crossing (> 0) from a topside one; iterations the steps made.  Both ends of every bracket go
        through the hull test on the device; the heights between them need none - the geodetic normal of a column is a straight
        line and the hull is convex -, so there is no host pass and no "left the hull" status.

        error=True: the named tuple grows by height_error = error() / |slope| at the crossing, first order - the height moves
        by -(error of the value) / slope, the level taken as exact -, NaN where status is not 0.  The existing entry called
        once per time at the crossings, not fused into the search.  Raises ValueError when the Estimate holds no covariance.
        sphharmlag only, at the orders of gradient."""
        tol = float(tol)
        if not (np.isfinite(tol) and tol > 0.):
            raise ValueError('tol must be finite and positive, not %r' % (tol,))
        if not isinstance(max_iter, (int, np.integer)) or isinstance(max_iter, bool) or not 0 <= max_iter <= 10000:
            raise ValueError('max_iter must be an integer in [0, 10000], not %r' % (max_iter,))
        if error:
            self._need_covariance()
        single = isinstance(times, dt.datetime)
        times = [times] if single else list(times)
        lat, lon = np.asarray(gdlat, dtype=np.float64), np.asarray(gdlon, dtype=np.float64)
        if lat.shape != lon.shape:
            raise ValueError('gdlat and gdlon must have one shape, not %r and %r' % (lat.shape, lon.shape))
        T, Q, N = len(times), lat.size, self.model.nbasis
        full = (T,) + lat.shape
        try:
            lev, a, b = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), full)).reshape(T, Q)
                         for v in (level, lo, hi))
        except ValueError:
            raise ValueError('level, lo and hi must broadcast to the shape %r' % (full,))
        C = np.empty((T, N))
        for t, time in enumerate(times):
            C[t] = self.get_C(time)[0]
        shape = lat.shape if single else full
        res, status, iters = np.full((3, T, Q), np.nan), np.full((T, Q), 3, dtype=np.int32), np.zeros((T, Q), dtype=np.int32)
        if T and Q:
            # both ends of every bracket in one hull pass: the columns twice, the lower ends, then the upper ends
            latq, lonq, ends = np.tile(lat.ravel(), 2 * T), np.tile(lon.ravel(), 2 * T), np.stack((a, b))
            eq, F, htol = self._hull_args(check_hull)
            with self.model.ctx.scope() as dev:
                dlat, dlon, dends, dlev, dC_ = (dev.up(v) for v in (latq, lonq, ends, lev, C))
                dO, dS, dI = dev.empty((3, T, Q)), dev.empty((T, Q), np.int32), dev.empty((T, Q), np.int32)
                _lib.check(_lib.lib.vi_eval_level_f64(self.model.handle(), T, Q, dlat.ptr, dlon.ptr, dends.ptr, dlev.ptr, dC_.ptr,
                                                      _ptr(None if eq is None else dev.up(eq)), F, htol, int(max_iter), tol,
                                                      dO.ptr, dS.ptr, dI.ptr), 'vi_eval_level_f64')
                res, status, iters = dO.download(), dS.download(), dI.download()
        res[:2, status != 0] = np.nan
        out = tuple(r.reshape(shape) for r in res) + (status.reshape(shape), iters.reshape(shape))
        if not error:
            return LevelHeight(*out)
        herr = np.full((T, Q), np.nan)
        for t, time in enumerate(times):
            ok = status[t] == 0
            if ok.any():
                pts = lat.ravel()[ok], lon.ravel()[ok], res[0, t][ok]
                with np.errstate(invalid='ignore', divide='ignore'):
                    herr[t, ok] = self.error(time, *pts, check_hull) / np.abs(res[2, t][ok])
        return LevelHeightError(*(out + (herr.reshape(shape),)))

    def ray_peak(self, times, start, end, s_start, s_lo, s_hi, kind='max', tol=1e-3, max_iter=48, coords='geodetic',
                 check_hull=True, error=False):
        """Peaks along straight rays: per ray from `start` to `end` and time the distance from `start`, in [s_lo, s_hi] metres,
        at which the fitted parameter has its maximum (kind='min': minimum) ALONG THE RAY, and the parameter there - the profile
        peak along a radar beam, to set beside its range gates.  peak_height's safeguarded Newton search with the distance s
        along the line in place of the height: value, slope df/ds = w . grad f and curvature d2f/ds2 = w^T H w - w the ray's unit
        direction in the orthonormal frame of gradient(frame='model') at the point, H the tensor of hessian(frame='model'), so
        that the curvature is exact on a straight line - come from one walk of the basis per iteration.  All rays and times in
        ONE library call (vi_eval_ray_peak_f64, kernel k_line_peak_sph, include/vinterp.h has the geometry and the iteration).

        times: one naive-UTC datetime or a sequence of T of them; the coefficients of get_C per time, as peak_height takes
        them (every ray at every time; rays with a time each: a call per group of rays).  start, end, coords: the rays, as slant
        takes them, of the broadcast shape S.  s_start, s_lo, s_hi: metres from `start`, broadcast to (T,) + S (to S for one
        time), s_lo <= s_start <= s_hi; ray_samples, a resident grid on its points and ray_peak_brackets make them.  tol: the
        search stops when a step is at most tol metres.  max_iter: at most 10000.

        Returns the named tuple (distance, value, slope, curvature, status, iterations), each (T,) + S (S for one time):
        status 0  an interior peak: converged, the curvature has the sign of the kind, farther than tol from s_lo and s_hi
               1  converged, but onto an end of the bracket or with a curvature of the wrong sign: no interior peak
               2  not converged within max_iter; max_iter=0 evaluates the start
               3  nothing to report: an end of the bracket - the point at s_lo or at s_hi - is outside the hull (check_hull), an
                  input is NaN (what ray_peak_brackets makes of a ray without a sampled peak), not s_lo <= s_start <= s_hi, the
                  ray has no length, or the record or the basis is not finite there
        distance and value are NaN wherever status is not 0; slope and curvature are those of the last iterate (NaN with status
        3).  Both ends of every bracket are tested against the hull on the device; the iterates between them need no test -
        the hull is convex -, so there is no host pass and no status 4.  ray_points gives the geodetic points of the distances.

        error=True: the named tuple grows by (distance_error, value_error), first order, NaN where status is not 0:
        distance_error = sqrt(w^T cov w) / |curvature| with gradient_covariance(frame='model') at the peak, value_error =
        error() there.  The existing entries called once per time at the found points, not fused into the search.  Raises
        ValueError when the Estimate holds no covariance.  sphharmlag only, at the orders of gradient."""
        if kind not in PEAK_HEIGHT_KINDS:
            raise ValueError("kind must be 'max' or 'min', not %r" % (kind,))
        q = self._ray_search(times, start, end, coords, (s_start, s_lo, s_hi), 's_start, s_lo and s_hi', tol, max_iter, error)
        T, P = q['T'], q['P']
        res, status, iters = np.full((4, T, P), np.nan), np.full((T, P), 3, dtype=np.int32), np.zeros((T, P), dtype=np.int32)
        if T and P:
            eq, F, htol = self._hull_args(check_hull)
            with self.model.ctx.scope() as dev:
                da, db, d0, dlo, dhi, dC_ = (dev.up(v) for v in (q['a'], q['b']) + q['per'] + (q['C'],))
                dO, dS, dI = dev.empty((4, T, P)), dev.empty((T, P), np.int32), dev.empty((T, P), np.int32)
                _lib.check(_lib.lib.vi_eval_ray_peak_f64(self.model.handle(), T, P, da.ptr, db.ptr, d0.ptr, dlo.ptr, dhi.ptr,
                                                         dC_.ptr, _ptr(None if eq is None else dev.up(eq)), F, htol,
                                                         PEAK_HEIGHT_KINDS[kind], int(max_iter), q['tol'], dO.ptr, dS.ptr, dI.ptr),
                           'vi_eval_ray_peak_f64')
                res, status, iters = dO.download(), dS.download(), dI.download()
        res[:2, status != 0] = np.nan
        shape = q['shape']
        out = tuple(r.reshape(shape) for r in res) + (status.reshape(shape), iters.reshape(shape))
        if not error:
            return RayPeak(*out)
        derr, verr = np.full((T, P), np.nan), np.full((T, P), np.nan)
        for t, time in enumerate(q['times']):
            ok = status[t] == 0
            if ok.any():
                pts, w = self._ray_frame(q, ok, res[0, t][ok])
                cov = gradcov_matrix(self._gradient_covariance(time, *pts, check_hull, 'model'))
                with np.errstate(invalid='ignore', divide='ignore'):
                    derr[t, ok] = np.sqrt(np.einsum('pi,pij,pj->p', w, cov, w)) / np.abs(res[3, t][ok])
                verr[t, ok] = self.error(time, *pts, check_hull)
        return RayPeakError(*(out + (derr.reshape(shape), verr.reshape(shape))))

    def ray_level(self, times, start, end, level, s_lo, s_hi, tol=1e-3, max_iter=48, coords='geodetic', check_hull=True,
                  error=False):
        """Level crossings along straight rays: per ray from `start` to `end` and time the distance from `start`, in
        [s_lo, s_hi] metres, at which the fitted parameter crosses `level` ALONG THE RAY - the point where an oblique sounder's
        ray meets the plasma frequency, the place where a line of sight enters a patch (crosses an isodensity surface).
        level_height's safeguarded Newton search with the distance s along the line in place of the height: value and slope
        df/ds = w . grad f, w the ray's unit direction in the frame of gradient(frame='model') at the point, from one gradient
        walk of the basis per iteration.  All rays and times in ONE library call (vi_eval_ray_level_f64, kernel
        k_line_level_sph).

        times, start, end, coords: as ray_peak.  level (the parameter's unit), s_lo, s_hi (metres from `start`): broadcast to
        (T,) + S (to S for one time), s_lo < s_hi; ray_samples, a resident grid on its points (ResidentGrid.crossing) and
        ray_level_brackets make the bracket.  tol, max_iter: as ray_peak.

        Returns the named tuple (distance, value, slope, status, iterations), each (T,) + S (S for one time):
        status 0  a crossing: the value is the level exactly, or the last step was at most tol
               1  the parameter minus the level has one sign at s_lo and at s_hi: no crossing is bracketed
               2  not converged within max_iter
               3  nothing to report: an end of the bracket is outside the hull (check_hull), an input is NaN, not s_lo < s_hi,
                  the ray has no length, or the record or the basis is not finite there
        distance and value are NaN wherever status is not 0; slope is that of the last iterate (NaN with status 1 and 3), its
        sign tells entering (> 0) from leaving.  The hull as in ray_peak.

        error=True: the named tuple grows by distance_error = error() / |slope| at the crossing, first order, NaN where status
        is not 0; the existing entry called once per time, not fused.  sphharmlag only, at the orders of gradient."""
        q = self._ray_search(times, start, end, coords, (level, s_lo, s_hi), 'level, s_lo and s_hi', tol, max_iter, error)
        T, P = q['T'], q['P']
        res, status, iters = np.full((3, T, P), np.nan), np.full((T, P), 3, dtype=np.int32), np.zeros((T, P), dtype=np.int32)
        if T and P:
            lev, lo, hi = q['per']
            eq, F, htol = self._hull_args(check_hull)
            with self.model.ctx.scope() as dev:
                da, db, dends, dlev, dC_ = (dev.up(v) for v in (q['a'], q['b'], np.stack((lo, hi)), lev, q['C']))
                dO, dS, dI = dev.empty((3, T, P)), dev.empty((T, P), np.int32), dev.empty((T, P), np.int32)
                _lib.check(_lib.lib.vi_eval_ray_level_f64(self.model.handle(), T, P, da.ptr, db.ptr, dends.ptr, dlev.ptr, dC_.ptr,
                                                          _ptr(None if eq is None else dev.up(eq)), F, htol, int(max_iter),
                                                          q['tol'], dO.ptr, dS.ptr, dI.ptr), 'vi_eval_ray_level_f64')
                res, status, iters = dO.download(), dS.download(), dI.download()
        res[:2, status != 0] = np.nan
        shape = q['shape']
        out = tuple(r.reshape(shape) for r in res) + (status.reshape(shape), iters.reshape(shape))
        if not error:
            return RayLevel(*out)
        derr = np.full((T, P), np.nan)
        for t, time in enumerate(q['times']):
            ok = status[t] == 0
            if ok.any():
                pts, _ = self._ray_frame(q, ok, res[0, t][ok])
                with np.errstate(invalid='ignore', divide='ignore'):
                    derr[t, ok] = self.error(time, *pts, check_hull) / np.abs(res[2, t][ok])
        return RayLevelError(*(out + (derr.reshape(shape),)))

    def extremum(self, times, gdlat, gdlon, gdalt, radius, kind='max', max_step=None, tol=1e-3, max_iter=48, check_hull=True,
                 error=False):
        """Maxima and minima in three dimensions: per start (gdlat, gdlon, gdalt) and time the point within `radius` metres of
        the start, and inside the hull, at which the fitted parameter has its maximum (kind='min': minimum) - the centre of a
        polar-cap patch or of a depletion -, the parameter there and its Hessian, whose principal curvatures are the size of the
        patch.  peak_height, level_height and ray_peak search along a direction the caller chooses and give the extremum along
        it; this one has no direction.  A safeguarded Newton iteration in ECEF on the analytic model itself: value, gradient and
        Hessian are closed-form and come from one walk of the basis per iteration, the Hessian - a tensor - turned into the plain
        Cartesian matrix of second derivatives, so that the iteration is exact; steps are limited to a trust length (max_step at
        most), curvature of the wrong sign is floored, a step that lowers the value or leaves the region is taken back in part.
        All starts and times in ONE library call (vi_eval_extremum_f64, kernel k_extremum_sph, include/vinterp.h has the
        iteration); the hull test of every iterate is in the kernel, there is no host pass.

        times: one naive-UTC datetime or a sequence of T of them; the coefficients of get_C per time, as peak_height takes
        them.  gdlat, gdlon (degrees): the starts' columns, broadcast to one shape S.  gdalt, radius (metres): broadcast to
        (T,) + S, as peak_height takes its start; with one time all four broadcast to S.  local_maxima makes the starts from
        the maps of ResidentGrid.peak.  max_step: metres, one number, the longest step;
        None: an eighth of each search's radius.  tol: the search stops when a step is at most tol metres.  max_iter: at most
        10000.

        Returns the named tuple (gdlat, gdlon, gdalt, value, gradient, hessian, status, iterations): gradient (T,) + S + (3,)
        and hessian (T,) + S + (3, 3) along local east, north, up at the RETURNED point, the others (T,) + S (S for one time):
        status 0  an interior extremum: the last step was an unmodified Newton step of at most tol, and the Hessian at the
                  result is definite with the sign of the kind
               1  converged without one: onto the boundary of the hull or of the ball, or at a point of the wrong curvature
               2  not converged within max_iter; max_iter=0 evaluates the start
               3  nothing to report: the start is outside the hull (check_hull) or NaN, radius is not finite and positive, or
                  the record or the basis is not finite there
        Position and value are NaN wherever status is not 0; gradient and hessian are those of the last iterate (NaN with
        status 3).  gdlon comes from geodesy.ecef2geodetic, in (-180, 180].

        error=True: the named tuple grows by (position_covariance, value_error), first order, NaN where status is not 0:
        position_covariance (..., 3, 3) = H^-1 S H^-1 in east, north, up with S = gradient_covariance(frame='enu') at the point
        and H the returned Hessian - the extremum is where the gradient is zero, so it moves by -H^-1 (error of the gradient),
        the three-dimensional form of peak_height's sqrt(cov) / |curvature| - and value_error = error() there.  The existing
        entries called once per time at the found points, not fused into the search.  Raises ValueError when the Estimate
        holds no covariance.  sphharmlag only, at the orders of gradient."""
        if kind not in PEAK_HEIGHT_KINDS:
            raise ValueError("kind must be 'max' or 'min', not %r" % (kind,))
        tol = float(tol)
        if not (np.isfinite(tol) and tol > 0.):
            raise ValueError('tol must be finite and positive, not %r' % (tol,))
        if not isinstance(max_iter, (int, np.integer)) or isinstance(max_iter, bool) or not 0 <= max_iter <= 10000:
            raise ValueError('max_iter must be an integer in [0, 10000], not %r' % (max_iter,))
        if max_step is not None:
            max_step = float(max_step)
            if not (np.isfinite(max_step) and max_step > 0.):
                raise ValueError('max_step must be finite and positive, not %r' % (max_step,))
        if error:
            self._need_covariance()
        single = isinstance(times, dt.datetime)
        times = [times] if single else list(times)
        T, N = len(times), self.model.nbasis
        args = tuple(np.asarray(v, dtype=np.float64) for v in (gdlat, gdlon, gdalt, radius))
        try:
            S = np.broadcast(*args).shape if single else np.broadcast(args[0], args[1]).shape
        except ValueError:
            raise ValueError('gdlat, gdlon, gdalt and radius do not broadcast to one shape')
        full, P = (T,) + S, int(np.prod(S, dtype=np.int64))
        try:
            lat, lon, alt, rad = (np.ascontiguousarray(np.broadcast_to(v, full)).reshape(T, P) for v in args)
        except ValueError:
            raise ValueError('gdlat, gdlon, gdalt and radius must broadcast to the shape %r' % (full,))
        C = np.empty((T, N))
        for t, time in enumerate(times):
            C[t] = self.get_C(time)[0]
        shape = S if single else full
        res, status, iters = np.full((13, T, P), np.nan), np.full((T, P), 3, dtype=np.int32), np.zeros((T, P), dtype=np.int32)
        if T and P:
            with np.errstate(invalid='ignore'):
                x0 = np.ascontiguousarray(np.stack(geodesy.geodetic2ecef(lat, lon, alt)))
            eq, F, htol = self._hull_args(check_hull)
            with self.model.ctx.scope() as dev:
                dx, dr, dC_ = dev.up(x0), dev.up(rad), dev.up(C)
                dO, dS, dI = dev.empty((13, T, P)), dev.empty((T, P), np.int32), dev.empty((T, P), np.int32)
                _lib.check(_lib.lib.vi_eval_extremum_f64(self.model.handle(), T, P, dx.ptr, dr.ptr, dC_.ptr,
                                                         _ptr(None if eq is None else dev.up(eq)), F, htol,
                                                         PEAK_HEIGHT_KINDS[kind], 0. if max_step is None else max_step,
                                                         int(max_iter), tol, dO.ptr, dS.ptr, dI.ptr), 'vi_eval_extremum_f64')
                res, status, iters = dO.download(), dS.download(), dI.download()
        # geodetic points, and gradient and Hessian along east, north, up there: A g and A H A^T with the geodetic axes A
        with np.errstate(invalid='ignore'):
            plat, plon, palt = geodesy.ecef2geodetic(res[0], res[1], res[2])
            sl, cl, so, co = (f(np.radians(v)) for v in (plat, plon) for f in (np.sin, np.cos))
            zero = np.zeros_like(sl)
            A = np.stack([np.stack([-so, co, zero], axis=-1), np.stack([-sl * co, -sl * so, cl], axis=-1),
                          np.stack([cl * co, cl * so, sl], axis=-1)], axis=-2)                    # (T, P, 3, 3): rows e, n, u
            grad = np.einsum('tpic,ctp->tpi', A, res[4:7])
            hess = np.einsum('tpic,tpcd,tpjd->tpij', A, gradcov_matrix(res[7:13].reshape(6, T * P)).reshape(T, P, 3, 3), A)
        value = res[3].copy()
        for v in (plat, plon, palt, value):
            v[status != 0] = np.nan
        out = tuple(v.reshape(shape) for v in (plat, plon, palt, value)) + (grad.reshape(shape + (3,)),
                                                                            hess.reshape(shape + (3, 3)),
                                                                            status.reshape(shape), iters.reshape(shape))
        if not error:
            return Extremum(*out)
        pcov, verr = np.full((T, P, 3, 3), np.nan), np.full((T, P), np.nan)
        for t, time in enumerate(times):
            ok = status[t] == 0
            if ok.any():
                pts = plat[t][ok], plon[t][ok], palt[t][ok]
                cov = gradcov_matrix(self._gradient_covariance(time, *pts, check_hull, 'enu'))
                Hi = np.linalg.inv(hess[t][ok])
                pcov[t, ok] = np.einsum('pij,pjk,plk->pil', Hi, cov, Hi)
                verr[t, ok] = self.error(time, *pts, check_hull)
        return ExtremumError(*(out + (pcov.reshape(shape + (3, 3)), verr.reshape(shape))))

    def _ray_search(self, times, start, end, coords, per, names, tol, max_iter, error):
        """What ray_peak and ray_level share ahead of their library call: the arguments checked, the rays as (3, P) planar end
        points, the three per-(time, ray) arrays `per` broadcast to (T, P) and the coefficient rows of the times."""
        tol = float(tol)
        if not (np.isfinite(tol) and tol > 0.):
            raise ValueError('tol must be finite and positive, not %r' % (tol,))
        if not isinstance(max_iter, (int, np.integer)) or isinstance(max_iter, bool) or not 0 <= max_iter <= 10000:
            raise ValueError('max_iter must be an integer in [0, 10000], not %r' % (max_iter,))
        if error:
            self._need_covariance()
        single = isinstance(times, dt.datetime)
        times = [times] if single else list(times)
        _, _, S, a, b = slant_rays(start, end, 1, None, coords)
        T, P, N = len(times), a.shape[1], self.model.nbasis
        full = (T,) + S
        try:
            per = tuple(np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), full)).reshape(T, P) for v in per)
        except ValueError:
            raise ValueError('%s must broadcast to the shape %r' % (names, full))
        C = np.empty((T, N))
        for t, time in enumerate(times):
            C[t] = self.get_C(time)[0]
        return dict(times=times, T=T, P=P, a=np.ascontiguousarray(a), b=np.ascontiguousarray(b), per=per, C=C, tol=tol,
                    shape=S if single else full)

    def _ray_frame(self, q, ok, distance):
        """((gdlat, gdlon, gdalt), w) at `distance` on the rays `ok` (a mask over the P rays) of _ray_search's `q`: the geodetic
        points, and the rays' unit directions in the model's orthonormal frame there - u turned into east, north, up at the
        point and then through Model.gradient_frame (orthogonal: w = F^T u_enu)."""
        a, b = q['a'][:, ok].T, q['b'][:, ok].T
        d = b - a
        u = d / np.sqrt(d[:, 0]**2 + d[:, 1]**2 + d[:, 2]**2)[:, None]
        X = a + distance[:, None] * u
        lat, lon, alt = geodesy.ecef2geodetic(X[:, 0], X[:, 1], X[:, 2])
        sl, cl, so, co = (f(np.radians(v)) for v in (lat, lon) for f in (np.sin, np.cos))
        enu = np.stack([-so * u[:, 0] + co * u[:, 1],
                        -sl * co * u[:, 0] - sl * so * u[:, 1] + cl * u[:, 2],
                        cl * co * u[:, 0] + cl * so * u[:, 1] + sl * u[:, 2]], axis=1)
        w = np.einsum('pic,pi->pc', self.model.gradient_frame(lat, lon, alt), enu)
        return (lat, lon, alt), w

    def _need_covariance(self):
        if self.Covariance is None:
            raise ValueError('this Estimate holds no covariance (Covariance is None): no standard error to evaluate')

    def _gradient_covariance(self, time, gdlat, gdlon, gdalt, check_hull, frame):
        """What gradient_covariance and gradient_error share: the packed (6, Q) result of vi_eval_grad_cov_f64."""
        if frame not in GRADIENT_FRAMES:
            raise ValueError("frame must be 'model' or 'enu', not %r" % (frame,))
        self._need_covariance()
        C, dC = self.get_C(time)
        lat, lon, alt = ravel_points(gdlat, gdlon, gdalt)
        Q = lat.size
        if Q == 0:
            return np.empty((6, 0))
        eq, F, tol = self._hull_args(check_hull)
        with self.model.ctx.scope() as dev:
            dlat, dlon, dalt = dev.up(lat), dev.up(lon), dev.up(alt)
            dD = dev.up(np.ascontiguousarray(dC, dtype=np.float64))
            dO = dev.empty((6, Q))
            _lib.check(_lib.lib.vi_eval_grad_cov_f64(self.model.handle(), Q, dlat.ptr, dlon.ptr, dalt.ptr, dD.ptr,
                                                     _ptr(None if eq is None else dev.up(eq)), F, tol, GRADIENT_FRAMES[frame],
                                                     dO.ptr), 'vi_eval_grad_cov_f64')
            return dO.download()

    def _at_points(self, entry, mat, gdlat, gdlon, gdalt, width, check_hull):
        """What gradient and error share: the library's `entry` (points and the record's matrix `mat` in, (Q,) + width
        out) on device copies, NaN outside the hull.  Returns (out, lat, lon, alt), the coordinates raveled."""
        lat, lon, alt = ravel_points(gdlat, gdlon, gdalt)
        Q = lat.size
        out = np.empty((Q,) + width)
        if Q:
            with self.model.ctx.scope() as dev:     # (a failed call must not keep device memory)
                dlat, dlon, dalt, dM = dev.up(lat), dev.up(lon), dev.up(alt), dev.up(np.ascontiguousarray(mat, dtype=np.float64))
                dO = dev.empty((Q,) + width)
                _lib.check(getattr(_lib.lib, entry)(self.model.handle(), Q, dlat.ptr, dlon.ptr, dalt.ptr, dM.ptr, dO.ptr), entry)
                out = dO.download()
            if check_hull:
                out[~self.check_hull(lat, lon, alt)] = np.nan
        return out, lat, lon, alt

    def select_records(self, times, outside='raise'):
        """(rec, w) of select_records for `times` - naive-UTC datetimes or float unix seconds, any shape - with this
        Estimate's records, timetol and timeinterp: what get_C selects for each of them."""
        return select_records(self.time, unix_seconds(times), self.timetol, self.timeinterp, outside)

    def track(self, times, gdlat, gdlon, gdalt, check_hull=True, outside='raise', out=None):
        """Densities along a trajectory: element q is what self(times[q], gdlat[q], gdlon[q], gdalt[q], check_hull=check_hull)
        returns - the record of get_C per point (nearest within timetol, or with timeinterp the blend of the two neighbours),
        NaN outside the hull and where a record the point needs holds a NaN - in ONE library call for all points
        (vi_eval_track_f64) instead of one __call__ per record of a satellite pass, another radar's gates or a series of
        profiles.  times: naive-UTC datetimes or float unix seconds, of the shape of gdlat or one value for all points.
        outside='raise': a time out of range of the file raises as get_C does; 'nan': those points are NaN.  Same shape as
        gdlat; `out`: optional C-contiguous float64 array of that shape to write into."""
        return self._along_track('vi_eval_track_f64', (), (), times, gdlat, gdlon, gdalt, check_hull, outside, out)

    def track_gradient(self, times, gdlat, gdlon, gdalt, check_hull=True, outside='raise', frame='model', out=None):
        """Gradients along a trajectory: element q is what self.gradient(times[q], gdlat[q], gdlon[q], gdalt[q], check_hull,
        frame) returns - the record of get_C per point (with timeinterp the blend of the gradients of the two neighbours,
        the gradient being linear in the coefficients), NaN triples outside the hull and where a record the point needs holds
        a NaN - in ONE library call for all points (vi_eval_track_grad_f64, kernel K2tg) instead of one gradient call per
        record.  times, outside as in track; frame as in gradient ('model': along z, theta, phi; 'enu': along local east,
        north, up, rotated on the device).  Shape gdlat.shape + (3,); `out`: optional C-contiguous float64 array of that
        shape to write into."""
        if frame not in GRADIENT_FRAMES:
            raise ValueError("frame must be 'model' or 'enu', not %r" % (frame,))
        return self._along_track('vi_eval_track_grad_f64', (3,), (GRADIENT_FRAMES[frame],), times, gdlat, gdlon, gdalt, check_hull,
                                 outside, out)

    def track_error(self, times, gdlat, gdlon, gdalt, check_hull=True, outside='raise', out=None):
        """Standard errors along a trajectory: element q is what self.error(times[q], gdlat[q], gdlon[q], gdalt[q], check_hull)
        returns - sqrt(a^T dC a) with the covariance of get_C per point (with timeinterp the blend of the two neighbours'
        covariances), NaN outside the hull, where a covariance the point needs holds a NaN and where the form is negative - in
        ONE library call for all points (vi_eval_track_err_f64, kernel K2te) instead of one error call, and one upload of a
        covariance, per record.  Only the covariances the points need go to the device (used_records).  times, outside and
        `out` as in track; same shape as gdlat.  Raises ValueError when the Estimate holds no covariance."""
        return self._along_track('vi_eval_track_err_f64', (), (), times, gdlat, gdlon, gdalt, check_hull, outside, out,
                                 covariance=True)

    def track_gradient_covariance(self, times, gdlat, gdlon, gdalt, check_hull=True, outside='raise', frame='model', out=None):
        """Gradient covariances along a trajectory: element q is what self.gradient_covariance(times[q], gdlat[q], gdlon[q],
        gdalt[q], check_hull, frame) returns - the symmetric 3 x 3 covariance of the gradient with the covariance of get_C per
        point, NaN outside the hull and where a covariance the point needs holds a NaN - in ONE library call for all points
        (vi_eval_track_grad_cov_f64, kernel K2tc) instead of one call, one upload of a covariance and one host hull test per
        record.  With timeinterp the two neighbours' forms are blended, (1 - w) U_r + w U_(r+1), where gradient_covariance
        blends the covariances before the form: the same quantity, the form being linear in dC, to rounding.  Only the
        covariances the points need go to the device (used_records).  times, outside as in track, frame as in gradient.
        Shape gdlat.shape + (3, 3); `out`: optional C-contiguous float64 array of that shape to write into.  Raises ValueError
        when the Estimate holds no covariance."""
        return self._track_gradient_covariance((3, 3), gradcov_matrix, times, gdlat, gdlon, gdalt, check_hull, outside, frame, out)

    def track_gradient_error(self, times, gdlat, gdlon, gdalt, check_hull=True, outside='raise', frame='model', out=None):
        """Standard errors of the three gradient components along a trajectory, shape gdlat.shape + (3,): the square root of
        the diagonal of track_gradient_covariance (NaN where it is negative, as gradient_error gives it); element q is what
        self.gradient_error(times[q], gdlat[q], gdlon[q], gdalt[q], check_hull, frame) returns.  Arguments as there."""
        def root(packed):
            with np.errstate(invalid='ignore'):
                return np.sqrt(packed[:3].T)
        return self._track_gradient_covariance((3,), root, times, gdlat, gdlon, gdalt, check_hull, outside, frame, out)

    def _track_gradient_covariance(self, width, unpack, times, gdlat, gdlon, gdalt, check_hull, outside, frame, out):
        """What track_gradient_covariance and track_gradient_error share: the packed (6, Q) result of
        vi_eval_track_grad_cov_f64 through _along_track, unpacked to (Q,) + width by `unpack`."""
        if frame not in GRADIENT_FRAMES:
            raise ValueError("frame must be 'model' or 'enu', not %r" % (frame,))
        return self._along_track('vi_eval_track_grad_cov_f64', width, (GRADIENT_FRAMES[frame],), times, gdlat, gdlon, gdalt,
                                 check_hull, outside, out, covariance=True, planar=(6, unpack))

    def _along_track(self, entry, width, extra, times, gdlat, gdlon, gdalt, check_hull, outside, out, covariance=False,
                     planar=None):
        """What track, track_gradient, track_error and the track_gradient_covariance pair share: the record (rec, w) of every
        point's time, the points sorted by record (stable), the library's `entry` - points, the arguments of _upload_records
        (`covariance`: of the covariances in place of the coefficients), `extra` arguments in, (Q,) + width out - on device
        copies, the result back in the caller's order: an array of shape gdlat.shape + width.  `planar` = (K, unpack): the
        entry writes K planes, (K, Q), which unpack turns into (Q,) + width on the host."""
        if covariance:
            self._need_covariance()
        lat, lon, alt = ravel_points(gdlat, gdlon, gdalt)
        shape, Q = np.shape(gdlat), lat.size
        t0 = self._times_for(times, shape, 'gdlat')
        out = _check_out(out, shape + width)
        if Q == 0:
            return out
        rec, w = self.select_records(t0, outside)
        order = np.argsort(rec, kind='stable')          # the kernel's cost grows with the span of records in 64 points
        with self.model.ctx.scope() as dev:
            dlat, dlon, dalt = dev.up(lat[order]), dev.up(lon[order]), dev.up(alt[order])
            records = self._upload_records(dev, rec[order], None if w is None else w[order], check_hull, covariance)
            dO = dev.empty((Q,) + width if planar is None else (planar[0], Q))
            _lib.check(getattr(_lib.lib, entry)(self.model.handle(), Q, dlat.ptr, dlon.ptr, dalt.ptr, *records, *extra, dO.ptr),
                       entry)
            res = dO.download()
        out.reshape((Q,) + width)[order] = res if planar is None else planar[1](res)
        return out

    def _times_for(self, times, shape, what):
        """The host half of what track and slant share: float64 unix seconds of `times`, one per point or ray, raveled."""
        t0 = unix_seconds(times)
        if t0.ndim and t0.shape != shape:
            raise ValueError('times must be one value or have the shape of ' + what)
        return np.broadcast_to(t0, shape).ravel()

    def _upload_records(self, dev, rec, w, check_hull, covariance=False):
        """The device half: the run of arguments vi_eval_track_f64 and vi_eval_slant_f64 share - (rec, w or None, R, Coeffs,
        hull or None, F, tol) - of the (rec, w) of select_records in the caller's order, the device copies in the scope `dev`.
        `covariance`: the run of vi_eval_track_err_f64 and vi_eval_slant_err_f64 - the covariances used_records keeps in place
        of the coefficients, their number for R and rec re-indexed into them."""
        eq, F, tol = self._hull_args(check_hull)
        M = self.Coeffs
        if covariance:
            rows, rec = used_records(rec, w, self.Covariance.shape[0])
            M = self.Covariance[rows]
        dr = dev.up(rec, np.int32)
        dw = None if w is None else dev.up(w)
        dM = dev.up(np.ascontiguousarray(M, dtype=np.float64))
        dh = None if eq is None else dev.up(eq)
        return dr.ptr, _ptr(dw), M.shape[0], dM.ptr, _ptr(dh), F, tol

    def slant(self, times, start, end, nodes=64, rule=None, coords='geodetic', check_hull=True, outside='raise', chord=False,
              out=None):
        """Line integrals of the fitted parameter along straight rays, every ray at its own time (slant TEC between a receiver
        and a satellite, an occultation link, an optical column), in ONE library call (vi_eval_slant_f64, kernel K2l).

        start, end: triples of arrays - (gdlat, gdlon, gdalt) in degrees, degrees, metres with coords='geodetic', (X, Y, Z) in
        metres with coords='ecef'.  The six arrays broadcast against each other (one receiver, many satellites); the ray shape
        is the broadcast shape.  times: one value or an array of the ray shape, naive-UTC datetimes or float unix seconds; the
        record (or the pair, with timeinterp) of each ray is what select_records gives, `outside` as in track.
        nodes: Gauss-Legendre nodes per ray, 1 to 256.  rule=(x, w): the caller's own rule on [-1, 1] instead (finite 1-D
        arrays of one length up to 65 536; a composite or trapezoid rule is one of these); `nodes` is then ignored.  The default
        is converged: 64 and 128 nodes differ by 1.4e-14 of the ray's absolute sum at most on receiver-to-GNSS rays through the
        hull of the default fixture (profiles/r10_perf_eval_slant.txt).

        With a, b the ECEF end points, ray p gives  sum_i w_i (s1 - s0) / 2 |b - a| f(a + s_i (b - a)),
        s_i = s0 + (s1 - s0) (1 + x_i) / 2, f the fitted parameter at the ray's time: the parameter's unit times metres.
        [s0, s1] is the part of the segment inside the data hull (hull_chords) with check_hull, else [0, 1]; the rule sits on
        exactly that interval, on which the model is analytic.  NaN where the segment does not enter the hull, where the ray
        has no record (outside='nan'), where a record it needs holds a NaN (with timeinterp: at w == 0 too, as get_C's blend)
        and where an end point is not finite; 0 for a segment of length zero inside the hull.

        chord=True: returns (value, d0, d1), d0 = s0 |b - a| and d1 = s1 |b - a| the distances from `start` in metres between
        which the ray is inside the hull - geometry only, given for a ray without a record too; NaN for a miss.
        `out`: optional C-contiguous float64 array of the ray shape to write the values into."""
        return self._along_rays('vi_eval_slant_f64', times, start, end, nodes, rule, coords, check_hull, outside, chord, out)

    def slant_error(self, times, start, end, nodes=64, rule=None, coords='geodetic', check_hull=True, outside='raise',
                    chord=False, out=None):
        """Standard errors of the line integrals of slant, every ray at its own time: element p is what
        resident_rays(ray p).error([times[p]]) gives - sqrt(b^T dC b) with b the ray-integrated basis of the ray (K1l: the
        clip and the rule of slant) and dC the covariance of get_C for the ray's time (with timeinterp the blend of the two
        neighbours' covariances), in the parameter's unit times metres - in ONE library call (vi_eval_slant_err_f64, kernels
        K1l and K2te).  Arguments, broadcasting, `chord` and `out` exactly as in slant; NaN where slant gives NaN - a ray that
        does not enter the hull, has no record (outside='nan') or a non-finite end point, a NaN in a covariance it needs - and
        where the form is negative; 0 for a segment of length zero inside the hull.  The rays are sorted by record on the host
        and only the covariances they need go to the device (used_records); results come back in the caller's order.  Raises
        ValueError when the Estimate holds no covariance."""
        return self._along_rays('vi_eval_slant_err_f64', times, start, end, nodes, rule, coords, check_hull, outside, chord, out,
                                covariance=True)

    def _along_rays(self, entry, times, start, end, nodes, rule, coords, check_hull, outside, chord, out, covariance=False):
        """What slant and slant_error share: the rays and the rule of slant_rays, the record (rec, w) of every ray's time, the
        library's `entry` - end points, the arguments of _upload_records, the rule in, values and chords out - on device copies.
        `covariance`: the records are covariances, and the rays go sorted by record (stable; K2te's cost grows with the runs of
        records, K2l's does not) and come back in the caller's order."""
        if covariance:
            self._need_covariance()
        x, wq, shape, a, b = slant_rays(start, end, nodes, rule, coords)
        t0 = self._times_for(times, shape, 'the rays')
        out = _check_out(out, shape)
        P = a.shape[1]
        if P == 0:
            return (out, np.empty(shape), np.empty(shape)) if chord else out
        rec, w = self.select_records(t0, outside)
        order = np.argsort(rec, kind='stable') if covariance else slice(None)
        with self.model.ctx.scope() as dev:
            da, db = dev.up(a[:, order]), dev.up(b[:, order])
            records = self._upload_records(dev, rec[order], None if w is None else w[order], check_hull, covariance)
            dx, dq = dev.up(x), dev.up(wq)
            dO = dev.empty(P)
            dS = dev.empty((2, P)) if chord else None
            _lib.check(getattr(_lib.lib, entry)(self.model.handle(), P, da.ptr, db.ptr, *records, x.size, dx.ptr, dq.ptr, dO.ptr,
                                                _ptr(dS)), entry)
            out.reshape(-1)[order] = dO.download()
            if chord:
                length = np.linalg.norm(b - a, axis=0)
                s = np.empty((2, P))
                s[:, order] = dS.download()
                return out, (s[0] * length).reshape(shape), (s[1] * length).reshape(shape)
        return out

    # estimate.py:153-178 (boolean mask, same shape as the inputs)
    def check_hull(self, lat0, lon0, alt0):
        alt0 = np.asarray(alt0, dtype=np.float64)
        z = np.zeros((1, self.model.nbasis))
        out = self.evaluate_coeffs(z, lat0, lon0, alt0, check_hull=True)
        return np.isfinite(out[0]).reshape(alt0.shape)

    # estimate.py:180-221
    def get_C(self, t):
        t0 = (t - dt.datetime(1970, 1, 1)).total_seconds()
        mt = np.mean(self.time, axis=1)
        try:
            if self.timeinterp:
                i = np.argwhere((t0 >= mt[:-1]) & (t0 < mt[1:])).flatten()[0]
                T = (t0 - mt[i]) / (mt[i + 1] - mt[i])
                C = (1 - T) * self.Coeffs[i, :] + T * self.Coeffs[i + 1, :]
                dC = (1 - T) * self.Covariance[i, :, :] + T * self.Covariance[i + 1, :, :]
            else:
                i = np.argmin(np.abs(mt - t0))
                if np.abs(mt[i] - t0) > self.timetol:
                    raise IndexError
                C = self.Coeffs[i]
                dC = self.Covariance[i]
        except IndexError:
            raise ValueError('Requested time out of range of data file.')
        return C, dC


class ResidentGrid(object):
    """Basis matrix of a fixed set of points, resident on the device (Estimate.resident_grid)."""

    def __init__(self, est, gdlat, gdlon, gdalt, check_hull=True, gradient=None, hessian=None):
        if gradient is not None and gradient not in GRADIENT_FRAMES:
            raise ValueError("gradient must be None, 'model' or 'enu', not %r" % (gradient,))
        if hessian is not None and hessian not in GRADIENT_FRAMES:
            raise ValueError("hessian must be None, 'model' or 'enu', not %r" % (hessian,))
        shape = np.asarray(gdlat).shape
        lat, lon, alt = ravel_points(gdlat, gdlon, gdalt)

        def build(up, hp, F, tol):
            h, Q = est.model.handle(), lat.size
            dlat, dlon, dalt = up(lat), up(lon), up(alt)
            if gradient is not None:    # first: the calls that refuse a model or an order
                _lib.check(_lib.lib.vi_eval_grad_basis_f64(h, Q, dlat.ptr, dlon.ptr, dalt.ptr, hp, F, tol,
                                                           GRADIENT_FRAMES[gradient], self.dG.ptr), 'vi_eval_grad_basis_f64')
            if hessian is not None:
                _lib.check(_lib.lib.vi_eval_hess_basis_f64(h, Q, dlat.ptr, dlon.ptr, dalt.ptr, hp, F, tol,
                                                           GRADIENT_FRAMES[hessian], self.dH.ptr), 'vi_eval_hess_basis_f64')
            _lib.check(_lib.lib.vi_eval_basis_f64(h, Q, dlat.ptr, dlon.ptr, dalt.ptr, hp, F, tol, self.dY.ptr), 'vi_eval_basis_f64')
        self._setup(est, shape, lat.size, check_hull, gradient, build, hessian)

    def _setup(self, est, shape, Q, check_hull, gradient, build, hessian=None):
        """What every resident matrix shares: the state, the free-memory check, the allocation of dY (N x Q) and - with a
        gradient frame - dG, with a Hessian frame dH, and build(up, hull pointer, F, tol) filling them: up(host array[, dtype])
        gives a device copy in the scope of the set-up, freed when it ends whatever happens.  A failed set-up closes the
        object."""
        self.est = est
        self.frame = gradient
        self.hessian_frame = hessian
        self.shape = shape
        self.Q = Q
        ctx = est.model.ctx
        N = est.model.nbasis
        free, _ = ctx.mem_info()
        # the basis matrix, three times as much for the gradient basis, six times as much for the Hessian basis
        nmat = 1 + (0 if gradient is None else 3) + (0 if hessian is None else 6)
        if nmat * self.Q * N * 8 > 0.9 * free:
            also = [what for what, frame in (('gradient basis', gradient), ('Hessian basis', hessian)) if frame is not None]
            raise MemoryError('basis matrix%s of %d points x %d functions (%.1f GB) does not fit the device (%.1f GB free)'
                              % (''.join(' and ' + what for what in also), self.Q, N, nmat * self.Q * N * 8 / 1e9, free / 1e9))
        self.dY = self.dG = self.dH = None
        self._reduced = {}              # (axis, weight bytes) -> reduced basis on the device (evaluate_integrals)
        with ctx.scope() as dev:        # the temporaries of the set-up; dY, dG and dH are the object's
            try:
                self.dY = ctx.empty((N, self.Q))
                if gradient is not None:
                    self.dG = ctx.empty((N, 3, self.Q))
                if hessian is not None:
                    self.dH = ctx.empty((N, 6, self.Q))
                if self.Q == 0:
                    return
                eq, F, tol = est._hull_args(check_hull)
                build(dev.up, None if eq is None else dev.up(eq).ptr, F, tol)
                ctx.sync()
            except BaseException:
                self.close()            # the matrices (19 + 57 GB at the default order on 256^3) must not outlive a failed set-up
                raise

    def _open(self, dM):
        """dM, a matrix of this grid on the device, unless close() has given it back."""
        if dM is None:
            raise ValueError('this ResidentGrid has been closed')
        return dM

    def _coeffs(self, C):
        C = np.ascontiguousarray(C, dtype=np.float64)
        N = self.est.model.nbasis
        if C.ndim != 2 or C.shape[1] != N:
            raise ValueError('coefficients must have shape (T, %d)' % N)
        return C

    def _coeffs_at(self, times):
        """The coefficient rows of Estimate.get_C per time: (len(times), N)."""
        C = [np.asarray(self.est.get_C(t)[0], dtype=np.float64) for t in times]
        return np.array(C).reshape(len(times), self.est.model.nbasis)

    def _slab(self, T, nbytes):
        """The timesteps per slab: what a timestep takes on the device (`nbytes`) fits a quarter of the free device memory."""
        free, _ = self.est.model.ctx.mem_info()
        return int(max(1, min(T, (free // 4) // max(1, nbytes))))

    def _slabs(self, C, out, width):
        """The checks of the products with coefficients: C as (T, N) float64, `out` or a new array of shape (T,) + width, and
        the timesteps per slab of that output.  Returns (C, out, slab); slab 0: nothing to compute."""
        C = self._coeffs(C)
        T = C.shape[0]
        out = _check_out(out, (T,) + width)
        if T == 0 or self.Q == 0:
            return C, out, 0
        return C, out, self._slab(T, int(np.prod(width)) * 8)

    def _run(self, slab, X, outs, call, work=None, once=True, also=()):
        """The slab loop of every map on the grid.  X holds the inputs of the T timesteps row by row: uploaded once, or (once
        False) slab by slab.  `also`: further inputs with a row per timestep, uploaded slab by slab.  Per slab of tc timesteps
        from t0: call(tc, pointer to row t0 of X on the device, device outputs..., work buffer of `work` bytes unless None,
        device copies of the rows of `also`...), then the device outputs to outs[k][t0:t0 + tc].  Every device buffer is freed
        whatever happens."""
        ctx = self.est.model.ctx
        T = X.shape[0]
        with ctx.scope() as dev:
            dX = dev.up(X) if once else dev.empty((slab,) + X.shape[1:])
            dOs = [dev.empty((slab,) + o.shape[1:], o.dtype) for o in outs]
            dW = [] if work is None else [dev.empty(work, np.uint8)]
            dAs = [dev.empty((slab,) + a.shape[1:], a.dtype) for a in also]
            for t0 in range(0, T, slab):
                tc = min(slab, T - t0)
                if not once:
                    dX.upload(X[t0:t0 + tc])
                for a, dA in zip(also, dAs):
                    dA.upload(a[t0:t0 + tc])
                call(tc, dX.offset_ptr(t0 * X[0].size if once else 0), *dOs, *dW, *dAs)
                for o, dO in zip(outs, dOs):
                    part = o[t0:t0 + tc]
                    _lib.check(_lib.lib.vi_d2h(ctx.handle, part.ctypes.data_as(_lib.VOIDP), dO.ptr, part.nbytes), 'd2h')
        return outs

    def _products(self, dM, cols, C, out, slab):
        """out[t0:t0 + slab] = vi_eval_resident_f64 of the resident matrix dM (N rows, `cols` columns) with C, slab by slab."""
        h = self.est.model.handle()

        def call(tc, dC, dO):
            _lib.check(_lib.lib.vi_eval_resident_f64(h, cols, tc, dM.ptr, dC, dO.ptr), 'vi_eval_resident_f64')
        return self._run(slab, C, (out,), call)[0]

    def evaluate_coeffs(self, C, out=None):
        """out[t] = density of coefficient row C[t] on the grid; (T, Q) host array."""
        C, out, slab = self._slabs(C, out, (self.Q,))
        if slab == 0:
            return out
        return self._products(self._open(self.dY), self.Q, C, out, slab)

    def evaluate_gradients(self, C, out=None):
        """out[t, c] = component c of the gradient of the parameter with coefficient row C[t] on the grid; (T, 3, Q) host
        array, c in the grid's frame (see gradient).  The same product as evaluate_coeffs on the gradient basis: 3Q columns."""
        self._need_gradient_basis()
        C, out, slab = self._slabs(C, out, (3, self.Q))
        if slab == 0:
            return out
        return self._products(self._open(self.dG), 3 * self.Q, C, out, slab)

    def __call__(self, times):
        """Densities at the grid for a list of datetimes (Estimate.get_C per time): array (len(times),) + grid shape."""
        return self.evaluate_coeffs(self._coeffs_at(times)).reshape((len(times),) + tuple(self.shape))

    def _need_gradient_basis(self):
        if self.frame is None:
            raise ValueError("this ResidentGrid holds no gradient basis: build it with resident_grid(..., gradient='model') "
                             "or gradient='enu'")

    def gradient(self, times):
        """Gradient maps at the grid for a list of datetimes (coefficients of Estimate.get_C per time, as __call__ takes them):
        array (len(times), 3) + grid shape.  The components follow the frame the grid was built with: (z, theta, phi) of the
        model coordinates for gradient='model', (east, north, up) for gradient='enu'; np.moveaxis(x, 1, -1) gives the
        trailing-3 convention of Estimate.gradient.  NaN outside the hull and for a timestep whose coefficients are NaN, as
        the density; non-finite at the pole of the cap (sin theta' = 0), where the reference's formula divides by zero, as
        Estimate.gradient is."""
        self._need_gradient_basis()
        return self.evaluate_gradients(self._coeffs_at(times)).reshape((len(times), 3) + tuple(self.shape))

    def _need_hessian_basis(self):
        if self.hessian_frame is None:
            raise ValueError("this ResidentGrid holds no Hessian basis: build it with resident_grid(..., hessian='model') "
                             "or hessian='enu'")

    def evaluate_hessians(self, C, out=None):
        """out[t, k] = entry GRADCOV_PAIRS[k] of the Hessian of the parameter with coefficient row C[t] on the grid; (T, 6, Q)
        host array, packed (gradcov_matrix unpacks it), in the frame the grid was built with (hessian=).  The same product as
        evaluate_coeffs on the Hessian basis: 6Q columns."""
        self._need_hessian_basis()
        C, out, slab = self._slabs(C, out, (6, self.Q))
        if slab == 0:
            return out
        return self._products(self._open(self.dH), 6 * self.Q, C, out, slab)

    def hessian(self, times):
        """Hessian maps at the grid for a list of datetimes (coefficients of Estimate.get_C per time): array (len(times), 6) +
        grid shape, the six distinct entries in the order of GRADCOV_PAIRS, in 1/m^2 times the parameter's unit and in the frame
        of hessian= - see Estimate.hessian for what the entries are.  NaN outside the hull and for a timestep whose
        coefficients are NaN; non-finite at the pole of the cap."""
        self._need_hessian_basis()
        return self.evaluate_hessians(self._coeffs_at(times)).reshape((len(times), 6) + tuple(self.shape))

    def laplacian(self, times):
        """Laplacian maps at the grid for a list of datetimes: array (len(times),) + grid shape, the sum of the first three
        planes of hessian (the trace, the same in either frame)."""
        H = self.hessian(times)
        return (H[:, 0] + H[:, 1]) + H[:, 2]

    def _covariances(self, dC):
        """The covariances of a batch as (T, N, N) float64, checked."""
        dC = np.ascontiguousarray(dC, dtype=np.float64)
        N = self.est.model.nbasis
        if dC.ndim != 3 or dC.shape[1:] != (N, N):
            raise ValueError('covariances must have shape (T, %d, %d)' % (N, N))
        return dC

    def _covariances_at(self, times):
        """The covariances of Estimate.get_C per time: (len(times), N, N)."""
        if self.est.Covariance is None:
            raise ValueError('this Estimate holds no covariance (Covariance is None): no standard error to evaluate')
        N = self.est.model.nbasis
        dC = np.empty((len(times), N, N))
        for k, t in enumerate(times):
            dC[k] = self.est.get_C(t)[1]
        return dC

    def _forms(self, entry, dM, cols, dC, out, width):
        """What the maps of covariances share: the library's `entry` (columns, timesteps, resident matrix, covariances in,
        (T,) + width out) on the resident matrix dM with `cols` columns, out[t] of covariance dC[t], slab by slab - the
        covariances of a slab go up with it, not all T at once."""
        dC = self._covariances(dC)
        T, N = dC.shape[0], dC.shape[1]
        out = _check_out(out, (T,) + width)
        if T == 0 or self.Q == 0:
            return out
        slab = self._slab(T, (int(np.prod(width)) + N * N) * 8)
        h, dM = self.est.model.handle(), self._open(dM)

        def call(tc, dD, dO):
            _lib.check(getattr(_lib.lib, entry)(h, cols, tc, dM.ptr, dD, dO.ptr), entry)
        return self._run(slab, dC, (out,), call, once=False)[0]

    def evaluate_errors(self, dC, out=None):
        """out[t] = standard error sqrt(a^T dC[t] a) of the fitted parameter on the grid for each covariance dC[t] (as stored
        in /Coeffs/dC, not assumed symmetric); (T, Q) host array, NaN outside the hull, for a covariance holding a NaN and
        where the form is negative.  `out` as in evaluate_coeffs."""
        return self._forms('vi_eval_resident_err_f64', self.dY, self.Q, dC, out, (self.Q,))

    def error(self, times):
        """Standard-error maps at the grid for a list of datetimes (the covariance of Estimate.get_C per time, as __call__
        selects the coefficients): array (len(times),) + grid shape."""
        return self.evaluate_errors(self._covariances_at(times)).reshape((len(times),) + tuple(self.shape))

    def _index_at(self, index, T, axis):
        """`index` of evaluate_errors_at, checked on the host (column_points' rules, a row per covariance): C-contiguous
        int32 (T, M)."""
        index = np.asarray(index)
        column_points(self.shape, axis, index)
        if index.shape[0] != T:
            raise ValueError('index must have a row per covariance (%d), not %d' % (T, index.shape[0]))
        return np.ascontiguousarray(index, dtype=np.int32)

    def evaluate_errors_at(self, dC, index, axis=-1, out=None):
        """out[t, m] = standard error sqrt(a^T dC[t] a) of the fitted parameter at ONE point per column and covariance: the
        point at position index[t, m] along `axis` in column m (columns as in evaluate_peaks; column_points gives its flat
        index).  index: (T, M) integers in [-1, L), checked before anything goes to the device; (T, M) host array, NaN
        where index is -1 and where evaluate_errors gives NaN.  What np.take_along_axis picks from evaluate_errors(dC), bit
        for bit where both run on the matrix cores, without the (T, Q) map (vi_eval_resident_err_at_f64, kernel K2eg)."""
        axis, outer, L, inner = self._columns(axis)
        M = outer * inner
        dC = self._covariances(dC)
        T, N = dC.shape[0], dC.shape[1]
        index = self._index_at(index, T, axis)
        out = _check_out(out, (T, M))
        if T == 0 or self.Q == 0:
            out.fill(np.nan)                # (columns of length zero: no point to select)
            return out
        h, dY = self.est.model.handle(), self._open(self.dY)

        def call(tc, dD, dO, dI):
            _lib.check(_lib.lib.vi_eval_resident_err_at_f64(h, outer, L, inner, tc, dY.ptr, dD, dI.ptr, dO.ptr),
                       'vi_eval_resident_err_at_f64')
        return self._run(self._slab(T, M * 12 + N * N * 8), dC, (out,), call, once=False, also=(index,))[0]

    def errors_at(self, times, index, axis=-1):
        """Standard errors at one point per column for a list of datetimes (covariances as error takes them): index of shape
        (len(times),) + the grid shape without `axis`, positions along `axis` in [-1, L) - what peak returns -; the result has
        the same shape.  See evaluate_errors_at."""
        axis, rest = self._rest(times, axis)
        dC = self._covariances_at(times)
        index = np.asarray(index)
        if index.shape != rest:
            raise ValueError('index must have shape %r, not %r' % (rest, index.shape))
        M = int(np.prod(rest[1:], dtype=np.int64))
        return self.evaluate_errors_at(dC, index.reshape(len(times), M), axis=axis).reshape(rest)

    def evaluate_gradient_errors(self, dC, out=None):
        """out[t, c] = standard error sqrt(g_c^T dC[t] g_c) of component c of the gradient on the grid for each covariance
        dC[t]; (T, 3, Q) host array, c in the grid's frame, NaN as in evaluate_errors.  The same form as evaluate_errors on the
        gradient basis: 3Q columns."""
        self._need_gradient_basis()
        return self._forms('vi_eval_resident_err_f64', self.dG, 3 * self.Q, dC, out, (3, self.Q))

    def gradient_error(self, times):
        """Standard-error maps of the gradient components at the grid for a list of datetimes (covariances as error takes
        them): array (len(times), 3) + grid shape, components as gradient gives them."""
        self._need_gradient_basis()
        return self.evaluate_gradient_errors(self._covariances_at(times)).reshape((len(times), 3) + tuple(self.shape))

    def evaluate_gradient_covariances(self, dC, out=None):
        """out[t, k] = entry GRADCOV_PAIRS[k] = (c, d) of the covariance of the gradient on the grid for each covariance dC[t],
        g_c^T 1/2 (dC[t] + dC[t]^T) g_d; (T, 6, Q) host array, packed (gradcov_matrix unpacks it), components in the grid's
        frame.  All six NaN outside the hull and for a covariance holding a NaN; a negative diagonal entry of an indefinite
        dC[t] is returned as it is.  `out` as in evaluate_coeffs."""
        self._need_gradient_basis()
        return self._forms('vi_eval_resident_gradcov_f64', self.dG, self.Q, dC, out, (6, self.Q))

    def gradient_covariance(self, times):
        """Covariance maps of the gradient at the grid for a list of datetimes (covariances as error takes them): array
        (len(times), 3, 3) + grid shape, symmetric in the two component axes, components as gradient gives them.  The standard
        error of the gradient along a unit vector u is the square root of u^T cov u."""
        self._need_gradient_basis()
        packed = self.evaluate_gradient_covariances(self._covariances_at(times))
        cov = np.empty((len(times), 3, 3, self.Q))
        for k, (c, d) in enumerate(GRADCOV_PAIRS):
            cov[:, c, d] = cov[:, d, c] = packed[:, k]
        return cov.reshape((len(times), 3, 3) + tuple(self.shape))

    def _columns(self, axis):
        """The grid as (outer, L, inner) about `axis`: point q = (o * L + l) * inner + i, column m = o * inner + i."""
        return _grid_columns(self.shape, axis)

    def _rest(self, times, axis):
        """(axis, shape) of the column maps of peak and integrate: `axis` as _columns checks it, (len(times),) + the grid
        shape without that axis."""
        axis = self._columns(axis)[0]
        return axis, (len(times),) + tuple(self.shape[:axis]) + tuple(self.shape[axis + 1:])

    def evaluate_peaks(self, C, axis=-1, kind='max', out=None):
        """(value, index) of the peak of the density of coefficient row C[t] along `axis` of the grid, column by column:
        value (T, M) float64 and index (T, M) int32, M = Q / L columns in C order of the remaining axes - np.nanmax
        (kind='min': np.nanmin) of evaluate_coeffs(C) and the first position that attains it, (NaN, -1) for a column without
        a number (outside the hull, or NaN coefficients).  Computed on the device from the resident basis; the volume is
        not copied to the host and, with the reduced axis last, not formed.  `out`: a pair of preallocated arrays."""
        return self._peaks(C, None, axis, kind, out)

    def _peaks(self, C, dC, axis, kind, out):
        """What evaluate_peaks and evaluate_peak_errors share: (value, index) of the peaks of C and - with covariances dC, a
        matrix per row of C - the standard error at each peak; `out`: None or preallocated arrays, one per result.  Slab by slab
        the peak call, then the form at the index map it left on the device (vi_eval_resident_err_at_f64)."""
        axis, outer, L, inner = self._columns(axis)
        if kind not in PEAK_KINDS:
            raise ValueError("kind must be 'max' or 'min', not %r" % (kind,))
        M = outer * inner
        C = self._coeffs(C)
        T, N = C.shape
        names = ('value', 'index') if dC is None else ('value', 'index', 'error')
        if dC is not None:
            dC = self._covariances(dC)
            if dC.shape[0] != T:
                raise ValueError('covariances must have shape (%d, %d, %d): one per coefficient row' % (T, N, N))
        try:
            outs = (None,) * len(names) if out is None else tuple(out)
            if len(outs) != len(names) or (out is not None and any(o is None for o in outs)):
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError('out must be a %s (%s) of arrays' % ('pair' if dC is None else 'triple', ', '.join(names)))
        outs = tuple(_check_out(o, (T, M), np.int32 if name == 'index' else np.float64) for o, name in zip(outs, names))
        if T == 0 or self.Q == 0:
            for o, name in zip(outs, names):
                o.fill(-1 if name == 'index' else np.nan)       # (columns of length zero: nothing to select)
            return outs
        h, dY = self.est.model.handle(), self._open(self.dY)
        work = lambda tc: int(_lib.lib.vi_eval_resident_peak_work_bytes(h, outer, L, inner, tc))
        # the work space and the maps; with covariances their slab too
        slab = self._slab(T, work(1) + M * 12 + (0 if dC is None else M * 8 + N * N * 8))

        def call(tc, dCo, dV, dI, *rest):
            dW = rest[-1] if dC is None else rest[1]
            _lib.check(_lib.lib.vi_eval_resident_peak_f64(h, outer, L, inner, tc, dY.ptr, dCo, PEAK_KINDS[kind], dV.ptr, dI.ptr,
                                                          dW.ptr, dW.nbytes), 'vi_eval_resident_peak_f64')
            if dC is not None:
                dE, _, dD = rest
                _lib.check(_lib.lib.vi_eval_resident_err_at_f64(h, outer, L, inner, tc, dY.ptr, dD.ptr, dI.ptr, dE.ptr),
                           'vi_eval_resident_err_at_f64')
        return self._run(slab, C, outs, call, work=work(slab), also=() if dC is None else (dC,))

    def peak(self, times, axis=-1, kind='max'):
        """Peak maps for a list of datetimes (coefficients of Estimate.get_C per time, as __call__ takes them): (value, index),
        each (len(times),) + the grid shape without `axis`.  On a (lat, lon, alt) grid with the default axis: the peak of the
        parameter along altitude and the altitude index where it sits."""
        axis, rest = self._rest(times, axis)
        val, idx = self.evaluate_peaks(self._coeffs_at(times), axis=axis, kind=kind)
        return val.reshape(rest), idx.reshape(rest)

    def evaluate_peak_errors(self, C, dC, axis=-1, kind='max', out=None):
        """(value, index, error): value and index as evaluate_peaks(C, axis, kind) gives them, bit for bit, and error (T, M)
        float64, the standard error sqrt(a^T dC[t] a) of the parameter at the peak of column m - first-order, the position
        taken as given; the uncertainty of the position itself is not part of it.  NaN where index is -1 and where
        evaluate_errors gives NaN at that point.  dC: (T, N, N), a covariance per row of C.  The index map goes from the peak
        call to the form call on the device; neither the density nor the error volume is formed (with the reduced axis last)
        or copied to the host.  `out`: a triple of preallocated arrays."""
        return self._peaks(C, dC, axis, kind, out)

    def peak_error(self, times, axis=-1, kind='max'):
        """Peak maps with their standard errors for a list of datetimes (coefficients and covariances of Estimate.get_C per
        time): (value, index, error), each (len(times),) + the grid shape without `axis`; value and index are those of peak.
        On a (lat, lon, alt) grid: NmF2, the altitude index of hmF2 and the standard error of NmF2."""
        axis, rest = self._rest(times, axis)
        dC = self._covariances_at(times)
        val, idx, err = self.evaluate_peak_errors(self._coeffs_at(times), dC, axis=axis, kind=kind)
        return val.reshape(rest), idx.reshape(rest), err.reshape(rest)

    def evaluate_crossings(self, C, level, axis=-1, which='first', direction='any', out=None):
        """index (T, M) int32, M = Q / L columns as in evaluate_peaks: the position l of the first (which='last': last) pair of
        neighbours (l, l + 1) along `axis` at which the density of coefficient row C[t] crosses `level` - both samples numbers
        and direction='up': f[l] <= level <= f[l + 1]; 'down': f[l] >= level >= f[l + 1]; 'any': either -, -1 for a column
        without such a pair: outside the hull, NaN coefficients, a NaN level, an axis of length 1.  level: a scalar, or
        anything that broadcasts to (T, M).  Computed on the device from the resident basis, slab by slab
        (vi_eval_resident_cross_f64); the volume is not copied to the host.  level_brackets turns the map into the brackets
        of Estimate.level_height.  `out`: a preallocated array."""
        axis, outer, L, inner = self._columns(axis)
        if which not in CROSSING_WHICH:
            raise ValueError("which must be 'first' or 'last', not %r" % (which,))
        if direction not in CROSSING_DIRECTIONS:
            raise ValueError("direction must be 'any', 'up' or 'down', not %r" % (direction,))
        M = outer * inner
        C = self._coeffs(C)
        T = C.shape[0]
        try:
            level = np.ascontiguousarray(np.broadcast_to(np.asarray(level, dtype=np.float64), (T, M)))
        except ValueError:
            raise ValueError('level must be a scalar or broadcast to the shape %r' % ((T, M),))
        out = _check_out(out, (T, M), np.int32)
        if T == 0 or self.Q == 0:
            out.fill(-1)                    # (columns of length zero: no pair of neighbours)
            return out
        h, dY = self.est.model.handle(), self._open(self.dY)
        slab = self._slab(T, self.Q * 8 + M * 12)
        work = slab * self.Q * 8

        def call(tc, dCo, dI, dW, dL):
            _lib.check(_lib.lib.vi_eval_resident_cross_f64(h, outer, L, inner, tc, dY.ptr, dCo, dL.ptr, CROSSING_WHICH[which],
                                                           CROSSING_DIRECTIONS[direction], dI.ptr, dW.ptr, dW.nbytes),
                       'vi_eval_resident_cross_f64')
        return self._run(slab, C, (out,), call, work=work, also=(level,))[0]

    def crossing(self, times, level, axis=-1, which='first', direction='any'):
        """Crossing maps for a list of datetimes (coefficients of Estimate.get_C per time): the index map of
        evaluate_crossings, (len(times),) + the grid shape without `axis`; level a scalar or anything that broadcasts to that
        shape.  On a (lat, lon, alt) grid with the default axis and direction='up': the altitude index below the bottomside
        crossing of the level - est.level_height(times, lat2d, lon2d, level, *level_brackets(alt, index)) refines it."""
        axis, rest = self._rest(times, axis)
        try:
            level = np.broadcast_to(np.asarray(level, dtype=np.float64), rest)
            level = level.reshape(len(times), int(np.prod(rest[1:], dtype=np.int64)))
        except ValueError:
            raise ValueError('level must be a scalar or broadcast to the shape %r' % (rest,))
        return self.evaluate_crossings(self._coeffs_at(times), level, axis=axis, which=which, direction=direction).reshape(rest)

    @staticmethod
    def _weights(L, weights):
        if weights is None:
            return np.ones(L)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.ndim != 1 or w.shape[0] != L:
            raise ValueError('weights must be a 1-D array of the length of the axis (%d)' % L)
        if not np.isfinite(w).all():
            raise ValueError('weights must be finite')
        return w

    def _reduced_basis(self, axis, outer, L, inner, w):
        """The device matrix Yr (N, M) of vi_reduce_basis_f64 for (axis, weights), built once and kept until close()."""
        key = (axis, w.tobytes())
        dYr = self._reduced.get(key)
        if dYr is None:
            ctx = self.est.model.ctx
            while len(self._reduced) >= REDUCED_BASES:          # the oldest entry goes: weights that change with every call
                self._reduced.pop(next(iter(self._reduced))).free()
            nbytes = self.est.model.nbasis * outer * inner * 8
            free, _ = ctx.mem_info()
            if nbytes > 0.9 * free:
                raise MemoryError('reduced basis of %d columns x %d functions (%.1f GB) does not fit the device (%.1f GB free)'
                                  % (outer * inner, self.est.model.nbasis, nbytes / 1e9, free / 1e9))
            with ctx.scope() as dev:
                dYr, dw = dev.empty((self.est.model.nbasis, outer * inner)), dev.up(w)
                _lib.check(_lib.lib.vi_reduce_basis_f64(self.est.model.handle(), outer, L, inner, self.dY.ptr, dw.ptr, dYr.ptr),
                           'vi_reduce_basis_f64')
                ctx.sync()
                self._reduced[key] = dev.detach(dYr)        # the set-up succeeded: the grid's until close()
        return dYr

    def evaluate_integrals(self, C, weights=None, axis=-1, out=None):
        """out[t, m] = sum_l weights[l] * density[t, m, l] over the points of column m along `axis` that are inside the hull;
        (T, M) host array, M as in evaluate_peaks.  weights: length of the axis, default ones (trapezoid weights in metres
        give a vertical integral).  NaN for a column without a point inside and for a timestep with NaN coefficients.  The
        sum is linear in the coefficients: the basis is summed along the axis once per (axis, weights) - a matrix 1 / L of
        the basis, kept on the device until close(), the last REDUCED_BASES of them - and every call is the density product on M points.  "Inside" is read
        from row 0 of the basis, as the density product reads it."""
        axis, outer, L, inner = self._columns(axis)
        w = self._weights(L, weights)
        M = outer * inner
        C, out, slab = self._slabs(C, out, (M,))
        if slab == 0:
            out.fill(np.nan)                # (columns of length zero: no point inside)
            return out
        self._open(self.dY)
        return self._products(self._reduced_basis(axis, outer, L, inner, w), M, C, out, slab)

    def integrate(self, times, weights=None, axis=-1):
        """Weighted column sums for a list of datetimes (coefficients of Estimate.get_C per time): (len(times),) + the grid
        shape without `axis`; see evaluate_integrals."""
        axis, rest = self._rest(times, axis)
        return self.evaluate_integrals(self._coeffs_at(times), weights=weights, axis=axis).reshape(rest)

    def evaluate_integral_errors(self, dC, weights=None, axis=-1, out=None):
        """out[t, m] = standard error of evaluate_integrals' weighted column sum for each covariance dC[t]: sqrt(b^T dC[t] b)
        with b column m of the reduced basis of (axis, weights) - the matrix evaluate_integrals multiplies, built once and kept
        with it - by the form of evaluate_errors on M columns (vi_eval_resident_err_f64).  (T, M) host array in the
        parameter's unit times the weights' unit; NaN for a column without a point inside the hull, for a covariance holding
        a NaN and where the form is negative.  weights, axis as in evaluate_integrals, `out` as in evaluate_coeffs."""
        axis, outer, L, inner = self._columns(axis)
        w = self._weights(L, weights)
        M = outer * inner
        dC = self._covariances(dC)
        out = _check_out(out, (dC.shape[0], M))
        if dC.shape[0] == 0 or self.Q == 0:
            out.fill(np.nan)                # (columns of length zero: no point inside)
            return out
        self._open(self.dY)
        return self._forms('vi_eval_resident_err_f64', self._reduced_basis(axis, outer, L, inner, w), M, dC, out, (M,))

    def integrate_error(self, times, weights=None, axis=-1):
        """Standard errors of integrate's weighted column sums for a list of datetimes (covariances as error takes them):
        (len(times),) + the grid shape without `axis`; see evaluate_integral_errors."""
        axis, rest = self._rest(times, axis)
        return self.evaluate_integral_errors(self._covariances_at(times), weights=weights, axis=axis).reshape(rest)

    def close(self):
        """Give the basis matrix (the gradient basis, the Hessian basis, the reduced bases of evaluate_integrals) back to the device
        (idempotent).  Also runs on `with est.resident_grid(...) as g:` exit and when the object is collected."""
        for name in ('dY', 'dG', 'dH'):
            a = getattr(self, name, None)
            setattr(self, name, None)
            if a is not None:
                a.free()
        red = getattr(self, '_reduced', None)
        if red:
            for a in red.values():
                a.free()
            red.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:               # interpreter shutdown: the library may already be gone
            pass


class ResidentRays(ResidentGrid):
    """Ray-integrated basis of a fixed set of rays, resident on the device (Estimate.resident_rays): a ResidentGrid whose
    "points" are the rays and whose matrix dY is B[n, p] = (s1 - s0) / 2 |b - a| sum_i w_i basis_n(a_p + s_i (b_p - a_p)), in
    metres.  Everything a ResidentGrid does with the basis of its points holds for the line integrals, in the parameter's unit
    times metres:
      r(times), evaluate_coeffs(C)    the integrals of slant at one time per image, (T,) + ray shape, as one product (K2r);
      error(times), evaluate_errors   their standard errors sqrt(b^T dC b) (K2e) - the parameter's unit times metres too;
      peak, evaluate_peaks            the largest (smallest) integral along an axis of the ray shape and where it sits;
      integrate, evaluate_integrals   weighted sums of the integrals along an axis, over the rays that enter the hull;
      crossing, evaluate_crossings    where the integrals cross a level along an axis of the ray shape.
    NaN for a ray that does not enter the hull or has a non-finite end point, 0 for a segment of length zero inside it.
    peak_error, errors_at and integrate_error give the standard errors of those maxima and weighted sums in the same way.
    It holds no gradient basis: gradient and evaluate_gradients raise."""

    def __init__(self, est, start, end, nodes=64, rule=None, coords='geodetic', check_hull=True):
        x, wq, shape, a, b = slant_rays(start, end, nodes, rule, coords)
        P = a.shape[1]
        self._length = np.linalg.norm(b - a, axis=0)
        self._s = np.empty((2, P))

        def build(up, hp, F, tol):
            da, db, dx, dq, dS = up(a), up(b), up(x), up(wq), up(self._s)
            _lib.check(_lib.lib.vi_eval_slant_basis_f64(est.model.handle(), P, da.ptr, db.ptr, hp, F, tol, x.size, dx.ptr, dq.ptr,
                                                        self.dY.ptr, dS.ptr), 'vi_eval_slant_basis_f64')
            self._s = dS.download()
        self._setup(est, shape, P, check_hull, None, build)

    def basis(self):
        """The matrix itself on the host, (N,) + ray shape, in the parameter-free unit metres: the linear forward operator of
        the rays - np.tensordot(C, r.basis(), 1) is the line integral of the model with coefficients C along every ray - in the
        public order of Model.basis.  NaN in all N entries of a ray that does not enter the hull."""
        return self._open(self.dY).download().reshape((self.est.model.nbasis,) + tuple(self.shape))

    @property
    def chords(self):
        """(d0, d1), each of the ray shape: the distances from `start` in metres between which the ray is inside the hull,
        NaN for a miss - as Estimate.slant(chord=True) returns them."""
        return (self._s[0] * self._length).reshape(self.shape), (self._s[1] * self._length).reshape(self.shape)
