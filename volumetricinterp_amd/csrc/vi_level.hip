// Level crossings of the sphharmlag model for gfx950: per column (lat, lon) and coefficient row the height between two bounds at
// which the fitted parameter crosses a given level along the geodetic normal - the reflection height of a sounding frequency,
// the half-peak heights of a layer, an isodensity surface -, by a safeguarded Newton search on the analytic model.  A root search
// needs no curvature: the value and the slope df/dh = u . grad f, u the `up` row of the point's east-north-up matrix (enu_frame),
// come from ONE gradient walk (grad_point, vi_sph_device.h), whose factors hold the value too - tz L0k is -(50/RE) times the
// basis function's value, zfac being -0.5 e 100/RE.  The reference has no counterpart.
//   k_level_sph<LCAP, KCAP>, a lane per column, the grid (blocks over Q, rows): a workgroup reads one coefficient row, wave-uniform.
//   The lane keeps four sums, each added in the order of the walk,
//       S0 = sum c tz L0k,  S1 = sum c tz L1k,  S2 = sum c tt L0k,  S3 = sum c tp L0k,
//   and after the walk f = -(RE/50) S0, d1 = u . (S0 + 2 S1, S2, S3).  With L the level of the point:
//     a = lo; b = hi
//     not finite(lat, lon, a, b, L), not a < b, or an end outside the hull: status 3, stop
//     fa = f(a) - L, da = d1(a);  fb = f(b) - L, db = d1(b)                (two walks, the walk of the loop)
//     fa or fb not finite: status 3, stop
//     fa == 0: h = a, report f, da, status 0, it = 0, stop.   fb == 0: the same at b.
//     fa, fb of one sign (by comparisons, not by their product): status 1, stop
//     h = a - fa (b - a)/(fb - fa);  not (a < h < b): h = (a + b)/2;   done = false; it = 0
//     loop:  f, d1 at h;  phi = f - L
//            phi or d1 not finite: status 3, stop
//            phi == 0 or done or it == max_iter: stop - status 0 if phi == 0 or done, else 2
//            it += 1;  (phi > 0) == (fa > 0) ? a = h : b = h
//            hn = d1 != 0 ? h - phi/d1 : NaN;  not (a < hn < b): hn = (a + b)/2
//            done = |hn - h| <= tol;  h = hn
//   Every pass of the loop either stops the lane or adds one to `it`, which max_iter (at most 10 000) bounds.  A lane that has
//   stopped stores its results at once and is frozen: it walks on with the wave at its last height and updates nothing; the wave
//   leaves when no lane is searching.  A point's bits depend on its column, row, level, bracket, max_iter and tol alone.
// The hull's byte mask is read once for BOTH ends of the bracket (plane 0: lower ends, plane 1: upper ends).  Later iterates need
// no test: a column's geodetic normal is a straight line in ECEF and the hull test is an intersection of half-spaces, a convex
// set, so every point between two points inside is inside.
//   k_cross_columns / k_cross_columns_last: on a slab (T, outer, L, inner) of densities the index l of the first (last) pair of
//   neighbours (l, l + 1) along the axis that are both numbers and hold the column's level between them - the grid bracket the
//   search above starts from (vi_eval_resident_cross_f64, vi_resident.hip).
#include <cmath>

#include "vi_sph_device.h"
#include "vi_eval_host.h"

namespace {

// the four sums of a lane
struct LevelSink {
    const double* __restrict__ Cv;
    double s0, s1, s2, s3;
    __device__ __forceinline__ void term(int n, double tz, double tt, double tp, double L0k, double L1k)
    {
        const double cf = Cv[n];
        const double cz = cf * tz;
        s0 = fma(cz, L0k, s0);
        s1 = fma(cz, L1k, s1);
        s2 = fma(cf * tt, L0k, s2);
        s3 = fma(cf * tp, L0k, s3);
    }
};

// lat, lon: the columns (plane 0 of the entry's arrays); ends: (2, PQ) planar, lo then hi; mask: (2, PQ) bytes or null.
// out: (3, PQ) planar - h, f, df/dh; point p = t*Q + q of row t = blockIdx.y writes column p of every plane, status[p] and
// iter[p] and nothing else, lanes past Q nothing at all.
template <int LCAP, int KCAP>
__global__ __launch_bounds__(BLOCK) void k_level_sph(SphDev M, int64_t Q, int64_t PQ, const double* __restrict__ lat,
                                                     const double* __restrict__ lon, const double* __restrict__ ends,
                                                     const double* __restrict__ level, const double* __restrict__ C,
                                                     const unsigned char* __restrict__ mask, int max_iter, double tol,
                                                     double* __restrict__ out, int32_t* __restrict__ status,
                                                     int32_t* __restrict__ iter)
{
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t p = (int64_t)blockIdx.y * Q + (q < Q ? q : Q - 1);
    const bool live = q < Q;
    const double la = lat[p], lg = lon[p], Lv = level[p];
    double a = ends[p], b = ends[PQ + p];
    bool ok = isfinite(la) && isfinite(lg) && isfinite(a) && isfinite(b) && isfinite(Lv) && a < b;
    if (mask) ok = ok && mask[p] != 0 && mask[PQ + p] != 0;
    const double nan = __builtin_nan("");
    // what a lane leaves when it stops
    auto store = [&](int st, double h, double f, double d1, int it) {
        out[p] = h;
        out[PQ + p] = f;
        out[2 * PQ + p] = d1;
        status[p] = st;
        if (iter) iter[p] = it;
    };
    if (live && !ok) store(3, nan, nan, nan, 0);
    bool active = live && ok;               // still searching
    if (!__any(active)) return;             // no lane of the wave has a search to run: no walk
    const double vfac = -(M.RE / 50.0);
    int phase = 0;                          // 0: the walk at a, 1: the walk at b, 2: the iteration
    double h = a;
    double fra = 0.0, da = 0.0;             // f and d1 at the lower end
    bool sa = false, done = false;          // sa: f(a) - L > 0
    int it = 0;
    LevelSink sink;
    sink.Cv = C + (int64_t)blockIdx.y * M.N;
    for (;;) {
        const Geom g = sph_geom(M, la, lg, h);
        sink.s0 = sink.s1 = sink.s2 = sink.s3 = 0.0;
        grad_point<LCAP, KCAP>(M, g, sink);
        if (active) {
            double F[9];
            enu_frame(M, g, la, lg, F);     // after the walk: nothing of it is live across the chains
            const double* u = F + 6;        // up
            const double f = vfac * sink.s0;
            const double d1 = fma(u[0], sink.s0 + 2.0 * sink.s1, fma(u[1], sink.s2, u[2] * sink.s3));
            if (phase == 0) {
                fra = f;
                da = d1;
                h = b;
                phase = 1;
            } else if (phase == 1) {
                const double fa = fra - Lv, fb = f - Lv;
                if (!(isfinite(fa) && isfinite(fb))) {
                    store(3, nan, nan, nan, 0);
                    active = false;
                } else if (fa == 0.0) {
                    store(0, a, fra, da, 0);
                    active = false;
                } else if (fb == 0.0) {
                    store(0, b, f, d1, 0);
                    active = false;
                } else if ((fa > 0.0) == (fb > 0.0)) {
                    store(1, nan, nan, nan, 0);
                    active = false;
                } else {
                    sa = fa > 0.0;
                    h = a - fa * (b - a) / (fb - fa);
                    if (!(a < h && h < b)) h = 0.5 * (a + b);
                    phase = 2;
                }
            } else {
                const double phi = f - Lv;
                if (!(isfinite(phi) && isfinite(d1))) {
                    store(3, nan, nan, nan, it);
                    active = false;
                } else if (phi == 0.0 || done || it >= max_iter) {
                    store((phi == 0.0 || done) ? 0 : 2, h, f, d1, it);
                    active = false;
                } else {
                    ++it;
                    if ((phi > 0.0) == sa) a = h;
                    else b = h;
                    double hn = d1 != 0.0 ? h - phi / d1 : nan;
                    if (!(a < hn && hn < b)) hn = 0.5 * (a + b);
                    done = fabs(hn - h) <= tol;
                    h = hn;
                }
            }
        }
        if (!__any(active)) return;
    }
}

// ---- crossings along an axis of a (T, outer, L, inner) slab of densities -------------------------------------------------------
// whether the neighbours f0, f1 hold the level between them in the asked direction (1 up, 2 down, 0 either): comparisons only,
// so that a NaN sample or a NaN level makes no crossing
__device__ __forceinline__ bool crosses(double f0, double f1, double Lv, int direction)
{
    const bool up = f0 <= Lv && Lv <= f1, down = f0 >= Lv && Lv >= f1;
    return direction == 1 ? up : direction == 2 ? down : (up || down);
}

// inner > 1: one thread per column, neighbouring threads neighbouring i - every load of a wave is contiguous
__global__ __launch_bounds__(256) void k_cross_columns(int64_t outer, int64_t L, int64_t inner, int64_t T, int last, int direction,
                                                       const double* __restrict__ in, const double* __restrict__ level,
                                                       int* __restrict__ idx)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, M = outer * inner;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < T * M; e += stride) {
        const int64_t tm = e / inner, i = e - tm * inner;          // tm = t * outer + o
        const double* src = in + tm * L * inner + i;
        const double Lv = level[e];
        int bi = -1;
        if (L > 1) {
            double f0 = src[0];
            for (int64_t l = 0; l + 1 < L; ++l) {
                const double f1 = src[(l + 1) * inner];
                if (crosses(f0, f1, Lv, direction) && (last || bi < 0)) bi = (int)l;
                f0 = f1;
            }
        }
        idx[e] = bi;
    }
}

// inner == 1: W lanes (a power of two, at most a wave) per column, lane s at the pairs l = s, s + W, ... - contiguous loads of
// src[l] and of src[l + 1] -, then a butterfly over the W lanes: the smallest found index (first) or the largest (last).
// ncol = T * M columns of L contiguous values.
__global__ __launch_bounds__(256) void k_cross_columns_last(int64_t ncol, int64_t L, int W, int last, int direction,
                                                            const double* __restrict__ in, const double* __restrict__ level,
                                                            int* __restrict__ idx)
{
    const int64_t gt = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int sub = (int)(gt & (W - 1));
    const int64_t grp = gt / W, ngrp = (int64_t)gridDim.x * blockDim.x / W;
    const int none = last ? -1 : 0x7fffffff;
    for (int64_t c0 = 0; c0 < ncol; c0 += ngrp) {                  // the same trip count in every lane: the shuffles below
        const int64_t c = c0 + grp;
        int bi = none;
        if (c < ncol) {
            const double* src = in + c * L;
            const double Lv = level[c];
            for (int64_t l = sub; l + 1 < L; l += W)
                if (crosses(src[l], src[l + 1], Lv, direction) && (last || bi == none)) bi = (int)l;
        }
        for (int off = 1; off < W; off <<= 1) {
            const int oi = __shfl_xor(bi, off);
            bi = last ? (oi > bi ? oi : bi) : (oi < bi ? oi : bi);
        }
        if (sub == 0 && c < ncol) idx[c] = bi == none ? -1 : bi;
    }
}

unsigned cross_blocks(int64_t threads)
{
    const int64_t b = (threads + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > (1 << 20) ? (1 << 20) : b));
}

}  // namespace

// idx (T, outer * inner) of a slab of densities (T, outer, L, inner) and the levels (T, outer * inner): k_cross_columns /
// k_cross_columns_last.  which: 0 the first pair, 1 the last; direction: 0 any, 1 up, 2 down.
int vi_cross_columns(vi_ctx* c, int64_t outer, int64_t L, int64_t inner, int64_t T, int which, int direction, const double* d_in,
                     const double* d_level, int32_t* d_idx)
{
    if (inner == 1) {
        int W = 1;
        while (W < 64 && W < L - 1) W <<= 1;
        return vi_launch(k_cross_columns_last, dim3(cross_blocks(T * outer * W)), dim3(256), 0, c->stream, T * outer, L, W, which,
                         direction, d_in, d_level, d_idx);
    }
    return vi_launch(k_cross_columns, dim3(cross_blocks(T * outer * inner)), dim3(256), 0, c->stream, outer, L, inner, T, which,
                     direction, d_in, d_level, d_idx);
}

extern "C" int vi_eval_level_f64(vi_model* m, int64_t T, int64_t Q, const double* d_lat, const double* d_lon, const double* d_ends,
                                 const double* d_level, const double* d_C, const double* d_hull_eq, int32_t F, double hull_tol,
                                 int32_t max_iter, double tol, double* d_out, int32_t* d_status, int32_t* d_iter)
{
    const char* who = "vi_eval_level_f64";
    VI_REQUIRE(m && d_lat && d_lon && d_ends && d_level && d_C && d_out && d_status, "null argument");
    VI_REQUIRE(T >= 0 && Q >= 0 && F >= 0, "negative size");
    VI_REQUIRE_HULL(F, d_hull_eq);
    VI_REQUIRE(max_iter >= 0 && max_iter <= 10000, "max_iter must lie in [0, 10000]");
    VI_REQUIRE(std::isfinite(tol) && tol > 0.0, "tol must be finite and positive");
    VI_REQUIRE(T == 0 || Q <= (INT64_MAX / 2) / T, "2 * T * Q overflows");
    int rc = grad_model_check(m, who);
    if (rc != VI_OK) return rc;
    rc = at_grad_cap(m, who, [](auto, auto) { return (int)VI_OK; });          // the order, before anything is launched
    if (rc != VI_OK || T == 0 || Q == 0) return rc;
    VI_HIP(hipSetDevice(m->ctx->device));
    const int64_t PQ = T * Q;
    // one hull pass for both ends of every bracket: 2 PQ points, the columns repeated in the second plane of d_lat and d_lon
    if (F > 0 && (rc = prepare_call(m, 2 * PQ, d_lat, d_lon, d_ends, d_hull_eq, F, hull_tol, 0, nullptr)) != VI_OK) return rc;
    const unsigned char* d_mask = F > 0 ? m->d_mask : nullptr;
    EvalTimer timer(m->ctx);
    // a grid's second dimension holds 65 535 rows: more go in slices, each on its own part of the arrays
    return for_chunks(T, 65535, [&](int64_t t0, int64_t tc) {
        const int64_t o = t0 * Q;
        return at_grad_cap(m, who, [&](auto lc, auto kc) {
            return vi_launch(k_level_sph<lc, kc>, dim3(nblocks(Q, BLOCK), (unsigned)tc), dim3(BLOCK), 0, m->ctx->stream, m->sph, Q,
                             PQ, d_lat + o, d_lon + o, d_ends + o, d_level + o, d_C + t0 * m->sph.N,
                             d_mask ? d_mask + o : nullptr, (int)max_iter, tol, d_out + o, d_status + o,
                             d_iter ? d_iter + o : nullptr);
        });
    });
}
