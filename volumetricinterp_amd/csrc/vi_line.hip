// Peaks and level crossings of the sphharmlag model along straight rays for gfx950: per ray a -> b (ECEF metres) and coefficient
// row the distance s from a, between two bounds, at which the fitted parameter has its maximum (or minimum) along the ray, or
// crosses a given level - the profile peak along a radar beam, the point where an oblique sounder's ray meets the plasma
// frequency, the place where a line of sight enters a patch.  The searches of vi_peak.hip and vi_level.hip, statement by
// statement, with the distance s along the line in place of the height h along a column's geodetic normal.  The reference has no
// counterpart.
//   geometry   d = b - a, len = sqrt(dx^2 + dy^2 + dz^2), u = d / len; the point at s is (fma(s, ux, ax), fma(s, uy, ay),
//              fma(s, uz, az)) and goes into sph_geom_ecef: no geodetic step anywhere.  After the walk u is turned as sph_geom_ecef
//              turns the position (Rodrigues, +theta0) and met with the unit vectors r', theta', phi' of the rotated spherical
//              coordinates at the point - the three dot products of enu_frame for the one direction u - : w, the components of u
//              in the orthonormal frame of the gradient.  Nothing of it lives across the chains.
//   derivatives  The Hessian of grad_hess_point is the tensor of second covariant derivatives in that frame, and along a straight
//              line the direction is constant (its covariant derivative along itself is zero), so
//                  df/ds = w . grad f,    d2f/ds2 = w^T H w      exactly - no term in the first derivative.
//   k_line_peak_sph<LCAP, KCAP>   the peak_point walk (ten sums) and the iteration of k_peak_sph
//   k_line_level_sph<LCAP, KCAP>  the grad_point walk (four sums) and the iteration of k_level_sph: the walk at lo, the walk at hi,
//              the secant start, safeguarded Newton - one copy of the walk for the three phases
//   both       a lane per ray, the grid (blocks over P, rows): a workgroup reads one coefficient row, wave-uniform.  A lane that
//              has stopped stores its results at once and is frozen; the wave leaves when no lane is searching; every pass of a
//              loop stops the lane or adds one to `it`, which max_iter (at most 10 000) bounds.  A ray's bits depend on the ray,
//              its row, its bracket (start, level), kind, max_iter and tol alone.
//   hull       each lane tests the two ends of ITS bracket, the points at lo and at hi, against the F half-spaces of the caller's
//              list, fma(nx, X, fma(ny, Y, fma(nz, Z, off))) <= tol as K2l's clip has it; the list is wave-uniform, the loop
//              plain.  An end outside: status 3.  The iterates stay between two points inside a convex set, so there is no mask
//              pass, no test of a later iterate and no "left the hull" status.  F = 0: no test.
#include <cmath>

#include "vi_sph_device.h"
#include "vi_eval_host.h"

namespace {

// the ten sums of a peak lane (those of k_peak_sph)
struct LinePeakSink {
    const double* __restrict__ Cv;
    double f, d[3], h[6];
    __device__ __forceinline__ void term(int n, double fn, const double* dn, const double* hn)
    {
        const double cf = Cv[n];
        f = fma(fn, cf, f);
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = fma(dn[k], cf, d[k]);
#pragma unroll
        for (int k = 0; k < 6; ++k) h[k] = fma(hn[k], cf, h[k]);
    }
};

// the four sums of a level lane (those of k_level_sph)
struct LineLevelSink {
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

// A ray of the launch: a, the unit direction and the length.  Every product stands in an fma or alone, so that the same ray has
// the same bits wherever this is inlined.
struct Line {
    double ax, ay, az, ux, uy, uz, len;
};

__device__ __forceinline__ Line line_of(int64_t p, int64_t P, const double* __restrict__ a, const double* __restrict__ b)
{
    Line y;
    y.ax = a[p];
    y.ay = a[P + p];
    y.az = a[2 * P + p];
    const double dx = b[p] - y.ax, dy = b[P + p] - y.ay, dz = b[2 * P + p] - y.az;
    y.len = sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
    y.ux = dx / y.len;
    y.uy = dy / y.len;
    y.uz = dz / y.len;
    return y;
}

// a has to be finite, and b with it: len is finite and positive only then (a NaN or an infinite difference makes it NaN or inf)
__device__ __forceinline__ bool line_ok(const Line& y)
{
    return isfinite(y.ax) && isfinite(y.ay) && isfinite(y.az) && isfinite(y.len) && y.len > 0.0;
}

__device__ __forceinline__ Geom line_geom(const SphDev& M, const Line& y, double s)
{
    return sph_geom_ecef(M, fma(s, y.ux, y.ax), fma(s, y.uy, y.ay), fma(s, y.uz, y.az));
}

// whether the point at s is inside every half-space of the list: K2l's expression and criterion.  A NaN point is outside.
__device__ __forceinline__ bool line_inside(const Line& y, double s, const double* __restrict__ eq, int F, double tol)
{
    const double X = fma(s, y.ux, y.ax), Y = fma(s, y.uy, y.ay), Z = fma(s, y.uz, y.az);
    bool in = true;
    for (int f = 0; f < F; ++f) {
        const double nx = eq[4 * f], ny = eq[4 * f + 1], nz = eq[4 * f + 2], off = eq[4 * f + 3];
        in = in && fma(nx, X, fma(ny, Y, fma(nz, Z, off))) <= tol;
    }
    return in;
}

// w[c] = u . (r', theta', phi')_c at the point g: u rotated as sph_geom_ecef rotates the position, then enu_frame's three dot
// products with the unit vectors of the rotated spherical coordinates
__device__ __forceinline__ void line_frame(const SphDev& M, const Geom& g, const Line& y, double* w)
{
    const double st = sqrt(g.Rx * g.Rx + g.Ry * g.Ry) / (M.RE * (g.z / 100.0 + 1.0));
    const double omc = 1.0 - M.rc;
    const double kd = M.kx * y.ux + M.ky * y.uy;
    const double wx = y.ux * M.rc + (M.ky * y.uz) * M.rs + M.kx * kd * omc;
    const double wy = y.uy * M.rc + (-M.kx * y.uz) * M.rs + M.ky * kd * omc;
    const double wz = y.uz * M.rc + (M.kx * y.uy - M.ky * y.ux) * M.rs;
    const double wh = wx * g.cphi + wy * g.sphi;
    w[0] = st * wh + g.x * wz;
    w[1] = g.x * wh - st * wz;
    w[2] = wy * g.cphi - wx * g.sphi;
}

// a, b: (3, P) planar, shared by the rows; s0, lo, hi: the row's part of the (T, P) arrays.  out: (4, TP) planar - s, f, df/ds,
// d2f/ds2; point p = t*P + q of row t = blockIdx.y writes column p of every plane, status[p] and iter[p] and nothing else, lanes
// past P nothing at all.
template <int LCAP, int KCAP>
__global__ __launch_bounds__(BLOCK) void k_line_peak_sph(SphDev M, int64_t P, int64_t TP, const double* __restrict__ a,
                                                         const double* __restrict__ b, const double* __restrict__ s0,
                                                         const double* __restrict__ lo, const double* __restrict__ hi,
                                                         const double* __restrict__ C, const double* __restrict__ eq, int F,
                                                         double htol, int kind, int max_iter, double tol,
                                                         double* __restrict__ out, int32_t* __restrict__ status,
                                                         int32_t* __restrict__ iter)
{
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t qc = q < P ? q : P - 1;
    const int64_t p = (int64_t)blockIdx.y * P + qc;
    const bool live = q < P;
    const Line y = line_of(qc, P, a, b);
    double s = s0[p], lb = lo[p], ub = hi[p];
    bool ok = line_ok(y) && isfinite(s) && isfinite(lb) && isfinite(ub) && lb <= s && s <= ub;
    if (F > 0) ok = ok && line_inside(y, lb, eq, F, htol) && line_inside(y, ub, eq, F, htol);
    const double nan = __builtin_nan("");
    if (live && !ok) {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[(int64_t)k * TP + p] = nan;
        status[p] = 3;
        if (iter) iter[p] = 0;
    }
    bool active = live && ok;               // still searching
    if (!__any(active)) return;             // no lane of the wave has a search to run: no walk
    const double sg = (double)kind;
    bool done = false;
    int it = 0;
    LinePeakSink sink;
    sink.Cv = C + (int64_t)blockIdx.y * M.N;
    for (;;) {
        const Geom g = line_geom(M, y, s);
        sink.f = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) sink.d[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) sink.h[k] = 0.0;
        peak_point<LCAP, KCAP>(M, g, sink);
        if (active) {
            double u[3];
            line_frame(M, g, y, u);         // after the walk: nothing of it is live across the chains
            const double* H = sink.h;       // rr tt pp rt rp tp
            const double f = sink.f;
            const double d1 = fma(u[0], sink.d[0], fma(u[1], sink.d[1], u[2] * sink.d[2]));
            const double w0 = fma(u[0], H[0], fma(u[1], H[3], u[2] * H[4]));
            const double w1 = fma(u[0], H[3], fma(u[1], H[1], u[2] * H[5]));
            const double w2 = fma(u[0], H[4], fma(u[1], H[5], u[2] * H[2]));
            const double d2 = fma(w0, u[0], fma(w1, u[1], w2 * u[2]));
            const bool fin = isfinite(f) && isfinite(d1) && isfinite(d2);
            if (!fin || done || it == max_iter) {
                int st = 3;
                if (fin) {
                    const double l0 = lo[p], l1 = hi[p];
                    st = !done ? 2 : (sg * d2 < 0.0 && fabs(s - l0) > tol && fabs(s - l1) > tol) ? 0 : 1;
                }
                out[p] = fin ? s : nan;
                out[TP + p] = fin ? f : nan;
                out[2 * TP + p] = fin ? d1 : nan;
                out[3 * TP + p] = fin ? d2 : nan;
                status[p] = st;
                if (iter) iter[p] = it;
                active = false;
            } else {
                ++it;
                if (sg * d1 > 0.0) lb = s;
                else ub = s;
                double sn = sg * d2 < 0.0 ? s - d1 / d2 : nan;
                if (!(lb < sn && sn < ub)) sn = 0.5 * (lb + ub);
                done = fabs(sn - s) <= tol;
                s = sn;
            }
        }
        if (!__any(active)) return;
    }
}

// ends: (2, TP) planar, lo then hi; out: (3, TP) planar - s, f, df/ds; otherwise as k_line_peak_sph.
template <int LCAP, int KCAP>
__global__ __launch_bounds__(BLOCK) void k_line_level_sph(SphDev M, int64_t P, int64_t TP, const double* __restrict__ a,
                                                          const double* __restrict__ b, const double* __restrict__ ends,
                                                          const double* __restrict__ level, const double* __restrict__ C,
                                                          const double* __restrict__ eq, int F, double htol, int max_iter,
                                                          double tol, double* __restrict__ out, int32_t* __restrict__ status,
                                                          int32_t* __restrict__ iter)
{
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t qc = q < P ? q : P - 1;
    const int64_t p = (int64_t)blockIdx.y * P + qc;
    const bool live = q < P;
    const Line y = line_of(qc, P, a, b);
    const double Lv = level[p];
    double lb = ends[p], ub = ends[TP + p];
    bool ok = line_ok(y) && isfinite(lb) && isfinite(ub) && isfinite(Lv) && lb < ub;
    if (F > 0) ok = ok && line_inside(y, lb, eq, F, htol) && line_inside(y, ub, eq, F, htol);
    const double nan = __builtin_nan("");
    // what a lane leaves when it stops
    auto store = [&](int st, double s, double f, double d1, int it) {
        out[p] = s;
        out[TP + p] = f;
        out[2 * TP + p] = d1;
        status[p] = st;
        if (iter) iter[p] = it;
    };
    if (live && !ok) store(3, nan, nan, nan, 0);
    bool active = live && ok;               // still searching
    if (!__any(active)) return;             // no lane of the wave has a search to run: no walk
    const double vfac = -(M.RE / 50.0);
    int phase = 0;                          // 0: the walk at lo, 1: the walk at hi, 2: the iteration
    double s = lb;
    double fra = 0.0, da = 0.0;             // f and d1 at the lower end
    bool sa = false, done = false;          // sa: f(lo) - L > 0
    int it = 0;
    LineLevelSink sink;
    sink.Cv = C + (int64_t)blockIdx.y * M.N;
    for (;;) {
        const Geom g = line_geom(M, y, s);
        sink.s0 = sink.s1 = sink.s2 = sink.s3 = 0.0;
        grad_point<LCAP, KCAP>(M, g, sink);
        if (active) {
            double u[3];
            line_frame(M, g, y, u);         // after the walk: nothing of it is live across the chains
            const double f = vfac * sink.s0;
            const double d1 = fma(u[0], sink.s0 + 2.0 * sink.s1, fma(u[1], sink.s2, u[2] * sink.s3));
            if (phase == 0) {
                fra = f;
                da = d1;
                s = ub;
                phase = 1;
            } else if (phase == 1) {
                const double fa = fra - Lv, fb = f - Lv;
                if (!(isfinite(fa) && isfinite(fb))) {
                    store(3, nan, nan, nan, 0);
                    active = false;
                } else if (fa == 0.0) {
                    store(0, lb, fra, da, 0);
                    active = false;
                } else if (fb == 0.0) {
                    store(0, ub, f, d1, 0);
                    active = false;
                } else if ((fa > 0.0) == (fb > 0.0)) {
                    store(1, nan, nan, nan, 0);
                    active = false;
                } else {
                    sa = fa > 0.0;
                    s = lb - fa * (ub - lb) / (fb - fa);
                    if (!(lb < s && s < ub)) s = 0.5 * (lb + ub);
                    phase = 2;
                }
            } else {
                const double phi = f - Lv;
                if (!(isfinite(phi) && isfinite(d1))) {
                    store(3, nan, nan, nan, it);
                    active = false;
                } else if (phi == 0.0 || done || it >= max_iter) {
                    store((phi == 0.0 || done) ? 0 : 2, s, f, d1, it);
                    active = false;
                } else {
                    ++it;
                    if ((phi > 0.0) == sa) lb = s;
                    else ub = s;
                    double sn = d1 != 0.0 ? s - phi / d1 : nan;
                    if (!(lb < sn && sn < ub)) sn = 0.5 * (lb + ub);
                    done = fabs(sn - s) <= tol;
                    s = sn;
                }
            }
        }
        if (!__any(active)) return;
    }
}

// what the two entries check alike, before anything is launched
int line_checks(vi_model* m, const char* who, int64_t T, int64_t P, int32_t F, const double* d_hull_eq, int32_t max_iter, double tol)
{
    if (!(T >= 0 && P >= 0 && F >= 0)) return vi_set_error("%s: negative size", who), VI_ERR_INVALID;
    if (!(F == 0 || d_hull_eq)) return vi_set_error("%s: hull facet count given without facet equations", who), VI_ERR_INVALID;
    if (!(max_iter >= 0 && max_iter <= 10000)) return vi_set_error("%s: max_iter must lie in [0, 10000]", who), VI_ERR_INVALID;
    if (!(std::isfinite(tol) && tol > 0.0)) return vi_set_error("%s: tol must be finite and positive", who), VI_ERR_INVALID;
    if (!(P <= 0x7fffffffLL)) return vi_set_error("%s: more rays than one launch takes", who), VI_ERR_INVALID;
    if (!(T == 0 || P <= (INT64_MAX / 4) / T)) return vi_set_error("%s: 4 * T * P overflows", who), VI_ERR_INVALID;
    const int rc = grad_model_check(m, who);
    if (rc != VI_OK) return rc;
    return at_grad_cap(m, who, [](auto, auto) { return (int)VI_OK; });        // the order, before anything is launched
}

}  // namespace

extern "C" int vi_eval_ray_peak_f64(vi_model* m, int64_t T, int64_t P, const double* d_a, const double* d_b, const double* d_start,
                                    const double* d_lo, const double* d_hi, const double* d_C, const double* d_hull_eq, int32_t F,
                                    double hull_tol, int32_t kind, int32_t max_iter, double tol, double* d_out, int32_t* d_status,
                                    int32_t* d_iter)
{
    const char* who = "vi_eval_ray_peak_f64";
    VI_REQUIRE(m && d_a && d_b && d_start && d_lo && d_hi && d_C && d_out && d_status, "null argument");
    VI_REQUIRE(kind == 1 || kind == -1, "kind must be +1 (maximum) or -1 (minimum)");
    const int rc = line_checks(m, who, T, P, F, d_hull_eq, max_iter, tol);
    if (rc != VI_OK || T == 0 || P == 0) return rc;
    VI_HIP(hipSetDevice(m->ctx->device));
    const int64_t TP = T * P;
    EvalTimer timer(m->ctx);
    // a grid's second dimension holds 65 535 rows: more go in slices, each on its own part of the arrays
    return for_chunks(T, 65535, [&](int64_t t0, int64_t tc) {
        const int64_t o = t0 * P;
        return at_grad_cap(m, who, [&](auto lc, auto kc) {
            return vi_launch(k_line_peak_sph<lc, kc>, dim3(nblocks(P, BLOCK), (unsigned)tc), dim3(BLOCK), 0, m->ctx->stream, m->sph,
                             P, TP, d_a, d_b, d_start + o, d_lo + o, d_hi + o, d_C + t0 * m->sph.N, d_hull_eq, (int)F, hull_tol,
                             (int)kind, (int)max_iter, tol, d_out + o, d_status + o, d_iter ? d_iter + o : nullptr);
        });
    });
}

extern "C" int vi_eval_ray_level_f64(vi_model* m, int64_t T, int64_t P, const double* d_a, const double* d_b, const double* d_ends,
                                     const double* d_level, const double* d_C, const double* d_hull_eq, int32_t F, double hull_tol,
                                     int32_t max_iter, double tol, double* d_out, int32_t* d_status, int32_t* d_iter)
{
    const char* who = "vi_eval_ray_level_f64";
    VI_REQUIRE(m && d_a && d_b && d_ends && d_level && d_C && d_out && d_status, "null argument");
    const int rc = line_checks(m, who, T, P, F, d_hull_eq, max_iter, tol);
    if (rc != VI_OK || T == 0 || P == 0) return rc;
    VI_HIP(hipSetDevice(m->ctx->device));
    const int64_t TP = T * P;
    EvalTimer timer(m->ctx);
    return for_chunks(T, 65535, [&](int64_t t0, int64_t tc) {
        const int64_t o = t0 * P;
        return at_grad_cap(m, who, [&](auto lc, auto kc) {
            return vi_launch(k_line_level_sph<lc, kc>, dim3(nblocks(P, BLOCK), (unsigned)tc), dim3(BLOCK), 0, m->ctx->stream,
                             m->sph, P, TP, d_a, d_b, d_ends + o, d_level + o, d_C + t0 * m->sph.N, d_hull_eq, (int)F, hull_tol,
                             (int)max_iter, tol, d_out + o, d_status + o, d_iter ? d_iter + o : nullptr);
        });
    });
}
