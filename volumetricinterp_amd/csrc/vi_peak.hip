// Sub-grid layer peaks of the sphharmlag model for gfx950: per column (lat, lon) and coefficient row the height at which the
// fitted parameter has its maximum (or minimum) along the geodetic normal, by a safeguarded Newton search on the analytic model -
// the value, the slope df/dh = u . grad f and the curvature d2f/dh2 = u^T H u, u the `up` row of the point's east-north-up matrix
// (enu_frame), are closed-form and come from ONE walk of the chains (peak_point, vi_sph_device.h).  The reference has no
// counterpart.
//   k_peak_sph<LCAP, KCAP>, a lane per column, the grid (blocks over Q, rows): a workgroup reads one coefficient row, wave-uniform.
//     h = h0; a = lo; b = hi; done = false; it = 0
//     loop:  f, d1, d2 at h                                   (one walk)
//            any of them not finite: status 3, NaN, stop
//            done or it == max_iter: stop
//            it += 1;  s d1 > 0 ? a = h : b = h               (s = kind: +1 maximum, -1 minimum)
//            hn = s d2 < 0 ? h - d1/d2 : NaN;  not (a < hn < b): hn = (a + b)/2
//            done = |hn - h| <= tol;  h = hn
//   The lane keeps ten sums - the value, three gradient components, six Hessian entries, each added in the order of the walk -
//   and contracts them with u after the walk: ten multiply-adds per basis function against twelve for three sums contracted per
//   term, and the sums are those of k_grad_sph and k_hess_sph (profiles/r26_kernel_resources.txt has the registers).  A lane
//   that has stopped stores its results at once and is frozen: it walks on with the wave at its last height and updates nothing;
//   the wave leaves when no lane is searching.  A column's bits depend on the column, its row, kind, max_iter and tol alone.
// The hull's byte mask is read once for the start points: a lane outside gives NaN and status 3, a wave without a lane inside
// leaves before any walk.
#include <cmath>

#include "vi_sph_device.h"
#include "vi_eval_host.h"

namespace {

// the ten sums of a lane
struct PeakSink {
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

// out: (4, T*Q) planar - h, f, df/dh, d2f/dh2; point p = t*Q + q of row t = blockIdx.y writes column p of every plane,
// status[p] and iter[p] and nothing else, lanes past Q nothing at all.
template <int LCAP, int KCAP>
__global__ __launch_bounds__(BLOCK) void k_peak_sph(SphDev M, int64_t Q, int64_t PQ, const double* __restrict__ lat,
                                                    const double* __restrict__ lon, const double* __restrict__ h0,
                                                    const double* __restrict__ lo, const double* __restrict__ hi,
                                                    const double* __restrict__ C, const unsigned char* __restrict__ mask,
                                                    int kind, int max_iter, double tol, double* __restrict__ out,
                                                    int32_t* __restrict__ status, int32_t* __restrict__ iter)
{
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t p = (int64_t)blockIdx.y * Q + (q < Q ? q : Q - 1);
    const bool live = q < Q;
    const double la = lat[p], lg = lon[p];
    double h = h0[p], a = lo[p], b = hi[p];
    bool ok = isfinite(la) && isfinite(lg) && isfinite(h) && isfinite(a) && isfinite(b) && a <= h && h <= b;
    if (mask) ok = ok && mask[p] != 0;
    const double nan = __builtin_nan("");
    if (live && !ok) {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[(int64_t)k * PQ + p] = nan;
        status[p] = 3;
        if (iter) iter[p] = 0;
    }
    bool active = live && ok;               // still searching
    if (!__any(active)) return;             // no lane of the wave has a search to run: no walk
    const double s = (double)kind;
    bool done = false;
    int it = 0;
    PeakSink sink;
    sink.Cv = C + (int64_t)blockIdx.y * M.N;
    for (;;) {
        const Geom g = sph_geom(M, la, lg, h);
        sink.f = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) sink.d[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) sink.h[k] = 0.0;
        peak_point<LCAP, KCAP>(M, g, sink);
        if (active) {
            double F[9];
            enu_frame(M, g, la, lg, F);     // after the walk: nothing of it is live across the chains
            const double* u = F + 6;        // up
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
                    st = !done ? 2 : (s * d2 < 0.0 && fabs(h - l0) > tol && fabs(h - l1) > tol) ? 0 : 1;
                }
                out[p] = fin ? h : nan;
                out[PQ + p] = fin ? f : nan;
                out[2 * PQ + p] = fin ? d1 : nan;
                out[3 * PQ + p] = fin ? d2 : nan;
                status[p] = st;
                if (iter) iter[p] = it;
                active = false;
            } else {
                ++it;
                if (s * d1 > 0.0) a = h;
                else b = h;
                double hn = s * d2 < 0.0 ? h - d1 / d2 : nan;
                if (!(a < hn && hn < b)) hn = 0.5 * (a + b);
                done = fabs(hn - h) <= tol;
                h = hn;
            }
        }
        if (!__any(active)) return;
    }
}

}  // namespace

extern "C" int vi_eval_peak_f64(vi_model* m, int64_t T, int64_t Q, const double* d_lat, const double* d_lon, const double* d_h0,
                                const double* d_lo, const double* d_hi, const double* d_C, const double* d_hull_eq, int32_t F,
                                double hull_tol, int32_t kind, int32_t max_iter, double tol, double* d_out, int32_t* d_status,
                                int32_t* d_iter)
{
    const char* who = "vi_eval_peak_f64";
    VI_REQUIRE(m && d_lat && d_lon && d_h0 && d_lo && d_hi && d_C && d_out && d_status, "null argument");
    VI_REQUIRE(T >= 0 && Q >= 0 && F >= 0, "negative size");
    VI_REQUIRE_HULL(F, d_hull_eq);
    VI_REQUIRE(kind == 1 || kind == -1, "kind must be +1 (maximum) or -1 (minimum)");
    VI_REQUIRE(max_iter >= 0, "negative max_iter");
    VI_REQUIRE(std::isfinite(tol) && tol > 0.0, "tol must be finite and positive");
    VI_REQUIRE(T == 0 || Q <= INT64_MAX / T, "T * Q overflows");
    int rc = grad_model_check(m, who);
    if (rc != VI_OK) return rc;
    rc = at_grad_cap(m, who, [](auto, auto) { return (int)VI_OK; });          // the order, before anything is launched
    if (rc != VI_OK || T == 0 || Q == 0) return rc;
    VI_HIP(hipSetDevice(m->ctx->device));
    const int64_t PQ = T * Q;
    if (F > 0 && (rc = prepare_call(m, PQ, d_lat, d_lon, d_h0, d_hull_eq, F, hull_tol, 0, nullptr)) != VI_OK) return rc;
    const unsigned char* d_mask = F > 0 ? m->d_mask : nullptr;
    EvalTimer timer(m->ctx);
    // a grid's second dimension holds 65 535 rows: more go in slices, each on its own part of the arrays
    return for_chunks(T, 65535, [&](int64_t t0, int64_t tc) {
        const int64_t o = t0 * Q;
        return at_grad_cap(m, who, [&](auto lc, auto kc) {
            return vi_launch(k_peak_sph<lc, kc>, dim3(nblocks(Q, BLOCK), (unsigned)tc), dim3(BLOCK), 0, m->ctx->stream, m->sph, Q,
                             PQ, d_lat + o, d_lon + o, d_h0 + o, d_lo + o, d_hi + o, d_C + t0 * m->sph.N,
                             d_mask ? d_mask + o : nullptr, (int)kind, (int)max_iter, tol, d_out + o, d_status + o,
                             d_iter ? d_iter + o : nullptr);
        });
    });
}
