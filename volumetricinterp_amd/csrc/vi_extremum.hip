// Maxima and minima of the sphharmlag model in three dimensions for gfx950: per start x0 (ECEF metres) and coefficient row the
// point inside the ball |x - x0| <= radius and inside the hull at which the fitted parameter has its maximum (or minimum), the
// value, the gradient and the Hessian there - the centre of a polar-cap patch, its peak density and, from the principal
// curvatures, its size.  The searches of vi_peak.hip and vi_line.hip follow a direction the caller chooses; this one has none.
// The reference has no counterpart.
//   walk       peak_point from the ECEF point (sph_geom_ecef, no geodetic step): f, the gradient and the Hessian tensor in the
//              model's orthonormal frame (r', theta', phi'), ten sums.
//   frame      after the walk: E, the three unit vectors of that frame at the point written in ECEF - the rotated spherical unit
//              vectors turned back by the transpose of the model's Rodrigues rotation, the frame line_frame of vi_line.hip dots
//              one direction with.  g = E^T g_model, H = E^T H_model E: the Hessian is a tensor, so H is the plain Cartesian
//              matrix of second derivatives and Newton's iteration in R^3 is exact, no connection terms.  Nothing of E lives
//              across the chains.
//   iteration  include/vinterp.h has it (vi_eval_extremum_f64), tests/extremum_ref.py mirrors it: Newton steps of an LDL^T solve
//              with floored pivots inside a trust length, acceptance by value or - for a full Newton step - by gradient norm, a
//              rejected or out-of-region iterate backtracks towards the best point.
//   k_extremum_sph<LCAP, KCAP>  a lane per search, the grid (blocks over P, rows): a workgroup reads one coefficient row,
//              wave-uniform.  A lane that has stopped stores its results at once and is frozen; the wave leaves when no lane is
//              searching; every pass stops the lane or adds one to `it`, which max_iter (at most 10 000) bounds.  Every product
//              stands in an fma or alone and the 3 x 3 arithmetic has one order: a search's bits depend on its start, radius,
//              row, the parameters and the facet list alone.  The start and the radius are read again at every pass (four loads
//              against a walk) instead of being held across the chains.
//   hull       every iterate is tested against the F half-spaces of the caller's list, fma(nx, X, fma(ny, Y, fma(nz, Z, off)))
//              <= tol as K2l's clip has it; the list is wave-uniform, the loop plain.  F = 0: no test.  No host pass.
#include <cmath>

#include "vi_sph_device.h"
#include "vi_eval_host.h"

namespace {

// the ten sums of a lane (those of k_peak_sph)
struct ExtremumSink {
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

__device__ __forceinline__ double norm3(double a, double b, double c) { return sqrt(fma(c, c, fma(b, b, a * a))); }

// E[3 c + i]: component i (ECEF) of the unit vector c - r', theta', phi' of the rotated spherical coordinates at the point g -,
// r' = (st cphi, st sphi, x), theta' = (x cphi, x sphi, -st), phi' = (-sphi, cphi, 0) in the rotated frame, each turned back by
// the transpose of the Rodrigues matrix of sph_geom_ecef: v rc - (k x v) rs + k (k . v)(1 - rc), k = (kx, ky, 0)
__device__ __forceinline__ void model_axes(const SphDev& M, const Geom& g, double* E)
{
    const double st = sqrt(fma(g.Ry, g.Ry, g.Rx * g.Rx)) / (M.RE * fma(g.z, 0.01, 1.0));
    const double omc = 1.0 - M.rc;
    const double v[3][3] = {{st * g.cphi, st * g.sphi, g.x}, {g.x * g.cphi, g.x * g.sphi, -st}, {-g.sphi, g.cphi, 0.0}};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double vx = v[c][0], vy = v[c][1], vz = v[c][2];
        const double kd = fma(M.kx, vx, M.ky * vy) * omc;
        const double cz = fma(M.kx, vy, -(M.ky * vx));          // (k x v)_z
        E[3 * c] = fma(M.kx, kd, fma(-(M.ky * vz), M.rs, vx * M.rc));
        E[3 * c + 1] = fma(M.ky, kd, fma(M.kx * vz, M.rs, vy * M.rc));
        E[3 * c + 2] = fma(-cz, M.rs, vz * M.rc);
    }
}

// whether (X, Y, Z) is inside every half-space of the list: K2l's expression and criterion.  A NaN point is outside.
__device__ __forceinline__ bool hull_inside(double X, double Y, double Z, const double* __restrict__ eq, int F, double tol)
{
    bool in = true;
    for (int f = 0; f < F; ++f) {
        const double nx = eq[4 * f], ny = eq[4 * f + 1], nz = eq[4 * f + 2], off = eq[4 * f + 3];
        in = in && fma(nx, X, fma(ny, Y, fma(nz, Z, off))) <= tol;
    }
    return in;
}

// The pivots of the LDL^T factorisation of the symmetric matrix a (packed 00 11 22 01 02 12) in the order 1, 2, 3 and its
// multipliers; with FLOOR every pivot that is not > mu is replaced by mu, and `mod` says that one was.
struct Ldl {
    double p1, p2, p3, l21, l31, l32;
    bool mod;
};
template <bool FLOOR>
__device__ __forceinline__ Ldl ldl3(const double* a, double mu)
{
    Ldl w;
    w.mod = false;
    w.p1 = a[0];
    if (FLOOR && !(w.p1 > mu)) { w.p1 = mu; w.mod = true; }
    w.l21 = a[3] / w.p1;
    w.l31 = a[4] / w.p1;
    w.p2 = fma(-w.l21, a[3], a[1]);
    if (FLOOR && !(w.p2 > mu)) { w.p2 = mu; w.mod = true; }
    const double t32 = fma(-w.l31, a[3], a[5]);
    w.l32 = t32 / w.p2;
    w.p3 = fma(-w.l32, t32, fma(-w.l31, a[4], a[2]));
    if (FLOOR && !(w.p3 > mu)) { w.p3 = mu; w.mod = true; }
    return w;
}

// x0: (3, TP) planar, radius: (TP); out: (13, TP) planar - x, y, z, f, g (3), H (6: 00 11 22 01 02 12), all in ECEF; search
// p = t*P + q of row t = blockIdx.y reads column p of x0 and radius and writes column p of every plane, status[p] and iter[p]
// and nothing else, lanes past P nothing at all.  max_step = 0: an eighth of the search's radius.
template <int LCAP, int KCAP>
__global__ __launch_bounds__(BLOCK) void k_extremum_sph(SphDev M, int64_t P, int64_t TP, const double* __restrict__ x0,
                                                        const double* __restrict__ radius, const double* __restrict__ C,
                                                        const double* __restrict__ eq, int F, double htol, int kind,
                                                        double max_step, int max_iter, double tol, double* __restrict__ out,
                                                        int32_t* __restrict__ status, int32_t* __restrict__ iter)
{
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t qc = q < P ? q : P - 1;
    const int64_t p = (int64_t)blockIdx.y * P + qc;
    const bool live = q < P;
    double x[3] = {x0[p], x0[TP + p], x0[2 * TP + p]};
    const double nan = __builtin_nan("");
    bool active;                                // still searching
    {
        const double rad = radius[p];
        const bool ok = isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && isfinite(rad) && rad > 0.0;
        if (live && !ok) {
#pragma unroll
            for (int k = 0; k < 13; ++k) out[(int64_t)k * TP + p] = nan;
            status[p] = 3;
            if (iter) iter[p] = 0;
        }
        active = live && ok;
    }
    if (!__any(active)) return;                 // no lane of the wave has a search to run: no walk
    const double sg = (double)kind;
    double xb[3] = {x[0], x[1], x[2]}, d[3] = {0.0, 0.0, 0.0};
    double fb = 0.0, gb = 0.0, delta = 0.0;
    bool have = false, done = false, full = false;
    int it = 0;
    ExtremumSink sink;
    sink.Cv = C + (int64_t)blockIdx.y * M.N;
    for (;;) {
        const Geom g = sph_geom_ecef(M, x[0], x[1], x[2]);
        sink.f = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) sink.d[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) sink.h[k] = 0.0;
        peak_point<LCAP, KCAP>(M, g, sink);
        if (active) {
            double E[9];
            model_axes(M, g, E);                // after the walk: nothing of it is live across the chains
            const double* Hm = sink.h;          // rr tt pp rt rp tp
            const double f = sink.f;
            double gv[3], W[9], H[6];
#pragma unroll
            for (int i = 0; i < 3; ++i) gv[i] = fma(E[i], sink.d[0], fma(E[3 + i], sink.d[1], E[6 + i] * sink.d[2]));
            // W = H_model E, row c of H_model: (rr rt rp), (rt tt tp), (rp tp pp)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                W[j] = fma(Hm[0], E[j], fma(Hm[3], E[3 + j], Hm[4] * E[6 + j]));
                W[3 + j] = fma(Hm[3], E[j], fma(Hm[1], E[3 + j], Hm[5] * E[6 + j]));
                W[6 + j] = fma(Hm[4], E[j], fma(Hm[5], E[3 + j], Hm[2] * E[6 + j]));
            }
            // H[i][j] = sum_c E[c][i] W[c][j], packed 00 11 22 01 02 12
            constexpr int PI[6] = {0, 1, 2, 0, 0, 1}, PJ[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
            for (int k = 0; k < 6; ++k)
                H[k] = fma(E[PI[k]], W[PJ[k]], fma(E[3 + PI[k]], W[3 + PJ[k]], E[6 + PI[k]] * W[6 + PJ[k]]));
            const double rad = radius[p];
            const double mstep = max_step > 0.0 ? max_step : 0.125 * rad;
            bool ins = norm3(x[0] - x0[p], x[1] - x0[TP + p], x[2] - x0[2 * TP + p]) <= rad;
            if (F > 0) ins = ins && hull_inside(x[0], x[1], x[2], eq, F, htol);
            bool fin = isfinite(f);
#pragma unroll
            for (int k = 0; k < 3; ++k) fin = fin && isfinite(gv[k]);
#pragma unroll
            for (int k = 0; k < 6; ++k) fin = fin && isfinite(H[k]);
            double a[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) a[k] = -sg * H[k];
            if (!fin || (!have && !ins)) {
#pragma unroll
                for (int k = 0; k < 13; ++k) out[(int64_t)k * TP + p] = nan;
                status[p] = 3;
                if (iter) iter[p] = it;
                active = false;
            } else if (done || it == max_iter) {
                const Ldl w = ldl3<false>(a, 0.0);
#pragma unroll
                for (int k = 0; k < 3; ++k) out[(int64_t)k * TP + p] = x[k];
                out[3 * TP + p] = f;
#pragma unroll
                for (int k = 0; k < 3; ++k) out[(int64_t)(4 + k) * TP + p] = gv[k];
#pragma unroll
                for (int k = 0; k < 6; ++k) out[(int64_t)(7 + k) * TP + p] = H[k];
                status[p] = !done ? 2 : (full && ins && w.p1 > 0.0 && w.p2 > 0.0 && w.p3 > 0.0) ? 0 : 1;
                if (iter) iter[p] = it;
                active = false;
            } else {
                ++it;
                const double gn = norm3(gv[0], gv[1], gv[2]);
                if (have && (!ins || !(sg * f >= sg * fb || (full && gn < gb)))) {
                    // reject: backtrack along the same step, towards the best point - or stop there, once the rejected step
                    // was within tol of it
                    const double dl = norm3(d[0], d[1], d[2]);
                    full = false;
                    done = dl <= tol;
                    if (!done) delta = 0.25 * dl;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        if (!done) d[k] = 0.25 * d[k];
                        x[k] = done ? xb[k] : xb[k] + d[k];
                    }
                } else {
                    if (have) delta = fmin(2.0 * delta, mstep);
                    else delta = mstep;
#pragma unroll
                    for (int k = 0; k < 3; ++k) xb[k] = x[k];
                    fb = f;
                    gb = gn;
                    have = true;
                    double dn = 0.0;
                    full = true;
                    d[0] = d[1] = d[2] = 0.0;   // a zero gradient is a step of zero length
                    if (gn > 0.0) {
                        const Ldl w = ldl3<true>(a, gn / delta);
                        const double y1 = sg * gv[0];
                        const double y2 = fma(-w.l21, y1, sg * gv[1]);
                        const double y3 = fma(-w.l32, y2, fma(-w.l31, y1, sg * gv[2]));
                        d[2] = y3 / w.p3;
                        d[1] = fma(-w.l32, d[2], y2 / w.p2);
                        d[0] = fma(-w.l31, d[2], fma(-w.l21, d[1], y1 / w.p1));
                        full = !w.mod;
                        dn = norm3(d[0], d[1], d[2]);
                        if (dn > delta) {
                            const double sc = delta / dn;
#pragma unroll
                            for (int k = 0; k < 3; ++k) d[k] = d[k] * sc;
                            full = false;
                            dn = delta;
                        }
                    }
                    done = dn <= tol;
#pragma unroll
                    for (int k = 0; k < 3; ++k) x[k] = x[k] + d[k];
                }
            }
        }
        if (!__any(active)) return;
    }
}

// what the entry checks before anything is launched
int extremum_checks(vi_model* m, const char* who, int64_t T, int64_t P, int32_t F, const double* d_hull_eq, int32_t kind,
                    double max_step, int32_t max_iter, double tol)
{
    if (!(T >= 0 && P >= 0 && F >= 0)) return vi_set_error("%s: negative size", who), VI_ERR_INVALID;
    if (!(F == 0 || d_hull_eq)) return vi_set_error("%s: hull facet count given without facet equations", who), VI_ERR_INVALID;
    if (!(kind == 1 || kind == -1)) return vi_set_error("%s: kind must be +1 (maximum) or -1 (minimum)", who), VI_ERR_INVALID;
    if (!(max_iter >= 0 && max_iter <= 10000)) return vi_set_error("%s: max_iter must lie in [0, 10000]", who), VI_ERR_INVALID;
    if (!(std::isfinite(tol) && tol > 0.0)) return vi_set_error("%s: tol must be finite and positive", who), VI_ERR_INVALID;
    if (!(std::isfinite(max_step) && max_step >= 0.0))
        return vi_set_error("%s: max_step must be finite and positive, or 0 for an eighth of each radius", who), VI_ERR_INVALID;
    if (!(P <= 0x7fffffffLL)) return vi_set_error("%s: more searches than one launch takes", who), VI_ERR_INVALID;
    if (!(T == 0 || P <= (INT64_MAX / 13) / T)) return vi_set_error("%s: 13 * T * P overflows", who), VI_ERR_INVALID;
    const int rc = grad_model_check(m, who);
    if (rc != VI_OK) return rc;
    return at_grad_cap(m, who, [](auto, auto) { return (int)VI_OK; });        // the order, before anything is launched
}

}  // namespace

extern "C" int vi_eval_extremum_f64(vi_model* m, int64_t T, int64_t P, const double* d_x0, const double* d_radius,
                                    const double* d_C, const double* d_hull_eq, int32_t F, double hull_tol, int32_t kind,
                                    double max_step, int32_t max_iter, double tol, double* d_out, int32_t* d_status,
                                    int32_t* d_iter)
{
    const char* who = "vi_eval_extremum_f64";
    VI_REQUIRE(m && d_x0 && d_radius && d_C && d_out && d_status, "null argument");
    const int rc = extremum_checks(m, who, T, P, F, d_hull_eq, kind, max_step, max_iter, tol);
    if (rc != VI_OK || T == 0 || P == 0) return rc;
    VI_HIP(hipSetDevice(m->ctx->device));
    const int64_t TP = T * P;
    EvalTimer timer(m->ctx);
    // a grid's second dimension holds 65 535 rows: more go in slices, each on its own part of the arrays
    return for_chunks(T, 65535, [&](int64_t t0, int64_t tc) {
        const int64_t o = t0 * P;
        return at_grad_cap(m, who, [&](auto lc, auto kc) {
            return vi_launch(k_extremum_sph<lc, kc>, dim3(nblocks(P, BLOCK), (unsigned)tc), dim3(BLOCK), 0, m->ctx->stream, m->sph,
                             P, TP, d_x0 + o, d_radius + o, d_C + t0 * m->sph.N, d_hull_eq, (int)F, hull_tol, (int)kind, max_step,
                             (int)max_iter, tol, d_out + o, d_status + o, d_iter ? d_iter + o : nullptr);
        });
    });
}
