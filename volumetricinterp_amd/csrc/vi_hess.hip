// Hessian basis of the sphharmlag model for gfx950: the second covariant derivatives of every basis function in the orthonormal
// frame of the gradient (hess_point, vi_sph_device.h, has the formulas), six distinct entries per function and point in the
// packed order of the gradient covariance - (0,0) (1,1) (2,2) (0,1) (0,2) (1,2).  The reference has no counterpart: its
// grad_basis (sphharmlag.py:148-184) stops at the first derivatives.
//   k_hess_sph<LCAP, KCAP, MODE, ENU>, a lane per point on the gradient's chains run with one more Laguerre recurrence:
//     HESS_CONTRACT  the six entries summed against ONE coefficient vector as they come, six fp64 accumulators per lane: the
//                    Hessian of the fitted parameter (vi_eval_hess_f64); the 6N values of a point are never formed.
//     HESS_RESIDENT  the planar matrix a resident grid keeps, H[(n*6 + k)*Q + q] (vi_eval_hess_basis_f64): every store of a
//                    wave is 64 consecutive doubles, and vi_eval_resident_f64 multiplies it as it multiplies the gradient basis.
// Both read the hull's byte mask: a lane outside stores NaN, a wave without a lane inside leaves before the chains.  With ENU
// the symmetric matrix is turned into east, north, up, F H F^T with the point's matrix (enu_frame) - per basis function before
// the stores (HESS_RESIDENT), once on the sums (HESS_CONTRACT: the turn is linear).
#include "vi_sph_device.h"
#include "vi_eval_host.h"

namespace {

enum { HESS_CONTRACT = 0, HESS_RESIDENT = 1 };

// h (packed, model frame) -> F h F^T (packed), F row-major 3 x 3
__device__ __forceinline__ void hess_turn(const double* F, const double* h, double* o)
{
    const double S[3][3] = {{h[0], h[3], h[4]}, {h[3], h[1], h[5]}, {h[4], h[5], h[2]}};
    double W[3][3];                     // F S
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) W[i][j] = fma(F[3 * i], S[0][j], fma(F[3 * i + 1], S[1][j], F[3 * i + 2] * S[2][j]));
    auto dot = [&](int i, int j) { return fma(W[i][0], F[3 * j], fma(W[i][1], F[3 * j + 1], W[i][2] * F[3 * j + 2])); };
    o[0] = dot(0, 0);
    o[1] = dot(1, 1);
    o[2] = dot(2, 2);
    o[3] = dot(0, 1);
    o[4] = dot(0, 2);
    o[5] = dot(1, 2);
}

// what k_hess_sph does with a term: adds its product with the coefficient to the point's six sums, or stores it
template <int MODE, bool ENU>
struct HessSink {
    const double* __restrict__ Cv;
    double* Hp;                         // the point's first entry; entries ld_c apart, basis functions 6 ld_c
    int64_t ld_c;
    double F[9];
    bool active;
    double acc[6];
    __device__ __forceinline__ void term(int n, const double* h)
    {
        if (MODE == HESS_CONTRACT) {
            const double cf = Cv[n];
#pragma unroll
            for (int k = 0; k < 6; ++k) acc[k] = fma(h[k], cf, acc[k]);
        } else if (active) {
            double* o = Hp + (int64_t)n * 6 * ld_c;
            if (ENU) {
                double t[6];
                hess_turn(F, h, t);
#pragma unroll
                for (int k = 0; k < 6; ++k) o[k * ld_c] = t[k];
            } else {
#pragma unroll
                for (int k = 0; k < 6; ++k) o[k * ld_c] = h[k];
            }
        }
    }
};

// Hout: (6, P) planar with HESS_CONTRACT, (N, 6, P) planar with HESS_RESIDENT; point p writes column p of every plane and
// nothing else, lanes past P nothing at all.
template <int LCAP, int KCAP, int MODE, bool ENU>
__global__ __launch_bounds__(BLOCK) void k_hess_sph(SphDev M, int64_t P, const double* __restrict__ lat,
                                                    const double* __restrict__ lon, const double* __restrict__ alt,
                                                    const double* __restrict__ Cv, const unsigned char* __restrict__ mask,
                                                    double* __restrict__ Hout)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t pc = p < P ? p : P - 1;
    bool active = p < P;
    double* Hp = Hout + pc;
    if (mask) {
        const bool in = mask[pc] != 0;
        if (active && !in) {
            const double nan = __builtin_nan("");
            const int rows = MODE == HESS_CONTRACT ? 6 : 6 * M.N;
            for (int i = 0; i < rows; ++i) Hp[(int64_t)i * P] = nan;
        }
        active = active && in;
        if (!__any(active)) return;           // whole wave outside the hull: skip the chains
    }
    const Geom g = sph_geom(M, lat[pc], lon[pc], alt[pc]);
    HessSink<MODE, ENU> sink;
    sink.Cv = Cv;
    sink.Hp = Hp;
    sink.ld_c = P;
    sink.active = active;
#pragma unroll
    for (int k = 0; k < 6; ++k) sink.acc[k] = 0.0;
    if (ENU) enu_frame(M, g, lat[pc], lon[pc], sink.F);
    hess_point<LCAP, KCAP>(M, g, sink);
    if (MODE == HESS_CONTRACT && active) {
        double t[6];
        if (ENU) hess_turn(sink.F, sink.acc, t);
#pragma unroll
        for (int k = 0; k < 6; ++k) Hp[k * P] = ENU ? t[k] : sink.acc[k];
    }
}

// The launch of both entries: the model and order checks of the gradient (grad_model_check, at_grad_cap: nothing is launched for
// a model or an order they refuse), the hull pass (prepare_call) when there is a hull, then the kernel under the evaluation timer.
template <int MODE>
int launch_hess_sph(vi_model* m, const char* who, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                    const double* d_C, const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame, double* d_H)
{
    int rc = grad_model_check(m, who);
    if (rc != VI_OK) return rc;
    rc = at_grad_cap(m, who, [](auto, auto) { return (int)VI_OK; });          // the order, before anything is launched
    if (rc != VI_OK || Q == 0) return rc;
    VI_HIP(hipSetDevice(m->ctx->device));
    if (F > 0 && (rc = prepare_call(m, Q, d_lat, d_lon, d_alt, d_hull_eq, F, hull_tol, 0, nullptr)) != VI_OK) return rc;
    const unsigned char* d_mask = F > 0 ? m->d_mask : nullptr;
    EvalTimer timer(m->ctx);
    return with_flag(frame == VI_FRAME_ENU, [&](auto enu) -> int {
        return at_grad_cap(m, who, [&](auto lc, auto kc) {
            return vi_launch(k_hess_sph<lc, kc, MODE, enu>, dim3(nblocks(Q, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, m->sph, Q,
                             d_lat, d_lon, d_alt, d_C, d_mask, d_H);
        });
    });
}

}  // namespace

extern "C" int vi_eval_hess_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                const double* d_C, const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame,
                                double* d_out)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_C && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && F >= 0, "negative size");
    VI_REQUIRE_HULL(F, d_hull_eq);
    VI_REQUIRE_FRAME(frame);
    return launch_hess_sph<HESS_CONTRACT>(m, "vi_eval_hess_f64", Q, d_lat, d_lon, d_alt, d_C, d_hull_eq, F, hull_tol, frame, d_out);
}

extern "C" int vi_eval_hess_basis_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                      const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame, double* d_H)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_H, "null argument");
    VI_REQUIRE(Q >= 0 && F >= 0, "negative size");
    VI_REQUIRE_HULL(F, d_hull_eq);
    VI_REQUIRE_FRAME(frame);
    return launch_hess_sph<HESS_RESIDENT>(m, "vi_eval_hess_basis_f64", Q, d_lat, d_lon, d_alt, nullptr, d_hull_eq, F, hull_tol,
                                          frame, d_H);
}
