// K2t and K2tg for gfx950: densities and gradients along a trajectory, every point at its own time - the tiled kernels at the
// orders of the fast list and of the gradient caps (k_track_sph_fast, k_track_grad_sph), the per-lane kernels for every other
// order and the RBF model (k_track_sph, k_track_rbf); entries vi_eval_track_f64 and vi_eval_track_grad_f64, and the standard
// errors and gradient covariances along a track, vi_eval_track_err_f64 and vi_eval_track_grad_cov_f64, which build the matrix of
// a chunk of points with vi_basis.hip's launchers and hand it to the records routines of vi_resident.hip.
#include "vi_chain_device.h"
#include "vi_eval_host.h"

namespace {

// ---------------------------------------------------------------------------------------------
// K2t: densities along a trajectory, every point at its own time (vi_eval_track_f64).  Point q takes prepared coefficient row
// rec[q] (nearest mode) or the blend (1 - w[q]) D(rec[q]) + w[q] D(rec[q] + 1) of the densities D of two neighbouring rows.
// The unit is a workgroup of ONE wave (64 points) with its own tile: the wave finds the lowest and highest row its live lanes
// need (shuffles over rec: nothing assumes sorted input), stages the window of TT prepared rows from the lowest one in LDS -
// rows past R - 1 zero-filled, never read - and runs the chains of k_eval_sph_fast once for TT accumulators; the epilogue takes
// each lane's own accumulator (two neighbours when blending) by an unrolled compare-select, never a product with zero: a NaN
// row touches no other row's points.  Where the wave's rows span more than a window the pass is repeated from the next window
// - consecutive windows share one row when blending, so that every pair (rec, rec + 1) lies inside one - until the highest row
// is covered; a lane keeps the value of the one pass whose window holds its rows.  With the points sorted by record the spans
// of all waves add up to at most R + (number of waves), so the passes beyond one per wave are at most about R / (TT - 1) wave
// passes in total, whatever Q is; unsorted input is correct and costs up to R / (TT - 1) passes per wave.  A wave without a
// live lane (outside the hull, no record, rows past R - 1) leaves before the table is staged.  One wave per workgroup: the
// barriers around the staging are wave barriers, the windows follow the 64 points and not 256, and the LDS need is that of
// k_eval_sph_fast at the same TT, so the same orders fit.
constexpr int TRACK_BLOCK = 64;
constexpr int TRACK_TT = 4;         // the tile width: 3.9e10 / 4 point-rows per second against 1.4e10 at TT = 1 (launch_eval_sph_fast)

// what a point of a track needs to be computed at all: a record, its row(s) inside the R rows, inside the hull
__device__ __forceinline__ bool track_live(int64_t q, int64_t qc, int64_t Q, int r, int R, int pair,
                                           const unsigned char* __restrict__ mask, int F)
{
    return q < Q && r >= 0 && r <= R - 1 - pair && (F == 0 || mask[qc] != 0);
}

template <int L, int K, int TT, bool INTERP>
__global__ __launch_bounds__(TRACK_BLOCK) void k_track_sph_fast(SphDev M, int64_t Q, const double* __restrict__ lat,
                                                                const double* __restrict__ lon, const double* __restrict__ alt,
                                                                const int* __restrict__ rec, const double* __restrict__ wgt, int R,
                                                                const double* __restrict__ Cp,
                                                                const unsigned char* __restrict__ mask, int F,
                                                                double* __restrict__ out)
{
    constexpr int NB = L * L * K;
    constexpr int PAIR = INTERP ? 1 : 0;
    constexpr int STEP = TT - PAIR;                     // rows from one window to the next
    static_assert(STEP >= 1, "a blending window holds at least two rows");
    extern __shared__ __align__(16) double sh[];
    const int64_t q = (int64_t)blockIdx.x * TRACK_BLOCK + threadIdx.x;
    const int64_t qc = q < Q ? q : Q - 1;
    const int r = rec[qc];
    const bool live = track_live(q, qc, Q, r, R, PAIR, mask, F);
    if (!__any(live)) {                                 // (the whole workgroup: no barrier has been met)
        if (q < Q) out[q] = __builtin_nan("");
        return;
    }
    int lo = live ? r : 0x7fffffff, hi = live ? r + PAIR : -1;
#pragma unroll
    for (int off = TRACK_BLOCK / 2; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, TRACK_BLOCK));
        hi = max(hi, __shfl_xor(hi, off, TRACK_BLOCK));
    }
    lo = __builtin_amdgcn_readfirstlane(lo);            // 0 <= lo <= hi <= R - 1
    hi = __builtin_amdgcn_readfirstlane(hi);
    const SphGroupDev G = M.groups[0];
    const int nj = G.nvmax + 1;
    double* shc = sh;                                   // [nj][L] recurrence table
    double* shC = sh + ((nj * L + 1) & ~1);             // [TT][NB] the window
    int* nvl = reinterpret_cast<int*>(shC + TT * NB);   // [L]
    stage_chain_table(G, nj, L, shc, nvl, TRACK_BLOCK);
    const Geom g = sph_geom(M, lat[qc], lon[qc], alt[qc]);
    const double Ez = exp(-0.5 * g.z);
    const double w = INTERP ? wgt[qc] : 0.0;
    double val = __builtin_nan("");
    for (int base = lo;; base += STEP) {
        __syncthreads();                                // the pass before has read the window
        for (int i = threadIdx.x; i < TT * NB; i += TRACK_BLOCK)
            shC[i] = i / NB < R - base ? Cp[(int64_t)base * NB + i] : 0.0;
        __syncthreads();
        FastEval<L, K, TT> E;
        E.shC = shC;
        fast_chains<L, K, TT, double>(E, G, g, shc, nvl, nj);
        const int d = live ? r - base : -1;             // the lane's row in this window
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            if (d == t) a = E.acc[t];
            if (INTERP && d + 1 == t) b = E.acc[t];
        }
        if (d >= 0 && d < STEP) val = INTERP ? (1.0 - w) * (Ez * a) + w * (Ez * b) : Ez * a;
        if (hi - base <= TT - 1) break;                 // wave-uniform
    }
    if (q < Q) out[q] = live ? val : __builtin_nan("");
}

// The frame of the two per-lane kernels, of either model M: rows(Cr, lat, lon, alt, v) gives the model's value at the point
// with the row Cr, v[0], and with INTERP that with the row after it, v[1].
template <bool INTERP, class Dev, class Rows>
__device__ __forceinline__ void track_per_lane(const Dev& M, int64_t Q, const double* __restrict__ lat,
                                               const double* __restrict__ lon, const double* __restrict__ alt,
                                               const int* __restrict__ rec, const double* __restrict__ wgt, int R,
                                               const double* __restrict__ C, const unsigned char* __restrict__ mask, int F,
                                               double* __restrict__ out, Rows&& rows)
{
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t qc = q < Q ? q : Q - 1;
    const int r = rec[qc];
    const bool live = track_live(q, qc, Q, r, R, INTERP ? 1 : 0, mask, F);
    if (!__any(live)) {
        if (q < Q) out[q] = __builtin_nan("");
        return;
    }
    double v[2];
    rows(C + (int64_t)(live ? r : 0) * M.N, lat[qc], lon[qc], alt[qc], v);      // (a live lane exists: row 0 does)
    double val = v[0];
    if (INTERP) {
        const double w = wgt[qc];
        val = (1.0 - w) * v[0] + w * v[1];
    }
    if (q < Q) out[q] = live ? val : __builtin_nan("");
}

// The per-lane form for the orders without a fast kernel (and VINTERP_EVAL=generic): the generic sink reads the lane's own
// prepared row, or its two rows, from global memory.  Correct, not tuned.
template <int LCAP, int KCAP, bool INTERP>
__global__ __launch_bounds__(BLOCK) void k_track_sph(SphDev M, int64_t Q, const double* __restrict__ lat,
                                                     const double* __restrict__ lon, const double* __restrict__ alt,
                                                     const int* __restrict__ rec, const double* __restrict__ wgt, int R,
                                                     const double* __restrict__ Cp, const unsigned char* __restrict__ mask,
                                                     int F, double* __restrict__ out)
{
    track_per_lane<INTERP>(M, Q, lat, lon, alt, rec, wgt, R, Cp, mask, F, out,
                           [&](const double* __restrict__ Cr, double la, double lo, double al, double* v) {
                               eval_point<LCAP, KCAP, INTERP ? 2 : 1>(M, sph_geom(M, la, lo, al), Cr, v);
                           });
}

// K2t for the RBF model, per lane: the lane's own coefficient row, or its two rows, from global memory
template <bool INTERP>
__global__ __launch_bounds__(BLOCK) void k_track_rbf(RbfDev M, int64_t Q, const double* __restrict__ lat,
                                                     const double* __restrict__ lon, const double* __restrict__ alt,
                                                     const int* __restrict__ rec, const double* __restrict__ wgt, int R,
                                                     const double* __restrict__ C, const unsigned char* __restrict__ mask, int F,
                                                     double* __restrict__ out)
{
    track_per_lane<INTERP>(M, Q, lat, lon, alt, rec, wgt, R, C, mask, F, out,
                           [&](const double* __restrict__ Cr, double la, double lo, double al, double* v) {
                               double X, Y, Z;
                               geodetic2ecef(la, lo, al, X, Y, Z);
                               rbf_rows<INTERP>(M, Cr, X, Y, Z, v[0], v[1]);
                           });
}

// ---------------------------------------------------------------------------------------------
// K2tg: gradients along a trajectory, every point at its own time (vi_eval_track_grad_f64): k_grad_sph's chains (grad_point) in
// K2t's frame.  A workgroup is ONE wave of 64 points; it finds the lowest and highest row its live lanes need (shuffles: nothing
// assumes sorted input) and stages a window of TT RAW coefficient rows from the lowest one in LDS - the gradient needs
// scale[r] P(nu) and scale1[r] P(nu + 1), so the rows k_prep_coef prepares for the density do not serve; rows past R - 1 are
// zero-filled and never selected - then runs the chains once for 3 TT accumulators, the coefficients read from LDS at
// wave-uniform addresses.  Each lane takes the triple of its own row (the pair of triples, when blending) by compare-select,
// never a product with zero, from the one window that holds its rows; windows follow each other as in K2t (one shared row when
// blending) until the wave's highest row is covered.  Every row's accumulators see the terms in the order k_grad_sph adds them,
// whatever the row's place in the window: a point's bits depend on the point, its row(s) and w only.  With ENU the point's
// matrix (enu_frame) turns the finished triple in the epilogue.  A wave without a live lane leaves before anything is staged.
constexpr int TRACK_GRAD_TT = 4;    // the window

template <int TT>
struct GradTrackSink {
    const double* shC;      // LDS [TT][N], raw rows
    int N;
    double az[TT], at[TT], ap[TT];
    __device__ __forceinline__ void term(int n, double tz, double tt, double tp, double L0k, double L1k)
    {
        const double gz = tz * (L0k + 2.0 * L1k), gt = tt * L0k, gp = tp * L0k;
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            const double cf = shC[t * N + n];
            az[t] = fma(gz, cf, az[t]);
            at[t] = fma(gt, cf, at[t]);
            ap[t] = fma(gp, cf, ap[t]);
        }
    }
};

template <int LCAP, int KCAP, int TT, bool INTERP, bool ENU>
__global__ __launch_bounds__(TRACK_BLOCK) void k_track_grad_sph(SphDev M, int64_t Q, const double* __restrict__ lat,
                                                                const double* __restrict__ lon, const double* __restrict__ alt,
                                                                const int* __restrict__ rec, const double* __restrict__ wgt, int R,
                                                                const double* __restrict__ C,
                                                                const unsigned char* __restrict__ mask, int F,
                                                                double* __restrict__ out)
{
    constexpr int PAIR = INTERP ? 1 : 0;
    constexpr int STEP = TT - PAIR;                     // rows from one window to the next
    static_assert(STEP >= 1, "a blending window holds at least two rows");
    extern __shared__ __align__(16) double sh[];        // [TT][N] the window
    const double nan = __builtin_nan("");
    const int64_t q = (int64_t)blockIdx.x * TRACK_BLOCK + threadIdx.x;
    const int64_t qc = q < Q ? q : Q - 1;
    const int r = rec[qc];
    const bool live = track_live(q, qc, Q, r, R, PAIR, mask, F);
    if (!__any(live)) {                                 // (the whole workgroup: no barrier has been met)
        if (q < Q) out[3 * q] = out[3 * q + 1] = out[3 * q + 2] = nan;
        return;
    }
    int lo = live ? r : 0x7fffffff, hi = live ? r + PAIR : -1;
#pragma unroll
    for (int off = TRACK_BLOCK / 2; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, TRACK_BLOCK));
        hi = max(hi, __shfl_xor(hi, off, TRACK_BLOCK));
    }
    lo = __builtin_amdgcn_readfirstlane(lo);            // 0 <= lo <= hi <= R - 1
    hi = __builtin_amdgcn_readfirstlane(hi);
    const int N = M.N;
    const Geom g = sph_geom(M, lat[qc], lon[qc], alt[qc]);
    const double w = INTERP ? wgt[qc] : 0.0;
    double vz = nan, vt = nan, vp = nan;
    for (int base = lo;; base += STEP) {                // lo <= base <= hi
        __syncthreads();                                // the pass before has read the window
        for (int i = threadIdx.x; i < TT * N; i += TRACK_BLOCK) sh[i] = i / N < R - base ? C[(int64_t)base * N + i] : 0.0;
        __syncthreads();
        GradTrackSink<TT> S;
        S.shC = sh;
        S.N = N;
#pragma unroll
        for (int t = 0; t < TT; ++t) S.az[t] = S.at[t] = S.ap[t] = 0.0;
        grad_point<LCAP, KCAP>(M, g, S);
        const int d = live ? r - base : -1;             // the lane's row in this window
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            if (d == t) { a0 = S.az[t]; a1 = S.at[t]; a2 = S.ap[t]; }
            if (INTERP && d + 1 == t) { b0 = S.az[t]; b1 = S.at[t]; b2 = S.ap[t]; }
        }
        if (d >= 0 && d < STEP) {
            vz = INTERP ? (1.0 - w) * a0 + w * b0 : a0;
            vt = INTERP ? (1.0 - w) * a1 + w * b1 : a1;
            vp = INTERP ? (1.0 - w) * a2 + w * b2 : a2;
        }
        if (hi - base <= TT - 1) break;                 // wave-uniform
    }
    if (ENU) {
        double Fm[9];
        enu_frame(M, g, lat[qc], lon[qc], Fm);
        const double gz = vz, gt = vt, gp = vp;
        vz = fma(Fm[0], gz, fma(Fm[1], gt, Fm[2] * gp));
        vt = fma(Fm[3], gz, fma(Fm[4], gt, Fm[5] * gp));
        vp = fma(Fm[6], gz, fma(Fm[7], gt, Fm[8] * gp));
    }
    if (q < Q) {
        out[3 * q] = live ? vz : nan;
        out[3 * q + 1] = live ? vt : nan;
        out[3 * q + 2] = live ? vp : nan;
    }
}

// The points, records and hull mask of a K2t or K2tg launch: w == nullptr is nearest mode.
struct TrackArgs {
    int64_t Q;
    const double *lat, *lon, *alt;
    const int* rec;
    const double* w;
    int R;
    const unsigned char* mask;
    int F;
    double* out;
};

// one launch on the points of t, a thread per point in workgroups of `block`; C: the R rows the kernel reads (prepared for K2t's
// sphharmlag kernels, raw for the others)
template <class K, class Dev>
int launch_track(vi_model* m, K kernel, int block, size_t lds, const Dev& dev, const TrackArgs& t, const double* C)
{
    return vi_launch(kernel, dim3(nblocks(t.Q, block)), dim3(block), lds, m->ctx->stream, dev, t.Q, t.lat, t.lon, t.alt, t.rec, t.w,
                     t.R, C, t.mask, t.F, t.out);
}

}  // namespace

// Densities along a trajectory (include/vinterp.h): K2t.  The hull pass and the coefficient preparation of vi_eval_f64 (all R
// rows prepared once into m->d_coef), then one launch: k_track_sph_fast for the orders of vi_eval_f64's fast list, the per-lane
// kernels for every other order, VINTERP_EVAL=generic and the RBF model.  fp64 chains whatever vi_model_set_eval_precision set.
extern "C" int vi_eval_track_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                 const int32_t* d_rec, const double* d_w, int64_t R, const double* d_C, const double* d_hull_eq,
                                 int32_t F, double hull_tol, double* d_out)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_rec && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && R >= 0 && F >= 0, "negative size");
    VI_REQUIRE_RECORDS(R, d_C, "coefficients");
    VI_REQUIRE(Q <= (int64_t)TRACK_BLOCK * 0x7fffffffLL, "more points than one launch takes");
    VI_REQUIRE_HULL(F, d_hull_eq);
    if (Q == 0) return VI_OK;
    VI_HIP(hipSetDevice(m->ctx->device));
    const bool sph = m->kind == VI_MODEL_SPHHARMLAG;
    // (R = 0 prepares no coefficients: every point is NaN, no kernel reads a row)
    const int rc = prepare_call(m, Q, d_lat, d_lon, d_alt, d_hull_eq, F, hull_tol, sph ? R : 0, d_C);
    if (rc != VI_OK) return rc;
    const TrackArgs t{Q, d_lat, d_lon, d_alt, d_rec, d_w, (int)R, F > 0 ? m->d_mask : nullptr, (int)F, d_out};
    EvalTimer timer(m->ctx);
    return with_flag(d_w != nullptr, [&](auto interp) {
        if (!sph) return launch_track(m, k_track_rbf<interp>, BLOCK, 0, m->rbf, t, d_C);
        int rcf;
        if (fast_eval_fits(m, TRACK_TT) && at_fast_order(m, &rcf, [&](auto l, auto k) {
                return launch_track(m, k_track_sph_fast<l, k, TRACK_TT, interp>, TRACK_BLOCK,
                                    chain_lds_bytes(m->nvmax0 + 1, l, (size_t)TRACK_TT * m->N), m->sph, t, m->d_coef);
            }))
            return rcf;
        return at_order_cap(m, "vi_eval_track_f64", [&](auto lc, auto kc) {
            return launch_track(m, k_track_sph<lc, kc, interp>, BLOCK, 0, m->sph, t, m->d_coef);
        });
    });
}

// Gradients along a trajectory (include/vinterp.h): K2tg.  The hull pass of vi_eval_track_f64 and no coefficient preparation -
// the kernel reads the R raw rows of d_C -, then one launch at the compiled gradient order that holds the model's.
extern "C" int vi_eval_track_grad_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                      const int32_t* d_rec, const double* d_w, int64_t R, const double* d_C,
                                      const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame, double* d_out)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_rec && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && R >= 0 && F >= 0, "negative size");
    VI_REQUIRE_RECORDS(R, d_C, "coefficients");
    VI_REQUIRE(Q <= (int64_t)TRACK_BLOCK * 0x7fffffffLL, "more points than one launch takes");
    VI_REQUIRE_HULL(F, d_hull_eq);
    VI_REQUIRE_FRAME(frame);
    int rc = grad_model_check(m, "vi_eval_track_grad_f64");
    if (rc != VI_OK || Q == 0) return rc;
    VI_HIP(hipSetDevice(m->ctx->device));
    return at_grad_cap(m, "vi_eval_track_grad_f64", [&](auto lc, auto kc) -> int {
        rc = prepare_call(m, Q, d_lat, d_lon, d_alt, d_hull_eq, F, hull_tol, 0, nullptr);
        if (rc != VI_OK) return rc;
        const TrackArgs t{Q, d_lat, d_lon, d_alt, d_rec, d_w, (int)R, F > 0 ? m->d_mask : nullptr, (int)F, d_out};
        const size_t lds = (size_t)TRACK_GRAD_TT * m->N * sizeof(double);       // the window: at most 4 x 1152 doubles, 36 KB
        EvalTimer timer(m->ctx);
        return with_flag(d_w != nullptr, [&](auto interp) {
            return with_flag(frame == VI_FRAME_ENU, [&](auto enu) {
                return launch_track(m, k_track_grad_sph<lc, kc, TRACK_GRAD_TT, interp, enu>, TRACK_BLOCK, lds, m->sph, t, d_C);
            });
        });
    });
}

// Standard errors along a trajectory (include/vinterp.h).  The hull pass of vi_eval_track_f64 for all points, then per chunk:
// the basis columns of vi_eval_basis_f64 (its builder and its mask kernel: the same bits) into the context workspace, and
// vi_eval_records_err_f64's routes on them - vi_eval_grad_cov_f64's scheme with the covariance chosen per point.  A chunk
// border inside a run of records changes no bits: a point's bits do not depend on the other points.
extern "C" int vi_eval_track_err_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                     const int32_t* d_rec, const double* d_w, int64_t R, const double* d_dC,
                                     const double* d_hull_eq, int32_t F, double hull_tol, double* d_out)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_rec && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && R >= 0 && F >= 0, "negative size");
    VI_REQUIRE_RECORDS(R, d_dC, "covariances");
    VI_REQUIRE_HULL(F, d_hull_eq);
    if (Q == 0) return VI_OK;
    VI_HIP(hipSetDevice(m->ctx->device));
    int rc = prepare_call(m, Q, d_lat, d_lon, d_alt, d_hull_eq, F, hull_tol, 0, nullptr);
    if (rc != VI_OK) return rc;
    const int64_t chunk = track_err_chunk(m->N, Q);
    double *Y, *none, *work;
    if ((rc = track_err_workspace(m, Q, chunk, d_out, 0, &Y, &none, &work)) != VI_OK) return rc;
    EvalTimer timer(m->ctx);
    return for_chunks(Q, chunk, [&](int64_t q0, int64_t qc) {
        int rc = vi_basis_f64(m, qc, d_lat + q0, d_lon + q0, d_alt + q0, Y, 1, qc);
        if (rc == VI_OK && F > 0) rc = mask_basis(m, qc, m->d_mask + q0, Y);
        if (rc != VI_OK) return rc;
        return vi_records_err(m, qc, Y, d_rec + q0, d_w ? d_w + q0 : nullptr, R, d_dC, d_out + q0, work);
    });
}

// Gradient covariances along a trajectory (include/vinterp.h).  The hull pass of vi_eval_track_f64 for all points, then per
// chunk: the planar gradient basis of the chunk into the context workspace by the launcher of vi_eval_grad_basis_f64, as
// vi_eval_grad_cov_f64 builds it - the same bits per point, the hull's NaN columns and the frame folded in -, and
// vi_eval_records_gradcov_f64's routes on it.  At most 256 MB of gradient basis per chunk (vi_forms_chunk);
// VINTERP_TRACK_GRADCOV_CHUNK: a smaller chunk (tests: several chunks at a small Q).  A chunk border inside a run of records
// changes no bits: a point's bits do not depend on the other points.
extern "C" int vi_eval_track_grad_cov_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                          const int32_t* d_rec, const double* d_w, int64_t R, const double* d_dC,
                                          const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame, double* d_out)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_rec && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && R >= 0 && F >= 0, "negative size");
    VI_REQUIRE_RECORDS(R, d_dC, "covariances");
    VI_REQUIRE_HULL(F, d_hull_eq);
    VI_REQUIRE_FRAME(frame);
    int rc = grad_model_check(m, "vi_eval_track_grad_cov_f64");
    if (rc != VI_OK || Q == 0) return rc;
    GradcovChunks k;
    rc = gradcov_setup(m, "VINTERP_TRACK_GRADCOV_CHUNK", true, Q, d_lat, d_lon, d_alt, d_hull_eq, F, hull_tol, &k);
    if (rc != VI_OK) return rc;
    EvalTimer timer(m->ctx);
    return for_chunks(Q, k.chunk, [&](int64_t q0, int64_t qc) -> int {
        const int rc = launch_grad_resident(m, "vi_eval_track_grad_cov_f64", qc, d_lat + q0, d_lon + q0, d_alt + q0,
                                            F > 0 ? m->d_mask + q0 : nullptr, frame, k.G);
        if (rc != VI_OK) return rc;
        return vi_records_gradcov(m, qc, k.G, d_rec + q0, d_w ? d_w + q0 : nullptr, R, d_dC, d_out + q0, Q, k.work);
    });
}
