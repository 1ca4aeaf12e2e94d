// K2 for gfx950: the fused evaluation  out[t,q] = sum_n A[q,n] C[t,n]  (Estimate.__call__, estimate.py:110-123) that never
// writes A, the hull mask of the call folded in: the per-lane kernel for any order (k_eval_sph), the tiled kernel at the orders
// of the fast list (k_eval_sph_fast, on the benchmarked path) and the RBF model's (k_eval_rbf); entry vi_eval_f64.  One thread
// per point, tables addressed wave-uniformly: as vi_basis.hip says of all these kernels.
#include "vi_chain_device.h"
#include "vi_eval_host.h"

namespace {

// The per-lane form, for every order (and VINTERP_EVAL=generic).  Correct, not tuned.
template <int LCAP, int KCAP, int TT>
__global__ __launch_bounds__(BLOCK) void k_eval_sph(SphDev M, int64_t Q, const double* __restrict__ lat,
                                                    const double* __restrict__ lon, const double* __restrict__ alt,
                                                    int tcount, const double* __restrict__ Cp,
                                                    const unsigned char* __restrict__ mask, int F, double tol,
                                                    double* __restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t qc = q < Q ? q : Q - 1;
    const Geom g = sph_geom(M, lat[qc], lon[qc], alt[qc]);
    bool in = true;
    if (F > 0) {
        in = mask[qc] != 0;
        if (!__any(in && q < Q)) {            // whole wave outside the hull: skip the basis work
            if (q < Q)
                for (int t = 0; t < tcount; ++t) out[(int64_t)t * Q + q] = __builtin_nan("");
            return;
        }
    }
    double val[TT];
    eval_point<LCAP, KCAP, TT>(M, g, Cp, val);
    if (q < Q) {
#pragma unroll
        for (int t = 0; t < TT; ++t)
            if (t < tcount) out[(int64_t)t * Q + q] = in ? val[t] : __builtin_nan("");
    }
}

// CT = arithmetic type of the Legendre chains: double, or float for the fp32 variant of BASELINE configs[4]'s tolerance
// sweep (seeds, trigonometric and Laguerre factors and the contraction with the coefficients stay fp64)
template <int L, int K, int TT, typename CT>
__global__ __launch_bounds__(BLOCK) void k_eval_sph_fast(SphDev M, int64_t Q, const double* __restrict__ lat,
                                                         const double* __restrict__ lon, const double* __restrict__ alt,
                                                         int tcount, const double* __restrict__ Cp,
                                                         const unsigned char* __restrict__ mask, int F, double tol,
                                                         double* __restrict__ out)
{
    extern __shared__ __align__(16) double sh[];
    constexpr int NB = L * L * K;
    const SphGroupDev G = M.groups[0];
    const int nj = G.nvmax + 1;
    CT* shc = reinterpret_cast<CT*>(sh);                // [nj][L] recurrence table in the chain's arithmetic type
    double* shC = sh + ((nj * L + 1) & ~1);             // [TT][NB]
    int* nvl = reinterpret_cast<int*>(shC + TT * NB);   // [L]
    for (int i = threadIdx.x; i < nj * L; i += BLOCK) shc[i] = (CT)G.c[i];
    for (int i = threadIdx.x; i < TT * NB; i += BLOCK) shC[i] = i < tcount * NB ? Cp[i] : 0.0;
    for (int j = threadIdx.x; j < nj; j += BLOCK) {
        const int l = G.pick[j];
        if (l >= 0) nvl[l] = j;
    }
    __syncthreads();

    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t qc = q < Q ? q : Q - 1;
    const Geom g = sph_geom(M, lat[qc], lon[qc], alt[qc]);
    bool in = true;
    if (F > 0) {
        in = mask[qc] != 0;
        if (!__any(in && q < Q)) {
            if (q < Q)
                for (int t = 0; t < tcount; ++t) out[(int64_t)t * Q + q] = __builtin_nan("");
            return;
        }
    }
    FastEval<L, K, TT> E;
    E.shC = shC;
    laguerre<K>(K, g.z, E.Lk);
#pragma unroll
    for (int t = 0; t < TT; ++t) E.acc[t] = 0.0;
    double cm[L], sm[L];
    cm[0] = 1.0;
    sm[0] = 0.0;
#pragma unroll
    for (int m = 1; m < L; ++m) {
        cm[m] = cm[m - 1] * g.cphi - sm[m - 1] * g.sphi;
        sm[m] = sm[m - 1] * g.cphi + cm[m - 1] * g.sphi;
    }
    const CT x = (CT)g.x;
    const double zz = seed_arg(G, g.x);
    const bool intseed = (G.nterms == 0);
    CT cur[L], prev[L];
#pragma unroll
    for (int m = 0; m < L; ++m) { cur[m] = (CT)0.0; prev[m] = (CT)0.0; }
    double pmm = 1.0, spow = 1.0;
    // ---- start-up: degrees j = 0 .. L, compile-time triangular structure ------------------------------
#pragma unroll
    for (int j = 0; j <= L; ++j) {
#pragma unroll
        for (int m = 0; m < L; ++m) {
            if (j > m + 1) {
                if (j < nj) {
                    const CT nw = fma(x, cur[m], -(shc[j * L + m] * prev[m]));
                    prev[m] = cur[m];
                    cur[m] = nw;
                }
            } else if (j == m) {
                if (m > 0) { pmm *= -(2.0 * m - 1.0) * g.s; spow *= g.s; }
                if (intseed) cur[m] = (CT)pmm;
                else cur[m] = (CT)(G.pref[m] * spow * hyp_series(G.q + (size_t)m * G.nterms, G.nterms, zz));
            } else if (j == m + 1) {
                prev[m] = cur[m];
                if (intseed) cur[m] = (CT)(g.x * (2.0 * m + 1.0) * pmm);
                else cur[m] = (CT)(G.pref[L + m] * spow * hyp_series(G.q + (size_t)(L + m) * G.nterms, G.nterms, zz));
            }
        }
        ConsumeAt<L, FastEval<L, K, TT>, 0>::run(E, nvl, j, cur, cm, sm);
    }
    // ---- main: all chains in recurrence mode; one segment per degree l --------------------------------
    int j = L + 1;
    MainSegments<L, FastEval<L, K, TT>, 0>::run(E, shc, nvl, j, x, cur, prev, cm, sm);
    const double Ez = exp(-0.5 * g.z);
    if (q < Q) {
#pragma unroll
        for (int t = 0; t < TT; ++t)
            if (t < tcount) out[(int64_t)t * Q + q] = in ? Ez * E.acc[t] : __builtin_nan("");
    }
}

template <int TT>
__global__ __launch_bounds__(BLOCK) void k_eval_rbf(RbfDev M, int64_t Q, const double* __restrict__ lat,
                                                    const double* __restrict__ lon, const double* __restrict__ alt,
                                                    int tcount, const double* __restrict__ C,
                                                    const unsigned char* __restrict__ mask, int F, double tol,
                                                    double* __restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t qc = q < Q ? q : Q - 1;
    double X, Y, Z;
    geodetic2ecef(lat[qc], lon[qc], alt[qc], X, Y, Z);
    bool in = true;
    if (F > 0) {
        in = mask[qc] != 0;
        if (!__any(in && q < Q)) {
            if (q < Q)
                for (int t = 0; t < tcount; ++t) out[(int64_t)t * Q + q] = __builtin_nan("");
            return;
        }
    }
    double acc[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) acc[t] = 0.0;
    const double* __restrict__ c = M.centers;
    for (int n = 0; n < M.N; ++n) {         // (its own copy of rbf_gauss: with the call the instruction stream changes)
        const double dx = X - c[3 * n], dy = Y - c[3 * n + 1], dz = Z - c[3 * n + 2];
        const double e = exp(-(dx * dx + dy * dy + dz * dz) * M.inv_eps2);
#pragma unroll
        for (int t = 0; t < TT; ++t)
            if (t < tcount) acc[t] = fma(e, C[(size_t)t * M.N + n], acc[t]);
    }
    if (q < Q) {
#pragma unroll
        for (int t = 0; t < TT; ++t)
            if (t < tcount) out[(int64_t)t * Q + q] = in ? acc[t] : __builtin_nan("");
    }
}

template <int L, int K, typename CT>
int launch_eval_sph_fast(vi_model* m, int64_t Q, const double* lat, const double* lon, const double* alt, int64_t T,
                         const double* Cp, const unsigned char* hull, int F, double tol, double* out)
{
    const int N = m->N;
    auto shm = [&](int TT) { return chain_lds_bytes(m->nvmax0 + 1, L, (size_t)TT * N); };
    // per call, not cached: the attribute is per device and several device contexts may live in one process
    VI_HIP(hipFuncSetAttribute((const void*)k_eval_sph_fast<L, K, 16, CT>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    VI_HIP(hipFuncSetAttribute((const void*)k_eval_sph_fast<L, K, 4, CT>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    VI_HIP(hipFuncSetAttribute((const void*)k_eval_sph_fast<L, K, 1, CT>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    // timestep tiles of 16 / 4 / 1: the basis is recomputed once per tile, so a wide tile amortises it and the
    // contraction (2N flop per point-timestep) dominates.  Measured at 128^3, N = 144: 1.4e10 / 3.9e10 / 6.2e10
    // point-timesteps/s for tiles of 1 / 4 / 16 (a tile of 8 is slower than 16).  Whole tiles of 16 timesteps normally
    // never get here: vi_eval_mfma.hip contracts them on the matrix cores (1.2e11).
    const bool wide_ok = shm(16) <= 60 * 1024;
    return for_tiles<16, 4, 1>(T, [&](int w) { return w < 16 || wide_ok; }, [&](auto w, int64_t t) {
        hipLaunchKernelGGL((k_eval_sph_fast<L, K, w, CT>), dim3(nblocks(Q, BLOCK)), dim3(BLOCK), shm(w), m->ctx->stream, m->sph,
                           Q, lat, lon, alt, (int)w, Cp + t * N, hull, F, tol, out + t * Q);
    });
}

}  // namespace

// VINTERP_EVAL=generic switches the tiled kernels off: every order runs the per-lane kernels
bool use_fast_eval()
{
    static const bool generic = vi_env_is("VINTERP_EVAL", "generic");
    return !generic;
}

// Whether a model of one of the orders of the fast list (VI_FAST_ORDERS, vi_eval_host.h) runs the tiled kernels at a tile of TT timesteps: one degree group, and table plus
// tile within 60 KB of LDS.  The test is coarser than chain_lds_bytes - it counts neither the padding, the L ints nor the spare
// 16 bytes - and is not replaced by it, because it decides the route: at (2, 8), (3, 4) and (3, 2) with nvmax0 = 3774, 2510 and
// 2534 it admits a model whose exact size is 61 448 / 61 452 bytes (the launchers allow 64 KB), which the exact size turns away.
bool fast_eval_fits(const vi_model* m, int TT)
{
    return use_fast_eval() && m->sph.ngroups == 1 &&
           (size_t)(m->nvmax0 + 1) * m->sph.maxl * 8 + (size_t)TT * m->N * 8 < 60 * 1024;
}

// Arithmetic of the Legendre degree recurrences of the fused evaluation: 0 = fp64 (default), 1 = fp32 chains (seeds,
// trigonometric and Laguerre factors and the contraction stay fp64).  BASELINE configs[4]'s fp32-vs-fp64 tolerance sweep.
extern "C" int vi_model_set_eval_precision(vi_model* m, int32_t chain_f32)
{
    VI_REQUIRE(m, "null model");
    VI_REQUIRE(chain_f32 == 0 || chain_f32 == 1, "precision must be 0 (fp64) or 1 (fp32 chains)");
    if (chain_f32 && m->kind != VI_MODEL_SPHHARMLAG) {
        vi_set_error("vi_model_set_eval_precision: the fp32 variant exists for the sphharmlag model only");
        return VI_ERR_UNSUPPORTED;
    }
    m->chain_f32 = chain_f32 != 0;
    return VI_OK;
}

extern "C" int vi_eval_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                           int64_t T, const double* d_C, const double* d_hull_eq, int32_t F, double hull_tol,
                           double* d_out)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_C && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && T >= 0 && F >= 0, "negative size");
    VI_REQUIRE_HULL(F, d_hull_eq);
    if (Q == 0 || T == 0) return VI_OK;
    VI_HIP(hipSetDevice(m->ctx->device));
    const int N = m->N;
    const bool sph = m->kind == VI_MODEL_SPHHARMLAG;
    int rc = prepare_call(m, Q, d_lat, d_lon, d_alt, d_hull_eq, F, hull_tol, sph ? T : 0, d_C);
    if (rc != VI_OK) return rc;
    const unsigned char* d_mask = F > 0 ? m->d_mask : nullptr;
    EvalTimer timer(m->ctx);
    if (sph) {
        // whole tiles of 16 timesteps go to the matrix-core kernel (vi_eval_mfma.hip); the rest to the VALU kernels
        int64_t done = 0;
        if (use_fast_eval() && !m->chain_f32) {
            rc = vi_eval_sph_mfma(m, Q, d_lat, d_lon, d_alt, T, m->d_coef, d_mask, (int)F, d_out, &done);
            if (rc != VI_OK) return rc;
            if (done == T) return VI_OK;
        }
        const int64_t Tr = T - done;
        const double* coef = m->d_coef + done * N;
        double* outp = d_out + done * Q;
        if (use_fast_eval()) {                  // high orders: the chains in groups (vi_eval_split.hip)
            int handled = 0;
            rc = vi_eval_sph_split(m, Q, d_lat, d_lon, d_alt, Tr, coef, d_mask, (int)F, outp, &handled);
            if (rc != VI_OK || handled) return rc;
        }
        if (fast_eval_fits(m, 4)) {
            if (m->chain_f32) {     // fp32 Legendre chains (vi_model_set_eval_precision): the orders of the tolerance sweep
                if (at_fast_order<true>(m, &rc, [&](auto l, auto k) {
                        return launch_eval_sph_fast<l, k, float>(m, Q, d_lat, d_lon, d_alt, Tr, coef, d_mask, F, hull_tol, outp);
                    }))
                    return rc;
                vi_set_error("vi_eval_f64: no fp32-chain kernel for MAXL=%d MAXK=%d", m->sph.maxl, m->sph.maxk);
                return VI_ERR_UNSUPPORTED;
            }
            if (at_fast_order(m, &rc, [&](auto l, auto k) {
                    return launch_eval_sph_fast<l, k, double>(m, Q, d_lat, d_lon, d_alt, Tr, coef, d_mask, F, hull_tol, outp);
                }))
                return rc;
        }
        return at_order_cap(m, "vi_eval_f64", [&](auto lc, auto kc) {
            return for_tiles<4, 1>(Tr, [&](auto w, int64_t t) {
                hipLaunchKernelGGL((k_eval_sph<lc, kc, w>), dim3(nblocks(Q, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, m->sph, Q,
                                   d_lat, d_lon, d_alt, (int)w, coef + t * N, d_mask, F, hull_tol, outp + t * Q);
            });
        });
    }
    // the exponential of a (point, centre) pair is the cost (~20 of the ~28 fp64 operations per pair): it is computed once per
    // tile of timesteps, so the tile is as wide as the registers allow (16 accumulators; a tile of 4 recomputed every
    // exponential four times for 16 timesteps: 10.7 ms instead of 3.4 at 1000 centres x 128^3 points)
    return for_tiles<16, 4, 1>(T, [&](auto w, int64_t t) {
        hipLaunchKernelGGL(k_eval_rbf<w>, dim3(nblocks(Q, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, m->rbf, Q, d_lat, d_lon, d_alt,
                           (int)w, d_C + t * N, d_mask, F, hull_tol, d_out + t * Q);
    });
}

