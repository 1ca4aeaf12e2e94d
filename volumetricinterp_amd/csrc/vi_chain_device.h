// The Legendre chains run out of LDS at exact template orders (L = MAXL, K = MAXK, one degree group): the contraction of the
// tiled kernels (FastEval) and the start-up's consumption and the main segments for any sink: k_eval_sph_fast (vi_eval.hip),
// fast_chains (below) of K2t and K2l (vi_track.hip, vi_slant.hip), MfmaSink (vi_eval_mfma.hip).  Their dynamic LDS: chain_lds_bytes (vi_common.h).
#pragma once
#include "vi_sph_device.h"

namespace {

// ---------------------------------------------------------------------------------------------
// K2 fast path: exact template orders (L = MAXL, K = MAXK), one degree group.  Differences to the generic
// kernel (k_eval_sph), all aimed at keeping the fp64 VALU busy (the kernel is VALU-bound):
//  * the recurrence table c[j][m] and the coefficient tile are staged in LDS once per workgroup and read as
//    wave-uniform (broadcast) ds_read_b128 - no dependent scalar loads in the inner loop;
//  * the triangular start-up (degrees j <= L) is unrolled at compile time, so the main degree loop has no
//    branches: 2 fp64 ops per (degree, order);
//  * the loop over l is unrolled, so each contraction knows l at compile time (no predication).
template <int L, int K, int TT>
struct FastEval {
    const double* shC;      // LDS [TT][L*L*K] coefficient tile, [t][r = l(l+1)+m][k]
    double Lk[K];
    double acc[TT];
    template <int l, typename CT>
    __device__ __forceinline__ void consume(const CT* cur, const double* cm, const double* sm)
    {
        constexpr int r0 = l * (l + 1);
        constexpr int NB = L * L * K;
#pragma unroll
        for (int m = 0; m <= l; ++m) {
            const double pc = (double)cur[m] * cm[m];
            const double ps = (double)cur[m] * sm[m];
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                const double* cp = shC + t * NB + (r0 + m) * K;
                const double* cn = shC + t * NB + (r0 - m) * K;
                double Sp = 0.0, Sm = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    Sp = fma(cp[k], Lk[k], Sp);
                    if (m > 0) Sm = fma(cn[k], Lk[k], Sm);
                }
                acc[t] = fma(pc, Sp, acc[t]);
                if (m > 0) acc[t] = fma(ps, Sm, acc[t]);
            }
        }
    }
};

// Sink: FastEval or MfmaSink - anything with consume<l>(cur, cm, sm)
template <int L, class Sink, int l>
struct ConsumeAt {
    // consume degree l if its integer part equals j (start-up phase only: j <= L)
    template <typename CT>
    __device__ static __forceinline__ void run(Sink& E, const int* nvl, int j, const CT* cur,
                                               const double* cm, const double* sm)
    {
        if (nvl[l] == j) E.template consume<l>(cur, cm, sm);
        if constexpr (l + 1 < L) ConsumeAt<L, Sink, l + 1>::run(E, nvl, j, cur, cm, sm);
    }
};

template <int L, class Sink, int l>
struct MainSegments {
    template <typename CT>
    __device__ static __forceinline__ void run(Sink& E, const CT* shc, const int* nvl, int& j, CT x,
                                               CT* cur, CT* prev, const double* cm, const double* sm)
    {
        const int jend = nvl[l];
        if (jend > L) {
#pragma unroll 2
            for (; j <= jend; ++j) {
                const CT* cj = shc + j * L;
#pragma unroll
                for (int m = 0; m < L; ++m) {
                    const CT nw = fma(x, cur[m], -(cj[m] * prev[m]));
                    prev[m] = cur[m];
                    cur[m] = nw;
                }
            }
            E.template consume<l>(cur, cm, sm);
        }
        if constexpr (l + 1 < L) MainSegments<L, Sink, l + 1>::run(E, shc, nvl, j, x, cur, prev, cm, sm);
    }
};

// The recurrence table shc[nj][L] of degree group G and nvl[l], the degree at which chain segment l ends, staged in LDS by the
// `threads` threads of the workgroup (the caller's barrier follows): K2t and K2l.  k_eval_sph_fast, k_eval_sph_mfma and
// k_eval_sph_split keep their loops: there the staging of the tile stands between the two, and the table takes the chain type.
__device__ __forceinline__ void stage_chain_table(const SphGroupDev& G, int nj, int L, double* shc, int* nvl, int threads)
{
    for (int i = threadIdx.x; i < nj * L; i += threads) shc[i] = G.c[i];
    for (int j = threadIdx.x; j < nj; j += threads) {
        const int l = G.pick[j];
        if (l >= 0) nvl[l] = j;
    }
}

// One pass of the chains of a point over the tile E.shC, for K2t (k_track_sph_fast, vi_track.hip): E.acc[t] = sum_n basis_n(point) *
// tile[t][n] without the factor exp(-z/2), t = 0 .. TT-1.  shc: the recurrence table [nj][L] in LDS, nvl[l]: the degree at which
// chain segment l ends.  The contraction, the start-up's consumption and the main segments are the pieces k_eval_sph_fast runs
// (FastEval, ConsumeAt, MainSegments); the triangular start-up around them is written out here as it is in that kernel, which
// keeps its own: calling this function from it changed the register allocation of most of its instantiations (e.g. (6, 4) at
// TT = 1: 95 -> 99 VGPRs, five -> four waves per SIMD), and that kernel is on the benchmarked path.
template <int L, int K, int TT, typename CT>
__device__ __forceinline__ void fast_chains(FastEval<L, K, TT>& E, const SphGroupDev& G, const Geom& g, const CT* shc,
                                            const int* nvl, int nj)
{
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
}

}  // namespace
