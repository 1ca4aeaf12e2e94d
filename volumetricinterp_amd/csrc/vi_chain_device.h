// The Legendre chains run out of LDS at exact template orders (L = MAXL, K = MAXK, one degree group): the contraction of the
// tiled kernels (FastEval) and the start-up's consumption and the main segments for any sink: k_eval_sph_fast (vi_eval.hip),
// fast_chains of K2t and K2l (vi_basis.hip), MfmaSink (vi_eval_mfma.hip).  Their dynamic LDS: chain_lds_bytes (vi_common.h).
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

}  // namespace
