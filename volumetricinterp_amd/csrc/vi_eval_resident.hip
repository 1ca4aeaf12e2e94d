// K2r: evaluation of many timesteps on one grid from the RESIDENT basis matrix of the grid (vi_eval_basis_f64):
//
//   out[t][q] = sum_n C[t][n] * Y[n][q]        (Estimate.__call__, estimate.py:110-123, once per timestep in the reference)
//
// a matrix product with a short inner dimension (N = 144 at the default order) and a very long one (Q = 2^24 points of a
// 256^3 grid), on the fp64 matrix cores: per k-step of four basis functions one v_mfma_f64_16x16x4 per 16 x 16
// (timestep, point) tile, D[16 t][16 q] += A[16 t][4 n] * B[4 n][16 q].
//
// Work of a wave: 64 timesteps x 64 points = 4 x 4 tiles, 128 accumulator registers, 16 independent MFMA per k-step (no
// accumulator is touched again before 15 others have been issued).
//  * B comes straight from HBM / L2, 32 bytes per lane and k-step: lane (p = lane & 15, g = lane >> 4) reads the FOUR
//    consecutive points 4p .. 4p + 3 of basis row 4 ks + g and uses them as its column p of the four column tiles - tile j
//    holds the points 4p + j.  A row of 16 lanes reads 512 contiguous bytes, and on the way out each lane stores its four
//    points of a timestep as one 32-byte piece of that timestep's row (the 16 lanes: 512 contiguous bytes).  The loads of a
//    stage of four k-steps are issued before the MFMAs of the previous stage (two register buffers): a k-step is
//    16 x 64 = 1024 matrix-core cycles.
//  * A is the coefficient tile of the workgroup's 64 timesteps, laid out in LDS in operand order once per workgroup
//    ([k-step][row tile][lane]: ds_read_b64 at lane * 8, linear and conflict-free) and reused for `groups` x 256 points:
//    73 KB at N = 144, two workgroups per CU (one computes while the other sets up its tile).
//  * HBM: Y is 0.15 B per flop at 64 timesteps per pass, so the tiles of the SAME points for different timesteps must meet
//    in a cache.  Workgroups go round-robin over the 8 XCDs (each with its own L2): block b runs on XCD b % 8, so the
//    timestep tiles of one group of points get the block indices 8 apart - same XCD, launched together - and Y leaves HBM
//    once per call, whatever the number of timesteps.
//  * Points outside the hull are NaN columns of Y.  The 32-byte pieces that hold nothing else are not multiplied: live list,
//    see k_eval_resident below (VINTERP_K2R_LIVE=0: every piece is).
// Bound: the fp64 matrix peak (78.6 TF): 2 N flop per point-timestep of the live pieces against 8 (N / T_call + 1) bytes.
#include "vi_common.h"
#include "vi_solver.h"

#include <cstdlib>
#include <cstring>

namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int RT = 4;        // row tiles (16 timesteps each) per wave
constexpr int PF = 4;        // k-steps of B in flight
constexpr int LIVE_BATCH = 32;                       // groups of 256 points per live list
constexpr int LIVE_PIECES = LIVE_BATCH * 64;         // 32-byte pieces per live list (16-bit local indices)

// coefficient tile in operand order: shA[(ks * RT + i) * 64 + (g * 16 + p)] = C[t0 + 16 i + p][4 ks + g]
// (read along the coefficient rows - contiguous -, written to where the operand order wants them)
__device__ __forceinline__ void stage_coeffs(double* shA, int tid, int N, int KSp, int64_t T, int64_t t0, const double* __restrict__ C)
{
    const int Np = 4 * KSp;
    for (int e = tid; e < 16 * RT * Np; e += 256) {
        const int tl = e / Np, n = e - tl * Np;
        const int64_t t = t0 + tl;
        shA[((n >> 2) * RT + (tl >> 4)) * 64 + ((n & 3) * 16 + (tl & 15))] = (t < T && n < N) ? C[t * N + n] : 0.0;
    }
}

// 64 timesteps x 16 pieces of four points: lane (p, g) holds the piece at qa (valid: it exists; the others read the first
// points of Y and store nothing)
template <bool PAD>
__device__ __forceinline__ void tile_product(const double* shA, int lane, int g, int N, int KS, int KSp, int64_t Q, int64_t T,
                                             int64_t t0, int64_t qa, bool valid, const double* __restrict__ Y,
                                             double* __restrict__ out)
{
    const double* yp = Y + (valid ? qa : 0);
    v4f64 D[RT][4];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) D[i][j] = (v4f64){0.0, 0.0, 0.0, 0.0};
    // B in two named buffers of PF k-steps: while the MFMAs of one run, the loads of the next stage are in flight (written
    // as a ring of registers replaced one by one, the compiler moved every load next to its use: no distance at all)
    v4f64 yA[PF], yB[PF];
    auto load_stage = [&](v4f64 (&y)[PF], int ks0) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int n = 4 * (ks0 + u) + g;
            const bool in = ks0 + u < KS && n < N;
            const v4f64 v = *reinterpret_cast<const v4f64*>(yp + (int64_t)(in ? n : 0) * Q);
            // the rows from N on read row 0 and are set to zero: their zero coefficients times an infinite basis value
            // would be NaN.  Without padding (N % 16 == 0, the default order) the kernel has no select at all: with one
            // it measured 6 - 8 % slower at N = 144.
            y[u] = (PAD && !in) ? (v4f64){0.0, 0.0, 0.0, 0.0} : v;
        }
    };
    auto mfma_stage = [&](const v4f64 (&y)[PF], int ks0) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            double a[RT];
#pragma unroll
            for (int i = 0; i < RT; ++i) a[i] = shA[((ks0 + u) * RT + i) * 64 + lane];
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                D[i][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], y[u].x, D[i][0], 0, 0, 0);
                D[i][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], y[u].y, D[i][1], 0, 0, 0);
                D[i][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], y[u].z, D[i][2], 0, 0, 0);
                D[i][3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], y[u].w, D[i][3], 0, 0, 0);
            }
        }
    };
    load_stage(yA, 0);
    int ks0 = 0;
    for (; ks0 + PF < KSp; ks0 += 2 * PF) {
        load_stage(yB, ks0 + PF);
        asm volatile("" ::: "memory");
        mfma_stage(yA, ks0);
        if (ks0 + 2 * PF < KSp) load_stage(yA, ks0 + 2 * PF);
        asm volatile("" ::: "memory");
        mfma_stage(yB, ks0 + PF);
    }
    if (ks0 < KSp) mfma_stage(yA, ks0);
    // D[i][j][v]: timestep t0 + 16 i + g + 4 v, point qa + j
    if (valid) {
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t t = t0 + 16 * i + g + 4 * v;
                if (t < T)
                    *reinterpret_cast<v4f64*>(out + t * Q + qa) = (v4f64){D[i][0][v], D[i][1][v], D[i][2][v], D[i][3][v]};
            }
    }
}

// PAD: 4 KSp > N, the last k-steps hold rows past the basis.
// LIVE: the product runs over the 32-byte pieces (four consecutive points) that carry a point inside the hull.  A piece whose
// four values of basis row 0 are all NaN gives NaN at every timestep whatever the coefficients are (the first product of the
// chain is NaN): it is dead, gets its NaNs stored directly and costs neither matrix-core work nor reads of the other N - 1
// rows.  Liveness is read from row 0 of THIS call's Y, per batch of LIVE_BATCH groups; the indices of the live pieces are
// compacted into LDS in ascending order, and the waves take chunks of 16 of them round-robin where they took their 64 points of
// a group.  Every other piece (all inside, or mixed) runs exactly the chain of the plain loop: same bits.  A dead piece holds the
// bits the chain gives for the NaN that vi_eval_basis_f64 writes (0x7FF8000000000000); for a row-0 NaN of another payload or
// sign in a caller's own Y the plain loop carries that NaN through and the list stores the canonical one - NaN either way.
template <bool PAD, bool LIVE>
__global__ __launch_bounds__(256, 2) void k_eval_resident(int N, int KSp, int64_t Q, int64_t T, int ntt, int groups, int64_t npg,
                                                          const double* __restrict__ Y, const double* __restrict__ C,
                                                          double* __restrict__ out)
{
    extern __shared__ __align__(16) double shA[];            // [KSp][RT][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = lane & 15, g = lane >> 4;
    // XCD-aware decode: the timestep tiles of a group of points on one XCD, next to each other in launch order
    const int64_t bid = blockIdx.x;
    const int xcd = (int)(bid & 7);
    const int64_t r = bid >> 3;
    const int tt = (int)(r % ntt);
    // (with the live list the eight groups of points of a row of blocks rotate over the XCDs from row to row: on a grid whose
    // altitude-longitude planes are a multiple of eight groups - 256^3: eight groups per latitude - XCD k would otherwise
    // always get the k-th eighth of the longitudes, the outer ones mostly outside the hull, the inner ones mostly inside:
    // 1.24 times the mean live work on the busiest XCD of the bench grid, 1.002 rotated)
    const int64_t row = r / ntt;
    const int64_t pg = row * 8 + (LIVE ? (int)((xcd + row) & 7) : xcd);
    if (pg >= npg) return;
    const int64_t t0 = (int64_t)tt * (16 * RT);
    const int KS = (N + 3) >> 2;                              // k-steps that carry basis functions (the rest is padding)
    if constexpr (!LIVE) {
        stage_coeffs(shA, tid, N, KSp, T, t0, C);
        __syncthreads();
        for (int grp = 0; grp < groups; ++grp) {
            const int64_t qa = (pg * groups + grp) * 256 + wave * 64 + 4 * p;      // this lane's four points
            const bool valid = qa < Q;                                              // Q % 4 == 0: all four or none
            if (__ballot(valid) == 0) break;
            tile_product<PAD>(shA, lane, g, N, KS, KSp, Q, T, t0, qa, valid, Y, out);
        }
    } else {
        __shared__ unsigned short shList[LIVE_PIECES];       // local indices of the live pieces of the batch, ascending
        __shared__ int shCnt[4];                              // live pieces per wave's share of the batch
        const int wv = __builtin_amdgcn_readfirstlane(wave);                       // uniform: the loops below are scalar
        const int nt = (int)((T - t0) < 16 * RT ? (T - t0) : 16 * RT);             // timesteps of this tile
        const v4f64 nan4 = {__builtin_nan(""), __builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
        bool staged = false;
        for (int gb0 = 0; gb0 < groups; gb0 += LIVE_BATCH) {
            const int64_t q0 = (pg * groups + gb0) * 256;                           // first point of the batch
            if (q0 >= Q) break;
            const int ng = groups - gb0 < LIVE_BATCH ? groups - gb0 : LIVE_BATCH;
            const int64_t left = (Q - q0) >> 2;
            const int np = left < (int64_t)ng * 64 ? (int)left : ng * 64;          // pieces of the batch (Q % 4 == 0)
            // (the lane index behind an empty asm: nothing of the list phase is hoisted out of the batch loop and kept in
            // registers across the product, which has none to spare)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            // ---- row 0 of the batch: wave w looks at the pieces [512 w, 512 w + 512), 64 per round
            unsigned lv = 0, dd = 0;                                                // bit `it`: this lane's piece is live / dead
            int cnt = 0;
#pragma unroll
            for (int it = 0; it < LIVE_PIECES / 256; ++it) {
                const int pc = wv * (LIVE_PIECES / 4) + it * 64 + ln;
                const bool ex = pc < np;
                const v4f64 y = *reinterpret_cast<const v4f64*>(Y + q0 + 4 * (ex ? pc : 0));
                const bool dead = y.x != y.x && y.y != y.y && y.z != y.z && y.w != y.w;
                const bool live = ex && !dead;
                lv |= (unsigned)live << it;
                dd |= (unsigned)(ex && dead) << it;
                cnt += __popcll(__ballot(live));
            }
            if (ln == 0) shCnt[wv] = cnt;
            __syncthreads();
            int base = 0, nlive = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int c = shCnt[w];
                base += w < wv ? c : 0;
                nlive += c;
            }
#pragma unroll
            for (int it = 0; it < LIVE_PIECES / 256; ++it) {
                const bool live = (lv >> it) & 1;
                const unsigned long long m = __ballot(live);
                if (live) shList[base + __popcll(m & ((1ull << ln) - 1))] = (unsigned short)(wv * (LIVE_PIECES / 4) + it * 64 + ln);
                base += __popcll(m);
            }
            __syncthreads();
            // ---- dead pieces: NaN at the timesteps of this tile (the bits the product gives for a column of NaNs as
            // k_mask_basis writes them; a row-0 NaN of another payload or sign in a caller's own Y gives this NaN too, where the
            // plain loop carries the caller's through), by the wave that looked at them, before the product (measured: after
            // it, or a round after each chunk, 4 % slower)
            for (int it = 0; it < LIVE_PIECES / 256; ++it) {
                const bool dead = (dd >> it) & 1;
                if (__ballot(dead) == 0) continue;
                double* o = out + t0 * Q + q0 + 4 * (wv * (LIVE_PIECES / 4) + it * 64 + ln);
                if (dead)
                    for (int tl = 0; tl < nt; ++tl) *reinterpret_cast<v4f64*>(o + (int64_t)tl * Q) = nan4;
            }
            if (nlive == 0) continue;
            if (!staged) {                                                          // a workgroup without a live piece never needs it
                int td = tid;
                asm volatile("" : "+v"(td));                                     // as ln above
                stage_coeffs(shA, td, N, KSp, T, t0, C);
                __syncthreads();
                staged = true;
            }
            // ---- live pieces: chunks of 16, the waves round-robin; lane (p, g) takes piece 16 chunk + p of the list
            const int nchunks = (nlive + 15) >> 4;
            for (int ch = wv; ch < nchunks; ch += 4) {
                const int idx = 16 * ch + p;
                const bool valid = idx < nlive;                                     // past the end of the list: no piece
                const int64_t qa = q0 + 4 * (int64_t)shList[valid ? idx : 0];
                // (the row group behind an empty asm, as ln above: the 16 row offsets t Q of the stores are formed per chunk,
                // not kept across the product; & 3 tells the compiler that it is not negative - one select per load address)
                int gc = g;
                asm volatile("" : "+v"(gc));
                gc &= 3;
                tile_product<PAD>(shA, lane, gc, N, KS, KSp, Q, T, t0, qa, valid, Y, out);
            }
        }
    }
}

bool use_live_list()
{
    static const bool plain = vi_env_is("VINTERP_K2R_LIVE", "0");
    return !plain;
}

bool use_own_kernel()
{
    static const bool blas = vi_env_is("VINTERP_EVAL_RESIDENT", "blas");
    return !blas;
}

}  // namespace

// out[t*Q + q] = sum_n Y[n*Q + q] C[t*N + n] by K2r; *handled = 0 when the shape is not the kernel's (the caller then uses the
// library): Q a multiple of 4 and the matrices 32-byte aligned (the 32-byte pieces), the coefficient tile within the LDS.
int vi_eval_resident_mfma(vi_ctx* c, int N, int64_t Q, int64_t T, const double* d_Y, const double* d_C, double* d_out, int* handled)
{
    *handled = 0;
    if (!use_own_kernel()) return VI_OK;
    const int KSp = (((N + 3) / 4 + PF - 1) / PF) * PF;
    const size_t shm = (size_t)KSp * RT * 64 * sizeof(double);
    if ((Q & 3) != 0 || (((uintptr_t)d_Y | (uintptr_t)d_out) & 31) != 0 || shm > 150 * 1024 || Q < 256) return VI_OK;
    const int ntt = (int)((T + 16 * RT - 1) / (16 * RT));
    // points per workgroup: 256 x groups - the coefficient tile (73 KB through L2) is set up once per workgroup
    // (measured, T = 256: 128^3 points 52 TF with 4 groups, 57 with 32; 256^3 the same from 16 up: as many as leave every CU
    // a few workgroups)
    int groups = (int)((Q >> 16) < 1 ? 1 : ((Q >> 16) > 32 ? 32 : (Q >> 16)));
    if (const char* e = getenv("VINTERP_K2R_GROUPS")) { const int g = atoi(e); if (g >= 1 && g <= 256) groups = g; }      // experiments
    const int64_t npg = (Q + (int64_t)256 * groups - 1) / ((int64_t)256 * groups);
    const int64_t nblk = ((npg + 7) / 8) * 8 * ntt;
    if (nblk > 0x7fffffffLL) return VI_OK;
    const bool pad = 4 * KSp > N;                                       // N % 16 != 0: rows past the basis
    // VINTERP_K2R_LIVE=0: the plain loop over every point (the live list: 4 KB + counters of LDS next to the tile)
    const bool live = use_live_list();
    auto kern = pad ? (live ? k_eval_resident<true, true> : k_eval_resident<true, false>)
                    : (live ? k_eval_resident<false, true> : k_eval_resident<false, false>);
    VI_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(256), shm, c->stream, N, KSp, Q, T, ntt, groups, npg, d_Y, d_C, d_out);
    VI_HIP(hipGetLastError());
    *handled = 1;
    return VI_OK;
}

// K2e: standard-error maps of many timesteps on the same resident grid (the `calcerr` output of estimate.py:139-145, for a
// batch of covariances):
//
//   err[t][q] = sqrt( sum_i sum_k Y[i][q] * dC[t][i][k] * Y[k][q] )
//
// The covariances are NOT symmetric (the fit's dC differs from its transpose by up to 1e-5 of its largest entry at the default
// order) and the form cancels by up to six decades, so the full matrix is what is evaluated.  In 16 x 16 blocks (NB = N / 16
// rounded up): with S_II = dC_II and S_IJ = dC_IJ + dC_JI^T for I < J, err^2 = sum_{I <= J} y_I^T S_IJ y_J - the same sum up
// to the rounding of one addition per entry, with NB (NB + 1) / 2 block products instead of NB^2 (45 of 81 at N = 144).
//  * S of the workgroup's timestep sits in LDS in operand order ([block (I, J)][k-step][lane], 90 KB at N = 144), staged once
//    per workgroup and reused for `groups` x 256 points; one workgroup of 8 waves per CU, two waves per SIMD.
//  * A wave takes 32 points as two 16-point column tiles: lane (p = lane & 15, g = lane >> 4) reads the TWO consecutive points
//    2p, 2p + 1 of basis row 16 J + 4 u + g (one 16-byte load; tile j holds the points 2p + j) - the B operand of k-step u of
//    block column J.
//  * Z_I = sum_{J >= I} S_IJ y_J accumulates with J descending, all NB accumulators live at the start (NB x 2 x 8 = 144
//    registers at N = 144).  Z_I is complete right after block column J = I, whose B registers still hold rows 16 I + 4 u + g:
//    exactly the rows (lane >> 4) + 4 v of Z_I's accumulator (f64 D layout: col = lane & 15, row = (lane >> 4) + 4 reg), so
//    y_I^T Z_I is lane-local and every Y value is loaded once per (timestep, point tile).  Two cross-lane adds (lanes p,
//    p + 16, p + 32, p + 48) and a sqrt finish the point.
//  * Workgroups in the XCD-aware order of K2r, one timestep each: the timesteps of one group of points run on one XCD together
//    and read its Y through the same L2.
// Bound: the fp64 matrix peak, N_p (N_p + 16) flop issued per point-timestep (N_p = 16 NB; 23 040 at N = 144) against
// 8 (N / T_concurrent + 1) bytes.
namespace {

typedef double v2f64 __attribute__((ext_vector_type(2)));

constexpr int ERR_WAVES = 8;                              // waves per workgroup
constexpr int ERR_PTS = ERR_WAVES * 32;                   // points per workgroup and group
constexpr int ERR_NBMAX = 9;                              // N <= 144

template <int NB>
__global__ __launch_bounds__(ERR_WAVES * 64) void k_eval_resident_err(int N, int64_t Q, int64_t T, int groups, int64_t npg,
                                                                      const double* __restrict__ Y, const double* __restrict__ dC,
                                                                      double* __restrict__ out)
{
    constexpr int NBLK = NB * (NB + 1) / 2;
    extern __shared__ __align__(16) double shS[];         // [block J (J + 1) / 2 + I][k-step u][lane]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4;
    const int64_t bid = blockIdx.x;
    const int xcd = (int)(bid & 7);
    const int64_t r = bid >> 3;
    const int64_t t = r % T;
    const int64_t pg = (r / T) * 8 + xcd;
    if (pg >= npg) return;
    // ---- S of timestep t in operand order: shS[(blk * 4 + u) * 64 + (g * 16 + p)] = S_IJ[16 I + p][16 J + 4 u + g]
    const double* D = dC + t * N * N;
    for (int e = tid; e < NBLK * 256; e += ERR_WAVES * 64) {
        const int l = e & 63, u = (e >> 6) & 3, blk = e >> 8;
        int J = 0;
        while ((J + 1) * (J + 2) / 2 <= blk) ++J;
        const int I = blk - J * (J + 1) / 2;
        const int i = 16 * I + (l & 15), k = 16 * J + 4 * u + (l >> 4);
        double v = 0.0;
        if (i < N && k < N) {
            v = D[(int64_t)i * N + k];
            if (I != J) v += D[(int64_t)k * N + i];
        }
        shS[e] = v;
    }
    __syncthreads();
    for (int grp = 0; grp < groups; ++grp) {
        const int64_t qa = (pg * groups + grp) * ERR_PTS + wave * 32 + 2 * (lane & 15);   // this lane's two points
        const bool valid = qa < Q;                                                         // Q even: both or none
        if (__ballot(valid) == 0) break;
        const double* yp = Y + (valid ? qa : 0);
        const double* yg = yp + (int64_t)g * Q;             // basis row g; row 16 J + 4 u + g is a uniform offset away
        v4f64 Z[NB][2];
#pragma unroll
        for (int I = 0; I < NB; ++I) Z[I][0] = Z[I][1] = (v4f64){0.0, 0.0, 0.0, 0.0};
        v2f64 y[2][4];                                     // B of block column J (y[J & 1]) and of the next one, in flight
        auto load = [&](v2f64 (&b)[4], int J) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double* src = yg + (int64_t)(16 * J + 4 * u) * Q;
                if (J < NB - 1) {
                    b[u] = *reinterpret_cast<const v2f64*>(src);
                } else {                                    // the last block column: rows from N on are zero padding
                    const bool in = 16 * J + 4 * u + g < N;
                    const v2f64 v = *reinterpret_cast<const v2f64*>(in ? src : yp);
                    b[u] = in ? v : (v2f64){0.0, 0.0};
                }
            }
        };
        double acc0 = 0.0, acc1 = 0.0;
        load(y[(NB - 1) & 1], NB - 1);
#pragma unroll
        for (int J = NB - 1; J >= 0; --J) {
            if (J > 0) load(y[(J - 1) & 1], J - 1);
            // scheduling barriers: the next block column's loads and one k-step's LDS reads in flight, not all of them (254 VGPRs
            // at NB = 9, no scratch)
            __builtin_amdgcn_sched_barrier(0);
            const v2f64(&b)[4] = y[J & 1];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int I = 0; I <= J; ++I) {
                    const double a = shS[((J * (J + 1) / 2 + I) * 4 + u) * 64 + lane];
                    Z[I][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[u].x, Z[I][0], 0, 0, 0);
                    Z[I][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[u].y, Z[I][1], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);        // the LDS reads of one k-step at a time (J + 1 register pairs)
            }
            // Z_J is complete; its row g + 4 v is basis row 16 J + 4 v + g, the one b[v] holds
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                acc0 = fma(Z[J][0][v], b[v].x, acc0);
                acc1 = fma(Z[J][1][v], b[v].y, acc1);
            }
        }
        acc0 += __shfl_xor(acc0, 16);
        acc1 += __shfl_xor(acc1, 16);
        acc0 += __shfl_xor(acc0, 32);
        acc1 += __shfl_xor(acc1, 32);
        if (valid && g == 0)                                // a negative form gives NaN, as np.sqrt does
            *reinterpret_cast<v2f64*>(out + t * Q + qa) = (v2f64){sqrt(acc0), sqrt(acc1)};
    }
}

template <int NB>
int launch_eval_resident_err(vi_ctx* c, int N, int64_t Q, int64_t T, const double* d_Y, const double* d_dC, double* d_out,
                             int* handled)
{
    const size_t shm = (size_t)(NB * (NB + 1) / 2) * 4 * 64 * sizeof(double);
    // points per workgroup: 256 x groups - S (up to 166 KB of covariance through L2) is staged once per workgroup, against
    // 22 us of matrix-core work per group of 256 points at N = 144
    int groups = (int)((Q >> 16) < 1 ? 1 : ((Q >> 16) > 8 ? 8 : (Q >> 16)));
    if (const char* e = getenv("VINTERP_K2E_GROUPS")) { const int gr = atoi(e); if (gr >= 1 && gr <= 256) groups = gr; }  // experiments
    const int64_t npg = (Q + (int64_t)ERR_PTS * groups - 1) / ((int64_t)ERR_PTS * groups);
    const int64_t nblk = ((npg + 7) / 8) * 8 * T;
    if (nblk > 0x7fffffffLL) return VI_OK;
    VI_HIP(hipFuncSetAttribute((const void*)k_eval_resident_err<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    hipLaunchKernelGGL(k_eval_resident_err<NB>, dim3((unsigned)nblk), dim3(ERR_WAVES * 64), shm, c->stream, N, Q, T, groups, npg,
                       d_Y, d_dC, d_out);
    VI_HIP(hipGetLastError());
    *handled = 1;
    return VI_OK;
}

}  // namespace

// out[t*Q + q] = sqrt(sum_ik Y[i*Q + q] dC[t*N*N + i*N + k] Y[k*Q + q]) by K2e; *handled = 0 when the shape is not the kernel's
// (the caller then uses the library): N <= 144, Q even and Y / out 16-byte aligned (the 16-byte pieces of two points).
int vi_eval_resident_err_mfma(vi_ctx* c, int N, int64_t Q, int64_t T, const double* d_Y, const double* d_dC, double* d_out,
                              int* handled)
{
    *handled = 0;
    if (!use_own_kernel()) return VI_OK;
    if (N < 1 || N > 16 * ERR_NBMAX || (Q & 1) != 0 || (((uintptr_t)d_Y | (uintptr_t)d_out) & 15) != 0) return VI_OK;
    switch ((N + 15) / 16) {
    case 1: return launch_eval_resident_err<1>(c, N, Q, T, d_Y, d_dC, d_out, handled);
    case 2: return launch_eval_resident_err<2>(c, N, Q, T, d_Y, d_dC, d_out, handled);
    case 3: return launch_eval_resident_err<3>(c, N, Q, T, d_Y, d_dC, d_out, handled);
    case 4: return launch_eval_resident_err<4>(c, N, Q, T, d_Y, d_dC, d_out, handled);
    case 5: return launch_eval_resident_err<5>(c, N, Q, T, d_Y, d_dC, d_out, handled);
    case 6: return launch_eval_resident_err<6>(c, N, Q, T, d_Y, d_dC, d_out, handled);
    case 7: return launch_eval_resident_err<7>(c, N, Q, T, d_Y, d_dC, d_out, handled);
    case 8: return launch_eval_resident_err<8>(c, N, Q, T, d_Y, d_dC, d_out, handled);
    default: return launch_eval_resident_err<9>(c, N, Q, T, d_Y, d_dC, d_out, handled);
    }
}
