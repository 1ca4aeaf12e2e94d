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
typedef double v2f64 __attribute__((ext_vector_type(2)));

// ---- the stores of K2r's densities, cache policy a compile-time constant per site ----------------------------------------------
// K2r writes as many bytes as it reads, nobody reads them again within the call, and every written line that stays in the XCD's
// L2 takes the place of a line of Y that the sibling timestep tiles of the same points are about to ask for.  The policies, as
// measured on the bench grid (profiles/r23_k2r_stores.txt; one call of 512 timesteps, 32.5 - 34.4 ms with plain stores):
#define VI_STORE_PLAIN  0    // global_store_dwordx4            write back
#define VI_STORE_SC1    1    // global_store_dwordx4 ... sc1    write through: a lane's two 16-byte halves leave L2 one by one as
                             //                                 partial writes, WRITE_SIZE doubles (53.5 ms at both sites)
#define VI_STORE_SC0SC1 2    // global_store_dwordx4 ... sc0 sc1   the same (53.6 ms)
#define VI_STORE_NT     3    // global_store_dwordx4 ... nt     write back, the line first in turn to leave: reads of Y - 11 .. - 25 %
// The two sites, each with its own constant (make EXTRA="-DVI_K2R_PRODUCT_STORE=3 -DVI_K2R_DEAD_STORE=0" builds a variant
// library to be selected with VINTERP_LIB; no run-time switch): the product stores of tile_product, 32 bytes per lane, and the
// NaN stores of the dead pieces in the LIVE branch of k_eval_resident, 16-byte chunks contiguous over the wave.  What ships: nt
// on the dead stores - whole lines from one instruction, written bytes unchanged, 29.0 - 29.3 ms - and plain product stores: nt
// there takes another 1.0 ms off (28.1 - 28.2) but a lane's halves then reach HBM apart more often, WRITE_SIZE + 7 %.
#ifndef VI_K2R_PRODUCT_STORE
#define VI_K2R_PRODUCT_STORE VI_STORE_PLAIN
#endif
#ifndef VI_K2R_DEAD_STORE
#define VI_K2R_DEAD_STORE VI_STORE_NT
#endif

// plain and nt are the compiler's own stores.  sc1 and sc0 sc1, kept for the record, are inline asm, not
// __builtin_amdgcn_raw_buffer_store_b128(..., aux): a buffer store wants a wave-uniform base and a 32-bit offset, one call's tile
// of densities spans 64 rows of Q doubles (8 GB on a 256^3 grid) and the lanes of the list path hold unrelated pieces - a
// descriptor per row group, offsets next to the 64-bit addresses and a plain path for the rows that do not fit 32 bits, where
// this is one route with the addresses the plain store has.  The compiler sees no store in an asm statement, so the statement
// itself ends with the wait states a 16-byte store needs before a VALU instruction may overwrite its data registers (s_nop 1),
// and the "memory" clobber orders it against the compiler's own loads and stores.
#define VI_STORE32_ASM(BITS)                                                                                                      \
    asm volatile("global_store_dwordx4 %0, %1, off" BITS "\n\tglobal_store_dwordx4 %0, %2, off offset:16" BITS "\n\ts_nop 1"      \
                 :: "v"(dst), "v"(lo), "v"(hi) : "memory")
#define VI_STORE16_ASM(BITS) asm volatile("global_store_dwordx4 %0, %1, off" BITS "\n\ts_nop 1" :: "v"(dst), "v"(v) : "memory")

template <int POLICY>
__device__ __forceinline__ void store32(double* dst, v4f64 v)
{
    static_assert(POLICY >= VI_STORE_PLAIN && POLICY <= VI_STORE_NT, "store policy");
    if constexpr (POLICY == VI_STORE_PLAIN) {
        *reinterpret_cast<v4f64*>(dst) = v;
    } else if constexpr (POLICY == VI_STORE_NT) {
        __builtin_nontemporal_store(v, reinterpret_cast<v4f64*>(dst));
    } else {
        const v2f64 lo = {v.x, v.y}, hi = {v.z, v.w};
        if constexpr (POLICY == VI_STORE_SC1) VI_STORE32_ASM(" sc1");
        else VI_STORE32_ASM(" sc0 sc1");
    }
}

template <int POLICY>
__device__ __forceinline__ void store16(double* dst, v2f64 v)
{
    static_assert(POLICY >= VI_STORE_PLAIN && POLICY <= VI_STORE_NT, "store policy");
    if constexpr (POLICY == VI_STORE_PLAIN) *reinterpret_cast<v2f64*>(dst) = v;
    else if constexpr (POLICY == VI_STORE_NT) __builtin_nontemporal_store(v, reinterpret_cast<v2f64*>(dst));
    else if constexpr (POLICY == VI_STORE_SC1) VI_STORE16_ASM(" sc1");
    else VI_STORE16_ASM(" sc0 sc1");
}

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

// 64 timesteps x 16 pieces of four points, the MFMA chain K2r and K2p share: lane (p, g) holds the piece at yp (row 0 of Y at
// its four points); on return D[i][j][v] is timestep t0 + 16 i + g + 4 v at point j of the piece
template <bool PAD>
__device__ __forceinline__ void tile_accumulate(const double* shA, int lane, int g, int N, int KS, int KSp, int64_t Q,
                                                const double* __restrict__ yp, v4f64 (&D)[RT][4])
{
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
}

// K2r's tile: lane (p, g) holds the piece at qa (valid: it exists; the others read the first points of Y and store nothing)
template <bool PAD>
__device__ __forceinline__ void tile_product(const double* shA, int lane, int g, int N, int KS, int KSp, int64_t Q, int64_t T,
                                             int64_t t0, int64_t qa, bool valid, const double* __restrict__ Y,
                                             double* __restrict__ out)
{
    v4f64 D[RT][4];
    tile_accumulate<PAD>(shA, lane, g, N, KS, KSp, Q, Y + (valid ? qa : 0), D);
    // D[i][j][v]: timestep t0 + 16 i + g + 4 v, point qa + j
    if (valid) {
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t t = t0 + 16 * i + g + 4 * v;
                if (t < T)
                    store32<VI_K2R_PRODUCT_STORE>(out + t * Q + qa, (v4f64){D[i][0][v], D[i][1][v], D[i][2][v], D[i][3][v]});
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
        const v2f64 nan2 = {__builtin_nan(""), __builtin_nan("")};
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
            // it, or a round after each chunk, 4 % slower).  The 64 pieces of a round are 2048 contiguous bytes of a row and every
            // dead one gets the same bits, so the lanes do not store their own piece (16 bytes at a stride of 32 per instruction:
            // half-written lines) but the 16-byte chunks ln and 64 + ln of the round, where those belong to a dead piece: an
            // instruction writes whole lines wherever a run of pieces is dead, and the same bytes in all.
#pragma unroll
            for (int it = 0; it < LIVE_PIECES / 256; ++it) {
                const unsigned long long m = __ballot((dd >> it) & 1);
                if (m == 0) continue;
                double* o = out + t0 * Q + q0 + 4 * (wv * (LIVE_PIECES / 4) + it * 64);   // the round's first piece
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int c = 64 * h + ln;                                          // chunk c: a half of piece c >> 1
                    if ((m >> (c >> 1)) & 1)
                        for (int tl = 0; tl < nt; ++tl) store16<VI_K2R_DEAD_STORE>(o + 2 * c + (int64_t)tl * Q, nan2);
                }
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


// ---- K2p: peak maps along the last axis of the grid, K2r with the stores replaced by a reduction ------------------------------
//
//   val[t][m] = max (min) over the non-NaN l of out[t][m L + l],  idx[t][m] = the first l that attains it
//
// (np.nanmax / first np.nanargmax of the density map along altitude: NmF2 and hmF2 of a (lat, lon, alt) grid), from the same
// stage_coeffs and the same MFMA chain as K2r - every product has K2r's bits - without a T x Q buffer.  L % 4 == 0: a 32-byte
// piece never straddles two columns.
//  * After the k-loop a lane holds four consecutive points x 16 timesteps.  Per timestep it reduces its four points in
//    registers, ascending with a strict compare (the first occurrence wins; a NaN never does), then the 16 lanes p of its DPP row
//    - 16 pieces ascending in q - run a segmented inclusive scan (row_shr 1, 2, 4, 8; no LDS), the lower lane winning a tie.
//    Segments are runs of equal key = column + 64-point block of the grid: the last lane of a run holds its reduction.
//  * Partials: one slot per (timestep, chunk parity, key).  Keys are unique per (column, block) because both grow along q
//    (S = M + Q / 64 keys, rounded up).  The live pieces of a 64-point block are contiguous in the ascending live list and at most
//    16: they fall into at most two consecutive chunks of 16, whose parities differ; batches begin on 256-point boundaries, so a
//    block never straddles two lists.  Every slot therefore has ONE writer - no atomics, and the result does not depend on the
//    order the workgroups run in or on how T is cut into calls.  A 0xFF memset marks every slot empty (a NaN, -1); dead pieces
//    and all-NaN runs store nothing.  Without the list (VINTERP_K2R_LIVE=0) a wave's 64 points are one block: parity 0.
//  * k_peak_finish folds the slots of a column (two per 64-point block it touches) with the total order "better value, or equal
//    value and lower index", which does not depend on the folding order.
// kind = min runs on the negated values (exact, and undone when the value is stored: the bits of the selected element).
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int x)
{
    return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, false);
}

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x)
{
    return __hiloint2double(dpp_i32<CTRL>(__double2hiint(x)), dpp_i32<CTRL>(__double2loint(x)));
}

// x takes the place of b: x is a number and b is none, or x is larger
__device__ __forceinline__ bool peak_better(double x, double b) { return x == x && !(x <= b); }

// ... or x equals b at a lower index (the total order of the cross-lane finish and of k_peak_finish)
__device__ __forceinline__ bool peak_takes(double x, int xi, double b, int bi)
{
    return x == x && (!(x <= b) || (x == b && xi < bi));
}

constexpr int ROW_SHR = 0x110, ROW_SHL = 0x100;              // DPP controls: lane p reads lane p - n / p + n of its row of 16

template <int OFF>
__device__ __forceinline__ void peak_scan_step(bool same, double& b, int& bi)
{
    const double pb = dpp_f64<ROW_SHR + OFF>(b);
    const int pi = dpp_i32<ROW_SHR + OFF>(bi);
    if (same && !peak_better(b, pb)) {                          // the lower lane keeps a tie
        b = pb;
        bi = pi;
    }
}

// all 64 lanes call this together (DPP reads neighbours): lane (p, g) holds the piece at qa in D, valid: it exists
__device__ __forceinline__ void peak_epilogue(const v4f64 (&D)[RT][4], int p, int g, int64_t qa, bool valid, int par, int64_t L,
                                              bool neg, int64_t S, int64_t T, int64_t t0, double* __restrict__ pval,
                                              int* __restrict__ pidx)
{
    const int64_t col = qa / L;
    const int l0 = (int)(qa - col * L);                        // position of the piece in its column
    const int key = valid ? (int)(col + (qa >> 6)) : -1;      // (the lanes past the end of the list: runs of their own, never stored)
    // (every DPP read before its condition: behind `p >= 1 &&` it would run with the lanes it reads from switched off)
    const int k1 = dpp_i32<ROW_SHR + 1>(key), k2 = dpp_i32<ROW_SHR + 2>(key), k4 = dpp_i32<ROW_SHR + 4>(key);
    const int k8 = dpp_i32<ROW_SHR + 8>(key), kn = dpp_i32<ROW_SHL + 1>(key);
    const bool s1 = p >= 1 && k1 == key, s2 = p >= 2 && k2 == key, s4 = p >= 4 && k4 == key, s8 = p >= 8 && k8 == key;
    const bool last = valid && (p == 15 || kn != key);
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            double b = neg ? -D[i][0][v] : D[i][0][v];
            int bi = l0;
#pragma unroll
            for (int j = 1; j < 4; ++j) {
                const double x = neg ? -D[i][j][v] : D[i][j][v];
                if (peak_better(x, b)) {
                    b = x;
                    bi = l0 + j;
                }
            }
            peak_scan_step<1>(s1, b, bi);
            peak_scan_step<2>(s2, b, bi);
            peak_scan_step<4>(s4, b, bi);
            peak_scan_step<8>(s8, b, bi);
            const int64_t t = t0 + 16 * i + g + 4 * v;
            if (last && t < T && b == b) {
                const int64_t s = (t * 2 + par) * S + key;
                pval[s] = neg ? -b : b;
                pidx[s] = bi;
            }
        }
}

// the decode, the list and the walk of k_eval_resident (see there), launched with its geometry (k2r_plan); the list is built by
// a copy of K2r's code, not by a shared function: with the scan in a function of its own the compiler emits another K2r
template <bool PAD, bool LIVE>
__global__ __launch_bounds__(256, 2) void k_eval_resident_peak(int N, int KSp, int64_t Q, int64_t T, int ntt, int groups,
                                                               int64_t npg, const double* __restrict__ Y,
                                                               const double* __restrict__ C, int64_t L, int neg, int64_t S,
                                                               double* __restrict__ pval, int* __restrict__ pidx)
{
    extern __shared__ __align__(16) double shA[];            // [KSp][RT][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = lane & 15, g = lane >> 4;
    const int64_t bid = blockIdx.x;
    const int xcd = (int)(bid & 7);
    const int64_t r = bid >> 3;
    const int tt = (int)(r % ntt);
    const int64_t row = r / ntt;
    const int64_t pg = row * 8 + (LIVE ? (int)((xcd + row) & 7) : xcd);
    if (pg >= npg) return;
    const int64_t t0 = (int64_t)tt * (16 * RT);
    const int KS = (N + 3) >> 2;
    if constexpr (!LIVE) {
        stage_coeffs(shA, tid, N, KSp, T, t0, C);
        __syncthreads();
        for (int grp = 0; grp < groups; ++grp) {
            const int64_t qa = (pg * groups + grp) * 256 + wave * 64 + 4 * p;
            const bool valid = qa < Q;
            if (__ballot(valid) == 0) break;
            v4f64 D[RT][4];
            tile_accumulate<PAD>(shA, lane, g, N, KS, KSp, Q, Y + (valid ? qa : 0), D);
            peak_epilogue(D, p, g, qa, valid, 0, L, neg != 0, S, T, t0, pval, pidx);
        }
    } else {
        __shared__ unsigned short shList[LIVE_PIECES];
        __shared__ int shCnt[4];
        const int wv = __builtin_amdgcn_readfirstlane(wave);
        bool staged = false;
        for (int gb0 = 0; gb0 < groups; gb0 += LIVE_BATCH) {
            const int64_t q0 = (pg * groups + gb0) * 256;
            if (q0 >= Q) break;
            const int ng = groups - gb0 < LIVE_BATCH ? groups - gb0 : LIVE_BATCH;
            const int64_t left = (Q - q0) >> 2;
            const int np = left < (int64_t)ng * 64 ? (int)left : ng * 64;
            int ln = lane;
            asm volatile("" : "+v"(ln));
            unsigned lv = 0;
            int cnt = 0;
#pragma unroll
            for (int it = 0; it < LIVE_PIECES / 256; ++it) {
                const int pc = wv * (LIVE_PIECES / 4) + it * 64 + ln;
                const bool ex = pc < np;
                const v4f64 y = *reinterpret_cast<const v4f64*>(Y + q0 + 4 * (ex ? pc : 0));
                const bool dead = y.x != y.x && y.y != y.y && y.z != y.z && y.w != y.w;
                const bool live = ex && !dead;
                lv |= (unsigned)live << it;
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
            if (nlive == 0) continue;                                               // dead pieces store nothing: their slots stay empty
            if (!staged) {
                int td = tid;
                asm volatile("" : "+v"(td));
                stage_coeffs(shA, td, N, KSp, T, t0, C);
                __syncthreads();
                staged = true;
            }
            const int nchunks = (nlive + 15) >> 4;
            for (int ch = wv; ch < nchunks; ch += 4) {
                const int idx = 16 * ch + p;
                const bool valid = idx < nlive;
                const int64_t qa = q0 + 4 * (int64_t)shList[valid ? idx : 0];
                int gc = g;
                asm volatile("" : "+v"(gc));
                gc &= 3;
                v4f64 D[RT][4];
                tile_accumulate<PAD>(shA, lane, gc, N, KS, KSp, Q, Y + (valid ? qa : 0), D);
                peak_epilogue(D, p, gc, qa, valid, ch & 1, L, neg != 0, S, T, t0, pval, pidx);
            }
        }
    }
}

// val[t][m], idx[t][m] from the slots of column m: the blocks (m L) >> 6 .. ((m + 1) L - 1) >> 6, both parities
__global__ __launch_bounds__(256) void k_peak_finish(int64_t M, int64_t L, int64_t T, int neg, int64_t S,
                                                     const double* __restrict__ pval, const int* __restrict__ pidx,
                                                     double* __restrict__ val, int* __restrict__ idx)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < T * M; e += stride) {
        const int64_t t = e / M, m = e - t * M;
        const int64_t b0 = (m * L) >> 6, b1 = ((m + 1) * L - 1) >> 6;
        double bx = __builtin_nan(""), bv = __builtin_nan("");
        int bi = -1;
        for (int64_t b = b0; b <= b1; ++b)
            for (int par = 0; par < 2; ++par) {
                const int64_t s = (t * 2 + par) * S + m + b;
                const double v = pval[s];
                const double x = neg ? -v : v;
                const int i = pidx[s];
                if (peak_takes(x, i, bx, bi)) {
                    bx = x;
                    bv = v;
                    bi = i;
                }
            }
        val[e] = bv;
        idx[e] = bi;
    }
}

// ---- the two-pass path: columns of a (T, outer, L, inner) slab of densities ---------------------------------------------------
// inner > 1: one thread per column, neighbouring threads neighbouring i - every load of a wave is contiguous
__global__ __launch_bounds__(256) void k_peak_columns(int64_t outer, int64_t L, int64_t inner, int64_t T, int neg,
                                                      const double* __restrict__ in, double* __restrict__ val,
                                                      int* __restrict__ idx)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, M = outer * inner;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < T * M; e += stride) {
        const int64_t tm = e / inner, i = e - tm * inner;          // tm = t * outer + o
        const double* src = in + tm * L * inner + i;
        double bx = __builtin_nan(""), bv = __builtin_nan("");
        int bi = -1;
        for (int64_t l = 0; l < L; ++l) {
            const double v = src[l * inner];
            const double x = neg ? -v : v;
            if (peak_better(x, bx)) {
                bx = x;
                bv = v;
                bi = (int)l;
            }
        }
        val[e] = bv;
        idx[e] = bi;
    }
}

// inner == 1: W lanes (a power of two, at most a wave) per column, lane s at l = s, s + W, ... - contiguous loads -, then a
// butterfly over the W lanes with the total order of peak_takes.  ncol = T * M columns of L contiguous values.
__global__ __launch_bounds__(256) void k_peak_columns_last(int64_t ncol, int64_t L, int W, int neg, const double* __restrict__ in,
                                                           double* __restrict__ val, int* __restrict__ idx)
{
    const int64_t gt = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int sub = (int)(gt & (W - 1));
    const int64_t grp = gt / W, ngrp = (int64_t)gridDim.x * blockDim.x / W;
    for (int64_t c0 = 0; c0 < ncol; c0 += ngrp) {                  // the same trip count in every lane: the shuffles below
        const int64_t c = c0 + grp;
        double bx = __builtin_nan(""), bv = __builtin_nan("");
        int bi = -1;
        if (c < ncol) {
            const double* src = in + c * L;
            for (int64_t l = sub; l < L; l += W) {
                const double v = src[l];
                const double x = neg ? -v : v;
                if (peak_better(x, bx)) {
                    bx = x;
                    bv = v;
                    bi = (int)l;
                }
            }
        }
        for (int off = 1; off < W; off <<= 1) {
            const double ox = __shfl_xor(bx, off), ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (peak_takes(ox, oi, bx, bi)) {
                bx = ox;
                bv = ov;
                bi = oi;
            }
        }
        if (sub == 0 && c < ncol) {
            val[c] = bv;
            idx[c] = bi;
        }
    }
}

// Yr[n][m] = sum_l w[l] Y[n][(o L + l) inner + i] over the l whose point has a number in ROW 0 of Y (K2r's liveness rule:
// vi_eval_basis_f64 makes every row of a point outside the hull NaN), sequentially in ascending l; NaN for a column without
// such a point.  One thread per (n, m), neighbouring threads neighbouring columns.
__global__ __launch_bounds__(256) void k_reduce_basis(int N, int64_t outer, int64_t L, int64_t inner, const double* __restrict__ Y,
                                                      const double* __restrict__ w, double* __restrict__ Yr)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, M = outer * inner, Q = M * L;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < N * M; e += stride) {
        const int64_t n = e / M, m = e - n * M;
        const int64_t o = m / inner, i = m - o * inner;
        const double* y0 = Y + o * L * inner + i;
        const double* yn = y0 + n * Q;
        double acc = 0.0;
        bool any = false;
        for (int64_t l = 0; l < L; ++l) {
            const double r0 = y0[l * inner];
            if (r0 == r0) {
                acc += w[l] * yn[l * inner];
                any = true;
            }
        }
        Yr[e] = any ? acc : __builtin_nan("");
    }
}

unsigned reduce_blocks(int64_t threads)
{
    const int64_t b = (threads + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > (1 << 20) ? (1 << 20) : b));
}

bool use_fused_peak()
{
    static const bool twopass = vi_env_is("VINTERP_K2P", "twopass");
    return !twopass;
}

// The launch of K2r and of K2p for N functions, Q points, T timesteps: K2p's one-writer argument needs K2r's geometry exactly.
// The environment has a say: `groups` (VINTERP_K2R_GROUPS, read at every construction), `live` (VINTERP_K2R_LIVE, once per process).
struct k2r_plan {
    int KSp, ntt, groups;       // k-steps with padding; timestep tiles; points per workgroup: 256 x groups
    size_t shm;                 // the coefficient tile in LDS
    int64_t npg, nblk;          // groups of points; workgroups: the groups rounded up to the 8 XCDs, times the timestep tiles
    bool pad, live;             // the kernel's template arguments
    bool fits;                  // the shape is the kernel's: the 32-byte pieces, two workgroups per CU, a 32-bit grid

    k2r_plan(int N, int64_t Q, int64_t T)
    {
        KSp = (((N + 3) / 4 + PF - 1) / PF) * PF;
        shm = (size_t)KSp * RT * 64 * sizeof(double);
        ntt = (int)((T + 16 * RT - 1) / (16 * RT));
        // the coefficient tile (73 KB through L2) is set up once per workgroup (measured, T = 256: 128^3 points 52 TF with 4
        // groups, 57 with 32; 256^3 the same from 16 up: as many as leave every CU a few workgroups)
        groups = (int)((Q >> 16) < 1 ? 1 : ((Q >> 16) > 32 ? 32 : (Q >> 16)));
        if (const char* e = getenv("VINTERP_K2R_GROUPS")) { const int g = atoi(e); if (g >= 1 && g <= 256) groups = g; }  // experiments
        npg = (Q + (int64_t)256 * groups - 1) / ((int64_t)256 * groups);
        nblk = ((npg + 7) / 8) * 8 * ntt;
        pad = 4 * KSp > N;                                       // N % 16 != 0: rows past the basis
        live = use_live_list();     // VINTERP_K2R_LIVE=0: the plain loop over every point (the list: 4 KB + counters of LDS)
        fits = (Q & 3) == 0 && Q >= 256 && shm <= 150 * 1024 && nblk <= 0x7fffffffLL;
    }
};

}  // namespace

// K2p takes the reduced axis last (inner == 1) with L % 4 == 0 and K2r's own shapes (Q % 4 == 0, Q >= 256, the coefficient
// tile within the LDS); 32-bit keys and indices.  Host arithmetic only: what vi_eval_resident_peak_work_bytes rests on.
bool vi_peak_fused_shape(int N, int64_t outer, int64_t L, int64_t inner)
{
    if (!use_own_kernel() || !use_fused_peak()) return false;
    const int64_t Q = outer * L * inner;
    // (one timestep tile: under the bound on the keys the grid of any one tile is far within 32 bits)
    return inner == 1 && (L & 3) == 0 && outer + (Q + 63) / 64 < 0x7fffffffLL && k2r_plan(N, Q, 1).fits;
}

// slots of the partials per timestep and parity, and the bytes of T timesteps: values, then indices
int64_t vi_peak_fused_slots(int64_t outer, int64_t L) { return outer + (outer * L + 63) / 64; }

size_t vi_peak_fused_work_bytes(int64_t outer, int64_t L, int64_t T)
{
    return (size_t)T * 2 * (size_t)vi_peak_fused_slots(outer, L) * (sizeof(double) + sizeof(int32_t));
}

// val / idx (T, outer) by K2p; *handled = 0 when the call is not the kernel's after all (alignment of d_Y, too many blocks): the
// caller then runs the two-pass path
int vi_eval_resident_peak_mfma(vi_ctx* c, int N, int64_t outer, int64_t L, int64_t T, const double* d_Y, const double* d_C, int kind,
                               double* d_val, int32_t* d_idx, void* d_work, size_t work_bytes, int* handled)
{
    *handled = 0;
    const int64_t Q = outer * L;
    if (!vi_peak_fused_shape(N, outer, L, 1) || ((uintptr_t)d_Y & 31) != 0 || ((uintptr_t)d_work & 7) != 0) return VI_OK;
    const size_t need = vi_peak_fused_work_bytes(outer, L, T);
    if (work_bytes < need) return VI_OK;
    const k2r_plan pl(N, Q, T);
    if (!pl.fits) return VI_OK;
    const int64_t S = vi_peak_fused_slots(outer, L);
    double* pval = (double*)d_work;
    int* pidx = (int*)(pval + (size_t)T * 2 * S);
    VI_HIP(hipMemsetAsync(d_work, 0xFF, need, c->stream));               // every slot empty: (a NaN, -1)
    auto kern = pl.pad ? (pl.live ? k_eval_resident_peak<true, true> : k_eval_resident_peak<true, false>)
                       : (pl.live ? k_eval_resident_peak<false, true> : k_eval_resident_peak<false, false>);
    VI_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.shm));
    hipLaunchKernelGGL(kern, dim3((unsigned)pl.nblk), dim3(256), pl.shm, c->stream, N, pl.KSp, Q, T, pl.ntt, pl.groups, pl.npg,
                       d_Y, d_C, L, kind, S, pval, pidx);
    VI_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_peak_finish, dim3(reduce_blocks(T * outer)), dim3(256), 0, c->stream, outer, L, T, kind, S, pval, pidx,
                       d_val, d_idx);
    VI_HIP(hipGetLastError());
    *handled = 1;
    return VI_OK;
}

// val / idx (T, outer * inner) of a slab of densities (T, outer, L, inner): k_peak_columns / k_peak_columns_last
int vi_peak_columns(vi_ctx* c, int64_t outer, int64_t L, int64_t inner, int64_t T, int kind, const double* d_in, double* d_val,
                    int32_t* d_idx)
{
    if (inner == 1) {
        int W = 1;
        while (W < 64 && W < L) W <<= 1;
        hipLaunchKernelGGL(k_peak_columns_last, dim3(reduce_blocks(T * outer * W)), dim3(256), 0, c->stream, T * outer, L, W, kind,
                           d_in, d_val, d_idx);
    } else {
        hipLaunchKernelGGL(k_peak_columns, dim3(reduce_blocks(T * outer * inner)), dim3(256), 0, c->stream, outer, L, inner, T,
                           kind, d_in, d_val, d_idx);
    }
    VI_HIP(hipGetLastError());
    return VI_OK;
}

int vi_reduce_basis(vi_ctx* c, int N, int64_t outer, int64_t L, int64_t inner, const double* d_Y, const double* d_w, double* d_Yr)
{
    hipLaunchKernelGGL(k_reduce_basis, dim3(reduce_blocks((int64_t)N * outer * inner)), dim3(256), 0, c->stream, N, outer, L, inner,
                       d_Y, d_w, d_Yr);
    VI_HIP(hipGetLastError());
    return VI_OK;
}

// out[t*Q + q] = sum_n Y[n*Q + q] C[t*N + n] by K2r; *handled = 0 when the shape is not the kernel's (the caller then uses the
// library): Q a multiple of 4 and the matrices 32-byte aligned (the 32-byte pieces), the coefficient tile within the LDS.
int vi_eval_resident_mfma(vi_ctx* c, int N, int64_t Q, int64_t T, const double* d_Y, const double* d_C, double* d_out, int* handled)
{
    *handled = 0;
    if (!use_own_kernel()) return VI_OK;
    const k2r_plan pl(N, Q, T);
    if (!pl.fits || (((uintptr_t)d_Y | (uintptr_t)d_out) & 31) != 0) return VI_OK;
    auto kern = pl.pad ? (pl.live ? k_eval_resident<true, true> : k_eval_resident<true, false>)
                       : (pl.live ? k_eval_resident<false, true> : k_eval_resident<false, false>);
    VI_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.shm));
    hipLaunchKernelGGL(kern, dim3((unsigned)pl.nblk), dim3(256), pl.shm, c->stream, N, pl.KSp, Q, T, pl.ntt, pl.groups, pl.npg,
                       d_Y, d_C, d_out);
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

constexpr int ERR_WAVES = 8;                              // waves per workgroup
constexpr int ERR_PTS = ERR_WAVES * 32;                   // points per workgroup and group (= RUN_PTS, the block of K2te's walk)
constexpr int ERR_NBMAX = 9;                              // N <= 144

// The staging K2e, K2te, K2c and K2tc share: S of the covariance D in operand order,
// shS[(blk * 4 + u) * 64 + (g * 16 + p)] = S_IJ[16 I + p][16 J + 4 u + g], by the WAVES waves of the workgroup
template <int NB, int WAVES>
__device__ __forceinline__ void err_stage(int N, const double* __restrict__ D, double* shS, int tid)
{
    constexpr int NBLK = NB * (NB + 1) / 2;
    for (int e = tid; e < NBLK * 256; e += WAVES * 64) {
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
}

// K2e's per-tile body, shared with K2te and K2eg: the forms y^T S y of the wave's 32 points with the staged S - acc0, acc1
// those of the lane's two points (columns of Y, row stride Q), complete in every lane after the two cross-lane adds.
// How the two points are fetched is the one thing that varies: yp[0], yp[1], neighbours, one 16-byte load per basis row (K2e,
// K2te), or with GATHER yp[0], yp[dq], two columns chosen independently, two 8-byte loads `dq` doubles apart, nothing asked of
// the alignment of Y (K2eg).  An MFMA output column depends on its own B column alone: a point's bits do not depend on the tile
// or the lane half that carries it, nor on how it was fetched.
template <int NB, bool GATHER = false>
__device__ __forceinline__ void err_forms(int N, int64_t Q, const double* __restrict__ yp, const double* shS, int lane,
                                          double& acc0, double& acc1, int64_t dq = 0)
{
    const int g = lane >> 4;
    const double* yg = yp + (int64_t)g * Q;             // basis row g; row 16 J + 4 u + g is a uniform offset away
    v4f64 Z[NB][2];
#pragma unroll
    for (int I = 0; I < NB; ++I) Z[I][0] = Z[I][1] = (v4f64){0.0, 0.0, 0.0, 0.0};
    v2f64 y[2][4];                                     // B of block column J (y[J & 1]) and of the next one, in flight
    auto load = [&](v2f64 (&b)[4], int J) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double* src = yg + (int64_t)(16 * J + 4 * u) * Q;
            // the last block column: rows from N on are zero padding - such a lane reads row 0 of its columns and takes zero
            const bool in = J < NB - 1 || 16 * J + 4 * u + g < N;
            if constexpr (GATHER) {
                const double* s = in ? src : yp;
                b[u] = in ? (v2f64){s[0], s[dq]} : (v2f64){0.0, 0.0};
            } else if (J < NB - 1) {
                b[u] = *reinterpret_cast<const v2f64*>(src);
            } else {
                const v2f64 v = *reinterpret_cast<const v2f64*>(in ? src : yp);
                b[u] = in ? v : (v2f64){0.0, 0.0};
            }
        }
    };
    acc0 = acc1 = 0.0;
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
}

template <int NB>
__global__ __launch_bounds__(ERR_WAVES * 64) void k_eval_resident_err(int N, int64_t Q, int64_t T, int groups, int64_t npg,
                                                                      const double* __restrict__ Y, const double* __restrict__ dC,
                                                                      double* __restrict__ out)
{
    extern __shared__ __align__(16) double shS[];         // [block J (J + 1) / 2 + I][k-step u][lane]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4;
    const int64_t bid = blockIdx.x;
    const int xcd = (int)(bid & 7);
    const int64_t r = bid >> 3;
    const int64_t t = r % T;
    const int64_t pg = (r / T) * 8 + xcd;
    if (pg >= npg) return;
    err_stage<NB, ERR_WAVES>(N, dC + t * N * N, shS, tid);
    __syncthreads();
    for (int grp = 0; grp < groups; ++grp) {
        const int64_t qa = (pg * groups + grp) * ERR_PTS + wave * 32 + 2 * (lane & 15);   // this lane's two points
        const bool valid = qa < Q;                                                         // Q even: both or none
        if (__ballot(valid) == 0) break;
        const double* yp = Y + (valid ? qa : 0);
        double acc0, acc1;
        err_forms<NB>(N, Q, yp, shS, lane, acc0, acc1);
        if (valid && g == 0)                                // a negative form gives NaN, as np.sqrt does
            *reinterpret_cast<v2f64*>(out + t * Q + qa) = (v2f64){sqrt(acc0), sqrt(acc1)};
    }
}

// ---- what the launches of K2e, K2eg, K2te, K2c and K2tc share on the host ----

// f(integral_constant NB) at the block count NB = N / 16 rounded up of an order N <= 16 ERR_NBMAX (the callers' shape tests):
// every kernel of the family is compiled at each of the nine
template <class F>
int at_block_count(int N, F&& f)
{
    switch ((N + 15) / 16) {
#define VI_NB(NB) \
    case NB: return f(std::integral_constant<int, NB>{});
        VI_NB(1) VI_NB(2) VI_NB(3) VI_NB(4) VI_NB(5) VI_NB(6) VI_NB(7) VI_NB(8)
#undef VI_NB
    default: return f(std::integral_constant<int, ERR_NBMAX>{});
    }
}

// the bytes of S as err_stage lays it out at block count NB: NB (NB + 1) / 2 blocks of 4 k-steps x 64 lanes
constexpr size_t staged_bytes(int NB) { return (size_t)(NB * (NB + 1) / 2) * 4 * 64 * sizeof(double); }

// blocks of points per workgroup: `cols` columns >> shift, within [1, cap], unless the switch `name` - read at every launch:
// tests, experiments - gives a count in [1, 256]
int groups_switch(int64_t cols, int shift, int cap, const char* name)
{
    int groups = (int)((cols >> shift) < 1 ? 1 : ((cols >> shift) > cap ? cap : (cols >> shift)));
    if (const char* e = getenv(name)) { const int gr = atoi(e); if (gr >= 1 && gr <= 256) groups = gr; }
    return groups;
}

// The timestep-major launch of K2e, K2eg and K2c: *npg groups of pts x groups columns, and *nblk workgroups - the groups rounded
// up to the 8 XCDs, times the T timesteps.  false: more workgroups than a launch takes (the caller leaves the call unhandled).
bool timestep_blocks(int64_t cols, int pts, int groups, int64_t T, int64_t* npg, int64_t* nblk)
{
    *npg = (cols + (int64_t)pts * groups - 1) / ((int64_t)pts * groups);
    *nblk = ((*npg + 7) / 8) * 8 * T;
    return *nblk <= 0x7fffffffLL;
}

// One launch of a kernel of the family with shm bytes of dynamic LDS; *handled = 1 once it is on the stream
template <class K, class... A>
int launch_forms(vi_ctx* c, K kernel, int64_t nblk, int waves, size_t shm, int* handled, A... args)
{
    VI_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(waves * 64), shm, c->stream, args...);
    VI_HIP(hipGetLastError());
    *handled = 1;
    return VI_OK;
}

// points per workgroup of K2e and K2eg on `cols` columns: 256 x groups - S (up to 166 KB of covariance through L2) is staged
// once per workgroup, against 22 us of matrix-core work per group of 256 points at N = 144.
int err_groups(int64_t cols) { return groups_switch(cols, 16, 8, "VINTERP_K2E_GROUPS"); }

// K2eg: K2e's form at ONE chosen point per column and timestep (vi_eval_resident_err_at_f64: the standard error at the peak
// that K2p found).  The grid is (outer, L, inner), column m = o inner + i, and idx[t][m] = l selects point
// q = (o L + l) inner + i:
//
//   out[t][m] = sqrt( sum_i sum_k Y[i][q] * dC[t][i][k] * Y[k][q] ),   NaN where l is outside [0, L)
//
//  * K2e's launch: one timestep per workgroup in the XCD-aware order, S staged once by err_stage and reused for `groups` x 256
//    COLUMNS, a wave 32 of them as two 16-column tiles, lane (p, g) the columns 2p, 2p + 1 of its wave's 32.
//  * The lane's two points are two columns of Y gathered independently (err_forms<NB, true>): L or L inner doubles apart, not
//    neighbours, so two 8-byte loads per basis row from 64-bit offsets - a cache line per value.  Everything after the load is
//    err_forms: the bits at a point are K2e's bits at that point with that covariance.
//  * An index outside [0, L) never becomes an address: the lane half reads column 0, as a lane past the end does, and stores
//    NaN.  Validity is per lane half, any M >= 1; the two results go out as one 16-byte store where that is aligned, else as two
//    8-byte stores.
template <int NB>
__global__ __launch_bounds__(ERR_WAVES * 64) void k_eval_resident_err_at(int N, int64_t Q, int64_t L, int64_t inner, int64_t M,
                                                                         int64_t T, int groups, int64_t npg,
                                                                         const double* __restrict__ Y,
                                                                         const double* __restrict__ dC,
                                                                         const int* __restrict__ idx, double* __restrict__ out)
{
    extern __shared__ __align__(16) double shS[];         // [block J (J + 1) / 2 + I][k-step u][lane]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bid = blockIdx.x;
    const int xcd = (int)(bid & 7);
    const int64_t r = bid >> 3;
    const int64_t t = r % T;
    const int64_t pg = (r / T) * 8 + xcd;
    if (pg >= npg) return;
    err_stage<NB, ERR_WAVES>(N, dC + t * N * N, shS, tid);
    __syncthreads();
    const int* const it = idx + t * M;
    double* const ot = out + t * M;
    for (int grp = 0; grp < groups; ++grp) {
        const int64_t m0 = (pg * groups + grp) * ERR_PTS + wave * 32;                       // the wave's first column
        if (m0 >= M) break;                                                                 // (uniform in the wave)
        // the lane's two points: the flat index of (column, idx[column]), or point 0 for a lane half without one
        int64_t q[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t m = m0 + 2 * (lane & 15) + j;
            const int64_t l = m < M ? it[m] : -1;
            const int64_t o = m / inner;
            q[j] = (l >= 0 && l < L) ? (o * L + l) * inner + (m - o * inner) : 0;
        }
        double acc0, acc1;
        err_forms<NB, true>(N, Q, Y + q[0], shS, lane, acc0, acc1, q[1] - q[0]);
        // what the store needs is made again from an opaque copy of the lane index: nothing but the two forms lives across
        // err_forms (K2e's body leaves two registers free at N = 144)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int64_t m = m0 + 2 * (ln & 15);
        if ((ln >> 4) == 0 && m < M) {
            const int64_t la = it[m], lb = m + 1 < M ? it[m + 1] : -1;
            const double nan = __builtin_nan("");         // a negative form gives NaN, as np.sqrt does
            const double ea = (la >= 0 && la < L) ? sqrt(acc0) : nan, eb = (lb >= 0 && lb < L) ? sqrt(acc1) : nan;
            if (m + 1 < M && ((uintptr_t)(ot + m) & 15) == 0) {
                *reinterpret_cast<v2f64*>(ot + m) = (v2f64){ea, eb};
            } else {
                ot[m] = ea;
                if (m + 1 < M) ot[m + 1] = eb;
            }
        }
    }
}

// The run walk K2te and K2tc share.  A workgroup owns RUN_PTS consecutive columns and walks the RUNS of equal rec inside them:
// the block's rec and a bit mask of its run starts (four ballots) sit in LDS, every wave holds the mask in scalar registers
// and finds the next run with a count of trailing zeros - the walk is uniform, costs no vector register and needs no table
// from the host.
constexpr int RUN_PTS = 256;
static_assert(ERR_PTS == RUN_PTS, "K2te's block is the block of the walk");

// by the threads 0 ... RUN_PTS - 1 (whole waves), a column each: bit c of the mask <=> a run starts at column c of the block
__device__ __forceinline__ void runs_setup(const int* __restrict__ rec, int64_t q0, int nq, int tid, int* shRec, uint64_t* shStart)
{
    const int mine = tid < nq ? rec[q0 + tid] : 0;
    const bool start = tid < nq && (tid == 0 || rec[q0 + tid - 1] != mine);
    const uint64_t mask = __ballot(start);
    shRec[tid] = mine;
    if ((tid & 63) == 0) shStart[tid >> 6] = mask;
}

__device__ __forceinline__ void runs_masks(const uint64_t* shStart, uint64_t (&starts)[RUN_PTS / 64])
{
#pragma unroll
    for (int k = 0; k < RUN_PTS / 64; ++k) {
        const uint64_t v = shStart[k];
        starts[k] = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)v) |
                    (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32;
    }
}

// the next run start after column p, or the end nq of the block
__device__ __forceinline__ int runs_end(const uint64_t (&starts)[RUN_PTS / 64], int p, int nq)
{
    int e = nq;
#pragma unroll
    for (int k = RUN_PTS / 64 - 1; k >= 0; --k) {
        const int from = p + 1 - 64 * k;              // the bits of word k from this one on
        const uint64_t x = from >= 64 ? 0 : from > 0 ? starts[k] & (~(uint64_t)0 << from) : starts[k];
        if (x) e = 64 * k + __builtin_ctzll(x);
    }
    return e;
}

// K2te: K2e with the covariance chosen per COLUMN (vi_eval_records_err_f64: every point of a track, every ray, has its own
// record), F(r, q) = sum_ik Y[i][q] dC[r][i][k] Y[k][q]:
//
//   nearest mode:   out[q] = sqrt(F(rec[q], q))          blend: out[q] = sqrt((1 - w[q]) F(rec[q], q) + w[q] F(rec[q] + 1, q))
//
// K2t's rule: correct for any order of rec, the cost grows with the disorder, callers sort.
//  * A workgroup owns the 256 consecutive columns 256 b ... - 8 waves x 32 points, a lane's two points one 16-byte load, every
//    column at its natural place as in K2e - and walks the RUNS of equal rec inside them (runs_setup, runs_masks, runs_end
//    above).
//  * Per run: S of the run's record is staged as in K2e (err_stage; 90 KB at N = 144: one record fits the LDS, two do not),
//    the waves whose 32 columns meet the run compute their tile with K2e's body (err_forms; the others skip it, a
//    wave-uniform branch), and a lane keeps the result only for those of its two columns that lie in the run.  Sorted input
//    costs one staging per record and block; a tile that two runs share is computed once for each.
//  * Blend mode: two stagings per run, records r and r + 1; the first form waits in LDS (a lane reads back what it wrote
//    itself) - no register lives across the second pass.  (1 - w) F0 + w F1 as written: a NaN in either covariance gives NaN
//    at any w.
//  * A run without a record (rec < 0, or a row it needs >= R) stages nothing and stores NaN; dC is never read outside its R
//    matrices.  A NaN anywhere in a staged S reaches every column of the tile, of which only the run's own are kept.
// A point's bits depend on its column of Y, its record(s) and its weight alone - K2e's order of operations per point (J
// descending, k-steps ascending, the lane-local fma chain, the two cross-lane adds) - and in nearest mode they are K2e's bits
// for that column with that covariance.
template <int NB, bool INTERP>
__global__ __launch_bounds__(ERR_WAVES * 64) void k_eval_records_err(int N, int64_t Q, const double* __restrict__ Y,
                                                                     const int* __restrict__ rec, const double* __restrict__ w,
                                                                     int R, const double* __restrict__ dC,
                                                                     double* __restrict__ out)
{
    constexpr int NBLK = NB * (NB + 1) / 2;
    extern __shared__ __align__(16) double shS[];         // S as in K2e | ERR_PTS first forms | ERR_PTS records | run starts
    double* const shF = shS + NBLK * 256;
    int* const shRec = reinterpret_cast<int*>(shF + ERR_PTS);
    uint64_t* const shStart = reinterpret_cast<uint64_t*>(shRec + ERR_PTS);
    const int tid = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * ERR_PTS;
    const int nq = (int)((Q - q0) < ERR_PTS ? (Q - q0) : ERR_PTS);       // the block's columns
    if (tid < ERR_PTS) runs_setup(rec, q0, nq, tid, shRec, shStart);     // waves 0 ... 3, a column each
    __syncthreads();
    // the walk is scalar: the masks, the run [p, e) and its record r are the same in every lane and held as such
    uint64_t starts[RUN_PTS / 64];
    runs_masks(shStart, starts);
    for (int p = 0, e; p < nq; p = e) {
        const int r = __builtin_amdgcn_readfirstlane(shRec[p]);
        e = runs_end(starts, p, nq);
        if (r < 0 || (int64_t)r + (INTERP ? 1 : 0) >= R) {               // no record: NaN for the run's columns
            if (tid >= p && tid < e) out[q0 + tid] = __builtin_nan("");
            continue;
        }
#pragma unroll 1
        for (int pass = 0; pass <= (INTERP ? 1 : 0); ++pass) {
            // the lane's view of the run, from an opaque copy of its index: what derives from it is made again for every
            // staging, not kept in registers over the tiles (K2e's body leaves two free at N = 144)
            int t = tid;
            asm volatile("" : "+v"(t));
            const int lane = t & 63, wave = t >> 6;
            // its two columns of the block, ca and ca + 1 (Q even: both in the block or none), kept where they lie in the run
            const int ca = wave * 32 + 2 * (lane & 15);
            auto keep = [&](int c) { return (lane >> 4) == 0 && c >= p && c < e; };
            __syncthreads();                              // the tiles of the previous staging are done with S
            err_stage<NB, ERR_WAVES>(N, dC + (int64_t)(r + pass) * N * N, shS, t);
            __syncthreads();
            if (wave * 32 >= e || wave * 32 + 32 <= p) continue;          // the wave's columns do not meet the run
            double f0, f1;
            err_forms<NB>(N, Q, Y + (ca < nq ? q0 + ca : 0), shS, lane, f0, f1);
            if (INTERP && pass == 0) {                    // the first form waits in LDS for the lane that wrote it
                if (keep(ca)) shF[ca] = f0;
                if (keep(ca + 1)) shF[ca + 1] = f1;
            } else if (INTERP) {
                if (keep(ca)) out[q0 + ca] = vi_err_blend_sqrt(w[q0 + ca], shF[ca], f0);
                if (keep(ca + 1)) out[q0 + ca + 1] = vi_err_blend_sqrt(w[q0 + ca + 1], shF[ca + 1], f1);
            } else {                                      // a negative form gives NaN, as np.sqrt does
                if (keep(ca)) out[q0 + ca] = sqrt(f0);
                if (keep(ca + 1)) out[q0 + ca + 1] = sqrt(f1);
            }
        }
    }
}

}  // namespace

// whether K2te takes this call: K2e's shapes - N <= 144, Q even, Y / out 16-byte aligned - unless VINTERP_EVAL_RESIDENT=blas
bool vi_eval_records_err_shape(int N, int64_t Q, const double* d_Y, const double* d_out)
{
    return use_own_kernel() && N >= 1 && N <= 16 * ERR_NBMAX && (Q & 1) == 0 && (((uintptr_t)d_Y | (uintptr_t)d_out) & 15) == 0;
}

// out[q] of vi_eval_records_err_f64 by K2te; *handled = 0 when the shape is not the kernel's (the caller then goes run by run
// through the library)
int vi_eval_records_err_mfma(vi_ctx* c, int N, int64_t Q, const double* d_Y, const int32_t* d_rec, const double* d_w, int64_t R,
                             const double* d_dC, double* d_out, int* handled)
{
    *handled = 0;
    if (!vi_eval_records_err_shape(N, Q, d_Y, d_out)) return VI_OK;
    const int64_t nblk = (Q + ERR_PTS - 1) / ERR_PTS;
    if (nblk > 0x7fffffffLL) return VI_OK;
    return at_block_count(N, [&](auto nb) -> int {
        // S, a first form per column, the block's rec and the mask of its run starts
        const size_t shm = staged_bytes(nb) + ERR_PTS * sizeof(double) + ERR_PTS * sizeof(int) + ERR_PTS / 8;
        return with_flag(d_w != nullptr, [&](auto interp) -> int {
            return launch_forms(c, k_eval_records_err<nb, interp>, nblk, ERR_WAVES, shm, handled, N, Q, d_Y, d_rec, d_w, (int)R,
                                d_dC, d_out);
        });
    });
}

// out[t*Q + q] = sqrt(sum_ik Y[i*Q + q] dC[t*N*N + i*N + k] Y[k*Q + q]) by K2e; *handled = 0 when the shape is not the kernel's
// (the caller then uses the library): N <= 144, Q even and Y / out 16-byte aligned (the 16-byte pieces of two points).
int vi_eval_resident_err_mfma(vi_ctx* c, int N, int64_t Q, int64_t T, const double* d_Y, const double* d_dC, double* d_out,
                              int* handled)
{
    *handled = 0;
    if (!vi_eval_records_err_shape(N, Q, d_Y, d_out)) return VI_OK;
    const int groups = err_groups(Q);
    int64_t npg, nblk;
    if (!timestep_blocks(Q, ERR_PTS, groups, T, &npg, &nblk)) return VI_OK;
    return at_block_count(N, [&](auto nb) -> int {
        return launch_forms(c, k_eval_resident_err<nb>, nblk, ERR_WAVES, staged_bytes(nb), handled, N, Q, T, groups, npg, d_Y,
                            d_dC, d_out);
    });
}

// out[t*M + m] of vi_eval_resident_err_at_f64 by K2eg; *handled = 0 when the order is not the kernel's (N > 144) or with
// VINTERP_EVAL_RESIDENT=blas (the caller then gathers the columns and uses the library).  Any M, any alignment.
int vi_eval_resident_err_at_mfma(vi_ctx* c, int N, int64_t outer, int64_t L, int64_t inner, int64_t T, const double* d_Y,
                                 const double* d_dC, const int32_t* d_idx, double* d_out, int* handled)
{
    *handled = 0;
    if (!use_own_kernel() || N < 1 || N > 16 * ERR_NBMAX) return VI_OK;
    const int64_t M = outer * inner;
    const int groups = err_groups(M);
    int64_t npg, nblk;
    if (!timestep_blocks(M, ERR_PTS, groups, T, &npg, &nblk)) return VI_OK;
    return at_block_count(N, [&](auto nb) -> int {
        return launch_forms(c, k_eval_resident_err_at<nb>, nblk, ERR_WAVES, staged_bytes(nb), handled, N, M * L, L, inner, M, T,
                            groups, npg, d_Y, d_dC, d_idx, d_out);
    });
}

// K2c: gradient-covariance maps of many timesteps on the resident GRADIENT basis of the grid (vi_eval_grad_basis_f64,
// G[(n*3 + c)*Q + q]): the 3 x 3 covariance of the gradient at every point, first-order error propagation of the coefficient
// covariance through the three gradient components g_0, g_1, g_2 (columns of G),
//
//   cov[t][c][d][q] = g_c^T 1/2 (dC[t] + dC[t]^T) g_d,   out[(t*6 + k)*ldo + q], k over (0,0) (1,1) (2,2) (0,1) (0,2) (1,2)
//
// K2e gives the diagonal (its square root) of any resident matrix; the cross terms need the three components of a point side
// by side.  With K2e's S (S_II = dC_II, S_IJ = dC_IJ + dC_JI^T for I < J) and U(c, d) = sum_{I <= J} g_c,I^T S_IJ g_d,J:
// U(c, d) + U(d, c) = g_c^T dC g_d + g_d^T dC g_c, so cov[c][d] = 1/2 (U(c, d) + U(d, c)) and cov[c][c] = U(c, c), K2e's sum.
//  * S of the workgroup's timestep in LDS in operand order exactly as in K2e (90 KB at N = 144), staged once per workgroup and
//    reused for `groups` x 64 points; one workgroup of 4 waves per CU, ONE wave per SIMD: the 3 NB accumulator quads (216
//    registers at N = 144) and the B registers of two block columns need the whole unified file of a SIMD lane (VGPR + AGPR).
//  * A wave takes 16 points as three 16-column tiles, tile c = component c of the same 16 points: lane (p = lane & 15,
//    g = lane >> 4) reads G[16 J + 4 u + g][c][q0 + p], one 8-byte load per component (a row of 16 lanes: 128 contiguous
//    bytes).  No condition on Q or on the alignment of G.  The rows from N on of the last block column are zero and not loaded.
//  * Z_I[d] = sum_{J >= I} S_IJ g_d,J with J descending; Z_I[d] is complete right after block column I, whose B registers
//    hold rows 16 I + 4 u + g of all three components - the rows of Z_I's accumulator in this lane - so the nine dots
//    M[c][d] += g_c,I^T Z_I[d] are lane-local.  Two cross-lane adds, the symmetrising half-sum, six 8-byte stores per point
//    (the 16 lanes with g = 0: 128 contiguous bytes of each plane).
//  * Per k-step the MFMAs run over I and the three tiles: no accumulator is touched again before 3 J + 2 others.
// Bound: the fp64 matrix peak, 3 N_p (N_p + 16) flop issued per point-timestep (three times K2e's: the least for three
// vectors) against 8 (3 N / T_concurrent + 6) bytes.
namespace {

constexpr int COV_WAVES = 4;                              // waves per workgroup: one per SIMD
constexpr int COV_PTS = COV_WAVES * 16;                   // points per workgroup and group

// K2c's per-tile body, shared with K2tc: the nine forms M[c][d] = sum_{I <= J} g_c,I^T S_IJ g_d,J of the wave's 16 points with
// the staged S - gq: row 0, component 0 of the lane's point (G[(n*3 + c)*Q + q]) -, complete in every lane after the two
// cross-lane adds
template <int NB>
__device__ __forceinline__ void cov_forms(int N, int64_t Q, const double* __restrict__ gq, const double* shS, int lane,
                                          double (&M)[3][3])
{
    const int g = lane >> 4;
    const double* gp = gq + (int64_t)g * 3 * Q;        // row g, component 0; row 16 J + 4 u + g is a uniform offset away
    v4f64 Z[NB][3];
#pragma unroll
    for (int I = 0; I < NB; ++I) Z[I][0] = Z[I][1] = Z[I][2] = (v4f64){0.0, 0.0, 0.0, 0.0};
    double y[2][3][4];                                 // B of block column J (y[J & 1][c][u]) and of the next one, in flight
    auto load = [&](double (&b)[3][4], int J) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double* src = gp + (int64_t)(16 * J + 4 * u) * 3 * Q;
            // the last block column: rows from N on are zero padding, never loaded (a loaded infinity times a zero of S
            // would be NaN)
            const bool in = J < NB - 1 || 16 * J + 4 * u + g < N;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double v = 0.0;
                if (in) v = src[c * Q];
                b[c][u] = v;
            }
        }
    };
#pragma unroll
    for (int c = 0; c < 3; ++c) M[c][0] = M[c][1] = M[c][2] = 0.0;
    load(y[(NB - 1) & 1], NB - 1);
#pragma unroll
    for (int J = NB - 1; J >= 0; --J) {
        if (J > 0) load(y[(J - 1) & 1], J - 1);
        __builtin_amdgcn_sched_barrier(0);            // the next block column's loads in flight before this one's products
        const double(&b)[3][4] = y[J & 1];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int I = 0; I <= J; ++I) {
                const double a = shS[((J * (J + 1) / 2 + I) * 4 + u) * 64 + lane];
                Z[I][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[0][u], Z[I][0], 0, 0, 0);
                Z[I][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[1][u], Z[I][1], 0, 0, 0);
                Z[I][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[2][u], Z[I][2], 0, 0, 0);
            }
            // the LDS reads of one k-step at a time; reading them a k-step ahead measured 0.7 % faster: not worth its code
            __builtin_amdgcn_sched_barrier(0);
        }
        // Z_J[d] is complete; its row g + 4 v is basis row 16 J + 4 v + g, the one b[c][v] holds
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int d = 0; d < 3; ++d) M[c][d] = fma(b[c][v], Z[J][d][v], M[c][d]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            M[c][d] += __shfl_xor(M[c][d], 16);
            M[c][d] += __shfl_xor(M[c][d], 32);
        }
}

// the six entries of the symmetric part 1/2 (M + M^T), in the order of GRADCOV_PAIRS: (0,0) (1,1) (2,2) (0,1) (0,2) (1,2)
__device__ __forceinline__ void cov_pack(const double (&M)[3][3], double (&U)[6])
{
    U[0] = M[0][0];
    U[1] = M[1][1];
    U[2] = M[2][2];
    U[3] = 0.5 * (M[0][1] + M[1][0]);
    U[4] = 0.5 * (M[0][2] + M[2][0]);
    U[5] = 0.5 * (M[1][2] + M[2][1]);
}

template <int NB>
__global__ __launch_bounds__(COV_WAVES * 64) void k_eval_resident_gradcov(int N, int64_t Q, int64_t T, int groups, int64_t npg,
                                                                          int64_t ldo, const double* __restrict__ G,
                                                                          const double* __restrict__ dC, double* __restrict__ out)
{
    extern __shared__ __align__(16) double shS[];         // [block J (J + 1) / 2 + I][k-step u][lane]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4;
    const int64_t bid = blockIdx.x;
    const int xcd = (int)(bid & 7);
    const int64_t r = bid >> 3;
    const int64_t t = r % T;
    const int64_t pg = (r / T) * 8 + xcd;
    if (pg >= npg) return;
    err_stage<NB, COV_WAVES>(N, dC + t * N * N, shS, tid);   // S of timestep t in operand order, as K2e
    __syncthreads();
    double* const ot = out + t * 6 * ldo;
    for (int grp = 0; grp < groups; ++grp) {
        const int64_t q = (pg * groups + grp) * COV_PTS + wave * 16 + (lane & 15);         // this lane's point
        const bool valid = q < Q;
        if (__ballot(valid) == 0) break;
        double M[3][3];
        cov_forms<NB>(N, Q, G + (valid ? q : 0), shS, lane, M);
        if (valid && g == 0) {                              // a negative diagonal entry (indefinite dC) is stored as it is
            double U[6];
            cov_pack(M, U);
#pragma unroll
            for (int k = 0; k < 6; ++k) ot[k * ldo + q] = U[k];
        }
    }
}

// points per workgroup of K2c: 64 x groups, by the size of Q as in K2e and up to K2e's 2048 - S (up to 166 KB of covariance
// through L2, by 4 waves) is staged once per workgroup, against 17 us of matrix-core work per group of 64 points at N = 144,
// and no second workgroup fits the CU to hide it: 42.1 ms at 8 groups, 36.8 at 32, 35.9 at 64 (128^3 x 16 timesteps)
int gradcov_groups(int64_t Q) { return groups_switch(Q, 14, 32, "VINTERP_K2C_GROUPS"); }

// K2tc: K2c with the covariance chosen per COLUMN (vi_eval_records_gradcov_f64: every point of a track has its own record), as
// K2te is to K2e.  With U_r(q)[k] the six packed entries of g_c^T 1/2 (dC_r + dC_r^T) g_d at point q:
//
//   nearest mode:   out[k*ldo + q] = U_rec[q](q)[k]      blend: out[k*ldo + q] = (1 - w[q]) U_rec[q](q)[k] + w[q] U_(rec[q]+1)(q)[k]
//
// K2t's rule: correct for any order of rec, the cost grows with the number of runs, callers sort.
//  * A workgroup of COV_WAVES waves takes `groups` blocks of RUN_PTS = 256 consecutive points, one after the other; a block is
//    16 tiles of 16 points, tile t goes to wave t & 3 - a run of 64 columns occupies all four SIMDs - and the runs of equal rec
//    inside the block are walked as in K2te (runs_setup, runs_masks, runs_end).
//  * Per run: S of the run's record is staged as in K2c (err_stage), every tile that meets the run is computed by its wave with
//    K2c's body (cov_forms, cov_pack), and a lane keeps the result only if its point lies in the run.  A tile that two runs
//    share is computed once for each.  The record whose S sits in LDS is remembered: a run that goes on across a block border
//    of the same workgroup is not staged again.
//  * Blend mode: two stagings per run, records r and r + 1; the six values of the first wait in LDS (6 x 256 doubles; a lane
//    reads back what it wrote itself) - no register lives across the second staging.  The pass whose record is already staged
//    goes first, so sorted input alternates r, r + 1 | r + 1, r | ... across block borders: the blend takes its two values
//    by record, not by pass, (1 - w) U_r + w U_(r+1) as written - a NaN in either covariance gives NaN at any w.
//  * A run without a record (rec < 0, or a row it needs >= R) stages nothing and stores six NaN; dC is never read outside its R
//    matrices.  A NaN anywhere in a staged S reaches every column of the tile, of which only the run's own are kept.
// A point's bits depend on its three columns of G, its record(s) and its weight alone, and in nearest mode they are K2c's bits
// for that point with that covariance.  No condition on Q or on the alignment of G.
template <int NB, bool INTERP>
__global__ __launch_bounds__(COV_WAVES * 64) void k_eval_records_gradcov(int N, int64_t Q, int groups, int64_t ldo,
                                                                         const double* __restrict__ G, const int* __restrict__ rec,
                                                                         const double* __restrict__ w, int R,
                                                                         const double* __restrict__ dC, double* __restrict__ out)
{
    static_assert(COV_WAVES * 64 == RUN_PTS, "a thread per column of the block");
    constexpr int NBLK = NB * (NB + 1) / 2;
    extern __shared__ __align__(16) double shS[];         // S as in K2c | 6 x RUN_PTS first values | RUN_PTS records | run starts
    double* const shF = shS + NBLK * 256;
    int* const shRec = reinterpret_cast<int*>(shF + 6 * RUN_PTS);
    uint64_t* const shStart = reinterpret_cast<uint64_t*>(shRec + RUN_PTS);
    const int tid = threadIdx.x;
    int staged = -1;                                      // the record whose S sits in LDS (uniform)
    for (int grp = 0; grp < groups; ++grp) {
        const int64_t q0 = ((int64_t)blockIdx.x * groups + grp) * RUN_PTS;
        if (q0 >= Q) break;
        const int nq = (int)((Q - q0) < RUN_PTS ? (Q - q0) : RUN_PTS);   // the block's columns
        if (grp > 0) __syncthreads();                     // the walk of the previous block is done with its records
        runs_setup(rec, q0, nq, tid, shRec, shStart);
        __syncthreads();
        uint64_t starts[RUN_PTS / 64];
        runs_masks(shStart, starts);
        for (int p = 0, e; p < nq; p = e) {
            const int r = __builtin_amdgcn_readfirstlane(shRec[p]);
            e = runs_end(starts, p, nq);
            if (r < 0 || (int64_t)r + (INTERP ? 1 : 0) >= R) {           // no record: NaN for the run's columns
                if (tid >= p && tid < e) {
#pragma unroll
                    for (int k = 0; k < 6; ++k) out[k * ldo + q0 + tid] = __builtin_nan("");
                }
                continue;
            }
            const int first = INTERP && staged == r + 1 ? 1 : 0;         // the pass that finds its S staged goes first
#pragma unroll 1
            for (int it = 0; it <= (INTERP ? 1 : 0); ++it) {
                const int pass = it ^ first;                              // S of record r + pass
                // the lane's view of the run, from an opaque copy of its index: what derives from it is made again for every
                // staging, not kept in registers over the tiles
                int t = tid;
                asm volatile("" : "+v"(t));
                const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
                if (staged != r + pass) {
                    __syncthreads();                      // the tiles of the previous staging are done with S
                    err_stage<NB, COV_WAVES>(N, dC + (int64_t)(r + pass) * N * N, shS, t);
                    __syncthreads();
                    staged = r + pass;
                }
#pragma unroll 1
                for (int tile = (p >> 4) + ((wave - (p >> 4)) & 3); 16 * tile < e; tile += COV_WAVES) {   // this wave's tiles of the run
                    const int c = 16 * tile + (lane & 15);                // this lane's column of the block
                    double M[3][3];
                    cov_forms<NB>(N, Q, G + (c < nq ? q0 + c : 0), shS, lane, M);
                    const bool keep = (lane >> 4) == 0 && c >= p && c < e;   // the point lies in the run (e <= nq)
                    if (!keep) continue;                  // (after the cross-lane adds of cov_forms; the tile loop is uniform)
                    double U[6];
                    cov_pack(M, U);
                    if (INTERP && it == 0) {              // the first values wait in LDS for the lane that wrote them
#pragma unroll
                        for (int k = 0; k < 6; ++k) shF[k * RUN_PTS + c] = U[k];
                    } else if (INTERP) {
                        const double wq = w[q0 + c];
#pragma unroll
                        for (int k = 0; k < 6; ++k) {
                            const double a = shF[k * RUN_PTS + c], b = U[k];
                            out[k * ldo + q0 + c] = pass == 1 ? vi_err_blend(wq, a, b) : vi_err_blend(wq, b, a);
                        }
                    } else {                              // a negative diagonal entry is stored as it is (K2c's rule)
#pragma unroll
                        for (int k = 0; k < 6; ++k) out[k * ldo + q0 + c] = U[k];
                    }
                }
            }
        }
    }
}

// blocks of 256 points per workgroup of K2tc: S stays staged across the block borders of a workgroup where the record does not
// change.
int records_gradcov_groups(int64_t Q) { return groups_switch(Q, 16, 8, "VINTERP_K2TC_GROUPS"); }

}  // namespace

// out[k*ldo + q] of vi_eval_records_gradcov_f64 by K2tc; *handled = 0 when the shape is not the kernel's - N > 144,
// VINTERP_EVAL_RESIDENT=blas - (the caller then goes run by run through the library)
int vi_eval_records_gradcov_mfma(vi_ctx* c, int N, int64_t Q, const double* d_G, const int32_t* d_rec, const double* d_w, int64_t R,
                                 const double* d_dC, double* d_out, int64_t ldo, int* handled)
{
    *handled = 0;
    if (!vi_eval_resident_gradcov_shape(N)) return VI_OK;
    const int groups = records_gradcov_groups(Q);
    const int64_t nblk = (Q + (int64_t)RUN_PTS * groups - 1) / ((int64_t)RUN_PTS * groups);
    if (nblk > 0x7fffffffLL) return VI_OK;
    return at_block_count(N, [&](auto nb) -> int {
        // S, six first entries per column, the block's rec and the mask of its run starts
        const size_t shm = staged_bytes(nb) + 6 * RUN_PTS * sizeof(double) + RUN_PTS * sizeof(int) + RUN_PTS / 8;
        return with_flag(d_w != nullptr, [&](auto interp) -> int {
            return launch_forms(c, k_eval_records_gradcov<nb, interp>, nblk, COV_WAVES, shm, handled, N, Q, groups, ldo, d_G, d_rec,
                                d_w, (int)R, d_dC, d_out);
        });
    });
}

// whether K2c takes gradient bases of N rows at all (what a caller that carves a workspace for the library path asks first)
bool vi_eval_resident_gradcov_shape(int N) { return use_own_kernel() && N >= 1 && N <= 16 * ERR_NBMAX; }

// out[(t*6 + k)*ldo + q] = g_c^T 1/2 (dC_t + dC_t^T) g_d of the gradient basis d_G[(n*3 + c)*Q + q] by K2c, (c, d) the k-th of
// (0,0) (1,1) (2,2) (0,1) (0,2) (1,2); *handled = 0 when the shape is not the kernel's (the caller then uses the library): N <= 144.
int vi_eval_resident_gradcov_mfma(vi_ctx* c, int N, int64_t Q, int64_t T, const double* d_G, const double* d_dC, double* d_out,
                                  int64_t ldo, int* handled)
{
    *handled = 0;
    if (!vi_eval_resident_gradcov_shape(N)) return VI_OK;
    const int groups = gradcov_groups(Q);
    int64_t npg, nblk;
    if (!timestep_blocks(Q, COV_PTS, groups, T, &npg, &nblk)) return VI_OK;
    return at_block_count(N, [&](auto nb) -> int {
        return launch_forms(c, k_eval_resident_gradcov<nb>, nblk, COV_WAVES, staged_bytes(nb), handled, N, Q, T, groups, npg, ldo,
                            d_G, d_dC, d_out);
    });
}
