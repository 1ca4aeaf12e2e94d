// K_walk: the rotated systems of the bracket walk in shared bases (vi_basis_solve_f64, vi_fit.hip), formed in one kernel
// on the fp64 matrix cores.  For system i = (record, basis, alpha), with A = AWA[record], V = V[basis] stored "row k =
// basis vector k", D2 = D2[basis]:
//   X[i]  = f (V A V^T + alpha D2),  f the power of two that brings max|X| into [1, 2), scl[i] = 1 / f
//   yt[i] = V y[record]
// the formulas of the rocBLAS chain it replaces (two batched products, k_vt_vec, k_form_pair_scaled), whose three
// intermediate N x N matrices per system never reach HBM here.
//
// One workgroup per system, one wave per 16-column block (NT = ceil(N / 16) waves; N = 144: 9).  Wave w keeps its two B
// operands in registers for the whole system, one fp64 per lane and k-step (lane: n = lane & 15, g = lane >> 4):
//   bA[u] = A[4u + g][16w + n]     the column block w of A
//   bV[u] = V[16w + n][4u + g]     the row block w of V, transposed by the operand layout
// and the system is worked a row panel I of 16 rows at a time, with two v_mfma_f64_16x16x4 chains of 4 NT k-steps each:
//   W_I   = V[panel I] A           wave w: the 16 x 16 tile of columns 16w.. .  The A operand V[16I + m][4u + g] is exactly
//                                  bV of wave I, which puts it into LDS in operand order ([k-step][lane], linear reads)
//   X[I, w] = W_I V[block w]^T     waves w <= I.  W_I goes through LDS from the accumulator layout (col = lane & 15,
//                                  row = (lane >> 4) + 4 reg) into operand order; 2 x 18 KB of LDS at N = 144
// K3 reads X[i][j] for j <= i only, so the tiles above the block diagonal (36 of 81 at N = 144) are neither computed nor
// written - X above them keeps whatever the workspace held.  The maximum is taken over every element that IS computed: the
// lower block triangle, whole diagonal tiles included.  A wave writes its tiles unscaled, the workgroup reduces the
// maximum, and a second, L2-hot pass scales what was written.
//
// Every element of X is one accumulator chain per product over k ascending in steps of 4, and nothing in the kernel depends
// on the batch, on the system's place in it or on the chunk: a walk system's bits are a function of (record, basis, alpha).
// yt has the summation order of k_vt_vec (vi_fit.hip), which does not depend on the number of waves either.
//
// Registers: 16 NT for the two operands and about 48 beside them, of the 512 / (waves per SIMD) a wave may have.  Up to
// N = 128 that fits.  At N = 144 (9 waves, 3 on one SIMD, 168 registers each) the last KL = 16 k-steps of bV live in LDS
// instead ([wave][k-step][lane], 74 KB; each lane reads back what it wrote): 168 registers, no scratch.  Orders that are
// not a multiple of 16 (PAD) load zeros past N, and the masks cost registers: N = 129..143 and every N > 144 (RES = false)
// fetch the B operands from L2 at every use instead of holding them - correct, and nobody's default order.
#include "vi_common.h"
#include "vi_solver.h"

namespace {

using v4f64 = __attribute__((__vector_size__(4 * sizeof(double)))) double;

template <int NT, bool RES, int KL, bool PAD>
__global__ __launch_bounds__(NT * 64) void k_walk_rotate(int N, const double* __restrict__ AWA, const int* __restrict__ rec,
                                                         const double* __restrict__ V, const double* __restrict__ D2,
                                                         const int* __restrict__ basis, const double* __restrict__ y,
                                                         const double* __restrict__ alpha, double* __restrict__ X,
                                                         double* __restrict__ scl, double* __restrict__ yt)
{
    constexpr int KS = 4 * NT;                    // k-steps of 4 over the padded order 16 NT
    constexpr int UNR = RES ? NT : 1;             // operands in registers: the k loops unrolled (register indices)
    __shared__ double shV[KS * 64];               // V[panel I] as the A operand: [k-step][lane]
    __shared__ double shW[KS * 64];               // W_I as the A operand
    __shared__ double shB[KL > 0 ? NT * KL * 64 : 1];   // the last KL k-steps of every wave's bV, [wave][k-step][lane]
    __shared__ double red[NT];
    const int64_t i = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = lane & 15, g = lane >> 4;
    const int64_t NN = (int64_t)N * N;
    const double* Ai = AWA + (int64_t)rec[i] * NN;
    const double* Vi = V + (int64_t)basis[i] * NN;
    const double* D2i = D2 + (int64_t)basis[i] * NN;
    const double* yi = y + (int64_t)rec[i] * N;
    double* Xi = X + i * NN;
    const double a = alpha[i];
    const int c = 16 * w + n;                     // this lane's column of A and of X, and its row of V
    const bool cok = c < N;

    // PAD (N < 16 NT): past N the operands are zero.  Every load goes to a clamped (valid) address and is multiplied by 0
    // or 1 - exact, the matrices being finite - so that no load sits behind a branch and a wave's loads are in flight together.
    const int cc = (!PAD || cok) ? c : N - 1;
    auto loadA = [&](int u) {
        const int k = 4 * u + g;
        if (!PAD) return Ai[(int64_t)k * N + c];
        return Ai[(int64_t)(k < N ? k : N - 1) * N + cc] * ((cok && k < N) ? 1.0 : 0.0);
    };
    auto loadV = [&](int blk, int u) {
        const int r = 16 * blk + n, k = 4 * u + g;
        if (!PAD) return Vi[(int64_t)r * N + k];
        return Vi[(int64_t)(r < N ? r : N - 1) * N + (k < N ? k : N - 1)] * ((r < N && k < N) ? 1.0 : 0.0);
    };
    // ---- yt = V y   (k_vt_vec: one fma chain per lane over r = lane, lane + 64, ..., then the shuffle tree)
    for (int k = w; k < N; k += NT) {
        double acc = 0.0;
        for (int r = lane; r < N; r += 64) acc = fma(Vi[(int64_t)k * N + r], yi[r], acc);
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
        if (lane == 0) yt[i * N + k] = acc;
    }

    constexpr int KR = KS - KL;                   // k-steps of bV in registers
    double bA[RES ? KS : 1], bV[RES ? KR : 1];
    if (RES) {
#pragma unroll
        for (int u = 0; u < KS; ++u) bA[u] = loadA(u);
#pragma unroll
        for (int u = 0; u < KR; ++u) bV[u] = loadV(w, u);
#pragma unroll
        for (int u = KR; u < KS; ++u) shB[(w * KL + u - KR) * 64 + lane] = loadV(w, u);   // read back by this lane only
    }
    auto getV = [&](int u) { return !RES ? loadV(w, u) : u < KR ? bV[u] : shB[(w * KL + u - KR) * 64 + lane]; };

    double mx = 0.0;
    for (int I = 0; I < NT; ++I) {
        if (RES) {
            if (w == I) {
#pragma unroll
                for (int u = 0; u < KS; ++u) shV[u * 64 + lane] = getV(u);
            }
        } else {
            for (int u = w; u < KS; u += NT) shV[u * 64 + lane] = loadV(I, u);
        }
        __syncthreads();          // shV(I) written; every wave is past its reads of shW(I - 1)
        v4f64 t = {0.0, 0.0, 0.0, 0.0};
        // scheduling barriers: the LDS reads of four k-steps in flight, not all of them (at N = 144 the resident operands
        // leave 24 of the 168 registers of a wave)
#pragma unroll UNR
        for (int u0 = 0; u0 < KS; u0 += 4) {
            double av[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) av[u] = shV[(u0 + u) * 64 + lane];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                t = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], RES ? bA[u0 + u] : loadA(u0 + u), t, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // W_I[m = g + 4 r][c = 16 w + n] -> operand order: k-step c / 4, lane m + 16 (c % 4)
#pragma unroll
        for (int r = 0; r < 4; ++r) shW[(4 * w + (n >> 2)) * 64 + (g + 4 * r) + 16 * (n & 3)] = t[r];
        __syncthreads();          // shW(I) written; every wave is past its reads of shV(I)
        if (w <= I) {
            // this lane's four elements of D2, asked for ahead of the chain that hides their latency
            double d2v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * I + g + 4 * r;
                d2v[r] = (!PAD || (cok && row < N)) ? D2i[(int64_t)row * N + c] : 0.0;
            }
            v4f64 d = {0.0, 0.0, 0.0, 0.0};
#pragma unroll UNR
            for (int u0 = 0; u0 < KS; u0 += 4) {
                double av[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) av[u] = shW[(u0 + u) * 64 + lane];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    d = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], getV(u0 + u), d, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * I + g + 4 * r;
                if (!PAD || (cok && row < N)) {
                    const double v = fma(a, d2v[r], d[r]);
                    mx = fmax(mx, fabs(v));
                    Xi[(int64_t)row * N + c] = v;
                }
            }
        }
    }

    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if (lane == 0) red[w] = mx;
    __syncthreads();
    mx = 0.0;
#pragma unroll
    for (int q = 0; q < NT; ++q) mx = fmax(mx, red[q]);
    int ex = 0;
    double f = 1.0;
    if (mx > 0.0 && mx < 1.7e308) {
        (void)frexp(mx, &ex);            // mx = m * 2^ex, m in [0.5, 1)
        f = ldexp(1.0, ex > -1022 ? 1 - ex : 1023);     // mx * f in [1, 2); below 2^-1023 the largest power of two, not Inf
    }
    // The second pass, L2-hot, after the barrier above (every wave's stores of X are visible to the workgroup): a wave per
    // row, eight rows' loads in flight together.  Loads are unconditional, to clamped addresses inside the row's written
    // part; only the stores are predicated.
    // A system with an infinite element comes out as NaN all over (k_scale_system, vi_fit.hip): without this an Inf in A gave
    // +-Inf in the exact variants and NaN in a padded one whose clamped loads met it.  scl stays 1.
    const double fx = isinf(mx) ? NAN : f;
    constexpr int RB = 8, CG = (16 * NT + 63) / 64;
    for (int r0 = w; r0 < N; r0 += RB * NT) {
        double xv[RB][CG];
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            const int row = r0 + q * NT < N ? r0 + q * NT : N - 1;
            const int lim = 16 * (row / 16 + 1) < N ? 16 * (row / 16 + 1) : N;
#pragma unroll
            for (int m = 0; m < CG; ++m) {
                const int col = lane + 64 * m;
                xv[q][m] = Xi[(int64_t)row * N + (col < lim ? col : lim - 1)];
            }
        }
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            const int row = r0 + q * NT;
            const int lim = 16 * (row / 16 + 1) < N ? 16 * (row / 16 + 1) : N;
#pragma unroll
            for (int m = 0; m < CG; ++m) {
                const int col = lane + 64 * m;
                if (row < N && col < lim) Xi[(int64_t)row * N + col] = xv[q][m] * fx;
            }
        }
    }
    if (tid == 0) scl[i] = 1.0 / f;      // exact (power of two)
}

// RESP: RES of the padded variant (N < 16 NT), which never keeps operands in LDS
template <int NT, bool RES, int KL, bool RESP>
void launch_walk_rotate(vi_ctx* c, int64_t B, int N, const double* AWA, const int* rec, const double* V, const double* D2,
                        const int* basis, const double* y, const double* alpha, double* X, double* scl, double* yt)
{
    if (N == 16 * NT)
        hipLaunchKernelGGL((k_walk_rotate<NT, RES, KL, false>), dim3((unsigned)B), dim3(NT * 64), 0, c->stream, N, AWA, rec, V, D2,
                           basis, y, alpha, X, scl, yt);
    else
        hipLaunchKernelGGL((k_walk_rotate<NT, RESP, 0, true>), dim3((unsigned)B), dim3(NT * 64), 0, c->stream, N, AWA, rec, V, D2,
                           basis, y, alpha, X, scl, yt);
}

}  // namespace

// X, scl and yt of B walk systems (see the head of this file).  X: B x N x N, of which the lower block triangle is written.
int vi_walk_rotate(vi_ctx* c, int64_t B, int N, const double* d_AWA, const int* d_rec, const double* d_V, const double* d_D2,
                   const int* d_basis, const double* d_y, const double* d_alpha, double* d_X, double* d_scl, double* d_yt)
{
#define VI_W(NT, RES, KL, RESP)                                                                                                \
    case NT:                                                                                                          \
        launch_walk_rotate<NT, RES, KL, RESP>(c, B, N, d_AWA, d_rec, d_V, d_D2, d_basis, d_y, d_alpha, d_X, d_scl, d_yt);       \
        break
    switch ((N + 15) / 16) {
        VI_W(1, true, 0, true);
        VI_W(2, true, 0, true);
        VI_W(3, true, 0, true);
        VI_W(4, true, 0, true);
        VI_W(5, true, 0, true);
        VI_W(6, true, 0, true);
        VI_W(7, true, 0, true);
        VI_W(8, true, 0, true);
        VI_W(9, true, 16, false);
        VI_W(10, false, 0, false);
        VI_W(11, false, 0, false);
        VI_W(12, false, 0, false);
        VI_W(13, false, 0, false);
    default:                             // beyond the orders of K3 (vi_jacobi_supported), which the caller has checked
        vi_set_error("vi_walk_rotate: N=%d outside 1..208", N);
        return VI_ERR_UNSUPPORTED;
    }
#undef VI_W
    VI_HIP(hipGetLastError());
    return VI_OK;
}
