// Entries that work on a matrix ALREADY BUILT on the device - the resident basis Y (N x Q) of vi_eval_basis_f64, the gradient
// basis G (N x 3 x Q) of vi_eval_grad_basis_f64, the ray-integrated basis of vi_eval_slant_basis_f64 - and evaluate no basis
// function themselves (those are vi_basis.hip's, vi_track.hip's and vi_slant.hip's):
//   products        out = Y C of many timesteps (K2r), peak maps of it (K2p), the reduced basis along an axis;
//   forms           y^T dC y (standard errors: K2e, K2eg, K2te) and g_c^T dC g_d (gradient covariances: K2c, K2tc).
// Each entry asks its own kernel first (vi_eval_resident.hip).  What that declines - N > 144, odd Q, unaligned pointers,
// VINTERP_EVAL_RESIDENT=blas - goes through the library: one route for every form, below.
#include "vi_common.h"
#include "vi_solver.h"

#include <algorithm>

namespace {

// the product of vi_eval_resident_f64 without its timer (vi_eval_resident_peak_f64 runs it per slab inside its own)
int eval_resident(vi_model* m, int64_t Q, int64_t T, const double* d_Y, const double* d_C, double* d_out)
{
    vi_ctx* c = m->ctx;
    const int N = m->N;
    int handled = 0;
    const int rc = vi_eval_resident_mfma(c, N, Q, T, d_Y, d_C, d_out, &handled);      // K2r (vi_eval_resident.hip)
    if (rc != VI_OK || handled) return rc;
    // shapes outside K2r's (Q not a multiple of 4, orders whose coefficient tile exceeds the LDS): the library's product
    const double one = 1.0, zero = 0.0;
    const int64_t TT = 128;                          // timesteps per product
    const int64_t QQ = (int64_t)1 << 30;             // points per product (the library's dimensions are 32-bit)
    for (int64_t t0 = 0; t0 < T; t0 += TT) {
        const int64_t tc = (T - t0) < TT ? (T - t0) : TT;
        for (int64_t q0 = 0; q0 < Q; q0 += QQ) {
            const int64_t qc = (Q - q0) < QQ ? (Q - q0) : QQ;
            // column-major: out(qc x tc, ld Q) = Y(qc x N, ld Q) * C(N x tc, ld N)
            VI_ROCBLAS(rocblas_dgemm(c->blas, rocblas_operation_none, rocblas_operation_none, (rocblas_int)qc, (rocblas_int)tc, N,
                                     &one, d_Y + q0, (rocblas_int)Q, d_C + t0 * N, N, &zero, d_out + t0 * Q + q0, (rocblas_int)Q));
        }
    }
    return VI_OK;
}

}  // namespace

// ---- evaluation of many timesteps on one grid from a RESIDENT basis (BASELINE configs[3]: a GPU's share of 10 000 timesteps on
// one 256^3 grid).  vi_eval_f64 recomputes the basis of a point for every tile of 32 timesteps - right for one timestep or a
// few, and it keeps the matrix cores waiting for the recurrences half of the time.  With hundreds of
// timesteps on the same grid the basis matrix is worth keeping: N x Q doubles - 19 GB at the default order on 256^3, a
// fifteenth of this GPU's HBM - assembled once by K1 (vi_eval_basis_f64 in vi_basis.hip, basis-major so that every access is a
// contiguous run of points), the rows of points outside the hull set to NaN, so that the mask costs nothing afterwards: NaN
// times anything is NaN.  The evaluation is then a plain product out(Q x T) = Y(Q x N) C(N x T) - K2r, or the library's GEMM in
// tiles of 128 timesteps (tools/microbench/dgemm_eval_shape.hip: 59 TFLOP/s at 128, 32 at 64, 56 at 256; Y is read once per
// tile: 0.15 B/flop).
extern "C" int vi_eval_resident_f64(vi_model* m, int64_t Q, int64_t T, const double* d_Y, const double* d_C, double* d_out)
{
    VI_REQUIRE(m && d_Y && d_C && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && T >= 0, "negative size");
    if (Q == 0 || T == 0) return VI_OK;
    VI_HIP(hipSetDevice(m->ctx->device));
    EvalTimer timer(m->ctx);
    return eval_resident(m, Q, T, d_Y, d_C, d_out);
}

// Peak maps along one axis of a resident grid (include/vinterp.h).  K2p where the shape is its own; else, and with
// VINTERP_K2P=twopass or VINTERP_EVAL_RESIDENT=blas: the density product of vi_eval_resident_f64 into d_work, a slab of as many
// timesteps as it holds, and k_peak_columns over the slab.
extern "C" size_t vi_eval_resident_peak_work_bytes(vi_model* m, int64_t outer, int64_t L, int64_t inner, int64_t T)
{
    if (!m || outer <= 0 || L <= 0 || inner <= 0 || T <= 0) return 0;
    if (vi_peak_fused_shape(m->N, outer, L, inner)) return vi_peak_fused_work_bytes(outer, L, T);
    return (size_t)T * (size_t)(outer * L * inner) * sizeof(double);
}

extern "C" int vi_eval_resident_peak_f64(vi_model* m, int64_t outer, int64_t L, int64_t inner, int64_t T, const double* d_Y,
                                         const double* d_C, int32_t kind, double* d_val, int32_t* d_idx, void* d_work,
                                         size_t work_bytes)
{
    VI_REQUIRE(m && d_Y && d_C && d_val && d_idx, "null argument");
    VI_REQUIRE(outer >= 0 && L >= 0 && inner >= 0 && T >= 0, "negative size");
    VI_REQUIRE(kind == 0 || kind == 1, "kind must be 0 (max) or 1 (min)");
    VI_REQUIRE(L <= 0x7fffffffLL, "the reduced axis is longer than a 32-bit index");
    const int64_t M = outer * inner, Q = M * L;
    if (Q == 0 || T == 0) return VI_OK;
    VI_REQUIRE(d_work, "null work space");
    vi_ctx* c = m->ctx;
    VI_HIP(hipSetDevice(c->device));
    EvalTimer timer(c);
    if (inner == 1) {
        int handled = 0;
        const int rc = vi_eval_resident_peak_mfma(c, m->N, outer, L, T, d_Y, d_C, kind, d_val, d_idx, d_work, work_bytes, &handled);
        if (rc != VI_OK || handled) return rc;
    }
    const int64_t slab = (int64_t)(work_bytes / ((size_t)Q * sizeof(double)));
    VI_REQUIRE(slab >= 1, "work space smaller than the density map of one timestep");
    for (int64_t t0 = 0; t0 < T; t0 += slab) {
        const int64_t tc = (T - t0) < slab ? (T - t0) : slab;
        int rc = eval_resident(m, Q, tc, d_Y, d_C + t0 * m->N, (double*)d_work);
        if (rc != VI_OK) return rc;
        rc = vi_peak_columns(c, outer, L, inner, tc, kind, (const double*)d_work, d_val + t0 * M, d_idx + t0 * M);
        if (rc != VI_OK) return rc;
    }
    return VI_OK;
}

// Crossing maps along one axis of a resident grid (include/vinterp.h): the slab loop of the peak's two-pass path - the density
// product of vi_eval_resident_f64 into d_work, as many timesteps as it holds, and k_cross_columns (vi_level.hip) over the slab.
// An axis of one sample has no pair of neighbours: no product, every column -1.
extern "C" int vi_eval_resident_cross_f64(vi_model* m, int64_t outer, int64_t L, int64_t inner, int64_t T, const double* d_Y,
                                          const double* d_C, const double* d_level, int32_t which, int32_t direction,
                                          int32_t* d_idx, void* d_work, size_t work_bytes)
{
    VI_REQUIRE(m && d_Y && d_C && d_level && d_idx, "null argument");
    VI_REQUIRE(outer >= 0 && L >= 0 && inner >= 0 && T >= 0, "negative size");
    VI_REQUIRE(which == 0 || which == 1, "which must be 0 (first) or 1 (last)");
    VI_REQUIRE(direction >= 0 && direction <= 2, "direction must be 0 (any), 1 (up) or 2 (down)");
    VI_REQUIRE(L <= 0x7fffffffLL, "the axis is longer than a 32-bit index");
    const int64_t M = outer * inner, Q = M * L;
    if (Q == 0 || T == 0) return VI_OK;
    VI_REQUIRE(d_work, "null work space");
    vi_ctx* c = m->ctx;
    VI_HIP(hipSetDevice(c->device));
    EvalTimer timer(c);
    const int64_t slab = (int64_t)(work_bytes / ((size_t)Q * sizeof(double)));
    VI_REQUIRE(slab >= 1, "work space smaller than the density map of one timestep");
    for (int64_t t0 = 0; t0 < T; t0 += slab) {
        const int64_t tc = (T - t0) < slab ? (T - t0) : slab;
        int rc = L > 1 ? eval_resident(m, Q, tc, d_Y, d_C + t0 * m->N, (double*)d_work) : (int)VI_OK;
        if (rc != VI_OK) return rc;
        rc = vi_cross_columns(c, outer, L, inner, tc, which, direction, (const double*)d_work, d_level + t0 * M, d_idx + t0 * M);
        if (rc != VI_OK) return rc;
    }
    return VI_OK;
}

// The reduced basis of a resident grid along one axis (include/vinterp.h): k_reduce_basis (vi_eval_resident.hip)
extern "C" int vi_reduce_basis_f64(vi_model* m, int64_t outer, int64_t L, int64_t inner, const double* d_Y, const double* d_w,
                                   double* d_Yr)
{
    VI_REQUIRE(m && d_Y && d_w && d_Yr, "null argument");
    VI_REQUIRE(outer >= 0 && L >= 0 && inner >= 0, "negative size");
    if (outer * inner == 0) return VI_OK;
    VI_HIP(hipSetDevice(m->ctx->device));
    return vi_reduce_basis(m->ctx, m->N, outer, L, inner, d_Y, d_w, d_Yr);
}

// ---- the library route of the forms.  A point has C components: 1, a column y of a basis matrix, the form y^T dC y and its
// square root, the standard error (first-order error propagation of the coefficient covariance; the `calcerr` output the
// reference's Estimate.__call__ advertises but never computes, estimate.py:139-145); or 3, the columns g_0, g_1, g_2 of a
// gradient basis, the nine forms g_c^T dC g_d and the six entries (0,0) (1,1) (2,2) (0,1) (0,2) (1,2) of their symmetric part,
// as K2c packs them.  Three steps, the same for every entry:
//   1. the points of a chunk are turned points-major into the work space: row d * P + q of A is component d of point q
//      (k_points_major, or k_points_major_at's gather);
//   2. B = A dC^T by the library (forms_product): 2 N^2 flop per row, MFMA-bound;
//   3. a wave per point takes the dots of its C rows of A with its C rows of B (k_rowdot).
// With the covariance chosen per point (the records entries) the three steps run once per run of equal record, raw, and
// k_records_finish blends the two records of a point or writes the NaN of a missing one (records_walk).
namespace {

constexpr int form_planes(int C) { return C * (C + 1) / 2; }          // what a point gives: 1 form, or 6 entries

// A[(d*P + q)*N + n] = Y[(n*C + d)*ldy + q]
template <int C>
__global__ void k_points_major(int64_t P, int N, const double* __restrict__ Y, int64_t ldy, double* __restrict__ A)
{
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;     // e = (n * C + d) * P + q: the reads along the rows
    if (e >= C * P * N) return;
    const int64_t nd = e / P, q = e - nd * P;
    const int64_t n = nd / C, d = nd - C * n;
    A[(d * P + q) * N + n] = Y[nd * ldy + q];
}

// k_points_major at one chosen point per column of a grid (outer, L, inner): row p of A is point (o, idx[m], i) of column
// m = m0 + p = o inner + i; a row of NaN for an index outside [0, L), which is never turned into an address
__global__ void k_points_major_at(int64_t P, int N, const double* __restrict__ Y, int64_t Q, int64_t L, int64_t inner, int64_t m0,
                                  const int* __restrict__ idx, double* __restrict__ A)
{
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;     // e = n * P + p, as k_points_major
    if (e >= P * N) return;
    const int64_t n = e / P, p = e - n * P;
    const int64_t m = m0 + p, l = idx[m], o = m / inner;
    A[p * N + n] = (l >= 0 && l < L) ? Y[n * Q + (o * L + l) * inner + (m - o * inner)] : __builtin_nan("");
}

// A wave per point: the C x C dots M[c][d] = A_c[p] . B_d[p] of its rows of A with its rows of B.  One component: out[p] = M,
// or with ROOT its square root - a negative variance (indefinite dC) gives NaN, as np.sqrt would.  Three: the six entries of
// the symmetric part, 1/2 (M[c][d] + M[d][c]), into the planes out[k*ldo + p].
template <int C, bool ROOT>
__global__ void k_rowdot(int64_t P, int N, const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ out,
                         int64_t ldo)
{
    static_assert(C == 1 || (C == 3 && !ROOT), "a form and its root, or the raw entries of a 3 x 3 covariance");
    const int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= P) return;
    double M[C][C];
    for (int c = 0; c < C; ++c)
        for (int d = 0; d < C; ++d) M[c][d] = 0.0;
    for (int n = lane; n < N; n += 64) {
        double a[C], b[C];
        for (int c = 0; c < C; ++c) {
            a[c] = A[(c * P + p) * N + n];
            b[c] = B[(c * P + p) * N + n];
        }
        for (int c = 0; c < C; ++c)
            for (int d = 0; d < C; ++d) M[c][d] = fma(a[c], b[d], M[c][d]);
    }
    for (int c = 0; c < C; ++c)
        for (int d = 0; d < C; ++d)
            for (int o = 32; o > 0; o >>= 1) M[c][d] += __shfl_down(M[c][d], o);
    if (lane != 0) return;
    if constexpr (C == 1) {
        out[p] = ROOT ? sqrt(M[0][0]) : M[0][0];
    } else {
        out[0 * ldo + p] = M[0][0];
        out[1 * ldo + p] = M[1][1];
        out[2 * ldo + p] = M[2][2];
        out[3 * ldo + p] = 0.5 * (M[0][1] + M[1][0]);
        out[4 * ldo + p] = 0.5 * (M[0][2] + M[2][0]);
        out[5 * ldo + p] = 0.5 * (M[1][2] + M[2][1]);
    }
}

// out[k*ldo + q], k < K, from the raw values F0[k*ldf + q] of record rec[q] and - in blend mode, w != nullptr - F1[k*ldf + q] of
// the next one (vi_err_blend), with ROOT the square root of that; NaN without a record
template <int K, bool ROOT>
__global__ void k_records_finish(int64_t P, const int* __restrict__ rec, const double* __restrict__ w, int R,
                                 const double* __restrict__ F0, const double* __restrict__ F1, int64_t ldf,
                                 double* __restrict__ out, int64_t ldo)
{
    const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (q >= P) return;
    const int r = rec[q];
    const bool none = r < 0 || (int64_t)r + (w ? 1 : 0) >= R;
    for (int k = 0; k < K; ++k) {
        double v = __builtin_nan("");
        if (!none && ROOT) v = w ? vi_err_blend_sqrt(w[q], F0[k * ldf + q], F1[k * ldf + q]) : sqrt(F0[k * ldf + q]);
        if (!none && !ROOT) v = w ? vi_err_blend(w[q], F0[k * ldf + q], F1[k * ldf + q]) : F0[k * ldf + q];
        out[k * ldo + q] = v;
    }
}

// Row-major B (rows x N) = A (rows x N) dC^T, B[q][i] = sum_k dC[i][k] A[q][k], so that A[q] . B[q] = a_q^T dC a_q.  To the
// library, which reads column-major: B^T (N x rows) = op(dC^T) A^T, the row-major dC being the column-major dC^T.
int forms_product(vi_ctx* c, int N, int64_t rows, const double* d_dC, const double* A, double* B)
{
    const double one = 1.0, zero = 0.0;
    VI_ROCBLAS(rocblas_dgemm(c->blas, rocblas_operation_transpose, rocblas_operation_none, N, (rocblas_int)rows, N, &one, d_dC, N,
                             A, N, &zero, B, N));
    return VI_OK;
}

// steps 2 and 3 on the P points of a points-major tile A with one covariance
template <int C, bool ROOT>
int forms_tile(vi_ctx* c, int N, int64_t P, const double* A, const double* d_dC, double* B, double* d_out, int64_t ldo)
{
    const int rc = forms_product(c, N, C * P, d_dC, A, B);
    if (rc != VI_OK) return rc;
    hipLaunchKernelGGL((k_rowdot<C, ROOT>), dim3(nblocks(P, 4)), dim3(256), 0, c->stream, P, N, A, B, d_out, ldo);
    VI_HIP(hipGetLastError());
    return VI_OK;
}

// T covariances on the Q points of a resident matrix d_Y with row stride ldy (Q of its columns): a chunk points-major once,
// then steps 2 and 3 per timestep into d_out[(t * planes + k)*ldo + q] - the error maps at one component, the raw entries at
// three.  AB: 2 C min(Q, vi_forms_chunk(N, C)) N doubles.
template <int C>
int forms_library(vi_ctx* c, int N, int64_t Q, int64_t T, const double* d_Y, int64_t ldy, const double* d_dC, double* d_out,
                  int64_t ldo, double* AB)
{
    const int64_t chunk = std::min(Q, vi_forms_chunk(N, C));
    double* A = AB;
    double* B = A + C * chunk * N;
    return for_chunks(Q, chunk, [&](int64_t q0, int64_t qc) -> int {
        hipLaunchKernelGGL(k_points_major<C>, dim3(nblocks(C * qc * N, 256)), dim3(256), 0, c->stream, qc, N, d_Y + q0, ldy, A);
        VI_HIP(hipGetLastError());
        for (int64_t t = 0; t < T; ++t) {
            const int rc = forms_tile<C, C == 1>(c, N, qc, A, d_dC + t * N * N, B, d_out + t * form_planes(C) * ldo + q0, ldo);
            if (rc != VI_OK) return rc;
        }
        return VI_OK;
    });
}

// The walk of the records entries over Q points with C components.  It reads d_rec back to find the runs, so it waits for the
// stream.  Per chunk of `chunk` points: turn(AB, q0, qc) once; for every run [a, b) of equal record r inside it, in nearest mode
// run(AB, q0, a, b, dC_r, F0 + a), in blend mode again with dC_(r+1) and F1 - the raw values of the run into planes of pitch
// `chunk` -, a run without a record skipped; then k_records_finish.  work: vi_forms_work_doubles(N, C, chunk) doubles - AB in
// front, the two sets of planes behind - or nullptr: taken from the context workspace.
template <int C, class Turn, class Run>
int records_walk(vi_ctx* c, int N, int64_t Q, int64_t chunk, const int32_t* d_rec, const double* d_w, int64_t R,
                 const double* d_dC, double* d_out, int64_t ldo, double* work, Turn&& turn, Run&& run)
{
    constexpr int K = form_planes(C);
    std::vector<int32_t> rec((size_t)Q);
    VI_HIP(hipMemcpyAsync(rec.data(), d_rec, (size_t)Q * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    VI_HIP(hipStreamSynchronize(c->stream));
    if (!work) {
        void* ws = nullptr;
        const int rc = vi_ctx_workspace(c, vi_forms_work_doubles(N, C, chunk) * sizeof(double), &ws);
        if (rc != VI_OK) return rc;
        work = (double*)ws;
    }
    double* AB = work;
    double* F[2] = {AB + 2 * C * chunk * N, AB + 2 * C * chunk * N + K * chunk};
    const int npass = d_w ? 2 : 1;
    return for_chunks(Q, chunk, [&](int64_t q0, int64_t qc) -> int {
        int rc = turn(AB, q0, qc);
        if (rc != VI_OK) return rc;
        for (int64_t a = 0, b; a < qc; a = b) {              // the run [a, b) of record r
            const int64_t r = rec[q0 + a];
            for (b = a + 1; b < qc && rec[q0 + b] == r; ++b) {}
            if (r < 0 || r + npass - 1 >= R) continue;       // no record: k_records_finish reads no value
            for (int pass = 0; pass < npass; ++pass)
                if ((rc = run(AB, q0, a, b, d_dC + (r + pass) * N * N, F[pass] + a)) != VI_OK) return rc;
        }
        hipLaunchKernelGGL((k_records_finish<K, C == 1>), dim3(nblocks(qc, 256)), dim3(256), 0, c->stream, qc, d_rec + q0,
                           d_w ? d_w + q0 : nullptr, (int)R, F[0], F[1], chunk, d_out + q0, ldo);
        VI_HIP(hipGetLastError());
        return VI_OK;
    });
}

}  // namespace

// points per chunk of the library route: a work space of at most 512 MB for A and B (233 000 points at N = 144 and one
// component, 77 000 at three).  Callers clip it to their point count.
int64_t vi_forms_chunk(int N, int components) { return std::max<int64_t>(1, ((int64_t)1 << 25) / ((int64_t)components * N)); }

// the doubles of the work space of the records entries at chunks of `chunk` points: A, B and two sets of planes
size_t vi_forms_work_doubles(int N, int components, int64_t chunk)
{
    return (size_t)2 * components * chunk * N + (size_t)2 * form_planes(components) * chunk;
}

// Points (rays) per chunk of vi_eval_track_err_f64 and vi_eval_slant_err_f64: the basis of a chunk takes at most 256 MB of the
// context workspace, half of what the library route of vi_eval_resident_err_f64 asks for its two matrices - with which the
// library route of a chunk (vi_records_err) fits beside it.  Even, so that every chunk of an even call keeps K2te's shape.
// VINTERP_TRACK_ERR_CHUNK: a smaller chunk (tests: several chunks at a small Q).
int64_t track_err_chunk(int N, int64_t Q)
{
    const int64_t chunk = std::max<int64_t>(2, vi_forms_chunk(N, 1) & ~(int64_t)1);
    return std::min(Q, test_chunk("VINTERP_TRACK_ERR_CHUNK", chunk, 2));
}

// The workspace of a chunked call: the basis Y (N x chunk), `extra` doubles for the caller, and - unless every chunk is K2te's -
// the work space of the library route (else *work = nullptr)
int track_err_workspace(vi_model* m, int64_t Q, int64_t chunk, const double* d_out, size_t extra, double** Y, double** X,
                        double** work)
{
    const bool own = vi_eval_records_err_shape(m->N, Q, nullptr, d_out);      // (chunks are even, Y is the workspace's)
    return ws_carve(m->ctx, [&](ws_carver& w) {
        *Y = w.take<double>((size_t)chunk * m->N, 256);
        *X = w.take<double>(extra, 256);
        *work = w.take<double>(own ? 0 : vi_forms_work_doubles(m->N, 1, chunk), 256);
        if (own) *work = nullptr;
    });
}

// d_out[p] = sqrt(a_p^T dC a_p) of the P rows of the row-major tile A (P x N); B: P N doubles
int vi_forms_tile(vi_ctx* c, int N, int64_t P, const double* A, const double* d_dC, double* B, double* d_out)
{
    return forms_tile<1, true>(c, N, P, A, d_dC, B, d_out, 0);
}

// Standard-error maps of many timesteps on the resident grid: out[t*Q + q] = sqrt(sum_ik Y[i][q] dC[t][i][k] Y[k][q]).  K2e
// (vi_eval_resident.hip) for N <= 144; other shapes and orders, and VINTERP_EVAL_RESIDENT=blas: forms_library on the context
// workspace.
extern "C" int vi_eval_resident_err_f64(vi_model* m, int64_t Q, int64_t T, const double* d_Y, const double* d_dC, double* d_out)
{
    VI_REQUIRE(m && d_Y && d_dC && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && T >= 0, "negative size");
    if (Q == 0 || T == 0) return VI_OK;
    vi_ctx* c = m->ctx;
    VI_HIP(hipSetDevice(c->device));
    const int N = m->N;
    {
        EvalTimer timer(c);
        int handled = 0;
        const int rc = vi_eval_resident_err_mfma(c, N, Q, T, d_Y, d_dC, d_out, &handled);      // K2e
        if (rc != VI_OK || handled) return rc;
    }
    void* ws = nullptr;
    const int rc = vi_ctx_workspace(c, (size_t)2 * std::min(Q, vi_forms_chunk(N, 1)) * N * sizeof(double), &ws);
    if (rc != VI_OK) return rc;
    EvalTimer timer(c);
    return forms_library<1>(c, N, Q, T, d_Y, Q, d_dC, d_out, Q, (double*)ws);
}

// The form of vi_eval_resident_err_f64 at one chosen point per column and timestep (include/vinterp.h): K2eg
// (vi_eval_resident.hip) for N <= 144.  Other orders, and VINTERP_EVAL_RESIDENT=blas: timestep by timestep the chosen columns
// of a chunk are gathered point-major into the context workspace (k_points_major_at), then steps 2 and 3; the NaN row of an
// index outside [0, L) gives the NaN of the column.
extern "C" int vi_eval_resident_err_at_f64(vi_model* m, int64_t outer, int64_t L, int64_t inner, int64_t T, const double* d_Y,
                                           const double* d_dC, const int32_t* d_idx, double* d_out)
{
    VI_REQUIRE(m && d_Y && d_dC && d_idx && d_out, "null argument");
    VI_REQUIRE(outer >= 0 && L >= 0 && inner >= 0 && T >= 0, "negative size");
    VI_REQUIRE(L <= 0x7fffffffLL, "the indexed axis is longer than a 32-bit index");
    const int64_t M = outer * inner, Q = M * L;
    if (M == 0 || T == 0) return VI_OK;
    vi_ctx* c = m->ctx;
    VI_HIP(hipSetDevice(c->device));
    const int N = m->N;
    if (L == 0) {                            // columns of length zero: no index is inside, d_Y holds nothing to read - all NaN
        VI_HIP(hipMemsetAsync(d_out, 0xFF, (size_t)(T * M) * sizeof(double), c->stream));
        return VI_OK;
    }
    {
        EvalTimer timer(c);
        int handled = 0;
        const int rc = vi_eval_resident_err_at_mfma(c, N, outer, L, inner, T, d_Y, d_dC, d_idx, d_out, &handled);   // K2eg
        if (rc != VI_OK || handled) return rc;
    }
    const int64_t chunk = std::min(M, vi_forms_chunk(N, 1));          // columns per chunk
    void* ws = nullptr;
    const int rc = vi_ctx_workspace(c, (size_t)2 * chunk * N * sizeof(double), &ws);
    if (rc != VI_OK) return rc;
    double* A = (double*)ws;
    double* B = A + chunk * N;
    EvalTimer timer(c);
    for (int64_t t = 0; t < T; ++t) {
        const int rc = for_chunks(M, chunk, [&](int64_t m0, int64_t mc) -> int {
            hipLaunchKernelGGL(k_points_major_at, dim3(nblocks(mc * N, 256)), dim3(256), 0, c->stream, mc, N, d_Y, Q, L, inner, m0,
                               d_idx + t * M, A);
            VI_HIP(hipGetLastError());
            return forms_tile<1, true>(c, N, mc, A, d_dC + t * N * N, B, d_out + t * M + m0, 0);
        });
        if (rc != VI_OK) return rc;
    }
    return VI_OK;
}

// vi_eval_records_err_f64 without its checks and its timer: K2te (vi_eval_resident.hip) for the shapes K2e takes; other shapes
// and orders, and VINTERP_EVAL_RESIDENT=blas, through records_walk - the columns of a chunk points-major once, a run a slice of
// that tile.  work: vi_forms_work_doubles(N, 1, min(Q, vi_forms_chunk(N, 1))) doubles for the library route, or nullptr.
int vi_records_err(vi_model* m, int64_t Q, const double* d_Y, const int32_t* d_rec, const double* d_w, int64_t R,
                   const double* d_dC, double* d_out, double* work)
{
    vi_ctx* c = m->ctx;
    const int N = m->N;
    int handled = 0;
    const int rc = vi_eval_records_err_mfma(c, N, Q, d_Y, d_rec, d_w, R, d_dC, d_out, &handled);     // K2te
    if (rc != VI_OK || handled) return rc;
    const int64_t chunk = std::min(Q, vi_forms_chunk(N, 1));
    return records_walk<1>(
        c, N, Q, chunk, d_rec, d_w, R, d_dC, d_out, 0, work,
        [&](double* A, int64_t q0, int64_t qc) -> int {
            hipLaunchKernelGGL(k_points_major<1>, dim3(nblocks(qc * N, 256)), dim3(256), 0, c->stream, qc, N, d_Y + q0, Q, A);
            VI_HIP(hipGetLastError());
            return VI_OK;
        },
        [&](double* A, int64_t, int64_t a, int64_t b, const double* dC, double* f) -> int {
            return forms_tile<1, false>(c, N, b - a, A + a * N, dC, A + (chunk + a) * N, f, 0);
        });
}

extern "C" int vi_eval_records_err_f64(vi_model* m, int64_t Q, const double* d_Y, const int32_t* d_rec, const double* d_w,
                                       int64_t R, const double* d_dC, double* d_out)
{
    VI_REQUIRE(m && d_Y && d_rec && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && R >= 0, "negative size");
    VI_REQUIRE(R == 0 || d_dC, "record count given without covariances");
    VI_REQUIRE(R <= 0x7fffffffLL, "more records than a 32-bit record index");
    if (Q == 0) return VI_OK;
    VI_HIP(hipSetDevice(m->ctx->device));
    EvalTimer timer(m->ctx);
    return vi_records_err(m, Q, d_Y, d_rec, d_w, R, d_dC, d_out, nullptr);
}

// Gradient-covariance maps on a resident gradient basis: out[(t*6 + k)*ldo + q] = g_c^T 1/2 (dC_t + dC_t^T) g_d, (c, d) the
// k-th of (0,0) (1,1) (2,2) (0,1) (0,2) (1,2), g_c = column (c, q) of d_G[(n*3 + c)*Q + q].  K2c (vi_eval_resident.hip) for
// N <= 144; other orders, and VINTERP_EVAL_RESIDENT=blas: forms_library at three components.  AB: 6 min(Q, vi_forms_chunk(N, 3))
// N doubles for the library route, or nullptr: taken from the context workspace when that route runs.
int vi_resident_gradcov(vi_model* m, int64_t Q, int64_t T, const double* d_G, const double* d_dC, double* d_out, int64_t ldo,
                        double* AB)
{
    vi_ctx* c = m->ctx;
    const int N = m->N;
    int handled = 0;
    int rc = vi_eval_resident_gradcov_mfma(c, N, Q, T, d_G, d_dC, d_out, ldo, &handled);      // K2c
    if (rc != VI_OK || handled) return rc;
    if (!AB) {
        void* ws = nullptr;
        rc = vi_ctx_workspace(c, (size_t)6 * std::min(Q, vi_forms_chunk(N, 3)) * N * sizeof(double), &ws);
        if (rc != VI_OK) return rc;
        AB = (double*)ws;
    }
    return forms_library<3>(c, N, Q, T, d_G, Q, d_dC, d_out, ldo, AB);
}

// vi_eval_records_gradcov_f64 without its checks and its timer: the Q points of the gradient basis d_G (N x 3 x Q) into d_out
// with plane stride ldo.  K2tc (vi_eval_resident.hip) for N <= 144; other orders, and VINTERP_EVAL_RESIDENT=blas, through
// records_walk - every run turned points-major on its own, forms_library with T = 1 on the run's columns.  work:
// vi_forms_work_doubles(N, 3, min(Q, vi_forms_chunk(N, 3))) doubles for the library route, or nullptr.
int vi_records_gradcov(vi_model* m, int64_t Q, const double* d_G, const int32_t* d_rec, const double* d_w, int64_t R,
                       const double* d_dC, double* d_out, int64_t ldo, double* work)
{
    vi_ctx* c = m->ctx;
    const int N = m->N;
    int handled = 0;
    const int rc = vi_eval_records_gradcov_mfma(c, N, Q, d_G, d_rec, d_w, R, d_dC, d_out, ldo, &handled);      // K2tc
    if (rc != VI_OK || handled) return rc;
    const int64_t chunk = std::min(Q, vi_forms_chunk(N, 3));
    return records_walk<3>(
        c, N, Q, chunk, d_rec, d_w, R, d_dC, d_out, ldo, work, [](double*, int64_t, int64_t) -> int { return VI_OK; },
        [&](double* AB, int64_t q0, int64_t a, int64_t b, const double* dC, double* f) -> int {
            return forms_library<3>(c, N, b - a, 1, d_G + q0 + a, Q, dC, f, chunk, AB);
        });
}

extern "C" int vi_eval_records_gradcov_f64(vi_model* m, int64_t Q, const double* d_G, const int32_t* d_rec, const double* d_w,
                                           int64_t R, const double* d_dC, double* d_out)
{
    VI_REQUIRE(m && d_G && d_rec && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && R >= 0, "negative size");
    VI_REQUIRE(R == 0 || d_dC, "record count given without covariances");
    VI_REQUIRE(R <= 0x7fffffffLL, "more records than a 32-bit record index");
    if (Q == 0) return VI_OK;
    VI_HIP(hipSetDevice(m->ctx->device));
    EvalTimer timer(m->ctx);
    return vi_records_gradcov(m, Q, d_G, d_rec, d_w, R, d_dC, d_out, Q, nullptr);
}

extern "C" int vi_eval_resident_gradcov_f64(vi_model* m, int64_t Q, int64_t T, const double* d_G, const double* d_dC,
                                            double* d_out)
{
    VI_REQUIRE(m && d_G && d_dC && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && T >= 0, "negative size");
    if (Q == 0 || T == 0) return VI_OK;
    vi_ctx* c = m->ctx;
    VI_HIP(hipSetDevice(c->device));
    EvalTimer timer(c);
    return vi_resident_gradcov(m, Q, T, d_G, d_dC, d_out, Q, nullptr);
}
