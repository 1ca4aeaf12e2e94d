/* vinterp.h - C-ABI of libvinterp.so, the MI355X (gfx950) implementation of the per-timestep
 * fit + evaluate hot path of amisr/volumetricinterp.
 *
 * The reference is pure Python and has NO C/FFI boundary: its only plug-in seam is
 * the Python `Model` class contract (volumetricinterp/models/sphharmlag.py:11-15).  This header is
 * therefore the boundary *underneath* the reference's Python surface; each entry point cites the
 * reference function whose arithmetic it replaces.  The binding a maintainer adds on the reference
 * side is a ctypes stub - see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 (VI_OK) or a negative vi_status; nothing throws across the ABI;
 *     vi_last_error() returns a thread-local message for the last failure.
 *   - one vi_ctx per GPU, used from one host thread at a time.  All work is enqueued on the
 *     context's own HIP stream; entry points taking device pointers are ASYNCHRONOUS on that
 *     stream (call vi_ctx_sync), entry points taking host pointers stage H2D/D2H and return when
 *     the result is in the caller's buffer.
 *   - "d_" parameters are device pointers obtained from vi_dmalloc on the same context;
 *     "h_" parameters are caller-owned, C-contiguous host buffers.  All reals are IEEE fp64.
 *   - a failed timestep is reported through its outputs (NaN rows), never through the status.
 */
#ifndef VINTERP_H
#define VINTERP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): vi_warm_solve_f64 / vi_basis_solve_f64 / vi_warm_rebase_f64 take a trailing d_sweeps pointer,
 * vi_warm_chi2_one_f64 writes THREE doubles to h_chi2, vi_brent_warm_supported added, h_rebase of vi_brent_warm_f64 /
 * vi_brent_host_one_f64 is 10 doubles (jump rule).  _lib.py refuses any other version. */
#define VI_ABI_VERSION 2

typedef enum vi_status {
    VI_OK = 0,
    VI_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, unsupported order) */
    VI_ERR_HIP = -2,         /* HIP runtime failure */
    VI_ERR_ROCBLAS = -3,
    VI_ERR_ROCSOLVER = -4,
    VI_ERR_NOMEM = -5,
    VI_ERR_UNSUPPORTED = -6,
    VI_ERR_RCCL = -7
} vi_status;

typedef struct vi_ctx vi_ctx;       /* one per GPU: device id, stream, rocBLAS handle, workspaces */
typedef struct vi_model vi_model;   /* device-resident tables of one basis model */

enum { VI_MODEL_SPHHARMLAG = 1, VI_MODEL_RADBASFUN = 2 };

/* One group of spherical-cap-harmonic degrees nu_l = nv_l + v0 that share the fractional part v0
 * (sphharmlag.py:101-115 `nu`).  The Legendre functions P_nu^m(cos theta) of scipy.special.lpmv
 * (called at sphharmlag.py:141) are produced by an upward degree recurrence seeded at degrees
 * v0+m and v0+m+1, normalised so that one step is  p_j = x p_{j-1} - c[j][m] p_{j-2}. */
typedef struct vi_sph_group {
    double v0;               /* fractional part of the degrees of this group (0 -> closed-form seeds) */
    int32_t nvmax;           /* largest integer part in the group */
    int32_t nterms;          /* length of the 2F1 series tables (0 when v0 == 0) */
    const int32_t* pick;     /* [nvmax+2]   l whose degree has integer part j, or -1 */
    const double* c;         /* [(nvmax+2) x maxl]  normalised recurrence coefficient c[j][m] (one degree beyond
                                nvmax: grad_basis evaluates lpmv(m, nu+1, x), sphharmlag.py:177) */
    const double* seed_pref; /* [2 x maxl]  prefactor of the two seeds of chain m (v0 != 0) */
    const double* seed_q;    /* [2 x maxl x nterms]  term ratios of the 2F1 series (v0 != 0) */
} vi_sph_group;

/* Model description (host side).  Built by volumetricinterp_amd.models.<NAME>.Model from the same
 * INI keys the reference parses (sphharmlag.py:65-75, radbasfun.py:65-78). */
typedef struct vi_model_desc {
    int32_t kind;            /* VI_MODEL_* */
    int32_t nbasis;          /* N = maxk*maxl^2 (sphharmlag.py:59) or NUMGRIDPNT^3 (radbasfun.py:60) */
    /* --- sphharmlag --- */
    int32_t maxk, maxl;
    double rot_cos, rot_sin; /* cos/sin(theta0) of the Rodrigues rotation, sphharmlag.py:346,353 */
    double rot_kx, rot_ky;   /* rotation axis k = (kx, ky, 0), sphharmlag.py:349 */
    double earth_radius;     /* RE, sphharmlag.py:9 */
    int32_t ngroups;
    const vi_sph_group* groups;
    const double* coef_scale;/* [maxl^2] per (l, signed m): Kvm(nu_l,|m|) (sphharmlag.py:305-321) x the
                                lpmv negative-order factor x the chain normalisation */
    const double* coef_scale1;/* [maxl^2] the same constant for degree nu_l + 1 (gradient basis only) */
    const double* nu;        /* [maxl] the degrees nu_l (gradient basis only) */
    /* --- radbasfun --- */
    const double* centers;   /* [N x 3] ECEF metres (radbasfun.py:59) */
    double eps;              /* radbasfun.py:72 */
} vi_model_desc;

/* ---- context / memory --------------------------------------------------------------------- */
int  vi_abi_version(void);
int  vi_device_count(int* count);
int  vi_ctx_create(int device, vi_ctx** out);
void vi_ctx_destroy(vi_ctx* ctx);
int  vi_ctx_sync(vi_ctx* ctx);
const char* vi_last_error(void);

int  vi_dmalloc(vi_ctx* ctx, size_t bytes, void** d_ptr);
int  vi_dfree(vi_ctx* ctx, void* d_ptr);
int  vi_h2d(vi_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);   /* synchronous */
int  vi_d2h(vi_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);   /* synchronous */
int  vi_dmemset(vi_ctx* ctx, void* d_ptr, int value, size_t bytes);
/* A download that does not hold the context's stream (the reference has no counterpart: its covariances, interpolate.py:466,
 * are host arrays already).  vi_d2h_side_mark: after the launches that produce the data, from the launching thread.
 * vi_d2h_side: blocking, from any host thread - copies on a second stream once the marked work has finished, while the
 * context's stream runs on.  The source must stay untouched until vi_d2h_side returns. */
int  vi_d2h_side_mark(vi_ctx* ctx);
int  vi_d2h_side(vi_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);

/* HIP-event timing on the context's stream (bench.py measures kernels on the stream they run on) */
/* free / total memory of the context's device (hipMemGetInfo) */
int  vi_mem_info(vi_ctx* ctx, size_t* free_bytes, size_t* total_bytes);
int  vi_timer_start(vi_ctx* ctx);
int  vi_timer_stop_ms(vi_ctx* ctx, double* ms);   /* synchronises on the stop event */

/* ---- model -------------------------------------------------------------------------------- */
int  vi_model_create(vi_ctx* ctx, const vi_model_desc* desc, vi_model** out);
void vi_model_destroy(vi_model* model);

/* ---- basis assembly: replaces Model.basis (sphharmlag.py:118-145, radbasfun.py:83-112) ------
 * A[p*ld_p + n*ld_n] for p < P, n < N.  (ld_p, ld_n) = (N, 1) gives the reference's row-major
 * (P, N) layout; (1, P) gives the N x P layout the fit kernels consume (coalesced stores). */
int  vi_basis_f64(vi_model* model, int64_t P, const double* d_lat, const double* d_lon,
                  const double* d_alt, double* d_A, int64_t ld_p, int64_t ld_n);
/* gradient basis: replaces Model.grad_basis (sphharmlag.py:148-184; next row N1 - the reference never calls it).
 * G[p*ld_p + c*ld_c + n*ld_n], c = 0,1,2 = components along z, theta, phi.  sphharmlag only, (MAXL, MAXK) within (6, 4),
 * (12, 8) or (2, 12); other orders return VI_ERR_UNSUPPORTED (here and in vi_eval_grad_f64 / vi_eval_grad_basis_f64). */
int  vi_grad_basis_f64(vi_model* model, int64_t P, const double* d_lat, const double* d_lon,
                       const double* d_alt, double* d_G, int64_t ld_p, int64_t ld_c, int64_t ld_n);
/* gradient of the fitted parameter, out[q*3 + c] = sum_n grad_basis[q][c][n] * C[n] (c = z, theta, phi components as
 * sphharmlag.py:148-184 defines them): the contraction the reference's Estimate.__call__ advertises as `calcgrad`
 * (estimate.py:125-147, dead code there); the (Q, 3, N) array is never formed. */
int  vi_eval_grad_f64(vi_model* model, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                      const double* d_C, double* d_out);
/* standard error of the fitted parameter, err[q] = sqrt(a_q^T dC a_q) with a_q the basis row of point q and dC the
 * (N x N) coefficient covariance of the record: the `calcerr` output of the same dead branch (estimate.py:139-145) */
int  vi_eval_err_f64(vi_model* model, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                     const double* d_dC, double* d_out);
/* model coordinates (z, theta, phi) of sphharmlag.py:324-359 `transform_coord`; ECEF x,y,z for RBF */
int  vi_transform_f64(vi_model* model, int64_t P, const double* d_lat, const double* d_lon,
                      const double* d_alt, double* d_c0, double* d_c1, double* d_c2);

/* ---- fused evaluation: replaces Estimate.__call__ (estimate.py:110-123) ---------------------
 * out[t*Q + q] = sum_n basis_n(q) * C[t*N + n]; NaN where the point fails the convex-hull test
 * (estimate.py:119-121, :153-178) when hull_eq != NULL: a point is inside iff
 * max_f (hull_eq[f][0..2] . ecef(q) + hull_eq[f][3]) <= hull_tol.  The basis matrix is never
 * materialised.  hull_eq is what scipy.spatial.ConvexHull(...).equations holds (unit normals, metres); the test is exact
 * in fp64 for any list - a reduced-precision pass only sorts out the points further from the surface than its own error
 * bound, which assumes nothing but scales with the longest normal (lists of much shorter normals run slower, not wrong). */
int  vi_eval_f64(vi_model* model, int64_t Q, const double* d_lat, const double* d_lon,
                 const double* d_alt, int64_t T, const double* d_C,
                 const double* d_hull_eq, int32_t F, double hull_tol, double* d_out);
/* Points that each carry their OWN time (a satellite pass, another radar's range gates, a profile every few minutes): one call
 * for a whole trajectory in place of one vi_eval_f64 call per record.  d_C holds the R coefficient rows of the file (R x N, as
 * stored), d_rec[q] the row of point q - what Estimate.get_C (estimate.py:180-221) selects for the point's time.
 *   nearest mode (d_w == NULL):   d_out[q] = D(d_rec[q], q),  D(r, q) = sum_n basis_n(q) * d_C[r*N + n]
 *   interpolation (d_w != NULL):  d_out[q] = (1 - d_w[q]) * D(d_rec[q], q) + d_w[q] * D(d_rec[q] + 1, q), computed as written:
 *                                 no shortcut at d_w = 0 or 1, so a NaN in either row of the pair gives NaN, as get_C's blend
 * NaN where the point fails the hull test (hull_eq != NULL, as in vi_eval_f64), where d_rec[q] < 0 (no record for the time)
 * and where the row the point needs - d_rec[q], in interpolation mode d_rec[q] + 1 - is >= R.  In nearest mode a NaN in a row
 * reaches the points of that row only (the row is selected, not multiplied by zero).  d_C is never read outside its R rows.
 * Correct for ANY order of d_rec, but the cost grows with the span of rows inside a group of 64 consecutive points: a group
 * evaluates its points once per window of 4 rows (3 in interpolation mode) between its lowest and highest row.  SORT the
 * points by d_rec: the passes beyond one per group are then at most about R / 3 in the whole call, whatever Q is.
 * Models and orders as vi_eval_f64 (sphharmlag up to (24, 16), RBF), fp64 chains whatever vi_model_set_eval_precision set.
 * The orders of vi_eval_f64's fast kernels run the tiled kernel K2t (csrc/vi_track.hip); other orders, VINTERP_EVAL=generic and the RBF model
 * read each point's own row(s) from global memory (correct, not tuned).  Asynchronous on the context's stream; timed for
 * vi_eval_kernel_ms like its siblings (tests/test_gpu_track.py). */
int  vi_eval_track_f64(vi_model* model, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                       const int32_t* d_rec, const double* d_w, int64_t R, const double* d_C,
                       const double* d_hull_eq, int32_t F, double hull_tol, double* d_out);
/* The gradient of the fitted parameter at points that each carry their OWN time: vi_eval_grad_f64's values with
 * vi_eval_track_f64's row selection, one call for a whole trajectory in place of one vi_eval_grad_f64 call per record.
 * d_out[q*3 + c], the layout of vi_eval_grad_f64: c = z, theta', phi' as vi_grad_basis_f64 defines them (VI_FRAME_MODEL, below)
 * or east, north, geodetic up (VI_FRAME_ENU: each point's triple turned by the point's own matrix in the kernel).  With
 * G(r, q)[c] = sum_n grad_basis[q][c][n] * d_C[r*N + n]:
 *   nearest mode (d_w == NULL):   d_out[q] = G(d_rec[q], q)
 *   interpolation (d_w != NULL):  d_out[q] = (1 - d_w[q]) * G(d_rec[q], q) + d_w[q] * G(d_rec[q] + 1, q), as written: a NaN in
 *                                 either row of the pair gives NaN at any d_w
 * A NaN triple where the point fails the hull test (the mask pass of vi_eval_track_f64; F = 0: no test), where d_rec[q] < 0,
 * where a row the point needs is >= R (R = 0: every point) and where such a row holds a NaN; a NaN row reaches no other row's
 * points (rows are selected, never multiplied by zero).  d_C (R x N, as stored) is never read outside its R rows.  A point's
 * bits depend on the point, its row(s) and d_w[q], not on the other points or their order.  Correct for ANY order of d_rec;
 * the cost grows with the span of rows in a group of 64 consecutive points as in vi_eval_track_f64 (windows of 4 rows, 3 when
 * blending): SORT the points by d_rec.  sphharmlag only, at the orders of vi_grad_basis_f64 - (MAXL, MAXK) within (6, 4),
 * (12, 8) or (2, 12) -, else VI_ERR_UNSUPPORTED.  Kernel K2tg (csrc/vi_track.hip).  Asynchronous on the context's stream;
 * timed for vi_eval_kernel_ms like its siblings (tests/test_gpu_track_gradient.py). */
int  vi_eval_track_grad_f64(vi_model* model, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                            const int32_t* d_rec, const double* d_w, int64_t R, const double* d_C,
                            const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame, double* d_out);
/* Line integrals of the fitted parameter along straight rays that each carry their OWN time (slant TEC between a receiver and a
 * satellite, an occultation link, an optical column): one call for all rays.  d_a, d_b: start and end of the P rays in ECEF
 * metres, planar (3 x P: X of all rays, then Y, then Z); d_rec, d_w, R, d_C select and blend the coefficient rows as in
 * vi_eval_track_f64 (d_w == NULL: nearest mode; the blend is formed on the rows, as get_C does, as written: a NaN in either
 * row of the pair gives NaN at any d_w).  (d_x, d_wq): a quadrature rule of n >= 1 nodes on [-1, 1].
 *   d_out[p] = (s1 - s0) / 2 * |b - a| * sum_i d_wq[i] * f(a + s_i (b - a)),   s_i = s0 + (s1 - s0) (1 + d_x[i]) / 2
 * in the parameter's unit times metres, with [s0, s1] the part of [0, 1] where the segment is inside the hull - ONE interval,
 * the hull being convex: the segment clipped against the F half-spaces hull_eq[f][0..2] . x + hull_eq[f][3] <= hull_tol in
 * fp64, straight from hull_eq (a segment whose two ends are inside keeps [0, 1] exactly) - or [0, 1] with F = 0.
 * d_chord (or NULL): 2 x P doubles, s0 of all rays, then s1; geometry only, written for a ray without a record too.
 * NaN - d_out, and the chord - where the segment does not enter the hull (not s0 < s1) and where an end point is not finite;
 * NaN d_out where d_rec[p] < 0 or a row the ray needs is >= R (R = 0: every ray), and where such a row holds a NaN.  A segment
 * of length zero inside the hull gives 0.  A wave integrates a ray, 64 nodes per pass, and adds the nodes in a fixed order: a
 * ray's bits depend on the ray, its row(s) and the rule, not on the other rays or their order - no sorting is needed.
 * Models and orders as vi_eval_track_f64; the orders of vi_eval_f64's fast kernels run K2l's tiled form (csrc/vi_slant.hip),
 * other orders, VINTERP_EVAL=generic and the RBF model the per-lane forms (correct, not tuned).  fp64 chains.  Asynchronous
 * on the context's stream; timed for vi_eval_kernel_ms like its siblings (tests/test_gpu_slant.py). */
int  vi_eval_slant_f64(vi_model* model, int64_t P, const double* d_a, const double* d_b, const int32_t* d_rec, const double* d_w,
                       int64_t R, const double* d_C, const double* d_hull_eq, int32_t F, double hull_tol, int32_t n,
                       const double* d_x, const double* d_wq, double* d_out, double* d_chord);
/* The ray-integrated basis of P rays that stay where they are (an imager's lines of sight, links to geostationary satellites, a
 * fixed optical column) while the records change: the integral of vi_eval_slant_f64 is linear in the coefficients, so
 *   d_Y[n*P + p] = (s1 - s0) / 2 * |b - a| * sum_i d_wq[i] * basis_n(a + s_i (b - a))
 * is built once - N x P doubles, basis_n in the PUBLIC order and scaling of vi_basis_f64 / vi_eval_basis_f64 (not the prepared
 * order of the evaluation kernels), in metres.  d_Y is a matrix of the kind vi_eval_basis_f64 makes for a grid:
 * vi_eval_resident_f64 with the coefficients as stored gives the line integrals of T timesteps as one product,
 * vi_eval_resident_err_f64 with the covariances as stored their standard errors sqrt(b^T dC b), vi_eval_resident_peak_f64 and
 * vi_reduce_basis_f64 maxima and weighted sums over an axis of the rays; d_Y itself is the linear forward operator of the links.
 * d_a, d_b, d_hull_eq, F, hull_tol, (n, d_x, d_wq) and d_chord (or NULL) exactly as in vi_eval_slant_f64: the same clip, in fp64,
 * straight from the facet list; F = 0 keeps [0, 1].  A ray that does not enter the hull (not s0 < s1) or has a non-finite end
 * point gets the NaN of vi_eval_basis_f64 in ALL N rows (and a NaN chord); a segment of length zero inside the hull a column
 * of zeros.  Kernel K1l (csrc/vi_slant.hip): a wave per ray, 64 nodes per pass, every basis function summed over the lanes
 * through an LDS tile in one fixed order, the passes in pass order, no atomics - a column's bits depend on the ray and the rule,
 * not on P, the other rays or their order.  Models and orders as vi_basis_f64 while the N accumulators of a ray fit a
 * workgroup's LDS (N <= 7000; beyond: VI_ERR_UNSUPPORTED).  Asynchronous on the context's stream; timed for vi_eval_kernel_ms
 * like its siblings (tests/test_gpu_resident_rays.py). */
int  vi_eval_slant_basis_f64(vi_model* model, int64_t P, const double* d_a, const double* d_b, const double* d_hull_eq, int32_t F,
                             double hull_tol, int32_t n, const double* d_x, const double* d_wq, double* d_Y, double* d_chord);
/* Many timesteps on ONE grid (BASELINE configs[3]: a GPU's share of 10 000 timesteps, all on the same 256^3 grid - Estimate.__call__
 * (estimate.py:110-123) once per timestep in the reference, which rebuilds the basis of the grid every time): the basis matrix
 * of the grid is assembled once and kept in HBM, and every batch of timesteps is one matrix product.
 *   vi_eval_basis_f64     d_Y[n*Q + q] = basis_n(q), N x Q doubles (19 GB at N = 144 on 256^3); with hull_eq != NULL the
 *                         entries of a point that fails the hull test (as in vi_eval_f64) are NaN
 *   vi_eval_resident_f64  out[t*Q + q] = sum_n d_Y[n*Q + q] * C[t*N + n]  - NaN outside the hull through the NaN of d_Y,
 *                         NaN for a timestep whose coefficients are NaN (a failed fit), as vi_eval_f64 gives them.
 * Agrees with vi_eval_f64 to rounding (the sum over n is taken in the library's order; tests/test_gpu_eval_resident.py).
 * vi_eval_resident_f64 multiplies ANY matrix of N rows and Q columns laid out like d_Y: with the gradient basis of
 * vi_eval_grad_basis_f64 (below) and 3Q for Q it gives the gradient maps of the T timesteps, out[(t*3 + c)*Q + q].  The
 * matrix-core kernel K2r takes the shapes with Q a multiple of 4, Q >= 256 and d_Y / d_out 32-byte aligned (for the gradient:
 * 3Q >= 256 and the number of points a multiple of 4, which also keeps every component plane 32-byte aligned); other shapes,
 * and VINTERP_EVAL_RESIDENT=blas, go through the library's product. */
int  vi_eval_basis_f64(vi_model* model, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                       const double* d_hull_eq, int32_t F, double hull_tol, double* d_Y);
int  vi_eval_resident_f64(vi_model* model, int64_t Q, int64_t T, const double* d_Y, const double* d_C, double* d_out);
/* Gradient maps of many timesteps on the same resident grid: the gradient is linear in the coefficients, so its basis is kept
 * like d_Y and multiplied by the same call.
 *   d_G[(n*3 + c)*Q + q]: component c of the gradient of basis function n at point q; N x 3Q doubles.
 * c = z, theta, phi (VI_FRAME_MODEL, as vi_grad_basis_f64) or east, north, up (VI_FRAME_ENU: the local geodetic directions,
 * `up` the ellipsoid's normal; the per-point rotation is folded into d_G, so the frame costs nothing per timestep).
 * With hull_eq != NULL every entry of a point that fails the hull test (as in vi_eval_basis_f64) is NaN.  Orders and models as
 * vi_grad_basis_f64; others return VI_ERR_UNSUPPORTED. */
enum { VI_FRAME_MODEL = 0, VI_FRAME_ENU = 1 };
int  vi_eval_grad_basis_f64(vi_model* model, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                            const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame, double* d_G);
/* Standard-error maps of many timesteps on the same resident grid (the `calcerr` output of estimate.py:139-145 for a batch of
 * covariances, e.g. the /Coeffs/dC of a whole fit):
 *   vi_eval_resident_err_f64  out[t*Q + q] = sqrt( sum_i sum_k d_Y[i*Q + q] * d_dC[t*N*N + i*N + k] * d_Y[k*Q + q] )
 * with d_Y from vi_eval_basis_f64 and d_dC the T row-major N x N covariances as stored.  The full matrix is evaluated, never
 * assumed symmetric.  NaN outside the hull through the NaN of d_Y, NaN for every point of a timestep whose covariance holds a
 * NaN (a failed fit), NaN where the form is negative (as np.sqrt gives it, as vi_eval_err_f64 does).  The matrix-core kernel
 * K2e takes N <= 144 with Q even and d_Y / d_out 16-byte aligned; other shapes, and VINTERP_EVAL_RESIDENT=blas, go through
 * the library's product and a row dot, as vi_eval_err_f64 (tests/test_gpu_resident_error.py). */
int  vi_eval_resident_err_f64(vi_model* model, int64_t Q, int64_t T, const double* d_Y, const double* d_dC, double* d_out);
/* The same form at ONE chosen point per column and timestep, without the map: the standard error of a peak at the position
 * vi_eval_resident_peak_f64 (below) found, from its index map as it lies on the device.  The grid is seen as (outer, L, inner)
 * as there, column m = o*inner + i, M = outer*inner columns, and d_idx[t*M + m] = l selects point q = (o*L + l)*inner + i:
 *   vi_eval_resident_err_at_f64  d_out[t*M + m] = sqrt( sum_i sum_k d_Y[i*Q + q] * d_dC[t*N*N + i*N + k] * d_Y[k*Q + q] )
 * First-order, the position taken as given.  NaN where l is outside [0, L) - the -1 of a column without a peak -, and
 * vi_eval_resident_err_f64's NaN cases: a NaN column of d_Y, a NaN anywhere in d_dC[t], a negative form.  An index outside
 * [0, L) is never turned into an address.  T = 0 or M = 0: nothing is written.
 * Kernel K2eg (csrc/vi_eval_resident.hip) takes N <= 144 with any M and any alignment: K2e's launch and arithmetic on M columns,
 * the two points of a lane gathered independently (two 8-byte loads per basis row, 64-bit offsets).  A result has the bits
 * vi_eval_resident_err_f64's K2e gives at that point with that covariance.  Other orders, and VINTERP_EVAL_RESIDENT=blas, gather
 * the chosen columns into the context workspace timestep by timestep and go through the library's product and a row dot.
 * VINTERP_K2E_GROUPS sets the groups of 256 columns per workgroup as for K2e.  Asynchronous on the context's stream; timed for
 * vi_eval_kernel_ms like its siblings (tests/test_gpu_resident_column_error.py). */
int  vi_eval_resident_err_at_f64(vi_model* model, int64_t outer, int64_t L, int64_t inner, int64_t T, const double* d_Y,
                                 const double* d_dC, const int32_t* d_idx, double* d_out);
/* Standard errors where every column has its OWN record (the points of a track, rays at their own times): the covariance is
 * chosen per column of d_Y instead of per map.  d_Y: any N x Q matrix laid out as vi_eval_basis_f64 / vi_eval_slant_basis_f64
 * make it; d_dC: the R row-major N x N covariances as stored, the full matrix, never assumed symmetric; d_rec[q], d_w select and
 * blend the records as in vi_eval_track_f64.  With F(r, q) = sum_i sum_k d_Y[i*Q + q] * d_dC[r*N*N + i*N + k] * d_Y[k*Q + q]:
 *   nearest mode (d_w == NULL):   d_out[q] = sqrt(F(d_rec[q], q))
 *   interpolation (d_w != NULL):  d_out[q] = sqrt((1 - d_w[q]) * F(d_rec[q], q) + d_w[q] * F(d_rec[q] + 1, q)), computed as
 *                                 written, no shortcut at d_w = 0 or 1: get_C's blend dC = (1 - T) dC_i + T dC_(i+1)
 *                                 (estimate.py:578) pushed through the form, which is linear in dC
 * NaN where the column is a NaN column of d_Y, where d_rec[q] < 0, where a row the point needs is >= R (R = 0: every point),
 * where a covariance the point needs holds a NaN anywhere, and where the (blended) form is negative, as np.sqrt gives it.  A NaN
 * covariance reaches only the points that select it; d_dC is never read outside its R matrices.
 * Kernel K2te (csrc/vi_eval_resident.hip) takes the shapes of K2e - N <= 144, Q even, d_Y / d_out 16-byte aligned: a workgroup
 * owns 256 consecutive columns, walks the runs of equal d_rec inside them and stages one covariance per run (two in
 * interpolation mode) for K2e's matrix-core body.  Correct for ANY order of d_rec, but the cost grows with the number of runs:
 * SORT the columns by d_rec - one staging per record and block.  A point's bits depend on its column of d_Y, its record(s) and
 * d_w[q], not on Q, the other points or their order; in nearest mode they are the bits vi_eval_resident_err_f64's K2e gives for
 * that column with that covariance.  Other shapes, N > 144 and VINTERP_EVAL_RESIDENT=blas go run by run through the library's
 * product and a row dot, as vi_eval_resident_err_f64 does map by map; that route reads d_rec back and waits for the stream.
 * Otherwise asynchronous on the context's stream; timed for vi_eval_kernel_ms like its siblings
 * (tests/test_gpu_track_error.py). */
int  vi_eval_records_err_f64(vi_model* model, int64_t Q, const double* d_Y, const int32_t* d_rec, const double* d_w, int64_t R,
                             const double* d_dC, double* d_out);
/* vi_eval_records_err_f64 for points and for rays, the matrix built chunk by chunk in the context workspace (at most 256 MB of
 * it; VINTERP_TRACK_ERR_CHUNK: a smaller chunk, for tests) and never leaving the device:
 *   vi_eval_track_err_f64  the standard error of the fitted parameter at points that each carry their own time - the columns of
 *                          vi_eval_basis_f64 (the same bits, the NaN of a point that fails the hull test included; models and
 *                          orders as that entry), then the form with the covariance of d_rec[q] (and d_w[q]).  What
 *                          vi_eval_err_f64 gives record by record.
 *   vi_eval_slant_err_f64  the standard error sqrt(b^T dC b) of the line integral of vi_eval_slant_f64, in the parameter's unit
 *                          times metres - the columns of vi_eval_slant_basis_f64 (K1l: the same clip and rule, a NaN column
 *                          for a ray that misses the hull or has a non-finite end point, N <= 7000).  Arguments as
 *                          vi_eval_slant_f64 with the covariances d_dC in place of d_C; d_chord (or NULL) as there.
 * NaN cases beyond the matrix's, and the cost of unsorted d_rec, as vi_eval_records_err_f64.  A chunk border inside a run of
 * records changes no bits.  Timed for vi_eval_kernel_ms like their siblings. */
int  vi_eval_track_err_f64(vi_model* model, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                           const int32_t* d_rec, const double* d_w, int64_t R, const double* d_dC,
                           const double* d_hull_eq, int32_t F, double hull_tol, double* d_out);
int  vi_eval_slant_err_f64(vi_model* model, int64_t P, const double* d_a, const double* d_b, const int32_t* d_rec, const double* d_w,
                           int64_t R, const double* d_dC, const double* d_hull_eq, int32_t F, double hull_tol, int32_t n,
                           const double* d_x, const double* d_wq, double* d_out, double* d_chord);
/* The uncertainty of the GRADIENT (the `graderr` the reference's Estimate.__call__ advertises, estimate.py:125-147): the 3 x 3
 * covariance of the gradient at each point from the coefficient covariance, first-order error propagation through the three
 * columns g_0, g_1, g_2 of the gradient basis at the point (components in the frame of the basis),
 *   cov[c][d] = g_c^T 1/2 (dC + dC^T) g_d,
 * its six distinct entries packed in the order (0,0) (1,1) (2,2) (0,1) (0,2) (1,2).  The standard error of component c is
 * sqrt(cov[c][c]) - also vi_eval_resident_err_f64 on d_G with 3Q columns -, that of the gradient along a unit vector u
 * sqrt(u^T cov u).  dC as stored, never assumed symmetric.  All six entries are NaN for a point outside the hull (a NaN column)
 * and for a covariance holding a NaN; a negative diagonal entry of an indefinite dC is returned as it is.
 *   vi_eval_resident_gradcov_f64  d_out[(t*6 + k)*Q + q] for the T row-major N x N covariances d_dC on the resident gradient
 *                         basis d_G of vi_eval_grad_basis_f64 (N x 3 x Q).  The matrix-core kernel K2c takes N <= 144, any Q;
 *                         other orders, and VINTERP_EVAL_RESIDENT=blas, go through the library's product and row dots.
 *   vi_eval_grad_cov_f64  d_out[k*Q + q] for ONE covariance at arbitrary points: the gradient basis of a chunk of points is
 *                         built in the context workspace (hull, F, hull_tol and frame as in vi_eval_grad_basis_f64) and the
 *                         same kernel runs on it.  Models and orders as vi_eval_grad_basis_f64.
 * Asynchronous on the context's stream; timed for vi_eval_kernel_ms like their siblings (tests/test_gpu_resident_gradcov.py). */
int  vi_eval_resident_gradcov_f64(vi_model* model, int64_t Q, int64_t T, const double* d_G, const double* d_dC, double* d_out);
int  vi_eval_grad_cov_f64(vi_model* model, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                          const double* d_dC, const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame, double* d_out);
/* The gradient covariance where every point has its OWN record (the points of a track): the covariance is chosen per column
 * triple of d_G instead of per map, as vi_eval_records_err_f64 does for the scalar form.  d_G: any planar N x 3 x Q gradient
 * basis laid out as vi_eval_grad_basis_f64 makes it; d_dC: the R row-major N x N covariances as stored, never assumed
 * symmetric; d_rec[q], d_w select and blend the records as in vi_eval_track_f64.  With U(r, q)[k] the k-th packed entry of
 * g_c^T 1/2 (dC_r + dC_r^T) g_d at point q (order as above), d_out[k*Q + q], (6, Q):
 *   nearest mode (d_w == NULL):   d_out[k*Q + q] = U(d_rec[q], q)[k]
 *   interpolation (d_w != NULL):  d_out[k*Q + q] = (1 - d_w[q]) * U(d_rec[q], q)[k] + d_w[q] * U(d_rec[q] + 1, q)[k], computed
 *                                 as written, no shortcut at d_w = 0 or 1: get_C's blend of the two covariances pushed through
 *                                 the form, which is linear in dC
 * All six entries are NaN where the column is a NaN column of d_G, where d_rec[q] < 0, where a row the point needs is >= R
 * (R = 0: every point) and where a covariance the point needs holds a NaN anywhere; a negative diagonal entry is returned as it
 * is.  A NaN covariance reaches only the points that select it; d_dC is never read outside its R matrices.
 * Kernel K2tc (csrc/vi_eval_resident.hip) takes N <= 144, any Q, any alignment: a workgroup owns blocks of 256 consecutive
 * points, walks the runs of equal d_rec inside them as K2te does and stages one covariance per run (two in interpolation mode)
 * for K2c's matrix-core body.  Correct for ANY order of d_rec, but the cost grows with the number of runs: SORT the points by
 * d_rec.  A point's bits depend on its three columns of d_G, its record(s) and d_w[q], not on Q, the other points or their
 * order; in nearest mode they are the bits vi_eval_resident_gradcov_f64's K2c gives for that point with that covariance.
 * N > 144 and VINTERP_EVAL_RESIDENT=blas go run by run through the library's product and row dots, as
 * vi_eval_resident_gradcov_f64 does map by map; that route reads d_rec back and waits for the stream.  Otherwise asynchronous on
 * the context's stream.
 *   vi_eval_track_grad_cov_f64  the same at points that each carry their own time: the hull pass once for all points, then chunk
 *                         by chunk the gradient basis in the context workspace as vi_eval_grad_cov_f64 builds it (the same bits;
 *                         hull, F, hull_tol and frame as there; at most 256 MB of it, VINTERP_TRACK_GRADCOV_CHUNK: fewer points
 *                         per chunk, for tests) and the routes above on it.  What vi_eval_grad_cov_f64 gives record by record.
 *                         A chunk border inside a run of records changes no bits.  Models and orders as
 *                         vi_eval_grad_basis_f64, others return VI_ERR_UNSUPPORTED.
 * Both are timed for vi_eval_kernel_ms like their siblings (tests/test_gpu_track_gradcov.py). */
int  vi_eval_records_gradcov_f64(vi_model* model, int64_t Q, const double* d_G, const int32_t* d_rec, const double* d_w, int64_t R,
                                 const double* d_dC, double* d_out);
int  vi_eval_track_grad_cov_f64(vi_model* model, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                const int32_t* d_rec, const double* d_w, int64_t R, const double* d_dC,
                                const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame, double* d_out);
/* SECOND derivatives of the fitted parameter (the reference has none; its grad_basis, sphharmlag.py:148-184, stops at the first):
 * the Hessian of a basis function f = g(r) T(theta') A(phi') in closed form - Legendre's equation gives T'', the azimuth
 * A'' = -m^2 A, the radial part one more generalised-Laguerre recurrence - as a true tensor in 1/m^2 times the function's unit:
 * the second covariant derivatives in the orthonormal frame of the gradient, (r', theta', phi') of the rotated cap
 * (VI_FRAME_MODEL) or east, north, geodetic up (VI_FRAME_ENU: F H F^T with the point's matrix of vi_eval_grad_basis_f64, on the
 * device; entry (2, 2) is then the second derivative along the ellipsoid's normal, the horizontal entries second derivatives
 * along straight tangent lines, not along curves of constant altitude).  Its six distinct entries are packed in the order of
 * the gradient covariance, (0,0) (1,1) (2,2) (0,1) (0,2) (1,2); their first three add up to the Laplacian in either frame.
 *   vi_eval_hess_f64        d_out[k*Q + q] = sum_n hess_basis[q][k][n] * d_C[n], (6, Q) planar, for ONE coefficient vector; the
 *                           6N values of a point are never formed.
 *   vi_eval_hess_basis_f64  d_H[(n*6 + k)*Q + q], N x 6 x Q doubles: the Hessian basis of a resident grid, a matrix of the kind
 *                           vi_eval_grad_basis_f64 makes - vi_eval_resident_f64 with 6Q for Q gives the Hessian maps of T
 *                           timesteps, out[(t*6 + k)*Q + q].
 * Both run the hull pass of vi_eval_grad_cov_f64 first (F = 0: no test) and write NaN into every entry of a point that fails it.
 * Non-finite at the pole of the cap (sin theta' = 0), as the gradient is; next to it the accuracy falls as eps / sin^2 theta'.
 * Models and orders as vi_grad_basis_f64 - sphharmlag within (6, 4), (12, 8) or (2, 12) -, others return VI_ERR_UNSUPPORTED and
 * launch nothing.  Q = 0 is a no-op.  Kernel k_hess_sph (csrc/vi_hess.hip), a lane per point.  Asynchronous on the context's
 * stream; timed for vi_eval_kernel_ms like their siblings (tests/test_gpu_hessian.py). */
int  vi_eval_hess_f64(vi_model* model, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                      const double* d_C, const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame, double* d_out);
int  vi_eval_hess_basis_f64(vi_model* model, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                            const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame, double* d_H);
/* SUB-GRID PEAKS of the fitted parameter along the geodetic normal (the reference has none): for T coefficient rows and Q
 * columns per row the height at which the parameter has its maximum (kind = +1) or minimum (kind = -1) between two bounds, by
 * a safeguarded Newton search on the analytic model itself.  Value f, slope d1 = df/dh = u . grad f and curvature
 * d2 = d2f/dh2 = u^T H u - u the `up` row of the point's east-north-up matrix, so d2 is entry (2, 2) of vi_eval_hess_f64 with
 * VI_FRAME_ENU - come from ONE walk of the chains per iteration.  Point p = t*Q + q (column q of row t) reads d_lat[p],
 * d_lon[p] (degrees), the start d_h0[p] and the bracket d_lo[p] <= d_h0[p] <= d_hi[p] (metres) and the raw coefficient row
 * d_C + t*N, and runs, with s = kind:
 *     h = h0; a = lo; b = hi; done = false; it = 0
 *     loop:  f, d1, d2 at (lat, lon, h)
 *            any of them not finite: status 3, stop
 *            done or it == max_iter: stop
 *            it += 1;  if s*d1 > 0: a = h, else b = h
 *            hn = h - d1/d2 if s*d2 < 0, else NaN;  if not (a < hn < b): hn = (a + b)/2
 *            done = |hn - h| <= tol;  h = hn
 * so that the reported f, d1, d2 belong to the returned h (a converged search makes it + 1 walks).
 *   d_out     (4, T*Q) planar: d_out[k*T*Q + p] = h, f, d1, d2 for k = 0..3
 *   d_status  0  done, s*d2 < 0 and h farther than tol from both d_lo[p] and d_hi[p]: an interior peak
 *             1  done otherwise: the search ran into an end of the bracket or the curvature has the wrong sign
 *             2  not done within max_iter; h is the last iterate (max_iter = 0: the start itself and its values)
 *             3  the four outputs are NaN: the start is outside the hull, an input is not finite or not lo <= h0 <= hi, or the
 *                coefficient row or the chains gave a non-finite f, d1 or d2
 *   d_iter    the iterations made, or NULL
 * The hull pass of vi_eval_grad_cov_f64 runs once on the T*Q start points (F = 0: no test); later iterates are not tested.
 * Kernel k_peak_sph (csrc/vi_peak.hip): a lane per column, the grid (blocks of 256 columns, rows), coefficient reads
 * wave-uniform; a lane that has stopped is frozen, a wave leaves when none of its lanes is searching, a wave without a lane to
 * search leaves before any walk.  The bits of a point depend on its column, its row, kind, max_iter and tol - not on Q, T, the
 * other points or its place among them.  A NaN in a row reaches only that row.
 * Models and orders as vi_grad_basis_f64 - sphharmlag within (6, 4), (12, 8) or (2, 12) -, others return VI_ERR_UNSUPPORTED and
 * launch nothing; kind other than +-1, max_iter < 0, tol not finite or <= 0, a null pointer (d_iter excepted), a negative size
 * or F > 0 without facets return VI_ERR_INVALID.  T = 0 or Q = 0 is a no-op.  Asynchronous on the context's stream; timed for
 * vi_eval_kernel_ms like its siblings (tests/test_gpu_peak.py). */
int  vi_eval_peak_f64(vi_model* model, int64_t T, int64_t Q, const double* d_lat, const double* d_lon, const double* d_h0,
                      const double* d_lo, const double* d_hi, const double* d_C, const double* d_hull_eq, int32_t F,
                      double hull_tol, int32_t kind, int32_t max_iter, double tol, double* d_out, int32_t* d_status,
                      int32_t* d_iter);
/* LEVEL CROSSINGS of the fitted parameter along the geodetic normal (the reference has none): for T coefficient rows and Q
 * columns per row the height between two bounds at which the parameter crosses a given level - the reflection height of a
 * sounding frequency, the half-peak heights of a layer, an isodensity surface -, by a safeguarded Newton search on the analytic
 * model itself.  A root search needs no curvature: value f and slope d1 = df/dh = u . grad f - u the `up` row of the point's
 * east-north-up matrix - come from ONE gradient walk of the chains per iteration, four sums against the ten of
 * vi_eval_peak_f64.  Point p = t*Q + q (column q of row t) reads d_lat[p], d_lon[p] (degrees), the bracket lo = d_ends[p],
 * hi = d_ends[T*Q + p] (metres), the level L = d_level[p] and the raw coefficient row d_C + t*N, and runs
 *     a = lo; b = hi
 *     not finite(lat, lon, a, b, L), not a < b, or an end outside the hull: status 3, stop
 *     fa = f(a) - L, da = d1(a);  fb = f(b) - L, db = d1(b)              (two walks)
 *     fa or fb not finite: status 3, stop
 *     fa == 0: h = a, report f(a), da, status 0, it = 0, stop.   fb == 0: the same at b.
 *     fa and fb of one sign (tested by comparisons, not by their product): status 1, stop
 *     h = a - fa (b - a)/(fb - fa);  if not (a < h < b): h = (a + b)/2;   done = false; it = 0
 *     loop:  f, d1 at (lat, lon, h);  phi = f - L
 *            phi or d1 not finite: status 3, stop
 *            phi == 0 or done or it == max_iter: stop - status 0 if phi == 0 or done, else 2
 *            it += 1;  if (phi > 0) == (fa > 0): a = h, else b = h
 *            hn = h - phi/d1 if d1 != 0, else NaN;  if not (a < hn < b): hn = (a + b)/2
 *            done = |hn - h| <= tol;  h = hn
 * so that the reported f and d1 belong to the returned h (a converged search makes it + 3 walks), and every pass of the loop
 * either stops or adds one to `it`, which max_iter bounds.
 *   d_lat, d_lon  (2, T*Q) planar, the second plane a copy of the first: point T*Q + p is the column of point p again
 *   d_ends    (2, T*Q) planar: plane 0 the lower ends, plane 1 the upper ends
 *   d_out     (3, T*Q) planar: d_out[k*T*Q + p] = h, f, d1 for k = 0..2; all NaN with status 1 and 3, the last iterate with 2
 *   d_status  0  a crossing: phi == 0 exactly, or the last step was at most tol
 *             1  f - L has one sign at both ends: no crossing is bracketed
 *             2  not done within max_iter; h is the last iterate (max_iter = 0: the secant point of the two ends)
 *             3  the outputs are NaN: an end of the bracket is outside the hull, an input is not finite, not lo < hi, or the
 *                coefficient row or the chains gave a non-finite f or d1
 *   d_iter    the iterations made (0 with status 1, and with status 3 before the loop), or NULL
 * The hull pass of vi_eval_grad_cov_f64 runs ONCE on the 2*T*Q points (d_lat, d_lon, d_ends) - both ends of every bracket
 * (F = 0: no test).  Later iterates need no test and there is no "left the hull" status: a column's geodetic normal is a
 * straight line in ECEF and the hull test is an intersection of half-spaces, a convex set, so every point between two points
 * inside is inside.
 * Kernel k_level_sph (csrc/vi_level.hip): a lane per column, the grid (blocks of 256 columns, rows), coefficient reads
 * wave-uniform; a lane that has stopped stores at once and is frozen, a wave leaves when none of its lanes is searching, a wave
 * without a lane to search leaves before any walk.  The bits of a point depend on its column, its row, level, bracket, max_iter
 * and tol - not on Q, T, the other points or its place among them.  A NaN in a row reaches only that row.
 * Models and orders as vi_eval_peak_f64, others return VI_ERR_UNSUPPORTED and launch nothing; max_iter < 0 or > 10000, tol not
 * finite or <= 0, a null pointer (d_iter excepted), a negative size or F > 0 without facets return VI_ERR_INVALID.  T = 0 or
 * Q = 0 is a no-op.  Asynchronous on the context's stream; timed for vi_eval_kernel_ms like its siblings
 * (tests/test_gpu_level.py). */
int  vi_eval_level_f64(vi_model* model, int64_t T, int64_t Q, const double* d_lat, const double* d_lon, const double* d_ends,
                       const double* d_level, const double* d_C, const double* d_hull_eq, int32_t F, double hull_tol,
                       int32_t max_iter, double tol, double* d_out, int32_t* d_status, int32_t* d_iter);
/* PEAKS AND LEVEL CROSSINGS ALONG STRAIGHT RAYS (the reference has none): the two searches above along an oblique line instead
 * of a column's geodetic normal - the profile peak along a radar beam, the point where an oblique sounder's ray meets the plasma
 * frequency, the place where a line of sight crosses an isodensity surface.  P rays, shared by the T coefficient rows: ray q runs
 * from a_q to b_q, d_a and d_b (3, P) planar in ECEF metres (vi_eval_slant_f64's layout); with d = b - a,
 * len = sqrt(dx^2 + dy^2 + dz^2) and u = d / len the point at the distance s metres from a is
 * (fma(s, ux, ax), fma(s, uy, ay), fma(s, uz, az)), evaluated without a geodetic step.  After the walk of the chains u is turned
 * as the model turns a position (Rodrigues, +theta0) and met with the unit vectors r', theta', phi' of the rotated spherical
 * coordinates at the point: w, its components in the orthonormal frame of VI_FRAME_MODEL.  The Hessian of vi_eval_hess_f64 is a
 * tensor in that frame and the direction of a straight line is constant, so
 *     d1 = df/ds = w . grad f      d2 = d2f/ds2 = w^T H w      exactly.
 * Point p = t*P + q (ray q of row t) reads the raw coefficient row d_C + t*N and
 *   vi_eval_ray_peak_f64   the start d_start[p] and the bracket d_lo[p] <= d_start[p] <= d_hi[p] (metres from a), and runs the
 *                          iteration of vi_eval_peak_f64 with s in place of h;
 *                          d_out (4, T*P) planar: s, f, d1, d2.  d_status 0, 1, 2 as there, and
 *                          3  the four outputs are NaN: an input is not finite, len is not positive and finite, not
 *                             lo <= start <= hi, an END of the bracket (the points at lo and at hi) is outside the hull, or the
 *                             coefficient row or the chains gave a non-finite f, d1 or d2
 *   vi_eval_ray_level_f64  the bracket lo = d_ends[p] < hi = d_ends[T*P + p] and the level d_level[p], and runs the iteration
 *                          of vi_eval_level_f64 with s in place of h (the walk at lo, the walk at hi, the secant start,
 *                          safeguarded Newton); d_out (3, T*P) planar: s, f, d1.  d_status 0, 1, 2, 3 as there, 3 also for a
 *                          ray whose len is not positive and finite.
 * The hull: each lane tests the two ends of its own bracket against the F half-spaces d_hull_eq (F x 4 doubles, device memory)
 * with K2l's expression and criterion, fma(nx, X, fma(ny, Y, fma(nz, Z, off))) <= hull_tol; F = 0: no test.  There is no mask
 * pass, no test of a later iterate and no "left the hull" status in either search: the iterates stay between two points inside
 * a convex set.
 * Kernels k_line_peak_sph and k_line_level_sph (csrc/vi_line.hip): a lane per ray, the grid (blocks of 256 rays, rows), the
 * coefficient reads wave-uniform; a lane that has stopped stores at once and is frozen, a wave leaves when none of its lanes is
 * searching, a wave without a lane to search leaves before any walk; more than 65 535 rows go in slices.  The bits of a point
 * depend on its ray, its row, bracket, start or level, kind, max_iter and tol - not on P, T, the other points or its place among
 * them.  A NaN in a row reaches only that row.
 * Models and orders as vi_eval_peak_f64, others return VI_ERR_UNSUPPORTED and launch nothing; kind other than +-1, max_iter < 0
 * or > 10000, tol not finite or <= 0, a null pointer (d_iter excepted), a negative size, P > 2^31 - 1 or F > 0 without facets
 * return VI_ERR_INVALID.  T = 0 or P = 0 is a no-op.  Asynchronous on the context's stream; timed for vi_eval_kernel_ms like
 * their siblings (tests/test_gpu_ray.py). */
int  vi_eval_ray_peak_f64(vi_model* model, int64_t T, int64_t P, const double* d_a, const double* d_b, const double* d_start,
                          const double* d_lo, const double* d_hi, const double* d_C, const double* d_hull_eq, int32_t F,
                          double hull_tol, int32_t kind, int32_t max_iter, double tol, double* d_out, int32_t* d_status,
                          int32_t* d_iter);
int  vi_eval_ray_level_f64(vi_model* model, int64_t T, int64_t P, const double* d_a, const double* d_b, const double* d_ends,
                           const double* d_level, const double* d_C, const double* d_hull_eq, int32_t F, double hull_tol,
                           int32_t max_iter, double tol, double* d_out, int32_t* d_status, int32_t* d_iter);
/* MAXIMA AND MINIMA IN THREE DIMENSIONS (the reference has none): the searches above follow a direction the caller chooses - a
 * column's normal, a line of sight - and give the extremum along it.  This one gives the point itself: for T coefficient rows and
 * P searches per row the point x inside the ball |x - x0| <= radius and inside the hull at which the fitted parameter has its
 * maximum (kind +1) or minimum (-1) - the centre of a polar-cap patch or of a depletion -, its value, gradient and Hessian there
 * (the principal curvatures are the size of the patch).  Search p = t*P + q reads the start d_x0[p], d_x0[T*P + p],
 * d_x0[2*T*P + p] (ECEF metres), d_radius[p] (metres) and the raw coefficient row d_C + t*N.  One walk of the chains from the
 * ECEF point (no geodetic step) gives f, the gradient and the Hessian tensor in the orthonormal frame (r', theta', phi') of
 * VI_FRAME_MODEL; with E the three unit vectors of that frame at the point written in ECEF,
 *     g = E^T g_model      H = E^T H_model E
 * are the plain Cartesian gradient and matrix of second derivatives - the Hessian is a tensor, there are no connection terms -,
 * and Newton's iteration runs in R^3.  With sg = kind, |.| the Euclidean norm and ms = max_step, or radius / 8 where max_step
 * is 0:
 *     x0 or radius not finite, or not radius > 0: status 3, stop
 *     x = x0; have = done = full = false; it = 0; D = ms
 *     loop:  f, g, H at x                                                        (one walk)
 *            ins = x inside every facet (K2l's expression and tolerance, as the rays' ends) and |x - x0| <= radius
 *            f, g or H not finite, or (not have and not ins): status 3, stop
 *            done or it == max_iter: report x, f, g, H;
 *                  status = 2 if not done, else 0 if full and ins and all three pivots of -sg H > 0, else 1;  stop
 *            it += 1;  gn = |g|
 *            have and (not ins or not (sg f >= sg fb or (full and gn < gb))):     reject - backtrack along the same step
 *                  full = false;  |d| <= tol: x = xb, done = true;  else: d = d / 4, D = |d|, x = xb + d;  next pass
 *            have: D = min(2 D, ms)
 *            xb = x; fb = f; gb = gn; have = true
 *            gn == 0: d = 0, n = 0, full = true  (a zero gradient is a step of zero length; nothing is divided by it)
 *            else: solve (-sg H) d = sg g by LDL^T in the fixed order 1, 2, 3 - p1 = a11, l21 = a21/p1, l31 = a31/p1,
 *                  p2 = a22 - l21 a21, t = a32 - l31 a21, l32 = t/p2, p3 = a33 - l31 a31 - l32 t -, every pivot that is not
 *                  > mu = gn / D replaced by mu;  full = no pivot was replaced;  n = |d|;
 *                  n > D: d = d (D / n), n = D, full = false
 *            done = n <= tol;  x = x + d
 * The floored pivots make every step an ascent direction of sg f and bound its length by about D where the curvature has the
 * wrong sign.  A step is accepted by the value, or - a full Newton step - by the gradient norm: close to the extremum the gain
 * 1/2 |H| d^2 falls below the rounding of f and the value alone cannot decide.  A rejected iterate, or one outside the hull or
 * the ball, backtracks towards the best point - a quarter of the step at a time, until a step of at most tol is rejected too -, so
 * that the result lies in the region (a last Newton step of at most tol is not tested) and a search that ends on the boundary
 * ends within tol of a point outside.  Every pass stops the search or adds one to `it`, which max_iter bounds; a converged search makes it + 1 walks.
 *   d_out     (13, T*P) planar: x, y, z, f, g (3), H (6: xx yy zz xy xz yz, the order of vi_eval_hess_f64), all in ECEF; NaN
 *             with status 3, the last iterate's with 1 and 2 (max_iter = 0: the start and its values)
 *   d_status  0  an interior extremum: the last step was an unmodified, unclipped Newton step of at most tol, the result is
 *                inside the region and H there is definite with the sign of the kind
 *             1  converged without one: onto the boundary of the hull or of the ball, or at a point of the wrong curvature
 *             2  not done within max_iter
 *             3  the outputs are NaN: the start is outside the hull or not finite, radius is not finite and positive, or the
 *                coefficient row or the chains gave a non-finite f, g or H
 *   d_iter    the passes that did not stop the search, or NULL
 * Kernel k_extremum_sph (csrc/vi_extremum.hip): a lane per search, the grid (blocks of 256 searches, rows), the coefficient and
 * facet reads wave-uniform; a lane that has stopped stores at once and is frozen, a wave leaves when none of its lanes is
 * searching, a wave without a lane to search leaves before any walk; more than 65 535 rows go in slices.  The hull test of
 * every iterate is in the kernel (F = 0: no test); there is no host pass.  The bits of a search depend on its start, radius,
 * row, kind, max_step, max_iter, tol and the facet list - not on P, T, the other searches or its place among them.  A NaN in a
 * row reaches only that row.
 * Models and orders as vi_eval_peak_f64, others return VI_ERR_UNSUPPORTED and launch nothing; kind other than +-1, max_iter < 0
 * or > 10000, tol not finite or <= 0, max_step not finite or < 0, a null pointer (d_iter excepted), a negative size,
 * P > 2^31 - 1 or F > 0 without facets return VI_ERR_INVALID.  T = 0 or P = 0 is a no-op.  Asynchronous on the context's
 * stream; timed for vi_eval_kernel_ms like its siblings (tests/test_gpu_extremum.py). */
int  vi_eval_extremum_f64(vi_model* model, int64_t T, int64_t P, const double* d_x0, const double* d_radius, const double* d_C,
                          const double* d_hull_eq, int32_t F, double hull_tol, int32_t kind, double max_step, int32_t max_iter,
                          double tol, double* d_out, int32_t* d_status, int32_t* d_iter);
/* Column maps of many timesteps on the same resident grid, without the volume.  The grid is seen as (outer, L, inner), point
 * q = (o*L + l)*inner + i, column m = o*inner + i: any axis of a C-ordered grid, the last one with inner = 1.  What a user of
 * Estimate.__call__ (estimate.py:110-123) takes from a (lat, lon, alt) volume per column: the peak of the parameter along
 * altitude and where it sits, and its vertical integral.
 *   vi_eval_resident_peak_f64  d_val[t*M + m] = max (kind 0) or min (kind 1) over l of the density of vi_eval_resident_f64 at the
 *                         points of column m that are not NaN, the bits of the selected element; d_idx[t*M + m] = the lowest l
 *                         that attains it (+0 and -0 tie, +-inf are ordinary values): np.nanmax / the first np.nanargmax.  A
 *                         column without a number - wholly outside the hull, or a timestep whose coefficients hold a NaN -
 *                         gives (NaN, -1).
 * d_work: vi_eval_resident_peak_work_bytes(model, outer, L, inner, T) bytes, host arithmetic for the path the call will take
 * PROVIDED d_Y is 32-byte aligned and d_work 8-byte aligned (any hipMalloc pointer is): the size is computed from the shape
 * alone, and a call whose shape is K2p's but whose pointers are not (or whose launch would exceed 2^31 - 1 blocks) takes the
 * two-pass path, which needs T x Q doubles or at least Q, and fails with VI_ERR_ARG on a smaller work space.
 * K2p, the matrix-core kernel, takes inner = 1 with L a multiple of 4 and K2r's shapes (Q a multiple of 4, Q >= 256, d_Y 32-byte
 * aligned): K2r's product with a reduction in place of the stores, its work space holds partial results only (12 bytes per
 * timestep and 64-point block or column, twice).  Other shapes, VINTERP_K2P=twopass and VINTERP_EVAL_RESIDENT=blas run
 * vi_eval_resident_f64 into d_work, a slab of T x Q doubles or as many timesteps of it as work_bytes holds (at least one), and
 * a column reduction over it.  Same bits either way, and whatever the cut of T into calls.  Asynchronous on the context's
 * stream; timed for vi_eval_kernel_ms like its siblings.
 *   vi_reduce_basis_f64   d_Yr[n*M + m] = sum_l d_w[l] * d_Y[n*Q + (o*L + l)*inner + i] over the l whose point is not NaN in
 *                         ROW 0 of d_Y (K2r's rule for a point outside the hull), in ascending l; NaN where the column has no
 *                         such point.  The weighted column sum of the density is linear in the coefficients:
 *                         vi_eval_resident_f64(model, M, T, d_Yr, ...) gives sum_l w[l] * density[t][m][l] over the points inside
 *                         the hull at 1/L of the cost of the density product (tests/test_gpu_resident_integrate.py). */
int    vi_eval_resident_peak_f64(vi_model* model, int64_t outer, int64_t L, int64_t inner, int64_t T, const double* d_Y,
                                 const double* d_C, int32_t kind, double* d_val, int32_t* d_idx, void* d_work, size_t work_bytes);
size_t vi_eval_resident_peak_work_bytes(vi_model* model, int64_t outer, int64_t L, int64_t inner, int64_t T);
int    vi_reduce_basis_f64(vi_model* model, int64_t outer, int64_t L, int64_t inner, const double* d_Y, const double* d_w,
                           double* d_Yr);
/* Crossing maps on the same view (outer, L, inner) of a resident grid: d_idx[t*M + m] = the index l of the first (which = 0) or
 * last (which = 1) pair of neighbours (l, l + 1) along the axis of column m whose densities f_l, f_{l+1} of
 * vi_eval_resident_f64 are both numbers and hold the level d_level[t*M + m] between them - direction 1 (up):
 * f_l <= level <= f_{l+1}; 2 (down): f_l >= level >= f_{l+1}; 0: either -, decided by comparisons, never by a product; -1 where
 * the column has no such pair: a NaN level, a timestep whose coefficients hold a NaN, a column outside the hull, L = 1.  The
 * grid bracket vi_eval_level_f64 starts from.  d_work: at least Q doubles; the product of vi_eval_resident_f64 runs into it, a
 * slab of as many timesteps as work_bytes holds (VI_ERR_INVALID below one), then a column kernel over the slab
 * (k_cross_columns, csrc/vi_level.hip): the same map whatever the cut of T into slabs or calls.  VINTERP_EVAL_RESIDENT=blas
 * applies as in vi_eval_resident_f64.  Asynchronous on the context's stream; timed for vi_eval_kernel_ms. */
int    vi_eval_resident_cross_f64(vi_model* model, int64_t outer, int64_t L, int64_t inner, int64_t T, const double* d_Y,
                                  const double* d_C, const double* d_level, int32_t which, int32_t direction, int32_t* d_idx,
                                  void* d_work, size_t work_bytes);
/* Arithmetic of the Legendre degree recurrences inside vi_eval_f64 for this model: 0 = fp64 (default; the reference
 * computes in float64 throughout, sphharmlag.py:118-145), 1 = fp32 chains with everything else in fp64 - the variant
 * BASELINE configs[4] sweeps against the 1e-6 tolerance.  Orders with an fp32 kernel: (MAXL, MAXK) = (6,4), (2,8), (12,8);
 * others return VI_ERR_UNSUPPORTED from vi_eval_f64 while the flag is set. */
int  vi_model_set_eval_precision(vi_model* model, int32_t chain_f32);
/* device time (ms) of the evaluation kernel launches of the last vi_eval_f64 / vi_eval_track_f64 / vi_eval_track_grad_f64 / vi_eval_slant_f64 / vi_eval_slant_basis_f64 / vi_eval_resident_f64 /
 * vi_eval_resident_err_f64 / vi_eval_resident_err_at_f64 / vi_eval_resident_gradcov_f64 / vi_eval_grad_cov_f64 (its last chunk) / vi_eval_hess_f64 / vi_eval_hess_basis_f64 / vi_eval_peak_f64 / vi_eval_level_f64 / vi_eval_ray_peak_f64 / vi_eval_ray_level_f64 / vi_eval_extremum_f64 / vi_eval_records_gradcov_f64 / vi_eval_track_grad_cov_f64 /vi_eval_resident_peak_f64 / vi_eval_resident_cross_f64 call on this context, from HIP events recorded on the context's stream around them (the preparation kernels are excluded).
 * The events are recorded only while vi_ctx_set_eval_timing(ctx, 1) is in force (default: off - the pair costs a 0.2 ms call about 7 us);
 * vi_eval_kernel_ms fails with VI_ERR_ARG while it is off or before a call has been timed. */
int  vi_ctx_set_eval_timing(vi_ctx* ctx, int32_t on);
int  vi_eval_kernel_ms(vi_ctx* ctx, double* ms);
/* device time of the eigen-solve kernel launches (the kernel the fit spends its time in), from one HIP event pair
 * per launch on the context's stream.  enable = 1 starts / resets recording, 0 stops it, -1 only reads; the
 * outputs (each may be NULL) describe the period since the last reset: launches, systems solved, number of
 * launches whose duration is included (the 2048 most recent at most), their summed and maximal duration (ms). */
int  vi_solve_timing(vi_ctx* ctx, int enable, int64_t* launches, int64_t* systems, int64_t* timed,
                     double* total_ms, double* max_ms);
/* Jacobi rounds (one round = one pass of the LDS-resident matrix through the registers) summed over the systems of
 * all launches since vi_solve_timing(enable = 1); read it BEFORE the next vi_solve_timing call with enable >= 0,
 * which resets it.  The unit the LDS roofline of the eigen-solve kernel is priced in (bench.py). */
int  vi_solve_rounds(vi_ctx* ctx, int64_t* rounds);
/* host-pointer form of the same call (what Estimate.__call__ uses): chunked, coordinates up on one stream while densities
 * come down on another; the staging buffers live on the model.  h_out rows have length Q. */
int  vi_eval_f64_host(vi_model* model, int64_t Q, const double* h_lat, const double* h_lon,
                      const double* h_alt, int64_t T, const double* h_C,
                      const double* h_hull_eq, int32_t F, double hull_tol, double* h_out);

/* page-locked host memory: arrays handed to vi_eval_f64_host from it move at the full rate of the link in both directions
 * at once (pageable arrays go through the runtime's own staging) */
int  vi_host_alloc(size_t bytes, void** out);
int  vi_host_free(void* p);

/* ---- fit: replaces Interpolate.eval_C (interpolate.py:432-469) -----------------------------
 * Normal equations for T records sharing one basis matrix (records differ only in W and b;
 * dropped points carry W = 0, b = 0 - algebraically the row removal of interpolate.py:516-520):
 *   AWA[t] = A^T diag(W[t]) A  (interpolate.py:456),  y[t] = A^T (W[t] .* b[t])  (interpolate.py:458)
 * d_At is the N x P basis (ld_n = P layout of vi_basis_f64). */
int  vi_normal_eq_f64(vi_ctx* ctx, int64_t T, int64_t P, int32_t N, const double* d_At,
                      const double* d_W, const double* d_b, double* d_AWA, double* d_y);

/* X[i] = AWA[rec[i]] + alpha[i] * R   for a batch of B (record, alpha) pairs (interpolate.py:460-461);
 * d_rec == NULL means rec[i] = i; d_AWA == NULL accumulates a further penalty term, X[i] += alpha[i] * R. */
int  vi_form_system_f64(vi_ctx* ctx, int64_t B, int32_t N, const double* d_AWA, const int32_t* d_rec,
                        const double* d_alpha, const double* d_R, double* d_X);

/* Minimum-norm solve of the symmetric systems X[i] c = y[rec[i]] with singular values below
 * rcond * sigma_max treated as zero - scipy.linalg.lstsq / LAPACK gelsd at interpolate.py:462
 * (rcond = eps), via a batched symmetric eigendecomposition (sigma_i = |lambda_i|).
 * d_X is destroyed.  Optionally also H = pinv(X) with its own cutoff (interpolate.py:465). */
int  vi_solve_trunc_f64(vi_ctx* ctx, int64_t B, int32_t N, double* d_X, const double* d_y,
                        const int32_t* d_rec, double rcond, double* d_C, int32_t* d_rank,
                        double pinv_rcond, double* d_H /* may be NULL */);

/* chi2[i] = sum_p W[rec[i]][p] (A[p,:] . C[i] - b[rec[i]][p])^2   (interpolate.py:258-259, :569) */
int  vi_chi2_f64(vi_ctx* ctx, int64_t B, int64_t P, int32_t N, const double* d_At, const double* d_C,
                 const int32_t* d_rec, const double* d_W, const double* d_b, double* d_chi2);

/* dC[t] = H[t] AWA[t] H[t]   (interpolate.py:466) */
int  vi_cov_f64(vi_ctx* ctx, int64_t T, int32_t N, const double* d_H, const double* d_AWA, double* d_dC);

/* ---- warm-started regularisation-parameter search ----------------------------------------------
 * Brent's iterates (interpolate.py:214) solve nearly identical systems X(alpha) = AWA[rec] + alpha R.
 * vi_warm_prepare_f64 decomposes X(alpha0[i]) of B records with eigenvectors (returning the solution C
 * at alpha0 like vi_solve_trunc_f64) and stores V, D1 = V^T AWA V, D2 = V^T R V, yt = V^T y per record
 * (slot i); vi_warm_solve_f64 then solves (D1 + alpha D2) c' = yt for B (slot, alpha) pairs with the same
 * truncation rule and returns C = V c'.  Used for the chi^2 search only; the final coefficients of a
 * record always come from vi_solve_trunc_f64 on the untransformed system. */
int  vi_warm_prepare_f64(vi_ctx* ctx, int64_t B, int32_t N, const double* d_AWA, const int32_t* d_rec,
                         const double* d_alpha0, const double* d_R, const double* d_y, double rcond,
                         double* d_C, int32_t* d_rank, double* d_V, double* d_D1, double* d_D2, double* d_yt);
int  vi_warm_solve_f64(vi_ctx* ctx, int64_t B, int32_t N, const double* d_D1, const double* d_D2,
                       const double* d_yt, const double* d_V, const int32_t* d_slot, const double* d_alpha,
                       double rcond, double* d_C, int32_t* d_rank, int32_t* d_sweeps /* may be NULL */);
/* d_sweeps (here and in vi_basis_solve_f64 / vi_warm_rebase_f64): Jacobi sweeps each system took, or the sweep cap + 1
 * (vi_max_sweeps() + 1) when the cap ended the iteration before it converged - such a solution must not decide a sign
 * of chi^2 - nu (interpolate.py:193-203); the caller solves that system again from X(alpha) itself. */
int  vi_max_sweeps(void);

/* The two phases of vi_warm_prepare_f64 as separate calls: vi_decompose_f64 forms and decomposes X(alpha0[i]) of B records
 * (solution to d_C as vi_solve_trunc_f64 gives it) and leaves the rotation logs - vi_rotation_log_bytes(N) per system - and
 * the rounds they hold in buffers of the caller; vi_warm_finish_f64 turns B consecutive logs into V, D1, D2, yt.  A record
 * fitted alone decomposes the middle of every candidate bracket in the launch of its bracket walk and finishes only the one
 * the walk points at. */
size_t vi_rotation_log_bytes(int32_t N);
int  vi_decompose_f64(vi_ctx* ctx, int64_t B, int32_t N, const double* d_AWA, const int32_t* d_rec,
                      const double* d_alpha0, const double* d_R, const double* d_y, double rcond, double* d_C,
                      int32_t* d_rank, void* d_log, int32_t* d_nround);
int  vi_warm_finish_f64(vi_ctx* ctx, int64_t B, int32_t N, const void* d_log, const int32_t* d_nround,
                        const double* d_AWA, const int32_t* d_rec, const double* d_R, const double* d_y,
                        double* d_V, double* d_D1, double* d_D2, double* d_yt);

/* vi_warm_solve_f64 for B (slot, record, alpha) triples that also MOVES each slot's rotated system to alpha: the
 * eigenvectors of the rotated system come out of the rotation log, V <- V Vw, and D1, D2, yt are formed again from the
 * untransformed AWA[rec], R, y[rec].  Brent's late iterates (interpolate.py:214) sit within 1e-3 decades of each other;
 * from a basis that close a warm solve takes 1-3 sweeps instead of 6-13.  A slot may appear once per call.  The first
 * nplain triples are plain warm solves (no re-basing) that share the eigen-solve launch of the others. */
int  vi_warm_rebase_f64(vi_ctx* ctx, int64_t B, int64_t nplain, int32_t N, const double* d_AWA, const double* d_R,
                        const double* d_y, const int32_t* d_rec, const int32_t* d_slot, const double* d_alpha, double rcond,
                        double* d_V, double* d_D1, double* d_D2, double* d_yt, double* d_C, int32_t* d_rank,
                        int32_t* d_sweeps /* may be NULL */);

/* out[t] = the alpha below which alpha R vanishes from AWA[t] + alpha R in floating point (alpha |R_ij| under a quarter
 * of eps |AWA_ij| in every element): the systems of the bracket walk (interpolate.py:186-203) below it are one and the
 * same matrix and are solved once. */
int  vi_reg_floor_f64(vi_ctx* ctx, int64_t T, int32_t N, const double* d_AWA, const double* d_R, double* d_out);

/* The bracket walk (interpolate.py:186-203) in SHARED bases: the walk systems of the records of one geometry resemble each
 * other decade by decade, so they are solved in the eigenbasis of a reference system of the same decade - d_V / d_D2 as
 * vi_warm_prepare_f64 leaves them for a reference record (mean weights of the batch), one slot per decade.  For B
 * (record, basis slot, alpha) triples: (V^T AWA[rec] V + alpha D2) c' = V^T y[rec] with the truncation rule of
 * vi_solve_trunc_f64, C = V c'.  1-4 Jacobi sweeps per system instead of 8-24.  Its chi^2 only decides the signs of the
 * walk (the search asks for the bracket ends, and for values near the target, again from cold solves), so the iteration ends
 * at |a_pq| <= 1e-6 sqrt|a_pp a_qq| (VINTERP_WALK_TOL; csrc/vi_fit.hip walk_tolerance). */
int  vi_basis_solve_f64(vi_ctx* ctx, int64_t B, int32_t N, const double* d_AWA, const double* d_y,
                        const int32_t* d_rec, const int32_t* d_basis, const double* d_alpha, const double* d_V,
                        const double* d_D2, double rcond, double* d_C, int32_t* d_rank, int32_t* d_sweeps /* may be NULL */);

/* One root-finder iterate of ONE record in a single call (single-record latency path): vi_warm_solve_f64 for
 * (slot, alpha) followed by vi_chi2_f64 against record `rec`; the scalars travel as kernel arguments and the only
 * synchronisation is the read-back into h_chi2 (host, THREE doubles: chi^2, an internal word, and in the low 32 bits of
 * the third the sweep count of the solve - cap + 1 when it did not converge).  d_scratch: N + 8 doubles of device memory. */
int  vi_warm_chi2_one_f64(vi_ctx* ctx, int32_t N, int64_t P, const double* d_D1, const double* d_D2,
                          const double* d_yt, const double* d_V, int32_t slot, double alpha, double rcond,
                          const double* d_At, int32_t rec, const double* d_W, const double* d_b,
                          double* d_scratch, double* h_chi2);

/* The whole root-finder phase of the search (scipy.optimize.brentq at interpolate.py:214 on chi^2(10^x) - nu) for ntask
 * records in ONE launch: a workgroup owns a record from its unit bracket [xa, xb] (values fa, fb) to its root, every
 * function value computed in place in the rotated system of the record's slot (vi_warm_prepare_f64) by the code of
 * vi_warm_solve_f64 + vi_chi2_f64, alpha = vi_exp10 (below).  Device arrays of length ntask in and out: root and other end
 * of the final bracket (log10 alpha), iterations / function calls as brentq counts them, status (low byte; bits 8 and up
 * count how often the record's rotated system was re-based) 0 = converged, 2 = a solve
 * was ended by the sweep cap (run that record's iteration on the host), 3 = more than 100 iterations.  Bit for bit the
 * result of the host-driven iteration from the same rotated system.
 * The rotated systems (d_D1, d_D2, d_yt, d_V, by slot) are MOVED next to the root as the host path does
 * (vi_warm_rebase_f64) by the rule in h_rebase (host, 10 doubles: number of thresholds, up to four thresholds in decades
 * between consecutive abscissae, then the late move: after so many requests, within so many decades, enabled; then the early
 * end on a JUMP of chi^2(alpha) - a sign change without a root, where an eigenvalue of X(alpha) crosses the truncation cut,
 * which brentq bisects to 2e-12 in 40-60 values: [8] width in decades of log10 alpha, [9] fraction of nu - the iteration ends
 * once the bracket is narrower than the width while both ends miss nu by more than that fraction; zeros: brentq's own end)
 * - from d_AWA, d_y (by record) and d_R. */
int  vi_brent_warm_f64(vi_ctx* ctx, int64_t ntask, int32_t N, int64_t P, double* d_D1, double* d_D2, double* d_yt,
                       double* d_V, const double* d_AWA, const double* d_R, const double* d_y, const double* h_rebase,
                       const double* d_At, const double* d_W, const double* d_b,
                       const int32_t* d_rec, const int32_t* d_slot, const double* d_xa, const double* d_xb,
                       const double* d_fa, const double* d_fb, const double* d_nu, double rcond, double* d_root,
                       double* d_other, int32_t* d_iters, int32_t* d_funcalls, int32_t* d_status);
/* 1 when vi_brent_warm_f64 serves order N with P data points per record (in-LDS Jacobi range, and the chi^2 partial sums of
 * a record - one per 256 points - fit beside its system in a CU's LDS: P <= ~2 million at N = 144), else 0: drive Brent's
 * iteration from the host then (vi_warm_solve_f64 + vi_chi2_f64), which has no such limit - the reference accepts any P
 * (interpolate.py:214). */
int  vi_brent_warm_supported(int32_t N, int64_t P);
/* The same root-finder phase for ONE record, driven from the host in C (the loop of a record fitted alone: one dependent
 * launch chain per function value, vi_warm_chi2_one_f64, and vi_warm_rebase_f64 + vi_chi2_f64 for the value that moves the
 * rotated system) - brentq's state machine and the re-basing rule are the ones vi_brent_warm_f64 runs on the device, compiled
 * for the host: same requests, same values, same root, without an interpreter between a value and the next request.
 * h_out (host, 6 doubles): root, other end of the final bracket, iterations, function calls, status (0 / 2 / 3 as above),
 * re-basings.  d_scratch: N + 8 doubles of device memory. */
int  vi_brent_host_one_f64(vi_ctx* ctx, int32_t N, int64_t P, double* d_D1, double* d_D2, double* d_yt, double* d_V,
                           const double* d_AWA, const double* d_R, const double* d_y, const double* h_rebase,
                           const double* d_At, const double* d_W, const double* d_b, int32_t rec, int32_t slot,
                           double xa, double xb, double fa, double fb, double nu, double rcond, double* d_scratch,
                           double* h_out);
/* out[i] = 10^x[i] (host arrays) in plain IEEE operations - the routine the device-side iteration uses, so that host and
 * device form alpha = 10^(log10 alpha) identically (interpolate.py:216, :246) */
int  vi_exp10_f64(const double* x, double* out, int64_t n);

/* ---- generalised cross validation: replaces the loop of Interpolate.gcvobjfunct (interpolate.py:332-351) ----
 * For ONE record (d_AWA N x N, d_y N, d_W / d_b P) and one alpha: res[i] = W_p (a_p . C_(-p) - b_p)^2 for the np
 * data points p = pidx[i], where C_(-p) is the regularised truncated solution of the fit that leaves point p
 * out - a rank-one down-date of the normal equations, np eigen-solves in one batch.  Synchronous. */
int  vi_gcv_terms_f64(vi_ctx* ctx, int64_t np, int64_t P, int32_t N, const double* d_At, const int32_t* d_pidx,
                      const double* d_AWA, const double* d_y, const double* d_W, const double* d_b,
                      double alpha, const double* d_R, double rcond, double* d_res);

/* ---- multi-GPU: one broadcast of shared parameters over RCCL (xGMI) -----------------------------
 * Records are independent (interpolate.py:511), so the fit/evaluate path has no collective; the caller shards
 * records across one process per GPU.  The only exchange is this broadcast of the parameters every rank
 * needs (beam geometry, regularisation matrices, hull facets).  Rank 0 obtains a 128-byte id, ships it over
 * its own control channel, then every rank calls vi_rccl_init.  RCCL is dlopen'ed on first use. */
int  vi_rccl_unique_id(char* out128);
int  vi_rccl_init(vi_ctx* ctx, int nranks, int rank, const char* id128);
int  vi_rccl_bcast_f64(vi_ctx* ctx, double* d_buf, int64_t count, int root);
int  vi_rccl_destroy(vi_ctx* ctx);

/* Diagnostic: eigenvalues (unsorted) of B symmetric N x N systems by the in-LDS Jacobi kernel that
 * vi_solve_trunc_f64 uses, and the sweeps each system needed.  d_X is rescaled in place. */
int  vi_eigvals_f64(vi_ctx* ctx, int64_t B, int32_t N, double* d_X, double* d_lam, int32_t* d_sweeps);

/* Stage-test entry of the pre-conditioner of the cold solves (csrc/vi_qr.hip): one column-pivoted Householder QR step
 * X P = Q R of each of B symmetric systems, returned as the similar matrix X1 = Q^T X Q (same eigenvalues; the matrix
 * the Jacobi kernel then iterates on), y1 = Q^T y and the explicit Q (Q[:, j] contiguous).  The solve it serves is
 * scipy.linalg.lstsq at interpolate.py:462; d_X is only read. */
int  vi_qr_similarity_f64(vi_ctx* ctx, int64_t B, int32_t N, const double* d_X, const double* d_y, double* d_X1,
                          double* d_y1, double* d_Q);

/* Stage-test entry of the three kernels of that pre-conditioner, called as the solves call them.  vi_qr_hh_doubles(N) is
 * the packed size of one system's reflector set in doubles (v_0 .. v_{N-1} in the layout of csrc/vi_qr.hip, then the N
 * taus), 0 where the pre-conditioner does not serve N.  vi_qr_stage_f64 factors B systems: d_y is read at row d_rec[i]
 * (row i with d_rec NULL); d_X1 (may be d_X) and d_y1 receive Q^T X Q and Q^T y; d_hh receives the reflector sets
 * hh_stride doubles apart (0: packed; the gaps of a larger stride are not written); d_RPt (B x N x N) receives the rows of
 * R P^T.  Then d_C (B x N, or NULL) becomes Q c by the vector back-transformation and d_V (B x N x N, vector j contiguous,
 * or NULL) becomes Q V by the matrix one.  N outside the served range: VI_ERR_UNSUPPORTED, nothing written. */
int64_t vi_qr_hh_doubles(int32_t N);
int  vi_qr_stage_f64(vi_ctx* ctx, int64_t B, int32_t N, const double* d_X, const double* d_y, const int32_t* d_rec,
                     double* d_X1, double* d_y1, double* d_hh, int64_t hh_stride, double* d_RPt, double* d_C, double* d_V);

/* Stage-test entry of the forming step of vi_basis_solve_f64 (csrc/vi_walk.hip, or the library chain with
 * VINTERP_WALK_FORM=blas; the routine vi_basis_solve_f64 itself calls before its eigen-solve).  For B (record, basis,
 * alpha) triples, with A = AWA[rec[i]], V = V[basis[i]] stored "row k = basis vector k" and D2 = D2[basis[i]]:
 *   X[i] = f (V A V^T + alpha[i] D2), f the power of two that brings max|X[i]| into [1, 2) (1 for a zero or non-finite
 *   system), scl[i] = 1 / f, yt[i] = V y[rec[i]].
 * A system with a NaN or an infinite element (a bad record) comes out as NaN all over the lower block triangle, scl = 1.
 * Of d_X (B x N x N, row-major) only the lower block triangle is defined: element (row, column) with
 * column < 16 (row / 16 + 1).  What lies above it may be written or left as it was.  Same argument checks and the same
 * refusal of an N outside the in-LDS Jacobi range (VI_ERR_UNSUPPORTED, nothing launched) as vi_basis_solve_f64; B = 0
 * is a no-op. */
int  vi_walk_form_f64(vi_ctx* ctx, int64_t B, int32_t N, const double* d_AWA, const int32_t* d_rec, const double* d_V,
                      const double* d_D2, const int32_t* d_basis, const double* d_y, const double* d_alpha, double* d_X,
                      double* d_scl, double* d_yt);

#ifdef __cplusplus
}
#endif
#endif /* VINTERP_H */
