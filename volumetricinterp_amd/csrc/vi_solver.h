// Host interface of the solver and evaluation translation units of libvinterp.so: every function that one vi_*.hip defines
// and another calls is declared here, once, and this header is included by both sides - a definition that drifts from its
// declaration does not compile.
#pragma once
#include "vi_common.h"

// ---- K3, the in-LDS Jacobi solver (vi_jacobi.hip) ----
size_t vi_jacobi_lds_bytes(int N);
size_t vi_jacobi_log_bytes(int N, int max_sweeps);
bool vi_jacobi_supported(int N);
bool vi_jacobi_use_v2(int N);            // the role-separated kernel serves this order
int vi_jacobi_solve(vi_ctx* c, int64_t B, int N, const double* d_X, const double* d_scl, const double* d_y,
                    const int* d_rec, double rcond, double* d_C, int* d_rank, void* d_log, int max_sweeps,
                    int* d_sweeps, double* d_lam, int lam_raw, int* d_nround, double abs_floor, int64_t log_stride = 0,
                    double conv_tol = 0.0);
bool vi_jacobi_vectors_supported(int N);
int vi_jacobi_vectors(vi_ctx* c, int64_t B, int N, const void* d_log, int max_sweeps, const int* d_nround, double* d_V,
                      int64_t log_stride = 0);

// ---- K3p (vi_qr.hip): X1 = Q^T X Q, y1 = Q^T y by one column-pivoted Householder QR step; back-transformations c <- Q c ----
bool vi_qr_supported(int N);
size_t vi_qr_hh_bytes(int N);
int vi_qr_precond(vi_ctx* c, int64_t B, int N, const double* d_X, const double* d_y, const int* d_rec, double* d_X1,
                  double* d_y1, double* d_hh, double* d_scr, int64_t hh_stride = 0);
int vi_qr_back_vec(vi_ctx* c, int64_t B, int N, const double* d_hh, double* d_C, int64_t hh_stride = 0);
int vi_qr_back_mat(vi_ctx* c, int64_t B, int N, const double* d_hh, double* d_V, int64_t hh_stride = 0);

// ---- K_walk (vi_walk.hip): X = f (V AWA V^T + alpha D2), scl = 1 / f, yt = V y of the bracket walk in shared bases ----
int vi_walk_rotate(vi_ctx* c, int64_t B, int N, const double* d_AWA, const int* d_rec, const double* d_V, const double* d_D2,
                   const int* d_basis, const double* d_y, const double* d_alpha, double* d_X, double* d_scl, double* d_yt);

// ---- vi_fit.hip ----
double vi_floor_warm();                  // absolute rotation floor of the rotated-system solves

// ---- evaluation on the matrix cores / in column groups (vi_eval_mfma.hip, vi_eval_split.hip, vi_eval_resident.hip) ----
int vi_eval_sph_mfma(vi_model* m, int64_t Q, const double* lat, const double* lon, const double* alt, int64_t T,
                     const double* Cp, const unsigned char* hull, int F, double* out, int64_t* done);
int vi_eval_sph_split(vi_model* m, int64_t Q, const double* lat, const double* lon, const double* alt, int64_t T,
                      const double* Cp, const unsigned char* hull, int F, double* out, int* handled);
int vi_eval_resident_mfma(vi_ctx* c, int N, int64_t Q, int64_t T, const double* d_Y, const double* d_C, double* d_out, int* handled);
int vi_eval_resident_err_mfma(vi_ctx* c, int N, int64_t Q, int64_t T, const double* d_Y, const double* d_dC, double* d_out,
                              int* handled);
int vi_eval_resident_err_at_mfma(vi_ctx* c, int N, int64_t outer, int64_t L, int64_t inner, int64_t T, const double* d_Y,
                                 const double* d_dC, const int32_t* d_idx, double* d_out, int* handled);
bool vi_eval_records_err_shape(int N, int64_t Q, const double* d_Y, const double* d_out);
int vi_eval_records_err_mfma(vi_ctx* c, int N, int64_t Q, const double* d_Y, const int32_t* d_rec, const double* d_w, int64_t R,
                             const double* d_dC, double* d_out, int* handled);
bool vi_eval_resident_gradcov_shape(int N);
int vi_eval_resident_gradcov_mfma(vi_ctx* c, int N, int64_t Q, int64_t T, const double* d_G, const double* d_dC, double* d_out,
                                  int64_t ldo, int* handled);
int vi_eval_records_gradcov_mfma(vi_ctx* c, int N, int64_t Q, const double* d_G, const int32_t* d_rec, const double* d_w, int64_t R,
                                 const double* d_dC, double* d_out, int64_t ldo, int* handled);
// peak maps and reduced bases of a resident grid seen as (outer, L, inner) (vi_eval_resident.hip)
bool vi_peak_fused_shape(int N, int64_t outer, int64_t L, int64_t inner);
size_t vi_peak_fused_work_bytes(int64_t outer, int64_t L, int64_t T);
int vi_eval_resident_peak_mfma(vi_ctx* c, int N, int64_t outer, int64_t L, int64_t T, const double* d_Y, const double* d_C, int kind,
                               double* d_val, int32_t* d_idx, void* d_work, size_t work_bytes, int* handled);
int vi_peak_columns(vi_ctx* c, int64_t outer, int64_t L, int64_t inner, int64_t T, int kind, const double* d_in, double* d_val,
                    int32_t* d_idx);
int vi_reduce_basis(vi_ctx* c, int N, int64_t outer, int64_t L, int64_t inner, const double* d_Y, const double* d_w, double* d_Yr);
// crossing maps of a slab of densities (T, outer, L, inner) (vi_level.hip)
int vi_cross_columns(vi_ctx* c, int64_t outer, int64_t L, int64_t inner, int64_t T, int which, int direction, const double* d_in,
                     const double* d_level, int32_t* d_idx);

// ---- what vi_basis.hip and the evaluation units vi_eval.hip (K2), vi_track.hip (K2t, K2tg) and vi_slant.hip (K2l, K1l) share
//      on the host; internal to the library, not among its dynamic symbols ----
#define VI_INTERNAL __attribute__((visibility("hidden")))
VI_INTERNAL int prepare_call(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,      // vi_basis.hip
                             const double* d_hull_eq, int32_t F, double hull_tol, int64_t rows, const double* d_C);
VI_INTERNAL int grad_model_check(const vi_model* m, const char* who);
VI_INTERNAL int launch_grad_resident(vi_model* m, const char* who, int64_t Q, const double* d_lat, const double* d_lon,
                                     const double* d_alt, const unsigned char* d_mask, int32_t frame, double* d_G);
VI_INTERNAL int mask_basis(vi_model* m, int64_t Q, const unsigned char* d_mask, double* d_Y);
struct GradcovChunks { int64_t chunk; double *G, *work; };
VI_INTERNAL int gradcov_setup(vi_model* m, const char* chunk_env, bool records, int64_t Q, const double* d_lat,
                              const double* d_lon, const double* d_alt, const double* d_hull_eq, int32_t F, double hull_tol,
                              GradcovChunks* k);
VI_INTERNAL bool use_fast_eval();                                                                                        // vi_eval.hip
VI_INTERNAL bool fast_eval_fits(const vi_model* m, int TT);

// ---- forms y^T dC y and g_c^T dC g_d on matrices already built (vi_resident.hip), for the entries of vi_basis.hip, vi_track.hip
//      and vi_slant.hip that build the matrix of a chunk themselves; `components`: 1 (a basis column per point) or 3 (a
//      gradient basis) ----
int64_t vi_forms_chunk(int N, int components);                            // points per chunk of the library route, unclipped
size_t vi_forms_work_doubles(int N, int components, int64_t chunk);       // work space of the two records routines below
VI_INTERNAL int64_t track_err_chunk(int N, int64_t Q);                    // chunk and workspace of the track and ray error entries
VI_INTERNAL int track_err_workspace(vi_model* m, int64_t Q, int64_t chunk, const double* d_out, size_t extra, double** Y,
                                    double** X, double** work);
int vi_forms_tile(vi_ctx* c, int N, int64_t P, const double* A, const double* d_dC, double* B, double* d_out);
int vi_records_err(vi_model* m, int64_t Q, const double* d_Y, const int32_t* d_rec, const double* d_w, int64_t R,
                   const double* d_dC, double* d_out, double* work);
int vi_records_gradcov(vi_model* m, int64_t Q, const double* d_G, const int32_t* d_rec, const double* d_w, int64_t R,
                       const double* d_dC, double* d_out, int64_t ldo, double* work);
int vi_resident_gradcov(vi_model* m, int64_t Q, int64_t T, const double* d_G, const double* d_dC, double* d_out, int64_t ldo,
                        double* AB);
