// Internal definitions shared by the translation units of libvinterp.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/vinterp.h"

void vi_set_error(const char* fmt, ...);

#define VI_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            vi_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return VI_ERR_HIP;                                                                \
        }                                                                                     \
    } while (0)

#define VI_ROCBLAS(call)                                                                      \
    do {                                                                                      \
        rocblas_status s_ = (call);                                                           \
        if (s_ != rocblas_status_success) {                                                   \
            vi_set_error("%s:%d: %s -> rocblas status %d", __FILE__, __LINE__, #call, (int)s_); \
            return VI_ERR_ROCBLAS;                                                            \
        }                                                                                     \
    } while (0)

#define VI_ROCSOLVER(call)                                                                      \
    do {                                                                                        \
        rocblas_status s_ = (call);                                                             \
        if (s_ != rocblas_status_success) {                                                     \
            vi_set_error("%s:%d: %s -> rocsolver status %d", __FILE__, __LINE__, #call, (int)s_); \
            return VI_ERR_ROCSOLVER;                                                            \
        }                                                                                       \
    } while (0)

#define VI_REQUIRE(cond, msg)                                  \
    do {                                                       \
        if (!(cond)) {                                         \
            vi_set_error("%s: %s", __func__, msg);             \
            return VI_ERR_INVALID;                             \
        }                                                      \
    } while (0)

struct vi_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    rocblas_handle blas = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t evk0 = nullptr, evk1 = nullptr;   // around the dominant kernel of the last vi_eval_f64 call
    bool evk_valid = false;
    bool evk_enabled = false;                    // vi_ctx_set_eval_timing: the event pair costs ~7 us per call
    // grow-only device workspace for the fit entry points
    void* ws = nullptr;
    size_t ws_bytes = 0;
    int n_cu = 256;
    void* rccl_comm = nullptr;   // ncclComm_t, created by vi_rccl_init
    // opt-in timing of the eigen-solve kernel launches (vi_solve_timing): ring of HIP event pairs on the stream
    static constexpr int NSOLVE_EV = 2048;
    bool solve_timing = false;
    hipEvent_t evs[NSOLVE_EV][2] = {};
    long long solve_launches = 0;      // launches recorded since the last reset
    long long solve_systems = 0;       // systems in those launches
    unsigned long long* d_rounds = nullptr;   // device counter: Jacobi rounds (LDS passes) of the recorded launches
    // downloads that do not hold the stream (vi_d2h_side_mark / vi_d2h_side): a second stream and the event it waits for
    hipStream_t side = nullptr;
    hipEvent_t ev_side = nullptr;
};

int vi_ctx_workspace(vi_ctx* ctx, size_t bytes, void** out);

// records HIP events around the evaluation kernel launches of one evaluation call (see vi_eval_kernel_ms)
struct EvalTimer {
    vi_ctx* c;
    explicit EvalTimer(vi_ctx* ctx) : c(ctx)
    {
        c->evk_valid = c->evk_enabled && hipEventRecord(c->evk0, c->stream) == hipSuccess;
    }
    ~EvalTimer()
    {
        if (c->evk_valid) c->evk_valid = hipEventRecord(c->evk1, c->stream) == hipSuccess;
    }
};

// A grow-only device buffer (p, *have bytes) made to hold `need` bytes.  Growing drains the context's stream before the old
// block is freed: a kernel of an earlier call may still be reading it.
template <class T>
int vi_grow(vi_ctx* ctx, T** p, size_t* have, size_t need)
{
    if (need <= *have) return VI_OK;
    VI_HIP(hipStreamSynchronize(ctx->stream));
    if (*p) VI_HIP(hipFree(*p));
    *p = nullptr;
    *have = 0;
    VI_HIP(hipMalloc((void**)p, need));
    *have = need;
    return VI_OK;
}

// Carves consecutive arrays out of one allocation.  On a null base it only counts: ws_carve below runs a layout on both.
struct ws_carver {
    char* base;
    size_t off = 0;
    template <class T>
    T* take(size_t n, size_t align = 16)
    {
        off = (off + align - 1) / align * align;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

// The context workspace laid out by `layout(ws_carver&)`, which takes every array a call keeps there: run once on a null
// base for the byte count to ask for, then on the workspace for the pointers - the count and the layout cannot disagree.
template <class L>
int ws_carve(vi_ctx* ctx, L&& layout)
{
    ws_carver count{nullptr};
    layout(count);
    void* ws = nullptr;
    const int rc = vi_ctx_workspace(ctx, count.off, &ws);
    if (rc != VI_OK) return rc;
    ws_carver w{static_cast<char*>(ws)};
    layout(w);
    return VI_OK;
}

// A batch in chunks of a workspace budget: the chunk size, budget / per (beyond `whole`: a multiple of it) clamped to [1, B],
// and f(i0, bc) for every chunk in order until one fails
inline int64_t chunk_size(size_t budget, size_t per, int64_t B, int64_t whole = 1)
{
    int64_t Bc = (int64_t)(budget / per);
    if (Bc > whole) Bc -= Bc % whole;
    return Bc < 1 ? 1 : (Bc > B ? B : Bc);
}
template <class F>
int for_chunks(int64_t B, int64_t Bc, F&& f)
{
    for (int64_t i0 = 0; i0 < B; i0 += Bc) {
        const int rc = f(i0, (B - i0) < Bc ? (B - i0) : Bc);
        if (rc != VI_OK) return rc;
    }
    return VI_OK;
}

inline unsigned nblocks(int64_t n, int64_t b) { return (unsigned)((n + b - 1) / b); }

// One kernel launch on a stream and its check.  A launch with dynamic LDS first raises the kernel's limit to the 64 KB of a
// workgroup.  (static: an instantiation is its unit's own, none is among the library's dynamic symbols)
template <class K, class... A>
static int vi_launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... args)
{
    if (lds > 0) VI_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    VI_HIP(hipGetLastError());
    return VI_OK;
}

// T timesteps in tiles of the widths W..., given widest first and ending in 1: launch(integral_constant<int, w>, t0) for the
// first width w that what is left fills and that ok(w) admits (ok(1) must hold), then the launch check, until all are done
template <int... W, class OK, class F>
int for_tiles(int64_t T, OK&& ok, F&& launch)
{
    for (int64_t t = 0; t < T;) {
        const int64_t t0 = t;
        // one term per width, in the order given: a term that launches also advances t and yields true, which ends the fold
        (void)((T - t0 >= W && ok(W) ? (launch(std::integral_constant<int, W>{}, t0), t += W, true) : false) || ...);
        VI_REQUIRE(t > t0, "no admissible tile width");
        VI_HIP(hipGetLastError());
    }
    return VI_OK;
}
template <int... W, class F>
int for_tiles(int64_t T, F&& launch)
{
    return for_tiles<W...>(T, [](int) { return true; }, launch);
}

// f(std::true_type) or f(std::false_type): a run-time flag as the template argument of a kernel
template <class F>
int with_flag(bool b, F&& f)
{
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// The standard error of a point between two records from its two forms f0 = y^T dC_r y, f1 = y^T dC_(r+1) y: get_C's blend
// of the covariances pushed through the form, as written - a NaN in either form gives NaN at any w, a negative blend NaN as
// np.sqrt gives it.  One definition for K2te and the library route of vi_eval_records_err_f64.
__device__ __forceinline__ double vi_err_blend(double w, double f0, double f1) { return (1.0 - w) * f0 + w * f1; }
__device__ __forceinline__ double vi_err_blend_sqrt(double w, double f0, double f1) { return sqrt(vi_err_blend(w, f0, f1)); }
// (vi_err_blend alone: an entry of the gradient covariance of a point between two records, K2tc and the library route of
// vi_eval_records_gradcov_f64 - no root, a negative diagonal entry is returned as it is)

// The VINTERP_* switches.  A switch is read once per process into a function-local `static const` where it is used: the
// language initialises such a variable once and thread-safely, and FitEngine calls in from several host threads.
inline int vi_env_int(const char* name, int dflt)
{
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
inline double vi_env_double(const char* name, double dflt)
{
    const char* e = getenv(name);
    return e ? atof(e) : dflt;
}
inline bool vi_env_is(const char* name, const char* value)
{
    const char* e = getenv(name);
    return e && !strcmp(e, value);
}

// A smaller chunk for a call from the switch `name` (tests: several chunks at a small point count), read at every call: its
// value rounded down to a multiple of `multiple`, taken where it is at least that and below `chunk`
inline int64_t test_chunk(const char* name, int64_t chunk, int multiple)
{
    if (const char* e = getenv(name)) {
        const long long v = atoll(e) / multiple * multiple;
        if (v >= multiple && v < chunk) chunk = v;
    }
    return chunk;
}

// ---- device-side model tables ----------------------------------------------------------------
struct SphGroupDev {
    double v0;
    int nvmax;
    int nterms;
    const int* pick;        // [nvmax+1]
    const double* c;        // [(nvmax+1) x maxl]
    const double* pref;     // [2 x maxl]
    const double* q;        // [2 x maxl x nterms]
    double zzmax;           // the largest (1 - x)/2 with every seed series converged at the end of its table; +inf if nterms == 0
};

struct SphDev {
    int maxk, maxl, N, ngroups;
    double rc, rs, kx, ky, RE;
    const SphGroupDev* groups;
    const double* scale;    // [maxl^2]
    const double* scale1;   // [maxl^2] for degree nu_l + 1 (gradient basis)
    const double* nu;       // [maxl]
};

struct RbfDev {
    int N;
    double inv_eps2;
    const double* centers;  // [N x 3]
};

struct vi_model {
    vi_ctx* ctx = nullptr;
    int kind = 0;
    int N = 0;
    SphDev sph{};
    int nvmax0 = 0;              // nvmax of the first degree group (host copy, for LDS sizing)
    RbfDev rbf{};
    std::vector<void*> allocs;   // device allocations owned by the model
    double* d_coef = nullptr;    // reordered + scaled coefficient staging for vi_eval (grow-only)
    size_t coef_bytes = 0;
    double* d_hull = nullptr;    // internal hull buffer of vi_eval (fp64 facets + fp32 prefilter), grow-only
    size_t hull_bytes = 0;
    unsigned char* d_mask = nullptr;   // inside-hull byte mask of the last vi_eval grid, grow-only
    size_t mask_bytes = 0;
    bool chain_f32 = false;      // evaluate the Legendre degree recurrences in fp32 (vi_model_set_eval_precision)
    // staging of vi_eval_f64_host, grow-only: device coordinates / coefficients / facets / output, second stream + events
    double* h_din = nullptr;     size_t h_din_bytes = 0;
    double* h_dC = nullptr;      size_t h_dC_bytes = 0;
    double* h_dhull = nullptr;   size_t h_dhull_bytes = 0;
    double* h_dout = nullptr;    size_t h_dout_bytes = 0;
    hipStream_t h_stream2 = nullptr;
    hipEvent_t h_ev[2] = {nullptr, nullptr};
    hipEvent_t h_evdown[2] = {nullptr, nullptr};   // "the download out of staging slot s has finished" (h_stream2)
};

// Dynamic LDS of the kernels that run the Legendre chains out of LDS (k_eval_sph_fast, k_track_sph_fast, k_eval_sph_split,
// k_eval_sph_mfma), which all lay it out as [nj x L recurrence table, padded to an even count of doubles | coefficient tile of
// tile_doubles | L ints: the degree each chain segment ends at | 16 bytes spare], nj = nvmax0 + 1
inline size_t chain_lds_bytes(int nj, int L, size_t tile_doubles)
{
    return ((size_t)((nj * L + 1) & ~1) + tile_doubles) * sizeof(double) + L * sizeof(int) + 16;
}
