// K2l and K1l for gfx950: line integrals along straight rays, every ray at its own time, and the ray-integrated basis - a wave
// per ray, a lane per node of the caller's rule.  K2l: the tiled kernel at the orders of the fast list (k_slant_sph_fast), the
// per-lane kernels for every other order and the RBF model (k_slant_sph, k_slant_rbf); K1l: k_slant_basis_sph and
// k_slant_basis_rbf.  Entries vi_eval_slant_f64, vi_eval_slant_basis_f64 and vi_eval_slant_err_f64, the last of which hands
// K1l's matrix of a chunk of rays to the records routine of vi_resident.hip.
#include "vi_chain_device.h"
#include "vi_eval_host.h"

namespace {

// ---------------------------------------------------------------------------------------------
// K2l: line integrals along straight rays, every ray at its own time (vi_eval_slant_f64).  Ray p runs from a_p to b_p (ECEF);
// the part of it inside the hull is ONE interval [s0, s1] of the segment parameter (the hull is convex, its facets half-spaces),
// and the integral is the caller's rule on [-1, 1] mapped onto that interval:
//   out[p] = (s1 - s0) / 2 * |b - a| * sum_i wq[i] * f(a + s_i (b - a)),   s_i = s0 + (s1 - s0) (1 + x[i]) / 2.
// The unit is a WAVE per ray.  The model coordinates are functions of ECEF only (sph_geom_ecef), so the nodes need no geodetic
// step, and every node of a ray shares the ray's time: the wave needs one coefficient row - in interpolation mode the blend
// (1 - w) Cp[r] + w Cp[r + 1] of two prepared rows, the preparation being linear - and no window.

constexpr int SLANT_WAVES = 4;      // rays (waves) of a workgroup at most; they share the recurrence table of the fast kernel

// a value that is the same in every lane of the wave, moved to scalar registers
__device__ __forceinline__ double wave_uniform(double v)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// the wave of the workgroup this thread belongs to, as a scalar: what is indexed with it is loaded and kept on the scalar path
__device__ __forceinline__ int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// What a wave knows about its ray after the prologue: every field is the same in all 64 lanes.
struct SlantRay {
    double ax, ay, az, dx, dy, dz;  // a and b - a
    double s0, s1;                  // the part of the segment inside the hull
    double len;                     // |b - a|
    int r;                          // the ray's row
    bool live;                      // to be integrated: a ray of the launch that enters the hull and whose row(s) exist
};

// The prologue of every K2l kernel.  Clips the segment against the F half-spaces n_f . x + d_f <= tol straight from the caller's
// list in fp64, the lanes striding over the facets: with the plane distances ga, gb of the two ends, a facet that has both ends
// inside does not bound the segment, one with both ends outside (a segment parallel to it and outside among them) is missed by
// the whole segment, the others bound s from below at (ga - tol) / (ga - gb) or from above at (tol - ga) / (gb - ga); max / min
// butterflies make [s0, s1] of the lanes' bounds.  A segment with both ends inside the hull keeps [0, 1] exactly.  A miss
// (not s0 < s1) and non-finite end points give a NaN chord.  Writes the chord - geometry only: a ray without a record has one.
// slant_clip is the geometry alone (K1l has no records): live = a ray of the launch that enters the hull, r = 0.
__device__ __forceinline__ SlantRay slant_clip(int64_t p, int64_t P, const double* __restrict__ a, const double* __restrict__ b,
                                               const double* __restrict__ eq, int F, double tol, double* __restrict__ chord)
{
    const int lane = threadIdx.x & 63;
    const int64_t pc = p < P ? p : P - 1;
    SlantRay y;
    y.ax = a[pc];
    y.ay = a[P + pc];
    y.az = a[2 * P + pc];
    const double bx = b[pc], by = b[P + pc], bz = b[2 * P + pc];
    y.dx = bx - y.ax;
    y.dy = by - y.ay;
    y.dz = bz - y.az;
    y.len = sqrt(y.dx * y.dx + y.dy * y.dy + y.dz * y.dz);
    double lo = 0.0, hi = 1.0;
    bool miss = !(fabs(y.ax) + fabs(y.ay) + fabs(y.az) + fabs(bx) + fabs(by) + fabs(bz) < __builtin_inf());
    for (int f = lane; f < F; f += 64) {
        const double nx = eq[4 * f], ny = eq[4 * f + 1], nz = eq[4 * f + 2], off = eq[4 * f + 3];
        const double ga = fma(nx, y.ax, fma(ny, y.ay, fma(nz, y.az, off)));
        const double gb = fma(nx, bx, fma(ny, by, fma(nz, bz, off)));
        const bool ina = ga <= tol, inb = gb <= tol;
        if (!ina && !inb) miss = true;
        else if (!ina) lo = fmax(lo, (ga - tol) / (ga - gb));
        else if (!inb) hi = fmin(hi, (tol - ga) / (gb - ga));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmax(lo, __shfl_xor(lo, o, 64));
        hi = fmin(hi, __shfl_xor(hi, o, 64));
    }
    lo = wave_uniform(lo);
    hi = wave_uniform(hi);
    miss = __any(miss) || !(lo < hi);
    y.s0 = miss ? __builtin_nan("") : lo;
    y.s1 = miss ? __builtin_nan("") : hi;
    if (chord && p < P && lane == 0) {
        chord[p] = y.s0;
        chord[P + p] = y.s1;
    }
    y.r = 0;
    y.live = p < P && !miss;
    return y;
}

__device__ __forceinline__ SlantRay slant_ray(int64_t p, int64_t P, const double* __restrict__ a, const double* __restrict__ b,
                                              const int* __restrict__ rec, int R, int pair, const double* __restrict__ eq, int F,
                                              double tol, double* __restrict__ chord)
{
    SlantRay y = slant_clip(p, P, a, b, eq, F, tol, chord);
    y.r = rec[p < P ? p : P - 1];
    y.live = y.live && y.r >= 0 && y.r <= R - 1 - pair;
    return y;
}

// node i of the rule on the ray: the ECEF point, and the weight of the node in metres
__device__ __forceinline__ void slant_node(const SlantRay& y, double xi, double& X, double& Y, double& Z)
{
    const double s = y.s0 + (y.s1 - y.s0) * (0.5 * (1.0 + xi));
    X = fma(s, y.dx, y.ax);
    Y = fma(s, y.dy, y.ay);
    Z = fma(s, y.dz, y.az);
}

// the epilogue: the lanes' sums added in one fixed order (a butterfly: every lane ends with the same bits), scaled to metres
__device__ __forceinline__ double slant_sum(const SlantRay& y, double acc)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    return 0.5 * (y.s1 - y.s0) * y.len * acc;
}

// The passes of a wave over the n nodes of the rule, the one copy every K2l and K1l kernel runs: lane i of pass k takes node
// 64 k + i and hands body(X, Y, Z, w, on) the node's ECEF point and its weight; the lanes past n run node 0 again with
// on = false and must add nothing.  FENCE: nothing is carried in registers from pass to pass (k_slant_sph_fast has the why).
template <bool FENCE = false, class Body>
__device__ __forceinline__ void slant_nodes(const SlantRay& y, int n, const double* __restrict__ xq, const double* __restrict__ wq,
                                            Body&& body)
{
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += 64) {
        if (FENCE) asm volatile("" ::: "memory");
        const int i = i0 + lane;
        const bool on = i < n;
        double X, Y, Z;
        slant_node(y, xq[on ? i : 0], X, Y, Z);
        body(X, Y, Z, wq[on ? i : 0], on);
    }
}

// What every K2l kernel does with its ray after the prologue: NaN for a dead ray, whose wave leaves; else out[p] = the integral
// of value(X, Y, Z), the density at a node.
template <bool FENCE = false, class Value>
__device__ __forceinline__ void slant_integral(const SlantRay& y, int64_t p, int64_t P, int n, const double* __restrict__ xq,
                                               const double* __restrict__ wq, double* __restrict__ out, Value&& value)
{
    const int lane = threadIdx.x & 63;
    if (!y.live) {
        if (p < P && lane == 0) out[p] = __builtin_nan("");
        return;
    }
    double acc = 0.0;
    slant_nodes<FENCE>(y, n, xq, wq, [&](double X, double Y, double Z, double w, bool on) {
        const double term = w * value(X, Y, Z);
        acc += on ? term : 0.0;
    });
    const double val = slant_sum(y, acc);
    if (lane == 0) out[p] = val;
}

// The orders of the fast list.  A workgroup is `blockDim.x / 64` rays (SLANT_WAVES unless the LDS holds fewer rows beside the
// table): the recurrence table is staged once for all of them, as k_eval_sph_fast stages it for 256 points, and each wave stages
// its own row - blended while staging, as written: never a product that would drop a NaN.  ONE barrier, which every wave meets:
// a dead ray's wave (no record, a miss, rows past R - 1, past the end of the launch) stages zeros instead of a row it must not
// read, and leaves after the barrier without chain work.  Then ceil(n / 64) passes: lane i of pass k takes node 64 k + i and
// runs the chains of k_eval_sph_fast at TT = 1 on it; the lanes past n run node 0 again and add nothing.  No atomics: a ray's
// bits depend on the ray, its row(s) and the rule alone.
template <int L, int K, bool INTERP>
__global__ __launch_bounds__(SLANT_WAVES * 64) void k_slant_sph_fast(SphDev M, int64_t P, const double* __restrict__ a,
                                                                     const double* __restrict__ b, const int* __restrict__ rec,
                                                                     const double* __restrict__ wgt, int R,
                                                                     const double* __restrict__ Cp, const double* __restrict__ eq,
                                                                     int F, double tol, int n, const double* __restrict__ xq,
                                                                     const double* __restrict__ wq, double* __restrict__ out,
                                                                     double* __restrict__ chord)
{
    constexpr int NB = L * L * K;
    extern __shared__ __align__(16) double sh[];
    const int lane = threadIdx.x & 63, wave = wave_index(), waves = blockDim.x >> 6;
    const int64_t p = (int64_t)blockIdx.x * waves + wave;
    const SlantRay y = slant_ray(p, P, a, b, rec, R, INTERP ? 1 : 0, eq, F, tol, chord);
    const SphGroupDev G = M.groups[0];
    const int nj = G.nvmax + 1;
    double* shc = sh;                                           // [nj][L] recurrence table
    double* shC = sh + ((nj * L + 1) & ~1) + wave * NB;         // [waves][NB]: the wave's row
    int* nvl = reinterpret_cast<int*>(sh + ((nj * L + 1) & ~1) + waves * NB);      // [L]
    stage_chain_table(G, nj, L, shc, nvl, blockDim.x);
    if (y.live) {
        const double* __restrict__ row = Cp + (int64_t)y.r * NB;
        if (INTERP) {
            const double w = wgt[p];
            for (int i = lane; i < NB; i += 64) shC[i] = (1.0 - w) * row[i] + w * row[NB + i];
        } else {
            for (int i = lane; i < NB; i += 64) shC[i] = row[i];
        }
    } else {
        for (int i = lane; i < NB; i += 64) shC[i] = 0.0;
    }
    __syncthreads();                                            // the only barrier: every wave of the workgroup is here
    // a pass reads the table and the row as the one-pass kernel does: nothing is carried in registers from pass to pass, the
    // passes are fenced (left to hoist the loop-invariant LDS and table reads, the compiler spends 50 VGPRs - a wave per SIMD
    // or two - on them)
    slant_integral<true>(y, p, P, n, xq, wq, out, [&](double X, double Y, double Z) {
        const Geom g = sph_geom_ecef(M, X, Y, Z);
        FastEval<L, K, 1> E;
        E.shC = shC;
        fast_chains<L, K, 1, double>(E, G, g, shc, nvl, nj);
        return exp(-0.5 * g.z) * E.acc[0];
    });
}

// The frame of the two per-lane kernels, of either model M: rows(Cr, X, Y, Z, v) gives the model's value at the node with the
// ray's row Cr, v[0], and with INTERP that with the row after it, v[1].  The ray's weight and row are taken inside the passes,
// which a dead ray does not reach: its row does not exist and it may lie past the end of the launch.
template <bool INTERP, class Dev, class Rows>
__device__ __forceinline__ void slant_per_lane(const Dev& M, int64_t P, const double* __restrict__ a, const double* __restrict__ b,
                                               const int* __restrict__ rec, const double* __restrict__ wgt, int R,
                                               const double* __restrict__ C, const double* __restrict__ eq, int F, double tol, int n,
                                               const double* __restrict__ xq, const double* __restrict__ wq,
                                               double* __restrict__ out, double* __restrict__ chord, Rows&& rows)
{
    const int64_t p = (int64_t)blockIdx.x * (BLOCK / 64) + wave_index();
    const SlantRay y = slant_ray(p, P, a, b, rec, R, INTERP ? 1 : 0, eq, F, tol, chord);
    slant_integral(y, p, P, n, xq, wq, out, [&](double X, double Y, double Z) {
        const double w = INTERP ? wgt[p] : 0.0;
        double v[2];
        rows(C + (int64_t)y.r * M.N, X, Y, Z, v);
        return INTERP ? (1.0 - w) * v[0] + w * v[1] : v[0];
    });
}

// The per-lane form for the orders without a fast kernel (and VINTERP_EVAL=generic): the same wave per ray, the generic sink
// reading the ray's prepared row, or its two rows, from global memory (wave-uniform); in interpolation mode the two densities
// of a node are blended.  No LDS, no barrier: a dead ray's wave leaves at once.  Correct, not tuned.
template <int LCAP, int KCAP, bool INTERP>
__global__ __launch_bounds__(BLOCK) void k_slant_sph(SphDev M, int64_t P, const double* __restrict__ a, const double* __restrict__ b,
                                                     const int* __restrict__ rec, const double* __restrict__ wgt, int R,
                                                     const double* __restrict__ Cp, const double* __restrict__ eq, int F, double tol,
                                                     int n, const double* __restrict__ xq, const double* __restrict__ wq,
                                                     double* __restrict__ out, double* __restrict__ chord)
{
    slant_per_lane<INTERP>(M, P, a, b, rec, wgt, R, Cp, eq, F, tol, n, xq, wq, out, chord,
                           [&](const double* __restrict__ Cr, double X, double Y, double Z, double* v) {
                               eval_point<LCAP, KCAP, INTERP ? 2 : 1>(M, sph_geom_ecef(M, X, Y, Z), Cr, v);
                           });
}

// K2l for the RBF model: a wave per ray, a lane per node, the ray's coefficient row(s) from global memory
template <bool INTERP>
__global__ __launch_bounds__(BLOCK) void k_slant_rbf(RbfDev M, int64_t P, const double* __restrict__ a, const double* __restrict__ b,
                                                     const int* __restrict__ rec, const double* __restrict__ wgt, int R,
                                                     const double* __restrict__ C, const double* __restrict__ eq, int F, double tol,
                                                     int n, const double* __restrict__ xq, const double* __restrict__ wq,
                                                     double* __restrict__ out, double* __restrict__ chord)
{
    slant_per_lane<INTERP>(M, P, a, b, rec, wgt, R, C, eq, F, tol, n, xq, wq, out, chord,
                           [&](const double* __restrict__ Cr, double X, double Y, double Z, double* v) {
                               rbf_rows<INTERP>(M, Cr, X, Y, Z, v[0], v[1]);
                           });
}

// ---------------------------------------------------------------------------------------------
// K1l: the ray-integrated basis (vi_eval_slant_basis_f64).  The line integral is linear in the coefficients, so for rays that
// stay where they are the integrated basis functions are built once,
//   Y[n*P + p] = (s1 - s0) / 2 * |b - a| * sum_i wq[i] * basis_n(a + s_i (b - a)),
// N x P doubles in the public order of vi_basis_f64 - a matrix of the kind vi_eval_basis_f64 makes for a grid, which K2r, K2e,
// K2p and vi_reduce_basis_f64 take as it is.  K2l's structure: a wave per ray, slant_clip, a lane per node, ceil(n / 64) passes.
// New is the sum across the lanes of EVERY basis function instead of one density.  N accumulators per lane would be 288 VGPRs
// at N = 144, and a butterfly per value is 12 cross-lane moves for one number; the values go through an LDS tile instead:
//   - the sink writes a group of TR values (TR = 8 or 16: both parities of one (l, m) at up to 8 k) as TR rows of the wave's tile
//     [TR][64 + 1], lane i into column i: 64 consecutive doubles per row, no bank conflict;
//   - rayb_sum adds the columns: lane (part, r) = (lane / TR, lane % TR) adds the TR columns part * TR ... of row r in ascending
//     order (the row pitch of 65 doubles puts the 32 lanes of a half wave on 32 different bank pairs), 64 / TR - 1 butterfly
//     steps add the parts, and lane (0, r) adds the row's sum to the ray's accumulator of that basis function.
// All 64 lanes work in both halves, a value costs one LDS write and one LDS read, and the order of the additions is fixed: the
// columns of a part ascending, the parts as a butterfly, the passes in pass order - no atomics; a column's bits depend on the ray
// and the rule alone.  The accumulators are LDS too: [N][waves] doubles, ray-minor, so that after the one barrier the workgroup
// stores N pieces of `waves` neighbouring columns (32 bytes at four rays) instead of N x waves single doubles at stride P.
// A dead ray (a miss, a non-finite end point) runs no chain: its wave fills its accumulators with the NaN of vi_eval_basis_f64
// and waits at the barrier.  The tile is touched by its own wave only: LDS operations of a wave complete in order, so a fence
// at wavefront scope - which keeps the compiler from moving them - is all the reads after the writes need.
constexpr int RAYB_LD = 65;         // doubles per tile row: the 64 lanes and one of padding

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the column sums of the wave's tile: acc[row(r) * ld] += sum_c tile[r][c] for the rows with row(r) >= 0
template <int TR, class RowFn>
__device__ __forceinline__ void rayb_sum(double* tile, double* acc, int ld, RowFn&& row)
{
    static_assert(TR == 8 || TR == 16 || TR == 32 || TR == 64, "a part is TR columns and 64 / TR parts make a row");
    const int lane = threadIdx.x & 63, r = lane & (TR - 1), part = lane / TR;
    wave_lds_sync();
    const double* src = tile + r * RAYB_LD + part * TR;
    double s = src[0];
#pragma unroll
    for (int c = 1; c < TR; ++c) s += src[c];
#pragma unroll
    for (int o = TR; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
    const int n = row(r);
    if (part == 0 && n >= 0) acc[(size_t)n * ld] += s;
    wave_lds_sync();                // the tile is free again
}

// the sink of sph_point: BasisSink's values, weighted with the node's weight (0 in a lane past the rule), summed over the wave
template <int KCAP>
struct RayBasisSink {
    static constexpr int KG = KCAP < 8 ? KCAP : 8, TR = 2 * KG;
    double* tile;                   // the wave's [TR][RAYB_LD]
    double* acc;                    // the ray's accumulators, acc[n * ld]
    int ld, maxk, L2;
    const double* __restrict__ scale;
    double ELk[KCAP];               // exp(-z / 2) L_k(z), 0 from maxk on
    double wgt;
    template <int LCAP>
    __device__ __forceinline__ void consume(int l, const double* cur, const double* cm, const double* sm)
    {
        const int lane = threadIdx.x & 63;
        const int r0 = l * (l + 1);
#pragma unroll
        for (int m = 0; m < LCAP; ++m) {
            if (m <= l) {
                const double fp = scale[r0 + m] * cm[m] * cur[m];
                const double fm = scale[r0 - m] * sm[m] * cur[m];
#pragma unroll
                for (int k0 = 0; k0 < KCAP; k0 += KG) {
                    if (k0 < maxk) {
#pragma unroll
                        for (int k = 0; k < KG; ++k) {
                            tile[(2 * k) * RAYB_LD + lane] = wgt * (ELk[k0 + k] * fp);
                            tile[(2 * k + 1) * RAYB_LD + lane] = wgt * (ELk[k0 + k] * fm);
                        }
                        // row 2 k + 1 of m = 0 (sin 0) and the rows from maxk on are no basis function
                        rayb_sum<TR>(tile, acc, ld, [&](int r) {
                            const int k = k0 + (r >> 1);
                            const bool minus = (r & 1) != 0;
                            return (k < maxk && !(minus && m == 0)) ? k * L2 + r0 + (minus ? -m : m) : -1;
                        });
                    }
                }
            }
        }
    }
};

// LDS of a K1l workgroup: the accumulators and a tile per wave
__host__ __device__ constexpr size_t rayb_lds_bytes(int N, int waves, int TR)
{
    return ((size_t)N * waves + (size_t)waves * TR * RAYB_LD) * sizeof(double);
}

// after the passes: the ray's accumulators scaled to metres, or NaN for a dead ray; then, every wave of the workgroup through
// the one barrier, the stores - thread i takes accumulator i: `waves` neighbouring columns of a row are neighbouring threads
__device__ __forceinline__ void rayb_finish(const SlantRay& y, double* sh, int N, int waves, int wave, int64_t P,
                                            double* __restrict__ Yo)
{
    const int lane = threadIdx.x & 63;
    double* acc = sh + wave;
    if (y.live) {
        const double c = 0.5 * (y.s1 - y.s0) * y.len;
        wave_lds_sync();
        for (int i = lane; i < N; i += 64) acc[(size_t)i * waves] = c * acc[(size_t)i * waves];
    } else {
        for (int i = lane; i < N; i += 64) acc[(size_t)i * waves] = __builtin_nan("");
    }
    __syncthreads();                // the only barrier: every wave of the workgroup is here
    const int64_t p0 = (int64_t)blockIdx.x * waves;
    for (int i = threadIdx.x; i < N * waves; i += blockDim.x) {
        const int n = i / waves, w = i - n * waves;
        if (p0 + w < P) Yo[(int64_t)n * P + p0 + w] = sh[i];
    }
}

template <int LCAP, int KCAP>
__global__ __launch_bounds__(SLANT_WAVES * 64) void k_slant_basis_sph(SphDev M, int64_t P, const double* __restrict__ a,
                                                                      const double* __restrict__ b, const double* __restrict__ eq,
                                                                      int F, double tol, int n, const double* __restrict__ xq,
                                                                      const double* __restrict__ wq, double* __restrict__ Yo,
                                                                      double* __restrict__ chord)
{
    using Sink = RayBasisSink<KCAP>;
    extern __shared__ __align__(16) double sh[];
    const int lane = threadIdx.x & 63, wave = wave_index(), waves = blockDim.x >> 6;
    const int64_t p = (int64_t)blockIdx.x * waves + wave;
    const SlantRay y = slant_clip(p, P, a, b, eq, F, tol, chord);
    const int N = M.N;
    if (y.live) {
        Sink sink;
        sink.tile = sh + (size_t)N * waves + (size_t)wave * Sink::TR * RAYB_LD;
        sink.acc = sh + wave;
        sink.ld = waves;
        sink.maxk = M.maxk;
        sink.L2 = M.maxl * M.maxl;
        sink.scale = M.scale;
        for (int i = lane; i < N; i += 64) sink.acc[(size_t)i * waves] = 0.0;
        slant_nodes(y, n, xq, wq, [&](double X, double Y, double Z, double w, bool on) {
            const Geom g = sph_geom_ecef(M, X, Y, Z);
            double Lk[KCAP];
            laguerre<KCAP>(M.maxk, g.z, Lk);
            const double E = exp(-0.5 * g.z);
#pragma unroll
            for (int k = 0; k < KCAP; ++k) sink.ELk[k] = k < M.maxk ? E * Lk[k] : 0.0;
            sink.wgt = on ? w : 0.0;            // the lanes past n run node 0 again and add nothing
            sph_point<LCAP, KCAP>(M, g, sink);
        });
    }
    rayb_finish(y, sh, N, waves, wave, P, Yo);
}

// K1l for the RBF model: the same wave per ray and lane per node; the centres in groups of RAYB_RBF_TR, a group's Gaussians
// through the tile and rayb_sum
constexpr int RAYB_RBF_TR = 16;

__global__ __launch_bounds__(SLANT_WAVES * 64) void k_slant_basis_rbf(RbfDev M, int64_t P, const double* __restrict__ a,
                                                                      const double* __restrict__ b, const double* __restrict__ eq,
                                                                      int F, double tol, int n, const double* __restrict__ xq,
                                                                      const double* __restrict__ wq, double* __restrict__ Yo,
                                                                      double* __restrict__ chord)
{
    constexpr int TR = RAYB_RBF_TR;
    extern __shared__ __align__(16) double sh[];
    const int lane = threadIdx.x & 63, wave = wave_index(), waves = blockDim.x >> 6;
    const int64_t p = (int64_t)blockIdx.x * waves + wave;
    const SlantRay y = slant_clip(p, P, a, b, eq, F, tol, chord);
    const int N = M.N;
    if (y.live) {
        double* tile = sh + (size_t)N * waves + (size_t)wave * TR * RAYB_LD;
        double* acc = sh + wave;
        for (int i = lane; i < N; i += 64) acc[(size_t)i * waves] = 0.0;
        slant_nodes(y, n, xq, wq, [&](double X, double Y, double Z, double w, bool on) {
            const double wgt = on ? w : 0.0;
            for (int k0 = 0; k0 < N; k0 += TR) {
#pragma unroll
                for (int j = 0; j < TR; ++j) {
                    const int k = k0 + j < N ? k0 + j : N - 1;
                    tile[j * RAYB_LD + lane] = wgt * rbf_gauss(M, k, X, Y, Z);
                }
                rayb_sum<TR>(tile, acc, waves, [&](int r) { return k0 + r < N ? k0 + r : -1; });
            }
        });
    }
    rayb_finish(y, sh, N, waves, wave, P, Yo);
}

// The rays, records, hull and rule of a K2l or K1l launch (vi_eval_slant_f64): w == nullptr is nearest mode.
struct SlantArgs {
    int64_t P;
    const double *a, *b;
    const int* rec;
    const double* w;
    int R;
    const double* eq;
    int F;
    double tol;
    int n;
    const double *xq, *wq;
    double *out, *chord;
};

// one K2l launch on the rays of s, `waves` of them to a workgroup; C: the rows the kernel reads (the RBF model's: the raw ones)
template <class K, class Dev>
int launch_slant(vi_model* m, K kernel, int waves, size_t lds, const Dev& dev, const SlantArgs& s, const double* C)
{
    return vi_launch(kernel, dim3(nblocks(s.P, waves)), dim3(waves * 64), lds, m->ctx->stream, dev, s.P, s.a, s.b, s.rec, s.w, s.R,
                     C, s.eq, s.F, s.tol, s.n, s.xq, s.wq, s.out, s.chord);
}

// as many rays (waves) in a workgroup as the LDS holds: SLANT_WAVES, halved while lds_bytes(waves) is beyond the 64 KB of a
// workgroup, one at the least
template <class Bytes>
int slant_waves(Bytes&& lds_bytes)
{
    int waves = SLANT_WAVES;
    while (waves > 1 && lds_bytes(waves) > 64 * 1024) waves >>= 1;
    return waves;
}

// the tiled kernel on the R prepared rows: the LDS holds the rays' rows beside the table, fewer rays at the orders whose table
// and row fill most of it (one always fits: fast_eval_fits(m, 1))
template <int L, int K, bool INTERP>
int launch_slant_sph_fast(vi_model* m, const SlantArgs& s)
{
    const auto lds = [&](int waves) { return chain_lds_bytes(m->nvmax0 + 1, L, (size_t)waves * m->N); };
    const int waves = slant_waves(lds);
    return launch_slant(m, k_slant_sph_fast<L, K, INTERP>, waves, lds(waves), m->sph, s, m->d_coef);
}

// K1l launch (vi_eval_slant_basis_f64): the LDS holds the rays' accumulator columns beside the tiles, so SLANT_WAVES rays share a
// workgroup unless N is in the thousands
template <class K, class Dev>
int launch_slant_basis(vi_model* m, K kernel, const Dev& dev, int TR, const SlantArgs& s)
{
    const auto lds = [&](int waves) { return rayb_lds_bytes(m->N, waves, TR); };
    const int waves = slant_waves(lds);
    if (lds(waves) > 64 * 1024) {
        vi_set_error("vi_eval_slant_basis_f64: the %d accumulators of a ray exceed the LDS of a workgroup", m->N);
        return VI_ERR_UNSUPPORTED;
    }
    return vi_launch(kernel, dim3(nblocks(s.P, waves)), dim3(waves * 64), lds(waves), m->ctx->stream, dev, s.P, s.a, s.b, s.eq, s.F,
                     s.tol, s.n, s.xq, s.wq, s.out, s.chord);
}

// K1l on the rays of s (s.out: the matrix, N x s.P): what vi_eval_slant_basis_f64 and vi_eval_slant_err_f64 launch
int slant_basis(vi_model* m, const char* who, const SlantArgs& s)
{
    if (m->kind != VI_MODEL_SPHHARMLAG) return launch_slant_basis(m, k_slant_basis_rbf, m->rbf, RAYB_RBF_TR, s);
    return at_order_cap(m, who, [&](auto lc, auto kc) {
        return launch_slant_basis(m, k_slant_basis_sph<lc, kc>, m->sph, RayBasisSink<kc>::TR, s);
    });
}

}  // namespace

// Line integrals along straight rays (include/vinterp.h): K2l.  The coefficient preparation of vi_eval_track_f64 (all R rows
// prepared once into m->d_coef) and no hull pass - the kernel clips each ray against the caller's facet list itself -, then one
// launch: k_slant_sph_fast for the orders of vi_eval_f64's fast list, the per-lane kernels for every other order,
// VINTERP_EVAL=generic and the RBF model.  fp64 chains whatever vi_model_set_eval_precision set.
extern "C" int vi_eval_slant_f64(vi_model* m, int64_t P, const double* d_a, const double* d_b, const int32_t* d_rec,
                                 const double* d_w, int64_t R, const double* d_C, const double* d_hull_eq, int32_t F,
                                 double hull_tol, int32_t n, const double* d_x, const double* d_wq, double* d_out, double* d_chord)
{
    VI_REQUIRE(m && d_a && d_b && d_rec && d_x && d_wq && d_out, "null argument");
    VI_REQUIRE(P >= 0 && R >= 0 && F >= 0, "negative size");
    VI_REQUIRE_RULE(n);
    VI_REQUIRE_RECORDS(R, d_C, "coefficients");
    VI_REQUIRE_RAYS(P);
    VI_REQUIRE_HULL(F, d_hull_eq);
    if (P == 0) return VI_OK;
    VI_HIP(hipSetDevice(m->ctx->device));
    const bool sph = m->kind == VI_MODEL_SPHHARMLAG;
    // (R = 0 prepares no coefficients: every ray is NaN, no kernel reads a row)
    const int rc = prepare_call(m, 0, nullptr, nullptr, nullptr, nullptr, 0, 0., sph ? R : 0, d_C);
    if (rc != VI_OK) return rc;
    const SlantArgs s{P, d_a, d_b, d_rec, d_w, (int)R, d_hull_eq, (int)F, hull_tol, (int)n, d_x, d_wq, d_out, d_chord};
    EvalTimer timer(m->ctx);
    return with_flag(d_w != nullptr, [&](auto interp) {
        if (!sph) return launch_slant(m, k_slant_rbf<interp>, BLOCK / 64, 0, m->rbf, s, d_C);
        int rcf;
        if (fast_eval_fits(m, 1) && at_fast_order(m, &rcf, [&](auto l, auto k) { return launch_slant_sph_fast<l, k, interp>(m, s); }))
            return rcf;
        return at_order_cap(m, "vi_eval_slant_f64", [&](auto lc, auto kc) {
            return launch_slant(m, k_slant_sph<lc, kc, interp>, BLOCK / 64, 0, m->sph, s, m->d_coef);
        });
    });
}

// The ray-integrated basis (include/vinterp.h): K1l.  No preparation - the kernel clips each ray against the caller's facet list
// itself and reads no coefficients - and one launch (slant_basis).
extern "C" int vi_eval_slant_basis_f64(vi_model* m, int64_t P, const double* d_a, const double* d_b, const double* d_hull_eq,
                                       int32_t F, double hull_tol, int32_t n, const double* d_x, const double* d_wq, double* d_Y,
                                       double* d_chord)
{
    VI_REQUIRE(m && d_a && d_b && d_x && d_wq && d_Y, "null argument");
    VI_REQUIRE(P >= 0 && F >= 0, "negative size");
    VI_REQUIRE_RULE(n);
    VI_REQUIRE_RAYS(P);
    VI_REQUIRE_HULL(F, d_hull_eq);
    if (P == 0) return VI_OK;
    VI_HIP(hipSetDevice(m->ctx->device));
    const SlantArgs s{P, d_a, d_b, nullptr, nullptr, 0, d_hull_eq, (int)F, hull_tol, (int)n, d_x, d_wq, d_Y, d_chord};
    EvalTimer timer(m->ctx);
    return slant_basis(m, "vi_eval_slant_basis_f64", s);
}

// Standard errors of line integrals (include/vinterp.h): per chunk of rays K1l's matrix into the context workspace - the same
// clip, the same rule, a NaN column for a miss - and vi_eval_records_err_f64's routes on it, as vi_eval_track_err_f64 does with
// the basis of its points.  K1l takes planar end points and gives a planar chord, each with the ray count as its pitch: a chunk
// that is not the whole call has its end points copied side by side into the workspace and its chord copied out of it.
extern "C" int vi_eval_slant_err_f64(vi_model* m, int64_t P, const double* d_a, const double* d_b, const int32_t* d_rec,
                                     const double* d_w, int64_t R, const double* d_dC, const double* d_hull_eq, int32_t F,
                                     double hull_tol, int32_t n, const double* d_x, const double* d_wq, double* d_out,
                                     double* d_chord)
{
    VI_REQUIRE(m && d_a && d_b && d_rec && d_x && d_wq && d_out, "null argument");
    VI_REQUIRE(P >= 0 && R >= 0 && F >= 0, "negative size");
    VI_REQUIRE_RULE(n);
    VI_REQUIRE_RECORDS(R, d_dC, "covariances");
    VI_REQUIRE_HULL(F, d_hull_eq);
    if (P == 0) return VI_OK;
    vi_ctx* c = m->ctx;
    VI_HIP(hipSetDevice(c->device));
    const int64_t chunk = track_err_chunk(m->N, P);
    double *Y, *ends, *work;                              // ends: a (3 x chunk), b (3 x chunk), chord (2 x chunk) of a chunk
    const int rc = track_err_workspace(m, P, chunk, d_out, chunk < P ? (size_t)8 * chunk : 0, &Y, &ends, &work);
    if (rc != VI_OK) return rc;
    const size_t row = sizeof(double);
    EvalTimer timer(c);
    return for_chunks(P, chunk, [&](int64_t p0, int64_t pc) -> int {
        SlantArgs s{pc, d_a, d_b, nullptr, nullptr, 0, d_hull_eq, (int)F, hull_tol, (int)n, d_x, d_wq, Y, d_chord};
        if (pc < P) {
            VI_HIP(hipMemcpy2DAsync(ends, pc * row, d_a + p0, P * row, pc * row, 3, hipMemcpyDeviceToDevice, c->stream));
            VI_HIP(hipMemcpy2DAsync(ends + 3 * pc, pc * row, d_b + p0, P * row, pc * row, 3, hipMemcpyDeviceToDevice, c->stream));
            s.a = ends;
            s.b = ends + 3 * pc;
            s.chord = d_chord ? ends + 6 * pc : nullptr;
        }
        int rc = slant_basis(m, "vi_eval_slant_err_f64", s);
        if (rc != VI_OK) return rc;
        if (pc < P && d_chord)
            VI_HIP(hipMemcpy2DAsync(d_chord + p0, P * row, s.chord, pc * row, pc * row, 2, hipMemcpyDeviceToDevice, c->stream));
        return vi_records_err(m, pc, Y, d_rec + p0, d_w ? d_w + p0 : nullptr, R, d_dC, d_out + p0, work);
    });
}
