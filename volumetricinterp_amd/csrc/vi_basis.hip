// Basis-function kernels for gfx950: geodetic -> model coordinates, Laguerre x spherical-cap
// harmonics (reference: volumetricinterp/models/sphharmlag.py:118-145, :324-359) and Gaussian RBF
// (reference: volumetricinterp/models/radbasfun.py:83-112), as
//   K1  k_basis_*  : materialise A (used by the fit),
//   K2  k_eval_*   : fused evaluation  out[t,q] = sum_n A[q,n] C[t,n]  (Estimate.__call__,
//                    estimate.py:110-123) that never writes A, with the convex-hull test fused in: a unit of its own,
//                    vi_eval.hip, as are its kin along tracks (vi_track.hip) and rays (vi_slant.hip); here are the hull pass
//                    and the call preparation of them all, and the gradient basis.
// One thread per point; lat/lon/alt are read as coalesced SoA streams; every table the 64 lanes of
// a wave share (recurrence coefficients, coefficient tiles) is addressed wave-uniformly so it is
// served by the scalar data path / LDS broadcast and never costs per-lane HBM traffic.
#include "vi_sph_device.h"
#include "vi_eval_host.h"

#include <algorithm>

namespace {

// ---------------------------------------------------------------------------------------------
// K1: basis assembly.  A[p*ld_p + n*ld_n], n = k*maxl^2 + l(l+1) + m  (sphharmlag.py:79-99)
template <int KCAP>
struct BasisSink {
    double* A;
    int64_t ld_n;
    int maxk, L2;
    const double* __restrict__ scale;
    double ELk[KCAP];
    bool active;
    template <int LCAP>
    __device__ __forceinline__ void consume(int l, const double* cur, const double* cm, const double* sm)
    {
        const int r0 = l * (l + 1);
#pragma unroll
        for (int m = 0; m < LCAP; ++m) {
            if (m <= l) {
                const double fp = scale[r0 + m] * cm[m] * cur[m];
                const double fm = scale[r0 - m] * sm[m] * cur[m];
#pragma unroll
                for (int k = 0; k < KCAP; ++k) {
                    if (k < maxk && active) {
                        A[(int64_t)(k * L2 + r0 + m) * ld_n] = ELk[k] * fp;
                        if (m > 0) A[(int64_t)(k * L2 + r0 - m) * ld_n] = ELk[k] * fm;
                    }
                }
            }
        }
    }
};

template <int LCAP, int KCAP>
__global__ __launch_bounds__(BLOCK) void k_basis_sph(SphDev M, int64_t P, const double* __restrict__ lat,
                                                     const double* __restrict__ lon, const double* __restrict__ alt,
                                                     double* __restrict__ A, int64_t ld_p, int64_t ld_n)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t pc = p < P ? p : P - 1;
    const Geom g = sph_geom(M, lat[pc], lon[pc], alt[pc]);
    BasisSink<KCAP> sink;
    sink.A = A + pc * ld_p;
    sink.ld_n = ld_n;
    sink.maxk = M.maxk;
    sink.L2 = M.maxl * M.maxl;
    sink.scale = M.scale;
    sink.active = p < P;
    double Lk[KCAP];
    laguerre<KCAP>(M.maxk, g.z, Lk);
    const double E = exp(-0.5 * g.z);
#pragma unroll
    for (int k = 0; k < KCAP; ++k) sink.ELk[k] = E * Lk[k];
    sph_point<LCAP, KCAP>(M, g, sink);
}

// ---------------------------------------------------------------------------------------------
// Gradient basis (sphharmlag.py:148-184): for every basis function the components along z, theta, phi,
//   zhat = -e/2 (L0 + 2 L1) Pmv A 100/RE,  that = e L0 (-(v+1) x Pmv + (v-m+1) Pmv1) A / (y (z/100+1) RE),
//   phat = e L0 Pmv dAz / (y (z/100+1) RE),
// with L1 = eval_genlaguerre(k-1, 1, z), Pmv1 = lpmv(m, v+1, x).  Same chains as the basis, run one degree
// further: when the chain has reached degree nu_l + 1, prev holds P at nu_l and cur at nu_l + 1.
// GRAD_STORE: store the gradient basis at the caller's strides.  GRAD_CONTRACT: contract it on the fly with one coefficient
// vector Cv (N) and store only the three gradient components per point (ld_p = 3, ld_c = 1): the gradient of the fitted
// parameter, never materialising 3N values per point.  GRAD_RESIDENT: the store of GRAD_STORE for the matrix a resident grid
// keeps (vi_eval_grad_basis_f64: planar strides, a lane is a point and every store of a wave is 64 consecutive doubles) with
// the hull mask - a lane outside stores NaN into its 3N entries and a wave without a lane inside leaves before the chains -
// and, with ENU, every (z, theta, phi) triple turned into east, north, up by the point's matrix (enu_frame) before the stores.
enum { GRAD_STORE = 0, GRAD_CONTRACT = 1, GRAD_RESIDENT = 2 };

// what k_grad_sph does with a term: adds its product with the coefficient to the point's triple (GRAD_CONTRACT), or stores it
template <int MODE, bool ENU>
struct GradSink {
    const double* __restrict__ Cv;
    double* Gp;
    int64_t ld_c, ld_n;
    double F[9];
    bool active;
    double az, at, ap;
    __device__ __forceinline__ void term(int n, double tz, double tt, double tp, double L0k, double L1k)
    {
        if (MODE == GRAD_CONTRACT) {
            const double cf = Cv[n];
            az = fma(tz * (L0k + 2.0 * L1k), cf, az);
            at = fma(tt * L0k, cf, at);
            ap = fma(tp * L0k, cf, ap);
        } else if (active) {
            double* o = Gp + (int64_t)n * ld_n;
            const double gz = tz * (L0k + 2.0 * L1k), gt = tt * L0k, gp = tp * L0k;
            if (ENU) {
                o[0] = fma(F[0], gz, fma(F[1], gt, F[2] * gp));
                o[ld_c] = fma(F[3], gz, fma(F[4], gt, F[5] * gp));
                o[2 * ld_c] = fma(F[6], gz, fma(F[7], gt, F[8] * gp));
            } else {
                o[0] = gz;
                o[ld_c] = gt;
                o[2 * ld_c] = gp;
            }
        }
    }
};

template <int LCAP, int KCAP, int MODE, bool ENU>
__global__ __launch_bounds__(BLOCK) void k_grad_sph(SphDev M, int64_t P, const double* __restrict__ lat,
                                                    const double* __restrict__ lon, const double* __restrict__ alt,
                                                    const double* __restrict__ Cv, const unsigned char* __restrict__ mask,
                                                    double* __restrict__ Gout, int64_t ld_p, int64_t ld_c, int64_t ld_n)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t pc = p < P ? p : P - 1;
    bool active = p < P;
    double* Gp = Gout + pc * ld_p;
    if (MODE == GRAD_RESIDENT && mask) {
        const bool in = mask[pc] != 0;
        if (active && !in) {
            const double nan = __builtin_nan("");
            for (int n = 0; n < M.N; ++n) {
                double* o = Gp + (int64_t)n * ld_n;
                o[0] = nan;
                o[ld_c] = nan;
                o[2 * ld_c] = nan;
            }
        }
        active = active && in;
        if (!__any(active)) return;           // whole wave outside the hull: skip the chains
    }
    const Geom g = sph_geom(M, lat[pc], lon[pc], alt[pc]);
    GradSink<MODE, ENU> sink;
    sink.Cv = Cv;
    sink.Gp = Gp;
    sink.ld_c = ld_c;
    sink.ld_n = ld_n;
    sink.active = active;
    sink.az = sink.at = sink.ap = 0.0;
    if (ENU) enu_frame(M, g, lat[pc], lon[pc], sink.F);
    grad_point<LCAP, KCAP>(M, g, sink);
    if (MODE == GRAD_CONTRACT && active) {
        Gp[0] = sink.az;
        Gp[ld_c] = sink.at;
        Gp[2 * ld_c] = sink.ap;
    }
}

// Convex-hull test (estimate.py:153-178 semantics: inside <=> max_f (n_f . x + d_f) <= tol), as a mask pass.
// `hull` is the internal buffer built by k_prep_hull: [c0 (3 doubles, 1 pad)] [F x 4 fp64 facet equations]
// [F x float4 facets relative to c0].  With ~460 facets an fp64 test inside the evaluation kernel cost twice the
// whole basis (dependent scalar loads), so the test is its own pass: the fp32 facets (wave-uniform scalar loads, see
// k_hull_mask) are evaluated relative to a reference point c0 on the plane of facet 0; only points within a band of the
// surface repeat the test in fp64.  The band covers the fp32 error of the prefilter: the float casts of normal and
// offset plus three FMA roundings are a few units of 2^-24 |x - c0|, and c0 - the foot of the origin's perpendicular
// on a facet plane - may lie far from the hull when that plane passes near the Earth's centre, so the band grows with
// the distance: HULL_BAND + HULL_BAND_REL |x - c0| (4 m at the reference point, ~10 m at 6000 km).  Points with
// non-finite coordinates are outside.  The byte mask is reused by every timestep tile of the evaluation.
constexpr float HULL_BAND = 4.0f;
constexpr float HULL_BAND_REL = 1.0e-6f;
constexpr int HULL_HDR = 8;          // doubles in front of the facet equations: c0 (3), s, offmax, 3 spare

constexpr int HULL_PP = 8;          // points per thread: every facet fetched serves eight points
constexpr int HULL_PAD = 16;        // the fp32 facet list is padded to a multiple of 16 with repeats of facet 0

// Round 3: the facets come through wave-uniform (scalar) loads - four planes per s_load_dwordx16, used as SGPR operands
// of the packed FMAs - instead of LDS broadcasts: at 4 points per thread the pass issued one ds_read_b128 per facet and
// thread, 8 LDS clocks for every 46 VALU clocks of a SIMD with four SIMDs on one LDS pipe (~70 % busy), plus a v_mov
// per facet; eight points per thread halve what is left per point (early-exit test, plane set-up).
__global__ __launch_bounds__(BLOCK, 4) void k_hull_mask(int64_t Q, const double* __restrict__ lat,
                                                     const double* __restrict__ lon, const double* __restrict__ alt,
                                                     const double* __restrict__ hull, int F, double tol,
                                                     unsigned char* __restrict__ mask)
{
    typedef float f2 __attribute__((ext_vector_type(2)));
    const float4* __restrict__ pl = reinterpret_cast<const float4*>(hull + HULL_HDR + 4 * (size_t)F);
    const int Fp = (F + HULL_PAD - 1) / HULL_PAD * HULL_PAD;
    const int64_t q0 = (int64_t)blockIdx.x * (BLOCK * HULL_PP) + threadIdx.x;      // points q0 + u * BLOCK
    const double c0x = hull[0], c0y = hull[1], c0z = hull[2];
    // geodetic -> ECEF one point after the other (one copy of the fp64 trigonometry, few registers), the fp32 offsets
    // from c0 handed to the facet loop's registers through LDS (each thread reads back what it wrote: no barrier)
    __shared__ float sh_d[HULL_PP][3][BLOCK];
#pragma unroll 1
    for (int u = 0; u < HULL_PP; ++u) {
        const int64_t q = q0 + (int64_t)u * BLOCK;
        const int64_t qc = q < Q ? q : Q - 1;
        double X, Y, Z;
        geodetic2ecef(lat[qc], lon[qc], alt[qc], X, Y, Z);
        sh_d[u][0][threadIdx.x] = (float)(X - c0x);
        sh_d[u][1][threadIdx.x] = (float)(Y - c0y);
        sh_d[u][2][threadIdx.x] = (float)(Z - c0z);
    }
    f2 px[HULL_PP / 2], py[HULL_PP / 2], pz[HULL_PP / 2], dmax[HULL_PP / 2], thr[HULL_PP / 2];
    bool finite[HULL_PP];
#pragma unroll
    for (int u = 0; u < HULL_PP; ++u) {
        const float dx = sh_d[u][0][threadIdx.x], dy = sh_d[u][1][threadIdx.x], dz = sh_d[u][2][threadIdx.x];
        finite[u] = fabsf(dx) + fabsf(dy) + fabsf(dz) < 3.0e38f;                   // false for NaN / inf coordinates
        px[u / 2][u % 2] = dx;
        py[u / 2][u % 2] = dy;
        pz[u / 2][u % 2] = dz;
        dmax[u / 2][u % 2] = -3.0e38f;
        thr[u / 2][u % 2] = HULL_BAND + HULL_BAND_REL * sqrtf(dx * dx + dy * dy + dz * dz);       // the band of the point
    }
    auto dist = [&](const float4 p, int h) {
        return __builtin_elementwise_fma(f2{p.x, p.x}, px[h],
                                         __builtin_elementwise_fma(f2{p.y, p.y}, py[h],
                                                                   __builtin_elementwise_fma(f2{p.z, p.z}, pz[h], f2{p.w, p.w})));
    };
    // four facets per round, the next four fetched while these are applied (the list carries one spare group)
    float4 n0 = pl[0], n1 = pl[1], n2 = pl[2], n3 = pl[3];
#pragma unroll 1
    for (int f = 0; f < Fp; f += 4) {
        const float4 p0 = n0, p1 = n1, p2 = n2, p3 = n3;
        n0 = pl[f + 4]; n1 = pl[f + 5]; n2 = pl[f + 6]; n3 = pl[f + 7];
#pragma unroll
        for (int h = 0; h < HULL_PP / 2; ++h) {
            const f2 d0 = dist(p0, h), d1 = dist(p1, h), d2 = dist(p2, h), d3 = dist(p3, h);
            dmax[h].x = fmaxf(fmaxf(dmax[h].x, d0.x), d1.x);
            dmax[h].y = fmaxf(fmaxf(dmax[h].y, d0.y), d1.y);
            dmax[h].x = fmaxf(fmaxf(dmax[h].x, d2.x), d3.x);
            dmax[h].y = fmaxf(fmaxf(dmax[h].y, d2.y), d3.y);
        }
        if ((f & (HULL_PAD - 4)) == HULL_PAD - 4) {
            // a point is outside as soon as ONE facet says so: leave when every point of the wave is decided
            float slack = 3.0e38f;
#pragma unroll
            for (int h = 0; h < HULL_PP / 2; ++h)
                slack = fminf(slack, fminf(dmax[h].x - thr[h].x, dmax[h].y - thr[h].y));
            if (__all(slack > (float)tol)) break;
        }
    }
    unsigned inbits = 0, border = 0;
#pragma unroll
    for (int u = 0; u < HULL_PP; ++u) {
        const float dm = dmax[u / 2][u % 2], bd = thr[u / 2][u % 2];
        if (!finite[u] || dm > (float)tol + bd) continue;                // outside
        if (dm < (float)tol - bd) inbits |= 1u << u;                      // inside
        else border |= 1u << u;                                           // within the band of the surface
    }
    // Points within the band: the exact fp64 test, one point at a time with the facets spread over the 64 lanes of the wave
    // (a lane running all F facets alone - F dependent scalar loads - held its whole wave for longer than the fp32 pass of
    // the entire grid takes: 150 us measured against 95 us with every point deep inside the hull)
    const int lane = threadIdx.x & 63;
    const double* __restrict__ eq = hull + HULL_HDR;
#pragma unroll 1
    for (int u = 0; u < HULL_PP; ++u) {
        const int64_t q = q0 + (int64_t)u * BLOCK;
        const bool bl = ((border >> u) & 1u) && q < Q;
        bool in = (inbits >> u) & 1u;
        unsigned long long todo = __ballot(bl);
        if (todo) {
            double X = 0.0, Y = 0.0, Z = 0.0;
            if (bl) geodetic2ecef(lat[q], lon[q], alt[q], X, Y, Z);
            while (todo) {
                const int src = __ffsll(todo) - 1;
                todo &= todo - 1;
                const double xs = __shfl(X, src), ys = __shfl(Y, src), zs = __shfl(Z, src);
                bool viol = false;
                for (int g = lane; g < F; g += 64) {
                    const double d = fma(eq[4 * g], xs, fma(eq[4 * g + 1], ys, fma(eq[4 * g + 2], zs, eq[4 * g + 3])));
                    viol = viol || !(d <= tol);
                }
                const bool any = __any(viol);
                if (lane == src) in = !any;
            }
        }
        if (q < Q) mask[q] = in ? 1 : 0;
    }
}

// ---- the hull pass on the matrix cores (round 4) -------------------------------------------------------------------------
// The plane distances of 32 points from 32 facets are ONE v_mfma_f32_32x32x16_f16: every coordinate (relative to c0, in units
// of HULL_UNIT metres) and every normal component (times HULL_NSCALE) is split into two halves hi + lo (22 bits together), and
// the sixteen k-slots of the instruction hold the four cross products of the three components plus the plane offset:
//      k     0    1    2    3    4    5    6    7  |  8    9    10   11   12    13    14 15
//  A  facet  nxh  nyh  nzh  nxl  nyl  nzl  nxh  nyh |  nzh  nxl  nyl  nzl  offh  offl  0  0
//  B  point  xh   yh   zh   xh   yh   zh   xl   yl  |  zl   xl   yl   zl   1024  1024  0  0
// (lanes 0-31 carry k 0-7 of row / column lane, lanes 32-63 k 8-15: cdna4 32x32x16 operand map).  The products of two halves
// are exact in fp32; what is lost is the split (2^-22 of |x|, |n|, |off| each), the flush of a subnormal lo half (6e-8 |x|)
// and the fp32 accumulation of sixteen terms (<= 16 x 2^-23 of (|x - c0| + |off|)): together < 2.5e-6 (|x - c0| + max |off|),
// covered by the band HULL_BAND + HULL_MX_REL (|x - c0| + max |off|), inside which a point repeats the test in fp64 - the
// mask is the fp64 definition's whatever the prefilter does inside its band.  The result column is the lane's point and the
// sixteen registers are sixteen facets, so the maximum over the facets is eight v_max3_f32 per tile and lane and one
// v_permlane32_swap at the end.  Measured (tools/microbench/mfma_max3_overlap.hip): 53 cycles per 1024 distances and SIMD with
// zero operands, 74 with real ones - the shader clock drops from 2.3 to 1.6 GHz under the load, the loop is power-bound -
// against ~190 of the packed-fp32 loop (k_hull_mask); 128^3 points x 460 facets: 88 -> 46 us over the call without a hull.
// Normals longer than 1 are scaled down by s = max |n| (Qhull's are unit vectors: s = 1), points further than HULL_FAR from c0
// and lists with a non-finite entry or an offset beyond the fp16 range go to the fp64 test as they are.
constexpr float HULL_UNIT = 256.0f;          // metres per unit of the fp16 coordinates: 65504 units = 16 769 km
constexpr float HULL_NSCALE = 1024.0f;       // the unit normal's components times this: the lo half stays a normal fp16 number
constexpr float HULL_FAR = 1.6e7f;           // metres from c0 beyond which a point skips the fp16 prefilter
constexpr float HULL_MX_REL = 4.0e-6f;
constexpr int HULL_MX_PP = 4;                // points per thread = eight 32-point groups per wave and facet tile

__device__ __forceinline__ unsigned hull_split(float v)          // (hi, lo) halves of v packed: hi in bits 0-15
{
    const _Float16 hi = (_Float16)v;
    const _Float16 lo = (_Float16)(v - (float)hi);
    return (unsigned)__builtin_bit_cast(unsigned short, hi) | ((unsigned)__builtin_bit_cast(unsigned short, lo) << 16);
}

// geodetic2ecef with sincos_cw (vi_sph_device.h); false when an angle is outside the range of its reduction (or NaN)
__device__ __forceinline__ bool hull_geodetic2ecef(double lat, double lon, double alt, double& X, double& Y, double& Z)
{
    const double la = lat * DEG2RAD, lo = lon * DEG2RAD;
    double sl, cl, so, co;
    sincos_cw(la, sl, cl);
    sincos_cw(lo, so, co);
    const double a2 = WGS84_A * WGS84_A, b2 = WGS84_B * WGS84_B;
    const double Nn = a2 / sqrt(a2 * cl * cl + b2 * sl * sl);
    const double ba = WGS84_B / WGS84_A;
    X = (Nn + alt) * cl * co;
    Y = (Nn + alt) * cl * so;
    Z = (Nn * (ba * ba) + alt) * sl;
    return fabs(la) < 1.0e4 && fabs(lo) < 1.0e4;
}

typedef float hull_f16v __attribute__((ext_vector_type(16)));
__device__ __forceinline__ float hull_max16(const hull_f16v& c, float d)       // max(d, the sixteen results): eight v_max3_f32
{
    const float t0 = fmaxf(fmaxf(c[0], c[1]), c[2]), t1 = fmaxf(fmaxf(c[3], c[4]), c[5]), t2 = fmaxf(fmaxf(c[6], c[7]), c[8]),
                t3 = fmaxf(fmaxf(c[9], c[10]), c[11]), t4 = fmaxf(fmaxf(c[12], c[13]), c[14]), t5 = fmaxf(fmaxf(c[15], d), t0),
                t6 = fmaxf(fmaxf(t1, t2), t3);
    return fmaxf(fmaxf(t4, t5), t6);
}

template <int PP>
__global__ __launch_bounds__(BLOCK, 4) void k_hull_mask_mx(int64_t Q, const double* __restrict__ lat,
                                                           const double* __restrict__ lon, const double* __restrict__ alt,
                                                           const double* __restrict__ hull, int F, double tol,
                                                           unsigned char* __restrict__ mask)
{
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    typedef float f16v __attribute__((ext_vector_type(16)));
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    const int Fp = (F + HULL_PAD - 1) / HULL_PAD * HULL_PAD;
    const int T = (F + 31) / 32;
    const u4* __restrict__ tiles = reinterpret_cast<const u4*>(hull + HULL_HDR + 4 * (size_t)F) + (Fp + 4);
    const int lane = threadIdx.x & 63;
    const int64_t q0 = (int64_t)blockIdx.x * (BLOCK * PP) + threadIdx.x;           // points q0 + u * BLOCK
    const double c0x = hull[0], c0y = hull[1], c0z = hull[2];
    const float s = (float)hull[3];
    const float offmax = (float)hull[4];                                         // max |n . c0 + d| / s; inf: no prefilter
    // geodetic -> ECEF of the thread's PP points, unrolled: their 3 PP loads are in flight together (one after the other a
    // wave waited out a memory latency per point: the pass reads 24 B a point, 50 MB for 128^3).  thr < 0 marks a point the
    // prefilter does not judge (non-finite, far away, angle beyond the range of sincos_cw).
    // The B operands: lanes 0-31 hold k 0-7 of their column, lanes 32-63 k 8-15; one swap of the upper half of one register
    // with the lower half of another makes a register of each of the two groups a 64-lane set of points consists of.
    unsigned Bf[2 * PP][4];
    float thr[PP];
    double qlat[PP], qlon[PP], qalt[PP];
#pragma unroll
    for (int u = 0; u < PP; ++u) {
        const int64_t q = q0 + (int64_t)u * BLOCK;
        const int64_t qc = q < Q ? q : Q - 1;
        qlat[u] = lat[qc];
        qlon[u] = lon[qc];
        qalt[u] = alt[qc];
    }
#pragma unroll
    for (int u = 0; u < PP; ++u) {
        double X, Y, Z;
        const bool inrange = hull_geodetic2ecef(qlat[u], qlon[u], qalt[u], X, Y, Z);
        float vx = (float)((X - c0x) * (1.0 / HULL_UNIT)), vy = (float)((Y - c0y) * (1.0 / HULL_UNIT)),
              vz = (float)((Z - c0z) * (1.0 / HULL_UNIT));
        const float r = HULL_UNIT * sqrtf(vx * vx + vy * vy + vz * vz);
        const bool ok = inrange && r < HULL_FAR;                                 // false for NaN / inf coordinates too
        if (!ok) vx = vy = vz = 0.0f;
        const unsigned sx = hull_split(vx), sy = hull_split(vy), sz = hull_split(vz);
        thr[u] = ok ? s * (HULL_BAND + HULL_MX_REL * (r + offmax)) : -1.0f;
        const unsigned p0 = (sx & 0xffffu) | (sy << 16);                         // (xh, yh)
        const unsigned p1 = (sz & 0xffffu) | (sx & 0xffff0000u);                 // (zh, xl)
        const unsigned p2 = (sy >> 16) | (sz & 0xffff0000u);                     // (yl, zl)
        const unsigned lo[4] = {p0,                                              // (xh, yh)
                                (p1 & 0xffffu) | (p0 << 16),                     // (zh, xh)
                                (p0 >> 16) | (p1 << 16),                         // (yh, zh)
                                (p1 >> 16) | (p2 << 16)};                        // (xl, yl)
        const unsigned hi[4] = {(p2 >> 16) | (p1 & 0xffff0000u),                 // (zl, xl)
                                p2,                                              // (yl, zl)
                                0x64006400u,                                     // (1024, 1024)
                                0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const auto w = __builtin_amdgcn_permlane32_swap(lo[j], hi[j], false, false);
            Bf[2 * u][j] = w[0];                    // lanes 0-31: lo of their own point; 32-63: hi of the point of lane - 32
            Bf[2 * u + 1][j] = w[1];                // lanes 0-31: lo of the point of lane + 32; 32-63: hi of their own
        }
    }
    float dmax[2 * PP];
#pragma unroll
    for (int g = 0; g < 2 * PP; ++g) dmax[g] = -3.0e38f;
    const float cs = s * (HULL_UNIT / HULL_NSCALE);                              // accumulator units -> the equations' units
    const float tolf = (float)tol;
    u4 An = tiles[lane];
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        const u4 A = An;
        An = tiles[(size_t)(t + 1 < T ? t + 1 : t) * 64 + lane];
        // Two accumulators by hand: the product of group g + 1 is issued before the maxima of group g are taken.  Left to the
        // compiler the loop is product -> wait -> eight maxima -> next product on ONE accumulator, 85 cycles per product
        // and SIMD at four waves against 53 this way (tools/microbench/mfma_max3_overlap.hip).  The products are inline
        // assembly, so the wait between a matrix-core write and a vector read of it is ours to keep: s_nop 15 (16 wait
        // states; the 8-pass product needs 12) inside the same statement, so that nothing the compiler may place behind
        // it - the maxima, a copy - reads the accumulator early; "=&v": the result does not share registers with A or B.
        f16v pa, pb;
        // (`held`: the other accumulator, named as an operand so that its maxima stay behind this product - the compiler is
        // otherwise free to take them first and to put both accumulators into the same registers)
#define VI_HULL_MFMA(acc, g, held)                                                                                        \
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %2, %3, 0\n\ts_nop 15"                                                      \
                 : "=&v"(acc), "+v"(held)                                                                                 \
                 : "v"(A), "v"((u4){Bf[g][0], Bf[g][1], Bf[g][2], Bf[g][3]}))
        asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0\n\ts_nop 15"
                     : "=&v"(pa) : "v"(A), "v"((u4){Bf[0][0], Bf[0][1], Bf[0][2], Bf[0][3]}));
#pragma unroll
        for (int g = 0; g < 2 * PP; g += 2) {
            VI_HULL_MFMA(pb, g + 1, pa);
            dmax[g] = hull_max16(pa, dmax[g]);
            if (g + 2 < 2 * PP) VI_HULL_MFMA(pa, g + 2, pb);
            dmax[g + 1] = hull_max16(pb, dmax[g + 1]);
        }
#undef VI_HULL_MFMA
        if ((t & (t + 1)) == 0 && t + 1 < T) {
            // after tiles 0, 1, 3, 7, ...: a point is outside as soon as ONE facet says so - leave when every point of the
            // wave is decided (the host hands the facets over in greedy-cover order: the first tile decides 98 % of them)
            float slack = 3.0e38f;
#pragma unroll
            for (int u = 0; u < PP; ++u) {
                const auto w = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, dmax[2 * u]),
                                                                __builtin_bit_cast(unsigned, dmax[2 * u + 1]), false, false);
                const unsigned w0 = w[0], w1 = w[1];                  // (a bit_cast of w[1] itself reads w[0]: through scalars)
                const float dm = cs * fmaxf(__uint_as_float(w0), __uint_as_float(w1));
                slack = fminf(slack, thr[u] < 0.0f ? 3.0e38f : dm - thr[u]);
            }
            if (__all(slack > tolf)) break;
        }
    }
    unsigned inbits = 0, border = 0;
#pragma unroll
    for (int u = 0; u < PP; ++u) {
        // lanes 0-31: the point's two partial maxima are dmax[2u] of this lane and of lane + 32; lanes 32-63: dmax[2u + 1]
        const auto w = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, dmax[2 * u]),
                                                        __builtin_bit_cast(unsigned, dmax[2 * u + 1]), false, false);
        const unsigned w0 = w[0], w1 = w[1];                  // (a bit_cast of w[1] itself reads w[0]: through scalars)
        const float dm = cs * fmaxf(__uint_as_float(w0), __uint_as_float(w1));
        const float bd = thr[u];
        if (bd < 0.0f || !(fabsf(dm - tolf) > bd)) border |= 1u << u;             // not judged, or within the band (NaN too)
        else if (dm < tolf) inbits |= 1u << u;                                    // inside
    }
    // Points within the band: the exact fp64 test, one point at a time with the facets spread over the 64 lanes of the wave
    const double* __restrict__ eq = hull + HULL_HDR;
#pragma unroll 1
    for (int u = 0; u < PP; ++u) {
        const int64_t q = q0 + (int64_t)u * BLOCK;
        const bool bl = ((border >> u) & 1u) && q < Q;
        bool in = (inbits >> u) & 1u;
        unsigned long long todo = __ballot(bl);
        if (todo) {
            double X = 0.0, Y = 0.0, Z = 0.0;
            if (bl) geodetic2ecef(lat[q], lon[q], alt[q], X, Y, Z);
            while (todo) {
                const int src = __ffsll(todo) - 1;
                todo &= todo - 1;
                const double xs = __shfl(X, src), ys = __shfl(Y, src), zs = __shfl(Z, src);
                bool viol = false;
                for (int g = lane; g < F; g += 64) {
                    const double d = fma(eq[4 * g], xs, fma(eq[4 * g + 1], ys, fma(eq[4 * g + 2], zs, eq[4 * g + 3])));
                    viol = viol || !(d <= tol);
                }
                const bool any = __any(viol);
                if (lane == src) in = !any;
            }
        }
        if (q < Q) mask[q] = in ? 1 : 0;
    }
}

// hullbuf <- [c0, s, offmax][eq][float4 facets][fp16 operand tiles]; c0 = foot of the origin's perpendicular on facet 0 (a
// point of the hull surface), s = max(1, longest normal), offmax = max |n . c0 + d| / s (inf: a non-finite entry in the list or
// an offset beyond the fp16 range - every point then takes the fp64 test).  Every block forms s and offmax itself.
inline size_t hull_buf_bytes(size_t F)
{
    const size_t Fp = (F + HULL_PAD - 1) / HULL_PAD * HULL_PAD, T = (F + 31) / 32;
    return (HULL_HDR + 4 * F) * sizeof(double) + (Fp + 4) * sizeof(float4) + T * 64 * 16 + 64;
}

constexpr int HULL_PREP_BLOCKS = 4;
__device__ __forceinline__ void prep_hull_body(int F, const double* __restrict__ eq, double* __restrict__ hullbuf, int bid, int nb)
{
    const double c0x = -eq[3] * eq[0], c0y = -eq[3] * eq[1], c0z = -eq[3] * eq[2];
    __shared__ double sh_n[256], sh_o[256];
    double nm = 0.0, om = 0.0;
    for (int f = threadIdx.x; f < F; f += blockDim.x) {
        const double nx = eq[4 * f], ny = eq[4 * f + 1], nz = eq[4 * f + 2], off = nx * c0x + ny * c0y + nz * c0z + eq[4 * f + 3];
        const double n2 = nx * nx + ny * ny + nz * nz;
        nm = !(n2 <= 1.0e300) ? __builtin_inf() : fmax(nm, n2);
        om = !(fabs(off) <= 1.0e300) ? __builtin_inf() : fmax(om, fabs(off));
    }
    sh_n[threadIdx.x] = nm;
    sh_o[threadIdx.x] = om;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sh_n[threadIdx.x] = fmax(sh_n[threadIdx.x], sh_n[threadIdx.x + w]);
            sh_o[threadIdx.x] = fmax(sh_o[threadIdx.x], sh_o[threadIdx.x + w]);
        }
        __syncthreads();
    }
    const double s = fmax(1.0, sqrt(sh_n[0]));
    double offmax = sh_o[0] / s;
    if (!(s <= 1.0e150) || !(offmax <= 65000.0 * HULL_UNIT)) offmax = __builtin_inf();
    if (threadIdx.x == 0 && bid == 0) {
        hullbuf[0] = c0x; hullbuf[1] = c0y; hullbuf[2] = c0z; hullbuf[3] = s;
        hullbuf[4] = offmax; hullbuf[5] = 0.0; hullbuf[6] = 0.0; hullbuf[7] = 0.0;
    }
    float4* pl = reinterpret_cast<float4*>(hullbuf + HULL_HDR + 4 * (size_t)F);
    for (int f = bid * blockDim.x + threadIdx.x; f < F; f += nb * blockDim.x) {
        const double nx = eq[4 * f], ny = eq[4 * f + 1], nz = eq[4 * f + 2], off = eq[4 * f + 3];
        double* e = hullbuf + HULL_HDR + 4 * (size_t)f;
        e[0] = nx; e[1] = ny; e[2] = nz; e[3] = off;
        pl[f] = make_float4((float)nx, (float)ny, (float)nz, (float)(nx * c0x + ny * c0y + nz * c0z + off));
    }
    // padding of the fp32 list (k_hull_mask reads it in groups of HULL_PAD): facet 0 again - the maximum does not change
    const int Fp = (F + HULL_PAD - 1) / HULL_PAD * HULL_PAD;
    for (int f = F + bid * blockDim.x + threadIdx.x; f < Fp + 4; f += nb * blockDim.x)      // + the spare group
        pl[f] = make_float4((float)eq[0], (float)eq[1], (float)eq[2], (float)(eq[0] * c0x + eq[1] * c0y + eq[2] * c0z + eq[3]));
    // the fp16 operand tiles of k_hull_mask_mx: tile t, lane l = facet 32 t + (l & 31) (facet 0 again past the end), k-slots
    // 8 (l >> 5) ... + 7 of the table above its kernel
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    u4* tiles = reinterpret_cast<u4*>(pl + Fp + 4);
    const int T = (F + 31) / 32;
    const bool usable = offmax < __builtin_inf();
    for (int i = bid * blockDim.x + threadIdx.x; i < T * 64; i += nb * blockDim.x) {
        int f = 32 * (i >> 6) + (i & 31);
        if (f >= F) f = 0;
        const double nx = eq[4 * f], ny = eq[4 * f + 1], nz = eq[4 * f + 2];
        const double off = nx * c0x + ny * c0y + nz * c0z + eq[4 * f + 3];
        u4 v = {0u, 0u, 0u, 0u};
        if (usable) {
            const unsigned sx = hull_split((float)(nx / s * HULL_NSCALE)), sy = hull_split((float)(ny / s * HULL_NSCALE)),
                           sz = hull_split((float)(nz / s * HULL_NSCALE)), so = hull_split((float)(off / s / HULL_UNIT));
            if (((i >> 5) & 1) == 0) {
                v[0] = (sx & 0xffffu) | (sy << 16);                  // (nxh, nyh)
                v[1] = (sz & 0xffffu) | (sx & 0xffff0000u);          // (nzh, nxl)
                v[2] = (sy >> 16) | (sz & 0xffff0000u);              // (nyl, nzl)
                v[3] = v[0];                                         // (nxh, nyh)
            } else {
                v[0] = (sz & 0xffffu) | (sx & 0xffff0000u);          // (nzh, nxl)
                v[1] = (sy >> 16) | (sz & 0xffff0000u);              // (nyl, nzl)
                v[2] = so;                                           // (offh, offl)
                v[3] = 0u;
            }
        }
        tiles[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_prep_hull(int F, const double* __restrict__ eq, double* __restrict__ hullbuf)
{
    prep_hull_body(F, eq, hullbuf, (int)blockIdx.x, (int)gridDim.x);
}

// Cp[t][r*maxk + k] = C[t][k*L2 + r] * scale[r]
__device__ __forceinline__ void prep_coef_body(int T, int maxk, int L2, const double* __restrict__ C,
                                               const double* __restrict__ scale, double* __restrict__ Cp, int64_t bid)
{
    const int N = maxk * L2;
    const int64_t i = bid * blockDim.x + threadIdx.x;
    if (i >= (int64_t)T * N) return;
    const int t = (int)(i / N), n = (int)(i % N);
    const int r = n / maxk, k = n % maxk;
    Cp[i] = C[(int64_t)t * N + k * L2 + r] * scale[r];
}

__global__ void k_prep_coef(int T, int maxk, int L2, const double* __restrict__ C, const double* __restrict__ scale,
                            double* __restrict__ Cp)
{
    prep_coef_body(T, maxk, L2, C, scale, Cp, (int64_t)blockIdx.x);
}

// the two preparations of a masked evaluation call in one launch: blocks 0-3 the hull buffer, the others the coefficients
__global__ __launch_bounds__(256) void k_prep_hull_coef(int F, const double* __restrict__ eq, double* __restrict__ hullbuf, int T,
                                                        int maxk, int L2, const double* __restrict__ C,
                                                        const double* __restrict__ scale, double* __restrict__ Cp)
{
    if (blockIdx.x < HULL_PREP_BLOCKS) prep_hull_body(F, eq, hullbuf, (int)blockIdx.x, HULL_PREP_BLOCKS);
    else prep_coef_body(T, maxk, L2, C, scale, Cp, (int64_t)blockIdx.x - HULL_PREP_BLOCKS);
}

__global__ void k_transform_sph(SphDev M, int64_t P, const double* __restrict__ lat, const double* __restrict__ lon,
                                const double* __restrict__ alt, double* z, double* th, double* ph)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const Geom g = sph_geom(M, lat[p], lon[p], alt[p]);
    z[p] = g.z;
    th[p] = acos(g.x);
    ph[p] = atan2(g.Ry, g.Rx);
}

// ---------------------------------------------------------------------------------------------
// Gaussian RBF model (radbasfun.py:83-112): A[p,n] = exp(-|R_p - c_n|^2 / eps^2), R in ECEF metres
__global__ __launch_bounds__(BLOCK) void k_basis_rbf(RbfDev M, int64_t P, const double* __restrict__ lat,
                                                     const double* __restrict__ lon, const double* __restrict__ alt,
                                                     double* __restrict__ A, int64_t ld_p, int64_t ld_n)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    double X, Y, Z;
    geodetic2ecef(lat[p], lon[p], alt[p], X, Y, Z);
    const double* __restrict__ c = M.centers;
    for (int n = 0; n < M.N; ++n) {
        const double dx = X - c[3 * n], dy = Y - c[3 * n + 1], dz = Z - c[3 * n + 2];
        const double r2 = dx * dx + dy * dy + dz * dz;
        A[p * ld_p + (int64_t)n * ld_n] = exp(-r2 * M.inv_eps2);
    }
}

__global__ void k_transform_rbf(int64_t P, const double* __restrict__ lat, const double* __restrict__ lon,
                                const double* __restrict__ alt, double* X, double* Y, double* Z)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    geodetic2ecef(lat[p], lon[p], alt[p], X[p], Y[p], Z[p]);
}

template <int LCAP, int KCAP>
int launch_basis_sph(vi_model* m, int64_t P, const double* lat, const double* lon, const double* alt, double* A,
                     int64_t ld_p, int64_t ld_n)
{
    return vi_launch(k_basis_sph<LCAP, KCAP>, dim3(nblocks(P, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, m->sph, P, lat, lon, alt, A,
                     ld_p, ld_n);
}

}  // namespace

// ---------------------------------------------------------------------------------------------
extern "C" int vi_basis_f64(vi_model* m, int64_t P, const double* d_lat, const double* d_lon, const double* d_alt,
                            double* d_A, int64_t ld_p, int64_t ld_n)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_A, "null argument");
    VI_REQUIRE(P >= 0, "negative point count");
    if (P == 0) return VI_OK;
    VI_HIP(hipSetDevice(m->ctx->device));
    if (m->kind == VI_MODEL_SPHHARMLAG)
        return at_order_cap(m, "vi_basis_f64", [&](auto lc, auto kc) {
            return launch_basis_sph<lc, kc>(m, P, d_lat, d_lon, d_alt, d_A, ld_p, ld_n);
        });
    return vi_launch(k_basis_rbf, dim3(nblocks(P, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, m->rbf, P, d_lat, d_lon, d_alt, d_A,
                     ld_p, ld_n);
}

// The gradient kernels at the compiled order that holds the model's (at_grad_cap, vi_eval_host.h).
// whether the model has a gradient basis at all (else the error is set)
int grad_model_check(const vi_model* m, const char* who)
{
    if (m->kind != VI_MODEL_SPHHARMLAG || !m->sph.scale1 || !m->sph.nu) {
        vi_set_error("%s: only the sphharmlag model provides a gradient basis", who);
        return VI_ERR_UNSUPPORTED;
    }
    return VI_OK;
}

namespace {
template <int MODE, bool ENU>
int launch_grad_sph(vi_model* m, const char* who, int64_t P, const double* d_lat, const double* d_lon, const double* d_alt,
                    const double* d_C, const unsigned char* d_mask, double* d_G, int64_t ld_p, int64_t ld_c, int64_t ld_n)
{
    const int rc = grad_model_check(m, who);
    if (rc != VI_OK || P == 0) return rc;
    VI_HIP(hipSetDevice(m->ctx->device));
    return at_grad_cap(m, who, [&](auto lc, auto kc) {
        return vi_launch(k_grad_sph<lc, kc, MODE, ENU>, dim3(nblocks(P, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, m->sph, P, d_lat,
                         d_lon, d_alt, d_C, d_mask, d_G, ld_p, ld_c, ld_n);
    });
}
}  // namespace

// The planar gradient basis of Q points, G[(n*3 + c)*Q + q], in the frame asked for - vi_eval_grad_basis_f64's matrix, and that
// of a chunk of vi_eval_grad_cov_f64 and vi_eval_track_grad_cov_f64 (vi_track.hip).  mask: the hull's bytes for these points, or
// nullptr.
int launch_grad_resident(vi_model* m, const char* who, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                         const unsigned char* d_mask, int32_t frame, double* d_G)
{
    return with_flag(frame == VI_FRAME_ENU, [&](auto enu) -> int {
        return launch_grad_sph<GRAD_RESIDENT, enu>(m, who, Q, d_lat, d_lon, d_alt, nullptr, d_mask, d_G, 1, Q, 3 * Q);
    });
}

extern "C" int vi_grad_basis_f64(vi_model* m, int64_t P, const double* d_lat, const double* d_lon, const double* d_alt,
                                 double* d_G, int64_t ld_p, int64_t ld_c, int64_t ld_n)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_G, "null argument");
    VI_REQUIRE(P >= 0, "negative point count");
    return launch_grad_sph<GRAD_STORE, false>(m, "vi_grad_basis_f64", P, d_lat, d_lon, d_alt, nullptr, nullptr, d_G, ld_p, ld_c,
                                              ld_n);
}

// Gradient of the fitted parameter: out[q][c] = sum_n grad_basis[q][c][n] * C[n], c = z, theta, phi components
// (sphharmlag.py:148-184 contracted with one coefficient vector; the (Q, 3, N) array is never formed).
extern "C" int vi_eval_grad_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                const double* d_C, double* d_out)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_C && d_out, "null argument");
    VI_REQUIRE(Q >= 0, "negative point count");
    return launch_grad_sph<GRAD_CONTRACT, false>(m, "vi_eval_grad_f64", Q, d_lat, d_lon, d_alt, d_C, nullptr, d_out, 3, 1, 0);
}

// Standard error of the fitted parameter from the coefficient covariance: err[q] = sqrt(a_q^T dC a_q), a_q = basis row
// of point q (first-order error propagation; the `calcerr` output the reference's Estimate.__call__ advertises but never
// computes, estimate.py:139-145).  Chunks of points: basis tile A (K1), row-major, then the product and the row dot of the
// forms' library route (vi_forms_tile, vi_resident.hip).  2 N^2 flop per point: MFMA-bound.
extern "C" int vi_eval_err_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                               const double* d_dC, double* d_out)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_dC && d_out, "null argument");
    VI_REQUIRE(Q >= 0, "negative point count");
    if (Q == 0) return VI_OK;
    VI_HIP(hipSetDevice(m->ctx->device));
    const int N = m->N;
    const int64_t chunk = 1 << 16;
    void* ws = nullptr;
    int rc = vi_ctx_workspace(m->ctx, (size_t)2 * chunk * N * sizeof(double), &ws);
    if (rc != VI_OK) return rc;
    double* A = (double*)ws;
    double* B = A + chunk * N;
    return for_chunks(Q, chunk, [&](int64_t q0, int64_t qc) -> int {
        const int rc = vi_basis_f64(m, qc, d_lat + q0, d_lon + q0, d_alt + q0, A, N, 1);            // row-major (qc, N)
        if (rc != VI_OK) return rc;
        return vi_forms_tile(m->ctx, N, qc, A, d_dC, B, d_out + q0);
    });
}

extern "C" int vi_transform_f64(vi_model* m, int64_t P, const double* d_lat, const double* d_lon, const double* d_alt,
                                double* d_c0, double* d_c1, double* d_c2)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_c0 && d_c1 && d_c2, "null argument");
    if (P <= 0) return P == 0 ? VI_OK : VI_ERR_INVALID;
    VI_HIP(hipSetDevice(m->ctx->device));
    if (m->kind == VI_MODEL_SPHHARMLAG)
        return vi_launch(k_transform_sph, dim3(nblocks(P, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, m->sph, P, d_lat, d_lon, d_alt,
                         d_c0, d_c1, d_c2);
    return vi_launch(k_transform_rbf, dim3(nblocks(P, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, P, d_lat, d_lon, d_alt, d_c0, d_c1,
                     d_c2);
}

// ---- the RESIDENT basis of a grid that many timesteps are evaluated on (vi_eval_resident_f64 and the other entries of
// vi_resident.hip, which has the why): N x Q doubles assembled once by K1 (vi_basis_f64, basis-major so that every access is a
// contiguous run of points), the rows of points outside the hull set to NaN, so that the mask costs nothing afterwards: NaN
// times anything is NaN.
namespace {
__global__ void k_mask_basis(int64_t Q, int N, const unsigned char* __restrict__ mask, double* __restrict__ Y)
{
    const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (q >= Q || mask[q] != 0) return;
    const double nan = __builtin_nan("");
    for (int n = 0; n < N; ++n) Y[(int64_t)n * Q + q] = nan;
}
}  // namespace

// the second half of vi_eval_basis_f64: NaN into the columns of the basis matrix d_Y (N x Q) whose mask byte is 0
int mask_basis(vi_model* m, int64_t Q, const unsigned char* d_mask, double* d_Y)
{
    return vi_launch(k_mask_basis, dim3(nblocks(Q, 256)), dim3(256), 0, m->ctx->stream, Q, m->N, d_mask, d_Y);
}

namespace {
// the hull pass of a call: on the matrix cores (k_hull_mask_mx) unless VINTERP_HULL=fp32 asks for the packed-fp32 loop
void launch_hull_mask(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt, int F, double tol)
{
    static const bool fp32 = vi_env_is("VINTERP_HULL", "fp32");
    if (fp32)
        hipLaunchKernelGGL(k_hull_mask, dim3(nblocks(Q, BLOCK * HULL_PP)), dim3(BLOCK), 0, m->ctx->stream, Q, d_lat, d_lon, d_alt,
                           m->d_hull, F, tol, m->d_mask);
    else
        hipLaunchKernelGGL(k_hull_mask_mx<HULL_MX_PP>, dim3(nblocks(Q, BLOCK * HULL_MX_PP)), dim3(BLOCK), 0, m->ctx->stream, Q,
                           d_lat, d_lon, d_alt, m->d_hull, F, tol, m->d_mask);
}
}  // namespace

// Gets a call ready, the one routine that does: grows the model's hull, mask and coefficient buffers; builds the hull buffer from
// the F facet equations and m->d_coef from the `rows` coefficient rows of d_C (sphharmlag only: the RBF kernels read d_C as
// it is, their callers pass rows = 0) - in one launch where the call has both -; then, with F > 0, m->d_mask[q] <- 1 where point
// q passes the hull test, else 0.
int prepare_call(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt, const double* d_hull_eq,
                 int32_t F, double hull_tol, int64_t rows, const double* d_C)
{
    vi_ctx* c = m->ctx;
    const int N = m->N, K = m->sph.maxk, L2 = m->sph.maxl * m->sph.maxl;
    int rc = VI_OK;
    if (F > 0 && (rc = vi_grow(c, &m->d_hull, &m->hull_bytes, hull_buf_bytes((size_t)F))) != VI_OK) return rc;
    if (F > 0 && (rc = vi_grow(c, &m->d_mask, &m->mask_bytes, (size_t)Q)) != VI_OK) return rc;
    if (rows > 0 && (rc = vi_grow(c, &m->d_coef, &m->coef_bytes, (size_t)rows * N * sizeof(double))) != VI_OK) return rc;
    const unsigned coef_blocks = nblocks(rows * N, 256);
    if (F == 0 && rows == 0) return VI_OK;             // nothing to prepare, nothing launched
    if (F > 0 && rows > 0)
        hipLaunchKernelGGL(k_prep_hull_coef, dim3(HULL_PREP_BLOCKS + coef_blocks), dim3(256), 0, c->stream, (int)F, d_hull_eq,
                           m->d_hull, (int)rows, K, L2, d_C, m->sph.scale, m->d_coef);
    else if (F > 0)
        hipLaunchKernelGGL(k_prep_hull, dim3(HULL_PREP_BLOCKS), dim3(256), 0, c->stream, (int)F, d_hull_eq, m->d_hull);
    else if (rows > 0)
        hipLaunchKernelGGL(k_prep_coef, dim3(coef_blocks), dim3(256), 0, c->stream, (int)rows, K, L2, d_C, m->sph.scale, m->d_coef);
    VI_HIP(hipGetLastError());
    if (F > 0) {
        launch_hull_mask(m, Q, d_lat, d_lon, d_alt, (int)F, hull_tol);
        VI_HIP(hipGetLastError());
    }
    return VI_OK;
}

extern "C" int vi_eval_basis_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                 const double* d_hull_eq, int32_t F, double hull_tol, double* d_Y)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_Y, "null argument");
    VI_REQUIRE(Q >= 0 && F >= 0, "negative size");
    VI_REQUIRE_HULL(F, d_hull_eq);
    if (Q == 0) return VI_OK;
    int rc = vi_basis_f64(m, Q, d_lat, d_lon, d_alt, d_Y, 1, Q);
    if (rc != VI_OK || F == 0) return rc;
    rc = prepare_call(m, Q, d_lat, d_lon, d_alt, d_hull_eq, F, hull_tol, 0, nullptr);
    if (rc != VI_OK) return rc;
    return mask_basis(m, Q, m->d_mask, d_Y);
}

// The gradient basis of a resident grid: d_G[(n*3 + c)*Q + q], N x 3Q doubles, the matrix vi_eval_resident_f64 multiplies with
// the coefficients of many timesteps (Q -> 3Q).  Planar so that every 32-byte piece of K2r holds one component of four
// neighbouring points - dead exactly when the four are outside the hull - and every component of the product is a contiguous
// map.  The hull pass runs first: the kernel stores the NaNs itself and skips the chains of a wave without a point inside.
extern "C" int vi_eval_grad_basis_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                      const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame, double* d_G)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_G, "null argument");
    VI_REQUIRE(Q >= 0 && F >= 0, "negative size");
    VI_REQUIRE_HULL(F, d_hull_eq);
    VI_REQUIRE_FRAME(frame);
    if (Q > 0 && F > 0 && m->kind == VI_MODEL_SPHHARMLAG) {          // (the launcher refuses the other model)
        VI_HIP(hipSetDevice(m->ctx->device));
        const int rc = prepare_call(m, Q, d_lat, d_lon, d_alt, d_hull_eq, F, hull_tol, 0, nullptr);
        if (rc != VI_OK) return rc;
    }
    return launch_grad_resident(m, "vi_eval_grad_basis_f64", Q, d_lat, d_lon, d_alt, F > 0 ? m->d_mask : nullptr, frame, d_G);
}

// What the two gradient-covariance entries (vi_eval_grad_cov_f64 here, vi_eval_track_grad_cov_f64 in vi_track.hip) set up alike:
// the hull pass for all Q points, the chunk - vi_forms_chunk(N, 3), or the smaller one of the switch `chunk_env` -, and the
// context workspace: the planar gradient basis G of a chunk and, unless every chunk takes the kernels of vi_eval_resident.hip, the
// work space of the library route behind it without a gap (else nullptr) - A and B of vi_resident_gradcov, or with `records`
// what vi_records_gradcov asks for.  Each entry walks the chunks itself.
int gradcov_setup(vi_model* m, const char* chunk_env, bool records, int64_t Q, const double* d_lat, const double* d_lon,
                  const double* d_alt, const double* d_hull_eq, int32_t F, double hull_tol, GradcovChunks* k)
{
    VI_HIP(hipSetDevice(m->ctx->device));
    const int N = m->N;
    int rc = VI_OK;
    if (F > 0 && (rc = prepare_call(m, Q, d_lat, d_lon, d_alt, d_hull_eq, F, hull_tol, 0, nullptr)) != VI_OK) return rc;
    k->chunk = std::min(Q, test_chunk(chunk_env, vi_forms_chunk(N, 3), 1));
    const bool own = vi_eval_resident_gradcov_shape(N);
    return ws_carve(m->ctx, [&](ws_carver& w) {
        k->G = w.take<double>((size_t)3 * k->chunk * N);
        k->work = w.take<double>(own ? 0 : records ? vi_forms_work_doubles(N, 3, k->chunk) : (size_t)6 * k->chunk * N, 8);
        if (own) k->work = nullptr;
    });
}

// The gradient covariance of ONE covariance at arbitrary points, d_out[k*Q + q]: in chunks of points the planar gradient basis
// of the chunk (the launcher of vi_eval_grad_basis_f64: hull mask and frame on the device) goes into the context workspace,
// then K2c or the library path with T = 1 writes the chunk's six planes at their place in the (6, Q) result.
// VINTERP_GRADCOV_CHUNK: points per chunk (tests: several chunks at a small Q).
extern "C" int vi_eval_grad_cov_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                    const double* d_dC, const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame,
                                    double* d_out)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_dC && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && F >= 0, "negative size");
    VI_REQUIRE_HULL(F, d_hull_eq);
    VI_REQUIRE_FRAME(frame);
    int rc = grad_model_check(m, "vi_eval_grad_cov_f64");
    if (rc != VI_OK || Q == 0) return rc;
    GradcovChunks k;
    rc = gradcov_setup(m, "VINTERP_GRADCOV_CHUNK", false, Q, d_lat, d_lon, d_alt, d_hull_eq, F, hull_tol, &k);
    if (rc != VI_OK) return rc;
    return for_chunks(Q, k.chunk, [&](int64_t q0, int64_t qc) -> int {
        const int rc = launch_grad_resident(m, "vi_eval_grad_cov_f64", qc, d_lat + q0, d_lon + q0, d_alt + q0,
                                            F > 0 ? m->d_mask + q0 : nullptr, frame, k.G);
        if (rc != VI_OK) return rc;
        EvalTimer timer(m->ctx);
        return vi_resident_gradcov(m, qc, 1, k.G, d_dC, d_out + q0, Q, k.work);
    });
}
