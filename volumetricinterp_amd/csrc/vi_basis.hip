// Basis-function kernels for gfx950: geodetic -> model coordinates, Laguerre x spherical-cap
// harmonics (reference: volumetricinterp/models/sphharmlag.py:118-145, :324-359) and Gaussian RBF
// (reference: volumetricinterp/models/radbasfun.py:83-112), as
//   K1  k_basis_*  : materialise A (used by the fit),
//   K2  k_eval_*   : fused evaluation  out[t,q] = sum_n A[q,n] C[t,n]  (Estimate.__call__,
//                    estimate.py:110-123) that never writes A, with the convex-hull test fused in: a unit of its own,
//                    vi_eval.hip; here are its hull pass and call preparation and its kin along tracks and rays.
// One thread per point; lat/lon/alt are read as coalesced SoA streams; every table the 64 lanes of
// a wave share (recurrence coefficients, coefficient tiles) is addressed wave-uniformly so it is
// served by the scalar data path / LDS broadcast and never costs per-lane HBM traffic.
#include "vi_chain_device.h"
#include "vi_eval_host.h"

#include <algorithm>
#include <cstdlib>

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

// F[3 i + c] = (east, north, up)_i . (model direction z, theta, phi)_c at the point.  The local geodetic unit vectors are
// rotated as sph_geom rotates the position (Rodrigues, +theta0) and meet the unit vectors of the rotated spherical coordinates
// there: r' = (s c_phi, s s_phi, x), theta' = (x c_phi, x s_phi, -s), phi' = (-s_phi, c_phi, 0) with s = rho / r.  `up` is the
// geodetic normal, not the radial direction.
__device__ __forceinline__ void enu_frame(const SphDev& M, const Geom& g, double lat, double lon, double* F)
{
    double sl, cl, so, co;
    sincos(lat * DEG2RAD, &sl, &cl);
    sincos(lon * DEG2RAD, &so, &co);
    const double enu[3][3] = {{-so, co, 0.0}, {-sl * co, -sl * so, cl}, {cl * co, cl * so, sl}};
    const double st = sqrt(g.Rx * g.Rx + g.Ry * g.Ry) / (M.RE * (g.z / 100.0 + 1.0));
    const double omc = 1.0 - M.rc;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double vx = enu[i][0], vy = enu[i][1], vz = enu[i][2];
        const double kd = M.kx * vx + M.ky * vy;
        const double wx = vx * M.rc + (M.ky * vz) * M.rs + M.kx * kd * omc;
        const double wy = vy * M.rc + (-M.kx * vz) * M.rs + M.ky * kd * omc;
        const double wz = vz * M.rc + (M.kx * vy - M.ky * vx) * M.rs;
        const double wh = wx * g.cphi + wy * g.sphi;            // component along the horizontal direction of azimuth phi'
        F[3 * i] = st * wh + g.x * wz;
        F[3 * i + 1] = g.x * wh - st * wz;
        F[3 * i + 2] = wy * g.cphi - wx * g.sphi;
    }
}

// The chains of the gradient basis at one point, the one copy k_grad_sph and K2tg (k_track_grad_sph) instantiate:
// sink.term(n, tz, tt, tp, L0k, L1k) is called once per basis function n = k L2 + r; its three gradient components at the point
// are tz (L0k + 2 L1k), tt L0k and tp L0k - handed over as factors, so that k_grad_sph's sink forms them where that kernel did.
template <int LCAP, int KCAP, class Sink>
__device__ __forceinline__ void grad_point(const SphDev& M, const Geom& g, Sink& sink)
{
    const int maxl = M.maxl, maxk = M.maxk, L2 = maxl * maxl;
    double L0[KCAP], L1[KCAP];          // L_k(z) and L^(1)_{k-1}(z)
    laguerre<KCAP>(maxk, g.z, L0);
    L1[0] = 0.0;                        // eval_genlaguerre(-1, 1, z) = 0
    if (KCAP > 1) L1[1] = 1.0;
    if (KCAP > 2) L1[2] = 2.0 - g.z;
#pragma unroll
    for (int k = 3; k < KCAP; ++k) {    // n L^(1)_n = (2n - z) L^(1)_{n-1} - n L^(1)_{n-2},  n = k-1
        const int n = k - 1;
        L1[k] = ((2.0 * n - g.z) * L1[k - 1] - (double)n * L1[k - 2]) / (double)n;
    }
    const double e = exp(-0.5 * g.z);
    const double x = g.x, y = g.s;
    const double inv_hr = 1.0 / (y * (g.z / 100.0 + 1.0) * M.RE);       // 1 / (y (z/100+1) RE)
    const double zfac = -0.5 * e * 100.0 / M.RE;
    double cm[LCAP], sm[LCAP];
    cm[0] = 1.0;
    sm[0] = 0.0;
#pragma unroll
    for (int m = 1; m < LCAP; ++m) {
        cm[m] = cm[m - 1] * g.cphi - sm[m - 1] * g.sphi;
        sm[m] = sm[m - 1] * g.cphi + cm[m - 1] * g.sphi;
    }
    const double zz = 0.5 * (1.0 - x);
    for (int gi = 0; gi < M.ngroups; ++gi) {
        const SphGroupDev G = M.groups[gi];
        const bool intseed = (G.nterms == 0);
        double cur[LCAP], prev[LCAP];
#pragma unroll
        for (int m = 0; m < LCAP; ++m) { cur[m] = 0.0; prev[m] = 0.0; }
        double pmm = 1.0, spow = 1.0;
        for (int j = 0; j <= G.nvmax + 1; ++j) {
            const double* __restrict__ cj = G.c + (size_t)j * maxl;
#pragma unroll
            for (int m = 0; m < LCAP; ++m) {
                if (m < maxl) {
                    if (j > m + 1) {
                        const double nw = fma(x, cur[m], -(cj[m] * prev[m]));
                        prev[m] = cur[m];
                        cur[m] = nw;
                    } else if (j == m) {
                        if (m > 0) { pmm *= -(2.0 * m - 1.0) * g.s; spow *= g.s; }
                        if (intseed) cur[m] = pmm;
                        else cur[m] = G.pref[m] * spow * hyp_series(G.q + (size_t)m * G.nterms, G.nterms, zz);
                    } else if (j == m + 1) {
                        prev[m] = cur[m];
                        if (intseed) cur[m] = x * (2.0 * m + 1.0) * cur[m];
                        else cur[m] = G.pref[maxl + m] * spow *
                                      hyp_series(G.q + (size_t)(maxl + m) * G.nterms, G.nterms, zz);
                    }
                }
            }
            const int l = j >= 1 ? G.pick[j - 1] : -1;      // degree nu_l + 1 reached
            if (l >= 0) {
                const int r0 = l * (l + 1);
                const double v = M.nu[l];
#pragma unroll
                for (int m = 0; m < LCAP; ++m) {
                    if (m <= l) {
#pragma unroll
                        for (int sgn = 0; sgn < 2; ++sgn) {
                            if (sgn == 1 && m == 0) continue;
                            const int r = sgn ? r0 - m : r0 + m;
                            const double ms = sgn ? -(double)m : (double)m;            // signed order
                            const double Q0 = M.scale[r] * prev[m];                      // Kvm * lpmv(m, v, x)
                            const double Q1 = M.scale1[r] * cur[m];                      // Kvm * lpmv(m, v+1, x)
                            const double trig = sgn ? sm[m] : cm[m];
                            const double dtrig = sgn ? (double)m * cm[m] : -(double)m * sm[m];
                            const double tz = zfac * Q0 * trig;
                            const double tt = e * (-(v + 1.0) * x * Q0 + (v - ms + 1.0) * Q1) * trig * inv_hr;
                            const double tp = e * Q0 * dtrig * inv_hr;
#pragma unroll
                            for (int k = 0; k < KCAP; ++k)
                                if (k < maxk) sink.term(k * L2 + r, tz, tt, tp, L0[k], L1[k]);
                        }
                    }
                }
            }
        }
    }
}

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

// One pass of the chains of a point over the tile E.shC, for K2t (k_track_sph_fast below): E.acc[t] = sum_n basis_n(point) *
// tile[t][n] without the factor exp(-z/2), t = 0 .. TT-1.  shc: the recurrence table [nj][L] in LDS, nvl[l]: the degree at which
// chain segment l ends.  The contraction, the start-up's consumption and the main segments are the pieces k_eval_sph_fast runs
// (FastEval, ConsumeAt, MainSegments); the triangular start-up around them is written out here as it is in that kernel, which
// keeps its own: calling this function from it changed the register allocation of most of its instantiations (e.g. (6, 4) at
// TT = 1: 95 -> 99 VGPRs, five -> four waves per SIMD), and that kernel is on the benchmarked path.
template <int L, int K, int TT, typename CT>
__device__ __forceinline__ void fast_chains(FastEval<L, K, TT>& E, const SphGroupDev& G, const Geom& g, const CT* shc,
                                            const int* nvl, int nj)
{
    laguerre<K>(K, g.z, E.Lk);
#pragma unroll
    for (int t = 0; t < TT; ++t) E.acc[t] = 0.0;
    double cm[L], sm[L];
    cm[0] = 1.0;
    sm[0] = 0.0;
#pragma unroll
    for (int m = 1; m < L; ++m) {
        cm[m] = cm[m - 1] * g.cphi - sm[m - 1] * g.sphi;
        sm[m] = sm[m - 1] * g.cphi + cm[m - 1] * g.sphi;
    }
    const CT x = (CT)g.x;
    const double zz = 0.5 * (1.0 - g.x);
    const bool intseed = (G.nterms == 0);
    CT cur[L], prev[L];
#pragma unroll
    for (int m = 0; m < L; ++m) { cur[m] = (CT)0.0; prev[m] = (CT)0.0; }
    double pmm = 1.0, spow = 1.0;
    // ---- start-up: degrees j = 0 .. L, compile-time triangular structure ------------------------------
#pragma unroll
    for (int j = 0; j <= L; ++j) {
#pragma unroll
        for (int m = 0; m < L; ++m) {
            if (j > m + 1) {
                if (j < nj) {
                    const CT nw = fma(x, cur[m], -(shc[j * L + m] * prev[m]));
                    prev[m] = cur[m];
                    cur[m] = nw;
                }
            } else if (j == m) {
                if (m > 0) { pmm *= -(2.0 * m - 1.0) * g.s; spow *= g.s; }
                if (intseed) cur[m] = (CT)pmm;
                else cur[m] = (CT)(G.pref[m] * spow * hyp_series(G.q + (size_t)m * G.nterms, G.nterms, zz));
            } else if (j == m + 1) {
                prev[m] = cur[m];
                if (intseed) cur[m] = (CT)(g.x * (2.0 * m + 1.0) * pmm);
                else cur[m] = (CT)(G.pref[L + m] * spow * hyp_series(G.q + (size_t)(L + m) * G.nterms, G.nterms, zz));
            }
        }
        ConsumeAt<L, FastEval<L, K, TT>, 0>::run(E, nvl, j, cur, cm, sm);
    }
    // ---- main: all chains in recurrence mode; one segment per degree l --------------------------------
    int j = L + 1;
    MainSegments<L, FastEval<L, K, TT>, 0>::run(E, shc, nvl, j, x, cur, prev, cm, sm);
}

// ---------------------------------------------------------------------------------------------
// K2t: densities along a trajectory, every point at its own time (vi_eval_track_f64).  Point q takes prepared coefficient row
// rec[q] (nearest mode) or the blend (1 - w[q]) D(rec[q]) + w[q] D(rec[q] + 1) of the densities D of two neighbouring rows.
// The unit is a workgroup of ONE wave (64 points) with its own tile: the wave finds the lowest and highest row its live lanes
// need (shuffles over rec: nothing assumes sorted input), stages the window of TT prepared rows from the lowest one in LDS -
// rows past R - 1 zero-filled, never read - and runs the chains of k_eval_sph_fast once for TT accumulators; the epilogue takes
// each lane's own accumulator (two neighbours when blending) by an unrolled compare-select, never a product with zero: a NaN
// row touches no other row's points.  Where the wave's rows span more than a window the pass is repeated from the next window
// - consecutive windows share one row when blending, so that every pair (rec, rec + 1) lies inside one - until the highest row
// is covered; a lane keeps the value of the one pass whose window holds its rows.  With the points sorted by record the spans
// of all waves add up to at most R + (number of waves), so the passes beyond one per wave are at most about R / (TT - 1) wave
// passes in total, whatever Q is; unsorted input is correct and costs up to R / (TT - 1) passes per wave.  A wave without a
// live lane (outside the hull, no record, rows past R - 1) leaves before the table is staged.  One wave per workgroup: the
// barriers around the staging are wave barriers, the windows follow the 64 points and not 256, and the LDS need is that of
// k_eval_sph_fast at the same TT, so the same orders fit.
constexpr int TRACK_BLOCK = 64;
constexpr int TRACK_TT = 4;         // the tile width: 3.9e10 / 4 point-rows per second against 1.4e10 at TT = 1 (launch_eval_sph_fast)

// what a point of a track needs to be computed at all: a record, its row(s) inside the R rows, inside the hull
__device__ __forceinline__ bool track_live(int64_t q, int64_t qc, int64_t Q, int r, int R, int pair,
                                           const unsigned char* __restrict__ mask, int F)
{
    return q < Q && r >= 0 && r <= R - 1 - pair && (F == 0 || mask[qc] != 0);
}

template <int L, int K, int TT, bool INTERP>
__global__ __launch_bounds__(TRACK_BLOCK) void k_track_sph_fast(SphDev M, int64_t Q, const double* __restrict__ lat,
                                                                const double* __restrict__ lon, const double* __restrict__ alt,
                                                                const int* __restrict__ rec, const double* __restrict__ wgt, int R,
                                                                const double* __restrict__ Cp,
                                                                const unsigned char* __restrict__ mask, int F,
                                                                double* __restrict__ out)
{
    constexpr int NB = L * L * K;
    constexpr int PAIR = INTERP ? 1 : 0;
    constexpr int STEP = TT - PAIR;                     // rows from one window to the next
    static_assert(STEP >= 1, "a blending window holds at least two rows");
    extern __shared__ __align__(16) double sh[];
    const int64_t q = (int64_t)blockIdx.x * TRACK_BLOCK + threadIdx.x;
    const int64_t qc = q < Q ? q : Q - 1;
    const int r = rec[qc];
    const bool live = track_live(q, qc, Q, r, R, PAIR, mask, F);
    if (!__any(live)) {                                 // (the whole workgroup: no barrier has been met)
        if (q < Q) out[q] = __builtin_nan("");
        return;
    }
    int lo = live ? r : 0x7fffffff, hi = live ? r + PAIR : -1;
#pragma unroll
    for (int off = TRACK_BLOCK / 2; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, TRACK_BLOCK));
        hi = max(hi, __shfl_xor(hi, off, TRACK_BLOCK));
    }
    lo = __builtin_amdgcn_readfirstlane(lo);            // 0 <= lo <= hi <= R - 1
    hi = __builtin_amdgcn_readfirstlane(hi);
    const SphGroupDev G = M.groups[0];
    const int nj = G.nvmax + 1;
    double* shc = sh;                                   // [nj][L] recurrence table
    double* shC = sh + ((nj * L + 1) & ~1);             // [TT][NB] the window
    int* nvl = reinterpret_cast<int*>(shC + TT * NB);   // [L]
    for (int i = threadIdx.x; i < nj * L; i += TRACK_BLOCK) shc[i] = G.c[i];
    for (int j = threadIdx.x; j < nj; j += TRACK_BLOCK) {
        const int l = G.pick[j];
        if (l >= 0) nvl[l] = j;
    }
    const Geom g = sph_geom(M, lat[qc], lon[qc], alt[qc]);
    const double Ez = exp(-0.5 * g.z);
    const double w = INTERP ? wgt[qc] : 0.0;
    double val = __builtin_nan("");
    for (int base = lo;; base += STEP) {
        __syncthreads();                                // the pass before has read the window
        for (int i = threadIdx.x; i < TT * NB; i += TRACK_BLOCK)
            shC[i] = i / NB < R - base ? Cp[(int64_t)base * NB + i] : 0.0;
        __syncthreads();
        FastEval<L, K, TT> E;
        E.shC = shC;
        fast_chains<L, K, TT, double>(E, G, g, shc, nvl, nj);
        const int d = live ? r - base : -1;             // the lane's row in this window
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            if (d == t) a = E.acc[t];
            if (INTERP && d + 1 == t) b = E.acc[t];
        }
        if (d >= 0 && d < STEP) val = INTERP ? (1.0 - w) * (Ez * a) + w * (Ez * b) : Ez * a;
        if (hi - base <= TT - 1) break;                 // wave-uniform
    }
    if (q < Q) out[q] = live ? val : __builtin_nan("");
}

// The per-lane form for the orders without a fast kernel (and VINTERP_EVAL=generic): the generic sink reads the lane's own
// prepared row, or its two rows, from global memory.  Correct, not tuned.
template <int LCAP, int KCAP, bool INTERP>
__global__ __launch_bounds__(BLOCK) void k_track_sph(SphDev M, int64_t Q, const double* __restrict__ lat,
                                                     const double* __restrict__ lon, const double* __restrict__ alt,
                                                     const int* __restrict__ rec, const double* __restrict__ wgt, int R,
                                                     const double* __restrict__ Cp, const unsigned char* __restrict__ mask,
                                                     int F, double* __restrict__ out)
{
    constexpr int TT = INTERP ? 2 : 1;
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t qc = q < Q ? q : Q - 1;
    const int r = rec[qc];
    const bool live = track_live(q, qc, Q, r, R, TT - 1, mask, F);
    if (!__any(live)) {
        if (q < Q) out[q] = __builtin_nan("");
        return;
    }
    const Geom g = sph_geom(M, lat[qc], lon[qc], alt[qc]);
    double v[TT];
    eval_point<LCAP, KCAP, TT>(M, g, Cp + (int64_t)(live ? r : 0) * M.N, v);      // (a live lane exists: row 0 does)
    double val = v[0];
    if (INTERP) {
        const double w = wgt[qc];
        val = (1.0 - w) * val + w * v[TT - 1];
    }
    if (q < Q) out[q] = live ? val : __builtin_nan("");
}

// ---------------------------------------------------------------------------------------------
// K2tg: gradients along a trajectory, every point at its own time (vi_eval_track_grad_f64): k_grad_sph's chains (grad_point) in
// K2t's frame.  A workgroup is ONE wave of 64 points; it finds the lowest and highest row its live lanes need (shuffles: nothing
// assumes sorted input) and stages a window of TT RAW coefficient rows from the lowest one in LDS - the gradient needs
// scale[r] P(nu) and scale1[r] P(nu + 1), so the rows k_prep_coef prepares for the density do not serve; rows past R - 1 are
// zero-filled and never selected - then runs the chains once for 3 TT accumulators, the coefficients read from LDS at
// wave-uniform addresses.  Each lane takes the triple of its own row (the pair of triples, when blending) by compare-select,
// never a product with zero, from the one window that holds its rows; windows follow each other as in K2t (one shared row when
// blending) until the wave's highest row is covered.  Every row's accumulators see the terms in the order k_grad_sph adds them,
// whatever the row's place in the window: a point's bits depend on the point, its row(s) and w only.  With ENU the point's
// matrix (enu_frame) turns the finished triple in the epilogue.  A wave without a live lane leaves before anything is staged.
constexpr int TRACK_GRAD_TT = 4;    // the window

template <int TT>
struct GradTrackSink {
    const double* shC;      // LDS [TT][N], raw rows
    int N;
    double az[TT], at[TT], ap[TT];
    __device__ __forceinline__ void term(int n, double tz, double tt, double tp, double L0k, double L1k)
    {
        const double gz = tz * (L0k + 2.0 * L1k), gt = tt * L0k, gp = tp * L0k;
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            const double cf = shC[t * N + n];
            az[t] = fma(gz, cf, az[t]);
            at[t] = fma(gt, cf, at[t]);
            ap[t] = fma(gp, cf, ap[t]);
        }
    }
};

template <int LCAP, int KCAP, int TT, bool INTERP, bool ENU>
__global__ __launch_bounds__(TRACK_BLOCK) void k_track_grad_sph(SphDev M, int64_t Q, const double* __restrict__ lat,
                                                                const double* __restrict__ lon, const double* __restrict__ alt,
                                                                const int* __restrict__ rec, const double* __restrict__ wgt, int R,
                                                                const double* __restrict__ C,
                                                                const unsigned char* __restrict__ mask, int F,
                                                                double* __restrict__ out)
{
    constexpr int PAIR = INTERP ? 1 : 0;
    constexpr int STEP = TT - PAIR;                     // rows from one window to the next
    static_assert(STEP >= 1, "a blending window holds at least two rows");
    extern __shared__ __align__(16) double sh[];        // [TT][N] the window
    const double nan = __builtin_nan("");
    const int64_t q = (int64_t)blockIdx.x * TRACK_BLOCK + threadIdx.x;
    const int64_t qc = q < Q ? q : Q - 1;
    const int r = rec[qc];
    const bool live = track_live(q, qc, Q, r, R, PAIR, mask, F);
    if (!__any(live)) {                                 // (the whole workgroup: no barrier has been met)
        if (q < Q) out[3 * q] = out[3 * q + 1] = out[3 * q + 2] = nan;
        return;
    }
    int lo = live ? r : 0x7fffffff, hi = live ? r + PAIR : -1;
#pragma unroll
    for (int off = TRACK_BLOCK / 2; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, TRACK_BLOCK));
        hi = max(hi, __shfl_xor(hi, off, TRACK_BLOCK));
    }
    lo = __builtin_amdgcn_readfirstlane(lo);            // 0 <= lo <= hi <= R - 1
    hi = __builtin_amdgcn_readfirstlane(hi);
    const int N = M.N;
    const Geom g = sph_geom(M, lat[qc], lon[qc], alt[qc]);
    const double w = INTERP ? wgt[qc] : 0.0;
    double vz = nan, vt = nan, vp = nan;
    for (int base = lo;; base += STEP) {                // lo <= base <= hi
        __syncthreads();                                // the pass before has read the window
        for (int i = threadIdx.x; i < TT * N; i += TRACK_BLOCK) sh[i] = i / N < R - base ? C[(int64_t)base * N + i] : 0.0;
        __syncthreads();
        GradTrackSink<TT> S;
        S.shC = sh;
        S.N = N;
#pragma unroll
        for (int t = 0; t < TT; ++t) S.az[t] = S.at[t] = S.ap[t] = 0.0;
        grad_point<LCAP, KCAP>(M, g, S);
        const int d = live ? r - base : -1;             // the lane's row in this window
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            if (d == t) { a0 = S.az[t]; a1 = S.at[t]; a2 = S.ap[t]; }
            if (INTERP && d + 1 == t) { b0 = S.az[t]; b1 = S.at[t]; b2 = S.ap[t]; }
        }
        if (d >= 0 && d < STEP) {
            vz = INTERP ? (1.0 - w) * a0 + w * b0 : a0;
            vt = INTERP ? (1.0 - w) * a1 + w * b1 : a1;
            vp = INTERP ? (1.0 - w) * a2 + w * b2 : a2;
        }
        if (hi - base <= TT - 1) break;                 // wave-uniform
    }
    if (ENU) {
        double Fm[9];
        enu_frame(M, g, lat[qc], lon[qc], Fm);
        const double gz = vz, gt = vt, gp = vp;
        vz = fma(Fm[0], gz, fma(Fm[1], gt, Fm[2] * gp));
        vt = fma(Fm[3], gz, fma(Fm[4], gt, Fm[5] * gp));
        vp = fma(Fm[6], gz, fma(Fm[7], gt, Fm[8] * gp));
    }
    if (q < Q) {
        out[3 * q] = live ? vz : nan;
        out[3 * q + 1] = live ? vt : nan;
        out[3 * q + 2] = live ? vp : nan;
    }
}

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
    for (int i = threadIdx.x; i < nj * L; i += blockDim.x) shc[i] = G.c[i];
    for (int j = threadIdx.x; j < nj; j += blockDim.x) {
        const int l = G.pick[j];
        if (l >= 0) nvl[l] = j;
    }
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
    if (!y.live) {
        if (p < P && lane == 0) out[p] = __builtin_nan("");
        return;
    }
    double acc = 0.0;
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += 64) {
        // a pass reads the table and the row as the one-pass kernel does: nothing is carried in registers from pass to pass
        // (left to hoist the loop-invariant LDS and table reads, the compiler spends 50 VGPRs - a wave per SIMD or two - on them)
        asm volatile("" ::: "memory");
        const int i = i0 + lane;
        const bool on = i < n;
        double X, Y, Z;
        slant_node(y, xq[on ? i : 0], X, Y, Z);
        const Geom g = sph_geom_ecef(M, X, Y, Z);
        FastEval<L, K, 1> E;
        E.shC = shC;
        fast_chains<L, K, 1, double>(E, G, g, shc, nvl, nj);
        const double term = wq[on ? i : 0] * (exp(-0.5 * g.z) * E.acc[0]);
        acc += on ? term : 0.0;
    }
    const double val = slant_sum(y, acc);
    if (lane == 0) out[p] = val;
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
    constexpr int TT = INTERP ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * (BLOCK / 64) + wave_index();
    const SlantRay y = slant_ray(p, P, a, b, rec, R, TT - 1, eq, F, tol, chord);
    if (!y.live) {
        if (p < P && lane == 0) out[p] = __builtin_nan("");
        return;
    }
    const double w = INTERP ? wgt[p] : 0.0;
    double acc = 0.0;
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool on = i < n;
        double X, Y, Z;
        slant_node(y, xq[on ? i : 0], X, Y, Z);
        const Geom g = sph_geom_ecef(M, X, Y, Z);
        double v[TT];
        eval_point<LCAP, KCAP, TT>(M, g, Cp + (int64_t)y.r * M.N, v);
        double val = v[0];
        if (INTERP) val = (1.0 - w) * val + w * v[TT - 1];
        const double term = wq[on ? i : 0] * val;
        acc += on ? term : 0.0;
    }
    const double val = slant_sum(y, acc);
    if (lane == 0) out[p] = val;
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
#pragma unroll 1
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const bool on = i < n;
            double X, Y, Z;
            slant_node(y, xq[on ? i : 0], X, Y, Z);
            const Geom g = sph_geom_ecef(M, X, Y, Z);
            double Lk[KCAP];
            laguerre<KCAP>(M.maxk, g.z, Lk);
            const double E = exp(-0.5 * g.z);
#pragma unroll
            for (int k = 0; k < KCAP; ++k) sink.ELk[k] = k < M.maxk ? E * Lk[k] : 0.0;
            const double w = wq[on ? i : 0];
            sink.wgt = on ? w : 0.0;            // the lanes past n run node 0 again and add nothing
            sph_point<LCAP, KCAP>(M, g, sink);
        }
    }
    rayb_finish(y, sh, N, waves, wave, P, Yo);
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

// K2t for the RBF model, per lane: the lane's own coefficient row, or its two rows, from global memory (see k_track_sph)
template <bool INTERP>
__global__ __launch_bounds__(BLOCK) void k_track_rbf(RbfDev M, int64_t Q, const double* __restrict__ lat,
                                                     const double* __restrict__ lon, const double* __restrict__ alt,
                                                     const int* __restrict__ rec, const double* __restrict__ wgt, int R,
                                                     const double* __restrict__ C, const unsigned char* __restrict__ mask, int F,
                                                     double* __restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t qc = q < Q ? q : Q - 1;
    const int r = rec[qc];
    const bool live = track_live(q, qc, Q, r, R, INTERP ? 1 : 0, mask, F);
    if (!__any(live)) {
        if (q < Q) out[q] = __builtin_nan("");
        return;
    }
    double X, Y, Z;
    geodetic2ecef(lat[qc], lon[qc], alt[qc], X, Y, Z);
    double a, b;
    rbf_rows<INTERP>(M, C + (int64_t)(live ? r : 0) * M.N, X, Y, Z, a, b);      // (a live lane exists: row 0 does)
    double val = a;
    if (INTERP) {
        const double w = wgt[qc];
        val = (1.0 - w) * a + w * b;
    }
    if (q < Q) out[q] = live ? val : __builtin_nan("");
}

// K2l for the RBF model: a wave per ray, a lane per node, the ray's coefficient row(s) from global memory (see k_slant_sph)
template <bool INTERP>
__global__ __launch_bounds__(BLOCK) void k_slant_rbf(RbfDev M, int64_t P, const double* __restrict__ a, const double* __restrict__ b,
                                                     const int* __restrict__ rec, const double* __restrict__ wgt, int R,
                                                     const double* __restrict__ C, const double* __restrict__ eq, int F, double tol,
                                                     int n, const double* __restrict__ xq, const double* __restrict__ wq,
                                                     double* __restrict__ out, double* __restrict__ chord)
{
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * (BLOCK / 64) + wave_index();
    const SlantRay y = slant_ray(p, P, a, b, rec, R, INTERP ? 1 : 0, eq, F, tol, chord);
    if (!y.live) {
        if (p < P && lane == 0) out[p] = __builtin_nan("");
        return;
    }
    const double w = INTERP ? wgt[p] : 0.0;
    const double* __restrict__ Cr = C + (int64_t)y.r * M.N;
    double acc = 0.0;
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool on = i < n;
        double X, Y, Z;
        slant_node(y, xq[on ? i : 0], X, Y, Z);
        double va, vb;
        rbf_rows<INTERP>(M, Cr, X, Y, Z, va, vb);
        const double val = INTERP ? (1.0 - w) * va + w * vb : va;
        const double term = wq[on ? i : 0] * val;
        acc += on ? term : 0.0;
    }
    const double val = slant_sum(y, acc);
    if (lane == 0) out[p] = val;
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
#pragma unroll 1
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const bool on = i < n;
            double X, Y, Z;
            slant_node(y, xq[on ? i : 0], X, Y, Z);
            const double w = wq[on ? i : 0];
            const double wgt = on ? w : 0.0;
            for (int k0 = 0; k0 < N; k0 += TR) {
#pragma unroll
                for (int j = 0; j < TR; ++j) {
                    const int k = k0 + j < N ? k0 + j : N - 1;
                    tile[j * RAYB_LD + lane] = wgt * rbf_gauss(M, k, X, Y, Z);
                }
                rayb_sum<TR>(tile, acc, waves, [&](int r) { return k0 + r < N ? k0 + r : -1; });
            }
        }
    }
    rayb_finish(y, sh, N, waves, wave, P, Yo);
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
    hipLaunchKernelGGL((k_basis_sph<LCAP, KCAP>), dim3(nblocks(P, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, m->sph, P,
                       lat, lon, alt, A, ld_p, ld_n);
    VI_HIP(hipGetLastError());
    return VI_OK;
}

// K2t launches (vi_eval_track_f64): w == nullptr is nearest mode.  Cp: the R prepared rows.
template <int L, int K>
int launch_track_sph_fast(vi_model* m, int64_t Q, const double* lat, const double* lon, const double* alt, const int* rec,
                          const double* w, int R, const double* Cp, const unsigned char* hull, int F, double* out)
{
    const size_t shm = chain_lds_bytes(m->nvmax0 + 1, L, (size_t)TRACK_TT * m->N);
    return with_flag(w != nullptr, [&](auto interp) -> int {
        VI_HIP(hipFuncSetAttribute((const void*)k_track_sph_fast<L, K, TRACK_TT, interp>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   64 * 1024));
        hipLaunchKernelGGL((k_track_sph_fast<L, K, TRACK_TT, interp>), dim3(nblocks(Q, TRACK_BLOCK)), dim3(TRACK_BLOCK), shm,
                           m->ctx->stream, m->sph, Q, lat, lon, alt, rec, w, R, Cp, hull, F, out);
        VI_HIP(hipGetLastError());
        return VI_OK;
    });
}

template <int LCAP, int KCAP>
int launch_track_sph(vi_model* m, int64_t Q, const double* lat, const double* lon, const double* alt, const int* rec,
                     const double* w, int R, const double* Cp, const unsigned char* hull, int F, double* out)
{
    return with_flag(w != nullptr, [&](auto interp) -> int {
        hipLaunchKernelGGL((k_track_sph<LCAP, KCAP, interp>), dim3(nblocks(Q, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, m->sph, Q,
                           lat, lon, alt, rec, w, R, Cp, hull, F, out);
        VI_HIP(hipGetLastError());
        return VI_OK;
    });
}

// K2l launches (vi_eval_slant_f64): w == nullptr is nearest mode.  Cp: the R prepared rows.
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

template <int L, int K>
int launch_slant_sph_fast(vi_model* m, const SlantArgs& s, const double* Cp)
{
    // as many rays in a workgroup as the LDS holds rows beside the table: SLANT_WAVES, fewer at the orders whose table and row
    // fill most of it (one always fits: fast_eval_fits(m, 1))
    int waves = SLANT_WAVES;
    while (waves > 1 && chain_lds_bytes(m->nvmax0 + 1, L, (size_t)waves * m->N) > 64 * 1024) waves >>= 1;
    const size_t shm = chain_lds_bytes(m->nvmax0 + 1, L, (size_t)waves * m->N);
    return with_flag(s.w != nullptr, [&](auto interp) -> int {
        VI_HIP(hipFuncSetAttribute((const void*)k_slant_sph_fast<L, K, interp>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   64 * 1024));
        hipLaunchKernelGGL((k_slant_sph_fast<L, K, interp>), dim3(nblocks(s.P, waves)), dim3(waves * 64), shm, m->ctx->stream,
                           m->sph, s.P, s.a, s.b, s.rec, s.w, s.R, Cp, s.eq, s.F, s.tol, s.n, s.xq, s.wq, s.out, s.chord);
        VI_HIP(hipGetLastError());
        return VI_OK;
    });
}

template <int LCAP, int KCAP>
int launch_slant_sph(vi_model* m, const SlantArgs& s, const double* Cp)
{
    return with_flag(s.w != nullptr, [&](auto interp) -> int {
        hipLaunchKernelGGL((k_slant_sph<LCAP, KCAP, interp>), dim3(nblocks(s.P, BLOCK / 64)), dim3(BLOCK), 0, m->ctx->stream, m->sph,
                           s.P, s.a, s.b, s.rec, s.w, s.R, Cp, s.eq, s.F, s.tol, s.n, s.xq, s.wq, s.out, s.chord);
        VI_HIP(hipGetLastError());
        return VI_OK;
    });
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
    hipLaunchKernelGGL(k_basis_rbf, dim3(nblocks(P, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, m->rbf, P, d_lat, d_lon,
                       d_alt, d_A, ld_p, ld_n);
    VI_HIP(hipGetLastError());
    return VI_OK;
}

// The gradient kernels at the compiled order that holds the model's: (MAXL, MAXK) up to (6, 4), (12, 8) or (2, 12).
namespace {
// whether the model has a gradient basis at all (else the error is set)
int grad_model_check(const vi_model* m, const char* who)
{
    if (m->kind != VI_MODEL_SPHHARMLAG || !m->sph.scale1 || !m->sph.nu) {
        vi_set_error("%s: only the sphharmlag model provides a gradient basis", who);
        return VI_ERR_UNSUPPORTED;
    }
    return VI_OK;
}

// f(integral_constant LCAP, KCAP) at the first of those orders that holds the model's
template <class F>
int at_grad_cap(const vi_model* m, const char* who, F&& f)
{
    const int L = m->sph.maxl, K = m->sph.maxk;
#define VI_CAP(LC, KC) \
    if (L <= LC && K <= KC) return f(std::integral_constant<int, LC>{}, std::integral_constant<int, KC>{});
    VI_CAP(6, 4) VI_CAP(12, 8) VI_CAP(2, 12)
#undef VI_CAP
    vi_set_error("%s: order MAXL=%d MAXK=%d beyond the compiled limits (6, 4), (12, 8) and (2, 12)", who, L, K);
    return VI_ERR_UNSUPPORTED;
}

template <int MODE, bool ENU>
int launch_grad_sph(vi_model* m, const char* who, int64_t P, const double* d_lat, const double* d_lon, const double* d_alt,
                    const double* d_C, const unsigned char* d_mask, double* d_G, int64_t ld_p, int64_t ld_c, int64_t ld_n)
{
    const int rc = grad_model_check(m, who);
    if (rc != VI_OK || P == 0) return rc;
    VI_HIP(hipSetDevice(m->ctx->device));
    return at_grad_cap(m, who, [&](auto lc, auto kc) -> int {
        hipLaunchKernelGGL((k_grad_sph<lc, kc, MODE, ENU>), dim3(nblocks(P, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, m->sph, P,
                           d_lat, d_lon, d_alt, d_C, d_mask, d_G, ld_p, ld_c, ld_n);
        VI_HIP(hipGetLastError());
        return VI_OK;
    });
}

// The planar gradient basis of Q points, G[(n*3 + c)*Q + q], in the frame asked for - vi_eval_grad_basis_f64's matrix, and that
// of a chunk of vi_eval_grad_cov_f64 and vi_eval_track_grad_cov_f64.  mask: the hull's bytes for these points, or nullptr.
int launch_grad_resident(vi_model* m, const char* who, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                         const unsigned char* d_mask, int32_t frame, double* d_G)
{
    return with_flag(frame == VI_FRAME_ENU, [&](auto enu) -> int {
        return launch_grad_sph<GRAD_RESIDENT, enu>(m, who, Q, d_lat, d_lon, d_alt, nullptr, d_mask, d_G, 1, Q, 3 * Q);
    });
}

// A smaller chunk for a call from the switch `name` (tests: several chunks at a small point count), read at every call: its
// value rounded down to a multiple of `multiple`, taken where it is at least that and below `chunk`
int64_t test_chunk(const char* name, int64_t chunk, int multiple)
{
    if (const char* e = getenv(name)) {
        const long long v = atoll(e) / multiple * multiple;
        if (v >= multiple && v < chunk) chunk = v;
    }
    return chunk;
}

// K2tg launch (vi_eval_track_grad_f64): w == nullptr is nearest mode.  C: the R raw rows.
template <int LCAP, int KCAP>
int launch_track_grad_sph(vi_model* m, int64_t Q, const double* lat, const double* lon, const double* alt, const int* rec,
                          const double* w, int R, const double* C, const unsigned char* hull, int F, bool enu, double* out)
{
    const size_t shm = (size_t)TRACK_GRAD_TT * m->N * sizeof(double);       // at most 4 x 1152 doubles: 36 KB
    return with_flag(w != nullptr, [&](auto interp) -> int {
        return with_flag(enu, [&](auto e) -> int {
            VI_HIP(hipFuncSetAttribute((const void*)k_track_grad_sph<LCAP, KCAP, TRACK_GRAD_TT, interp, e>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
            hipLaunchKernelGGL((k_track_grad_sph<LCAP, KCAP, TRACK_GRAD_TT, interp, e>), dim3(nblocks(Q, TRACK_BLOCK)),
                               dim3(TRACK_BLOCK), shm, m->ctx->stream, m->sph, Q, lat, lon, alt, rec, w, R, C, hull, F, out);
            VI_HIP(hipGetLastError());
            return VI_OK;
        });
    });
}
}  // namespace

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
        hipLaunchKernelGGL(k_transform_sph, dim3(nblocks(P, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, m->sph, P, d_lat,
                           d_lon, d_alt, d_c0, d_c1, d_c2);
    else
        hipLaunchKernelGGL(k_transform_rbf, dim3(nblocks(P, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, P, d_lat, d_lon,
                           d_alt, d_c0, d_c1, d_c2);
    VI_HIP(hipGetLastError());
    return VI_OK;
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

// the second half of vi_eval_basis_f64: NaN into the columns of the basis matrix d_Y (N x Q) whose mask byte is 0
int mask_basis(vi_model* m, int64_t Q, const unsigned char* d_mask, double* d_Y)
{
    hipLaunchKernelGGL(k_mask_basis, dim3(nblocks(Q, 256)), dim3(256), 0, m->ctx->stream, Q, m->N, d_mask, d_Y);
    VI_HIP(hipGetLastError());
    return VI_OK;
}
}  // namespace

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

namespace {
// What the two gradient-covariance entries set up alike: the hull pass for all Q points, the chunk - vi_forms_chunk(N, 3), or the
// smaller one of the switch `chunk_env` -, and the context workspace: the planar gradient basis G of a chunk and, unless every
// chunk takes the kernels of vi_eval_resident.hip, the work space of the library route behind it without a gap (else nullptr) -
// A and B of vi_resident_gradcov, or with `records` what vi_records_gradcov asks for.  Each entry walks the chunks itself.
struct GradcovChunks { int64_t chunk; double *G, *work; };
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
}  // namespace

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

// Densities along a trajectory (include/vinterp.h): K2t.  The hull pass and the coefficient preparation of vi_eval_f64 (all R
// rows prepared once into m->d_coef), then one launch: k_track_sph_fast for the orders of vi_eval_f64's fast list, the per-lane
// kernels for every other order, VINTERP_EVAL=generic and the RBF model.  fp64 chains whatever vi_model_set_eval_precision set.
extern "C" int vi_eval_track_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                 const int32_t* d_rec, const double* d_w, int64_t R, const double* d_C, const double* d_hull_eq,
                                 int32_t F, double hull_tol, double* d_out)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_rec && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && R >= 0 && F >= 0, "negative size");
    VI_REQUIRE_RECORDS(R, d_C, "coefficients");
    VI_REQUIRE(Q <= (int64_t)TRACK_BLOCK * 0x7fffffffLL, "more points than one launch takes");
    VI_REQUIRE_HULL(F, d_hull_eq);
    if (Q == 0) return VI_OK;
    VI_HIP(hipSetDevice(m->ctx->device));
    const bool sph = m->kind == VI_MODEL_SPHHARMLAG;
    // (R = 0 prepares no coefficients: every point is NaN, no kernel reads a row)
    const int rc = prepare_call(m, Q, d_lat, d_lon, d_alt, d_hull_eq, F, hull_tol, sph ? R : 0, d_C);
    if (rc != VI_OK) return rc;
    const unsigned char* d_mask = F > 0 ? m->d_mask : nullptr;
    const int Ri = (int)R;
    EvalTimer timer(m->ctx);
    if (!sph)
        return with_flag(d_w != nullptr, [&](auto interp) -> int {
            hipLaunchKernelGGL(k_track_rbf<interp>, dim3(nblocks(Q, BLOCK)), dim3(BLOCK), 0, m->ctx->stream, m->rbf, Q, d_lat, d_lon,
                               d_alt, d_rec, d_w, Ri, d_C, d_mask, (int)F, d_out);
            VI_HIP(hipGetLastError());
            return VI_OK;
        });
    const double* coef = m->d_coef;
    int rcf;
    if (fast_eval_fits(m, TRACK_TT) && at_fast_order(m, &rcf, [&](auto l, auto k) {
            return launch_track_sph_fast<l, k>(m, Q, d_lat, d_lon, d_alt, d_rec, d_w, Ri, coef, d_mask, F, d_out);
        }))
        return rcf;
    return at_order_cap(m, "vi_eval_track_f64", [&](auto lc, auto kc) {
        return launch_track_sph<lc, kc>(m, Q, d_lat, d_lon, d_alt, d_rec, d_w, Ri, coef, d_mask, F, d_out);
    });
}

// Gradients along a trajectory (include/vinterp.h): K2tg.  The hull pass of vi_eval_track_f64 and no coefficient preparation -
// the kernel reads the R raw rows of d_C -, then one launch at the compiled gradient order that holds the model's.
extern "C" int vi_eval_track_grad_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                      const int32_t* d_rec, const double* d_w, int64_t R, const double* d_C,
                                      const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame, double* d_out)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_rec && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && R >= 0 && F >= 0, "negative size");
    VI_REQUIRE_RECORDS(R, d_C, "coefficients");
    VI_REQUIRE(Q <= (int64_t)TRACK_BLOCK * 0x7fffffffLL, "more points than one launch takes");
    VI_REQUIRE_HULL(F, d_hull_eq);
    VI_REQUIRE_FRAME(frame);
    int rc = grad_model_check(m, "vi_eval_track_grad_f64");
    if (rc != VI_OK || Q == 0) return rc;
    VI_HIP(hipSetDevice(m->ctx->device));
    return at_grad_cap(m, "vi_eval_track_grad_f64", [&](auto lc, auto kc) -> int {
        rc = prepare_call(m, Q, d_lat, d_lon, d_alt, d_hull_eq, F, hull_tol, 0, nullptr);
        if (rc != VI_OK) return rc;
        EvalTimer timer(m->ctx);
        return launch_track_grad_sph<lc, kc>(m, Q, d_lat, d_lon, d_alt, d_rec, d_w, (int)R, d_C, F > 0 ? m->d_mask : nullptr,
                                             (int)F, frame == VI_FRAME_ENU, d_out);
    });
}

namespace {
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
}  // namespace

// Standard errors along a trajectory (include/vinterp.h).  The hull pass of vi_eval_track_f64 for all points, then per chunk:
// the basis columns of vi_eval_basis_f64 (its builder and its mask kernel: the same bits) into the context workspace, and
// vi_eval_records_err_f64's routes on them - vi_eval_grad_cov_f64's scheme with the covariance chosen per point.  A chunk
// border inside a run of records changes no bits: a point's bits do not depend on the other points.
extern "C" int vi_eval_track_err_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                     const int32_t* d_rec, const double* d_w, int64_t R, const double* d_dC,
                                     const double* d_hull_eq, int32_t F, double hull_tol, double* d_out)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_rec && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && R >= 0 && F >= 0, "negative size");
    VI_REQUIRE_RECORDS(R, d_dC, "covariances");
    VI_REQUIRE_HULL(F, d_hull_eq);
    if (Q == 0) return VI_OK;
    VI_HIP(hipSetDevice(m->ctx->device));
    int rc = prepare_call(m, Q, d_lat, d_lon, d_alt, d_hull_eq, F, hull_tol, 0, nullptr);
    if (rc != VI_OK) return rc;
    const int64_t chunk = track_err_chunk(m->N, Q);
    double *Y, *none, *work;
    if ((rc = track_err_workspace(m, Q, chunk, d_out, 0, &Y, &none, &work)) != VI_OK) return rc;
    EvalTimer timer(m->ctx);
    return for_chunks(Q, chunk, [&](int64_t q0, int64_t qc) {
        int rc = vi_basis_f64(m, qc, d_lat + q0, d_lon + q0, d_alt + q0, Y, 1, qc);
        if (rc == VI_OK && F > 0) rc = mask_basis(m, qc, m->d_mask + q0, Y);
        if (rc != VI_OK) return rc;
        return vi_records_err(m, qc, Y, d_rec + q0, d_w ? d_w + q0 : nullptr, R, d_dC, d_out + q0, work);
    });
}

// Gradient covariances along a trajectory (include/vinterp.h).  The hull pass of vi_eval_track_f64 for all points, then per
// chunk: the planar gradient basis of the chunk into the context workspace by the launcher of vi_eval_grad_basis_f64, as
// vi_eval_grad_cov_f64 builds it - the same bits per point, the hull's NaN columns and the frame folded in -, and
// vi_eval_records_gradcov_f64's routes on it.  At most 256 MB of gradient basis per chunk (vi_forms_chunk);
// VINTERP_TRACK_GRADCOV_CHUNK: a smaller chunk (tests: several chunks at a small Q).  A chunk border inside a run of records
// changes no bits: a point's bits do not depend on the other points.
extern "C" int vi_eval_track_grad_cov_f64(vi_model* m, int64_t Q, const double* d_lat, const double* d_lon, const double* d_alt,
                                          const int32_t* d_rec, const double* d_w, int64_t R, const double* d_dC,
                                          const double* d_hull_eq, int32_t F, double hull_tol, int32_t frame, double* d_out)
{
    VI_REQUIRE(m && d_lat && d_lon && d_alt && d_rec && d_out, "null argument");
    VI_REQUIRE(Q >= 0 && R >= 0 && F >= 0, "negative size");
    VI_REQUIRE_RECORDS(R, d_dC, "covariances");
    VI_REQUIRE_HULL(F, d_hull_eq);
    VI_REQUIRE_FRAME(frame);
    int rc = grad_model_check(m, "vi_eval_track_grad_cov_f64");
    if (rc != VI_OK || Q == 0) return rc;
    GradcovChunks k;
    rc = gradcov_setup(m, "VINTERP_TRACK_GRADCOV_CHUNK", true, Q, d_lat, d_lon, d_alt, d_hull_eq, F, hull_tol, &k);
    if (rc != VI_OK) return rc;
    EvalTimer timer(m->ctx);
    return for_chunks(Q, k.chunk, [&](int64_t q0, int64_t qc) -> int {
        const int rc = launch_grad_resident(m, "vi_eval_track_grad_cov_f64", qc, d_lat + q0, d_lon + q0, d_alt + q0,
                                            F > 0 ? m->d_mask + q0 : nullptr, frame, k.G);
        if (rc != VI_OK) return rc;
        return vi_records_gradcov(m, qc, k.G, d_rec + q0, d_w ? d_w + q0 : nullptr, R, d_dC, d_out + q0, Q, k.work);
    });
}

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
    if (!sph)
        return with_flag(d_w != nullptr, [&](auto interp) -> int {
            hipLaunchKernelGGL(k_slant_rbf<interp>, dim3(nblocks(P, BLOCK / 64)), dim3(BLOCK), 0, m->ctx->stream, m->rbf, s.P, s.a,
                               s.b, s.rec, s.w, s.R, d_C, s.eq, s.F, s.tol, s.n, s.xq, s.wq, s.out, s.chord);
            VI_HIP(hipGetLastError());
            return VI_OK;
        });
    int rcf;
    if (fast_eval_fits(m, 1) && at_fast_order(m, &rcf, [&](auto l, auto k) { return launch_slant_sph_fast<l, k>(m, s, m->d_coef); }))
        return rcf;
    return at_order_cap(m, "vi_eval_slant_f64", [&](auto lc, auto kc) { return launch_slant_sph<lc, kc>(m, s, m->d_coef); });
}

// The ray-integrated basis (include/vinterp.h): K1l.  No preparation - the kernel clips each ray against the caller's facet list
// itself and reads no coefficients - and one launch: as many rays in a workgroup as the LDS holds accumulator columns beside
// the tiles, SLANT_WAVES unless N is in the thousands.
namespace {
template <class K, class Dev>
int launch_slant_basis(vi_model* m, K kernel, const Dev& dev, int TR, const SlantArgs& s)
{
    int waves = SLANT_WAVES;
    while (waves > 1 && rayb_lds_bytes(m->N, waves, TR) > 64 * 1024) waves >>= 1;
    const size_t shm = rayb_lds_bytes(m->N, waves, TR);
    if (shm > 64 * 1024) {
        vi_set_error("vi_eval_slant_basis_f64: the %d accumulators of a ray exceed the LDS of a workgroup", m->N);
        return VI_ERR_UNSUPPORTED;
    }
    VI_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    hipLaunchKernelGGL(kernel, dim3(nblocks(s.P, waves)), dim3(waves * 64), shm, m->ctx->stream, dev, s.P, s.a, s.b, s.eq, s.F,
                       s.tol, s.n, s.xq, s.wq, s.out, s.chord);
    VI_HIP(hipGetLastError());
    return VI_OK;
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
