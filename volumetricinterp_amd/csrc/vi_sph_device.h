// Device helpers shared by the basis / evaluation kernels (vi_basis.hip, vi_eval.hip, vi_track.hip, vi_slant.hip,
// vi_eval_mfma.hip): geodetic -> model coordinates (sphharmlag.py:324-359), the 2F1 seed series and the Laguerre recurrence; the
// per-point engine of the basis (sph_point) with the evaluation's sink; the point's east-north-up matrix and the chains of the
// gradient basis (enu_frame, grad_point: k_grad_sph of vi_basis.hip and K2tg of vi_track.hip) and, on the same walk, of the
// Hessian basis (hess_point: k_hess_sph of vi_hess.hip) or of value, gradient and Hessian together (peak_point: k_peak_sph of
// vi_peak.hip).
#pragma once
#include "vi_common.h"

namespace {

constexpr int BLOCK = 256;
constexpr double WGS84_A = 6378137.0;
constexpr double WGS84_B = 6356752.31424518;
constexpr double DEG2RAD = 0.017453292519943295;   // pi/180, the constant np.radians multiplies by

struct Geom {
    double X, Y, Z;          // ECEF, metres
    double x, s;             // cos(theta), sin(theta) of the rotated colatitude
    double cphi, sphi;       // cos/sin of the rotated azimuth
    double z;                // 100 (r/RE - 1)
    double Rx, Ry;           // rotated equatorial components (for atan2 in vi_transform)
};

// sin and cos of an angle below 1e4 rad: Cody-Waite reduction by pi/2 in two pieces (exact for |x| < 1e4: k has 13 bits) and the
// two kernels of fdlibm on |r| <= pi/4; 2.2e-16 absolute against libm on 2e7 arguments, a third of the instructions of the
// library's sincos (which carries the Payne-Hanek path for huge arguments).  Used by the hull pass's prefilter.
__device__ __forceinline__ void sincos_cw(double x, double& sn, double& cs)
{
    const double k = rint(x * 0.63661977236758134308);
    double r = fma(-k, 1.57079632679489655800e+00, x);
    r = fma(-k, 6.12323399573676603587e-17, r);
    const double z = r * r;
    const double ps = fma(z, fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08),
                                               2.75573137070700676789e-06), -1.98412698298579493134e-04),
                                 8.33333333332248946124e-03), -1.66666666666666324348e-01);
    const double sr = fma(r * z, ps, r);
    const double pc = fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09),
                                               -2.75573143513906633035e-07), 2.48015872894767294178e-05),
                                 -1.38888888888741095749e-03), 4.16666666666666019037e-02);
    const double cr = fma(z * z, pc, fma(-0.5, z, 1.0));
    const int q = (int)k & 3;
    const double a = (q & 1) ? cr : sr, b = (q & 1) ? sr : cr;
    sn = (q & 2) ? -a : a;
    cs = ((q + 1) & 2) ? -b : b;
}

// pymap3d.geodetic2ecef (WGS84 closed form), called at sphharmlag.py:351 / radbasfun.py:253
__device__ __forceinline__ void geodetic2ecef(double lat, double lon, double alt, double& X, double& Y, double& Z)
{
    double sl, cl, so, co;
    sincos(lat * DEG2RAD, &sl, &cl);
    sincos(lon * DEG2RAD, &so, &co);
    const double a2 = WGS84_A * WGS84_A, b2 = WGS84_B * WGS84_B;
    const double Nn = a2 / sqrt(a2 * cl * cl + b2 * sl * sl);
    const double ba = WGS84_B / WGS84_A;
    X = (Nn + alt) * cl * co;
    Y = (Nn + alt) * cl * so;
    Z = (Nn * (ba * ba) + alt) * sl;
}

// Gaussian RBF model (radbasfun.py:83-112): basis function n at the ECEF point R, exp(-|R - c_n|^2 / eps^2)
__device__ __forceinline__ double rbf_gauss(const RbfDev& M, int n, double X, double Y, double Z)
{
    const double* __restrict__ c = M.centers;
    const double dx = X - c[3 * n], dy = Y - c[3 * n + 1], dz = Z - c[3 * n + 2];
    return exp(-(dx * dx + dy * dy + dz * dz) * M.inv_eps2);
}

// the RBF model's value at an ECEF point with the coefficient row Cr and, with INTERP, with the row after it: va, vb
template <bool INTERP>
__device__ __forceinline__ void rbf_rows(const RbfDev& M, const double* __restrict__ Cr, double X, double Y, double Z, double& va,
                                         double& vb)
{
    va = 0.0;
    vb = 0.0;
    for (int n = 0; n < M.N; ++n) {
        const double e = rbf_gauss(M, n, X, Y, Z);
        va = fma(e, Cr[n], va);
        if (INTERP) vb = fma(e, Cr[M.N + n], vb);
    }
}

// sphharmlag.py:345-359: the model coordinates of an ECEF point - Rodrigues rotation about k = (kx, ky, 0) by +theta0 (sign as
// written, F3).  K2l and K1l start here: the nodes of a ray need no geodetic step.
__device__ __forceinline__ Geom sph_geom_ecef(const SphDev& M, double X, double Y, double Z)
{
    Geom g;
    g.X = X;
    g.Y = Y;
    g.Z = Z;
    const double kd = M.kx * X + M.ky * Y;
    const double omc = 1.0 - M.rc;
    const double Rx = X * M.rc + (M.ky * Z) * M.rs + M.kx * kd * omc;
    const double Ry = Y * M.rc + (-M.kx * Z) * M.rs + M.ky * kd * omc;
    const double Rz = Z * M.rc + (M.kx * Y - M.ky * X) * M.rs;
    const double rho2 = Rx * Rx + Ry * Ry;
    const double r = sqrt(rho2 + Rz * Rz);
    g.x = Rz / r;
    g.s = sqrt(1.0 - g.x * g.x);          // scipy's lpmv forms (1-x^2)^(m/2) from x
    const double rho = sqrt(rho2);
    const bool pole = !(rho > 0.0);
    g.cphi = pole ? 1.0 : Rx / rho;       // arctan2(0,0) = 0
    g.sphi = pole ? 0.0 : Ry / rho;
    g.z = 100.0 * (r / M.RE - 1.0);
    g.Rx = Rx;
    g.Ry = Ry;
    return g;
}

__device__ __forceinline__ Geom sph_geom(const SphDev& M, double lat, double lon, double alt)
{
    double X, Y, Z;
    geodetic2ecef(lat, lon, alt, X, Y, Z);
    return sph_geom_ecef(M, X, Y, Z);
}

// 2F1(a,b;c;zz) series with host-tabulated term ratios q[i] = (a+i)(b+i)/((c+i)(i+1)); the exit test
// is wave-uniform so the table stays on the scalar path.
__device__ __forceinline__ double hyp_series(const double* __restrict__ q, int nterms, double zz)
{
    double r = 1.0, sum = 1.0;
    // four terms per exit test: the ratios of a block arrive in one wide scalar load instead of four dependent ones
    // (measured at MAXL = 12, CAP_LIM = 15: the 24 seed series were ~40 % of the evaluation kernel); the up to
    // three terms added past convergence are below 1e-17 of the sum
    int i = 0;
    for (; i + 3 < nterms; i += 4) {
        const double q0 = q[i], q1 = q[i + 1], q2 = q[i + 2], q3 = q[i + 3];
        r *= q0 * zz;
        sum += r;
        r *= q1 * zz;
        sum += r;
        r *= q2 * zz;
        sum += r;
        r *= q3 * zz;
        sum += r;
        if (__all(fabs(r) <= 1e-17 * fabs(sum))) return sum;
    }
    for (; i < nterms; ++i) {
        r *= q[i] * zz;
        sum += r;
    }
    return sum;
}

// The argument (1 - x)/2 of the seed series of degree group G, or NaN past G.zzmax - the largest argument at which every series
// of the group has met the exit test of hyp_series when its table ends (seed_limit, vi_api.hip).  Farther from the pole of the cap
// the seeds, and everything formed from them, are NaN and not the partial sums.  The test stands here, ahead of the chains and
// outside hyp_series, because one more live value inside the series costs k_eval_sph_fast<6, 4, 4> (168 VGPRs) its third wave.
__device__ __forceinline__ double seed_arg(const SphGroupDev& G, double x)
{
    const double zz = 0.5 * (1.0 - x);
    return zz <= G.zzmax ? zz : __builtin_nan("");
}

// scipy.special.eval_laguerre(k, z), k = 0..maxk-1, by the three-term recurrence (sphharmlag.py:141)
template <int KCAP>
__device__ __forceinline__ void laguerre(int maxk, double z, double* Lk)
{
    Lk[0] = 1.0;
    if (KCAP > 1) Lk[1] = 1.0 - z;
#pragma unroll
    for (int k = 1; k + 1 < KCAP; ++k) {
        const double inv = 1.0 / (double)(k + 1);
        Lk[k + 1] = ((2.0 * k + 1.0 - z) * Lk[k] - (double)k * Lk[k - 1]) * inv;
    }
    (void)maxk;
}

// The shared per-point engine.  Sink::consume(l, cur[], cm[], sm[]) is called once per degree l with
// cur[m] = (normalised) P_{nu_l}^m(cos theta), m = 0..l.
// ON_POWER: where the domain test of a degree group stands (seed_arg).  false: on the argument of the seed series; true: on
// s^m, the factor of every series seed, with the argument left alone - the same NaNs.  The register allocation decides: at
// (12, 8) the basis kernel loses its second wave with the test on s^m, at (6, 4) the per-lane track and ray kernels lose one with
// the test on the argument (profiles/r25_kernel_resources.txt), so eval_point takes the one and the basis sinks the other.
template <int LCAP, int KCAP, class Sink, bool ON_POWER = false>
__device__ __forceinline__ void sph_point(const SphDev& M, const Geom& g, Sink& sink)
{
    const int maxl = M.maxl;
    // azimuthal factors cos(m phi), sin(m phi) by angle addition (sphharmlag.py:278-281 takes them of |m| phi)
    double cm[LCAP], sm[LCAP];
    cm[0] = 1.0;
    sm[0] = 0.0;
#pragma unroll
    for (int m = 1; m < LCAP; ++m) {
        cm[m] = cm[m - 1] * g.cphi - sm[m - 1] * g.sphi;
        sm[m] = sm[m - 1] * g.cphi + cm[m - 1] * g.sphi;
    }
    const double x = g.x;
    const int ng = M.ngroups;
    for (int gi = 0; gi < ng; ++gi) {
        const SphGroupDev G = M.groups[gi];
        const bool intseed = (G.nterms == 0);
        const double zz = ON_POWER ? 0.5 * (1.0 - x) : seed_arg(G, x);
        double cur[LCAP], prev[LCAP];
#pragma unroll
        for (int m = 0; m < LCAP; ++m) { cur[m] = 0.0; prev[m] = 0.0; }
        double pmm = 1.0;       // (-1)^m (2m-1)!! s^m
        double spow = 1.0;      // s^m
        if (ON_POWER && !(zz <= G.zzmax)) spow = __builtin_nan("");
        const int nvmax = G.nvmax;
        for (int j = 0; j <= nvmax; ++j) {
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
            const int l = G.pick[j];
            if (l >= 0) sink.template consume<LCAP>(l, cur, cm, sm);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// K2: fused evaluation for TT timesteps per pass.  Cp is the coefficient tile reordered to
// [t][r = l(l+1)+m][k] and pre-multiplied by the per-(l,m) constant (see k_prep_coef).
template <int KCAP, int TT>
struct EvalSink {
    const double* __restrict__ Cp;   // [TT][L2*maxk], wave-uniform reads
    int maxk, NB;
    double Lk[KCAP];
    double acc[TT];
    template <int LCAP>
    __device__ __forceinline__ void consume(int l, const double* cur, const double* cm, const double* sm)
    {
        const int r0 = l * (l + 1);
#pragma unroll
        for (int m = 0; m < LCAP; ++m) {
            if (m <= l) {
                const double* __restrict__ cp = Cp + (size_t)(r0 + m) * maxk;
                const double* __restrict__ cn = Cp + (size_t)(r0 - m) * maxk;
                const double pc = cur[m] * cm[m];
                const double ps = cur[m] * sm[m];
#pragma unroll
                for (int t = 0; t < TT; ++t) {
                    double Sp = 0.0, Sm = 0.0;
#pragma unroll
                    for (int k = 0; k < KCAP; ++k) {
                        if (k < maxk) {
                            Sp = fma(cp[(size_t)t * NB + k], Lk[k], Sp);
                            if (m > 0) Sm = fma(cn[(size_t)t * NB + k], Lk[k], Sm);
                        }
                    }
                    acc[t] = fma(pc, Sp, acc[t]);
                    if (m > 0) acc[t] = fma(ps, Sm, acc[t]);
                }
            }
        }
    }
};

// The per-lane evaluation of one point over TT prepared rows through EvalSink, the one copy k_eval_sph, k_track_sph and
// k_slant_sph run: val[t] = exp(-z/2) sum_n basis_n(point) Cp[t][n], the rows M.N doubles apart.  Correct, not tuned.
template <int LCAP, int KCAP, int TT>
__device__ __forceinline__ void eval_point(const SphDev& M, const Geom& g, const double* __restrict__ Cp, double* val)
{
    EvalSink<KCAP, TT> sink;
    sink.Cp = Cp;
    sink.maxk = M.maxk;
    sink.NB = M.N;
    laguerre<KCAP>(M.maxk, g.z, sink.Lk);
#pragma unroll
    for (int t = 0; t < TT; ++t) sink.acc[t] = 0.0;
    sph_point<LCAP, KCAP, EvalSink<KCAP, TT>, true>(M, g, sink);
    const double E = exp(-0.5 * g.z);
#pragma unroll
    for (int t = 0; t < TT; ++t) val[t] = E * sink.acc[t];
}

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

// The chains of the gradient basis at one point and, with HESS, of the Hessian basis on the same walk - one copy of the Legendre
// seeds and recurrences for both (grad_point, hess_point below).  When chain m of a group has reached degree nu_l + 1, prev holds
// P at nu_l and cur at nu_l + 1: Q0 = Kvm lpmv(ms, v, x), Q1 = Kvm lpmv(ms, v+1, x) for the signed orders ms = +-m.
//   gradient: sink.term(n, tz, tt, tp, L0k, L1k) once per basis function n = k L2 + r; its three gradient components at the point
//             are tz (L0k + 2 L1k), tt L0k and tp L0k - handed over as factors, so that k_grad_sph's sink forms them where that
//             kernel did.
//   Hessian:  with the basis function f = g(r) T(theta') A(phi'), r = RE (z/100 + 1), a = 100/RE,
//               g0 = e L0,  g1 = dg/dr = -e/2 (L0 + 2 L1) a,  g2 = d2g/dr2 = e (L0/4 + L1 + L2) a^2,  L2 = L^(2)_{k-2}(z),
//               T = Q0,  T' = dT/dtheta' = (-(v+1) x Q0 + (v-ms+1) Q1) / y,  T'' = -(x/y) T' - (v(v+1) - m^2/y^2) T
//               (Legendre's equation),  A'' = -m^2 A,
//             the second covariant derivatives in the orthonormal frame (r', theta', phi') of the gradient, in 1/m^2:
//               H_rr = g2 T A                                        H_rt = (g1/r - g0/r^2) T' A
//               H_tt = g0 T'' A / r^2 + g1 T A / r                   H_rp = (g1/r - g0/r^2) T A' / y
//               H_pp = g0 (T A''/y^2 + x T' A/y) / r^2 + g1 T A / r  H_tp = g0 A' (T'/y - x T/y^2) / r^2
//             sink.term(n, h) once per basis function with h[6] in the packed order rr, tt, pp, rt, rp, tp - (0,0) (1,1) (2,2)
//             (0,1) (0,2) (1,2), the gradient covariance's.  Non-finite at the pole of the cap (y = 0), as the gradient is.
//   all:      the Hessian's walk, and sink.term(n, f, d, h) once per basis function with its value f = g0 T A, its gradient
//             d[3] = (g1 T A, g0 T' A / r, g0 T A' / (r y)) in the same orthonormal frame, in 1/m - the three components of the
//             gradient mode - and h[6] as above, all from the factors the Hessian's entries are made of.
enum { WALK_GRAD = 0, WALK_HESS = 1, WALK_ALL = 2 };
template <int LCAP, int KCAP, int MODE, class Sink>
__device__ __forceinline__ void grad_hess_point(const SphDev& M, const Geom& g, Sink& sink)
{
    constexpr bool HESS = MODE != WALK_GRAD;
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
    // the Hessian's radial factors of every k: g0, g1/r and g2
    constexpr int HK = HESS ? KCAP : 1;
    double G0[HK], G1[HK], G2[HK];
    const double inv_r = 1.0 / ((g.z / 100.0 + 1.0) * M.RE), inv_y = 1.0 / y;
    const double inv_r2 = inv_r * inv_r, inv_y2 = inv_y * inv_y;
    const double rr = (g.z / 100.0 + 1.0) * M.RE;                       // r, for the all mode: g1 T A = (g1 T A / r) r
    if constexpr (HESS) {
        const double a = 100.0 / M.RE;
        double Lb = 0.0, La = 0.0;      // L^(2)_{k-3}, L^(2)_{k-2}:  n L^(2)_n = (2n + 1 - z) L^(2)_{n-1} - (n + 1) L^(2)_{n-2}
#pragma unroll
        for (int k = 0; k < KCAP; ++k) {
            const int n = k - 2;
            const double Lc = n < 0 ? 0.0 : n == 0 ? 1.0 : ((2.0 * n + 1.0 - g.z) * La - (double)(n + 1) * Lb) / (double)n;
            Lb = La;
            La = Lc;
            G0[k] = e * L0[k];
            G1[k] = (-0.5 * e * a * inv_r) * (L0[k] + 2.0 * L1[k]);
            G2[k] = (e * a * a) * (0.25 * L0[k] + L1[k] + Lc);
        }
    }
    double cm[LCAP], sm[LCAP];
    cm[0] = 1.0;
    sm[0] = 0.0;
#pragma unroll
    for (int m = 1; m < LCAP; ++m) {
        cm[m] = cm[m - 1] * g.cphi - sm[m - 1] * g.sphi;
        sm[m] = sm[m - 1] * g.cphi + cm[m - 1] * g.sphi;
    }
    for (int gi = 0; gi < M.ngroups; ++gi) {
        const SphGroupDev G = M.groups[gi];
        const bool intseed = (G.nterms == 0);
        const double zz = seed_arg(G, x);
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
                            if constexpr (!HESS) {
                                const double tz = zfac * Q0 * trig;
                                const double tt = e * (-(v + 1.0) * x * Q0 + (v - ms + 1.0) * Q1) * trig * inv_hr;
                                const double tp = e * Q0 * dtrig * inv_hr;
#pragma unroll
                                for (int k = 0; k < KCAP; ++k)
                                    if (k < maxk) sink.term(k * L2 + r, tz, tt, tp, L0[k], L1[k]);
                            } else {
                                const double m2 = (double)(m * m);
                                const double Tp = (-(v + 1.0) * x * Q0 + (v - ms + 1.0) * Q1) * inv_y;
                                const double Tpp = -(x * inv_y) * Tp - (v * (v + 1.0) - m2 * inv_y2) * Q0;
                                const double TA = Q0 * trig;
                                const double a_tt = Tpp * trig * inv_r2;
                                const double a_pp = (x * inv_y * Tp - m2 * inv_y2 * Q0) * trig * inv_r2;
                                const double a_rt = Tp * trig;
                                const double a_rp = Q0 * dtrig * inv_y;
                                const double a_tp = dtrig * (Tp - x * inv_y * Q0) * inv_y * inv_r2;
#pragma unroll
                                for (int k = 0; k < KCAP; ++k) {
                                    if (k < maxk) {
                                        const double dr = G1[k] * TA;                          // g1 T A / r
                                        const double gd = fma(-G0[k], inv_r2, G1[k]);          // g1/r - g0/r^2
                                        const double h[6] = {G2[k] * TA,  fma(G0[k], a_tt, dr), fma(G0[k], a_pp, dr),
                                                             gd * a_rt,   gd * a_rp,            G0[k] * a_tp};
                                        if constexpr (MODE == WALK_ALL) {
                                            const double gi = G0[k] * inv_r;                   // g0 / r
                                            const double d[3] = {dr * rr, gi * a_rt, gi * a_rp};
                                            sink.term(k * L2 + r, G0[k] * TA, d, h);
                                        } else {
                                            sink.term(k * L2 + r, h);
                                        }
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
    }
}

// the gradient basis at one point: the one copy k_grad_sph and K2tg (k_track_grad_sph) instantiate
template <int LCAP, int KCAP, class Sink>
__device__ __forceinline__ void grad_point(const SphDev& M, const Geom& g, Sink& sink)
{
    grad_hess_point<LCAP, KCAP, WALK_GRAD>(M, g, sink);
}

// the Hessian basis at one point (k_hess_sph, vi_hess.hip)
template <int LCAP, int KCAP, class Sink>
__device__ __forceinline__ void hess_point(const SphDev& M, const Geom& g, Sink& sink)
{
    grad_hess_point<LCAP, KCAP, WALK_HESS>(M, g, sink);
}

// value, gradient and Hessian of every basis function at one point on one walk (k_peak_sph, vi_peak.hip)
template <int LCAP, int KCAP, class Sink>
__device__ __forceinline__ void peak_point(const SphDev& M, const Geom& g, Sink& sink)
{
    grad_hess_point<LCAP, KCAP, WALK_ALL>(M, g, sink);
}

}  // namespace
