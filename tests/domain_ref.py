"""Reference of the whole-domain tests (test infrastructure, no GPU): basis, gradient basis and Hessian basis assembled in
np.longdouble from the exact factors of tests/golden/domain_<tag>.npz (tools/gen_domain.py: float64 roundings of 50-digit
values of legenp at real degree, the Laguerre polynomials, the normalisations and the geometry of float64 inputs).  The closed
forms are those of the oracle's basis and grad_basis and of tests/hessian_ref.py, with sin theta' = rho/r from the fixture -
not sqrt(1 - x^2), whose conditioning near the pole of the cap both implementations share and the tests measure.

Layouts as the package returns them: basis (P, N), gradient (P, 3, N) along z, theta', phi', Hessian (P, 6, N) in the packed
order of hessian_ref.PAIRS; N = MAXK MAXL^2, n = k MAXL^2 + l (l + 1) + m with the signed order m."""
import numpy as np

from conftest import load_golden

RE = 6371.2e3
LD = np.longdouble

#        tag: (MAXK, MAXL, CAP_LIM)
TAGS = {'k4l6c10': (4, 6, 10.), 'k4l6c15': (4, 6, 15.), 'k3l4c15': (3, 4, 15.), 'k2l5c12p7': (2, 5, 12.7),
        'k8l12c15': (8, 12, 15.)}
INTEGER_TAGS = ('k4l6c10',)

# The oracle's own error against the fixture on the in-domain points, as tests/test_basis_domain_host.py measures and prints it,
# rounded up to two digits.  basis, grad, hess: column-norm errors over every class but `pole` (gradient and Hessian are exempt
# there); eval: the largest |A C - ref| / sum_n |C B| over rows and those points, tgrad: the same for the three components of the
# gradient, G C, where sin theta' >= 1e-3; basis_pole, eval_pole: the same over the `pole`
# class alone (theta' = 1e-9, 1e-6, 1e-3 rad); grad_beyond, hess_beyond, at the integer tag only: the column-norm errors over the
# `beyond` class, where the same loss of digits in sin theta' meets the antipode (179.5 deg: 1/sin^2 theta' = 1.3e4 in the Hessian).  The pole figures are the conditioning of sin theta' = sqrt(1 - x^2), which the
# oracle (scipy.special.lpmv) and the kernels (g.s) share on purpose: at theta' = 1e-6 the rounding of x = cos theta' alone moves
# 1 - x^2 = 1e-12 by 1e-4 of itself, and the columns of order m by m/2 times that.  Away from the pole the oracle is within 1e-12.
ORACLE_ERR = {
    'k4l6c10': dict(basis=3.7e-13, grad=3.6e-13, hess=3.8e-13, eval=6.0e-14, basis_pole=7.0e-8, eval_pole=5.2e-08, tgrad=1.4e-13,
                    grad_beyond=4.4e-7, hess_beyond=1.8e-6),
    'k4l6c15': dict(basis=6.9e-13, grad=3.1e-13, hess=5.9e-13, eval=6.4e-14, basis_pole=5.0e-8, eval_pole=3.8e-08, tgrad=1.5e-13),
    'k3l4c15': dict(basis=1.3e-13, grad=1.3e-13, hess=2.2e-13, eval=1.1e-13, basis_pole=2.3e-8, eval_pole=3.7e-08, tgrad=1.6e-13),
    'k2l5c12p7': dict(basis=2.0e-13, grad=2.8e-13, hess=2.4e-13, eval=1.8e-13, basis_pole=6.8e-8, eval_pole=7.8e-08, tgrad=2.0e-13),
    'k8l12c15': dict(basis=1.1e-12, grad=4.7e-13, hess=6.9e-13, eval=4.0e-14, basis_pole=2.5e-7, eval_pole=6.2e-08, tgrad=1.1e-13)}
# the project's gates: L2 (column-norm error of a basis) and L6 (an evaluation against the oracle)
FLOOR = dict(basis=1e-11, grad=1e-11, hess=1e-11, eval=1e-10, tgrad=1e-10, basis_pole=1e-11, eval_pole=1e-10, grad_beyond=1e-11,
             hess_beyond=1e-11)
# The largest theta' of the fixtures' scan (0.25 deg steps) up to which the device recurrence with its HYP_TERMS-term seed table
# holds the basis gate at every non-integer tag (tests/test_basis_domain_host.py: MAXL 12 sets it; 145 deg at MAXL 6, 147 deg at
# MAXL 4).  Past the limit of an order the seed series has not converged when its table ends and the outputs are NaN.
DOMAIN_LIMIT_DEG = 140.75


def gate(tag, what):
    """The larger of the project's gate and 4 x the oracle's own error against the fixture on the same points (the factor 4:
    the different summation order and the fmas of the kernels)."""
    return max(FLOOR[what], 4. * ORACLE_ERR[tag][what])


def point_gates(tag, what):
    """gate(tag, what) per point of the fixture: the `pole` class has its own figure."""
    f = fixture(tag)
    return np.where(in_class(f, 'pole'), gate(tag, what + '_pole'), gate(tag, what))


_cache = {}


def config_text(tag):
    maxk, maxl, cap = TAGS[tag]
    return ('[DEFAULT]\n[MODEL]\nNAME = sphharmlag\nMAXK = %d\nMAXL = %d\nCAP_LIM = %r\nMAX_Z_INT = INF\nLATCP = 78\n'
            'LONCP = 262\n' % (maxk, maxl, cap))


def fixture(tag):
    """The arrays of domain_<tag>.npz as a dict, with `classes` as a list of names; loaded once."""
    if tag not in _cache:
        f = dict(load_golden('domain_' + tag))
        f['classes'] = [str(c) for c in f['classes']]
        assert tuple(f['order']) == TAGS[tag][:2] and float(f['cap_lim']) == TAGS[tag][2]
        for v in f.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[tag] = f
    return _cache[tag]


def in_class(f, *names):
    return np.isin(f['cls'], [f['classes'].index(n) for n in names])


def in_domain(f):
    """Every point but the `beyond` class."""
    return ~in_class(f, 'beyond')


def _azimuth(f, pre, maxl):
    cp, sp = f[pre + 'cphi'].astype(LD), f[pre + 'sphi'].astype(LD)
    cm, sm = [np.ones_like(cp)], [np.zeros_like(cp)]
    for m in range(1, maxl):
        cm.append(cm[m - 1] * cp - sm[m - 1] * sp)
        sm.append(sm[m - 1] * cp + cm[m - 1] * sp)
    return cm, sm


def basis(tag, scan=False):
    """(P, N) longdouble: exp(-z/2) L_k(z) Kvm trig(|m| phi') lpmv(m, nu_l, x) at the fixture's points or its theta' scan."""
    key = (tag, 'basis', scan)
    if key in _cache:
        return _cache[key]
    f = fixture(tag)
    pre = 'scan_' if scan else ''
    maxk, maxl = (int(v) for v in f['order'])
    L2 = maxl * maxl
    cm, sm = _azimuth(f, pre, maxl)
    E, L0, P0 = f[pre + 'E'].astype(LD), f[pre + 'L0'].astype(LD), f[pre + 'P0'].astype(LD)
    Kvm, neg = f['Kvm'].astype(LD), f['neg'].astype(LD)
    B = np.zeros((E.size, maxk * L2), dtype=LD)
    for l in range(maxl):
        for m in range(-l, l + 1):
            am = abs(m)
            ang = Kvm[l, am] * (sm[am] * neg[l, am] if m < 0 else cm[am]) * P0[:, l, am]
            for k in range(maxk):
                B[:, k * L2 + l * (l + 1) + m] = E * L0[:, k] * ang
    B.setflags(write=False)
    _cache[key] = B
    return B


def grad_hess(tag):
    """((P, 3, N), (P, 6, N)) longdouble: the gradient basis in the model frame as the oracle's grad_basis lays it out and the
    Hessian basis as hessian_ref.hess_basis does.  Non-finite where sin theta' = 0."""
    key = (tag, 'gh')
    if key in _cache:
        return _cache[key]
    f = fixture(tag)
    maxk, maxl = (int(v) for v in f['order'])
    L2 = maxl * maxl
    cm, sm = _azimuth(f, '', maxl)
    E, z, x, y = (f[n].astype(LD) for n in ('E', 'z', 'x', 'y'))
    L0, L1, Lq = f['L0'].astype(LD), f['L1'].astype(LD), f['L2'].astype(LD)
    P0, P1 = f['P0'].astype(LD), f['P1'].astype(LD)
    Kvm, neg, neg1, nu = (f[n].astype(LD) for n in ('Kvm', 'neg', 'neg1', 'nu'))
    a = LD(100.) / LD(RE)
    r = LD(RE) * (z / 100 + 1)
    G = np.zeros((E.size, 3, maxk * L2), dtype=LD)
    H = np.zeros((E.size, 6, maxk * L2), dtype=LD)
    with np.errstate(all='ignore'):
        for l in range(maxl):
            v = nu[l]
            for m in range(-l, l + 1):
                am = abs(m)
                T = P0[:, l, am] * (neg[l, am] if m < 0 else 1)
                T1 = P1[:, l, am] * (neg1[l, am] if m < 0 else 1)
                A = Kvm[l, am] * (sm[am] if m < 0 else cm[am])
                Ap = am * Kvm[l, am] * cm[am] if m < 0 else -m * Kvm[l, am] * sm[am]
                App = -m * m * A
                Tp = (-(v + 1) * x * T + (v - m + 1) * T1) / y
                Tpp = -(x / y) * Tp - (v * (v + 1) - m * m / y**2) * T
                for k in range(maxk):
                    n = k * L2 + l * (l + 1) + m
                    g0 = E * L0[:, k]
                    g1 = -0.5 * E * (L0[:, k] + 2 * L1[:, k]) * a
                    g2 = E * (0.25 * L0[:, k] + L1[:, k] + Lq[:, k]) * a * a
                    gd = g1 / r - g0 / r**2
                    G[:, 0, n] = g1 * T * A
                    G[:, 1, n] = g0 * Tp * A / r
                    G[:, 2, n] = g0 * T * Ap / (y * r)
                    H[:, 0, n] = g2 * T * A
                    H[:, 1, n] = g0 * Tpp * A / r**2 + g1 * T * A / r
                    H[:, 2, n] = g0 * T * App / (r**2 * y**2) + g1 * T * A / r + x * g0 * Tp * A / (y * r**2)
                    H[:, 3, n] = gd * Tp * A
                    H[:, 4, n] = gd * T * Ap / y
                    H[:, 5, n] = g0 * Ap * (Tp / y - x * T / y**2) / r**2
    G.setflags(write=False)
    H.setflags(write=False)
    _cache[key] = (G, H)
    return G, H


def col_err(A, Aref, sel, dom):
    """The column-norm error of conftest.colnorm_err / hessian_ref.colnorm_err6 with the fixture as the reference: per basis
    function the largest |A - Aref| over the points `sel` (and the 3 or 6 entries) relative to the largest |Aref| over the
    points `dom`; the largest over the basis functions, as a float.  Differences are taken in longdouble."""
    ax = tuple(range(Aref.ndim - 1))
    scale = np.max(np.abs(Aref[dom]), axis=ax)
    scale = np.where(scale == 0, 1, scale)
    if not np.any(sel):
        return 0.
    d = np.abs(np.asarray(A)[sel].astype(LD) - Aref[sel])
    return float(np.max(np.max(d, axis=ax) / scale))


def coefficients(tag, T=21, seed=5):
    """(T, N) float64 coefficient rows randn / column maximum (over the in-domain points) and, per row and point, the gate's
    scale S[t, p] = sum_n |C[t, n] B[p, n]| with the reference densities ref[t, p] = sum_n C[t, n] B[p, n], in longdouble."""
    key = (tag, 'coef', T, seed)
    if key not in _cache:
        f, B = fixture(tag), basis(tag)
        cmax = np.max(np.abs(B[in_domain(f)]), axis=0)
        C = (np.random.default_rng(seed).standard_normal((T, B.shape[1])) / cmax.astype(np.float64))
        Cl = C.astype(LD)
        ref = Cl @ B.T
        S = np.abs(Cl) @ np.abs(B).T
        for v in (C, ref, S):
            v.setflags(write=False)
        _cache[key] = (C, ref, S)
    return _cache[key]
