#!/usr/bin/env python3
"""Exact factors of the Laguerre x spherical-cap-harmonic basis over the whole model domain (build container only; needs
mpmath).  Output tests/golden/domain_<tag>.npz, the yardstick of tests/test_basis_domain_host.py and
tests/test_gpu_basis_domain.py: float64 roundings of 50-digit values at a fixed point set, one file per order tag.

The points are laid out in the model frame as (height, theta', phi') by class - pole, cap, box, wide, beyond, azimuth,
radial, longitude, geodetic pole (POINT CLASSES below) - and turned into geodetic inputs by the inverse Rodrigues rotation
and geodesy.ecef2geodetic in float64.  Everything after that starts from those float64 inputs, exactly as the kernels
receive them, and runs in 50 digits:
  lat, lon, alt      the inputs
  cls, classes       class index per point and the class names
  z, x, y, cphi, sphi, E   100 (r/RE - 1), cos theta', sin theta' (= rho/r, not sqrt(1 - x^2)), cos phi', sin phi', exp(-z/2):
                     the WGS84 closed form, then the Rodrigues rotation written as csrc/vi_sph_device.h writes it with the
                     float64 constants rot_cos, rot_sin, kx, ky of Model.device_tables() taken as exact numbers - so the fixture
                     measures the kernels and not the rounding of a host constant
  nu                 the float64 degrees nu_l of device_tables(), exact from there on
  P0, P1             (P, MAXL, MAXL): mpmath.legenp(nu_l, m, x) and legenp(nu_l + 1, m, x) on the cut (type 2, the
                     Condon-Shortley phase scipy.special.lpmv has), m = 0 .. l, zero elsewhere
  Kvm, neg, neg1     (MAXL, MAXL): the normalisation sqrt((2 nu + 1)/(4 pi) Gamma(nu-m+1)/Gamma(nu+m+1)) (times sqrt 2 for m > 0)
                     and lpmv's negative-order ratio (-1)^m Gamma(v-m+1)/Gamma(v+m+1) at v = nu_l and v = nu_l + 1
  L0, L1, L2         (P, MAXK): L_k(z), L^(1)_(k-1)(z), L^(2)_(k-2)(z), zero where the lower index is negative
  scan_*             the same for a scan of theta' along one meridian (scan_points; scan_theta in degrees): what the basis needs,
                     lat, lon, alt, z, x, y, cphi, sphi, E, P0 and L0
Factors, not the basis: tests/domain_ref.py assembles basis, gradient basis and Hessian basis from them in np.longdouble.

    python tools/gen_domain.py            # every tag
    python tools/gen_domain.py k4l6c15    # one

The points of a tag are evaluated in parallel processes (--jobs).  Measured generation time with 8 processes: k4l6c10 30 s,
k4l6c15 15 s, k3l4c15 6 s, k2l5c12p7 11 s, k8l12c15 53 s (mpmath.legenp takes longest at integer degree and past 135 deg).
The files are written with fixed zip time stamps: a second run reproduces them byte for byte.  Data
only."""
import argparse
import io
import math
import os
import sys
import time
import zipfile
from multiprocessing import Pool

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

mp.mp.dps = 50

RE = 6371.2e3
WGS84_A = 6378137.0
WGS84_B = 6356752.31424518
LATCP, LONCP = 78., 262.

#        tag: (MAXK, MAXL, CAP_LIM, small point set)
TAGS = {'k4l6c10': (4, 6, 10., False),
        'k4l6c15': (4, 6, 15., False),
        'k3l4c15': (3, 4, 15., False),
        'k2l5c12p7': (2, 5, 12.7, False),
        'k8l12c15': (8, 12, 15., True)}

CLASSES = ('pole', 'cap', 'box', 'wide', 'beyond', 'azimuth', 'radial', 'longitude', 'geodetic_pole')
GOLDEN_ANGLE = math.pi * (3. - math.sqrt(5.))


def config_text(maxk, maxl, cap):
    return ('[DEFAULT]\n[MODEL]\nNAME = sphharmlag\nMAXK = %d\nMAXL = %d\nCAP_LIM = %r\nMAX_Z_INT = INF\nLATCP = %g\n'
            'LONCP = %g\n' % (maxk, maxl, cap, LATCP, LONCP))


def tables(maxk, maxl, cap):
    from volumetricinterp_amd.models.sphharmlag import Model
    return Model(io.StringIO(config_text(maxk, maxl, cap))).device_tables()


# ---- POINT CLASSES ----------------------------------------------------------------------------------------------------
def model_points(cap, small):
    """[(class, height above RE in m, theta' in rad, phi' in rad)], fixed; `small`: the thinner set of the MAXL 12 tag."""
    pts = []
    spin = [0]

    def phi_next():
        spin[0] += 1
        return (spin[0] * GOLDEN_ANGLE + math.pi) % (2 * math.pi) - math.pi

    def h_next():
        return 100e3 + 800e3 * ((spin[0] * 0.37) % 1.)

    d = math.radians
    for th in (1e-9, 1e-6, 1e-3):
        for ph in (0.3, -2.8) if small else (0.3, 2.0, -1.2, -2.8):
            pts.append(('pole', 300e3, th, ph))
    for th in np.linspace(0.5, cap, 28 if small else 36):                 # the last one is the cap edge itself
        pts.append(('cap', h_next(), d(float(th)), phi_next()))
    for th in np.linspace(18., 30., 32 if small else 40):
        pts.append(('box', h_next(), d(float(th)), phi_next()))
    for th in (45., 60., 89.9, 90., 90.1, 120., 135.):
        for _ in range(2 if small else 3):
            pts.append(('wide', h_next(), d(th), phi_next()))
    for th in (145., 150., 158., 166., 175., 179.5):
        for _ in range(2 if small else 4):
            pts.append(('beyond', h_next(), d(th), phi_next()))
    for th in (5., 100.) if small else (5., 24., 100.):
        for ph in (0., math.pi / 2, -math.pi / 2, math.pi - 1e-12, -math.pi + 1e-12, 0.7, 2.3, -0.7, -2.3):
            pts.append(('azimuth', 350e3, d(th), ph))
    for th in (7.,) if small else (7., 22.):
        for h in (-10e3, 0., 100e3, 250e3, 400e3, 550e3, 700e3, 850e3, 1000e3, 3000e3):
            pts.append(('radial', h, d(th), phi_next()))
    return pts


def geodetic_points(tb, cap, small):
    """(cls, lat, lon, alt) in float64: model_points through the inverse rotation and ecef2geodetic; the radial class at exact
    altitudes, the longitude class (points of the box given 360 deg lower and higher) and the geodetic pole added."""
    pts = model_points(cap, small)
    cls, lat, lon, alt = [], [], [], []
    for name, h, th, ph in pts:
        la, lo, al = to_geodetic(tb, h, th, ph)
        if name == 'radial':
            al = float(h)                    # the geodetic altitude itself: -10 km, 0, ..., 3000 km
        cls.append(CLASSES.index(name))
        lat.append(la)
        lon.append(lo)
        alt.append(al)
    box = [i for i, c in enumerate(cls) if CLASSES[c] == 'box']
    for i in box[:2] if small else box[:4]:
        for shift in (-360., 360.):
            cls.append(CLASSES.index('longitude'))
            lat.append(lat[i])
            lon.append(lon[i] + shift)
            alt.append(alt[i])
    cls.append(CLASSES.index('geodetic_pole'))
    lat.append(90.)
    lon.append(17.)
    alt.append(300e3)
    return np.array(cls, dtype=np.int8), np.array(lat), np.array(lon), np.array(alt)


def to_geodetic(tb, h, th, ph):
    """(lat, lon, alt) in float64 of the model-frame point (height above RE, theta', phi')."""
    from volumetricinterp_amd.geodesy import ecef2geodetic
    rc, rs, kx, ky = tb['rot_cos'], tb['rot_sin'], tb['kx'], tb['ky']
    Kx = np.array([[0., 0., ky], [0., 0., -kx], [-ky, kx, 0.]])
    k = np.array([kx, ky, 0.])
    Rot = rc * np.eye(3) + rs * Kx + (1. - rc) * np.outer(k, k)
    r = RE + h
    Rm = np.array([r * math.sin(th) * math.cos(ph), r * math.sin(th) * math.sin(ph), r * math.cos(th)])
    la, lo, al = (float(v) for v in ecef2geodetic(*(Rot.T @ Rm)))
    return la, lo % 360., al


def scan_points(tb):
    """The theta' scan of the host test's domain limit: one meridian (phi' = 0.4, 300 km above RE), every 4 deg from 2 to
    134, every 0.25 deg from 136 to 152 - where the seed series' table runs out - every 2 deg to 178, and 179.5."""
    th = np.concatenate([np.arange(2., 136., 4.), np.arange(136., 152., 0.25), np.arange(152., 180., 2.), [179.5]])
    g = np.array([to_geodetic(tb, 300e3, math.radians(float(t)), 0.4) for t in th])
    return th, g[:, 0], g[:, 1], g[:, 2]


# ---- 50 digits --------------------------------------------------------------------------------------------------------
def exact_geometry(rot, la, lo, al):
    """(z, x, y, cphi, sphi) of float64 inputs: the WGS84 closed form and the rotation as sph_geom_ecef writes it."""
    rc, rs, kx, ky = (mp.mpf(v) for v in rot)
    A_, B_ = mp.mpf(WGS84_A), mp.mpf(WGS84_B)
    la, lo, al = mp.radians(mp.mpf(la)), mp.radians(mp.mpf(lo)), mp.mpf(al)
    N = A_**2 / mp.sqrt(A_**2 * mp.cos(la)**2 + B_**2 * mp.sin(la)**2)
    X = (N + al) * mp.cos(la) * mp.cos(lo)
    Y = (N + al) * mp.cos(la) * mp.sin(lo)
    Z = (N * (B_ / A_)**2 + al) * mp.sin(la)
    kd = kx * X + ky * Y
    Rx = X * rc + (ky * Z) * rs + kx * kd * (1 - rc)
    Ry = Y * rc + (-kx * Z) * rs + ky * kd * (1 - rc)
    Rz = Z * rc + (kx * Y - ky * X) * rs
    rho = mp.sqrt(Rx**2 + Ry**2)
    r = mp.sqrt(Rx**2 + Ry**2 + Rz**2)
    return 100 * (r / mp.mpf(RE) - 1), Rz / r, rho / r, Rx / rho, Ry / rho


def _point_task(args):
    rot, nus, maxk, la, lo, al, degree_above = args
    mp.mp.dps = 50
    z, x, y, cphi, sphi = exact_geometry(rot, la, lo, al)
    maxl = len(nus)
    P0 = np.zeros((maxl, maxl))
    P1 = np.zeros((maxl, maxl))
    for l, v in enumerate(nus):
        v = mp.mpf(v)
        for m in range(l + 1):
            P0[l, m] = float(mp.legenp(v, m, x, type=2))
            if degree_above:
                P1[l, m] = float(mp.legenp(v + 1, m, x, type=2))
    L = np.zeros((3, maxk))
    for k in range(maxk):
        L[0, k] = float(mp.laguerre(k, 0, z))
        if k >= 1 and degree_above:
            L[1, k] = float(mp.laguerre(k - 1, 1, z))
        if k >= 2 and degree_above:
            L[2, k] = float(mp.laguerre(k - 2, 2, z))
    geo = np.array([float(v) for v in (z, x, y, cphi, sphi, mp.exp(-z / 2))])
    return geo, P0, P1, L


def constants(nus):
    maxl = len(nus)
    Kvm, neg, neg1 = np.zeros((maxl, maxl)), np.zeros((maxl, maxl)), np.zeros((maxl, maxl))
    for l, v in enumerate(nus):
        v = mp.mpf(float(v))
        for m in range(l + 1):
            K = mp.sqrt((2 * v + 1) / (4 * mp.pi) * mp.gamma(v - m + 1) / mp.gamma(v + m + 1))
            Kvm[l, m] = float(K * mp.sqrt(2) if m else K)
            neg[l, m] = float((-1)**m * mp.gamma(v - m + 1) / mp.gamma(v + m + 1))
            neg1[l, m] = float((-1)**m * mp.gamma(v + 1 - m + 1) / mp.gamma(v + 1 + m + 1))
    return Kvm, neg, neg1


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, buf.getvalue())


def generate(tag, jobs):
    maxk, maxl, cap, small = TAGS[tag]
    tb = tables(maxk, maxl, cap)
    cls, lat, lon, alt = geodetic_points(tb, cap, small)
    rot = (tb['rot_cos'], tb['rot_sin'], tb['kx'], tb['ky'])
    nus = [float(v) for v in tb['nus']]
    t0 = time.time()
    sth, slat, slon, salt = scan_points(tb)
    with Pool(jobs) as pool:
        res = pool.map(_point_task, [(rot, nus, maxk, float(a), float(b), float(c), True) for a, b, c in zip(lat, lon, alt)], 1)
        scan = pool.map(_point_task, [(rot, nus, maxk, float(a), float(b), float(c), False)
                                      for a, b, c in zip(slat, slon, salt)], 1)
    geo = np.array([r[0] for r in res])
    sgeo = np.array([r[0] for r in scan])
    Kvm, neg, neg1 = constants(nus)
    out = os.path.join(ROOT, 'tests', 'golden', 'domain_%s.npz' % tag)
    save_npz(out, dict(order=np.array([maxk, maxl]), cap_lim=np.array(cap), rot=np.array(rot), nu=np.array(nus),
                       classes=np.array(CLASSES), cls=cls, lat=lat, lon=lon, alt=alt,
                       z=geo[:, 0], x=geo[:, 1], y=geo[:, 2], cphi=geo[:, 3], sphi=geo[:, 4], E=geo[:, 5],
                       P0=np.array([r[1] for r in res]), P1=np.array([r[2] for r in res]),
                       L0=np.array([r[3][0] for r in res]), L1=np.array([r[3][1] for r in res]),
                       L2=np.array([r[3][2] for r in res]), Kvm=Kvm, neg=neg, neg1=neg1,
                       scan_theta=sth, scan_lat=slat, scan_lon=slon, scan_alt=salt, scan_z=sgeo[:, 0], scan_x=sgeo[:, 1],
                       scan_y=sgeo[:, 2], scan_cphi=sgeo[:, 3], scan_sphi=sgeo[:, 4], scan_E=sgeo[:, 5],
                       scan_P0=np.array([r[1] for r in scan]), scan_L0=np.array([r[3][0] for r in scan])))
    print('%s: %d points, %.0f s, %d bytes -> %s' % (tag, lat.size, time.time() - t0, os.path.getsize(out), out))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('tags', nargs='*', default=list(TAGS))
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    for t in a.tags:
        generate(t, a.jobs)
