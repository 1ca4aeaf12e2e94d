"""WGS84 geodetic -> ECEF on the host (pymap3d.geodetic2ecef; the reference calls it at
models/sphharmlag.py:345, interpolate.py:422, estimate.py:172), and its inverse.  Host one-offs only (rotation
constants, RBF centres, convex hull, the end points of Estimate.slant's rays); per-point work uses the device version in
csrc/vi_sph_device.h."""
import numpy as np

WGS84_A = 6378137.0
WGS84_B = 6356752.31424518


def geodetic2ecef(lat, lon, alt):
    lat = np.radians(np.asarray(lat, dtype=np.float64))
    lon = np.radians(np.asarray(lon, dtype=np.float64))
    alt = np.asarray(alt, dtype=np.float64)
    N = WGS84_A**2 / np.sqrt(WGS84_A**2 * np.cos(lat)**2 + WGS84_B**2 * np.sin(lat)**2)
    x = (N + alt) * np.cos(lat) * np.cos(lon)
    y = (N + alt) * np.cos(lat) * np.sin(lon)
    z = (N * (WGS84_B / WGS84_A)**2 + alt) * np.sin(lat)
    return x, y, z


def ecef2geodetic(X, Y, Z):
    """(lat, lon, alt) in degrees, degrees and metres of ECEF points in metres: the inverse of geodetic2ecef on WGS84, shape
    kept.  Bowring's start from the parametric latitude and two fixed-point iterations of it, with sines and cosines (no
    tangent: the poles are ordinary points); the altitude from p cos(lat) + Z sin(lat) - a sqrt(1 - e^2 sin^2(lat)), which
    does not cancel anywhere.  geodetic2ecef of the result is within a few ulps of the input from 10 km below the ellipsoid
    to 30 000 km above it (tests/test_slant_host.py).  At the poles the longitude is arctan2(Y, X) of what is left of them."""
    X, Y, Z = (np.asarray(v, dtype=np.float64) for v in (X, Y, Z))
    a, b = WGS84_A, WGS84_B
    e2 = (a * a - b * b) / (a * a)
    ep2 = (a * a - b * b) / (b * b)
    p = np.hypot(X, Y)
    beta = np.arctan2(a * Z, b * p)                     # parametric latitude of the point's direction
    for _ in range(3):
        lat = np.arctan2(Z + ep2 * b * np.sin(beta)**3, p - e2 * a * np.cos(beta)**3)
        beta = np.arctan2(b * np.sin(lat), a * np.cos(lat))
    sl, cl = np.sin(lat), np.cos(lat)
    alt = p * cl + Z * sl - a * np.sqrt(1. - e2 * sl * sl)
    return np.degrees(lat), np.degrees(np.arctan2(Y, X)), alt
