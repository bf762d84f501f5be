"""Host restatement of the front-view rasteriser (mv3d_tf_amd/csrc/front_view_raster.hip) in plain Python /
numpy, for tests/test_front_view_raster.py.  Every comparison against it is np.array_equal: each step below is an IEEE basic
operation in the dtype the device uses.

  pixel     fv_point of csrc/front_view.h on the f64 values of the f32 coordinates: theta = fv_atan2(y, x),
            rho = sqrt(fma(x, x, y*y)), phi = fv_atan2(z, rho), col = floor((45 deg - theta) / d_theta), row = floor((2 deg - phi) / d_phi).
            The arctangent is the oracle's (oracle.fv_atan2, the C restatement of the same table-driven function); the constants are
            the header's hexadecimal literals.
  fma       Python 3.10 has no math.fma: `fma` is float(Fraction(a) * Fraction(b) + Fraction(c)), the exact rational rounded once.
            `fma_ints` is the same value for the 70 000 points of the contention test only, where Fraction arithmetic takes
            seconds: see its docstring for why it rounds once, and the CPU test that holds the two together.
  dropped   non-finite x / y / z; x == 0 and y == 0; col outside [0, 512) or row outside [0, 64).  Nothing is clipped.
  distance  d = f32(sqrt(fma(z, z, fma(x, x, y*y)))): f64, rounded once to f32.
  winner    per pixel the smallest d, among equal d the last point in point order.
  values    [z, d, reflectance] of the winner, z and reflectance bit for bit; an empty pixel is [0, 0, 0]."""
from fractions import Fraction

import numpy as np

H, W = 64, 512
THETA_MAX = float.fromhex("0x1.921fb54442d18p-1")       # +45 deg
DTHETA = float.fromhex("0x1.921fb54442d18p-9")          # (pi / 2) / 512
PHI_TOP = float.fromhex("0x1.1df46a2529d39p-5")         # +2 deg
DPHI = float.fromhex("0x1.e0c2ec0e7b1eep-8")            # 26.9 deg / 64


def fma(a, b, c):
    """a * b + c of finite doubles with ONE rounding"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fma_ints(a, b, c):
    """The same value, ten times faster.  A finite double is exactly n / d with Python ints (float.as_integer_ratio), so a * b + c is
    exactly (na nb dc + nc da db) / (da db dc), a quotient of two ints.  Python's int / int true division returns the double nearest
    the exact quotient (round-half-even: CPython's long_true_divide scales the operands and rounds once), which is what
    float(Fraction) returns for the same rational: one rounding in both."""
    (na, da), (nb, db), (nc, dc) = a.as_integer_ratio(), b.as_integer_ratio(), c.as_integer_ratio()
    return (na * nb * dc + nc * da * db) / (da * db * dc)


def _fma_rows(a, b, c, fma):
    return np.array([fma(float(p), float(q), float(r)) for p, q, r in zip(a, b, c)], np.float64).reshape(np.shape(a))


def project(points, oracle, fma=fma):
    """points (P,4) f32 -> (keep (P,) bool, col (P,) int64, row (P,) int64, d (P,) f32); col / row / d are meaningful where keep"""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    P = pts.shape[0]
    xyz = pts[:, :3].astype(np.float64)
    ok = np.isfinite(xyz).all(axis=1) & ~((xyz[:, 0] == 0.0) & (xyz[:, 1] == 0.0))
    col, row, d = np.zeros(P, np.int64), np.zeros(P, np.int64), np.zeros(P, np.float32)
    keep = np.zeros(P, bool)
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return keep, col, row, d
    x, y, z = xyz[idx, 0], xyz[idx, 1], xyz[idx, 2]
    xy2 = _fma_rows(x, x, y * y, fma)
    theta = oracle.fv_atan2(y, x)
    rho = np.sqrt(xy2)
    phi = oracle.fv_atan2(z, rho)
    c = np.floor((THETA_MAX - theta) / DTHETA)
    r = np.floor((PHI_TOP - phi) / DPHI)
    with np.errstate(over="ignore"):
        dist = np.sqrt(_fma_rows(z, z, xy2, fma)).astype(np.float32)
    inside = (c >= 0) & (c < W) & (r >= 0) & (r < H)
    k = idx[inside]
    keep[k] = True
    col[k], row[k], d[k] = c[inside].astype(np.int64), r[inside].astype(np.int64), dist[inside]
    return keep, col, row, d


def winners(keep, col, row, d):
    """point index of every pixel's winner, (64,512) int64, -1 = empty: smallest d, then the largest index"""
    win = np.full(H * W, -1, np.int64)
    idx = np.flatnonzero(keep)
    if idx.size:
        pix = row[idx] * W + col[idx]
        order = np.lexsort((-idx, d[idx], pix))               # by pixel, then d ascending, then index descending
        first = np.ones(order.size, bool)
        first[1:] = pix[order][1:] != pix[order][:-1]
        win[pix[order][first]] = idx[order][first]
    return win.reshape(H, W)


def raster(points, oracle, projected=None):
    """points (P,4) f32 -> (map (64,512,3) f32, winners (64,512) int64)"""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    keep, col, row, d = projected if projected is not None else project(pts, oracle)
    win = winners(keep, col, row, d)
    fv = np.zeros((H, W, 3), np.float32)
    r, c = np.nonzero(win >= 0)
    w = win[r, c]
    fv[r, c, 0] = pts[w, 2]
    fv[r, c, 1] = d[w]
    fv[r, c, 2] = pts[w, 3]
    return fv, win


def raster_batch(points, offsets, oracle):
    """the frames' clouds back to back + (B + 1) offsets -> (B,64,512,3)"""
    return np.stack([raster(points[offsets[b]:offsets[b + 1]], oracle)[0] for b in range(len(offsets) - 1)]) \
        if len(offsets) > 1 else np.zeros((0, H, W, 3), np.float32)


def point_at(col, row, frac=0.5):
    """a direction (unit f64 x, y, z) through pixel (col, row) at fraction `frac` of the way across it in both angles"""
    theta = THETA_MAX - (col + frac) * DTHETA
    phi = PHI_TOP - (row + frac) * DPHI
    return np.array([np.cos(phi) * np.cos(theta), np.cos(phi) * np.sin(theta), np.sin(phi)])
