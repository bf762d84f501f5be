"""Host restatement of the MV3D paper's bird's-eye-view encoding (mv3d_tf_amd/csrc/bev_paper.hip) in plain
Python / numpy, for tests/test_bev_paper.py, written from the definition and importing nothing from mv3d_tf_amd.  Every comparison
against it is np.array_equal of the int32 views: each step is an IEEE basic operation in the dtype the definition names (f32 range
tests and divide, f64 slice tests, one f32 subtraction), or a copy.  It loops over the rows so that "the last row among equal
heights" is the loop's own order.  PARITY UNPINNED: the reference has no such raster; test_bev_paper.py ties the parts this definition
shares with point_cloud_2_top (cells, slices, z - height_lo) to the oracle's reference-encoding map."""
import math

import numpy as np

F32 = np.float32
MV3D_RANGES = (0.1, 0.3, -30.0, 30.0, 0.0, 60.0, -2.0, 0.4)      # res, zres, side_lo, side_hi, fwd_lo, fwd_hi, height_lo, height_hi


def density_table():
    """T[n] = (float)min(1, log(n + 1) / log 64), n = 0 .. 63"""
    return np.array([F32(min(1.0, math.log(n + 1) / math.log(64))) for n in range(64)], F32)


def shape(ranges=MV3D_RANGES):
    """(H, W, M + 2) and M; the arithmetic of read_lidar.py:49-51 in Python floats, M = ceil((h1 - h0) / zres)"""
    res, zres, s0, s1, f0, f1, h0, h1 = (float(v) for v in ranges)
    M = int(math.ceil((h1 - h0) / zres))
    return (int((f1 - f0) / res) + 1, int((s1 - s0) / res) + 1, M + 2), M


def slice_heights(ranges, M):
    """np.arange(h0, h1, zres)'s values for i < M: h0, h0 + zres, h0 + i * ((h0 + zres) - h0), in f64"""
    zres, h0 = float(ranges[1]), float(ranges[6])
    nxt = h0 + zres
    delta = nxt - h0
    return [h0 if i == 0 else (nxt if i == 1 else h0 + float(i) * delta) for i in range(M)]


def raster(points, ranges=MV3D_RANGES):
    """points (P, 4) f32 -> (H, W, M + 2) f32; IndexError where a kept row's cell lies outside the map"""
    res, zres, s0, s1, f0, f1, h0, h1 = (float(v) for v in ranges)
    (H, W, C), M = shape(ranges)
    heights = slice_heights(ranges, M)
    T = density_table()
    fwd0, fwd1, ylo, yhi, resf, h0f = F32(f0), F32(f1), F32(-s1), F32(-s0), F32(res), F32(h0)
    xoff, yoff = int(math.floor(s0 / res)), int(math.floor(f1 / res))
    top = np.zeros((H, W, C), F32)
    zmax = {}                   # (yi, xi, i) -> the slice's maximal z
    best = {}                   # (yi, xi) -> (z, reflectance) of the winner so far
    count = {}                  # (yi, xi) -> kept rows
    pts = np.ascontiguousarray(points, F32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        for x, y, z, r in pts:
            if not (x > fwd0 and x < fwd1) or not (y > ylo and y < yhi):
                continue
            zd = float(z)
            S = [i for i in range(M) if zd >= heights[i] and zd < heights[i] + zres]
            if not S:
                continue        # (NaN, +-inf and z outside the height range: dropped, not counted)
            xi = int(F32(-y) / resf) - xoff                      # f32 divide, truncation toward zero
            yi = int(F32(-x) / resf) + yoff
            if xi < 0:
                xi += W
            if yi < 0:
                yi += H
            if xi < 0 or xi >= W or yi < 0 or yi >= H:
                raise IndexError("cell (%d, %d) outside the (%d, %d) map" % (yi, xi, H, W))
            z = z + F32(0.0)                                     # -0.0 -> +0.0: one zero, before anything compares or stores it
            for i in S:
                if (yi, xi, i) not in zmax or z > zmax[yi, xi, i]:
                    zmax[yi, xi, i] = z
            if (yi, xi) not in best or z >= best[yi, xi][0]:     # >= : among equal z the later row
                best[yi, xi] = (z, r)
            count[yi, xi] = count.get((yi, xi), 0) + 1
    for (yi, xi, i), z in zmax.items():
        top[yi, xi, i] = F32(z) - h0f
    for (yi, xi), (_, r) in best.items():
        top[yi, xi, M] = r
    for (yi, xi), n in count.items():
        top[yi, xi, M + 1] = T[min(n, 63)]
    return top


def raster_batch(points, offsets, ranges=MV3D_RANGES):
    """frame b = raster(points[offsets[b]:offsets[b + 1]])"""
    return np.stack([raster(points[offsets[b]:offsets[b + 1]], ranges) for b in range(len(offsets) - 1)])
