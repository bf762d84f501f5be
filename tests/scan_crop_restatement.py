"""The crop of a Velodyne scan to the camera image (include/mv3d_hip.h: mv3d_scan_crop_to_image), in plain
Python: the definition the device code is held to, bit for bit.  PARITY UNPINNED: the reference has no such code -- the MV3D paper's
section 3.4 has the sentence ("we also remove points that are out of the image boundaries when projected to the image plane"), and
this file fixes what it means here.  Every step is one IEEE operation:

  a row [x, y, z, r] of frame b is KEPT iff x, y, z are finite and, with M = proj_matrix(calib[b]) (the f32 (P2 . R0) . Tr of
  tests/kitti_eval_restatement.py, pinned by tests/golden/proj_matrix.npz) and
      v[i] = fma(M[i][3], 1, fma(M[i][2], z, fma(M[i][1], y, fma(M[i][0], x, 0))))      in f64, i = 0, 1, 2   (homogeneous w = 1)
  v[2] > 0 and, u = v[0] / v[2], w = v[1] / v[2] (f64), 0 <= u < width and 0 <= w < height.  No margin, no minimum depth; a frame
  whose height or width is <= 0 keeps nothing; r is never looked at.

Frame b owns rows offsets[b] .. offsets[b + 1] by the rule of csrc/frame_rows.h, restated in `frame_of_row`; a row no frame owns is
dropped.  The result is the kept rows in their order and offsets_out[b] = the kept rows of the frames < b."""
import math

import numpy as np

from kitti_eval_restatement import _fma64, proj_matrix

F32 = np.float32


def image_vector(M, x, y, z):
    """v = M . [x, y, z, 1] in f64, one fma per term, from a zero accumulator"""
    v = []
    for i in range(3):
        acc = 0.0
        for m, c in ((M[4 * i], x), (M[4 * i + 1], y), (M[4 * i + 2], z), (M[4 * i + 3], 1.0)):
            acc = _fma64(float(m), float(c), acc)
        v.append(acc)
    return v


def keep_row(M, row, height, width):
    x, y, z = (float(c) for c in row[:3])
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
        return False
    v = image_vector(M, x, y, z)
    if not v[2] > 0.0 or height <= 0 or width <= 0:
        return False
    u, w = v[0] / v[2], v[1] / v[2]
    return 0.0 <= u < float(width) and 0.0 <= w < float(height)


def frame_of_row(offsets, p):
    """csrc/frame_rows.h: the binary search for the last b with offsets[b] <= p, and whether that frame owns p -> frame or None"""
    lo, hi = 0, len(offsets) - 2
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if offsets[mid] <= p:
            lo = mid
        else:
            hi = mid - 1
    return lo if offsets[lo] <= p < offsets[lo + 1] else None


def keep_mask(points, offsets, calibs, image_hw):
    """(P,) bool: the rows the crop keeps.  offsets None = one frame of every row."""
    points = np.asarray(points, F32)
    offsets = [0, len(points)] if offsets is None else [int(o) for o in offsets]
    mats = [proj_matrix(c) for c in calibs]
    seen = {}                                                # (the tests' clouds repeat a few template rows)
    keep = np.zeros(len(points), bool)
    for p, row in enumerate(points):
        b = frame_of_row(offsets, p)
        if b is None:
            continue
        key = (b, row[:3].tobytes())
        if key not in seen:
            seen[key] = keep_row(mats[b], row, int(image_hw[b][0]), int(image_hw[b][1]))
        keep[p] = seen[key]
    return keep


def crop(points, offsets, calibs, image_hw):
    """-> (kept rows (K,4) f32 in their order, offsets_out (B + 1) int32)"""
    points = np.asarray(points, F32)
    keep = keep_mask(points, offsets, calibs, image_hw)
    offs = [0, len(points)] if offsets is None else [int(o) for o in offsets]
    frames = np.array([-1 if frame_of_row(offs, p) is None else frame_of_row(offs, p) for p in range(len(points))], np.int64)
    out = np.array([int((keep & (frames < b)).sum()) for b in range(len(offs))], np.int32)
    return points[keep], out
