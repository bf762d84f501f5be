"""Scan augmentation (cfg.TRAIN.SCAN_AUGMENT; include/mv3d_hip.h: mv3d_scan_transform; mv3d_tf_amd/datasets/augment.py; DESIGN.md
section 3.27), in plain Python: the definition the device code and the host module are held to, bit for bit.  PARITY UNPINNED: the
reference trains from stored maps and has no such code.  Every step is one IEEE operation:

  the matrix   A = [s R(theta) | t], (3,4) f64, R the rotation about z: with c = s * cos(theta) and n = s * sin(theta) in f64
                   A = [[c, -n, 0, t0], [n, c, 0, t1], [0, 0, s, t2]]
               A_inv = [R^T / s | -R^T t / s]: with ci = cos(theta) / s, ni = sin(theta) / s
                   A_inv = [[ci, ni, 0, -(ci * t0 + ni * t1)], [-ni, ci, 0, -(-ni * t0 + ci * t1)], [0, 0, 1 / s, -(t2 / s)]]
  a point      a row [x, y, z, r] with finite x, y, z of a frame that owns it (csrc/frame_rows.h) becomes
                   c'_i = f32(fma(A[i][3], 1, fma(A[i][2], z, fma(A[i][1], y, fma(A[i][0], x, 0)))))     in f64, i = 0, 1, 2
               (scan_crop_restatement.image_vector), r bit for bit; every other row is copied bit for bit
  the boxes    boxes_corners (G,24) x0..x7 y0..y7 z0..z7: every corner as a point; boxes_3D centre = numpy's pairwise f32 mean of
               the eight transformed corners (csrc/gt_encode.hip), extents f32(f64(v) * s); boxes_bv = datasets.mirror.lidar_box_to_bv
               of that -- the reference's rule, which ignores yaw: the BEV box of a rotated car stays l x w, axis-aligned about the
               new centre.  ignore_boxes_3D: the centre as a point, the extents scaled; ignore_boxes_bv from it.  Everything else is
               copied.
  the table    rows 0-2 unchanged; row 3 = Tr' = f32(Tr . [A_inv; 0 0 0 1]), k-ascending fma from 0 in f64 from the stored values,
               stored as f64 holding f32 values (datasets.mirror.mirror_calib's convention)."""
import math

import numpy as np

from kitti_eval_restatement import _fma64
from scan_crop_restatement import frame_of_row, image_vector

from mv3d_tf_amd.datasets.mirror import lidar_box_to_bv

F32 = np.float32


def transform_matrix(theta, scale, shift):
    """-> (A, A_inv), (3,4) f64 each"""
    th, s = float(theta), float(scale)
    t = [float(v) for v in shift]
    c, n = s * math.cos(th), s * math.sin(th)
    A = np.array([[c, -n, 0.0, t[0]], [n, c, 0.0, t[1]], [0.0, 0.0, s, t[2]]], np.float64)
    ci, ni = math.cos(th) / s, math.sin(th) / s
    A_inv = np.array([[ci, ni, 0.0, -(ci * t[0] + ni * t[1])], [-ni, ci, 0.0, -(-ni * t[0] + ci * t[1])],
                      [0.0, 0.0, 1.0 / s, -(t[2] / s)]], np.float64)
    return A, A_inv


def point(A, x, y, z):
    """[x, y, z] f32 -> the three f32 coordinates of A . [x, y, z, 1]; None for a point with a non-finite coordinate, which stays"""
    if not all(math.isfinite(float(c)) for c in (x, y, z)):
        return None
    return [F32(v) for v in image_vector(np.asarray(A, np.float64).reshape(12), float(x), float(y), float(z))]


def transform_rows(points, offsets, xforms):
    """(P,4) f32 rows of B clouds back to back, (B,3,4) f64 -> the transformed (P,4) f32.  offsets None = one frame of every row."""
    points = np.ascontiguousarray(points, F32)
    out = points.copy()
    offs = [0, len(points)] if offsets is None else [int(o) for o in offsets]
    xforms = np.asarray(xforms, np.float64).reshape(-1, 12)
    for p, row in enumerate(points):
        b = frame_of_row(offs, p)
        moved = None if b is None else point(xforms[b], row[0], row[1], row[2])
        if moved is not None:                                # (else copied bit for bit, NaN payloads included: `out` is a byte copy)
            out[p, :3] = moved
    return out


def _mean8(r):
    """numpy's pairwise f32 sum of exactly 8 values, then / 8 (gt_encode.hip:58-65)"""
    r = [F32(v) for v in r]
    return F32(F32(F32(F32(r[0] + r[1]) + F32(r[2] + r[3])) + F32(F32(r[4] + r[5]) + F32(r[6] + r[7]))) / F32(8.0))


def _scaled(v, s):
    return F32(float(F32(v)) * float(s))


def augment_annotation(entry, A, scale):
    out = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in entry.items()}
    cnr = np.asarray(entry['boxes_corners'], F32).reshape(-1, 24)
    new = cnr.copy()
    b3 = np.array(entry['boxes_3D'], F32).reshape(-1, 6)
    for g in range(len(cnr)):
        for j in range(8):
            moved = point(A, cnr[g, j], cnr[g, 8 + j], cnr[g, 16 + j])
            if moved is not None:
                new[g, j], new[g, 8 + j], new[g, 16 + j] = moved
        for i in range(3):
            b3[g, i] = _mean8(new[g, 8 * i:8 * i + 8])
            b3[g, 3 + i] = _scaled(b3[g, 3 + i], scale)
    out['boxes_corners'] = new.astype(np.asarray(entry['boxes_corners']).dtype)
    out['boxes_3D'] = b3.astype(np.asarray(entry['boxes_3D']).dtype)
    out['boxes_bv'] = lidar_box_to_bv(b3).astype(np.asarray(entry['boxes_bv']).dtype)
    if 'ignore_boxes_3D' in entry:
        i3 = np.array(entry['ignore_boxes_3D'], F32).reshape(-1, 6)
        for g in range(len(i3)):
            moved = point(A, i3[g, 0], i3[g, 1], i3[g, 2])
            if moved is not None:
                i3[g, :3] = moved
            for i in range(3):
                i3[g, 3 + i] = _scaled(i3[g, 3 + i], scale)
        out['ignore_boxes_3D'] = i3.astype(np.asarray(entry['ignore_boxes_3D']).dtype)
        out['ignore_boxes_bv'] = lidar_box_to_bv(i3).astype(np.asarray(entry['ignore_boxes_bv']).dtype)
    return out


def augment_calib(table, A_inv):
    t = np.asarray(table, np.float64)
    out = t.copy()
    Tr = t[3]
    Ai = np.vstack([np.asarray(A_inv, np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])
    for i in range(3):
        for j in range(4):
            acc = 0.0
            for k in range(4):
                acc = _fma64(float(Tr[4 * i + k]), float(Ai[k, j]), acc)
            out[3, 4 * i + j] = float(F32(acc))
    return out
