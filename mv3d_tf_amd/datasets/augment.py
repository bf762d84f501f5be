"""Geometric augmentation of a KITTI training frame's Velodyne scan (cfg.TRAIN.SCAN_AUGMENT): a similarity
transform A = [s R(theta) | t] of the LIDAR frame -- a rotation about the vertical axis, a uniform scale, a shift -- drawn anew at
every visit of a frame.  Host numpy: a handful of numbers per frame.  The points are transformed on the device
(ops.scan_transform, csrc/scan_transform.hip).  PARITY UNPINNED: the reference trains from stored maps and has no such code;
tests/scan_augment_restatement.py states the rule, and this module equals it bit for bit.  No accuracy claim.

Like a mirrored frame (datasets/mirror.py) an augmented frame is just another frame, and nothing downstream knows:
    the image is not touched;
    Tr_velo_to_cam takes A^-1, Tr' = Tr . A^-1, so that Tr' (A X) = Tr X: every camera-frame quantity and every pixel a point projects
    to stay what they were -- `boxes`, `boxes_3D_cam`, `ry`, `alphas`, `xyz`, `boxes3D_cam_corners`, `ignore_boxes_img` are copied;
    what lives in LIDAR coordinates follows A: the points, `boxes_corners`, `boxes_3D`, `boxes_bv`, `ignore_boxes_3D`, `ignore_boxes_bv`.
`boxes_bv` is datasets.mirror.lidar_box_to_bv of the new `boxes_3D`, the reference's rule, which ignores yaw: the BEV box of a rotated
car stays l x w, axis-aligned about the new centre.  Objects that leave the BEV window are kept, as the loader keeps labels outside
the window.

The draws come from a generator of this module's own, seeded by `seed(cfg.RNG_SEED + rank)` (SolverWrapper.train_model), never from
numpy's global stream: the target layers' subsampling and the data layer's permutation see the same stream with the key on as with
it off."""
import math

import numpy as np

from .mirror import lidar_box_to_bv

try:
    _fma = math.fma                                        # (Python >= 3.13)
except AttributeError:
    import ctypes
    import ctypes.util
    _fma = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").fma
    _fma.restype, _fma.argtypes = ctypes.c_double, [ctypes.c_double] * 3

_F32 = np.float32
_rng = None


def seed(value):
    """(re)start the module's draw stream: np.random.RandomState(value)"""
    global _rng
    _rng = np.random.RandomState(int(value))
    return _rng


def check_config():
    """cfg.TRAIN.SCAN_AUGMENT* checked -> True where training augments its scans.  On without cfg.LIDAR_BV_FROM_SCAN raises ValueError
    (a stored lidar_bv/*.npy map cannot be rotated), as do a scale bound <= 0, an inverted scale range, a negative or non-finite
    rotation bound and a shift that is not three non-negative finite numbers.  ops.scan_augment is this function."""
    from ..fast_rcnn.config import cfg
    T = cfg.TRAIN
    if not T.get('SCAN_AUGMENT', False):
        return False
    if not cfg.LIDAR_BV_FROM_SCAN:
        raise ValueError("cfg.TRAIN.SCAN_AUGMENT needs cfg.LIDAR_BV_FROM_SCAN: a stored bird's-eye-view map cannot be rotated")
    rot = float(T.SCAN_AUGMENT_ROTATION)
    if not (math.isfinite(rot) and rot >= 0.0):
        raise ValueError("cfg.TRAIN.SCAN_AUGMENT_ROTATION must be a finite angle >= 0, got %r" % (T.SCAN_AUGMENT_ROTATION,))
    sc = tuple(float(v) for v in T.SCAN_AUGMENT_SCALE)
    if len(sc) != 2 or not all(math.isfinite(v) and v > 0.0 for v in sc) or sc[0] > sc[1]:
        raise ValueError("cfg.TRAIN.SCAN_AUGMENT_SCALE must be (lo, hi) with 0 < lo <= hi, got %r" % (T.SCAN_AUGMENT_SCALE,))
    sh = tuple(float(v) for v in T.SCAN_AUGMENT_SHIFT)
    if len(sh) != 3 or not all(math.isfinite(v) and v >= 0.0 for v in sh):
        raise ValueError("cfg.TRAIN.SCAN_AUGMENT_SHIFT must be three finite bounds >= 0 (dx, dy, dz), got %r" % (T.SCAN_AUGMENT_SHIFT,))
    return True


def draw_scan_transform(rng=None):
    """One frame's draw -> (theta, scale, (dx, dy, dz)): FIVE `uniform` calls in that order, all five always made (a degenerate range
    consumes its draw too), theta in [-ROTATION, ROTATION), scale in SCAN_AUGMENT_SCALE, d* in [-SHIFT, SHIFT).  rng = a
    np.random.RandomState; None = the module's own, seeded with cfg.RNG_SEED if `seed` was never called."""
    from ..fast_rcnn.config import cfg
    T = cfg.TRAIN
    if rng is None:
        rng = _rng if _rng is not None else seed(cfg.RNG_SEED)
    rot = float(T.SCAN_AUGMENT_ROTATION)
    theta = float(rng.uniform(-rot, rot))
    scale = float(rng.uniform(float(T.SCAN_AUGMENT_SCALE[0]), float(T.SCAN_AUGMENT_SCALE[1])))
    shift = tuple(float(rng.uniform(-float(b), float(b))) for b in T.SCAN_AUGMENT_SHIFT)
    return theta, scale, shift


def transform_matrix(theta, scale, shift):
    """-> (A, A_inv), (3,4) f64 each: A = [s R(theta) | t], R the rotation about z, A_inv = [R^T / s | -R^T t / s]"""
    th, s = float(theta), float(scale)
    t = [float(v) for v in shift]
    if not (math.isfinite(th) and math.isfinite(s) and s > 0.0) or len(t) != 3 or not all(math.isfinite(v) for v in t):
        raise ValueError("transform_matrix: a finite angle, a finite scale > 0 and three finite shifts are required, got %r, %r, %r"
                         % (theta, scale, shift))
    c, n = s * math.cos(th), s * math.sin(th)
    A = np.array([[c, -n, 0.0, t[0]], [n, c, 0.0, t[1]], [0.0, 0.0, s, t[2]]], np.float64)
    ci, ni = math.cos(th) / s, math.sin(th) / s
    A_inv = np.array([[ci, ni, 0.0, -(ci * t[0] + ni * t[1])], [-ni, ci, 0.0, -(-ni * t[0] + ci * t[1])],
                      [0.0, 0.0, 1.0 / s, -(t[2] / s)]], np.float64)
    return A, A_inv


def _point(A, x, y, z):
    """the kernel's chain for one point: f32(fma(A[i][3], 1, fma(A[i][2], z, fma(A[i][1], y, fma(A[i][0], x, 0))))) in f64; None
    for a point with a non-finite coordinate, which stays as it is"""
    x, y, z = float(x), float(y), float(z)
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
        return None
    return tuple(_F32(_fma(r[3], 1.0, _fma(r[2], z, _fma(r[1], y, _fma(r[0], x, 0.0))))) for r in A)


def _scaled(extents, scale):
    """f32 extents -> f32(f64(v) * s)"""
    return (np.asarray(extents, _F32).astype(np.float64) * float(scale)).astype(_F32)


def augment_annotation(entry, A, scale):
    """The roidb entry (parse_kitti_labels, mirrored or not, prepared or not) of the frame transformed by A = transform_matrix(.,
    scale, .)[0].  Every field is a copy, `entry` is not modified.  `boxes_corners`: every corner by the kernel's chain;
    `boxes_3D`: centre = the f32 pairwise mean of the eight new corners (csrc/gt_encode.hip), extents f32(f64(v) * scale);
    `boxes_bv` = lidar_box_to_bv of it; `ignore_boxes_3D` (an entry parsed with ignore_types): the centre as a point, the extents
    scaled, `ignore_boxes_bv` from it.  Every other field is copied as it is."""
    A = [[float(v) for v in row] for row in np.asarray(A, np.float64).reshape(3, 4)]
    out = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in entry.items()}
    cnr = np.asarray(entry['boxes_corners'])
    new = np.array(cnr, _F32).reshape(-1, 3, 8)
    for g in range(new.shape[0]):
        for j in range(8):
            moved = _point(A, new[g, 0, j], new[g, 1, j], new[g, 2, j])
            if moved is not None:
                new[g, :, j] = moved
    b3 = np.array(entry['boxes_3D'], _F32).reshape(-1, 6)
    if new.shape[0]:
        pair = new[:, :, 0::2] + new[:, :, 1::2]             # numpy's pairwise f32 sum of exactly 8 values, written out
        quad = pair[:, :, 0::2] + pair[:, :, 1::2]
        b3[:, :3] = (quad[:, :, 0] + quad[:, :, 1]) / _F32(8.0)
        b3[:, 3:] = _scaled(b3[:, 3:], scale)
    out['boxes_corners'] = new.reshape(-1, 24).astype(cnr.dtype)
    out['boxes_3D'] = b3.astype(np.asarray(entry['boxes_3D']).dtype)
    out['boxes_bv'] = lidar_box_to_bv(b3).astype(np.asarray(entry['boxes_bv']).dtype)
    if 'ignore_boxes_3D' in entry:
        i3 = np.array(entry['ignore_boxes_3D'], _F32).reshape(-1, 6)
        for g in range(i3.shape[0]):
            moved = _point(A, i3[g, 0], i3[g, 1], i3[g, 2])
            if moved is not None:
                i3[g, :3] = moved
        if i3.shape[0]:
            i3[:, 3:] = _scaled(i3[:, 3:], scale)
        out['ignore_boxes_3D'] = i3.astype(np.asarray(entry['ignore_boxes_3D']).dtype)
        out['ignore_boxes_bv'] = lidar_box_to_bv(i3).astype(np.asarray(entry['ignore_boxes_bv']).dtype)
    return out


def augment_calib(table, A_inv):
    """(4, 12) calibration table (pack_calib: P2 | P3 | R0 + 3 zeros | Tr_velo_to_cam) of the transformed frame: rows 0-2 unchanged,
    Tr' = Tr . [A_inv; 0 0 0 1], k-ascending fma from 0 in f64 from the stored values, rounded to f32, stored as f64 (the table stays
    "f64 holding f32 values", mirror_calib's convention)."""
    t = np.asarray(table, np.float64)
    if t.shape != (4, 12):
        raise ValueError("augment_calib: a (4, 12) table is required, got %s" % (t.shape,))
    Ai = np.vstack([np.asarray(A_inv, np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])
    out = t.copy()
    for i in range(3):
        for j in range(4):
            acc = 0.0
            for k in range(4):
                acc = _fma(float(t[3, 4 * i + k]), float(Ai[k, j]), acc)
            out[3, 4 * i + j] = acc
    out[3] = out[3].astype(_F32).astype(np.float64)
    return out
