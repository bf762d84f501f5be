"""Left/right mirror of a KITTI training frame (cfg.TRAIN.USE_FLIPPED): the annotation and the calibration
of the frame reflected in the LIDAR plane y = 0.  Host numpy: a handful of numbers per frame, once per split.  The maps are
mirrored on the device (ops.mirror_columns, csrc/mirror.hip).

With W the image width in pixels the reflection is
    M  = diag(1, -1, 1, 1)   in LIDAR coordinates,
    Mc = diag(-1, 1, 1[, 1]) in camera coordinates,
    F  = [[-1, 0, W - 1], [0, 1, 0], [0, 0, 1]] in pixels,
so that P2' R0' Tr' M X projects to (W - 1 - u, v) where P2 R0 Tr X projects to (u, v).  The reference's flip
(lib/datasets/imdb.py:104-121) mirrors the image boxes only; here every encoding of an object follows.  A box's corner j
becomes corner j ^ 1 of the mirrored box (the reflection reverses the corners' sense of rotation; the exchange keeps the
order `computeCorners3D` gives the mirrored label), which is what makes the result EQUAL to encoding the mirrored label
(tx -> -tx, ry -> pi - ry, Tr -> Tr')."""
import numpy as np

_SWAP = np.array([1, 0, 3, 2, 5, 4, 7, 6])            # corner j <- corner j ^ 1


def lidar_box_to_bv(boxes_3D):
    """(G, 6) LIDAR boxes x y z l w h -> (G, 4) f32 BEV pixel boxes: csrc/gt_encode.hip:68-74 (lidar_3d_to_bv of
    lib/utils/transform.py:113-142) restated.  The corners in f32, every product and sum rounded; the floor-divide in f64."""
    b = np.asarray(boxes_3D, np.float32).reshape(len(boxes_3D), 6)
    half = np.float32(0.5)
    x1, y1 = b[:, 0] + b[:, 3] * half, b[:, 1] + b[:, 4] * half
    x2, y2 = b[:, 0] - b[:, 3] * half, b[:, 1] - b[:, 4] * half
    cell = lambda v, lo: 600.0 - np.floor_divide(v.astype(np.float64) - lo, 0.1)
    return np.stack([cell(y1, -30.0), cell(x1, 0.0), cell(y2, -30.0), cell(x2, 0.0)], axis=1).astype(np.float32)


def _mirror_angle(a):
    """a' = pi - a in f64 from the stored f32, brought back into (-pi, pi], stored as f32"""
    m = np.pi - np.asarray(a, np.float32).astype(np.float64)
    m = np.where(m > np.pi, m - 2.0 * np.pi, m)
    return m.astype(np.float32)


def _mirror_corners(c):
    """(G, 24) x0..x7 y0..y7 z0..z7 -> corner j takes corner j ^ 1; the caller negates the mirrored coordinate"""
    c = np.asarray(c)
    return c.reshape(c.shape[0], 3, 8)[:, :, _SWAP].copy()


def mirror_annotation(entry, width):
    """The roidb entry (parse_kitti_labels) of the mirrored frame; `width` = the image's width in pixels.  Every field is a
    copy, `entry` is not modified.  Fields this module does not know (what prepare_roidb adds) are copied as they are, so
    mirror before prepare_roidb.  One field is added: `boxes_residual` (G, 4) f32, what the f32 rounding of the mirrored
    `boxes` dropped (see below); nothing else reads it.  An entry parsed with ignore_types has its `ignore_boxes_bv` / `ignore_boxes_3D`
    mirrored like `boxes_bv` / `boxes_3D` and its `ignore_boxes_img` like `boxes` (with `ignore_boxes_img_residual`).  Mirroring twice with one width restores every array field bit for
    bit, except ry / alphas, which take two f32 roundings (and +-pi may come back as the other sign)."""
    W = int(width)
    if W < 1:
        raise ValueError("mirror_annotation: image width %r" % (width,))
    out = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in entry.items()}
    box = np.asarray(entry['boxes'])
    # x1' = W - x2 - 1, x2' = W - x1 - 1 (imdb.py:113-116), in f64 from the stored values and rounded once.  (W - 1) - x as f32
    # drops the low bits of a small x, so the part the rounding dropped goes along as `boxes_residual` (f32, exact: the error
    # of one rounding is representable) and is added back before the next mirror: two mirrors restore `boxes` bit for bit.
    b64 = box.astype(np.float64) + (np.asarray(entry['boxes_residual'], np.float64) if 'boxes_residual' in entry else 0.0)
    m64 = np.stack([(W - 1) - b64[:, 2], b64[:, 1], (W - 1) - b64[:, 0], b64[:, 3]], axis=1)
    out['boxes'] = m64.astype(box.dtype)
    out['boxes_residual'] = (m64 - out['boxes'].astype(np.float64)).astype(np.float32)
    b3 = np.array(entry['boxes_3D'], copy=True)
    b3[:, 1] = -b3[:, 1]
    out['boxes_3D'] = b3
    out['boxes_bv'] = lidar_box_to_bv(b3).astype(np.asarray(entry['boxes_bv']).dtype)   # not a pixel flip: the floor is not symmetric
    lid = _mirror_corners(entry['boxes_corners'])
    lid[:, 1] = -lid[:, 1]
    out['boxes_corners'] = lid.reshape(lid.shape[0], 24)
    cam = _mirror_corners(entry['boxes3D_cam_corners'])
    cam[:, 0] = -cam[:, 0]
    out['boxes3D_cam_corners'] = cam.reshape(cam.shape[0], 24)
    for k in ('boxes_3D_cam', 'xyz'):
        a = np.array(entry[k], copy=True)
        a[:, 0] = -a[:, 0]
        out[k] = a
    for k in ('ry', 'alphas'):
        out[k] = _mirror_angle(entry[k])
    if 'ignore_boxes_bv' in entry:
        # the frame's ignore regions (cfg.TRAIN.IGNORE_TYPES): the BEV boxes as boxes_bv above, from their mirrored LIDAR boxes; the
        # DontCare image boxes as `boxes` above, with their own residual
        i3 = np.array(entry['ignore_boxes_3D'], copy=True)
        i3[:, 1] = -i3[:, 1]
        out['ignore_boxes_3D'] = i3
        out['ignore_boxes_bv'] = lidar_box_to_bv(i3).astype(np.asarray(entry['ignore_boxes_bv']).dtype)
        ibox = np.asarray(entry['ignore_boxes_img'])
        i64 = ibox.astype(np.float64) + (np.asarray(entry['ignore_boxes_img_residual'], np.float64)
                                         if 'ignore_boxes_img_residual' in entry else 0.0)
        n64 = np.stack([(W - 1) - i64[:, 2], i64[:, 1], (W - 1) - i64[:, 0], i64[:, 3]], axis=1)
        out['ignore_boxes_img'] = n64.astype(ibox.dtype)
        out['ignore_boxes_img_residual'] = (n64 - out['ignore_boxes_img'].astype(np.float64)).astype(np.float32)
    out['flipped'] = True
    return out


def mirror_calib(table, width):
    """(4, 12) calibration table (pack_calib: P2 | P3 | R0 + 3 zeros | Tr_velo_to_cam) of the mirrored frame:
    P' = F P Mc, R0' = Mc R0 Mc, Tr' = Mc Tr M.  Computed in f64 from the stored values, rounded to f32, stored as f64 (the
    table stays "f64 holding f32 values"); the sign changes are exact."""
    W = int(width)
    if W < 1:
        raise ValueError("mirror_calib: image width %r" % (width,))
    t = np.asarray(table, np.float64)
    if t.shape != (4, 12):
        raise ValueError("mirror_calib: a (4, 12) table is required, got %s" % (t.shape,))
    out = np.zeros((4, 12))
    for row in (0, 1):                                       # P2, P3
        P = t[row].reshape(3, 4).copy()
        P[0] = (W - 1) * P[2] - P[0]                         # F P
        P[:, 0] = -P[:, 0]                                   # ... Mc
        out[row] = P.ravel()
    R = t[2, :9].reshape(3, 3).copy()
    R[0], R[:, 0] = -R[0], -R[:, 0]                          # row 0 and column 0 negated, R[0][0] twice
    R[0, 0] = t[2, 0]
    out[2, :9] = R.ravel()
    T = t[3].reshape(3, 4).copy()
    T[0], T[:, 1] = -T[0], -T[:, 1]                          # row 0 and column 1 negated, T[0][1] twice
    T[0, 1] = t[3, 1]
    out[3] = T.ravel()
    return out.astype(np.float32).astype(np.float64) + 0.0   # (+ 0.0: a negated zero is stored as +0.0)
