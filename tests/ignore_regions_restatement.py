"""Ignore regions in training (this repository's definition, the reference has no such code): a plain numpy
statement of the rule ops.ignore_relabel / mv3d_ignore_relabel implement, f64, loop-level, written for reading.

    IoA(c, q)   intersection over the CANDIDATE's area, +1 pixel convention:
                iw = min(c2, q2) - max(c0, q0) + 1, ih likewise; both > 0, else 0;  iw * ih / ((c2 - c0 + 1) * (c3 - c1 + 1));
                0 when that area is not > 0; 0 when any of the eight numbers is NaN.
    relabel     label == 0 and (max_k IoA(c_bv, ignore_bv[b][k]) >= T or max_m IoA(c_img, ignore_img[b][m]) >= T)  ->  -1
                every other label passes through bit for bit.
    anchors     c_bv = grid_anchor(n, W, stride), integers, not clipped;
                c_img = image_box(proj_matrix(calib[b]), anchor_to_lidar(c_bv)): four int32 (csrc/geometry.h restated below).
    ROIs        c_bv = rois_bv[r, 1:5], c_img = rois_img[r, 1:5], frame = rois_bv[r, 0]; a row whose frame is no integer in [0, B) passes.
    a frame with more than 1024 boxes in a list (or offsets out of order) passes through whole, status ERR_INVALID_ARG = 1.
"""
import numpy as np

F32, F64 = np.float32, np.float64
BASE_ANCHORS = ((-19, -8, 20, 8), (-5, -2, 5, 3), (-8, -19, 8, 20), (-2, -5, 3, 5))     # generate_anchors.py:37-51
MAX_BOXES = 1024
ERR_INVALID_ARG = 1
INT32_MIN = -2 ** 31


def ioa(c, q):
    """intersection of candidate c and ignore box q over c's area; both are 4 python floats"""
    c = [float(v) for v in c]
    q = [float(v) for v in q]
    if any(v != v for v in c + q):
        return 0.0
    with np.errstate(all="ignore"):
        area = F64(c[2] - c[0] + 1) * F64(c[3] - c[1] + 1)
        if not area > 0:
            return 0.0
        iw = F64(min(c[2], q[2])) - F64(max(c[0], q[0])) + 1
        if not iw > 0:
            return 0.0
        ih = F64(min(c[3], q[3])) - F64(max(c[1], q[1])) + 1
        if not ih > 0:
            return 0.0
        return float(iw * ih / area)


def ignored(c, boxes, T):
    return any(ioa(c, q) >= T for q in boxes)


def grid_anchor(n, W, stride):
    a, cell = n % 4, n // 4
    w, h = cell % W, cell // W
    x1, y1, x2, y2 = BASE_ANCHORS[a]
    return x1 + w * stride, y1 + h * stride, x2 + w * stride, y2 + h * stride


def _fma32(a, b, acc):
    """f32 fused multiply-add: the product of two f32 is exact in f64, the sum is rounded to f64 and then to f32"""
    with np.errstate(all="ignore"):
        return F32(F64(a) * F64(b) + F64(acc))


def proj_matrix(calib):
    """(P2 . R0) . Tr in f32, k ascending, fused multiply-adds from a zero accumulator (csrc/geometry.h:proj_matrix)"""
    c = np.asarray(calib, F32).reshape(48)
    P2, R0, Tr = c[0:12], c[24:36], c[36:48]
    m1 = np.zeros(9, F32)
    for i in range(3):
        for j in range(3):
            acc = F32(0)
            for k in range(4):
                acc = _fma32(P2[i * 4 + k], R0[k * 3 + j], acc)
            m1[i * 3 + j] = acc
    M = np.zeros(12, F32)
    for i in range(3):
        for j in range(4):
            acc = F32(0)
            for k in range(3):
                acc = _fma32(m1[i * 3 + k], Tr[k * 4 + j], acc)
            M[i * 4 + j] = acc
    return M


def anchor_to_lidar(x1, y1, x2, y2):
    """the 3D prior of an integer BEV anchor, x y z l w h, f64 then f32 (transform.py:81-111)"""
    cx, cy = (x1 + x2) / 2.0, (y1 + y2) / 2.0
    return np.array([600 * 0.1 - (cy + 0.5) * 0.1 + 0.0, 600 * 0.1 - (cx + 0.5) * 0.1 + (-30.0), F32(-(1.73 - 1.56 / 2.0)),
                     (y2 - y1) * 0.1, (x2 - x1) * 0.1, F32(1.56)], F64).astype(F32)


def _to_i32(v):
    """astype(int32) of an f64 on x86-64: truncation; NaN and out of range give INT32_MIN"""
    if not (v > -2147483649.0 and v < 2147483648.0):
        return INT32_MIN
    return int(np.trunc(v))


def image_box(M, P):
    """the image box of the eight corners of box P under M with homogeneous w = 0 (transform.py:483-500): four int32"""
    M = np.asarray(M, F32)
    hl, hw, hh = P[3] / F32(2), P[4] / F32(2), P[5] / F32(2)
    px, py = [], []
    with np.errstate(all="ignore"):
        for k in range(8):
            sx = -hl if k & 2 else hl
            sy = -hw if (k + 1) & 2 else hw
            sz = hh if k & 4 else -hh
            c = [F64(F32(sx + P[0])), F64(F32(sy + P[1])), F64(F32(sz + P[2]))]
            v = []
            for r in range(3):
                acc = F64(0.0)
                for j in range(3):
                    acc = F64(M[r * 4 + j]) * c[j] + acc                # (the product of two f32 values is exact: this is the fma)
                acc = F64(M[r * 4 + 3]) * F64(0.0) + acc
                v.append(acc)
            px.append(v[0] / v[2])
            py.append(v[1] / v[2])

    def extent(p):
        if any(x != x for x in p):
            return float("nan"), float("nan")
        lo = hi = p[0]
        for x in p[1:]:
            if x < lo:
                lo = x
            if x > hi:
                hi = x
        return lo, hi

    (xmin, xmax), (ymin, ymax) = extent(px), extent(py)
    return _to_i32(xmin), _to_i32(ymin), _to_i32(xmax), _to_i32(ymax)


def anchor_image_box(M, n, W, stride):
    return image_box(M, anchor_to_lidar(*grid_anchor(n, W, stride)))


def _frame_ok(off, b, rows):
    o0, o1 = int(off[b]), int(off[b + 1])
    return 0 <= o0 <= o1 <= rows and o1 - o0 <= MAX_BOXES


def relabel(rpn_labels, roi_labels, rois_bv, rois_img, calib, H, W, ignore_bv, off_bv, ignore_img, off_img, T, stride=8):
    """-> (rpn_labels_out (B, N) f32, roi_labels_out int32 in roi_labels' shape, counts (B, 2) int32, status (B) int32).
    ignore_* are packed (rows, 4) f32 with (B + 1) offsets each."""
    rpn = np.array(rpn_labels, F32, copy=True)
    roi = np.array(roi_labels, np.int32, copy=True)
    flat = roi.reshape(-1)
    B, N = rpn.shape
    assert N == 4 * H * W
    ignore_bv, ignore_img = np.asarray(ignore_bv, F32).reshape(-1, 4), np.asarray(ignore_img, F32).reshape(-1, 4)
    counts, status = np.zeros((B, 2), np.int32), np.zeros(B, np.int32)
    T = float(T)
    for b in range(B):
        if not (_frame_ok(off_bv, b, len(ignore_bv)) and _frame_ok(off_img, b, len(ignore_img))):
            status[b] = ERR_INVALID_ARG
            continue
        q_bv = ignore_bv[off_bv[b]:off_bv[b + 1]]
        q_img = ignore_img[off_img[b]:off_img[b + 1]]
        M = None
        for n in np.flatnonzero(rpn[b] == 0):
            M = proj_matrix(calib[b]) if M is None else M
            if ignored(grid_anchor(int(n), W, stride), q_bv, T) or ignored(anchor_image_box(M, int(n), W, stride), q_img, T):
                rpn[b, n] = -1
                counts[b, 0] += 1
        for r in range(flat.shape[0]):
            if flat[r] != 0 or not (rois_bv[r, 0] == b):
                continue
            if ignored(rois_bv[r, 1:5], q_bv, T) or ignored(rois_img[r, 1:5], q_img, T):
                flat[r] = -1
                counts[b, 1] += 1
    return rpn, roi, counts, status
