"""Plain-Python restatement of csrc/kitti_eval.hip (test infrastructure; the product never imports it): the oriented-box
IoUs, the detections' image heights and the two statistics passes, as sequential loops in the kernels' operation order (the
header comment of csrc/kitti_eval.hip), so that the device results can be compared bit for bit."""
import math
from fractions import Fraction

import numpy as np

MIN_HEIGHT = (40, 25, 25)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (np.float32(0.15), np.float32(0.30), np.float32(0.50))
N_SAMPLE_PTS = 41


# ------------------------------------------------------------------ overlaps
def _load(c):
    c = np.asarray(c, np.float32).reshape(24)
    fin = bool(np.all(np.isfinite(c)))
    x = [float(c[k]) for k in range(4)]
    y = [float(c[8 + k]) for k in range(4)]
    s = 0.0
    for k in range(4):
        n = (k + 1) % 4
        s = s + (x[k] * y[n] - x[n] * y[k])
    a = 0.5 * s
    if a < 0.0:
        a = -a
        x, y = x[::-1], y[::-1]
    lo = hi = float(c[16])
    for k in range(1, 8):
        z = float(c[16 + k])
        if z < lo:
            lo = z
        if z > hi:
            hi = z
    return fin, x, y, a, lo, hi


def _shoelace(P):
    s = 0.0
    n = len(P)
    for k in range(n):
        (x0, y0), (x1, y1) = P[k], P[(k + 1) % n]
        s = s + (x0 * y1 - x1 * y0)
    return s


def iou_pair(det, gt):
    """(iou_bev, iou_3d) of two (24,) f32 LIDAR-corner boxes."""
    fa, ax, ay, aa, alo, ahi = _load(det)
    fb, bx, by, ba, blo, bhi = _load(gt)
    if not (fa and fb):
        return 0.0, 0.0
    P = list(zip(ax, ay))
    for i in range(4):
        b0x, b0y = bx[i], by[i]
        ex, ey = bx[(i + 1) % 4] - b0x, by[(i + 1) % 4] - b0y
        Q = []
        n = len(P)
        for j in range(n):
            (px, py), (qx, qy) = P[j], P[(j + 1) % n]
            cp = ex * (py - b0y) - ey * (px - b0x)
            cq = ex * (qy - b0y) - ey * (qx - b0x)
            if cp >= 0.0:
                Q.append((px, py))
            if (cp >= 0.0) != (cq >= 0.0):
                t = cp / (cp - cq)
                Q.append((px + t * (qx - px), py + t * (qy - py)))
        P = Q
    inter = 0.5 * _shoelace(P)
    if not (inter > 0.0):
        inter = 0.0
    u = (aa + ba) - inter
    iou_bev = inter / u if u > 0.0 else 0.0
    top = ahi if ahi < bhi else bhi
    bot = alo if alo > blo else blo
    h = top - bot
    if h < 0.0:
        h = 0.0
    vi = inter * h
    u3 = (aa * (ahi - alo) + ba * (bhi - blo)) - vi
    iou_3d = vi / u3 if u3 > 0.0 else 0.0
    return iou_bev, iou_3d


# ------------------------------------------------------------------ detection image height (geometry.h proj_matrix / image_point)
def _round_f32(q):
    f = np.float32(float(q))
    best = None
    for c in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
        d = abs(Fraction(float(c)) - q)
        if best is None or d < best[0] or (d == best[0] and int(np.array(c).view(np.uint32)) % 2 == 0):
            best = (d, c)
    return np.float32(best[1])


def _fma32(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _fma64(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def proj_matrix(calib):
    """(4,12) calibration table -> (3,4) f32 (P2 . R0) . Tr, k-ascending single-rounding f32 fma from 0."""
    cal = np.asarray(calib, np.float32).reshape(48)
    P2, R0, Tr = cal[0:12], cal[24:36], cal[36:48]          # (R0: 9 numbers + the 3 zeros of the table)
    m1 = np.zeros(9, np.float32)
    for i in range(3):
        for j in range(3):
            acc = np.float32(0.0)
            for k in range(4):
                acc = _fma32(P2[i * 4 + k], R0[k * 3 + j], acc)
            m1[i * 3 + j] = acc
    M = np.zeros(12, np.float32)
    for i in range(3):
        for j in range(4):
            acc = np.float32(0.0)
            for k in range(3):
                acc = _fma32(m1[i * 3 + k], Tr[k * 4 + j], acc)
            M[i * 4 + j] = acc
    return M


def det_height(cnr, M, img_height=375):
    c = np.asarray(cnr, np.float32).reshape(24)
    fin = True
    lo = hi = 0.0
    for k in range(8):
        fin = fin and bool(np.isfinite(c[k]) and np.isfinite(c[8 + k]) and np.isfinite(c[16 + k]))
        v = []
        for r in range(3):
            acc = 0.0
            if fin:
                acc = _fma64(float(M[r * 4 + 0]), float(c[k]), acc)
                acc = _fma64(float(M[r * 4 + 1]), float(c[8 + k]), acc)
                acc = _fma64(float(M[r * 4 + 2]), float(c[16 + k]), acc)     # + M[r,3] * 0: exact
            v.append(acc)
        with np.errstate(divide='ignore', invalid='ignore'):
            py = float(np.float64(v[1]) / np.float64(v[2])) if fin else math.nan
        fin = fin and math.isfinite(py)
        if k == 0:
            lo = hi = py
        else:
            if py < lo:
                lo = py
            if py > hi:
                hi = py
    if not fin:
        return 0.0
    hmax = float(img_height - 1)
    lo = 0.0 if lo < 0.0 else (hmax if lo > hmax else lo)
    hi = 0.0 if hi < 0.0 else (hmax if hi > hmax else hi)
    return hi - lo


def overlaps(det_cnr, det_off, gt_cnr, gt_off, calib, img_height=375):
    """-> iou_bev (P), iou_3d (P) in the pair-CSR layout, det heights (N)."""
    F = len(det_off) - 1
    bev, b3, hts = [], [], np.zeros(int(det_off[-1]))
    for f in range(F):
        for d in range(det_off[f], det_off[f + 1]):
            for g in range(gt_off[f], gt_off[f + 1]):
                a, b = iou_pair(det_cnr[d], gt_cnr[g])
                bev.append(a)
                b3.append(b)
        M = proj_matrix(calib[f])
        for d in range(det_off[f], det_off[f + 1]):
            hts[d] = det_height(det_cnr[d], M, img_height)
    return np.array(bev, np.float64), np.array(b3, np.float64), hts


# ------------------------------------------------------------------ the statistics passes
def gt_flag(cls, trunc, occ, y1, y2, diff, eval_class, neighbor_class):
    if cls == eval_class:
        height = float(np.float32(y2)) - float(np.float32(y1))
        hard = np.float32(occ) > np.float32(MAX_OCCLUSION[diff]) or np.float32(trunc) > MAX_TRUNCATION[diff] or height <= MIN_HEIGHT[diff]
        return 1 if hard else 0
    return 1 if cls == neighbor_class else -1


def frame_stats(iou, scores, heights, flags, diff, min_overlap, thresh=None):
    """One frame, one metric, one difficulty.  iou: (D, G) f64; flags: (G) GT flags.  thresh None: pass 1 -> per GT the
    true-positive score or -inf; else pass 2 at score threshold `thresh` -> (tp, fp, fn)."""
    D, G = iou.shape
    ign = [heights[j] < MIN_HEIGHT[diff] for j in range(D)]
    assigned = [False] * D
    slots = [-np.inf] * G
    tp = fp = fn = 0
    for g in range(G):
        if flags[g] == -1:
            continue
        det_idx, valid, max_iou, assigned_ign = -1, -10000000.0, 0.0, False
        found = False
        for j in range(D):
            if assigned[j]:
                continue
            if thresh is not None and np.float32(scores[j]) < np.float32(thresh):
                continue
            o = iou[j, g]
            if thresh is None:
                if o > min_overlap and float(scores[j]) > valid:
                    det_idx, valid, found = j, float(scores[j]), True
            elif o > min_overlap and (o > max_iou or assigned_ign) and not ign[j]:
                max_iou, det_idx, found, assigned_ign = o, j, True, False
            elif o > min_overlap and not found and ign[j]:
                det_idx, found, assigned_ign = j, True, True
        if not found:
            if flags[g] == 0:
                fn += 1
        elif flags[g] == 1 or ign[det_idx]:
            assigned[det_idx] = True
        else:
            tp += 1
            slots[g] = np.float32(scores[det_idx])
            assigned[det_idx] = True
    if thresh is None:
        return np.array(slots, np.float32)
    for j in range(D):
        if not (assigned[j] or ign[j] or np.float32(scores[j]) < np.float32(thresh)):
            fp += 1
    return tp, fp, fn


def get_thresholds(scores, n_gt):
    v = sorted((float(s) for s in scores), reverse=True)
    t, current = [], 0.0
    for i in range(len(v)):
        l_recall = (i + 1) / float(n_gt)
        r_recall = (i + 2) / float(n_gt) if i < len(v) - 1 else l_recall
        if (r_recall - current) < (current - l_recall) and i < len(v) - 1:
            continue
        t.append(v[i])
        current += 1.0 / (N_SAMPLE_PTS - 1.0)
    return np.array(t[:N_SAMPLE_PTS], np.float32)


def ap_from_counts(counts, recall_points=11):
    """counts: list of (tp, fp, fn) per threshold -> AP in percent."""
    prec = [0.0] * N_SAMPLE_PTS
    for i, (tp, fp, _) in enumerate(counts):
        prec[i] = tp / float(tp + fp) if tp + fp > 0 else 0.0
    for i in range(N_SAMPLE_PTS - 2, -1, -1):
        prec[i] = max(prec[i], prec[i + 1])
    if recall_points == 11:
        return sum(prec[0::4]) / 11.0 * 100.0
    return sum(prec[1:]) / 40.0 * 100.0


def evaluate(frames, eval_class, neighbor_class, min_overlap, recall_points=11):
    """frames: list of dicts {'iou': ((D,G) bev, (D,G) 3d), 'scores' (D), 'heights' (D), 'cls', 'trunc', 'occ', 'y1', 'y2' (G)}
    -> {'matched': [metric][diff] list of per-frame slots, 'thresholds', 'counts' [metric][diff] (T, 3), 'ap' [metric][diff]}."""
    out = {'matched': [[[], [], []], [[], [], []]], 'thresholds': [[None] * 3, [None] * 3], 'counts': [[None] * 3, [None] * 3],
           'ap': [[None] * 3, [None] * 3]}
    for di in range(3):
        flags = [[gt_flag(c, t, o, a, b, di, eval_class, neighbor_class) for c, t, o, a, b in
                  zip(fr['cls'], fr['trunc'], fr['occ'], fr['y1'], fr['y2'])] for fr in frames]
        n_gt = sum(f.count(0) for f in flags)
        for mi in range(2):
            slots = [frame_stats(fr['iou'][mi], fr['scores'], fr['heights'], fl, di, min_overlap) for fr, fl in zip(frames, flags)]
            out['matched'][mi][di] = slots
            v = [s for sl in slots for s in sl if s > -np.inf]
            thr = get_thresholds(v, n_gt) if n_gt > 0 else np.zeros(0, np.float32)
            counts = []
            for t in thr:
                tot = [0, 0, 0]
                for fr, fl in zip(frames, flags):
                    r = frame_stats(fr['iou'][mi], fr['scores'], fr['heights'], fl, di, min_overlap, t)
                    tot = [a + b for a, b in zip(tot, r)]
                counts.append(tot)
            out['thresholds'][mi][di] = thr
            out['counts'][mi][di] = np.array(counts, np.int64).reshape(-1, 3)
            out['ap'][mi][di] = ap_from_counts(counts, recall_points)
    return out
