"""Plain-Python restatement of the 2D side of csrc/kitti_eval.hip (test infrastructure; the product never imports it): the
detections' image and camera boxes, the 2D overlap, and the two statistics passes with the DontCare rule and the orientation
similarity, as sequential loops in the kernels' operation order (the header comment of csrc/kitti_eval.hip)."""
import math

import numpy as np

import kitti_eval_restatement as R

N_SAMPLE_PTS = R.N_SAMPLE_PTS


def _div(a, b):
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.float64(a) / np.float64(b))


def _mean4(a, b, c, d):
    return ((a + b) + (c + d)) / 4.0


def camera_corners(cnr, calib):
    """(24,) f32 LIDAR corners -> 8 camera corners (x, y, z) f64: R . p with R = Tr_velo_to_cam[:, :3]."""
    c = np.asarray(cnr, np.float32).reshape(24)
    Tr = [float(v) for v in np.asarray(calib, np.float32).reshape(48)[36:48]]
    out = []
    for k in range(8):
        px, py, pz = float(c[k]), float(c[8 + k]), float(c[16 + k])
        out.append(tuple((Tr[4 * i] * px + Tr[4 * i + 1] * py) + Tr[4 * i + 2] * pz for i in range(3)))
    return out


def image_box(cnr, calib, image_shape=(375, 1242)):
    """(24,) f32 LIDAR corners -> [x1, y1, x2, y2] f64 clipped image box (all zeros when it cannot be formed)."""
    c = np.asarray(cnr, np.float32).reshape(24)
    P = [float(v) for v in np.asarray(calib, np.float32).reshape(48)[0:12]]
    ok = bool(np.all(np.isfinite(c)))
    x1 = y1 = x2 = y2 = 0.0
    for k, (cx, cy, cz) in enumerate(camera_corners(c, calib)):
        q = [((P[4 * r] * cx + P[4 * r + 1] * cy) + P[4 * r + 2] * cz) + P[4 * r + 3] for r in range(3)]
        u, v = _div(q[0], q[2]), _div(q[1], q[2])
        ok = ok and cz > 0.0 and math.isfinite(u) and math.isfinite(v)
        if k == 0:
            x1 = x2 = u
            y1 = y2 = v
        else:
            if u < x1:
                x1 = u
            if u > x2:
                x2 = u
            if v < y1:
                y1 = v
            if v > y2:
                y2 = v
    if not ok:
        return [0.0, 0.0, 0.0, 0.0]
    wm, hm = float(int(image_shape[1]) - 1), float(int(image_shape[0]) - 1)
    clip = lambda a, m: 0.0 if a < 0.0 else (m if a > m else a)
    return [clip(x1, wm), clip(y1, hm), clip(x2, wm), clip(y2, hm)]


def camera_box(cnr, calib):
    """(24,) f32 LIDAR corners -> [h, w, l, x, y, z, ry, alpha] f64, mv3d_gt_encode's local corner order."""
    cc = camera_corners(cnr, calib)
    cx, cy, cz = [p[0] for p in cc], [p[1] for p in cc], [p[2] for p in cc]
    x, y, z = _mean4(cx[0], cx[1], cx[2], cx[3]), _mean4(cy[0], cy[1], cy[2], cy[3]), _mean4(cz[0], cz[1], cz[2], cz[3])
    dx = _mean4(cx[0], cx[1], cx[4], cx[5]) - _mean4(cx[2], cx[3], cx[6], cx[7])
    dz = _mean4(cz[0], cz[1], cz[4], cz[5]) - _mean4(cz[2], cz[3], cz[6], cz[7])
    ex = _mean4(cx[0], cx[3], cx[4], cx[7]) - _mean4(cx[1], cx[2], cx[5], cx[6])
    ez = _mean4(cz[0], cz[3], cz[4], cz[7]) - _mean4(cz[1], cz[2], cz[5], cz[6])
    ry = math.atan2(-dz, dx)
    alpha = ry - math.atan2(x, z)
    if alpha >= math.pi:
        alpha -= 2.0 * math.pi
    elif alpha < -math.pi:
        alpha += 2.0 * math.pi
    h = y - _mean4(cy[4], cy[5], cy[6], cy[7])
    return [h, math.sqrt(ex * ex + ez * ez), math.sqrt(dx * dx + dz * dz), x, y, z, ry, alpha]


# ------------------------------------------------------------------ 2D overlap (the devkit's boxoverlap, no +1 pixel)
def inter2d(a, b):
    a = [float(v) for v in a]
    b = [float(v) for v in b]
    iw = (a[2] if a[2] < b[2] else b[2]) - (a[0] if a[0] > b[0] else b[0])
    ih = (a[3] if a[3] < b[3] else b[3]) - (a[1] if a[1] > b[1] else b[1])
    if iw <= 0.0 or ih <= 0.0:
        return 0.0
    return iw * ih


def iou2d(det, gt):
    """det: f64 image box, gt: the label's f32 box."""
    inter = inter2d(det, gt)
    if inter == 0.0:
        return 0.0
    det = [float(v) for v in det]
    gt = [float(v) for v in gt]
    return inter / (((det[2] - det[0]) * (det[3] - det[1]) + (gt[2] - gt[0]) * (gt[3] - gt[1])) - inter)


def dontcare_overlap(det, dc):
    inter = inter2d(det, dc)
    if inter == 0.0:
        return 0.0
    det = [float(v) for v in det]
    return inter / ((det[2] - det[0]) * (det[3] - det[1]))


# ------------------------------------------------------------------ the statistics passes
def frame_stats_2d(boxes, alphas, scores, gt_boxes, gt_alpha, dontcare, flags, diff, min_overlap, thresh=None):
    """One frame, one difficulty.  boxes (D, 4) f64 detection image boxes, alphas (D) their alpha; gt_boxes (G, 4) f32,
    gt_alpha (G) f32, dontcare (K, 4) f32; flags (G) GT flags.  thresh None: pass 1 -> per GT the true-positive score or -inf
    (the BEV / 3D pass with the 2D IoU); else pass 2 -> (tp, fp, fn, S) with fp after the DontCare rule and S the sum of
    (1 + cos(a_gt - a_det)) / 2 over the true positives in object order."""
    D, G = len(boxes), len(gt_boxes)
    iou = np.zeros((D, G))
    for j in range(D):
        for g in range(G):
            iou[j, g] = iou2d(boxes[j], gt_boxes[g])
    heights = [float(b[3]) - float(b[1]) for b in boxes]
    if thresh is None:
        return R.frame_stats(iou, scores, heights, flags, diff, min_overlap)
    ign = [heights[j] < R.MIN_HEIGHT[diff] for j in range(D)]
    assigned = [False] * D
    tp = fp = fn = 0
    s = 0.0
    for g in range(G):
        if flags[g] == -1:
            continue
        det_idx, max_iou, assigned_ign, found = -1, 0.0, False, False
        for j in range(D):
            if assigned[j] or np.float32(scores[j]) < np.float32(thresh):
                continue
            o = iou[j, g]
            if o > min_overlap and (o > max_iou or assigned_ign) and not ign[j]:
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
            s = s + (1.0 + math.cos(float(np.float32(gt_alpha[g])) - float(alphas[det_idx]))) / 2.0
            assigned[det_idx] = True
    counted = [not (assigned[j] or ign[j] or np.float32(scores[j]) < np.float32(thresh)) for j in range(D)]
    fp = sum(counted)
    for j in range(D):
        if counted[j] and any(dontcare_overlap(boxes[j], q) > min_overlap for q in dontcare):
            fp -= 1
    return tp, fp, fn, s


def aos_from_counts(counts, sims, recall_points=11):
    """counts: (tp, fp, fn) per threshold, sims: the frame-summed similarity per threshold -> AOS in percent."""
    aos = [0.0] * N_SAMPLE_PTS
    for i, ((tp, fp, _), sm) in enumerate(zip(counts, sims)):
        aos[i] = sm / float(tp + fp) if tp + fp > 0 else 0.0
    for i in range(N_SAMPLE_PTS - 2, -1, -1):
        aos[i] = max(aos[i], aos[i + 1])
    if recall_points == 11:
        return sum(aos[0::4]) / 11.0 * 100.0
    return sum(aos[1:]) / 40.0 * 100.0


def evaluate_2d(frames, eval_class, neighbor_class, min_overlap, recall_points=11):
    """frames: list of dicts {'boxes' (D,4), 'alphas' (D), 'scores' (D), 'gt_boxes' (G,4), 'gt_alpha' (G), 'dontcare' (K,4),
    'cls', 'trunc', 'occ' (G)} (the GT flags take y1 / y2 from gt_boxes) -> {'matched' [diff] per-frame slots, 'thresholds'
    [diff], 'counts' [diff] (T, 3), 'sim' [diff] (F, T) per-frame sums, 'ap' [diff], 'aos' [diff]}."""
    out = {k: [None] * 3 for k in ('matched', 'thresholds', 'counts', 'sim', 'ap', 'aos')}
    for di in range(3):
        flags = [[R.gt_flag(c, t, o, b[1], b[3], di, eval_class, neighbor_class) for c, t, o, b in
                  zip(fr['cls'], fr['trunc'], fr['occ'], fr['gt_boxes'])] for fr in frames]
        n_gt = sum(f.count(0) for f in flags)
        args = lambda fr: (fr['boxes'], fr['alphas'], fr['scores'], fr['gt_boxes'], fr['gt_alpha'], fr['dontcare'])
        slots = [frame_stats_2d(*args(fr), fl, di, min_overlap) for fr, fl in zip(frames, flags)]
        out['matched'][di] = slots
        v = [s for sl in slots for s in sl if s > -np.inf]
        thr = R.get_thresholds(v, n_gt) if n_gt > 0 else np.zeros(0, np.float32)
        counts, sim = [], np.zeros((len(frames), len(thr)))
        for ti, t in enumerate(thr):
            tot = [0, 0, 0]
            for f, (fr, fl) in enumerate(zip(frames, flags)):
                tp, fp, fn, s = frame_stats_2d(*args(fr), fl, di, min_overlap, t)
                tot = [tot[0] + tp, tot[1] + fp, tot[2] + fn]
                sim[f, ti] = s
            counts.append(tot)
        sums = []
        for ti in range(len(thr)):
            acc = 0.0
            for f in range(len(frames)):
                acc = acc + sim[f, ti]
            sums.append(acc)
        out['thresholds'][di] = thr
        out['counts'][di] = np.array(counts, np.int64).reshape(-1, 3)
        out['sim'][di] = sim
        out['ap'][di] = R.ap_from_counts(counts, recall_points)
        out['aos'][di] = aos_from_counts(counts, sums, recall_points)
    return out


def frames_from(dets, gts, calibs, image_shapes=None):
    """The restatement's frames of a split: dets per frame (D, 25), gts per frame load_eval_labels-style dicts."""
    frames = []
    for f, (d, g, c) in enumerate(zip(dets, gts, calibs)):
        d = np.asarray(d, np.float32).reshape(-1, 25)
        shape = (375, 1242) if image_shapes is None else image_shapes[f]
        frames.append({'boxes': [image_box(x[:24], c, shape) for x in d], 'alphas': [camera_box(x[:24], c)[7] for x in d],
                       'scores': d[:, 24], 'gt_boxes': np.asarray(g['boxes'], np.float32).reshape(-1, 4),
                       'gt_alpha': np.asarray(g['alpha'], np.float32), 'dontcare': np.asarray(g['dontcare'], np.float32).reshape(-1, 4),
                       'cls': g['cls'], 'trunc': g['truncation'], 'occ': g['occlusion']})
    return frames
