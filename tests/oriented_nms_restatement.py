"""Plain-numpy restatement of mv3d_detect_post_oriented: the contract in the header comment of
mv3d_tf_amd/csrc/detect_post_oriented.hip line by line -- detect_post's candidates and order, the footprint of a row, the extent
pretest (recall3d_restatement.extents / pretest), the evaluator's polygon clip (kitti_eval_restatement.iou_pair) with the EARLIER
box as the polygon and the later one as the clipper, the greedy walk in sorted order, the cap.  The checker of
tests/test_detect_post_oriented.py and the host side of tools/detect_post_oriented_bench.py; never the thing under test."""
import numpy as np

import kitti_eval_restatement as KR
import recall3d_restatement as R3

STATUS_NONFINITE = 2


def score_key(s):
    """mv3d_score_key: f32 score -> order-preserving key, larger = earlier; NaN first, -0.0 and +0.0 one score"""
    s = np.float32(s)
    if s != s:
        return 0xFFFFFFFF
    if s == 0:
        return 0x80000000
    u = int(np.asarray(s, np.float32).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def candidate_order(scores, n, score_thresh):
    """rows r < n with scores[r] > score_thresh in f32 (NaN drops out), by descending key, equal keys by larger row"""
    s = np.asarray(scores, np.float32)
    with np.errstate(invalid='ignore'):
        rows = [r for r in range(min(int(n), len(s))) if s[r] > np.float32(score_thresh)]
    return sorted(rows, key=lambda r: (-score_key(s[r]), -r))


def overlap(a, b, ea, eb, stats=None, passed=None):
    """iou_bev of (earlier box a, later box b), (24,) f32 each; ea / eb their extents (minx, maxx, miny, maxy) in f64.
    passed: the pair's R3.pretest result where the caller has it already (greedy tests a whole row at once)"""
    if passed is None:
        passed = R3.pretest(np.asarray(ea, np.float64)[None], np.asarray(eb, np.float64)[None])[0, 0]
    if not passed:
        return 0.0
    if stats is not None:
        stats['clipped'] = stats.get('clipped', 0) + 1
    return KR.iou_pair(a, b)[0]                              # a the polygon, b the clipper; 0.0 if either is non-finite


def greedy(cnr, nms_thresh, strict, stats=None, cache=None):
    """cnr (n, 24) f32 in processing order -> kept positions.  Position i is kept iff no kept k < i suppresses it; only the pairs
    the walk needs are clipped (the overlap is a pure function of the pair, so this is the reduction of the full mask).
    cache: {(i, j): iou} shared between calls on the same boxes."""
    n = cnr.shape[0]
    with np.errstate(invalid='ignore'):
        ext = R3.extents(cnr) if n else np.zeros((0, 4))
    thr = float(nms_thresh)
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        ok = R3.pretest(ext[i:i + 1], ext[i + 1:])[0] if i + 1 < n else ()
        for j in range(i + 1, n):
            if removed[j]:
                continue
            if cache is not None and (i, j) in cache:
                v = cache[(i, j)]
            else:
                v = overlap(cnr[i], cnr[j], ext[i], ext[j], stats, passed=bool(ok[j - i - 1]))
                if cache is not None:
                    cache[(i, j)] = v
            if (v > thr) if strict else (v >= thr):
                removed[j] = True
    return keep


def frame_tail(scores, pred_bv, corners, pred_cnr_r, K, max_per_image, nms_thresh, score_thresh=0.05, strict=False, source=1,
               stats=None, cache=None):
    """One frame's n rows (scores (n, K), pred_bv (n, 4K), corners (n, 24), pred_cnr_r (n, 24K) or None, all f32)
    -> (rows[j] kept source rows in output order, status).  cache: {j: {(i, j): iou}} for repeated calls on the same arrays."""
    n = scores.shape[0]
    rows, status = [[]], 0
    for j in range(1, K):
        order = candidate_order(scores[:, j], n, score_thresh)
        foot = (pred_cnr_r[order, 24 * j:24 * j + 24] if source == 1 else corners[order]).astype(np.float32).reshape(-1, 24)
        if not np.isfinite(foot).all():
            status |= STATUS_NONFINITE
        keep = greedy(foot, nms_thresh, strict, stats, None if cache is None else cache.setdefault(j, {}))
        rows.append([order[p] for p in keep])
    if max_per_image > 0:                                    # lib/fast_rcnn/test_mv.py:491-501
        image_scores = np.hstack([scores[rows[j], j] for j in range(1, K)]) if K > 1 else np.zeros(0)
        if len(image_scores) > max_per_image:
            t = np.sort(image_scores)[-max_per_image]
            for j in range(1, K):
                rows[j] = [r for r in rows[j] if scores[r, j] >= t]
    return rows, status


def lists(scores, pred_bv, corners, pred_cnr_r, K, rows):
    """the kept rows of one frame -> (dets[j] (N, 5), dets_cnr[j] (N, 25), dets_cnr_r[j] (N, 25) | None): index 0 an empty list"""
    dets, cnr, cnr_r = [[]], [[]], [[]]
    for j in range(1, K):
        r = np.asarray(rows[j], np.int64)
        sc = scores[r, j].astype(np.float32)[:, None]
        dets.append(np.hstack([pred_bv[r, 4 * j:4 * j + 4], sc]).astype(np.float32).reshape(-1, 5))
        cnr.append(np.hstack([corners[r], sc]).astype(np.float32).reshape(-1, 25))
        cnr_r.append(None if pred_cnr_r is None else np.hstack([pred_cnr_r[r, 24 * j:24 * j + 24], sc]).astype(np.float32).reshape(-1, 25))
    return dets, cnr, cnr_r


def detect_post_oriented(scores, pred_bv, corners, pred_cnr_r, num_rois, rows_per_frame, K, max_per_image, nms_thresh,
                         score_thresh=0.05, strict=False, source=1, stats=None, cache=None):
    """The contract on a batch laid out as the device call takes it (B * rows_per_frame rows; num_rois (B) or None, clamped to
    [0, rows_per_frame]) -> per frame (rows, status, dets, dets_cnr, dets_cnr_r).  cache: {} to share the IoUs between calls
    on the same arrays and source (thresholds and rules may differ)."""
    cap = int(rows_per_frame)
    B = scores.shape[0] // cap
    out = []
    for f in range(B):
        n = cap if num_rois is None else max(0, min(cap, int(num_rois[f])))
        sl = slice(f * cap, f * cap + n)
        a = (scores[sl], pred_bv[sl], corners[sl], None if pred_cnr_r is None else pred_cnr_r[sl])
        rows, status = frame_tail(*a, K, max_per_image, nms_thresh, score_thresh, strict, source, stats,
                                  None if cache is None else cache.setdefault(f, {}))
        out.append((rows, status) + lists(*a, K, rows))
    return out
