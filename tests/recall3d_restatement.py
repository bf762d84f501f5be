"""Plain-numpy restatement of proposal recall by oriented IoU: the array-level contract of mv3d_proposal_recall_3d (the header
comment of mv3d_tf_amd/csrc/proposal_recall_3d.hip) line by line: corner formation, the extent pretest, the evaluator's polygon
clip (kitti_eval_restatement.iou_pair) and the matching loop of lib/datasets/imdb.py:174-194 (recall_restatement.match_frame) fed
the resulting matrix, per metric.  The checker of tests/test_proposal_recall_3d.py and the host side of
tools/proposal_recall_3d_bench.py; never the thing under test."""
import numpy as np

import kitti_eval_restatement as KR
import recall_restatement as RR

STATUS_SHORT, STATUS_NONFINITE = RR.STATUS_SHORT, RR.STATUS_NONFINITE
METRICS = ('bev', '3d')
SIGN_X = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float32)
SIGN_Y = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float32)
SIGN_Z = np.array([-1, -1, -1, -1, 1, 1, 1, 1], np.float32)


def box6_corners(boxes):
    """(N, 6) f32 x y z l w h -> (N, 24) f32 x0..7, y0..7, z0..7, every operation in f32: half = size / 2, corner = (+-half) + centre"""
    b = np.asarray(boxes, np.float32).reshape(-1, 6)
    two = np.float32(2.0)
    with np.errstate(all='ignore'):
        hl, hw, hh = (b[:, 3:4] / two).astype(np.float32), (b[:, 4:5] / two).astype(np.float32), (b[:, 5:6] / two).astype(np.float32)
        x = (SIGN_X * hl + b[:, 0:1]).astype(np.float32)
        y = (SIGN_Y * hw + b[:, 1:2]).astype(np.float32)
        z = (SIGN_Z * hh + b[:, 2:3]).astype(np.float32)
    return np.hstack([x, y, z]).astype(np.float32)


def corners_of(boxes):
    """one frame's proposals, (R, 6) or (R, 24) -> (R, 24) f32"""
    b = np.asarray(boxes, np.float32)
    if b.ndim != 2:
        b = b.reshape(-1, 6)
    return box6_corners(b) if b.shape[1] == 6 else b


def extents(cnr):
    """step 1: f64 (minx, maxx, miny, maxy) over the footprint vertices k = 0..3 (k = 0 first, then strict < / >; numpy's min / max
    give the same for finite values, and the scan's value for a NaN at k = 0; a NaN elsewhere only occurs in frames that record
    0.0 throughout)"""
    c = np.asarray(cnr, np.float64).reshape(-1, 24)
    out = np.empty((c.shape[0], 4))
    for col, base in ((0, 0), (2, 8)):
        lo, hi = c[:, base].copy(), c[:, base].copy()
        for k in range(1, 4):
            v = c[:, base + k]
            lo = np.where(v < lo, v, lo)
            hi = np.where(v > hi, v, hi)
        out[:, col], out[:, col + 1] = lo, hi
    return out


def pretest(ea, eb):
    """step 2 for every pair -> (R, G) bool: True where the clip runs"""
    a, b = ea[:, None, :], eb[None, :, :]
    reject = (a[..., 1] < b[..., 0]) | (b[..., 1] < a[..., 0]) | (a[..., 3] < b[..., 2]) | (b[..., 3] < a[..., 2])
    return ~reject


def overlap_matrices(cnr_a, cnr_b):
    """(R, 24), (G, 24) f32 corners -> (iou_bev (R, G), iou_3d (R, G)) f64, and the number of pairs that passed the pretest"""
    R, G = cnr_a.shape[0], cnr_b.shape[0]
    bev, vol = np.zeros((R, G)), np.zeros((R, G))
    ok = pretest(extents(cnr_a), extents(cnr_b)) if R and G else np.zeros((R, G), bool)
    for i, g in zip(*np.nonzero(ok)):
        bev[i, g], vol[i, g] = KR.iou_pair(cnr_a[i], cnr_b[g])
    return bev, vol, int(ok.sum())


def recall_vectors_3d(boxes, gts, limits=(None,), thresholds=None, on_short='raise', return_passed=False):
    """The contract of mv3d_proposal_recall_3d on per-frame lists of (R, 6) / (R, 24) proposals and (G, 24) object corners (f32):
    -> gt_overlaps (2, L, G_total) f64, counts (2, L, T) int32, status (F) int32."""
    thresholds = np.arange(0.5, 0.95 + 1e-5, 0.05) if thresholds is None else np.asarray(thresholds, np.float64)
    F, L = len(boxes), len(limits)
    gt_off = np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int64)
    out = np.full((2, L, int(gt_off[-1])), -1.0)
    counts = np.zeros((2, L, len(thresholds)), np.int32)
    status = np.zeros(F, np.int32)
    passed = 0
    for f in range(F):
        raw = np.asarray(boxes[f], np.float32)
        g = np.asarray(gts[f], np.float32).reshape(-1, 24)
        if raw.shape[0] == 0:
            continue                                                            # skipped: -1.0, counted nowhere
        finite = np.isfinite(raw).all() and np.isfinite(g).all()
        if finite:
            planes = overlap_matrices(corners_of(raw), g)
            passed += planes[2]
        for mi in range(2):
            for li, limit in enumerate(limits):
                if not finite:
                    rec = np.zeros(g.shape[0])
                    status[f] |= STATUS_NONFINITE
                else:
                    m = planes[mi] if limit is None else planes[mi][:limit]
                    rec, ran_short = RR.match_frame(m, g, lambda a, b, m=m: m.copy(), short=0.0 if on_short == 'zero' else -1.0)
                    if ran_short and on_short != 'zero':
                        status[f] |= STATUS_SHORT
                out[mi, li, gt_off[f]:gt_off[f + 1]] = rec
                for t, thr in enumerate(thresholds):
                    counts[mi, li, t] += int((rec >= thr).sum())
    return (out, counts, status, passed) if return_passed else (out, counts, status)
