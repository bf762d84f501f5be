"""Plain-numpy restatement of proposal recall: lib/datasets/imdb.py:121-209 (evaluate_recall) line by line, and the array-level
contract of mv3d_proposal_recall (the header comment of mv3d_tf_amd/csrc/proposal_recall.hip) on top of the same matching loop.
`bbox_overlaps` is passed in (the oracle's restatement of lib/utils/bbox.pyx:15, f64).  The checker of tests/test_proposal_recall.py
and the host side of tools/proposal_recall_bench.py; never the thing under test."""
import numpy as np

AREAS = {'all': 0, 'small': 1, 'medium': 2, 'large': 3, '96-128': 4, '128-256': 5, '256-512': 6, '512-inf': 7}
AREA_RANGES = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2], [96 ** 2, 128 ** 2], [128 ** 2, 256 ** 2],
               [256 ** 2, 512 ** 2], [512 ** 2, 1e5 ** 2]]
STATUS_SHORT, STATUS_NONFINITE = 1, 2


def match_frame(boxes, gt_boxes, bbox_overlaps, short=None):
    """imdb.py:174-194: the recorded overlap of every round.  short=None: the reference's assert; short=v: the rounds for which no
    box is left record v (and the second return value says that there were such rounds)."""
    overlaps = bbox_overlaps(boxes.astype(np.float64), gt_boxes.astype(np.float64))
    _gt_overlaps = np.zeros((gt_boxes.shape[0]))
    ran_short = False
    for j in range(gt_boxes.shape[0]):
        argmax_overlaps = overlaps.argmax(axis=0)
        max_overlaps = overlaps.max(axis=0)
        gt_ind = max_overlaps.argmax()
        gt_ovr = max_overlaps.max()
        if short is None:
            assert (gt_ovr >= 0)
        elif not gt_ovr >= 0:
            _gt_overlaps[j:] = short
            ran_short = True
            break
        box_ind = argmax_overlaps[gt_ind]
        _gt_overlaps[j] = overlaps[box_ind, gt_ind]
        assert (_gt_overlaps[j] == gt_ovr)
        overlaps[box_ind, :] = -1
        overlaps[:, gt_ind] = -1
    return _gt_overlaps, ran_short


def evaluate_recall(roidb, bbox_overlaps, candidate_boxes=None, thresholds=None, area='all', limit=None):
    """imdb.evaluate_recall over a list of roidb entries; raises AssertionError where the reference does."""
    assert area in AREAS, 'unknown area range: {}'.format(area)
    area_range = AREA_RANGES[AREAS[area]]
    gt_overlaps = np.zeros(0)
    num_pos = 0
    for i in range(len(roidb)):
        max_gt_overlaps = roidb[i]['gt_overlaps'].toarray().max(axis=1)
        gt_inds = np.where((roidb[i]['gt_classes'] > 0) & (max_gt_overlaps == 1))[0]
        gt_boxes = roidb[i]['boxes'][gt_inds, :]
        gt_areas = roidb[i]['seg_areas'][gt_inds]
        valid_gt_inds = np.where((gt_areas >= area_range[0]) & (gt_areas <= area_range[1]))[0]
        gt_boxes = gt_boxes[valid_gt_inds, :]
        num_pos += len(valid_gt_inds)
        if candidate_boxes is None:
            non_gt_inds = np.where(roidb[i]['gt_classes'] == 0)[0]
            boxes = roidb[i]['boxes'][non_gt_inds, :]
        else:
            boxes = candidate_boxes[i]
        if boxes.shape[0] == 0:
            continue
        if limit is not None and boxes.shape[0] > limit:
            boxes = boxes[:limit, :]
        gt_overlaps = np.hstack((gt_overlaps, match_frame(boxes, gt_boxes, bbox_overlaps)[0]))
    gt_overlaps = np.sort(gt_overlaps)
    if thresholds is None:
        step = 0.05
        thresholds = np.arange(0.5, 0.95 + 1e-5, step)
    recalls = np.zeros_like(thresholds)
    for i, t in enumerate(thresholds):
        recalls[i] = (gt_overlaps >= t).sum() / float(num_pos)
    ar = recalls.mean()
    return {'ar': ar, 'recalls': recalls, 'thresholds': thresholds, 'gt_overlaps': gt_overlaps}


def recall_vectors(boxes, gts, bbox_overlaps, limits=(None,), thresholds=None, on_short='raise'):
    """The contract of mv3d_proposal_recall on per-frame lists of (R, 4) boxes and (G, 4) objects (f32):
    -> gt_overlaps (L, G_total) f64, counts (L, T) int32, status (F) int32."""
    thresholds = np.arange(0.5, 0.95 + 1e-5, 0.05) if thresholds is None else np.asarray(thresholds, np.float64)
    F, L = len(boxes), len(limits)
    gt_off = np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int64)
    out = np.full((L, int(gt_off[-1])), -1.0)
    counts = np.zeros((L, len(thresholds)), np.int32)
    status = np.zeros(F, np.int32)
    for f in range(F):
        b, g = np.asarray(boxes[f], np.float32).reshape(-1, 4), np.asarray(gts[f], np.float32).reshape(-1, 4)
        if b.shape[0] == 0:
            continue                                                            # skipped: -1.0, counted nowhere
        finite = np.isfinite(b).all() and np.isfinite(g).all()
        for li, limit in enumerate(limits):
            if not finite:
                rec = np.zeros(g.shape[0])
                status[f] |= STATUS_NONFINITE
            else:
                rec, ran_short = match_frame(b if limit is None else b[:limit], g, bbox_overlaps, short=0.0 if on_short == 'zero' else -1.0)
                if ran_short and on_short != 'zero':
                    status[f] |= STATUS_SHORT
            out[li, gt_off[f]:gt_off[f + 1]] = rec
            for t, thr in enumerate(thresholds):
                counts[li, t] += int((rec >= thr).sum())
    return out, counts, status
