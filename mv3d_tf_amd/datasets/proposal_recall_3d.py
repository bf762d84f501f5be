"""Proposal recall by oriented IoU: how many labelled objects do the first N 3D proposals cover, at which BEV / 3D IoU (MV3D's
proposal experiment: recall of the `(x, y, z, l, w, h)` LIDAR boxes of proposal_layer_3d over the number of proposals, at IoU
0.25 / 0.5).  The matching is lib/datasets/imdb.py:162-196 as in datasets/proposal_recall.py; the overlap is the KITTI evaluator's
oriented-box clip against the roidb's `boxes_corners`, BEV and 3D IoU from the same launches (mv3d_proposal_recall_3d,
csrc/proposal_recall_3d.hip).

The objects are the ones `proposal_recall.select_objects(roidb, area, 'bv')` selects (its areas are those of the BEV pixel boxes),
so a 'bv' table and a '3d' table are over the same objects and the same num_pos.

    python -m mv3d_tf_amd.datasets.proposal_recall_3d --kitti <root> --image-set val --proposals <dir>/proposals_3d.pkl
        [--limits 10,50,100,300,1000,2000] [--metric bev,3d] [--area all] [--on-short zero]

scores the 3D proposals that rpn_msr.generate.imdb_proposals(..., with_3d=True) saved."""
import argparse
import pickle

import numpy as np

from .proposal_recall import AREAS, DEFAULT_LIMITS, kept_objects, launch_split, parse_limits, result_dicts, select_indices, table

METRICS = ('bev', '3d')                                    # the planes of the device result, in this order
MAX_PAIRS = 2 ** 31 - 1
CLI_THRESHOLDS = np.concatenate([[0.25], np.arange(0.5, 0.95 + 1e-5, 0.05)])


def select_corners(roidb, area='all'):
    """-> (per-frame (G, 24) f32 LIDAR corners, num_pos): the rows of `boxes_corners` that proposal_recall.select_objects(roidb,
    area, 'bv') selects (imdb.py:149-160 on `boxes_bv`)."""
    inds = select_indices(roidb, area, 'boxes_bv')
    return [np.asarray(e['boxes_corners'], np.float32).reshape(-1, 24)[i, :] for e, i in zip(roidb, inds)], sum(len(i) for i in inds)


def _boxes3d(a):
    """one frame's proposals -> (R, 6) or (R, 24); a device tensor passes through (ops.Recall3dSplit strips a batch column)"""
    if hasattr(a, 'is_cuda'):
        return a
    a = np.asarray(a)
    if a.ndim != 2:
        a = a.reshape(-1, 6)
    return a[:, 1:7] if a.shape[1] == 7 else a


def _launch_3d(boxes, gts, limits, thresholds, on_short):
    """per-frame proposal / object-corner lists -> host (gt_overlaps (2, L, G), counts (2, L, T)): one upload, the two launches,
    one read-back"""
    from .. import ops
    return launch_split(ops.Recall3dSplit, ops.proposal_recall_3d, (6, 24), boxes, gts, limits, thresholds, on_short)


def frame_chunks(pairs, max_workspace_bytes):
    """consecutive frame ranges [(a, b)] whose (proposal, object) pairs fit the workspace (16 bytes a pair) and stay below 2^31"""
    cap = min(int(max_workspace_bytes) // 16, MAX_PAIRS)
    chunks, a, total = [], 0, 0
    for f, p in enumerate(pairs):
        p = int(p)
        if p > cap:
            raise ValueError("proposal recall 3d: frame {} alone has {} (proposal, object) pairs, more than max_workspace_bytes "
                             "/ 16 or 2^31 - 1 allow".format(f, p))
        if total + p > cap:
            chunks.append((a, f))
            a, total = f, 0
        total += p
    chunks.append((a, len(pairs)))
    return chunks


def evaluate_recall_3d(roidb, candidate_boxes, thresholds=None, area='all', limit=None, metric='3d', on_short='raise',
                       max_workspace_bytes=1 << 30):
    """imdb.evaluate_recall by oriented IoU on the device -> {'ar', 'recalls', 'thresholds', 'gt_overlaps'} as the reference returns
    them (`gt_overlaps` sorted, without the objects of frames that have no proposal, which the reference skips; they still count
    in num_pos).  `limit`: None, an int, or a sequence of those -> a list of one dictionary per limit.  `metric`: 'bev' or '3d', or
    a tuple of those -> {'bev': ..., '3d': ...}; both always come from the same launches.  candidate_boxes: per-frame (R, 6)
    x y z l w h, (R, 7) with the batch column in front, or (R, 24) corner arrays / device tensors in proposal order, or the
    dictionary imdb_proposals(..., with_3d=True) returns.  The objects are the rows of roidb['boxes_corners'] that space 'bv'
    selects.  on_short as in proposal_recall.evaluate_recall.  The frames are processed in consecutive chunks whose IoU workspace
    (16 bytes per pair) fits max_workspace_bytes: one launch pair per chunk, counts summed, overlaps concatenated in frame order."""
    many_metrics = isinstance(metric, (list, tuple))
    metrics = list(metric) if many_metrics else [metric]
    if not metrics or any(m not in METRICS for m in metrics):
        raise ValueError("metric is 'bev' or '3d', or a tuple of those")
    many = isinstance(limit, (list, tuple, np.ndarray))
    limits = list(limit) if many else [limit]
    gts, num_pos = select_corners(roidb, area)
    if isinstance(candidate_boxes, dict):
        candidate_boxes = candidate_boxes['3d']
    if candidate_boxes is None:
        raise ValueError("evaluate_recall_3d needs proposals: the roidb holds no 3D boxes other than its objects")
    assert len(candidate_boxes) == len(roidb), 'Number of boxes must match number of ground-truth images'
    boxes = [_boxes3d(b) for b in candidate_boxes]
    if thresholds is None:
        step = 0.05
        thresholds = np.arange(0.5, 0.95 + 1e-5, step)
    thresholds = np.asarray(thresholds, np.float64)
    ovs, counts = [], np.zeros((2, len(limits), thresholds.size), np.int64)
    for a, b in frame_chunks([bx.shape[0] * g.shape[0] for bx, g in zip(boxes, gts)], max_workspace_bytes):
        ov, c = _launch_3d(boxes[a:b], gts[a:b], limits, thresholds, on_short)
        ovs.append(np.asarray(ov, np.float64).reshape(2, len(limits), -1))
        counts += np.asarray(c, np.int64).reshape(counts.shape)
    ov = np.concatenate(ovs, axis=2)
    kept = kept_objects(boxes, gts)
    out = {}
    for m in metrics:
        mi = METRICS.index(m)
        results = result_dicts(ov[mi], counts[mi], kept, num_pos, thresholds, limits)
        out[m] = results if many else results[0]
    return out if many_metrics else out[metrics[0]]


def parse_metrics(text):
    m = tuple(t for t in text.split(',') if t)
    if not m or any(t not in METRICS for t in m):
        raise argparse.ArgumentTypeError("metrics are 'bev' and '3d', comma separated")
    return m


def score_pickle(imdb, path, limits=DEFAULT_LIMITS, metric=METRICS, area='all', on_short='zero'):
    """the saved 3D proposals of imdb_proposals(..., with_3d=True) against imdb.roidb -> {metric: one result dictionary per limit},
    at IoU 0.25 and the reference's ten thresholds from the same call; 'ar' is the mean over those ten only."""
    with open(path, 'rb') as f:
        proposals = pickle.load(f)
    res = evaluate_recall_3d(imdb.roidb, proposals, thresholds=CLI_THRESHOLDS, area=area, limit=list(limits), metric=tuple(metric),
                             on_short=on_short)
    for rows in res.values():
        for r in rows:
            r['ar'] = r['recalls'][1:].mean()
    return res


def parser():
    ap = argparse.ArgumentParser(description="recall of saved 3D RPN proposals by oriented BEV / 3D IoU (proposals_3d.pkl of "
                                             "imdb_proposals(..., with_3d=True))")
    ap.add_argument("--kitti", required=True, help="KITTI root (holds object/ and ImageSets/)")
    ap.add_argument("--image-set", default="val")
    ap.add_argument("--proposals", required=True, help="proposals_3d.pkl written by rpn_msr.generate.imdb_proposals(..., with_3d=True)")
    ap.add_argument("--limits", type=parse_limits, default=list(DEFAULT_LIMITS), help="comma separated, 'all' = every proposal")
    ap.add_argument("--metric", type=parse_metrics, default=METRICS, help="comma separated: bev, 3d")
    ap.add_argument("--area", choices=sorted(AREAS), default="all")
    ap.add_argument("--on-short", choices=("raise", "zero"), default="zero",
                    help="frames with fewer proposals than objects: 'zero' counts the objects left over as misses (not the "
                         "reference's behaviour), 'raise' fails like the reference's assert")
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    from .kitti_mv3d import kitti_mv3d
    imdb = kitti_mv3d(a.image_set, a.kitti)
    res = score_pickle(imdb, a.proposals, a.limits, a.metric, a.area, a.on_short)
    for m in a.metric:
        print('oriented {} IoU'.format('BEV' if m == 'bev' else '3D'))
        print(table(res[m], a.limits, thresholds=(0.25, 0.5, 0.7)))
    return res


if __name__ == "__main__":
    main()
