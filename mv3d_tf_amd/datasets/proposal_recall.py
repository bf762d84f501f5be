"""Proposal recall: how many ground-truth objects do the first N RPN proposals cover, at which IoU (lib/datasets/imdb.py:121-209
`evaluate_recall`, MV3D's first experiment), for a whole split and several N in ONE launch of mv3d_proposal_recall
(csrc/proposal_recall.hip).

The object selection is the reference's and runs on the host (it is G-sized): `gt_classes > 0`, `gt_overlaps.toarray().max(axis=1)
== 1` (no crowd rows) and the eight named area ranges with the reference's bounds.  The area of an object is
`roidb[i]['seg_areas']` where the roidb has it, otherwise (x2 - x1 + 1) * (y2 - y1 + 1) of the selected space's box stored as f32,
which is what lib/datasets/pascal_voc.py stores there.  The reference's own kitti_mv3d never sets `seg_areas`, so its
evaluate_recall could not run on this dataset at all (KeyError at imdb.py:156); here it can.

    python -m mv3d_tf_amd.datasets.proposal_recall --kitti <root> --image-set val --proposals <dir>/proposals.pkl
        [--limits 10,50,100,300,1000,2000] [--space bv] [--area all]

scores the proposals that rpn_msr.generate.imdb_proposals saved."""
import argparse
import pickle

import numpy as np

AREAS = {'all': 0, 'small': 1, 'medium': 2, 'large': 3, '96-128': 4, '128-256': 5, '256-512': 6, '512-inf': 7}
AREA_RANGES = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2], [96 ** 2, 128 ** 2], [128 ** 2, 256 ** 2],
               [256 ** 2, 512 ** 2], [512 ** 2, 1e5 ** 2]]                           # imdb.py:134-144
SPACES = {'bv': ('boxes_bv', 0), 'image': ('boxes', 1)}                               # roidb key, index into a `rois` triple
DEFAULT_LIMITS = (10, 50, 100, 300, 1000, 2000)


def _boxes4(a):
    a = np.asarray(a)
    if a.ndim != 2:
        a = a.reshape(-1, 4)
    return a[:, 1:5] if a.shape[1] == 5 else a


def select_indices(roidb, area='all', area_key='boxes_bv'):
    """imdb.py:149-160 -> per roidb entry the row indices of its selected objects: class > 0, no crowd row, and `seg_areas`
    (where the entry has them, else the f32 area of its `area_key` box) within the named range"""
    assert area in AREAS, 'unknown area range: {}'.format(area)
    lo, hi = AREA_RANGES[AREAS[area]]
    inds = []
    for entry in roidb:
        max_gt_overlaps = entry['gt_overlaps'].toarray().max(axis=1) if entry['gt_overlaps'].shape[0] else np.zeros(0)
        gt_inds = np.where((np.asarray(entry['gt_classes']) > 0) & (max_gt_overlaps == 1))[0]
        if 'seg_areas' in entry:
            gt_areas = np.asarray(entry['seg_areas'])[gt_inds]
        else:
            b = np.asarray(entry[area_key]).reshape(-1, 4)[gt_inds, :].astype(np.float64)
            gt_areas = ((b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)).astype(np.float32)
        inds.append(gt_inds[(gt_areas >= lo) & (gt_areas <= hi)])
    return inds


def select_objects(roidb, area='all', space='bv'):
    """imdb.py:149-160 -> (per-frame (G, 4) object boxes, num_pos)"""
    key = SPACES[space][0]
    inds = select_indices(roidb, area, key)
    return [np.asarray(e[key]).reshape(-1, 4)[i, :] for e, i in zip(roidb, inds)], sum(len(i) for i in inds)


def launch_split(split_cls, op, widths, boxes, gts, limits, thresholds, on_short):
    """per-frame row / object lists -> host (gt_overlaps, counts) of `op` on one `split_cls` of ops: one upload, the launches of
    one call, one read-back; `widths`: the columns of the empty (row, object) arrays of a call without frames"""
    import torch
    from .. import ops
    from ..fast_rcnn.config import cfg
    dev = next((b.device for b in boxes if isinstance(b, torch.Tensor) and b.is_cuda), None) or torch.device("cuda", cfg.GPU_ID)
    box_off = np.concatenate([[0], np.cumsum([b.shape[0] for b in boxes])])
    gt_off = np.concatenate([[0], np.cumsum([g.shape[0] for g in gts])])
    if boxes and all(isinstance(b, torch.Tensor) for b in boxes):
        allb = torch.cat([b.to(dev) for b in boxes])
    else:
        host = [b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b) for b in boxes]
        allb = np.concatenate(host) if host else np.zeros((0, widths[0]), np.float32)
    allg = np.concatenate(gts) if gts else np.zeros((0, widths[1]), np.float32)
    ov, counts, _ = ops.proposal_recall_host(op(split_cls(allb, box_off, allg, gt_off, dev), limits, thresholds, on_short))
    return ov, counts


def _launch(boxes, gts, limits, thresholds, on_short):
    """per-frame box / object lists -> host (gt_overlaps (L, G), counts (L, T)): one upload, one launch, one read-back"""
    from .. import ops
    return launch_split(ops.RecallSplit, ops.proposal_recall, (4, 4), boxes, gts, limits, thresholds, on_short)


def result_dicts(ov, counts, kept, num_pos, thresholds, limits):
    """(gt_overlaps (L, G), counts (L, T)) of one metric -> the reference's result dictionary per limit; `kept`: the objects of
    frames that have boxes (the reference skips the others; they still count in num_pos)"""
    results = []
    for li in range(len(limits)):
        with np.errstate(divide='ignore', invalid='ignore'):
            recalls = np.asarray(counts[li], np.int64) / np.float64(num_pos)
        results.append({'ar': recalls.mean(), 'recalls': recalls, 'thresholds': thresholds,
                        'gt_overlaps': np.sort(np.asarray(ov[li], np.float64)[kept])})
    return results


def kept_objects(boxes, gts):
    return np.concatenate([np.full(g.shape[0], b.shape[0] > 0) for b, g in zip(boxes, gts)]) if gts else np.zeros(0, bool)


def evaluate_recall(roidb, candidate_boxes, thresholds=None, area='all', limit=None, space='bv', on_short='raise'):
    """imdb.evaluate_recall on the device -> {'ar', 'recalls', 'thresholds', 'gt_overlaps'} as the reference returns them
    (`gt_overlaps` sorted, without the objects of frames that have no box, which the reference skips; they still count in
    num_pos).  `limit`: None, an int, or a sequence of those -> a list of one dictionary per limit, all from ONE launch.
    candidate_boxes: per-frame (R, 4) or (R, 5) arrays / device tensors in proposal order, the {'bv', 'image'} dictionary
    imdb_proposals returns, or None = the roidb's own class-0 boxes as in the reference (kitti_mv3d's roidb has none: every
    frame is skipped, recalls are 0).  space: 'bv' matches against roidb['boxes_bv'], 'image' against roidb['boxes'].
    on_short: a frame with fewer boxes than selected objects raises AssertionError as the reference's assert does ('raise'), or
    counts the objects left over as misses ('zero': this repository's definition for sweeps over small limits, NOT the
    reference's)."""
    if space not in SPACES:
        raise ValueError("space is 'bv' or 'image'")
    many = isinstance(limit, (list, tuple, np.ndarray))
    limits = list(limit) if many else [limit]
    key = SPACES[space][0]
    gts, num_pos = select_objects(roidb, area, space)
    if isinstance(candidate_boxes, dict):
        candidate_boxes = candidate_boxes[space]
    if candidate_boxes is None:
        boxes = [np.asarray(e[key]).reshape(-1, 4)[np.where(np.asarray(e['gt_classes']) == 0)[0], :] for e in roidb]
    else:
        assert len(candidate_boxes) == len(roidb), 'Number of boxes must match number of ground-truth images'
        boxes = [b if hasattr(b, 'is_cuda') else _boxes4(b) for b in candidate_boxes]
    if thresholds is None:
        step = 0.05
        thresholds = np.arange(0.5, 0.95 + 1e-5, step)
    thresholds = np.asarray(thresholds, np.float64)
    ov, counts = _launch(boxes, gts, limits, thresholds, on_short)
    results = result_dicts(ov, counts, kept_objects(boxes, gts), num_pos, thresholds, limits)
    return results if many else results[0]


def table(results, limits, thresholds=(0.5, 0.7)):
    """recall at the given IoU thresholds (the nearest evaluated one) and AR, one line per limit"""
    lines = ['{:>10s}'.format('proposals') + ''.join('{:>12s}'.format('recall@%.2f' % t) for t in thresholds) + '{:>10s}'.format('AR')]
    for lim, r in zip(limits, results):
        cols = [r['recalls'][int(np.argmin(np.abs(np.asarray(r['thresholds']) - t)))] for t in thresholds]
        lines.append('{:>10s}'.format('all' if lim is None else str(lim)) + ''.join('{:12.4f}'.format(c) for c in cols) +
                     '{:10.4f}'.format(r['ar']))
    return '\n'.join(lines)


def parse_limits(text):
    return [None if t in ('all', 'None', '0') else int(t) for t in text.split(',') if t]


def score_pickle(imdb, path, limits=DEFAULT_LIMITS, space='bv', area='all', on_short='zero'):
    """the saved proposals of imdb_proposals against imdb.roidb -> one result dictionary per limit"""
    with open(path, 'rb') as f:
        proposals = pickle.load(f)
    return evaluate_recall(imdb.roidb, proposals, area=area, limit=list(limits), space=space, on_short=on_short)


def parser():
    ap = argparse.ArgumentParser(description="proposal recall of saved RPN proposals (proposals.pkl of imdb_proposals)")
    ap.add_argument("--kitti", required=True, help="KITTI root (holds object/ and ImageSets/)")
    ap.add_argument("--image-set", default="val")
    ap.add_argument("--proposals", required=True, help="proposals.pkl written by rpn_msr.generate.imdb_proposals")
    ap.add_argument("--limits", type=parse_limits, default=list(DEFAULT_LIMITS), help="comma separated, 'all' = every proposal")
    ap.add_argument("--space", choices=sorted(SPACES), default="bv")
    ap.add_argument("--area", choices=sorted(AREAS), default="all")
    ap.add_argument("--on-short", choices=("raise", "zero"), default="zero",
                    help="frames with fewer proposals than objects: 'zero' counts the objects left over as misses (not the "
                         "reference's behaviour), 'raise' fails like the reference's assert")
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    from .kitti_mv3d import kitti_mv3d
    imdb = kitti_mv3d(a.image_set, a.kitti)
    results = score_pickle(imdb, a.proposals, a.limits, a.space, a.area, a.on_short)
    print(table(results, a.limits))
    return results


if __name__ == "__main__":
    main()
