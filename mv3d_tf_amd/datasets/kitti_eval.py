"""KITTI object evaluation on the device: AP of the bird's-eye-view box (AP_BEV) and of the 3D box (AP_3D) per class and
difficulty, the numbers MV3D is judged by, and on request the 2D table: AP of the image box (AP_2D) and the average
orientation similarity (AOS).

    python -m mv3d_tf_amd.datasets.kitti_eval --kitti <root> --image-set val --detections <dir>/detections_cnr.pkl \
        [--metrics bev,3d,2d,aos] [--write-results <dir>]

scores an existing `test_net` pickle (all_boxes_cnr[cls][frame] = (N, 25): 24 LIDAR corners + score) without running the
network again; --write-results also writes devkit-complete result lines (`write_results`).

The whole split goes to the device in one upload of packed CSR arrays; `mv3d_kitti_eval_overlaps` computes the oriented-box
IoUs of every (detection, object) pair of every frame and the detections' image heights, `mv3d_kitti_eval_match` runs the
devkit's first statistics pass (matched true-positive scores), the host picks <= 41 score thresholds from them
(`get_thresholds`), `mv3d_kitti_eval_count` runs the second pass for every threshold, and one download of the integer counts
gives precision, recall and AP.  The 2D metrics take each detection's image box and camera box from its corners
(`mv3d_kitti_eval_image_boxes`) and run the same two passes with the 2D IoU, the DontCare rule and the orientation similarity
(`mv3d_kitti_eval_match_2d`, `mv3d_kitti_eval_count_2d`).  The rules (restated from the public KITTI object devkit), the IoU convention of this project
(LIDAR-frame corners; values differ from the devkit's camera-frame boxes at the 1e-3 level) and the launch shapes:
DESIGN.md §3.12."""
import json
import os

import numpy as np
import torch

from .. import ops
from ..fast_rcnn.config import cfg

# class codes of the label types (any other type: OTHER); the neighbouring class whose objects are ignored, not missed
CLASS_CODES = {'Car': 0, 'Van': 1, 'Truck': 2, 'Pedestrian': 3, 'Person_sitting': 4, 'Cyclist': 5, 'Tram': 6, 'Misc': 7}
OTHER = 8
NEIGHBOR = {'Car': 'Van', 'Pedestrian': 'Person_sitting'}
MIN_OVERLAP = {'Car': 0.7, 'Pedestrian': 0.5, 'Cyclist': 0.5}
METRICS = ('bev', '3d')
ALL_METRICS = ('bev', '3d', '2d', 'aos')
DIFFICULTIES = ('easy', 'moderate', 'hard')
MIN_HEIGHT = (40, 25, 25)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = np.array([0.15, 0.30, 0.50], np.float32)
N_SAMPLE_PTS = 41
IMG_HEIGHT = 375            # the image the proposal layer clips to (ops.proposal_params' default), for the detections' height
IMAGE_SHAPE = (375, 1242)   # (H, W) the detections' image boxes are clipped to when a frame's shape is not given


def _device():
    return torch.device("cuda", cfg.GPU_ID)


def load_eval_labels(lines, calib):
    """Every object of one label file (all types: Van and Pedestrian matter for the ignore rules; DontCare rows kept apart) ->
    {'type', 'cls' int32 codes, 'truncation' f32, 'occlusion' f32, 'boxes' (G,4) f32 image box, 'corners' (G,24) f32 LIDAR
    corners, 'alpha' (G,) f32 observation angle, 'dontcare' (K,4) f32 image boxes of the DontCare rows}.  `calib`: the dict
    of `load_kitti_calib`.  The corners come from the roidb's own path (`parse_kitti_labels`, i.e. `mv3d_gt_encode`, one
    upload per frame)."""
    from .kitti_mv3d import parse_kitti_labels
    rows = [ln for ln in lines if ln.strip() and ln.split()[0] != 'DontCare']
    types = [ln.split()[0] for ln in rows]
    codes = {t: CLASS_CODES.get(t, OTHER) for t in types}
    ann = parse_kitti_labels(rows, calib['Tr_velo2cam'], codes, OTHER + 1)
    num = np.array([ln.split()[1:3] for ln in rows], dtype=np.float32).reshape(len(rows), 2)
    dc = [ln.split() for ln in lines if ln.strip() and ln.split()[0] == 'DontCare']
    dontcare = np.array([t[4:8] for t in dc], dtype=np.float64).reshape(len(dc), 4).astype(np.float32)
    return {'type': types, 'cls': ann['gt_classes'].astype(np.int32), 'truncation': num[:, 0], 'occlusion': num[:, 1],
            'boxes': ann['boxes'], 'corners': ann['boxes_corners'], 'alpha': ann['alphas'], 'dontcare': dontcare}


def gt_flags(cls, truncation, occlusion, y1, y2, diff, eval_class, neighbor_class):
    """Devkit ignore flag per object for one difficulty: 0 counted, 1 ignored, -1 skipped (the kernels' rule, vectorised)."""
    height = np.asarray(y2, np.float32).astype(np.float64) - np.asarray(y1, np.float32).astype(np.float64)
    hard = ((np.asarray(occlusion, np.float32) > np.float32(MAX_OCCLUSION[diff])) |
            (np.asarray(truncation, np.float32) > MAX_TRUNCATION[diff]) | (height <= MIN_HEIGHT[diff]))
    cls = np.asarray(cls)
    return np.where(cls == eval_class, np.where(hard, 1, 0), np.where(cls == neighbor_class, 1, -1)).astype(np.int32)


def get_thresholds(scores, n_gt):
    """The devkit's score thresholds: scores of the true positives in descending order, one kept whenever its recall is the
    nearest to the next of the 41 recall steps (1/40 apart); at most 41."""
    v = np.sort(np.asarray(scores, np.float32))[::-1]
    t, current = [], 0.0
    for i in range(len(v)):
        l_recall = (i + 1) / float(n_gt)
        r_recall = (i + 2) / float(n_gt) if i < len(v) - 1 else l_recall
        if (r_recall - current) < (current - l_recall) and i < len(v) - 1:
            continue
        t.append(v[i])
        current += 1.0 / (N_SAMPLE_PTS - 1.0)
    return np.array(t[:N_SAMPLE_PTS], np.float32)


def threshold_tables(matched, n_gt):
    """The host step between the passes: matched (..., 3, G) pass-1 slots and n_gt[di] counted objects per difficulty ->
    (thr (..., 3, 41) f32, nthr (..., 3) int32), `get_thresholds` of the true-positive scores of every (metric, difficulty)."""
    matched = np.asarray(matched)
    thr = np.zeros(matched.shape[:-1] + (N_SAMPLE_PTS,), np.float32)
    nthr = np.zeros(matched.shape[:-1], np.int32)
    for idx in np.ndindex(*nthr.shape):
        if n_gt[idx[-1]] > 0:
            t = get_thresholds(matched[idx][matched[idx] > -np.inf], n_gt[idx[-1]])
            thr[idx][:len(t)], nthr[idx] = t, len(t)
    return thr, nthr


def average_precision(counts, n_thresholds, recall_points=11):
    """counts (41, 3) tp | fp | fn of the first n_thresholds thresholds -> (AP in percent, precision (41), recall (41)).
    precision = tp / (tp + fp) (0 where nothing is counted), then the running maximum from the right; AP = mean of the
    precision at i = 0, 4, ..., 40 (11 points, the MV3D paper and the original devkit) or i = 1..40 (40 points)."""
    c = np.asarray(counts, np.float64)[:n_thresholds]
    prec, rec = np.zeros(N_SAMPLE_PTS), np.zeros(N_SAMPLE_PTS)
    tp, fp, fn = c[:, 0], c[:, 1], c[:, 2]
    with np.errstate(invalid='ignore', divide='ignore'):
        prec[:n_thresholds] = np.where(tp + fp > 0, tp / (tp + fp), 0.0)
        rec[:n_thresholds] = np.where(tp + fn > 0, tp / (tp + fn), 0.0)
    prec = np.maximum.accumulate(prec[::-1])[::-1]
    if recall_points == 11:
        ap = prec[0::4].sum() / 11.0 * 100.0
    elif recall_points == 40:
        ap = prec[1:].sum() / 40.0 * 100.0
    else:
        raise ValueError("recall_points: 11 or 40")
    return ap, prec, rec


def orientation_similarity(counts, similarity, n_thresholds, recall_points=11):
    """counts (41, 3) tp | fp | fn and similarity (41,) the frame-summed orientation similarity of the first n_thresholds
    thresholds -> (AOS in percent, the filtered AOS curve (41)).  aos = similarity / (tp + fp) (fp after the DontCare rule; 0
    where nothing is counted), then the running maximum from the right and the same sampling as `average_precision`."""
    c = np.asarray(counts, np.float64)[:n_thresholds]
    aos = np.zeros(N_SAMPLE_PTS)
    n = c[:, 0] + c[:, 1]
    with np.errstate(invalid='ignore', divide='ignore'):
        aos[:n_thresholds] = np.where(n > 0, np.asarray(similarity, np.float64)[:n_thresholds] / n, 0.0)
    aos = np.maximum.accumulate(aos[::-1])[::-1]
    if recall_points == 11:
        return aos[0::4].sum() / 11.0 * 100.0, aos
    if recall_points == 40:
        return aos[1:].sum() / 40.0 * 100.0, aos
    raise ValueError("recall_points: 11 or 40")


class EvalResult(dict):
    """{(class, 'bev' | '3d' | '2d' | 'aos', 'easy' | 'moderate' | 'hard'): AP (AOS) in percent}; .precision / .recall (41,)
    arrays, .counts (41, 3) tp | fp | fn and .thresholds under the same keys ('aos' keys: those of the 2D passes), and
    .similarity (41,) the filtered AOS curve under the 'aos' keys."""

    def __init__(self):
        super().__init__()
        self.precision, self.recall, self.counts, self.thresholds = {}, {}, {}, {}
        self.similarity = {}

    def table(self):
        lines = []
        for cls in sorted({k[0] for k in self}):
            lines.append('%-10s %8s %8s %8s' % (cls, 'easy', 'moderate', 'hard'))
            for m, name in (('bev', 'AP_BEV'), ('3d', 'AP_3D'), ('2d', 'AP_2D'), ('aos', 'AOS')):
                if (cls, m, DIFFICULTIES[0]) in self:
                    lines.append('%-10s %8.2f %8.2f %8.2f' % ((name,) + tuple(self[(cls, m, d)] for d in DIFFICULTIES)))
        return '\n'.join(lines)

    def to_json(self):
        return {'%s/%s/%s' % k: float(v) for k, v in self.items()}


def _frame_dets(d):
    a = np.zeros((0, 25), np.float32) if d is None or len(d) == 0 else np.asarray(d, np.float32).reshape(-1, 25)
    return a


def _check_metrics(metrics):
    metrics = tuple(metrics)
    bad = [m for m in metrics if m not in ALL_METRICS]
    if bad or not metrics:
        raise ValueError("KITTI evaluation: metrics are a non-empty subset of %s, not %s" % (ALL_METRICS, metrics))
    return metrics


def _image_shapes(image_shapes, F):
    if image_shapes is None:
        return np.tile(np.array(IMAGE_SHAPE, np.int32), (F, 1))
    shapes = np.asarray(image_shapes, np.int32).reshape(-1, 2)
    if len(shapes) != F:
        raise ValueError("KITTI evaluation: %d image shapes for %d frames" % (len(shapes), F))
    return shapes


def evaluate(dets_cnr, gts, calibs, classes=('Car',), min_overlap=None, recall_points=11, img_height=IMG_HEIGHT, metrics=METRICS,
             image_shapes=None):
    """dets_cnr: per class (a dict class -> per-frame list, or the per-frame list itself when one class is evaluated) the
    frame's (N, 25) detections: 24 LIDAR corners (x0..x7, y0..y7, z0..z7) and the score, as test_net's all_boxes_cnr[cls];
    gts: per frame `load_eval_labels`; calibs: per frame the (4, 12) calibration table (`pack_calib`).  metrics: any subset
    of 'bev', '3d', '2d', 'aos' ('2d' and 'aos' need the labels' 'alpha' and 'dontcare'); image_shapes: per frame (H, W) the
    detections' image boxes are clipped to (default IMAGE_SHAPE).
    Returns an EvalResult: {(cls, metric, 'easy' | 'moderate' | 'hard'): AP in percent} for the requested metrics, plus the
    curves."""
    metrics = _check_metrics(metrics)
    mo = dict(MIN_OVERLAP, **(min_overlap or {}))
    F = len(gts)
    if len(calibs) != F:
        raise ValueError("evaluate: %d label frames but %d calibration tables" % (F, len(calibs)))
    if not isinstance(dets_cnr, dict):
        if len(classes) != 1:
            raise ValueError("evaluate: detections of several classes are given as {class: per-frame list}")
        dets_cnr = {classes[0]: dets_cnr}
    dev = _device()
    gt_off = np.concatenate([[0], np.cumsum([len(g['cls']) for g in gts])]).astype(np.int32)
    gt_cnr = np.concatenate([np.asarray(g['corners'], np.float32).reshape(-1, 24) for g in gts] + [np.zeros((0, 24), np.float32)])
    gt_cls = np.concatenate([np.asarray(g['cls'], np.int32) for g in gts] + [np.zeros(0, np.int32)])
    gt_attr = np.concatenate([np.stack([g['truncation'], g['occlusion'], np.asarray(g['boxes'])[:, 1], np.asarray(g['boxes'])[:, 3]], 1)
                              .astype(np.float32).reshape(-1, 4) for g in gts] + [np.zeros((0, 4), np.float32)])
    calib = np.asarray(calibs, np.float32).reshape(F, 4, 12)
    image = None
    if '2d' in metrics or 'aos' in metrics:
        for key in ('alpha', 'dontcare'):
            if any(key not in g for g in gts):
                raise ValueError("evaluate: the 2D metrics need the labels' %r (load_eval_labels)" % key)
        dc = [np.asarray(g['dontcare'], np.float32).reshape(-1, 4) for g in gts]
        image = (np.concatenate([np.asarray(g['boxes'], np.float32).reshape(-1, 4) for g in gts] + [np.zeros((0, 4), np.float32)]),
                 np.concatenate([np.asarray(g['alpha'], np.float32).reshape(-1) for g in gts] + [np.zeros(0, np.float32)]),
                 np.concatenate([[0], np.cumsum([len(d) for d in dc])]).astype(np.int32),
                 np.concatenate(dc + [np.zeros((0, 4), np.float32)]), _image_shapes(image_shapes, F))
    res = EvalResult()
    for cls in classes:
        frames = dets_cnr[cls]
        if len(frames) != F:
            raise ValueError("evaluate: %d frames of %s detections for %d label frames" % (len(frames), cls, F))
        fd = [_frame_dets(d) for d in frames]
        det = np.concatenate(fd + [np.zeros((0, 25), np.float32)])
        det_off = np.concatenate([[0], np.cumsum([len(d) for d in fd])]).astype(np.int32)
        code, nb = CLASS_CODES.get(cls, OTHER), CLASS_CODES.get(NEIGHBOR.get(cls), -1)
        sp = ops.KittiEvalSplit(det[:, :24], det[:, 24], det_off, calib, gt_cnr, gt_off, gt_cls, gt_attr, dev, img_height)
        if image is not None:
            _evaluate_2d(res, metrics, cls, sp, ops.KittiImageSplit(sp, *image), code, nb, mo[cls], gt_cls, gt_attr, recall_points)
        if 'bev' not in metrics and '3d' not in metrics:
            continue
        iou, height = ops.kitti_eval_overlaps(sp)
        matched = ops.kitti_eval_match(sp, iou, height, code, nb, mo[cls]).cpu().numpy()
        n_gt = [int((gt_flags(gt_cls, gt_attr[:, 0], gt_attr[:, 1], gt_attr[:, 2], gt_attr[:, 3], di, code, nb) == 0).sum())
                for di in range(3)]
        thr, nthr = threshold_tables(matched, n_gt)
        d_thr, d_nthr = ops.upload_packed([thr, nthr], dev)
        counts = ops.kitti_eval_count(sp, iou, height, code, nb, mo[cls], d_thr, d_nthr).cpu().numpy()
        for mi, m in enumerate(METRICS):
            if m not in metrics:
                continue
            for di, dname in enumerate(DIFFICULTIES):
                key = (cls, m, dname)
                ap, prec, rec = average_precision(counts[mi, di], nthr[mi, di], recall_points)
                res[key] = ap
                res.precision[key], res.recall[key] = prec, rec
                res.counts[key], res.thresholds[key] = counts[mi, di], thr[mi, di, :nthr[mi, di]]
    return res


def _evaluate_2d(res, metrics, cls, sp, im, code, nb, min_overlap, gt_cls, gt_attr, recall_points):
    """The 2D passes of one class: AP_2D and / or AOS into `res`."""
    box, cam = ops.kitti_eval_image_boxes(sp, im)
    matched = ops.kitti_eval_match_2d(sp, im, box, code, nb, min_overlap).cpu().numpy()
    n_gt = [int((gt_flags(gt_cls, gt_attr[:, 0], gt_attr[:, 1], gt_attr[:, 2], gt_attr[:, 3], di, code, nb) == 0).sum())
            for di in range(3)]
    thr, nthr = threshold_tables(matched, n_gt)
    d_thr, d_nthr = ops.upload_packed([thr, nthr], sp.device)
    counts, sim = ops.kitti_eval_count_2d(sp, im, box, cam, code, nb, min_overlap, d_thr, d_nthr)
    counts, sim = counts.cpu().numpy(), sim.cpu().numpy()
    # frames summed in frame order (add.accumulate is sequential): deterministic, and the restatement's order
    sim_sum = np.cumsum(sim, axis=0)[-1] if len(sim) else np.zeros((3, N_SAMPLE_PTS))
    for di, dname in enumerate(DIFFICULTIES):
        ap, prec, rec = average_precision(counts[di], nthr[di], recall_points)
        for m in ('2d', 'aos'):
            if m not in metrics:
                continue
            key = (cls, m, dname)
            if m == '2d':
                res[key] = ap
            else:
                res[key], res.similarity[key] = orientation_similarity(counts[di], sim_sum[di], nthr[di], recall_points)
            res.precision[key], res.recall[key] = prec, rec
            res.counts[key], res.thresholds[key] = counts[di], thr[di, :nthr[di]]


def _per_class(dets, class_name):
    return dets if isinstance(dets, dict) else {class_name: dets}


def detection_boxes(dets, calibs, image_shapes=None):
    """dets: per frame the (N, 25) (or (N, 24)) LIDAR-corner detections; calibs: per frame the (4, 12) table -> (boxes, cams):
    per frame the (N, 4) f64 image box x1 y1 x2 y2 (clipped to the frame's image; all zeros when the box cannot be formed)
    and the (N, 8) f64 camera box h w l x y z ry alpha, both from `mv3d_kitti_eval_image_boxes`."""
    F = len(dets)
    if len(calibs) != F:
        raise ValueError("detection_boxes: %d detection frames but %d calibration tables" % (F, len(calibs)))
    fd = [np.zeros((0, 24), np.float32) if d is None or len(d) == 0 else np.asarray(d, np.float32).reshape(len(d), -1)[:, :24]
          for d in dets]
    det = np.concatenate(fd + [np.zeros((0, 24), np.float32)])
    det_off = np.concatenate([[0], np.cumsum([len(d) for d in fd])]).astype(np.int32)
    zeros = np.zeros(F + 1, np.int32)
    sp = ops.KittiEvalSplit(det, np.zeros(len(det), np.float32), det_off, np.asarray(calibs, np.float32).reshape(F, 4, 12),
                            np.zeros((0, 24), np.float32), zeros, np.zeros(0, np.int32), np.zeros((0, 4), np.float32), _device())
    im = ops.KittiImageSplit(sp, np.zeros((0, 4), np.float32), np.zeros(0, np.float32), zeros, np.zeros((0, 4), np.float32),
                             _image_shapes(image_shapes, F))
    box, cam = ops.kitti_eval_image_boxes(sp, im)
    box, cam = box.cpu().numpy(), cam.cpu().numpy()
    return ([box[det_off[f]:det_off[f + 1]] for f in range(F)], [cam[det_off[f]:det_off[f + 1]] for f in range(F)])


def write_results(names, dets, calibs, out_dir, class_name='Car', image_shapes=None):
    """One <out_dir>/<name>.txt per frame in the KITTI devkit's result format, every field filled:
    `type -1 -1 alpha x1 y1 x2 y2 h w l x y z ry score` (the image and camera boxes of `detection_boxes`).  dets: per frame
    the (N, 25) detections of `class_name`, or {class: per-frame list} for several classes.  (The reference-format files of
    `kitti_mv3d.evaluate_detections` are written as before.)"""
    per = _per_class(dets, class_name)
    boxes = {c: detection_boxes(d, calibs, image_shapes) for c, d in per.items()}
    os.makedirs(out_dir, exist_ok=True)
    for f, name in enumerate(names):
        with open(os.path.join(out_dir, name + '.txt'), 'wt') as out:
            for c, d in per.items():
                sc = _frame_dets(d[f])[:, 24]
                for b, k, s in zip(boxes[c][0][f], boxes[c][1][f], sc):
                    out.write('%s -1 -1 %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.6f\n'
                              % ((c, k[7]) + tuple(b) + tuple(k[:7]) + (s,)))
    return out_dir


def evaluate_split(imdb, all_boxes3D, output_dir=None, recall_points=11, metrics=METRICS):
    """Scores test_net's all_boxes_cnr against the split's label_2 files, each frame's calibration loaded by its index name;
    prints the AP table and, with an output_dir, writes it to <output_dir>/kitti_ap.json.  metrics: as `evaluate`."""
    from .kitti_mv3d import load_kitti_calib, pack_calib
    gts, calibs = [], []
    for index in imdb.image_index:
        c = load_kitti_calib(os.path.join(imdb._dir('calib'), index + '.txt'))
        with open(os.path.join(imdb._data_path, 'training', 'label_2', index + '.txt')) as f:
            gts.append(load_eval_labels(f.readlines(), c))
        calibs.append(pack_calib(c))
    classes = [c for c in imdb.classes if c != '__background__']
    dets = {c: all_boxes3D[imdb.classes.index(c)] for c in classes}
    res = evaluate(dets, gts, calibs, classes=classes, recall_points=recall_points, metrics=metrics)
    print(res.table())
    if output_dir is not None:
        with open(os.path.join(output_dir, 'kitti_ap.json'), 'w') as f:
            json.dump(res.to_json(), f, indent=1, sort_keys=True)
    return res


def main(argv=None):
    import argparse
    import pickle
    from .kitti_mv3d import kitti_mv3d
    ap = argparse.ArgumentParser(description="AP_BEV / AP_3D (and AP_2D / AOS) of a test_net detections_cnr.pkl on a KITTI split")
    ap.add_argument('--kitti', required=True, help="KITTI root (object/, ImageSets/)")
    ap.add_argument('--image-set', default='val')
    ap.add_argument('--detections', required=True, help="detections_cnr.pkl written by test_net")
    ap.add_argument('--recall-points', type=int, default=11, choices=(11, 40))
    ap.add_argument('--metrics', default=','.join(METRICS), help="comma-separated subset of %s" % ','.join(ALL_METRICS))
    ap.add_argument('--write-results', metavar='DIR', help="also write devkit-complete result files (write_results) to DIR")
    args = ap.parse_args(argv)
    metrics = _check_metrics(m for m in args.metrics.split(',') if m)
    with open(args.detections, 'rb') as f:
        all_boxes_cnr = pickle.load(f)
    imdb = kitti_mv3d(args.image_set, args.kitti)
    if args.write_results:
        from .kitti_mv3d import load_kitti_calib, pack_calib
        calibs = [pack_calib(load_kitti_calib(os.path.join(imdb._dir('calib'), i + '.txt'))) for i in imdb.image_index]
        dets = {c: all_boxes_cnr[imdb.classes.index(c)] for c in imdb.classes if c != '__background__'}
        write_results(imdb.image_index, dets, calibs, args.write_results)
    return evaluate_split(imdb, all_boxes_cnr, os.path.dirname(os.path.abspath(args.detections)), args.recall_points, metrics)


if __name__ == '__main__':
    main()
