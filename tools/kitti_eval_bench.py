"""KITTI evaluator timing on the synthetic KITTI-val-sized split (3 769 frames x 300 detections x 10 objects): event-timed
device time of each launch (overlap, pass 1, pass 2), the host threshold step, and the end-to-end `evaluate()` wall time
with the ground truth already loaded and a warm-up done.  With '2d' or 'aos' in --metrics, the same for the 2D launches
(image boxes, 2D pass 1, 2D pass 2) on `synth.kitti_eval_split_2d` (3 DontCare boxes per frame).  Prints one JSON line.

    python tools/kitti_eval_bench.py [--frames 3769] [--dets 300] [--objects 10] [--reps 5] [--metrics bev,3d,2d,aos]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mv3d_tf_amd import build, ops, synth  # noqa: E402
from mv3d_tf_amd.datasets import kitti_eval as KE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--objects", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--metrics", default="bev,3d")
    a = ap.parse_args()
    metrics = KE._check_metrics(m for m in a.metrics.split(",") if m)
    build.build()
    out = {"bench": "kitti_eval", "frames": a.frames, "dets_per_frame": a.dets, "objects_per_frame": a.objects, "reps": a.reps,
           "metrics": ",".join(metrics), "device": torch.cuda.get_device_name(0)}
    if "bev" in metrics or "3d" in metrics:
        out.update(bench_3d(a))
    if "2d" in metrics or "aos" in metrics:
        out.update(bench_2d(a, metrics))
    print(json.dumps(out))


def _med(v):
    return float(np.median(v))


def bench_2d(a, metrics):
    dets, gts, calibs = synth.kitti_eval_split_2d(7, F=a.frames, D=a.dets, G=a.objects, K=3)
    dev = torch.device("cuda", 0)
    KE.evaluate(dets, gts, calibs, metrics=metrics)                      # warm-up
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        KE.evaluate(dets, gts, calibs, metrics=metrics)
        wall.append(time.perf_counter() - t0)
    det = np.concatenate(dets)
    det_off = np.concatenate([[0], np.cumsum([len(d) for d in dets])]).astype(np.int32)
    gt_off = np.concatenate([[0], np.cumsum([len(g['cls']) for g in gts])]).astype(np.int32)
    attr = np.concatenate([np.stack([g['truncation'], g['occlusion'], g['boxes'][:, 1], g['boxes'][:, 3]], 1) for g in gts])
    sp = ops.KittiEvalSplit(det[:, :24], det[:, 24], det_off, np.asarray(calibs, np.float32), np.concatenate([g['corners'] for g in gts]),
                            gt_off, np.concatenate([g['cls'] for g in gts]), attr, dev)
    dc_off = np.concatenate([[0], np.cumsum([len(g['dontcare']) for g in gts])]).astype(np.int32)
    im = ops.KittiImageSplit(sp, np.concatenate([g['boxes'] for g in gts]), np.concatenate([g['alpha'] for g in gts]), dc_off,
                             np.concatenate([g['dontcare'] for g in gts]), np.tile(np.int32(KE.IMAGE_SHAPE), (a.frames, 1)))
    box, cam = ops.kitti_eval_image_boxes(sp, im)
    m = ops.kitti_eval_match_2d(sp, im, box, 0, 1, 0.7).cpu().numpy()
    flags = [KE.gt_flags(np.concatenate([g['cls'] for g in gts]), attr[:, 0], attr[:, 1], attr[:, 2], attr[:, 3], d, 0, 1) for d in range(3)]
    thr, nthr = KE.threshold_tables(m, [int((fl == 0).sum()) for fl in flags])
    d_thr, d_nthr = ops.upload_packed([thr, nthr], dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t_box, t_p1, t_p2 = [], [], []
    for _ in range(a.reps + 1):
        ev[0].record()
        box, cam = ops.kitti_eval_image_boxes(sp, im)
        ev[1].record()
        ops.kitti_eval_match_2d(sp, im, box, 0, 1, 0.7)
        ev[2].record()
        ops.kitti_eval_count_2d(sp, im, box, cam, 0, 1, 0.7, d_thr, d_nthr)
        ev[3].record()
        torch.cuda.synchronize()
        t_box.append(ev[0].elapsed_time(ev[1]))
        t_p1.append(ev[1].elapsed_time(ev[2]))
        t_p2.append(ev[2].elapsed_time(ev[3]))
    t_box, t_p1, t_p2 = t_box[1:], t_p1[1:], t_p2[1:]
    return {"image_box_ms": round(_med(t_box), 3), "pass1_2d_ms": round(_med(t_p1), 3), "pass2_2d_ms": round(_med(t_p2), 3),
            "kernel_2d_ms": round(_med(t_box) + _med(t_p1) + _med(t_p2), 3), "evaluate_2d_wall_ms": round(1e3 * _med(wall), 3),
            "dontcare_boxes": int(dc_off[-1])}


def bench_3d(a):
    dets, gts, calibs = synth.kitti_eval_split(7, F=a.frames, D=a.dets, G=a.objects)
    dev = torch.device("cuda", 0)
    KE.evaluate(dets, gts, calibs)                                       # warm-up
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        KE.evaluate(dets, gts, calibs)
        wall.append(time.perf_counter() - t0)
    # the launches alone, on one uploaded split
    det = np.concatenate(dets)
    det_off = np.concatenate([[0], np.cumsum([len(d) for d in dets])]).astype(np.int32)
    gt_off = np.concatenate([[0], np.cumsum([len(g['cls']) for g in gts])]).astype(np.int32)
    attr = np.concatenate([np.stack([g['truncation'], g['occlusion'], g['boxes'][:, 1], g['boxes'][:, 3]], 1) for g in gts])
    sp = ops.KittiEvalSplit(det[:, :24], det[:, 24], det_off, np.asarray(calibs, np.float32), np.concatenate([g['corners'] for g in gts]),
                            gt_off, np.concatenate([g['cls'] for g in gts]), attr, dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t_ov, t_p2, t_host = [], [], []
    for _ in range(a.reps):
        ev[0].record()
        iou, height = ops.kitti_eval_overlaps(sp)
        ev[1].record()
        matched = ops.kitti_eval_match(sp, iou, height, 0, 1, 0.7)
        ev[2].record()
        m = matched.cpu().numpy()
        h0 = time.perf_counter()
        flags = [KE.gt_flags(np.concatenate([g['cls'] for g in gts]), attr[:, 0], attr[:, 1], attr[:, 2], attr[:, 3], d, 0, 1)
                 for d in range(3)]
        thr, nthr = KE.threshold_tables(m, [int((fl == 0).sum()) for fl in flags])
        t_host.append(time.perf_counter() - h0)
        d_thr, d_nthr = ops.upload_packed([thr, nthr], dev)
        ev[2].record()
        ops.kitti_eval_count(sp, iou, height, 0, 1, 0.7, d_thr, d_nthr)
        ev[3].record()
        torch.cuda.synchronize()
        t_ov.append(ev[0].elapsed_time(ev[1]))
        t_p2.append(ev[2].elapsed_time(ev[3]))
    # pass 1 alone (the host step above sits between its events)
    p1 = []
    for _ in range(a.reps):
        ev[0].record()
        ops.kitti_eval_match(sp, iou, height, 0, 1, 0.7)
        ev[1].record()
        torch.cuda.synchronize()
        p1.append(ev[0].elapsed_time(ev[1]))
    med = _med
    kernel_ms = med(t_ov) + med(p1) + med(t_p2)
    return {"pairs": sp.num_pairs, "overlap_ms": round(med(t_ov), 3), "pass1_ms": round(med(p1), 3),
            "pass2_ms": round(med(t_p2), 3), "kernel_ms": round(kernel_ms, 3),
            "host_thresholds_ms": round(1e3 * med(t_host), 3), "evaluate_wall_ms": round(1e3 * med(wall), 3),
            "pairs_per_s_overlap": round(sp.num_pairs / (med(t_ov) * 1e-3)),
            "pairs_per_s_evaluate": round(sp.num_pairs / med(wall))}


if __name__ == "__main__":
    main()
