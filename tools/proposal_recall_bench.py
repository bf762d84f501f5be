"""Proposal-recall timing on the synthetic KITTI-val-sized split (3 769 frames x 10 objects, 300 and 2000 proposals per frame,
limits 10 / 50 / 100 / 300 / 1000 / all in ONE launch): the event-timed kernel alone, the wall time from device arrays to the
result dictionaries (`datasets.proposal_recall.evaluate_recall` on per-frame device tensors), the same from host arrays, and the
host restatement (tests/recall_restatement.py with the oracle's bbox_overlaps) on the same box.  One warm-up, then --reps timed
repetitions, medians reported.  Prints one JSON line per proposal count and writes profiles/proposal_recall_bench.json.

    python tools/proposal_recall_bench.py [--frames 3769] [--objects 10] [--proposals 300,2000] [--reps 5] [--host-reps 1]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402
import scipy.sparse  # noqa: E402
import torch  # noqa: E402

from mv3d_tf_amd import build, ops, synth  # noqa: E402
from mv3d_tf_amd.datasets import proposal_recall as PR  # noqa: E402

LIMITS = [10, 50, 100, 300, 1000, None]


def _med(v):
    return float(np.median(v))


def bench(a, R, oracle, RR):
    boxes, gts = synth.recall_split(11, F=a.frames, R=R, G=a.objects)
    dev = torch.device("cuda", 0)
    roidb = [dict(boxes_bv=g, gt_classes=np.ones(len(g), np.int32),
                  gt_overlaps=scipy.sparse.csr_matrix(np.tile(np.float32([0, 1]), (len(g), 1)))) for g in gts]
    d_boxes = [torch.as_tensor(b).to(dev) for b in boxes]
    res = PR.evaluate_recall(roidb, d_boxes, limit=LIMITS, on_short="zero")           # warm-up
    torch.cuda.synchronize()
    wall_dev, wall_host = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        PR.evaluate_recall(roidb, d_boxes, limit=LIMITS, on_short="zero")
        wall_dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        PR.evaluate_recall(roidb, boxes, limit=LIMITS, on_short="zero")
        wall_host.append(time.perf_counter() - t0)
    # the launch alone, on one uploaded split
    box_off = np.concatenate([[0], np.cumsum([len(b) for b in boxes])])
    gt_off = np.concatenate([[0], np.cumsum([len(g) for g in gts])])
    sp = ops.RecallSplit(np.concatenate(boxes), box_off, np.concatenate(gts), gt_off, dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kern = []
    for _ in range(a.reps + 1):
        ev[0].record()
        out = ops.proposal_recall(sp, LIMITS, None, "zero")
        ev[1].record()
        torch.cuda.synchronize()
        kern.append(ev[0].elapsed_time(ev[1]))
    kern = kern[1:]                                          # (includes the two small uploads and memsets in front of the kernel)
    host = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        ov, counts, _ = RR.recall_vectors(boxes, gts, oracle.bbox_overlaps, LIMITS, None, "zero")
        host.append(time.perf_counter() - t0)
    h_ov, h_counts, _ = ops.proposal_recall_host(out)
    same = bool(np.array_equal(h_ov, ov) and np.array_equal(h_counts, counts))
    r = {"bench": "proposal_recall", "frames": a.frames, "objects_per_frame": a.objects, "proposals_per_frame": R,
         "limits": ["all" if v is None else v for v in LIMITS], "reps": a.reps, "device": torch.cuda.get_device_name(0),
         "kernel_ms": round(_med(kern), 3), "evaluate_recall_device_arrays_wall_ms": round(1e3 * _med(wall_dev), 3),
         "evaluate_recall_host_arrays_wall_ms": round(1e3 * _med(wall_host), 3), "host_restatement_wall_ms": round(1e3 * _med(host), 3),
         "host_reps": a.host_reps, "device_equals_restatement": same,
         "recall_at_0.5": [round(float(x["recalls"][0]), 4) for x in res], "ar": [round(float(x["ar"]), 4) for x in res]}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--objects", type=int, default=10)
    ap.add_argument("--proposals", default="300,2000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proposal_recall_bench.json"))
    a = ap.parse_args()
    build.build()
    import oracle
    import recall_restatement as RR
    oracle.build()
    runs = [bench(a, int(R), oracle, RR) for R in a.proposals.split(",") if R]
    with open(a.out, "w") as f:
        json.dump({"runs": runs}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
