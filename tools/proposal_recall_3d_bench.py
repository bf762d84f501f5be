"""Timing of proposal recall by oriented IoU on the synthetic KITTI-val-sized split of synth.recall_split_3d (3 769 frames x 10
objects, 300 and 2000 proposals per frame, limits 10 / 50 / 100 / 300 / 1000 / all, both metrics): the event-timed overlap and match
launches on their own (mv3d_proposal_recall_3d_overlaps / _match on one uploaded split), the share of pairs that pass the extent
pretest and the overlap time per clipped pair (the yardstick: tools/kitti_eval_bench.py's overlap kernel, the same clip, per pair),
and the wall time of `datasets.proposal_recall_3d.evaluate_recall_3d` from per-frame device tensors and from host arrays to the
result dictionaries.  One warm-up, then --reps windows of >= --seconds each; median, minimum and maximum of the per-call time.
The first --check-frames frames are compared with the host restatement (tests/recall3d_restatement.py) before anything is timed.
Prints one JSON line per proposal count and writes profiles/proposal_recall_3d_bench.json.

    python tools/proposal_recall_3d_bench.py [--frames 3769] [--objects 10] [--proposals 300,2000] [--reps 5] [--seconds 1.0]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import scipy.sparse  # noqa: E402
import torch  # noqa: E402

from mv3d_tf_amd import _lib, build, ops, synth  # noqa: E402
from mv3d_tf_amd.datasets import proposal_recall_3d as P3  # noqa: E402

LIMITS = [10, 50, 100, 300, 1000, None]


def windows(fn, seconds, reps_hint=1):
    """per-call seconds of one window of >= `seconds`"""
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(reps_hint):
            fn()
        n += reps_hint
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n


def stats(v):
    return {"median_ms": round(1e3 * float(np.median(v)), 4), "min_ms": round(1e3 * min(v), 4), "max_ms": round(1e3 * max(v), 4)}


def event_windows(fn, seconds, reps):
    """event-timed per-call seconds of `reps` windows of >= `seconds` of back-to-back calls"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn(); torch.cuda.synchronize()
    ev[0].record(); fn(); ev[1].record(); torch.cuda.synchronize()
    n = max(1, int(seconds / max(ev[0].elapsed_time(ev[1]) * 1e-3, 1e-6)))
    out = []
    for _ in range(reps):
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]) * 1e-3 / n)
    return out


def bench(a, R, R3):
    boxes, gts = synth.recall_split_3d(11, F=a.frames, R=R, G=a.objects)
    dev = torch.device("cuda", 0)
    roidb = [dict(boxes_bv=np.tile(np.float32([10, 10, 49, 25]), (len(g), 1)), boxes_corners=g, gt_classes=np.ones(len(g), np.int32),
                  gt_overlaps=scipy.sparse.csr_matrix(np.tile(np.float32([0, 1]), (len(g), 1)))) for g in gts]
    d_boxes = [torch.as_tensor(b).to(dev) for b in boxes]
    kw = dict(limit=LIMITS, metric=("bev", "3d"), on_short="zero")
    res = P3.evaluate_recall_3d(roidb, d_boxes, thresholds=P3.CLI_THRESHOLDS, **kw)          # warm-up
    torch.cuda.synchronize()
    # parity on the first frames, and the share of pairs the pretest lets through (host, vectorised)
    k = min(a.check_frames, a.frames)
    box_off = np.concatenate([[0], np.cumsum([len(b) for b in boxes])])
    gt_off = np.concatenate([[0], np.cumsum([len(g) for g in gts])])
    sp_k = ops.Recall3dSplit(np.concatenate(boxes[:k]), box_off[:k + 1], np.concatenate(gts[:k]), gt_off[:k + 1], dev)
    got = ops.proposal_recall_3d_host(ops.proposal_recall_3d(sp_k, LIMITS, None, "zero"))
    want = R3.recall_vectors_3d(boxes[:k], gts[:k], LIMITS, None, "zero")
    same = bool(all(np.array_equal(x, y) for x, y in zip(got, want)))
    passed = sum(int(R3.pretest(R3.extents(R3.box6_corners(b)), R3.extents(g)).sum()) for b, g in zip(boxes, gts))
    # the two launches alone, on one uploaded split
    sp = ops.Recall3dSplit(np.concatenate(boxes), box_off, np.concatenate(gts), gt_off, dev)
    desc, ws, out = ops.recall3d_prepare(sp, LIMITS, None, "zero")
    ov, counts, status = out
    L, st = _lib.lib(), lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def overlap():
        _lib.check(L.mv3d_proposal_recall_3d_overlaps(C.byref(desc), ws.data_ptr(), status.data_ptr(), st()), "overlaps")

    def match():
        _lib.check(L.mv3d_proposal_recall_3d_match(C.byref(desc), ws.data_ptr(), ov.data_ptr(), counts.data_ptr(), status.data_ptr(), st()), "match")

    t_ov = event_windows(overlap, a.seconds, a.reps)
    t_ma = event_windows(match, a.seconds, a.reps)
    wall_dev, wall_host = [], []
    for _ in range(a.reps):
        wall_dev.append(windows(lambda: P3.evaluate_recall_3d(roidb, d_boxes, **kw), a.seconds))
        wall_host.append(windows(lambda: P3.evaluate_recall_3d(roidb, boxes, **kw), a.seconds))
    thr = list(np.round(P3.CLI_THRESHOLDS, 2))
    r = {"bench": "proposal_recall_3d", "frames": a.frames, "objects_per_frame": a.objects, "proposals_per_frame": R,
         "limits": ["all" if v is None else v for v in LIMITS], "reps": a.reps, "window_s": a.seconds, "device": torch.cuda.get_device_name(0),
         "pairs": sp.P, "pairs_passing_pretest": passed, "share_passing_pretest": round(passed / max(sp.P, 1), 5),
         "overlap_launch": stats(t_ov), "match_launch": stats(t_ma),
         "overlap_ns_per_pair": round(1e9 * float(np.median(t_ov)) / max(sp.P, 1), 4),
         "overlap_ns_per_clipped_pair": round(1e9 * float(np.median(t_ov)) / max(passed, 1), 3),
         "workspace_bytes": ops.proposal_recall_3d_workspace_bytes(sp.P),
         "evaluate_recall_3d_device_arrays_wall": stats(wall_dev), "evaluate_recall_3d_host_arrays_wall": stats(wall_host),
         "launch_pairs_per_evaluate_call": len(P3.frame_chunks([len(b) * len(g) for b, g in zip(boxes, gts)], 1 << 30)),
         "checked_frames": k, "device_equals_restatement": same}
    for m in ("bev", "3d"):
        r["recall_" + m] = {"at_%.2f" % t: [round(float(x["recalls"][thr.index(t)]), 4) for x in res[m]] for t in (0.25, 0.5, 0.7)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--objects", type=int, default=10)
    ap.add_argument("--proposals", default="300,2000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--check-frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proposal_recall_3d_bench.json"))
    a = ap.parse_args()
    build.build()
    import recall3d_restatement as R3
    runs = [bench(a, int(R), R3) for R in a.proposals.split(",") if R]
    with open(a.out, "w") as f:
        json.dump({"runs": runs}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
