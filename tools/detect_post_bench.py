"""Test-time detection tail (score cut, NMS, cap) of a batch of frames, host path against device path, from device arrays ready
to per-frame lists on the host.  In ONE process, alternating A / B so that both see the same machine state, on seeded inputs:

  A = the four arrays to the host, then test_mv.class_detections + limit_detections per frame (one mv3d_nms_host per frame and class);
  B = ops.detect_post + the compact read-back (ops.detect_post_lists).

A's and B's lists are asserted equal before anything is timed.  Each variant runs --reps windows of >= --seconds after a warm-up;
median, minimum and maximum of the per-call time are reported, plus the event-timed device time of the detect_post launches alone.
--serve adds the ServeGraph replay (MV3D_test_3view, f16 MFMA trunks, TEST cfg 6000 -> 300) with `post` on and off.
--profile-loop N only enqueues N detect_post calls per size (for a `rocprofv3 --kernel-trace --stats -- python tools/...` run).
Prints one JSON line; --out also writes it to a file.

    python tools/detect_post_bench.py [--batch 16] [--rows 300,2000] [--classes 2] [--max-per-image 300] [--nms 0.1] [--serve]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mv3d_tf_amd import build, ops, synth  # noqa: E402
from mv3d_tf_amd.fast_rcnn import detect_batch, test_mv  # noqa: E402
from mv3d_tf_amd.fast_rcnn.config import cfg  # noqa: E402


def inputs(seed, B, rows, K):
    """scores ** 3 and boxes of 8 - 40 px in a 600 px field, as the parity tests draw them"""
    rng = np.random.RandomState(seed)
    R = B * rows
    scores = rng.random_sample((R, K)).astype(np.float32) ** 3
    scores[:, 0] = 1 - scores[:, 1:].max(1)
    ctr = rng.uniform(20, 580, (R, 1, 2)); wh = rng.uniform(8, 40, (R, K, 2))
    bx = np.concatenate([ctr - wh / 2, ctr + wh / 2], 2).reshape(R, 4 * K).astype(np.float32)
    cnr = rng.uniform(-30, 60, (R, 24)).astype(np.float32)
    cnr_r = (np.hstack([cnr] * K) + rng.uniform(-1, 1, (R, 24 * K))).astype(np.float32)
    return [torch.as_tensor(a).cuda() for a in (scores, bx, cnr, cnr_r)]


def host_path(dev_arrays, B, rows, K, mpi):
    scores, bx, cnr, cnr_r = (t.cpu().numpy() for t in dev_arrays)
    frames = []
    for f in range(B):
        sl = slice(f * rows, (f + 1) * rows)
        dets, dets_cnr, _ = test_mv.class_detections(scores[sl], bx[sl].astype(np.float64), np.hstack([cnr[sl]] * K), cnr_r[sl], K, 0.05)
        frames.append(test_mv.limit_detections(dets, dets_cnr, mpi))
    return frames


def windows(fn, seconds, reps_hint):
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


def bench_size(a, rows):
    B, K, mpi = a.batch, a.classes, a.max_per_image
    arrays = inputs(100 + rows, B, rows, K)
    out = ops.detect_post_outputs(B, K, rows, arrays[0].device)

    def device_path():
        return ops.detect_post_lists(ops.detect_post(*arrays, None, rows, K, mpi, cfg.TEST.NMS, out=out))

    A, Bv = host_path(arrays, B, rows, K, mpi), device_path()
    kept = 0
    for (da, ca), (db, cb) in zip(A, Bv):
        for j in range(1, K):
            assert np.array_equal(da[j], db[j]) and np.array_equal(ca[j], cb[j]), "host and device tails differ"
            kept += len(da[j])
    if a.profile_loop:
        for _ in range(a.profile_loop):
            ops.detect_post(*arrays, None, rows, K, mpi, cfg.TEST.NMS, out=out)
        torch.cuda.synchronize()
        return {"rows": rows, "profile_loop": a.profile_loop}
    ta, tb = [], []
    for _ in range(a.reps):
        ta.append(windows(lambda: host_path(arrays, B, rows, K, mpi), a.seconds, 1))
        tb.append(windows(device_path, a.seconds, 8))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kern = []
    for _ in range(a.reps):
        ev[0].record()
        for _ in range(50):
            ops.detect_post(*arrays, None, rows, K, mpi, cfg.TEST.NMS, out=out)
        ev[1].record()
        torch.cuda.synchronize()
        kern.append(ev[0].elapsed_time(ev[1]) * 1e-3 / 50)
    return {"rows": rows, "kept_detections": kept, "A_host_path": stats(ta), "B_detect_post": stats(tb),
            "B_launches_device_only": stats(kern), "B_below_A_by_more_than_A_spread": bool(np.median(ta) - np.median(tb) > max(ta) - min(ta))}


def bench_serve(a):
    from mv3d_tf_amd.networks import get_network
    B = a.batch
    rng = np.random.RandomState(200)
    feed = {"lidar_bv_data": torch.as_tensor(((rng.random_sample((B, 608, 608, 9)) < 0.03) * rng.uniform(0, 2.4, (B, 608, 608, 9))).astype(np.float32)).cuda(),
            "image_data": torch.as_tensor((rng.randint(0, 255, (B, 375, 1242, 3)) - cfg.PIXEL_MEANS).astype(np.float32)).cuda(),
            "lidar_fv_data": torch.as_tensor(rng.uniform(0, 1, (B, 64, 512, 3)).astype(np.float32)).cuda(),
            "im_info": np.array([[608, 608, 1]] * B, np.float32), "calib": np.stack([synth.KITTI_CALIB] * B), "keep_prob": 1.0}
    saved = (cfg.TEST.RPN_PRE_NMS_TOP_N, cfg.TEST.RPN_POST_NMS_TOP_N)
    cfg.TEST.RPN_PRE_NMS_TOP_N, cfg.TEST.RPN_POST_NMS_TOP_N = 6000, 300
    try:
        net = get_network("MV3D_test_3view")
        net.amp_dtype, net.mfma_trunk = torch.float16, True
        graphs = {"post_off": test_mv.ServeGraph(net, feed), "post_on": detect_batch.ServeGraph(net, feed, post=dict(max_per_image=a.max_per_image))}
        times = {k: [] for k in graphs}
        for _ in range(a.reps):
            for name, sg in graphs.items():
                def step():
                    sg.replay()
                    sg.stream.synchronize()
                step()
                times[name].append(windows(step, a.seconds, 4))
        return {"serve_graph_replay": {k: stats(v) for k, v in times.items()},
                "serve_graph_post_adds_ms": round(1e3 * float(np.median(times["post_on"]) - np.median(times["post_off"])), 4)}
    finally:
        cfg.TEST.RPN_PRE_NMS_TOP_N, cfg.TEST.RPN_POST_NMS_TOP_N = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rows", default="300,2000")
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--max-per-image", type=int, default=300)
    ap.add_argument("--nms", type=float, default=0.1)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--serve", action="store_true")
    ap.add_argument("--profile-loop", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    saved = cfg.TEST.NMS
    cfg.TEST.NMS = a.nms
    try:
        out = {"bench": "detect_post", "batch": a.batch, "classes": a.classes, "max_per_image": a.max_per_image, "nms": a.nms,
               "reps": a.reps, "window_s": a.seconds, "device": torch.cuda.get_device_name(0),
               "sizes": [bench_size(a, int(r)) for r in a.rows.split(",") if r]}
        if a.serve and not a.profile_loop:
            out.update(bench_serve(a))
    finally:
        cfg.TEST.NMS = saved
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
