"""Scan augmentation's transform of the points (ops.scan_transform, csrc/scan_transform.hip): what the launch
costs, a torch restatement of it as the yardstick, and the training step with cfg.TRAIN.SCAN_AUGMENT off and on.  Scans are
synth.point_cloud(seed, 120000) (the size of a KITTI scan), batches of 1, 2 and 16 frames, every frame with its own matrix.  In ONE
process, every variant warmed up and then timed over --reps windows of >= --seconds each (HIP events around a window of calls on
tensors that are already on the device), the variants of a batch alternating and their order rotating from window to window:

      transform        = ops.scan_transform with out= given (out of place; in place is the same launch): nothing allocated
      transform_entry  = the mv3d_scan_transform entry itself, without the Python argument checks
      torch_transform  = the same rule with torch ops on the same tensors: points[lo:hi, :3] @ R.T * s + t in f32, frame by frame
                         (the frames' row ranges known on the host), the reflectance copied.  Its f32 products are not the kernel's
                         f64 chain: `torch_max_abs_difference` is the largest coordinate difference in metres

`roofline_fraction` is the 2 * 16 * P bytes the launch moves (every row read once and written once) at 8 TB/s over the measured time of
`transform_entry`.  A variant is "below" another when the gap of the medians exceeds the larger of the two spreads (max - min over
the windows).  `train_step` is the 3-view bf16 step of bench.py's network fed by the data layer itself -- get_minibatch on two in-memory
frames (scan of 120000 points, 375 x 1242 image) under cfg.LIDAR_BV_FROM_SCAN and cfg.FRONT_VIEW_INPUT, stack, forward, losses, backward,
Adam -- with the key off and on; the difference holds the host side (draw, annotation, table) as well as the launch.  Real KITTI scans
are not measured here, and nothing here says anything about accuracy.  Prints one JSON line; --out also writes it.

    python tools/scan_augment_bench.py [--batches 1,2,16] [--points 120000] [--seconds 1.0] [--reps 3] [--no-step] [--out profiles/scan_augment_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mv3d_tf_amd import build, ops, synth  # noqa: E402
from mv3d_tf_amd.datasets import augment  # noqa: E402

HBM_BYTES_PER_S = 8e12


def stats(v):
    return {"median_ms": round(1e3 * float(np.median(v)), 4), "min_ms": round(1e3 * min(v), 4), "max_ms": round(1e3 * max(v), 4)}


def below(a, b):
    """median(a) under median(b) by more than the larger spread of the two"""
    return bool(np.median(b) - np.median(a) > max(max(a) - min(a), max(b) - min(b)))


def event_window(fn, seconds):
    """seconds per call of fn() over one event-timed window of >= `seconds` (the count comes from a short pilot)"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def run(n):
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3

    n = max(20, int(np.ceil(1.1 * seconds / max(run(20) / 20, 1e-7))))
    while True:
        dt = run(n)
        if dt >= seconds:
            return dt / n
        n *= 2


def draws(B):
    rng = np.random.RandomState(7)
    return [(rng.uniform(-0.1745, 0.1745), rng.uniform(0.95, 1.05), rng.uniform(-1.0, 1.0, 3)) for _ in range(B)]


def device_calls(clouds):
    B = len(clouds)
    pts = torch.from_numpy(np.concatenate(clouds, 0)).cuda()
    P = int(pts.shape[0])
    off = torch.from_numpy(np.cumsum([0] + [len(c) for c in clouds]).astype(np.int32)).cuda()
    A = torch.from_numpy(np.stack([augment.transform_matrix(*d)[0] for d in draws(B)])).cuda()
    out, t_out = torch.empty((P, 4), device="cuda"), torch.empty((P, 4), device="cuda")
    entry, stream = ops.lib().mv3d_scan_transform, torch.cuda.current_stream().cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())
    # the yardstick's per-frame f32 R^T, s and t, and the frames' row ranges known on the host
    Rt = [torch.tensor([[np.cos(th), np.sin(th), 0.0], [-np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32, device="cuda")
          for th, _, _ in draws(B)]
    s32 = [float(s) for _, s, _ in draws(B)]
    t32 = [torch.tensor(t, dtype=torch.float32, device="cuda") for _, _, t in draws(B)]
    bounds = np.cumsum([0] + [len(c) for c in clouds]).tolist()

    def transform():
        return ops.scan_transform(pts, off, A, out=out)

    def transform_entry():
        ops.check(entry(p(pts), p(off), B, P, p(A), p(out), C.c_void_p(stream)), "mv3d_scan_transform")

    def torch_transform():
        for b in range(B):
            lo, hi = bounds[b], bounds[b + 1]
            t_out[lo:hi, :3] = pts[lo:hi, :3] @ Rt[b] * s32[b] + t32[b]
        t_out[:, 3] = pts[:, 3]

    calls = {"transform": transform, "transform_entry": transform_entry, "torch_transform": torch_transform}
    return calls, (pts, out, t_out)


def bench_batch(a, B):
    clouds = [synth.point_cloud(100 + b, a.points) for b in range(B)]
    calls, (pts, out, t_out) = device_calls(clouds)
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    diff = float((out[:, :3].double() - t_out[:, :3].double()).abs().max())
    P = int(pts.shape[0])
    t = {k: [] for k in calls}
    order = list(calls)
    for r in range(a.reps):
        for k in order[r % len(order):] + order[:r % len(order)]:
            t[k].append(event_window(calls[k], a.seconds))
    moved = 2 * 16 * P
    return {"batch": B, "points_per_frame": a.points, "rows": P, "torch_max_abs_difference": diff, "device": {k: stats(t[k]) for k in calls},
            "bytes_moved": moved, "roofline_ms_at_8TBps": round(1e3 * moved / HBM_BYTES_PER_S, 5),
            "roofline_fraction": round(moved / HBM_BYTES_PER_S / float(np.median(t["transform_entry"])), 4),
            "transform_below_torch_transform": below(t["transform"], t["torch_transform"]),
            "torch_transform_below_transform": below(t["torch_transform"], t["transform"])}


def bench_step(a):
    """the 3-view bf16 training step of bench.py's network, fed by get_minibatch from in-memory frames, with the key off / on"""
    from mv3d_tf_amd import sharding
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.fast_rcnn.train_mv import SolverWrapper, stack_blobs, total_loss
    from mv3d_tf_amd.networks import get_network
    from mv3d_tf_amd.optim import Adam
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    np.random.seed(cfg.RNG_SEED)
    augment.seed(cfg.RNG_SEED)
    net = get_network("MV3D_train_3view")
    net.amp_dtype, net.mfma_trunk, net.cast_many, net.fused_head = torch.bfloat16, True, True, True
    params = net.parameters()
    opt = Adam(params, lr=SolverWrapper.LEARNING_RATE)
    net.attach_optimizer(opt)
    bucketer = sharding.GradBucketer(params, None)
    rng = np.random.RandomState(100)
    roidb = []
    for k in range(2):
        _, _, _, calib, (gt_bv, gt_3d, gt_cnr) = synth.rpn_head(7000 + k, 76, 76, "peaky", return_gt=True)
        G = len(gt_bv)
        x1, y1 = rng.uniform(0, 1000, G), rng.uniform(0, 250, G)
        roidb.append({"image": rng.randint(0, 255, (375, 1242, 3)).astype(np.uint8), "velodyne": synth.point_cloud(200 + k, a.points),
                      "calib": np.asarray(calib, np.float64).reshape(4, 12), "flipped": False, "gt_classes": np.ones(G, np.int32),
                      "boxes": np.stack([x1, y1, x1 + 120, y1 + 80], 1).astype(np.float32), "boxes_bv": np.asarray(gt_bv, np.float32)[:, :4],
                      "boxes_3D": np.asarray(gt_3d, np.float32)[:, :6], "boxes_corners": np.asarray(gt_cnr, np.float32)[:, :24]})
    seen = {}

    def step(on):
        def run():
            cfg.TRAIN.SCAN_AUGMENT = on
            feed = stack_blobs([get_minibatch([e], 2) for e in roidb])
            feed["keep_prob"] = 0.5
            bucketer.zero_grad()
            layers = net.forward(feed)
            loss, _ = total_loss(layers)
            bucketer.reset()
            bucketer.dist_enabled = True
            loss.backward()
            bucketer.finish()
            opt.step()
            seen[on] = float(loss.detach())
        return run

    calls = {"step_off": step(False), "step_on": step(True)}
    saved = (cfg.TRAIN.SCAN_AUGMENT, cfg.LIDAR_BV_FROM_SCAN, cfg.FRONT_VIEW_INPUT)
    cfg.LIDAR_BV_FROM_SCAN = cfg.FRONT_VIEW_INPUT = True
    try:
        for _ in range(3):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        order = list(calls)
        for r in range(a.reps):
            for k in order[r % 2:] + order[:r % 2]:
                t[k].append(event_window(calls[k], a.seconds))
    finally:
        cfg.TRAIN.SCAN_AUGMENT, cfg.LIDAR_BV_FROM_SCAN, cfg.FRONT_VIEW_INPUT = saved
    bucketer.close()
    ms = lambda v: {"median_ms": round(1e3 * float(np.median(v)), 3), "min_ms": round(1e3 * min(v), 3), "max_ms": round(1e3 * max(v), 3)}
    return {"workload": "MV3D_train_3view, bf16 MFMA trunks, 2 frames a step through get_minibatch (scan of %d points -> 601x601x9 BEV + 64x512x3 "
                        "front view on the device, 375x1242 image from the host), %d objects a frame" % (a.points, len(roidb[0]["boxes"])),
            "step_off": ms(t["step_off"]), "step_on": ms(t["step_on"]), "losses_finite": bool(np.isfinite(list(seen.values())).all()),
            "step_on_below_step_off": below(t["step_on"], t["step_off"]), "step_off_below_step_on": below(t["step_off"], t["step_on"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,16")
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("scan_augment_bench: no GPU -- nothing here can be timed without one")
    out = {"bench": "scan_transform", "reps": a.reps, "window_s": a.seconds, "device_name": torch.cuda.get_device_name(0),
           "sizes": [bench_batch(a, int(B)) for B in a.batches.split(",") if B], "accuracy": "no claim: no KITTI data, no checkpoint"}
    if not a.no_step:
        out["train_step"] = bench_step(a)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
