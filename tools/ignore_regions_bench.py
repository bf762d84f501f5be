"""Ignore regions in training (ops.ignore_relabel, csrc/ignore_regions.hip): what the one launch costs at the
training shapes, a torch restatement of the same rule as the yardstick, and the 3-view bf16 training step with cfg.TRAIN.IGNORE_TYPES on
against off.  Shapes: B = 2 and 16 frames, H = W = 76 (23,104 anchors a frame), 128 labelled anchors and 128 ROIs a frame,
4 and 64 ignore boxes per frame and list.  In ONE process, every variant warmed up and then timed over --reps windows of >= --seconds
each (HIP events around a window of calls on tensors that are already on the device), the variants alternating and their order rotating
from window to window:

      relabel        = ops.ignore_relabel with packed device lists and out= given: one launch, nothing allocated
      relabel_entry  = the mv3d_ignore_relabel entry itself, without the Python argument checks
      torch_relabel  = the same rule with torch ops on the same tensors: the labelled candidates by nonzero (which reads their count
                       back), the anchors' 3D priors and their eight projected corners in f64, IoA against the frames' padded lists,
                       index_put of -1.  Its f32 matrix product is not fused like the kernel's, so an image box may differ by a pixel:
                       `torch_labels_differing` counts the labels that came out differently
      step_off / step_on = MV3D_train_3view, bf16 MFMA trunks, 2 frames a step (bench.py's training workload): forward, four losses,
                       backward, Adam -- with the key off and on (4 ignore boxes per frame and list), alternating window by window

A variant is "below" another when the gap of the medians exceeds the larger of the two spreads (max - min over the windows).  The
launch is expected to be bound by launch latency and two dependent passes, not by bandwidth; no figure is fixed in advance.  The share
of real KITTI anchors and ROIs the rule relabels is not measured here: there is no KITTI data.  Prints one JSON line; --out writes it.

    python tools/ignore_regions_bench.py [--batches 2,16] [--boxes 4,64] [--seconds 1.0] [--reps 3] [--no-step] [--out profiles/ignore_regions_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mv3d_tf_amd import build, ops, synth  # noqa: E402

H = W = 76
STRIDE = 8
BASE = np.array([[-19, -8, 20, 8], [-5, -2, 5, 3], [-8, -19, 8, 20], [-2, -5, 3, 5]], np.float64)


def stats(v):
    return {"median_us": round(1e6 * float(np.median(v)), 3), "min_us": round(1e6 * min(v), 3), "max_us": round(1e6 * max(v), 3)}


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


def inputs(seed, B, K, labelled=128, rois=128):
    r = np.random.RandomState(seed)
    N = 4 * H * W
    rpn = np.full((B, N), -1, np.float32)
    for b in range(B):
        at = r.choice(N, labelled, replace=False)
        rpn[b, at] = (r.random_sample(labelled) < 0.25).astype(np.float32)

    def boxes(n, span, size):
        x1, y1 = r.uniform(0, span, n), r.uniform(0, span, n)
        return np.stack([x1, y1, x1 + r.uniform(10, size, n), y1 + r.uniform(10, size, n)], 1).astype(np.float32)

    S = B * rois
    frame = np.repeat(np.arange(B), rois).astype(np.float32)
    rois_bv = np.hstack([frame[:, None], np.round(boxes(S, 560, 60))]).astype(np.float32)
    rois_img = np.hstack([frame[:, None], np.round(boxes(S, 1100, 200))]).astype(np.float32)
    roi = (r.random_sample((S, 1)) < 0.25).astype(np.int32)
    ign_bv = [boxes(K, 560, 120) for _ in range(B)]
    ign_img = [boxes(K, 1100, 300) for _ in range(B)]
    return rpn, roi, rois_bv, rois_img, np.stack([synth.KITTI_CALIB] * B).astype(np.float32), ign_bv, ign_img


def torch_rule(dev, B, K):
    """the rule with torch ops; the frames' lists as dense (B, K, 4) f64 (every frame has K boxes here)"""
    n = torch.arange(4 * H * W, device=dev)
    cell = n // 4
    shift = torch.stack([cell % W, cell // W, cell % W, cell // W], 1).double() * STRIDE
    anchors = torch.as_tensor(BASE, device=dev)[n % 4] + shift                         # (N, 4) f64, integral
    sign = torch.tensor([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]],
                        dtype=torch.float32, device=dev)
    z, hgt = np.float32(-(1.73 - 1.56 / 2.0)), np.float32(1.56)

    def ioa_any(c, q, T):
        """c (n, 4), q (n, K, 4) f64 -> (n) bool"""
        area = (c[:, 2] - c[:, 0] + 1) * (c[:, 3] - c[:, 1] + 1)
        iw = torch.minimum(c[:, None, 2], q[:, :, 2]) - torch.maximum(c[:, None, 0], q[:, :, 0]) + 1
        ih = torch.minimum(c[:, None, 3], q[:, :, 3]) - torch.maximum(c[:, None, 1], q[:, :, 1]) + 1
        hit = (iw > 0) & (ih > 0) & (area[:, None] > 0) & (iw * ih / area[:, None] >= T)
        return hit.any(1)

    def fn(rpn, roi, rois_bv, rois_img, calib, q_bv, q_img, T, out_rpn, out_roi):
        out_rpn.copy_(rpn)
        out_roi.copy_(roi)
        fb, at = (rpn == 0).nonzero(as_tuple=True)
        c = anchors[at]
        P2, R0, Tr = calib[:, 0].reshape(B, 3, 4), calib[:, 2, :9].reshape(B, 3, 3), calib[:, 3].reshape(B, 3, 4)
        M = (torch.bmm(torch.bmm(P2[:, :, :3], R0), Tr)).double()[fb]                  # (n, 3, 4); the w = 0 column takes no part
        cx, cy = (c[:, 0] + c[:, 2]) / 2.0, (c[:, 1] + c[:, 3]) / 2.0
        ctr = torch.stack([600 * 0.1 - (cy + 0.5) * 0.1, 600 * 0.1 - (cx + 0.5) * 0.1 - 30.0, torch.full_like(cx, float(z))], 1).float()
        half = torch.stack([(c[:, 3] - c[:, 1]) * 0.1, (c[:, 2] - c[:, 0]) * 0.1, torch.full_like(cx, float(hgt))], 1).float() / 2.0
        corners = (ctr[:, None, :] + sign[None] * half[:, None, :]).double()          # (n, 8, 3)
        v = torch.einsum("nij,nkj->nki", M[:, :, :3], corners)
        px, py = v[:, :, 0] / v[:, :, 2], v[:, :, 1] / v[:, :, 2]
        img = torch.stack([px.min(1).values, py.min(1).values, px.max(1).values, py.max(1).values], 1).trunc()
        hit = ioa_any(c, q_bv[fb], T) | ioa_any(img, q_img[fb], T)
        out_rpn.index_put_((fb[hit], at[hit]), torch.tensor(-1.0, device=dev))
        rows = (roi.view(-1) == 0).nonzero(as_tuple=True)[0]
        fr = rois_bv[rows, 0].long()
        rhit = ioa_any(rois_bv[rows, 1:].double(), q_bv[fr], T) | ioa_any(rois_img[rows, 1:].double(), q_img[fr], T)
        out_roi.view(-1).index_put_((rows[rhit],), torch.tensor(-1, dtype=torch.int32, device=dev))

    return fn


def bench_launch(a, B, K):
    dev = torch.device("cuda")
    rpn, roi, rois_bv, rois_img, calib, ign_bv, ign_img = inputs(1000 + B + K, B, K)
    t_ = lambda x: torch.as_tensor(x).to(dev)
    rpn, roi, rois_bv, rois_img, calib = (t_(x) for x in (rpn, roi, rois_bv, rois_img, calib))
    (rb, ob), (ri, oi) = (tuple(t_(x) for x in ops.pack_box_lists(f)) for f in (ign_bv, ign_img))
    T = 0.5
    out = ops.ignore_relabel(rpn, roi, rois_bv, rois_img, calib, H, W, (rb, ob), (ri, oi), T, want_counts=True)
    t_out = (torch.empty_like(rpn), torch.empty_like(roi))
    rule = torch_rule(dev, B, K)
    q_bv, q_img = rb.view(B, K, 4).double(), ri.view(B, K, 4).double()
    entry, stream = ops.lib().mv3d_ignore_relabel, torch.cuda.current_stream().cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())
    S = int(roi.numel())

    def relabel():
        ops.ignore_relabel(rpn, roi, rois_bv, rois_img, calib, H, W, (rb, ob), (ri, oi), T, want_counts=True, out=out)

    def relabel_entry():
        ops.check(entry(p(rpn), p(roi), p(rois_bv), p(rois_img), S, p(calib), B, H, W, STRIDE, p(rb), p(ob), B * K, p(ri), p(oi), B * K,
                        C.c_double(T), p(out[0]), p(out[1]), p(out[2]), p(out[3]), C.c_void_p(stream)), "mv3d_ignore_relabel")

    def torch_relabel():
        rule(rpn, roi, rois_bv, rois_img, calib, q_bv, q_img, T, *t_out)

    calls = {"relabel": relabel, "relabel_entry": relabel_entry, "torch_relabel": torch_relabel}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    differing = int((out[0] != t_out[0]).sum() + (out[1] != t_out[1]).sum())
    counts = out[2].cpu().numpy()
    t = {k: [] for k in calls}
    order = list(calls)
    for r in range(a.reps):
        for k in order[r % len(order):] + order[:r % len(order)]:
            t[k].append(event_window(calls[k], a.seconds))
    return {"batch": B, "boxes_per_frame_and_list": K, "labelled_anchors_per_frame": 128, "rois_per_frame": 128,
            "background_anchors": int((rpn == 0).sum()), "background_rois": int((roi == 0).sum()),
            "relabelled_anchors": int(counts[:, 0].sum()), "relabelled_rois": int(counts[:, 1].sum()), "torch_labels_differing": differing,
            "device": {k: stats(t[k]) for k in calls},
            "relabel_below_torch_relabel": below(t["relabel"], t["torch_relabel"]), "torch_relabel_below_relabel": below(t["torch_relabel"], t["relabel"])}


def bench_step(a):
    """the 3-view bf16 training step of bench.py (fast_rcnn.train_mv.bench_train_step's network, frames and step) with the key off / on"""
    from mv3d_tf_amd import sharding
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.fast_rcnn.train_mv import SolverWrapper, stack_blobs, total_loss
    from mv3d_tf_amd.networks import get_network
    from mv3d_tf_amd.optim import Adam
    np.random.seed(cfg.RNG_SEED)
    net = get_network("MV3D_train_3view")
    net.amp_dtype, net.mfma_trunk, net.cast_many, net.fused_head = torch.bfloat16, True, True, True
    params = net.parameters()
    opt = Adam(params, lr=SolverWrapper.LEARNING_RATE)
    net.attach_optimizer(opt)
    bucketer = sharding.GradBucketer(params, None)
    rng = np.random.RandomState(100)
    frames = []
    for k in range(2):
        _, _, info, calib, (gt_bv, gt_3d, gt_cnr) = synth.rpn_head(7000 + k, 76, 76, "peaky", return_gt=True)
        bev = (rng.random_sample((1, 608, 608, 9)) < 0.03).astype(np.float32) * rng.uniform(0, 2.4, (1, 608, 608, 9)).astype(np.float32)
        img = rng.randint(0, 255, (1, 375, 1242, 3)).astype(np.float32) - cfg.PIXEL_MEANS.astype(np.float32)
        x1, y1 = rng.uniform(0, 500, 4), rng.uniform(0, 500, 4)
        ign_bv = np.stack([x1, y1, x1 + rng.uniform(20, 120, 4), y1 + rng.uniform(20, 120, 4)], 1).astype(np.float32)
        ign_img = np.stack([x1 * 2, y1 / 2, x1 * 2 + 150, y1 / 2 + 80], 1).astype(np.float32)
        frames.append({"lidar_bv_data": bev, "image_data": img.astype(np.float32), "lidar_fv_data": rng.uniform(0, 1, (1, 64, 512, 3)).astype(np.float32),
                       "im_info": info, "calib": calib, "gt_boxes_bv": gt_bv, "gt_boxes_3d": gt_3d, "gt_boxes_corners": gt_cnr,
                       "ignore_boxes_bv": ign_bv, "ignore_boxes_img": ign_img})
    feed = stack_blobs(frames)
    for k in ("lidar_bv_data", "image_data", "lidar_fv_data"):
        feed[k] = torch.as_tensor(feed[k]).cuda()
    feed["keep_prob"] = 0.5
    seen = {}

    def step(types):
        def run():
            cfg.TRAIN.IGNORE_TYPES = types
            bucketer.zero_grad()
            layers = net.forward(feed)
            loss, _ = total_loss(layers)
            bucketer.reset()
            bucketer.dist_enabled = True
            loss.backward()
            bucketer.finish()
            opt.step()
            seen[bool(types)] = layers.get("ignored")
        return run

    calls = {"step_off": step(()), "step_on": step(("Van", "DontCare"))}
    saved = cfg.TRAIN.IGNORE_TYPES
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
        cfg.TRAIN.IGNORE_TYPES = saved
    bucketer.close()
    ms = lambda v: {"median_ms": round(1e3 * float(np.median(v)), 3), "min_ms": round(1e3 * min(v), 3), "max_ms": round(1e3 * max(v), 3)}
    return {"workload": "MV3D_train_3view, bf16 MFMA trunks, 2 frames a step, 4 ignore boxes per frame and list", "step_off": ms(t["step_off"]),
            "step_on": ms(t["step_on"]), "relabelled_last_step": seen[True].cpu().numpy().tolist(), "key_off_has_no_counts": seen[False] is None,
            "step_on_below_step_off": below(t["step_on"], t["step_off"]), "step_off_below_step_on": below(t["step_off"], t["step_on"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,16")
    ap.add_argument("--boxes", default="4,64")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("ignore_regions_bench: no GPU -- nothing here can be timed without one")
    out = {"bench": "ignore_relabel", "reps": a.reps, "window_s": a.seconds, "device_name": torch.cuda.get_device_name(0), "grid": [H, W],
           "launch": [bench_launch(a, int(B), int(K)) for B in a.batches.split(",") if B for K in a.boxes.split(",") if K],
           "kitti_share_relabelled": "not measured: no KITTI data"}
    if not a.no_step:
        out["train_step"] = bench_step(a)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
