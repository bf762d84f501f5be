"""The paper's empty-anchor removal (ops.anchor_occupancy, mv3d_proposal_3d_masked): what the mask costs and what it saves the proposal
layer, on the 601 x 601 x 9 maps of the two synthetic scans (synth.point_cloud, P = 20000 and P = 2000 points) for B = 1, 2, 16 frames.
In ONE process, every variant warmed up and then timed over --reps event windows of >= --seconds each, the variants alternating:

  occupancy_hbm       ops.anchor_occupancy, the launches rotating over enough copies of the batch (>= --footprint-mb in all) that none is
                      still in the 256 MiB Infinity Cache when its turn comes again; bytes/s = B * Hm * Wm * C * 4 (the one read of the
                      map) over the time per call, also as a fraction of the 8 TB/s HBM peak DESIGN.md uses.  The call is two launches
                      (row prefixes, anchors); the second one's traffic (the prefix table, ~0.7 MB per frame, L2) is not counted.
  occupancy_hbm_graph the same rotating launches, 24 calls captured once as a hipGraph and replayed: the device's time per call without
                      the Python wrapper's (at batch 1 and 2 the eager figure is how fast the host can issue the call).
  occupancy_resident  the same call on ONE buffer (the map still in the caches, as right behind the first convolution of a step).
  torch               the same mask through torch: (bev != 0).any(-1), two cumsums, a padded table and four gathers at precomputed
                      corner indices -- asserted equal to the kernel's mask before anything is timed.
  proposal            mv3d_proposal_3d against mv3d_proposal_3d_masked with those masks, 76 x 76 peaky heads, TRAIN cfg (12000 -> 2000)
                      and the end2end yml's TEST cfg (6000 -> 300), with the empty share and the proposals each returns.

The synthetic scan is close to uniform over the map: its empty shares say nothing about real KITTI frames (unmeasured: no KITTI data
here).  Prints one JSON line; --out also writes it to a file.

    python tools/empty_anchors_bench.py [--batches 1,2,16] [--seconds 0.5] [--reps 3] [--out profiles/empty_anchors_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mv3d_tf_amd import build, ops, synth  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, the figure DESIGN.md measures against
GRID = 76
GRAPH_CALLS = 24
SECTIONS = {"TRAIN": dict(RPN_PRE_NMS_TOP_N=12000, RPN_POST_NMS_TOP_N=2000, RPN_NMS_THRESH=0.7, RPN_MIN_SIZE=5),
            "TEST": dict(RPN_PRE_NMS_TOP_N=6000, RPN_POST_NMS_TOP_N=300, RPN_NMS_THRESH=0.7, RPN_MIN_SIZE=5)}
BASE = np.array([[-19, -8, 20, 8], [-5, -2, 5, 3], [-8, -19, 8, 20], [-2, -5, 3, 5]], np.int64)     # lib/rpn_msr/generate_anchors.py:37-51


def stats(v):
    return {"median_us": round(1e6 * float(np.median(v)), 2), "min_us": round(1e6 * min(v), 2), "max_us": round(1e6 * max(v), 2)}


def event_window(fn, seconds):
    """seconds per call of fn(i) over one event-timed window of >= `seconds` (the count comes from a short pilot)"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def run(n):
        ev[0].record()
        for i in range(n):
            fn(i)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3

    pilot = 20
    n = max(pilot, int(np.ceil(1.1 * seconds / max(run(pilot) / pilot, 1e-7))))
    while True:
        dt = run(n)
        if dt >= seconds:
            return dt / n
        n *= 2


def torch_mask_fn(Hm, Wm, H, W, stride, min_cells, dev):
    """the mask through torch ops; the clipped corner indices are made once, outside the timed region"""
    sx, sy = np.meshgrid(np.arange(W) * stride, np.arange(H) * stride)
    a = (BASE[None] + np.stack([sx.ravel(), sy.ravel(), sx.ravel(), sy.ravel()], 1)[:, None, :]).reshape(-1, 4)
    x1, y1 = np.maximum(a[:, 0], 0), np.maximum(a[:, 1], 0)
    x2, y2 = np.minimum(a[:, 2], Wm - 1), np.minimum(a[:, 3], Hm - 1)
    empty = (x1 > x2) | (y1 > y2)
    x1, y1, x2, y2 = (np.where(empty, 0, v) for v in (x1, y1, x2, y2))
    t = lambda v: torch.as_tensor(v, dtype=torch.int64, device=dev)
    i11, i01, i10, i00 = t((y2 + 1) * (Wm + 1) + x2 + 1), t(y1 * (Wm + 1) + x2 + 1), t((y2 + 1) * (Wm + 1) + x1), t(y1 * (Wm + 1) + x1)
    keep = torch.as_tensor(~empty, device=dev)

    def fn(bev):
        occ = (bev != 0).any(-1)
        ii = F.pad(occ.to(torch.int32).cumsum(1, dtype=torch.int32).cumsum(2, dtype=torch.int32), (1, 0, 1, 0)).reshape(bev.shape[0], -1)
        cnt = ii[:, i11] - ii[:, i01] - ii[:, i10] + ii[:, i00]
        return ((cnt >= min_cells) & keep).to(torch.uint8)
    return fn


def scan_maps(P, B, dev):
    return torch.stack([ops.point_cloud_2_top(torch.as_tensor(synth.point_cloud(1 + b, P)).to(dev)) for b in range(B)])


def bench_occupancy(a, P, B, dev):
    bev = scan_maps(P, B, dev)
    nbytes = bev.numel() * 4
    copies = max(2, int(np.ceil(a.footprint_mb * 2 ** 20 / nbytes)))
    tmask = torch_mask_fn(601, 601, GRID, GRID, 8, 1, dev)
    mask = ops.anchor_occupancy(bev, GRID, GRID)
    assert torch.equal(mask, tmask(bev)), "kernel and torch masks differ"
    src = [bev] + [bev.clone() for _ in range(copies - 1)]
    out = (torch.empty_like(mask), None)
    hbm = lambda i: ops.anchor_occupancy(src[i % copies], GRID, GRID, out=out)
    resident = lambda i: ops.anchor_occupancy(bev, GRID, GRID, out=out)
    base = lambda i: tmask(src[i % copies])
    for i in range(copies):
        hbm(i)
    for i in range(3):
        resident(i), base(i)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                               # (the stream's workspace exists before the capture)
        hbm(0)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for i in range(GRAPH_CALLS):
            hbm(i)
    replay = lambda i: graph.replay()
    replay(0)
    torch.cuda.synchronize()
    assert torch.equal(out[0], mask), "the captured calls give another mask"
    th, tg, tr, tt = [], [], [], []
    for _ in range(a.reps):
        th.append(event_window(hbm, a.seconds))
        tg.append(event_window(replay, a.seconds) / GRAPH_CALLS)
        tr.append(event_window(resident, a.seconds))
        tt.append(event_window(base, a.seconds))
    rate = nbytes / float(np.median(th))
    grate = nbytes / float(np.median(tg))
    res = {"points": P, "batch": B, "map_bytes": nbytes, "rotating_copies": copies, "empty_share": round(1.0 - float(mask.float().mean()), 4),
           "occupancy_hbm": dict(stats(th), TB_per_s=round(rate / 1e12, 3), fraction_of_8TBps=round(rate / HBM_PEAK, 3)),
           "occupancy_hbm_graph": dict(stats(tg), TB_per_s=round(grate / 1e12, 3), fraction_of_8TBps=round(grate / HBM_PEAK, 3)),
           "occupancy_resident": stats(tr), "torch": stats(tt),
           "torch_over_kernel": round(float(np.median(tt)) / float(np.median(th)), 1)}
    del src
    torch.cuda.empty_cache()
    return res, mask


def bench_proposal(a, B, masks, dev):
    frames = [synth.rpn_head(700 + b, GRID, GRID, "peaky") for b in range(B)]
    t = lambda arrs: torch.as_tensor(np.ascontiguousarray(arrs, np.float32)).to(dev)
    prob, pred = t(np.concatenate([f[0] for f in frames])), t(np.concatenate([f[1] for f in frames]))
    info, cal = t(np.concatenate([f[2] for f in frames])), t(np.stack([f[3] for f in frames]))
    res = []
    for key, sec in SECTIONS.items():
        params = ops.proposal_params(sec)
        keep = ops.proposal_3d(prob, pred, info, cal, params)                     # (one set of outputs, reused)
        plain = lambda i: ops.proposal_3d(prob, pred, info, cal, params, out=keep)
        n_plain = [int(v) for v in plain(0)[3].cpu()]
        for P, mask in masks.items():
            masked = lambda i: ops.proposal_3d(prob, pred, info, cal, params, out=keep, anchor_mask=mask)
            n_masked = [int(v) for v in masked(0)[3].cpu()]
            for i in range(3):
                plain(i), masked(i)
            tp, tm = [], []
            for _ in range(a.reps):
                tp.append(event_window(plain, a.seconds))
                tm.append(event_window(masked, a.seconds))
            res.append({"cfg": key, "batch": B, "points": P, "empty_share": round(1.0 - float(mask.float().mean()), 4),
                        "proposal_3d": stats(tp), "proposal_3d_masked": stats(tm),
                        "masked_over_plain": round(float(np.median(tm)) / float(np.median(tp)), 3),
                        "proposals_plain": n_plain, "proposals_masked": n_masked})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,16")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--footprint-mb", type=float, default=1024.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("empty_anchors_bench: no GPU -- nothing here can be timed without one")
    dev = torch.device("cuda")
    occ, prop = [], []
    for B in (int(b) for b in a.batches.split(",") if b):
        masks = {}
        for P in (20000, 2000):
            r, masks[P] = bench_occupancy(a, P, B, dev)
            occ.append(r)
        prop += bench_proposal(a, B, masks, dev)
    out = {"bench": "empty_anchors", "reps": a.reps, "window_s": a.seconds, "footprint_mb": a.footprint_mb,
           "device": torch.cuda.get_device_name(0), "map": [601, 601, 9], "grid": [GRID, GRID],
           "bytes_counted": "B * 601 * 601 * 9 * 4 (the one read of the map)",
           "note": "synthetic, near-uniform scans: the empty shares say nothing about real KITTI frames (unmeasured)",
           "occupancy": occ, "proposal": prop}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
