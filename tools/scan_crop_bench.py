"""Crop of Velodyne scans to the camera image (ops.scan_crop_to_image, csrc/scan_crop.hip): what the stage
costs alone, what it costs or saves in front of the two rasters that read its output, and a torch restatement of it as the yardstick.
Scans are synth.point_cloud(seed, 120000) (the size of a KITTI scan) under synth.KITTI_CALIB and a 375 x 1242 image, batches of 1, 2
and 16 frames.  In ONE process, every variant warmed up and then timed over --reps windows of >= --seconds each (HIP events around
a window of calls on tensors that are already on the device), the variants of a batch alternating and their order rotating from
window to window:

      crop          = ops.scan_crop_to_image with out=, offsets_out= and workspace= given: three launches, nothing allocated
      crop_entry    = the mv3d_scan_crop_to_image entry itself, without the Python argument checks
      torch_crop    = the same rule with torch ops on the same tensors: the frame of a row by bucketize, the f64 projection by the
                      frames' matrices, a boolean mask, points[mask] (which reads the count back: boolean indexing synchronises) and a
                      per-frame count by index_add_.  Its f64 products are not fused, so a row within an ulp of the image border may
                      fall on the other side: `torch_rows_differing` counts them
      rasters       = ops.scan_bev + ops.point_cloud_2_front on the uncropped batch (what the feeds run with the key off)
      crop_rasters  = crop, then the same two rasters on the cropped batch (what the feeds run with the key on)

`rasters` and `crop_rasters` trade their two pairs of output maps from window to window.  `kept_share` is the share of the synthetic
scans' rows the crop keeps; real KITTI scans are not measured here.  `roofline_fraction` is (2 * 16 * P + 16 * K) bytes at 8 TB/s
over the measured time of `crop_entry`: P rows read by the flags and (at most) by the copy launch, K kept rows written.  A variant is "below" another when the gap of the medians exceeds the
larger of the two spreads (max - min over the windows).  Prints one JSON line; --out also writes it.

    python tools/scan_crop_bench.py [--batches 1,2,16] [--points 120000] [--seconds 1.0] [--reps 3] [--out profiles/scan_crop_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mv3d_tf_amd import build, ops, synth  # noqa: E402

IMAGE_HW = (375, 1242)
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


def host_matrices(calibs):
    """(B,3,4) f64: the f32 (P2 . R0) . Tr of every table, each product rounded to f32 as numpy rounds it (the yardstick's matrices; the
    kernel's own are fused, csrc/geometry.h)"""
    out = []
    for c in calibs:
        c = np.asarray(c, np.float32).reshape(48)
        P2, R0, Tr = c[0:12].reshape(3, 4), np.vstack([c[24:33].reshape(3, 3), np.zeros((1, 3), np.float32)]), c[36:48].reshape(3, 4)
        out.append(((P2 @ R0) @ Tr).astype(np.float64))
    return np.stack(out)


def device_calls(clouds):
    B = len(clouds)
    pts = torch.from_numpy(np.concatenate(clouds, 0)).cuda()
    P = int(pts.shape[0])
    off = torch.from_numpy(np.cumsum([0] + [len(c) for c in clouds]).astype(np.int32)).cuda()
    cal = torch.from_numpy(np.stack([synth.KITTI_CALIB] * B).reshape(B, 48)).cuda()
    hw = torch.tensor([IMAGE_HW] * B, dtype=torch.int32, device="cuda")
    out, off_out = torch.empty((P, 4), device="cuda"), torch.empty(B + 1, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.scan_crop_workspace_bytes(P), dtype=torch.uint8, device="cuda")
    fv_ws = torch.empty(ops.point_cloud_2_front_workspace_bytes(B), dtype=torch.uint8, device="cuda")
    maps = [(torch.empty((B,) + ops.BEV_SHAPE, device="cuda"), torch.empty((B,) + ops.FV_SHAPE, device="cuda")) for _ in range(2)]
    turn = [0]
    maps_of = lambda i: maps[(i + turn[0]) % 2]
    entry, stream = ops.lib().mv3d_scan_crop_to_image, torch.cuda.current_stream().cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())
    M = torch.from_numpy(host_matrices([synth.KITTI_CALIB] * B)).cuda()
    ones = torch.ones((P, 1), dtype=torch.float64, device="cuda")
    rows = torch.arange(P, device="cuda", dtype=torch.int32)
    held = {}

    def crop():
        return ops.scan_crop_to_image(pts, off, cal, hw, out=out, offsets_out=off_out, workspace=ws)

    def crop_entry():
        ops.check(entry(p(pts), p(off), B, P, p(cal), p(hw), p(out), p(off_out), p(ws), ws.numel(), C.c_void_p(stream)), "mv3d_scan_crop_to_image")

    def torch_crop():
        frame = torch.bucketize(rows, off[1:], right=True).clamp_(max=B - 1).long()
        v = torch.einsum("pij,pj->pi", M[frame], torch.cat([pts[:, :3].double(), ones], 1))
        u, w = v[:, 0] / v[:, 2], v[:, 1] / v[:, 2]
        keep = torch.isfinite(pts[:, :3]).all(1) & (v[:, 2] > 0) & (u >= 0) & (u < hw[frame, 1]) & (w >= 0) & (w < hw[frame, 0])
        counts = torch.zeros(B + 1, dtype=torch.int32, device="cuda").index_add_(0, frame + 1, keep.int())
        held["torch"] = (pts[keep], torch.cumsum(counts, 0).int())

    def rasters(i):
        bev, fv = maps_of(i)
        return lambda: (ops.point_cloud_2_top_batch(pts, off, out=bev), ops.point_cloud_2_front(pts, off, out=fv, workspace=fv_ws))

    def crop_rasters(i):
        def run():
            bev, fv = maps_of(i)
            c, o = crop()
            ops.point_cloud_2_top_batch(c, o, out=bev)
            ops.point_cloud_2_front(c, o, out=fv, workspace=fv_ws)
        return run

    calls = {"crop": crop, "crop_entry": crop_entry, "torch_crop": torch_crop, "rasters": lambda: rasters(0)(), "crop_rasters": crop_rasters(1)}
    return calls, turn, (pts, off, out, off_out, held)


def bench_batch(a, B):
    clouds = [synth.point_cloud(100 + b, a.points) for b in range(B)]
    calls, turn, (pts, off, out, off_out, held) = device_calls(clouds)
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    K = int(off_out[B])
    t_pts, t_off = held["torch"]
    differing = abs(int(t_pts.shape[0]) - K) if t_pts.shape[0] != K else int((t_pts.view(torch.int32) != out[:K].view(torch.int32)).any(1).sum())
    P = int(pts.shape[0])
    t = {k: [] for k in calls}
    order = list(calls)
    for r in range(a.reps):
        turn[0] = r
        for k in order[r % len(order):] + order[:r % len(order)]:
            t[k].append(event_window(calls[k], a.seconds))
    moved = 2 * 16 * P + 16 * K
    return {"batch": B, "points_per_frame": a.points, "rows": P, "kept_rows": K, "kept_share": round(K / max(P, 1), 4),
            "torch_rows_differing": differing, "device": {k: stats(t[k]) for k in calls},
            "bytes_moved": moved, "roofline_ms_at_8TBps": round(1e3 * moved / HBM_BYTES_PER_S, 5),
            "roofline_fraction": round(moved / HBM_BYTES_PER_S / float(np.median(t["crop_entry"])), 4),
            "crop_below_torch_crop": below(t["crop"], t["torch_crop"]), "torch_crop_below_crop": below(t["torch_crop"], t["crop"]),
            "crop_rasters_below_rasters": below(t["crop_rasters"], t["rasters"]), "rasters_below_crop_rasters": below(t["rasters"], t["crop_rasters"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,16")
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("scan_crop_bench: no GPU -- nothing here can be timed without one")
    out = {"bench": "scan_crop_to_image", "reps": a.reps, "window_s": a.seconds, "device_name": torch.cuda.get_device_name(0),
           "image_hw": list(IMAGE_HW), "sizes": [bench_batch(a, int(B)) for B in a.batches.split(",") if B]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
