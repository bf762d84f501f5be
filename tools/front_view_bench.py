"""Front-view rasteriser (ops.point_cloud_2_front, csrc/front_view_raster.hip) against the path a user had
before it: a vectorised numpy rasteriser of the same definition on the host plus the upload of the (B, 64, 512, 3) map.  Scans are
synth.point_cloud(seed, 120000) (the size of a KITTI scan), batches of 1, 2 and 16 frames.  In ONE process, every variant warmed
up and then timed over --reps windows of >= --seconds each, the variants of a batch alternating:

  device    = the three launches alone on points that are already on the device: HIP events around a window of calls (out= and
              workspace= given, nothing allocated).  The clouds stay where the upload left them -- a scan is rasterised right
              after it arrives, so nothing is rotated out of the caches.
  A         = the host way, from the frames' host arrays to a finished device tensor: numpy raster per frame, np.stack, upload
              (host clock, synchronised).
  B         = the device way, from the same host arrays to the same tensor: np.concatenate, upload, one batched call.
  piled     = (batch 1 only) the device time for a cloud of the same size whose points all fall on an 8 x 8 block of pixels
              (1875 atomics per key): what same-pixel contention costs at its worst.

The numpy rasteriser uses np.arctan2 where the device uses its table-driven arctangent, so a point within an ulp of a bin edge may
land one pixel over: the count of differing pixels is reported, not asserted to be zero.  Prints one JSON line; --out also writes it.

    python tools/front_view_bench.py [--batches 1,2,16] [--points 120000] [--seconds 1.0] [--reps 3] [--out profiles/front_view_bench.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mv3d_tf_amd import build, ops, synth  # noqa: E402

H, W = 64, 512
THETA_MAX, DTHETA = np.pi / 4, (np.pi / 2) / 512
PHI_TOP, DPHI = np.radians(2.0), np.radians(26.9) / 64


def numpy_front_view(pts):
    """(P,4) f32 -> (64,512,3) f32: nearest point per pixel, among equal distances the last (libm arctangent)"""
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    xy2 = x * x + y * y
    with np.errstate(invalid="ignore", over="ignore"):
        col = np.floor((THETA_MAX - np.arctan2(y, x)) / DTHETA)
        row = np.floor((PHI_TOP - np.arctan2(z, np.sqrt(xy2))) / DPHI)
        d = np.sqrt(z * z + xy2).astype(np.float32)
    keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~((x == 0) & (y == 0)) & (col >= 0) & (col < W) & (row >= 0) & (row < H)
    idx = np.flatnonzero(keep)
    pix = row[idx].astype(np.int64) * W + col[idx].astype(np.int64)
    order = np.lexsort((-idx, d[idx], pix))
    first = np.ones(order.size, bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    win = idx[order][first]
    fv = np.zeros((H * W, 3), np.float32)
    fv[pix[order][first]] = np.stack([pts[win, 2], d[win], pts[win, 3]], 1)
    return fv.reshape(H, W, 3)


def piled_cloud(P, seed=7):
    rng = np.random.RandomState(seed)
    theta = THETA_MAX - (300 + rng.randint(0, 8, P) + rng.uniform(0.25, 0.75, P)) * DTHETA
    phi = PHI_TOP - (20 + rng.randint(0, 8, P) + rng.uniform(0.25, 0.75, P)) * DPHI
    r = rng.uniform(5, 60, P)
    return np.stack([r * np.cos(phi) * np.cos(theta), r * np.cos(phi) * np.sin(theta), r * np.sin(phi), rng.random_sample(P)], 1).astype(np.float32)


def stats(v):
    return {"median_ms": round(1e3 * float(np.median(v)), 4), "min_ms": round(1e3 * min(v), 4), "max_ms": round(1e3 * max(v), 4)}


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


def host_window(fn, seconds):
    """seconds per call of fn() (which ends synchronised) over one host-clock window of >= `seconds`"""
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n


def device_call(clouds):
    """(a zero-argument launch of the batched call on device-resident copies of `clouds`, its output tensor)"""
    B = len(clouds)
    pts = torch.from_numpy(np.concatenate(clouds, 0)).cuda()
    off = torch.from_numpy(np.cumsum([0] + [len(c) for c in clouds]).astype(np.int32)).cuda()
    out = torch.empty((B, H, W, 3), device="cuda")
    ws = torch.empty(ops.point_cloud_2_front_workspace_bytes(B), dtype=torch.uint8, device="cuda")
    return (lambda: ops.point_cloud_2_front(pts, offsets=off, out=out, workspace=ws)), out


def bench_batch(a, B):
    clouds = [synth.point_cloud(100 + b, a.points) for b in range(B)]

    def host_way():
        t = torch.from_numpy(np.stack([numpy_front_view(c) for c in clouds])).cuda()
        torch.cuda.synchronize()
        return t

    def device_way():
        t = ops.point_cloud_2_front(np.concatenate(clouds, 0), offsets=np.cumsum([0] + [len(c) for c in clouds]))
        torch.cuda.synchronize()
        return t

    launch, out = device_call(clouds)
    ha, hb = host_way(), device_way()
    launch()
    torch.cuda.synchronize()
    assert torch.equal(hb.view(torch.int32), out.view(torch.int32)), "host-fed and device-fed calls differ"
    differing = int((ha.view(torch.int32) != hb.view(torch.int32)).any(-1).sum().item())
    td, ta, tb = [], [], []
    for _ in range(a.reps):
        td.append(event_window(launch, a.seconds))
        ta.append(host_window(host_way, a.seconds))
        tb.append(host_window(device_way, a.seconds))
    res = {"batch": B, "points_per_frame": a.points, "occupied_pixels_per_frame": round(float((hb[..., 1] != 0).sum().item()) / B, 1),
           "pixels_differing_from_numpy": differing, "device": stats(td), "A_numpy_raster_plus_upload": stats(ta),
           "B_upload_plus_device_raster": stats(tb), "B_below_A_by_more_than_A_spread": bool(np.median(ta) - np.median(tb) > max(ta) - min(ta))}
    if B == 1:
        piled = device_call([piled_cloud(a.points)])[0]
        piled()
        res["device_piled"] = stats([event_window(piled, a.seconds) for _ in range(a.reps)])
    return res


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
        raise SystemExit("front_view_bench: no GPU -- nothing here can be timed without one")
    out = {"bench": "point_cloud_2_front", "reps": a.reps, "window_s": a.seconds, "device_name": torch.cuda.get_device_name(0),
           "sizes": [bench_batch(a, int(B)) for B in a.batches.split(",") if B]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
