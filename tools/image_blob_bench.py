"""Image blob on the device (ops.image_blob, csrc/image_blob.hip) against the host expression the loops use
with cfg.IMAGE_BLOB_ON_DEVICE off.  Frames are seeded random uint8 images of KITTI's sizes: batches of 1, 2 and 16 frames of
375 x 1242, and one mixed batch of 16 with the four KITTI sizes on the (376, 1242) canvas.  In ONE process, every variant warmed up
and then timed over --reps windows of >= --seconds each, the variants of a size alternating and their order rotating from window to
window:

  (a) device time, HIP events around a window of calls on pixels and a table that are already on the device, into a given buffer
      (nothing allocated):
      call    = ops.image_blob, the call the loops make
      entry   = the mv3d_image_blob entry itself, without the Python argument checks
      The two trade their output buffers from window to window.  `hbm_roofline_share` is the least time the memory system could take
      -- bytes from the shapes, sum of 3 h w read plus 12 B H W written, over 8 TB/s -- over the median time of `entry`.  That time is
      a call's share of a window of back-to-back calls, launch included; it is not a kernel time from a trace.
  (b) from the frames on the host to the finished device blob (host clock, synchronised):
      device_route = pack_image_frames, ONE uint8 upload, ONE ops.image_blob call (what detect_batch.image_feed does)
      host_route   = np.stack of (np.asarray(im, np.float64) - cfg.PIXEL_MEANS).astype(np.float32) per frame, one f32 upload.
                     The mixed batch has no host route (its frames do not stack): it is timed against the host expression padded by
                     the reference's im_list_to_blob rule, which no loop here runs -- named `host_route_padded`.

Both routes are checked to give the same bits before anything is timed.  A variant is "below" another when the gap of the medians
exceeds the larger of the two spreads (max - min over the windows).  Prints one JSON line; --out also writes it.

    python tools/image_blob_bench.py [--seconds 1.0] [--reps 3] [--out profiles/image_blob_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mv3d_tf_amd import build, ops  # noqa: E402
from mv3d_tf_amd.fast_rcnn.config import cfg  # noqa: E402

KITTI_SHAPES = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]
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


def host_window(fn, seconds):
    """seconds per call of fn() (which ends synchronised) over one host-clock window of >= `seconds`"""
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n


def bench_size(a, name, shapes, canvas):
    rng = np.random.RandomState(len(shapes))
    ims = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    B, (Hc, Wc) = len(ims), canvas
    equal = all(s == shapes[0] for s in shapes) and tuple(shapes[0]) == tuple(canvas)
    px, tab, _ = ops.pack_image_frames(ims)
    d_px, d_tab = torch.from_numpy(px).cuda(), torch.from_numpy(tab).cuda()
    pool, turn = [torch.empty((B, Hc, Wc, 3), device="cuda") for _ in range(2)], [0]
    out_of = lambda i: pool[(i + turn[0]) % 2]
    means = (C.c_double * 3)(*np.asarray(cfg.PIXEL_MEANS, np.float64).reshape(-1))
    entry, stream = ops.lib().mv3d_image_blob, torch.cuda.current_stream().cuda_stream
    calls = {"call": lambda: ops.image_blob(d_px, d_tab, canvas=canvas, out=out_of(0)),
             "entry": lambda: ops.check(entry(C.c_void_p(d_px.data_ptr()), len(px), C.c_void_p(d_tab.data_ptr()), B, means, Hc, Wc,
                                              C.c_void_p(out_of(1).data_ptr()), C.c_void_p(stream)), "mv3d_image_blob")}

    def device_route():
        t = ops.image_blob(ims, canvas=canvas)
        torch.cuda.synchronize()
        return t

    def host_route():
        frames = [(np.asarray(im, np.float64) - cfg.PIXEL_MEANS).astype(np.float32) for im in ims]
        if equal:
            blob = np.stack(frames)
        else:                                                            # im_list_to_blob's rule (no loop here runs it on the host)
            blob = np.zeros((B, Hc, Wc, 3), np.float32)
            for b, f in enumerate(frames):
                blob[b, :f.shape[0], :f.shape[1]] = f
        t = torch.from_numpy(blob).cuda()
        torch.cuda.synchronize()
        return t

    want = host_route().view(torch.int32)
    assert torch.equal(device_route().view(torch.int32), want), "the two routes differ"
    for k, fn in calls.items():
        for turn[0] in (0, 1):
            fn()
            torch.cuda.synchronize()
            assert torch.equal(out_of(0 if k == "call" else 1).view(torch.int32), want), "{} and the host route differ".format(k)
    t = {k: [] for k in ("call", "entry", "device_route", "host_route")}
    for r in range(a.reps):
        turn[0] = r % 2
        for k in (("call", "entry"), ("entry", "call"))[r % 2]:          # (another variant goes first in every window)
            t[k].append(event_window(calls[k], a.seconds))
        for k, fn in ((("device_route", device_route), ("host_route", host_route)), (("host_route", host_route), ("device_route", device_route)))[r % 2]:
            t[k].append(host_window(fn, a.seconds))
    read, written = int(sum(3 * h * w for h, w in shapes)), 12 * B * Hc * Wc
    least = (read + written) / HBM_BYTES_PER_S
    host_name = "host_route" if equal else "host_route_padded"
    return {"size": name, "batch": B, "canvas": [Hc, Wc], "bytes_read": read, "bytes_written": written,
            "hbm_least_ms_at_8TBps": round(1e3 * least, 5),
            "device": {k: stats(t[k]) for k in ("call", "entry")},
            "hbm_roofline_share": round(least / float(np.median(t["entry"])), 4),
            "hbm_roofline_share_range": [round(least / max(t["entry"]), 4), round(least / min(t["entry"]), 4)],
            "uint8_upload_bytes": int(len(px)), "f32_upload_bytes": written,
            "device_route": stats(t["device_route"]), host_name: stats(t["host_route"]),
            "host_over_device_route": round(float(np.median(t["host_route"]) / np.median(t["device_route"])), 3),
            "device_route_below_host_route": below(t["device_route"], t["host_route"]),
            "host_route_below_device_route": below(t["host_route"], t["device_route"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("image_blob_bench: no GPU -- nothing here can be timed without one")
    sizes = [("batch%d" % B, [KITTI_SHAPES[0]] * B, KITTI_SHAPES[0]) for B in (1, 2, 16)]
    sizes.append(("mixed16", [KITTI_SHAPES[b % 4] for b in range(16)], (376, 1242)))
    out = {"bench": "image_blob", "reps": a.reps, "window_s": a.seconds, "device_name": torch.cuda.get_device_name(0),
           "sizes": [bench_size(a, *s) for s in sizes]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
