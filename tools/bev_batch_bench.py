"""Batched BEV rasteriser (ops.point_cloud_2_top_batch, csrc/bev_raster.hip) against what was here
before it: the single-cloud entry once per frame (the same body on one frame: three launches a call), and the stored (601, 601, 9)
maps a loop used to read from disk.  Scans are
synth.point_cloud(seed, 120000) (the size of a KITTI scan), batches of 1, 2 and 16 frames.  In ONE process, every variant warmed
up and then timed over --reps windows of >= --seconds each, the variants of a batch alternating and their order rotating from
window to window:

  (a) device time, HIP events around a window of calls on points that are already on the device, nothing allocated by the batched calls:
      batched       = ops.point_cloud_2_top_batch (three launches; the resolve stores only the 16-byte vectors that hold a point),
                      the call the loops make
      batched_entry = the mv3d_point_cloud_2_top_batch entry itself, without the Python argument checks
      dense_entry   = mv3d_point_cloud_2_top_batch_dense, the same call with the resolve that stores every element: the form that
                      was measured against the entry and not kept
      loop_ops    = B calls of ops.point_cloud_2_top, one per cloud (3 B launches and B allocations from torch's caching allocator)
      loop_entry  = B calls of the mv3d_point_cloud_2_top entry itself into B preallocated maps (3 B launches, nothing else)
      piled       = (batch 1 only) the batched call on a cloud of the same size whose points all fall on an 8 x 8 block of cells:
                    what same-cell contention costs at its worst (its windows follow the others: it alternates with nothing)
  (b) from the frames' host scans to finished device maps (host clock, synchronised):
      scans       = np.concatenate, one upload, one batched call
      stored      = np.load of B stored .npy maps from a temporary directory (page cache warm), np.stack, one upload

The three batched variants trade their output buffers from window to window (see `device_calls`).  All five device variants are
checked to give the same bits before anything is timed.  A variant is "below" another when the gap of the medians exceeds the larger of the two spreads (max - min over the windows).  The synthetic clouds are uniform apart from one dense
patch; the share of same-cell contention on real KITTI scans is not measured here.  Prints one JSON line; --out also writes it.

    python tools/bev_batch_bench.py [--batches 1,2,16] [--points 120000] [--seconds 1.0] [--reps 3] [--out profiles/bev_batch_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mv3d_tf_amd import build, ops, synth  # noqa: E402


def piled_cloud(P, seed=7):
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(30.0, 30.8, P), rng.uniform(2.0, 2.8, P), rng.uniform(-2.0, 0.39, P), rng.random_sample(P)], 1).astype(np.float32)


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


def device_calls(clouds):
    """({variant: (zero-argument launch on device-resident copies of `clouds`, a function returning its output tensor)}, turn)"""
    B = len(clouds)
    pts = torch.from_numpy(np.concatenate(clouds, 0)).cuda()
    off = torch.from_numpy(np.cumsum([0] + [len(c) for c in clouds]).astype(np.int32)).cuda()
    singles = [torch.from_numpy(c).cuda() for c in clouds]
    # The three batched variants share a pool of three output buffers and trade places in it from window to window (turn[0]): where
    # the allocator put a buffer moves the time of IDENTICAL device work by a microsecond or two, far more than the windows of one
    # buffer differ, and that must show as a variant's spread, not as its median.
    pool, turn = [torch.empty((B,) + ops.BEV_SHAPE, device="cuda") for _ in range(3)], [0]
    out_of = lambda i: pool[(i + turn[0]) % 3]
    own = [torch.empty(ops.BEV_SHAPE, device="cuda") for _ in range(B)]      # (that entry wants each map 16-byte aligned: no batch buffer)
    held = {}
    entry, stream = ops.lib().mv3d_point_cloud_2_top, torch.cuda.current_stream().cuda_stream

    def loop_ops():
        held["maps"] = [ops.point_cloud_2_top(s) for s in singles]

    def loop_entry():
        for b, s in enumerate(singles):
            ops.check(entry(C.c_void_p(s.data_ptr()), s.shape[0], C.c_void_p(own[b].data_ptr()), C.c_void_p(stream)), "mv3d_point_cloud_2_top")

    def raw(name, i):
        fn = getattr(ops.lib(), name)
        return (lambda: ops.check(fn(C.c_void_p(pts.data_ptr()), C.c_void_p(off.data_ptr()), B, pts.shape[0], None,
                                     C.c_void_p(out_of(i).data_ptr()), None, C.c_void_p(stream)), name)), (lambda: out_of(i))

    return {"batched": (lambda: ops.point_cloud_2_top_batch(pts, off, out=out_of(0)), lambda: out_of(0)),
            "batched_entry": raw("mv3d_point_cloud_2_top_batch", 1), "dense_entry": raw("mv3d_point_cloud_2_top_batch_dense", 2),
            "loop_ops": (loop_ops, lambda: torch.stack(held["maps"])),
            "loop_entry": (loop_entry, lambda: torch.stack(own))}, turn


def bench_batch(a, B, tmp):
    clouds = [synth.point_cloud(100 + b, a.points) for b in range(B)]
    calls, turn = device_calls(clouds)
    maps = {}
    for k, (launch, result) in calls.items():
        launch()
        torch.cuda.synchronize()
        maps[k] = result().view(torch.int32)
    for k in ("batched_entry", "dense_entry", "loop_ops", "loop_entry"):
        assert torch.equal(maps["batched"], maps[k]), "batched and {} differ".format(k)
    occupied = float((maps["batched"] != 0).sum().item()) / B
    paths = []
    for b in range(B):                                               # the stored maps a loop used to read
        paths.append(os.path.join(tmp, "%02d_%06d.npy" % (B, b)))
        np.save(paths[-1], maps["batched"][b].view(torch.float32).cpu().numpy())

    def from_scans():
        t = ops.point_cloud_2_top_batch(np.concatenate(clouds, 0), np.cumsum([0] + [len(c) for c in clouds]))
        torch.cuda.synchronize()
        return t

    def from_stored():
        t = torch.from_numpy(np.stack([np.load(p) for p in paths])).cuda()
        torch.cuda.synchronize()
        return t

    assert torch.equal(from_scans().view(torch.int32), from_stored().view(torch.int32)), "the stored maps are not the scans' rasters"
    t = {k: [] for k in list(calls) + ["scans", "stored"]}
    order = list(calls)
    for r in range(a.reps):
        turn[0] = r
        for k in order[r % len(order):] + order[:r % len(order)]:        # (another variant goes first in every window: the first one
            t[k].append(event_window(calls[k][0], a.seconds))            # follows a host-bound stretch, and its place must not be its time)
        t["scans"].append(host_window(from_scans, a.seconds))
        t["stored"].append(host_window(from_stored, a.seconds))
    res = {"batch": B, "points_per_frame": a.points, "occupied_elements_per_frame": round(occupied, 1),
           "occupied_share": round(occupied / float(np.prod(ops.BEV_SHAPE)), 4),
           "device": {k: stats(t[k]) for k in calls},
           "dense_entry_below_batched_entry": below(t["dense_entry"], t["batched_entry"]),
           "batched_entry_below_dense_entry": below(t["batched_entry"], t["dense_entry"]),
           "batched_below_loop_ops": below(t["batched"], t["loop_ops"]), "loop_ops_below_batched": below(t["loop_ops"], t["batched"]),
           "batched_entry_below_loop_entry": below(t["batched_entry"], t["loop_entry"]),
           "loop_entry_below_batched_entry": below(t["loop_entry"], t["batched_entry"]),
           "host_scans_upload_raster": stats(t["scans"]), "host_stored_load_stack_upload": stats(t["stored"]),
           "scans_below_stored": below(t["scans"], t["stored"])}
    if B == 1:
        piled = device_calls([piled_cloud(a.points)])[0]["batched"][0]
        piled()
        res["device"]["piled"] = stats([event_window(piled, a.seconds) for _ in range(a.reps)])
    for p in paths:
        os.remove(p)
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
        raise SystemExit("bev_batch_bench: no GPU -- nothing here can be timed without one")
    with tempfile.TemporaryDirectory() as tmp:
        out = {"bench": "point_cloud_2_top_batch", "reps": a.reps, "window_s": a.seconds, "device_name": torch.cuda.get_device_name(0),
               "sizes": [bench_batch(a, int(B), tmp) for B in a.batches.split(",") if B]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
