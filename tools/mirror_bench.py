"""Left/right mirror of a training frame's maps (cfg.TRAIN.USE_FLIPPED): the device kernel against the host flip it replaces, on the
two maps of a frame -- image (B, 375, 1242, 3) and BEV (B, 601, 601, 9), f32 -- for B = 2 and B = 16.  In ONE process, on seeded
arrays, every variant warmed up and then timed over --reps windows of >= --seconds each, the variants of a size alternating:

  kernel   = ops.mirror_columns (mv3d_mirror_columns) alone, HIP events around a window of launches.  The launches rotate over
             enough copies of the array (>= --footprint-mb in all) that none is still in the 256 MiB Infinity Cache when its
             turn comes again; bytes/s = 2 x the array size (every element read once, written once) over the time per launch,
             also as a fraction of the 8 TB/s HBM peak DESIGN.md uses.
  copy     = torch.Tensor.copy_ between two such sets of the same arrays, same rotation, same byte count: the yardstick.
  A        = the host way: np.ascontiguousarray(x[:, :, ::-1]) + upload, to a finished device tensor (host clock, synchronised).
  B        = upload + kernel, to the same tensor.

A's and B's tensors are asserted bit-identical before anything is timed.  Prints one JSON line; --out also writes it to a file.

    python tools/mirror_bench.py [--batches 2,16] [--seconds 1.0] [--reps 3] [--out profiles/mirror_bench.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mv3d_tf_amd import build, ops  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, the figure DESIGN.md measures against
MAPS = (("image", (375, 1242, 3)), ("bev", (601, 601, 9)))


def stats(v):
    return {"median_ms": round(1e3 * float(np.median(v)), 4), "min_ms": round(1e3 * min(v), 4), "max_ms": round(1e3 * max(v), 4)}


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


def host_window(fn, seconds):
    """seconds per call of fn() (which ends synchronised) over one host-clock window of >= `seconds`"""
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n


def bench_map(a, name, shape, B):
    rng = np.random.RandomState(B * 1000 + shape[1])
    x = rng.uniform(-128, 128, (B,) + shape).astype(np.float32)
    nbytes = x.nbytes
    copies = max(2, int(np.ceil(a.footprint_mb * 2 ** 20 / nbytes)))

    def host_way():
        t = torch.from_numpy(np.ascontiguousarray(x[:, :, ::-1])).cuda()
        torch.cuda.synchronize()
        return t

    def device_way():
        t = ops.mirror_columns(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        return t

    assert torch.equal(host_way().view(torch.int32), device_way().view(torch.int32)), "host and device mirrors differ"
    src = [torch.from_numpy(x).cuda() for _ in range(copies)]
    dst = [torch.empty_like(src[0]) for _ in range(copies)]
    kernel = lambda i: ops.mirror_columns(src[i % copies])
    copy = lambda i: dst[i % copies].copy_(src[i % copies])
    for i in range(copies):                                          # warm-up: every buffer, every variant
        kernel(i)
        copy(i)
    host_way()
    device_way()
    tk, tc, ta, tb = [], [], [], []
    for _ in range(a.reps):
        tk.append(event_window(kernel, a.seconds))
        tc.append(event_window(copy, a.seconds))
        ta.append(host_window(host_way, a.seconds))
        tb.append(host_window(device_way, a.seconds))
    rate = lambda t: 2.0 * nbytes / float(np.median(t))
    out = {"map": name, "shape": [B] + list(shape), "array_bytes": nbytes, "rotating_copies": copies,
           "kernel": dict(stats(tk), TB_per_s=round(rate(tk) / 1e12, 3), fraction_of_8TBps=round(rate(tk) / HBM_PEAK, 3)),
           "copy_": dict(stats(tc), TB_per_s=round(rate(tc) / 1e12, 3), fraction_of_8TBps=round(rate(tc) / HBM_PEAK, 3)),
           "kernel_rate_over_copy_rate": round(rate(tk) / rate(tc), 3),
           "A_host_flip_plus_upload": stats(ta), "B_upload_plus_kernel": stats(tb),
           "B_below_A_by_more_than_A_spread": bool(np.median(ta) - np.median(tb) > max(ta) - min(ta))}
    del src, dst
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,16")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--footprint-mb", type=float, default=1024.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("mirror_bench: no GPU -- nothing here can be timed without one")
    out = {"bench": "mirror_columns", "reps": a.reps, "window_s": a.seconds, "footprint_mb": a.footprint_mb,
           "device": torch.cuda.get_device_name(0), "bytes_counted": "2 x array (one read, one write per element)",
           "sizes": [bench_map(a, name, shape, int(B)) for B in a.batches.split(",") if B for name, shape in MAPS]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
