"""Upsampled ROI features, measured two ways in ONE process on seeded tensors:

  kernels  = ops.upsample_bilinear_views / ops.upsample_bilinear_backward_views (one launch each) at the shapes the graphs give them:
             serving (batch 16: the bird's-eye-view conv5_3 76 x 76 x 512 read out of its FRAMED f16 buffer through strides, the image
             conv5_3 46 x 155 x 512 f32) and training (batch 2, f32), factors 2 and 4, forward and backward -- next to torch's
             F.interpolate(mode='bilinear') / aten.upsample_bilinear2d_backward on the same tensors (as channels-last views, so both
             walk NHWC memory).  torch uses ANOTHER coordinate rule (half-pixel centres), so the values differ and nothing is compared;
             for a 16-bit input torch also writes a 16-bit map, half the bytes of the f32 map RoiPool reads: every variant is reported
             with the bytes IT moves (input read once + output written once; backward: g_y read once + g_x written once).
             HIP events around windows of >= --seconds, the variants alternating, --reps windows each; the launches rotate over enough
             copies of the tensors (>= --footprint-mb) that none is still in the 256 MiB Infinity Cache at its next turn.  Reported:
             time per call and the fraction of the 8 TB/s HBM roofline for those bytes (a whole-call figure from a back-to-back
             window; kernel times come from a kernel trace in a run of its own).
  steps    = the 3-view bf16 training step (fast_rcnn.train_mv.bench_train_step) and the batch-16 f16 serving step as a captured graph
             (fast_rcnn.test_mv.bench_serve_step) under cfg.ROI_UPSAMPLE (1, 1, 1), (2, 2, 2) and (4, 2, 4), alternating.

Prints one JSON line and writes it to profiles/upsample_bench.json (--out: another file).

    python tools/upsample_bench.py [--seconds 0.3] [--reps 3] [--skip-steps] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mv3d_tf_amd import build, ops  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, the figure DESIGN.md measures against
#        name,          batch, H,  W,   C,   input type,     framed
SHAPES = [("serve_bev", 16, 76, 76, 512, torch.float16, True),
          ("serve_image", 16, 46, 155, 512, torch.float32, False),
          ("train_bev", 2, 76, 76, 512, torch.float32, False),
          ("train_image", 2, 46, 155, 512, torch.float32, False)]
FACTORS = (2, 4)


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

    pilot = 10
    n = max(pilot, int(np.ceil(1.1 * seconds / max(run(pilot) / pilot, 1e-7))))
    while True:
        dt = run(n)
        if dt >= seconds:
            return dt / n
        n *= 2


def bench_shape(a, name, B, H, W, C, dt, framed, s):
    size = torch.empty((), dtype=dt).element_size()
    n_in, n_up = B * H * W * C, B * s * H * s * W * C
    fwd_bytes, bwd_bytes = n_in * size + n_up * 4, n_up * 4 + n_in * 4
    t_fwd_bytes, t_bwd_bytes = n_in * size + n_up * size, n_up * 4 + n_in * 4
    copies = max(2, int(np.ceil(a.footprint_mb * 2 ** 20 / fwd_bytes)))
    gen = torch.Generator(device="cuda").manual_seed(B + H + s)
    xs = []
    for _ in range(copies):
        if framed:
            buf = torch.zeros((B, H + 2, W + 2, C), dtype=dt, device="cuda")
            buf[:, 1:-1, 1:-1] = torch.randn((B, H, W, C), device="cuda", generator=gen).to(dt)
            xs.append(buf[:, 1:-1, 1:-1])
        else:
            xs.append(torch.randn((B, H, W, C), device="cuda", generator=gen).to(dt))
    gs = [torch.randn((B, s * H, s * W, C), device="cuda", generator=gen) for _ in range(copies)]
    ys = [torch.empty((B, s * H, s * W, C), device="cuda") for _ in range(copies)]
    gxs = [torch.empty((B, H, W, C), device="cuda") for _ in range(copies)]
    k_fwd = lambda i: ops.upsample_bilinear_views([(xs[i % copies], s)], outs=[ys[i % copies]])
    k_bwd = lambda i: ops.upsample_bilinear_backward_views([(gs[i % copies], s)], outs=[gxs[i % copies]])
    t_fwd = lambda i: F.interpolate(xs[i % copies].permute(0, 3, 1, 2), scale_factor=s, mode="bilinear", align_corners=False)
    t_bwd = lambda i: torch.ops.aten.upsample_bilinear2d_backward(gs[i % copies].permute(0, 3, 1, 2), [s * H, s * W], [B, C, H, W], False, None, None)
    variants = [("kernel_forward", k_fwd, fwd_bytes), ("torch_forward", t_fwd, t_fwd_bytes), ("kernel_backward", k_bwd, bwd_bytes),
                ("torch_backward", t_bwd, t_bwd_bytes)]
    for _, fn, _ in variants:                                        # warm-up: every buffer, every variant
        for i in range(copies):
            fn(i)
    torch.cuda.synchronize()
    times = {n: [] for n, _, _ in variants}
    for _ in range(a.reps):
        for n, fn, _ in variants:                                    # the variants alternate
            times[n].append(event_window(fn, a.seconds))
    out = {"shape": name, "factor": s, "batch": B, "height": H, "width": W, "channels": C, "input": str(dt).split(".")[-1],
           "input_layout": "interior of a framed buffer, read through strides" if framed else "contiguous", "rotating_copies": copies}
    for n, _, nbytes in variants:
        t = float(np.median(times[n]))
        out[n] = dict(stats(times[n]), bytes=nbytes, TB_per_s=round(nbytes / t / 1e12, 3), fraction_of_8TBps=round(nbytes / t / HBM_PEAK, 4))
    out["torch_over_kernel_forward_time"] = round(out["torch_forward"]["median_us"] / out["kernel_forward"]["median_us"], 2)
    out["torch_over_kernel_backward_time"] = round(out["torch_backward"]["median_us"] / out["kernel_backward"]["median_us"], 2)
    print("upsample_bench: %s x%d done" % (name, s), file=sys.stderr, flush=True)
    del xs, gs, ys, gxs
    torch.cuda.empty_cache()
    return out


def bench_steps(a):
    from mv3d_tf_amd.fast_rcnn import test_mv, train_mv
    from mv3d_tf_amd.fast_rcnn.config import cfg
    variants = [(1, 1, 1), (2, 2, 2), (4, 2, 4)]
    keys = ("ms_per_step", "ms_per_step_min", "ms_per_step_median")
    train = {str(v): [] for v in variants}
    serve = {str(v): [] for v in variants}
    try:
        for _ in range(a.step_reps):
            for v in variants:                                       # the variants alternate
                cfg.ROI_UPSAMPLE = v
                np.random.seed(cfg.RNG_SEED)
                r = train_mv.bench_train_step(0, 1, None, amp=torch.bfloat16, views=3, mfma=True, seconds=a.step_seconds)
                train[str(v)].append({k: r[k] for k in keys if k in r})
                torch.cuda.empty_cache()
                r = test_mv.bench_serve_step(0, 1, None, batch=16, seconds=a.step_seconds, dtypes=("fp16_mfma_graph",))["fp16_mfma_graph"]
                serve[str(v)].append({k: r[k] for k in keys if k in r})
                print("upsample_bench: steps under %s done" % (v,), file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
    finally:
        cfg.ROI_UPSAMPLE = (1, 1, 1)
    return {"train_step_3view_bf16_2_frames": train, "serve_step_batch16_f16_graph": serve,
            "note": "every entry is one run of the repository's own step benchmark (a new network each) under that cfg.ROI_UPSAMPLE; at "
                    "(4, 2, 4) the bird's-eye-view up-map has 304 x 304 = 92 416 pixels, more than the RoiPool pair's own kernels take "
                    "(65 534): all views of the training step then go through the plain forward and the index + gather backward"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--footprint-mb", type=float, default=1024.0)
    ap.add_argument("--step-seconds", type=float, default=1.0)
    ap.add_argument("--step-reps", type=int, default=2)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "upsample_bench.json"))
    a = ap.parse_args()
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("upsample_bench: no GPU -- nothing here can be timed without one")
    out = {"bench": "upsample", "reps": a.reps, "window_s": a.seconds, "footprint_mb": a.footprint_mb,
           "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "kernels": [bench_shape(a, *sh, s) for sh in SHAPES for s in FACTORS]}
    if not a.skip_steps:
        out["steps"] = bench_steps(a)
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
