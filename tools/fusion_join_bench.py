"""The deep-fusion join, measured two ways in ONE process on seeded tensors:

  join     = ops.fusion_join / ops.fusion_join_backward (one launch each) against the torch sequence they replace, written with
             as few launches as torch needs -- relu_, the mean over the views (mean(1); for several paths or partial keeps ONE
             weighted reduction, a GEMM with the (P, V) weights keep / n), native_dropout; and native_dropout_backward, one scale
             (the same GEMM transposed), one threshold_backward on the whole tensor: three launches each way -- on the same
             values, equal up to rounding (asserted before anything is timed).
             Shapes: the training head's joins (R = 256 rows, C = 2048, V = 3; P = 1 and P = 4 = main + auxiliary paths; bf16 and
             f32; join 1 reads one h for all paths, join 2 one per path) and the serving head's (R = 4800, f16, P = 1, no mask).
             HIP events around windows of >= --seconds, the variants alternating, --reps windows each; the launches rotate over
             enough copies of the tensors (>= --footprint-mb) that none is still in the 256 MiB Infinity Cache at its next turn.
             bytes = what the contract must move (h once, the mask, the output; backward: h, g_out, the mask, g_h), reported
             over the time per call and as a fraction of the 8 TB/s HBM peak DESIGN.md uses.  At R = 256 a join moves 4 - 30 MB:
             the time per call of such a window is the DISPATCH cost (the Python wrapper and the launch), not kernel time and not
             the memory system, and is to be read that way; kernel times come from a kernel trace in a run of its own.
  steps    = the 3-view bf16 training step (fast_rcnn.train_mv.bench_train_step) and the batch-16 f16 serving step as a captured
             graph (fast_rcnn.test_mv.bench_serve_step) under cfg.FUSION 'early', 'deep', and 'deep' with cfg.TRAIN.AUX_LOSSES and
             DROP_PATH (at inference the auxiliary paths are removed: the third serving variant is the second one again).

Prints one JSON line and writes it to profiles/fusion_join_bench.json (--out: another file).

    python tools/fusion_join_bench.py [--seconds 0.5] [--reps 3] [--skip-steps] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mv3d_tf_amd import build, ops  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, the figure DESIGN.md measures against
MAIN_AUX = [[1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
#        name,              dtype,          R,    C,    V, keep,        sets_in = P?, masked
SHAPES = [("train_join1_P1", torch.bfloat16, 256, 2048, 3, [[1, 1, 1]], False, True),
          ("train_join1_P4", torch.bfloat16, 256, 2048, 3, MAIN_AUX, False, True),
          ("train_join2_P4", torch.bfloat16, 256, 2048, 3, MAIN_AUX, True, True),
          ("train_join1_P1_f32", torch.float32, 256, 2048, 3, [[1, 1, 1]], False, True),
          ("train_join1_P4_f32", torch.float32, 256, 2048, 3, MAIN_AUX, False, True),
          ("serve_join_P1", torch.float16, 4800, 2048, 3, [[1, 1, 1]], False, False)]


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


def torch_weights(keep, dt, device):
    """(P, V) keep[p][v] / n_p in the tensors' type: the weights of the mean over each path's kept views"""
    k = torch.tensor(keep, dtype=torch.float32, device=device)
    return (k / k.sum(1, keepdim=True)).to(dt)


def torch_forward(h, W, all_kept, p_drop):
    """the sequence the join replaces, as few launches as torch needs: relu_ (in place: h is the torch variant's own copy), the mean
    over the views -- mean(1) when one path keeps every view, otherwise ONE weighted reduction (a GEMM with the (P, V) weights) --
    and native_dropout on the mean.  Returns (out, mask); h holds the ReLU output afterwards."""
    a = h.relu_()
    S, V, R, C = a.shape
    P = W.shape[0]
    if all_kept:
        m = a.mean(1)
    elif S == 1:
        m = torch.mm(W, a.view(V, R * C)).view(P, R, C)
    else:
        m = torch.bmm(W.unsqueeze(1), a.view(P, V, R * C)).view(P, R, C)
    if p_drop is None:
        return m, None
    return torch.native_dropout(m, p_drop, True)


def torch_backward(a, g_out, W, all_kept, mask, scale):
    """native_dropout_backward, one scale (for several paths or partial keeps the weighted sum over the paths, one GEMM), one
    threshold_backward on the whole (S, V, R, C)"""
    S, V, R, C = a.shape
    P = W.shape[0]
    g = g_out if mask is None else torch.ops.aten.native_dropout_backward(g_out, mask, scale)
    if all_kept:
        pre = (g * (1.0 / V)).unsqueeze(1).expand(S, V, R, C)
    elif S == 1:
        pre = torch.mm(W.t(), g.view(P, R * C)).view(1, V, R, C)
    else:
        pre = torch.bmm(W.unsqueeze(2), g.view(P, 1, R * C)).view(P, V, R, C)
    return torch.ops.aten.threshold_backward(pre, a, 0.0)


def bench_shape(a, name, dt, R, C, V, keep, per_path, masked):
    P = len(keep)
    S = P if per_path else 1
    size = torch.empty((), dtype=dt).element_size()
    E = R * C
    used = sum(1 for s in range(S) for v in range(V) if any(keep[p][v] for p in range(P) if S == 1 or p == s))
    fwd_bytes = used * E * size + P * E * size + (P * E if masked else 0)
    bwd_bytes = used * E * size + P * E * size + (P * E if masked else 0) + S * V * E * size
    copies = max(2, int(np.ceil(a.footprint_mb * 2 ** 20 / max(fwd_bytes, bwd_bytes))))
    gen = torch.Generator(device="cuda").manual_seed(R + P + S)
    hs = [torch.randn((S, V, R, C), device="cuda", generator=gen).to(dt) for _ in range(copies)]
    gs = [torch.randn((P, R, C), device="cuda", generator=gen).to(dt) for _ in range(copies)]
    drops = [(torch.rand((P, R, C), device="cuda", generator=gen) < 0.5).to(torch.uint8) if masked else None for _ in range(copies)]
    scale = 2.0 if masked else 1.0
    # the two ways agree (torch's dropout draws its own mask: the join is given that mask)
    W = torch_weights(keep, dt, "cuda")
    all_kept = P == 1 and all(keep[0])
    relus = [h.clone() for h in hs]                                  # the torch variant's own copies: relu_ works in place
    out_t, mask_t = torch_forward(relus[0], W, all_kept, 0.5 if masked else None)
    relu_t = relus[0]
    out_k = ops.fusion_join(hs[0], keep, None if mask_t is None else mask_t.to(torch.uint8), scale)
    tol = {torch.float32: 1e-6, torch.float16: 2e-3, torch.bfloat16: 1.6e-2}[dt]
    assert torch.allclose(out_k.float(), out_t.float(), rtol=tol, atol=tol), name
    g_t = torch_backward(relu_t, gs[0], W, all_kept, mask_t, scale)
    g_k = ops.fusion_join_backward(hs[0], gs[0], keep, None if mask_t is None else mask_t.to(torch.uint8), scale)
    assert torch.allclose(g_k.float(), g_t.float(), rtol=tol, atol=tol * float(gs[0].float().abs().max()) * P), name
    for r in relus:
        r.relu_()
    masks = [None if d is None else d.bool() for d in drops]
    k_fwd = lambda i: ops.fusion_join(hs[i % copies], keep, drops[i % copies], scale)
    k_bwd = lambda i: ops.fusion_join_backward(hs[i % copies], gs[i % copies], keep, drops[i % copies], scale)
    t_fwd = lambda i: torch_forward(relus[i % copies], W, all_kept, 0.5 if masked else None)
    t_bwd = lambda i: torch_backward(relus[i % copies], gs[i % copies], W, all_kept, masks[i % copies], scale)
    variants = [("join_forward", k_fwd, fwd_bytes), ("torch_forward", t_fwd, fwd_bytes), ("join_backward", k_bwd, bwd_bytes),
                ("torch_backward", t_bwd, bwd_bytes)]
    for _, fn, _ in variants:                                        # warm-up: every buffer, every variant
        for i in range(copies):
            fn(i)
    torch.cuda.synchronize()
    times = {n: [] for n, _, _ in variants}
    for _ in range(a.reps):
        for n, fn, _ in variants:                                    # the variants alternate
            times[n].append(event_window(fn, a.seconds))
    out = {"shape": name, "dtype": str(dt).split(".")[-1], "rows": R, "channels": C, "views": V, "paths": P, "sets_in": S, "mask": masked,
           "rotating_copies": copies, "launches": {"join": "1 forward, 1 backward"}}
    for n, _, nbytes in variants:
        t = float(np.median(times[n]))
        out[n] = dict(stats(times[n]), contract_bytes=nbytes, TB_per_s=round(nbytes / t / 1e12, 3), fraction_of_8TBps=round(nbytes / t / HBM_PEAK, 4))
    out["torch_over_join_forward"] = round(out["torch_forward"]["median_us"] / out["join_forward"]["median_us"], 2)
    out["torch_over_join_backward"] = round(out["torch_backward"]["median_us"] / out["join_backward"]["median_us"], 2)
    out["bound"] = ("dispatch: the time per call is the Python wrapper's and the launch's cost in a back-to-back window, not kernel "
                    "time (a few MB per launch)") if R <= 256 else "memory"
    print("fusion_join_bench: %s done" % name, file=sys.stderr, flush=True)
    del hs, gs, drops, relus, masks
    torch.cuda.empty_cache()
    return out


def bench_steps(a):
    from mv3d_tf_amd.fast_rcnn import test_mv, train_mv
    from mv3d_tf_amd.fast_rcnn.config import cfg
    variants = [("early", "early", False), ("deep", "deep", False), ("deep_aux_drop_path", "deep", True)]
    train = {n: [] for n, _, _ in variants}
    serve = {n: [] for n, _, _ in variants}
    try:
        for _ in range(a.step_reps):
            for n, fusion, extras in variants:                       # the variants alternate
                cfg.FUSION, cfg.TRAIN.AUX_LOSSES, cfg.TRAIN.DROP_PATH = fusion, extras, extras
                np.random.seed(cfg.RNG_SEED)
                r = train_mv.bench_train_step(0, 1, None, amp=torch.bfloat16, views=3, mfma=True, seconds=a.step_seconds)
                train[n].append({k: r[k] for k in ("ms_per_step", "ms_per_step_min", "ms_per_step_median") if k in r})
                torch.cuda.empty_cache()
                r = test_mv.bench_serve_step(0, 1, None, batch=16, seconds=a.step_seconds, dtypes=("fp16_mfma_graph",))["fp16_mfma_graph"]
                serve[n].append({k: r[k] for k in ("ms_per_step", "ms_per_step_min", "ms_per_step_median") if k in r})
                print("fusion_join_bench: steps under %s done" % n, file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
    finally:
        cfg.FUSION, cfg.TRAIN.AUX_LOSSES, cfg.TRAIN.DROP_PATH = "early", False, False
    return {"train_step_3view_bf16_2_frames": train, "serve_step_batch16_f16_graph": serve,
            "note": "every entry is one run of the repository's own step benchmark (a new network each); the serving step has no auxiliary paths "
                    "and no drop-path, so its third variant repeats the second"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--footprint-mb", type=float, default=1024.0)
    ap.add_argument("--step-seconds", type=float, default=1.0)
    ap.add_argument("--step-reps", type=int, default=2)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fusion_join_bench.json"))
    a = ap.parse_args()
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("fusion_join_bench: no GPU -- nothing here can be timed without one")
    out = {"bench": "fusion_join", "reps": a.reps, "window_s": a.seconds, "footprint_mb": a.footprint_mb,
           "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "join": [bench_shape(a, *s) for s in SHAPES]}
    if not a.skip_steps:
        out["steps"] = bench_steps(a)
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
