"""The training solver's launches (csrc/solver.hip, csrc/adam.hip) on the parameter list of the 3-view graph
(214 M f32 elements): device time of each, its share of the time 8 TB/s would need for its bytes, and the same work through torch on the
same tensors.  In ONE process, every variant warmed up and then timed over --reps windows of >= --seconds each (HIP events around a
window of back-to-back calls), the variants alternating and their order rotating from window to window:

      norm          = mv3d_grad_norm: two launches, 4 B read per element
      sgd           = mv3d_sgd_step with a control record (coef < 1) and weight decay on the matrices: 12 B read + 8 B written
      sgd_plain     = mv3d_sgd_step without a record and without decay
      adam          = mv3d_adam_step, the existing launch: the yardstick, 16 B read + 12 B written
      adam_ctl      = mv3d_adam_step_ctl with the same record and decay
      torch_norm    = torch.nn.utils.clip_grad_norm_(foreach=True) (a max_norm that never clips: it still multiplies every gradient)
      torch_sgd     = torch.optim.SGD(foreach=True, momentum 0.9, weight_decay 5e-4).step()
      torch_adam    = torch.optim.Adam(foreach=True, weight_decay 5e-4).step()
      step_reference / step_sgd = MV3D_train_3view, bf16 MFMA trunks, 2 frames a step (bench.py's training workload): forward, four
                      losses, backward, then optim.Adam as cfg.TRAIN.SOLVER = 'reference' builds it / optim.SGD with CLIP_GRAD_NORM,
                      SKIP_NON_FINITE and WEIGHT_DECAY on as SOLVER = 'sgd' builds it, on the same network, alternating

A variant is "below" another when the gap of the medians exceeds the larger of the two spreads (max - min over the windows).  No figure
is fixed in advance.  The rates are tiny (1e-9) so that a second of steps leaves the values where they were.  Prints one JSON line;
--out writes it.

    python tools/solver_bench.py [--seconds 1.0] [--reps 3] [--no-step] [--out profiles/solver_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mv3d_tf_amd import build, optim, synth  # noqa: E402
from mv3d_tf_amd._lib import check, lib  # noqa: E402

HBM = 8.0e12                        # bytes / s: the MI355X's nominal HBM3E bandwidth
BYTES = {"norm": 4, "sgd": 20, "sgd_plain": 20, "adam": 28, "adam_ctl": 28}       # per element, without the optional 16-bit copies


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

    n = max(5, int(np.ceil(1.1 * seconds / max(run(5) / 5, 1e-7))))
    while True:
        dt = run(n)
        if dt >= seconds:
            return dt / n
        n *= 2


def windows(calls, a):
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    order = list(calls)
    for r in range(a.reps):
        for k in order[r % len(order):] + order[:r % len(order)]:
            t[k].append(event_window(calls[k], a.seconds))
    return t


def bench_launches(a, shapes):
    dev = torch.device("cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    ps = [(torch.randn(s, device=dev, generator=gen) * 0.05).requires_grad_(True) for s in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
    n = sum(p.numel() for p in ps)
    wd = lambda p: 5e-4 if p.ndim >= 2 else 0.0
    groups = lambda: [{"params": [p for p in ps if p.ndim >= 2], "weight_decay": 5e-4}, {"params": [p for p in ps if p.ndim < 2], "weight_decay": 0.0}]
    lr = 1e-9
    # the library's classes build the tables (one group here, so that every variant is ONE update launch over all tensors); the entries
    # are then called on those tables directly: device time, not the host's table checks
    sgd = optim.SGD(ps, lr=lr, momentum=0.9, clip_grad_norm=1e-3, skip_non_finite=True)
    adam = optim.Adam(ps, lr=lr)
    sgd.step()
    adam.step()
    ctl = sgd._grad_norm(ps, dev)
    record = sgd.control()
    norm_ent = sgd.__dict__["_cache"][("norm", tuple(id(p) for p in ps))]
    bufs = [sgd.state[p]["momentum_buffer"] for p in ps]
    moments = [(adam.state[p]["exp_avg"], adam.state[p]["exp_avg_sq"]) for p in ps]
    ids = tuple(id(p) for p in ps)
    table = lambda key, items, decay: sgd._tables_for(key, [p.numel() for p in ps], tuple(
        (p.data_ptr(), p.grad.data_ptr(), s0.data_ptr(), s1.data_ptr() if s1 is not None else None, p.numel(), None, wd(p) if decay else 0.0, 0)
        for p, s0, s1 in items), optim.SolverTensor, dev)
    t_sgd = table(("bench", "sgd"), [(p, b, None) for p, b in zip(ps, bufs)], True)
    t_sgd0 = table(("bench", "sgd0"), [(p, b, None) for p, b in zip(ps, bufs)], False)
    t_ctl = table(("bench", "ctl"), [(p, m, v) for p, (m, v) in zip(ps, moments)], True)
    t_adam = adam.__dict__["_cache"][(0, ids)]
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    tabs = lambda e: (P(e["dev"]), P(e["ct"]), P(e["cf"]), e["n"])
    L = lib()
    t_opt = {"torch_sgd": torch.optim.SGD(groups(), lr=lr, momentum=0.9, foreach=True),
             "torch_adam": torch.optim.Adam(groups(), lr=lr, foreach=True)}
    calls = {
        "norm": lambda: check(L.mv3d_grad_norm(*tabs(norm_ent), 1e-3, 1, P(norm_ent["partials"]), ctl, s), "mv3d_grad_norm"),
        "sgd": lambda: check(L.mv3d_sgd_step(*tabs(t_sgd), lr, 0.9, ctl, 0, s), "mv3d_sgd_step"),
        "sgd_plain": lambda: check(L.mv3d_sgd_step(*tabs(t_sgd0), lr, 0.9, None, 0, s), "mv3d_sgd_step"),
        "adam": lambda: check(L.mv3d_adam_step(*tabs(t_adam), lr, 0.9, 0.999, 1e-8, 1000, 0, s), "mv3d_adam_step"),
        "adam_ctl": lambda: check(L.mv3d_adam_step_ctl(*tabs(t_ctl), lr, 0.9, 0.999, 1e-8, 1000, ctl, 0, s), "mv3d_adam_step_ctl"),
        "torch_norm": lambda: torch.nn.utils.clip_grad_norm_(ps, 1e30, foreach=True),
        "torch_sgd": t_opt["torch_sgd"].step,
        "torch_adam": t_opt["torch_adam"].step,
    }
    t = windows(calls, a)
    out = {"elements": n, "tensors": len(ps), "chunks": t_sgd["n"], "control_record": record, "device": {k: stats(v) for k, v in t.items()}}
    out["hbm_fraction"] = {k: {"at_median": round(b * n / HBM / float(np.median(t[k])), 4), "at_min_time": round(b * n / HBM / min(t[k]), 4),
                               "at_max_time": round(b * n / HBM / max(t[k]), 4)} for k, b in BYTES.items()}
    pairs = [("sgd", "adam"), ("sgd_plain", "adam"), ("adam", "adam_ctl"), ("norm", "torch_norm"), ("sgd", "torch_sgd"), ("adam_ctl", "torch_adam")]
    out["below"] = {"%s_below_%s" % (x, y): below(t[x], t[y]) for x, y in pairs + [(y, x) for x, y in pairs]}
    out["norm_hbm_fraction_over_adam_hbm_fraction"] = round(out["hbm_fraction"]["norm"]["at_median"] / out["hbm_fraction"]["adam"]["at_median"], 4)
    return out


def bench_step(a):
    """the 3-view bf16 training step of bench.py (fast_rcnn.train_mv.bench_train_step's network, frames and step) under the two solvers"""
    from mv3d_tf_amd import sharding
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.fast_rcnn.train_mv import SolverWrapper, stack_blobs, total_loss
    from mv3d_tf_amd.networks import get_network
    np.random.seed(cfg.RNG_SEED)
    net = get_network("MV3D_train_3view")
    net.amp_dtype, net.mfma_trunk, net.cast_many, net.fused_head = torch.bfloat16, True, True, True
    params = net.parameters()
    ref = optim.Adam(params, lr=SolverWrapper.LEARNING_RATE)
    sgd = optim.SGD([{"params": [p for p in params if p.ndim >= 2], "weight_decay": 5e-4}, {"params": [p for p in params if p.ndim < 2], "weight_decay": 0.0}],
                    lr=1e-5, momentum=0.9, clip_grad_norm=10.0, skip_non_finite=True)
    net.attach_optimizer(ref)
    bucketer = sharding.GradBucketer(params, None)
    rng = np.random.RandomState(100)
    frames = []
    for k in range(2):
        _, _, info, calib, (gt_bv, gt_3d, gt_cnr) = synth.rpn_head(7000 + k, 76, 76, "peaky", return_gt=True)
        bev = (rng.random_sample((1, 608, 608, 9)) < 0.03).astype(np.float32) * rng.uniform(0, 2.4, (1, 608, 608, 9)).astype(np.float32)
        img = rng.randint(0, 255, (1, 375, 1242, 3)).astype(np.float32) - cfg.PIXEL_MEANS.astype(np.float32)
        frames.append({"lidar_bv_data": bev, "image_data": img.astype(np.float32), "lidar_fv_data": rng.uniform(0, 1, (1, 64, 512, 3)).astype(np.float32),
                       "im_info": info, "calib": calib, "gt_boxes_bv": gt_bv, "gt_boxes_3d": gt_3d, "gt_boxes_corners": gt_cnr})
    feed = stack_blobs(frames)
    for k in ("lidar_bv_data", "image_data", "lidar_fv_data"):
        feed[k] = torch.as_tensor(feed[k]).cuda()
    feed["keep_prob"] = 0.5

    def step(opt):
        def run():
            bucketer.zero_grad()
            layers = net.forward(feed)
            loss, _ = total_loss(layers)
            bucketer.reset()
            bucketer.dist_enabled = True
            loss.backward()
            bucketer.finish()
            opt.step()
        return run

    step(ref)()                                                       # the head's 16-bit weight buffers exist from here on:
    net._register_lowp(sgd)                                           # both optimizers write them in their update launch
    calls = {"step_reference": step(ref), "step_sgd": step(sgd)}
    for _ in range(2):
        for fn in calls.values():
            fn()
    t = windows(calls, a)
    bucketer.close()
    ms = lambda v: {"median_ms": round(1e3 * float(np.median(v)), 3), "min_ms": round(1e3 * min(v), 3), "max_ms": round(1e3 * max(v), 3)}
    return {"workload": "MV3D_train_3view, bf16 MFMA trunks, 2 frames a step; 'sgd' = momentum 0.9, weight decay 5e-4 on the matrices, "
                        "clip 10, guard on", "step_reference": ms(t["step_reference"]), "step_sgd": ms(t["step_sgd"]),
            "control_record_after": sgd.control(),
            "step_sgd_below_step_reference": below(t["step_sgd"], t["step_reference"]),
            "step_reference_below_step_sgd": below(t["step_reference"], t["step_sgd"])}, [tuple(p.shape) for p in params]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("solver_bench: no GPU -- nothing here can be timed without one")
    out = {"bench": "solver", "reps": a.reps, "window_s": a.seconds, "device_name": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM}
    if a.no_step:
        from mv3d_tf_amd.networks import get_network
        shapes = [tuple(p.shape) for p in get_network("MV3D_train_3view").parameters()]
    else:
        out["train_step"], shapes = bench_step(a)
        torch.cuda.empty_cache()
    out["launches"] = bench_launches(a, shapes)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
