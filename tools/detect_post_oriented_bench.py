"""The test-time tail with oriented NMS (ops.detect_post_oriented) against the axis-aligned tail (ops.detect_post, unchanged code, the
baseline) on the SAME inputs in ONE process, alternating so that both see the same machine state.  Inputs are
synth.kitti_eval_split-style scenes: per frame a few rotated car-sized objects, 70 % of the rows jittered copies of them, the rest
scattered boxes, uniform scores; pred_bv is the pixel hull of the regressed footprint (0.1 m per pixel), so both tails do real work.

Per size and tail: device arrays -> per-frame host lists (the call + ops.detect_post_lists), in --reps windows of >= --seconds after a
warm-up (median, minimum, maximum of the per-call time), and the event-timed device time of the launches alone.  Also reported: the
share of candidate pairs (i < j, per frame) that pass the extent pretest and so reach the polygon clip, and the kept detections of
both tails.  Frame 0 of the first size is checked against tests/oriented_nms_restatement.py before anything is timed.
--profile-loop N only enqueues N calls of each tail per size (for a `rocprofv3 --kernel-trace --stats -- python tools/...` run).
Prints one JSON line; --out also writes it to a file.

Run it from a source checkout: it puts tests/ on sys.path and imports oriented_nms_restatement and recall3d_restatement from there.

    python tools/detect_post_oriented_bench.py [--batch 16] [--rows 300,2000] [--max-per-image 300] [--nms 0.1] [--footprint regressed]
    (needs <repository>/tests next to tools/)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mv3d_tf_amd import build, ops, synth  # noqa: E402


def inputs(seed, B, rows, K=2):
    rng = np.random.RandomState(seed)
    R, G = B * rows, max(10, rows // 30)

    def unit(v):
        v = v + np.array([1e-3, 0])
        return v / np.sqrt((v * v).sum(1, keepdims=True))

    def boxes(n):
        ctr = np.stack([rng.uniform(5, 55, n), rng.uniform(-20, 20, n), rng.uniform(-1.9, -1.5, n)], 1)
        lwh = np.stack([rng.uniform(3, 5, n), rng.uniform(1.4, 2, n), rng.uniform(1.3, 2, n)], 1)
        return ctr, lwh, unit(rng.uniform(-1, 1, (n, 2)))

    corners, cnr_r = np.empty((R, 24), np.float32), np.empty((R, 24 * K), np.float32)
    for f in range(B):
        ctr, lwh, cs = boxes(G)
        pick, copy = rng.randint(0, G, rows), rng.random_sample(rows) < 0.7
        sc, sl_, scs = boxes(rows)

        def jitter(amount):
            jc = np.where(copy[:, None], ctr[pick] + np.hstack([rng.uniform(-amount, amount, (rows, 2)), rng.uniform(-0.1, 0.1, (rows, 1))]), sc)
            jl = np.where(copy[:, None], lwh[pick] * rng.uniform(0.9, 1.1, (rows, 3)), sl_)
            jcs = np.where(copy[:, None], unit(cs[pick] + rng.uniform(-0.05, 0.05, (rows, 2))), scs)
            return synth.box_corners(jc, jl, jcs)

        sl = slice(f * rows, (f + 1) * rows)
        corners[sl] = jitter(0.8)
        for j in range(K):
            cnr_r[sl, 24 * j:24 * j + 24] = jitter(0.4)
    scores = rng.random_sample((R, K)).astype(np.float32)
    scores[:, 0] = 1 - scores[:, 1:].max(1)
    bv = np.empty((R, 4 * K), np.float32)
    for j in range(K):                                       # the pixel hull of the regressed footprint
        x, y = cnr_r[:, 24 * j:24 * j + 4] * 10, cnr_r[:, 24 * j + 8:24 * j + 12] * 10 + 300
        bv[:, 4 * j:4 * j + 4] = np.round(np.stack([x.min(1), y.min(1), x.max(1), y.max(1)], 1))
    return scores, bv, corners, cnr_r


def pretest_share(host, B, rows, K, footprint):
    """candidate pairs i < j of every (frame, class), and how many of them pass the extent pretest"""
    import recall3d_restatement as R3
    scores, _, corners, cnr_r = host
    pairs = passed = 0
    for f in range(B):
        sl = slice(f * rows, (f + 1) * rows)
        for j in range(1, K):
            cand = scores[sl, j] > np.float32(0.05)
            foot = (cnr_r[sl, 24 * j:24 * j + 24] if footprint == "regressed" else corners[sl])[cand]
            n = foot.shape[0]
            ok = R3.pretest(*(R3.extents(foot),) * 2)
            pairs += n * (n - 1) // 2
            passed += (int(ok.sum()) - n) // 2
    return pairs, passed


def windows(fn, seconds, reps_hint):
    """per-call seconds of one window of >= `seconds`"""
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(reps_hint):
            fn()
        n += reps_hint
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n


def stats(v):
    return {"median_ms": round(1e3 * float(np.median(v)), 4), "min_ms": round(1e3 * min(v), 4), "max_ms": round(1e3 * max(v), 4)}


def bench_size(a, rows, check):
    B, K, mpi = a.batch, 2, a.max_per_image
    host = inputs(100 + rows, B, rows, K)
    arrays = [torch.as_tensor(x).cuda() for x in host]
    out_o, out_p = ops.detect_post_outputs(B, K, rows, "cuda"), ops.detect_post_outputs(B, K, rows, "cuda")
    ws = ops.detect_post_oriented_workspace(B, K, rows, "cuda")

    def oriented():
        return ops.detect_post_oriented(*arrays, None, rows, K, mpi, a.nms, footprint=a.footprint, out=out_o, workspace=ws)

    def plain():
        return ops.detect_post(*arrays, None, rows, K, mpi, a.nms, use_gpu_nms=False, out=out_p)

    tails = {"detect_post_oriented": oriented, "detect_post": plain}
    lists = {k: ops.detect_post_lists(fn()) for k, fn in tails.items()}
    if check:
        import oriented_nms_restatement as ON
        sl = slice(0, rows)
        keep, status = ON.frame_tail(host[0][sl], host[1][sl], host[2][sl], host[3][sl], K, mpi, a.nms, source=1 if a.footprint == "regressed" else 0)
        want = ON.lists(host[0][sl], host[1][sl], host[2][sl], host[3][sl], K, keep)
        assert status == 0 and np.array_equal(lists["detect_post_oriented"][0][0][1], want[0][1]), "device tail and restatement differ"
        assert np.array_equal(lists["detect_post_oriented"][0][1][1], want[1][1])
    if a.profile_loop:
        for fn in tails.values():
            for _ in range(a.profile_loop):
                fn()
        torch.cuda.synchronize()
        return {"rows": rows, "profile_loop": a.profile_loop}
    pairs, passed = pretest_share(host, B, rows, K, a.footprint)
    res = {"rows": rows, "candidate_pairs": pairs, "pairs_past_pretest": passed, "pretest_pass_share": round(passed / max(pairs, 1), 5),
           "kept_detections": {k: int(sum(len(d[1]) for d, _ in v)) for k, v in lists.items()}}
    t = {k: [] for k in tails}
    for _ in range(a.reps):
        for k, fn in tails.items():
            t[k].append(windows(lambda: ops.detect_post_lists(fn()), a.seconds, 8))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kern = {k: [] for k in tails}
    for _ in range(a.reps):
        for k, fn in tails.items():
            ev[0].record()
            for _ in range(50):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            kern[k].append(ev[0].elapsed_time(ev[1]) * 1e-3 / 50)
    for k in tails:
        res[k] = {"to_host_lists": stats(t[k]), "launches_device_only": stats(kern[k])}
    res["oriented_over_plain_to_host_lists"] = round(float(np.median(t["detect_post_oriented"]) / np.median(t["detect_post"])), 3)
    res["oriented_over_plain_launches"] = round(float(np.median(kern["detect_post_oriented"]) / np.median(kern["detect_post"])), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rows", default="300,2000")
    ap.add_argument("--max-per-image", type=int, default=300)
    ap.add_argument("--nms", type=float, default=0.1)
    ap.add_argument("--footprint", default="regressed", choices=("regressed", "proposal"))
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile-loop", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    rows = [int(r) for r in a.rows.split(",") if r]
    out = {"bench": "detect_post_oriented", "batch": a.batch, "classes": 2, "max_per_image": a.max_per_image, "nms": a.nms,
           "footprint": a.footprint, "reps": a.reps, "window_s": a.seconds, "device": torch.cuda.get_device_name(0),
           "sizes": [bench_size(a, r, check=(i == 0)) for i, r in enumerate(rows)]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
