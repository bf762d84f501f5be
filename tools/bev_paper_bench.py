"""The paper's BEV encoding (ops.point_cloud_2_top_paper, csrc/bev_paper.hip) against the reference-encoding
call on the same inputs (ops.point_cloud_2_top_batch, csrc/bev_raster.hip) and against a host raster of the same definition.  Scans
are synth.point_cloud(seed, 120000) (the size of a KITTI scan), batches of 1, 2 and 16 frames.  In ONE process, every variant warmed
up and then timed over --reps windows of >= --seconds each, the two device paths alternating and their order rotating from window to
window:

  (a) device time, HIP events around a window of calls on points that are already on the device, out= and workspace= given (nothing
      allocated):
      paper       = ops.point_cloud_2_top_paper: clear of maps + winner words, scatter (one atomic per slice hit, the count, the 64-bit
                    winner), resolve -> (B, 601, 601, 10)
      reference   = ops.point_cloud_2_top_batch -> (B, 601, 601, 9)
      ratio       = paper / reference, window by window (the two of a window run back to back), with its spread
      piled       = (batch 1 only) the paper call on a cloud of the same size whose points all fall on an 8 x 8 block of cells = 64
                    cells: what same-cell contention costs at its worst; piled_reference = the reference-encoding call on that cloud
                    (their windows follow the others)
  (b) from the frames' host scans to finished device maps (host clock, synchronised):
      scans       = np.concatenate, one upload, one paper call
      numpy       = a vectorised numpy raster of the same definition frame by frame (`numpy_paper` below), np.stack, one upload

The two device paths write into TWO buffers that they trade from window to window (the reference map is a view of the first 9 / 10 of
one), as tools/bev_batch_bench.py trades its pool: where the allocator put a buffer moves the time of identical device work.  Before
anything is timed the paper map is checked against `numpy_paper` bit for bit, at every batch.  The synthetic clouds are uniform apart
from one dense patch; the share of same-cell contention on real KITTI scans is not measured here.  Prints one JSON line; --out also
writes it.

    python tools/bev_paper_bench.py [--batches 1,2,16] [--points 120000] [--seconds 1.0] [--reps 3] [--out profiles/bev_paper_bench.json]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bev_batch_bench import below, event_window, host_window, piled_cloud, stats  # noqa: E402
from mv3d_tf_amd import build, ops, synth  # noqa: E402

F32 = np.float32


def numpy_paper(pts):
    """(P, 4) f32 -> (601, 601, 10) f32: the definition of DESIGN.md section 3.24 on MV3D's ranges, vectorised (no cell of that map can
    fall outside it and no index is negative, so neither the wrap nor the IndexError of the general definition occurs)"""
    H, W, M = 601, 601, 8
    x, y, z, r = pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]
    keep = (x > F32(0.0)) & (x < F32(60.0)) & (y > F32(-30.0)) & (y < F32(30.0))
    nxt = -2.0 + 0.3
    heights = np.array([-2.0, nxt] + [-2.0 + i * (nxt - -2.0) for i in range(2, M)])
    with np.errstate(invalid="ignore"):
        zd = z.astype(np.float64)[:, None]
        S = (zd >= heights[None]) & (zd < heights[None] + 0.3) & keep[:, None]
    kept = S.any(1)
    idx = np.nonzero(kept)[0]
    xi = (-y[idx] / F32(0.1)).astype(np.int32) + 300
    yi = (-x[idx] / F32(0.1)).astype(np.int32) + 600
    cell = yi.astype(np.int64) * W + xi
    zc = z[idx] + F32(0.0)
    top = np.zeros((H * W, M + 2), F32)
    for i in range(M):
        m = S[idx, i]
        hi = np.full(H * W, -np.inf, F32)
        np.maximum.at(hi, cell[m], zc[m])
        hit = hi > -np.inf
        top[hit, i] = hi[hit] - F32(-2.0)
    order = np.lexsort((idx, zc, cell))                                  # by cell, then z, then row: a cell's winner is its last
    last = np.nonzero(np.append(cell[order][1:] != cell[order][:-1], True))[0] if len(order) else np.zeros(0, np.int64)
    top[cell[order][last], M] = r[idx][order][last]
    T = np.array([F32(min(1.0, math.log(n + 1) / math.log(64))) for n in range(64)], F32)
    n = np.bincount(cell, minlength=H * W)
    top[:, M + 1] = np.where(n > 0, T[np.minimum(n, 63)], F32(0.0))
    return top.reshape(H, W, M + 2)


def device_calls(clouds):
    """({variant: (launch on device-resident copies of `clouds`, a function returning its output tensor)}, turn)"""
    B = len(clouds)
    pts = torch.from_numpy(np.concatenate(clouds, 0)).cuda()
    off = torch.from_numpy(np.cumsum([0] + [len(c) for c in clouds]).astype(np.int32)).cuda()
    n10, n9 = int(np.prod(ops.BEV_PAPER_SHAPE)), int(np.prod(ops.BEV_SHAPE))
    pool, turn = [torch.empty(B * n10, device="cuda") for _ in range(2)], [0]
    ws = torch.empty(ops.point_cloud_2_top_paper_workspace_bytes(B), dtype=torch.uint8, device="cuda")
    paper_out = lambda: pool[turn[0] % 2].view((B,) + ops.BEV_PAPER_SHAPE)
    ref_out = lambda: pool[(turn[0] + 1) % 2][:B * n9].view((B,) + ops.BEV_SHAPE)
    return {"paper": (lambda: ops.point_cloud_2_top_paper(pts, off, out=paper_out(), workspace=ws), paper_out),
            "reference": (lambda: ops.point_cloud_2_top_batch(pts, off, out=ref_out()), ref_out)}, turn


def bench_batch(a, B):
    clouds = [synth.point_cloud(100 + b, a.points) for b in range(B)]
    calls, turn = device_calls(clouds)
    calls["reference"][0]()
    calls["paper"][0]()
    torch.cuda.synchronize()
    host_maps = np.stack([numpy_paper(c) for c in clouds])
    got = calls["paper"][1]().cpu().numpy()
    assert np.array_equal(got.view(np.int32), host_maps.view(np.int32)), "the device map and the numpy raster of the definition differ"
    occupied = float(np.count_nonzero(got)) / B

    def from_scans():
        t = ops.point_cloud_2_top_paper(np.concatenate(clouds, 0), np.cumsum([0] + [len(c) for c in clouds]))
        torch.cuda.synchronize()
        return t

    def from_numpy():
        t = torch.from_numpy(np.stack([numpy_paper(c) for c in clouds])).cuda()
        torch.cuda.synchronize()
        return t

    t = {k: [] for k in ("paper", "reference", "scans", "numpy")}
    for r in range(a.reps):
        turn[0] = r
        for k in (("paper", "reference"), ("reference", "paper"))[r % 2]:
            t[k].append(event_window(calls[k][0], a.seconds))
        t["scans"].append(host_window(from_scans, a.seconds))
        t["numpy"].append(host_window(from_numpy, min(a.seconds, 0.2)))          # (one call is already seconds at batch 16)
    ratio = [p / q for p, q in zip(t["paper"], t["reference"])]
    res = {"batch": B, "points_per_frame": a.points, "occupied_elements_per_frame": round(occupied, 1),
           "occupied_share": round(occupied / float(np.prod(ops.BEV_PAPER_SHAPE)), 4),
           "device": {k: stats(t[k]) for k in ("paper", "reference")},
           "paper_over_reference": {"median": round(float(np.median(ratio)), 4), "min": round(min(ratio), 4), "max": round(max(ratio), 4)},
           "reference_below_paper": below(t["reference"], t["paper"]),
           "host_scans_upload_raster": stats(t["scans"]), "host_numpy_raster_upload": stats(t["numpy"]),
           "scans_below_numpy": below(t["scans"], t["numpy"])}
    if B == 1:
        pile = piled_cloud(a.points)
        calls, turn = device_calls([pile])
        calls["paper"][0]()
        torch.cuda.synchronize()
        got = calls["paper"][1]().cpu().numpy()
        assert np.array_equal(got.view(np.int32), numpy_paper(pile)[None].view(np.int32)), "piled: device and numpy differ"
        assert np.count_nonzero(got[..., 9]) == 64
        res["device"]["piled"] = stats([event_window(calls["paper"][0], a.seconds) for _ in range(a.reps)])
        res["device"]["piled_reference"] = stats([event_window(calls["reference"][0], a.seconds) for _ in range(a.reps)])
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
        raise SystemExit("bev_paper_bench: no GPU -- nothing here can be timed without one")
    out = {"bench": "point_cloud_2_top_paper", "reps": a.reps, "window_s": a.seconds, "device_name": torch.cuda.get_device_name(0),
           "sizes": [bench_batch(a, int(B)) for B in a.batches.split(",") if B]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
