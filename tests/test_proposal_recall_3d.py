"""Proposal recall by oriented BEV / 3D IoU on the device (mv3d_proposal_recall_3d, ops.proposal_recall_3d,
datasets.proposal_recall_3d.evaluate_recall_3d, rpn_msr.generate.imdb_proposals(..., with_3d=True)).  The checker is the plain-numpy
restatement tests/recall3d_restatement.py (corner formation pinned to the reference's lidar_3d_to_corners through the oracle, the
evaluator's clip restatement, the reference's matching loop).  All comparisons are equalities: overlaps are f64 in a fixed order,
counts are integers."""
import ctypes as C
import inspect
import os
import pickle

import numpy as np
import pytest
import scipy.sparse

import kitti_eval_restatement as KR
import recall3d_restatement as R3
from mv3d_tf_amd import synth

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def hiplib():
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def ops(torch_cuda, hiplib):
    from mv3d_tf_amd import ops as o
    return o


def restated_launch(calls=None):
    """datasets.proposal_recall_3d._launch_3d with the restatement in the kernels' place"""
    def launch(boxes, gts, limits, thresholds, on_short):
        if calls is not None:
            calls.append(dict(boxes=boxes, gts=gts, limits=list(limits), thresholds=thresholds, on_short=on_short))
        ov, counts, status = R3.recall_vectors_3d(boxes, gts, limits, thresholds, on_short)
        if (status & 2).any():
            raise ValueError("non-finite")
        if (status & 1).any():
            raise AssertionError("short frame")
        return ov, counts
    return launch


def unit(rng, n):
    v = rng.uniform(-1, 1, (n, 2)) + np.array([1e-3, 0])
    return v / np.sqrt((v * v).sum(1, keepdims=True))


def scene(rng, R, G, rotated):
    """one frame: G rotated car-sized objects (every third one axis-aligned) in a small area, so that many pairs overlap, and R
    proposals, (R, 6) axis-aligned or (R, 24) rotated corners; every second object has a copy among the proposals (exact for the
    axis-aligned proposals of axis-aligned objects, jittered otherwise), three proposals are exact duplicates of each other and the
    last object is a duplicate of the first"""
    n = R + G
    ctr = np.stack([rng.uniform(5, 25, n), rng.uniform(-8, 8, n), rng.uniform(-1.9, -1.5, n)], 1)      # bottom centres
    lwh = np.stack([rng.uniform(3, 5, n), rng.uniform(1.4, 2, n), rng.uniform(1.3, 2, n)], 1)
    cs = unit(rng, n)
    cs[R::3] = [1.0, 0.0]
    for j in range(0, min(R, G), 2):
        i = (7 * j) % R
        jit = np.zeros(3) if j % 4 == 0 else np.append(rng.uniform(-0.4, 0.4, 2), rng.uniform(-0.1, 0.1))
        ctr[i], lwh[i], cs[i] = ctr[R + j] + jit, lwh[R + j], cs[R + j]
    if rotated:
        cnr = synth.box_corners(ctr, lwh, cs)
        b, g = cnr[:R].copy(), cnr[R:].copy()
    else:
        mid = ctr + np.hstack([np.zeros((n, 2)), lwh[:, 2:3] / 2])
        b = np.hstack([mid[:R], lwh[:R]]).astype(np.float32)
        g = synth.box_corners(ctr[R:], lwh[R:], cs[R:])
        for j in range(0, G, 3):                                                 # axis-aligned objects: the corners a proposal would have
            g[j] = R3.box6_corners(np.hstack([mid[R + j], lwh[R + j]]).astype(np.float32))[0]
    if R > 4:
        b[R - 1] = b[2]
        b[R // 2] = b[2]
    if G > 2:
        g[G - 1] = g[0]
    return b, g


SWEEP_LIMITS = (None, 1, 5, 64, 1000)
SWEEP_R = (0, 1, 63, 64, 65, 300)
SWEEP_G = (0, 1, 5, 17)


def sweep_frames(rotated, seed=5):
    rng = np.random.RandomState(seed + (100 if rotated else 0))
    frames = [scene(rng, R, G, rotated) for R in SWEEP_R for G in SWEEP_G]
    return [b for b, _ in frames], [g for _, g in frames]


@pytest.fixture(scope="module", params=["box6", "cnr24"])
def sweep(request):
    boxes, gts = sweep_frames(request.param == "cnr24")
    want = {mode: R3.recall_vectors_3d(boxes, gts, SWEEP_LIMITS, None, mode) for mode in ("zero", "raise")}
    for v in want.values():
        for a in v:
            a.setflags(write=False)
    return boxes, gts, want


# ------------------------------------------------------------------ without a GPU
def test_box6_corners_equal_the_reference(oracle):
    rng = np.random.RandomState(2)
    b = np.hstack([rng.uniform(-70, 70, (500, 3)), rng.uniform(0.1, 12, (500, 3))]).astype(np.float32)
    b[10:20, 3:] = 0                                                             # zero-size boxes
    b[20:25, 3] = 0; b[25:30, 5] = 0
    b[30:60, :3] = (rng.uniform(-1, 1, (30, 3)) * 1e6).astype(np.float32)        # large coordinates: the half is rounded away in part
    b[60:70, 3:] = (rng.uniform(1e3, 1e5, (10, 3))).astype(np.float32)
    b[70:80] = np.round(b[70:80])                                                # odd integer sizes: halves on .5
    got, want = R3.box6_corners(b), oracle.lidar_3d_to_corners(b)
    assert got.dtype == np.float32 and got.shape == (500, 24) and np.array_equal(got, want)
    assert np.array_equal(R3.corners_of(b), want) and np.array_equal(R3.corners_of(want), want)
    # the footprint is k = 0..3 with x [+,+,-,-], y [+,-,-,+]; z is - for the first four corners
    one = R3.box6_corners(np.float32([[10, 2, -1, 4, 2, 1.5]]))[0]
    assert one[:4].tolist() == [12, 12, 8, 8] and one[8:12].tolist() == [3, 1, 1, 3] and one[16:].tolist() == [-1.75] * 4 + [-0.25] * 4


def test_pretest_rejects_no_overlapping_pair():
    """the vectorised pretest against the sequential definition, and: every pair it rejects has a zero clipped IoU"""
    rng = np.random.RandomState(4)
    b, g = scene(rng, 120, 17, True)
    ea, eb = R3.extents(b), R3.extents(g)
    ok = R3.pretest(ea, eb)
    for i in range(0, 120, 7):
        for j in range(17):
            xa, ya, xb, yb = b[i, :4].astype(np.float64), b[i, 8:12].astype(np.float64), g[j, :4].astype(np.float64), g[j, 8:12].astype(np.float64)
            reject = xa.max() < xb.min() or xb.max() < xa.min() or ya.max() < yb.min() or yb.max() < ya.min()
            assert ok[i, j] == (not reject)
            if reject:
                assert KR.iou_pair(b[i], g[j]) == (0.0, 0.0)
    assert ok.any() and not ok.all()
    # equal bounds pass: touching boxes are clipped, not rejected
    e = np.float64([[0, 4, 0, 2]])
    assert R3.pretest(e, np.float64([[4, 8, 0, 2]]))[0, 0] and not R3.pretest(e, np.float64([[np.nextafter(4, 5), 8, 0, 2]]))[0, 0]


def small_roidb(rng, frames=(5, 0, 3, 7, 4)):
    """a roidb with boxes_bv / boxes_corners whose rows carry their own index, one background row and one crowd row per frame"""
    roidb = []
    for G in frames:
        n = G + 2
        side = np.float32([20, 40, 100, 30, 60, 110, 25, 90, 35])[:n]
        bv = np.stack([np.arange(n, dtype=np.float32), np.zeros(n, np.float32), np.arange(n, dtype=np.float32) + side - 1, side - 1], 1)
        cls = np.ones(n, np.int32); cls[G] = 0
        ov = np.tile(np.float32([0, 1]), (n, 1)); ov[G] = [1, 0]; ov[G + 1] = [0, 0.5]
        _, cnr = scene(rng, 0, n, True)
        roidb.append(dict(boxes_bv=bv, boxes_corners=cnr, gt_classes=cls, gt_overlaps=scipy.sparse.csr_matrix(ov)))
    return roidb


def test_object_selection_is_the_bev_rule():
    from mv3d_tf_amd.datasets import proposal_recall as PR, proposal_recall_3d as P3
    roidb = small_roidb(np.random.RandomState(3))
    seen = 0
    for area in PR.AREAS:
        gts_bv, num_bv = PR.select_objects(roidb, area, "bv")
        gts, num_pos = P3.select_corners(roidb, area)
        assert num_pos == num_bv and [len(g) for g in gts] == [len(g) for g in gts_bv]
        for e, g, gb in zip(roidb, gts, gts_bv):
            rows = gb[:, 0].astype(int)                                          # boxes_bv rows carry their index in x1
            assert g.dtype == np.float32 and g.shape == (len(rows), 24) and np.array_equal(g, e["boxes_corners"][rows])
        seen += num_pos
    assert seen > 0 and P3.select_corners(roidb, "all")[1] == 19 and P3.select_corners(roidb, "small")[1] < 19
    with pytest.raises(AssertionError):
        P3.select_corners(roidb, "huge")
    # seg_areas, where present, decide, as in select_objects
    e = dict(roidb[0], seg_areas=np.float32([5000, 10, 10, 10, 10, 10, 10]))
    assert P3.select_corners([e], "small")[1] == PR.select_objects([e], "small", "bv")[1] == 4


def same_dict(a, b):
    assert sorted(a) == sorted(b) == ["ar", "gt_overlaps", "recalls", "thresholds"]
    assert all(np.array_equal(a[k], b[k]) for k in a) and a["gt_overlaps"].dtype == np.float64


def test_dataset_layer_without_a_device(monkeypatch):
    from mv3d_tf_amd.datasets import proposal_recall as PR, proposal_recall_3d as P3
    rng = np.random.RandomState(8)
    roidb = small_roidb(rng)
    gts, num_pos = P3.select_corners(roidb, "all")
    # proposals: copies of some objects plus scattered boxes; frame 2 has none
    cands = []
    for f, g in enumerate(gts):
        b, _ = scene(rng, 0 if f == 2 else 12, 0, False)
        for j in range(0, min(len(b), len(g)), 2):
            x, y, z = g[j, :4].mean(), g[j, 8:12].mean(), g[j, 16:].mean()
            b[j + 1] = np.float32([x, y, z, 4, 1.8, 1.5])
        cands.append(b)
    calls = []
    monkeypatch.setattr(P3, "_launch_3d", restated_launch(calls))
    res = P3.evaluate_recall_3d(roidb, cands)
    assert len(calls) == 1 and calls[0]["limits"] == [None] and calls[0]["thresholds"].dtype == np.float64
    assert np.array_equal(calls[0]["thresholds"], np.arange(0.5, 0.95 + 1e-5, 0.05)) and calls[0]["on_short"] == "raise"
    assert all(np.array_equal(a, b) for a, b in zip(calls[0]["gts"], gts))
    ov, counts, _ = R3.recall_vectors_3d(cands, gts, (None,))
    keep = np.concatenate([np.full(len(g), len(b) > 0) for b, g in zip(cands, gts)])
    want = {m: {"ar": (counts[mi, 0] / float(num_pos)).mean(), "recalls": counts[mi, 0] / float(num_pos),
                "thresholds": np.arange(0.5, 0.95 + 1e-5, 0.05), "gt_overlaps": np.sort(ov[mi, 0][keep])} for mi, m in enumerate(R3.METRICS)}
    same_dict(res, want["3d"])
    assert num_pos == 19 and keep.sum() == 16 and res["gt_overlaps"].size == 16 and (res["gt_overlaps"] > 0).any()
    same_dict(P3.evaluate_recall_3d(roidb, cands, metric="bev"), want["bev"])
    assert (want["bev"]["gt_overlaps"] != want["3d"]["gt_overlaps"]).any()
    # a tuple of metrics: a dictionary, from the same launch
    calls.clear()
    both = P3.evaluate_recall_3d(roidb, cands, metric=("bev", "3d"))
    assert len(calls) == 1 and sorted(both) == ["3d", "bev"]
    same_dict(both["bev"], want["bev"]); same_dict(both["3d"], want["3d"])
    # a list of limits: one dictionary per limit from ONE launch per chunk
    calls.clear()
    limits = [None, 1, 3, 1000]
    many = P3.evaluate_recall_3d(roidb, cands, limit=limits, metric=("bev", "3d"), on_short="zero")
    assert len(calls) == 1 and calls[0]["limits"] == limits and calls[0]["on_short"] == "zero"
    assert isinstance(many["3d"], list) and len(many["3d"]) == 4 and len(many["bev"]) == 4
    same_dict(many["3d"][0], want["3d"]); same_dict(many["3d"][3], want["3d"])
    same_dict(P3.evaluate_recall_3d(roidb, cands, limit=3, metric="bev", on_short="zero"), many["bev"][2])
    with pytest.raises(AssertionError):                                          # limit 1 leaves frames short: the reference's assert
        P3.evaluate_recall_3d(roidb, cands, limit=1)
    # a workspace small enough to force one chunk per frame with pairs: the same result
    pairs = [len(b) * len(g) for b, g in zip(cands, gts)]
    calls.clear()
    split = P3.evaluate_recall_3d(roidb, cands, limit=limits, metric=("bev", "3d"), on_short="zero", max_workspace_bytes=16 * max(pairs))
    assert len(calls) >= 3 and sum(len(c["boxes"]) for c in calls) == len(roidb)
    assert P3.frame_chunks(pairs, 16 * max(pairs)) == [(0, 3), (3, 4), (4, 5)] and P3.frame_chunks(pairs, 1 << 30) == [(0, 5)]
    for m in R3.METRICS:
        for a, b in zip(split[m], many[m]):
            same_dict(a, b)
    with pytest.raises(ValueError):
        P3.frame_chunks(pairs, 16 * max(pairs) - 16)
    # the dictionary of imdb_proposals(..., with_3d=True), rows with the batch column in front, explicit thresholds
    res7 = P3.evaluate_recall_3d(roidb, {"bv": None, "image": None, "3d": [np.hstack([np.zeros((len(b), 1), np.float32), b]) for b in cands]},
                                 thresholds=[0.25, 0.5])
    assert np.array_equal(res7["gt_overlaps"], want["3d"]["gt_overlaps"]) and res7["recalls"].shape == (2,)
    assert res7["recalls"][1] == want["3d"]["recalls"][0] and res7["recalls"][0] >= res7["recalls"][1]
    for bad in (dict(metric="2d"), dict(metric=()), dict(metric=("bev", "bv"))):
        with pytest.raises(ValueError):
            P3.evaluate_recall_3d(roidb, cands, **bad)
    with pytest.raises(ValueError):
        P3.evaluate_recall_3d(roidb, None)


def test_signatures():
    from mv3d_tf_amd.datasets.kitti_mv3d import kitti_mv3d
    from mv3d_tf_amd.datasets.proposal_recall_3d import evaluate_recall_3d
    from mv3d_tf_amd.rpn_msr.generate import imdb_proposals
    p = inspect.signature(imdb_proposals).parameters
    assert list(p) == ["sess", "net", "imdb", "with_3d"] and p["with_3d"].default is False
    q = inspect.signature(evaluate_recall_3d).parameters
    assert list(q) == ["roidb", "candidate_boxes", "thresholds", "area", "limit", "metric", "on_short", "max_workspace_bytes"]
    assert [q[k].default for k in list(q)[2:]] == [None, "all", None, "3d", "raise", 1 << 30]
    k = inspect.signature(kitti_mv3d.evaluate_recall_3d).parameters
    assert list(k)[:2] == ["self", "candidate_boxes"] and k["metric"].default == "3d" and k["limit"].default is None


def test_argument_validation_before_any_device_call(hiplib):
    L = hiplib.lib()
    assert hiplib.Recall3dSplit is not None and "mv3d_proposal_recall_3d" in hiplib.EXPORTS
    assert "mv3d_proposal_recall_3d_workspace_bytes" in hiplib.EXPORTS
    for pairs in (0, 1, 30000, 2 ** 31 - 1):
        assert L.mv3d_proposal_recall_3d_workspace_bytes(pairs) == 16 * pairs
    A = 4096                                                 # a non-NULL "pointer" (never dereferenced: refused before any HIP call)

    def call(box_off, gt_off, pair_off=None, num_boxes=None, num_gts=None, num_pairs=None, ptrs=None, outs=(A, A, A, A), limits=1,
             thresholds=10, mode=0, fmt=0, split=True):
        bo, go = np.asarray(box_off, np.int32), np.asarray(gt_off, np.int32)
        po = np.concatenate([[0], np.cumsum(np.diff(bo.astype(np.int64)) * np.diff(go.astype(np.int64)))]) if pair_off is None else pair_off
        po = np.asarray(po, np.int32)
        p = [bo.ctypes.data, go.ctypes.data, po.ctypes.data, A, A, A, A, A, A, A] if ptrs is None else ptrs(bo, go, po)
        s = hiplib.Recall3dSplit(len(bo) - 1, int(go[-1]) if num_gts is None else num_gts, limits, thresholds, mode, fmt,
                                 int(bo[-1]) if num_boxes is None else num_boxes, int(po[-1]) if num_pairs is None else num_pairs, *p)
        return L.mv3d_proposal_recall_3d(C.byref(s) if split else None, outs[0], outs[1], outs[2], outs[3], None)

    good = ([0, 3, 3, 10], [0, 2, 4, 4])                     # pairs 6, 0, 0
    bad = hiplib.ERR_INVALID_ARG
    assert call(*good, split=False) == bad
    for k in range(10):                                      # every pointer of the descriptor, one at a time
        def ptrs(bo, go, po, k=k):
            p = [bo.ctypes.data, go.ctypes.data, po.ctypes.data, A, A, A, A, A, A, A]
            p[k] = None
            return p
        assert call(*good, ptrs=ptrs) == bad, k
    for k in range(4):                                       # the workspace and every output
        outs = [A, A, A, A]
        outs[k] = None
        assert call(*good, outs=outs) == bad, k
    assert call([0, 3, 2, 10], good[1], pair_off=[0, 6, 6, 6]) == bad                      # non-monotone proposal offsets
    assert call(good[0], [0, 2, 1, 4], pair_off=[0, 6, 6, 6]) == bad                       # non-monotone object offsets
    assert call([1, 3, 3, 10], good[1]) == bad and call([-1, 3, 3, 10], good[1]) == bad    # offsets that do not start at 0
    assert call(good[0], [1, 2, 4, 4]) == bad and call(*good, pair_off=[1, 6, 6, 6]) == bad
    assert call(good[0], [0, 2, 4, -4]) == bad
    assert call(*good, num_boxes=11) == bad and call(*good, num_gts=5) == bad and call(*good, num_pairs=7) == bad
    assert call(*good, pair_off=[0, 6, 6, 7]) == bad and call(*good, pair_off=[0, 5, 6, 6]) == bad and call(*good, pair_off=[0, 6, 5, 6]) == bad
    assert call([0, 3, 3, 10], [0, 2, 259, 259]) == bad                                    # 257 objects in one frame
    assert call(*good, num_boxes=2 ** 31) == bad and call(*good, num_pairs=2 ** 31) == bad # 2^31 proposals / pairs
    assert call([0, 2 ** 23], [0, 256], pair_off=[0, -2 ** 31], num_pairs=2 ** 31) == bad  # a frame whose pairs reach 2^31
    assert call(*good, limits=0) == bad and call(*good, thresholds=-1) == bad
    assert call(*good, mode=2) == bad and call(*good, mode=-1) == bad and call(*good, fmt=2) == bad and call(*good, fmt=-1) == bad
    # the two launches on their own validate the same way
    bo, go, po = (np.asarray(a, np.int32) for a in (good[0], good[1], [0, 6, 6, 6]))
    def desc(**kw):
        v = dict(F=3, G=4, L=1, T=10, mode=0, fmt=0, N=10, P=6)
        v.update(kw)
        return hiplib.Recall3dSplit(v["F"], v["G"], v["L"], v["T"], v["mode"], v["fmt"], v["N"], v["P"], bo.ctypes.data, go.ctypes.data,
                                    po.ctypes.data, A, A, A, A, A, A, A)
    for kw in (dict(P=7), dict(N=11), dict(G=5), dict(L=0), dict(T=-1), dict(mode=2), dict(fmt=2)):
        assert L.mv3d_proposal_recall_3d_overlaps(C.byref(desc(**kw)), A, A, None) == bad, kw
        assert L.mv3d_proposal_recall_3d_match(C.byref(desc(**kw)), A, A, A, A, None) == bad, kw
    assert L.mv3d_proposal_recall_3d_overlaps(None, A, A, None) == bad and L.mv3d_proposal_recall_3d_match(None, A, A, A, A, None) == bad
    assert L.mv3d_proposal_recall_3d_overlaps(C.byref(desc()), None, A, None) == bad
    assert L.mv3d_proposal_recall_3d_overlaps(C.byref(desc()), A, None, None) == bad
    for k in range(4):
        outs = [A, A, A, A]
        outs[k] = None
        assert L.mv3d_proposal_recall_3d_match(C.byref(desc()), *outs, None) == bad, k
    # the Python layer: shapes and dtypes
    from mv3d_tf_amd import ops
    assert ops.RECALL3D_METRICS == R3.METRICS
    assert ops._recall3d_boxes(np.zeros((3, 7), np.float32), "boxes")[0].shape == (3, 6)
    assert ops._recall3d_boxes(np.zeros((3, 6), np.float64), "boxes")[1] == 0 and ops._recall3d_boxes(np.zeros((3, 24), np.float32), "boxes")[1] == 1
    for shape in ((3, 4), (3, 5), (3, 8), (24,)):
        with pytest.raises(ValueError):
            ops._recall3d_boxes(np.zeros(shape, np.float32), "boxes")
    with pytest.raises(ValueError):
        ops._recall3d_boxes(np.full((1, 6), 0.1, np.float64), "boxes")


def test_cli_parses_its_options():
    from mv3d_tf_amd.datasets import proposal_recall_3d as P3
    a = P3.parser().parse_args(["--kitti", "/data/kitti", "--proposals", "out/proposals_3d.pkl"])
    assert (a.kitti, a.image_set, a.proposals, a.limits, a.metric, a.area, a.on_short) == (
        "/data/kitti", "val", "out/proposals_3d.pkl", [10, 50, 100, 300, 1000, 2000], ("bev", "3d"), "all", "zero")
    a = P3.parser().parse_args(["--kitti", "k", "--image-set", "train", "--proposals", "p.pkl", "--limits", "10,all,300", "--metric", "3d",
                                "--area", "96-128", "--on-short", "raise"])
    assert (a.image_set, a.limits, a.metric, a.area, a.on_short) == ("train", [10, None, 300], ("3d",), "96-128", "raise")
    assert P3.parser().parse_args(["--kitti", "k", "--proposals", "p", "--metric", "3d,bev"]).metric == ("3d", "bev")
    for bad in (["--proposals", "p.pkl"], ["--kitti", "k", "--proposals", "p", "--metric", "bv"], ["--kitti", "k", "--proposals", "p", "--metric", ""],
                ["--kitti", "k", "--proposals", "p", "--area", "x"], ["--kitti", "k", "--proposals", "p", "--on-short", "skip"]):
        with pytest.raises(SystemExit):
            P3.parser().parse_args(bad)
    # AR is over the reference's ten thresholds; 0.25 is the extra one in front
    assert P3.CLI_THRESHOLDS[0] == 0.25 and np.array_equal(P3.CLI_THRESHOLDS[1:], np.arange(0.5, 0.95 + 1e-5, 0.05))


# ------------------------------------------------------------------ on the device
def run(ops, torch, boxes, gts, limits=(None,), thresholds=None, on_short="raise", as_tensors=False, batch_column=False):
    """per-frame lists -> (the device result, host (gt_overlaps, counts, status)) of ONE call, without the raising read-back"""
    box_off = np.concatenate([[0], np.cumsum([len(b) for b in boxes])])
    gt_off = np.concatenate([[0], np.cumsum([len(g) for g in gts])])
    width = next((np.asarray(b).shape[1] for b in boxes if len(b)), 6)
    allb = np.concatenate([np.asarray(b, np.float32).reshape(-1, width) for b in boxes] + [np.zeros((0, width), np.float32)])
    allg = np.concatenate([np.asarray(g, np.float32).reshape(-1, 24) for g in gts] + [np.zeros((0, 24), np.float32)])
    if batch_column:
        allb = np.hstack([np.full((len(allb), 1), 7, np.float32), allb])
    if as_tensors:
        allb, allg = torch.as_tensor(allb).cuda(), torch.as_tensor(allg).cuda()
    sp = ops.Recall3dSplit(allb, box_off, allg, gt_off, torch.device("cuda", 0))
    out = ops.proposal_recall_3d(sp, limits, thresholds, on_short)
    torch.cuda.synchronize()
    return out, tuple(t.cpu().numpy() for t in out)


def same(got, want):
    return all(np.array_equal(a, b) and a.dtype == b.dtype and a.shape == b.shape for a, b in zip(got, want))


@gpu
def test_sweep_equals_restatement(ops, torch_cuda, sweep):
    boxes, gts, want = sweep
    out, got = run(ops, torch_cuda, boxes, gts, SWEEP_LIMITS, None, "zero")
    ov, counts, status = got
    assert same(got, want["zero"])
    assert ov.shape[:2] == (2, len(SWEEP_LIMITS)) and ov.dtype == np.float64 and counts.dtype == np.int32 and not status.any()
    assert counts.min(axis=(1, 2)).tolist() != counts.max(axis=(1, 2)).tolist() and counts[0].max() > 0 and counts[1].max() > 0
    assert (ov > 0.99).any() and (ov == -1.0).any() and (ov == 0.0).any() and (ov[0] != ov[1]).any()     # both planes, the clip ran
    h = ops.proposal_recall_3d_host(out)
    assert same(h, got)
    # several limits in one call == that many single-limit calls
    for li, lim in enumerate(SWEEP_LIMITS):
        _, (ov1, counts1, _) = run(ops, torch_cuda, boxes, gts, (lim,), None, "zero")
        assert np.array_equal(ov1[:, 0], ov[:, li]) and np.array_equal(counts1[:, 0], counts[:, li]), lim


@gpu
def test_short_frames_raise_or_count_as_misses(ops, torch_cuda, sweep):
    boxes, gts, want = sweep
    out, got = run(ops, torch_cuda, boxes, gts, SWEEP_LIMITS, None, "raise")
    ov, counts, status = got
    assert same(got, want["raise"])
    assert (status & 1).any() and not (status & 2).any()
    ov0 = want["zero"][0]
    short = (ov != ov0)
    assert short.any() and (ov[short] == -1.0).all() and (ov0[short] == 0.0).all()      # 'zero' records 0.0 exactly where 'raise' has -1.0
    with pytest.raises(AssertionError):
        ops.proposal_recall_3d_host(out)


@gpu
def test_box_formats_and_input_kinds_agree(ops, torch_cuda):
    """(N, 6) rows == their corners as (N, 24); device tensors == host arrays; the batch column in front is dropped"""
    boxes, gts = sweep_frames(False)
    _, ref = run(ops, torch_cuda, boxes, gts, SWEEP_LIMITS, None, "zero")
    _, got = run(ops, torch_cuda, [R3.box6_corners(b) for b in boxes], gts, SWEEP_LIMITS, None, "zero")
    assert same(got, ref)
    _, got = run(ops, torch_cuda, boxes, gts, SWEEP_LIMITS, None, "zero", as_tensors=True, batch_column=True)
    assert same(got, ref)
    _, got = run(ops, torch_cuda, boxes, gts, SWEEP_LIMITS, None, "zero", batch_column=True)
    assert same(got, ref)
    _, got = run(ops, torch_cuda, [R3.box6_corners(b) for b in boxes], gts, SWEEP_LIMITS, None, "zero", as_tensors=True)
    assert same(got, ref)


def edge_pairs():
    """(proposal corners, object corners) of one-pair frames, and what each is about"""
    c6 = lambda *v: R3.box6_corners(np.float32([v]))[0]
    rot = lambda ctr, lwh, deg: synth.box_corners([ctr], [lwh], [[np.cos(np.radians(deg)), np.sin(np.radians(deg))]])[0]
    flip = lambda c: np.concatenate([c[k:k + 4][::-1] for k in range(0, 24, 4)])          # reversed winding, bottom and top face
    pairs = [
        ("touching in x", c6(16, 1, 0, 4, 2, 2), c6(12, 1, 0, 4, 2, 2)),                  # a.minx == b.maxx == 14: passes the pretest
        ("touching in y", c6(12, 3, 0, 4, 2, 2), c6(12, 1, 0, 4, 2, 2)),
        ("touching at a corner", c6(16, 3, 0, 4, 2, 2), c6(12, 1, 0, 4, 2, 2)),
        ("one ulp apart", c6(np.nextafter(np.float32(16), np.float32(17)), 1, 0, 4, 2, 2), c6(12, 1, 0, 4, 2, 2)),
        ("object at 45 degrees", c6(20, 0, -0.8, 3.9, 1.6, 1.56), rot([20.3, 0.2, -1.6], [4.2, 1.7, 1.5], 45)),
        ("extents overlap, boxes do not", c6(22.6, 2.6, -0.8, 1.6, 1.6, 1.56), rot([20, 0, -1.6], [5, 1.5, 1.5], 45)),
        ("reversed winding", c6(20, 0, -0.8, 3.9, 1.6, 1.56), flip(rot([20.3, 0.2, -1.6], [4.2, 1.7, 1.5], 20))),
        ("reversed proposal", flip(rot([20, 0, -1.6], [3.9, 1.6, 1.56], 10)), rot([20.3, 0.2, -1.6], [4.2, 1.7, 1.5], 20)),
        ("zero length", c6(20, 0, -0.8, 0, 1.6, 1.56), rot([20.3, 0.2, -1.6], [4.2, 1.7, 1.5], 20)),
        ("zero height", c6(20, 0, -0.8, 3.9, 1.6, 0), rot([20.3, 0.2, -1.6], [4.2, 1.7, 1.5], 20)),
        ("disjoint in z", c6(20, 0, 3.0, 3.9, 1.6, 1.56), rot([20.3, 0.2, -1.6], [4.2, 1.7, 1.5], 20)),
        ("identical", c6(20, 0, -0.8, 3.9, 1.6, 1.56), c6(20, 0, -0.8, 3.9, 1.6, 1.56)),
        ("identical, rotated", rot([20.3, 0.2, -1.6], [4.2, 1.7, 1.5], 33), rot([20.3, 0.2, -1.6], [4.2, 1.7, 1.5], 33)),
        ("far apart", c6(50, 20, -0.8, 3.9, 1.6, 1.56), rot([20.3, 0.2, -1.6], [4.2, 1.7, 1.5], 20)),
    ]
    return [p[0] for p in pairs], [p[1][None] for p in pairs], [p[2][None] for p in pairs]


@gpu
def test_geometry_edge_pairs(ops, torch_cuda):
    names, boxes, gts = edge_pairs()
    want = R3.recall_vectors_3d(boxes, gts, (None,), None, "raise")
    _, got = run(ops, torch_cuda, boxes, gts)
    assert same(got, want)
    ov = dict(zip(names, got[0][:, 0, :].T))                                    # name -> (bev, 3d) of that one pair
    for name, b, g in zip(names, boxes, gts):
        passes = R3.pretest(R3.extents(b), R3.extents(g))[0, 0]
        assert tuple(ov[name]) == (KR.iou_pair(b[0], g[0]) if passes else (0.0, 0.0)), name
        assert passes == (name not in ("one ulp apart", "far apart")), name
    for name in ("touching in x", "touching in y", "touching at a corner", "one ulp apart", "extents overlap, boxes do not", "far apart"):
        assert tuple(ov[name]) == (0.0, 0.0), name
    for name in ("object at 45 degrees", "reversed winding", "reversed proposal"):
        assert 0.1 < ov[name][1] < ov[name][0] < 1.0, name
    assert ov["disjoint in z"][0] > 0.1 and ov["disjoint in z"][1] == 0.0 and ov["disjoint in z"][0] == ov["reversed winding"][0]
    assert ov["zero height"][0] == ov["reversed winding"][0] and ov["zero height"][1] == 0.0
    assert abs(ov["identical"][0] - 1.0) < 1e-12 and abs(ov["identical"][1] - 1.0) < 1e-12 and abs(ov["identical, rotated"][1] - 1.0) < 1e-12
    # the same pairs as ONE frame (14 proposals x 14 objects): the matching over a matrix with ties at 0.0 and near 1.0
    one = ([np.concatenate(boxes)], [np.concatenate(gts)])
    _, got = run(ops, torch_cuda, *one, limits=(None, 3))
    assert same(got, R3.recall_vectors_3d(*one, (None, 3), None, "raise"))


@gpu
def test_non_finite_coordinate_flags_its_frame_only(ops, torch_cuda):
    rng = np.random.RandomState(9)
    frames = [scene(rng, 40, 4, False) for _ in range(5)]
    boxes, gts = [b for b, _ in frames], [g for _, g in frames]
    boxes[1][30, 2] = np.nan                                 # behind limit 10, and z is no part of the footprint: flagged for every limit
    gts[3][1, 21] = np.inf                                   # a top-face z
    want = R3.recall_vectors_3d(boxes, gts, (None, 10), None, "raise")
    out, got = run(ops, torch_cuda, boxes, gts, (None, 10))
    ov, counts, status = got
    assert status.tolist() == [0, 2, 0, 2, 0] and same(got, want)
    assert (ov[:, :, 4:8] == 0.0).all() and (ov[:, :, 12:16] == 0.0).all() and (ov[:, :, :4] >= 0).all() and (ov[:, :, :4] > 0).any()
    with pytest.raises(ValueError):
        ops.proposal_recall_3d_host(out)
    # (R, 24) proposals: a non-finite top-face value of a row that no limit reaches
    cn = [R3.box6_corners(b) for b in boxes]
    cn[1][30, 16:] = boxes[0][30, 2]; cn[1][39, 23] = -np.inf
    _, got = run(ops, torch_cuda, cn, gts, (None, 10))
    assert got[2].tolist() == [0, 2, 0, 2, 0] and same(got, R3.recall_vectors_3d(cn, gts, (None, 10), None, "raise"))


@gpu
def test_frames_beyond_one_workgroup_and_beyond_the_used_row_mask(ops, torch_cuda):
    """R = 2000 spans 16 row chunks of the overlap kernel; R = 4096 + 300 has its matches behind the match kernel's used-row bits"""
    rng = np.random.RandomState(13)
    b0, g0 = scene(rng, 2000, 3, False)
    b0[:, 0] = rng.uniform(0, 60, 2000); b0[:, 1] = rng.uniform(-30, 30, 2000)             # spread out: few pairs are clipped
    for k, row in enumerate((1999, 1029, 127, 128, 1023, 1024)):                           # copies at the chunk borders
        b0[row] = np.float32([g0[k % 3, :4].mean(), g0[k % 3, 8:12].mean(), g0[k % 3, 16:].mean(), 4 + 0.1 * k, 1.7, 1.5])
    R = 4096 + 300
    b1, g1 = scene(rng, R, 2, False)
    b1[:, 0] += 100                                                                        # far from the objects ...
    g1[1] = g1[0]
    mid = np.float32([g1[0, :4].mean(), g1[0, 8:12].mean(), g1[0, 16:].mean()])
    b1[4096 + 200] = np.append(mid, np.float32([4, 1.7, 1.5]))                             # ... except two rows behind the mask:
    b1[4096 + 250] = np.append(mid + np.float32([0.3, 0.1, 0]), np.float32([4, 1.7, 1.5])) # both objects prefer the first
    b1[4095] = np.append(mid + np.float32([0.9, 0.3, 0]), np.float32([4, 1.7, 1.5]))
    boxes, gts = [b0, b1], [g0, g1]
    limits = (None, 4096 + 225, 1025, 128)
    want = R3.recall_vectors_3d(boxes, gts, limits, None, "raise")
    _, got = run(ops, torch_cuda, boxes, gts, limits)
    assert same(got, want) and not got[2].any()
    ov = got[0]
    assert (ov[:, 0, :3] > 0.05).all() and (ov[1, 0, 3:] > 0.05).all() and ov[1, 0, 3] > ov[1, 0, 4] > ov[1, 1, 4] > 0 and (ov[:, 2:, 3:] == 0).all()


@gpu
def test_256_objects_in_one_frame(ops, torch_cuda):
    rng = np.random.RandomState(21)
    b, g = scene(rng, 300, 256, False)
    b[:, 0] = rng.uniform(0, 60, 300); b[:, 1] = rng.uniform(-30, 30, 300)
    spread = np.stack([rng.uniform(0, 60, 256), rng.uniform(-30, 30, 256)], 1).astype(np.float32)
    g[:, :8] += (spread[:, :1] - g[:, :1]); g[:, 8:16] += (spread[:, 1:] - g[:, 8:9])
    for j in range(0, 256, 3):
        b[j] = np.float32([g[j, :4].mean(), g[j, 8:12].mean(), g[j, 16:].mean(), 4, 1.7, 1.5])
    limits = (None, 100, 256)
    want = R3.recall_vectors_3d([b], [g], limits, None, "zero")
    _, got = run(ops, torch_cuda, [b], [g], limits, None, "zero")
    assert same(got, want) and not got[2].any() and (got[0] > 0.1).sum() > 100 and (got[0][:, 1] == 0.0).sum() >= 2 * 156


def tied_columns_frame():
    """one frame, 70 objects x 80 proposals, axis-aligned 4 x 2 x 2 boxes on multiples of 1 / 64 (every overlap is exact in f64):
    objects 3 and 67 (another wave of the round reduction) are copies of their best proposal X shifted by -0.25 and +0.25 in x,
    the same overlap 7.5 / 8.5, the largest of the frame; their second-best proposals differ clearly.  Every other object has
    one proposal of its own with an overlap of its own, footprint intersection 8 - (33 + 2 k) / 32, which no value of the two
    tied objects equals (their intersections are multiples of 1 / 2)."""
    box = lambda x, y: [x, y, -1.0, 4.0, 2.0, 2.0]
    gts, boxes = [], []
    for k in range(70):
        x, y = 10.0 * (k % 10), 10.0 * (k // 10) - 30.0
        gts.append(box(x, y))
        if k not in (3, 67):
            boxes.append(box(x + (33 + 2 * k) / 64.0, y))
    x, y = 30.0, -30.0                                       # the slot of object 3; object 67 moves next to it
    gts[3], gts[67] = box(x - 0.25, y), box(x + 0.25, y)
    boxes += [box(x, y), box(x - 1.25, y), box(x + 2.25, y)] # X; 6 / 10 with object 3, 5 / 11 with 67; 4 / 12 with 67
    boxes += [box(200.0 + 10.0 * i, 0.0) for i in range(9)]  # far from everything
    b = np.float32(boxes)[np.random.RandomState(3).permutation(80)]
    return b, R3.box6_corners(np.float32(gts))


@gpu
def test_tied_columns_across_waves_take_the_first(ops, torch_cuda):
    """the first-index tie-break of the round reduction across waves: whichever of the two tied objects stands at index 3 takes
    the shared proposal, and the one at index 67 is left with its own second best, which differs between the two"""
    b, g = tied_columns_frame()
    assert b.shape == (80, 6) and g.shape == (70, 24)
    cb = R3.box6_corners(b)
    x = int(np.flatnonzero((b[:, 0] == 30.0) & (b[:, 1] == -30.0))[0])
    assert KR.iou_pair(cb[x], g[3]) == KR.iou_pair(cb[x], g[67]) == (7.5 / 8.5, 15.0 / 17.0)
    swapped = g.copy()
    swapped[[3, 67]] = g[[67, 3]]
    want = [R3.recall_vectors_3d([b], [gg], (None,), None, "raise") for gg in (g, swapped)]
    for m in range(2):
        assert not np.array_equal(want[0][0][m], want[1][0][m])                  # the order of the two decides: the test cannot pass vacuously
        assert want[0][0][m, 0, 0] == want[1][0][m, 0, 0] == want[0][0][m].max() == 7.5 / 8.5
        assert sorted(set(want[0][0][m, 0]) ^ set(want[1][0][m, 0])) == [5.0 / 11.0, 6.0 / 10.0]
    for gg, w in zip((g, swapped), want):
        _, got = run(ops, torch_cuda, [b], [gg])
        assert same(got, w) and not got[2].any()


# ------------------------------------------------------------------ end to end
def small_net(torch):
    from mv3d_tf_amd.networks import get_network
    net = get_network("MV3D_test")
    with torch.no_grad():                                    # spread the RPN scores a little (random init is flat)
        net.params["rpn_cls_score"][0].mul_(40.0)
        net.params["rpn_bbox_pred"][0].mul_(5.0)
    return net


class SmallImdb3d:
    """four synthetic frames; the objects (boxes_bv for the selection, boxes_corners for the overlap) are set by the test once
    the proposals are known, so that some of them overlap"""
    name = "synthetic_4frames_3d"
    num_classes = 2
    image_index = ["000000", "000001", "000002", "000003"]
    objects = (3, 0, 2, 4)

    def __init__(self):
        r = np.random.RandomState(1)
        n = len(self.image_index)
        self.bvs = [(r.random_sample((64, 72, 9)) * (r.random_sample((64, 72, 9)) < 0.05)).astype(np.float32) for _ in range(n)]
        self.ims = [r.randint(0, 255, (48 if i != 2 else 56, 160, 3)).astype(np.float32) for i in range(n)]
        self.roidb = [dict(boxes_bv=np.tile(np.float32([10, 10, 49, 25]), (G, 1)), boxes_corners=np.zeros((G, 24), np.float32),
                           gt_classes=np.ones(G, np.int32), gt_overlaps=scipy.sparse.csr_matrix(np.tile(np.float32([0, 1]), (G, 1)).reshape(G, 2)))
                      for G in self.objects]

    def image_at(self, i): return self.ims[i]
    def bv_at(self, i): return self.bvs[i]
    def calib_at(self, i): return synth.KITTI_CALIB


@gpu
def test_imdb_proposals_with_3d_end_to_end(ops, torch_cuda, tmp_path):
    torch = torch_cuda
    from mv3d_tf_amd.datasets import proposal_recall_3d as P3
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.rpn_msr.generate import imdb_proposals
    net, imdb = small_net(torch), SmallImdb3d()
    saved, root = dict(cfg.TEST), cfg.ROOT_DIR
    cfg.ROOT_DIR = str(tmp_path)
    got = {}
    try:
        for bs in (1, 3):
            cfg.TEST.update(RPN_PRE_NMS_TOP_N=600, RPN_POST_NMS_TOP_N=50, BATCH_SIZE=bs)
            got[bs] = imdb_proposals(None, net, imdb, with_3d=True)
            assert net.fixed_rois is False and sorted(got[bs]) == ["3d", "bv", "image"]
        out_dir = os.path.join(str(tmp_path), "output", cfg.EXP_DIR, imdb.name)
        path, path3 = os.path.join(out_dir, "proposals.pkl"), os.path.join(out_dir, "proposals_3d.pkl")
        assert os.path.isfile(path) and os.path.isfile(path3)
        with open(path, "rb") as f:                          # proposals.pkl is what it was
            assert sorted(pickle.load(f)) == ["bv", "image"]
        for i in range(4):                                   # a direct forward of every frame: its rois[2] rows are the frame's 3D proposals
            with torch.no_grad():
                L = net.forward({"image_data": (imdb.ims[i][None].astype(np.float64) - cfg.PIXEL_MEANS).astype(np.float32),
                                 "lidar_bv_data": imdb.bvs[i][None], "im_info": np.array([[64, 72, 1]], np.float32),
                                 "calib": synth.KITTI_CALIB[None].astype(np.float32), "keep_prob": 1.0})
            direct = L["rois"][2].cpu().numpy()[:, 1:7]
            assert got[1]["3d"][i].dtype == np.float32 and got[1]["3d"][i].shape == direct.shape and len(direct) > 0
            assert np.array_equal(got[1]["3d"][i], direct) and np.array_equal(got[3]["3d"][i], direct), i
            assert len(got[3]["bv"][i]) == len(direct)
    finally:
        cfg.TEST.clear()
        cfg.TEST.update(saved)
        cfg.ROOT_DIR = root
    # objects: rotated, resized, shifted (by a share of their size) copies of some of each frame's proposals
    rng = np.random.RandomState(6)
    for i, G in enumerate(imdb.objects):
        p = got[3]["3d"][i][[(3 * j + 1) % len(got[3]["3d"][i]) for j in range(G)]].astype(np.float64)
        ang = rng.uniform(-0.3, 0.3, G)
        imdb.roidb[i]["boxes_corners"] = synth.box_corners(p[:, :3] - np.stack([0 * ang, 0 * ang, p[:, 5] / 2], 1) + rng.uniform(-0.05, 0.05, (G, 3)) * p[:, 3:6],
                                                           p[:, 3:6] * rng.uniform(0.9, 1.1, (G, 3)), np.stack([np.cos(ang), np.sin(ang)], 1))
    limits = [None, 1, 5, 20]
    res = P3.evaluate_recall_3d(imdb.roidb, got[3], thresholds=P3.CLI_THRESHOLDS, limit=limits, metric=("bev", "3d"), on_short="zero")
    gts = [e["boxes_corners"] for e in imdb.roidb]
    ov, counts, _ = R3.recall_vectors_3d(got[3]["3d"], gts, limits, P3.CLI_THRESHOLDS, "zero")
    keep = np.concatenate([np.full(len(g), len(b) > 0) for b, g in zip(got[3]["3d"], gts)])
    for mi, m in enumerate(R3.METRICS):
        for li in range(len(limits)):
            assert np.array_equal(res[m][li]["gt_overlaps"], np.sort(ov[mi, li][keep])) and np.array_equal(res[m][li]["recalls"], counts[mi, li] / 9.0)
            assert res[m][li]["ar"] == (counts[mi, li] / 9.0).mean()
    assert res["3d"][0]["recalls"][0] > 0 and (res["bev"][0]["gt_overlaps"] > 0.25).sum() >= 5
    # proposals_3d.pkl round-trips through the CLI's scoring function; its AR is over the ten reference thresholds only
    again = P3.score_pickle(imdb, path3, limits)
    for m in R3.METRICS:
        for a, b in zip(again[m], res[m]):
            assert np.array_equal(a["gt_overlaps"], b["gt_overlaps"]) and np.array_equal(a["recalls"], b["recalls"])
            assert a["ar"] == b["recalls"][1:].mean()
    from mv3d_tf_amd.datasets.proposal_recall import table
    assert table(again["3d"], limits, thresholds=(0.25, 0.5, 0.7)).splitlines()[0].split() == ["proposals", "recall@0.25", "recall@0.50", "recall@0.70", "AR"]
