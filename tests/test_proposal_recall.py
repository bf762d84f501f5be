"""Proposal recall on the device (mv3d_proposal_recall, ops.proposal_recall, datasets.proposal_recall.evaluate_recall,
rpn_msr.generate.imdb_proposals).  The fixtures tests/golden/recall_*.npz were produced by the reference's own imdb.evaluate_recall
(tests/golden/make_recall_golden.py); the checker of everything else is the plain-numpy restatement tests/recall_restatement.py
with the oracle's bbox_overlaps.  All comparisons are equalities: overlaps are f64 in a fixed order, counts are integers."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import scipy.sparse

import recall_restatement as RR
from conftest import golden
from mv3d_tf_amd import synth

gpu = pytest.mark.gpu

FIXTURES = ("recall_int_all", "recall_int_limit_below", "recall_int_limit_above", "recall_int_small", "recall_int_96_128",
            "recall_frac_thresholds", "recall_own_boxes", "recall_short_raises")


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


def load_case(name):
    """fixture -> (roidb, candidate boxes or None, keyword arguments of evaluate_recall, the fixture)"""
    z = golden(name)
    ro, co = z["roidb_off"], z["cand_off"]
    roidb = [dict(boxes=z["roidb_boxes"][ro[f]:ro[f + 1]], gt_classes=z["gt_classes"][ro[f]:ro[f + 1]],
                  gt_overlaps=scipy.sparse.csr_matrix(z["roidb_gt_overlaps"][ro[f]:ro[f + 1]]), seg_areas=z["seg_areas"][ro[f]:ro[f + 1]])
             for f in range(len(ro) - 1)]
    cands = [z["cand_boxes"][co[f]:co[f + 1]] for f in range(len(co) - 1)] if int(z["use_candidates"]) else None
    kw = dict(thresholds=z["thresholds_in"] if int(z["has_thresholds"]) else None, area=str(z["area"]),
              limit=None if int(z["limit"]) < 0 else int(z["limit"]))
    return roidb, cands, kw, z


def same_result(res, z):
    assert sorted(res) == ["ar", "gt_overlaps", "recalls", "thresholds"]
    assert np.array_equal(res["gt_overlaps"], z["gt_overlaps"]) and res["gt_overlaps"].dtype == np.float64
    assert np.array_equal(res["recalls"], z["recalls"]) and np.array_equal(res["thresholds"], z["thresholds"])
    assert res["ar"] == z["ar"]


def restated_launch(oracle, calls=None):
    """datasets.proposal_recall._launch with the restatement in the kernel's place"""
    def launch(boxes, gts, limits, thresholds, on_short):
        if calls is not None:
            calls.append(dict(boxes=boxes, gts=gts, limits=list(limits), thresholds=thresholds, on_short=on_short))
        ov, counts, status = RR.recall_vectors(boxes, gts, oracle.bbox_overlaps, limits, thresholds, on_short)
        if (status & 2).any():
            raise ValueError("non-finite")
        if (status & 1).any():
            raise AssertionError("short frame")
        return ov, counts
    return launch


# ------------------------------------------------------------------ without a GPU
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_the_reference(oracle, name):
    roidb, cands, kw, z = load_case(name)
    if int(z["raises_assertion"]):
        with pytest.raises(AssertionError):
            RR.evaluate_recall(roidb, oracle.bbox_overlaps, cands, **kw)
        return
    same_result(RR.evaluate_recall(roidb, oracle.bbox_overlaps, cands, **kw), z)
    # ... and the array-level contract holds the same numbers: sorted entries of the frames with boxes, counts = recalls * num_pos
    from mv3d_tf_amd.datasets import proposal_recall as PR
    gts, num_pos = PR.select_objects(roidb, kw["area"], "image")
    boxes = cands if cands is not None else [e["boxes"][e["gt_classes"] == 0] for e in roidb]
    ov, counts, status = RR.recall_vectors(boxes, gts, oracle.bbox_overlaps, [kw["limit"]], z["thresholds"])
    assert not status.any()
    assert np.array_equal(np.sort(ov[0][ov[0] >= 0]), z["gt_overlaps"])
    assert np.array_equal(counts[0] / float(num_pos), z["recalls"])


@pytest.mark.parametrize("name", FIXTURES)
def test_dataset_layer_without_a_device(oracle, monkeypatch, name):
    """object selection, areas, num_pos, thresholds and the dictionary: evaluate_recall with the restatement injected for the launch"""
    from mv3d_tf_amd.datasets import proposal_recall as PR
    roidb, cands, kw, z = load_case(name)
    calls = []
    monkeypatch.setattr(PR, "_launch", restated_launch(oracle, calls))
    if int(z["raises_assertion"]):
        with pytest.raises(AssertionError):
            PR.evaluate_recall(roidb, cands, space="image", **kw)
        res = PR.evaluate_recall(roidb, cands, space="image", on_short="zero", **kw)      # this repository's mode: misses, no raise
        assert (res["gt_overlaps"] == 0.0).any() and calls[-1]["on_short"] == "zero"
        return
    same_result(PR.evaluate_recall(roidb, cands, space="image", **kw), z)
    assert len(calls) == 1 and calls[0]["limits"] == [kw["limit"]] and calls[0]["thresholds"].dtype == np.float64
    if kw["thresholds"] is None:
        assert np.array_equal(calls[0]["thresholds"], np.arange(0.5, 0.95 + 1e-5, 0.05))
    # a sequence of limits: one dictionary per limit from ONE launch, each equal to the single-limit call
    many = PR.evaluate_recall(roidb, cands, space="image", **dict(kw, limit=[kw["limit"], 1000]))
    assert len(calls) == 2 and isinstance(many, list) and len(many) == 2
    same_result(many[0], z)


def test_object_selection_and_areas(oracle, monkeypatch):
    from mv3d_tf_amd.datasets import proposal_recall as PR
    assert PR.AREAS == RR.AREAS and PR.AREA_RANGES == RR.AREA_RANGES
    b = np.array([[0, 0, 31, 31], [0, 0, 31, 32], [10, 10, 105, 105], [0, 0, 127, 127], [0, 0, 9, 9], [5, 5, 20, 20]], np.float32)
    entry = dict(boxes=b, boxes_bv=b[::-1].copy(), gt_classes=np.array([1, 1, 1, 1, 0, 1], np.int32),
                 gt_overlaps=scipy.sparse.csr_matrix(np.array([[0, 1], [0, 1], [0, 1], [0, 1], [1, 0], [0, .5]], np.float32)))
    # no seg_areas: (x2 - x1 + 1) * (y2 - y1 + 1) of the selected space's box; the background row and the crowd row never count
    for area, want in (("all", [0, 1, 2, 3]), ("small", [0]), ("medium", [0, 1, 2]), ("large", [2, 3]), ("96-128", [2, 3]), ("128-256", [3]),
                       ("256-512", []), ("512-inf", [])):
        gts, num_pos = PR.select_objects([entry, entry], area, "image")
        assert num_pos == 2 * len(want) and np.array_equal(gts[0], b[want]) and np.array_equal(gts[1], b[want]), area
    gts, num_pos = PR.select_objects([entry], "all", "bv")
    assert np.array_equal(gts[0], b[::-1][[0, 1, 2, 3]])
    # seg_areas, where present, decide
    gts, num_pos = PR.select_objects([dict(entry, seg_areas=np.array([5000, 10, 10, 10, 10, 10], np.float32))], "small", "image")
    assert num_pos == 3 and np.array_equal(gts[0], b[[1, 2, 3]])
    with pytest.raises(AssertionError):
        PR.select_objects([entry], "huge", "image")
    # num_pos counts the objects of frames without boxes; candidate_boxes=None on a roidb without class-0 rows: nothing raises
    monkeypatch.setattr(PR, "_launch", restated_launch(oracle))
    only_gt = dict(entry, boxes=b[:4], boxes_bv=b[:4], gt_classes=entry["gt_classes"][:4], gt_overlaps=entry["gt_overlaps"][:4])
    res = PR.evaluate_recall([only_gt, only_gt], None, space="bv")
    assert res["gt_overlaps"].size == 0 and np.array_equal(res["recalls"], np.zeros(10)) and res["ar"] == 0.0
    res = PR.evaluate_recall([only_gt, only_gt], [b[:4], np.zeros((0, 4), np.float32)], space="bv")
    assert np.array_equal(res["gt_overlaps"], np.ones(4)) and np.array_equal(res["recalls"], np.full(10, 0.5))
    # the {'bv', 'image'} dictionary of imdb_proposals and rows with the batch column in front
    res5 = PR.evaluate_recall([only_gt, only_gt], {"bv": [np.hstack([np.zeros((4, 1), np.float32), b[:4]]), np.zeros((0, 5), np.float32)],
                                                    "image": None}, space="bv")
    assert np.array_equal(res5["gt_overlaps"], res["gt_overlaps"])
    with pytest.raises(ValueError):
        PR.evaluate_recall([only_gt], [b], space="3d")
    text = PR.table([res, res5], [10, None])
    assert text.splitlines()[0].split() == ["proposals", "recall@0.50", "recall@0.70", "AR"]
    assert text.splitlines()[1].split() == ["10", "0.5000", "0.5000", "0.5000"] and text.splitlines()[2].split()[0] == "all"


def test_kitti_mv3d_has_the_reference_signature():
    import inspect
    from mv3d_tf_amd.datasets.kitti_mv3d import kitti_mv3d
    from mv3d_tf_amd.datasets.proposal_recall import evaluate_recall
    p = inspect.signature(kitti_mv3d.evaluate_recall).parameters
    assert list(p) == ["self", "candidate_boxes", "thresholds", "area", "limit", "space"]
    assert [p[k].default for k in list(p)[1:]] == [None, None, "all", None, "bv"]
    q = inspect.signature(evaluate_recall).parameters
    assert list(q) == ["roidb", "candidate_boxes", "thresholds", "area", "limit", "space", "on_short"]
    assert [q[k].default for k in list(q)[2:]] == [None, "all", None, "bv", "raise"]


def test_argument_validation_before_any_device_call(hiplib):
    L = hiplib.lib()
    assert hiplib.RecallSplit is not None and "mv3d_proposal_recall" in hiplib.EXPORTS
    A = 4096                                                 # a non-NULL "pointer" (never dereferenced: refused before any HIP call)

    def call(box_off, gt_off, num_boxes=None, num_gts=None, ptrs=None, outs=(A, A, A), limits=1, thresholds=10, mode=0, split=True):
        bo, go = np.asarray(box_off, np.int32), np.asarray(gt_off, np.int32)
        p = [bo.ctypes.data, go.ctypes.data, A, A, A, A, A, A] if ptrs is None else ptrs
        s = hiplib.RecallSplit(len(bo) - 1, int(go[-1]) if num_gts is None else num_gts, limits, thresholds, mode, 0,
                               int(bo[-1]) if num_boxes is None else num_boxes, *p)
        return L.mv3d_proposal_recall(C.byref(s) if split else None, outs[0], outs[1], outs[2], None)

    good = ([0, 3, 3, 10], [0, 2, 4, 4])
    assert call(*good, split=False) == hiplib.ERR_INVALID_ARG
    for k in range(8):                                       # every pointer of the descriptor, one at a time
        bo, go = np.asarray(good[0], np.int32), np.asarray(good[1], np.int32)
        ptrs = [bo.ctypes.data, go.ctypes.data, A, A, A, A, A, A]
        ptrs[k] = None
        assert call(*good, ptrs=ptrs) == hiplib.ERR_INVALID_ARG, k
    for k in range(3):                                       # every output
        outs = [A, A, A]
        outs[k] = None
        assert call(*good, outs=outs) == hiplib.ERR_INVALID_ARG, k
    assert call([0, 3, 2, 10], good[1]) == hiplib.ERR_INVALID_ARG                    # non-monotone box offsets
    assert call(good[0], [0, 2, 1, 4]) == hiplib.ERR_INVALID_ARG                     # non-monotone object offsets
    assert call([1, 3, 3, 10], good[1]) == hiplib.ERR_INVALID_ARG and call([-1, 3, 3, 10], good[1]) == hiplib.ERR_INVALID_ARG
    assert call(good[0], [0, 2, 4, -4]) == hiplib.ERR_INVALID_ARG
    assert call(*good, num_boxes=11) == hiplib.ERR_INVALID_ARG and call(*good, num_gts=5) == hiplib.ERR_INVALID_ARG
    assert call([0, 3, 3, 10], [0, 2, 259, 259]) == hiplib.ERR_INVALID_ARG           # 257 objects in one frame
    assert call(*good, num_boxes=2 ** 31) == hiplib.ERR_INVALID_ARG                  # more than 2^31 - 1 boxes
    assert call(*good, limits=0) == hiplib.ERR_INVALID_ARG and call(*good, thresholds=-1) == hiplib.ERR_INVALID_ARG
    assert call(*good, mode=2) == hiplib.ERR_INVALID_ARG
    # the Python layer: limits, dtypes that do not convert exactly, shapes
    from mv3d_tf_amd import ops
    assert ops.recall_limits((None, 1, 300)).tolist() == [0, 1, 300]
    for bad in ((0,), (-3,), (1.5,), ()):
        with pytest.raises(ValueError):
            ops.recall_limits(bad)
    assert np.array_equal(ops.default_recall_thresholds(), np.arange(0.5, 0.95 + 1e-5, 0.05))
    assert ops._exact_f32(np.array([[1, 2, 3, 4]], np.uint16), "boxes").dtype == np.float32
    assert ops._exact_f32(np.array([[0.5, 2, np.nan, 4]], np.float64), "boxes").dtype == np.float32
    with pytest.raises(ValueError):
        ops._exact_f32(np.array([[0.1, 2, 3, 4]], np.float64), "boxes")
    with pytest.raises(ValueError):
        ops._exact_f32(np.array([[2 ** 24 + 1, 2, 3, 4]], np.int64), "boxes")
    with pytest.raises(ValueError):
        ops._recall_boxes(np.zeros((3, 6), np.float32), "boxes")


def test_cli_parses_its_options():
    from mv3d_tf_amd.datasets import proposal_recall as PR
    a = PR.parser().parse_args(["--kitti", "/data/kitti", "--proposals", "out/proposals.pkl"])
    assert (a.kitti, a.image_set, a.proposals, a.limits, a.space, a.area) == ("/data/kitti", "val", "out/proposals.pkl",
                                                                              [10, 50, 100, 300, 1000, 2000], "bv", "all")
    a = PR.parser().parse_args(["--kitti", "k", "--image-set", "train", "--proposals", "p.pkl", "--limits", "10,all,300", "--space", "image",
                                "--area", "96-128", "--on-short", "raise"])
    assert (a.image_set, a.limits, a.space, a.area, a.on_short) == ("train", [10, None, 300], "image", "96-128", "raise")
    for bad in (["--proposals", "p.pkl"], ["--kitti", "k", "--proposals", "p", "--space", "3d"], ["--kitti", "k", "--proposals", "p", "--area", "x"]):
        with pytest.raises(SystemExit):
            PR.parser().parse_args(bad)


# ------------------------------------------------------------------ on the device
def run(ops, torch, boxes, gts, limits=(None,), thresholds=None, on_short="raise", as_tensors=False, batch_column=False):
    """per-frame lists -> host (gt_overlaps, counts, status) of ONE launch, without the raising read-back"""
    box_off = np.concatenate([[0], np.cumsum([len(b) for b in boxes])])
    gt_off = np.concatenate([[0], np.cumsum([len(g) for g in gts])])
    allb = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for b in boxes] + [np.zeros((0, 4), np.float32)])
    allg = np.concatenate([np.asarray(g, np.float32).reshape(-1, 4) for g in gts] + [np.zeros((0, 4), np.float32)])
    if batch_column:
        allb = np.hstack([np.full((len(allb), 1), 7, np.float32), allb])
    if as_tensors:
        allb, allg = torch.as_tensor(allb).cuda(), torch.as_tensor(allg).cuda()
    sp = ops.RecallSplit(allb, box_off, allg, gt_off, torch.device("cuda", 0))
    out = ops.proposal_recall(sp, limits, thresholds, on_short)
    torch.cuda.synchronize()
    return out, tuple(t.cpu().numpy() for t in out)


@gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_the_reference(ops, torch_cuda, name):
    from mv3d_tf_amd.datasets import proposal_recall as PR
    roidb, cands, kw, z = load_case(name)
    if int(z["raises_assertion"]):
        with pytest.raises(AssertionError):
            PR.evaluate_recall(roidb, cands, space="image", **kw)
        return
    same_result(PR.evaluate_recall(roidb, cands, space="image", **kw), z)
    gts, num_pos = PR.select_objects(roidb, kw["area"], "image")
    boxes = cands if cands is not None else [e["boxes"][e["gt_classes"] == 0] for e in roidb]
    out, (ov, counts, status) = run(ops, torch_cuda, boxes, gts, [kw["limit"]], z["thresholds"])
    assert not status.any() and ov.dtype == np.float64 and counts.dtype == np.int32
    assert np.array_equal(np.sort(ov[0][ov[0] >= 0]), z["gt_overlaps"])
    assert np.array_equal(counts[0] / float(num_pos), z["recalls"])
    h = ops.proposal_recall_host(out)
    assert all(np.array_equal(a, b) for a, b in zip(h, (ov, counts, status)))


SWEEP_LIMITS = (None, 1, 10, 64, 300)
SWEEP_R = (0, 1, 63, 64, 65, 255, 256, 257, 513, 2000)
SWEEP_G = (0, 1, 3, 17, 256)


def sweep_frames(seed=5):
    """every (R, G) of the sweep as one frame: a third of the frames on integer coordinates, duplicated boxes and objects, boxes
    that are exact copies of objects"""
    rng = np.random.RandomState(seed)
    boxes, gts = [], []
    for k, (R, G) in enumerate((r, g) for r in SWEEP_R for g in SWEEP_G):
        xy = rng.uniform(0, 600, (R + G, 2))
        a = np.hstack([xy, xy + rng.uniform(3, 90, (R + G, 2))])
        if k % 3 == 0:
            a = np.floor(a)
        a = a.astype(np.float32)
        b, g = a[:R], a[R:]
        for j in range(0, min(R, G), 2):
            b[(7 * j) % R] = g[j] + (np.floor(rng.uniform(-4, 5, 4)) if j % 4 else np.zeros(4)).astype(np.float32)
        if R > 4:
            b[R - 1] = b[2]
            b[R // 2] = b[2]
        if G > 2:
            g[G - 1] = g[0]
        boxes.append(b); gts.append(g)
    return boxes, gts


@pytest.fixture(scope="module")
def sweep(oracle):
    boxes, gts = sweep_frames()
    zero = RR.recall_vectors(boxes, gts, oracle.bbox_overlaps, SWEEP_LIMITS, None, "zero")
    for a in zero:
        a.setflags(write=False)
    return boxes, gts, zero


@gpu
def test_sweep_equals_restatement(ops, torch_cuda, sweep):
    boxes, gts, (ov0, counts0, status0) = sweep
    _, (ov, counts, status) = run(ops, torch_cuda, boxes, gts, SWEEP_LIMITS, None, "zero")
    assert np.array_equal(ov, ov0) and np.array_equal(counts, counts0) and np.array_equal(status, status0)
    assert not status.any() and counts.max() > 0 and (ov == 1.0).any() and (ov == -1.0).any() and (ov == 0.0).any()
    # device tensors in, the batch column in front: the same
    _, (ov5, counts5, status5) = run(ops, torch_cuda, boxes, gts, SWEEP_LIMITS, None, "zero", as_tensors=True, batch_column=True)
    assert np.array_equal(ov5, ov) and np.array_equal(counts5, counts) and np.array_equal(status5, status)
    _, (ov4, counts4, _) = run(ops, torch_cuda, boxes, gts, SWEEP_LIMITS, None, "zero", batch_column=True)
    assert np.array_equal(ov4, ov) and np.array_equal(counts4, counts)
    # several limits in one launch == that many single-limit launches
    for li, lim in enumerate(SWEEP_LIMITS):
        _, (ov1, counts1, _) = run(ops, torch_cuda, boxes, gts, (lim,), None, "zero")
        assert np.array_equal(ov1[0], ov[li]) and np.array_equal(counts1[0], counts[li]), lim


@gpu
def test_short_frames_raise_or_count_as_misses(ops, torch_cuda, oracle, sweep):
    boxes, gts, (ov0, _, _) = sweep
    want = RR.recall_vectors(boxes, gts, oracle.bbox_overlaps, SWEEP_LIMITS, None, "raise")
    out, (ov, counts, status) = run(ops, torch_cuda, boxes, gts, SWEEP_LIMITS, None, "raise")
    assert np.array_equal(ov, want[0]) and np.array_equal(counts, want[1]) and np.array_equal(status, want[2])
    assert (status & 1).any() and not (status & 2).any()
    short = (ov != ov0)
    assert short.any() and (ov[short] == -1.0).all() and (ov0[short] == 0.0).all()      # 'zero' records 0.0 exactly where 'raise' has -1.0
    with pytest.raises(AssertionError):
        ops.proposal_recall_host(out)


@gpu
def test_non_finite_coordinate_flags_its_frame_only(ops, torch_cuda, oracle):
    rng = np.random.RandomState(9)
    boxes = [synth_boxes(rng, 40) for _ in range(5)]
    gts = [synth_boxes(rng, 4) for _ in range(5)]
    boxes[1][30, 2] = np.nan                                 # behind limit 10: the frame is flagged for every limit
    gts[3][1, 0] = np.inf
    want = RR.recall_vectors(boxes, gts, oracle.bbox_overlaps, (None, 10), None, "raise")
    out, (ov, counts, status) = run(ops, torch_cuda, boxes, gts, (None, 10))
    assert status.tolist() == [0, 2, 0, 2, 0] and np.array_equal(status, want[2])
    assert np.array_equal(ov, want[0]) and np.array_equal(counts, want[1])
    assert (ov[:, 4:8] == 0.0).all() and (ov[:, 12:16] == 0.0).all() and (ov[:, :4] >= 0).all()
    with pytest.raises(ValueError):
        ops.proposal_recall_host(out)


def synth_boxes(rng, n):
    xy = np.floor(rng.uniform(0, 200, (n, 2)))
    return np.hstack([xy, xy + np.floor(rng.uniform(5, 80, (n, 2)))]).astype(np.float32)


@gpu
def test_frame_with_more_boxes_than_the_used_bit_mask(ops, torch_cuda, oracle):
    """more boxes than are staged in LDS (2048) and than the used-box bits cover (16384): the matches of this frame sit behind both"""
    rng = np.random.RandomState(13)
    R, G = 16384 + 700, 5
    b = synth_boxes(rng, R)
    b[:, :2] += 1000; b[:, 2:] += 1000                       # far from the objects ...
    g = synth_boxes(rng, G)
    g[4] = g[3]
    b[16384 + 100:16384 + 110] = g[3]                        # ... except a run of copies of the duplicated object behind the mask
    b[16384 + 300] = g[0]; b[5000] = g[1] + np.float32([1, 0, 0, 2]); b[3] = g[2] + np.float32([0, 3, 0, 0])
    boxes, gts = [b, synth_boxes(rng, 3000)], [g, synth_boxes(rng, 7)]
    want = RR.recall_vectors(boxes, gts, oracle.bbox_overlaps, (None, 16384, 2049), None, "raise")
    _, (ov, counts, status) = run(ops, torch_cuda, boxes, gts, (None, 16384, 2049))
    assert np.array_equal(ov, want[0]) and np.array_equal(counts, want[1]) and not status.any()
    assert (ov[0, :5] == 1.0).sum() == 3 and (ov[1, :5] == 1.0).sum() == 0


def tied_columns_frame():
    """one frame, 70 objects x 80 boxes, integer coordinates: objects 3 and 67 (another wave of the round reduction) share their
    best box X with exactly the same overlap, 9500 / 10500, the largest of the frame; their second-best boxes differ clearly.
    Every other object has one box of its own with an overlap of its own, 97 (100 - dx) / (20000 - 97 (100 - dx)) < 0.64, which
    no value of the two tied objects equals (those are multiples of 100 over multiples of 100)."""
    sq = lambda x, y: [x, y, x + 99, y + 99]
    gts, boxes = [], []
    for k in range(70):
        x, y = 300 * (k % 10), 300 * (k // 10)
        gts.append(sq(x, y))
        if k not in (3, 67):
            boxes.append(sq(x + 20 + k, y + 3))
    x, y = 900, 0                                            # the slot of object 3; object 67 moves next to it
    gts[3], gts[67] = sq(x - 5, y), sq(x + 5, y)
    boxes += [sq(x, y), sq(x - 35, y), sq(x + 55, y)]        # X; 7000 / 13000 with object 3, 6000 / 14000 with 67; 5000 / 15000 with 67
    boxes += [sq(5000 + 150 * i, 5000) for i in range(9)]    # far from everything
    b = np.float32(boxes)[np.random.RandomState(3).permutation(80)]
    return b, np.float32(gts)


@gpu
def test_tied_columns_across_waves_take_the_first(ops, torch_cuda, oracle):
    """the first-index tie-break of the round reduction across waves: whichever of the two tied objects stands at index 3 takes
    the shared box, and the one at index 67 is left with its own second best, which differs between the two"""
    b, g = tied_columns_frame()
    assert b.shape == (80, 4) and g.shape == (70, 4)
    o = oracle.bbox_overlaps(b.astype(np.float64), g.astype(np.float64))
    x = int(o[:, 3].argmax())
    assert o[x, 3] == o[x, 67] == o.max() == 9500.0 / 10500.0 and int(o[:, 67].argmax()) == x and (o == o.max()).sum() == 2
    swapped = g.copy()
    swapped[[3, 67]] = g[[67, 3]]
    want = [RR.recall_vectors([b], [gg], oracle.bbox_overlaps, (None,), None, "raise") for gg in (g, swapped)]
    assert not np.array_equal(want[0][0], want[1][0])        # the order of the two decides: the test cannot pass vacuously
    assert want[0][0][0, 0] == want[1][0][0, 0] == o.max()
    assert sorted(set(want[0][0][0]) ^ set(want[1][0][0])) == [6000.0 / 14000.0, 7000.0 / 13000.0]
    for gg, w in zip((g, swapped), want):
        _, (ov, counts, status) = run(ops, torch_cuda, [b], [gg])
        assert np.array_equal(ov, w[0]) and np.array_equal(counts, w[1]) and np.array_equal(status, w[2]) and not status.any()


# ------------------------------------------------------------------ end to end
def small_net(torch):
    from mv3d_tf_amd.networks import get_network
    net = get_network("MV3D_test")
    with torch.no_grad():                                    # spread the RPN scores a little (random init is flat)
        net.params["rpn_cls_score"][0].mul_(40.0)
        net.params["rpn_bbox_pred"][0].mul_(5.0)
    return net


class SmallImdb:
    name = "synthetic_4frames"
    num_classes = 2
    image_index = ["000000", "000001", "000002", "000003"]

    def __init__(self):
        r = np.random.RandomState(1)
        n = len(self.image_index)
        self.bvs = [(r.random_sample((64, 72, 9)) * (r.random_sample((64, 72, 9)) < 0.05)).astype(np.float32) for _ in range(n)]
        self.ims = [r.randint(0, 255, (48 if i != 2 else 56, 160, 3)).astype(np.float32) for i in range(n)]
        self.roidb = []
        for i in range(n):
            G = (3, 0, 2, 4)[i]
            bv, im = synth_boxes(r, G) * np.float32(0.3), synth_boxes(r, G) * np.float32(0.5)
            self.roidb.append(dict(boxes=im, boxes_bv=bv, gt_classes=np.ones(G, np.int32),
                                   gt_overlaps=scipy.sparse.csr_matrix(np.tile(np.float32([0, 1]), (G, 1)).reshape(G, 2))))

    def image_at(self, i): return self.ims[i]
    def bv_at(self, i): return self.bvs[i]
    def calib_at(self, i): return synth.KITTI_CALIB


@gpu
def test_imdb_proposals_end_to_end(ops, torch_cuda, oracle, tmp_path):
    torch = torch_cuda
    from mv3d_tf_amd.datasets import proposal_recall as PR
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.rpn_msr.generate import imdb_proposals
    net, imdb = small_net(torch), SmallImdb()
    saved, root = dict(cfg.TEST), cfg.ROOT_DIR
    cfg.ROOT_DIR = str(tmp_path)
    got = {}
    try:
        for bs in (1, 3):
            cfg.TEST.update(RPN_PRE_NMS_TOP_N=600, RPN_POST_NMS_TOP_N=50, BATCH_SIZE=bs)
            got[bs] = imdb_proposals(None, net, imdb)
            assert net.fixed_rois is False
        path = os.path.join(str(tmp_path), "output", cfg.EXP_DIR, imdb.name, "proposals.pkl")
        assert os.path.isfile(path)
        # a direct forward of every frame: its first num_rois rows are the frame's proposals
        for i in range(4):
            with torch.no_grad():
                L = net.forward({"image_data": (imdb.ims[i][None].astype(np.float64) - cfg.PIXEL_MEANS).astype(np.float32),
                                 "lidar_bv_data": imdb.bvs[i][None], "im_info": np.array([[64, 72, 1]], np.float32),
                                 "calib": synth.KITTI_CALIB[None].astype(np.float32), "keep_prob": 1.0})
            for s, key in enumerate(("bv", "image")):
                direct = L["rois"][s].cpu().numpy()[:, 1:5]
                assert got[1][key][i].dtype == np.float32 and got[1][key][i].shape == direct.shape and len(direct) > 0
                assert np.array_equal(got[1][key][i], direct), (i, key)
                assert np.array_equal(got[3][key][i], got[1][key][i]), (i, key)      # the same per frame for both batch sizes
    finally:
        cfg.TEST.clear()
        cfg.TEST.update(saved)
        cfg.ROOT_DIR = root
    limits = [None, 1, 5, 20]
    for space, key in (("bv", "boxes_bv"), ("image", "boxes")):
        res = PR.evaluate_recall(imdb.roidb, got[3], limit=limits, space=space, on_short="zero")
        gts = [e[key] for e in imdb.roidb]
        ov, counts, _ = RR.recall_vectors(got[3][space], gts, oracle.bbox_overlaps, limits, None, "zero")
        keep = np.concatenate([np.full(len(g), len(b) > 0) for b, g in zip(got[3][space], gts)])
        for li in range(len(limits)):
            assert np.array_equal(res[li]["gt_overlaps"], np.sort(ov[li][keep])) and np.array_equal(res[li]["recalls"], counts[li] / 9.0)
            assert res[li]["ar"] == (counts[li] / 9.0).mean()
        with open(path, "rb") as f:                          # proposals.pkl round-trips through the CLI's scoring function
            assert sorted(pickle.load(f)) == ["bv", "image"]
        again = PR.score_pickle(imdb, path, limits, space=space)
        assert all(np.array_equal(a["gt_overlaps"], b["gt_overlaps"]) and np.array_equal(a["recalls"], b["recalls"]) for a, b in zip(again, res))
    assert "recall@0.50" in PR.table(res, limits)
