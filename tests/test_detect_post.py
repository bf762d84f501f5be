"""mv3d_detect_post: the per-frame tail of test_net (score cut at 0.05, greedy NMS of the class's BEV boxes, cap of max_per_image over
all classes; lib/fast_rcnn/test_mv.py:420-444, 491-501) for a batch of frames on the device.  The checker of every GPU test is
oracle.test_net_frame fed with the arrays the device call was given; all comparisons are np.array_equal on the rows in front of
det_count.  The no-GPU tests cover what never touches a device: argument validation, the workspace query, the frame grouping of the
batched test_net and the new config key."""
import ctypes as C
import os

import numpy as np
import pytest

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


# ------------------------------------------------------------------ without a GPU
def test_argument_validation_and_workspace_query(hiplib):
    L = hiplib.lib()
    P = hiplib.DetectPostParams
    A = 4096                                                 # a non-NULL "pointer" (never dereferenced: refused before any HIP call)
    good = P(2, 300, 300, 0, 0.05, 0, 0.1)

    def call(batch, p, ptrs=None):
        a = [A] * 12 if ptrs is None else ptrs               # cls_prob, pred_bv, corners, pred_cnr_r, num_rois | det_bv, det_cnr, det_cnr_r, det_row, det_count, status
        return L.mv3d_detect_post(a[0], a[1], a[2], a[3], a[4], batch, None if p is None else C.byref(p), a[5], a[6], a[7], a[8], a[9],
                                  a[10], None, 0, None)

    assert call(1, P(2, 2049, 300, 0, 0.05, 0, 0.1)) == hiplib.ERR_INVALID_ARG       # rows_per_frame above 2048
    assert call(1, P(2, 0, 300, 0, 0.05, 0, 0.1)) == hiplib.ERR_INVALID_ARG
    assert call(1, P(1, 300, 300, 0, 0.05, 0, 0.1)) == hiplib.ERR_INVALID_ARG        # no foreground class
    assert call(1, P(9, 300, 300, 0, 0.05, 0, 0.1)) == hiplib.ERR_INVALID_ARG
    assert call(0, good) == hiplib.ERR_INVALID_ARG and call(-3, good) == hiplib.ERR_INVALID_ARG
    assert call(1, None) == hiplib.ERR_INVALID_ARG
    for required in (0, 1, 2, 5, 6, 8, 9, 10):                                      # every required pointer, one at a time
        ptrs = [A] * 12
        ptrs[required] = None
        assert call(1, good, ptrs) == hiplib.ERR_INVALID_ARG, required
    ptrs = [A] * 12
    ptrs[7] = None                                                                   # pred_cnr_r given, det_cnr_r missing
    assert call(1, good, ptrs) == hiplib.ERR_INVALID_ARG
    # no global scratch: everything lives in LDS and in the outputs
    assert L.mv3d_detect_post_workspace_bytes(16, C.byref(good)) == 0
    assert L.mv3d_detect_post_workspace_bytes(4, C.byref(P(8, 2048, 0, 1, 0.05, 0, 0.5))) == 0


def test_frame_grouping():
    from mv3d_tf_amd.fast_rcnn.detect_batch import group_frames, iter_frame_groups
    a, b = ((375, 1242, 3), (608, 608, 9)), ((370, 1224, 3), (608, 608, 9))
    assert group_frames([a, a, b], 2) == [[0, 1], [2]]
    assert group_frames([a] * 5, 2) == [[0, 1], [2, 3], [4]]
    assert group_frames([a, b, a, a, a, a, b, b], 3) == [[0], [1], [2, 3, 4], [5], [6, 7]]      # never reordered, never padded
    assert group_frames([], 4) == [] and group_frames([a], 4) == [[0]]
    assert group_frames([a, a, a], 1) == [[0], [1], [2]]
    seen = []

    def keys():                                              # lazy: a group is handed out before the frames behind the next one's first are loaded
        for i, k in enumerate([a, a, a, b]):
            seen.append(i)
            yield k

    it = iter_frame_groups(keys(), 2)
    assert next(it) == [0, 1] and seen == [0, 1, 2]


def test_batch_size_key_defaults_to_one(monkeypatch):
    from mv3d_tf_amd.fast_rcnn import detect_batch, test_mv
    from mv3d_tf_amd.fast_rcnn.config import cfg
    assert cfg.TEST.BATCH_SIZE == 1 and type(cfg.TEST.BATCH_SIZE) is int
    # ... and with 1 the batched entry point IS the frame-by-frame loop: it hands its arguments to test_mv.test_net
    monkeypatch.setattr(test_mv, "test_net", lambda *a, **k: ("frame by frame", a, k))
    assert detect_batch.test_net(None, "net", "imdb", "w", max_per_image=7) == \
        ("frame by frame", (None, "net", "imdb", "w"), dict(max_per_image=7, thresh=0.05, vis=False))


# ------------------------------------------------------------------ on the device
def dev(t, torch, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(t), dtype=dtype).cuda()


def make_batch(rng, K, rows, B, quant=None):
    """the generator of test_test_net_postprocessing_and_loop for B frames of `rows` rows; quant: scores in steps of 1 / quant"""
    R = B * rows
    scores = rng.random_sample((R, K)).astype(np.float32) ** 3
    if quant:
        scores = (np.floor(scores * quant) / quant).astype(np.float32)
    scores[:, 0] = 1 - scores[:, 1:].max(1)
    ctr = rng.uniform(20, 580, (R, 1, 2)); wh = rng.uniform(8, 40, (R, K, 2))
    bx = np.concatenate([ctr - wh / 2, ctr + wh / 2], 2).reshape(R, 4 * K).astype(np.float32)
    cnr = rng.uniform(-30, 60, (R, 24)).astype(np.float32)
    cnr_r = (np.hstack([cnr] * K) + rng.uniform(-1, 1, (R, 24 * K))).astype(np.float32)
    return scores, bx, cnr, cnr_r


def gpu_rule_frame(oracle, scores, boxes_bv, boxes_cnr, K, nms_thresh, max_per_image):
    """oracle.test_net_frame with the NMS replaced by the `_nms` rule (oracle.gpu_nms_rule on the boxes in the library's processing
    order: descending score, ties by descending index).  Parity unpinned, as for `_nms` itself."""
    dets, dets_cnr = [[]], [[]]
    for j in range(1, K):
        inds = np.where(scores[:, j] > 0.05)[0]
        s = scores[inds, j]
        d = np.hstack((boxes_bv[inds, 4 * j:4 * j + 4], s[:, None])).astype(np.float32)
        c = np.hstack((boxes_cnr[inds, 24 * j:24 * j + 24], s[:, None])).astype(np.float32)
        order = np.lexsort((-np.arange(len(s)), -s))
        keep = order[oracle.gpu_nms_rule(d[order], nms_thresh)] if len(s) else []
        dets.append(d[keep, :]); dets_cnr.append(c[keep, :])
    if max_per_image > 0:
        image_scores = np.hstack([dets[j][:, -1] for j in range(1, K)])
        if len(image_scores) > max_per_image:
            t = np.sort(image_scores)[-max_per_image]
            for j in range(1, K):
                k = np.where(dets[j][:, -1] >= t)[0]
                dets[j], dets_cnr[j] = dets[j][k, :], dets_cnr[j][k, :]
    return dets, dets_cnr


def frame_inputs(arrays, f, rows, n, K):
    scores, bx, cnr, cnr_r = arrays
    sl = slice(f * rows, f * rows + n)
    return scores[sl], bx[sl].astype(np.float64), np.hstack([cnr[sl]] * K), cnr_r[sl]


def compare(oracle, got, arrays, num, K, rows, mpi, nms_thresh, zero_frames=(), gpu_rule=False, equal_nan=False):
    """got: host copies of detect_post's outputs; every frame against the oracle's tail of the same arrays.  Returns the kept totals."""
    bv, cnr, cnr_r, row, cnt, st = got
    B = cnt.shape[0]
    eq = lambda a, b: np.array_equal(a, b, equal_nan=equal_nan)
    totals = []
    for f in range(B):
        n = rows if num is None else int(num[f])
        sc, bxf, cn, cr = frame_inputs(arrays, f, rows, n, K)
        if f in zero_frames:
            with pytest.raises(ZeroDivisionError):
                oracle.test_net_frame(sc, bxf, cn, cr, K, nms_thresh, mpi)
            assert st[f] & 1, f
            totals.append(None)
            continue
        if gpu_rule:
            o_dets, o_cnr = gpu_rule_frame(oracle, sc, bxf, cn, K, nms_thresh, mpi)
        else:
            o_dets, o_cnr = oracle.test_net_frame(sc, bxf, cn, cr, K, nms_thresh, mpi)
        assert st[f] == 0 and cnt[f, 0] == 0, f
        for j in range(1, K):
            c = int(cnt[f, j])
            assert c == len(o_dets[j]), (f, j, c, len(o_dets[j]))
            assert eq(bv[f, j, :c], o_dets[j]) and eq(cnr[f, j, :c], o_cnr[j]), (f, j)
            r = row[f, j, :c]                                 # det_row points at the rows the oracle kept
            assert r.min(initial=0) >= 0 and r.max(initial=0) < max(n, 1)
            assert eq(sc[r, j], o_dets[j][:, 4]) and eq(bxf[r, 4 * j:4 * j + 4].astype(np.float32), o_dets[j][:, :4]), (f, j)
            if cnr_r is not None:
                assert eq(cnr_r[f, j, :c, :24], cr[r, 24 * j:24 * j + 24]) and eq(cnr_r[f, j, :c, 24], sc[r, j]), (f, j)
        totals.append(sum(int(cnt[f, j]) for j in range(1, K)))
    return totals


def run(ops, torch, arrays, num, K, rows, mpi, nms_thresh, use_gpu_nms=False, with_r=True):
    scores, bx, cnr, cnr_r = arrays
    out = ops.detect_post(dev(scores, torch), dev(bx, torch), dev(cnr, torch), dev(cnr_r, torch) if with_r else None,
                          None if num is None else dev(np.asarray(num, np.int32), torch), rows, K, mpi, nms_thresh, use_gpu_nms=use_gpu_nms)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


SWEEP = ((2, 300, 300, 16), (2, 300, 40, 16), (2, 2000, 300, 4), (4, 200, 25, 3), (3, 60, 0, 2), (2, 2048, 0, 1), (8, 130, 50, 2), (2, 1, 5, 3))


@gpu
@pytest.mark.parametrize("K,rows,mpi,B", SWEEP)
def test_synthetic_sweep_equals_oracle(ops, torch_cuda, oracle, K, rows, mpi, B):
    rng = np.random.RandomState(1000 + 7 * rows + K + mpi)
    for nms_thresh in (0.1, 0.5):
        arrays = make_batch(rng, K, rows, B)
        got = run(ops, torch_cuda, arrays, None, K, rows, mpi, nms_thresh)
        totals = compare(oracle, got, arrays, None, K, rows, mpi, nms_thresh)
        if mpi > 0:                                          # (tie-free scores: the cap is exact)
            assert max(totals) <= mpi
        assert max(totals) > 0
    # without the regressed corners: the same detections, det_cnr_r not touched
    got = run(ops, torch_cuda, arrays, None, K, rows, mpi, 0.5, with_r=False)
    assert got[2] is None
    compare(oracle, got, arrays, None, K, rows, mpi, 0.5)


@gpu
def test_ragged_num_rois(ops, torch_cuda, oracle):
    """frames with fewer rows than the capacity (one with none), a frame with no score above the cut, counts above the capacity and
    below zero: rows at or behind a frame's count are never candidates"""
    rng = np.random.RandomState(11)
    for K, rows, mpi in ((2, 300, 40), (3, 700, 100)):
        B = 6
        arrays = make_batch(rng, K, rows, B)
        arrays[0][3 * rows:4 * rows, 1:] *= 0.04             # frame 3: nothing above 0.05
        num = [rows, 0, 1, rows, rows // 2 + 3, 65]
        got = run(ops, torch_cuda, arrays, num, K, rows, mpi, 0.1)
        totals = compare(oracle, got, arrays, num, K, rows, mpi, 0.1)
        assert totals[1] == 0 and totals[3] == 0 and totals[0] > 0 and totals[4] > 0
        wild = [rows + 500, -4, 1, rows, rows // 2 + 3, 65]  # clamped to [0, rows]
        got = run(ops, torch_cuda, arrays, wild, K, rows, mpi, 0.1)
        compare(oracle, got, arrays, num, K, rows, mpi, 0.1)


@gpu
def test_ties_in_sort_and_cap(ops, torch_cuda, oracle):
    """scores in steps of 1/64 and 1/16: the sort's tie rule (descending row index) and the cap's `>=` (ties keep more than
    max_per_image) decide; exactly duplicated boxes"""
    rng = np.random.RandomState(21)
    for K, rows, mpi, B, quant in ((2, 2000, 300, 2, 64), (4, 200, 25, 3, 16), (2, 300, 40, 4, 16), (3, 512, 64, 2, 64)):
        arrays = make_batch(rng, K, rows, B, quant=quant)
        arrays[1][5:40] = arrays[1][4]                       # duplicates: the first processed suppresses the others
        arrays[1][rows - 3:rows] = arrays[1][rows - 4]
        got = run(ops, torch_cuda, arrays, None, K, rows, mpi, 0.1)
        totals = compare(oracle, got, arrays, None, K, rows, mpi, 0.1)
        assert max(totals) > mpi, (K, rows, totals)          # the `>=` rule kept tied scores beyond the cap


@gpu
def test_nan_inf_scores_and_wild_boxes(ops, torch_cuda, oracle):
    rng = np.random.RandomState(31)
    K, rows, B = 3, 300, 3
    arrays = make_batch(rng, K, rows, B)
    scores, bx = arrays[0], arrays[1]
    scores[3, 1] = scores[rows + 9, 2] = np.nan              # dropped by the cut
    scores[7, 1] = scores[8, 1] = scores[2 * rows + 1, 2] = np.inf
    scores[20, 2] = -np.inf
    bx[7, 4:8] = [np.nan, 30, 60, 70]                        # a kept box with a NaN coordinate
    bx[40, 4] = np.nan
    bx[41, 4:8] = [-1e30, -1e30, 1e30, 1e30]
    bx[rows + 2, 8:12] = [1e30, 1e30, 1e30, 1e30]
    sc = np.where(np.isnan(scores), 0, scores)
    scores[:, 0] = 1 - np.clip(sc[:, 1:], 0, 1).max(1)
    for mpi in (0, 50):
        got = run(ops, torch_cuda, arrays, None, K, rows, mpi, 0.1)
        compare(oracle, got, arrays, None, K, rows, mpi, 0.1, equal_nan=True)


def zero_union_batch(rng, K=2, rows=60, B=3, frame=1):
    arrays = make_batch(rng, K, rows, B)
    arrays[0][frame * rows + 10, 1], arrays[0][frame * rows + 30, 1] = 0.9, 0.8
    arrays[1][frame * rows + 10, 4:8] = arrays[1][frame * rows + 30, 4:8] = [5, 5, 4, 4]
    return arrays


@gpu
def test_zero_union_flags_its_frame_only(ops, torch_cuda, oracle):
    arrays = zero_union_batch(np.random.RandomState(41))
    got = run(ops, torch_cuda, arrays, None, 2, 60, 20, 0.1)
    assert got[5].tolist() == [0, 1, 0]
    compare(oracle, got, arrays, None, 2, 60, 20, 0.1, zero_frames=(1,))
    out = ops.detect_post(*(dev(a, torch_cuda) for a in arrays), None, 60, 2, 20, 0.1)
    with pytest.raises(ZeroDivisionError):
        ops.detect_post_lists(out)


@gpu
def test_gpu_nms_rule(ops, torch_cuda, oracle):
    """use_gpu_nms=True = the same tail on the `_nms` rule (IoU > thresh in f32).  Parity unpinned, as for `_nms`: the checker is the
    restatement oracle.gpu_nms_rule.  Two isolated pairs per frame have an IoU of exactly 0.5 / 0.25, where the two rules differ."""
    rng = np.random.RandomState(51)
    differs = 0
    for K, rows, mpi, B in ((2, 300, 300, 4), (4, 200, 25, 3)):
        arrays = make_batch(rng, K, rows, B)
        for f in range(B):
            r = f * rows
            arrays[0][r:r + 4, 1] = [0.95, 0.9, 0.85, 0.8]
            arrays[1][r:r + 4, 4:8] = [[1000, 1000, 1009, 1009], [1000, 1000, 1009, 1004],       # 50 / 100
                                       [2000, 2000, 2009, 2009], [2000, 2000, 2004, 2004]]       # 25 / 100
        for thresh in (0.5, 0.25):
            got = run(ops, torch_cuda, arrays, None, K, rows, mpi, thresh, use_gpu_nms=True)
            compare(oracle, got, arrays, None, K, rows, mpi, thresh, gpu_rule=True)
            differs += int(not np.array_equal(got[4], run(ops, torch_cuda, arrays, None, K, rows, mpi, thresh)[4]))
    assert differs >= 2


@gpu
def test_captured_in_a_graph(ops, torch_cuda, oracle):
    """kernel launches only: the call sits in a captured graph; two replays on changed inputs equal the eager call and the oracle"""
    torch = torch_cuda
    K, rows, B, mpi = 3, 300, 4, 60
    rng = np.random.RandomState(61)
    first = make_batch(rng, K, rows, B)
    num0 = np.array([rows, 120, rows, 7], np.int32)
    static = [dev(a, torch) for a in first] + [dev(num0, torch)]
    out = ops.detect_post_outputs(B, K, rows, static[0].device)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.detect_post(*static, rows, K, mpi, 0.1, out=out)
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        ops.detect_post(*static, rows, K, mpi, 0.1, out=out)
    for seed, num in ((62, [rows, rows, 0, 200]), (63, [5, rows, 299, 64])):
        arrays = zero_union_batch(np.random.RandomState(seed), K, rows, B, frame=2) if seed == 63 else make_batch(np.random.RandomState(seed), K, rows, B)
        with torch.cuda.stream(stream):
            for s, a in zip(static, list(arrays) + [np.asarray(num, np.int32)]):
                s.copy_(torch.as_tensor(a), non_blocking=False)
            g.replay()
        stream.synchronize()
        got = tuple(t.cpu().numpy() for t in out)
        eager = run(ops, torch, arrays, num, K, rows, mpi, 0.1)
        zero = (2,) if seed == 63 else ()
        assert np.array_equal(got[4], eager[4]) and np.array_equal(got[5], eager[5])
        assert got[5].tolist() == [1 if f in zero else 0 for f in range(B)]      # the status word is cleared inside the graph
        for f in range(B):
            for j in range(1, K):
                c = int(got[4][f, j])
                for a, b in zip(got[:4], eager[:4]):
                    assert np.array_equal(a[f, j, :c], b[f, j, :c])
        compare(oracle, got, arrays, num, K, rows, mpi, 0.1, zero_frames=zero)


def small_net(torch):
    from mv3d_tf_amd.networks import get_network
    net = get_network("MV3D_test")
    with torch.no_grad():                                    # spread the RPN scores a little (random init is flat)
        net.params["rpn_cls_score"][0].mul_(40.0)
        net.params["rpn_bbox_pred"][0].mul_(5.0)
    return net


def small_feed(seed, B, torch):
    from mv3d_tf_amd.fast_rcnn.config import cfg
    r = np.random.RandomState(seed)
    bv = (r.random_sample((B, 64, 72, 9)) * (r.random_sample((B, 64, 72, 9)) < 0.05)).astype(np.float32)
    im = (r.randint(0, 255, (B, 48, 160, 3)) - cfg.PIXEL_MEANS).astype(np.float32)
    return {"lidar_bv_data": torch.as_tensor(bv).cuda(), "image_data": torch.as_tensor(im).cuda(),
            "im_info": np.array([[64, 72, 1]] * B, np.float32), "calib": np.stack([synth.KITTI_CALIB] * B), "keep_prob": 1.0}


@gpu
def test_serve_graph_ends_in_final_detections(ops, torch_cuda, oracle, monkeypatch):
    """ServeGraph(..., post=...): final_detections() == the oracle's tail of what detections() returns from the same replay;
    post=None stays the graph it was; a zero union raises"""
    torch = torch_cuda
    from mv3d_tf_amd.fast_rcnn import detect_batch, test_mv
    from mv3d_tf_amd.fast_rcnn.config import cfg
    B, mpi = 3, 10
    saved = dict(cfg.TEST)
    cfg.TEST.update(RPN_PRE_NMS_TOP_N=600, RPN_POST_NMS_TOP_N=50)
    try:
        net = small_net(torch)
        sg = detect_batch.ServeGraph(net, small_feed(1, B, torch), post=dict(max_per_image=mpi))
        kept = 0
        for seed in (1, 2):
            sg.replay(small_feed(seed, B, torch))
            final = sg.final_detections()
            frames = sg.detections()
            assert len(final) == len(frames) == B
            for (dets, dets_cnr), (sc, pbv, cnr, cnr_r) in zip(final, frames):
                o_dets, o_cnr = oracle.test_net_frame(sc, pbv.astype(np.float64), np.hstack([cnr] * 2), cnr_r, 2, cfg.TEST.NMS, mpi)
                assert dets[0] == [] and dets_cnr[0] == [] and len(dets) == 2
                assert np.array_equal(dets[1], o_dets[1]) and np.array_equal(dets_cnr[1], o_cnr[1])
                assert dets[1].dtype == np.float32 and dets[1].shape[1] == 5 and dets_cnr[1].shape[1] == 25
                kept += len(dets[1])
        assert kept > 0
        plain = detect_batch.ServeGraph(net, small_feed(1, B, torch))         # post=None: the graph test_mv.ServeGraph captures
        base = test_mv.ServeGraph(net, small_feed(1, B, torch))
        assert "post" not in plain.out and sorted(plain.out) == sorted(base.out)
        plain.replay(); base.replay()
        plain.stream.synchronize(); base.stream.synchronize()
        for k in ("cls_prob", "pred_bv", "corners", "pred_corners_r", "num_rois"):
            assert torch.equal(plain.out[k], base.out[k]), k
        with pytest.raises(ValueError):
            plain.final_detections()
        # two zero-area boxes at one place in frame 1: their union is 0 / 0 whatever they score
        real_tail = ops.box_detect_tail
        bad = torch.tensor([5.0, 5.0, 4.0, 4.0], device="cuda")

        def tail(rois_3d, bbox_pred, num_classes):
            cnr, pr, bv, bvr = real_tail(rois_3d, bbox_pred, num_classes)
            bv[50:52, 4:8] = bad
            return cnr, pr, bv, bvr

        monkeypatch.setattr(ops, "box_detect_tail", tail)
        sgz = detect_batch.ServeGraph(net, small_feed(1, B, torch), post=dict(max_per_image=mpi))
        sgz.replay()
        sgz.stream.synchronize()
        assert int(sgz.out["num_rois"][1].item()) >= 2
        assert sgz.out["post"][5].cpu().numpy().tolist() == [0, 1, 0]
        with pytest.raises(ZeroDivisionError):
            sgz.final_detections()
    finally:
        cfg.TEST.clear()
        cfg.TEST.update(saved)


@gpu
def test_batched_test_net(ops, torch_cuda, oracle, tmp_path, monkeypatch):
    """test_net with cfg.TEST.BATCH_SIZE = 2 over three frames, the third with another image shape: groups [0,1], [2]; both pickles are
    written, evaluate_detections is called once, and every frame's lists equal the oracle's tail of that group's network outputs as
    they were handed to detect_post.  (Batched and per-frame forwards need not agree bitwise -- the head's GEMMs may pick another kernel
    for another M -- the tail is exact given its inputs, and that is what is pinned.)"""
    torch = torch_cuda
    from mv3d_tf_amd.fast_rcnn import detect_batch
    from mv3d_tf_amd.fast_rcnn.config import cfg

    class Imdb:
        name = "synthetic_3frames"
        num_classes = 2
        image_index = ["000000", "000001", "000002"]

        def __init__(self):
            r = np.random.RandomState(1)
            self.bvs = [(r.random_sample((64, 72, 9)) * (r.random_sample((64, 72, 9)) < 0.05)).astype(np.float32) for _ in range(3)]
            self.ims = [r.randint(0, 255, (48 if i < 2 else 56, 160, 3)).astype(np.float32) for i in range(3)]
            self.evaluated = []

        def image_at(self, i): return self.ims[i]
        def bv_at(self, i): return self.bvs[i]
        def calib_at(self, i): return synth.KITTI_CALIB

        def evaluate_detections(self, all_boxes, all_boxes_cnr, output_dir):
            self.evaluated.append((all_boxes, all_boxes_cnr, output_dir))

    calls = []
    real = ops.detect_post

    def recording(cls_prob, pred_bv, corners, pred_cnr_r, num_rois, rows_per_frame, num_classes, max_per_image, nms_thresh, **kw):
        calls.append(dict(scores=cls_prob.float().cpu().numpy(), bv=pred_bv.cpu().numpy(), cnr=corners.cpu().numpy(),
                          num=num_rois.cpu().numpy(), rows=int(rows_per_frame), K=int(num_classes), mpi=int(max_per_image), nms=nms_thresh))
        return real(cls_prob, pred_bv, corners, pred_cnr_r, num_rois, rows_per_frame, num_classes, max_per_image, nms_thresh, **kw)

    net = small_net(torch)
    imdb = Imdb()
    saved, root = dict(cfg.TEST), cfg.ROOT_DIR
    cfg.TEST.update(RPN_PRE_NMS_TOP_N=600, RPN_POST_NMS_TOP_N=50, BATCH_SIZE=2)
    cfg.ROOT_DIR = str(tmp_path)
    monkeypatch.setattr(ops, "detect_post", recording)
    try:
        all_boxes, all_cnr = detect_batch.test_net(None, net, imdb, "w", max_per_image=10)
        assert net.fixed_rois is False
        assert len(imdb.evaluated) == 1 and imdb.evaluated[0][0] is all_boxes
        out = imdb.evaluated[0][2]
        assert os.path.isfile(os.path.join(out, "detections.pkl")) and os.path.isfile(os.path.join(out, "detections_cnr.pkl"))
        assert [len(c["num"]) for c in calls] == [2, 1]      # groups [0, 1], [2]
        i, kept = 0, 0
        for c in calls:
            assert (c["rows"], c["K"], c["mpi"], c["nms"]) == (50, 2, 10, cfg.TEST.NMS)
            for f in range(len(c["num"])):
                sl = slice(f * 50, f * 50 + int(c["num"][f]))
                o_dets, o_cnr = oracle.test_net_frame(c["scores"][sl], c["bv"][sl].astype(np.float64), np.hstack([c["cnr"][sl]] * 2),
                                                      None, 2, cfg.TEST.NMS, 10)
                assert all_boxes[0][i] == [] and all_cnr[0][i] == []
                assert np.array_equal(all_boxes[1][i], o_dets[1]) and np.array_equal(all_cnr[1][i], o_cnr[1]), i
                kept += len(o_dets[1])
                i += 1
        assert i == 3 and kept > 0
        # a zero union in a group raises, as the frame-by-frame loop does
        real_tail = ops.box_detect_tail

        def tail(rois_3d, bbox_pred, num_classes):
            cnr, pr, bv, bvr = real_tail(rois_3d, bbox_pred, num_classes)
            bv[0:2, 4:8] = torch.tensor([5.0, 5.0, 4.0, 4.0], device=bv.device)
            return cnr, pr, bv, bvr

        monkeypatch.setattr(ops, "box_detect_tail", tail)
        with pytest.raises(ZeroDivisionError):
            detect_batch.test_net(None, net, imdb, "w", max_per_image=10)
        assert len(imdb.evaluated) == 1
    finally:
        cfg.TEST.clear()
        cfg.TEST.update(saved)
        cfg.ROOT_DIR = root
