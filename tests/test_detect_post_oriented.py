"""mv3d_detect_post_oriented: detect_post's tail (score cut, order, cap) with the greedy NMS judged by the IoU of the oriented BEV
footprints.  The checker of every GPU test is tests/oriented_nms_restatement.py fed with the arrays the device call was given; all
comparisons are equality (np.array_equal) of det_row, det_count, status and the float rows in front of det_count.  The no-GPU tests
cover what never touches a device: the two symbols, argument validation, the workspace query, the config keys and the guard of the
frame-by-frame entry point."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

import kitti_eval_restatement as KR
import oriented_nms_restatement as ON
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


# ------------------------------------------------------------------ without a GPU
def test_symbols_in_table_and_library(hiplib):
    names = ("mv3d_detect_post_oriented_workspace_bytes", "mv3d_detect_post_oriented")
    raw = C.CDLL(hiplib.LIB_PATH)
    for name in names:
        assert name in hiplib.EXPORTS and hasattr(raw, name), name
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mv3d_hip.h")).read()
    assert "#define MV3D_DETECT_STATUS_NONFINITE 2" in hdr


def test_argument_validation_without_a_device(hiplib):
    L = hiplib.lib()
    P = hiplib.DetectPostParams
    A = 4096                                                 # a non-NULL, aligned "pointer" (never dereferenced: refused before any HIP call)
    good = P(2, 300, 300, 0, 0.05, 0, 0.1)
    big = 1 << 40

    def call(batch, p, source=1, ptrs=None, ws=A, ws_bytes=big):
        a = [A] * 11 if ptrs is None else ptrs               # cls_prob, pred_bv, corners, pred_cnr_r, num_rois | det_bv, det_cnr, det_cnr_r, det_row, det_count, status
        return L.mv3d_detect_post_oriented(a[0], a[1], a[2], a[3], a[4], batch, None if p is None else C.byref(p), source, a[5], a[6],
                                           a[7], a[8], a[9], a[10], ws, ws_bytes, None)

    E = hiplib.ERR_INVALID_ARG
    for required in (0, 1, 2, 5, 6, 8, 9, 10):               # every required pointer, one at a time
        ptrs = [A] * 11
        ptrs[required] = None
        assert call(1, good, ptrs=ptrs) == E, required
    ptrs = [A] * 11
    ptrs[7] = None                                           # pred_cnr_r given, det_cnr_r missing
    assert call(1, good, ptrs=ptrs) == E
    ptrs = [A] * 11
    ptrs[3] = ptrs[7] = None                                 # the regressed footprint without the regressed corners
    assert call(1, good, source=1, ptrs=ptrs) == E
    assert call(1, good, source=2) == E and call(1, good, source=-1) == E
    assert call(1, P(2, 0, 300, 0, 0.05, 0, 0.1)) == E and call(1, P(2, 2049, 300, 0, 0.05, 0, 0.1)) == E
    assert call(1, P(1, 300, 300, 0, 0.05, 0, 0.1)) == E and call(1, P(9, 300, 300, 0, 0.05, 0, 0.1)) == E
    assert call(0, good) == E and call(65536, good) == E and call(1, None) == E
    need = L.mv3d_detect_post_oriented_workspace_bytes(1, C.byref(good))
    assert need > 0
    assert call(1, good, ws=None) == E and call(1, good, ws_bytes=need - 1) == E and call(1, good, ws_bytes=0) == E


def test_workspace_query(hiplib):
    L = hiplib.lib()
    P = hiplib.DetectPostParams

    def q(batch, K, cap):
        return L.mv3d_detect_post_oriented_workspace_bytes(batch, C.byref(P(K, cap, 300, 0, 0.05, 0, 0.1)))

    sizes = [q(1, 2, 64), q(1, 2, 65), q(1, 2, 300), q(1, 2, 2048), q(2, 2, 2048), q(16, 2, 2048), q(16, 3, 2048)]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert sizes == sorted(set(sizes))                       # grows with cap, batch and classes
    mask = 16 * 2048 * 32 * 8                                # batch 16, K 2, cap 2048: the 8 MiB of the mask plus the order lists
    assert mask < q(16, 2, 2048) <= mask + 16 * 2048 * (4 + 16) + 3 * 256
    assert q(1, 2, 0) == 0 and q(1, 2, 2049) == 0 and q(1, 1, 300) == 0 and q(0, 2, 300) == 0


def test_config_keys_default_off():
    from mv3d_tf_amd.fast_rcnn.config import cfg
    assert cfg.TEST.NMS_ORIENTED is False and cfg.TEST.NMS_ORIENTED_BOXES == 'regressed'


def test_frame_by_frame_entry_refuses_the_key(monkeypatch, tmp_path):
    from mv3d_tf_amd.fast_rcnn import test_mv                 # alone: the check does not hang on any other import
    from mv3d_tf_amd.fast_rcnn.config import cfg, get_output_dir

    class Imdb:                                              # the frame list's length and the class count are all test_net may ask for
        image_index = ["000000", "000001"]
        num_classes = 2

        def __getattr__(self, name):                         # name, image_at, bv_at, calib_at, ...: a frame being loaded, a directory made
            raise AssertionError("test_net touched imdb.%s before checking the key" % name)

    monkeypatch.setitem(cfg.TEST, "NMS_ORIENTED", True)
    monkeypatch.setattr(cfg, "ROOT_DIR", str(tmp_path))
    with pytest.raises(ValueError, match="detect_batch.test_net"):
        test_mv.test_net(None, object(), Imdb(), "w")
    assert os.listdir(str(tmp_path)) == []                   # nothing was created

    class Named:
        name = "some_imdb"

    assert get_output_dir(Named(), "w", oriented_nms=True).startswith(str(tmp_path))       # a loop that has the oriented tail
    assert os.path.isdir(get_output_dir(Named(), None))      # no detection loop (proposals): the key does not concern it
    monkeypatch.setitem(cfg.TEST, "NMS_ORIENTED", False)
    assert os.path.isdir(get_output_dir(Named(), "w"))       # the key off: as before


def test_key_off_keeps_the_frame_by_frame_route(monkeypatch):
    from mv3d_tf_amd.fast_rcnn import detect_batch, test_mv
    from mv3d_tf_amd.fast_rcnn.config import cfg
    assert cfg.TEST.BATCH_SIZE == 1 and not cfg.TEST.NMS_ORIENTED
    monkeypatch.setattr(test_mv, "test_net", lambda *a, **k: ("frame by frame", a, k))
    assert detect_batch.test_net(None, "net", "imdb", "w", max_per_image=7)[0] == "frame by frame"


def test_restatement_on_hand_cases():
    """the checker itself, where the answer is known by hand"""
    sq = lambda x0, x1, y0, y1: np.array([x1, x1, x0, x0, 0, 0, 0, 0, y1, y0, y0, y1, 0, 0, 0, 0] + [0] * 4 + [1] * 4, np.float32)
    a, b = sq(0, 2, 0, 2), sq(0, 2, 0, 1)
    assert KR.iou_pair(a, b)[0] == 0.5
    cnr = np.stack([a, b, sq(10, 12, 0, 2)])
    assert ON.greedy(cnr, 0.5, False) == [0, 2] and ON.greedy(cnr, 0.5, True) == [0, 1, 2]
    s = np.array([0.5, np.nan, 0.5, -0.0, 0.0, 0.9, 0.01], np.float32)
    assert ON.candidate_order(s, 7, 0.05) == [5, 2, 0]       # NaN never passes the cut; equal scores by larger row
    assert ON.candidate_order(s, 7, -1.0) == [5, 2, 0, 6, 4, 3]
    assert ON.candidate_order(s, 2, 0.05) == [0]


# ------------------------------------------------------------------ on the device
def dev(t, torch, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(t), dtype=dtype).cuda()


def unit(rng, n):
    v = rng.uniform(-1, 1, (n, 2)) + np.array([1e-3, 0])
    return v / np.sqrt((v * v).sum(1, keepdims=True))


def scene(rng, K, rows, B, objects=None):
    """B frames of `rows` rows: rotated car-sized boxes (synth.box_corners), jittered copies clustered around a few objects per frame
    so that chains of overlaps occur; the regressed corners of every class are another jitter of the same objects.
    -> scores (R, K), pred_bv (R, 4K), corners (R, 24), pred_cnr_r (R, 24K), all f32"""
    R, G = B * rows, objects or max(1, rows // 8)
    scores = (rng.random_sample((R, K)) ** 2).astype(np.float32)
    scores[:, 0] = 1 - scores[:, 1:].max(1)
    corners, cnr_r = np.empty((R, 24), np.float32), np.empty((R, 24 * K), np.float32)
    for f in range(B):
        ctr = np.stack([rng.uniform(5, 55, G), rng.uniform(-20, 20, G), rng.uniform(-1.9, -1.5, G)], 1)
        lwh = np.stack([rng.uniform(3, 5, G), rng.uniform(1.4, 2, G), rng.uniform(1.3, 2, G)], 1)
        cs, pick = unit(rng, G), rng.randint(0, G, rows)

        def jitter():
            jc = ctr[pick] + np.hstack([rng.uniform(-0.8, 0.8, (rows, 2)), rng.uniform(-0.1, 0.1, (rows, 1))])
            jcs = cs[pick] + rng.uniform(-0.1, 0.1, (rows, 2))
            return synth.box_corners(jc, lwh[pick] * rng.uniform(0.9, 1.1, (rows, 3)), jcs / np.sqrt((jcs * jcs).sum(1, keepdims=True)))

        sl = slice(f * rows, (f + 1) * rows)
        corners[sl] = jitter()
        for j in range(K):
            cnr_r[sl, 24 * j:24 * j + 24] = jitter()
    c = rng.uniform(20, 580, (R, 1, 2)); wh = rng.uniform(8, 40, (R, K, 2))
    bx = np.concatenate([c - wh / 2, c + wh / 2], 2).reshape(R, 4 * K).astype(np.float32)
    return scores, bx, corners, cnr_r


def run(ops, torch, arrays, num, K, rows, mpi, thresh, strict=False, footprint="regressed", with_r=True, workspace=None, score_thresh=0.05):
    scores, bx, cnr, cnr_r = arrays
    out = ops.detect_post_oriented(dev(scores, torch), dev(bx, torch), dev(cnr, torch), dev(cnr_r, torch) if with_r else None,
                                   None if num is None else dev(np.asarray(num, np.int32), torch), rows, K, mpi, thresh,
                                   score_thresh=score_thresh, strict_gt=strict, footprint=footprint, workspace=workspace)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def restate(arrays, num, K, rows, mpi, thresh, strict=False, footprint="regressed", score_thresh=0.05, stats=None, cache=None, with_r=True):
    scores, bx, cnr, cnr_r = arrays
    return ON.detect_post_oriented(scores, bx, cnr, cnr_r if with_r else None, num, rows, K, mpi, thresh, score_thresh=score_thresh,
                                   strict=strict, source=1 if footprint == "regressed" else 0, stats=stats, cache=cache)


def check(got, ref, K, equal_nan=False):
    """got: host copies of the device call's outputs; ref: the restatement's frames.  Returns the kept total of every frame."""
    bv, cnr, cnr_r, row, cnt, st = got
    eq = lambda a, b: np.array_equal(a, b, equal_nan=equal_nan)
    assert cnt.shape[0] == st.shape[0] == len(ref)
    totals = []
    for f, (rows_, status, dets, dcnr, dcnr_r) in enumerate(ref):
        assert st[f] == status and cnt[f, 0] == 0, (f, st[f], status)
        for j in range(1, K):
            c = int(cnt[f, j])
            assert c == len(rows_[j]), (f, j, c, len(rows_[j]))
            assert row[f, j, :c].tolist() == [int(r) for r in rows_[j]], (f, j)
            assert eq(bv[f, j, :c], dets[j]) and eq(cnr[f, j, :c], dcnr[j]), (f, j)
            if cnr_r is not None:
                assert eq(cnr_r[f, j, :c], dcnr_r[j]), (f, j)
        totals.append(int(cnt[f, 1:].sum()))
    return totals


SWEEP = ((2, 1, 0, 1), (2, 63, 0, 1), (2, 64, 0, 2), (2, 65, 300, 2), (3, 130, 40, 3), (4, 300, 100, 2))


@gpu
@pytest.mark.parametrize("K,rows,mpi,B", SWEEP)
def test_sweep_equals_restatement(ops, torch_cuda, K, rows, mpi, B):
    """mask-word and tile boundaries (63 / 64 / 65 / 130 / 300 rows), several classes, the cap biting; both footprints, both rules;
    the last frame of a batch of several has every score below the cut"""
    rng = np.random.RandomState(2000 + 7 * rows + K + mpi)
    arrays = scene(rng, K, rows, B)
    if B > 1:
        arrays[0][(B - 1) * rows:, 1:] *= 0.04
    if rows > 2:                                             # exact duplicates: an IoU at the top of the range
        arrays[2][1] = arrays[2][0]
        arrays[3][1] = arrays[3][0]
    candidates, suppressed = int((arrays[0][:, 1:] > np.float32(0.05)).sum()), 0
    for footprint in ("regressed", "proposal"):
        cache = {}
        for strict, thresh in ((False, 0.1), (True, 0.1), (False, 0.45)):
            got = run(ops, torch_cuda, arrays, None, K, rows, mpi, thresh, strict, footprint)
            ref = restate(arrays, None, K, rows, mpi, thresh, strict, footprint, cache=cache)
            totals = check(got, ref, K)
            if B > 1:
                assert totals[-1] == 0
            if mpi > 0:                                      # (tie-free scores: the cap is exact)
                assert max(totals) <= mpi
            suppressed += candidates - sum(len(r) for fr in restate(arrays, None, K, rows, 0, thresh, strict, footprint, cache=cache) for r in fr[0])
        assert max(totals) > 0
    if rows >= 63:
        assert suppressed > 0
    got = run(ops, torch_cuda, arrays, None, K, rows, mpi, 0.1, False, "proposal", with_r=False)   # without the regressed corners
    assert got[2] is None
    check(got, restate(arrays, None, K, rows, mpi, 0.1, False, "proposal", with_r=False), K)


@gpu
def test_ragged_num_rois(ops, torch_cuda):
    """frames with fewer rows than the capacity (one with none, one with one), counts above the capacity and below zero are clamped"""
    rng = np.random.RandomState(12)
    K, rows, B, mpi = 3, 70, 6, 30
    arrays = scene(rng, K, rows, B)
    num = [rows, 0, 1, rows + 500, 37, -4]
    got = run(ops, torch_cuda, arrays, num, K, rows, mpi, 0.1)
    totals = check(got, restate(arrays, num, K, rows, mpi, 0.1), K)
    assert totals[1] == 0 and totals[5] == 0 and totals[0] > 0 and totals[4] > 0
    clamped = check(got, restate(arrays, [rows, 0, 1, rows, 37, 0], K, rows, mpi, 0.1), K)
    assert clamped == totals


def rect(cx, cy, l, w, yaw_deg=0.0):
    a = np.deg2rad(yaw_deg)
    return synth.box_corners([[cx, cy, -1.7]], [[l, w, 1.5]], [[np.cos(a), np.sin(a)]])[0]


def one_class(cnr, scores, bv=None):
    """rows of one frame, K = 2, the same corners as proposal and regressed footprint"""
    n = len(scores)
    s = np.zeros((n, 2), np.float32)
    s[:, 1] = scores
    cnr = np.asarray(cnr, np.float32).reshape(n, 24)
    bx = np.zeros((n, 8), np.float32) if bv is None else np.hstack([np.zeros((n, 4)), bv]).astype(np.float32)
    return s, bx, cnr, np.hstack([cnr, cnr]).astype(np.float32)


@gpu
def test_greedy_is_not_transitive(ops, torch_cuda):
    """A suppresses B, B overlaps C above the threshold, A and C do not: {A, C} are kept.  A, B, C are sorted positions 0, 70 and 140,
    three different 64-blocks; the rows between them are boxes far from everything"""
    n = 141
    cnr = np.stack([rect(1000.0 + 10.0 * r, 500.0, 4, 2) for r in range(n)])
    cnr[0], cnr[70], cnr[140] = rect(10, 0, 4, 2), rect(11.5, 0, 4, 2), rect(13, 0, 4, 2)
    scores = (0.9 - 0.001 * np.arange(n)).astype(np.float32)  # row r is sorted position r
    arrays = one_class(cnr, scores)
    ab, bc, ac = (KR.iou_pair(cnr[i], cnr[k])[0] for i, k in ((0, 70), (70, 140), (0, 140)))
    assert ab > 0.3 and bc > 0.3 and ac < 0.3
    got = run(ops, torch_cuda, arrays, None, 2, n, 0, 0.3, footprint="proposal")
    check(got, restate(arrays, None, 2, n, 0, 0.3, footprint="proposal"), 2)
    assert got[4][0, 1] == n - 1 and got[3][0, 1, :n - 1].tolist() == [r for r in range(n) if r != 70]


def pixel_box(c, scale=10.0):
    x, y = c[:4] * scale, c[8:12] * scale
    return np.array([x.min(), y.min(), x.max(), y.max()], np.float32).round()


def pixel_iou(a, b):
    iw = min(a[2], b[2]) - max(a[0], b[0]) + 1
    ih = min(a[3], b[3]) - max(a[1], b[1]) + 1
    inter = max(iw, 0) * max(ih, 0)
    area = lambda q: (q[2] - q[0] + 1) * (q[3] - q[1] + 1)
    return inter / (area(a) + area(b) - inter)


@gpu
def test_crossing_cars_are_both_kept(ops, torch_cuda):
    """the point of the feature: two car-sized boxes at +45 and -45 degrees that cross at their ends.  Their axis-aligned pixel boxes
    overlap above nms_thresh (ops.detect_post keeps one), their footprints below it (detect_post_oriented keeps both); two
    coincident rotated boxes keep one under both rules"""
    torch = torch_cuda
    a, b = rect(20, 0, 4.5, 1.8, 45), rect(22, 0, 4.5, 1.8, -45)
    thresh = 0.3
    bv = np.stack([pixel_box(a), pixel_box(b)])
    assert pixel_iou(bv[0], bv[1]) > thresh + 0.05 and 0 < KR.iou_pair(a, b)[0] < thresh - 0.05
    arrays = one_class([a, b], [0.9, 0.8], bv)
    plain = ops.detect_post(*(dev(x, torch) for x in arrays), None, 2, 2, 0, thresh)
    torch.cuda.synchronize()
    assert plain[4].cpu().numpy().tolist() == [[0, 1]]
    for strict in (False, True):
        got = run(ops, torch, arrays, None, 2, 2, 0, thresh, strict)
        check(got, restate(arrays, None, 2, 2, 0, thresh, strict), 2)
        assert got[4].tolist() == [[0, 2]] and got[3][0, 1, :2].tolist() == [0, 1]
        assert np.array_equal(got[0][0, 1, :2, :4], bv)      # det_bv still carries the pixel boxes
        same = one_class([a, a], [0.9, 0.8], bv[[0, 0]])
        got = run(ops, torch, same, None, 2, 2, 0, thresh, strict)
        check(got, restate(same, None, 2, 2, 0, thresh, strict), 2)
        assert got[4].tolist() == [[0, 1]] and got[3][0, 1, 0] == 0


@gpu
def test_threshold_edge(ops, torch_cuda):
    """[0,2]x[0,2] and [0,2]x[0,1]: IoU exactly 0.5.  At nms_thresh 0.5 `>=` suppresses and `>` does not; one ulp (f64) below both
    suppress, one ulp above neither"""
    sq = lambda x0, x1, y0, y1: np.array([x1, x1, x0, x0, 0, 0, 0, 0, y1, y0, y0, y1, 0, 0, 0, 0] + [0] * 4 + [1] * 4, np.float32)
    arrays = one_class([sq(0, 2, 0, 2), sq(0, 2, 0, 1)], [0.9, 0.8])
    assert KR.iou_pair(arrays[2][0], arrays[2][1])[0] == 0.5
    below, above = float(np.nextafter(0.5, 0.0)), float(np.nextafter(0.5, 1.0))
    assert below < 0.5 < above
    for thresh, strict, kept in ((0.5, False, 1), (0.5, True, 2), (below, False, 1), (below, True, 1), (above, False, 2), (above, True, 2)):
        got = run(ops, torch_cuda, arrays, None, 2, 2, 0, thresh, strict)
        check(got, restate(arrays, None, 2, 2, 0, thresh, strict), 2)
        assert got[4][0, 1] == kept, (thresh, strict)


@gpu
def test_ties_and_order(ops, torch_cuda):
    """scores in steps of 1/16: equal scores are processed (and kept) by larger row index, and the cap's `>=` keeps tied scores beyond
    max_per_image; -0.0 and +0.0 are one score; a NaN score is no candidate (the cut `score > score_thresh` is false for it, as in
    detect_post, so the key rule's "NaN first" cannot show through this entry)"""
    rng = np.random.RandomState(22)
    over = 0
    for K, rows, mpi, B in ((2, 130, 12, 2), (3, 70, 9, 3)):
        arrays = scene(rng, K, rows, B, objects=rows // 3)
        arrays[0][:, 1:] = np.floor(arrays[0][:, 1:] * 16) / 16
        arrays[0][3, 1] = arrays[0][rows + 5, 1] = np.nan
        got = run(ops, torch_cuda, arrays, None, K, rows, mpi, 0.1)
        totals = check(got, restate(arrays, None, K, rows, mpi, 0.1), K)
        over += int(max(totals) > mpi)
        for f in range(B):
            for j in range(1, K):
                r = got[3][f, j, :got[4][f, j]]
                s = arrays[0][f * rows + r, j]
                assert not np.isnan(s).any() and (np.diff(s) <= 0).all()
                assert all(r[i] > r[i + 1] for i in range(len(r) - 1) if s[i] == s[i + 1]), (f, j)
    assert over >= 1
    # +-0 with the cut below zero: rows 0..5 far apart, all kept; the zeros of either sign order by row alone
    cnr = np.stack([rect(10.0 * r, 0, 4, 2) for r in range(6)])
    arrays = one_class(cnr, np.array([0.0, -0.0, 0.5, -0.0, 0.0, -0.5], np.float32))
    arrays[0][2, 1] = np.nan
    got = run(ops, torch_cuda, arrays, None, 2, 6, 0, 0.1, score_thresh=-1.0)
    check(got, restate(arrays, None, 2, 6, 0, 0.1, score_thresh=-1.0), 2)
    assert got[3][0, 1, :got[4][0, 1]].tolist() == [4, 3, 1, 0, 5]


def quad(pts, z0=-1.7, z1=-0.2):
    """four (x, y) footprint vertices -> (24,) corners; the top face repeats them"""
    p = np.asarray(pts, np.float64)
    return np.hstack([p[:, 0], p[:, 0], p[:, 1], p[:, 1], [z0] * 4, [z1] * 4]).astype(np.float32)


@gpu
def test_odd_footprints(ops, torch_cuda):
    """the regressed corners are eight free points: clockwise and counter-clockwise footprints, a zero-area one, a self-intersecting
    one and a non-convex one, the last both as the earlier box (the polygon) and as the later one (the clipper).  All defined by the
    operation order, all equal to the restatement"""
    box = [(0, 0), (4, 0), (4, 2), (0, 2)]                                    # counter-clockwise
    dart = [(0, 0), (4, 0), (1, 1), (0, 4)]                                   # non-convex at (1, 1)
    shift = lambda pts, dx, dy: [(x + dx, y + dy) for x, y in pts]
    cnr = np.stack([
        quad(box), quad(shift(box, 0.5, 0.3)[::-1]),                          # 0, 1: ccw, then its clockwise neighbour
        quad(shift([(0, 0), (2, 0), (4, 0), (1, 0)], 20, 0)), quad(shift(box, 20, -1)),       # 2, 3: zero area, inside 3
        quad(shift([(0, 0), (4, 2), (4, 0), (0, 2)], 40, 0)), quad(shift(box, 40.5, 0.2)),    # 4, 5: a bow tie and a box on it
        quad(shift(dart, 60, 0)), quad(shift(box, 60.2, 0.1)),                # 6, 7: dart first (polygon), box later
        quad(shift(box, 80.2, 0.1)), quad(shift(dart, 80, 0)),                # 8, 9: box first, dart later (clipper)
        quad(shift(dart, 100, 0)), quad(shift(dart, 100.3, 0.2)),             # 10, 11: two darts
    ])
    scores = (0.95 - 0.01 * np.arange(len(cnr))).astype(np.float32)
    d, b = cnr[6], cnr[7]
    assert KR.iou_pair(d, b)[0] > 0 and KR.iou_pair(b, d)[0] > 0
    arrays = one_class(cnr, scores)
    ious = sorted({ON.overlap(cnr[i], cnr[i + 1], *R3.extents(cnr[i:i + 2])) for i in range(0, 12, 2)})
    kept = set()
    for thresh in [0.05, 0.3, 0.6] + [v for v in ious if v > 0]:              # each pair's own IoU too: `>=` and `>` part there
        for strict in (False, True):
            got = run(ops, torch_cuda, arrays, None, 2, len(cnr), 0, thresh, strict)
            check(got, restate(arrays, None, 2, len(cnr), 0, thresh, strict), 2)
            kept.add(int(got[4][0, 1]))
    assert len(kept) > 2
    rev = one_class(cnr[::-1].copy(), scores)                                 # every pair the other way round
    for thresh in (0.05, 0.3):
        got = run(ops, torch_cuda, rev, None, 2, len(cnr), 0, thresh)
        check(got, restate(rev, None, 2, len(cnr), 0, thresh), 2)


@gpu
def test_non_finite_boxes(ops, torch_cuda):
    """a NaN and an inf corner in rows that pass the cut: bit 2 on that frame only, the rows are kept and suppress nothing (a copy of
    the box the NaN row had, scored lower, stays); a non-finite value behind the cut, or in the corner set that is not the footprint,
    sets nothing"""
    rng = np.random.RandomState(32)
    K, rows, B = 2, 70, 3
    arrays = scene(rng, K, rows, B)
    scores, bx, cnr, cnr_r = arrays
    f1 = rows
    scores[f1 + 5, 1], scores[f1 + 9, 1], scores[f1 + 11, 1] = 2.0, 1.5, 1.25      # the frame's three best, in this order
    cnr_r[f1 + 11, 24:48] = cnr_r[f1 + 5, 24:48]             # the twin of row 5's box
    cnr_r[f1 + 5, 24 + 1] = np.nan
    cnr_r[f1 + 9, 24 + 10] = np.inf
    scores[2 * rows + 3, 1] = 0.01                           # frame 2: behind the cut
    cnr_r[2 * rows + 3, 24 + 2] = np.nan
    cnr[4, 3] = np.nan                                       # frame 0: not the footprint of this call
    cnr_r[7, 5] = np.inf                                     # frame 0: class 0's slice
    scores[4, 1] = 2.0
    got = run(ops, torch_cuda, arrays, None, K, rows, 0, 0.1)
    check(got, restate(arrays, None, K, rows, 0, 0.1), K, equal_nan=True)
    assert got[5].tolist() == [0, ON.STATUS_NONFINITE, 0]
    kept = got[3][1, 1, :got[4][1, 1]].tolist()
    assert kept[:3] == [5, 9, 11]
    got = run(ops, torch_cuda, arrays, None, K, rows, 0, 0.1, footprint="proposal")
    check(got, restate(arrays, None, K, rows, 0, 0.1, footprint="proposal"), K, equal_nan=True)
    assert got[5].tolist() == [ON.STATUS_NONFINITE, 0, 0]
    out = ops.detect_post_oriented(*(dev(a, torch_cuda) for a in arrays), None, rows, K, 0, 0.1)
    assert len(ops.detect_post_lists(out)) == B             # bit 2 is no ZeroDivisionError


def full_size_scene(seed=1, n=2048):
    rng = np.random.RandomState(seed)
    i = np.arange(n)
    ctr = np.stack([3.0 * (i % 64) + rng.uniform(-1, 1, n), 2.0 * (i // 64) + rng.uniform(-0.6, 0.6, n), np.full(n, -1.7)], 1)
    lwh = np.stack([rng.uniform(3, 5, n), rng.uniform(1.4, 2, n), np.full(n, 1.5)], 1)
    yaw = rng.uniform(0, 2 * np.pi, n)
    cnr = synth.box_corners(ctr, lwh, np.stack([np.cos(yaw), np.sin(yaw)], 1))
    return one_class(cnr, (rng.permutation(n) / n).astype(np.float32))


@gpu
def test_full_size(ops, torch_cuda):
    """one frame of 2048 rows (32 mask words, 528 tiles), a grid of car-sized boxes with uniform yaw at nms_thresh 0.1"""
    n = 2048
    arrays = full_size_scene()
    stats = {}
    ref = restate(arrays, None, 2, n, 0, 0.1, stats=stats)
    assert stats["clipped"] <= 40000                          # (keeps the checker fast; not a measurement)
    kept, candidates = len(ref[0][0][1]), int((arrays[0][:, 1] > np.float32(0.05)).sum())
    assert kept >= n // 4 and candidates - kept >= n // 4     # neither trivial answer passes
    got = run(ops, torch_cuda, arrays, None, 2, n, 0, 0.1)
    check(got, ref, 2)


@gpu
@pytest.mark.parametrize("K,rows,mpi,B", ((2, 65, 0, 2), (3, 130, 40, 3)))
def test_poisoned_workspace(ops, torch_cuda, K, rows, mpi, B):
    """the workspace is never memset: filled with 0xFF or with zeros before the call, the result is the same (a mask word, a count or
    an order entry read without having been written would show)"""
    arrays = scene(np.random.RandomState(42 + rows), K, rows, B)
    ref = restate(arrays, None, K, rows, mpi, 0.1)
    results = []
    for fill in (0xFF, 0x00):
        ws = ops.detect_post_oriented_workspace(B, K, rows, "cuda")
        ws.fill_(fill)
        got = run(ops, torch_cuda, arrays, None, K, rows, mpi, 0.1, workspace=ws)
        check(got, ref, K)
        results.append(got)
    assert np.array_equal(results[0][4], results[1][4]) and np.array_equal(results[0][5], results[1][5])


@gpu
def test_nms_oriented_entries(ops, torch_cuda):
    from mv3d_tf_amd.fast_rcnn import nms_wrapper
    torch = torch_cuda
    rng = np.random.RandomState(52)
    for n in (0, 1, 64, 65, 300):
        _, _, cnr, _ = scene(rng, 2, max(n, 1), 1)
        cnr = cnr[:n]
        scores = rng.random_sample(n).astype(np.float32)
        order = ON.candidate_order(scores, n, -np.inf)
        for thresh, strict in ((0.1, False), (0.4, True)):
            want = [order[p] for p in ON.greedy(cnr[order].reshape(-1, 24), thresh, strict)]
            keep = ops.nms_oriented(dev(cnr, torch), dev(scores, torch), thresh, strict_gt=strict)
            assert keep.dtype == torch.int64 and keep.is_cuda and keep.cpu().numpy().tolist() == want, (n, thresh)
        want = [order[p] for p in ON.greedy(cnr[order].reshape(-1, 24), 0.1, False)]
        assert nms_wrapper.nms_oriented(np.hstack([cnr, scores[:, None]]).astype(np.float32), 0.1) == want
        if n >= 64:
            assert 0 < len(want) < n
    with pytest.raises(ValueError, match="2048"):
        ops.nms_oriented(torch.zeros((2049, 24), device="cuda"), torch.zeros(2049, device="cuda"), 0.1)
    with pytest.raises(ValueError, match="2048"):
        nms_wrapper.nms_oriented(np.zeros((2049, 25), np.float32), 0.1)


@gpu
def test_captured_in_a_graph(ops, torch_cuda):
    """kernel launches only: the call sits in a captured graph with `out=` and `workspace=`; replays on changed inputs equal the eager
    call and the restatement"""
    torch = torch_cuda
    K, rows, B, mpi = 3, 130, 3, 40
    first = scene(np.random.RandomState(61), K, rows, B)
    static = [dev(a, torch) for a in first] + [dev(np.array([rows, 100, 7], np.int32), torch)]
    out = ops.detect_post_outputs(B, K, rows, static[0].device)
    ws = ops.detect_post_oriented_workspace(B, K, rows, static[0].device)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.detect_post_oriented(*static, rows, K, mpi, 0.1, out=out, workspace=ws)
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        ops.detect_post_oriented(*static, rows, K, mpi, 0.1, out=out, workspace=ws)
    for seed, num in ((62, [rows, rows, 0]), (63, [5, rows, 64])):
        arrays = scene(np.random.RandomState(seed), K, rows, B)
        if seed == 63:
            arrays[0][rows + 2, 1] = 0.99
            arrays[3][rows + 2, 24 + 3] = np.nan
        with torch.cuda.stream(stream):
            for s, a in zip(static, list(arrays) + [np.asarray(num, np.int32)]):
                s.copy_(torch.as_tensor(a), non_blocking=False)
            g.replay()
        stream.synchronize()
        got = tuple(t.cpu().numpy() for t in out)
        eager = run(ops, torch, arrays, num, K, rows, mpi, 0.1)
        assert np.array_equal(got[4], eager[4]) and np.array_equal(got[5], eager[5])
        assert got[5].tolist() == ([0, 2, 0] if seed == 63 else [0, 0, 0])       # the status word is cleared inside the graph
        for f in range(B):
            for j in range(1, K):
                c = int(got[4][f, j])
                for a, b in zip(got[:4], eager[:4]):
                    assert np.array_equal(a[f, j, :c], b[f, j, :c], equal_nan=True)
        check(got, restate(arrays, num, K, rows, mpi, 0.1), K, equal_nan=True)


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


def frame_lists(sc, pbv, cnr, cnr_r, mpi, nms, footprint):
    """the restatement's final lists of one frame's rows"""
    rows, status = ON.frame_tail(sc, pbv, cnr, cnr_r, 2, mpi, nms, source=1 if footprint == "regressed" else 0)
    dets, dcnr, dcnr_r = ON.lists(sc, pbv, cnr, cnr_r, 2, rows)
    return dets, (dcnr_r if footprint == "regressed" else dcnr), status


@gpu
def test_serve_graph_with_oriented_post(ops, torch_cuda, oracle):
    """ServeGraph(..., post=dict(max_per_image=..., oriented=True)): final_detections() == the restatement applied to what
    detections() returns from the same replay (the regressed corners as dets_cnr); `footprint='proposal'` keeps det_cnr; without
    `oriented` (the key off) the graph ends in ops.detect_post as before"""
    torch = torch_cuda
    from mv3d_tf_amd.fast_rcnn import detect_batch
    from mv3d_tf_amd.fast_rcnn.config import cfg
    B, mpi = 3, 300
    saved = dict(cfg.TEST)
    cfg.TEST.update(RPN_PRE_NMS_TOP_N=600, RPN_POST_NMS_TOP_N=50)
    try:
        net = small_net(torch)
        for post in (dict(max_per_image=mpi, oriented=True), dict(max_per_image=10, oriented=True, footprint="proposal")):
            sg = detect_batch.ServeGraph(net, small_feed(1, B, torch), post=post)
            footprint = post.get("footprint", "regressed")
            kept = 0
            for seed in (1, 2):
                sg.replay(small_feed(seed, B, torch))
                final = sg.final_detections()
                frames = sg.detections()
                assert len(final) == len(frames) == B
                for (dets, dets_cnr), (sc, pbv, cnr, cnr_r) in zip(final, frames):
                    o_dets, o_cnr, status = frame_lists(sc, pbv, cnr, cnr_r, post["max_per_image"], cfg.TEST.NMS, footprint)
                    assert status == 0 and dets[0] == [] and dets_cnr[0] == [] and len(dets) == 2
                    assert np.array_equal(dets[1], o_dets[1]) and np.array_equal(dets_cnr[1], o_cnr[1])
                    assert dets[1].dtype == np.float32 and dets[1].shape[1] == 5 and dets_cnr[1].shape[1] == 25
                    kept += len(dets[1])
            assert kept > 0
        assert not cfg.TEST.NMS_ORIENTED                      # the key off: the axis-aligned tail, as before
        sg = detect_batch.ServeGraph(net, small_feed(1, B, torch), post=dict(max_per_image=10))
        assert sg.post["oriented"] is False
        sg.replay(small_feed(2, B, torch))
        for (dets, dets_cnr), (sc, pbv, cnr, cnr_r) in zip(sg.final_detections(), sg.detections()):
            o_dets, o_cnr = oracle.test_net_frame(sc, pbv.astype(np.float64), np.hstack([cnr] * 2), cnr_r, 2, cfg.TEST.NMS, 10)
            assert np.array_equal(dets[1], o_dets[1]) and np.array_equal(dets_cnr[1], o_cnr[1])
    finally:
        cfg.TEST.clear()
        cfg.TEST.update(saved)


class ThreeFrames:
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


@gpu
def test_test_net_with_the_key(ops, torch_cuda, oracle, tmp_path, monkeypatch):
    """detect_batch.test_net with cfg.TEST.NMS_ORIENTED at BATCH_SIZE 1 (groups of one frame) and 2 (groups [0, 1], [2]): the pickles'
    all_boxes_cnr rows are the REGRESSED corners of the restatement's kept rows ('proposal': the proposal's corners), given the arrays
    handed to the tail; with the key off the batched route ends in ops.detect_post as before"""
    torch = torch_cuda
    from mv3d_tf_amd.fast_rcnn import detect_batch
    from mv3d_tf_amd.fast_rcnn.config import cfg
    calls = []
    real, real_plain = ops.detect_post_oriented, ops.detect_post

    def recording(cls_prob, pred_bv, corners, pred_cnr_r, num_rois, rows_per_frame, num_classes, max_per_image, nms_thresh, **kw):
        calls.append(dict(scores=cls_prob.float().cpu().numpy(), bv=pred_bv.cpu().numpy(), cnr=corners.cpu().numpy(),
                          cnr_r=None if pred_cnr_r is None else pred_cnr_r.cpu().numpy(), num=num_rois.cpu().numpy(),
                          rows=int(rows_per_frame), K=int(num_classes), mpi=int(max_per_image), nms=nms_thresh, kw=kw))
        return (real if "footprint" in kw else real_plain)(cls_prob, pred_bv, corners, pred_cnr_r, num_rois, rows_per_frame, num_classes,
                                                           max_per_image, nms_thresh, **kw)

    net = small_net(torch)
    saved, root = dict(cfg.TEST), cfg.ROOT_DIR
    cfg.ROOT_DIR = str(tmp_path)
    monkeypatch.setattr(ops, "detect_post_oriented", recording)
    monkeypatch.setattr(ops, "detect_post", recording)
    try:
        for batch_size, footprint, groups in ((1, "regressed", [1, 1, 1]), (2, "regressed", [2, 1]), (2, "proposal", [2, 1])):
            cfg.TEST.update(RPN_PRE_NMS_TOP_N=600, RPN_POST_NMS_TOP_N=50, BATCH_SIZE=batch_size, NMS_ORIENTED=True,
                            NMS_ORIENTED_BOXES=footprint)
            del calls[:]
            imdb = ThreeFrames()
            all_boxes, all_cnr = detect_batch.test_net(None, net, imdb, "w", max_per_image=10)
            assert net.fixed_rois is False and len(imdb.evaluated) == 1 and imdb.evaluated[0][1] is all_cnr
            out = imdb.evaluated[0][2]
            with open(os.path.join(out, "detections_cnr.pkl"), "rb") as fh:
                pickled_cnr = pickle.load(fh)
            with open(os.path.join(out, "detections.pkl"), "rb") as fh:
                pickled = pickle.load(fh)
            assert [len(c["num"]) for c in calls] == groups
            i, kept = 0, 0
            for c in calls:
                assert (c["rows"], c["K"], c["mpi"], c["nms"], c["kw"]["footprint"]) == (50, 2, 10, cfg.TEST.NMS, footprint)
                assert c["cnr_r"] is not None
                for f in range(len(c["num"])):
                    sl = slice(f * 50, f * 50 + int(c["num"][f]))
                    o_dets, o_cnr, status = frame_lists(c["scores"][sl], c["bv"][sl], c["cnr"][sl], c["cnr_r"][sl], 10, cfg.TEST.NMS, footprint)
                    assert status == 0 and all_boxes[0][i] == [] and all_cnr[0][i] == []
                    assert np.array_equal(all_boxes[1][i], o_dets[1]) and np.array_equal(all_cnr[1][i], o_cnr[1]), i
                    assert np.array_equal(pickled[1][i], o_dets[1]) and np.array_equal(pickled_cnr[1][i], o_cnr[1]), i
                    kept += len(o_dets[1])
                    i += 1
            assert i == 3 and kept > 0
        # the key off: BATCH_SIZE 2 ends in ops.detect_post, equal to the oracle's tail, as before
        cfg.TEST.update(BATCH_SIZE=2, NMS_ORIENTED=False, NMS_ORIENTED_BOXES="regressed")
        del calls[:]
        imdb = ThreeFrames()
        all_boxes, all_cnr = detect_batch.test_net(None, net, imdb, "w", max_per_image=10)
        assert [len(c["num"]) for c in calls] == [2, 1] and all("footprint" not in c["kw"] and c["cnr_r"] is None for c in calls)
        i = 0
        for c in calls:
            for f in range(len(c["num"])):
                sl = slice(f * 50, f * 50 + int(c["num"][f]))
                o_dets, o_cnr = oracle.test_net_frame(c["scores"][sl], c["bv"][sl].astype(np.float64), np.hstack([c["cnr"][sl]] * 2), None,
                                                      2, cfg.TEST.NMS, 10)
                assert np.array_equal(all_boxes[1][i], o_dets[1]) and np.array_equal(all_cnr[1][i], o_cnr[1]), i
                i += 1
    finally:
        cfg.TEST.clear()
        cfg.TEST.update(saved)
        cfg.ROOT_DIR = root
