"""KITTI 2D detection and orientation (csrc/kitti_eval.hip, mv3d_tf_amd/datasets/kitti_eval.py): AP_2D and AOS on the device.

CPU tests pin the plain-Python restatement (tests/kitti_eval_image_restatement.py) against hand values, the golden labels'
camera boxes and the heading-flip case, check the product's host arithmetic and the new C-ABI entries' argument validation.
`gpu` tests compare the device image boxes, camera boxes, pass-1 scores, pass-2 counts and orientation similarity sums with
the restatement and run test_net -> kitti_mv3d.evaluate_detections with all four metrics."""
import ctypes as C
import os

import numpy as np
import pytest

import kitti_eval_image_restatement as RI
from conftest import golden
from mv3d_tf_amd import synth

CAR, VAN = 0, 1
PERM = np.array([2, 3, 0, 1, 6, 7, 4, 5])             # the same cuboid, front and back swapped: heading turned by pi


def _flip(cnr):
    c = np.asarray(cnr, np.float32).reshape(3, 8)
    return c[:, PERM].reshape(24)


def _angle_diff(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


# ------------------------------------------------------------------ restatement (CPU)
def test_iou2d_hand_values():
    a = np.array([100.0, 50.0, 200.0, 150.0])
    assert RI.iou2d(a, np.float32(a)) == 1.0
    assert RI.iou2d(a, np.float32([150, 50, 250, 150])) == pytest.approx(1 / 3, abs=1e-15)      # half shifted: 50 / 150
    assert RI.iou2d(a, np.float32([200, 50, 300, 150])) == 0.0                                 # touching edges
    assert RI.iou2d(a, np.float32([100, 150, 200, 250])) == 0.0
    assert RI.dontcare_overlap(a, np.float32([150, 0, 400, 400])) == 0.5                       # inter / detection area


def _dc_frame(dc):
    """One counted car found by detection 0; detection 1 (score 0.95) elsewhere, under DontCare box `dc`."""
    return dict(boxes=[[100.0, 100.0, 200.0, 200.0], [400.0, 100.0, 500.0, 200.0]], alphas=[0.5, 0.0],
                scores=np.float32([0.9, 0.95]), gt_boxes=np.float32([[100, 100, 200, 200]]), gt_alpha=np.float32([0.5]),
                dontcare=np.float32(dc).reshape(-1, 4))


def test_dontcare_rule():
    args = lambda fr: (fr['boxes'], fr['alphas'], fr['scores'], fr['gt_boxes'], fr['gt_alpha'], fr['dontcare'], [0], 1, 0.7)
    # fully inside a DontCare box: neither tp nor fp
    tp, fp, fn, s = RI.frame_stats_2d(*args(_dc_frame([[390, 90, 510, 210]])), thresh=np.float32(0.9))
    assert (tp, fp, fn) == (1, 0, 0) and s == 1.0
    # half inside (DontCare overlap 0.5, not > 0.7): still a false positive; without DontCare boxes too
    for dc in ([[450, 90, 600, 210]], np.zeros((0, 4))):
        assert RI.frame_stats_2d(*args(_dc_frame(dc)), thresh=np.float32(0.9))[:3] == (1, 1, 0)
    # a detection below the threshold is not counted at all
    assert RI.frame_stats_2d(*args(_dc_frame(np.zeros((0, 4)))), thresh=np.float32(0.92))[:3] == (0, 1, 1)


def test_camera_box_fit_on_golden_labels():
    g = golden("kitti_label")
    n = 0
    for i in range(int(g["n_frames"])):
        calib = g["calib_%d" % i]
        for cnr, lwh, xyz, ry in zip(g["ann%d_boxes_corners" % i], g["ann%d_lwh" % i], g["ann%d_xyz" % i], g["ann%d_ry" % i]):
            h, w, l, x, y, z, fry, _ = RI.camera_box(cnr, calib)
            assert np.allclose([h, w, l], [lwh[2], lwh[1], lwh[0]], atol=1e-3) and np.allclose([x, y, z], xyz, atol=1e-3)
            assert _angle_diff(fry, ry) < 1e-5
            n += 1
    assert n == 14


def _found_split():
    """A synthetic split whose detections are copies of the objects' corners (image boxes and alphas from the restatement),
    plus the scattered ones: every copy matches its object in 2D."""
    dets, gts, calibs = synth.kitti_eval_split_2d(3, F=12, D=14, G=6, K=2)
    for d, g, c in zip(dets, gts, calibs):
        k = len(g['corners'])
        d[:k, :24] = g['corners']
        g['boxes'] = np.float32([RI.image_box(x, c) for x in g['corners']])
        g['alpha'] = np.float32([RI.camera_box(x, c)[7] for x in g['corners']])
        g['cls'][:] = CAR
    return dets, gts, calibs


def test_aos_equals_ap_when_alphas_agree():
    dets, gts, calibs = _found_split()
    frames = RI.frames_from(dets, gts, calibs)
    for fr in frames:
        fr['alphas'] = [float(np.float32(0.25))] * len(fr['boxes'])
        fr['gt_alpha'] = np.full(len(fr['gt_boxes']), 0.25, np.float32)
    out = RI.evaluate_2d(frames, CAR, VAN, 0.7)
    for d in range(3):
        assert out['ap'][d] > 0 and out['aos'][d] == pytest.approx(out['ap'][d], abs=1e-12)


def test_heading_flip_zeroes_aos_and_keeps_ap():
    dets, gts, calibs = _found_split()
    base = RI.evaluate_2d(RI.frames_from(dets, gts, calibs), CAR, VAN, 0.7)
    flipped = [np.hstack([np.stack([_flip(x[:24]) for x in d]), d[:, 24:]]).astype(np.float32) for d in dets]
    for d, f, c in zip(dets, flipped, calibs):
        for x, y in zip(d, f):
            assert RI.image_box(x[:24], c) == RI.image_box(y[:24], c)
    out = RI.evaluate_2d(RI.frames_from(flipped, gts, calibs), CAR, VAN, 0.7)
    for d in range(3):
        assert base['ap'][d] > 0 and out['ap'][d] == base['ap'][d]
        assert np.array_equal(out['counts'][d], base['counts'][d])
        assert base['aos'][d] == pytest.approx(base['ap'][d], abs=1e-6)
        assert out['aos'][d] == pytest.approx(0.0, abs=1e-9)


def test_product_aos_arithmetic_and_table():
    from mv3d_tf_amd.datasets import kitti_eval as KE
    counts = np.array([[1, 1, 3], [2, 1, 2]])
    sims = [0.5, 1.5]
    aos, curve = KE.orientation_similarity(counts, sims, 2, 11)
    assert curve[0] == curve[1] == 0.5 and curve[2] == 0 and aos == pytest.approx(RI.aos_from_counts(counts, sims, 11), abs=1e-15)
    assert KE.orientation_similarity(counts, sims, 2, 40)[0] == pytest.approx(RI.aos_from_counts(counts, sims, 40), abs=1e-15)
    res = KE.EvalResult()
    for m in ('2d', 'aos'):
        for d in KE.DIFFICULTIES:
            res[('Car', m, d)] = 50.0
    assert res.table().splitlines()[1:] == ['AP_2D         50.00    50.00    50.00', 'AOS           50.00    50.00    50.00']
    assert set(res.to_json()) == {'Car/%s/%s' % (m, d) for m in ('2d', 'aos') for d in KE.DIFFICULTIES}
    with pytest.raises(ValueError):
        KE._check_metrics(('bev', 'ap2d'))


# ------------------------------------------------------------------ ABI argument validation (CPU, no device call)
def test_abi_rejects_bad_arguments():
    from mv3d_tf_amd import _lib, build
    build.build()
    L = _lib.lib()
    A = 4096                                                         # non-NULL fake device pointer, never dereferenced
    det_off, gt_off = np.int32([0, 2, 5]), np.int32([0, 1, 3])
    s = _lib.KittiSplit(2, 5, 3, 375, det_off.ctypes.data, gt_off.ctypes.data, A, A, A, A, A, A, A)
    bad = _lib.ERR_INVALID_ARG

    def image(dc_off, K=None, shape=A, gt_box=A):
        dc_off = np.ascontiguousarray(dc_off, np.int32)
        im = _lib.KittiImageSplit(dc_off[-1] if K is None else K, 0, dc_off.ctypes.data, A, gt_box, A, A, shape)
        im._keep = dc_off
        return im

    def calls(sp, im):
        return (L.mv3d_kitti_eval_image_boxes(C.byref(sp), C.byref(im), A, A, None),
                L.mv3d_kitti_eval_match_2d(C.byref(sp), C.byref(im), A, 0, 1, 0.7, A, None),
                L.mv3d_kitti_eval_count_2d(C.byref(sp), C.byref(im), A, A, 0, 1, 0.7, A, A, A, A, None))
    assert L.mv3d_kitti_eval_image_boxes(C.byref(s), None, A, A, None) == bad
    assert L.mv3d_kitti_eval_match_2d(None, C.byref(image([0, 1, 1])), A, 0, 1, 0.7, A, None) == bad
    assert calls(s, image([0, 2, 1])) == (bad,) * 3                                   # dc_off not monotone
    assert calls(s, image([1, 1, 2])) == (bad,) * 3                                   # dc_off[0] != 0
    assert calls(s, image([0, 1, 2], K=3)) == (bad,) * 3                              # dc_off does not end at num_dontcare
    assert calls(s, image([0, 1, 2], shape=None)) == (bad,) * 3                       # NULL image shapes
    assert calls(s, image([0, 1, 2], gt_box=None)) == (bad,) * 3                      # NULL label boxes
    big_off = np.int32([0, 3000])
    big = _lib.KittiSplit(1, 3000, 1, 375, big_off.ctypes.data, np.int32([0, 1]).ctypes.data, A, A, A, A, A, A, A)
    big._keep = big_off
    assert calls(big, image([0, 0])) == (bad,) * 3                                    # more than MV3D_KITTI_MAX_DETS detections
    im = image([0, 1, 2])
    assert L.mv3d_kitti_eval_image_boxes(C.byref(s), C.byref(im), None, A, None) == bad
    assert L.mv3d_kitti_eval_match_2d(C.byref(s), C.byref(im), A, 0, 1, -0.5, A, None) == bad
    assert L.mv3d_kitti_eval_match_2d(C.byref(s), C.byref(im), A, 0, 1, float('nan'), A, None) == bad
    assert L.mv3d_kitti_eval_count_2d(C.byref(s), C.byref(im), A, A, 0, 1, 0.7, A, A, A, None, None) == bad
    assert L.mv3d_kitti_eval_count_2d(C.byref(s), C.byref(im), A, None, 0, 1, 0.7, A, A, A, A, None) == bad


# ------------------------------------------------------------------ device (MI355X)
def _cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    return torch


def _odd_split(seed, F, D, G, K):
    """The synthetic 2D split plus detections the image box cannot be formed for (NaN, behind the camera) and frames of
    other image shapes."""
    dets, gts, calibs = synth.kitti_eval_split_2d(seed, F=F, D=D, G=G, K=K)
    rng = np.random.RandomState(seed)
    for d in dets[::3]:
        d[-1, rng.randint(24)] = np.nan
        d[-2, :8] = -d[-2, :8]                                   # LIDAR x < 0: behind the camera
    shapes = np.tile(np.int32([375, 1242]), (F, 1))
    shapes[1::4] = (370, 1224)
    return dets, gts, calibs, shapes


def _device_2d(dets, gts, calibs, shapes):
    import torch
    from mv3d_tf_amd import ops
    from mv3d_tf_amd.datasets import kitti_eval as KE
    det = np.concatenate(dets)
    det_off = np.concatenate([[0], np.cumsum([len(d) for d in dets])]).astype(np.int32)
    gt_off = np.concatenate([[0], np.cumsum([len(g['cls']) for g in gts])]).astype(np.int32)
    attr = np.concatenate([np.stack([g['truncation'], g['occlusion'], g['boxes'][:, 1], g['boxes'][:, 3]], 1).reshape(-1, 4) for g in gts])
    dev = torch.device('cuda', 0)
    sp = ops.KittiEvalSplit(det[:, :24], det[:, 24], det_off, np.asarray(calibs, np.float32), np.concatenate([g['corners'] for g in gts]),
                            gt_off, np.concatenate([g['cls'] for g in gts]), attr, dev)
    dc_off = np.concatenate([[0], np.cumsum([len(g['dontcare']) for g in gts])]).astype(np.int32)
    im = ops.KittiImageSplit(sp, np.concatenate([g['boxes'] for g in gts]), np.concatenate([g['alpha'] for g in gts]), dc_off,
                             np.concatenate([g['dontcare'] for g in gts]), shapes)
    return sp, im, det, det_off, KE


@pytest.mark.gpu
def test_device_image_and_camera_boxes_equal_restatement():
    _cuda()
    from mv3d_tf_amd import ops
    dets, gts, calibs, shapes = _odd_split(21, 30, 40, 8, 3)
    sp, im, det, det_off, KE = _device_2d(dets, gts, calibs, shapes)
    box, cam = (t.cpu().numpy() for t in ops.kitti_eval_image_boxes(sp, im))
    f_of = np.searchsorted(det_off, np.arange(len(det)), side='right') - 1
    want_box = np.array([RI.image_box(x[:24], calibs[f], shapes[f]) for x, f in zip(det, f_of)])
    want_cam = np.array([RI.camera_box(x[:24], calibs[f]) for x, f in zip(det, f_of)])
    assert np.array_equal(box, want_box)
    assert np.array_equal(cam[:, :6], want_cam[:, :6], equal_nan=True)
    fin = np.isfinite(want_cam[:, 6])
    assert np.array_equal(np.isfinite(cam[:, 6:]), np.isfinite(want_cam[:, 6:]))
    assert (_angle_diff(cam[fin, 6:], want_cam[fin, 6:]) <= 1e-12).all()
    assert (box == 0).all(1).sum() >= 20 and ((box[:, 0] == 0) & (box[:, 2] > 0)).any() and (box[:, 2] == 1241).any()
    assert (box[:, 2] == 1223).any()
    # detection_boxes: the same values per frame
    boxes, cams = KE.detection_boxes(dets, calibs, shapes)
    assert np.array_equal(np.concatenate(boxes), box) and np.array_equal(np.concatenate(cams), cam, equal_nan=True)


@pytest.mark.gpu
def test_device_2d_statistics_equal_restatement():
    torch = _cuda()
    from mv3d_tf_amd import ops
    dets, gts, calibs, shapes = _odd_split(22, 40, 30, 8, 3)
    sp, im, det, det_off, KE = _device_2d(dets, gts, calibs, shapes)
    want = RI.evaluate_2d(RI.frames_from(dets, gts, calibs, shapes), CAR, VAN, 0.7)
    box, cam = ops.kitti_eval_image_boxes(sp, im)
    matched = ops.kitti_eval_match_2d(sp, im, box, CAR, VAN, 0.7).cpu().numpy()
    thr = np.zeros((3, 41), np.float32)
    nthr = np.zeros(3, np.int32)
    for d in range(3):
        assert np.array_equal(matched[d], np.concatenate(want['matched'][d]))
        t = want['thresholds'][d]
        thr[d, :len(t)], nthr[d] = t, len(t)
    assert nthr.min() > 5
    d_thr, d_nthr = ops.upload_packed([thr, nthr], torch.device('cuda', 0))
    counts, sim = ops.kitti_eval_count_2d(sp, im, box, cam, CAR, VAN, 0.7, d_thr, d_nthr)
    counts, sim = counts.cpu().numpy(), sim.cpu().numpy()
    res = KE.evaluate(dets, gts, calibs, metrics=('2d', 'aos'), image_shapes=shapes)
    assert set(res) == {('Car', m, d) for m in ('2d', 'aos') for d in KE.DIFFICULTIES}
    for d, dn in enumerate(KE.DIFFICULTIES):
        n = nthr[d]
        assert np.array_equal(counts[d, :n], want['counts'][d]) and not counts[d, n:].any()
        assert np.abs(sim[:, d, :n] - want['sim'][d]).max() <= 1e-12 and not sim[:, d, n:].any()
        assert res[('Car', '2d', dn)] == pytest.approx(want['ap'][d], abs=1e-9)
        assert res[('Car', 'aos', dn)] == pytest.approx(want['aos'][d], abs=1e-9)
        assert np.array_equal(res.counts[('Car', '2d', dn)], counts[d])
    # the scene has DontCare-covered false positives and flipped headings: AOS below AP_2D
    assert 0 < res[('Car', 'aos', 'moderate')] < res[('Car', '2d', 'moderate')]


@pytest.mark.gpu
def test_device_full_size_2d_split_deterministic():
    _cuda()
    from mv3d_tf_amd.datasets import kitti_eval as KE
    dets, gts, calibs = synth.kitti_eval_split_2d(7, F=3769, D=300, G=10, K=3)
    a = KE.evaluate(dets, gts, calibs, metrics=('2d', 'aos'))
    b = KE.evaluate(dets, gts, calibs, metrics=('2d', 'aos'))
    for k in a:
        assert np.array_equal(a.counts[k], b.counts[k]) and a[k] == b[k]
        assert 0.0 <= a[k] <= 100.0
    assert a[('Car', '2d', 'hard')] > a[('Car', 'aos', 'hard')] > 0.0


@pytest.mark.gpu
def test_test_net_reports_2d_and_aos(tmp_path, monkeypatch):
    _cuda()
    from test_kitti_eval import _tree
    from mv3d_tf_amd.datasets import kitti_mv3d, load_kitti_calib, pack_calib
    from mv3d_tf_amd.datasets import kitti_eval as KE
    from mv3d_tf_amd.fast_rcnn import test_mv
    from mv3d_tf_amd.fast_rcnn.config import cfg
    root, n = _tree(tmp_path, golden("kitti_label"))
    db = kitti_mv3d("val", root)
    roidb = db.gt_roidb()
    # the fixture's label image boxes are not the projections of its 3D boxes; the last frame's car gets its own projection
    # (and the matching alpha) as label box, so that one car is found in 2D (an easy one: unoccluded, over 40 px)
    last = os.path.join(root, "object/training/label_2/%06d.txt" % (n - 1))
    cal = pack_calib(load_kitti_calib(os.path.join(root, "object/training/calib/%06d.txt" % (n - 1))))
    b = RI.image_box(roidb[n - 1]['boxes_corners'][0], cal)
    alpha = RI.camera_box(roidb[n - 1]['boxes_corners'][0], cal)[7]
    rows = open(last).read().splitlines()
    t = rows[0].split()
    t[3:8] = ['%.2f' % v for v in [alpha] + b]
    assert b[3] - b[1] > 40
    with open(last, 'w') as f:
        f.write('\n'.join([' '.join(t)] + rows[1:]) + '\n')
    gts, calibs = [], []
    for i in range(n):
        cal = load_kitti_calib(os.path.join(root, "object/training/calib/%06d.txt" % i))
        with open(os.path.join(root, "object/training/label_2/%06d.txt" % i)) as f:
            gts.append(KE.load_eval_labels(f.readlines(), cal))
        calibs.append(pack_calib(cal))
    assert sum(len(g['dontcare']) for g in gts) >= 1 and all(len(g['alpha']) == len(g['cls']) for g in gts)

    def fake_box_detect(sess, net, im, bv, calib, boxes=None):
        ann = roidb[int(bv[0, 0, 0])]
        R_ = len(ann['gt_classes'])
        scores = np.stack([np.full(R_, 0.1), np.linspace(0.9, 0.6, R_)], 1).astype(np.float32).reshape(R_, 2)
        bvb = np.tile(ann['boxes_bv'].astype(np.float64), (1, 2)).reshape(R_, 8)
        cnr = np.tile(ann['boxes_corners'], (1, 2)).reshape(R_, 48)
        return scores, bvb, cnr, cnr
    monkeypatch.setattr(test_mv, "box_detect", fake_box_detect)
    saved_root, saved_metrics = cfg.ROOT_DIR, cfg.TEST.KITTI_EVAL_METRICS
    cfg.ROOT_DIR = str(tmp_path)
    try:
        all_boxes, all_cnr = test_mv.test_net(None, None, db, "w")
        out = os.path.join(str(tmp_path), "output", cfg.EXP_DIR, db.name, "w")
        default = db.evaluate_detections(all_boxes, all_cnr, out)
        cfg.TEST.KITTI_EVAL_METRICS = ('bev', '3d', '2d', 'aos')
        res = db.evaluate_detections(all_boxes, all_cnr, out)
    finally:
        cfg.ROOT_DIR, cfg.TEST.KITTI_EVAL_METRICS = saved_root, saved_metrics
    assert set(res) == {("Car", m, d) for m in KE.ALL_METRICS for d in KE.DIFFICULTIES}
    for k in default:
        assert res[k] == default[k] and np.array_equal(res.counts[k], default.counts[k])
    assert 'AP_2D' in res.table() and 'AOS' in res.table() and 'AP_2D' not in default.table()
    dets = [np.asarray(all_cnr[1][i], np.float32).reshape(-1, 25) for i in range(n)]
    want = RI.evaluate_2d(RI.frames_from(dets, gts, calibs), KE.CLASS_CODES['Car'], KE.CLASS_CODES['Van'], 0.7)
    for di, dn in enumerate(KE.DIFFICULTIES):
        assert res[("Car", "2d", dn)] == pytest.approx(want['ap'][di], abs=1e-9)
        assert res[("Car", "aos", dn)] == pytest.approx(want['aos'][di], abs=1e-9)
    # the rewritten car is found in 2D with its own heading (the alpha in the label is rounded to 0.01 rad): AOS ~ AP_2D
    assert res.counts[("Car", "2d", "easy")][0][0] == 1 and res[("Car", "2d", "easy")] > 0
    assert res[("Car", "aos", "easy")] == pytest.approx(res[("Car", "2d", "easy")], rel=1e-4)


@pytest.mark.gpu
def test_write_results_parse_back(tmp_path):
    _cuda()
    from mv3d_tf_amd.datasets import kitti_eval as KE
    dets, gts, calibs = synth.kitti_eval_split_2d(5, F=6, D=12, G=4, K=1)
    names = ["%06d" % i for i in range(6)]
    KE.write_results(names, dets, calibs, str(tmp_path))
    boxes, cams = KE.detection_boxes(dets, calibs)
    for f, name in enumerate(names):
        lines = open(os.path.join(str(tmp_path), name + ".txt")).read().splitlines()
        assert len(lines) == len(dets[f])
        for ln, b, k, d in zip(lines, boxes[f], cams[f], dets[f]):
            t = ln.split()
            assert t[:3] == ['Car', '-1', '-1'] and len(t) == 16
            v = np.array(t[3:15], np.float64)
            want = np.concatenate([[k[7]], b, k[:7]])
            assert np.array_equal(v, np.array(['%.2f' % x for x in want], np.float64))
            assert float(t[15]) == pytest.approx(float(d[24]), abs=1e-6)
