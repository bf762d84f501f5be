"""KITTI evaluation (csrc/kitti_eval.hip, mv3d_tf_amd/datasets/kitti_eval.py): AP_BEV / AP_3D on the device.

CPU tests pin the plain-Python restatement (tests/kitti_eval_restatement.py) against closed forms, a Monte-Carlo estimate and
hand-computed AP cases, and check the C-ABI's argument validation.  `gpu` tests compare the device overlaps, heights and
statistics with the restatement bit for bit and run test_net -> kitti_mv3d.evaluate_detections end to end."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import kitti_eval_restatement as R
from conftest import golden
from mv3d_tf_amd import synth


def _box(cx, cy, l, w, yaw=0.0, z0=-1.7, h=1.5):
    return synth.box_corners([[cx, cy, z0]], [[l, w, h]], [[math.cos(yaw), math.sin(yaw)]])[0]


# ------------------------------------------------------------------ IoU analytic cases (CPU)
def test_iou_identical_and_axis_aligned():
    rng = np.random.RandomState(0)
    for _ in range(50):
        b = _box(*rng.uniform([5, -10, 2, 1], [50, 10, 6, 3]), yaw=rng.uniform(-3, 3))
        assert R.iou_pair(b, b) == (1.0, 1.0)
    for _ in range(200):
        x1, y1, x2, y2 = rng.uniform(-5, 5, 4)
        l1, w1, l2, w2 = rng.uniform(0.5, 4, 4)
        z1, h1, z2, h2 = rng.uniform(-2, 0, 1)[0], rng.uniform(0.5, 2), rng.uniform(-2, 0), rng.uniform(0.5, 2)
        a, b = _box(x1, y1, l1, w1, z0=z1, h=h1), _box(x2, y2, l2, w2, z0=z2, h=h2)
        fa, fb = a.astype(np.float64), b.astype(np.float64)
        ix = max(0.0, min(fa[:8].max(), fb[:8].max()) - max(fa[:8].min(), fb[:8].min()))
        iy = max(0.0, min(fa[8:16].max(), fb[8:16].max()) - max(fa[8:16].min(), fb[8:16].min()))
        iz = max(0.0, min(fa[16:].max(), fb[16:].max()) - max(fa[16:].min(), fb[16:].min()))
        area = lambda c: (c[:8].max() - c[:8].min()) * (c[8:16].max() - c[8:16].min())
        hgt = lambda c: c[16:].max() - c[16:].min()
        bev, b3 = R.iou_pair(a, b)
        assert abs(bev - ix * iy / (area(fa) + area(fb) - ix * iy)) < 1e-12
        vi = ix * iy * iz
        assert abs(b3 - vi / (area(fa) * hgt(fa) + area(fb) * hgt(fb) - vi)) < 1e-12


def test_iou_rotated_square_and_invariance():
    sq, rot = _box(0, 0, 2, 2), _box(0, 0, 2, 2, yaw=math.pi / 4)
    want = (2 * math.sqrt(2) - 2) / (4 - 2 * math.sqrt(2))
    for a, b in ((sq, rot), (rot, sq)):
        bev, b3 = R.iou_pair(a, b)
        assert abs(bev - want) < 1e-12 and abs(b3 - want) < 1e-12
    rng = np.random.RandomState(1)
    for _ in range(100):
        p = rng.uniform([-3, -3, 1, 1, -3], [3, 3, 5, 3, 3])
        q = rng.uniform([-3, -3, 1, 1, -3], [3, 3, 5, 3, 3])
        a, b = _box(*p[:4], yaw=p[4]), _box(*q[:4], yaw=q[4])
        ab, ba = R.iou_pair(a, b), R.iou_pair(b, a)
        assert abs(ab[0] - ba[0]) < 1e-12 and abs(ab[1] - ba[1]) < 1e-12
        t, d = rng.uniform(-3, 3), rng.uniform(-5, 5, 2)
        a2 = _box(p[0] * math.cos(t) - p[1] * math.sin(t) + d[0], p[0] * math.sin(t) + p[1] * math.cos(t) + d[1], p[2], p[3], yaw=p[4] + t)
        b2 = _box(q[0] * math.cos(t) - q[1] * math.sin(t) + d[0], q[0] * math.sin(t) + q[1] * math.cos(t) + d[1], q[2], q[3], yaw=q[4] + t)
        moved = R.iou_pair(a2, b2)
        # (the corners are f32: a moved box is the same box only to ~1e-7 relative, which bounds the comparison)
        assert abs(moved[0] - ab[0]) < 1e-5 and abs(moved[1] - ab[1]) < 1e-5
    # exact invariance where the f32 corners move exactly: rectangles on a 1/8 grid (edges along (3, 4) and (-4, 3)),
    # translated by (8, -4), rotated by 90 and 180 degrees
    def quad(bx, by, s, t):
        e1, e2 = (3 * s, 4 * s), (-4 * t, 3 * t)
        x = [bx, bx + e1[0], bx + e1[0] + e2[0], bx + e2[0]]
        y = [by, by + e1[1], by + e1[1] + e2[1], by + e2[1]]
        return np.array(x * 2 + y * 2 + [-1.5] * 4 + [0.25] * 4, np.float32)
    a, b = quad(1.0, 0.5, 0.5, 0.25), quad(1.5, 0.25, 0.375, 0.5)
    ab = R.iou_pair(a, b)
    assert 0 < ab[0] < 1
    sh = lambda c: np.concatenate([c[:8] + 8.0, c[8:16] - 4.0, c[16:]]).astype(np.float32)
    r90 = lambda c: np.concatenate([-c[8:16], c[:8], c[16:]]).astype(np.float32)
    r180 = lambda c: np.concatenate([-c[:8], -c[8:16], c[16:]]).astype(np.float32)
    for f in (sh, r90, r180):
        m = R.iou_pair(f(a), f(b))
        assert abs(m[0] - ab[0]) < 1e-12 and abs(m[1] - ab[1]) < 1e-12


def test_iou_monte_carlo():
    rng = np.random.RandomState(2)
    for _ in range(6):
        a = _box(0, 0, rng.uniform(2, 4), rng.uniform(1, 2), yaw=rng.uniform(-3, 3))
        b = _box(rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 4), rng.uniform(1, 2), yaw=rng.uniform(-3, 3))
        pts = rng.uniform(-4, 4, (200000, 2))

        def inside(c, p):
            x, y = c[:4].astype(np.float64), c[8:12].astype(np.float64)
            s = np.ones(len(p), bool)
            sg = np.sign(np.sum([x[k] * y[(k + 1) % 4] - x[(k + 1) % 4] * y[k] for k in range(4)]))
            for k in range(4):
                n = (k + 1) % 4
                s &= sg * ((x[n] - x[k]) * (p[:, 1] - y[k]) - (y[n] - y[k]) * (p[:, 0] - x[k])) >= 0
            return s
        ia, ib = inside(a, pts), inside(b, pts)
        union = (ia | ib).sum()
        assert abs(R.iou_pair(a, b)[0] - (ia & ib).sum() / union) < 1e-2


def test_iou_degenerate():
    a = _box(0, 0, 3, 2)
    assert R.iou_pair(a, _box(0, 0, 3, 2, h=0.0)) == (1.0, 0.0)
    flat = _box(0, 0, 3, 2, h=0.0)
    assert R.iou_pair(flat, flat)[1] == 0.0
    nan = a.copy()
    nan[3] = np.nan
    assert R.iou_pair(a, nan) == (0.0, 0.0) and R.iou_pair(nan, a) == (0.0, 0.0)
    assert R.iou_pair(a, np.zeros(24, np.float32)) == (0.0, 0.0)


def test_restated_projection_matches_the_pinned_matrices():
    g = golden("proj_matrix")
    for c, m in zip(g["calibs"][:16], g["mats"][:16]):
        assert np.array_equal(R.proj_matrix(c), m.reshape(12))


# ------------------------------------------------------------------ AP semantics on hand-built frames (CPU)
CAR, VAN, TRUCK = 0, 1, 2


def _frame(gt, dets, classes=None, occ=None, heights=None, gt_h=50.0):
    """gt / dets: lists of corner boxes; dets as (box, score)."""
    G, D = len(gt), len(dets)
    iou = [np.zeros((D, G)), np.zeros((D, G))]
    for j, (b, _) in enumerate(dets):
        for g, c in enumerate(gt):
            iou[0][j, g], iou[1][j, g] = R.iou_pair(b, c)
    return {'iou': iou, 'scores': np.array([s for _, s in dets], np.float32),
            'heights': np.full(D, 60.0) if heights is None else np.asarray(heights, np.float64),
            'cls': [CAR] * G if classes is None else classes, 'trunc': [0.0] * G, 'occ': [0] * G if occ is None else occ,
            'y1': [100.0] * G, 'y2': [100.0 + gt_h] * G}


def _ap(frames, rp=11):
    return R.evaluate(frames, CAR, VAN, 0.7, rp)


def test_ap_perfect_and_half_recall():
    # 100 cars over 10 frames, all found: 41 thresholds, precision 1 at each -> 100 with 11 and with 40 points
    frames = []
    for f in range(10):
        cars = [_box(8 + 5 * i, 4 * (f % 3), 4, 1.8) for i in range(10)]
        frames.append(_frame(cars, [(c, np.float32(0.99 - 0.0097 * (10 * f + i))) for i, c in enumerate(cars)]))
    for rp in (11, 40):
        o = _ap(frames, rp)
        assert all(o['ap'][m][d] == 100.0 for m in range(2) for d in range(3))
        assert len(o['thresholds'][0][0]) == 41 and o['counts'][1][2][-1].tolist() == [100, 0, 0]
    # 4 cars, two found (scores 0.9, 0.8), one false positive scoring 0.95: thresholds [0.9, 0.8];
    # precision at them 1/2 and 2/3 -> running max [2/3, 2/3, 0, ...]: 11 points (2/3) / 11, 40 points (2/3) / 40
    # (with fewer than 40 objects the devkit's threshold list is short, so even perfect detections score below 100)
    cars = [_box(10 + 6 * i, 0, 4, 1.8) for i in range(4)]
    fpbox = _box(40, 15, 4, 1.8)
    o11 = _ap([_frame(cars, [(fpbox, 0.95), (cars[0], 0.9), (cars[1], 0.8)])], 11)
    o40 = _ap([_frame(cars, [(fpbox, 0.95), (cars[0], 0.9), (cars[1], 0.8)])], 40)
    assert o11['thresholds'][0][0].tolist() == [np.float32(0.9), np.float32(0.8)]
    assert o11['counts'][0][0].tolist() == [[1, 1, 3], [2, 1, 2]]
    assert abs(o11['ap'][0][0] - (2 / 3) / 11 * 100) < 1e-12 and abs(o40['ap'][0][0] - (2 / 3) / 40 * 100) < 1e-12


def test_ap_neighbour_class_small_detection_and_occlusion():
    car, van, truck = _box(10, 0, 4, 1.8), _box(20, 5, 4.5, 2), _box(30, -5, 6, 2.5)
    one = 100.0 / 11                                                   # one threshold, precision 1 there
    # a Car detection on a Van consumes the detection and counts nothing; on a Truck it is a false positive
    o = _ap([_frame([car, van], [(car, 0.9), (van, 0.95)], classes=[CAR, VAN])])
    assert o['counts'][0][1].tolist() == [[1, 0, 0]] and abs(o['ap'][0][1] - one) < 1e-12
    o = _ap([_frame([car, truck], [(car, 0.9), (truck, 0.95)], classes=[CAR, TRUCK])])
    assert o['counts'][0][1].tolist() == [[1, 1, 0]] and abs(o['ap'][0][1] - one / 2) < 1e-12
    # a detection under 25 px is ignored in moderate (not a false positive), at 30 px it counts
    stray = _box(40, 15, 4, 1.8)
    o = _ap([_frame([car], [(car, 0.9), (stray, 0.95)], heights=[60.0, 20.0])])
    assert o['counts'][0][1].tolist() == [[1, 0, 0]] and abs(o['ap'][0][1] - one) < 1e-12
    o = _ap([_frame([car], [(car, 0.9), (stray, 0.95)], heights=[60.0, 30.0])])
    assert o['counts'][0][1].tolist() == [[1, 1, 0]] and abs(o['ap'][0][1] - one / 2) < 1e-12
    # an occlusion-1 car is ignored in easy but counted (and missed) in moderate
    car2 = _box(25, -8, 4, 1.8)
    o = _ap([_frame([car, car2], [(car, 0.9)], occ=[0, 1])])
    assert o['counts'][0][0].tolist() == [[1, 0, 0]] and o['counts'][0][1].tolist() == [[1, 0, 1]]
    assert abs(o['ap'][0][0] - one) < 1e-12 and abs(o['ap'][0][1] - one) < 1e-12
    assert R.evaluate([_frame([car, car2], [(car, 0.9)], occ=[0, 1])], CAR, VAN, 0.7, 40)['ap'][0][1] == 0.0


def test_get_thresholds_hand_example():
    from mv3d_tf_amd.datasets import kitti_eval as KE
    v = np.linspace(1.0, 0.005, 200).astype(np.float32)
    want = v[[0] + [5 * k - 1 for k in range(1, 41)]]                  # recall (i+1)/200 nearest to k/40: i = 5k - 1
    assert np.array_equal(R.get_thresholds(v, 200), want) and np.array_equal(KE.get_thresholds(v[::-1], 200), want)
    assert R.get_thresholds(np.float32([0.9, 0.8, 0.7]), 3).tolist() == np.float32([0.9, 0.8, 0.7]).tolist()
    # the product's AP arithmetic == the restatement's on the hand case above
    ap, prec, _ = KE.average_precision(np.array([[1, 1, 3], [2, 1, 2]]), 2, 11)
    assert abs(ap - (2 / 3) / 11 * 100) < 1e-12 and prec[0] == prec[1] == 2 / 3 and prec[2] == 0


# ------------------------------------------------------------------ ABI argument validation (CPU, no device call)
def test_abi_rejects_bad_arguments():
    from mv3d_tf_amd import _lib, build
    build.build()
    L = _lib.lib()
    A = 4096                                                         # non-NULL fake device pointer, never dereferenced
    def split(det_off, gt_off, N=None, G=None, F=None, img_h=375, offs=A):
        det_off, gt_off = np.ascontiguousarray(det_off, np.int32), np.ascontiguousarray(gt_off, np.int32)
        s = _lib.KittiSplit(len(det_off) - 1 if F is None else F, det_off[-1] if N is None else N, gt_off[-1] if G is None else G,
                            img_h, det_off.ctypes.data, gt_off.ctypes.data, offs, A, A, A, A, A, A)
        s._keep = (det_off, gt_off)
        return s
    bad = _lib.ERR_INVALID_ARG
    ok_args = lambda s, P: (L.mv3d_kitti_eval_overlaps(C.byref(s), P, A, A, None),
                            L.mv3d_kitti_eval_match(C.byref(s), P, A, A, 0, 1, 0.7, A, None),
                            L.mv3d_kitti_eval_count(C.byref(s), P, A, A, 0, 1, 0.7, A, A, A, None))
    assert L.mv3d_kitti_eval_overlaps(None, 0, A, A, None) == bad
    assert ok_args(split([0, 2, 5], [0, 1, 3], F=-1), 8) == (bad,) * 3                   # negative count
    assert ok_args(split([0, 3, 2, 5], [0, 1, 2, 3]), 6) == (bad,) * 3                 # det_off not monotone
    assert ok_args(split([0, 2, 5], [0, 1, 3]), 9) == (bad,) * 3                       # pairs != sum D_f G_f (2*1 + 3*2 = 8)
    assert ok_args(split([0, 2, 5], [0, 1, 3], N=6), 8) == (bad,) * 3                  # det_off does not end at num_dets
    assert ok_args(split([0, 2, 5], [0, 1, 3], offs=None), 8) == (bad,) * 3            # NULL device offsets
    assert ok_args(split([1, 2, 5], [0, 1, 3]), 8) == (bad,) * 3                       # det_off[0] != 0
    assert ok_args(split([0, 3000], [0, 1]), 3000) == (bad,) * 3                       # more than MV3D_KITTI_MAX_DETS in a frame
    s = split([0, 2, 5], [0, 1, 3])
    assert L.mv3d_kitti_eval_overlaps(C.byref(s), 8, None, A, None) == bad
    assert L.mv3d_kitti_eval_overlaps(C.byref(split([0, 2, 5], [0, 1, 3], img_h=0)), 8, A, A, None) == bad
    assert L.mv3d_kitti_eval_match(C.byref(s), 8, A, A, 0, 1, -0.5, A, None) == bad
    assert L.mv3d_kitti_eval_match(C.byref(s), 8, A, A, 0, 1, float('nan'), A, None) == bad
    assert L.mv3d_kitti_eval_count(C.byref(s), 8, A, A, 0, 1, 0.7, None, A, A, None) == bad
    assert L.mv3d_kitti_eval_count(C.byref(s), 8, A, A, 0, 1, 0.7, A, A, None, None) == bad


# ------------------------------------------------------------------ device (MI355X)
def _cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    return torch


def _calib_dict():
    from mv3d_tf_amd.datasets import load_kitti_calib
    import tempfile
    with tempfile.NamedTemporaryFile('w', suffix='.txt', delete=False) as f:
        f.write(str(golden("kitti_label")["calib_txt_0"]))
    try:
        return load_kitti_calib(f.name)
    finally:
        os.unlink(f.name)


def _label_lines(rng, G):
    types = rng.choice(['Car', 'Car', 'Car', 'Van', 'Pedestrian', 'Misc'], G)
    lines = []
    for t in types:
        y1 = rng.uniform(100, 250)
        lines.append("%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (
            t, rng.choice([0.0, 0.15, 0.2, 0.4, 0.6]), rng.randint(0, 4), 0.0, 300.0, y1, 400.0, y1 + rng.uniform(10, 100),
            rng.uniform(1.3, 2.0), rng.uniform(1.4, 2.0), rng.uniform(3.0, 5.0), rng.uniform(-15, 15), rng.uniform(1.4, 1.9),
            rng.uniform(4, 50), rng.uniform(-math.pi, math.pi)))
    return lines


def _dets_for(rng, gt_cnr, D):
    """Detections around a frame's objects: exact copies (shared edges / vertices), regressed-corner jitter, axis-aligned
    boxes, contained boxes, scattered boxes, degenerate and NaN boxes; scores with ties."""
    out = []
    G = len(gt_cnr)
    for j in range(D):
        kind = j % 8
        g = gt_cnr[rng.randint(G)] if G else synth.box_corners([[20, 0, -1.7]], [[4, 2, 1.5]], [[1, 0]])[0]
        if kind == 0:
            c = g.copy()
        elif kind == 1:
            c = g + rng.uniform(-0.3, 0.3, 24).astype(np.float32)
        elif kind == 2:
            x, y = g[:8].astype(np.float64), g[8:16].astype(np.float64)
            c = synth.box_corners([[x.mean(), y.mean(), g[16:].min()]], [[x.max() - x.min(), y.max() - y.min(), g[16:].max() - g[16:].min()]],
                                  [[1.0, 0.0]])[0]
        elif kind == 3:
            ctr = np.concatenate([np.repeat(g[:8].mean(), 8), np.repeat(g[8:16].mean(), 8), np.repeat(g[16:].mean(), 8)])
            c = (ctr + (g - ctr) * 0.6).astype(np.float32)
        elif kind == 4:
            c = synth.box_corners([[rng.uniform(5, 50), rng.uniform(-15, 15), -1.7]], [[4, 1.8, 1.5]],
                                  [[math.cos(rng.uniform(-3, 3)), math.sin(rng.uniform(-3, 3))]])[0]
        elif kind == 5:
            c = np.concatenate([g[:8], g[8:16], np.repeat(g[16], 8)]).astype(np.float32)     # zero height
        elif kind == 6:
            c = np.concatenate([np.repeat(g[0], 8), np.repeat(g[8], 8), g[16:]]).astype(np.float32)  # zero footprint
        else:
            c = g.copy()
            if rng.rand() < 0.5:
                c[rng.randint(24)] = np.nan
            else:
                c = (g + np.float32(rng.uniform(-1, 1))).astype(np.float32)
        out.append(np.append(c, np.float32(rng.choice([0.5, 0.75, rng.rand()]))))
    return np.array(out, np.float32).reshape(D, 25)


def _split(seed, F, D, G):
    from mv3d_tf_amd.datasets.kitti_eval import load_eval_labels
    from mv3d_tf_amd.datasets import pack_calib
    rng = np.random.RandomState(seed)
    cal = _calib_dict()
    gts = [load_eval_labels(_label_lines(rng, G if f % 7 else 0), cal) for f in range(F)]
    dets = [_dets_for(rng, g['corners'], D if f % 11 else 0) for f, g in enumerate(gts)]
    return dets, gts, [pack_calib(cal)] * F


def _device_passes(dets, gts, calibs, cls='Car'):
    import torch
    from mv3d_tf_amd import ops
    from mv3d_tf_amd.datasets import kitti_eval as KE
    det = np.concatenate(dets)
    det_off = np.concatenate([[0], np.cumsum([len(d) for d in dets])]).astype(np.int32)
    gt_off = np.concatenate([[0], np.cumsum([len(g['cls']) for g in gts])]).astype(np.int32)
    attr = np.concatenate([np.stack([g['truncation'], g['occlusion'], g['boxes'][:, 1], g['boxes'][:, 3]], 1).reshape(-1, 4) for g in gts])
    sp = ops.KittiEvalSplit(det[:, :24], det[:, 24], det_off, np.asarray(calibs, np.float32), np.concatenate([g['corners'] for g in gts]),
                            gt_off, np.concatenate([g['cls'] for g in gts]), attr, torch.device('cuda', 0))
    iou, height = ops.kitti_eval_overlaps(sp)
    code, nb = KE.CLASS_CODES[cls], KE.CLASS_CODES[KE.NEIGHBOR[cls]]
    return sp, iou, height, code, nb, det, det_off, gt_off


@pytest.mark.gpu
def test_device_overlaps_bit_identical():
    _cuda()
    dets, gts, calibs = _split(11, 40, 50, 10)
    sp, iou, height, *_ , det, det_off, gt_off = _device_passes(dets, gts, calibs)
    assert sp.num_pairs > 15000
    gt_cnr = np.concatenate([g['corners'] for g in gts])
    bev, b3, hts = R.overlaps(det[:, :24], det_off, gt_cnr, gt_off, np.asarray(calibs, np.float32))
    got = iou.cpu().numpy()
    assert np.array_equal(got[0], bev) and np.array_equal(got[1], b3)
    assert np.array_equal(height.cpu().numpy(), hts)
    assert (bev == 1.0).any() and ((bev > 0) & (bev < 1)).any() and (bev == 0).any() and (hts > 0).any()


@pytest.mark.gpu
def test_device_statistics_equal_restatement():
    torch = _cuda()
    from mv3d_tf_amd import ops
    from mv3d_tf_amd.datasets import kitti_eval as KE
    dets, gts, calibs = _split(12, 60, 40, 8)
    sp, iou, height, code, nb, det, det_off, gt_off = _device_passes(dets, gts, calibs)
    gt_cnr = np.concatenate([g['corners'] for g in gts])
    bev, b3, hts = R.overlaps(det[:, :24], det_off, gt_cnr, gt_off, np.asarray(calibs, np.float32))
    frames = []
    po = 0
    for f, g in enumerate(gts):
        D, G = det_off[f + 1] - det_off[f], gt_off[f + 1] - gt_off[f]
        frames.append({'iou': (bev[po:po + D * G].reshape(D, G), b3[po:po + D * G].reshape(D, G)),
                       'scores': det[det_off[f]:det_off[f + 1], 24], 'heights': hts[det_off[f]:det_off[f + 1]], 'cls': g['cls'],
                       'trunc': g['truncation'], 'occ': g['occlusion'], 'y1': g['boxes'][:, 1], 'y2': g['boxes'][:, 3]})
        po += D * G
    want = R.evaluate(frames, code, nb, 0.7, 11)
    matched = ops.kitti_eval_match(sp, iou, height, code, nb, 0.7).cpu().numpy()
    thr = np.zeros((2, 3, 41), np.float32)
    nthr = np.zeros((2, 3), np.int32)
    for m in range(2):
        for d in range(3):
            assert np.array_equal(matched[m, d], np.concatenate(want['matched'][m][d]))
            t = want['thresholds'][m][d]
            thr[m, d, :len(t)], nthr[m, d] = t, len(t)
    assert nthr.min() > 5
    d_thr, d_nthr = ops.upload_packed([thr, nthr], torch.device('cuda', 0))
    counts = ops.kitti_eval_count(sp, iou, height, code, nb, 0.7, d_thr, d_nthr).cpu().numpy()
    res = KE.evaluate(dets, gts, calibs)
    for m, mn in enumerate(KE.METRICS):
        for d, dn in enumerate(KE.DIFFICULTIES):
            assert np.array_equal(counts[m, d, :nthr[m, d]], want['counts'][m][d]), (m, d)
            assert not counts[m, d, nthr[m, d]:].any()
            assert res[('Car', mn, dn)] == pytest.approx(want['ap'][m][d], abs=1e-9)
            assert np.array_equal(res.counts[('Car', mn, dn)], counts[m, d])


@pytest.mark.gpu
def test_device_full_size_split_deterministic():
    _cuda()
    from mv3d_tf_amd.datasets import kitti_eval as KE
    dets, gts, calibs = synth.kitti_eval_split(7, F=3769, D=300, G=10)
    a = KE.evaluate(dets, gts, calibs)
    b = KE.evaluate(dets, gts, calibs)
    for k in a:
        assert np.array_equal(a.counts[k], b.counts[k]) and a[k] == b[k]
        assert 0.0 <= a[k] <= 100.0
    assert a[('Car', 'bev', 'hard')] > 0.0


# ------------------------------------------------------------------ end to end: test_net -> kitti_mv3d.evaluate_detections
# The fixture's frames hold no easy car (every Car is occluded, truncated or under 40 px in the image), so the tree gets
# one more frame: frame 0's calibration and one unoccluded, untruncated car 45 px tall in the image.
EXTRA_FRAME = "Car 0.00 0 1.85 815.38 149.54 844.45 194.54 1.88 1.88 3.23 1.43 1.93 17.43 -1.35\n" \
              "DontCare 0.25 0 -1.33 842.79 131.87 949.49 166.75 -1 -1 -1 -1000 -1000 -1000 -10\n"


def _tree(tmp_path, g):
    from PIL import Image
    root = tmp_path / "KITTI"
    for sub in ("ImageSets", "object/training/calib", "object/training/label_2", "object/training/image_2",
                "object/training/lidar_bv"):
        os.makedirs(root / sub)
    n = int(g["n_frames"])
    texts = [(str(g["labels_txt_%d" % i]), str(g["calib_txt_%d" % i])) for i in range(n)] + [(EXTRA_FRAME, str(g["calib_txt_0"]))]
    for i, (lab, cal) in enumerate(texts):
        idx = "%06d" % i
        (root / "object/training/label_2" / (idx + ".txt")).write_text(lab)
        (root / "object/training/calib" / (idx + ".txt")).write_text(cal)
        Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(str(root / "object/training/image_2" / (idx + ".png")))
        np.save(root / "object/training/lidar_bv" / (idx + ".npy"), np.full((8, 9, 9), i, np.float32))
    (root / "ImageSets" / "val.txt").write_text("".join("%06d\n" % i for i in range(len(texts))))
    return str(root), len(texts)


@pytest.mark.gpu
def test_test_net_evaluates_a_kitti_tree(tmp_path, monkeypatch):
    torch = _cuda()
    from mv3d_tf_amd.datasets import kitti_mv3d, load_kitti_calib, pack_calib
    from mv3d_tf_amd.datasets import kitti_eval as KE
    from mv3d_tf_amd.fast_rcnn import test_mv
    from mv3d_tf_amd.fast_rcnn.config import cfg
    root, n = _tree(tmp_path, golden("kitti_label"))
    db = kitti_mv3d("val", root)
    roidb = db.gt_roidb()
    gts, calibs = [], []
    for i in range(n):
        cal = load_kitti_calib(os.path.join(root, "object/training/calib/%06d.txt" % i))
        with open(os.path.join(root, "object/training/label_2/%06d.txt" % i)) as f:
            gts.append(KE.load_eval_labels(f.readlines(), cal))
        calibs.append(pack_calib(cal))
    # (CPU restatement) the easy cars project above 40 px, so their detections are not ignored in easy
    easy = 0
    for g, c in zip(gts, calibs):
        M = R.proj_matrix(c)
        for k in np.flatnonzero(KE.gt_flags(g['cls'], g['truncation'], g['occlusion'], g['boxes'][:, 1], g['boxes'][:, 3], 0, 0, 1) == 0):
            assert R.det_height(g['corners'][k], M) > 40
            easy += 1
    assert easy >= 1

    def fake_box_detect(sess, net, im, bv, calib, boxes=None):
        ann = roidb[int(bv[0, 0, 0])]                    # the frame index is the BEV map's value
        R_ = len(ann['gt_classes'])
        scores = np.stack([np.full(R_, 0.1), np.linspace(0.9, 0.6, R_)], 1).astype(np.float32).reshape(R_, 2)
        bvb = np.tile(ann['boxes_bv'].astype(np.float64), (1, 2)).reshape(R_, 8)
        cnr = np.tile(ann['boxes_corners'], (1, 2)).reshape(R_, 48)
        return scores, bvb, cnr, cnr
    monkeypatch.setattr(test_mv, "box_detect", fake_box_detect)
    saved_root = cfg.ROOT_DIR
    cfg.ROOT_DIR = str(tmp_path)
    try:
        all_boxes, all_cnr = test_mv.test_net(None, None, db, "w")
    finally:
        cfg.ROOT_DIR = saved_root
    out = os.path.join(str(tmp_path), "output", cfg.EXP_DIR, db.name, "w")
    res = db.evaluate_detections(all_boxes, all_cnr, out)          # (test_net has called it once already)
    assert isinstance(res, dict) and set(res) == {("Car", m, d) for m in KE.METRICS for d in KE.DIFFICULTIES}
    with open(os.path.join(out, "kitti_ap.json")) as f:
        js = json.load(f)
    assert js == {"Car/%s/%s" % (m, d): res[("Car", m, d)] for m in KE.METRICS for d in KE.DIFFICULTIES}
    for i in range(n):
        lines = open(os.path.join(out, "results", "data", "%06d.txt" % i)).read().splitlines()
        assert len(lines) == len(all_boxes[1][i])
        for ln, d in zip(lines, all_boxes[1][i]):
            assert ln == "car -1 -1 0.00 %.2f %.2f %.2f %.2f -1 -1 -1 -1 -1 -1 -1 -1" % tuple(d[:4])
    # every counted car found, nothing else counted: precision 1 at every threshold (with so few objects the devkit's
    # threshold list is short, so the AP is not 100: one easy car gives 100 / 11)
    for key in res:
        n_thr = len(res.thresholds[key])
        assert n_thr >= 1 and (res.precision[key][:n_thr] == 1.0).all() and res.counts[key][n_thr - 1][1:].tolist() == [0, 0]
    assert res[("Car", "bev", "easy")] == res[("Car", "3d", "easy")] == pytest.approx(100.0 / 11, abs=1e-12)
    # every AP == the restatement's on the same input
    frames = []
    for i, g in enumerate(gts):
        d = np.asarray(all_cnr[1][i], np.float32).reshape(-1, 25)
        M = R.proj_matrix(calibs[i])
        iou = [np.zeros((len(d), len(g['cls']))), np.zeros((len(d), len(g['cls'])))]
        for j in range(len(d)):
            for k in range(len(g['cls'])):
                iou[0][j, k], iou[1][j, k] = R.iou_pair(d[j, :24], g['corners'][k])
        frames.append({'iou': iou, 'scores': d[:, 24], 'heights': [R.det_height(x[:24], M) for x in d], 'cls': g['cls'],
                       'trunc': g['truncation'], 'occ': g['occlusion'], 'y1': g['boxes'][:, 1], 'y2': g['boxes'][:, 3]})
    want = R.evaluate(frames, KE.CLASS_CODES['Car'], KE.CLASS_CODES['Van'], 0.7)
    for m, mn in enumerate(KE.METRICS):
        for di, dn in enumerate(KE.DIFFICULTIES):
            assert res[("Car", mn, dn)] == pytest.approx(want['ap'][m][di], abs=1e-9)
