"""The four statistics-pass kernels of csrc/kitti_eval.hip pinned against the restatements at every path they take: one,
two, three and 32 chunks of 64 detections, both sides of each LDS staging limit (KE_LDS_IOU doubles of a frame's IoU block,
KE2_MATCH_LDS / KE2_COUNT_LDS detection boxes), empty frames, idle waves in the last pass-1 workgroup, and every clip of
num_thresholds.  The pass entries take the overlaps, heights and image boxes as inputs, so the tests synthesise those directly
(small discrete value sets: ties everywhere) and need no polygon clip and no projection; corners and calibrations are zeros.

`_case_3d`, `_case_hand` and `_case_2d` build the inputs and the restatements' results once and assert, from those results
alone, that the draw reaches every rule (tp / fp / fn, objects consumed by ignored detections, -inf slots of counted objects,
the DontCare rule on both sides of min_overlap, fractional similarity sums), so a degenerate draw cannot pass silently."""
import functools

import numpy as np
import pytest

import kitti_eval_image_restatement as RI
import kitti_eval_restatement as R

CAR, VAN, TRUCK = 0, 1, 2
MIN_OVERLAP = 0.7
NPTS = R.N_SAMPLE_PTS
MAX_DETS = 2048                                          # MV3D_KITTI_MAX_DETS
IOUS = (0.0, 0.3, 0.7, 0.71, 0.8, 0.8, 0.95)             # 0.7 itself must not match
SCORES = np.float32([0.1, 0.25, 0.5, 0.5, 0.75, 0.9])
NO_SCORE = np.float32(-2e7)                              # below pass 1's NO_DETECTION start value
# thresholds: some equal to detection scores (a candidate is !(score < t)), some between, one below NO_SCORE
T_POOL = np.float32([0.9, 0.8, 0.75, 0.5, 0.3, 0.25, 0.1, -3e7])
# (D, G) per frame: 13 frames x 6 tasks = 78, two idle waves in the last pass-1 workgroup
SHAPES_3D = ((0, 0), (0, 4), (5, 0), (1, 3), (63, 4), (64, 4), (65, 4), (129, 5), (512, 8), (513, 8), (MAX_DETS, 2), (MAX_DETS, 5),
             (40, 6))
# (D, G, K) per frame: 33 tasks, three idle waves; the D = 384 and D = 385 frames share a pass-1 workgroup
SHAPES_2D = ((0, 0, 0), (0, 4, 2), (5, 0, 1), (64, 4, 0), (65, 4, 3), (384, 5, 2), (385, 5, 2), (384, 3, 0), (1024, 4, 3),
             (1025, 4, 3), (MAX_DETS, 5, 2))
# num_thresholds of the count calls: each of 0, 1, 4, 5, 41, and 50 (clipped to 41) and -3 (clipped to 0)
NTHR_3D = (((0, 1, 4), (5, 41, 50)), ((-3, 41, 5), (41, 1, 41)))
NTHR_2D = ((0, 1, 4), (5, 41, 50), (-3, 41, 41))


def _clip_n(n):
    return min(max(int(n), 0), NPTS)


def _labels(rng, G, heights):
    """G objects: classes among the evaluated, the neighbour and another one; occlusion, truncation and image height chosen so
    that every GT flag occurs at every difficulty."""
    cls = rng.choice([CAR] * 6 + [VAN, TRUCK], G).astype(np.int32)
    trunc = rng.choice(np.float32([0.0] * 6 + [0.15, 0.2, 0.4, 0.6]), G).astype(np.float32)
    occ = rng.choice(np.float32([0] * 6 + [1, 2, 3]), G).astype(np.float32)
    y1 = np.full(G, 100.0, np.float32)
    y2 = (y1 + rng.choice(np.float32(heights), G)).astype(np.float32)
    return cls, trunc, occ, y1, y2


def _flags(fr, di):
    return [R.gt_flag(c, t, o, a, b, di, CAR, VAN) for c, t, o, a, b in zip(fr['cls'], fr['trunc'], fr['occ'], fr['y1'], fr['y2'])]


def _scores(rng, D):
    s = rng.choice(SCORES, D).astype(np.float32)
    s[rng.rand(D) < 0.03] = NO_SCORE
    return s


def _check_flags(frames):
    for di in range(3):
        seen = {fl for fr in frames for fl in _flags(fr, di)}
        assert seen == {-1, 0, 1}, (di, seen)


# ------------------------------------------------------------------ BEV / 3D
def _frame_3d(rng, D, G):
    keep = min(0.4, 8.0 / max(D, 1))                    # a handful of overlapping detections per object, whatever D
    iou = tuple(rng.choice(IOUS, (D, G)) * (rng.rand(D, G) < keep) for _ in range(2))
    cls, trunc, occ, y1, y2 = _labels(rng, G, (24, 30, 50, 60, 60, 60))
    return {'iou': iou, 'scores': _scores(rng, D), 'heights': rng.choice([20.0, 30.0, 50.0], D, p=[0.2, 0.2, 0.6]),
            'cls': cls, 'trunc': trunc, 'occ': occ, 'y1': y1, 'y2': y2}


def _hand_frame():
    """D = 130, G = 3.  Column 0: the largest IoU at j = 3, 67, 69, 129 (a tie inside lane 3 across chunks, and across lanes);
    column 1: only the (at easy) ignored detections j = 70 and j = 5 overlap it, the first index must win; column 2: nothing
    above min_overlap."""
    D, G = 130, 3
    iou = np.zeros((D, G))
    iou[:, 2] = np.resize([0.0, 0.3, 0.7], D)
    iou[np.arange(1, D, 7), 0] = 0.8
    iou[[3, 67, 69, 129], 0] = 0.95
    iou[[70, 5], 1] = 0.8
    scores = np.resize(np.float32([0.1, 0.25, 0.5, 0.75]), D)
    scores[[3, 67, 69, 129]] = [0.25, 0.5, 0.5, 0.9]
    scores[[5, 70]] = [0.5, 0.5]
    heights = np.full(D, 50.0)
    heights[[5, 70]] = 30.0
    heights[np.arange(1, D, 14)] = 20.0
    return {'iou': (iou, iou.copy()), 'scores': scores, 'heights': heights, 'cls': np.int32([CAR, CAR, CAR]),
            'trunc': np.float32([0, 0, 0]), 'occ': np.float32([0, 0, 0]), 'y1': np.float32([100, 100, 100]),
            'y2': np.float32([160, 160, 160])}


def _oracle_3d(frames, thr):
    """-> matched [m][d] (Gtot) f32, stats {(f, m, d, t): (tp, fp, fn)} for every threshold value of thr[m, d]."""
    matched = [[None] * 3 for _ in range(2)]
    stats = {}
    for di in range(3):
        flags = [_flags(fr, di) for fr in frames]
        for mi in range(2):
            matched[mi][di] = np.concatenate([R.frame_stats(fr['iou'][mi], fr['scores'], fr['heights'], fl, di, MIN_OVERLAP)
                                              for fr, fl in zip(frames, flags)] + [np.zeros(0, np.float32)])
            for t in np.unique(thr[mi, di]):
                for f, (fr, fl) in enumerate(zip(frames, flags)):
                    stats[(f, mi, di, float(t))] = R.frame_stats(fr['iou'][mi], fr['scores'], fr['heights'], fl, di, MIN_OVERLAP, t)
    return matched, stats


def _conditions_3d(frames, thr, matched, stats):
    _check_flags(frames)
    consumed = False
    for di in range(3):
        flags = [_flags(fr, di) for fr in frames]
        n0 = [fl.count(0) for fl in flags]
        flat = np.concatenate([np.int32(fl) for fl in flags])
        for mi in range(2):
            assert ((matched[mi][di] == -np.inf) & (flat == 0)).any(), "no -inf slot of a counted object"
            assert (matched[mi][di][flat == 0] > -np.inf).any()
            all_three = False
            for t in np.unique(thr[mi, di]):
                tot = np.sum([stats[(f, mi, di, float(t))] for f in range(len(frames))], axis=0)
                all_three = all_three or bool((tot > 0).all())
                # an object that is counted (flag 0), matched, and neither tp nor fn was consumed by an ignored detection
                consumed = consumed or any(n0[f] - stats[(f, mi, di, float(t))][0] - stats[(f, mi, di, float(t))][2] > 0
                                           for f in range(len(frames)))
            assert all_three, "tp, fp and fn never all non-zero (metric %d, difficulty %d)" % (mi, di)
    assert consumed, "no object consumed by an ignored detection"


def _thresholds(rng, shape):
    return rng.choice(T_POOL, shape + (NPTS,)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case_3d():
    rng = np.random.RandomState(2048)
    frames = [_frame_3d(rng, D, G) for D, G in SHAPES_3D]
    thr = _thresholds(rng, (2, 3))
    matched, stats = _oracle_3d(frames, thr)
    _conditions_3d(frames, thr, matched, stats)
    return frames, thr, matched, stats


@functools.lru_cache(maxsize=None)
def _case_hand():
    frames = [_hand_frame()]
    thr = np.tile(np.resize(T_POOL, NPTS), (2, 3, 1)).astype(np.float32)
    matched, stats = _oracle_3d(frames, thr)
    # the rules the frame was built for, read off the restatement: column 0 takes the first of the tied detections that is a
    # candidate; column 1 is consumed by an ignored detection at easy and matched at moderate / hard; column 2 is missed
    for di, want in enumerate(([0.9, -np.inf, -np.inf], [0.9, 0.5, -np.inf], [0.9, 0.5, -np.inf])):
        assert np.array_equal(matched[0][di], np.float32(want)), di
    assert stats[(0, 0, 0, 0.5)][0::2] == (1, 1) and stats[(0, 0, 1, 0.5)][0::2] == (2, 1)
    return frames, thr, matched, stats


# ------------------------------------------------------------------ 2D
def _frame_2d(rng, D, G, K):
    """Boxes on a coarse grid.  Objects in a row at y = 100, DontCare boxes in a row at y = 250; a detection sits on an object
    (offsets from a small set: exact IoU ties, IoU exactly min_overlap), on a DontCare box (covered by 1, 0.7, 0.5 or 0.2 of
    its area) or elsewhere."""
    cls, trunc, occ, y1, y2 = _labels(rng, G, (24, 26, 41, 41, 50, 60, 60))
    gx = 20.0 + 220.0 * np.arange(G)
    gt_boxes = np.stack([gx, y1, gx + 100.0, y2], 1).astype(np.float32).reshape(G, 4)
    kx = 50.0 + 300.0 * np.arange(K)
    dc = np.stack([kx, np.full(K, 250.0), kx + 100.0, np.full(K, 300.0)], 1).astype(np.float32).reshape(K, 4)
    boxes = np.zeros((D, 4))
    for j in range(D):
        kind = rng.rand()
        if G and kind < 0.5:
            g = gt_boxes[int(G * rng.rand() ** 3)].astype(np.float64)      # the later objects get few detections
            x1 = g[0] + rng.choice([0.0, 0.0, 10.0, -10.0, 30.0])
            x2 = g[2] + rng.choice([0.0, 0.0, -10.0, 10.0])
            b1 = g[1] + rng.choice([0.0, 0.0, 0.0, 5.0])
            boxes[j] = (x1, b1, x2, b1 + rng.choice([20.0, 30.0, 40.0, 50.0, 60.0]))
        elif K and kind < 0.8:
            q = dc[rng.randint(K)].astype(np.float64)
            x1 = q[0] + rng.choice([0.0, 30.0, 50.0, 80.0])
            boxes[j] = (x1, q[1], x1 + 100.0, q[3])
        else:
            x1 = 40.0 * rng.randint(25)
            boxes[j] = (x1, 320.0, x1 + 80.0, 320.0 + rng.choice([20.0, 30.0, 50.0]))
    return {'boxes': boxes, 'alphas': rng.uniform(-np.pi, np.pi, D), 'scores': _scores(rng, D), 'gt_boxes': gt_boxes,
            'gt_alpha': rng.uniform(-np.pi, np.pi, G).astype(np.float32), 'dontcare': dc, 'cls': cls, 'trunc': trunc, 'occ': occ,
            'y1': gt_boxes[:, 1], 'y2': gt_boxes[:, 3]}


def _args_2d(fr):
    return fr['boxes'], fr['alphas'], fr['scores'], fr['gt_boxes'], fr['gt_alpha'], fr['dontcare']


def _oracle_2d(frames, thr):
    """-> matched [d] (Gtot) f32, stats {(f, d, t): (tp, fp, fn, S)} for every threshold value of thr[d]."""
    matched, stats = [None] * 3, {}
    for di in range(3):
        flags = [_flags(fr, di) for fr in frames]
        matched[di] = np.concatenate([RI.frame_stats_2d(*_args_2d(fr), fl, di, MIN_OVERLAP) for fr, fl in zip(frames, flags)] +
                                     [np.zeros(0, np.float32)])
        for t in np.unique(thr[di]):
            for f, (fr, fl) in enumerate(zip(frames, flags)):
                stats[(f, di, float(t))] = RI.frame_stats_2d(*_args_2d(fr), fl, di, MIN_OVERLAP, t)
    return matched, stats


def _conditions_2d(frames, thr, matched, stats):
    _check_flags(frames)
    consumed = removed = stays = fractional = False
    t_low = float(T_POOL[-2])
    for di in range(3):
        flags = [_flags(fr, di) for fr in frames]
        n0 = [fl.count(0) for fl in flags]
        flat = np.concatenate([np.int32(fl) for fl in flags])
        assert ((matched[di] == -np.inf) & (flat == 0)).any(), "no -inf slot of a counted object"
        all_three = False
        for t in np.unique(thr[di]):
            per = [stats[(f, di, float(t))] for f in range(len(frames))]
            all_three = all_three or bool((np.sum([p[:3] for p in per], axis=0) > 0).all())
            consumed = consumed or any(n0[f] - p[0] - p[2] > 0 for f, p in enumerate(per))
            fractional = fractional or any(0.0 < p[3] < p[0] for p in per)
        assert all_three, "tp, fp and fn never all non-zero (difficulty %d)" % di
        for f, (fr, fl) in enumerate(zip(frames, flags)):
            if not len(fr['dontcare']) or (f, di, t_low) not in stats:
                continue
            # the DontCare rule removes a counted fp: the same frame without its DontCare boxes counts more
            bare = RI.frame_stats_2d(fr['boxes'], fr['alphas'], fr['scores'], fr['gt_boxes'], fr['gt_alpha'], fr['dontcare'][:0], fl,
                                     di, MIN_OVERLAP, np.float32(t_low))
            removed = removed or bare[1] > stats[(f, di, t_low)][1]
            # a detection that is a candidate, not ignored and overlaps no object above min_overlap is a counted fp; one that a
            # DontCare box covers by (0, min_overlap] of its area stays
            for j, b in enumerate(fr['boxes']):
                if stays or b[3] - b[1] < R.MIN_HEIGHT[di] or fr['scores'][j] < np.float32(t_low):
                    continue
                if any(RI.iou2d(b, g) > MIN_OVERLAP for g in fr['gt_boxes']):
                    continue
                cover = max(RI.dontcare_overlap(b, q) for q in fr['dontcare'])
                stays = 0.0 < cover <= MIN_OVERLAP and stats[(f, di, t_low)][1] > 0
    assert consumed, "no object consumed by an ignored detection"
    assert removed, "the DontCare rule removes no counted fp"
    assert stays, "no counted fp under a DontCare box stays"
    assert fractional, "no similarity sum strictly between 0 and tp"


@functools.lru_cache(maxsize=None)
def _case_2d():
    rng = np.random.RandomState(385)
    frames = [_frame_2d(rng, D, G, K) for D, G, K in SHAPES_2D]
    thr = _thresholds(rng, (3,))
    thr[:, 0] = T_POOL[-2]                              # every difficulty has the threshold the DontCare conditions look at
    matched, stats = _oracle_2d(frames, thr)
    _conditions_2d(frames, thr, matched, stats)
    return frames, thr, matched, stats


def test_inputs_reach_every_rule():
    """No GPU: the shapes are the ones the kernels' paths turn on, and the restatements' results on the drawn inputs meet every
    condition (asserted while the cases are built)."""
    assert len(SHAPES_3D) * 6 % 4 == 2 and len(SHAPES_2D) * 3 % 4 == 1
    assert {D * G for D, G in SHAPES_3D} >= {4096, 4104, MAX_DETS * 2, MAX_DETS * 5}
    assert {D for D, _, _ in SHAPES_2D} >= {64, 65, 384, 385, 1024, 1025, MAX_DETS}
    for nthr in (NTHR_3D, NTHR_2D):
        assert set(np.ravel(nthr)) == {0, 1, 4, 5, 41, 50, -3}
    assert set(SCORES) & set(T_POOL)
    _case_3d()
    _case_hand()
    _case_2d()


# ------------------------------------------------------------------ device (MI355X)
def _cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    return torch


def _split_of(frames, key_d, key_g):
    """The device split of the frames: scores, offsets and labels real, corners and calibrations zeros (no pass reads them)."""
    import torch
    from mv3d_tf_amd import ops
    F = len(frames)
    det_off = np.concatenate([[0], np.cumsum([len(fr[key_d]) for fr in frames])]).astype(np.int32)
    gt_off = np.concatenate([[0], np.cumsum([len(fr[key_g]) for fr in frames])]).astype(np.int32)
    cat = lambda k, dt: np.concatenate([np.asarray(fr[k], dt) for fr in frames])
    attr = np.stack([cat('trunc', np.float32), cat('occ', np.float32), cat('y1', np.float32), cat('y2', np.float32)], 1)
    return ops.KittiEvalSplit(np.zeros((det_off[-1], 24), np.float32), cat('scores', np.float32), det_off, np.zeros((F, 4, 12), np.float32),
                              np.zeros((gt_off[-1], 24), np.float32), gt_off, cat('cls', np.int32), attr, torch.device('cuda', 0))


def _run_3d(case, nthr_calls):
    torch = _cuda()
    from mv3d_tf_amd import ops
    frames, thr, want_matched, stats = case
    dev = torch.device('cuda', 0)
    sp = _split_of(frames, 'scores', 'cls')
    iou = np.stack([np.concatenate([fr['iou'][mi].reshape(-1) for fr in frames]) for mi in range(2)])
    assert iou.shape == (2, sp.num_pairs)
    d_iou = torch.from_numpy(iou).to(dev)
    d_height = torch.from_numpy(np.concatenate([fr['heights'] for fr in frames]).astype(np.float64)).to(dev)
    matched = ops.kitti_eval_match(sp, d_iou, d_height, CAR, VAN, MIN_OVERLAP).cpu().numpy()
    for mi in range(2):
        for di in range(3):
            assert np.array_equal(matched[mi, di], want_matched[mi][di]), (mi, di)
    for nthr in nthr_calls:
        d_thr, d_nthr = ops.upload_packed([thr, np.int32(nthr)], dev)
        counts = ops.kitti_eval_count(sp, d_iou, d_height, CAR, VAN, MIN_OVERLAP, d_thr, d_nthr).cpu().numpy()
        for mi in range(2):
            for di in range(3):
                n = _clip_n(nthr[mi][di])
                want = [np.sum([stats[(f, mi, di, float(t))] for f in range(len(frames))], axis=0) for t in thr[mi, di, :n]]
                assert np.array_equal(counts[mi, di, :n], np.reshape(want, (n, 3))), (nthr, mi, di)
                assert not counts[mi, di, n:].any(), (nthr, mi, di)


@pytest.mark.gpu
def test_3d_passes_equal_restatement_at_every_path():
    _run_3d(_case_3d(), NTHR_3D)


@pytest.mark.gpu
def test_3d_passes_hand_built_ties():
    _run_3d(_case_hand(), (((41, 41, 41), (41, 41, 41)),))


@pytest.mark.gpu
def test_2d_passes_equal_restatement_at_every_path():
    torch = _cuda()
    from mv3d_tf_amd import ops
    frames, thr, want_matched, stats = _case_2d()
    F = len(frames)
    dev = torch.device('cuda', 0)
    sp = _split_of(frames, 'scores', 'cls')
    dc_off = np.concatenate([[0], np.cumsum([len(fr['dontcare']) for fr in frames])]).astype(np.int32)
    im = ops.KittiImageSplit(sp, np.concatenate([fr['gt_boxes'] for fr in frames]), np.concatenate([fr['gt_alpha'] for fr in frames]),
                             dc_off, np.concatenate([fr['dontcare'] for fr in frames]), np.tile(np.int32([375, 1242]), (F, 1)))
    cam = np.zeros((sp.N, 8))
    cam[:, 7] = np.concatenate([fr['alphas'] for fr in frames])
    d_box, d_cam = torch.from_numpy(np.concatenate([fr['boxes'] for fr in frames])).to(dev), torch.from_numpy(cam).to(dev)
    matched = ops.kitti_eval_match_2d(sp, im, d_box, CAR, VAN, MIN_OVERLAP).cpu().numpy()
    for di in range(3):
        assert np.array_equal(matched[di], want_matched[di]), di
    for nthr in NTHR_2D:
        d_thr, d_nthr = ops.upload_packed([thr, np.int32(nthr)], dev)
        counts, sim = ops.kitti_eval_count_2d(sp, im, d_box, d_cam, CAR, VAN, MIN_OVERLAP, d_thr, d_nthr)
        counts, sim = counts.cpu().numpy(), sim.cpu().numpy()
        for di in range(3):
            n = _clip_n(nthr[di])
            per = np.array([[stats[(f, di, float(t))] for t in thr[di, :n]] for f in range(F)], np.float64).reshape(F, n, 4)
            assert np.array_equal(counts[di, :n], per[:, :, :3].sum(0).astype(np.int64)), (nthr, di)
            assert not counts[di, n:].any(), (nthr, di)
            assert np.abs(sim[:, di, :n] - per[:, :, 3]).max(initial=0.0) <= 1e-12, (nthr, di)
            assert not sim[:, di, n:].any(), (nthr, di)
