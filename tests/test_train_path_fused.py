"""The training path's own launches (csrc/train_stream.hip) against the public single-purpose entries, bit for bit.

The path pairs independent launches of a batch in one grid each -- proposal decode || anchor overlap, local rank || anchor labels,
merge rank || anchor compaction in stage 1, anchor emit + relabel || ROI emit in stage 2 -- and lets stage 1's last launch
(pt_compact_kernel, one workgroup per frame) write the batch's reports into the pinned host buffers.  The public entries keep
their launches, so they are the reference here: proposal layer, anchor-target stage 1 / 2, proposal-target stage 1 / 2, called
one by one on the same inputs with the very lists the path drew (read from the slot's pinned list buffer by `draw_sizes`).
`mv3d_train_path_launch_plan` says, without a device, what a configuration enqueues.

Shapes: the smallest at which a shared grid can go wrong -- one workgroup per body (3 x 5), a different number for every body with a
ragged last compaction workgroup (20 x 24: 1920 anchors = 16 decode / rank, 8 overlap / label and 2 compaction workgroups, the second
with 896 items), the workload's own grid (76 x 76) and a grid on the counting rank path, which keeps the single-purpose launches
(80 x 80); B = 1, 2 and 16 (the argument block at its largest), one and max_gt
ground-truth boxes, with and without an anchor mask, helper thread on and off."""
import ctypes as C

import numpy as np
import pytest

from mv3d_tf_amd import synth

MAX_GT = 64


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    return torch


def _config(B, H, W):
    """the configuration TrainPathStream hands to the library, built without a device"""
    from mv3d_tf_amd import _lib, ops
    from mv3d_tf_amd.fast_rcnn.config import cfg
    T = cfg.TRAIN
    c = _lib.TrainPathConfig()
    c.batch, c.H, c.W, c.num_classes = B, H, W, 2
    c.proposal = ops.proposal_params(T)
    c.proposal_cap = _lib.lib().mv3d_proposal_3d_capacity(H, W, C.byref(c.proposal))
    c.anchor_cap, c.roi_cap, c.max_gt = ops.anchor_debug_rows(T), int(T.BATCH_SIZE), MAX_GT
    c.anchor = ops.anchor_target_params(T)
    c.target = ops.proposal_target_params(T, 2)
    c.draw = _lib.DrawParams(int(T.RPN_BATCHSIZE), int(T.RPN_FG_FRACTION * T.RPN_BATCHSIZE), int(T.BATCH_SIZE),
                             int(np.round(T.FG_FRACTION * T.BATCH_SIZE)))
    return c


def test_launch_plan():
    """76 x 76, B = 2, TRAIN cfg: 3 paired launches + 5 of the NMS (tiles, chain, three later rounds) + 2 of the proposal targets
    = 10 in stage 1, upload + disable + the paired emit = 3 in stage 2; 80 x 80 (25 600 anchors: the counting rank path) keeps the
    single-purpose 14 and 4."""
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import _lib
    L = _lib.lib()
    s1, s2 = C.c_int32(), C.c_int32()
    assert L.mv3d_train_path_launch_plan(C.byref(_config(2, 76, 76)), C.byref(s1), C.byref(s2)) == 1
    assert (s1.value, s2.value) == (10, 3)
    assert L.mv3d_train_path_launch_plan(C.byref(_config(2, 80, 80)), C.byref(s1), C.byref(s2)) == 0
    assert (s1.value, s2.value) == (14, 4)
    assert L.mv3d_train_path_launch_plan(C.byref(_config(16, 20, 24)), None, None) == 1
    bad = _config(2, 76, 76)
    bad.batch = 0
    assert L.mv3d_train_path_launch_plan(C.byref(bad), C.byref(s1), C.byref(s2)) == -1
    assert L.mv3d_train_path_launch_plan(None, None, None) == -1


def _frames(seed, H, W, B, G):
    """B frames of synth.rpn_head; G boxes per frame when given (else the head's own 8).  On a grid smaller than KITTI's the boxes
    are scaled into the image, so that anchors and proposals still overlap them."""
    out = []
    for b in range(B):
        prob, pred, info, calib, gt = synth.rpn_head(seed + b, H, W, "peaky", return_gt=True)
        if G is not None:
            gt = synth.gt_cars(np.random.RandomState(seed + 1000 + b), G)
        gt = [a.copy() for a in gt]
        gt[0][:, :4] = np.floor(gt[0][:, :4] * np.float32(float(info[0, 0]) / 608.0))
        out.append((prob, pred, info, calib, tuple(gt)))
    return out


#        H   W   B   G        mask   helper  positive overlap
CASES = [(3, 5, 1, 1, False, False, None),
         (3, 5, 2, MAX_GT, True, True, None),
         (20, 24, 2, None, False, True, None),
         (20, 24, 16, 1, True, False, None),
         (20, 24, 16, MAX_GT, False, True, None),
         (76, 76, 2, None, False, True, None),
         (76, 76, 2, None, True, False, None),
         (76, 76, 1, MAX_GT, False, False, 0.0),           # every inside anchor is a positive: the report's head spills
         (76, 76, 2, 1, False, True, 0.0),
         (80, 80, 2, None, False, True, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,B,G,masked,helper,pos_ov", CASES)
def test_path_equals_the_single_entries(gpu, H, W, B, G, masked, helper, pos_ov):
    torch = gpu
    from mv3d_tf_amd import ops
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.rpn_msr.anchor_target_layer_tf import draw_subsamples_host
    from mv3d_tf_amd.rpn_msr.proposal_target_layer_tf import draw_samples_host
    from mv3d_tf_amd.train_path import TrainPathStream
    T = cfg.TRAIN
    saved = T.RPN_POSITIVE_OVERLAP
    if pos_ov is not None:
        T.RPN_POSITIVE_OVERLAP = pos_ov
    path = None
    try:
        dev = torch.device("cuda")
        N = 4 * H * W
        frames = _frames(7000 + 31 * H + B, H, W, B, G)
        t = lambda a, dt=np.float32: torch.as_tensor(np.ascontiguousarray(a, dt)).to(dev)
        prob, pred = t(np.concatenate([f[0] for f in frames])), t(np.concatenate([f[1] for f in frames]))
        info, calib = t(np.concatenate([f[2] for f in frames])), t(np.stack([f[3] for f in frames]))
        gt = [tuple(t(a) for a in f[4]) for f in frames]
        mask = t(np.random.RandomState(H + W + B).random_sample((B, N)) < 0.7, np.uint8) if masked else None

        # ---- the path
        path = TrainPathStream(B, H, W, dev, depth=1, max_gt=MAX_GT, async_draws=helper)
        np.random.seed(1234 + H)
        slot = path.submit(prob, pred, info, calib, gt, anchor_mask=mask)
        out = path.finish(slot)
        torch.cuda.synchronize()
        state_after = np.random.get_state()
        sizes = np.asarray(out["draw_sizes"], np.int64).reshape(B, 5)
        offs = np.concatenate([[0], np.cumsum(sizes.reshape(-1))])
        lists = [[slot.h_lists[offs[5 * b + k]:offs[5 * b + k + 1]].numpy().copy() for k in range(5)] for b in range(B)]

        # ---- the reports as the host got them == the device copies
        head = slot.h_report.shape[1]
        assert torch.equal(slot.h_report, slot.report[:, :head].cpu())
        assert torch.equal(slot.h_small, slot.pt_counts.cpu())
        assert torch.equal(slot.h_tail, slot.tail.cpu())
        assert out["num_proposals"] == slot.tail[:B].cpu().tolist()

        # ---- the single entries, one by one, on the same inputs and lists
        bv, img, b3, num, status = ops.proposal_3d(prob, pred, info, calib, path.pparams, anchor_mask=mask)
        for got, want in zip(out["proposals"], (bv, img, b3, num, status)):
            assert torch.equal(got, want)
        ap = ops.anchor_target_params(T)
        np.random.seed(1234 + H)
        row = 0
        for b in range(B):
            gt_bv, gt_3d, gt_c = gt[b]
            labels, targets, counts, fg_hi, ws, cf = ops.anchor_target_stage1(H, W, info[b], gt_bv, gt_3d, ap,
                                                                              anchor_mask=None if mask is None else mask[b])
            n_fg = int(counts[1])
            assert torch.equal(cf[:16], slot.report[b, :16]) and torch.equal(fg_hi[:n_fg], slot.report[b, 32:32 + n_fg])
            assert torch.equal(targets, out["rpn_targets"][b])
            # the numpy statement of the draws, on the reports the host got: the same lists, in the same order
            dis = draw_subsamples_host(slot.h_report[b].numpy(), lambda: slot.report[b, 32:].cpu().numpy(), N)
            dis = [np.zeros(0, np.int32) if d is None else d for d in dis]
            for k in range(3):
                assert np.array_equal(dis[k], lists[b][k])
            anchors, anchors_3d, n_anc = ops.anchor_target_stage2(H, W, ap, *lists[b][:3], labels, ws, path.anchor_cap)
            m = int(n_anc)
            assert m == int(out["n_anchors"][b]) and torch.equal(labels, out["rpn_labels"][b])
            m = min(m, path.anchor_cap)
            assert torch.equal(anchors[:m], out["anchors"][b, :m]) and torch.equal(anchors_3d[:m], out["anchors_3d"][b, :m])

            tp = ops.proposal_target_params(T, path.nc, frame_index=b)
            n = int(num[b])
            pcounts, pws = ops.proposal_target_stage1(bv[b, :n], b3[b, :n], gt_bv, gt_3d, tp)
            assert torch.equal(pcounts, slot.pt_counts[b])
            picks = draw_samples_host(slot.h_small[b].numpy())
            assert np.array_equal(picks[0], lists[b][3]) and np.array_equal(picks[1], lists[b][4])
            S = len(lists[b][3]) + len(lists[b][4])
            assert out["S"][b] == S
            if S:
                r_bv, r_img, r_lab, r_tg, r_3d = ops.proposal_target_stage2(bv[b, :n], b3[b, :n], gt_bv, gt_3d, gt_c, calib[b], tp,
                                                                            lists[b][3], lists[b][4], pws)
                sl = slice(row, row + S)
                assert torch.equal(r_bv, out["rois"]["bev"][sl]) and torch.equal(r_img, out["rois"]["rgb"][sl])
                assert torch.equal(r_lab, out["labels"][sl]) and torch.equal(r_tg, out["bbox_targets"][sl])
                assert torch.equal(r_3d, out["rois_3d"][sl])
                assert torch.equal(ops.rois_3d_to_fv(r_3d), out["rois"]["fv"][sl])
            row += S
        assert row == out["rois"]["bev"].shape[0]
        # the generator ends where the numpy draws leave it
        now = np.random.get_state()
        assert np.array_equal(now[1], state_after[1]) and now[2] == state_after[2]

        # ---- the cases are what they are here for
        if N < T.RPN_BATCHSIZE // 2:                       # fewer anchors than either quota: nothing is disabled, no disable launch
            assert not sizes[:, :3].any()
        else:
            assert sizes[:, :3].any()
        if pos_ov == 0.0:                                  # more positives than travel with the report's head
            assert int(slot.h_report[0, :16].view(torch.int32)[1]) > head - 32
    finally:
        T.RPN_POSITIVE_OVERLAP = saved
        if path is not None:
            path.close()
