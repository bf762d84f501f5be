"""numpy restatement of the paper's empty-anchor rule (include/mv3d_hip.h: mv3d_anchor_occupancy and the masked entries), on top
of the unchanged oracle.  The checker of tests/test_empty_anchors.py, never the thing under test.

  anchor_counts / anchor_mask   occupancy = (bev != 0).any(-1); a padded int64 double cumsum; the anchors' boxes clipped to the map
  masked_stage1                 anchor_target_layer_tf.py:93-143 with `inside &= mask`, oracle.bbox_overlaps on the survivors
  masked_anchor_target_layer    oracle.anchor_target_layer's draw sequence over that reduced inds_inside
  masked_pred                   the proposal layer needs no restatement: a masked anchor's three size deltas are set to -200
                                (exp -> 0: a 1-pixel box, which fails RPN_MIN_SIZE * scale = 5)"""
import numpy as np
import numpy.random as npr


def all_anchors(oracle, H, W, stride=8):
    """(4 H W, 4) int64 pixel boxes, anchor n = (h, w, a), a fastest (proposal_layer_tf.py:79-95)"""
    base = oracle.generate_anchors_bv()
    sx, sy = np.meshgrid(np.arange(W) * stride, np.arange(H) * stride)
    shifts = np.stack([sx.ravel(), sy.ravel(), sx.ravel(), sy.ravel()], 1).astype(np.int64)
    return (base[None, :, :] + shifts[:, None, :]).reshape(-1, 4)


def anchor_counts(oracle, bev, H, W, stride=8):
    """bev (Hm, Wm, C) f32 -> (4 H W,) int64 occupied cells under every anchor"""
    bev = np.asarray(bev)
    Hm, Wm = bev.shape[:2]
    occ = (bev != 0).any(-1)
    ii = np.zeros((Hm + 1, Wm + 1), np.int64)
    ii[1:, 1:] = occ.astype(np.int64).cumsum(0).cumsum(1)
    a = all_anchors(oracle, H, W, stride)
    x1, y1 = np.maximum(a[:, 0], 0), np.maximum(a[:, 1], 0)
    x2, y2 = np.minimum(a[:, 2], Wm - 1), np.minimum(a[:, 3], Hm - 1)
    empty = (x1 > x2) | (y1 > y2)
    x1, y1, x2, y2 = (np.where(empty, 0, v) for v in (x1, y1, x2, y2))
    cnt = ii[y2 + 1, x2 + 1] - ii[y1, x2 + 1] - ii[y2 + 1, x1] + ii[y1, x1]
    return np.where(empty, 0, cnt)


def anchor_mask(oracle, bev, H, W, stride=8, min_cells=1):
    return (anchor_counts(oracle, bev, H, W, stride) >= min_cells).astype(np.uint8)


def masked_stage1(oracle, H, W, gt_boxes, gt_boxes_3d, im_info, mask, stride=8, train=None):
    """(inds_inside, max_overlaps, labels before the draws, targets) over the anchors that are inside AND not masked"""
    t = train or oracle.TRAIN
    a = all_anchors(oracle, H, W, stride)
    info = np.asarray(im_info, np.float32).reshape(-1)
    inside = (a[:, 0] >= 0) & (a[:, 1] >= 0) & (a[:, 2] < info[1]) & (a[:, 3] < info[0])           # :93-98
    inside &= np.asarray(mask).astype(bool)
    inds = np.where(inside)[0]
    labels = np.full(len(inds), -1, np.float32)                                                     # :110-111
    targets = np.zeros((len(inds), 6), np.float32)
    if len(inds) == 0:
        return inds, np.zeros(0, np.float64), labels, targets
    ov = oracle.bbox_overlaps(a[inds].astype(np.float64), np.asarray(gt_boxes, np.float32)[:, :4].astype(np.float64))
    argmax = ov.argmax(1)
    max_ov = ov[np.arange(len(inds)), argmax]
    gt_max = ov[ov.argmax(0), np.arange(ov.shape[1])]
    gt_argmax = np.where(ov == gt_max)[0]                                                          # :123
    if not t["RPN_CLOBBER_POSITIVES"]:
        labels[(0 < max_ov) & (max_ov < t["RPN_NEGATIVE_OVERLAP"])] = 0                             # :129-130
    labels[gt_argmax] = 1                                                                           # :133
    labels[max_ov >= t["RPN_POSITIVE_OVERLAP"]] = 1                                                 # :139
    if t["RPN_CLOBBER_POSITIVES"]:
        labels[max_ov < t["RPN_NEGATIVE_OVERLAP"]] = 0                                              # :141-143
    # an anchor's argmax (hence its target) does not depend on the other anchors: the unmasked oracle's
    u_inds, _, _, _, u_tg = oracle.anchor_target_stage1(H, W, gt_boxes, gt_boxes_3d, im_info, stride, t)
    full = np.zeros((4 * H * W, 6), np.float32)
    full[u_inds] = u_tg
    return inds, max_ov, labels, full[inds]


def masked_anchor_target_layer(oracle, H, W, gt_boxes, gt_boxes_3d, im_info, mask, stride=8, train=None):
    """(rpn_labels (N,), rpn_bbox_targets (N,6), anchors (M,5), anchors_3d (M,7)) with the draws of
    anchor_target_layer_tf.py:146-183 from the numpy global RNG, over the reduced inds_inside"""
    import ctypes as C
    t = train or oracle.TRAIN
    N = 4 * H * W
    inds, max_ov, labels, targets = masked_stage1(oracle, H, W, gt_boxes, gt_boxes_3d, im_info, mask, stride, t)
    labels = labels.copy()
    choice = lambda x, k: x[npr.permutation(len(x))[:k]]
    num_fg = int(t["RPN_FG_FRACTION"] * t["RPN_BATCHSIZE"])
    fg = np.where(labels == 1)[0]
    if len(fg) > num_fg:
        labels[choice(fg, len(fg) - num_fg)] = -1
    num_bg = t["RPN_BATCHSIZE"] - np.sum(labels == 1)
    bg = np.where(labels == 0)[0]
    if len(bg) > num_bg:
        labels[choice(bg, len(bg) - num_bg)] = -1
    sel = inds[labels != -1]                                                                        # :170-174
    anc = all_anchors(oracle, H, W, stride)[sel]
    anc3d = np.zeros((len(sel), 6), np.float64)
    if len(sel):
        anc_c = np.ascontiguousarray(anc, np.int64)
        oracle.lib().mv3d_ref_bv_anchor_to_lidar(anc_c.ctypes.data_as(C.c_void_p), C.c_int(len(sel)), anc3d.ctypes.data_as(C.c_void_p))
    zeros = np.zeros((len(sel), 1), np.float32)
    anchors = np.hstack((zeros, anc)).astype(np.float32)
    anchors_3d = np.hstack((zeros, anc3d)).astype(np.float32)
    labels[max_ov < t["RPN_NEGATIVE_OVERLAP"]] = 0                                                  # :176-183
    num_bg = t["RPN_BATCHSIZE"] - np.sum(labels == 1)
    bg = np.where(labels == 0)[0]
    if len(bg) > num_bg:
        labels[choice(bg, len(bg) - num_bg)] = -1
    rpn_labels = np.full((N,), -1, np.float32)
    rpn_labels[inds] = labels
    rpn_targets = np.zeros((N, 6), np.float32)
    rpn_targets[inds] = targets
    return rpn_labels, rpn_targets, anchors, anchors_3d


def masked_pred(rpn_bbox_pred, mask):
    """rpn_bbox_pred (1, H, W, 24) with the three size deltas of every masked anchor at -200"""
    p = np.array(rpn_bbox_pred, np.float32).reshape(-1, 6)
    p[np.asarray(mask).reshape(-1) == 0, 3:6] = -200.0
    return p.reshape(np.asarray(rpn_bbox_pred).shape)
