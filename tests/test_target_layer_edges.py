"""The two training target layers at their edges: `anchor_target_layer` (csrc/anchor_target.hip) and
`proposal_target_layer_3d` (csrc/proposal_target.hip).

One case table (`cases`) feeds three descriptions of the same thing:
  1. a recording of the reference's own layers (tests/golden/target_layer_edges.npz, written by
     tests/golden/make_target_edge_golden.py, which imports this table),
  2. a numpy float64 restatement written here from the layers' definition (`restate_anchor`, `restate_proposal`),
  3. the CPU oracle (oracle/), called with `train=`.
They are compared with one another without a GPU; the device (numpy-contract layers and the C entries) is then compared with
them bit for bit under `-m gpu`.  Every selection, label, ordering, draw and slot is compared with np.array_equal: no tolerances.
"""
import ctypes as C
import os

import numpy as np
import numpy.random as npr
import pytest

from conftest import GOLDEN, golden
from mv3d_tf_amd import synth

FIXTURE = "target_layer_edges"
F32 = np.float32

# cfg.TRAIN values the two layers read, at the reference's defaults (the shape of oracle.TRAIN)
TRAIN_DEFAULTS = dict(RPN_CLOBBER_POSITIVES=False, RPN_NEGATIVE_OVERLAP=0.5, RPN_POSITIVE_OVERLAP=0.7,
                      RPN_FG_FRACTION=0.25, RPN_BATCHSIZE=128, BATCH_SIZE=128, FG_FRACTION=0.25,
                      FG_THRESH=0.5, BG_THRESH_HI=0.5, BG_THRESH_LO=0.1)

# Cases the reference itself cannot run: name -> the exception type it raised (recorded in the fixture under exc__<name>).
# They drop out of the comparison with the recording only; restatement, oracle and device are still compared on them.
REFERENCE_RAISES = {
    "at_nothing_inside": "ValueError",          # overlaps.argmax(axis=0) of a (0, G) matrix
    "pt_empty_both": "AssertionError",          # _compute_targets_cnr: "gt rois cnr should not be empty" on S = 0
}

AT_FIELDS = ("labels", "targets", "anchors", "anchors_3d")
PT_FIELDS = ("rois_bv", "rois_img", "labels", "bbox_targets", "rois_3d")


# ------------------------------------------------------------------ arithmetic shared by table and restatement
def base_anchors():
    """generate_anchors_bv() as the reference returns it (fixture anchors_bv.npz)"""
    return golden("anchors_bv")["base"].astype(np.int64)


def all_anchors(H, W, stride=8):
    """(H*W*4, 4) i64 anchors in (h, w, a) order: anchor_target_layer_tf.py:76-89"""
    sx, sy = np.meshgrid(np.arange(0, W) * stride, np.arange(0, H) * stride)
    shifts = np.vstack((sx.ravel(), sy.ravel(), sx.ravel(), sy.ravel())).transpose()
    return (base_anchors().reshape((1, 4, 4)) + shifts.reshape((1, -1, 4)).transpose((1, 0, 2))).reshape((-1, 4))


def iou_pair(b, q):
    """lib/utils/bbox.pyx:33-54 for one pair, Python floats (f64)"""
    b = [float(v) for v in b]
    q = [float(v) for v in q]
    iw = min(b[2], q[2]) - max(b[0], q[0]) + 1
    if iw > 0:
        ih = min(b[3], q[3]) - max(b[1], q[1]) + 1
        if ih > 0:
            return iw * ih / ((b[2] - b[0] + 1) * (b[3] - b[1] + 1) + (q[2] - q[0] + 1) * (q[3] - q[1] + 1) - iw * ih)
    return 0.0


def iou_matrix(boxes, query):
    """bbox.pyx over the full N x G matrix, f64, the same IEEE operations in the same order"""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)[:, None, :]
    q = np.asarray(query, np.float64).reshape(-1, 4)[None, :, :]
    iw = np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0]) + 1
    ih = np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1]) + 1
    qarea = (q[..., 2] - q[..., 0] + 1) * (q[..., 3] - q[..., 1] + 1)
    with np.errstate(all="ignore"):
        ua = (b[..., 2] - b[..., 0] + 1) * (b[..., 3] - b[..., 1] + 1) + qarea - iw * ih
        o = iw * ih / ua
    return np.where((iw > 0) & (ih > 0), o, 0.0)


# ------------------------------------------------------------------ the case table
def hand_gt(rows):
    """BEV pixel rows (x1, y1, x2, y2, cls) -> (gt_bv (G,5), gt_3d (G,7), gt_corners (G,25)) f32 of upright boxes at those
    pixels (transform.py's pixel <-> metre convention, basic IEEE operations only)"""
    bv = np.array(rows, np.float64).reshape(-1, 5)
    cx, cy = (bv[:, 0] + bv[:, 2]) / 2.0, (bv[:, 1] + bv[:, 3]) / 2.0
    x, y = 60.0 - (cy + 0.5) * 0.1, 60.0 - (cx + 0.5) * 0.1 - 30.0
    l = np.maximum(np.abs(bv[:, 3] - bv[:, 1]), 1.0) * 0.1
    w = np.maximum(np.abs(bv[:, 2] - bv[:, 0]), 1.0) * 0.1
    G = len(bv)
    h, z = np.full(G, 1.5), np.full(G, -0.95)
    gt3d = np.stack([x, y, z, l, w, h, bv[:, 4]], 1).astype(F32)
    sx = np.array([1, 1, -1, -1, 1, 1, -1, -1]) * 0.5
    sy = np.array([1, -1, -1, 1, 1, -1, -1, 1]) * 0.5
    sz = np.array([-1, -1, -1, -1, 1, 1, 1, 1]) * 0.5
    cn = np.concatenate([x[:, None] + l[:, None] * sx, y[:, None] + w[:, None] * sy, z[:, None] + h[:, None] * sz,
                         bv[:, 4:5]], 1).astype(F32)
    return bv.astype(F32), gt3d, cn


def hand_rois(rows):
    """BEV pixel rows (x1, y1, x2, y2) -> proposal blobs (rois_bv (R,5), rois_3d (R,7)) with a zero batch column"""
    rows = np.array(rows, np.float64).reshape(-1, 4)
    bv, b3, _ = hand_gt(np.hstack([rows, np.zeros((len(rows), 1))]))
    return (np.hstack([np.zeros((len(rows), 1), F32), bv[:, :4]]).astype(F32),
            np.hstack([np.zeros((len(rows), 1), F32), b3[:, :6]]).astype(F32))


def scaled_cars(seed, G, H, W):
    """synth.gt_cars squeezed into an (8H, 8W) map, on whole pixels"""
    gtbv, gt3d, gtc = synth.gt_cars(np.random.RandomState(seed), G)
    gtbv[:, [0, 2]] = np.clip(np.floor(gtbv[:, [0, 2]] * (W / 76.0)), 0, W * 8 - 1)
    gtbv[:, [1, 3]] = np.clip(np.floor(gtbv[:, [1, 3]] * (H / 76.0)), 0, H * 8 - 1)
    return gtbv.astype(F32), gt3d, gtc


def grid_rows(H, W):
    """ground truth spread over an (8H, 8W) map, some of it in the part a transposed reading of the map would lose"""
    w, h = 8 * W, 8 * H
    rows = []
    for fx, fy, bw, bh in ((0.80, 0.45, 38, 15), (0.45, 0.80, 15, 38), (0.30, 0.35, 9, 5), (0.85, 0.80, 5, 9),
                           (0.50, 0.50, 36, 16), (0.15, 0.60, 12, 7)):
        x1, y1 = int(fx * w) - bw // 2, int(fy * h) - bh // 2
        rows.append([x1, y1, x1 + bw, y1 + bh, 1])
    return rows


GRIDS = ((5, 9), (9, 5), (16, 64), (76, 47))
TIE_SHIFTS = (("at", 0.0), ("above", 1.0), ("below", -1.0))


def _neighbour(v, direction):
    return v if direction == 0.0 else float(np.nextafter(v, direction * np.inf))


def anchor_cases():
    out = {}

    def add(name, grid, im_info, gt, seed, **train):
        gt_bv, gt_3d, gt_cnr = gt if isinstance(gt, tuple) else hand_gt(gt)
        out["at_" + name] = dict(kind="anchor", grid=grid, im_info=np.array([im_info], F32), gt_bv=gt_bv, gt_3d=gt_3d,
                                 gt_corners=gt_cnr, train=dict(TRAIN_DEFAULTS, **train), seed=seed)
        return out["at_" + name]

    # non-square grids, each with the full map and with one a few pixels smaller by different amounts per direction
    for k, (H, W) in enumerate(GRIDS):
        add("grid_%dx%d_full" % (H, W), (H, W), (8 * H, 8 * W, 1), grid_rows(H, W), 11 + k)
        add("grid_%dx%d_cut" % (H, W), (H, W), (8 * H - 13, 8 * W - 5, 1), grid_rows(H, W), 21 + k)
    # clobber: a car near a wide anchor, one near a tall anchor, a 3 x 3 box (every small anchor that holds it ties its column
    # maximum 9 / 66 < 0.3) and a box whose anchors land between the thresholds
    clob = [[60, 70, 98, 86, 1], [30, 20, 47, 58, 1], [100, 100, 102, 102, 1], [110, 40, 140, 60, 1]]
    add("clobber_default", (20, 20), (160, 160, 1), clob, 31, RPN_CLOBBER_POSITIVES=True)
    add("clobber_03", (20, 20), (160, 160, 1), clob, 31, RPN_CLOBBER_POSITIVES=True, RPN_NEGATIVE_OVERLAP=0.3)
    add("noclobber_03", (20, 20), (160, 160, 1), clob, 31, RPN_NEGATIVE_OVERLAP=0.3)
    # an overlap equal to a threshold: box 0 = the wide anchor of cell (10, 10) moved by (3, 2) pixels; the tied pair is that box
    # with the wide anchor of cell (10, 11), which is not the box's best anchor.  Box 1 is an anchor itself (IoU 1).
    A = all_anchors(20, 20)
    a_best, a_tied, a_same = A[(10 * 20 + 10) * 4 + 0], A[(10 * 20 + 11) * 4 + 0], A[(5 * 20 + 5) * 4 + 2]
    ties = [list(a_best + np.array([3, 2, 3, 2])) + [1], list(a_same) + [1]]
    v = iou_pair(a_tied, ties[0][:4])
    for key, short, dirs in (("RPN_POSITIVE_OVERLAP", "pos", (0.0, 1.0)), ("RPN_NEGATIVE_OVERLAP", "neg", (0.0, -1.0, 1.0))):
        for d in dirs:
            c = add("tie_%s_%s" % (short, {0.0: "at", 1.0: "above", -1.0: "below"}[d]), (20, 20), (160, 160, 1), ties, 41,
                    **{key: _neighbour(v, d)})
            c["tie"] = v
    # the reference's flood: box 1 lies beyond im_info, no inside anchor overlaps it, every inside anchor ties its column maximum 0
    add("flood", (40, 40), (320, 320, 1), [[150, 140, 188, 156, 1], [400, 400, 420, 440, 1]], 51)
    # ties for the argmax: one BEV box twice (different 3D rows), and two different boxes mirrored about the tall anchor of
    # cell (10, 10), whose centre column is x = 80; the right one comes first in the list
    dup = [[150, 60, 166, 99, 1], [150, 60, 166, 99, 1], [80, 61, 96, 100, 1], [64, 61, 80, 100, 1]]
    gt = hand_gt(dup)
    gt[1][1, :6] = [31.25, 14.5, -1.1, 4.5, 1.75, 1.25]
    gt[2][1, :24] += F32(0.5)
    add("argmax_ties", (40, 40), (320, 320, 1), gt, 61)
    # degenerate ground truth, G = 1
    add("degenerate_inverted", (20, 20), (160, 160, 1), [[100, 60, 90, 90, 1]], 71)
    add("degenerate_pixel", (20, 20), (160, 160, 1), [[77, 77, 77, 77, 1]], 72)
    # no inside anchor at all
    add("nothing_inside", (5, 9), (8, 8, 1), [[10, 10, 30, 20, 1]], 81)
    # none of the three draws (76 inside anchors in all), and another batch shape
    add("no_subsampling", (5, 9), (40, 72, 1), [[24, 10, 60, 26, 1]], 91)
    add("batch_shape", (37, 37), (296, 296, 1), scaled_cars(92, 12, 37, 37), 92, RPN_BATCHSIZE=256, RPN_FG_FRACTION=0.5)
    # TARGET_MAX_GT
    add("g_limit", (20, 20), (160, 160, 1), scaled_cars(93, 1024, 20, 20), 93)
    return out


def base_proposals(oracle):
    """Proposals of a 20 x 20 head with five cars on whole pixels; the first 40 proposals are moved onto the cars"""
    prob, pred, im_info, calib = synth.rpn_head(9, 20, 20, "rand")
    bv, _, b3 = oracle.proposal_layer_3d(prob, pred, im_info, calib, "TRAIN", [8, ], [1.0, 1.0])
    bv, b3 = bv.copy(), b3.copy()
    gt = hand_gt([[20, 30, 36, 69, 1], [60, 100, 98, 116, 1], [100, 20, 116, 58, 1], [110, 90, 148, 106, 1], [40, 120, 56, 158, 1]])
    r = np.random.RandomState(19)
    for i in range(min(len(bv), 40)):
        bv[i, 1:] = gt[0][i % 5, :4] + np.floor(r.uniform(-3, 3, 4))
    return bv, b3, gt, calib


def proposal_cases(oracle):
    out = {}
    bv, b3, gt5, calib = base_proposals(oracle)

    def add(name, rois, gt, seed, nc=2, **train):
        out["pt_" + name] = dict(kind="proposal", rois_bv=np.ascontiguousarray(rois[0], F32).reshape(-1, 5),
                                 rois_3d=np.ascontiguousarray(rois[1], F32).reshape(-1, 7), gt_bv=gt[0], gt_3d=gt[1],
                                 gt_corners=gt[2], calib=calib, num_classes=nc, train=dict(TRAIN_DEFAULTS, **train), seed=seed)
        return out["pt_" + name]

    add("only_gt_R0", (bv[:0], b3[:0]), gt5, 101)
    add("only_gt_R1", (bv[:1], b3[:1]), gt5, 102)
    for S in (1, 7, 17, 100):
        add("odd_S_%d" % S, (bv, b3), gt5, 110 + S, BATCH_SIZE=S, BG_THRESH_LO=0.0)
    add("empty_fg", (bv, b3), gt5, 121, FG_THRESH=1.5)
    add("empty_bg", (bv, b3), gt5, 122, BG_THRESH_LO=0.5, BG_THRESH_HI=0.5)
    add("empty_both", (bv, b3), gt5, 123, FG_THRESH=1.5, BG_THRESH_LO=0.5, BG_THRESH_HI=0.5)
    # an overlap equal to a threshold: proposal 0 is ground-truth box 0 moved by (3, 2) pixels; few enough candidates that all are
    # sampled, so the membership of the tied proposal shows in the outputs
    tgt = hand_gt([[40, 50, 56, 89, 1], [100, 30, 139, 46, 1]])
    trois = hand_rois([[43, 52, 59, 91], [100, 32, 139, 48], [5, 5, 20, 20], [40, 70, 56, 109], [110, 30, 149, 46], [44, 60, 50, 70]])
    v = iou_pair(trois[0][0, 1:5], tgt[0][0, :4])
    others = {"FG_THRESH": dict(), "BG_THRESH_HI": dict(FG_THRESH=0.7), "BG_THRESH_LO": dict(FG_THRESH=0.95, BG_THRESH_HI=0.9)}
    for key, short in (("FG_THRESH", "fg"), ("BG_THRESH_HI", "hi"), ("BG_THRESH_LO", "lo")):
        for tag, d in TIE_SHIFTS:
            c = add("tie_%s_%s" % (short, tag), trois, tgt, 131, **dict(others[key], **{key: _neighbour(v, d)}))
            c["tie"] = v
    # class slots
    g4 = hand_gt([[20, 30, 36, 69, 1], [60, 100, 98, 116, 2], [100, 20, 116, 58, 3], [110, 90, 148, 106, 2], [40, 120, 56, 158, 3]])
    add("classes_4", (bv, b3), g4, 141, nc=4)
    g0 = hand_gt([[20, 30, 36, 69, 0], [60, 100, 98, 116, 1], [100, 20, 116, 58, 1], [110, 90, 148, 106, 1], [40, 120, 56, 158, 1]])
    add("classes_0", (bv, b3), g0, 142)
    # ties for the argmax: BEV row 0 twice with different corners and class; proposal 2 overlaps nothing (box 0, maximum 0),
    # background exactly when BG_THRESH_LO <= 0
    gd = hand_gt([[40, 50, 56, 89, 2], [40, 50, 56, 89, 1], [100, 30, 139, 46, 1]])
    gd[2][0, :24] += F32(0.25)
    gd[1][0, :6] = [52.5, 25.0, -1.0, 4.25, 1.5, 1.75]
    add("argmax_ties_lo0", trois, gd, 151, nc=3, BG_THRESH_LO=0.0)
    add("argmax_ties_lo01", trois, gd, 151, nc=3)
    # a ground-truth row whose corners 0 and 6 coincide: its ROIs' targets divide by a zero diagonal
    gz = tuple(a.copy() for a in tgt)
    gz[2][0, [6, 14, 22]] = gz[2][0, [0, 8, 16]]
    add("zero_diagonal", trois, gz, 161)
    # TARGET_MAX_GT
    add("g_limit", (bv, b3), scaled_cars(171, 1024, 20, 20), 171)
    return out


_CASES = None


def cases(oracle):
    """name -> case; built once.  `oracle` is the CPU oracle module (its proposal layer makes the proposal blobs)."""
    global _CASES
    if _CASES is None:
        _CASES = dict(anchor_cases(), **proposal_cases(oracle))
        for c in _CASES.values():
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _CASES


def case_inputs_sha(c):
    keys = ("im_info", "gt_bv", "gt_3d") if c["kind"] == "anchor" else ("rois_bv", "rois_3d", "gt_bv", "gt_3d", "gt_corners", "calib")
    return synth.sha256(*[c[k] for k in keys])


# names only (no oracle needed to enumerate: the table's keys are fixed by the code above)
AT_NAMES = (["grid_%dx%d_%s" % (H, W, s) for H, W in GRIDS for s in ("full", "cut")] +
            ["clobber_default", "clobber_03", "noclobber_03", "tie_pos_at", "tie_pos_above", "tie_neg_at", "tie_neg_below",
             "tie_neg_above", "flood", "argmax_ties", "degenerate_inverted", "degenerate_pixel", "nothing_inside",
             "no_subsampling", "batch_shape", "g_limit"])
PT_NAMES = (["only_gt_R0", "only_gt_R1"] + ["odd_S_%d" % S for S in (1, 7, 17, 100)] + ["empty_fg", "empty_bg", "empty_both"] +
            ["tie_%s_%s" % (k, t) for k in ("fg", "hi", "lo") for t, _ in TIE_SHIFTS] +
            ["classes_4", "classes_0", "argmax_ties_lo0", "argmax_ties_lo01", "zero_diagonal", "g_limit"])
ALL_NAMES = ["at_" + n for n in AT_NAMES] + ["pt_" + n for n in PT_NAMES]


# ------------------------------------------------------------------ the restatement (numpy f64, from the definition)
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def restate_anchor_stage1(c):
    """Everything before the first draw: inside set, the N x G overlap matrix, the label rules."""
    H, W = c["grid"]
    T = c["train"]
    info = c["im_info"].reshape(-1).astype(np.float64)
    A = all_anchors(H, W)
    inside = np.where((A[:, 0] >= 0) & (A[:, 1] >= 0) & (A[:, 2] < info[1]) & (A[:, 3] < info[0]))[0]
    anc = A[inside]
    ov = iou_matrix(anc, c["gt_bv"][:, :4])
    n = len(inside)
    labels = np.full(n, -1, F32)
    if n:
        argmax, mx, gtmax = ov.argmax(axis=1), ov.max(axis=1), ov.max(axis=0)
        flood = np.where(ov == gtmax)[0]
    else:                                    # (the reference raises here; the header defines: nothing labelled)
        argmax, mx, flood = np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64)
    neg, pos = T["RPN_NEGATIVE_OVERLAP"], T["RPN_POSITIVE_OVERLAP"]
    if not T["RPN_CLOBBER_POSITIVES"]:
        labels[(0 < mx) & (mx < neg)] = 0
    labels[flood] = 1
    labels[mx >= pos] = 1
    if T["RPN_CLOBBER_POSITIVES"]:
        labels[mx < neg] = 0
    fg = np.where(labels == 1)[0]
    return dict(N=len(A), inside=inside, anchors=anc, ov=ov, argmax=argmax, mx=mx, labels=labels,
                counts=(n, len(fg), int((labels == 0).sum()), int((mx < neg).sum())), fg_hi=(mx[fg] >= neg).astype(np.uint8))


def restate_anchor(c, oracle, lists=None):
    """(rpn_labels (N,), rpn_bbox_targets (N,6), anchors (M,5), anchors_3d (M,7)) f32 + the positions disabled by the three
    draws.  lists = (dis_fg, dis_bg1, dis_bg2) replaces the draws (positions in the fg / bg / low lists)."""
    T = c["train"]
    s = restate_anchor_stage1(c)
    labels, mx, anc, inside = s["labels"].copy(), s["mx"], s["anchors"], s["inside"]
    B, neg = T["RPN_BATCHSIZE"], T["RPN_NEGATIVE_OVERLAP"]
    dis = [np.zeros(0, np.int64)] * 3

    def subsample(k, keep):
        cand = np.where(labels == (1 if k == 0 else 0))[0]
        if lists is not None:
            dis[k] = np.asarray(lists[k] if lists[k] is not None else [], np.int64)
        elif len(cand) > keep:
            dis[k] = npr.permutation(len(cand))[:len(cand) - keep]
        labels[cand[dis[k]]] = -1

    subsample(0, int(T["RPN_FG_FRACTION"] * B))
    subsample(1, B - int((labels == 1).sum()))
    sel = np.where(labels != -1)[0]
    a3 = np.zeros((len(anc), 6), np.float64)
    if len(anc):
        oracle.lib().mv3d_ref_bv_anchor_to_lidar(_ptr(np.ascontiguousarray(anc, np.int64)), C.c_int(len(anc)), _ptr(a3))
    zeros = np.zeros((len(sel), 1), F32)
    anchors = np.hstack((zeros, anc[sel])).astype(F32)
    anchors_3d = np.hstack((zeros, a3[sel])).astype(F32)
    labels[mx < neg] = 0
    subsample(2, B - int((labels == 1).sum()))
    g = c["gt_3d"].astype(np.float64)[s["argmax"]]
    with np.errstate(all="ignore"):
        tg = np.stack([(g[:, 0] - a3[:, 0]) / a3[:, 4], (g[:, 1] - a3[:, 1]) / a3[:, 3], (g[:, 2] - a3[:, 2]) / a3[:, 5],
                       oracle.log(g[:, 3] / a3[:, 3]), oracle.log(g[:, 4] / a3[:, 4]), oracle.log(g[:, 5] / a3[:, 5])],
                      1).astype(F32) if len(anc) else np.zeros((0, 6), F32)
    rpn_labels = np.full(s["N"], -1, F32)
    rpn_labels[inside] = labels
    rpn_targets = np.zeros((s["N"], 6), F32)
    rpn_targets[inside] = tg
    return (rpn_labels, rpn_targets, anchors, anchors_3d), dis


def restate_proposal_stage1(c, frame_index=0):
    T = c["train"]
    G = c["gt_bv"].shape[0]
    col = np.full((G, 1), frame_index, F32)
    all_bv = np.vstack((c["rois_bv"], np.hstack((col, c["gt_bv"][:, :4]))))
    all_3d = np.vstack((c["rois_3d"], np.hstack((col, c["gt_3d"][:, :6]))))
    ov = iou_matrix(all_bv[:, 1:5], c["gt_bv"][:, :4])
    assign, mx = ov.argmax(axis=1), ov.max(axis=1)
    fg = np.where(mx >= T["FG_THRESH"])[0]
    bg = np.where((mx < T["BG_THRESH_HI"]) & (mx >= T["BG_THRESH_LO"]))[0]
    return dict(all_bv=all_bv, all_3d=all_3d, ov=ov, assign=assign, mx=mx, fg=fg, bg=bg, counts=(len(all_bv), len(fg), len(bg)))


def draw_rois(T, n_fg, n_bg):
    """the two choices of _sample_rois_3d as positions in the candidate lists: numpy's legacy choice without replacement is
    permutation(n)[:k], and is only called on a non-empty list"""
    rois_per_image = T["BATCH_SIZE"] // 1
    fg_n = int(min(np.round(T["FG_FRACTION"] * rois_per_image), n_fg))
    fg_pick = npr.permutation(n_fg)[:fg_n] if n_fg > 0 else np.zeros(0, np.int64)
    bg_n = int(min(rois_per_image - fg_n, n_bg))
    bg_pick = npr.permutation(n_bg)[:bg_n] if n_bg > 0 else np.zeros(0, np.int64)
    return fg_pick, bg_pick


def restate_proposal(c, oracle, frame_index=0, picks=None):
    """(rois_bv, rois_img, labels, bbox_targets, rois_3d) and the picks; `picks` replaces the draws."""
    s = restate_proposal_stage1(c, frame_index)
    fg_pick, bg_pick = picks if picks is not None else draw_rois(c["train"], len(s["fg"]), len(s["bg"]))
    fg_n = len(fg_pick)
    keep = np.append(s["fg"][fg_pick], s["bg"][bg_pick]).astype(np.int64)
    S, nc = len(keep), c["num_classes"]
    labels = c["gt_bv"][s["assign"][keep], 4].copy()
    labels[fg_n:] = 0
    rois_bv, rois_3d = s["all_bv"][keep], s["all_3d"][keep]
    cnr = oracle.lidar_3d_to_corners(rois_3d[:, 1:7])
    tg = np.zeros((S, 24), F32)
    if S:
        gsel = np.ascontiguousarray(c["gt_corners"][s["assign"][keep], :24], F32)
        oracle.lib().mv3d_ref_bbox_transform_cnr(_ptr(np.ascontiguousarray(cnr, F32)), _ptr(gsel), C.c_int(S), _ptr(tg))
    clss = labels.astype(np.uint16)
    slots = np.zeros((S, nc, 24), F32)
    own = np.where(clss > 0)[0]
    slots[own, clss[own]] = tg[own]
    img = oracle.lidar_cnr_to_img(cnr, c["calib"]) if S else np.zeros((0, 4), np.int32)
    rois_img = np.hstack((rois_bv[:, :1].astype(np.float64), img.astype(np.float64))).astype(F32)
    return (rois_bv.reshape(-1, 5).astype(F32), rois_img.reshape(-1, 5), labels.reshape(-1, 1).astype(np.int32),
            slots.reshape(S, 24 * nc), rois_3d.reshape(-1, 7).astype(F32)), (fg_pick, bg_pick)


# ------------------------------------------------------------------ running one case through a description
def run_seeded(c, fn):
    """fn() under the case's seed -> (outputs, the next value of numpy's global stream)"""
    np.random.seed(c["seed"])
    out = fn()
    return tuple(out), int(np.random.randint(1 << 30))


def oracle_call(c, oracle):
    if c["kind"] == "anchor":
        H, W = c["grid"]
        return lambda: oracle.anchor_target_layer(np.zeros((1, H, W, 8), F32), c["gt_bv"], c["gt_3d"], c["im_info"], [8, ],
                                                  [1.0, 1.0], train=c["train"])
    return lambda: oracle.proposal_target_layer_3d(c["rois_bv"], c["rois_3d"], c["gt_bv"], c["gt_3d"], c["gt_corners"], c["calib"],
                                                   c["num_classes"], train=c["train"])


def restate_call(c, oracle):
    return lambda: (restate_anchor if c["kind"] == "anchor" else restate_proposal)(c, oracle)[0]


_MEMO = {}


def described(name, which, oracle):
    """(outputs, rng) of the oracle / the restatement for a case: computed once, shared by the tests, never modified"""
    key = (name, which)
    if key not in _MEMO:
        c = cases(oracle)[name]
        with np.errstate(all="ignore"):
            out, pos = run_seeded(c, (oracle_call if which == "oracle" else restate_call)(c, oracle))
        for a in out:
            a.setflags(write=False)
        _MEMO[key] = (out, pos)
    return _MEMO[key]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def assert_same_outputs(got, want, what):
    assert len(got) == len(want), what
    for k, (x, y) in enumerate(zip(got, want)):
        assert same(x, y), "%s: output %d differs" % (what, k)


def recorded_form(field, a):
    """an output in the form the fixture stores it"""
    a = np.asarray(a)
    if field == "labels" and a.dtype != np.int32:                  # the anchor layer's {-1, 0, 1} in f32
        assert np.array_equal(a, a.astype(np.int8))
        return a.astype(np.int8)
    return np.ascontiguousarray(a)


RECORD_ARRAY_BYTES = 16384        # larger outputs are stored as synth.sha256


def assert_matches_recording(g, name, fields, out, pos, what):
    assert int(g["%s__rng" % name]) == pos, "%s: %s leaves numpy's stream elsewhere than the reference" % (name, what)
    for f, a in zip(fields, out):
        a = recorded_form(f, a)
        if "%s__%s" % (name, f) in g.files:
            assert same(a, g["%s__%s" % (name, f)]), "%s: %s of %s differs from the reference" % (name, f, what)
        else:
            assert synth.sha256(a) == str(g["%s__%s__sha" % (name, f)]), "%s: %s of %s differs from the reference" % (name, f, what)


def fields_of(c):
    return AT_FIELDS if c["kind"] == "anchor" else PT_FIELDS


# ------------------------------------------------------------------ tests that need no GPU
def test_case_table_is_what_the_names_say(oracle):
    assert list(cases(oracle)) == ALL_NAMES
    assert oracle.TRAIN == TRAIN_DEFAULTS
    from mv3d_tf_amd.fast_rcnn.config import cfg
    assert {k: cfg.TRAIN[k] for k in TRAIN_DEFAULTS} == TRAIN_DEFAULTS
    for c in cases(oracle).values():
        if c["kind"] == "anchor":
            assert max(c["grid"]) <= 76


def test_every_case_is_in_the_fixture_or_listed(oracle):
    """each case is recorded, or the reference raised on it and the type is listed here; at most a quarter may be left out"""
    g = golden(FIXTURE)
    assert [str(n) for n in g["case_names"]] == ALL_NAMES
    raised = {}
    for name, c in cases(oracle).items():
        assert str(g["%s__inputs_sha" % name]) == case_inputs_sha(c), name
        if "exc__" + name in g.files:
            raised[name] = str(g["exc__" + name])
        else:
            assert "%s__rng" % name in g.files, name
    assert raised == REFERENCE_RAISES
    assert 4 * len(raised) <= len(ALL_NAMES)


@pytest.mark.parametrize("name", ALL_NAMES)
def test_oracle_matches_the_recording(oracle, name):
    g = golden(FIXTURE)
    if name in REFERENCE_RAISES:
        assert str(g["exc__" + name]) == REFERENCE_RAISES[name]
        return
    out, pos = described(name, "oracle", oracle)
    assert_matches_recording(g, name, fields_of(cases(oracle)[name]), out, pos, "the oracle")


@pytest.mark.parametrize("name", ALL_NAMES)
def test_restatement_matches_the_oracle(oracle, name):
    out, pos = described(name, "restate", oracle)
    ref, ref_pos = described(name, "oracle", oracle)
    assert pos == ref_pos, name
    assert_same_outputs(out, ref, name)


def test_flood_and_large_draw(oracle):
    c = cases(oracle)["at_flood"]
    H, W = c["grid"]
    lab = oracle.anchor_target_stage1(H, W, c["gt_bv"], c["gt_3d"], c["im_info"], 8, c["train"])[3]
    s = restate_anchor_stage1(c)
    assert int((lab == 1).sum()) > 4064 and s["counts"][1] == int((lab == 1).sum())
    assert s["ov"][:, 1].max() == 0.0 and s["ov"][:, 0].max() > 0.5      # the far box overlaps nothing, the car is ordinary


def test_argmax_ties_are_real(oracle):
    s = restate_anchor_stage1(cases(oracle)["at_argmax_ties"])
    ov, mx = s["ov"], s["mx"]
    assert np.any((ov[:, 0] == mx) & (ov[:, 1] == mx) & (mx > 0))            # the duplicated box
    mirrored = (ov[:, 2] == mx) & (ov[:, 3] == mx) & (mx > 0)                # two different boxes
    assert np.any(mirrored) and np.all(s["argmax"][mirrored] == 2)
    gt3 = cases(oracle)["at_argmax_ties"]["gt_3d"]
    assert not np.array_equal(gt3[0], gt3[1])
    p = restate_proposal_stage1(cases(oracle)["pt_argmax_ties_lo0"])
    assert np.any((p["ov"][:, 0] == p["mx"]) & (p["ov"][:, 1] == p["mx"]) & (p["mx"] > 0))
    assert p["mx"][2] == 0.0 and p["assign"][2] == 0                           # the proposal that overlaps nothing
    for name, member in (("pt_argmax_ties_lo0", True), ("pt_argmax_ties_lo01", False)):
        assert (2 in restate_proposal_stage1(cases(oracle)[name])["bg"]) == member


def test_clobber_case_has_ties_below_the_threshold(oracle):
    s = restate_anchor_stage1(cases(oracle)["at_clobber_03"])
    gtmax = s["ov"].max(axis=0)
    low = np.where((gtmax > 0) & (gtmax < 0.3))[0]
    assert len(low) and any((s["ov"][:, g] == gtmax[g]).sum() > 1 for g in low)
    # they are positives without clobber and negatives with it
    tied = np.where(s["ov"][:, low[0]] == gtmax[low[0]])[0]
    assert np.all(s["labels"][tied] == 0)
    assert np.all(restate_anchor_stage1(cases(oracle)["at_noclobber_03"])["labels"][tied] == 1)


@pytest.mark.parametrize("name", [n for n in ALL_NAMES if "_tie_" in n])
def test_threshold_tie_is_attained(oracle, name):
    """an attained maximal overlap is bit-equal to the case's value, and the threshold under test is it or a neighbouring double"""
    c = cases(oracle)[name]
    v = c["tie"]
    s = restate_anchor_stage1(c) if c["kind"] == "anchor" else restate_proposal_stage1(c)
    assert np.any(s["mx"] == v)
    key = {"pos": "RPN_POSITIVE_OVERLAP", "neg": "RPN_NEGATIVE_OVERLAP", "fg": "FG_THRESH", "hi": "BG_THRESH_HI",
           "lo": "BG_THRESH_LO"}[name.split("_")[2]]
    t = c["train"][key]
    want = {"at": v, "above": np.nextafter(v, np.inf), "below": np.nextafter(v, -np.inf)}[name.split("_")[3]]
    assert t == want and (name.endswith("_at") or t != v)
    if c["kind"] == "anchor":          # the tied anchor is not its box's best one, so only the threshold decides its label
        tied = np.where(s["mx"] == v)[0]
        assert np.all(s["ov"][tied, 0] < s["ov"][:, 0].max())
        assert s["ov"][:, 1].max() == 1.0                                     # the box that is an anchor


def test_draw_counts_are_what_the_cases_claim(oracle):
    cs = cases(oracle)
    fresh = lambda seed: (np.random.seed(seed), int(np.random.randint(1 << 30)))[1]
    for name in ("at_nothing_inside", "at_no_subsampling"):                    # no draw: the stream has not moved
        assert described(name, "restate", oracle)[1] == fresh(cs[name]["seed"]), name
    out = described("at_nothing_inside", "restate", oracle)[0]
    assert np.all(out[0] == -1) and not out[1].any() and out[2].shape == (0, 5) and out[3].shape == (0, 7)
    assert restate_anchor_stage1(cs["at_no_subsampling"])["counts"][0] == 76
    for S in (1, 7, 17, 100):
        assert described("pt_odd_S_%d" % S, "restate", oracle)[0][0].shape[0] == S
    assert described("pt_empty_both", "restate", oracle)[0][0].shape[0] == 0
    assert described("pt_empty_both", "restate", oracle)[1] == fresh(cs["pt_empty_both"]["seed"])
    assert restate_proposal_stage1(cs["pt_empty_fg"])["counts"][1] == 0 and restate_proposal_stage1(cs["pt_empty_fg"])["counts"][2] > 0
    assert restate_proposal_stage1(cs["pt_empty_bg"])["counts"][2] == 0 and restate_proposal_stage1(cs["pt_empty_bg"])["counts"][1] > 0
    assert cs["pt_only_gt_R0"]["rois_bv"].shape == (0, 5) and cs["pt_only_gt_R1"]["rois_bv"].shape == (1, 5)
    assert cs["at_g_limit"]["gt_bv"].shape[0] == 1024 and cs["pt_g_limit"]["gt_bv"].shape[0] == 1024
    # class slots: every class of the table is sampled as foreground; class 0 foreground rows have all-zero targets
    lab4 = described("pt_classes_4", "restate", oracle)[0][2].ravel()
    assert set(lab4.tolist()) == {0, 1, 2, 3}
    out0, _ = described("pt_classes_0", "restate", oracle)
    s0 = restate_proposal_stage1(cs["pt_classes_0"])
    np.random.seed(cs["pt_classes_0"]["seed"])
    fg_pick, _ = draw_rois(cs["pt_classes_0"]["train"], len(s0["fg"]), len(s0["bg"]))
    zero_rows = np.where(s0["assign"][s0["fg"][fg_pick]] == 0)[0]
    assert len(zero_rows) and not out0[3][zero_rows].any() and out0[3].any()
    zd = described("pt_zero_diagonal", "restate", oracle)[0][3]
    assert np.isinf(zd).any() or np.isnan(zd).any()


@pytest.mark.parametrize("H,W", GRIDS)
def test_transposed_reading_changes_the_result(oracle, H, W):
    """a kernel (or an oracle) that exchanged rows and columns of the grid, or of im_info, could not pass by luck"""
    for s in ("full", "cut"):
        c = cases(oracle)["at_grid_%dx%d_%s" % (H, W, s)]
        lab = described("at_grid_%dx%d_%s" % (H, W, s), "oracle", oracle)[0][0]
        call = lambda h, w, info: run_seeded(c, lambda: oracle.anchor_target_layer(
            np.zeros((1, h, w, 8), F32), c["gt_bv"], c["gt_3d"], info, [8, ], [1.0, 1.0], train=c["train"]))[0][0]
        assert not np.array_equal(call(W, H, c["im_info"]), lab)
        assert not np.array_equal(call(H, W, c["im_info"][:, [1, 0, 2]]), lab)


# ------------------------------------------------------------------ ABI limits (no device call is made)
@pytest.fixture(scope="module")
def hiplib():
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import _lib
    return _lib


def test_more_than_1024_ground_truth_boxes_are_refused(hiplib):
    L = hiplib.lib()
    assert L.mv3d_anchor_target_workspace_bytes(20, 20, 1024) > 0 and L.mv3d_anchor_target_workspace_bytes(20, 20, 1025) == 0
    assert L.mv3d_proposal_target_workspace_bytes(100, 1024) > 0 and L.mv3d_proposal_target_workspace_bytes(100, 1025) == 0
    host = np.zeros(4096, np.uint8)                      # non-NULL arguments; refused before anything is read or launched
    P = C.c_void_p(host.ctypes.data)
    ap = hiplib.AnchorTargetParams(8, 0, 0.5, 0.7)
    assert L.mv3d_anchor_target_stage1(20, 20, P, P, P, 1025, C.byref(ap), P, P, P, P, P, C.c_size_t(1 << 30), None) == hiplib.ERR_INVALID_ARG
    one = (C.c_void_p * 1)(host.ctypes.data)
    G = (C.c_int * 1)(1025)
    assert L.mv3d_anchor_target_stage1_batch(1, 20, 20, P, one, one, G, C.byref(ap), P, P, one, one, one, C.c_size_t(1 << 30),
                                             None) == hiplib.ERR_INVALID_ARG
    tp = hiplib.ProposalTargetParams(2, 0, 0.5, 0.5, 0.1)
    assert L.mv3d_proposal_target_stage1(P, P, 100, P, P, 1025, C.byref(tp), P, P, C.c_size_t(1 << 30), None) == hiplib.ERR_INVALID_ARG
    R, sz = (C.c_int * 1)(100), (C.c_size_t * 1)(1 << 30)
    assert L.mv3d_proposal_target_stage1_batch(1, one, one, R, one, one, G, C.byref(tp), one, one, sz, None) == hiplib.ERR_INVALID_ARG
    assert L.mv3d_proposal_target_stage1_batch_devn(1, one, one, R, one, one, one, G, C.byref(tp), one, one, sz,
                                                    None) == hiplib.ERR_INVALID_ARG


# ------------------------------------------------------------------ the device
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


@pytest.fixture(scope="module")
def ops(torch_cuda):
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops as o
    return o


def patch_train(monkeypatch, c):
    from mv3d_tf_amd.fast_rcnn.config import cfg
    for k, v in c["train"].items():
        monkeypatch.setattr(cfg.TRAIN, k, v)


def compare_device(name, oracle, out, pos):
    c = cases(oracle)[name]
    want, want_pos = described(name, "oracle", oracle)
    assert pos == want_pos, "%s: numpy's stream after the device layer" % name
    assert_same_outputs(out, want, name)
    if name not in REFERENCE_RAISES:
        assert_matches_recording(golden(FIXTURE), name, fields_of(c), out, pos, "the device")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["at_" + n for n in AT_NAMES])
def test_anchor_target_layer_on_the_device(ops, oracle, monkeypatch, name):
    from mv3d_tf_amd.rpn_msr.anchor_target_layer_tf import anchor_target_layer
    c = cases(oracle)[name]
    patch_train(monkeypatch, c)
    H, W = c["grid"]
    for rep in range(2):                                  # the second call meets the dirty cached workspace
        out, pos = run_seeded(c, lambda: anchor_target_layer(np.zeros((1, H, W, 8), F32), c["gt_bv"], c["gt_3d"], c["im_info"],
                                                             [8, ], [1.0, 1.0]))
        compare_device(name, oracle, out, pos)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pt_" + n for n in PT_NAMES])
def test_proposal_target_layer_on_the_device(ops, oracle, monkeypatch, name):
    from mv3d_tf_amd.rpn_msr.proposal_target_layer_tf import proposal_target_layer_3d
    c = cases(oracle)[name]
    patch_train(monkeypatch, c)
    out, pos = run_seeded(c, lambda: proposal_target_layer_3d(c["rois_bv"], c["rois_3d"], c["gt_bv"], c["gt_3d"], c["gt_corners"],
                                                              c["calib"], c["num_classes"]))
    compare_device(name, oracle, out, pos)


# ---- the shared ground-truth staging (geometry.h: stage_gt_bv) at its bound, on a grid whose height is not its width
def staging_bound_cases(oracle):
    """G = 1024 integer boxes inside a 56 x 40 map (H, W = 5, 7 at stride 8: N = 140 anchors); the last 16 repeat the first 16
    pixel for pixel with other 3D rows, corners and class, so a first-argmax tie between g and g + 1008 shows in every output
    that follows the assignment.  The proposal layer gets R = 8 proposals, four of them one pixel off a repeated box, and a
    BATCH_SIZE above R + G, all of it open to foreground, with BG_THRESH_LO = 0: every candidate row is sampled, so every row's
    assignment is compared."""
    G, H, W = 1024, 5, 7
    r = np.random.RandomState(1024)
    xs, ys = np.sort(r.randint(0, 8 * W, (G, 2)), 1), np.sort(r.randint(0, 8 * H, (G, 2)), 1)
    rows = np.stack([xs[:, 0], ys[:, 0], xs[:, 1], ys[:, 1], np.ones(G, np.int64)], 1)
    rows[-16:, :4] = rows[:16, :4]
    rows[-16:, 4] = 2
    gt = hand_gt(rows)
    gt[1][-16:, :6] += np.array([0.5, -0.25, 0.125, 0.75, 0.5, 0.25], F32)
    gt[2][-16:, :24] += F32(0.25)
    at = dict(kind="anchor", grid=(H, W), im_info=np.array([[8 * H, 8 * W, 1]], F32), gt_bv=gt[0], gt_3d=gt[1], gt_corners=gt[2],
              train=dict(TRAIN_DEFAULTS), seed=1024)
    near = rows[:4, :4] + np.array([1, 0, 1, 0])
    rois = hand_rois(np.vstack([near, rows[500:504, :4] + np.array([0, 1, 0, 1])]))
    pt = dict(kind="proposal", rois_bv=rois[0], rois_3d=rois[1], gt_bv=gt[0], gt_3d=gt[1], gt_corners=gt[2],
              calib=synth.rpn_head(9, H, W, "rand")[3], num_classes=3, seed=1025,
              train=dict(TRAIN_DEFAULTS, BATCH_SIZE=2048, FG_FRACTION=1.0, BG_THRESH_LO=0.0))
    return at, pt


@pytest.mark.gpu
def test_ground_truth_staging_at_its_bound(ops, oracle, monkeypatch):
    from mv3d_tf_amd.rpn_msr.anchor_target_layer_tf import anchor_target_layer
    from mv3d_tf_amd.rpn_msr.proposal_target_layer_tf import proposal_target_layer_3d
    at, pt = staging_bound_cases(oracle)
    H, W = at["grid"]
    assert at["gt_bv"].shape == (1024, 5) and H * W * 4 == 140 and pt["rois_bv"].shape == (8, 5)
    assert np.array_equal(at["gt_bv"], np.floor(at["gt_bv"])) and np.array_equal(at["gt_bv"][-16:, :4], at["gt_bv"][:16, :4])
    # the ties are real: some inside anchor has its maximum on a repeated box, and the four proposals next to one have theirs there
    A = all_anchors(H, W)
    inside = (A[:, 0] >= 0) & (A[:, 1] >= 0) & (A[:, 2] < 8 * W) & (A[:, 3] < 8 * H)
    assert any(ov.argmax() < 16 and ov[ov.argmax() + 1008] == ov.max() for ov in iou_matrix(A[inside], at["gt_bv"][:, :4]))
    assert all(ov.argmax() < 16 for ov in iou_matrix(pt["rois_bv"][:4, 1:], pt["gt_bv"][:, :4]))
    with np.errstate(all="ignore"):
        want_at, want_pt = run_seeded(at, oracle_call(at, oracle)), run_seeded(pt, oracle_call(pt, oracle))
    assert want_pt[0][0].shape[0] == 8 + 1024                               # every candidate row was sampled
    patch_train(monkeypatch, at)
    got = run_seeded(at, lambda: anchor_target_layer(np.zeros((1, H, W, 8), F32), at["gt_bv"], at["gt_3d"], at["im_info"], [8, ],
                                                     [1.0, 1.0]))
    assert got[1] == want_at[1]
    assert_same_outputs(got[0], want_at[0], "anchor_target_layer at G = 1024")
    patch_train(monkeypatch, pt)
    got = run_seeded(pt, lambda: proposal_target_layer_3d(pt["rois_bv"], pt["rois_3d"], pt["gt_bv"], pt["gt_3d"], pt["gt_corners"],
                                                          pt["calib"], pt["num_classes"]))
    assert got[1] == want_pt[1]
    assert_same_outputs(got[0], want_pt[0], "proposal_target_layer_3d at G = 1024")


# ---- the C entries directly
def dev(torch, a, dtype=None):
    return torch.as_tensor(np.array(a, order="C"), dtype=dtype).cuda()        # a copy: the table's arrays are read-only


def ptrs(ts):
    return (C.c_void_p * len(ts))(*[0 if t is None else t.data_ptr() for t in ts])


def ints(vs):
    return (C.c_int * len(vs))(*[int(v) for v in vs])


def dirty(torch, nbytes):
    """a buffer of 0xFF bytes: NaN as f32 / f64, -1 as i32"""
    return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device="cuda")


def anchor_params(ops, c):
    from mv3d_tf_amd._lib import AnchorTargetParams
    T = c["train"]
    return AnchorTargetParams(8, 1 if T["RPN_CLOBBER_POSITIVES"] else 0, float(T["RPN_NEGATIVE_OVERLAP"]),
                              float(T["RPN_POSITIVE_OVERLAP"]))


class AnchorFrame:
    """device buffers of one frame for the per-frame entries, everything the kernels write pre-filled with 0xFF"""

    def __init__(self, ops, torch, c, ws_bytes=None):
        from mv3d_tf_amd._lib import check, lib
        self.c, self.ops, self.check, self.L = c, ops, check, lib()
        self.H, self.W = c["grid"]
        self.N, self.G = self.H * self.W * 4, c["gt_bv"].shape[0]
        self.p = anchor_params(ops, c)
        self.info, self.gt_bv, self.gt_3d = dev(torch, c["im_info"].reshape(-1)[:3]), dev(torch, c["gt_bv"]), dev(torch, c["gt_3d"])
        self.ws = dirty(torch, ws_bytes or self.L.mv3d_anchor_target_workspace_bytes(self.H, self.W, self.G))
        self.cf = dirty(torch, 32 + self.N)
        self.labels = dirty(torch, 4 * self.N).view(torch.float32)[:self.N]
        self.targets = dirty(torch, 24 * self.N).view(torch.float32)[:6 * self.N].view(self.N, 6)

    def stage1(self):
        P = self.ops._ptr
        self.check(self.L.mv3d_anchor_target_stage1(self.H, self.W, P(self.info), P(self.gt_bv), P(self.gt_3d), self.G, C.byref(self.p),
                                                    P(self.labels), P(self.targets), P(self.cf[:32]), P(self.cf[32:]), P(self.ws),
                                                    C.c_size_t(self.ws.numel()), self.ops._stream()), "mv3d_anchor_target_stage1")
        counts = self.cf[:32].cpu().numpy().view(np.int32)
        return tuple(int(v) for v in counts[:4]), self.cf[32:32 + int(counts[1])].cpu().numpy()


STAGE1_CASES = ["at_flood", "at_clobber_default", "at_clobber_03", "at_noclobber_03"] + \
               ["at_grid_%dx%d_%s" % (H, W, s) for H, W in GRIDS for s in ("full", "cut")]


@pytest.mark.gpu
@pytest.mark.parametrize("name", STAGE1_CASES)
def test_anchor_stage1_on_a_dirty_workspace(ops, torch_cuda, oracle, name):
    c = cases(oracle)[name]
    f = AnchorFrame(ops, torch_cuda, c)
    counts, fg_hi = f.stage1()
    s = restate_anchor_stage1(c)
    assert counts == s["counts"]
    assert np.array_equal(fg_hi, s["fg_hi"])
    lab = np.full(s["N"], -1, F32)
    lab[s["inside"]] = s["labels"]
    assert np.array_equal(f.labels.cpu().numpy(), lab)


@pytest.mark.gpu
def test_anchor_batch_entries_equal_the_per_frame_entries(ops, torch_cuda, oracle, monkeypatch):
    """four frames of one 40 x 40 grid (G = 1, G = 300, the flood, the argmax ties) behind one launch of every kernel, on dirty
    workspaces, against the per-frame entries given the same disable lists (drawn by the host layer from the per-frame counts)"""
    from mv3d_tf_amd._lib import check, lib
    from mv3d_tf_amd.rpn_msr.anchor_target_layer_tf import draw_subsamples
    torch, L, P = torch_cuda, lib(), ops._ptr
    cs = cases(oracle)
    flood, ties = cs["at_flood"], cs["at_argmax_ties"]
    assert flood["grid"] == ties["grid"] == (40, 40) and np.array_equal(flood["im_info"], ties["im_info"])
    one = dict(flood, gt_bv=flood["gt_bv"][:1], gt_3d=flood["gt_3d"][:1])
    many = scaled_cars(300, 300, 40, 40)
    frames = [one, dict(flood, gt_bv=many[0], gt_3d=many[1]), flood, ties]
    patch_train(monkeypatch, flood)
    H, W, B, cap = 40, 40, len(frames), 256
    N = H * W * 4
    ws_bytes = L.mv3d_anchor_target_workspace_bytes(H, W, 300)
    per, lists = [], []
    np.random.seed(7)
    for c in frames:
        f = AnchorFrame(ops, torch, c)
        counts, _ = f.stage1()
        dis = draw_subsamples(f.cf, f.cf[32:], N)
        dl = [None if d is None or not len(d) else dev(torch, np.asarray(d, np.int32)) for d in dis]
        for d, limit in zip(dl, counts[1:]):              # every list is a valid one: positions below the reported counts
            assert d is None or (int(d.min()) >= 0 and int(d.max()) < limit)
        f.anchors, f.anchors_3d = dirty(torch, cap * 20).view(torch.float32).view(cap, 5), dirty(torch, cap * 28).view(torch.float32).view(cap, 7)
        f.n_anc = dirty(torch, 4).view(torch.int32)[:1]
        check(L.mv3d_anchor_target_stage2(H, W, C.byref(f.p), P(dl[0]), 0 if dl[0] is None else dl[0].numel(), P(dl[1]),
                                          0 if dl[1] is None else dl[1].numel(), P(dl[2]), 0 if dl[2] is None else dl[2].numel(),
                                          P(f.labels), P(f.anchors), P(f.anchors_3d), P(f.n_anc), cap, P(f.ws),
                                          C.c_size_t(f.ws.numel()), ops._stream()), "mv3d_anchor_target_stage2")
        per.append(f)
        lists.append(dl)
    assert per[2].cf[:32].cpu().numpy().view(np.int32)[1] > 4064
    # the same four frames behind the batched entries
    info = dev(torch, np.concatenate([c["im_info"].reshape(-1)[:3] for c in frames]))
    labels = dirty(torch, 4 * B * N).view(torch.float32).view(B, N)
    targets = dirty(torch, 24 * B * N).view(torch.float32).view(B, N, 6)
    cfs, wss = [dirty(torch, 32 + N) for _ in frames], [dirty(torch, ws_bytes) for _ in frames]
    anchors, anchors_3d = dirty(torch, B * cap * 20).view(torch.float32).view(B, cap, 5), dirty(torch, B * cap * 28).view(torch.float32).view(B, cap, 7)
    n_anc = dirty(torch, 4 * B).view(torch.int32)[:B]
    p = per[0].p
    a_ws = ptrs(wss)
    check(L.mv3d_anchor_target_stage1_batch(B, H, W, P(info), ptrs([f.gt_bv for f in per]), ptrs([f.gt_3d for f in per]),
                                            ints([f.G for f in per]), C.byref(p), P(labels), P(targets), ptrs([x[:32] for x in cfs]),
                                            ptrs([x[32:] for x in cfs]), a_ws, C.c_size_t(ws_bytes), ops._stream()),
          "mv3d_anchor_target_stage1_batch")
    n_of = lambda k: ints([0 if dl[k] is None else dl[k].numel() for dl in lists])
    check(L.mv3d_anchor_target_stage2_batch(B, H, W, C.byref(p), ptrs([dl[0] for dl in lists]), n_of(0), ptrs([dl[1] for dl in lists]),
                                            n_of(1), ptrs([dl[2] for dl in lists]), n_of(2), P(labels), P(anchors), P(anchors_3d),
                                            P(n_anc), cap, a_ws, C.c_size_t(ws_bytes), ops._stream()), "mv3d_anchor_target_stage2_batch")
    for b, f in enumerate(per):
        counts = f.cf[:32].cpu().numpy().view(np.int32)[:4]
        assert np.array_equal(cfs[b][:32].cpu().numpy().view(np.int32)[:4], counts), b
        assert torch.equal(cfs[b][32:32 + int(counts[1])], f.cf[32:32 + int(counts[1])]), b
        assert torch.equal(labels[b], f.labels) and torch.equal(targets[b], f.targets), b
        m = int(f.n_anc.item())
        assert int(n_anc[b].item()) == m and 0 < m <= 128, b
        assert torch.equal(anchors[b, :m], f.anchors[:m]) and torch.equal(anchors_3d[b, :m], f.anchors_3d[:m]), b
        # and the per-frame result is the restatement's under the same lists
        host = lambda d: None if d is None else d.cpu().numpy()
        want, _ = restate_anchor(frames[b], oracle, lists=[host(d) for d in lists[b]])
        got = (f.labels.cpu().numpy(), f.targets.cpu().numpy(), f.anchors[:m].cpu().numpy(), f.anchors_3d[:m].cpu().numpy())
        assert_same_outputs(got, want, "frame %d" % b)


def target_params(c, frame_index=0):
    from mv3d_tf_amd._lib import ProposalTargetParams
    T = c["train"]
    return ProposalTargetParams(int(c["num_classes"]), frame_index, float(T["FG_THRESH"]), float(T["BG_THRESH_HI"]),
                                float(T["BG_THRESH_LO"]))


class TargetFrame:
    """device buffers of one frame of the proposal-target entries; `cap` rows of proposals, the rows from `rows` on are NaN"""

    def __init__(self, torch, L, c, frame_index=0, cap=None, rows=None, with_fv=False):
        self.c, self.torch = c, torch
        R = c["rois_bv"].shape[0]
        self.cap = R if cap is None else cap
        self.rows = self.cap if rows is None else rows
        bv, b3 = np.full((self.cap, 5), np.nan, F32), np.full((self.cap, 7), np.nan, F32)
        bv[:self.rows], b3[:self.rows] = c["rois_bv"][:self.rows], c["rois_3d"][:self.rows]
        bv[:self.rows, 0] = b3[:self.rows, 0] = frame_index
        self.host = dict(c, rois_bv=bv[:self.rows], rois_3d=b3[:self.rows])
        self.G = c["gt_bv"].shape[0]
        self.bv, self.b3 = dev(torch, bv), dev(torch, b3)
        self.gt_bv, self.gt_3d, self.gt_cnr, self.calib = (dev(torch, c[k]) for k in ("gt_bv", "gt_3d", "gt_corners", "calib"))
        self.p = target_params(c, frame_index)
        self.counts = dirty(torch, 16).view(torch.int32)[:4]
        self.with_fv = with_fv

    def workspace(self, L, num_rois):
        self.ws = dirty(self.torch, L.mv3d_proposal_target_workspace_bytes(num_rois, self.G))
        return self.ws

    def outputs(self, S):
        t, nc = self.torch, self.c["num_classes"]
        f32 = lambda n: dirty(t, 4 * S * n).view(t.float32)[:S * n].view(S, n)
        self.out = [f32(5), f32(5), dirty(t, 4 * S).view(t.int32)[:S].view(S, 1), f32(24 * nc), f32(7)]
        self.fv = f32(5) if self.with_fv else None
        return self.out

    def picks(self, fg_pick, bg_pick):
        self.n_fg, self.n_bg = len(fg_pick), len(bg_pick)
        self.fg_pick = dev(self.torch, np.asarray(fg_pick, np.int32)) if self.n_fg else None
        self.bg_pick = dev(self.torch, np.asarray(bg_pick, np.int32)) if self.n_bg else None

    def results(self):
        return tuple(o.cpu().numpy() for o in self.out)


def stage1_args(frames, devn=None):
    a = [len(frames), ptrs([f.bv for f in frames]), ptrs([f.b3 for f in frames]), ints([f.cap if devn else f.rows for f in frames])]
    if devn:
        a.append(ptrs(devn))
    from mv3d_tf_amd._lib import ProposalTargetParams
    par = (ProposalTargetParams * len(frames))(*[f.p for f in frames])
    a += [ptrs([f.gt_bv for f in frames]), ptrs([f.gt_3d for f in frames]), ints([f.G for f in frames]), par,
          ptrs([f.counts for f in frames]), ptrs([f.ws for f in frames]), (C.c_size_t * len(frames))(*[f.ws.numel() for f in frames])]
    return a


def stage2_args(frames, devn=None):
    a = [len(frames), ptrs([f.bv for f in frames]), ptrs([f.b3 for f in frames]), ints([f.cap if devn else f.rows for f in frames])]
    if devn:
        a.append(ptrs(devn))
    from mv3d_tf_amd._lib import ProposalTargetParams
    par = (ProposalTargetParams * len(frames))(*[f.p for f in frames])
    a += [ptrs([f.gt_bv for f in frames]), ptrs([f.gt_3d for f in frames]), ptrs([f.gt_cnr for f in frames]), ints([f.G for f in frames]),
          ptrs([f.calib for f in frames]), par, ptrs([f.fg_pick for f in frames]), ints([f.n_fg for f in frames]),
          ptrs([f.bg_pick for f in frames]), ints([f.n_bg for f in frames])]
    a += [ptrs([f.out[k] for f in frames]) for k in range(5)]
    a += [ptrs([f.fv for f in frames]) if any(f.fv is not None for f in frames) else None,
          ptrs([f.ws for f in frames]), (C.c_size_t * len(frames))(*[f.ws.numel() for f in frames])]
    return a


@pytest.mark.gpu
def test_proposal_target_device_counts_are_clamped(ops, torch_cuda, oracle):
    """the _devn entries with the proposals' number on the device: counts of 0, cap - 3, cap, cap + 5 and -2 in one launch, NaN
    rows behind each count, against the host-count entries called with min(max(n, 0), cap) rows"""
    from mv3d_tf_amd._lib import check, lib
    torch, L, P = torch_cuda, lib(), ops._ptr
    c = dict(cases(oracle)["pt_odd_S_100"])
    cap = 40
    c["rois_bv"], c["rois_3d"] = c["rois_bv"][:cap], c["rois_3d"][:cap]
    given = [0, cap - 3, cap, cap + 5, -2]
    eff = [min(max(n, 0), cap) for n in given]
    frames = [TargetFrame(torch, L, c, cap=cap, rows=e) for e in eff]
    n_dev = [dev(torch, np.array([n], np.int32)) for n in given]
    for f in frames:
        f.workspace(L, cap)
    check(L.mv3d_proposal_target_stage1_batch_devn(*stage1_args(frames, devn=n_dev), ops._stream()), "stage1_batch_devn")
    rs = np.random.RandomState(5)
    hosts = []
    for f, e in zip(frames, eff):
        counts = f.counts.cpu().numpy()
        s = restate_proposal_stage1(f.host)
        assert counts[0] == e + f.G and tuple(counts[:3]) == s["counts"]
        h = TargetFrame(torch, L, c, cap=cap, rows=e)      # the host-count entry on the same buffers' first e rows
        h.workspace(L, e)
        check(L.mv3d_proposal_target_stage1(P(h.bv), P(h.b3), e, P(h.gt_bv), P(h.gt_3d), h.G, C.byref(h.p), P(h.counts), P(h.ws),
                                            C.c_size_t(h.ws.numel()), ops._stream()), "stage1")
        assert np.array_equal(h.counts.cpu().numpy()[:3], counts[:3])
        fg_pick = rs.permutation(int(counts[1]))[:min(32, int(counts[1]))]       # valid picks: positions below the counts
        bg_pick = rs.permutation(int(counts[2]))[:min(96, int(counts[2]))]
        for x in (f, h):
            x.picks(fg_pick, bg_pick)
            x.outputs(len(fg_pick) + len(bg_pick))
        hosts.append(h)
    check(L.mv3d_proposal_target_stage2_batch_devn(*stage2_args(frames, devn=n_dev), ops._stream()), "stage2_batch_devn")
    for f, h in zip(frames, hosts):
        check(L.mv3d_proposal_target_stage2(P(h.bv), P(h.b3), h.rows, P(h.gt_bv), P(h.gt_3d), P(h.gt_cnr), h.G, P(h.calib), C.byref(h.p),
                                            P(h.fg_pick), h.n_fg, P(h.bg_pick), h.n_bg, *[P(o) for o in h.out], P(h.ws),
                                            C.c_size_t(h.ws.numel()), ops._stream()), "stage2")
        assert h.n_fg > 0 and h.n_fg + h.n_bg > 0
        assert_same_outputs(f.results(), h.results(), "count %d" % f.rows)
        want, _ = restate_proposal(f.host, oracle, picks=(np.asarray(f.fg_pick.cpu()), np.zeros(0, np.int64) if f.bg_pick is None
                                                           else np.asarray(f.bg_pick.cpu())))
        assert_same_outputs(f.results(), want, "count %d against the restatement" % f.rows)


@pytest.mark.gpu
def test_proposal_target_batch_frame_index_and_front_view(ops, torch_cuda, oracle):
    """three frames with S = 1, 17 and 100 and ragged G in one launch of mv3d_proposal_target_stage1/2_batch: the appended
    ground-truth rows carry the frame's index, rois_fv_out is mv3d_rois_3d_to_fv of rois_3d_out, every output is the restatement's"""
    from mv3d_tf_amd._lib import check, lib
    torch, L = torch_cuda, lib()
    cs = cases(oracle)
    frames_c = [dict(cs["pt_odd_S_1"]), dict(cs["pt_odd_S_17"]), dict(cs["pt_odd_S_100"])]
    for k in ("gt_bv", "gt_3d", "gt_corners"):
        frames_c[1][k] = frames_c[1][k][:2]
    frames = [TargetFrame(torch, L, c, frame_index=b, with_fv=True) for b, c in enumerate(frames_c)]
    for f in frames:
        f.workspace(L, f.rows)
    check(L.mv3d_proposal_target_stage1_batch(*stage1_args(frames), ops._stream()), "stage1_batch")
    np.random.seed(23)
    want, gt_rows = [], []
    for b, f in enumerate(frames):
        s = restate_proposal_stage1(f.host, frame_index=b)
        assert tuple(f.counts.cpu().numpy()[:3]) == s["counts"]
        picks = draw_rois(f.c["train"], s["counts"][1], s["counts"][2])
        gt_rows.append(np.where(np.append(s["fg"][picks[0]], s["bg"][picks[1]]) >= f.rows)[0])    # sampled appended rows
        f.picks(*picks)
        f.outputs(len(picks[0]) + len(picks[1]))
        want.append(restate_proposal(f.host, oracle, frame_index=b, picks=picks)[0])
    assert [f.n_fg + f.n_bg for f in frames] == [1, 17, 100]
    assert len(gt_rows[2]) > 0                              # under this seed the last frame samples ground-truth rows
    check(L.mv3d_proposal_target_stage2_batch(*stage2_args(frames), ops._stream()), "stage2_batch")
    for b, f in enumerate(frames):
        got = f.results()
        assert_same_outputs(got, want[b], "frame %d" % b)
        assert np.all(got[0][:, 0] == b) and np.all(got[1][:, 0] == b) and np.all(got[4][:, 0] == b)
        for r in gt_rows[b]:                                # the appended ground-truth rows carry the frame's index
            assert got[0][r, 0] == b and got[4][r, 0] == b
            assert (got[0][r, 1:5] == f.c["gt_bv"][:, :4]).all(-1).any()
        assert torch.equal(f.fv, ops.rois_3d_to_fv(f.out[4]))
        assert np.array_equal(f.fv.cpu().numpy(), oracle.rois_3d_to_fv(got[4]))
