"""Ignore regions in training (not in the reference, off by default): ops.ignore_relabel / mv3d_ignore_relabel,
ops.rcnn_loss(ignore_label=-1) / mv3d_rcnn_loss_ignore, the dataset's ignore arrays and their mirror, and cfg.TRAIN.IGNORE_TYPES through
the TRAIN graph and one SolverWrapper step -- against the numpy statement of the rule in tests/ignore_regions_restatement.py.  Every
comparison of the relabelling is bit-equality of all four outputs (labels, labels, counts, status).

CPU tests (no mark): the restatement's anchor image box against the oracle's proposal decode at zero deltas, the rule's arithmetic at
its edges, the config keys, and the entry's argument checks that never touch a device."""
import ctypes as C
import types

import numpy as np
import pytest

from conftest import golden
from mv3d_tf_amd import synth

import ignore_regions_restatement as R

gpu = pytest.mark.gpu
F32 = np.float32
CALIB = synth.KITTI_CALIB.astype(F32)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def ops(torch_cuda):
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops as o
    return o


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == F32 else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ cases
def make_case(seed, B, H, W, S, K, M, labelled=24, calib=None):
    """rpn_labels (B, 4HW) all -1 but `labelled` per frame in {0, 1}; S ROI rows with random frames, labels in {0, 1} and boxes in the
    map / image; K[b] BEV and M[b] image ignore boxes per frame, large enough that some candidates fall on them"""
    r = np.random.RandomState(seed)
    N = 4 * H * W
    rpn = np.full((B, N), -1, F32)
    for b in range(B):
        at = r.choice(N, min(labelled, N), replace=False)
        rpn[b, at] = (r.random_sample(len(at)) < 0.25).astype(F32)
    side = 8.0 * max(H, W)

    def boxes(n, span):
        x1, y1 = r.uniform(-10, span, n), r.uniform(-10, span, n)
        return np.stack([x1, y1, x1 + r.uniform(2, span / 2, n), y1 + r.uniform(2, span / 2, n)], 1).astype(F32)

    frame = r.randint(0, B, S).astype(F32)
    rois_bv = np.hstack([frame[:, None], np.round(boxes(S, side))]).astype(F32)
    rois_img = np.hstack([frame[:, None], np.round(boxes(S, 600.0))]).astype(F32)
    roi = (r.random_sample((S, 1)) < 0.25).astype(np.int32)
    ign_bv = [boxes(K[b], side) for b in range(B)]
    ign_img = [boxes(M[b], 600.0) * F32(2) for b in range(B)]
    cal = np.stack([CALIB if calib is None else calib[b] for b in range(B)]).astype(F32)
    return dict(rpn=rpn, roi=roi, rois_bv=rois_bv, rois_img=rois_img, calib=cal, H=H, W=W, ign_bv=ign_bv, ign_img=ign_img)


def pack(frames):
    off = np.zeros(len(frames) + 1, np.int32)
    off[1:] = np.cumsum([len(f) for f in frames])
    return (np.concatenate(frames, 0) if frames else np.zeros((0, 4), F32)).astype(F32).reshape(-1, 4), off


def restated(c, T, packed=None):
    (rb, ob), (ri, oi) = packed or (pack(c["ign_bv"]), pack(c["ign_img"]))
    return R.relabel(c["rpn"], c["roi"], c["rois_bv"], c["rois_img"], c["calib"], c["H"], c["W"], rb, ob, ri, oi, T)


def run(ops, torch, c, T, packed=None, want=None):
    """the product on case c; asserts bit-equality of all four outputs with the restatement and that the inputs stay as they were"""
    dev = lambda a: torch.as_tensor(a).cuda()
    ins = [dev(c[k]) for k in ("rpn", "roi", "rois_bv", "rois_img", "calib")]
    lists = ((c["ign_bv"], c["ign_img"]) if packed is None else packed)
    out = ops.ignore_relabel(*ins, c["H"], c["W"], lists[0], lists[1], T, want_counts=True)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in out]
    want = want or restated(c, T, packed)
    for name, g, w in zip(("rpn_labels", "roi_labels", "counts", "status"), got, want):
        assert same(g, w), (name, np.flatnonzero(bits(g).reshape(-1) != bits(w).reshape(-1))[:8])
    for k, t in zip(("rpn", "roi", "rois_bv", "rois_img", "calib"), ins):
        assert same(t.cpu().numpy(), c[k]), k                                   # out of place: nothing written into the inputs
    return got


# ------------------------------------------------------------------ CPU: the restatement and the rule
def test_restated_anchor_image_box_equals_the_oracle_decode_at_zero_deltas(oracle):
    """the oracle's proposal layer decodes anchor + deltas and projects the box; at zero deltas its `img` is the anchor's own image box"""
    H = W = 6
    N = 4 * H * W
    prob = np.zeros((1, H, W, 8), F32)
    pred = np.zeros((1, H, W, 24), F32)
    dbg = oracle.proposal_layer_3d(prob, pred, np.array([[8 * H, 8 * W, 1]], F32), CALIB, "TRAIN", debug=True)[3]
    M = R.proj_matrix(CALIB)
    mine = np.array([R.anchor_image_box(M, n, W, 8) for n in range(N)], np.int64)
    assert np.array_equal(mine, dbg["img"].astype(np.int64))
    assert len(np.unique(mine, axis=0)) > N // 8


def test_rule_arithmetic_at_its_edges():
    c = (0.0, 0.0, 9.0, 9.0)                                                    # 10 x 10
    assert R.ioa(c, (5, -3, 20, 30)) == 0.5 and R.ioa(c, (6, -3, 20, 30)) == 0.4
    assert R.ioa(c, (5, 5, 20, 20)) == 0.25 and R.ioa(c, (0, 0, 9, 9)) == 1.0 and R.ioa(c, (-50, -50, 50, 50)) == 1.0
    assert R.ioa(c, (10, 0, 20, 9)) == 0.0 and R.ioa(c, (9, 9, 20, 20)) == 0.01
    nan = float("nan")
    assert R.ioa(c, (nan, 0, 9, 9)) == 0.0 and R.ioa((0, 0, nan, 9), (0, 0, 9, 9)) == 0.0
    assert R.ioa(c, (9, 0, 0, 9)) == 0.0 and R.ioa((9, 0, 0, 9), (-50, -50, 50, 50)) == 0.0      # x2 < x1 on either side
    assert R.ioa((R.INT32_MIN,) * 4, (-1e6, -1e6, 1e6, 1e6)) == 0.0                               # an image box that came from NaN
    assert R.grid_anchor(4 * (2 * 7 + 3) + 1, 7, 8) == (-5 + 24, -2 + 16, 5 + 24, 3 + 16)


def test_config_keys(tmp_path):
    from mv3d_tf_amd.fast_rcnn import config
    cfg = config.cfg
    assert cfg.TRAIN.IGNORE_TYPES == () and cfg.TRAIN.IGNORE_OVERLAP == 0.5
    saved = dict(cfg.TRAIN)
    try:
        p = tmp_path / "ign.yml"
        p.write_text("TRAIN:\n  IGNORE_TYPES: [Van, DontCare]\n  IGNORE_OVERLAP: 0.25\n")
        config.cfg_from_file(str(p))
        assert cfg.TRAIN.IGNORE_TYPES == ("Van", "DontCare") and cfg.TRAIN.IGNORE_OVERLAP == 0.25
        for text in ("[Van, Lorry]", "[Car]", "[Van, Car]"):
            p.write_text("TRAIN:\n  IGNORE_TYPES: %s\n" % text)
            with pytest.raises(ValueError):
                config.cfg_from_file(str(p))
        assert cfg.TRAIN.IGNORE_TYPES == ("Van", "DontCare")                    # a refused file changes nothing
        p.write_text("TRAIN:\n  IGNORE_TYPES: []\n")
        config.cfg_from_file(str(p))
        assert cfg.TRAIN.IGNORE_TYPES == ()
        config.cfg_from_list(["TRAIN.IGNORE_TYPES", "('Tram', 'Misc')"])
        assert cfg.TRAIN.IGNORE_TYPES == ("Tram", "Misc")
        with pytest.raises(ValueError):
            config.cfg_from_list(["TRAIN.IGNORE_TYPES", "('Car',)"])
    finally:
        cfg.TRAIN.update(saved)


def test_entry_refuses_bad_arguments_before_any_device_call():
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import _lib
    L = _lib.lib()
    A = C.c_void_p(4096)                                                        # a non-NULL "pointer", never dereferenced
    ok = [A, A, A, A, 4, A, 2, 3, 3, 8, A, A, 1, A, A, 1, C.c_double(0.5), A, A, None, None, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.mv3d_ignore_relabel(*a)

    for bad in (dict(_0=None), dict(_17=None), dict(_5=None), dict(_11=None), dict(_14=None), dict(_1=None), dict(_18=None), dict(_2=None),
                dict(_3=None), dict(_10=None), dict(_13=None), dict(_6=0), dict(_6=65536), dict(_7=0), dict(_8=0), dict(_9=0), dict(_4=-1),
                dict(_12=-1), dict(_15=-1), dict(_7=1 << 15, _8=1 << 15), dict(_9=1 << 30)):
        assert call(**bad) == _lib.ERR_INVALID_ARG, bad
    assert L.mv3d_rcnn_loss_ignore(None, None, None, None, 4, 2, 48, C.c_float(3.0), None, None, None, None, 0, None) == _lib.ERR_INVALID_ARG


# ------------------------------------------------------------------ GPU: the relabelling
@gpu
def test_empty_lists_at_either_end_and_the_real_grid(ops, torch_cuda):
    c = make_case(1, 2, 3, 3, 40, (0, 3), (2, 0), labelled=30)
    got = run(ops, torch_cuda, c, 0.5)
    assert got[2].sum() > 0
    run(ops, torch_cuda, make_case(2, 2, 3, 3, 40, (0, 0), (0, 0), labelled=30), 0.5)     # both lists empty: NULL rows
    c = make_case(3, 1, 76, 76, 128, (6,), (4,), labelled=128)
    got = run(ops, torch_cuda, c, 0.5)
    assert got[2][0, 0] > 0 and got[2][0, 1] > 0 and (got[0] == 0).any() and (got[1] == 0).any()


EDGE = {0.5: ((5, -3, 20, 30), (6, -3, 20, 30)), 0.25: ((5, 5, 20, 20), (6, 5, 20, 20)), 1.0: ((0, 0, 9, 9), (1, 0, 9, 9))}


@gpu
@pytest.mark.parametrize("T", sorted(EDGE))
def test_threshold_edge_on_both_sides(ops, torch_cuda, T):
    """a 10 x 10 ROI whose intersection with the ignore box gives IoA == T exactly is relabelled, one pixel less is not; the same pair in
    the image; and anchor 1 of cell (1, 1) (11 x 6) against a box that covers exactly half / one pixel row less at T = 0.5"""
    hit, miss = EDGE[T]
    for side in ("bv", "img"):
        c = make_case(0, 2, 3, 3, 2, (0, 0), (0, 0), labelled=0)
        c["roi"][:] = 0
        c["rois_bv"][:] = [[0, 0, 0, 9, 9], [1, 0, 0, 9, 9]]
        c["rois_img"][:] = [[0, 0, 0, 9, 9], [1, 0, 0, 9, 9]]
        other = "img" if side == "bv" else "bv"
        c["rois_" + other][:, 1:] += 1000                                       # the other view's box lies nowhere near
        c["ign_" + side] = [np.array([hit], F32), np.array([miss], F32)]
        got = run(ops, torch_cuda, c, T)
        assert got[1].reshape(-1).tolist() == [-1, 0] and got[2].tolist() == [[0, 1], [0, 0]]
    if T == 0.5:
        c = make_case(0, 2, 3, 3, 0, (0, 0), (0, 0), labelled=0)
        n = 4 * (1 * 3 + 1) + 1
        assert R.grid_anchor(n, 3, 8) == (3, 6, 13, 11)
        c["rpn"][:, n] = 0
        c["ign_bv"] = [np.array([[3, 6, 13, 8]], F32), np.array([[3, 6, 13, 7]], F32)]      # 11 x 3 of 11 x 6, then 11 x 2
        got = run(ops, torch_cuda, c, T)
        assert got[0][0, n] == -1 and got[0][1, n] == 0 and got[2].tolist() == [[1, 0], [0, 0]]


@gpu
def test_other_labels_pass_through_bit_for_bit(ops, torch_cuda):
    c = make_case(5, 2, 5, 4, 64, (1, 1), (1, 1), labelled=60)
    everywhere = np.array([[-1e6, -1e6, 1e6, 1e6]], F32)
    c["ign_bv"], c["ign_img"] = [everywhere, everywhere], [everywhere, everywhere]
    nan = np.array([0x7FC01234], np.int32).view(F32)[0]                         # a NaN with a payload
    c["rpn"][0, :6] = [1, -1, 2, nan, 0, -0.0]
    c["roi"][:6, 0] = [1, -1, 2, 7, 0, -2]
    got = run(ops, torch_cuda, c, 0.5)
    assert same(got[0][0, :4], c["rpn"][0, :4]) and got[0][0, 4] == -1 and got[0][0, 5] == -1      # (-0.0 == 0 is background too)
    assert got[1][:4, 0].tolist() == [1, -1, 2, 7] and got[1][4, 0] == -1 and got[1][5, 0] == -2
    # everything that was 0 is -1 now, nothing else moved, and the counts say so
    assert np.array_equal(got[0] == -1, (c["rpn"] == 0) | (c["rpn"] == -1)) and not (got[0] == 0).any()
    assert got[2][:, 0].tolist() == [(c["rpn"][b] == 0).sum() for b in range(2)]
    assert got[2][:, 1].sum() == (c["roi"] == 0).sum()
    # out= from an earlier call is written into, and without want_counts no counts come back
    dev = lambda a: torch_cuda.as_tensor(a).cuda()
    ins = [dev(c[k]) for k in ("rpn", "roi", "rois_bv", "rois_img", "calib")]
    out = ops.ignore_relabel(*ins, c["H"], c["W"], c["ign_bv"], c["ign_img"], 0.5)
    assert out[2] is None
    again = ops.ignore_relabel(*ins, c["H"], c["W"], c["ign_bv"], c["ign_img"], 2.0, out=out)       # T above every IoA: nothing moves
    assert again[0] is out[0] and same(out[0].cpu().numpy(), c["rpn"]) and same(out[1].cpu().numpy(), c["roi"])


@gpu
def test_degenerate_boxes_are_never_ignored_on(ops, torch_cuda):
    nan = float("nan")
    big = [-1e6, -1e6, 1e6, 1e6]
    # ignore boxes with a NaN or x2 < x1: nothing is relabelled
    c = make_case(6, 1, 4, 4, 32, (0,), (0,), labelled=40)
    c["ign_bv"] = [np.array([[nan, -1e6, 1e6, 1e6], [-1e6, -1e6, 1e6, nan], [1e6, -1e6, -1e6, 1e6]], F32)]
    c["ign_img"] = [np.array([[-1e6, nan, 1e6, 1e6], [-1e6, 1e6, 1e6, -1e6]], F32)]
    got = run(ops, torch_cuda, c, 0.5)
    assert got[2].sum() == 0
    # candidate ROIs with x2 < x1 or a NaN on one side are not ignored on that side
    c = make_case(7, 1, 4, 4, 4, (1,), (1,), labelled=0)
    c["roi"][:] = 0
    c["rois_bv"][:] = [[0, 9, 0, 0, 9], [0, 0, 0, 9, 9], [0, nan, 0, 9, 9], [0, 0, 0, 9, 9]]
    c["rois_img"][:] = [[0, 0, 9, 9, 0], [0, 0, 0, 9, nan], [0, 5000, 0, 5009, 9], [0, 5000, 0, 5009, 9]]
    c["ign_bv"], c["ign_img"] = [np.array([[-100, -100, 100, 100]], F32)], [np.array([[-100, -100, 100, 100]], F32)]
    got = run(ops, torch_cuda, c, 0.5)
    assert got[1].reshape(-1).tolist() == [0, -1, 0, -1]
    # an anchor whose image box came from NaN (a NaN calibration) is not ignored on in the image; the frame beside it is
    cal = np.stack([CALIB, CALIB])
    cal[0, 0, 0] = nan
    c = make_case(8, 2, 4, 4, 0, (0, 0), (1, 1), labelled=40, calib=cal)
    c["ign_img"] = [np.array([big], F32), np.array([big], F32)]
    M = R.proj_matrix(cal[0])
    assert R.anchor_image_box(M, 5, 4, 8)[0] == R.INT32_MIN
    got = run(ops, torch_cuda, c, 0.5)
    assert got[2][0, 0] == 0 and got[2][1, 0] == (c["rpn"][1] == 0).sum() > 0
    # ROI rows whose frame column names no frame pass through
    c = make_case(9, 2, 3, 3, 6, (1, 1), (1, 1), labelled=0)
    c["roi"][:] = 0
    c["rois_bv"][:, 0] = [0, 1, 2, -1, 0.5, nan]
    c["ign_bv"] = [np.array([big], F32)] * 2
    got = run(ops, torch_cuda, c, 0.5)
    assert got[1].reshape(-1).tolist() == [-1, -1, 0, 0, 0, 0]


@gpu
@pytest.mark.parametrize("K", [65, 256, 257, 1024])
def test_lists_longer_than_one_stage(ops, torch_cuda, K):
    """the one box that matters is the LAST of the list, so a stage that is dropped or read short shows"""
    c = make_case(10 + K, 2, 5, 5, 48, (K, 3), (2, K), labelled=24)
    for key in ("ign_bv", "ign_img"):
        for b in range(2):
            if len(c[key][b]) == K:
                c[key][b][:-1] = c[key][b][:-1] * F32(0.01) + F32(4000)         # small and far away
                c[key][b][-1] = [-1e5, -1e5, 1e5, 1e5]
    got = run(ops, torch_cuda, c, 0.5)
    assert got[2][0, 0] == (c["rpn"][0] == 0).sum() > 0 and got[2][1, 0] == (c["rpn"][1] == 0).sum() > 0


@gpu
def test_bad_frames_are_written_through_with_a_status(ops, torch_cuda):
    from mv3d_tf_amd import _lib
    everywhere = np.array([[-1e6, -1e6, 1e6, 1e6]], F32)
    for which in ("ign_bv", "ign_img"):
        c = make_case(20, 2, 4, 4, 40, (1, 1), (1, 1), labelled=40)
        c["ign_bv"], c["ign_img"] = [everywhere, everywhere], [everywhere, everywhere]
        c[which] = [np.tile(everywhere, (1025, 1)), everywhere]                 # frame 0: one box too many
        got = run(ops, torch_cuda, c, 0.5)
        assert got[3].tolist() == [_lib.ERR_INVALID_ARG, _lib.OK] and got[2][0].tolist() == [0, 0] and got[2][1].min() > 0
        own = c["rois_bv"][:, 0] == 0
        assert same(got[0][0], c["rpn"][0]) and same(got[1][own], c["roi"][own])
    # offsets that decrease, run past the rows or start below zero, as an already packed pair
    c = make_case(21, 3, 4, 4, 40, (2, 2, 2), (1, 1, 1), labelled=40)
    rows = np.tile(everywhere, (6, 1))
    good = pack(c["ign_img"])
    for off, status in (([0, 5, 3, 6], [0, 1, 0]), ([0, 2, 9, 6], [0, 1, 1]), ([-1, 2, 4, 6], [1, 0, 0]), ([6, 6, 6, 6], [0, 0, 0]),
                        ([0, 2, 4, 1 << 30], [0, 0, 1]), ([7, 7, 7, 7], [1, 1, 1])):
        got = run(ops, torch_cuda, c, 0.5, packed=((rows, np.array(off, np.int32)), good))
        assert got[3].tolist() == status, off
    # the same pair as device tensors is used where it lies
    dev = lambda a: torch_cuda.as_tensor(a).cuda()
    packed = ((dev(rows), dev(np.array([0, 2, 4, 6], np.int32))), (dev(good[0]), dev(good[1])))
    ins = [dev(c[k]) for k in ("rpn", "roi", "rois_bv", "rois_img", "calib")]
    out = ops.ignore_relabel(*ins, 4, 4, packed[0], packed[1], 0.5, want_counts=True)
    want = R.relabel(c["rpn"], c["roi"], c["rois_bv"], c["rois_img"], c["calib"], 4, 4, rows, [0, 2, 4, 6], good[0], good[1], 0.5)
    assert all(same(g.cpu().numpy(), w) for g, w in zip(out, want))


@gpu
def test_no_rois_and_sixteen_frames(ops, torch_cuda):
    run(ops, torch_cuda, make_case(30, 2, 4, 4, 0, (2, 2), (2, 2), labelled=30), 0.5)
    c = make_case(31, 16, 6, 5, 200, tuple(range(16)), tuple(range(15, -1, -1)), labelled=12)
    got = run(ops, torch_cuda, c, 0.5)
    assert (got[2].sum(0) > 0).all()
    # more background labels than the candidate queue holds at once: an unsampled frame, every anchor 0
    c = make_case(32, 1, 50, 50, 0, (1,), (0,), labelled=0)
    c["rpn"][:] = 0
    c["ign_bv"] = [np.array([[100, 100, 300, 300]], F32)]
    R_anchor = np.array([R.ignored(R.grid_anchor(n, 50, 8), c["ign_bv"][0], 0.5) for n in range(10000)])
    want = (np.where(R_anchor, F32(-1), F32(0))[None].astype(F32), c["roi"], np.array([[R_anchor.sum(), 0]], np.int32), np.zeros(1, np.int32))
    got = run(ops, torch_cuda, c, 0.5, want=want)
    assert 0 < got[2][0, 0] < 10000


# ------------------------------------------------------------------ GPU: the loss
def loss_case(seed, R_=5, K=2):
    r = np.random.RandomState(seed)
    z = r.uniform(-4, 4, (R_, K)).astype(F32)
    pred = r.uniform(-1, 1, (R_, 24 * K)).astype(F32)
    tgt = (pred + r.uniform(-0.3, 0.3, pred.shape) * (r.random_sample(pred.shape) < 0.5)).astype(F32)
    return z, r.randint(0, K, R_).astype(np.int32), pred, tgt


@gpu
def test_rcnn_loss_skips_the_ignored_rows(ops, torch_cuda, monkeypatch):
    import optim_loss_restatement as LR
    torch = torch_cuda
    dev = lambda a: torch.as_tensor(a).cuda()
    host = lambda t: t.cpu().numpy()
    z, lab, pred, tgt = loss_case(3)
    lab[[1, 3]] = -1
    keep = lab != -1
    # the module's f32 and f64 statements with the row selection label != -1 for both terms
    monkeypatch.setattr(LR, "_select", lambda labels, rows, rpn: (np.asarray(labels, np.int64).reshape(rows),) + (np.asarray(labels).reshape(rows) != -1,) * 2)
    losses, d_cls, d_pred = (host(t) for t in ops.rcnn_loss(dev(z), dev(lab), dev(pred), dev(tgt), sigma=3.0, ignore_label=-1))
    w_losses, w_cls, w_pred = LR.loss_f32(z, lab, pred, tgt, 3.0, False)
    ref = LR.loss_ref(z, lab, pred, tgt, 3.0, False)
    print("rcnn_loss(ignore_label=-1):", losses, "f32 statement:", w_losses, "f64:", ref["ce"], ref["box"])
    assert np.array_equal(losses, w_losses) and np.array_equal(d_cls, w_cls) and np.array_equal(d_pred, w_pred)
    assert np.allclose(losses, [ref["ce"], ref["box"]], rtol=1e-5, atol=0) and np.allclose(d_cls, ref["d_cls"], rtol=1e-5, atol=1e-7)
    # the gradient rows of the skipped rows are exactly +0.0, and the kept rows are what mv3d_rcnn_loss gives for them alone
    assert not bits(d_cls[~keep]).any() and not bits(d_pred[~keep]).any() and d_cls[keep].all()
    alone = [host(t) for t in ops.rcnn_loss(dev(z[keep]), dev(lab[keep]), dev(pred[keep]), dev(tgt[keep]), sigma=3.0)]
    assert same(losses, alone[0]) and same(d_cls[keep], alone[1]) and same(d_pred[keep], alone[2])
    # mv3d_rcnn_loss itself: a label of -1 stays the poison it is
    assert np.isnan(host(ops.rcnn_loss(dev(z), dev(lab), dev(pred), dev(tgt))[0])[0])
    with pytest.raises(ValueError):
        ops.rcnn_loss(dev(z), dev(lab), dev(pred), dev(tgt), ignore_label=0)


@gpu
@pytest.mark.parametrize("rows", [5, 300])
def test_rcnn_loss_ignore_without_and_with_only_ignored_rows(ops, torch_cuda, rows):
    torch = torch_cuda
    dev = lambda a: torch.as_tensor(a).cuda()
    z, lab, pred, tgt = loss_case(4, rows)
    plain = ops.rcnn_loss(dev(z), dev(lab), dev(pred), dev(tgt))
    flagged = ops.rcnn_loss(dev(z), dev(lab), dev(pred), dev(tgt), ignore_label=-1)
    assert all(same(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(plain, flagged))       # no row at -1: bit-equal
    none = ops.rcnn_loss(dev(z), dev(np.full(rows, -1, np.int32)), dev(pred), dev(tgt), ignore_label=-1)
    assert np.isnan(none[0].cpu().numpy()).all()
    assert not bits(none[1].cpu().numpy()).any() and not bits(none[2].cpu().numpy()).any()
    assert np.array_equal(ops.rcnn_loss(dev(z), dev(lab), dev(pred), dev(tgt), ignore_label=-1, want_grad=False)[0].cpu().numpy(),
                          plain[0].cpu().numpy())


# ------------------------------------------------------------------ GPU: the dataset
LINE = "%s 0 0 %r %r %r %r %r %r %r %r %r %r %r %r"


def label_lines(kinds, box, ry, b2, alpha):
    """label rows type trunc occ alpha x1 y1 x2 y2 h w l tx ty tz ry from camera boxes (tx ty tz l w h)"""
    return [LINE % (k, float(a), float(q[0]), float(q[1]), float(q[2]), float(q[3]), float(b[5]), float(b[4]), float(b[3]), float(b[0]),
                    float(b[1]), float(b[2]), float(r)) for k, a, q, b, r in zip(kinds, alpha, b2, box, ry)]


DONTCARE = ["DontCare -1 -1 -10 503.89 169.71 590.61 190.13 -1 -1 -1 -1000 -1000 -1000 -10",
            "DontCare -1 -1 -10 0.1 0.3333333333333333 1241.99 374.0000001 -1 -1 -1 -1000 -1000 -1000 -10"]


def population(seed, n):
    r = np.random.RandomState(seed)
    box = np.stack([r.uniform(-25, 25, n), r.uniform(0.8, 2.2, n), r.uniform(3, 55, n), r.uniform(2.5, 12, n), r.uniform(1.4, 3, n),
                    r.uniform(1.3, 3.5, n)], 1).astype(F32)
    ry = r.uniform(-np.pi, np.pi, n)
    x1 = r.randint(0, 4000, n) / 4.0
    b2 = np.stack([x1, r.randint(0, 1400, n) / 4.0, x1 + r.randint(4, 800, n) / 4.0, r.randint(1400, 1500, n) / 4.0], 1)
    kinds = np.array(["Car", "Van", "Pedestrian", "Misc"])[np.arange(n) % 4]
    return kinds, box, ry, b2, r.uniform(-np.pi, np.pi, n)


@gpu
def test_dataset_ignore_arrays_and_their_mirror(ops, torch_cuda):
    from test_kitti_formats import ANN_KEYS
    from mv3d_tf_amd.datasets import mirror_annotation, mirror_calib, parse_kitti_labels
    from mv3d_tf_amd.datasets.kitti_mv3d import ignore_blobs
    g = golden("kitti_label")
    table = g["calib_0"]
    tr = table[3].reshape(3, 4).astype(F32)
    cls = {"__background__": 0, "Car": 1}
    kinds, box, ry, b2, alpha = population(2, 200)
    lines = label_lines(kinds, box, ry, b2, alpha)
    lines = lines[:50] + DONTCARE[:1] + lines[50:] + DONTCARE[1:]
    off = parse_kitti_labels(lines, tr, cls, 2)
    assert set(off) == set(ANN_KEYS) | {"flipped"}                              # key off: exactly today's keys
    assert set(parse_kitti_labels(lines, tr, cls, 2, ignore_types=())) == set(off)
    on = parse_kitti_labels(lines, tr, cls, 2, ignore_types=("Van", "DontCare"))
    assert set(on) == set(off) | {"ignore_boxes_bv", "ignore_boxes_3D", "ignore_boxes_img"}
    for k in ANN_KEYS:                                                          # the trained objects do not notice
        assert same(on[k].toarray() if k == "gt_overlaps" else on[k], off[k].toarray() if k == "gt_overlaps" else off[k]), k
    vans = parse_kitti_labels([ln for ln in lines if ln.startswith("Van")], tr, {"__background__": 0, "Van": 1}, 2)
    assert len(vans["boxes_bv"]) == 50 and same(on["ignore_boxes_bv"], vans["boxes_bv"]) and same(on["ignore_boxes_3D"], vans["boxes_3D"])
    text = np.array([ln.split()[4:8] for ln in DONTCARE], np.float64).astype(F32)
    assert same(on["ignore_boxes_img"], text) and on["ignore_boxes_img"][1, 1] == F32(1.0 / 3.0)
    only_dc = parse_kitti_labels(lines, tr, cls, 2, ignore_types=("DontCare",))
    assert only_dc["ignore_boxes_bv"].shape == (0, 4) and same(only_dc["ignore_boxes_img"], text)
    only_van = parse_kitti_labels(lines, tr, cls, 2, ignore_types=("Van",))
    assert only_van["ignore_boxes_img"].shape == (0, 4) and same(only_van["ignore_boxes_bv"], vans["boxes_bv"])
    for bad in (("Lorry",), ("Car",), "Van"):
        with pytest.raises(ValueError):
            parse_kitti_labels(lines, tr, cls, 2, ignore_types=bad)
    blobs = ignore_blobs(on)
    assert same(blobs["ignore_boxes_bv"], on["ignore_boxes_bv"]) and same(blobs["ignore_boxes_img"], on["ignore_boxes_img"])
    with pytest.raises(KeyError):
        ignore_blobs(off)
    for W in (1242, 1224):
        m = mirror_annotation(on, W)
        mm = mirror_annotation(m, W)
        for k in ("ignore_boxes_bv", "ignore_boxes_3D", "ignore_boxes_img"):
            assert same(mm[k], on[k]), k                                        # twice = the identity, bit for bit
            assert m[k] is not on[k] and m[k].dtype == on[k].dtype and m[k].shape == on[k].shape
        x1, y1, x2, y2 = (float(v) for v in text[0])
        assert np.array_equal(m["ignore_boxes_img"][0], np.array([W - 1 - x2, y1, W - 1 - x1, y2]).astype(F32))
        # the mirrored BEV boxes against the encoding of the mirrored label (tx -> -tx, ry -> pi - ry, Tr -> Tr'): the bound
        # tests/test_mirror.py holds `boxes_bv` to -- within one pixel, no more than 1 % of the boxes differing
        box_m = box.copy()
        box_m[:, 0] = -box_m[:, 0]
        wrap = lambda a: np.where(np.pi - a > np.pi, -np.pi - a, np.pi - a)
        b2_m = np.stack([W - b2[:, 2] - 1, b2[:, 1], W - b2[:, 0] - 1, b2[:, 3]], 1)
        tr_m = mirror_calib(table, W)[3].reshape(3, 4).astype(F32)
        want = parse_kitti_labels(label_lines(kinds, box_m, wrap(ry), b2_m, wrap(alpha)), tr_m, cls, 2, ignore_types=("Van",))
        d = np.abs(m["ignore_boxes_bv"].astype(np.float64) - want["ignore_boxes_bv"])
        print("W=%d mirrored ignore_boxes_bv: max difference %g, boxes differing %d of %d" % (W, d.max(), np.count_nonzero(d.max(1)), len(d)))
        assert d.max() <= 1.0 and np.count_nonzero(d.max(1)) <= 0.01 * len(d)
        assert same(m["boxes_bv"], mirror_annotation(off, W)["boxes_bv"])


# ------------------------------------------------------------------ GPU: the graph and one solver step
def training_entry(ops):
    """one synthetic frame: two Cars, three large Vans where the targets draw background, and a DontCare box over the image's left part"""
    from mv3d_tf_amd.datasets import parse_kitti_labels
    g = golden("kitti_label")
    table = g["calib_0"]
    tr = table[3].reshape(3, 4).astype(F32)
    kinds = ["Car", "Car", "Van", "Van", "Van"]
    box = np.array([[-3, 1.6, 15, 3.9, 1.6, 1.5], [6, 1.6, 32, 4.2, 1.7, 1.5], [-14, 1.8, 20, 25, 10, 3], [12, 1.8, 45, 25, 10, 3],
                    [-8, 1.8, 48, 25, 10, 3]], F32)
    ry = np.array([0.1, -1.5, 0.0, 1.57, 0.3])
    b2 = np.array([[100, 40, 140, 70], [180, 35, 200, 50], [0, 30, 60, 90], [250, 30, 300, 60], [120, 30, 160, 50]], np.float64)
    lines = label_lines(kinds, box, ry, b2, ry) + ["DontCare -1 -1 -10 0.0 0.0 150.0 95.0 -1 -1 -1 -1000 -1000 -1000 -10"]
    ann = parse_kitti_labels(lines, tr, {"__background__": 0, "Car": 1}, 2, ignore_types=("Van", "DontCare"))
    r = np.random.RandomState(11)
    ann["image"] = r.randint(0, 255, (96, 320, 3)).astype(np.uint8)
    ann["lidar_bv"] = ((r.random_sample((601, 601, 9)) < 0.02) * r.uniform(0.1, 2.4, (601, 601, 9))).astype(F32)
    ann["calib"] = np.asarray(table)
    ann["max_overlaps"] = np.ones(2, F32)
    return ann


@gpu
def test_train_graph_and_solver_step_with_ignore_types(ops, torch_cuda, tmp_path, monkeypatch):
    torch = torch_cuda
    from mv3d_tf_amd.fast_rcnn import train_mv
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.networks import get_network
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    saved = dict(cfg.TRAIN)
    try:
        cfg.TRAIN.BG_THRESH_LO = 0.0
        entry = training_entry(ops)
        assert len(entry["ignore_boxes_bv"]) == 3 and len(entry["ignore_boxes_img"]) == 1
        net = get_network("MV3D_train")
        net.mfma_trunk, net.amp_dtype = True, None                              # (this library's exact-f32 trunks: no algorithm search)
        np.random.seed(2)
        blobs_off = get_minibatch([entry], 2)
        assert "ignore_boxes_bv" not in blobs_off
        feed_off = dict(train_mv.stack_blobs([blobs_off, blobs_off]), keep_prob=1.0)
        np.random.seed(5)
        L = net.forward(feed_off)
        torch.cuda.synchronize()
        state_off = np.random.get_state()
        assert "ignored" not in L
        off = dict(rpn=L["rpn_data"][0].cpu().numpy().copy(), roi=L["roi_data_3d"][2].cpu().numpy().copy(),
                   rois_bv=L["roi_data_3d"][0].cpu().numpy().copy(), rois_img=L["roi_data_3d"][1].cpu().numpy().copy())
        h, w = L["rpn_cls_score"].shape[1:3]
        cfg.TRAIN.IGNORE_TYPES = ("Van", "DontCare")
        with pytest.raises(ValueError, match="ignore_boxes"):
            net.forward(feed_off)                                               # the key is on and the feed has no ignore blobs
        np.random.seed(2)
        blobs_on = get_minibatch([entry], 2)
        assert set(blobs_on) == set(blobs_off) | {"ignore_boxes_bv", "ignore_boxes_img"}
        feed_on = dict(train_mv.stack_blobs([blobs_on, blobs_on]), keep_prob=1.0)
        assert len(feed_on["ignore_boxes_bv"]) == 2 and feed_on["ignore_boxes_bv"][1].shape == (3, 4)
        np.random.seed(5)
        L = net.forward(feed_on)
        torch.cuda.synchronize()
        state_on = np.random.get_state()
        assert all(np.array_equal(a, b) for a, b in zip(state_off[1:], state_on[1:]))        # the draws did not notice
        cal = np.stack([np.asarray(entry["calib"], F32)] * 2)
        (rb, ob), (ri, oi) = pack([entry["ignore_boxes_bv"]] * 2), pack([entry["ignore_boxes_img"]] * 2)
        want = R.relabel(off["rpn"], off["roi"], off["rois_bv"], off["rois_img"], cal, h, w, rb, ob, ri, oi, cfg.TRAIN.IGNORE_OVERLAP)
        print("relabelled (anchors, ROIs) per frame:", want[2].tolist(), "of", (off["rpn"] == 0).sum(1).tolist(), "background anchors and",
              (off["roi"] == 0).sum(), "background ROIs")
        assert want[2][:, 0].sum() >= 1 and want[2][:, 1].sum() >= 1            # the frame was chosen so that the rule alone relabels both kinds
        assert same(L["rpn_data"][0].cpu().numpy(), want[0]) and same(L["roi_data_3d"][2].cpu().numpy(), want[1])
        assert same(L["ignored"].cpu().numpy(), want[2]) and not L["ignore_status"].cpu().numpy().any()
        assert same(L["roi_data_3d"][0].cpu().numpy(), off["rois_bv"])
        loss, parts = train_mv.total_loss(L)
        assert np.isfinite(float(loss.detach())) and all(np.isfinite(float(p.detach())) for p in parts)
        # one SolverWrapper step on the frame under the key, and its display line
        cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.DISPLAY, cfg.TRAIN.MFMA_TRUNK = 1, 1, True
        monkeypatch.setattr(train_mv.SolverWrapper, "snapshot", lambda self, sess, it: None)
        sw = train_mv.SolverWrapper(None, None, net, types.SimpleNamespace(num_classes=2), [entry], str(tmp_path / "out"))
        lines = []
        sw.log = lines.append
        np.random.seed(5)
        hist = sw.train_model(None, 1)
        assert len(hist) == 1 and np.isfinite(hist[0]).all()
        shown = [ln for ln in lines if ln.startswith("ignored:")]
        assert len(shown) == 1 and int(shown[0].split()[1]) >= 1, lines
        cfg.TRAIN.IGNORE_TYPES = ()
        lines.clear()
        sw.train_model(None, 1)
        assert not any("ignored" in ln for ln in lines)                         # key off: the log is as before
    finally:
        cfg.TRAIN.update(saved)
