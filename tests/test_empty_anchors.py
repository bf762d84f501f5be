"""The MV3D paper's empty-anchor removal (section 3.2; not in the reference, off by default): the occupancy kernel, the masked
proposal layer / anchor target layer / train path, and the two cfg switches in the graphs -- against the numpy restatement of
tests/empty_anchor_restatement.py on top of the unchanged oracle.  Every comparison is np.array_equal.

CPU tests (no mark): the restatement itself against the oracle (all-ones mask == oracle.anchor_target_stage1; the -200 size
deltas make the oracle's `valid` flags equal valid & mask)."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from mv3d_tf_amd import synth
from test_oracle_golden import AT_CASES, proposal_case

import empty_anchor_restatement as R

gpu = pytest.mark.gpu
PROPOSAL_FIXTURES = ["proposal3d_20_TRAIN_peaky", "proposal3d_76_TEST_rand", "proposal3d_75_TRAIN_rand", "proposal3d_76_TRAIN_peaky"]
SECTIONS = {"TRAIN": dict(RPN_PRE_NMS_TOP_N=12000, RPN_POST_NMS_TOP_N=2000, RPN_NMS_THRESH=0.7, RPN_MIN_SIZE=5),
            "TEST": dict(RPN_PRE_NMS_TOP_N=6000, RPN_POST_NMS_TOP_N=300, RPN_NMS_THRESH=0.7, RPN_MIN_SIZE=5)}   # (the end2end yml's TEST)


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


_scans = {}


def scan(oracle, seed, P):
    """the synthetic scan's 601 x 601 x 9 map, computed once and shared (never modified)"""
    key = (seed, P)
    if key not in _scans:
        top = oracle.point_cloud_2_top(synth.point_cloud(seed, P))
        top.setflags(write=False)
        _scans[key] = top
    return _scans[key]


_masks = {}


def scan_mask(oracle, seed, P, H):
    key = (seed, P, H)
    if key not in _masks:
        _masks[key] = R.anchor_mask(oracle, scan(oracle, seed, P), H, H)
    return _masks[key]


# ------------------------------------------------------------------ CPU: the restatement against the oracle
@pytest.mark.parametrize("name", AT_CASES)
def test_restated_labels_with_all_ones_mask_equal_the_oracle(oracle, name):
    g = golden(name)
    H = int(g["H"])
    inds, max_ov, labels, targets = R.masked_stage1(oracle, H, H, g["gt_bv"], g["gt_3d"], g["im_info"], np.ones(4 * H * H, np.uint8))
    o_inds, _, o_max, o_lab, o_tg = oracle.anchor_target_stage1(H, H, g["gt_bv"], g["gt_3d"], g["im_info"])
    assert np.array_equal(inds, o_inds) and np.array_equal(labels, o_lab) and np.array_equal(max_ov, o_max)
    assert np.array_equal(targets, o_tg)


@pytest.mark.parametrize("name", PROPOSAL_FIXTURES)
def test_minus_200_size_deltas_take_exactly_the_masked_anchors_out(oracle, name):
    g, (prob, pred, info, calib), _ = proposal_case(name)
    H = int(g["H"])
    N = 4 * H * H
    valid = oracle.proposal_layer_3d(prob, pred, info, calib, "TRAIN", [8, ], debug=True)[3]["valid"].astype(bool)
    assert valid.any()
    rng = np.random.RandomState(7)
    for share in (0.0, 0.5, 0.9, 1.0):
        mask = (rng.random_sample(N) >= share).astype(np.uint8)
        got = oracle.proposal_layer_3d(prob, R.masked_pred(pred, mask), info, calib, "TRAIN", [8, ], debug=True)[3]["valid"].astype(bool)
        assert np.array_equal(got, valid & mask.astype(bool))


def test_restated_counts_on_a_hand_made_map(oracle):
    """3 x 3 grid at stride 8 over a 20 x 24 map: anchor (h=1, w=1, a=1) is the box x 3..13, y 6..11"""
    bev = np.zeros((20, 24, 2), np.float32)
    bev[6, 3, 1] = 1.0; bev[11, 13, 0] = -2.0; bev[5, 8, 0] = 1.0; bev[12, 8, 0] = 1.0; bev[8, 2, 0] = 1.0; bev[8, 14, 0] = 1.0
    bev[9, 9, 0] = -0.0
    n = (1 * 3 + 1) * 4 + 1
    assert R.all_anchors(oracle, 3, 3)[n].tolist() == [3, 6, 13, 11]
    assert R.anchor_counts(oracle, bev, 3, 3)[n] == 2
    assert R.anchor_mask(oracle, bev, 3, 3, min_cells=2)[n] == 1 and R.anchor_mask(oracle, bev, 3, 3, min_cells=3)[n] == 0


def test_switches_default_to_the_reference():
    from mv3d_tf_amd.fast_rcnn.config import cfg
    for sec in (cfg.TRAIN, cfg.TEST):
        assert sec.RPN_SKIP_EMPTY_ANCHORS is False and sec.RPN_EMPTY_ANCHOR_MIN_CELLS == 1


def test_occupancy_entry_refuses_bad_arguments_before_any_device_call():
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import _lib
    L, A, bad, ws = _lib.lib(), 4096, _lib.ERR_INVALID_ARG, 1 << 30
    occ = L.mv3d_anchor_occupancy
    ok = dict(bev=A, batch=1, mh=601, mw=601, c=9, H=76, W=76, stride=8, mc=1, mask=A, count=None, wsp=A, wsz=ws)
    call = lambda **kw: occ(*[dict(ok, **kw)[k] for k in ok], None)
    for kw in (dict(bev=None), dict(mask=None), dict(wsp=None), dict(batch=0), dict(batch=65536), dict(mh=0), dict(mh=4097), dict(mw=0),
               dict(mw=4097), dict(c=0), dict(c=65), dict(stride=0), dict(mc=0), dict(H=129, W=128), dict(bev=A + 2)):
        assert call(**kw) == bad, kw
    assert call(wsz=16) == _lib.ERR_WORKSPACE and call(wsp=A + 16) == _lib.ERR_WORKSPACE
    assert L.mv3d_anchor_occupancy_workspace_bytes(1, 601, 601) >= 601 * 602 * 2
    assert L.mv3d_anchor_occupancy_workspace_bytes(0, 601, 601) == 0 and L.mv3d_anchor_occupancy_workspace_bytes(1, 4097, 601) == 0
    p = _lib.ProposalParams(8, 12000, 2000, 375, 1242, 50, 0, 0, 0.7, 5.0)
    assert L.mv3d_proposal_3d_masked(None, None, 1, 76, 76, None, None, C.byref(p), None, None, None, None, None, None, None, 0, None) == bad
    assert L.mv3d_anchor_target_stage1_batch_masked(0, 76, 76, *([None] * 11), 0, None) == bad
    assert L.mv3d_train_path_submit_masked(None, 0, *([None] * 11)) == bad


# ------------------------------------------------------------------ 1. occupancy
def special_map(oracle, Hm, Wm, Cc, H, W):
    """one occupied cell at each map corner; around one anchor that lies inside the map single cells exactly ON and one pixel
    OUTSIDE each of its four edges; cells holding only -0.0 (empty), only a NaN, only a subnormal, only channel C - 1 (occupied)"""
    bev = np.zeros((Hm, Wm, Cc), np.float32)
    for y, x in ((0, 0), (0, Wm - 1), (Hm - 1, 0), (Hm - 1, Wm - 1)):
        bev[y, x, 0] = 1.0
    a = R.all_anchors(oracle, H, W)
    inside = np.where((a[:, 0] >= 1) & (a[:, 1] >= 1) & (a[:, 2] < Wm - 1) & (a[:, 3] < Hm - 1))[0]
    if len(inside):
        x1, y1, x2, y2 = a[inside[len(inside) // 2]]
        ym, xm = (y1 + y2) // 2, (x1 + x2) // 2
        bev[ym, x1, Cc - 1] = 1.0; bev[ym, x1 - 1, 0] = 1.0                     # left edge: on (last channel alone), outside
        bev[ym, x2, 0] = np.nan; bev[ym, x2 + 1, 0] = 1.0                       # right edge: on (a NaN alone), outside
        bev[y1, xm, 0] = np.float32(1e-42); bev[y1 - 1, xm, 0] = 1.0            # top edge: on (a subnormal alone), outside
        bev[y2, xm, 0] = -3.0; bev[y2 + 1, xm, 0] = 1.0                         # bottom edge
        bev[ym, xm, :] = -0.0                                                   # every channel -0.0: empty
    bev[Hm // 2, Wm // 3, :] = -0.0
    return bev


def run_occupancy(ops, torch, oracle, frames, H, W, misalign=False):
    bev = np.stack(frames)
    if misalign:                                                                # a batch that starts 4 bytes behind a 16-byte boundary
        buf = torch.empty(bev.size + 1, dtype=torch.float32, device="cuda")
        t = buf[1:].view(bev.shape)
        t.copy_(torch.as_tensor(bev))
        assert t.data_ptr() % 16 == 4
    else:
        t = torch.as_tensor(bev).cuda()
    want = np.stack([R.anchor_counts(oracle, f, H, W) for f in frames])
    for mc in (1, 2, 17):
        mask, counts = ops.anchor_occupancy(t, H, W, 8, mc, want_counts=True)
        assert mask.dtype == torch.uint8 and counts.dtype == torch.int32 and mask.shape == (len(frames), 4 * H * W)
        assert np.array_equal(counts.cpu().numpy(), want)
        assert np.array_equal(mask.cpu().numpy(), (want >= mc).astype(np.uint8))
    only = ops.anchor_occupancy(t, H, W, 8, 2)                                  # (no counts asked for)
    assert np.array_equal(only.cpu().numpy(), (want >= 2).astype(np.uint8))
    return want


@gpu
@pytest.mark.parametrize("Hm,Wm,Cc,H", [(37, 53, 1, 20), (37, 53, 3, 20), (37, 53, 9, 20), (37, 53, 9, 5), (160, 160, 9, 20)])
def test_occupancy_small_maps(ops, torch_cuda, oracle, Hm, Wm, Cc, H):
    rng = np.random.RandomState(Hm + Cc)
    full = rng.uniform(0.5, 2.0, (Hm, Wm, Cc)).astype(np.float32)
    sparse = (rng.uniform(-1, 1, (Hm, Wm, Cc)) * (rng.random_sample((Hm, Wm, Cc)) < 0.01)).astype(np.float32)
    last = np.zeros((Hm, Wm, Cc), np.float32)
    last[..., Cc - 1] = (rng.random_sample((Hm, Wm)) < 0.03)
    frames = [np.zeros((Hm, Wm, Cc), np.float32), full, special_map(oracle, Hm, Wm, Cc, H, H), -np.zeros((Hm, Wm, Cc), np.float32), sparse, last]
    for f in frames:                                                            # batch 1
        run_occupancy(ops, torch_cuda, oracle, [f], H, H)
    want = run_occupancy(ops, torch_cuda, oracle, frames[1:3], H, H, misalign=True)           # batch 2
    a = R.all_anchors(oracle, H, H)
    area = np.maximum(np.minimum(a[:, 2], Wm - 1) - np.maximum(a[:, 0], 0) + 1, 0) * np.maximum(np.minimum(a[:, 3], Hm - 1) - np.maximum(a[:, 1], 0) + 1, 0)
    assert np.array_equal(want[0], area)                                        # fully occupied: the count is the clipped area
    run_occupancy(ops, torch_cuda, oracle, [frames[i % len(frames)] for i in range(16)], H, H)   # batch 16


@gpu
@pytest.mark.parametrize("Hm,H", [(601, 75), (601, 76), (601, 80), (608, 76), (601, 20)])
def test_occupancy_kitti_maps(ops, torch_cuda, oracle, Hm, H):
    rng = np.random.RandomState(Hm + H)
    scans = [scan(oracle, 1 + i // 2, (20000, 2000)[i % 2]) for i in range(6)]
    if Hm != 601:
        scans = [np.pad(s, ((0, Hm - 601), (0, Hm - 601), (0, 0))) for s in scans]
    full = rng.uniform(0.5, 2.0, (Hm, Hm, 9)).astype(np.float32)
    frames = scans[:2] + [np.zeros((Hm, Hm, 9), np.float32), full, special_map(oracle, Hm, Hm, 9, H, H)]
    for i, f in enumerate(scans + frames[2:3]):                                 # batch 1: every scan and the all-zero map
        w = run_occupancy(ops, torch_cuda, oracle, [f], H, H)
        if i == 0:
            want = w
        if i < len(scans) and Hm == 601 and H in (75, 76):                      # what was just checked cannot pass trivially
            share = 1.0 - (w[0] >= 1).mean()
            assert 0.05 < share < 0.95, share
    run_occupancy(ops, torch_cuda, oracle, frames[3:5], H, H)                   # batch 2
    if H == 80:
        a = R.all_anchors(oracle, H, H)
        assert ((a[:, 0] > Hm - 1) | (a[:, 1] > Hm - 1)).any()                  # anchors wholly outside the map ...
        assert want.shape == (1, 4 * H * H) and (want[0][(a[:, 0] > Hm - 1) | (a[:, 1] > Hm - 1)] == 0).all()    # ... count 0
    if (Hm, H) in ((601, 76), (608, 76)):
        run_occupancy(ops, torch_cuda, oracle, [(scans + frames[2:])[i % 9] for i in range(16)], H, H)           # batch 16


@gpu
def test_occupancy_out_buffers_are_checked(ops, torch_cuda):
    torch = torch_cuda
    bev = torch.zeros((2, 37, 53, 3), device="cuda")
    N = 4 * 5 * 5
    good = (torch.empty((2, N), dtype=torch.uint8, device="cuda"), torch.empty((2, N), dtype=torch.int32, device="cuda"))
    assert ops.anchor_occupancy(bev, 5, 5, want_counts=True, out=good)[0] is good[0]
    bad = [(torch.empty((2, N - 1), dtype=torch.uint8, device="cuda"), None), (torch.empty((2, N), dtype=torch.int64, device="cuda"), None),
           (torch.empty((2, N), dtype=torch.uint8), None), (torch.empty((N, 2), dtype=torch.uint8, device="cuda").t(), None),
           (good[0], torch.empty((2, N), dtype=torch.int64, device="cuda")), (good[0], good[1][:1]), (None, good[1])]
    for out in bad:
        with pytest.raises(ValueError):
            ops.anchor_occupancy(bev, 5, 5, out=out)
    with pytest.raises(ValueError):
        ops.anchor_occupancy(bev, 5, 5, want_counts=True, out=(good[0], None))


# ------------------------------------------------------------------ 2. proposal layer
def proposal_masks(oracle, H):
    N = 4 * H * H
    return {"scan20000": scan_mask(oracle, 1, 20000, H), "scan2000": scan_mask(oracle, 2, 2000, H), "ones": np.ones(N, np.uint8),
            "zeros": np.zeros(N, np.uint8)}


def masked_proposal_case(ops, torch, oracle, name):
    """-> in how many of the fixture's SCAN-mask cases (2 cfg x 2 scans) the masked call returned fewer rows than the unmasked one"""
    g, (prob, pred, info, calib), _ = proposal_case(name)
    H = int(g["H"])
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()
    t_prob, t_pred, t_info, t_cal = dev(prob), dev(pred), dev(info), dev(calib[None])
    fewer = 0
    for key, sec in SECTIONS.items():
        params = ops.proposal_params(sec)
        plain = tuple(t.cpu().numpy() for t in ops.proposal_3d(t_prob, t_pred, t_info, t_cal, params))
        for mname, mask in proposal_masks(oracle, H).items():
            got = tuple(t.cpu().numpy() for t in ops.proposal_3d(t_prob, t_pred, t_info, t_cal, params, anchor_mask=torch.as_tensor(mask).cuda()))
            o_bv, o_img, o_3d = oracle.proposal_layer_3d(prob, R.masked_pred(pred, mask), info, calib, key, [8, ], cfg={key: sec})
            r = int(got[3][0])
            assert r == o_bv.shape[0] and int(got[4][0]) == 0, (key, mname)
            assert np.array_equal(got[0][0, :r], o_bv) and np.array_equal(got[1][0, :r], o_img)
            # (the masked anchors' sizes are the oracle's trick, not the layer's: their 3D boxes never reach the output)
            assert np.array_equal(got[2][0, :r], o_3d)
            assert not got[0][0, r:].any() and not got[2][0, r:].any()
            if mname == "ones":                                                 # bit for bit the unmasked call: blobs, num_out, status
                assert all(np.array_equal(a, b) for a, b in zip(got, plain))
            if mname == "zeros":
                assert r == 0
            if mname.startswith("scan"):
                fewer += r < int(plain[3][0])
    return fewer


@gpu
def test_masked_proposal_layer_vs_oracle(ops, torch_cuda, oracle):
    """the four fixtures x TRAIN / TEST cfg x {two scan masks, all ones, all zeros}.  At least one SCAN mask makes the layer return
    fewer rows than the unmasked call (the all-zeros mask does so trivially and is not counted): on the 20 x 20 fixture under the TRAIN
    cfg the 1600 anchors do not fill post_nms_topN = 2000, so masked anchors are missing rows (1448 -> 1216 and 477 by the oracle); on
    the 75 / 76 grids top-N caps both calls at the same count."""
    fewer = {name: masked_proposal_case(ops, torch_cuda, oracle, name) for name in PROPOSAL_FIXTURES}
    assert fewer["proposal3d_20_TRAIN_peaky"] == 2 and sum(fewer.values()) >= 2, fewer


@gpu
def test_masked_proposal_layer_batch_of_three_and_numpy_contract(ops, torch_cuda, oracle):
    torch = torch_cuda
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.rpn_msr.proposal_layer_tf import proposal_layer_3d
    frames = [synth.rpn_head(s, 76, 76, v) for s, v in ((11, "rand"), (12, "peaky"), (13, "peaky"))]
    masks = [scan_mask(oracle, 1, 20000, 76), scan_mask(oracle, 2, 2000, 76), scan_mask(oracle, 3, 2000, 76)]
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    sec = SECTIONS["TEST"]
    bv, img, b3, num, status = ops.proposal_3d(dev(np.concatenate([f[0] for f in frames])), dev(np.concatenate([f[1] for f in frames])),
                                               dev(np.concatenate([f[2] for f in frames])), dev(np.stack([f[3] for f in frames])),
                                               ops.proposal_params(sec), anchor_mask=dev(np.stack(masks)))
    num = num.cpu().numpy()
    assert int(status.max().item()) == 0
    for b, (f, m) in enumerate(zip(frames, masks)):
        o_bv, o_img, o_3d = oracle.proposal_layer_3d(f[0], R.masked_pred(f[1], m), f[2], f[3], "TEST", [8, ], cfg={"TEST": sec})
        r = int(num[b])
        assert r == o_bv.shape[0]
        o_bv[:, 0] = b; o_img[:, 0] = b; o_3d[:, 0] = b
        assert np.array_equal(bv[b, :r].cpu().numpy(), o_bv) and np.array_equal(img[b, :r].cpu().numpy(), o_img)
        assert np.array_equal(b3[b, :r].cpu().numpy(), o_3d)
    # the numpy contract: host arrays in, host arrays out, the mask as a bool or uint8 array
    saved = dict(cfg.TEST)
    cfg.TEST.update(sec)
    try:
        f, m = frames[1], masks[1]
        want = oracle.proposal_layer_3d(f[0], R.masked_pred(f[1], m), f[2], f[3], "TEST", [8, ], cfg={"TEST": sec})
        for mm in (m, m.astype(bool)):
            got = proposal_layer_3d(*f, "TEST", [8, ], [1.0, 1.0], anchor_mask=mm)
            assert all(isinstance(a, np.ndarray) and np.array_equal(a, w) for a, w in zip(got, want))
        with pytest.raises(ValueError):
            proposal_layer_3d(*f, "TEST", [8, ], anchor_mask=m[:-1])
    finally:
        cfg.TEST.update(saved)


# ------------------------------------------------------------------ 3. anchor target layer
def positives_mask(oracle, g, H):
    """the mask that removes exactly the unmasked positives"""
    inds, _, _, lab, _ = oracle.anchor_target_stage1(H, H, g["gt_bv"], g["gt_3d"], g["im_info"])
    m = np.ones(4 * H * H, np.uint8)
    m[inds[lab == 1]] = 0
    return m


@gpu
@pytest.mark.parametrize("name", AT_CASES)
def test_masked_anchor_target_layer_vs_restatement(ops, oracle, name):
    from mv3d_tf_amd.rpn_msr.anchor_target_layer_tf import anchor_target_layer
    g = golden(name)
    H, seed = int(g["H"]), int(g["np_seed"])
    score = np.zeros((1, H, H, 8), np.float32)
    masks = {"ones": np.ones(4 * H * H, np.uint8), "scan20000": scan_mask(oracle, 1, 20000, H), "scan2000": scan_mask(oracle, 2, 2000, H),
             "positives": positives_mask(oracle, g, H)}
    for mname, mask in masks.items():
        np.random.seed(seed)
        got = anchor_target_layer(score, g["gt_bv"], g["gt_3d"], g["im_info"], [8, ], [1.0, 1.0], anchor_mask=mask)
        state = np.random.get_state()[1].copy()
        np.random.seed(seed)
        want = R.masked_anchor_target_layer(oracle, H, H, g["gt_bv"], g["gt_3d"], g["im_info"], mask)
        for a, w in zip(got, want):
            assert np.array_equal(a, w), (name, mname)
        assert np.array_equal(np.random.get_state()[1], state), (name, mname)   # the generator ends where the restated draws leave it
        assert (got[0][mask == 0] == -1).all() and not got[1][mask == 0].any()
        if mname == "ones":
            np.random.seed(seed)
            plain = anchor_target_layer(score, g["gt_bv"], g["gt_3d"], g["im_info"], [8, ], [1.0, 1.0])
            assert all(np.array_equal(a, b) for a, b in zip(got, plain))
        if mname == "positives":
            inds, _, lab, _ = R.masked_stage1(oracle, H, H, g["gt_bv"], g["gt_3d"], g["im_info"], mask)
            n_pos = int((lab == 1).sum())
            if "gt_outside" in name:                                            # no inside anchor is left: nothing labelled, nothing drawn
                assert len(inds) == 0 and (got[0] == -1).all() and got[2].shape[0] == 0
                np.random.seed(seed)
                assert np.array_equal(np.random.get_state()[1], state)
            elif name == "anchor_target_76_normal":
                assert n_pos == 3
            elif name == "anchor_target_76_many_gt":
                assert n_pos == 24
            elif name == "anchor_target_76_tiny_gt":
                assert n_pos == 2


@gpu
@pytest.mark.parametrize("G", [1, 20])
def test_masked_stage1_batch_with_a_null_entry(ops, torch_cuda, oracle, G):
    torch = torch_cuda
    from mv3d_tf_amd._lib import lib
    H = 76
    N = 4 * H * H
    gts = [synth.gt_cars(np.random.RandomState(50 + 3 * G + b), G) for b in range(3)]
    info = np.array([[608, 608, 1]] * 3, np.float32)
    masks = [scan_mask(oracle, 1, 20000, H), None, scan_mask(oracle, 2, 2000, H)]
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    t_bv, t_3d = [dev(g[0]) for g in gts], [dev(g[1]) for g in gts]
    t_mask = [None if m is None else dev(m) for m in masks]
    t_info = dev(info)
    params = ops.anchor_target_params(oracle.TRAIN)
    labels = torch.empty((3, N), dtype=torch.float32, device="cuda")
    targets = torch.empty((3, N, 6), dtype=torch.float32, device="cuda")
    cf = torch.empty((3, 32 + N), dtype=torch.uint8, device="cuda")
    wsz = (lib().mv3d_anchor_target_workspace_bytes(H, H, G) + 255) // 256 * 256
    ws = torch.empty((3, wsz), dtype=torch.uint8, device="cuda")
    P3 = C.c_void_p * 3
    ptrs = lambda ts: P3(*[None if t is None else t.data_ptr() for t in ts])
    for mask_arg in (ptrs(t_mask), None):                                       # a NULL entry among masks; the array itself NULL
        rc = lib().mv3d_anchor_target_stage1_batch_masked(3, H, H, t_info.data_ptr(), ptrs(t_bv), ptrs(t_3d), (C.c_int * 3)(G, G, G), C.byref(params),
                                                          mask_arg, labels.data_ptr(), targets.data_ptr(), ptrs([cf[b, :32] for b in range(3)]),
                                                          ptrs([cf[b, 32:] for b in range(3)]), ptrs([ws[b] for b in range(3)]), wsz,
                                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        h_lab, h_tg, h_cf = labels.cpu().numpy(), targets.cpu().numpy(), cf.cpu().numpy()
        for b in range(3):
            m = np.ones(N, np.uint8) if (mask_arg is None or masks[b] is None) else masks[b]
            inds, max_ov, lab, tg = R.masked_stage1(oracle, H, H, gts[b][0], gts[b][1], info[b], m)
            w_lab = np.full(N, -1, np.float32); w_lab[inds] = lab
            w_tg = np.zeros((N, 6), np.float32); w_tg[inds] = tg
            assert np.array_equal(h_lab[b], w_lab) and np.array_equal(h_tg[b], w_tg)
            counts = h_cf[b, :32].copy().view(np.int32)
            neg = oracle.TRAIN["RPN_NEGATIVE_OVERLAP"]
            assert counts[:4].tolist() == [len(inds), int((lab == 1).sum()), int((lab == 0).sum()), int((max_ov < neg).sum())]
            assert np.array_equal(h_cf[b, 32:32 + counts[1]], (max_ov[lab == 1] >= neg).astype(np.uint8))


# ------------------------------------------------------------------ 4. train path
def numpy_contract_frame(frame, b, mask):
    from mv3d_tf_amd.rpn_msr.anchor_target_layer_tf import anchor_target_layer
    from mv3d_tf_amd.rpn_msr.proposal_layer_tf import proposal_layer_3d
    from mv3d_tf_amd.rpn_msr.proposal_target_layer_tf import proposal_target_layer_3d
    prob, pred, info, calib, (gt_bv, gt_3d, gt_cnr) = frame
    H, W = prob.shape[1:3]
    lab, tg, anc, anc3 = anchor_target_layer(np.zeros((1, H, W, 8), np.float32), gt_bv, gt_3d, info, [8, ], [1.0, 1.0], anchor_mask=mask)
    bv, img, b3 = proposal_layer_3d(prob, pred, info, calib, "TRAIN", [8, ], [1.0, 1.0], anchor_mask=mask)
    r_bv, r_img, r_lab, r_tg, r_3d = (np.array(a) for a in proposal_target_layer_3d(bv, b3, gt_bv, gt_3d, gt_cnr, calib, 2))
    for a in (r_bv, r_img, r_3d):
        a[:, 0] = b
    return dict(labels=lab, targets=tg, anchors=anc, anchors_3d=anc3, n_prop=bv.shape[0], rois_bv=r_bv, rois_img=r_img, rois_lab=r_lab,
                rois_tg=r_tg, rois_3d=r_3d)


@gpu
@pytest.mark.parametrize("helper,form", [(True, "uint8"), (False, "uint8"), (True, "numpy"), (True, "bool")])
def test_train_path_submit_with_anchor_mask(ops, torch_cuda, oracle, helper, form):
    """form: how the mask is handed over -- a ready uint8 device tensor on the default stream, or a numpy array / a bool device tensor
    with the path on streams of its own.  Those two are uploaded / converted by submit() on the CALLER's stream, which the slot's stream
    must be ordered behind: the caller's stream is kept busy (a few large matmuls) when submit() is called, and the block the converted
    mask is likely to be allocated in holds the INVERTED mask, so kernels that ran ahead of the conversion would not pass."""
    torch = torch_cuda
    from mv3d_tf_amd.train_path import TrainPathStream
    B, H = 2, 20
    dev = torch.device("cuda")
    frames = [synth.rpn_head(6100 + b, H, H, "peaky", return_gt=True) for b in range(B)]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev)
    args = (t(np.concatenate([f[0] for f in frames])), t(np.concatenate([f[1] for f in frames])), t(np.concatenate([f[2] for f in frames])),
            t(np.stack([f[3] for f in frames])), [tuple(t(a) for a in f[4]) for f in frames])
    masks = np.stack([scan_mask(oracle, 1, 20000, H), scan_mask(oracle, 2, 2000, H)])
    assert 0 < masks[0].sum() < masks[0].size and 0 < masks[1].sum() < masks[1].size
    own = form != "uint8"
    path = TrainPathStream(B, H, H, dev, depth=2, async_draws=helper, streams=[torch.cuda.Stream(), torch.cuda.Stream()] if own else None)
    busy = torch.randn(6144, 6144, device=dev) if own else None
    try:
        for use in (masks, None):
            np.random.seed(44)
            if use is None:
                given = None
            elif form == "uint8":
                given = torch.as_tensor(use).to(dev)
            else:
                given = use.copy() if form == "numpy" else torch.as_tensor(use.astype(bool)).to(dev)
                stale = torch.as_tensor(1 - use).to(dev)                        # the inverted mask, in a block the allocator hands out again
                torch.cuda.synchronize()
                del stale
                for _ in range(3):
                    busy = torch.tanh(busy @ busy)                              # the caller's stream has work queued in front of the conversion
            out = path.finish(path.submit(*args, anchor_mask=given))
            torch.cuda.synchronize()
            got = {k: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in out.items() if k not in ("rois", "proposals", "stream")}
            rois = {k: v.cpu().numpy().copy() for k, v in out["rois"].items()}
            state = np.random.get_state()[1].copy()
            np.random.seed(44)
            off = 0
            for b in range(B):
                w = numpy_contract_frame(frames[b], b, None if use is None else use[b])
                assert np.array_equal(got["rpn_labels"][b], w["labels"]) and np.array_equal(got["rpn_targets"][b], w["targets"])
                m = int(got["n_anchors"][b])
                assert m == w["anchors"].shape[0] and np.array_equal(got["anchors"][b, :m], w["anchors"])
                assert np.array_equal(got["anchors_3d"][b, :m], w["anchors_3d"])
                assert got["num_proposals"][b] == w["n_prop"]
                S = w["rois_bv"].shape[0]
                assert got["S"][b] == S
                sl = slice(off, off + S)
                assert np.array_equal(rois["bev"][sl], w["rois_bv"]) and np.array_equal(rois["rgb"][sl], w["rois_img"])
                assert np.array_equal(got["rois_3d"][sl], w["rois_3d"]) and np.array_equal(got["labels"][sl], w["rois_lab"])
                assert np.array_equal(got["bbox_targets"][sl], w["rois_tg"])
                if use is not None:
                    assert (got["rpn_labels"][b][use[b] == 0] == -1).all()
                off += S
            assert off == rois["bev"].shape[0]
            assert np.array_equal(np.random.get_state()[1], state)
    finally:
        path.close()


# ------------------------------------------------------------------ 5. the graphs
def sparse_feed(seed, B, torch, Hm=64, Wm=72, train=False):
    from mv3d_tf_amd.fast_rcnn.config import cfg
    r = np.random.RandomState(seed)
    bv = (r.random_sample((B, Hm, Wm, 9)) * (r.random_sample((B, Hm, Wm, 9)) < 0.0004)).astype(np.float32)
    im = (r.randint(0, 255, (B, 48, 160, 3)) - cfg.PIXEL_MEANS).astype(np.float32)
    feed = {"lidar_bv_data": torch.as_tensor(bv).cuda(), "image_data": torch.as_tensor(im).cuda(),
            "im_info": np.array([[Hm, Wm, 1]] * B, np.float32), "calib": np.stack([synth.KITTI_CALIB] * B), "keep_prob": 1.0}
    if train:
        gts = []
        for b in range(B):
            x1, y1 = r.randint(20, Wm - 60, 3), r.randint(20, Hm - 60, 3)
            gt_bv = np.stack([x1, y1, x1 + 17, y1 + 40, np.ones(3)], 1).astype(np.float32)
            g3, gc = synth.gt_cars(np.random.RandomState(seed + b), 3)[1:]
            gts.append((gt_bv, g3, gc))
        feed.update(gt_boxes_bv=[g[0] for g in gts], gt_boxes_3d=[g[1] for g in gts], gt_boxes_corners=[g[2] for g in gts])
    return feed, bv


@gpu
def test_train_graph_skips_empty_anchors(ops, torch_cuda, oracle):
    torch = torch_cuda
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.networks import get_network
    from mv3d_tf_amd.rpn_msr.proposal_layer_tf import proposal_layer_3d
    B, Hm = 2, 160
    saved = dict(cfg.TRAIN)
    try:
        net = get_network("MV3D_train")
        with torch.no_grad():
            net.params["rpn_cls_score"][0].mul_(40.0)
        feed, bv = sparse_feed(3, B, torch, Hm, Hm, train=True)
        np.random.seed(5)
        L = net.forward(feed)
        assert "rpn_anchor_mask" not in L                                       # off by default
        plain_labels = L["rpn_data"][0].cpu().numpy().copy()
        cfg.TRAIN.RPN_SKIP_EMPTY_ANCHORS = True
        for mc in (1, 2):
            cfg.TRAIN.RPN_EMPTY_ANCHOR_MIN_CELLS = mc
            np.random.seed(5)
            L = net.forward(feed)
            torch.cuda.synchronize()
            h, w = L["rpn_cls_score"].shape[1:3]
            want = np.stack([R.anchor_mask(oracle, bv[b], h, w, 8, mc) for b in range(B)])
            mask = L["rpn_anchor_mask"].cpu().numpy()
            assert mask.dtype == np.uint8 and np.array_equal(mask, want)
            assert 0.05 < 1.0 - want.mean() < 0.95
            labels = L["rpn_data"][0].cpu().numpy()
            assert (labels[mask == 0] == -1).all() and (labels != -1).any()
            assert not np.array_equal(labels, plain_labels)
            info = torch.as_tensor(feed["im_info"]).cuda()
            cal = torch.as_tensor(feed["calib"].astype(np.float32)).cuda()
            hand = proposal_layer_3d(L["rpn_cls_prob_reshape"].detach().contiguous(), L["rpn_bbox_pred"].detach().contiguous(), info, cal, "TRAIN",
                                     [8, ], [1.0, 1.0], anchor_mask=torch.as_tensor(want).cuda())
            for a, b_ in zip(L["rpn_rois"][:3], hand):
                assert torch.equal(a, b_)
    finally:
        cfg.TRAIN.update(saved)


@gpu
def test_serve_graph_skips_empty_anchors(ops, torch_cuda, oracle):
    """cfg.TEST.RPN_SKIP_EMPTY_ANCHORS in the captured serving step at batch 2, in the configuration whose replay the suite already pins
    against the eager step (tests/test_gpu_configs.py, configs[4]: MV3D_test_3view, f16 MFMA trunks, TEST cfg 6000 -> 300, 608 x 608 maps,
    here the two synthetic scans).  Every output of the replay equals the eager fixed-shape step bit for bit -- fusion head and box tail
    included -- also after new inputs were written into the graph's buffers; the occupancy launches are inside the graph (a replay on a
    new feed gives the new feed's mask); num_rois and the ROI rows equal proposal_layer_3d_fixed(..., anchor_mask=) called by hand."""
    torch = torch_cuda
    from mv3d_tf_amd.fast_rcnn import test_mv
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.networks import get_network
    from mv3d_tf_amd.rpn_msr.proposal_layer_tf import proposal_layer_3d_fixed
    B, cap = 2, 300
    saved = dict(cfg.TEST)
    cfg.TEST.update(RPN_PRE_NMS_TOP_N=6000, RPN_POST_NMS_TOP_N=cap, RPN_SKIP_EMPTY_ANCHORS=True)
    try:
        net = get_network("MV3D_test_3view")
        net.amp_dtype, net.mfma_trunk = torch.float16, True
        with torch.no_grad():
            net.params["rpn_cls_score"][0].mul_(30.0)

        def feed(seed):
            rng = np.random.RandomState(seed)
            bv = np.stack([np.pad(scan(oracle, seed + b, (20000, 2000)[b]), ((0, 7), (0, 7), (0, 0))) for b in range(B)])
            return {"lidar_bv_data": torch.as_tensor(bv).cuda(),
                    "image_data": torch.as_tensor((rng.randint(0, 255, (B, 375, 1242, 3)) - cfg.PIXEL_MEANS).astype(np.float32)).cuda(),
                    "lidar_fv_data": torch.as_tensor(rng.uniform(0, 1, (B, 64, 512, 3)).astype(np.float32)).cuda(),
                    "im_info": np.array([[608, 608, 1]] * B, np.float32), "calib": np.stack([synth.KITTI_CALIB] * B), "keep_prob": 1.0}, bv

        (f1, bv1), (f2, bv2) = feed(1), feed(2)
        wants = [np.stack([R.anchor_mask(oracle, bv[b], 76, 76) for b in range(B)]) for bv in (bv1, bv2)]
        assert not np.array_equal(wants[0], wants[1]) and all(0.05 < 1.0 - w[b].mean() < 0.95 for w in wants for b in range(B))
        sg = test_mv.ServeGraph(net, f1)
        captured = dict(net.layers)                                             # the graph's static tensors: every replay rewrites them
        keys = ("cls_prob", "bbox_pred", "rois_bv", "rois_img", "rois_3d", "corners", "pred_corners_r", "pred_bv", "num_rois", "status")
        info = torch.as_tensor(f1["im_info"]).cuda()
        cal = torch.as_tensor(f1["calib"].astype(np.float32)).cuda()
        for f, want in ((f1, wants[0]), (f2, wants[1]), (f1, wants[0])):
            got = sg.replay(f)
            sg.stream.synchronize()
            got = {k: got[k].clone() for k in keys}
            assert np.array_equal(captured["rpn_anchor_mask"].cpu().numpy(), want)
            args = (captured["rpn_cls_prob_reshape"].contiguous(), captured["rpn_bbox_pred"].contiguous(), info, cal, "TEST", 8)
            bvh, imgh, b3h, numh, sth, caph = proposal_layer_3d_fixed(*args, anchor_mask=torch.as_tensor(want).cuda())
            assert caph == cap and int(sth.max().item()) == 0 and int(got["status"].max().item()) == 0
            assert torch.equal(numh, got["num_rois"]) and torch.equal(bvh, got["rois_bv"])
            assert torch.equal(imgh, got["rois_img"]) and torch.equal(b3h, got["rois_3d"])
            assert int(numh.min().item()) > 0 and not torch.equal(proposal_layer_3d_fixed(*args)[0], bvh)    # the mask changes this step's proposals
            net.fixed_rois = True
            try:
                with torch.no_grad():
                    L = net.forward(f)
                    cnr, pr, pbv, _ = ops.box_detect_tail(L["rois"][2].contiguous(), L["bbox_pred"].contiguous(), 2)
            finally:
                net.fixed_rois = False
            torch.cuda.synchronize()
            assert np.array_equal(L["rpn_anchor_mask"].cpu().numpy(), want)
            eager = {"cls_prob": L["cls_prob"], "bbox_pred": L["bbox_pred"], "rois_bv": L["rois"][0], "rois_img": L["rois"][1], "rois_3d": L["rois"][2],
                     "corners": cnr, "pred_corners_r": pr, "pred_bv": pbv, "num_rois": L["num_rois"], "status": L["rois_status"]}
            for k in keys:
                assert torch.equal(got[k], eager[k]), k
    finally:
        cfg.TEST.update(saved)


# ------------------------------------------------------------------ 6. one pixel frame for the rasteriser and the anchors
@gpu
def test_best_anchor_of_every_labelled_car_is_not_empty(ops, torch_cuda, oracle):
    torch = torch_cuda
    z = golden("kitti_label")
    rng = np.random.RandomState(0)
    checked = 0
    for f in (0, 1):
        gt_bv, gt_3d = z["blob%d_gt_boxes_bv" % f], z["blob%d_gt_boxes_3d" % f]
        pts = []
        for x, y, zc, l, w, h, _ in gt_3d:                                       # points well inside each labelled box
            r = 0.25 * min(l, w)
            p = np.stack([x + rng.uniform(-r, r, 40), y + rng.uniform(-r, r, 40), np.full(40, min(zc, 0.3)), np.full(40, 0.5)], 1)
            pts.append(p)
        top = ops.point_cloud_2_top(torch.as_tensor(np.concatenate(pts).astype(np.float32)).cuda())
        for H in (75, 76):
            mask = ops.anchor_occupancy(top, H, H).cpu().numpy()[0]
            a = R.all_anchors(oracle, H, H)
            inside = np.where((a[:, 0] >= 0) & (a[:, 1] >= 0) & (a[:, 2] < 601) & (a[:, 3] < 601))[0]
            ov = oracle.bbox_overlaps(a[inside].astype(np.float64), gt_bv[:, :4].astype(np.float64))
            for g in range(gt_bv.shape[0]):
                if ov[:, g].max() > 0:
                    assert mask[inside[ov[:, g].argmax()]] == 1, (f, H, g)
                    checked += 1
    assert checked >= 20
