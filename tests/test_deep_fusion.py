"""The deep-fusion head (cfg.FUSION = 'deep'): the drop-path draw rule, configuration and parameter shapes,
fused_head.DeepFusedHead against the head written op by op, and the training / serving graphs under 'deep'."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fusion_join_restatement as fj
from conftest import ROOT

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- no GPU
def test_drop_path_draw_rule_over_4000_steps():
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.networks.mv3d import draw_drop_path
    V, N = 3, 4000
    a, b = np.random.RandomState(cfg.RNG_SEED), np.random.RandomState(cfg.RNG_SEED)
    before = np.random.get_state()
    n_global, chosen = 0, np.zeros(V)
    for _ in range(N):
        got = draw_drop_path(a, V)
        want, is_global = fj.draw_drop_path(b, V)
        assert got.dtype == np.uint8 and got.shape == (2, V) and np.array_equal(got, want)
        assert got.any(1).all()                                        # every join keeps at least one view
        if is_global:
            assert got.sum() == 2 and np.array_equal(got[0], got[1])   # the same single view at both joins
            n_global += 1
            chosen[int(got[0].argmax())] += 1
    assert abs(n_global / N - 0.5) <= 0.03                             # 3.8 binomial standard deviations at N = 4000
    assert (np.abs(chosen / n_global - 1.0 / 3) <= 0.04).all()
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2] == after[2]   # the global generator is not touched


def test_config_defaults():
    from mv3d_tf_amd.fast_rcnn import config
    c = config.cfg
    assert c.FUSION == 'early' and c.TRAIN.DROP_PATH is False and c.TRAIN.AUX_LOSSES is False
    config._merge({"FUSION": "deep", "TRAIN": {"DROP_PATH": True, "AUX_LOSSES": True}}, c)
    try:
        assert c.FUSION == 'deep' and c.TRAIN.DROP_PATH and c.TRAIN.AUX_LOSSES
    finally:
        config._merge({"FUSION": "early", "TRAIN": {"DROP_PATH": False, "AUX_LOSSES": False}}, c)


def test_parameter_shapes_under_both_settings():
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.networks import factory
    from mv3d_tf_amd.networks.mv3d import MV3D
    early, deep = MV3D(phase="TEST", device="cpu", views=2), MV3D(phase="TEST", device="cpu", views=2, fusion="deep")
    assert early.fusion == 'early' and early.params["cls_score"][0].shape == (2, 4096) and early.params["bbox_pred"][0].shape == (48, 4096)
    assert deep.fusion == 'deep' and deep.params["cls_score"][0].shape == (2, 2048) and deep.params["bbox_pred"][0].shape == (48, 2048)
    assert list(early.params) == list(deep.params)                    # layer names unchanged
    for k in early.params:
        if k not in ("cls_score", "bbox_pred"):
            assert early.params[k][0].shape == deep.params[k][0].shape, k
    assert isinstance(deep.drop_path_rng, np.random.RandomState)
    with pytest.raises(ValueError):
        MV3D(phase="TEST", device="cpu", fusion="late")
    # the factory passes the setting through, None = cfg.FUSION
    seen = []
    real = factory.MV3D
    factory.MV3D = lambda **kw: seen.append(kw) or kw
    try:
        factory.get_network("MV3D_train_3view", fusion="deep")
        factory.get_network("MV3D_test")
    finally:
        factory.MV3D = real
    assert seen == [dict(phase="TRAIN", views=3, fusion="deep"), dict(phase="TEST", views=2, fusion=None)]
    # the 16-bit head buffer the optimizer writes
    import torch
    from mv3d_tf_amd.fused_head import head_buffers
    small = {"fc6_1": [torch.zeros(8, 12), torch.zeros(8)], "fc7_1": [torch.zeros(8, 8), torch.zeros(8)],
             "fc6_2": [torch.zeros(8, 12), torch.zeros(8)], "fc7_2": [torch.zeros(8, 8), torch.zeros(8)]}
    for fusion, width in (("early", 16), ("deep", 8)):
        small["cls_score"], small["bbox_pred"] = [torch.zeros(2, width), torch.zeros(2)], [torch.zeros(48, width), torch.zeros(48)]
        bufs, pieces = head_buffers(small, ["fc6_1", "fc6_2"], ["fc7_1", "fc7_2"], torch.bfloat16, "cpu", fusion=fusion)
        assert bufs[4].shape == (50, width) and len(pieces) == 12
        assert all(p.shape == d.shape for p, d in pieces)
    assert cfg.FUSION == 'early'


def test_load_of_an_early_checkpoint_under_deep(tmp_path, capsys):
    """an early-fusion `.npy` into MV3D(fusion='deep'): towers load, the cls_score / bbox_pred weights (4096 wide for two views) do
    not fit the 2048-wide variables: skipped with the reference's "ignore <layer>" under ignore_missing (their biases still load), an
    error otherwise"""
    import torch
    from mv3d_tf_amd.networks.mv3d import MV3D
    net = MV3D(phase="TEST", device="cpu", views=2, fusion="deep")
    assert net.params["cls_score"][0].shape == (2, 2048)
    rng = np.random.RandomState(0)
    ckpt = {"fc7_2": {"weights": rng.randn(2048, 2048).astype(np.float32), "biases": rng.randn(2048).astype(np.float32)},
            "cls_score": {"weights": rng.randn(4096, 2).astype(np.float32), "biases": rng.randn(2).astype(np.float32)},
            "bbox_pred": {"weights": rng.randn(4096, 48).astype(np.float32), "biases": rng.randn(48).astype(np.float32)}}
    path = str(tmp_path / "early.npy")
    np.save(path, ckpt, allow_pickle=True)
    before = [net.params[k][0].detach().clone() for k in ("cls_score", "bbox_pred")]
    net.load(path, ignore_missing=True)
    out = capsys.readouterr().out
    assert "ignore cls_score" in out and "ignore bbox_pred" in out and "ignore fc7_2" not in out
    assert torch.equal(net.params["fc7_2"][0].detach(), torch.as_tensor(ckpt["fc7_2"]["weights"]).t())
    assert torch.equal(net.params["cls_score"][0].detach(), before[0]) and torch.equal(net.params["bbox_pred"][0].detach(), before[1])
    assert torch.equal(net.params["cls_score"][1].detach(), torch.as_tensor(ckpt["cls_score"]["biases"]))
    assert torch.equal(net.params["bbox_pred"][1].detach(), torch.as_tensor(ckpt["bbox_pred"]["biases"]))
    with pytest.raises(ValueError):
        net.load(path, ignore_missing=False)
    # the same file fits the early network whole
    early = MV3D(phase="TEST", device="cpu", views=2)
    early.load(path, ignore_missing=False)
    assert torch.equal(early.params["cls_score"][0].detach(), torch.as_tensor(ckpt["cls_score"]["weights"]).t())


def test_snapshot_carries_the_drop_path_generator(tmp_path):
    """SolverWrapper.snapshot writes net.drop_path_rng's state next to the optimizer's, as plain values torch.load accepts; set back,
    the draw stream continues where it was"""
    import torch
    from mv3d_tf_amd.fast_rcnn import train_mv
    from mv3d_tf_amd.networks.mv3d import draw_drop_path
    w = torch.zeros(3, requires_grad=True)
    net = types.SimpleNamespace(params={"fc": [w, torch.zeros(1)]}, drop_path_rng=np.random.RandomState(3))
    for _ in range(5):
        draw_drop_path(net.drop_path_rng, 3)
    sw = train_mv.SolverWrapper(None, None, net, None, [], str(tmp_path))
    sw.log = lambda *_: None
    sw.optimizer = torch.optim.Adam([w], lr=1e-3)
    name = sw.snapshot(None, 6)
    want = [draw_drop_path(net.drop_path_rng, 3) for _ in range(20)]
    state = torch.load(name + ".optim.pt")
    fresh = np.random.RandomState(0)
    train_mv.rng_set_state_plain(fresh, state["drop_path_rng"])
    assert all(np.array_equal(draw_drop_path(fresh, 3), k) for k in want)


def test_build_module_cross_compiles_the_join():
    out = subprocess.run([sys.executable, "-m", "mv3d_tf_amd.build"], cwd=ROOT, capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().endswith("libmv3d_hip.so")
    assert os.path.isfile(os.path.join(ROOT, "mv3d_tf_amd", "csrc", "fusion_join.hip"))
    from mv3d_tf_amd import _lib
    assert hasattr(_lib.lib(), "mv3d_fusion_join_forward") and hasattr(_lib.lib(), "mv3d_fusion_join_backward")


# ---------------------------------------------------------------------------------------------------- the head
@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops
    return torch, ops


SFX = ("_1", "_2", "_3")


def head_inputs(torch, V, R, C, N):
    """the pooled maps and parameters of test_train_entry.py::test_fused_head_equals_the_op_by_op_head, drawn the same way from the same
    seed (cls_score / bbox_pred N wide: the deep head), as float64 masters whose values are f32 values"""
    torch.manual_seed(0)
    pools = [torch.randn(R, 7, 7, C).double() for _ in range(V)]
    params = {}
    for t in SFX[:V]:
        params["fc6" + t] = [(torch.randn(N, C * 49) * 0.1).double(), torch.randn(N).double()]
        params["fc7" + t] = [(torch.randn(N, N) * 0.1).double(), torch.randn(N).double()]
    params["cls_score"] = [torch.randn(2, N).double(), torch.randn(2).double()]
    params["bbox_pred"] = [torch.randn(48, N).double(), torch.randn(48).double()]
    return pools, params


def leaves_of(torch, pools, params, dtype, device):
    """fresh leaf copies of the float64 masters in dtype on device"""
    mk = lambda t: t.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
    return [mk(p) for p in pools], {k: [mk(w), mk(b)] for k, (w, b) in params.items()}


def deep_head_op_by_op(torch, pools, params, keep1, keep2, masks, scale):
    """the deep head in torch ops, in the dtype and on the device of its inputs: (cls (P, R, 2), box (P, R, 48), join 1, join 2)"""
    import torch.nn.functional as F
    V, P, R = len(pools), len(keep1), pools[0].shape[0]

    def join(hs, keep_row, mask):
        kept = [F.relu(h) for h, k in zip(hs, keep_row) if k]
        m = sum(kept[1:], kept[0]) / float(len(kept))
        return m if mask is None else m * mask.to(m.dtype) * scale

    h6 = [F.linear(pools[v].permute(0, 3, 1, 2).reshape(R, -1), *params["fc6" + SFX[v]]) for v in range(V)]
    j1 = [join(h6, keep1[p], None if masks is None else masks[0][p]) for p in range(P)]
    j2 = [join([F.linear(j1[p], *params["fc7" + SFX[v]]) for v in range(V)], keep2[p], None if masks is None else masks[1][p]) for p in range(P)]
    cls = torch.stack([F.linear(j, *params["cls_score"]) for j in j2])
    box = torch.stack([F.linear(j, *params["bbox_pred"]) for j in j2])
    return cls, box, torch.stack(j1), torch.stack(j2)


def run_and_grads(torch, fn, pools, params):
    cls, box = fn(pools, params)[:2]
    ((cls.double() ** 2).sum() + box.double().sum() * 0.3).backward()
    leaves = list(pools) + [q for k in params for q in params[k]]
    assert all(p.is_leaf and p.requires_grad for p in leaves)
    # (a view that every path drops at join 1 is not in the op-by-op graph at all: no gradient there is a zero gradient)
    return [cls.detach().double().cpu(), box.detach().double().cpu()] + \
        [(torch.zeros_like(p) if p.grad is None else p.grad).detach().double().cpu() for p in leaves]


def max_error(got, want):
    """the maximum error: the largest |got - want| over the outputs and every gradient; and tensor by tensor, for the printout"""
    errs = [float((g - w).abs().max()) if w.numel() else 0.0 for g, w in zip(got, want)]
    return max(errs), errs


@gpu
@pytest.mark.parametrize("P", [1, 4])
def test_deep_fused_head_equals_the_op_by_op_head(dev, P):
    """DeepFusedHead (V = 3, R = 6, 4 channels, N = 8) in f32 on the device against the head op by op in float64 on the CPU: the
    two outputs and every gradient (pooled maps, fc6 / fc7 of every view, cls_score, bbox_pred), with dropout masks and keep tables
    that drop views.  Yardstick: the same op-by-op head in f32 on the device against the same float64 values; the fused head's
    maximum error (the largest absolute difference over the outputs and all gradients) may be at most twice the op-by-op head's --
    batching changes the GEMMs' summation order, nothing else.  Both errors are printed, and the per-tensor ones beside them."""
    torch, ops = dev
    from mv3d_tf_amd.fused_head import deep_fused_head
    V, R, C, N = 3, 6, 4, 8
    pools64, params64 = head_inputs(torch, V, R, C, N)
    g = torch.Generator().manual_seed(0)                               # (the dropout masks)
    n6, n7 = ["fc6" + t for t in SFX], ["fc7" + t for t in SFX]
    tables = {1: [([[1, 1, 1]], [[1, 1, 1]]), ([[1, 0, 1]], [[0, 1, 1]])],
              4: [([[1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1]],) * 2, ([[0, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 1, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])]}[P]
    for (keep1, keep2), keep_prob in zip(tables, (1.0, 0.5)):
        keep1, keep2 = np.array(keep1, np.uint8), np.array(keep2, np.uint8)
        masks = None if keep_prob == 1.0 else tuple((torch.rand(P, R, N, generator=g) < keep_prob).to(torch.uint8) for _ in range(2))
        scale = 1.0 / keep_prob
        want = run_and_grads(torch, lambda po, pa: deep_head_op_by_op(torch, po, pa, keep1, keep2, masks, scale),
                             *leaves_of(torch, pools64, params64, torch.float64, "cpu"))
        dmasks = None if masks is None else tuple(m.cuda() for m in masks)
        ref = run_and_grads(torch, lambda po, pa: deep_head_op_by_op(torch, po, pa, keep1, keep2, dmasks, scale),
                            *leaves_of(torch, pools64, params64, torch.float32, "cuda"))
        got = run_and_grads(torch, lambda po, pa: deep_fused_head(po, pa, n6, n7, keep_prob, torch.float32, keep1, keep2, masks=dmasks),
                            *leaves_of(torch, pools64, params64, torch.float32, "cuda"))
        e_got, per_got = max_error(got, want)
        e_ref, per_ref = max_error(ref, want)
        print("P = %d keep_prob = %.1f: fused head max error %.3e, op-by-op f32 head %.3e" % (P, keep_prob, e_got, e_ref))
        print("  per tensor, fused:    " + " ".join("%.1e" % e for e in per_got))
        print("  per tensor, op by op: " + " ".join("%.1e" % e for e in per_ref))
        assert all(a.shape == b.shape for a, b in zip(got, want))
        assert e_got <= 2.0 * e_ref, (P, keep_prob, e_got, e_ref)


@gpu
def test_deep_fused_head_with_one_view_matches_the_early_fused_head(dev):
    """V = 1: a join of one view is the ReLU, so deep and early fusion are the same network.  Both fused heads and the op-by-op head in
    f32 on the device against float64 on the CPU, the same yardstick: at most twice the op-by-op head's largest error."""
    torch, ops = dev
    import torch.nn.functional as F
    from mv3d_tf_amd.fused_head import deep_fused_head, fused_head
    V, R, C, N = 1, 6, 4, 8
    pools64, params64 = head_inputs(torch, V, R, C, N)
    one = np.ones((1, 1), np.uint8)

    def early(po, pa):
        x = F.relu(F.linear(po[0].permute(0, 3, 1, 2).reshape(R, -1), *pa["fc6_1"]))
        x = F.relu(F.linear(x, *pa["fc7_1"]))
        return F.linear(x, *pa["cls_score"]), F.linear(x, *pa["bbox_pred"])

    want = run_and_grads(torch, early, *leaves_of(torch, pools64, params64, torch.float64, "cpu"))
    ref = run_and_grads(torch, early, *leaves_of(torch, pools64, params64, torch.float32, "cuda"))
    deep = run_and_grads(torch, lambda po, pa: tuple(t[0] for t in deep_fused_head(po, pa, ["fc6_1"], ["fc7_1"], 1.0, torch.float32, one, one)[:2]),
                         *leaves_of(torch, pools64, params64, torch.float32, "cuda"))
    fused = run_and_grads(torch, lambda po, pa: fused_head(po, pa, ["fc6_1"], ["fc7_1"], 1.0, torch.float32)[:2],
                          *leaves_of(torch, pools64, params64, torch.float32, "cuda"))
    e_ref, e_deep, e_fused = max_error(ref, want)[0], max_error(deep, want)[0], max_error(fused, want)[0]
    print("V = 1: deep fused head %.3e, early fused head %.3e, op-by-op f32 head %.3e" % (e_deep, e_fused, e_ref))
    assert e_deep <= 2.0 * e_ref and max_error(deep, fused)[0] <= 2.0 * e_ref + e_fused


@gpu
def test_main_row_forced_to_one_view_equals_that_auxiliary_path(dev):
    """keep_prob = 1, main row = e_v: the main outputs are auxiliary path v's, bit for bit"""
    torch, ops = dev
    from mv3d_tf_amd.fused_head import deep_fused_head
    V, R, C, N = 3, 6, 4, 8
    pools, params = head_inputs(torch, V, R, C, N)
    pools, params = [p.float().cuda() for p in pools], {k: [w.float().cuda(), b.float().cuda()] for k, (w, b) in params.items()}
    n6, n7 = ["fc6" + t for t in SFX], ["fc7" + t for t in SFX]
    for v in range(V):
        keep = np.concatenate([np.eye(V, dtype=np.uint8)[v:v + 1], np.eye(V, dtype=np.uint8)])
        cls, box, j1, j2, masks = deep_fused_head(pools, params, n6, n7, 1.0, torch.float32, keep, keep)
        assert masks is None and cls.shape == (4, R, 2) and box.shape == (4, R, 48)
        assert torch.equal(cls[0], cls[1 + v]) and torch.equal(box[0], box[1 + v]) and torch.equal(j2[0], j2[1 + v])
        assert not torch.equal(cls[0], cls[1 + (v + 1) % V])


@gpu
def test_dropout_acts_once_on_the_joined_vector(dev):
    """keep_prob = 0.5: the zero pattern of join 1 is the mask's (on top of the mean's own zeros), the survivors are the undropped
    join times 1 / keep_prob; a mask drawn inside has the right shape, type and density"""
    torch, ops = dev
    from mv3d_tf_amd.fused_head import deep_fused_head
    V, R, C, N = 3, 64, 4, 8
    pools, params = head_inputs(torch, V, R, C, N)
    pools, params = [p.float().cuda() for p in pools], {k: [w.float().cuda(), b.float().cuda()] for k, (w, b) in params.items()}
    n6, n7 = ["fc6" + t for t in SFX], ["fc7" + t for t in SFX]
    keep = np.array([[1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.uint8)
    plain = deep_fused_head(pools, params, n6, n7, 1.0, torch.float32, keep, keep)[2]
    j1, (M1, M2) = deep_fused_head(pools, params, n6, n7, 0.5, torch.float32, keep, keep)[2:5:2]
    assert M1.shape == (4, R, N) and M2.shape == (4, R, N) and M1.dtype == torch.uint8 and M1.is_cuda
    assert 0.4 < float(M1.float().mean()) < 0.6 and 0.4 < float(M2.float().mean()) < 0.6 and not torch.equal(M1, M2)
    assert torch.equal(j1 != 0, (M1 != 0) & (plain != 0))
    assert torch.equal(j1, torch.where(M1 != 0, plain * 2.0, torch.zeros_like(plain)))


# ---------------------------------------------------------------------------------------------------- the graphs
def _train_frames():
    from mv3d_tf_amd import synth
    rng = np.random.RandomState(1)
    frames = []
    for k in range(2):
        _, _, info, calib, (gt_bv, gt_3d, gt_cnr) = synth.rpn_head(55 + k, 76, 76, "peaky", return_gt=True)
        frames.append({"lidar_bv_data": (rng.random_sample((1, 608, 608, 9)) < 0.02).astype(np.float32),
                       "image_data": rng.randint(0, 255, (1, 96, 320, 3)).astype(np.float32),
                       "lidar_fv_data": rng.random_sample((1, 64, 512, 3)).astype(np.float32),
                       "im_info": info, "calib": calib, "gt_boxes_bv": gt_bv, "gt_boxes_3d": gt_3d, "gt_boxes_corners": gt_cnr})
    return frames


@gpu
def test_three_view_training_graph_under_deep_fusion(dev):
    torch, ops = dev
    from mv3d_tf_amd import optim
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.fast_rcnn.train_mv import stack_blobs, total_loss
    from mv3d_tf_amd.networks import get_network
    cfg.FUSION = 'deep'
    try:
        net = get_network("MV3D_train_3view")
        assert net.fusion == 'deep' and net.params["cls_score"][0].shape == (2, 2048) and net.params["bbox_pred"][0].shape == (48, 2048)
        with torch.no_grad():
            net.params["rpn_cls_score"][0].mul_(40.0)
        feed = stack_blobs(_train_frames())
        feed["keep_prob"] = 0.5
        # the same step with the switches off: what the global generator looks like afterwards
        np.random.seed(3)
        L = net.forward(feed)
        assert "cls_score_aux" not in L and L["fusion_keep"].shape == (2, 1, 3) and L["fusion_keep"].all()
        loss0, _ = total_loss(L)
        assert "loss_aux" not in L and torch.isfinite(loss0)
        state_off = np.random.get_state()
        cfg.TRAIN.DROP_PATH = cfg.TRAIN.AUX_LOSSES = True
        np.random.seed(3)
        L = net.forward(feed)
        state_on = np.random.get_state()
        assert np.array_equal(state_off[1], state_on[1]) and state_off[2] == state_on[2]
        R = L["cls_score"].shape[0]
        assert L["cls_score_aux"].shape == (3, R, 2) and L["bbox_pred_aux"].shape == (3, R, 48) and L["bbox_pred"].shape == (R, 48)
        want_keep, _ = fj.draw_drop_path(np.random.RandomState(cfg.RNG_SEED), 3)     # the network's first draw
        keep = L["fusion_keep"]
        assert keep.shape == (2, 4, 3) and np.array_equal(keep[:, 0], want_keep)
        assert np.array_equal(keep[0, 1:], np.eye(3, dtype=np.uint8)) and np.array_equal(keep[1, 1:], np.eye(3, dtype=np.uint8))
        loss, parts = total_loss(L)
        assert len(parts) == 4 and L["loss_aux"].shape == (3, 2)
        assert torch.isfinite(loss) and torch.isfinite(L["loss_aux"]).all()
        want = torch.stack(parts).sum() + L["loss_aux"].sum()
        assert abs(float(loss) - float(want)) <= 1e-6 * abs(float(want))
        loss.backward()
        for name, wb in net.params.items():
            for p in wb:
                assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert float(net.params["fc6_3"][0].grad.abs().sum()) > 0 and float(net.params["cls_score"][0].grad.abs().sum()) > 0
        # a second step in mixed precision with the kernel Adam attached: its launch writes the head's 16-bit copies, (50, 2048) included
        net.amp_dtype, net.mfma_trunk = torch.bfloat16, True
        opt = optim.Adam(net.parameters(), lr=1e-5)
        net.attach_optimizer(opt)
        for p in net.parameters():
            p.grad = None
        L = net.forward(feed)
        loss, _ = total_loss(L)
        assert torch.isfinite(loss)
        loss.backward()
        opt.step()
        bufs, current = net._held_head(SFX)
        assert current is True and bufs[4].shape == (50, 2048)
        assert torch.equal(bufs[4][:2], net.params["cls_score"][0].detach().to(torch.bfloat16))
        assert torch.equal(bufs[4][2:], net.params["bbox_pred"][0].detach().to(torch.bfloat16))
        assert torch.equal(bufs[2][2], net.params["fc7_3"][0].detach().to(torch.bfloat16))
        L = net.forward(feed)                                          # ... and the next forward reads them
        assert torch.isfinite(total_loss(L)[0]) and net._held_head(SFX)[1] is True
    finally:
        cfg.FUSION = 'early'
        cfg.TRAIN.DROP_PATH = cfg.TRAIN.AUX_LOSSES = False


def _small_net(torch, name="MV3D_test"):
    from mv3d_tf_amd.networks import get_network
    net = get_network(name, fusion="deep")
    with torch.no_grad():                                    # spread the RPN scores a little (random init is flat)
        net.params["rpn_cls_score"][0].mul_(40.0)
        net.params["rpn_bbox_pred"][0].mul_(5.0)
    return net


@gpu
def test_serving_under_deep_fusion(dev, tmp_path):
    """the fixed-ROI serving step under 'deep' (P = 1, every view kept, no mask): both ServeGraph classes replay it bit for bit (3-view
    model, f16 MFMA trunks as in BASELINE configs[4]: torch's f32 convolutions are not bit-reproducible from run to run), and
    detect_batch.test_net runs a synthetic split end to end"""
    torch, ops = dev
    from mv3d_tf_amd import synth
    from mv3d_tf_amd.fast_rcnn import detect_batch, test_mv
    from mv3d_tf_amd.fast_rcnn.config import cfg
    B, cap = 2, 300
    saved, root = dict(cfg.TEST), cfg.ROOT_DIR
    cfg.TEST.update(RPN_PRE_NMS_TOP_N=6000, RPN_POST_NMS_TOP_N=cap)
    try:
        net = _small_net(torch, "MV3D_test_3view")
        net.amp_dtype, net.mfma_trunk = torch.float16, True
        assert net.params["cls_score"][0].shape == (2, 2048)

        def feed(seed):
            rng = np.random.RandomState(seed)
            return {"lidar_bv_data": torch.as_tensor(((rng.random_sample((B, 608, 608, 9)) < 0.03) * rng.uniform(0, 2.4, (B, 608, 608, 9))).astype(np.float32)).cuda(),
                    "image_data": torch.as_tensor((rng.randint(0, 255, (B, 375, 1242, 3)) - cfg.PIXEL_MEANS).astype(np.float32)).cuda(),
                    "lidar_fv_data": torch.as_tensor(rng.uniform(0, 1, (B, 64, 512, 3)).astype(np.float32)).cuda(),
                    "im_info": np.array([[608, 608, 1]] * B, np.float32), "calib": np.stack([synth.KITTI_CALIB] * B), "keep_prob": 1.0}

        feeds = {1: feed(1), 2: feed(2)}
        for cls, kw in ((test_mv.ServeGraph, {}), (detect_batch.ServeGraph, dict(post=dict(max_per_image=10)))):
            sg = cls(net, feeds[1], **kw)
            for seed in (2, 1):
                f = feeds[seed]
                got = sg.replay(f)
                sg.stream.synchronize()
                got = {k: got[k].clone() for k in ("cls_prob", "bbox_pred", "rois_3d", "pred_bv", "num_rois")}
                net.fixed_rois = True
                try:
                    with torch.no_grad():
                        L = net.forward(f)
                        pbv = ops.box_detect_tail(L["rois"][2].contiguous(), L["bbox_pred"].contiguous(), 2)[2]
                finally:
                    net.fixed_rois = False
                want = {"cls_prob": L["cls_prob"], "bbox_pred": L["bbox_pred"], "rois_3d": L["rois"][2], "pred_bv": pbv, "num_rois": L["num_rois"]}
                for k in got:
                    assert torch.equal(got[k], want[k]), (cls.__module__, k)
                assert got["cls_prob"].shape == (B * cap, 2) and torch.isfinite(got["bbox_pred"]).all()
                assert int(got["num_rois"].min()) > 0
            if kw:
                assert len(sg.final_detections()) == B
            del sg
        del net, feeds
        cfg.TEST.update(RPN_PRE_NMS_TOP_N=600, RPN_POST_NMS_TOP_N=50)
        net = _small_net(torch)

        class Imdb:
            name = "synthetic_deep"
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

        imdb = Imdb()
        cfg.TEST.BATCH_SIZE = 2
        cfg.ROOT_DIR = str(tmp_path)
        all_boxes, all_cnr = detect_batch.test_net(None, net, imdb, "w", max_per_image=10)
        assert len(imdb.evaluated) == 1 and len(all_boxes[1]) == 3 and len(all_cnr[1]) == 3
        assert all(np.asarray(all_boxes[1][i]).shape[1:] == (5,) and np.isfinite(np.asarray(all_boxes[1][i])).all() for i in range(3))
        assert os.path.isfile(os.path.join(imdb.evaluated[0][2], "detections.pkl"))
    finally:
        cfg.TEST.clear()
        cfg.TEST.update(saved)
        cfg.ROOT_DIR = root
