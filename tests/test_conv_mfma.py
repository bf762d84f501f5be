"""-m gpu numerics of the serving trunk's contraction (mv3d_conv3x3_f16 / mv3d_maxpool2x2_f16, csrc/conv3x3_mfma.hip) against
a plain PyTorch fp32 convolution of the SAME f16-rounded operands.

Tolerance: the kernel multiplies f16 operands exactly and accumulates in f32 (MFMA), so against the fp32 reference it differs by
the f32 accumulation order (~1e-6 relative) plus, for f16 outputs, one rounding to f16 (2^-11 relative): |got - want| <=
2e-3 * max|want| for f16 maps, 2e-5 * max|want| for f32 maps.  Operands are asymmetric random values, so a transposed
fragment / tap / channel mapping cannot pass.

These small maps reach the "few tiles" 64 x 128, the 256 x 64 and the input-layer tiles; the paths that larger launches select
(conv3x3_pp_kernel, 128 x 128, f32 output, gated, f32 128 x 128) are pinned exactly in tests/test_conv_paths.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    return torch


def _reference(torch, x, w, b, relu):
    """fp32 conv of f16-rounded operands; x (B,H,W,Cin), w (O,I,3,3) -> (B,H,W,O)"""
    y = torch.nn.functional.conv2d(x.half().float().permute(0, 3, 1, 2), w.half().float(), b, padding=1)
    if relu:
        y = torch.relu(y)
    return y.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("B,H,W,cin,cout,out_f32,relu,framed", [
    (2, 76, 76, 512, 512, False, True, True),        # conv4_2 / conv5_x of the BEV trunk
    (1, 46, 155, 512, 512, True, True, False),       # conv5_3_2 (RGB), the f32 map RoiPool reads; M % 128 != 0
    (1, 20, 36, 64, 64, False, True, True),          # conv1_2 shape class (64-cout tile)
    (1, 33, 17, 64, 128, False, False, True),        # conv2_1 class, odd sizes, no ReLU
    (1, 19, 23, 128, 256, True, False, False),
    (1, 8, 64, 256, 512, False, True, False),        # FV trunk conv4_1
])
def test_conv3x3_matches_fp32_reference(gpu, B, H, W, cin, cout, out_f32, relu, framed):
    torch = gpu
    from mv3d_tf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + H * 7 + cin)
    x = torch.randn((B, H, W, cin), device="cuda", generator=g)
    w = torch.randn((cout, cin, 3, 3), device="cuda", generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn((cout,), device="cuda", generator=g)
    want = _reference(torch, x, w, b, relu)
    xf = ops.frame_nhwc_f16(x, ops.framed_buffer(B, H, W, cin, x.device))
    assert float(xf[:, 0].abs().max()) == 0 and float(xf[:, :, -1].abs().max()) == 0
    got = ops.conv3x3_f16(xf, ops.pack_conv3x3_weights(w), b, out_framed=framed, out_f32=out_f32, relu=relu)
    torch.cuda.synchronize()
    if framed:
        assert got.shape == (B, H + 2, W + 2, cout)
        assert float(got[:, 0].abs().max()) == 0 and float(got[:, -1].abs().max()) == 0            # the frame is never written
        assert float(got[:, :, 0].abs().max()) == 0 and float(got[:, :, -1].abs().max()) == 0
        got = got[:, 1:-1, 1:-1]
    assert got.dtype == (torch.float32 if out_f32 else torch.float16)
    scale = float(want.abs().max())
    err = float((got.float() - want).abs().max())
    assert err <= (2e-5 if out_f32 else 2e-3) * scale, (err, scale)


@pytest.mark.parametrize("B,H,W,cin,cout", [(2, 40, 52, 9, 64), (1, 31, 45, 3, 64), (1, 16, 16, 9, 128)])
def test_input_layer_variant(gpu, B, H, W, cin, cout):
    """conv1_1: 9 / 3 input channels zero-padded to 16, K steps of 4 taps x 16 channels"""
    torch = gpu
    from mv3d_tf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(H + cin)
    x = torch.randn((B, H, W, cin), device="cuda", generator=g)
    w = torch.randn((cout, cin, 3, 3), device="cuda", generator=g) * 0.3
    b = torch.randn((cout,), device="cuda", generator=g)
    want = _reference(torch, x, w, b, True)
    xf = ops.frame_nhwc_f16(x, ops.framed_buffer(B, H, W, 16, x.device))
    got = ops.conv3x3_f16(xf, ops.pack_conv3x3_weights_input_layer(w), b)[:, 1:-1, 1:-1]
    torch.cuda.synchronize()
    assert float((got.float() - want).abs().max()) <= 2e-3 * float(want.abs().max())


@pytest.mark.parametrize("B,H,W,cin,framed,relu", [(3, 33, 71, 9, False, True), (1, 17, 31, 3, False, False), (2, 50, 97, 3, True, False),
                                                  (5, 1, 1, 9, True, True), (1, 3, 200, 9, False, True)])
def test_input_layer_kernel_odd_shapes_and_bare_output(gpu, B, H, W, cin, framed, relu):
    """csrc/conv_input.hip: widths that are no multiple of its 32-pixel blocks, heights that are no multiple of its 16-row strips (rows past
    the map are computed from clamped rows and dropped by the store's range check), a 1 x 1 map, bare (unframed) outputs, no ReLU -- every
    pixel against torch's f32 convolution of the rounded operands, and a framed output's frame left untouched"""
    torch = gpu
    import torch.nn.functional as F
    from mv3d_tf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + H * 10 + W)
    x = torch.randn((B, H, W, cin), device="cuda", generator=g)
    w = torch.randn((64, cin, 3, 3), device="cuda", generator=g) * 0.25
    b = torch.randn((64,), device="cuda", generator=g)
    T = torch.float16
    want = F.conv2d(x.to(T).float().permute(0, 3, 1, 2), w.to(T).float(), b, padding=1).permute(0, 2, 3, 1)
    if relu:
        want = F.relu(want)
    xf = ops.frame_nhwc_f16(x, ops.framed_buffer(B, H, W, 16, x.device))
    out = ops.framed_buffer(B, H, W, 64, x.device) if framed else torch.full((B, H, W, 64), 7.0, dtype=T, device="cuda")
    got = ops.conv3x3_f16(xf, ops.pack_conv3x3_weights_input_layer(w), b, out=out, out_framed=framed, relu=relu)
    torch.cuda.synchronize()
    inner = got[:, 1:-1, 1:-1] if framed else got
    assert not bool(torch.isnan(inner.float()).any())
    assert float((inner.float() - want).abs().max()) <= 4e-3 * max(1.0, float(want.abs().max()))
    if framed:
        fr = got.clone()
        fr[:, 1:-1, 1:-1] = 0
        assert float(fr.abs().max()) == 0.0


@pytest.mark.parametrize("half", ["float16", "bfloat16"])
def test_input_layer_kernel_at_full_occupancy(gpu, half):
    """csrc/conv_input.hip on maps large enough that every CU holds a full workgroup (two waves per SIMD: 1444 + 120 + 64 column strips),
    three views in one launch, bare and framed outputs, no ReLU: every pixel against torch's f32 convolution of the rounded operands, no
    NaN anywhere, the output's frame untouched.  (The second wave of a SIMD once stored garbage here: a 128-bit store's data registers
    were rewritten while the store waited for the bus behind the other wave -- profiles/EXPERIMENTS.md R5.13.)"""
    torch = gpu
    import torch.nn.functional as F
    from mv3d_tf_amd import ops
    T = getattr(torch, half)
    g = torch.Generator(device="cuda").manual_seed(5)
    views = [(2, 608, 608, 9), (2, 96, 320, 3), (1, 64, 512, 3)]
    for relu in (True, False):
        xs, ws, bs, refs = [], [], [], []
        for B, H, W, cin in views:
            x = torch.randn((B, H, W, cin), device="cuda", generator=g)
            w = torch.randn((64, cin, 3, 3), device="cuda", generator=g) * 0.2
            b = torch.randn(64, device="cuda", generator=g)
            xs.append(ops.frame_nhwc_f16(x, ops.framed_buffer(B, H, W, 16, "cuda", T)))
            ws.append(ops.pack_conv3x3_weights_input_layer(w, dtype=T))
            bs.append(b)
            r = F.conv2d(x.to(T).float().permute(0, 3, 1, 2), w.to(T).float(), b, padding=1).permute(0, 2, 3, 1)
            refs.append(F.relu(r) if relu else r)
        outs = [ops.framed_buffer(B, H, W, 64, "cuda", T) for B, H, W, _ in views]
        ops.conv3x3_views([(x, w, b, None, o) for x, w, b, o in zip(xs, ws, bs, outs)], relu=relu)
        torch.cuda.synchronize()
        tol = 4e-3 if half == "float16" else 3e-2
        for o, r in zip(outs, refs):
            inner = o[:, 1:-1, 1:-1].float()
            assert not bool(torch.isnan(inner).any())
            assert float((inner - r).abs().max()) <= tol * float(r.abs().max())
            frame = o.clone()
            frame[:, 1:-1, 1:-1] = 0
            assert float(frame.abs().max()) == 0.0


@pytest.mark.parametrize("dt", ["float16", "bfloat16", "float32"])
@pytest.mark.parametrize("B,H,W,C,Co", [(2, 37, 53, 9, 16), (1, 5, 7, 3, 16), (3, 16, 20, 64, 64), (1, 9, 9, 40, 40), (2, 8, 8, 9, 32), (1, 1, 1, 3, 16)])
def test_frame_nhwc_in_16_byte_pieces(gpu, dt, B, H, W, C, Co):
    """mv3d_frame_nhwc_*: the interior of the framed map = the input rounded to the map's type, channels past C and the frame zero -- through
    the 16-byte-piece kernel (C_out a multiple of the piece) and the element kernel (the rest), on a buffer that held garbage in its interior"""
    torch = gpu
    from mv3d_tf_amd import ops
    T = getattr(torch, dt)
    g = torch.Generator(device="cuda").manual_seed(C * 100 + W)
    x = torch.randn((B, H, W, C), device="cuda", generator=g) * 3.0
    out = ops.framed_buffer(B, H, W, Co, "cuda", T)
    out[:, 1:-1, 1:-1, :C] = 7.0                                       # (the owner zeroes frame and padding channels once; the interior is rewritten)
    ops.frame_nhwc_f16(x, out)
    torch.cuda.synchronize()
    assert torch.equal(out[:, 1:-1, 1:-1, :C], x.to(T))
    assert float(out[:, 1:-1, 1:-1, C:].abs().max()) == 0.0 if Co > C else True
    fr = out.clone()
    fr[:, 1:-1, 1:-1] = 0
    assert float(fr.abs().max()) == 0.0


def test_maxpool_and_two_layer_chain(gpu):
    torch = gpu
    from mv3d_tf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(3)
    B, H, W = 2, 37, 50
    x = torch.randn((B, H, W, 64), device="cuda", generator=g)
    w1 = torch.randn((64, 64, 3, 3), device="cuda", generator=g) * 0.06
    w2 = torch.randn((128, 64, 3, 3), device="cuda", generator=g) * 0.06
    b1, b2 = torch.randn(64, device="cuda", generator=g), torch.randn(128, device="cuda", generator=g)
    xf = ops.frame_nhwc_f16(x, ops.framed_buffer(B, H, W, 64, x.device))
    y1 = ops.conv3x3_f16(xf, ops.pack_conv3x3_weights(w1), b1)
    p1 = ops.maxpool2x2_f16(y1)
    y2 = ops.conv3x3_f16(p1, ops.pack_conv3x3_weights(w2), b2, out_framed=False, out_f32=True)
    torch.cuda.synchronize()
    # pool: exact on the f16 values (VALID / floor: the odd last row is dropped)
    want_p = torch.nn.functional.max_pool2d(y1[:, 1:-1, 1:-1].float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert p1.shape == (B, H // 2 + 2, W // 2 + 2, 64) and torch.equal(p1[:, 1:-1, 1:-1].float(), want_p)
    assert float(p1[:, 0].abs().max()) == 0 and float(p1[:, :, -1].abs().max()) == 0
    want = _reference(torch, want_p, w2, b2, True)
    assert float((y2 - want).abs().max()) <= 2e-5 * float(want.abs().max())


def test_bf16_entries_match_fp32_reference(gpu):
    """the training trunk's type: bf16 operands (8 mantissa bits), f32 accumulate; vs torch fp32 on the bf16-rounded operands:
    <= 1e-2 x max|want| for bf16 maps (one output rounding, 2^-8), 2e-5 for f32 maps; pool exact"""
    torch = gpu
    from mv3d_tf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(77)
    bf = torch.bfloat16
    B, H, W, cin, cout = 2, 38, 50, 128, 256
    x = torch.randn((B, H, W, cin), device="cuda", generator=g)
    w = torch.randn((cout, cin, 3, 3), device="cuda", generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn((cout,), device="cuda", generator=g)
    want = torch.relu(torch.nn.functional.conv2d(x.to(bf).float().permute(0, 3, 1, 2), w.to(bf).float(), b, padding=1)).permute(0, 2, 3, 1)
    xf = ops.frame_nhwc_f16(x, ops.framed_buffer(B, H, W, cin, x.device, bf))
    y16 = ops.conv3x3_f16(xf, ops.pack_conv3x3_weights(w, dtype=bf), b)
    y32 = ops.conv3x3_f16(xf, ops.pack_conv3x3_weights(w, dtype=bf), b, out_framed=False, out_f32=True)
    p16 = ops.maxpool2x2_f16(y16)
    torch.cuda.synchronize()
    scale = float(want.abs().max())
    assert y16.dtype == bf and float((y16[:, 1:-1, 1:-1].float() - want).abs().max()) <= 1e-2 * scale
    assert float((y32 - want).abs().max()) <= 2e-5 * scale
    wp = torch.nn.functional.max_pool2d(y16[:, 1:-1, 1:-1].float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert p16.dtype == bf and torch.equal(p16[:, 1:-1, 1:-1].float(), wp)
    # the input-layer variant
    x9 = torch.randn((1, 20, 24, 9), device="cuda", generator=g)
    w9 = torch.randn((64, 9, 3, 3), device="cuda", generator=g) * 0.3
    b9 = torch.zeros(64, device="cuda")
    want9 = torch.relu(torch.nn.functional.conv2d(x9.to(bf).float().permute(0, 3, 1, 2), w9.to(bf).float(), b9, padding=1)).permute(0, 2, 3, 1)
    got9 = ops.conv3x3_f16(ops.frame_nhwc_f16(x9, ops.framed_buffer(1, 20, 24, 16, "cuda", bf)), ops.pack_conv3x3_weights_input_layer(w9, bf), b9)
    assert float((got9[:, 1:-1, 1:-1].float() - want9).abs().max()) <= 1e-2 * float(want9.abs().max())


def test_large_batches_are_split_into_chunks(gpu, monkeypatch):
    """buffers beyond the kernel's 32-bit offsets: the wrapper runs the frames in chunks (here forced by a tiny limit)"""
    torch = gpu
    from mv3d_tf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(8)
    x = torch.randn((5, 12, 20, 64), device="cuda", generator=g)
    w = torch.randn((64, 64, 3, 3), device="cuda", generator=g) * 0.06
    b = torch.randn(64, device="cuda", generator=g)
    xf = ops.frame_nhwc_f16(x, ops.framed_buffer(5, 12, 20, 64, x.device))
    want = ops.conv3x3_f16(xf, ops.pack_conv3x3_weights(w), b)
    calls = []
    real = ops.lib().mv3d_conv3x3_f16
    monkeypatch.setattr(ops.lib(), "mv3d_conv3x3_f16", lambda *a: calls.append(a[4]) or real(*a))
    import builtins
    monkeypatch.setattr(ops, "max", lambda *a: 2 ** 30 if len(a) == 2 and a[0] == 14 * 22 * 64 * 2 else builtins.max(*a), raising=False)
    got = ops.conv3x3_f16(xf, ops.pack_conv3x3_weights(w), b)
    torch.cuda.synchronize()
    assert calls == [1, 1, 1, 1, 1] and torch.equal(got, want)


def test_weight_gradient_of_a_large_batch_is_summed_over_chunks(gpu, monkeypatch):
    """maps beyond the kernel's 32-bit offsets were refused; the wrapper now sums the gradient over batch chunks (here
    forced by a tiny limit) -- same values up to the f32 summation order"""
    torch = gpu
    from mv3d_tf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(9)
    B, H, W = 5, 12, 20
    x = ops.frame_nhwc_f16(torch.randn((B, H, W, 64), device="cuda", generator=g), ops.framed_buffer(B, H, W, 64, "cuda", torch.bfloat16))
    dy = ops.frame_nhwc_f16(torch.randn((B, H, W, 128), device="cuda", generator=g), ops.framed_buffer(B, H, W, 128, "cuda", torch.bfloat16))
    want_w, want_b = ops.conv3x3_wgrad_bf16(x, dy, want_bias=True)
    monkeypatch.setattr(ops, "_WGRAD_CHUNK_BYTES", 2 * (H + 2) * (W + 2) * 128 * 2)          # two frames per launch
    got_w, got_b = ops.conv3x3_wgrad_bf16(x, dy, want_bias=True)
    assert float((got_w - want_w).abs().max()) <= 1e-4 * float(want_w.abs().max())
    assert float((got_b - want_b).abs().max()) <= 1e-4 * float(want_b.abs().max())


def test_bad_arguments_are_refused(gpu):
    torch = gpu
    from mv3d_tf_amd import _lib, ops
    xf = ops.framed_buffer(1, 8, 8, 48, "cuda")
    with pytest.raises(_lib.Mv3dError):
        ops.conv3x3_f16(xf, torch.zeros((64, 9 * 48), dtype=torch.float16, device="cuda"), torch.zeros(64, device="cuda"))


@pytest.mark.parametrize("half", ["float16", "bfloat16"])
def test_serving_graph_on_the_mfma_trunk_matches_the_torch_f16_trunk(gpu, half):
    """MV3D_test forward with mfma_trunk = True against the same graph on torch's autocast f16 convolutions (He-scaled weights
    so that 13 layers keep O(1) activations): conv5_3 maps within 2 % of their max (two different f16 pipelines, 13 roundings
    deep), the same proposal count, finite detections."""
    torch = gpu
    import numpy as np
    from mv3d_tf_amd import synth
    from mv3d_tf_amd.networks import get_network
    net = get_network("MV3D_test")
    g = torch.Generator(device="cuda").manual_seed(11)
    with torch.no_grad():
        for name, (w, b) in net.params.items():
            if w.ndim == 4:
                w.copy_(torch.randn(w.shape, device="cuda", generator=g) * (2.0 / (w.shape[1] * w.shape[2] * w.shape[3])) ** 0.5)
                b.copy_(torch.randn(b.shape, device="cuda", generator=g) * 0.05)
    rng = np.random.RandomState(4)
    B = 2
    feed = {"lidar_bv_data": ((rng.random_sample((B, 608, 608, 9)) < 0.05) * rng.uniform(0, 2.4, (B, 608, 608, 9))).astype(np.float32),
            "image_data": rng.uniform(-1, 1, (B, 96, 320, 3)).astype(np.float32),
            "im_info": np.array([[608, 608, 1]] * B, np.float32), "calib": np.stack([synth.KITTI_CALIB] * B)}
    outs = {}
    dt = getattr(torch, half)
    tol = 0.02 if half == "float16" else 0.12            # (bf16: 8 mantissa bits, 13 layers deep, two different pipelines)
    for mfma in (False, True):
        net.amp_dtype, net.mfma_trunk = dt, mfma
        with torch.no_grad():
            L = net.forward(feed)
        torch.cuda.synchronize()
        outs[mfma] = {k: L[k].float().clone() for k in ("conv5_3", "conv5_3_2", "rpn_cls_score", "rpn_bbox_pred", "cls_prob", "bbox_pred")}
        outs[mfma]["n"] = L["rois"][0].shape[0]
        assert L["conv5_3"].dtype == torch.float32 and L["conv5_3"].shape == (B, 76, 76, 512) and L["conv5_3_2"].shape == (B, 12, 40, 512)
    a, b = outs[False], outs[True]
    for k in ("conv5_3", "conv5_3_2", "rpn_cls_score", "rpn_bbox_pred"):
        scale = float(a[k].abs().max())
        assert scale > 1e-3 and float((a[k] - b[k]).abs().max()) <= tol * scale, (k, scale, float((a[k] - b[k]).abs().max()))
    assert torch.isfinite(b["cls_prob"]).all() and torch.isfinite(b["bbox_pred"]).all() and b["n"] > 0
    net.mfma_trunk = True
    with pytest.raises(RuntimeError):
        net.forward(feed)                                  # grad mode + trainable parameters: the serving trunk refuses


def _torch_trunk(torch, layers, x_nhwc, params, amp=False):
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        x = x_nhwc.permute(0, 3, 1, 2)
        for name, _, pool in layers:
            w, b = params[name]
            x = torch.relu(torch.nn.functional.conv2d(x, w, b, padding=1))
            if pool:
                x = torch.nn.functional.max_pool2d(x, 2, 2)
        return x.permute(0, 2, 3, 1).float()


@pytest.mark.parametrize("wgrad", ["torch", "mfma"])
def test_training_trunk_gradients_match_torch_autograd(gpu, wgrad):
    """mv3d_tf_amd.trunk_train.TrunkFunction (bf16 activations / gradients, f32 accumulation) against torch autograd of the same
    trunk (5 layers, 2 pools) in fp32.  A bf16 pipeline differs from fp32 by more than rounding: ReLU masks and pool routes of
    near-ties flip, so even torch's own bf16 autocast only reaches cosine 0.988 - 0.999 per gradient tensor here
    (tools/trunk_grad_debug.py).  The bar: every weight / bias gradient has cosine >= 0.98 with the fp32 gradient AND is no
    further from it than torch's bf16 autocast gradient is (cosine within 0.003); a wrong tap flip / channel swap / pool routing
    gives a cosine near 0."""
    torch = gpu
    from mv3d_tf_amd import trunk_train
    if wgrad == "mfma" and not hasattr(trunk_train, "wgrad_mfma"):
        pytest.skip("weight gradient on the MFMA kernel not built")
    layers = [("a", 64, False), ("b", 64, True), ("c", 128, False), ("d", 128, True), ("e", 256, False)]
    g = torch.Generator(device="cuda").manual_seed(5)
    params, cin = {}, 9
    for name, cout, _ in layers:
        w = (torch.randn((cout, cin, 3, 3), device="cuda", generator=g) * (2.0 / (9 * cin)) ** 0.5).requires_grad_(True)
        b = (torch.randn((cout,), device="cuda", generator=g) * 0.1).requires_grad_(True)
        params[name] = [w, b]
        cin = cout
    x = torch.randn((2, 42, 54, 9), device="cuda", generator=g)            # 42 x 54 -> 21 x 27 -> 10 x 13 (an odd size is dropped)
    R = torch.randn((2, 10, 13, 256), device="cuda", generator=g)

    def grads(fn):
        for v in params.values():
            v[0].grad = v[1].grad = None
        out = fn()
        (out * R).sum().backward()
        return out.detach(), {k: (v[0].grad.clone().float(), v[1].grad.clone().float()) for k, v in params.items()}

    o32, g32 = grads(lambda: _torch_trunk(torch, layers, x, params))
    _, gam = grads(lambda: _torch_trunk(torch, layers, x, params, amp=True))
    fn = trunk_train._wgrad_torch if wgrad == "torch" else trunk_train.wgrad_mfma
    out, got = grads(lambda: trunk_train.trunk(layers, x, params, "", wgrad=fn))
    torch.cuda.synchronize()
    assert out.shape == o32.shape and float((out - o32).abs().max()) <= 0.04 * float(o32.abs().max())
    cos = lambda a, b: float(torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0))
    for name, _, _ in layers:
        for k in (0, 1):
            c_mine, c_amp = cos(got[name][k], g32[name][k]), cos(gam[name][k], g32[name][k])
            assert c_mine >= 0.98 and c_mine >= c_amp - 0.003, (name, k, c_mine, c_amp)


def test_train_graph_on_the_mfma_trunk(gpu):
    """MV3D_train with mfma_trunk = True (bf16 trunks forward + backward on the MFMA kernels, fp32 master weights): the step's
    loss is within 2 % of the fp32 graph's on the same frame / seed / weights, every trunk parameter gets a finite non-zero
    gradient whose direction agrees with the fp32 graph's (cosine >= 0.9 on the layers next to the heads, where the gradient
    has not yet passed through a dozen bf16 layers and the sampled-ROI noise is the same), and an Adam step runs."""
    torch = gpu
    import numpy as np
    from mv3d_tf_amd import synth
    from mv3d_tf_amd.fast_rcnn.train_mv import total_loss
    from mv3d_tf_amd.networks import get_network
    net = get_network("MV3D_train")
    g = torch.Generator(device="cuda").manual_seed(21)
    with torch.no_grad():
        for name, (w, b) in net.params.items():
            if w.ndim == 4 and w.shape[2] == 3:
                w.copy_(torch.randn(w.shape, device="cuda", generator=g) * (2.0 / (w.shape[1] * 9)) ** 0.5)
        net.params["rpn_cls_score"][0].mul_(20.0)
    rng = np.random.RandomState(2)
    r = np.random.RandomState(31)
    gt = synth.gt_cars(r, 4)
    feed = {"lidar_bv_data": ((rng.random_sample((1, 608, 608, 9)) < 0.05) * rng.uniform(0, 2.4, (1, 608, 608, 9))).astype(np.float32),
            "image_data": rng.uniform(-1, 1, (1, 375, 1242, 3)).astype(np.float32), "im_info": np.array([[608, 608, 1]], np.float32),
            "calib": synth.KITTI_CALIB[None], "gt_boxes_bv": gt[0], "gt_boxes_3d": gt[1], "gt_boxes_corners": gt[2], "keep_prob": 1.0}
    res = {}
    for mfma in (False, True):
        net.mfma_trunk, net.amp_dtype = mfma, (torch.bfloat16 if mfma else None)
        for p in net.parameters():
            p.grad = None
        np.random.seed(4)
        loss, _ = total_loss(net.forward(feed))
        loss.backward()
        torch.cuda.synchronize()
        res[mfma] = (float(loss), {k: v[0].grad.clone() for k, v in net.params.items() if v[0].grad is not None})
    l32, g32 = res[False]
    l16, g16 = res[True]
    assert np.isfinite(l16) and abs(l16 - l32) <= 0.02 * abs(l32), (l16, l32)
    cos = lambda a, b: float(torch.nn.functional.cosine_similarity(a.flatten().float(), b.flatten().float(), dim=0))
    for name, _, _ in [(s + sfx, 0, 0) for s in ("conv1_1", "conv3_2", "conv5_3") for sfx in ("", "_2")]:
        assert name in g16 and torch.isfinite(g16[name]).all() and float(g16[name].abs().sum()) > 0 and float(g32[name].abs().sum()) > 0, name
    for name in ("conv5_3", "conv5_2", "conv5_3_2"):
        assert cos(g16[name], g32[name]) >= 0.9, (name, cos(g16[name], g32[name]))
    opt = torch.optim.Adam(net.parameters(), lr=1e-5, fused=True)
    before = net.params["conv4_1"][0].detach().clone()
    opt.step()
    assert not torch.equal(before, net.params["conv4_1"][0])


@pytest.mark.parametrize("B,H,W,cin,cout,creal", [(2, 38, 50, 128, 256, None), (1, 21, 33, 64, 64, 9), (2, 12, 40, 256, 512, None)])
def test_f32_weight_gradient_kernel_matches_torch(gpu, B, H, W, cin, cout, creal):
    """mv3d_conv3x3_wgrad_f32 (exact f32 on v_mfma_f32_32x32x2_f32) against torch's fp32 conv2d_weight: <= 2e-5 of the largest entry"""
    torch = gpu
    from mv3d_tf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(B + H + cin + 1)
    x = torch.randn((B, H, W, cin), device="cuda", generator=g)
    dy = torch.randn((B, H, W, cout), device="cuda", generator=g)
    xf = ops.framed_buffer(B, H, W, cin, "cuda", torch.float32)
    xf[:, 1:-1, 1:-1] = x
    dyf = ops.framed_buffer(B, H, W, cout, "cuda", torch.float32)
    dyf[:, 1:-1, 1:-1] = dy
    got, got_b = ops.conv3x3_wgrad_bf16(xf, dyf, creal, want_bias=True)
    want = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (cout, cin, 3, 3), dy.permute(0, 3, 1, 2), padding=1)
    if creal:
        want = want[:, :creal]
    want_b = dy.sum((0, 1, 2))
    torch.cuda.synchronize()
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max())
    assert float((got_b - want_b).abs().max()) <= 2e-5 * float(want_b.abs().max())


@pytest.mark.parametrize("B,H,W,cin,cout,creal", [(2, 38, 50, 128, 256, None), (1, 21, 33, 64, 64, 9), (2, 12, 40, 256, 512, None)])
def test_weight_gradient_kernel_matches_torch(gpu, B, H, W, cin, cout, creal):
    """mv3d_conv3x3_wgrad_bf16 against torch's conv2d_weight in fp32 on the SAME bf16-rounded operands: the kernel multiplies
    bf16 exactly and accumulates in f32 (per split, then over the splits), so only the summation order differs: <= 1e-4 of the
    largest entry.  Asymmetric random operands: a wrong tap / transposed-read mapping cannot pass."""
    torch = gpu
    from mv3d_tf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(B + H + cin)
    bf = torch.bfloat16
    x = torch.randn((B, H, W, cin), device="cuda", generator=g).to(bf)
    dy = torch.randn((B, H, W, cout), device="cuda", generator=g).to(bf)
    xf = ops.framed_buffer(B, H, W, cin, "cuda", bf)
    xf[:, 1:-1, 1:-1] = x
    dyf = ops.framed_buffer(B, H, W, cout, "cuda", bf)
    dyf[:, 1:-1, 1:-1] = dy
    got, got_b = ops.conv3x3_wgrad_bf16(xf, dyf, creal, want_bias=True)
    want_b = dy.float().sum((0, 1, 2))
    assert float((got_b - want_b).abs().max()) <= 1e-4 * float(want_b.abs().max())
    want = torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (cout, cin, 3, 3), dy.float().permute(0, 3, 1, 2), padding=1)
    if creal:
        want = want[:, :creal]
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.is_contiguous()
    assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max())


def test_one_launch_weight_packing(gpu):
    """mv3d_conv3x3_pack_bf16 = the torch packing of the forward filter and of the flipped / channel-swapped data-gradient filter"""
    torch = gpu
    from mv3d_tf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(3)
    w = torch.randn((128, 64, 3, 3), device="cuda", generator=g)
    fwd, dg = ops.pack_conv3x3_train_bf16(w)
    assert torch.equal(fwd, ops.pack_conv3x3_weights(w, dtype=torch.bfloat16))
    assert torch.equal(dg, ops.pack_conv3x3_weights(w.flip(2, 3).transpose(0, 1), dtype=torch.bfloat16))
    w9 = torch.randn((64, 9, 3, 3), device="cuda", generator=g)
    fwd9, none = ops.pack_conv3x3_train_bf16(w9, 64, want_dgrad=False)
    assert none is None and torch.equal(fwd9, ops.pack_conv3x3_weights(w9, 64, dtype=torch.bfloat16))


def test_gated_data_gradient_and_pool_backward(gpu):
    """mv3d_conv3x3_gated_bf16 = convolution, then zero where the gate map is <= 0; mv3d_maxpool2x2_bwd_bf16 = torch's max_pool2d
    backward (first maximum of the window) times the ReLU mask -- both exact on the bf16 values"""
    torch = gpu
    from mv3d_tf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(12)
    bf = torch.bfloat16
    B, H, W, cin, cout = 2, 21, 30, 128, 64
    x = torch.randn((B, H, W, cin), device="cuda", generator=g)
    w = torch.randn((cout, cin, 3, 3), device="cuda", generator=g) * 0.03
    zero = torch.zeros(cout, device="cuda")
    gate = torch.randn((B, H, W, cout), device="cuda", generator=g).to(bf)
    xf = ops.frame_nhwc_f16(x, ops.framed_buffer(B, H, W, cin, "cuda", bf))
    gf = ops.framed_buffer(B, H, W, cout, "cuda", bf)
    gf[:, 1:-1, 1:-1] = gate
    wp = ops.pack_conv3x3_weights(w, dtype=bf)
    plain = ops.conv3x3_f16(xf, wp, zero, relu=False)
    gated = ops.conv3x3_gated_bf16(xf, wp, zero, gf, ops.framed_buffer(B, H, W, cout, "cuda", bf))
    torch.cuda.synchronize()
    assert torch.equal(gated, torch.where(gf > 0, plain, torch.zeros_like(plain)))
    # pool backward on a ReLU output with ties at 0
    y = torch.relu(torch.randn((B, H, W, cout), device="cuda", generator=g)).to(bf)
    yf = ops.framed_buffer(B, H, W, cout, "cuda", bf)
    yf[:, 1:-1, 1:-1] = y
    gp = torch.randn((B, H // 2, W // 2, cout), device="cuda", generator=g).to(bf)
    gpf = ops.framed_buffer(B, H // 2, W // 2, cout, "cuda", bf)
    gpf[:, 1:-1, 1:-1] = gp
    got = ops.maxpool2x2_bwd_bf16(yf, gpf, ops.framed_buffer(B, H, W, cout, "cuda", bf))[:, 1:-1, 1:-1].float()
    yy = y.float().permute(0, 3, 1, 2).requires_grad_(True)
    torch.nn.functional.max_pool2d(yy, 2, 2).backward(gp.float().permute(0, 3, 1, 2))
    want = (yy.grad * (yy > 0)).permute(0, 2, 3, 1)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_mixed_precision_training_converges_like_fp32(gpu):
    """Ten Adam steps (lr 1e-4) on ONE fixed frame with frozen sampling: the loss of the graph on the bf16 MFMA trunks falls like the
    fp32 graph's (tools/train_converge_probe.py: 3.69 -> 0.80 vs 3.69 -> 0.81 in 12 steps): both end below 40 % of the start, the
    first losses agree to 1 %, the last ones to 30 % of each other (the two runs are different floating-point trajectories)."""
    torch = gpu
    import numpy as np
    from mv3d_tf_amd import synth
    from mv3d_tf_amd.fast_rcnn.train_mv import total_loss
    from mv3d_tf_amd.networks import get_network
    rng = np.random.RandomState(2)
    gt = synth.gt_cars(np.random.RandomState(31), 4)
    feed = {"lidar_bv_data": ((rng.random_sample((1, 608, 608, 9)) < 0.05) * rng.uniform(0, 2.4, (1, 608, 608, 9))).astype(np.float32),
            "image_data": rng.uniform(-1, 1, (1, 375, 1242, 3)).astype(np.float32), "im_info": np.array([[608, 608, 1]], np.float32),
            "calib": synth.KITTI_CALIB[None], "gt_boxes_bv": gt[0], "gt_boxes_3d": gt[1], "gt_boxes_corners": gt[2], "keep_prob": 1.0}
    hist = {}
    for mixed in (False, True):
        net = get_network("MV3D_train")
        g = torch.Generator(device="cuda").manual_seed(21)
        with torch.no_grad():
            for name, (w, b) in net.params.items():
                if w.ndim == 4 and w.shape[2] == 3:
                    w.copy_(torch.randn(w.shape, device="cuda", generator=g) * (2.0 / (w.shape[1] * 9)) ** 0.5)
            net.params["rpn_cls_score"][0].mul_(20.0)
        net.mfma_trunk, net.amp_dtype = mixed, (torch.bfloat16 if mixed else None)
        opt = torch.optim.Adam(net.parameters(), lr=1e-4, fused=True)
        hist[mixed] = []
        for _ in range(10):
            np.random.seed(4)
            opt.zero_grad(set_to_none=True)
            loss, _ = total_loss(net.forward(feed))
            loss.backward()
            opt.step()
            hist[mixed].append(float(loss.detach()))
        del net, opt
        torch.cuda.empty_cache()
    a, b = hist[False], hist[True]
    assert all(np.isfinite(b)) and abs(a[0] - b[0]) <= 0.01 * a[0]
    assert a[-1] < 0.4 * a[0] and b[-1] < 0.4 * b[0], (a, b)
    assert abs(a[-1] - b[-1]) <= 0.3 * max(a[-1], b[-1]), (a, b)


@pytest.mark.parametrize("B,H,W,cin,cout,relu,framed", [(2, 38, 50, 128, 256, True, True), (1, 21, 33, 32, 64, False, False),
                                                        (1, 46, 155, 512, 512, True, False)])
def test_exact_f32_convolution(gpu, B, H, W, cin, cout, relu, framed):
    """mv3d_conv3x3_f32 (v_mfma_f32_32x32x2_f32: exact f32 products and sums) against torch's fp32 convolution: only the summation
    order differs -> <= 2e-5 of the map's largest value; the f32 pool is exact"""
    torch = gpu
    from mv3d_tf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(B + H + cout)
    x = torch.randn((B, H, W, cin), device="cuda", generator=g)
    w = torch.randn((cout, cin, 3, 3), device="cuda", generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn((cout,), device="cuda", generator=g)
    prev = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    want = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1).permute(0, 2, 3, 1)
    torch.backends.cudnn.allow_tf32 = prev
    if relu:
        want = torch.relu(want)
    xf = ops.frame_nhwc_f16(x, ops.framed_buffer(B, H, W, cin, "cuda", torch.float32))
    got = ops.conv3x3_f16(xf, ops.pack_conv3x3_weights(w, dtype=torch.float32), b, out_framed=framed, relu=relu)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32
    if framed:
        assert float(got[:, 0].abs().max()) == 0 and float(got[:, :, -1].abs().max()) == 0
        p = ops.maxpool2x2_f16(got)
        assert torch.equal(p[:, 1:-1, 1:-1], torch.nn.functional.max_pool2d(got[:, 1:-1, 1:-1].permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1))
        got = got[:, 1:-1, 1:-1]
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max())


def test_serving_graph_in_reference_precision_on_the_f32_mfma_trunk(gpu):
    """MV3D_test with mfma_trunk = True and amp_dtype = None (fp32) against the torch / MIOpen fp32 graph: the conv5_3 maps and the
    RPN head agree to 1e-4 of their largest value (13 layers of re-ordered f32 sums), the detections' shapes match"""
    torch = gpu
    import numpy as np
    from mv3d_tf_amd import synth
    from mv3d_tf_amd.networks import get_network
    net = get_network("MV3D_test")
    g = torch.Generator(device="cuda").manual_seed(11)
    with torch.no_grad():
        for name, (w, b) in net.params.items():
            if w.ndim == 4:
                w.copy_(torch.randn(w.shape, device="cuda", generator=g) * (2.0 / (w.shape[1] * w.shape[2] * w.shape[3])) ** 0.5)
                b.copy_(torch.randn(b.shape, device="cuda", generator=g) * 0.05)
    rng = np.random.RandomState(4)
    B = 2
    feed = {"lidar_bv_data": ((rng.random_sample((B, 608, 608, 9)) < 0.05) * rng.uniform(0, 2.4, (B, 608, 608, 9))).astype(np.float32),
            "image_data": rng.uniform(-1, 1, (B, 96, 320, 3)).astype(np.float32),
            "im_info": np.array([[608, 608, 1]] * B, np.float32), "calib": np.stack([synth.KITTI_CALIB] * B)}
    outs = {}
    for mfma in (False, True):
        net.amp_dtype, net.mfma_trunk = None, mfma
        with torch.no_grad():
            L = net.forward(feed)
        torch.cuda.synchronize()
        outs[mfma] = {k: L[k].float().clone() for k in ("conv5_3", "conv5_3_2", "rpn_cls_score", "rpn_bbox_pred")}
        assert L["conv5_3"].dtype == torch.float32 and (L["conv5_3"].is_contiguous() or not mfma)
    for k in outs[True]:
        scale = float(outs[False][k].abs().max())
        assert float((outs[False][k] - outs[True][k]).abs().max()) <= 1e-4 * scale, (k, scale)


def test_fp32_training_trunk_matches_torch_autograd(gpu):
    """trunk_train.trunk(dtype=float32): forward, data gradient and weight gradient on the exact-f32 MFMA kernels -- the reference's
    precision, so against torch fp32 autograd of the same trunk the gradients agree to 1e-3 of their largest entry
    (re-ordered f32 sums through 5 layers and 2 pools; no ReLU / pool-route flips as in the 16-bit trunks) with cosine >= 0.99999"""
    torch = gpu
    from mv3d_tf_amd import trunk_train
    layers = [("a", 64, False), ("b", 64, True), ("c", 128, False), ("d", 128, True), ("e", 256, False)]
    g = torch.Generator(device="cuda").manual_seed(5)
    params, cin = {}, 9
    for name, cout, _ in layers:
        params[name] = [(torch.randn((cout, cin, 3, 3), device="cuda", generator=g) * (2.0 / (9 * cin)) ** 0.5).requires_grad_(True),
                        (torch.randn((cout,), device="cuda", generator=g) * 0.1).requires_grad_(True)]
        cin = cout
    x = torch.randn((2, 42, 54, 9), device="cuda", generator=g)
    R = torch.randn((2, 10, 13, 256), device="cuda", generator=g)

    def grads(fn):
        for v in params.values():
            v[0].grad = v[1].grad = None
        out = fn()
        (out * R).sum().backward()
        return out.detach(), {k: (v[0].grad.clone().float(), v[1].grad.clone().float()) for k, v in params.items()}

    o32, g32 = grads(lambda: _torch_trunk(torch, layers, x, params))
    out, got = grads(lambda: trunk_train.trunk(layers, x, params, "", dtype=torch.float32))
    torch.cuda.synchronize()
    assert float((out - o32).abs().max()) <= 1e-4 * float(o32.abs().max())
    cos = lambda a, b: float(torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0))
    for name, _, _ in layers:
        for k in (0, 1):
            assert cos(got[name][k], g32[name][k]) >= 0.99999, (name, k, cos(got[name][k], g32[name][k]))
            assert float((got[name][k] - g32[name][k]).abs().max()) <= 1e-3 * float(g32[name][k].abs().max()), (name, k)


# ---------------------------------------------------------------------------------------------------- grouped launches (round 4)
_VIEW_SIZES = [(2, 19, 23), (1, 37, 50), (2, 8, 64)]            # three "trunks" of one layer shape, different maps


@pytest.mark.parametrize("dt,cin,cout", [("f16", 64, 64), ("bf16", 128, 256), ("f32", 64, 128), ("bf16", 512, 512)])
def test_grouped_views_equal_the_single_view_entries(gpu, dt, cin, cout):
    """mv3d_conv3x3_views_* / maxpool2x2[_bwd]_views_* / conv3x3_wgrad_views_*: one launch for several maps of one layer shape gives,
    per view, the bits of the single-view entry.  At these sizes the grouped launch runs the same kernel and tiles (a view's workgroups
    only start at another block index); the kernel is chosen by the tile count of ALL views, so larger views can move a grouped launch to
    a bigger tile than each view alone would get -- tests/test_conv_paths.py covers those, the bits stay the same."""
    torch = gpu
    from mv3d_tf_amd import ops
    T = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[dt]
    g = torch.Generator(device="cuda").manual_seed(11)
    xs, ws, bs = [], [], []
    for B, H, W in _VIEW_SIZES:
        xs.append(ops.frame_nhwc_f16(torch.randn((B, H, W, cin), device="cuda", generator=g), ops.framed_buffer(B, H, W, cin, "cuda", T)))
        ws.append(ops.pack_conv3x3_weights(torch.randn((cout, cin, 3, 3), device="cuda", generator=g) * 0.05, dtype=T))
        bs.append(torch.randn(cout, device="cuda", generator=g))
    single = [ops.conv3x3_f16(x, w, b) for x, w, b in zip(xs, ws, bs)]
    outs = [torch.zeros_like(y) for y in single]
    ops.conv3x3_views([(x, w, b, None, o) for x, w, b, o in zip(xs, ws, bs, outs)])
    for a, b in zip(single, outs):
        assert torch.equal(a, b)
    # gate (the data-gradient form): grouped == conv followed by the mask
    if dt != "f16":
        gates = [torch.randn(y.shape, device="cuda", generator=g).to(T) * (y != 0) for y in single]
        outs2 = [torch.zeros_like(y) for y in single]
        ops.conv3x3_views([(x, w, b, gt, o) for x, w, b, gt, o in zip(xs, ws, bs, gates, outs2)], relu=False)
        for x, w, b, gt, o in zip(xs, ws, bs, gates, outs2):
            want = ops.conv3x3_f16(x, w, b, relu=False) * (gt > 0)
            assert torch.equal(o, want)
    # pools
    pooled = [ops.maxpool2x2_f16(y) for y in single]
    pouts = [torch.zeros_like(p) for p in pooled]
    ops.maxpool2x2_views([(y, o) for y, o in zip(single, pouts)])
    for a, b in zip(pooled, pouts):
        assert torch.equal(a, b)
    if dt != "f16":
        gs = [torch.randn(p.shape, device="cuda", generator=g).to(T) for p in pooled]
        for gq in gs:
            gq[:, 0] = 0; gq[:, -1] = 0; gq[:, :, 0] = 0; gq[:, :, -1] = 0
        want = [ops.maxpool2x2_bwd_bf16(y, gq, torch.zeros_like(y)) for y, gq in zip(single, gs)]
        got = ops.maxpool2x2_bwd_views([(y, gq, torch.zeros_like(y)) for y, gq in zip(single, gs)])
        for a, b in zip(want, got):
            assert torch.equal(a, b)
        # weight gradients: grouped plans split K differently from single launches -> same values up to the f32 summation order
        dys = [torch.randn(y.shape, device="cuda", generator=g).to(T) * (y != 0) for y in single]
        want = [ops.conv3x3_wgrad_bf16(x, dy, want_bias=True) for x, dy in zip(xs, dys)]
        got = ops.conv3x3_wgrad_views(list(zip(xs, dys)), want_bias=True)
        for (dw, db), (gw, gb) in zip(want, got):
            assert float((dw - gw).abs().max()) <= 2e-4 * float(dw.abs().max()) and float((db - gb).abs().max()) <= 2e-4 * float(db.abs().max())
        again = ops.conv3x3_wgrad_views(list(zip(xs, dys)), want_bias=True)
        for (gw, gb), (hw, hb) in zip(got, again):
            assert torch.equal(gw, hw) and torch.equal(gb, hb)                  # deterministic: a fixed fold order


@pytest.mark.parametrize("dt,cin,cout", [("f16", 64, 64), ("f16", 128, 128), ("bf16", 64, 256)])
def test_convolution_with_the_pool_in_its_epilogue(gpu, dt, cin, cout):
    """mv3d_conv3x3_pool_views_*: convolution + ReLU + 2x2 VALID max pool in one launch == the convolution entry followed by the pool
    entry, bit for bit (odd heights / widths drop their last row / column; maps narrower than a tile; tiles over the right edge)"""
    torch = gpu
    from mv3d_tf_amd import ops
    T = {"f16": torch.float16, "bf16": torch.bfloat16}[dt]
    g = torch.Generator(device="cuda").manual_seed(5)
    views, want = [], []
    for B, H, W in [(2, 19, 23), (1, 37, 150), (2, 8, 64), ][:3]:
        x = ops.frame_nhwc_f16(torch.randn((B, H, W, cin), device="cuda", generator=g), ops.framed_buffer(B, H, W, cin, "cuda", T))
        w = ops.pack_conv3x3_weights(torch.randn((cout, cin, 3, 3), device="cuda", generator=g) * 0.05, dtype=T)
        b = torch.randn(cout, device="cuda", generator=g)
        want.append(ops.maxpool2x2_f16(ops.conv3x3_f16(x, w, b)))
        views.append((x, w, b, ops.framed_buffer(B, H // 2, W // 2, cout, "cuda", T)))
    got = ops.conv3x3_pool_views(views)
    torch.cuda.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b)


def test_one_launch_packing_of_many_filters(gpu):
    torch = gpu
    from mv3d_tf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(2)
    ws = [torch.randn(s, device="cuda", generator=g) for s in [(64, 9, 3, 3), (64, 64, 3, 3), (128, 64, 3, 3), (512, 256, 3, 3), (64, 3, 3, 3)]]
    for T in (torch.bfloat16, torch.float32):
        got = ops.pack_conv3x3_train_many([(w, 64 if w.shape[1] < 64 else None, w.shape[1] >= 64) for w in ws], dtype=T)
        for w, (fwd, dg) in zip(ws, got):
            assert torch.equal(fwd, ops.pack_conv3x3_weights(w, 64 if w.shape[1] < 64 else None, dtype=T))
            if w.shape[1] >= 64:
                assert torch.equal(dg, ops.pack_conv3x3_weights(w.flip(2, 3).transpose(0, 1), dtype=T))
            else:
                assert dg is None
