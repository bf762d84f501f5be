"""Upsampled ROI features: the bilinear 2x / 4x upsampling in front of RoiPool.

CPU: the numpy restatement (tests/upsample_restatement.py) against float64 interpolation matrices, the properties of the coordinate rule,
the argument errors of the C entries (they return before any HIP call), roi_pool_views' per-view scale and the constructor's errors.
GPU: the kernels against the restatement on raw bits, and the graphs with cfg.ROI_UPSAMPLE / MV3D(roi_upsample=)."""
import itertools

import numpy as np
import pytest

import upsample_restatement as ur

gpu = pytest.mark.gpu
EPS = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- the restatement (no GPU)
def _rand(rng, shape):
    return (rng.standard_normal(shape) * np.exp(rng.uniform(-3, 3, shape))).astype(np.float32)


@pytest.mark.parametrize("s", (2, 4))
@pytest.mark.parametrize("hw", ((1, 1), (1, 5), (2, 2), (3, 2), (7, 9)))
def test_restatement_forward_against_float64_matrices(hw, s):
    """|restated - A_y X A_x^T| <= 5 * 2^-24 * max|the taps' values| per output: four roundings on any path to first order (two products
    and a sum horizontally, the same vertically, the horizontal error scaled by weights that sum to 1), plus room for second order"""
    H, W = hw
    rng = np.random.RandomState(10 * H + W + s)
    x = _rand(rng, (2, H, W, 3))
    y = ur.forward(x, s)
    Ay, Ax = ur.matrix(H, s), ur.matrix(W, s)
    want = np.einsum("oi,biwc,pw->bopc", Ay, x.astype(np.float64), Ax)
    big = np.zeros(want.shape, np.float64)                # max |value| over the (at most four) source pixels an output has taps on
    ty, tx = ur.taps(H, s), ur.taps(W, s)
    for oy in range(s * H):
        for ox in range(s * W):
            big[:, oy, ox] = np.max([np.abs(x[:, iy, ix]).astype(np.float64) for iy, _ in ty[oy] for ix, _ in tx[ox]], axis=0)
    assert y.dtype == np.float32 and y.shape == want.shape
    assert (np.abs(y.astype(np.float64) - want) <= 5 * EPS * big).all()


@pytest.mark.parametrize("s", (2, 4))
@pytest.mark.parametrize("hw", ((1, 1), (1, 5), (2, 2), (3, 2), (7, 9)))
def test_restatement_backward_against_float64_matrices(hw, s):
    """|restated - A_y^T G A_x| <= (T + 2) * 2^-24 * sum|W g| per element, T the number of terms: the any-order summation bound
    (T - 1 additions and one product rounding per term)"""
    H, W = hw
    rng = np.random.RandomState(100 + 10 * H + W + s)
    g = _rand(rng, (2, s * H, s * W, 3))
    gx = ur.backward(g, s, H, W)
    Ay, Ax = ur.matrix(H, s), ur.matrix(W, s)
    want = np.einsum("oi,bopc,pw->biwc", Ay, g.astype(np.float64), Ax)
    mass = np.einsum("oi,bopc,pw->biwc", Ay, np.abs(g).astype(np.float64), Ax)
    T = np.einsum("oi,pw->iw", (Ay > 0).astype(np.float64), (Ax > 0).astype(np.float64))
    assert T.max() <= (2 * s - 1) ** 2
    assert gx.dtype == np.float32 and gx.shape == (2, H, W, 3)
    assert (np.abs(gx.astype(np.float64) - want) <= (T[None, :, :, None] + 2) * EPS * mass).all()


@pytest.mark.parametrize("s", (2, 4))
def test_adjointness_in_float64(s):
    rng = np.random.RandomState(s)
    H, W = 5, 7
    Ay, Ax = ur.matrix(H, s), ur.matrix(W, s)
    x, g = rng.standard_normal((H, W)), rng.standard_normal((s * H, s * W))
    lhs, rhs = ((Ay @ x @ Ax.T) * g).sum(), (x * (Ay.T @ g @ Ax)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


@pytest.mark.parametrize("s", (2, 4))
def test_rows_sum_to_one_and_interior_columns_to_s(s):
    for n in (1, 2, 3, 9):
        A = ur.matrix(n, s)
        assert np.array_equal(A.sum(1), np.ones(s * n))
        assert np.array_equal(A.sum(0)[1:-1], np.full(max(n - 2, 0), float(s)))
        assert A.sum() == s * n
        for tp in ur.taps(n, s):
            assert len(tp) in (1, 2) and (len(tp) == 2 or tp[0][1] == 1.0)
            assert all(w > 0 and (w * s) == int(w * s) for _, w in tp)


SPECIALS = (0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF)      # NaN, +Inf, -Inf, -0.0, subnormals


def _special_map(H, W, Cn, seed):
    """finite noise with a special value on every other pixel (a checkerboard) and on the whole last row and column"""
    rng = np.random.RandomState(seed)
    bits = _rand(rng, (1, H, W, Cn)).view(np.uint32).copy()
    k = 0
    for iy in range(H):
        for ix in range(W):
            if (iy + ix) % 2 == 1 or iy == H - 1 or ix == W - 1:
                bits[0, iy, ix, :] = SPECIALS[k % len(SPECIALS)]
                bits[0, iy, ix, 0] = SPECIALS[(k + 1) % len(SPECIALS)]
                k += 1
    return bits


def _aligned_and_clamped_bits_hold(ybits, xbits, s):
    H, W = xbits.shape[1:3]
    assert np.array_equal(ybits[:, ::s, ::s], xbits)                                      # up-pixel s i IS source pixel i
    for d in range(s):                                                                    # the clamped last rows / columns: one tap of weight 1
        assert np.array_equal(ybits[:, s * (H - 1) + d, ::s], xbits[:, H - 1])
        assert np.array_equal(ybits[:, ::s, s * (W - 1) + d], xbits[:, :, W - 1])
        for e in range(s):
            assert np.array_equal(ybits[:, s * (H - 1) + d, s * (W - 1) + e], xbits[:, H - 1, W - 1])


@pytest.mark.parametrize("s", (2, 4))
def test_restated_aligned_pixels_are_the_source_bits_next_to_specials(s):
    xbits = _special_map(4, 5, 3, 7)
    y = ur.forward(xbits.view(np.float32), s)
    _aligned_and_clamped_bits_hold(y.view(np.uint32), xbits, s)


# ---------------------------------------------------------------------------------------------------- arguments (no GPU)
@pytest.fixture(scope="module")
def hiplib():
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import _lib
    return _lib


def _view(_lib, in_=4096, out=8192, strides=None, dtype=0, batch=1, height=4, width=4, channels=8, factor=2):
    fs, rs, ps = strides or (height * width * channels, width * channels, channels)
    return _lib.UpsampleView(in_, out, fs, rs, ps, dtype, batch, height, width, channels, factor)


def test_c_entries_refuse_bad_arguments_before_any_hip_call(hiplib):
    """(the pointers are never dereferenced: every call returns from the argument checks)"""
    L, bad = hiplib.lib(), hiplib.ERR_INVALID_ARG
    fwd, bwd = L.mv3d_upsample_bilinear_views, L.mv3d_upsample_bilinear_backward_views

    def arr(*vs):
        a = (hiplib.UpsampleView * len(vs))()
        for k, v in enumerate(vs):
            a[k] = v
        return a

    ok = _view(hiplib)
    for fn in (fwd, bwd):
        assert fn(0, arr(ok), None) == bad and fn(5, arr(ok, ok, ok, ok, ok), None) == bad and fn(-1, arr(ok), None) == bad
        assert fn(1, None, None) == bad
        for kw in (dict(dtype=3), dict(dtype=-1), dict(factor=1), dict(factor=3), dict(factor=8), dict(factor=0), dict(batch=-1),
                   dict(height=0), dict(width=0), dict(channels=0), dict(in_=None), dict(out=None),
                   dict(height=1 << 13, width=1 << 13, channels=8),                       # 2 * 2^13 * 2 * 2^13 * 8 = 2^31 elements up
                   dict(height=1 << 12, width=1 << 13, channels=8, factor=4)):
            assert fn(1, arr(_view(hiplib, **kw)), None) == bad, kw
        assert fn(2, arr(ok, _view(hiplib, factor=3)), None) == bad                       # every view is checked
        # nothing to launch: batch == 0 (NULL buffers allowed) returns OK without a device
        assert fn(1, arr(_view(hiplib, batch=0, in_=None, out=None)), None) == hiplib.OK
    for st in ((128, 32, 7), (128, 31, 8), (127, 32, 8), (128, 32, -8), (0, 0, 0)):      # pixel < C, row < W * pixel, frame < H * row
        assert fwd(1, arr(_view(hiplib, strides=st)), None) == bad, st
    assert bwd(1, arr(_view(hiplib, dtype=1)), None) == bad                               # the gradient is f32
    assert bwd(1, arr(_view(hiplib, dtype=2)), None) == bad


def test_roi_pool_views_refuses_a_scale_sequence_of_the_wrong_length():
    import torch
    from mv3d_tf_amd.roi_pooling_layer.roi_pooling_op import _view_scales, roi_pool_views
    views = [(torch.zeros((1, 4, 4, 4)), torch.zeros((1, 5))), (torch.zeros((1, 4, 4, 4)), torch.zeros((1, 5)))]
    for scale in ((0.25,), (0.25, 0.5, 0.5), [], [0.125] * 4):
        with pytest.raises(ValueError, match="one value per view"):
            roi_pool_views(views, 7, 7, scale)
    assert _view_scales(0.125, 3) == (0.125, 0.125, 0.125) and _view_scales([0.5, 0.25], 2) == (0.5, 0.25)
    assert _view_scales(np.float32(0.125), 2) == (0.125, 0.125)


def test_network_constructor_refuses_bad_factors():
    from mv3d_tf_amd.fast_rcnn import config
    from mv3d_tf_amd.networks.mv3d import MV3D
    assert config.cfg.ROI_UPSAMPLE == (1, 1, 1)
    for up in ((1, 1), (1, 1, 1, 1), (3, 1, 1), (1, 8, 1), (0, 1, 1), (2.5, 2, 2), (True, 1, 1), 4, "424"):
        with pytest.raises(ValueError, match="roi_upsample"):
            MV3D(phase="TEST", device="cpu", roi_upsample=up)                             # (raised before any parameter is made)
    saved = config.cfg.ROI_UPSAMPLE
    try:
        config._merge({"ROI_UPSAMPLE": [4, 2, 3]}, config.cfg)                            # a YAML sequence; None = the cfg value
        with pytest.raises(ValueError, match="roi_upsample"):
            MV3D(phase="TEST", device="cpu")
    finally:
        config.cfg.ROI_UPSAMPLE = saved


# ---------------------------------------------------------------------------------------------------- the kernels
@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops
    return torch, ops


SHAPES = ((1, 1), (1, 5), (2, 2), (3, 2), (7, 9), (19, 39))            # (19, 39): several workgroups in both directions, no multiple of one
BATCHES = (1, 3)
CHANNELS = (4, 5, 8, 12, 512)


def _tdtype(torch, kind):
    return {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[kind]


def _to_device(torch, bits, kind, framed=False):
    """raw bits -> device tensor of the type; framed: the interior view of a (B, H + 2, W + 2, C) buffer whose frame is NaN"""
    signed = np.int32 if kind == "f32" else np.int16
    if not framed:
        return torch.from_numpy(bits.view(signed).copy()).cuda().view(_tdtype(torch, kind))
    B, H, W, Cn = bits.shape
    buf = np.full((B, H + 2, W + 2, Cn), 0x7FC00000 if kind == "f32" else (0x7E00 if kind == "f16" else 0x7FC0), ur.BITS[kind])
    buf[:, 1:-1, 1:-1] = bits
    return torch.from_numpy(buf.view(signed)).cuda().view(_tdtype(torch, kind))[:, 1:-1, 1:-1]


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _same(got_bits, want_f32, s=None):
    """raw-bit equality; where the restatement has a NaN that ARITHMETIC made (inf - inf, 0 * inf, a NaN operand of a product) the
    payload is the processor's, so there a NaN is asked for.  s: `want` is an up-map of factor s -- its up-pixels with ONE tap on both
    axes pass a source value through without arithmetic, so there the raw bits must match, a NaN's included"""
    want_bits = want_f32.view(np.uint32)
    loose = np.isnan(want_f32)
    if s is not None:
        one_y = np.array([len(tp) == 1 for tp in ur.taps(want_f32.shape[1] // s, s)])
        one_x = np.array([len(tp) == 1 for tp in ur.taps(want_f32.shape[2] // s, s)])
        loose = loose & ~(one_y[:, None] & one_x[None, :])[None, :, :, None]
    return np.array_equal(np.isnan(got_bits.view(np.float32))[loose], loose[loose]) and np.array_equal(got_bits[~loose], want_bits[~loose])


@gpu
@pytest.mark.parametrize("s", (2, 4))
@pytest.mark.parametrize("kind", ("f32", "f16", "bf16"))
def test_forward_bits_equal_the_restatement(dev, kind, s):
    torch, ops = dev
    rng = np.random.RandomState(10 * ("f32", "f16", "bf16").index(kind) + s)
    for (H, W), B, Cn in itertools.product(SHAPES, BATCHES, CHANNELS):
        bits = ur.from_f32(_rand(rng, (B, H, W, Cn)), kind)
        want = ur.forward(ur.to_f32(bits, kind), s)
        for framed in (False, True):
            x = _to_device(torch, bits, kind, framed)
            y = ops.upsample_bilinear(x, s)
            assert y.dtype == torch.float32 and tuple(y.shape) == (B, s * H, s * W, Cn) and y.is_contiguous()
            assert _same(_bits(y), want, s), (kind, s, H, W, B, Cn, framed)


@gpu
@pytest.mark.parametrize("s", (2, 4))
def test_backward_bits_equal_the_restatement(dev, s):
    torch, ops = dev
    rng = np.random.RandomState(40 + s)
    for (H, W), B, Cn in itertools.product(SHAPES, BATCHES, CHANNELS):
        g = _rand(rng, (B, s * H, s * W, Cn))
        want = ur.backward(g, s, H, W)
        gx = ops.upsample_bilinear_backward_views([(torch.from_numpy(g).cuda(), s)])[0]
        assert gx.dtype == torch.float32 and tuple(gx.shape) == (B, H, W, Cn)
        assert _same(_bits(gx), want), (s, H, W, B, Cn)


@gpu
@pytest.mark.parametrize("s", (2, 4))
@pytest.mark.parametrize("kind", ("f32", "f16", "bf16"))
def test_special_values(dev, kind, s):
    """NaN, +-Inf, -0.0 and subnormals on the dropped taps of aligned up-pixels and on the clamped last row and column"""
    torch, ops = dev
    for Cn in (8, 5):
        xb32 = _special_map(4, 5, Cn, 3)
        if kind == "f32":
            bits = xb32
        else:                                            # the same pattern in the type's own specials
            sp = {"f16": (0x7E00, 0x7C00, 0xFC00, 0x8000, 0x0001, 0x83FF), "bf16": (0x7FC0, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x807F)}[kind]
            bits = ur.from_f32(xb32.view(np.float32), kind)
            for k, v in enumerate(SPECIALS):
                bits[xb32 == v] = sp[k]
        src = ur.to_f32(bits, kind)
        for framed in (False, True):
            y = _bits(ops.upsample_bilinear(_to_device(torch, bits, kind, framed), s))
            _aligned_and_clamped_bits_hold(y, src.view(np.uint32), s)
            assert _same(y, ur.forward(src, s), s)
    # backward: specials in the gradient
    g = np.tile(_special_map(4, 5, 4, 5), (1, s, s, 1)).view(np.float32)
    gx = ops.upsample_bilinear_backward_views([(torch.from_numpy(g.copy()).cuda(), s)])[0]
    assert _same(_bits(gx), ur.backward(g, s, 4, 5))


@gpu
def test_grouped_launch_equals_the_single_view_calls(dev):
    torch, ops = dev
    rng = np.random.RandomState(8)
    spec = [((2, 5, 7, 8), "f16", 4), ((1, 3, 4, 12), "f32", 2), ((0, 4, 4, 8), "f32", 2), ((3, 2, 2, 5), "bf16", 4)]
    xs = [_to_device(torch, ur.from_f32(_rand(rng, sh), kind), kind, framed=(k == 0)) for k, (sh, kind, _) in enumerate(spec)]
    got = ops.upsample_bilinear_views([(x, s) for x, (_, _, s) in zip(xs, spec)])
    for x, y, (sh, kind, s) in zip(xs, got, spec):
        assert tuple(y.shape) == (sh[0], s * sh[1], s * sh[2], sh[3])
        if sh[0]:
            assert torch.equal(y, ops.upsample_bilinear(x, s))
            assert _same(_bits(y), ur.forward(ur.to_f32(_bits_of_input(x, kind), kind), s), s)
    gs = [torch.from_numpy(_rand(rng, tuple(y.shape))).cuda() for y in got]
    gxs = ops.upsample_bilinear_backward_views([(g, s) for g, (_, _, s) in zip(gs, spec)])
    for g, gx, (sh, _, s) in zip(gs, gxs, spec):
        assert tuple(gx.shape) == sh
        if sh[0]:
            assert torch.equal(gx, ops.upsample_bilinear_backward_views([(g, s)])[0])


def _bits_of_input(x, kind):
    import torch
    a = x.contiguous().cpu()
    return a.numpy().view(np.uint32) if kind == "f32" else a.view(torch.int16).numpy().view(np.uint16)


@gpu
def test_launch_hygiene(dev):
    """two launches on the same inputs give identical bits; a pre-filled g_x (and y) is fully overwritten"""
    torch, ops = dev
    rng = np.random.RandomState(9)
    for Cn, s in ((8, 2), (5, 4), (512, 4)):
        x = torch.from_numpy(_rand(rng, (2, 7, 9, Cn))).cuda()
        g = torch.from_numpy(_rand(rng, (2, 7 * s, 9 * s, Cn))).cuda()
        y1, y2 = ops.upsample_bilinear(x, s), torch.full((2, 7 * s, 9 * s, Cn), float("nan"), device="cuda")
        ops.upsample_bilinear_views([(x, s)], outs=[y2])
        assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))
        g1 = ops.upsample_bilinear_backward_views([(g, s)])[0]
        for fill in (float("nan"), 1e30):
            g2 = torch.full((2, 7, 9, Cn), fill, device="cuda")
            ops.upsample_bilinear_backward_views([(g, s)], outs=[g2])
            assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))


@gpu
def test_autograd_gradient_equals_the_restated_backward(dev):
    torch, ops = dev
    rng = np.random.RandomState(11)
    x0 = torch.from_numpy(_rand(rng, (2, 3, 5, 8))).cuda().requires_grad_(True)
    x1 = torch.from_numpy(_rand(rng, (1, 4, 2, 5))).cuda().requires_grad_(True)
    x2 = torch.from_numpy(_rand(rng, (1, 2, 2, 4))).cuda().requires_grad_(True)           # its output stays out of the loss
    w0, w1 = _rand(rng, (2, 12, 20, 8)), _rand(rng, (1, 8, 4, 5))
    y0, y1, y2 = ops.UpsampleBilinearViews.apply((4, 2, 2), x0, x1, x2)
    assert _same(_bits(y0), ur.forward(x0.detach().cpu().numpy(), 4), 4) and _same(_bits(y1), ur.forward(x1.detach().cpu().numpy(), 2), 2)
    g0, g1, g2 = torch.autograd.grad([y0, y1], [x0, x1, x2], [torch.from_numpy(w0).cuda(), torch.from_numpy(w1).cuda()], allow_unused=True)
    assert g0.dtype == torch.float32 and _same(_bits(g0), ur.backward(w0, 4, 3, 5))
    assert _same(_bits(g1), ur.backward(w1, 2, 4, 2))
    assert g2 is None or not g2.any()


@gpu
def test_roi_pool_views_per_view_scale_and_a_map_beyond_the_pair_kernels(dev):
    """roi_pool_views with one scale per view equals the single-view op at that scale, forward and gradient -- also when a view has more
    than 65 534 pixels (a 4x upsampled 608 x 608 bird's-eye view has 92 416): every view then leaves the pair's own kernels for the plain
    forward and the index + gather backward, which needs the workspace the autograd function now brings"""
    torch, ops = dev
    from mv3d_tf_amd.roi_pooling_layer.roi_pooling_op import roi_pool_views
    gen = torch.Generator(device="cuda").manual_seed(5)
    for shapes in (((2, 9, 11, 256), (1, 14, 6, 256)), ((1, 2, 32768, 256), (1, 14, 6, 256))):
        scales = (0.5, 0.25)
        datas = [torch.randn(sh, device="cuda", generator=gen).requires_grad_(True) for sh in shapes]
        rois = []
        for sh, sc in zip(shapes, scales):
            r = torch.rand((6, 5), device="cuda", generator=gen)
            x1, y1 = r[:, 1] * (sh[2] - 2) / sc, r[:, 2] * (sh[1] - 2) / sc
            rois.append(torch.stack([torch.floor(r[:, 0] * sh[0]), x1, y1, x1 + r[:, 3] * 12 / sc, y1 + r[:, 4] * 6 / sc], 1).contiguous())
        tops = roi_pool_views(list(zip(datas, rois)), 7, 7, scales)
        ws = [torch.randn(tuple(t.shape), device="cuda", generator=gen) for t in tops]
        grads = torch.autograd.grad(tops, datas, ws)
        for d, r, sc, t, w, g in zip(datas, rois, scales, tops, ws, grads):
            top, argmax = ops.roi_pool_forward(d.detach(), r, 7, 7, sc)
            assert torch.equal(t.detach(), top)
            assert torch.equal(g, ops.roi_pool_backward(w, r, argmax, tuple(d.shape), 7, 7, sc)) and float(g.abs().sum()) > 0
        with torch.no_grad():
            for t, t2 in zip(tops, roi_pool_views(list(zip(datas, rois)), 7, 7, list(scales))):
                assert torch.equal(t.detach(), t2)


# ---------------------------------------------------------------------------------------------------- the graphs
def _net(torch, name, up, amp_dtype=None, mfma_trunk=False):
    """a network of the test's own (nothing outlives the test that built it); the RPN scores spread a little (random init is flat)"""
    from mv3d_tf_amd.networks import get_network
    net = get_network(name, **({} if up is None else {"roi_upsample": up}))
    with torch.no_grad():
        net.params["rpn_cls_score"][0].mul_(40.0)
        net.params["rpn_bbox_pred"][0].mul_(5.0)
    net.amp_dtype, net.mfma_trunk = amp_dtype, mfma_trunk
    return net


def _test_feed(torch, seed, B=1, side=256):
    from mv3d_tf_amd import synth
    rng = np.random.RandomState(seed)
    return {"lidar_bv_data": torch.as_tensor(((rng.random_sample((B, side, side, 9)) < 0.03) * rng.uniform(0, 2.4, (B, side, side, 9))).astype(np.float32)).cuda(),
            "image_data": torch.as_tensor(rng.uniform(-100, 100, (B, 96, 320, 3)).astype(np.float32)).cuda(),
            "lidar_fv_data": torch.as_tensor(rng.uniform(0, 1, (B, 64, 512, 3)).astype(np.float32)).cuda(),
            "im_info": np.array([[side, side, 1]] * B, np.float32), "calib": np.stack([synth.KITTI_CALIB] * B), "keep_prob": 1.0}


class _TestCfg:
    """a handful of ROIs per frame"""

    def __enter__(self):
        from mv3d_tf_amd.fast_rcnn.config import cfg
        self.cfg, self.saved = cfg, dict(cfg.TEST)
        cfg.TEST.update(RPN_PRE_NMS_TOP_N=600, RPN_POST_NMS_TOP_N=12)

    def __exit__(self, *exc):
        self.cfg.TEST.update(self.saved)


def _check_test_graph(torch, ops, net, L, factors):
    keys = ("conv5_3", "conv5_3_2", "conv5_3_3")[:net.views]
    rois = (L["roi_data_bv"], L["roi_data_img"], L.get("roi_data_fv"))
    for k, key in enumerate(keys):
        s = factors[k]
        assert L[key].dtype == torch.float32 and (key + "_up" in L) == (s > 1)
        src = L[key]
        if s > 1:
            up = L[key + "_up"]
            assert tuple(up.shape) == (src.shape[0], s * src.shape[1], s * src.shape[2], src.shape[3])
            assert _same(_bits(up), ur.forward(src.contiguous().cpu().numpy(), s), s), key
            src = up
        assert rois[k].shape[0] > 0
        want = ops.roi_pool_forward(src.contiguous(), rois[k].contiguous(), 7, 7, s / 8, want_argmax=False)[0]
        pool = L["pool_5" + ("", "_2", "_3")[k]]
        assert torch.equal(pool, want.to(pool.dtype)), key


@gpu
def test_test_graph_two_views_2x(dev):
    torch, ops = dev
    with _TestCfg(), torch.no_grad():
        net = _net(torch, "MV3D_test", (2, 2, 2))
        assert net.roi_upsample == (2, 2, 2)
        L = net.forward(_test_feed(torch, 1))
        assert "conv5_3_3_up" not in L
        _check_test_graph(torch, ops, net, L, (2, 2, 2))
        assert torch.isfinite(L["cls_prob"]).all()


@gpu
def test_test_graph_three_views_paper_setting_on_the_serving_trunk(dev):
    """(4, 2, 4) on the 16-bit MFMA trunks: the BEV map is read out of its framed f16 buffer through strides"""
    torch, ops = dev
    with _TestCfg(), torch.no_grad():
        net = _net(torch, "MV3D_test_3view", (4, 2, 4), amp_dtype=torch.float16, mfma_trunk=True)
        L = net.forward(_test_feed(torch, 2))
        assert net._bev_interior is not None and net._bev_interior.dtype == torch.float16 and not net._bev_interior.is_contiguous()
        _check_test_graph(torch, ops, net, L, (4, 2, 4))
        assert L["pool_5"].dtype == torch.float16


@gpu
def test_factors_of_one_change_nothing(dev):
    torch, ops = dev
    with _TestCfg(), torch.no_grad():
        feed = _test_feed(torch, 3)
        got = []
        for up in (None, (1, 1, 1)):
            net = _net(torch, "MV3D_test", up, amp_dtype=torch.float16, mfma_trunk=True)     # (torch's f32 convolutions are not bit-reproducible)
            assert net.roi_upsample == (1, 1, 1)
            L = net.forward(feed)
            assert not [k for k in L if k.endswith("_up")]
            got.append((L["pool_5"].clone(), L["pool_5_2"].clone(), L["cls_prob"].clone()))
        for a, b in zip(*got):
            assert torch.equal(a, b)


@gpu
def test_captured_serving_step_replays_the_eager_pool_bits(dev):
    torch, ops = dev
    from mv3d_tf_amd.fast_rcnn import test_mv
    with _TestCfg(), torch.no_grad():
        net = _net(torch, "MV3D_test", (2, 2, 2), amp_dtype=torch.float16, mfma_trunk=True)
        feeds = {1: _test_feed(torch, 4, B=2), 2: _test_feed(torch, 5, B=2)}
        sg = test_mv.ServeGraph(net, feeds[1])
        static = {k: net.layers[k] for k in ("pool_5", "pool_5_2", "conv5_3_up")}            # the graph's static tensors
        for seed in (2, 1):
            sg.replay(feeds[seed])
            sg.stream.synchronize()
            got = {k: v.clone() for k, v in static.items()}
            net.fixed_rois = True
            try:
                L = net.forward(feeds[seed])
            finally:
                net.fixed_rois = False
            for k in got:
                assert torch.equal(got[k], L[k]), k
            assert got["pool_5"].shape[0] == 2 * 12
        del sg


@gpu
def test_train_graph_gradient_flows_through_the_upsampling(dev):
    """the gradient reaching conv5_3* = the restated upsampling backward of the RoiPool gradient of the up-map (taken from ops)"""
    torch, ops = dev
    from mv3d_tf_amd import synth
    from mv3d_tf_amd.fast_rcnn.train_mv import stack_blobs
    rng = np.random.RandomState(1)
    _, _, info, calib, (gt_bv, gt_3d, gt_cnr) = synth.rpn_head(55, 76, 76, "peaky", return_gt=True)
    feed = stack_blobs([{"lidar_bv_data": (rng.random_sample((1, 608, 608, 9)) < 0.02).astype(np.float32),
                         "image_data": rng.uniform(-100, 100, (1, 375, 1242, 3)).astype(np.float32),      # (the size the ROIs are projected into)
                         "im_info": info, "calib": calib, "gt_boxes_bv": gt_bv, "gt_boxes_3d": gt_3d, "gt_boxes_corners": gt_cnr}])
    feed["keep_prob"] = 0.5
    net = _net(torch, "MV3D_train", (2, 2, 2), amp_dtype=torch.bfloat16, mfma_trunk=True)      # the bf16 training trunks
    np.random.seed(3)
    L = net.forward(feed)
    keys = ("conv5_3", "conv5_3_2")
    for key in keys:
        assert L[key].requires_grad and L[key + "_up"].requires_grad
        L[key].retain_grad()
    pools = (L["pool_5"], L["pool_5_2"])
    ws = [torch.from_numpy(_rand(rng, tuple(p.shape))).cuda() for p in pools]
    torch.autograd.backward(list(pools), ws)
    for k, key in enumerate(keys):
        up, rois = L[key + "_up"].detach(), (L["roi_data_bv"], L["roi_data_img"])[k].contiguous()
        assert _same(_bits(up), ur.forward(L[key].detach().contiguous().cpu().numpy(), 2), 2)
        top, argmax = ops.roi_pool_forward(up, rois, 7, 7, 2 / 8)
        assert torch.equal(top, pools[k].detach())
        g_up = ops.roi_pool_backward(ws[k], rois, argmax, tuple(up.shape), 7, 7, 2 / 8)
        H, W = L[key].shape[1:3]
        assert _same(_bits(L[key].grad), ur.backward(g_up.cpu().numpy(), 2, H, W)), key
        assert float(L[key].grad.abs().sum()) > 0
