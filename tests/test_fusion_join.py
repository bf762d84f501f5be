"""The deep-fusion join kernel (csrc/fusion_join.hip): forward and backward against the numpy restatement
(tests/fusion_join_restatement.py) bit for bit, the autograd wrapper against torch autograd, and the argument rules."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fusion_join_restatement as fj

gpu = pytest.mark.gpu

ROWS = (0, 1, 5, 128)
CHANNELS = (1, 7, 8, 20, 2048)       # a row shorter than one vector, odd, one 16-bit vector, body + tail, the head's width
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -1e-40, 6e-8, -6e-8, 1.0, -1.0], np.float32)   # 1e-40: f32 / bf16 subnormal, 6e-8: f16's


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops
    return torch, ops


_TORCH = {"f32": "float32", "f16": "float16", "bf16": "bfloat16"}


def up(torch, bits, kind):
    """raw bits -> device tensor of the kind"""
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int32 if kind == "f32" else np.int16)).cuda()
    return t.view(getattr(torch, _TORCH[kind]))


def down(torch, t, kind):
    return t.view(torch.int32 if kind == "f32" else torch.int16).cpu().numpy().view(fj.BITS[kind])


def keep_tables(V):
    """every non-empty keep pattern of V views as a single path, and as rows of P = 4 tables (all patterns appear in some table)"""
    pats = [p for p in itertools.product((0, 1), repeat=V) if any(p)]
    tables = [[p] for p in pats]
    for i in range(0, len(pats), 3):                                  # rows of the P = 4 tables: the patterns taken round and round
        tables.append([pats[(i + k) % len(pats)] for k in range(4)])
    if V == 3:                                                        # the head's table: the main network and the auxiliary paths
        tables.append([(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)])
    return [np.array(t, np.uint8) for t in tables]


def values(rng, shape, kind):
    """random values, a sixth of the elements (at least one) replaced by special inputs at random places, as bits"""
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    if flat.size:
        idx = rng.choice(flat.size, size=max(1, flat.size // 6), replace=False)
        flat[idx] = SPECIALS[rng.randint(0, len(SPECIALS), idx.size)]
    return fj.from_f32(x, kind)


def test_keep_tables_cover_every_pattern():
    for V in (1, 2, 3):
        tabs = keep_tables(V)
        single = {tuple(t[0]) for t in tabs if len(t) == 1}
        multi = {tuple(r) for t in tabs if len(t) == 4 for r in t}
        assert len(single) == 2 ** V - 1 and single <= multi


def test_restatement_rounding_and_specials():
    """the checker's own conversions: ties to even, canonical NaN, the sign of zero through the sum"""
    assert fj.from_f32(np.array([1.00390625, 1.01171875, np.nan, np.inf], np.float32), "bf16").tolist() == [0x3F80, 0x3F82, 0x7FC0, 0x7F80]
    assert fj.from_f32(np.array([np.nan, -np.nan], np.float32), "f16").tolist() == [0x7E00, 0x7E00]
    h = fj.from_f32(np.array([-0.0, -1.0, np.nan, 2.0], np.float32), "f32").reshape(1, 1, 1, 4)
    out = fj.to_f32(fj.join_forward(h, [[1]], "f32"), "f32").reshape(-1)
    assert out[0] == 0 and not np.signbit(out[0]) and out[1] == 0 and np.isnan(out[2]) and out[3] == 2.0
    g = fj.join_backward(h, fj.from_f32(np.ones((1, 1, 4), np.float32), "f32"), [[1]], "f32")
    assert fj.to_f32(g, "f32").reshape(-1).tolist() == [0.0, 0.0, 0.0, 1.0]         # zero gradient at x == 0, through a NaN


@gpu
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("kind", fj.KINDS)
def test_join_equals_the_restatement_bit_for_bit(dev, kind, rows):
    """forward and backward, every channel count x view count x keep table x sets_in x with / without a mask, special values in h and
    g_out: np.array_equal on the raw bits"""
    torch, ops = dev
    rng = np.random.RandomState(1000 + 10 * fj.KINDS.index(kind) + ROWS.index(rows))
    cases = 0
    for Cn, V in itertools.product(CHANNELS, (1, 2, 3)):
        for keep in keep_tables(V):
            P = len(keep)
            for S, masked in itertools.product(sorted({1, P}), (False, True)):
                h = values(rng, (S, V, rows, Cn), kind)
                g_out = values(rng, (P, rows, Cn), kind)
                drop = (rng.random_sample((P, rows, Cn)) < 0.5).astype(np.uint8) if masked else None
                scale = 2.0 if masked else 1.0
                d_dev = torch.from_numpy(drop).cuda() if masked else None
                h_dev = up(torch, h, kind)
                out = ops.fusion_join(h_dev, keep, d_dev, scale)
                g_h = ops.fusion_join_backward(h_dev, up(torch, g_out, kind), keep, d_dev, scale)
                assert out.shape == (P, rows, Cn) and g_h.shape == h_dev.shape and out.dtype == h_dev.dtype
                what = (kind, rows, Cn, V, keep.tolist(), S, masked)
                assert np.array_equal(down(torch, out, kind), fj.join_forward(h, keep, kind, drop, scale)), what
                assert np.array_equal(down(torch, g_h, kind), fj.join_backward(h, g_out, keep, kind, drop, scale)), what
                cases += 1
    assert cases > 100


@gpu
@pytest.mark.parametrize("kind", fj.KINDS)
def test_dropped_views_are_never_read(dev, kind):
    """NaN in every view a path drops: the outputs and the gradients of the kept views stay finite, the dropped views' gradients are 0"""
    torch, ops = dev
    rng = np.random.RandomState(7)
    R, Cn, V = 5, 20, 3
    for keep in ([[1, 0, 0]], [[0, 1, 1]], [[0, 0, 1], [1, 0, 1], [0, 0, 1], [1, 0, 0]]):
        keep = np.array(keep, np.uint8)
        P = len(keep)
        for S in sorted({1, P}):
            x = rng.standard_normal((S, V, R, Cn)).astype(np.float32)
            for s in range(S):
                for v in range(V):
                    if not (keep[:, v].any() if S == 1 else keep[s, v]):
                        x[s, v] = np.nan
            h = fj.from_f32(x, kind)
            g = fj.from_f32(rng.standard_normal((P, R, Cn)).astype(np.float32), kind)
            out = fj.to_f32(down(torch, ops.fusion_join(up(torch, h, kind), keep), kind), kind)
            g_h = fj.to_f32(down(torch, ops.fusion_join_backward(up(torch, h, kind), up(torch, g, kind), keep), kind), kind)
            assert np.isfinite(out).all() and np.isfinite(g_h).all(), (keep.tolist(), S)
            for s in range(S):
                for v in range(V):
                    if not (keep[:, v].any() if S == 1 else keep[s, v]):
                        assert not g_h[s, v].any()


@gpu
def test_backward_adds_the_paths_in_ascending_order(dev):
    """sets_in == 1: four paths whose terms are 1e8, 1, -1e8, 1 -- ((1e8 + 1) - 1e8) + 1 = 1 in f32, any other order gives 0 or 2"""
    torch, ops = dev
    keep = np.ones((4, 1), np.uint8)
    h = fj.from_f32(np.ones((1, 1, 3, 7), np.float32), "f32")
    g = np.empty((4, 3, 7), np.float32)
    g[0], g[1], g[2], g[3] = 1e8, 1.0, -1e8, 1.0
    got = down(torch, ops.fusion_join_backward(up(torch, h, "f32"), up(torch, fj.from_f32(g, "f32"), "f32"), keep), "f32")
    assert np.array_equal(got, fj.join_backward(h, fj.from_f32(g, "f32"), keep, "f32"))
    assert (fj.to_f32(got, "f32") == 1.0).all()
    # ... and the same bits when run again (no atomics)
    again = down(torch, ops.fusion_join_backward(up(torch, h, "f32"), up(torch, fj.from_f32(g, "f32"), "f32"), keep), "f32")
    assert np.array_equal(got, again)


@gpu
def test_offsets_beyond_2_to_the_31(dev):
    """64-bit element offsets: three f16 views of 2^30 + 8 elements each, only the last one kept -- it starts past element 2^31.
    Checked on the device against the same expression in torch ops (the restatement on the host would take minutes); the two
    dropped views are left as allocated, they are never read."""
    torch, ops = dev
    E = (1 << 30) + 8
    R, Cn = E // 8, 8
    h = torch.empty((1, 3, R, Cn), dtype=torch.float16, device="cuda")
    keep = np.array([[0, 0, 1]], np.uint8)
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = h[0, 2].normal_(generator=gen)
    out = ops.fusion_join(h, keep)
    assert torch.equal(out[0], torch.where(x < 0, torch.zeros_like(x), x) + 0.0)
    g_h = ops.fusion_join_backward(h, out, keep)                        # (the output doubles as the incoming gradient)
    assert torch.equal(g_h[0, 2], torch.where(x > 0, out[0], torch.zeros_like(x)))
    assert not g_h[0, 0].any() and not g_h[0, 1].any()


def _entries():
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import _lib
    return _lib, _lib.lib()


def _bad_calls(keep_ok, keep_empty_path):
    """(name, dtype, sets_in, paths, views, rows, channels, keep) that the entries must refuse"""
    return [("dtype", 3, 1, 1, 3, 4, 8, keep_ok), ("dtype", -1, 1, 1, 3, 4, 8, keep_ok), ("views 0", 0, 1, 1, 0, 4, 8, keep_ok),
            ("views 5", 0, 1, 1, 5, 4, 8, keep_ok), ("paths 0", 0, 1, 0, 3, 4, 8, keep_ok), ("paths 9", 0, 1, 9, 3, 4, 8, keep_ok),
            ("sets_in", 0, 2, 4, 3, 4, 8, keep_ok), ("sets_in 0", 0, 0, 4, 3, 4, 8, keep_ok), ("rows < 0", 0, 1, 1, 3, -1, 8, keep_ok),
            ("channels 0", 0, 1, 1, 3, 4, 0, keep_ok), ("channels < 0", 0, 1, 1, 3, 4, -8, keep_ok), ("keep NULL", 0, 1, 1, 3, 4, 8, None),
            ("a path without a view", 0, 1, 2, 3, 4, 8, keep_empty_path)]


def test_invalid_arguments_are_refused_on_the_host():
    """no device needed: the argument rules are checked before any HIP call (the "pointers" are never dereferenced)"""
    _lib, L = _entries()
    A = C.c_void_p(4096)
    ok = (C.c_uint8 * 32)(*([1] * 32))
    empty = (C.c_uint8 * 32)(*([1, 1, 1, 0, 0, 0] + [1] * 26))
    for name, dt, S, P, V, R, Cn, keep in _bad_calls(ok, empty):
        assert L.mv3d_fusion_join_forward(A, dt, S, P, V, R, Cn, keep, None, 1.0, A, None) == _lib.ERR_INVALID_ARG, name
        assert L.mv3d_fusion_join_backward(A, A, dt, S, P, V, R, Cn, keep, None, 1.0, A, None) == _lib.ERR_INVALID_ARG, name
    assert L.mv3d_fusion_join_forward(None, 0, 1, 1, 3, 4, 8, ok, None, 1.0, A, None) == _lib.ERR_INVALID_ARG
    assert L.mv3d_fusion_join_forward(A, 0, 1, 1, 3, 4, 8, ok, None, 1.0, None, None) == _lib.ERR_INVALID_ARG
    assert L.mv3d_fusion_join_backward(A, None, 0, 1, 1, 3, 4, 8, ok, None, 1.0, A, None) == _lib.ERR_INVALID_ARG
    assert L.mv3d_fusion_join_backward(A, A, 0, 1, 1, 3, 4, 8, ok, None, 1.0, None, None) == _lib.ERR_INVALID_ARG
    # rows == 0 launches nothing and needs no buffers
    assert L.mv3d_fusion_join_forward(None, 0, 1, 1, 3, 0, 8, ok, None, 1.0, None, None) == _lib.OK
    assert L.mv3d_fusion_join_backward(None, None, 0, 1, 1, 3, 0, 8, ok, None, 1.0, None, None) == _lib.OK


def test_python_wrappers_take_device_tensors_only():
    import torch
    from mv3d_tf_amd import ops
    with pytest.raises(TypeError):
        ops.fusion_join(torch.zeros(1, 3, 4, 8), [[1, 1, 1]])            # a CPU tensor: there is no CPU path
    with pytest.raises(TypeError):
        ops.fusion_join(np.zeros((1, 3, 4, 8), np.float32), [[1, 1, 1]])


@gpu
def test_invalid_arguments_write_nothing(dev):
    torch, ops = dev
    _lib, L = _entries()
    h = torch.randn(4, 3, 4, 8, device="cuda")
    out = torch.full((4, 4, 8), 7.0, device="cuda")
    g_h = torch.full((4, 3, 4, 8), 7.0, device="cuda")
    ok = (C.c_uint8 * 32)(*([1] * 32))
    empty = (C.c_uint8 * 32)(*([1, 1, 1, 0, 0, 0] + [1] * 26))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    for name, dt, S, P, V, R, Cn, keep in _bad_calls(ok, empty):
        assert L.mv3d_fusion_join_forward(p(h), dt, S, P, V, R, Cn, keep, None, 1.0, p(out), st) == _lib.ERR_INVALID_ARG, name
        assert L.mv3d_fusion_join_backward(p(h), p(out), dt, S, P, V, R, Cn, keep, None, 1.0, p(g_h), st) == _lib.ERR_INVALID_ARG, name
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (g_h == 7.0).all()
    with pytest.raises(_lib.Mv3dError):
        ops.fusion_join(h, [[0, 0, 0]] * 4)
    with pytest.raises(ValueError):
        ops.fusion_join(h, [[1, 1]] * 4)                                 # keep rows of the wrong width
    with pytest.raises(ValueError):
        ops.fusion_join(h.transpose(2, 3), [[1, 1, 1]] * 4)              # not contiguous


@gpu
def test_autograd_function_equals_torch_autograd(dev):
    """ops.FusionJoin in f32 against relu -> masked mean over the kept views -> dropout written in torch ops, outputs and gradients.
    Every output is at most V + 2 roundings of non-negative terms from the exact value in both, hence 8 ulp apart at most; a gradient
    is a sum of P terms of either sign, bounded by 8 ulp of the sum of their magnitudes."""
    torch, ops = dev
    torch.manual_seed(0)
    eps = 2.0 ** -23
    for (S, P, V, R, Cn), masked in itertools.product(((1, 1, 3, 5, 20), (1, 4, 3, 5, 20), (4, 4, 3, 7, 8), (1, 2, 2, 128, 7)), (False, True)):
        keep = np.array(([[1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1]] if V == 3 else [[1, 1], [0, 1]])[:P], np.uint8)
        h = torch.randn(S, V, R, Cn, device="cuda", requires_grad=True)
        drop = (torch.rand(P, R, Cn, device="cuda") < 0.5).to(torch.uint8) if masked else None
        scale = 2.0 if masked else 1.0
        w = torch.randn(P, R, Cn, device="cuda")
        out = ops.FusionJoin.apply(h, keep, drop, scale)
        (out * w).sum().backward()
        got_g, h.grad = h.grad.clone(), None
        k = torch.as_tensor(keep, dtype=torch.float32, device="cuda")
        a = torch.relu(h).expand(P, V, R, Cn) * k[:, :, None, None]
        want = a.sum(1) / k.sum(1)[:, None, None]
        if masked:
            want = want * drop.float() * scale
        (want * w).sum().backward()
        assert torch.allclose(out, want, rtol=8 * eps, atol=0), (S, P, masked)
        bound = 8 * eps * (w.abs() * scale).sum(0).max().item()
        assert (got_g - h.grad).abs().max().item() <= bound, (S, P, masked)
        assert torch.equal(got_g == 0, h.grad == 0)
