"""Float64 references of the trunks' operations on framed NHWC maps, shared by tests/test_conv_paths.py (one kernel at a time) and
tests/test_trunk_train_chain.py (the links of a training step).  Plain torch in float64 on whatever device the operands live on
(rocBLAS dgemm on the GPU, not MIOpen; the CPU for the references' own checks): nothing here calls the library under test.

A framed map is (B, H + 2, W + 2, C) with a zero one-pixel frame: the SAME padding of a 3x3 convolution."""
import torch as _torch


def _chunk(B, per_frame_elems, budget=2 ** 26):
    return max(1, min(B, budget // max(1, per_frame_elems)))


def _conv_ref(torch, xp, w, b, relu=False, gate=None, pool=False, absval=False):
    """xp (B, H + 2, W + 2, Cin) framed f64 map, w (Cout, Cin, 3, 3) f64, b (Cout) f64 -> yields (b0, y) chunks of the float64
    result (nb, H, W, Cout) [gated by gate > 0, ReLU, 2x2 VALID max pool]: nine shifted GEMMs per chunk of frames"""
    B, Hp, Wp, cin = xp.shape
    H, W, cout = Hp - 2, Wp - 2, w.shape[0]
    if absval:
        xp, w, b = xp.abs(), w.abs(), b.abs()
    step = _chunk(B, H * W * max(cin, cout))
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        y = b.expand(nb * H * W, cout).clone()
        for ty in range(3):
            for tx in range(3):
                y.addmm_(xp[b0:b0 + nb, ty:ty + H, tx:tx + W].reshape(nb * H * W, cin), w[:, :, ty, tx].t())
        y = y.view(nb, H, W, cout)
        if gate is not None:
            y = torch.where(gate[b0:b0 + nb, 1:-1, 1:-1] > 0, y, torch.zeros_like(y))
        if relu:
            y = torch.relu(y)
        if pool:
            y = torch.nn.functional.max_pool2d(y.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
        yield b0, y


def _wgrad_ref(torch, xp, dyp, absval=False):
    """float64 dW (Cout, Cin, 3, 3) = sum over pixels of dy x x_shift(tap), db = sum dy"""
    B, Hp, Wp, cin = xp.shape
    H, W, cout = Hp - 2, Wp - 2, dyp.shape[3]
    if absval:
        xp, dyp = xp.abs(), dyp.abs()
    dw = torch.zeros((cout, cin, 3, 3), dtype=torch.float64, device=xp.device)
    step = _chunk(B, H * W * max(cin, cout))
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        d = dyp[b0:b0 + nb, 1:-1, 1:-1].reshape(nb * H * W, cout)
        for ty in range(3):
            for tx in range(3):
                dw[:, :, ty, tx] += d.t() @ xp[b0:b0 + nb, ty:ty + H, tx:tx + W].reshape(nb * H * W, cin)
    return dw, dyp.sum((0, 1, 2))


def _bound_check(torch, got, ref, S, L, out_dt, what):
    """|got - ref| <= 2^-p |ref| + 1.01 L 2^-24 S per element: one rounding of the result to the output type (p = 11 for f16, 8 for
    bf16, no term for f32) plus an f32 sum of L terms in any order (S = the same sum over absolute values)"""
    p = {"f16": 11, "bf16": 8}.get(out_dt)
    bound = 1.01 * L * 2.0 ** -24 * S
    if p is not None:
        bound = bound + 2.0 ** -p * ref.abs()
    err = (got.double() - ref).abs()
    ok = err <= bound
    if not bool(ok.all()):
        i = tuple((~ok).nonzero()[0].tolist())
        raise AssertionError("%s: %d elements beyond the bound, first at %s: got %r, float64 %r, bound %r" % (
            what, int((~ok).sum()), i, float(got[i]), float(ref[i]), float(bound[i])))


# ------------------------------------------------------------------------------- the links of a training step (whole maps, any device)
def frame(x, channels=None, dtype=None):
    """(B, H, W, c) -> framed (B, H + 2, W + 2, channels >= c): the interior's first c channels hold x, everything else is 0"""
    B, H, W, c = x.shape
    out = _torch.zeros((B, H + 2, W + 2, channels or c), dtype=dtype or x.dtype, device=x.device)
    out[:, 1:-1, 1:-1, :c] = x
    return out


def conv(xp, w, b, relu=False, gate=None, absval=False):
    """_conv_ref as one (B, H, W, Cout) float64 map"""
    return _torch.cat([y for _, y in _conv_ref(_torch, xp, w, b, relu=relu, gate=gate, absval=absval)])


def dgrad_filter(w):
    """(Cout, Cin, 3, 3) -> (Cin, Cout, 3, 3): the filter whose SAME convolution over dY is the data gradient of the SAME convolution
    with w -- turned by 180 degrees, channel axes swapped"""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def _windows(yp):
    """the four positions of every 2x2 VALID window of a framed map's interior, row-major: [(dy, dx, (B, Ho, Wo, C) view)]"""
    H, W = yp.shape[1] - 2, yp.shape[2] - 2
    Ho, Wo = H // 2, W // 2
    return [(dy, dx, yp[:, 1 + dy:1 + dy + 2 * Ho:2, 1 + dx:1 + dx + 2 * Wo:2]) for dy in (0, 1) for dx in (0, 1)]


def pool(yp):
    """framed map -> its 2x2 / stride 2 VALID max pool, framed, in the map's own type (a maximum rounds nothing)"""
    a = _windows(yp)
    m = _torch.maximum(_torch.maximum(a[0][2], a[1][2]), _torch.maximum(a[2][2], a[3][2]))
    return frame(m)


def pool_grad(yp, gp):
    """yp: framed pre-pool map (a ReLU output), gp: framed gradient w.r.t. its pooled map -> the framed gradient w.r.t. yp's
    pre-activation, in gp's type: the FIRST maximum of each window in row-major order gets the pooled gradient if that maximum
    is > 0, every other element -- the rest of the window, the row / column an odd size drops, the frame -- is 0"""
    a = _windows(yp)
    m = _torch.maximum(_torch.maximum(a[0][2], a[1][2]), _torch.maximum(a[2][2], a[3][2]))
    g = gp[:, 1:-1, 1:-1]
    out = _torch.zeros(yp.shape, dtype=gp.dtype, device=yp.device)
    taken = _torch.zeros(m.shape, dtype=_torch.bool, device=yp.device)
    H, W = yp.shape[1] - 2, yp.shape[2] - 2
    for dy, dx, v in a:
        first = (v == m) & ~taken
        taken = taken | first
        out[:, 1 + dy:1 + dy + 2 * (H // 2):2, 1 + dx:1 + dx + 2 * (W // 2):2] = _torch.where(first & (m > 0), g, _torch.zeros_like(g))
    return out
