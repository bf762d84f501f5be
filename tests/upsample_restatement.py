"""The bilinear upsampling in front of RoiPool (include/mv3d_hip.h) restated in numpy, f32 arithmetic exactly
as the contract states it.  Written from the statement of the operation, not from the kernel.  Not a test module: the checker of
tests/test_upsample.py, never the thing under test.

The rule (TensorFlow 1's resize_bilinear, align_corners=False): up-pixel o sits at source coordinate o / s.  Per axis, up-index o has
the taps i0 = o // s with weight (s - o % s) / s and i1 = min(i0 + 1, n - 1) with weight (o % s) / s; a tap of weight 0 is dropped and
two taps on one source index merge into one tap of weight 1."""
import numpy as np

BITS = {"f32": np.uint32, "f16": np.uint16, "bf16": np.uint16}


def to_f32(bits, kind):
    """raw bits (uint32 for f32, uint16 for f16 / bf16) -> float32 values (exact)"""
    bits = np.ascontiguousarray(bits, BITS[kind])
    if kind == "f32":
        return bits.view(np.float32)
    if kind == "f16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def from_f32(x, kind):
    """float32 values -> the raw bits of the type, rounded to nearest even (test inputs: finite values or specials, no NaN payload care)"""
    x = np.ascontiguousarray(x, np.float32)
    if kind == "f32":
        return x.view(np.uint32).copy()
    if kind == "f16":
        with np.errstate(over="ignore", invalid="ignore"):
            return x.astype(np.float16).view(np.uint16).copy()
    u = x.view(np.uint32).astype(np.uint64)
    out = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    out[np.isnan(x)] = 0x7FC0
    return out


def taps(n, s):
    """per up-index o of an axis of n source pixels: a list of (source index, weight) with one tap of weight 1 or two dyadic taps"""
    assert s in (2, 4) and n >= 1
    out = []
    for o in range(s * n):
        i0, r = o // s, o % s
        i1 = min(i0 + 1, n - 1)
        if r == 0:
            out.append([(i0, 1.0)])                      # the second tap has weight 0: dropped
        elif i1 == i0:
            out.append([(i0, 1.0)])                      # both taps on the clamped last pixel: merged
        else:
            out.append([(i0, (s - r) / s), (i1, r / s)])
    return out


def _mix(tp, rows):
    """one tap: the value itself; two taps: fadd(fmul(w0, a), fmul(w1, b)), each operation rounded to f32"""
    if len(tp) == 1:
        return rows(tp[0][0]).copy()
    (i0, w0), (i1, w1) = tp
    return (np.float32(w0) * rows(i0)).astype(np.float32) + (np.float32(w1) * rows(i1)).astype(np.float32)


def forward(x, s):
    """x (B, H, W, C) float32 -> y (B, s H, s W, C) float32: horizontally first on every source row, then vertically"""
    x = np.ascontiguousarray(x, np.float32)
    B, H, W, C = x.shape
    with np.errstate(all="ignore"):
        t = np.empty((B, H, s * W, C), np.float32)
        for ox, tp in enumerate(taps(W, s)):
            t[:, :, ox] = _mix(tp, lambda i: x[:, :, i])
        y = np.empty((B, s * H, s * W, C), np.float32)
        for oy, tp in enumerate(taps(H, s)):
            y[:, oy] = _mix(tp, lambda i: t[:, i])
    return y


def backward(g, s, H, W):
    """g (B, s H, s W, C) float32 -> g_x (B, H, W, C): the terms fmul(wy * wx, g[oy, ox]) added to 0.0f in raster order of (oy, ox)"""
    g = np.ascontiguousarray(g, np.float32)
    B, C = g.shape[0], g.shape[3]
    assert g.shape[1] == s * H and g.shape[2] == s * W
    ty, tx = taps(H, s), taps(W, s)
    gx = np.zeros((B, H, W, C), np.float32)
    with np.errstate(all="ignore"):
        for oy in range(s * H):                          # raster order: for a fixed (iy, ix) the terms arrive oy ascending, then ox ascending
            for iy, wy in ty[oy]:
                for ox in range(s * W):
                    for ix, wx in tx[ox]:
                        w = np.float32(np.float32(wy) * np.float32(wx))
                        gx[:, iy, ix] = gx[:, iy, ix] + (w * g[:, oy, ox]).astype(np.float32)
    return gx


def matrix(n, s):
    """the (s n, n) float64 interpolation matrix of one axis"""
    A = np.zeros((s * n, n), np.float64)
    for o, tp in enumerate(taps(n, s)):
        for i, w in tp:
            A[o, i] += w
    return A
