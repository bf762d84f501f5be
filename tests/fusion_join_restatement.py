"""The deep-fusion join (include/mv3d_hip.h) restated in numpy, f32 arithmetic exactly as the contract states
it, and the drop-path draw rule of networks/mv3d.py.  Tensors are carried as their RAW BITS (uint32 for f32, uint16 for f16 / bf16),
so that comparisons are bit comparisons and bf16 needs no numpy type.  Not a test module: the checker of tests/test_fusion_join.py
and tests/test_deep_fusion.py, never the thing under test."""
import numpy as np

KINDS = ("f32", "f16", "bf16")
BITS = {"f32": np.uint32, "f16": np.uint16, "bf16": np.uint16}
QNAN = {"f32": 0x7FC00000, "f16": 0x7E00, "bf16": 0x7FC0}


def to_f32(bits, kind):
    bits = np.ascontiguousarray(bits, BITS[kind])
    if kind == "f32":
        return bits.view(np.float32)
    if kind == "f16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def from_f32(x, kind):
    """round to nearest even; a NaN becomes the type's canonical quiet NaN"""
    x = np.ascontiguousarray(x, np.float32)
    nan = np.isnan(x)
    if kind == "f32":
        out = x.view(np.uint32).copy()
    elif kind == "f16":
        with np.errstate(over="ignore", invalid="ignore"):
            out = x.astype(np.float16).view(np.uint16).copy()
    else:
        u = x.view(np.uint32).astype(np.uint64)
        out = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    out[nan] = QNAN[kind]
    return out


def _tables(keep, views):
    keep = np.asarray(keep) != 0
    assert keep.ndim == 2 and keep.shape[1] == views and keep.any(1).all()
    return keep, keep.sum(1).astype(np.float32)


def join_forward(h_bits, keep, kind, drop=None, scale=1.0):
    """h_bits (sets_in, views, rows, channels) -> out bits (paths, rows, channels)"""
    S, V, R, C = h_bits.shape
    keep, n = _tables(keep, V)
    P = keep.shape[0]
    assert S in (1, P)
    scale = np.float32(scale)
    out = np.empty((P, R, C), BITS[kind])
    with np.errstate(all="ignore"):
        for p in range(P):
            s = np.zeros((R, C), np.float32)
            for v in range(V):
                if keep[p, v]:                                         # a view that is not kept is never read
                    x = to_f32(h_bits[p if S > 1 else 0, v], kind)
                    s = s + np.where(x < 0, np.float32(0), x)
            m = s / n[p]
            if drop is not None:
                m = np.where(drop[p] != 0, m * scale, np.float32(0))
            out[p] = from_f32(m, kind)
    return out


def join_backward(h_bits, g_out_bits, keep, kind, drop=None, scale=1.0):
    """-> g_h bits of h's shape; with sets_in == 1 the paths' terms are added to 0 in ascending p"""
    S, V, R, C = h_bits.shape
    keep, n = _tables(keep, V)
    P = keep.shape[0]
    assert S in (1, P) and g_out_bits.shape == (P, R, C)
    scale = np.float32(scale)
    g_h = np.empty((S, V, R, C), BITS[kind])
    acc = np.zeros((V, R, C), np.float32)
    with np.errstate(all="ignore"):
        for p in range(P):
            t = to_f32(g_out_bits[p], kind)
            if drop is not None:
                t = t * np.where(drop[p] != 0, scale, np.float32(0))
            q = t / n[p]
            for v in range(V):
                if keep[p, v]:
                    g = np.where(to_f32(h_bits[p if S > 1 else 0, v], kind) > 0, q, np.float32(0))
                else:
                    g = np.zeros((R, C), np.float32)
                if S == 1:
                    acc[v] = acc[v] + g
                else:
                    g_h[p, v] = from_f32(g, kind)
        if S == 1:
            for v in range(V):
                g_h[0, v] = from_f32(acc[v], kind)
    return g_h


def draw_drop_path(rng, views):
    """the main network's keep rows of one training forward, (2, views): join 1, join 2"""
    keep = np.zeros((2, views), np.uint8)
    u = rng.random_sample()
    if u < 0.5:                                                        # global: one view at both joins
        v = rng.randint(views)
        keep[0, v] = keep[1, v] = 1
        return keep, True
    for j in range(2):                                                 # local: every input of a join is a coin flip
        k = rng.random_sample(views) >= 0.5
        if not k.any():
            k[rng.randint(views)] = True
        keep[j] = k
    return keep, False
