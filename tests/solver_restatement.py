"""The training solver's three launches restated in numpy: the momentum-SGD step (csrc/solver.hip), the controlled Adam step (csrc/adam.hip,
the CTL instance) and the global gradient norm with its clip coefficient (csrc/solver.hip).  A float64 REFERENCE of each, a RESTATEMENT
of each in the kernel's order of operations, and an ERROR BOUND of each as a function of the operands.  Plain numpy, no project code, and
nothing imported from tests/optim_loss_restatement.py: what is needed of Adam is restated here.  Not a test module: the checker of
tests/test_solver.py, never the thing under test.

The references take the kernels' f32 operands (p, g, the state, the control record's coef, the tensor record's weight_decay) widened to
f64 and the hyper-parameters (lr, momentum, betas, eps) as the doubles the caller passed.

Notation of the derivations: u = 2^-24 is the unit roundoff of f32: every correctly rounded f32 operation (+ - * / sqrt, a constant
rounded from a double) returns its exact result times (1 + d), |d| <= u.  The library is built with contraction off, so a multiply-add
is two roundings.  Terms of order u^2 are covered by the factor SECOND on every bound, results that leave the normal range by the
absolute term TINY.  Each docstring derives the WORST CASE of a correct f32 implementation to first order; the bound a function returns
is SAFETY = 2 times that, and the unmarked tests of test_solver.py hold the f32 restatement to half of it (the figures it reaches stand
beside each bound).

The norm is different in kind: its squares are exact in f64 and its additions are f64, so its restatement here is not an approximation
of the kernel but the kernel's own order of additions, and u64 = 2^-53 takes u's place in its bound.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24                     # unit roundoff of f32
U64 = 2.0 ** -53                   # unit roundoff of f64
SECOND = 1.0 + 2.0 ** -10          # covers the second-order terms
TINY = 2.0 ** -120                 # absolute slack where an intermediate can be subnormal
SAFETY = 2.0                       # returned bound / derived worst case
CHUNK = 4096                       # elements per workgroup of all three launches (mv3d_adam_chunk_elements())
FINISH_THREADS = 1024              # threads of the norm's finishing workgroup (MV3D_GRAD_NORM_FINISH_THREADS)


def _w(a):
    return np.asarray(a, F32).astype(F64)


# =================================================================== g' = coef * g + weight_decay * p
def gprime_ref(p, g, coef, wd):
    """f64 from the f32 operands: coef g + wd p"""
    return float(F32(coef)) * _w(g) + float(F32(wd)) * _w(p)


def gprime_f32(p, g, coef, wd):
    """step_gradient of csrc/solver.h: the product with coef only when coef != 1, the decay term only when wd != 0"""
    p, g = np.asarray(p, F32), np.asarray(g, F32)
    with np.errstate(all="ignore"):
        if F32(coef) != F32(1):
            g = F32(coef) * g
        if F32(wd) != F32(0):
            g = g + F32(wd) * p
    assert g.dtype == F32
    return g


def gprime_bound(p, g, coef, wd):
    """UNSCALED first-order worst case of |g'_f32 - g'_ref| (the callers apply SECOND and SAFETY once, on their own totals):
    fl(coef g) carries u |coef g| (one rounding, none when coef == 1); fl(wd p) u |wd p| and the sum u |g'| (two more roundings, none
    when wd == 0).  ABSOLUTE in the operands: where coef g and wd p cancel the error does not shrink with g'."""
    c, w = float(F32(coef)), float(F32(wd))
    b = np.zeros(np.asarray(g).shape, F64)
    if c != 1.0:
        b = b + U * np.abs(c * _w(g))
    if w != 0.0:
        b = b + U * np.abs(w * _w(p)) + U * np.abs(gprime_ref(p, g, coef, wd))
    return b


# =================================================================== momentum SGD
def sgd_ref(p, g, buf, lr, momentum, coef=1.0, wd=0.0):
    """f64: buf = momentum buf + g';  p = p - lr buf  (torch.optim.SGD's and TensorFlow's MomentumOptimizer's rule)"""
    b = momentum * _w(buf) + gprime_ref(p, g, coef, wd)
    return _w(p) - lr * b, b


def sgd_f32(p, g, buf, lr, momentum, coef=1.0, wd=0.0):
    """sgd_one of csrc/solver.hip: lr and momentum rounded once from the doubles"""
    p, buf = np.asarray(p, F32), np.asarray(buf, F32)
    with np.errstate(all="ignore"):
        buf = F32(momentum) * buf + gprime_f32(p, g, coef, wd)
        p = p - F32(lr) * buf
    assert p.dtype == buf.dtype == F32
    return p, buf


def sgd_bound(p, g, buf, lr, momentum, coef=1.0, wd=0.0):
    """(bound_p, bound_buf): absolute bounds of |f32 result - sgd_ref| per element.

    buf: fl(fl(mu32 * buf) + g'_f32): the rounded constant and the product u |mu buf| each, g' its own error (gprime_bound), the sum
         u |buf_new|:
            |dbuf| <= 2 u |mu buf| + bound_g' + u |buf_new|
    p:   upd = fl(lr32 * buf_f32): lr times buf's error, the rounded constant and the product u |lr buf_new| each; fl(p - upd) adds
         half an ulp of the result:
            |dp| <= u |p_new| + lr (|dbuf| + 2 u |buf_new|)
    """
    pr, br = sgd_ref(p, g, buf, lr, momentum, coef, wd)
    bb = 2.0 * U * np.abs(momentum * _w(buf)) + gprime_bound(p, g, coef, wd) + U * np.abs(br)
    bp = U * np.abs(pr) + lr * (bb + 2.0 * U * np.abs(br))
    return SAFETY * (bp * SECOND + TINY), SAFETY * (bb * SECOND + TINY)      # f32 restatement's worst use, case tables: p 0.496, buf 0.476


# =================================================================== controlled Adam
def adam_consts(lr, b1, b2, eps, t):
    """the launch constants of mv3d_adam_step / mv3d_adam_step_ctl, doubles"""
    return lr / (1.0 - b1 ** t), 1.0 / np.sqrt(1.0 - b2 ** t)


def adam_ctl_ref(p, g, m, v, lr, b1, b2, eps, t, coef=1.0, wd=0.0):
    """f64 Adam on g': m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g' g';  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)"""
    gp = gprime_ref(p, g, coef, wd)
    p, m, v = _w(p), _w(m), _w(v)
    m = b1 * m + (1.0 - b1) * gp
    v = b2 * v + (1.0 - b2) * gp * gp
    p = p - lr / (1.0 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps)
    return p, m, v


def adam_ctl_f32(p, g, m, v, lr, b1, b2, eps, t, coef=1.0, wd=0.0):
    """adam_one of csrc/adam.hip on step_gradient's g': constants rounded once from doubles, lerp for the first moment, (omb2 * g') * g'"""
    p, m, v = (np.asarray(a, F32) for a in (p, m, v))
    g = gprime_f32(p, g, coef, wd)
    lrb, isb = adam_consts(lr, b1, b2, eps, t)
    lrb, isb, beta2, e = F32(lrb), F32(isb), F32(b2), F32(eps)
    omb1, omb2 = F32(1.0 - b1), F32(1.0 - b2)
    with np.errstate(all="ignore"):
        m = m + (g - m) * omb1
        v = beta2 * v + omb2 * g * g
        denom = np.sqrt(v) * isb + e
        p = p - lrb * (m / denom)
    assert p.dtype == m.dtype == v.dtype == F32
    return p, m, v


def adam_ctl_bound(p, g, m, v, lr, b1, b2, eps, t, coef=1.0, wd=0.0):
    """(bound_p, bound_m, bound_v) of |f32 result - adam_ctl_ref| per element: the plain step's derivation with g' in g's place, plus
    what g's own error e' = gprime_bound (two or three roundings) adds.

    m:  fl(m + fl(fl(g' - m) * omb1)): the difference u |g' - m|, the rounded constant and the product u each, all scaled by (1 - b1);
        the final sum u |m_new|; with |g' - m|, |m_new| <= |m| + |g'|; and g's error enters scaled by (1 - b1):
            |dm| <= u (1 + 3 (1 - b1)) (|m| + |g'|) + (1 - b1) e'
    v:  fl(fl(beta2 v) + fl(fl(omb2 g') g')): non-negative terms, 2 u on the first, 3 u on the second, u for the sum; g's error moves
        g'^2 by 2 |g'| e':
            |dv| <= 4 u v_new + dv',   dv' = 2 (1 - b2) |g'| e'
    p:  denom = fl(fl(sqrt(v) * isb) + eps): the plain step's 6 u relative, plus dv' through the root: d sqrt(v) <= dv' / (2 sqrt(v_new))
        (sqrt(dv') where v_new = 0), times isb.  q = fl(m / denom), upd = fl(lrb * q): |dm| / denom, |m_new| / denom times
        (6 u + u + 2 u) = 9 u and times the root's share over denom; fl(p - upd) adds u |p_new|:
            |dp| <= u |p_new| + lr_bc / denom * (|dm| + |m_new| (9 u + isb dsqrt / denom))
    """
    pr, mr, vr = adam_ctl_ref(p, g, m, v, lr, b1, b2, eps, t, coef, wd)
    gp, eg = gprime_ref(p, g, coef, wd), gprime_bound(p, g, coef, wd)
    lrb, isb = adam_consts(lr, b1, b2, eps, t)
    bm = U * (1.0 + 3.0 * (1.0 - b1)) * (np.abs(_w(m)) + np.abs(gp)) + (1.0 - b1) * eg
    dv = 2.0 * (1.0 - b2) * np.abs(gp) * eg
    bv = 4.0 * U * vr + dv
    with np.errstate(all="ignore"):
        dsq = np.where(vr > 0.0, dv / (2.0 * np.sqrt(vr)), np.sqrt(dv))
    denom = np.sqrt(vr) * isb + eps
    bp = U * np.abs(pr) + lrb / denom * (bm + np.abs(mr) * (9.0 * U + isb * dsq / denom))
    return SAFETY * (bp * SECOND + TINY), SAFETY * (bm * SECOND + TINY), SAFETY * (bv * SECOND + TINY)   # worst use: p 0.499, m 0.380, v 0.342


# =================================================================== the global gradient norm
def sumsq_ref(grads):
    """math.fsum of the exact squares of every element of every tensor: the correctly rounded sum (NaN / inf where one appears)"""
    sq = np.concatenate([_w(g).reshape(-1) ** 2 for g in grads]) if len(grads) else np.zeros(0)
    if not np.isfinite(sq).all():
        return float("nan") if np.isnan(sq).any() else float("inf")
    return math.fsum(sq.tolist())


def _butterfly(s):
    """lane 0 of `s + shuffle_xor(s, k)` for k = 32, 16, .. 1 over the last axis of 64 lanes: lanes l < k hold s[l] + s[l + k]"""
    k = s.shape[-1] // 2
    while k >= 1:
        s = s[..., :k] + s[..., k:2 * k]
        k //= 2
    return s[..., 0]


def chunk_partials(g):
    """grad_sumsq_kernel on one tensor: thread t of a chunk owns elements 1024 u + 4 t + j and adds their squares u-major, j-minor; 64
    threads -> wave by the butterfly; the chunk's partial is (w0 + w1) + (w2 + w3).  Elements past the tensor's end add +0."""
    x = _w(g).reshape(-1)
    n = -(-x.size // CHUNK)
    x = np.concatenate([x, np.zeros(n * CHUNK - x.size)]).reshape(n, 4, 256, 4)
    with np.errstate(all="ignore"):
        s = np.zeros((n, 256))
        for u in range(4):
            for j in range(4):
                s = s + x[:, u, :, j] * x[:, u, :, j]
        w = _butterfly(s.reshape(n, 4, 64))
        return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def sumsq_restated(grads):
    """mv3d_grad_norm's 64 bits: the chunks' partials in table order; finishing thread t adds partials t, t + 1024, ... in that order;
    the butterfly per wave; the 16 waves by halving (l < k: w[l] + w[l + k], k = 8, 4, 2, 1)"""
    parts = np.concatenate([chunk_partials(g) for g in grads]) if len(grads) else np.zeros(0)
    r = -(-parts.size // FINISH_THREADS)
    parts = np.concatenate([parts, np.zeros(r * FINISH_THREADS - parts.size)]).reshape(r, FINISH_THREADS)
    with np.errstate(all="ignore"):
        s = np.zeros(FINISH_THREADS)
        for row in parts:
            s = s + row
        w = _butterfly(s.reshape(FINISH_THREADS // 64, 64))
        k = w.size // 2
        while k >= 1:
            w = w[:k] + w[k:2 * k]
            k //= 2
    return float(w[0])


def sumsq_chain(sizes):
    """f64 additions on the longest chain from an element to the sum: 16 in its thread, 6 + 2 to the chunk's partial, one per round
    of the finishing thread (ceil(chunks / 1024)), 6 + 4 to the total"""
    chunks = sum(-(-int(n) // CHUNK) for n in sizes)
    return 16 + 6 + 2 + -(-chunks // FINISH_THREADS) + 6 + 4


def sumsq_bound(sizes):
    """bound of |sumsq - sumsq_ref| / sumsq_ref.  Every term is a non-negative exact square, so every addition's rounding is relative
    to a partial sum that is at most the total: an element passes through sumsq_chain(sizes) additions, each (1 + d), |d| <= u64, so
    the computed sum is sum_i x_i^2 (1 + D_i), |D_i| <= chain u64 to first order; fsum's own rounding adds u64."""
    return SAFETY * (sumsq_chain(sizes) + 1) * U64 * SECOND                 # restatement's worst use over the case tables: 0.023


def control_rule(sumsq, max_norm, guard, empty=False):
    """(norm f32, coef f32, skip) that grad_norm_finish_kernel writes on top of a given sumsq: skip = guard and not finite; coef 0
    under skip, 1 without clipping (or without chunks), else max_norm / (sqrt(sumsq) + 1e-6) in f64, 1 where that is >= 1, its f32
    rounding below (torch.nn.utils.clip_grad_norm_'s rule)"""
    with np.errstate(all="ignore"):
        root = np.sqrt(F64(sumsq))
        skip = int(bool(guard) and not np.isfinite(sumsq))
        if skip:
            coef = F32(0)
        elif max_norm == 0.0 or empty:
            coef = F32(1)
        else:
            q = F64(max_norm) / (root + F64(1e-6))
            coef = F32(1) if q >= 1.0 else F32(q)
        return F32(root), coef, skip


# =================================================================== 16-bit roundings (raw bits)
def lowp_bits(x, kind):
    """f32 -> the uint16 bits of its float16 ('f16') / bfloat16 ('bf16') rounding to nearest even; NaN -> the canonical quiet NaN"""
    x = np.ascontiguousarray(x, F32)
    nan = np.isnan(x)
    if kind == "f16":
        with np.errstate(over="ignore", invalid="ignore"):
            out = x.astype(np.float16).view(np.uint16).copy()
        out[nan] = 0x7E00
    else:
        w = x.view(np.uint32).astype(np.uint64)
        out = ((w + 0x7FFF + ((w >> 16) & 1)) >> 16).astype(np.uint16)
        out[nan] = 0x7FC0
    return out
