"""One Adam step (csrc/adam.hip), the two fused training losses with their gradients and the row softmax (csrc/losses.hip) restated in
numpy: a float64 REFERENCE of each, a float32 RESTATEMENT of each in the kernel's order of operations, and an ERROR BOUND of each as a
function of the operands.  Plain numpy, no project code.  Not a test module: the checker of tests/test_optim_loss_edges.py, never the
thing under test.

The references take the kernels' f32 operands widened to f64 and the hyper-parameters as the doubles the caller passed.  The f32
restatements exist for one purpose: the unmarked tests of test_optim_loss_edges.py run them against the references on every case list
and so prove that a correct f32 implementation CAN stay inside the bounds; a kernel that does not is then wrong, not unlucky.

Notation of the derivations: u = 2^-24 is the unit roundoff of f32 (half of numpy's eps32 = 2^-23): every correctly rounded f32
operation (+ - * / sqrt, a constant rounded from a double) returns its exact result times (1 + d), |d| <= u.  The library is built
with contraction off, so a multiply-add is two roundings.  expf and logf are allowed one ulp (the accuracy HIP documents for both),
that is a relative 2u.  Terms of order u^2 are covered by the factor SECOND on every bound; results that leave the normal range
(expf underflow) by the absolute term TINY.

Each docstring derives the WORST CASE of a correct f32 implementation to first order.  Round to nearest reaches its half ulp, so a
correct implementation comes arbitrarily close to that worst case wherever one rounding dominates (the f32 restatement reaches 0.996
of it on the parameter); the bound a function returns is therefore SAFETY = 2 times the derived worst case, a margin of 2 over the
worst error the f32 restatement shows on the case tables (the figures stand beside each bound).
"""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24                     # unit roundoff of f32
EPS32 = 2.0 ** -23                 # numpy's float32 eps = one ulp of 1.0
SECOND = 1.0 + 2.0 ** -10          # covers the second-order terms (products of at most ~100 u with each other)
TINY = 2.0 ** -120                 # absolute slack where an intermediate can be subnormal (f32's smallest normal is 2^-126)
EXP_CLIP = 104.0                   # expf(d) is below f32's smallest subnormal for d < -103.98: a larger |d| no longer adds error
ULP_FN = 2.0 * U                   # one ulp as a relative error: expf, logf
SAFETY = 2.0                       # returned bound / derived worst case


def _w(a):
    return np.asarray(a, F32).astype(F64)


# =================================================================== Adam
def adam_consts(lr, b1, b2, eps, t):
    """the launch constants of mv3d_adam_step, doubles"""
    return lr / (1.0 - b1 ** t), 1.0 / np.sqrt(1.0 - b2 ** t)


def adam_ref(p, g, m, v, lr, b1, b2, eps, t):
    """f64: m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)"""
    p, g, m, v = _w(p), _w(g), _w(m), _w(v)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - lr / (1.0 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps)
    return p, m, v


def adam_f32(p, g, m, v, lr, b1, b2, eps, t):
    """adam_one of csrc/adam.hip: the constants rounded once from doubles, lerp for the first moment, (omb2 * g) * g"""
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
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


def adam_bound(p, g, m, v, lr, b1, b2, eps, t):
    """(bound_p, bound_m, bound_v): absolute bounds of |f32 result - adam_ref| per element.

    m:  fl(m + fl(fl(g - m) * omb1)): the difference carries u |g - m|, the rounded constant and the product u each, all scaled by
        (1 - b1); the final sum u |m_new|.  With |g - m| <= |m| + |g| and |m_new| <= |m| + |g|:
            |dm| <= u (1 + 3 (1 - b1)) (|m| + |g|)                                  [<= 4 u (|m| + |g|)]
        ABSOLUTE in the operands: where the lerp cancels (m_new near 0) the error does not shrink with m_new.
    v:  fl(fl(beta2 * v) + fl(fl(omb2 * g) * g)): both terms are non-negative, so the errors stay relative: constant + product = 2 u
        on the first, constant + two products = 3 u on the second, u for the sum:
            |dv| <= 4 u v_new
    p:  denom = fl(fl(sqrt(v) * isb) + eps): sqrt halves v's 4 u and adds u (3 u), the rounded constant and the product (5 u), the
        rounded eps is smaller (u), the sum of the two non-negative terms keeps the larger and adds u: 6 u relative.
        q = fl(m / denom), upd = fl(lrb * q): dm / denom propagated, then |m_new| / denom times 6 u (denom) + u (division) + 2 u
        (constant, product) = 9 u.  p_new = fl(p - upd) adds half an ulp of the result, u |p_new|:
            |dp| <= u |p_new| + lr_bc / denom * (bound_m + 9 u |m_new|)
    """
    pr, mr, vr = adam_ref(p, g, m, v, lr, b1, b2, eps, t)
    g, m = _w(g), _w(m)
    lrb, isb = adam_consts(lr, b1, b2, eps, t)
    bm = U * (1.0 + 3.0 * (1.0 - b1)) * (np.abs(m) + np.abs(g)) * SECOND + TINY
    bv = 4.0 * U * vr * SECOND + TINY
    denom = np.sqrt(vr) * isb + eps
    bp = (U * np.abs(pr) + lrb / denom * (bm + 9.0 * U * np.abs(mr))) * SECOND + TINY
    return SAFETY * bp, SAFETY * bm, SAFETY * bv                        # f32 restatement's worst use, case tables: p 0.498, m 0.357, v 0.394


# =================================================================== the losses
def _smooth_l1(x, sigma):
    s2 = float(sigma) * float(sigma)
    quad = np.abs(x) < 1.0 / s2
    f = np.where(quad, 0.5 * s2 * x * x, np.abs(x) - 0.5 / s2)
    df = np.where(quad, s2 * x, np.sign(x))
    return f, df


def _select(labels, rows, rpn):
    if rpn:
        lf = np.asarray(labels, F32).reshape(rows)
        return lf.astype(np.int64), lf != F32(-1), lf == F32(1)
    return np.asarray(labels, np.int64).reshape(rows), np.ones(rows, bool), np.ones(rows, bool)


def loss_ref(cls, labels, pred, tgt, sigma, rpn):
    """f64.  cross-entropy: mean over the selected rows of logsumexp(z) - z[label]; box loss: mean over the selected rows of
    sum_d smoothL1_sigma(pred - tgt).  RPN (f32 labels): cross-entropy over label != -1, box loss over label == 1; RCNN (i32 labels):
    every row.  A mean over no rows is NaN with zero gradients; a label outside 0 .. K-1 makes the cross-entropy NaN and leaves its
    row's gradient the plain softmax over the count.
    -> dict(ce, box, d_cls, d_pred, n_ce, n_box) plus the per-row pieces the bound needs"""
    z, p, t = _w(cls), _w(pred), _w(tgt)
    R, K = z.shape
    label, use_ce, use_box = _select(labels, R, rpn)
    n_ce, n_box = int(use_ce.sum()), int(use_box.sum())
    with np.errstate(all="ignore"):
        mx = z.max(1, keepdims=True) if R else np.zeros((0, 1))
        e = np.exp(z - mx)
        se = e.sum(1, keepdims=True)
        ok = (label >= 0) & (label < K)
        zl = np.where(ok, z[np.arange(R), np.clip(label, 0, K - 1)], np.nan)
        ce_row = np.log(se[:, 0]) - (zl - mx[:, 0])
        onehot = (np.arange(K)[None, :] == label[:, None]).astype(F64)
        soft = e / se
        d_cls = np.where(use_ce[:, None], soft - onehot, 0.0) / max(n_ce, 1)
        f, df = _smooth_l1(p - t, sigma)
        d_pred = np.where(use_box[:, None], df, 0.0) / max(n_box, 1)
        ce = ce_row[use_ce].sum() / n_ce if n_ce else np.nan
        box = f[use_box].sum() / n_box if n_box else np.nan
    return dict(ce=ce, box=box, d_cls=d_cls, d_pred=d_pred, n_ce=n_ce, n_box=n_box, use_ce=use_ce, use_box=use_box, soft=soft,
                onehot=onehot, se=se[:, 0], mx=mx[:, 0], zl=zl, ce_row=ce_row, f=f, x=p - t)


def _expf(d):
    """expf of an f32 array, correctly rounded (numpy's own f32 exp is a SIMD approximation of several ulp)"""
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(d, F32).astype(F64)).astype(F32)


def _logf(s):
    with np.errstate(all="ignore"):
        return np.log(np.asarray(s, F32).astype(F64)).astype(F32)


def loss_f32(cls, labels, pred, tgt, sigma, rpn):
    """loss_partial_kernel + loss_final_kernel: every row in f32 in class / column order, the rows' sums in f64, the scale 1 / count
    rounded to f32 and applied to the unscaled f32 gradients  -> (losses f32[2], d_cls f32, d_pred f32)"""
    z, p, t = (np.asarray(a, F32) for a in (cls, pred, tgt))
    R, K = z.shape
    D = p.shape[1]
    label, use_ce, use_box = _select(labels, R, rpn)
    sigma2 = F32(F32(sigma) * F32(sigma))
    with np.errstate(all="ignore"):
        mx = z[:, 0].copy() if R else np.zeros(0, F32)
        for k in range(1, K):
            mx = np.fmax(mx, z[:, k])
        ek = [_expf(z[:, k] - mx) for k in range(K)]
        se = np.zeros(R, F32)
        for k in range(K):
            se = se + ek[k]
        ok = (label >= 0) & (label < K)
        zl = np.where(ok, z[np.arange(R), np.clip(label, 0, K - 1)], F32(np.nan)).astype(F32)
        ce_row = _logf(se) - (zl - mx)
        d_cls = np.stack([ek[k] / se - (label == k).astype(F32) for k in range(K)], 1)
        d_cls = np.where(use_ce[:, None], d_cls, F32(0)).astype(F32)
        thr = F32(1) / sigma2
        acc = np.zeros(R, F32)
        d_pred = np.zeros((R, D), F32)
        for j in range(D):
            x = p[:, j] - t[:, j]
            ax = np.abs(x)
            quad = ax < thr
            acc = acc + np.where(quad, (x * x) * (F32(0.5) * sigma2), ax - F32(0.5) / sigma2)
            d_pred[:, j] = np.where(quad, sigma2 * x, np.sign(x))
        d_pred = np.where(use_box[:, None], d_pred, F32(0)).astype(F32)
        n_ce, n_box = float(use_ce.sum()), float(use_box.sum())
        losses = np.array([ce_row[use_ce].astype(F64).sum() / n_ce if n_ce else np.nan,
                           acc[use_box].astype(F64).sum() / n_box if n_box else np.nan]).astype(F32)
        ice = F32(1.0 / n_ce) if n_ce else F32(0)
        ibox = F32(1.0 / n_box) if n_box else F32(0)
        d_cls, d_pred = d_cls * ice, d_pred * ibox
    assert d_cls.dtype == d_pred.dtype == acc.dtype == ce_row.dtype == F32
    return losses, d_cls, d_pred


def loss_bound(cls, labels, pred, tgt, sigma, rpn):
    """(bound_ce, bound_box, bound_d_cls (R, K), bound_d_pred (R, D)) against loss_ref.

    With d_k = z_k - max <= 0 and c_k = min(|d_k|, 104) (beyond that expf is 0 whatever the rounding of d_k):
      e_k = expf(fl(d_k)):    the rounded difference moves the exponent by u |d_k|, expf adds an ulp: relative  2 u + u c_k
      se  = sum in class order: a weighted mean of the e_k's errors plus K - 1 additions:              E_s = 2 u + u max_k c_k + (K - 1) u
      row = fl(logf(se) - fl(z_label - max)): d log(se) = E_s, logf's ulp 2 u |log se|, the two differences u each:
            |d row| <= E_s + 2 u |log se| + u |z_label - max| + u |row|
      cross-entropy = f32(f64 mean of the rows): mean of the rows' bounds + u |ce|
      unscaled gradient  g_k = fl(fl(e_k / se) - [k == label]):  softmax_k (2 u + u c_k + E_s + u) for the quotient, u |g_k| for the
            difference; scaled by fl(1 / n): constant and product, 2 u |g_k|:
            |d d_cls_k| <= (softmax_k (3 u + u c_k + E_s) + 3 u |g_k|) / n_ce
            (near a confident label g_k = p - 1 is ~0 while softmax_k is ~1: the error is an ABSOLUTE ~4 u / n_ce, not relative)
    smooth L1, x = fl(pred - tgt), |dx| <= u |x|, f is 1-Lipschitz and continuous with its derivative at 1/sigma^2, so a branch taken
    differently within an ulp of the threshold changes f by O(u^2) and f' by sigma^2 |x - 1/sigma^2| <= u:
      quad:   fl(fl(x x) * (0.5 sigma^2)): 2 u from x, u per product (0.5 sigma^2 is exact for the sigmas in use; u more otherwise)
      linear: fl(|x| - fl(0.5 / sigma^2)): u |x| from x, u 0.5 / sigma^2 from the constant, u f from the difference
            |d f| <= 5 u f + u (|x| + 0.5 / sigma^2)                               (an upper bound of both branches)
      a row adds D terms in column order: (D - 1) u sum_j f_j;  box loss = f32(f64 mean of the rows): mean of the rows' bounds + u |box|
      unscaled gradient: quad fl(sigma^2 x): u from x, u from the product (one more for sigma^2), linear exactly +-1, the branch
            mismatch u:  4 u min(1, sigma^2 |x|);  scaled by fl(1 / n): 2 u more:
            |d d_pred| <= 6 u min(1, sigma^2 |x|) / n_box
    """
    r = loss_ref(cls, labels, pred, tgt, sigma, rpn)
    z = _w(cls)
    R, K = z.shape
    D = np.asarray(pred).shape[1]
    s2 = float(sigma) * float(sigma)
    with np.errstate(all="ignore"):
        c = np.minimum(np.abs(z - r["mx"][:, None]), EXP_CLIP)
        c = np.where(np.isfinite(c), c, EXP_CLIP)
        Es = (2.0 + c.max(1) + (K - 1)) * U if R else np.zeros(0)
        row = Es + ULP_FN * np.abs(np.log(r["se"])) + U * np.abs(r["zl"] - r["mx"]) + U * np.abs(r["ce_row"]) + K * TINY
        b_ce = (row[r["use_ce"]].sum() / r["n_ce"] + U * abs(r["ce"])) * SECOND if r["n_ce"] else np.nan
        g = r["soft"] - r["onehot"]
        b_dcls = (r["soft"] * (3.0 * U + U * c + Es[:, None]) + 3.0 * U * np.abs(g) + TINY) / max(r["n_ce"], 1) * SECOND
        b_dcls = np.where(r["use_ce"][:, None], b_dcls, 0.0)
        f, ax = r["f"], np.abs(r["x"])
        bf = 5.0 * U * f + U * (ax + 0.5 / s2) + TINY
        rowb = bf.sum(1) + (D - 1) * U * f.sum(1)
        b_box = (rowb[r["use_box"]].sum() / r["n_box"] + U * abs(r["box"])) * SECOND if r["n_box"] else np.nan
        b_dpred = (6.0 * U * np.minimum(1.0, s2 * ax) + TINY) / max(r["n_box"], 1) * SECOND
        b_dpred = np.where(r["use_box"][:, None], b_dpred, 0.0)
    return SAFETY * b_ce, SAFETY * b_box, SAFETY * b_dcls, SAFETY * b_dpred   # f32 restatement's worst use: 0.130, 0.039, 0.211, 0.195


# =================================================================== softmax over rows
def softmax_ref(x):
    """f64 softmax over the last axis; a row holding NaN or +inf, or made of -inf only, is NaN throughout; a -inf entry of any other row
    is 0"""
    x = _w(x)
    with np.errstate(all="ignore"):
        e = np.exp(x - x.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)


def softmax_f32(x):
    """softmax_rows_kernel: max, expf of the differences, sum in class order, divide"""
    x = np.asarray(x, F32)
    K = x.shape[-1]
    with np.errstate(all="ignore"):
        mx = x[..., 0].copy()
        for k in range(1, K):
            mx = np.fmax(mx, x[..., k])
        e = _expf(x - mx[..., None])
        s = np.zeros(mx.shape, F32)
        for k in range(K):
            s = s + e[..., k]
        y = e / s[..., None]
    assert y.dtype == F32
    return y


def softmax_bound(x):
    """|d y_k| <= y_k (3 u + u c_k + E_s): e_k carries 2 u + u c_k and the quotient u, the sum E_s = 2 u + u max c + (K - 1) u (see
    loss_bound).  The row's sum: sum_k fl(e_k / s) with s = sum e_k (1 + at most (K - 1) u) is within (K - 1) u + u <= K eps32 of 1."""
    y = softmax_ref(x)
    xw = _w(x)
    K = xw.shape[-1]
    with np.errstate(all="ignore"):
        c = np.minimum(np.abs(xw - xw.max(-1, keepdims=True)), EXP_CLIP)
        c = np.where(np.isfinite(c), c, EXP_CLIP)
        Es = (2.0 + c.max(-1, keepdims=True) + (K - 1)) * U
        return SAFETY * (y * (3.0 * U + U * c + Es) * SECOND + TINY)      # f32 restatement's worst use: 0.231


# =================================================================== 16-bit roundings (raw bits, as fusion_join_restatement carries them)
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
