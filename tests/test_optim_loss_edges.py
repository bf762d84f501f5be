"""The three hand-written kernels every training step goes through, at their edges: mv3d_adam_step (csrc/adam.hip), mv3d_rpn_loss /
mv3d_rcnn_loss and mv3d_softmax_rows (csrc/losses.hip), and the two pinned staging buffers of the Python plumbing (optim.Adam's
tensor table, MV3D._stage_host_inputs).

One set of case tables feeds two things:
  1. unmarked tests: the f32 restatements of tests/optim_loss_restatement.py stay inside that module's derived error bounds against
     its f64 references, with a margin of 2 -- so the bounds are attainable by a correct f32 implementation;
  2. `-m gpu` tests: the kernels stay inside the same bounds against the same f64 references (never against the device or the
     library), every step reseeded from the kernel's own f32 state so that each assertion bounds ONE step.
Bit comparisons where the contract is exact: vector body against scalar loop, the 16-bit copies, repeatability, want_grad, the
workspace's contents.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import optim_loss_restatement as R

F32, F64 = np.float32, np.float64
CHUNK = 4096                      # ADAM_CHUNK
WG = 256                          # rows per workgroup of the loss and softmax kernels
MARGIN = 0.5                      # the f32 restatement must use at most half of every bound


# =================================================================== Adam: the case tables
ADAM_SIZES = (4097, 1, 8192, 3, 4095, 4096, 3 * CHUNK + 17)        # the 1-element tensor between two multi-chunk ones
ADAM_STEPS = (1, 2, 1000, 100000)
ADAM_BETAS = ((0.9, 0.999), (0.5, 0.9), (0.0, 0.0))
ADAM_EPS = (1e-8, 1e-3)
ADAM_LRS = (1e-5, 1e-3)
GRAD_SCALES = (1e-6, 1e-3, 1.0, 1e3)


def adam_hypers():
    return [dict(lr=lr, b1=b[0], b2=b[1], eps=e, t=t) for t, b, e, lr in itertools.product(ADAM_STEPS, ADAM_BETAS, ADAM_EPS, ADAM_LRS)]


def adam_state(sizes, seed):
    """[(p, g, m, v)] f32: tensor k's gradient at GRAD_SCALES[k % 4]; the moments of a run with gradients of that scale (a first
    moment of either sign against the gradient's: the lerp cancels in half of the elements), one element in 16 at the state of a
    first step (m = v = 0) and one in 16 with a zero gradient"""
    r = np.random.RandomState(seed)
    out = []
    for k, n in enumerate(sizes):
        s = GRAD_SCALES[k % len(GRAD_SCALES)]
        p = r.normal(0, 1, n)
        g = r.normal(0, s, n)
        m = r.normal(0, s, n) * r.choice([0.1, 1.0, 3.0], n)
        v = (r.normal(0, s, n) ** 2) * r.choice([0.01, 1.0, 10.0], n)
        first = r.randint(0, 16, n) == 0
        m[first] = 0.0
        v[first] = 0.0
        g[r.randint(0, 16, n) == 0] = 0.0
        out.append(tuple(a.astype(F32) for a in (p, g, m, v)))
    return out


def adam_worst(got, state, h):
    """the largest |got - f64| / bound over p, m, v of one tensor"""
    ref = R.adam_ref(*state, **h)
    bnd = R.adam_bound(*state, **h)
    return [float(np.max(np.abs(a.astype(F64) - b) / c)) for a, b, c in zip(got, ref, bnd)]


def test_adam_f32_restatement_meets_its_bound():
    worst = np.zeros(3)
    for i, h in enumerate(adam_hypers()):
        for st in adam_state((CHUNK + 17, 3, 1), seed=i):
            worst = np.maximum(worst, adam_worst(R.adam_f32(*st, **h), st, h))
    # (measured: p 0.498 -- half an ulp of p is reached --, m 0.357, v 0.394)
    assert (worst <= MARGIN).all(), worst


# the 16-bit copies: parameter values whose rounding is the test (g = 0, m = v = 0: the step leaves p as it is and writes its rounding)
def lowp_values():
    e = 2.0 ** -11                                                    # half an ulp of f16 at 1
    b = 2.0 ** -8                                                     # half an ulp of bf16 at 1
    vals = [1.0, 1 + e, 1 + 3 * e, 1 + e + 2.0 ** -23, 1 + e - 2.0 ** -23, -(1 + e), -(1 + 3 * e),          # f16 ties, and off them
            1 + b, 1 + 3 * b, 1 + b + 2.0 ** -23, 1 + b - 2.0 ** -23, -(1 + b), -(1 + 3 * b),               # bf16 ties
            65504.0, 65519.996, 65520.0, 65536.0, 1e5, -65520.0, -1e5, 3.0e38, -3.0e38,                     # f16 overflow to inf
            2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -25 * (1 + 2.0 ** -20), -(2.0 ** -24),
            2.0 ** -14, 2.0 ** -14 - 2.0 ** -26, 1023.5 * 2.0 ** -24, 2.0 ** -30,                            # f16 subnormals
            0.0, -0.0, float("nan"), float("inf"), float("-inf"), 0.1, -0.3, 3.14159274, 12345.678]
    return np.array(vals, F32)


def torch_lowp_bits(a, kind):
    """p.to(dtype) on the CPU, as bits"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(torch.float16 if kind == "f16" else torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def same_lowp_bits(got, want, kind):
    """bit for bit, except that any NaN matches any NaN: a NaN's bits are not part of the rounding (CPU torch itself writes 0x7FC0 from
    its scalar bfloat16 conversion and 0xFFFF from its vectorised one)"""
    exp, man = (0x7C00, 0x03FF) if kind == "f16" else (0x7F80, 0x007F)
    nan = lambda b: ((b & exp) == exp) & ((b & man) != 0)
    return bool(np.array_equal(nan(got), nan(want)) and np.array_equal(got[~nan(want)], want[~nan(want)]))


def test_lowp_values_hold_the_edges_they_claim():
    v = lowp_values()
    for kind in ("f16", "bf16"):                                                                      # two statements of one rounding
        assert same_lowp_bits(R.lowp_bits(v, kind), torch_lowp_bits(v, kind), kind)
        assert same_lowp_bits(R.lowp_bits(np.resize(v, 8229), kind), torch_lowp_bits(np.resize(v, 8229), kind), kind)
        assert not same_lowp_bits(R.lowp_bits(v, kind) ^ np.uint16(1), torch_lowp_bits(v, kind), kind)
    f16 = lambda x: int(R.lowp_bits(np.array([x], F32), "f16")[0])
    bf = lambda x: int(R.lowp_bits(np.array([x], F32), "bf16")[0])
    assert f16(1 + 2.0 ** -11) == 0x3C00 and f16(1 + 3 * 2.0 ** -11) == 0x3C02 and f16(1 + 2.0 ** -11 + 2.0 ** -23) == 0x3C01      # ties to even
    assert bf(1 + 2.0 ** -8) == 0x3F80 and bf(1 + 3 * 2.0 ** -8) == 0x3F82 and bf(1 + 2.0 ** -8 + 2.0 ** -23) == 0x3F81
    assert f16(65519.996) == 0x7BFF and f16(65520.0) == 0x7C00 and f16(-1e5) == 0xFC00
    assert f16(2.0 ** -24) == 1 and f16(2.0 ** -25) == 0 and f16(1.5 * 2.0 ** -24) == 2 and f16(2.5 * 2.0 ** -24) == 2
    assert f16(-0.0) == 0x8000 and bf(-0.0) == 0x8000 and f16(float("nan")) == 0x7E00 and bf(float("nan")) == 0x7FC0


# =================================================================== the losses: the case tables
def _logit_rows(r, rows, K):
    """N(0, 2) logits; every eighth row one of: differences of +-100 (expf underflows), all logits equal, magnitudes of 1e4"""
    z = r.normal(0, 2, (rows, K))
    pat = [lambda k: np.where(np.arange(K) == k % K, 50.0, -50.0), lambda k: np.where(np.arange(K) == k % K, -50.0, 50.0),
           lambda k: np.full(K, 7.5), lambda k: np.where(np.arange(K) == k % K, 1e4, -1e4),
           lambda k: np.where(np.arange(K) == k % K, 9999.5, 1e4), lambda k: -1e4 + 3.0 * (np.arange(K) == k % K),
           lambda k: np.where(np.arange(K) == k % K, 8.0, -8.0)]
    for i in range(0, rows, 8 if rows > 8 else 1):
        z[i] = pat[(i // 8 if rows > 8 else i) % len(pat)](i)
    return z.astype(F32)


def rpn_case(rows, sigma, seed):
    r = np.random.RandomState(seed)
    lab = np.full(rows, -1, F32)
    pick = r.rand(rows) < 0.3
    lab[pick] = r.randint(0, 2, int(pick.sum()))
    for i, e in enumerate(sorted({0, rows - 1} | {b for b in range(0, rows, WG)} | {b - 1 for b in range(WG, rows + 1, WG)})):
        lab[e] = 1 if i % 2 == 0 else 0                               # first and last row of every workgroup selected
    z = _logit_rows(r, rows, 2)
    return z, lab, r.normal(0, 0.3, (rows, 6)).astype(F32), r.normal(0, 0.3, (rows, 6)).astype(F32), sigma, True


def rcnn_case(S, K, D, sigma, seed):
    r = np.random.RandomState(seed)
    z = _logit_rows(r, S, K)
    lab = r.randint(0, K, S).astype(np.int32)
    tgt = (r.normal(0, 0.5, (S, D)) * (r.rand(S, D) < 0.5)).astype(F32)
    return z, lab, r.normal(0, 0.5, (S, D)).astype(F32), tgt, sigma, False


RPN_ROWS = (1, 255, 256, 257, 512, 513)
RCNN_SHAPES = ((1, 2, 48), (128, 2, 48), (37, 4, 96), (257, 21, 84))


def boundary_values(sigma):
    """x at +-thr, one f32 towards 0 and one away from it, and 0; thr = f32(1) / f32(sigma^2)"""
    thr = F32(1) / F32(sigma * sigma)
    xs = []
    for s in (F32(1), F32(-1)):
        t = F32(s * thr)
        xs += [t, np.nextafter(t, F32(0)), np.nextafter(t, F32(s * np.inf))]
    return np.array(xs + [F32(0)], F32)


def boundary_case(sigma):
    """one RCNN row of 48 columns: every boundary value three times, as pred - 0, as 0 - (-x) and as x/2 - (-x/2): each f32 difference
    IS the value; the other columns have pred == tgt"""
    xs = boundary_values(sigma)
    r = np.random.RandomState(3)
    pred = r.normal(0, 0.5, (1, 48)).astype(F32)
    tgt = pred.copy()
    want = np.zeros(48, F32)
    for i, x in enumerate(xs):
        pred[0, 3 * i], tgt[0, 3 * i] = x, 0
        pred[0, 3 * i + 1], tgt[0, 3 * i + 1] = 0, -x
        pred[0, 3 * i + 2], tgt[0, 3 * i + 2] = x / F32(2), -x / F32(2)
        want[3 * i:3 * i + 3] = x
    assert np.array_equal(pred[0] - tgt[0], want)
    return np.array([[0.5, -0.25]], F32), np.array([1], np.int32), pred, tgt, sigma, False


def single_value_case(x, sigma):
    """one row whose box loss is smoothL1(x) alone (the other 47 differences are 0): the f32 value tells the branch taken"""
    pred = np.zeros((1, 48), F32)
    pred[0, 5] = x
    return np.array([[0.5, -0.25]], F32), np.array([1], np.int32), pred, np.zeros((1, 48), F32), sigma, False


def loss_cases():
    cases = {}
    for i, rows in enumerate(RPN_ROWS):
        for sigma in (3.0, 1.0):
            cases["rpn-%d-s%d" % (rows, sigma)] = rpn_case(rows, sigma, 10 + i)
    for i, (S, K, D) in enumerate(RCNN_SHAPES):
        for sigma in (3.0, 1.0):
            cases["rcnn-%dx%dx%d-s%d" % (S, K, D, sigma)] = rcnn_case(S, K, D, sigma, 30 + i)
    for sigma in (3.0, 1.0):
        cases["boundary-s%d" % sigma] = boundary_case(sigma)
    z, lab, pred, tgt, _, _ = rcnn_case(37, 4, 96, 3.0, 50)
    lab = lab.copy()
    lab[5], lab[9] = 4, -1                                            # labels outside 0 .. K-1
    cases["rcnn-bad-label"] = (z, lab, pred, tgt, 3.0, False)
    return cases


def loss_worst(got, case):
    """the largest |got - f64| / bound over (ce, box, d_cls, d_pred); NaN where the reference is NaN must be NaN in `got`"""
    losses, d_cls, d_pred = got
    ref = R.loss_ref(*case)
    b_ce, b_box, b_dc, b_dp = R.loss_bound(*case)
    out = []
    for g, w, b in ((losses[0], ref["ce"], b_ce), (losses[1], ref["box"], b_box)):
        if np.isnan(w):
            assert np.isnan(g)
            out.append(0.0)
        else:
            out.append(abs(float(g) - w) / b)
    for g, w, b in ((d_cls, ref["d_cls"], b_dc), (d_pred, ref["d_pred"], b_dp)):
        assert g.shape == w.shape and np.isfinite(g).all()
        err = np.abs(g.astype(F64) - w)
        assert (err[b == 0] == 0).all()                               # rows outside the selection: exactly zero
        out.append(float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0))) if g.size else 0.0)
    return out


def outer_contract(got, case):
    """the project's stated contract (csrc/losses.hip): 1e-5 relative against the reference.  Absolute terms: eps32 on a value (an
    f32 logsumexp cannot resolve a row's loss below one ulp of 1) and eps32 / n_selected on a gradient (softmax - 1 at a confident label)"""
    losses, d_cls, d_pred = got
    ref = R.loss_ref(*case)
    for g, w in ((losses[0], ref["ce"]), (losses[1], ref["box"])):
        assert (np.isnan(g) and np.isnan(w)) or abs(float(g) - w) <= 1e-5 * abs(w) + R.EPS32, (g, w)
    assert np.allclose(d_cls, ref["d_cls"], rtol=1e-5, atol=R.EPS32 / max(ref["n_ce"], 1))
    assert np.allclose(d_pred, ref["d_pred"], rtol=1e-5, atol=R.EPS32 / max(ref["n_box"], 1))


def test_loss_f32_restatement_meets_its_bound():
    worst = np.zeros(4)
    for name, case in loss_cases().items():
        got = R.loss_f32(*case)
        worst = np.maximum(worst, loss_worst(got, case))
        outer_contract(got, case)
    assert (worst <= MARGIN).all(), worst


def test_loss_restatement_selection_rules():
    """no positive row: box loss NaN, zero box gradient; nothing selected: both NaN, both gradients zero; the reference and the f32
    restatement state the same rules"""
    for rows in (1, 256):
        z, lab, pred, tgt, sigma, _ = rpn_case(rows, 3.0, 70)
        for labels, ce_nan in ((np.where(lab == 1, 0, lab).astype(F32), False), (np.full(rows, -1, F32), True)):
            ref = R.loss_ref(z, labels, pred, tgt, sigma, True)
            losses, d_cls, d_pred = R.loss_f32(z, labels, pred, tgt, sigma, True)
            assert np.isnan(ref["box"]) and np.isnan(losses[1]) and np.isnan(ref["ce"]) == ce_nan == bool(np.isnan(losses[0]))
            assert not ref["d_pred"].any() and not d_pred.any()
            assert bool(ref["d_cls"].any()) == bool(d_cls.any()) == (not ce_nan)


STRICT_SIGMA = 0.7                # a sigma at which `<` and `<=` differ in f32 at |x| = thr (they do not at 3 and 1)


def test_boundary_value_is_linear_and_one_sigma_can_tell():
    """|x| == thr is NOT quadratic (train_mv.py:83: `<`).  smoothL1 and its derivative are continuous there, and at sigma = 3 and 1 (and
    every other sigma tried but 0.7) both branches give the same f32 BITS at x = thr, value and gradient: no test can tell `<` from `<=`
    at the reference's sigmas.  At sigma = 0.7 the quadratic gradient f32(sigma^2) * thr is one ulp short of the linear branch's 1.0;
    the gpu test pins the strict comparison there"""
    for sigma in (3.0, 1.0, STRICT_SIGMA):
        s2 = F32(F32(sigma) * F32(sigma))
        thr = F32(1) / s2
        assert thr - F32(0.5) / s2 == (thr * thr) * (F32(0.5) * s2)
        assert (s2 * thr != F32(1)) == (sigma == STRICT_SIGMA)
        for x in (thr, -thr):
            _, _, d_pred = R.loss_f32(*single_value_case(x, sigma))
            assert d_pred[0, 5] == np.sign(x)


# =================================================================== softmax: the case table
SOFTMAX_SHAPES = ((1, 2), (255, 2), (256, 2), (257, 2), (3, 1), (5, 3), (2, 1024))


def softmax_case(rows, K, special):
    """uniform(-30, 30) logits.  `special` (needs 5 rows): row 1 differences beyond +-88, row 2 a -inf entry among finite ones (K > 1),
    row 3 all -inf, and per variant row 0 or the last row holding +inf / NaN -- their neighbours must come out intact"""
    r = np.random.RandomState(rows * 1031 + K)
    x = r.uniform(-30, 30, (rows, K)).astype(F32)
    if rows == 2:
        x[0, ::7] = -100.0; x[0, 3] = 95.0; x[0, 5] = -np.inf          # differences beyond 88 either way, a -inf entry
    if special is not None and rows >= 5:
        x[1] = -100.0; x[1, 0] = 100.0
        if K > 1:
            x[2, K - 1] = -np.inf
        x[3] = -np.inf
        x[0 if special == "inf" else rows - 1, 0] = np.inf if special == "inf" else np.nan
    return x


def softmax_cases():
    out = {}
    for rows, K in SOFTMAX_SHAPES:
        for special in ((None,) if rows < 5 else (None, "inf", "nan")):
            out["%dx%d-%s" % (rows, K, special)] = softmax_case(rows, K, special)
    k1 = np.array([[0.5], [-np.inf], [np.inf], [np.nan], [-3e38], [7.0]], F32)
    out["6x1-specials"] = k1
    return out


def softmax_check(got, x):
    """-> the largest use of the bound; NaN rows exactly where the reference has them, 0 exactly where the logit is -inf, row sums"""
    ref, bnd = R.softmax_ref(x), R.softmax_bound(x)
    assert got.shape == ref.shape and got.dtype == F32
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    nanrow = np.isnan(ref).any(-1)
    assert np.array_equal(np.isnan(ref).all(-1), nanrow)               # a NaN row is NaN throughout, its neighbours not at all
    ok = ~nanrow
    assert (got[ok][np.isneginf(x[ok])] == 0).all()
    K = x.shape[-1]
    assert (np.abs(got[ok].astype(F64).sum(-1) - 1.0) <= K * R.EPS32).all()
    err = np.abs(got[ok].astype(F64) - ref[ok]) / bnd[ok]
    return float(err.max()) if err.size else 0.0


def test_softmax_f32_restatement_meets_its_bound():
    worst, seen_nan = 0.0, 0
    for name, x in softmax_cases().items():
        worst = max(worst, softmax_check(R.softmax_f32(x), x))
        seen_nan += int(np.isnan(R.softmax_ref(x)).any())
    assert worst <= MARGIN and seen_nan >= 9, (worst, seen_nan)


# =================================================================== the device
@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import _lib, ops, optim
    return dict(torch=torch, ops=ops, lib=_lib, optim=optim)


def dev(torch, a):
    return torch.as_tensor(np.array(a, order="C")).cuda()


def host(t):
    return t.detach().cpu().numpy()


class Flat:
    """a device buffer of n + 8 elements and the view of n elements at element offset `off` (0: the allocation's own 256-byte
    alignment; 1 .. 3: a view no vector access may touch); the elements outside the view hold a sentinel"""

    def __init__(self, torch, values, off, dtype=None, sentinel=777.0):
        values = np.asarray(values)
        self.n, self.off = values.size, off
        self.buf = torch.full((self.n + 8,), sentinel, dtype=dtype or torch.float32, device="cuda")
        self.view = self.buf[off:off + self.n]
        if dtype is None:
            self.view.copy_(torch.as_tensor(np.ascontiguousarray(values.reshape(-1))))
        self.sentinel = sentinel
        assert self.view.numel() == self.n and self.buf.data_ptr() % 256 == 0

    def get(self):
        return host(self.view)

    def untouched_outside(self):
        b = host(self.buf.float())
        return (b[:self.off] == self.sentinel).all() and (b[self.off + self.n:] == self.sentinel).all()


def adam_launch(gpu, tensors, h, lowp=0):
    """one mv3d_adam_step over `tensors` = [(p, g, m, v, lowp view or None)] device views of equal numel per tuple, tables built as
    optim.py builds them; synchronises (the tables are temporaries) and returns the status"""
    torch, L = gpu["torch"], gpu["lib"]
    arr = (L.AdamTensor * len(tensors))()
    ct, cf = [], []
    for k, (p, g, m, v, lp) in enumerate(tensors):
        n = p.numel()
        assert g.numel() == m.numel() == v.numel() == n and (lp is None or lp.numel() == n)
        assert all(a.dtype == torch.float32 and a.is_contiguous() and a.is_cuda for a in (p, g, m, v))
        arr[k] = L.AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lp.data_ptr() if lp is not None else None)
        c = (n + CHUNK - 1) // CHUNK
        ct.append(np.full(c, k, np.int32)); cf.append(np.arange(c, dtype=np.int32))
    assert L.lib().mv3d_adam_chunk_elements() == CHUNK
    t_dev = dev(torch, np.frombuffer(bytes(arr), np.uint8))
    ct_dev, cf_dev = dev(torch, np.concatenate(ct)), dev(torch, np.concatenate(cf))
    st = L.lib().mv3d_adam_step(C.c_void_p(t_dev.data_ptr()), C.c_void_p(ct_dev.data_ptr()), C.c_void_p(cf_dev.data_ptr()),
                                int(ct_dev.numel()), h["lr"], h["b1"], h["b2"], h["eps"], h["t"], lowp,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st


def adam_run(gpu, state, h, offs=(0, 0, 0, 0), lowp=0, lowp_off=None):
    """state [(p, g, m, v)] numpy -> the step's (p, m, v) per tensor (and the 16-bit copy's bits); offs: element offsets of p, g, m, v"""
    torch = gpu["torch"]
    flats = [[Flat(torch, a, o) for a, o in zip(st, offs)] for st in state]
    lps = None
    if lowp:
        dt = torch.float16 if lowp == 1 else torch.bfloat16
        lps = [Flat(torch, st[0], lowp_off, dtype=dt, sentinel=3.0) for st in state]
    assert adam_launch(gpu, [tuple(f.view for f in fl) + ((lps[k].view if lps else None),) for k, fl in enumerate(flats)], h, lowp) == 0
    for k, fl in enumerate(flats):
        assert all(f.untouched_outside() for f in fl), "wrote outside a tensor"
        assert np.array_equal(fl[1].get().view(np.uint32), state[k][1].view(np.uint32)), "the gradient was written"
        assert lps is None or lps[k].untouched_outside(), "wrote outside a 16-bit copy"
    out = [(fl[0].get(), fl[2].get(), fl[3].get()) for fl in flats]
    if lps:
        return out, [host(l.view.view(torch.int16)).view(np.uint16) for l in lps]
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
def test_adam_every_size_step_and_hyper_parameter_against_f64(gpu):
    """all sizes in one launch (only full chunks, a tail of 1 / 17 / 4095, one chunk short by one, 1 and 3 elements, the single
    element between two multi-chunk tensors), for t x betas x eps x lr, gradient scales 1e-6 .. 1e3 across the tensors"""
    worst = np.zeros(3)
    for i, h in enumerate(adam_hypers()):
        state = adam_state(ADAM_SIZES, seed=1000 + i)
        for st, got in zip(state, adam_run(gpu, state, h)):
            w = adam_worst(got, st, h)
            assert max(w) <= 1.0, (h, st[0].size, w)
            worst = np.maximum(worst, w)
    print("adam: worst use of the f64 bounds (p, m, v):", worst)


@pytest.mark.gpu
def test_adam_vector_body_and_scalar_loop_agree_bit_for_bit(gpu):
    """the same values at element offset 0 (16-byte aligned: the vector body on full chunks) and at element offset 1 of the
    parameter alone, the gradient alone, the moments alone, all four (the scalar loop on full chunks)"""
    h = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, t=3)
    state = adam_state((2 * CHUNK + 17, CHUNK, 2 * CHUNK), seed=7)
    base = adam_run(gpu, state, h)
    for st, got in zip(state, base):
        assert max(adam_worst(got, st, h)) <= 1.0
    for offs in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 1), (1, 1, 1, 1), (2, 0, 3, 1)):
        for k, (a, b) in enumerate(zip(base, adam_run(gpu, state, h, offs=offs))):
            for name, x, y in zip("pmv", a, b):
                assert np.array_equal(bits(x), bits(y)), (offs, k, name, int((bits(x) != bits(y)).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_adam_16_bit_copy_is_the_rounded_parameter(gpu, kind):
    """destination at element offsets 0 (8-byte stores), 1 .. 3 (the 2-byte fallback), full chunks and a tail chunk; the parameter
    aligned (vector body) and not (scalar loop).  g = 0, m = v = 0 leaves p as it is: the copy is p's rounding -- ties, f16 overflow
    and subnormals, +-0, NaN.  Then one ordinary step: the copy is the rounding of the parameter the kernel wrote."""
    code = 1 if kind == "f16" else 2
    h = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, t=1)
    vals = lowp_values()
    n = 2 * CHUNK + 37
    p = np.resize(vals, n).astype(F32)                                 # the values cycle through both full chunks and the tail
    p[-len(vals):] = vals
    zero = np.zeros(n, F32)
    want = torch_lowp_bits(p, kind)
    assert same_lowp_bits(R.lowp_bits(p, kind), want, kind)
    r = np.random.RandomState(5)
    step = [(r.normal(0, 1, n).astype(F32), r.normal(0, 1, n).astype(F32), np.zeros(n, F32), np.zeros(n, F32))]
    for lowp_off in (0, 1, 2, 3):
        for offs in ((0, 0, 0, 0), (1, 0, 0, 0)):
            out, lp = adam_run(gpu, [(p, zero, zero, zero)], h, offs=offs, lowp=code, lowp_off=lowp_off)
            assert np.array_equal(bits(out[0][0]), bits(p)), "g = 0 must leave the parameter as it is"
            assert same_lowp_bits(lp[0], want, kind), (kind, lowp_off, offs, np.flatnonzero(lp[0] != want)[:8])
            out, lp = adam_run(gpu, step, h, offs=offs, lowp=code, lowp_off=lowp_off)
            assert max(adam_worst(out[0], step[0], h)) <= 1.0
            assert np.array_equal(lp[0], torch_lowp_bits(out[0][0], kind))


@pytest.mark.gpu
def test_adam_non_finite_gradients(gpu):
    """a NaN gradient in one lane of a 16-byte piece poisons that element only.  Huge gradients: whatever a CPU f32
    torch.optim.Adam(foreach=False) gives.  |g| = 1e30 overflows (1 - beta2) g g in f32: v = inf, p unchanged (f64 does not overflow
    there: no f64 reference); |g| = 1e20 overflows g * g alone but not ((1 - beta2) g) g, the order of torch and of the kernel: finite"""
    torch = gpu["torch"]
    h = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, t=1)
    state = adam_state((CHUNK, 100), seed=11)
    for st in state:
        st[1][[5, st[1].size - 2]] = np.nan
    for st, got in zip(state, adam_run(gpu, state, h)):
        hit = np.isnan(st[1])
        ref, bnd = R.adam_ref(*st, **h), R.adam_bound(*st, **h)
        for a, b, c in zip(got, ref, bnd):
            assert np.isnan(a[hit]).all() and np.isfinite(a[~hit]).all()
            assert (np.abs(a[~hit].astype(F64) - b[~hit]) <= c[~hit]).all()
    n = CHUNK + 9
    r = np.random.RandomState(12)
    p0 = r.normal(0, 1, n).astype(F32)
    g = r.normal(0, 1, n).astype(F32)
    big = np.arange(n) % 3 == 0
    g[big] = np.where(np.arange(n)[big] % 2 == 0, 1e30, -1e30)
    mid = np.arange(n) % 3 == 1
    g[mid] = np.where(np.arange(n)[mid] % 2 == 0, 1e20, -1e20)
    pt = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], foreach=False)
    pt.grad = torch.from_numpy(g.copy())
    opt.step()
    want_p, want_m, want_v = pt.detach().numpy(), opt.state[pt]["exp_avg"].numpy(), opt.state[pt]["exp_avg_sq"].numpy()
    assert np.isinf(want_v[big]).all() and np.array_equal(want_p[big], p0[big])
    (gp, gm, gv), = adam_run(gpu, [(p0, g, np.zeros(n, F32), np.zeros(n, F32))], h)
    assert np.array_equal(bits(gp[big]), bits(p0[big])) and np.array_equal(bits(gv[big]), bits(want_v[big]))
    assert np.allclose(gm, want_m, rtol=4 * R.EPS32, atol=0)
    assert np.isfinite(want_v[mid]).all() and (np.abs(want_p[mid] - p0[mid]) > 0.5 * h["lr"]).all()      # 1e20: an ordinary step
    assert np.isfinite(gv[~big]).all() and np.allclose(gv[~big], want_v[~big], rtol=4 * R.EPS32, atol=0)
    assert np.allclose(gp[~big], want_p[~big], rtol=1e-6, atol=1e-6)


@pytest.mark.gpu
def test_adam_refusals(gpu):
    torch, L = gpu["torch"], gpu["lib"]
    t = [torch.zeros(8, device="cuda") for _ in range(4)]
    arr = (L.AdamTensor * 1)(L.AdamTensor(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), 8, None))
    tab = dev(torch, np.frombuffer(bytes(arr), np.uint8))
    z = torch.zeros(1, dtype=torch.int32, device="cuda")
    P = lambda x: C.c_void_p(x.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda a, b, c, n=1, b1=0.9, b2=0.999, step=1, lowp=0: L.lib().mv3d_adam_step(a, b, c, n, 1e-3, b1, b2, 1e-8, step, lowp, s)
    assert call(P(tab), P(z), P(z), step=0) == L.ERR_INVALID_ARG
    assert call(P(tab), P(z), P(z), b1=1.0) == L.ERR_INVALID_ARG and call(P(tab), P(z), P(z), b2=1.0) == L.ERR_INVALID_ARG
    assert call(P(tab), P(z), P(z), lowp=3) == L.ERR_INVALID_ARG
    assert call(None, P(z), P(z)) == L.ERR_INVALID_ARG and call(P(tab), None, P(z)) == L.ERR_INVALID_ARG
    assert call(P(tab), P(z), None) == L.ERR_INVALID_ARG
    assert call(P(tab), P(z), P(z), n=0) == L.OK
    torch.cuda.synchronize()
    assert all(float(x.abs().sum()) == 0.0 for x in t)                 # none of these calls ran a step


@pytest.mark.gpu
def test_adam_update_and_moments_against_f64(gpu):
    """optim.Adam on the shapes of test_train_entry.py::test_adam_step_kernel_equals_torch_adam, gradient scales 1e-2 .. 1e2: that test
    sees the parameter to 1e-6, so a 1e-3 update to 0.1 %.  Here p_new - p_old and both moments of every step against one f64 step
    from the kernel's own previous f32 state"""
    torch = gpu["torch"]
    g = torch.Generator().manual_seed(0)
    shapes = [(3,), (64, 9, 3, 3), (4096 * 3 + 17,), (513, 257), (1,)]
    ps = [torch.randn(s, generator=g).cuda().requires_grad_(True) for s in shapes]
    opt = gpu["optim"].Adam(ps, lr=1e-3)
    worst = np.zeros(3)
    for it in range(6):
        before = []
        for k, x in enumerate(ps):
            if k == 4 and it < 2:                                     # the last tensor joins at the third step
                x.grad = None
                before.append(None)
                continue
            x.grad = torch.randn(x.shape, generator=g).cuda() * (10.0 ** (k - 2))
            st = opt.state.get(x, {})
            z = np.zeros(x.numel(), F32)
            before.append((host(x).reshape(-1).copy(), host(x.grad).reshape(-1), host(st["exp_avg"]).reshape(-1).copy() if st else z,
                           host(st["exp_avg_sq"]).reshape(-1).copy() if st else z, int(float(st["step"])) + 1 if st else 1))
        opt.step()
        for x, b in zip(ps, before):
            if b is None:
                continue
            h = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, t=b[4])
            st = opt.state[x]
            got = (host(x).reshape(-1), host(st["exp_avg"]).reshape(-1), host(st["exp_avg_sq"]).reshape(-1))
            ref, bnd = R.adam_ref(*b[:4], **h), R.adam_bound(*b[:4], **h)
            upd, upd_ref = got[0].astype(F64) - b[0].astype(F64), ref[0] - b[0].astype(F64)
            assert (np.abs(upd - upd_ref) <= bnd[0]).all(), (it, x.shape)
            w = adam_worst(got, b[:4], h)
            assert max(w) <= 1.0, (it, x.shape, w)
            worst = np.maximum(worst, w)
    print("optim.Adam: worst use of the f64 bounds (p, m, v):", worst)


# ------------------------------------------------------------------- the losses
def run_loss(gpu, case, want_grad=True):
    torch, ops = gpu["torch"], gpu["ops"]
    z, lab, pred, tgt, sigma, rpn = case
    fn = ops.rpn_loss if rpn else ops.rcnn_loss
    losses, d_cls, d_pred = fn(dev(torch, z), dev(torch, lab), dev(torch, pred), dev(torch, tgt), sigma=sigma, want_grad=want_grad)
    return (host(losses),) + ((host(d_cls), host(d_pred)) if want_grad else (None, None))


@pytest.mark.gpu
def test_losses_every_case_against_f64(gpu):
    """row counts around the 256-row workgroup with the first and last row of every workgroup selected, the RCNN shapes, logits whose
    differences underflow expf / are all equal / have magnitudes of 1e4, sigma 3 and 1, both sides of |x| = 1 / sigma^2, labels out
    of range: the derived bound, the 1e-5 contract, bitwise repeatability and want_grad=False on every case"""
    worst = np.zeros(4)
    for name, case in loss_cases().items():
        got = run_loss(gpu, case)
        w = loss_worst(got, case)
        assert max(w) <= 1.0, (name, w)
        worst = np.maximum(worst, w)
        outer_contract(got, case)
        again = run_loss(gpu, case)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, again)), name
        assert np.array_equal(run_loss(gpu, case, want_grad=False)[0].view(np.uint32), got[0].view(np.uint32)), name
    print("losses: worst use of the f64 bounds (ce, box, d_cls, d_pred):", worst)


@pytest.mark.gpu
def test_smooth_l1_boundary_is_not_quadratic(gpu):
    """x = +-thr takes the linear branch: the gradient is exactly +-1, at sigma = 0.7 one ulp away from what the quadratic branch gives
    (see test_boundary_value_is_linear_and_one_sigma_can_tell); one f32 inside the threshold is quadratic.  Rows with this single
    difference, so the f32 results are the branch's own bits"""
    for sigma in (3.0, 1.0, STRICT_SIGMA):
        s2 = F32(F32(sigma) * F32(sigma))
        thr = F32(1) / s2
        for x in (thr, -thr):
            case = single_value_case(x, sigma)
            losses, _, d_pred = run_loss(gpu, case)
            assert losses[1].view(np.uint32) == (thr - F32(0.5) / s2).view(np.uint32) == R.loss_f32(*case)[0][1].view(np.uint32)
            assert d_pred[0, 5] == np.sign(x) and not np.delete(d_pred[0], 5).any(), (sigma, x, d_pred[0, 5])
        x = np.nextafter(thr, F32(0))
        losses, _, d_pred = run_loss(gpu, single_value_case(x, sigma))
        assert losses[1].view(np.uint32) == ((x * x) * (F32(0.5) * s2)).view(np.uint32)
        assert d_pred[0, 5] == s2 * x


@pytest.mark.gpu
def test_loss_selection_rules_at_1_and_256_rows(gpu):
    """no positive row: box loss NaN, zero box gradient, the cross-entropy and its gradient live; nothing selected: both NaN, both zero"""
    for rows in (1, 256):
        z, lab, pred, tgt, sigma, _ = rpn_case(rows, 3.0, 70)
        no_pos = (z, np.where(lab == 1, 0, lab).astype(F32), pred, tgt, sigma, True)
        losses, d_cls, d_pred = got = run_loss(gpu, no_pos)
        assert np.isfinite(losses[0]) and np.isnan(losses[1]) and d_cls.any() and not d_pred.any()
        assert max(loss_worst(got, no_pos)) <= 1.0
        none = (z, np.full(rows, -1, F32), pred, tgt, sigma, True)
        losses, d_cls, d_pred = run_loss(gpu, none)
        assert np.isnan(losses).all() and not d_cls.any() and not d_pred.any()
        assert np.array_equal(d_cls.view(np.uint32), np.zeros_like(d_cls).view(np.uint32))           # +0, not -0 or NaN * 0


@pytest.mark.gpu
def test_rcnn_label_out_of_range(gpu):
    """cross-entropy NaN; the box loss untouched; that row's d_cls is the plain softmax over the count; no other gradient changes"""
    bad = loss_cases()["rcnn-bad-label"]
    z, lab, pred, tgt, sigma, _ = bad
    good_lab = lab.copy()
    good_lab[[5, 9]] = 0
    l_bad, dc_bad, dp_bad = run_loss(gpu, bad)
    l_ok, dc_ok, dp_ok = run_loss(gpu, (z, good_lab, pred, tgt, sigma, False))
    assert np.isnan(l_bad[0]) and l_bad[1].view(np.uint32) == l_ok[1].view(np.uint32)
    assert np.array_equal(dp_bad.view(np.uint32), dp_ok.view(np.uint32))
    others = np.setdiff1d(np.arange(len(lab)), [5, 9])
    assert np.array_equal(dc_bad[others].view(np.uint32), dc_ok[others].view(np.uint32))
    soft = R.softmax_ref(z) / len(lab)
    bnd = R.loss_bound(*bad)[2]
    assert (np.abs(dc_bad[[5, 9]].astype(F64) - soft[[5, 9]]) <= bnd[[5, 9]]).all() and (dc_bad[[5, 9]] > 0).all()


@pytest.mark.gpu
def test_loss_workspace_contract(gpu):
    """a workspace full of 0xFF bytes gives the bits of a clean one; one byte short or misaligned: MV3D_ERR_WORKSPACE; the size covers
    every workgroup's partials"""
    torch, L = gpu["torch"], gpu["lib"]
    lib = L.lib()
    for rows in RPN_ROWS + (23104,):
        assert lib.mv3d_loss_workspace_bytes(rows) >= ((rows + WG - 1) // WG) * 4 * 8
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda x: C.c_void_p(x.data_ptr())
    for rows in (255, 513):
        case = rpn_case(rows, 3.0, 90)
        z, lab, pred, tgt = (dev(torch, a) for a in case[:4])
        want = run_loss(gpu, case)
        need = lib.mv3d_loss_workspace_bytes(rows)
        ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
        assert ws.data_ptr() % 256 == 0
        out = torch.empty(2, device="cuda"), torch.empty_like(z), torch.empty_like(pred)
        call = lambda w, nbytes: lib.mv3d_rpn_loss(P(z), P(lab), P(pred), P(tgt), rows, C.c_float(3.0), P(out[0]), P(out[1]), P(out[2]),
                                                   C.c_void_p(w), nbytes, s)
        assert call(ws.data_ptr(), need) == L.OK
        torch.cuda.synchronize()
        assert all(np.array_equal(host(a).view(np.uint32), b.view(np.uint32)) for a, b in zip(out, want))
        assert (host(ws[need:]) == 0xFF).all()                          # nothing written past the stated size
        assert call(ws.data_ptr(), need - 1) == L.ERR_WORKSPACE
        assert call(ws.data_ptr() + 8, need) == L.ERR_WORKSPACE and call(ws.data_ptr() + 128, need) == L.ERR_WORKSPACE
        assert call(None, need) == L.ERR_WORKSPACE
        torch.cuda.synchronize()


# ------------------------------------------------------------------- softmax
@pytest.mark.gpu
def test_softmax_rows_every_case_against_f64(gpu):
    """the shapes at the `classes` limits and around the 256-row workgroup; differences beyond +-88, -inf entries (probability 0), rows
    of -inf only / holding +inf / holding NaN (NaN rows) with intact neighbours; f64 with the derived bound, row sums within K eps32"""
    torch, ops = gpu["torch"], gpu["ops"]
    worst = 0.0
    for name, x in softmax_cases().items():
        w = softmax_check(host(ops.softmax_rows(dev(torch, x))), x)
        assert w <= 1.0, (name, w)
        worst = max(worst, w)
    print("softmax: worst use of the f64 bound:", worst)


@pytest.mark.gpu
def test_softmax_rows_refusals(gpu):
    """classes 0 and 1025; a pointer that is 4-byte but not 8-byte aligned, for EVERY K (the K = 2 body loads float2; the contract is
    stated once for all K); rows = 0 is OK and writes nothing"""
    torch, ops, L = gpu["torch"], gpu["ops"], gpu["lib"]
    lib = L.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.zeros(4096, device="cuda")
    y = torch.full((4096,), 5.0, device="cuda")
    call = lambda a, b, rows, K: lib.mv3d_softmax_rows(C.c_void_p(a), C.c_void_p(b), rows, K, s)
    assert call(x.data_ptr(), y.data_ptr(), 2, 0) == L.ERR_INVALID_ARG and call(x.data_ptr(), y.data_ptr(), 2, 1025) == L.ERR_INVALID_ARG
    assert call(x.data_ptr(), y.data_ptr(), -1, 2) == L.ERR_INVALID_ARG
    assert call(None, y.data_ptr(), 2, 2) == L.ERR_INVALID_ARG and call(x.data_ptr(), None, 2, 2) == L.ERR_INVALID_ARG
    for K in (1, 2, 3, 1024):
        assert call(x.data_ptr() + 4, y.data_ptr(), 2, K) == L.ERR_INVALID_ARG
        assert call(x.data_ptr(), y.data_ptr() + 4, 2, K) == L.ERR_INVALID_ARG
        view = x[1:1 + 2 * K].view(2, K)
        assert view.is_contiguous() and view.data_ptr() % 8 == 4
        with pytest.raises(L.Mv3dError):
            ops.softmax_rows(view)
        assert call(x.data_ptr() + 8, y.data_ptr() + 8, 2, K) == L.OK   # 8-byte aligned is enough
    assert call(x.data_ptr(), y.data_ptr(), 0, 2) == L.OK
    torch.cuda.synchronize()
    yh = host(y)
    assert (yh[0] == 5.0) and (yh[2 + 2 * 1024:] == 5.0).all()          # only the accepted calls wrote, inside their rows


# ------------------------------------------------------------------- staging run-ahead
class Delay:
    """puts the device behind the host with harmless work: a chain of large f32 matmuls on the current stream (about 100 ms), an event
    after it.  The host calls under test run while the chain does; `still_running` is what makes the test mean something"""

    def __init__(self, torch, n=8192, links=16):
        self.torch = torch
        self.a = torch.randn(n, n, device="cuda") * (1.0 / n ** 0.5)
        self.b = self.a.clone()
        torch.mm(self.a, self.a, out=self.b)                            # (the BLAS handle and its workspace: not inside the timed part)
        torch.cuda.synchronize()
        self.links, self.ev = links, torch.cuda.Event()

    def start(self):
        for _ in range(self.links):
            self.torch.mm(self.a, self.a, out=self.b)
        self.ev.record()

    def require_still_running(self):
        assert not self.ev.query(), "the device caught up with the host before the calls returned: lengthen the matmul chain"


@pytest.mark.gpu
def test_adam_tensor_table_survives_host_run_ahead(gpu):
    """two optim.Adam steps back to back with different live gradient tensors (the table is refilled both times) while the device is
    still busy: each launch must read ITS OWN table.  With one pinned buffer rewritten in place the first launch ran on the second
    step's gradient pointers: off by about 2 lr per element"""
    torch = gpu["torch"]
    r = np.random.RandomState(21)
    shapes = [(3000,), (CHUNK + 5,), (7,)]
    p0 = [r.normal(0, 1, s).astype(F32) for s in shapes]
    ps = [dev(torch, a).requires_grad_(True) for a in p0]
    opt = gpu["optim"].Adam(ps, lr=1e-3)
    h = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
    g0 = [r.normal(0, 1, s).astype(F32) for s in shapes]
    gA = [r.normal(0, 1, s).astype(F32) for s in shapes]
    d0, dA, dB = [dev(torch, a) for a in g0], [dev(torch, a) for a in gA], [dev(torch, -a) for a in gA]   # all alive to the end
    for x, g in zip(ps, d0):
        x.grad = g
    opt.step()                                                         # the state, the chunk tables and the pinned buffers: made here
    torch.cuda.synchronize()
    start = [(host(x).copy(), host(opt.state[x]["exp_avg"]).copy(), host(opt.state[x]["exp_avg_sq"]).copy()) for x in ps]
    delay = Delay(torch)
    delay.start()
    for grads in (dA, dB):
        for x, g in zip(ps, grads):
            x.grad = g
        opt.step()
    delay.require_still_running()
    torch.cuda.synchronize()
    for x, (p, m, v), a in zip(ps, start, gA):
        bound = [np.zeros(p.shape) for _ in range(3)]
        for t, g in ((2, a), (3, -a)):
            bnd = R.adam_bound(p, g, m, v, t=t, **h)
            pr, mr, vr = R.adam_ref(p, g, m, v, t=t, **h)
            bound = [b + c for b, c in zip(bound, bnd)]
            p, m, v = pr.astype(F32), mr.astype(F32), vr.astype(F32)
        # two f64 steps, the second from the f32 rounding of the first.  The kernel's second step started from ITS first step's
        # p, m, v, which lie within the first step's bounds of these; the moments carry that over scaled by beta <= 1, the update
        # moves with m and v by lr_bc / denom times their error, a term of the size bound_p already carries: 4 x the summed bounds
        # covers it.  The race is an error of 2 lr per element in p and 0.2 |g| in m, four orders of magnitude above
        st = opt.state[x]
        for name, got, want, b in zip("pmv", (x, st["exp_avg"], st["exp_avg_sq"]), (p, m, v), bound):
            err = np.abs(host(got).astype(F64) - want.astype(F64))
            assert (err <= 4.0 * b).all(), (name, x.shape, float(err.max()), float(b.max()))


@pytest.mark.gpu
def test_input_staging_survives_host_run_ahead(gpu):
    """three _stage_host_inputs calls on one network while the device is still busy: every call's device tensors hold ITS OWN feed
    (two pinned buffers alternate: the third call must not rewrite the first one's bytes before its copy has read them)"""
    torch = gpu["torch"]
    from mv3d_tf_amd.networks import get_network
    net = get_network("MV3D_test")
    device = net.device
    to_dev = lambda a: torch.as_tensor(np.asarray(a, F32)).to(device)

    def feed(c):
        return {"im_info": np.full((1, 3), c, F32), "calib": np.full((3, 4), c + 0.25, F32),
                "gt_boxes_bv": np.full((5, 5), c + 0.5, F32), "gt_boxes_3d": np.full((5, 7), c + 0.75, F32),
                "gt_boxes_corners": [np.full((5, 25), c + 0.125, F32), np.full((2, 25), c + 0.375, F32)]}

    feeds = [feed(c) for c in (10.0, 20.0, 30.0)]
    warm = {}
    net._stage_host_inputs(feed(1.0), warm, device, to_dev)            # the pinned buffers: made here
    torch.cuda.synchronize()
    delay = Delay(torch)
    delay.start()
    Ls = [{} for _ in feeds]
    for i, (f, L) in enumerate(zip(feeds, Ls)):
        if i == 2:
            # the first call's copy is still queued when the third call is made.  (Asked AFTER the third call this could not hold
            # on correct code: with two buffers the third call has to wait for that copy, so for the whole chain.)
            delay.require_still_running()
        net._stage_host_inputs(f, L, device, to_dev)
    torch.cuda.synchronize()
    for i, (f, L) in enumerate(zip(feeds, Ls)):
        for k, v in f.items():
            got, want = (L[k], v) if isinstance(v, list) else ([L[k]], [v])
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert np.array_equal(host(a), b), (i, k, float(host(a).reshape(-1)[0]), float(b.reshape(-1)[0]))
