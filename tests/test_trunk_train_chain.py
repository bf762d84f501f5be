"""The training trunks' backward chain and buffer reuse (mv3d_tf_amd/trunk_train.py: TrunksFunction, ConvReluFunction, BufferPool),
link by link against float64.

Every kernel of the trunks is pinned on its own in tests/test_conv_paths.py; this module pins the code that strings them into a
training step: which saved map gates which data gradient, which filter packing is the turned one, which real channel count belongs
to which view, which buffer a gradient lands in -- and that the standing zeros of the pooled buffers (the SAME-padding frame, the
input layers' padding channels, the row / column an odd-sized VALID pool drops) are still zeros when a buffer is used again.

The method.  A whole-trunk comparison against float64 cannot be tight in bf16 (ReLU masks and pool routes of near-ties flip), but
every intermediate of a step sits in a framed buffer that came from the pool.  A recording BufferPool remembers tag -> buffer; after
one forward + backward every link is recomputed in float64 FROM THE STORED INPUTS OF THAT LINK (never from the reference's own
previous layer) and compared with the link's stored output (`_check_step`):

  framing of the input     interior, real channels == x.to(T) bit for bit; padding channels and frame exactly 0
  conv + bias + ReLU       |got - ref| <= 2^-p |ref| + 1.01 (9 c_in + 1) 2^-24 S per element (p = 8 for bf16 maps, no such term for f32
                           maps -- the last layer's returned map is always f32), S = |x| (*) |w| + |b|; frame exactly 0
  pool                     bit for bit, whole buffer
  head gradient            interior == (g * (out > 0)).to(T) bit for bit, frame 0
  data gradient            float64 convolution of dY with the turned, channel-swapped w.to(T), zero where the gate (the output of the
                           layer below, when no pool sits between) is <= 0; the bound above with 9 c_out + 1 terms; frame exactly 0
  pool gradient            first maximum of the window in row-major order gets the pooled gradient if it is > 0, all else 0: bit for
                           bit over the WHOLE buffer, dropped last row / column and frame included
  weight / bias gradient   shape (O, c_in_real, 3, 3); |got - ref| <= 1.01 n 2^-24 S, n = B H W + 1

Where the bounds come from: operands are exact in their type T, products of two bf16 numbers are exact in f32, and an f32 sum of n
terms in ANY order (tile order, K splits, the reduce kernel) is within (n - 1) u / (1 - (n - 1) u) <= 1.01 n 2^-24 of S, the same sum over
absolute values; in f32 the n rounded products fit the same expression (the dot-product bound gamma_n).  Terms that are exactly zero
(padding channels, frame pixels) round nothing, so n counts real channels / interior pixels.  2^-p |ref| is one round-to-nearest of
the result to bf16.  At these shapes every bound is below 1e-4 S, and a wiring mistake -- the gate from the wrong layer, a packing
not turned, view 1's channel count used for view 0, a bias added to a data gradient -- is an error of the order of S or |ref|.
"Bit for bit" compares the raw bits.  No bound here is measured and none is a bare constant.

The float64 references (tests/conv_float64_reference.py) are checked themselves, without a device: chained through the same five
layers they reproduce torch autograd in float64 -- where no mask flips -- to 1e-12 of the largest entry, on random operands and on
small integers that make pool ties."""
import pytest

import conv_float64_reference as R

LAYERS = [("a", 64, False), ("b", 64, True), ("c", 128, False), ("d", 128, True), ("e", 256, False)]
SUFFIXES = ["", "_2", "_3"]
# 13x18 -> 6x9 -> 3x4, 10x21 -> 5x10 -> 2x5, 7x9 -> 3x4 -> 1x2: every pool level drops a row in some view and a column in some view,
# one view ends at a single row, the real input channel counts all differ
SHAPES = [(2, 13, 18, 9), (2, 10, 21, 3), (2, 7, 9, 5)]
# H and W swapped: the first view's height is even at the first pool level, the second view's odd
SHAPES_T = [(B, W, H, c) for B, H, W, c in SHAPES]
gpu_mark = pytest.mark.gpu
CPAD0 = 64                                      # the input layers' channels are zero-padded to this in their framed buffer


def _out_hw(H, W):
    for _, _, pool in LAYERS:
        if pool:
            H, W = H // 2, W // 2
    return H, W


def _data(torch, seed, shapes=SHAPES, dev="cuda", dtype=None, base=None, integers=False):
    """(xs, params, gs): per view an input, He-scaled filters with biases of about 0.1 (or `base`'s, perturbed), a random cotangent.
    integers: small non-negative inputs and small integer filters -- exact in float64, and full of ties"""
    dtype = dtype or torch.float32
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(s, device=dev, generator=g, dtype=dtype)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, device=dev, generator=g).to(dtype)
    xs, params, gs = [], {}, []
    for sfx, (B, H, W, c) in zip(SUFFIXES, shapes):
        xs.append(ri(0, 4, B, H, W, c) if integers else rn(B, H, W, c))
        cin = c
        for name, cout, _ in LAYERS:
            if base is not None:
                w0, b0 = base[name + sfx]
                w, b = w0.detach() * (1 + 0.1 * rn(cout, cin, 3, 3)), b0.detach() + 0.02 * rn(cout)
            elif integers:
                w, b = ri(-1, 2, cout, cin, 3, 3), ri(-3, 2, cout)
            else:
                w, b = rn(cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5, rn(cout) * 0.1
            params[name + sfx] = [w.requires_grad_(True), b.requires_grad_(True)]
            cin = cout
        Ho, Wo = _out_hw(H, W)
        gs.append(ri(-2, 3, B, Ho, Wo, LAYERS[-1][1]) if integers else rn(B, Ho, Wo, LAYERS[-1][1]))
    return xs, params, gs


# ------------------------------------------------------------------------------------- the references themselves (no device)
def _chain(torch, x, wb, g, cpad0=None):
    """one view's training step out of the per-link references alone, every link fed by the one before it: x (B, H, W, c), wb =
    [(w, b)] per layer, g the cotangent of the last map -> (last map, [(dW, db)] per layer)"""
    n = len(LAYERS)
    zeros = lambda k: torch.zeros(k, dtype=x.dtype, device=x.device)
    cur, saved = R.frame(x, cpad0), []
    for (name, cout, pool), (w, b) in zip(LAYERS, wb):
        wpad = torch.zeros((cout, cur.shape[3], 3, 3), dtype=x.dtype, device=x.device)
        wpad[:, :w.shape[1]] = w                                  # (the input layer: its filter over the padded channels)
        y = R.frame(R.conv(cur, wpad, b, relu=True))
        saved.append((cur, y))
        cur = R.pool(y) if pool else y
    out = saved[-1][1][:, 1:-1, 1:-1]
    dy = R.frame(g * (out > 0))
    grads = [None] * n
    for i in range(n - 1, -1, -1):
        w = wb[i][0]
        dw, db = R._wgrad_ref(torch, saved[i][0], dy)
        grads[i] = (dw[:, :w.shape[1]], db)
        if i == 0:
            break
        y_below = saved[i - 1][1]
        if LAYERS[i - 1][2]:
            dy = R.pool_grad(y_below, R.frame(R.conv(dy, R.dgrad_filter(w), zeros(w.shape[1]))))
        else:
            dy = R.frame(R.conv(dy, R.dgrad_filter(w), zeros(w.shape[1]), gate=y_below))
    return out, grads


def _autograd(torch, x, wb, g):
    t = x.permute(0, 3, 1, 2)
    for (_, _, pool), (w, b) in zip(LAYERS, wb):
        t = torch.relu(torch.nn.functional.conv2d(t, w, b, padding=1))
        if pool:
            t = torch.nn.functional.max_pool2d(t, 2, 2)
    out = t.permute(0, 2, 3, 1)
    flat = [p for pair in wb for p in pair]
    got = torch.autograd.grad([out], flat, [g])
    return out.detach(), [(got[2 * i], got[2 * i + 1]) for i in range(len(wb))]


def _tied_windows(torch, yp):
    """windows of a framed map whose positive maximum stands at more than one position"""
    a = [v for _, _, v in R._windows(yp)]
    m = torch.stack(a).amax(0)
    return int(((torch.stack([v == m for v in a]).sum(0) > 1) & (m > 0)).sum())


@pytest.mark.parametrize("integers", [False, True], ids=["random", "integers_with_ties"])
@pytest.mark.parametrize("cpad0", [None, CPAD0], ids=["bare_input", "padded_input"])
def test_chained_float64_references_reproduce_autograd(integers, cpad0):
    """no device: conv, gate, pool route, turned filter and weight gradient of tests/conv_float64_reference.py, chained through the
    five layers in float64 at the three view shapes, against torch autograd in float64 to 1e-12 of each tensor's largest entry.  The
    integer operands are exact in float64 and make pool ties (asserted), so the first-maximum rule is part of what must agree."""
    import torch
    xs, params, gs = _data(torch, 31 + integers, dev="cpu", dtype=torch.float64, integers=integers)
    for v, sfx in enumerate(SUFFIXES):
        wb = [tuple(params[name + sfx]) for name, _, _ in LAYERS]
        want_out, want = _autograd(torch, xs[v], wb, gs[v])
        out, got = _chain(torch, xs[v], [(w.detach(), b.detach()) for w, b in wb], gs[v], cpad0)
        close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
        assert float(want_out.abs().max()) > 0 and close(out, want_out), (v, "last map")
        for i, ((dw, db), (rw, rb)) in enumerate(zip(got, want)):
            assert dw.shape == rw.shape and db.shape == rb.shape
            assert float(rw.abs().max()) > 0 and close(dw, rw) and close(db, rb), (v, i)
    if integers:                                                   # the ties are really there, at the first pooled layer of view 0
        x, (w, b) = xs[0], params["a"]
        y0 = R.frame(R.conv(R.frame(x), w.detach(), b.detach(), relu=True))
        w1, b1 = params["b"]
        assert _tied_windows(torch, R.frame(R.conv(y0, w1.detach(), b1.detach(), relu=True))) > 0


def test_pool_gradient_reference_by_hand():
    """no device: the pool-gradient rule on windows written out by hand (5 x 4 map, so the last row is dropped)"""
    import torch
    y = torch.tensor([[2., 2., 0., 0.],
                      [1., 2., 0., 0.],
                      [0., 1., 3., 1.],
                      [4., 4., 1., 3.],
                      [9., 9., 9., 9.]], dtype=torch.float64).view(1, 5, 4, 1)
    g = torch.tensor([[10., 20.], [30., 40.]], dtype=torch.float64).view(1, 2, 2, 1)
    want = torch.tensor([[10., 0., 0., 0.],                      # tie of three 2s: the first; a window of zeros: nothing
                         [0., 0., 0., 0.],
                         [0., 0., 40., 0.],                      # tie of two 3s: the first in row-major order
                         [30., 0., 0., 0.],                      # tie of two 4s in the second row
                         [0., 0., 0., 0.]], dtype=torch.float64).view(1, 5, 4, 1)
    got = R.pool_grad(R.frame(y), R.frame(g))
    assert torch.equal(got, R.frame(want))
    assert torch.equal(R.pool(R.frame(y)), R.frame(torch.tensor([[2., 0.], [4., 3.]], dtype=torch.float64).view(1, 2, 2, 1)))
    f = R.dgrad_filter(torch.arange(2 * 3 * 9, dtype=torch.float64).view(2, 3, 3, 3))
    assert f.shape == (3, 2, 3, 3) and float(f[1, 0, 0, 0]) == 17.0 and float(f[0, 1, 2, 2]) == 27.0


# --------------------------------------------------------------------------------------------- BufferPool's own rules (no device)
def test_buffer_pool_rules_on_cpu_tensors():
    import torch
    from mv3d_tf_amd import trunk_train
    pool = trunk_train.BufferPool()
    assert pool.max_shapes == 4
    key = lambda k: (1, 2 + k, 3, 8)
    a = [pool.get("t/x", *key(k), "cpu") for k in range(4)]
    assert all(b.shape == (1, 4 + k, 5, 8) and b.dtype == torch.bfloat16 and int(b.count_nonzero()) == 0 for k, b in enumerate(a))
    assert all(pool.get("t/x", *key(k), "cpu") is a[k] for k in range(4))             # the same key: the same object
    assert pool.get("t/x", *key(1), "cpu", torch.float32) is not a[1]                 # (the type is part of the key; evicts key 0 ...)
    pool = trunk_train.BufferPool()
    a = [pool.get("t/x", *key(k), "cpu") for k in range(4)]
    other = pool.get("t/y", *key(0), "cpu")
    assert other is not a[0]
    for k in range(4):
        a[k].fill_(k + 1)
    assert pool.get("t/x", *key(0), "cpu") is a[0]                                     # key 0, the oldest created, is now the most recently USED
    fifth = pool.get("t/x", *key(4), "cpu")                                            # a fifth shape: out goes key 1, the least recently used
    assert int(fifth.count_nonzero()) == 0
    assert pool.get("t/x", *key(0), "cpu") is a[0] and pool.get("t/x", *key(2), "cpu") is a[2] and pool.get("t/x", *key(3), "cpu") is a[3]
    assert pool.get("t/x", *key(4), "cpu") is fifth
    again = pool.get("t/x", *key(1), "cpu")                                            # the evicted shape: a new, all-zero buffer
    assert again is not a[1] and int(again.count_nonzero()) == 0 and float(a[1].min()) == 2.0   # (whoever still holds the old one keeps it)
    assert pool.get("t/x", *key(0), "cpu") is not a[0]                                 # ... which in turn pushed out key 0, by then the oldest used
    assert pool.get("t/y", *key(0), "cpu") is other                                    # tags do not evict one another
    for k in range(1, 6):
        pool.get("u/%d" % k, *key(0), "cpu")
    assert pool.get("t/y", *key(0), "cpu") is other
    assert all(len(per) <= 4 for per in pool._buf.values())
    one = trunk_train.BufferPool(max_shapes=1)
    b0 = one.get("t", *key(0), "cpu")
    assert one.get("t", *key(0), "cpu") is b0 and one.get("t", *key(1), "cpu") is not b0 and one.get("t", *key(0), "cpu") is not b0
    # generations: a second begin() of a tag invalidates the first, and only that tag's
    g1, h1 = pool.begin("trunk"), pool.begin("trunk_2")
    pool.check("trunk", g1)
    pool.check("trunk_2", h1)
    g2 = pool.begin("trunk")
    assert g2 != g1
    with pytest.raises(RuntimeError, match=r"trunk 'trunk' ran forward again"):
        pool.check("trunk", g1)
    pool.check("trunk", g2)
    pool.check("trunk_2", h1)
    none = trunk_train._NoPool
    g1 = none.begin("trunk")
    none.begin("trunk")
    none.check("trunk", g1)
    none.check("never begun", 7)
    assert none.get("t", *key(0), "cpu") is not none.get("t", *key(0), "cpu")


# ------------------------------------------------------------------------------------------------------------------ device side
@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    return torch


@pytest.fixture(scope="module", params=["bf16", "f32"])
def T(request, gpu):
    return {"bf16": gpu.bfloat16, "f32": gpu.float32}[request.param]


def _recording_pool(max_shapes=4):
    from mv3d_tf_amd import trunk_train

    class RecordingPool(trunk_train.BufferPool):
        """BufferPool that remembers what it handed out since the last take()"""

        def __init__(self, max_shapes):
            super().__init__(max_shapes)
            self.calls = []

        def get(self, tag, B, H, W, C, dev, dtype=trunk_train.BF):
            buf = super().get(tag, B, H, W, C, dev, dtype)
            assert tuple(buf.shape) == (B, H + 2, W + 2, C) and buf.dtype == dtype and buf.is_contiguous()
            self.calls.append((tag, buf))
            return buf

        def take(self):
            """tag -> buffer of the step just run: one buffer per tag, and no two tags share memory"""
            calls, self.calls = self.calls, []
            tags = [t for t, _ in calls]
            assert len(set(tags)) == len(tags), "a tag was asked for twice in one step: %s" % sorted(t for t in set(tags) if tags.count(t) > 1)
            spans = sorted((b.data_ptr(), b.data_ptr() + b.numel() * b.element_size(), t) for t, b in calls)
            for (_, end, t0), (start, _, t1) in zip(spans, spans[1:]):
                assert end <= start, "%s and %s share memory" % (t0, t1)
            return dict(calls)

    return RecordingPool(max_shapes)


def _expected_tags():
    n = len(LAYERS)
    per = ["/in", "/g%d" % (n - 1)] + ["/y%d" % i for i in range(n - 1)] + ["/dx%d" % i for i in range(1, n)]
    for i, (_, _, pool) in enumerate(LAYERS):
        if pool:
            per += ["/p%d" % i, "/g%d" % i]
    return {"trunk" + sfx + t for sfx in SUFFIXES for t in per}


def _bits(torch, t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(torch, a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(torch, a), _bits(torch, b))


def _frame_is_zero(buf):
    return not any(int(s.count_nonzero()) for s in (buf[:, 0], buf[:, -1], buf[:, :, 0], buf[:, :, -1]))       # (a NaN counts as non-zero)


def _step(torch, data, T, pool, wgrad=None, used=(0, 1, 2)):
    """one forward + backward of the three trunks -> (returned maps, {name: (dW, db)})"""
    from mv3d_tf_amd import trunk_train
    xs, params, gs = data
    for p in params.values():
        p[0].grad = p[1].grad = None
    outs = trunk_train.trunks(LAYERS, xs, params, SUFFIXES, wgrad=wgrad, pool=pool, dtype=T)
    torch.autograd.backward([outs[v] for v in used], [gs[v] for v in used])
    torch.cuda.synchronize()
    return [o.detach() for o in outs], {k: (p[0].grad, p[1].grad) for k, p in params.items()}


def _check_step(torch, bufs, data, outs, grads, T, what, used=(0, 1, 2)):
    """every row of the module docstring's table, for every layer and view, on the buffers `bufs` of the step that gave
    `outs` and `grads`"""
    xs, params, gs = data
    n = len(LAYERS)
    out_dt = "bf16" if T == torch.bfloat16 else "f32"
    f64 = lambda t: t.detach().double()
    assert set(bufs) == _expected_tags(), sorted(set(bufs) ^ _expected_tags())
    for v, sfx in enumerate(SUFFIXES):
        tag = "trunk" + sfx
        at = lambda link: "%s, view %d, %s" % (what, v, link)
        B, H, W, c0 = xs[v].shape
        # ---- framing of the input
        fin = bufs[tag + "/in"]
        assert tuple(fin.shape) == (B, H + 2, W + 2, CPAD0) and fin.dtype == T, at("input shape")
        assert _same_bits(torch, fin[:, 1:-1, 1:-1, :c0], xs[v].to(T)), at("input interior")
        assert int(fin[..., c0:].count_nonzero()) == 0 and _frame_is_zero(fin), at("input padding channels / frame")
        # ---- forward
        cur, hw, inputs = fin, (H, W), []
        for i, (name, cout, pool) in enumerate(LAYERS):
            w, b = params[name + sfx]
            creal = w.shape[1]
            wpad = torch.zeros((cout, cur.shape[3], 3, 3), dtype=torch.float64, device=cur.device)
            wpad[:, :creal] = f64(w.detach().to(T))
            ref = R.conv(f64(cur), wpad, f64(b), relu=True)
            S = R.conv(f64(cur), wpad, f64(b), absval=True)
            inputs.append(cur)
            if i == n - 1:
                assert tuple(outs[v].shape) == (B, hw[0], hw[1], cout) and outs[v].dtype == torch.float32, at("returned map")
                R._bound_check(torch, outs[v], ref, S, 9 * creal + 1, "f32", at("last layer"))
                break
            y = bufs["%s/y%d" % (tag, i)]
            assert tuple(y.shape) == (B, hw[0] + 2, hw[1] + 2, cout) and y.dtype == T, at("y%d shape" % i)
            assert _frame_is_zero(y), at("frame of y%d" % i)
            R._bound_check(torch, y[:, 1:-1, 1:-1], ref, S, 9 * creal + 1, out_dt, at("forward y%d" % i))
            cur = y
            if pool:
                hw = (hw[0] // 2, hw[1] // 2)
                cur = bufs["%s/p%d" % (tag, i)]
                assert _same_bits(torch, cur, R.pool(y)), at("pool p%d" % i)
        # ---- head gradient
        g = gs[v] if v in used else torch.zeros_like(outs[v])
        dy = bufs["%s/g%d" % (tag, n - 1)]
        assert _same_bits(torch, dy, R.frame((g * (outs[v] > 0)).to(T))), at("head gradient")
        # ---- backward, last layer to first
        for i in range(n - 1, -1, -1):
            name, cout, _ = LAYERS[i]
            w, b = params[name + sfx]
            creal = w.shape[1]
            xin = inputs[i]
            Hi, Wi = xin.shape[1] - 2, xin.shape[2] - 2
            assert tuple(dy.shape) == (B, Hi + 2, Wi + 2, cout), at("dy of layer %d" % i)
            gw, gb = grads[name + sfx]
            assert gw is not None and gb is not None, at("gradient of layer %d is None" % i)
            assert tuple(gw.shape) == (cout, creal, 3, 3) and tuple(gb.shape) == (cout,) and gw.dtype == gb.dtype == torch.float32, at("dW shape")
            rw, rb = R._wgrad_ref(torch, f64(xin), f64(dy))
            Sw, Sb = R._wgrad_ref(torch, f64(xin), f64(dy), absval=True)
            if creal < xin.shape[3]:                               # (nothing may have leaked into the input layer's padding channels)
                assert float(Sw[:, creal:].max()) == 0.0, at("padding channels of the input")
            terms = B * Hi * Wi + 1
            R._bound_check(torch, gw, rw[:, :creal], Sw[:, :creal], terms, "f32", at("dW of layer %d" % i))
            R._bound_check(torch, gb, rb, Sb, terms, "f32", at("db of layer %d" % i))
            if i == 0:
                break
            dx = bufs["%s/dx%d" % (tag, i)]
            assert tuple(dx.shape) == (B, Hi + 2, Wi + 2, creal) and dx.dtype == T, at("dx%d shape" % i)
            below = bufs["%s/y%d" % (tag, i - 1)]
            pooled = LAYERS[i - 1][2]
            wd = R.dgrad_filter(f64(w.detach().to(T)))
            zero = torch.zeros(creal, dtype=torch.float64, device=dx.device)
            gate = None if pooled else f64(below)
            ref = R.conv(f64(dy), wd, zero, gate=gate)
            S = R.conv(f64(dy), wd, zero, gate=gate, absval=True)
            assert _frame_is_zero(dx), at("frame of dx%d" % i)
            R._bound_check(torch, dx[:, 1:-1, 1:-1], ref, S, 9 * cout + 1, out_dt, at("data gradient dx%d" % i))
            dy = dx
            if pooled:
                dy = bufs["%s/g%d" % (tag, i - 1)]
                assert _same_bits(torch, dy, R.pool_grad(below, dx)), at("pool gradient g%d" % (i - 1))


def _assert_same_results(torch, a, b, what, views=(0, 1, 2)):
    """returned maps and gradients of two steps, bit for bit"""
    (outs_a, grads_a), (outs_b, grads_b) = a, b
    for v in views:
        assert _same_bits(torch, outs_a[v], outs_b[v]), (what, "map", v)
        for name, _, _ in LAYERS:
            for k in (0, 1):
                assert _same_bits(torch, grads_a[name + SUFFIXES[v]][k], grads_b[name + SUFFIXES[v]][k]), (what, name + SUFFIXES[v], "dW" if k == 0 else "db")


def _keep(result):
    outs, grads = result
    return [o.clone() for o in outs], {k: (w.clone(), b.clone()) for k, (w, b) in grads.items()}


@pytest.fixture(scope="module")
def first(gpu, T):
    """the first step in a fresh recording pool, grouped weight gradient (the product's path): shared, and never touched again"""
    torch = gpu
    data = _data(torch, 101)
    pool = _recording_pool()
    result = _keep(_step(torch, data, T, pool))
    return {"data": data, "result": result, "bufs": pool.take()}


@gpu_mark
def test_chain_first_step(gpu, T, first):
    """case 1: every link of every layer and view, on fresh buffers"""
    _check_step(gpu, first["bufs"], first["data"], *first["result"], T, "first step")


@gpu_mark
def test_chain_under_buffer_reuse(gpu, T, first):
    """case 2: the same pool over three steps -- other inputs, cotangents and (perturbed) weights in the second, the first step's data
    again in the third.  A kernel that stopped writing part of what it owns would leave the step before's values there, a kernel
    that wrote into a frame, a padding channel or a dropped pool row would leave a non-zero for the next step: every link holds at
    every step, and every step equals the same step on fresh buffers (pool=None) bit for bit"""
    torch = gpu
    one = first["data"]
    two = _data(torch, 202, base=one[1])
    pool = _recording_pool()
    seen = {}
    for k, data in enumerate((one, two, one)):
        got = _keep(_step(torch, data, T, pool))
        bufs = pool.take()
        if k:                                                       # the pool really handed out the buffers of the step before
            assert all(bufs[t] is seen[t] for t in bufs), "step %d did not reuse the buffers" % (k + 1)
        seen = bufs
        _check_step(torch, bufs, data, *got, T, "step %d of 3 in one pool" % (k + 1))
        _assert_same_results(torch, got, _step(torch, data, T, None), "step %d: pooled against fresh buffers" % (k + 1))
        if k != 1:
            _assert_same_results(torch, got, first["result"], "step %d against the shared first step" % (k + 1))


@gpu_mark
def test_chain_across_shape_changes(gpu, T):
    """case 3: a pool that keeps ONE shape per tag, two sets of view shapes (H and W swapped) in turn over four steps: every buffer is
    evicted at every step and every link still holds.  Then a forward on the other shape while a step's graph is still alive: its
    buffers are gone from the pool, and its backward pass must raise through the generation guard, naming the trunk, instead of
    computing anything -- while the newer step's backward pass is still right.  With pool=None the same interleaving computes
    what the two steps compute on their own, bit for bit."""
    torch = gpu
    from mv3d_tf_amd import trunk_train
    sets = [_data(torch, 303), _data(torch, 404, shapes=SHAPES_T)]
    pool = _recording_pool(max_shapes=1)
    for k in range(4):
        data = sets[k % 2]
        got = _step(torch, data, T, pool)
        _check_step(torch, pool.take(), data, *got, T, "step %d of 4, shapes in turn" % (k + 1))
        assert all(len(per) == 1 for per in pool._buf.values())

    def forward(data, p):
        return trunk_train.trunks(LAYERS, data[0], data[1], SUFFIXES, pool=p, dtype=T)

    def clear(data):
        for p in data[1].values():
            p[0].grad = p[1].grad = None

    grads_of = lambda data: {k: (p[0].grad, p[1].grad) for k, p in data[1].items()}
    for data in sets:
        clear(data)
    outs_a = forward(sets[0], pool)
    pool.take()
    outs_b = forward(sets[1], pool)
    with pytest.raises(RuntimeError, match=r"BufferPool: trunk 'trunk' ran forward again"):
        torch.autograd.backward(outs_a, sets[0][2])
    assert all(p[0].grad is None and p[1].grad is None for p in sets[0][1].values())
    torch.autograd.backward(outs_b, sets[1][2])
    torch.cuda.synchronize()
    _check_step(torch, pool.take(), sets[1], [o.detach() for o in outs_b], grads_of(sets[1]), T, "the newer step after the refused one")
    # fresh buffers: interleaved == on their own
    alone = [_keep(_step(torch, data, T, None)) for data in sets]
    for data in sets:
        clear(data)
    outs_a = forward(sets[0], None)
    outs_b = forward(sets[1], None)
    torch.autograd.backward(outs_a, sets[0][2])
    torch.autograd.backward(outs_b, sets[1][2])
    torch.cuda.synchronize()
    _assert_same_results(torch, ([o.detach() for o in outs_a], grads_of(sets[0])), alone[0], "interleaved, first shapes")
    _assert_same_results(torch, ([o.detach() for o in outs_b], grads_of(sets[1])), alone[1], "interleaved, swapped shapes")


@gpu_mark
def test_unused_view_gets_zero_gradients(gpu, T, first):
    """case 4: only views 0 and 2 enter the loss: view 1's five (w, b) gradients are exact zeros (not None, not NaN), the other views'
    are the first step's bit for bit, and every link holds with a zero head gradient in view 1"""
    torch = gpu
    pool = _recording_pool()
    got = _step(torch, first["data"], T, pool, used=(0, 2))
    for name, _, _ in LAYERS:
        gw, gb = got[1][name + SUFFIXES[1]]
        assert gw is not None and gb is not None, name
        assert gw.shape == first["data"][1][name + SUFFIXES[1]][0].shape and gb.shape == (gw.shape[0],)
        assert int(gw.count_nonzero()) == 0 and int(gb.count_nonzero()) == 0, name
    _assert_same_results(torch, got, first["result"], "views 0 and 2 beside an unused view", views=(0, 2))
    assert _same_bits(torch, got[0][1], first["result"][0][1])
    _check_step(torch, pool.take(), first["data"], *got, T, "view 1 unused", used=(0, 2))


@gpu_mark
def test_grouped_against_per_view_weight_gradient(gpu, T, first):
    """case 5: wgrad=None (one grouped launch per depth) against wgrad=trunk_train.wgrad_mfma (one launch per view): returned maps
    and every stored buffer -- forward maps, data and pool gradients -- bit for bit, the weight and bias gradients of BOTH inside the
    float64 bound (their K-split plans differ, so they may differ from each other in the last bits)"""
    torch = gpu
    from mv3d_tf_amd import trunk_train
    pool = _recording_pool()
    got = _step(torch, first["data"], T, pool, wgrad=trunk_train.wgrad_mfma)
    bufs = pool.take()
    assert set(bufs) == set(first["bufs"])
    for t in sorted(bufs):
        assert _same_bits(torch, bufs[t], first["bufs"][t]), t
    for v in range(3):
        assert _same_bits(torch, got[0][v], first["result"][0][v]), v
    _check_step(torch, bufs, first["data"], *got, T, "per-view weight gradient")      # (the grouped one: test_chain_first_step)


@gpu_mark
def test_conv_relu_against_float64(gpu, T):
    """case 6: trunk_train.conv_relu (rpn_conv/3x3) between f32 maps: the forward on x.to(T), w.to(T); with dy = (g * (out > 0)).to(T)
    from the function's own output, dx (an f32 map) inside the data-gradient bound and dW, db inside the weight-gradient bound"""
    torch = gpu
    from mv3d_tf_amd import trunk_train
    B, H, W, cin, cout = 2, 9, 11, 64, 128
    gen = torch.Generator(device="cuda").manual_seed(606)
    rn = lambda *s: torch.randn(s, device="cuda", generator=gen)
    x = rn(B, H, W, cin).requires_grad_(True)
    w = (rn(cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5).requires_grad_(True)
    b = (rn(cout) * 0.1).requires_grad_(True)
    g = rn(B, H, W, cout)
    out = trunk_train.conv_relu(x, w, b, dtype=T)
    out.backward(g)
    torch.cuda.synchronize()
    out = out.detach()
    xp = R.frame(x.detach().to(T)).double()
    w64, b64 = w.detach().to(T).double(), b.detach().double()
    assert tuple(out.shape) == (B, H, W, cout) and out.dtype == torch.float32
    R._bound_check(torch, out, R.conv(xp, w64, b64, relu=True), R.conv(xp, w64, b64, absval=True), 9 * cin + 1, "f32", "conv_relu forward")
    dy = R.frame((g * (out > 0)).to(T)).double()
    zero = torch.zeros(cin, dtype=torch.float64, device="cuda")
    assert tuple(x.grad.shape) == (B, H, W, cin) and x.grad.dtype == torch.float32
    R._bound_check(torch, x.grad, R.conv(dy, R.dgrad_filter(w64), zero), R.conv(dy, R.dgrad_filter(w64), zero, absval=True), 9 * cout + 1, "f32",
                   "conv_relu dx")
    rw, rb = R._wgrad_ref(torch, xp, dy)
    Sw, Sb = R._wgrad_ref(torch, xp, dy, absval=True)
    assert tuple(w.grad.shape) == (cout, cin, 3, 3) and tuple(b.grad.shape) == (cout,)
    R._bound_check(torch, w.grad, rw, Sw, B * H * W + 1, "f32", "conv_relu dW")
    R._bound_check(torch, b.grad, rb, Sb, B * H * W + 1, "f32", "conv_relu db")
