"""The training solver at its edges: mv3d_grad_norm and mv3d_sgd_step (csrc/solver.hip), mv3d_adam_step_ctl (csrc/adam.hip), optim.SGD /
optim.Adam with clipping, the non-finite guard and weight decay, optim.learning_rate, and cfg.TRAIN.SOLVER in SolverWrapper.

One set of case tables feeds two things, as in tests/test_optim_loss_edges.py:
  1. unmarked tests: the restatements of tests/solver_restatement.py stay inside that module's derived bounds against its f64
     references with a margin of 2 (so a correct implementation CAN meet them), and the host side -- the schedule, the configuration
     keys, SolverWrapper on a CPU toy network, which runs the optimizers' host path;
  2. `-m gpu` tests: the kernels stay inside the same bounds against the same f64 references, never against the device or the library.
Bit comparisons where the contract is exact: the norm's order of summation (offsets, repeats, and the numpy statement of that order),
the coefficient rule on top of the device's sum, vector body against scalar loop, the 16-bit copies, a skipped step, the controlled
Adam step with nothing to control against mv3d_adam_step.

Worst use of the bounds seen on the MI355X: SGD p 0.498, buf 0.494; controlled Adam p 0.497, m 0.368, v 0.394; optim.SGD 0.497 / 0.445;
optim.Adam with clip, guard and decay 0.496 / 0.384 / 0.395; the norm's sum equalled math.fsum's on both size tables.

FINISH = 1024 threads reduce the chunks' partials: the single tensor of 1025 CHUNK + 5 elements has 1026 partials, so that
workgroup's loop wraps (threads 0 and 1 add two partials each).
"""
import contextlib
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

import solver_restatement as R

F32, F64 = np.float32, np.float64
CHUNK = R.CHUNK
FINISH = R.FINISH_THREADS
MARGIN = 0.5                      # the restatements must use at most half of every bound

SIZES = (4097, 1, 8192, 3, 4095, 4096, 3 * CHUNK + 17)             # the 1-element tensor between two multi-chunk ones
WRAP_SIZE = (FINISH + 1) * CHUNK + 5                                # 1026 partials: the finishing loop wraps past its thread count
GRAD_SCALES = (1e-6, 1e-3, 1.0, 1e3)
MOMENTA = (0.0, 0.5, 0.9)
LRS = (1e-5, 1e-3, 0.1)
DECAYS = (0.0, 5e-4)
COEFS = (1.0, 0.37)


def sgd_hypers():
    return [dict(lr=lr, momentum=mu, coef=c) for mu, lr, c in itertools.product(MOMENTA, LRS, COEFS)]


def tensor_decay(k):
    """weight decay mixed per tensor in one launch"""
    return DECAYS[k % 2]


def sgd_state(sizes, seed):
    """[(p, g, buf)] f32: tensor k's gradient at GRAD_SCALES[k % 4], a buffer of that scale and either sign, one element in 16 at the
    state of a first step (buf = 0) and one in 16 with a zero gradient"""
    r = np.random.RandomState(seed)
    out = []
    for k, n in enumerate(sizes):
        s = GRAD_SCALES[k % len(GRAD_SCALES)]
        p = r.normal(0, 1, n)
        g = r.normal(0, s, n)
        b = r.normal(0, s, n) * r.choice([0.1, 1.0, 10.0], n)
        b[r.randint(0, 16, n) == 0] = 0.0
        g[r.randint(0, 16, n) == 0] = 0.0
        out.append(tuple(a.astype(F32) for a in (p, g, b)))
    return out


def adam_state(sizes, seed):
    """[(p, g, m, v)] f32, the table of test_optim_loss_edges.py restated: moments of a run with gradients of the tensor's scale"""
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


def sgd_worst(got, st, h, wd):
    """the largest |got - f64| / bound over p, buf of one tensor"""
    ref = R.sgd_ref(*st, wd=wd, **h)
    bnd = R.sgd_bound(*st, wd=wd, **h)
    return [float(np.max(np.abs(a.astype(F64) - b) / c)) for a, b, c in zip(got, ref, bnd)]


def adam_worst(got, st, h, coef, wd):
    ref = R.adam_ctl_ref(*st, coef=coef, wd=wd, **h)
    bnd = R.adam_ctl_bound(*st, coef=coef, wd=wd, **h)
    return [float(np.max(np.abs(a.astype(F64) - b) / c)) for a, b, c in zip(got, ref, bnd)]


def norm_grads(sizes, seed):
    r = np.random.RandomState(seed)
    return [r.normal(0, GRAD_SCALES[k % len(GRAD_SCALES)], n).astype(F32) for k, n in enumerate(sizes)]


@functools.lru_cache(maxsize=None)
def norm_case(name):
    """(grads, fsum reference): computed once, shared, never changed"""
    grads = norm_grads(SIZES, 31) if name == "sizes" else norm_grads((WRAP_SIZE,), 32)
    for g in grads:
        g.setflags(write=False)
    return grads, R.sumsq_ref(grads)


# =================================================================== unmarked: the restatements meet their bounds
def test_sgd_f32_restatement_meets_its_bound():
    worst = np.zeros(2)
    for i, h in enumerate(sgd_hypers()):
        for k, st in enumerate(sgd_state((CHUNK + 17, 3, 1, 2 * CHUNK), seed=i)):
            wd = tensor_decay(k)
            worst = np.maximum(worst, sgd_worst(R.sgd_f32(*st, wd=wd, **h), st, h, wd))
    print("sgd restatement: worst use of the bounds (p, buf):", worst)
    assert (worst <= MARGIN).all(), worst


def test_controlled_adam_f32_restatement_meets_its_bound():
    worst = np.zeros(3)
    i = 0
    for t, (b1, b2), lr, coef in itertools.product((1, 2, 1000), ((0.9, 0.999), (0.5, 0.9)), (1e-5, 1e-3), COEFS):
        h = dict(lr=lr, b1=b1, b2=b2, eps=1e-8, t=t)
        for k, st in enumerate(adam_state((CHUNK + 17, 3, 1, 2 * CHUNK), seed=100 + i)):
            wd = tensor_decay(k)
            worst = np.maximum(worst, adam_worst(R.adam_ctl_f32(*st, coef=coef, wd=wd, **h), st, h, coef, wd))
        i += 1
    print("controlled adam restatement: worst use of the bounds (p, m, v):", worst)
    assert (worst <= MARGIN).all(), worst


def test_controlled_adam_restatement_with_nothing_to_control_is_the_plain_step():
    """coef 1, decay 0: g' is g bit for bit, so the restatement is adam_one's"""
    for st in adam_state((CHUNK + 17, 3), seed=5):
        assert np.array_equal(R.gprime_f32(st[0], st[1], 1.0, 0.0).view(np.uint32), st[1].view(np.uint32))
    p = np.array([np.inf, -np.inf, 1.0], F32)
    g = np.array([1.0, 2.0, np.inf], F32)
    assert np.array_equal(R.gprime_f32(p, g, 1.0, 0.0), g)           # no 0 * inf: the decay term is not evaluated at decay 0


def test_norm_restatement_meets_its_bound():
    worst = 0.0
    cases = [(sizes,) + norm_case(name) for name, sizes in (("sizes", SIZES), ("wrap", (WRAP_SIZE,)))]
    cases += [(SIZES, g, R.sumsq_ref(g)) for g in (norm_grads(SIZES, 40 + i) for i in range(12))]
    for sizes, grads, ref in cases:
        got = R.sumsq_restated(grads)
        worst = max(worst, abs(got - ref) / ref / R.sumsq_bound(sizes))
    assert R.sumsq_chain((WRAP_SIZE,)) == 16 + 6 + 2 + 2 + 6 + 4 and R.sumsq_chain(SIZES) == 35
    assert R.sumsq_restated([]) == 0.0 and R.sumsq_ref([]) == 0.0
    print("norm restatement: worst use of the bound:", worst)
    assert worst <= MARGIN, worst


def test_norm_restatement_order_is_a_function_of_the_sizes():
    """the same values cut into tensors differently give another tree (so the restatement does state an order), the same values in
    the same sizes the same bits; a NaN or an inf anywhere reaches the sum"""
    g = norm_grads((3 * CHUNK,), 33)[0]
    a = R.sumsq_restated([g])
    assert a == R.sumsq_restated([g.copy()])
    sums = {R.sumsq_restated([g[:k], g[k:]]) for k in (1, 2, 3, 5, 100, 1000, 4095)} | {a}
    assert len(sums) > 1
    for bad, want in ((np.nan, np.isnan), (np.inf, np.isposinf)):
        h = g.copy()
        h[CHUNK + 7] = bad
        assert want(R.sumsq_restated([h])) and want(R.sumsq_ref([h]))


def test_control_rule():
    one = lambda *a, **k: tuple(float(x) for x in R.control_rule(*a, **k))
    assert one(4.0, 0.0, 0) == (2.0, 1.0, 0.0)
    assert one(4.0, 3.0, 1) == (2.0, 1.0, 0.0)                        # above the norm: not scaled up
    n, c, s = R.control_rule(4.0, 2.0, 0)                             # AT the norm: 2 / (2 + 1e-6) < 1
    assert c == F32(2.0 / (2.0 + 1e-6)) and c < 1
    assert one(4.0, 1.0, 0)[1] == float(F32(1.0 / (2.0 + 1e-6)))
    assert one(0.0, 1.0, 1) == (0.0, 1.0, 0.0)                        # a zero gradient: 1 / 1e-6 >= 1
    assert one(np.inf, 1.0, 0) == (np.inf, 0.0, 0.0) and one(np.inf, 1.0, 1) == (np.inf, 0.0, 1.0)
    n, c, s = R.control_rule(np.nan, 1.0, 0)
    assert np.isnan(n) and np.isnan(c) and s == 0
    n, c, s = R.control_rule(np.nan, 0.0, 1)
    assert np.isnan(n) and c == 0 and s == 1
    assert one(0.0, 1e-9, 0, empty=True)[1] == 1.0


# =================================================================== unmarked: schedule, configuration, SolverWrapper on the host path
@contextlib.contextmanager
def train_cfg(**kw):
    from mv3d_tf_amd.fast_rcnn.config import cfg
    saved = {k: cfg.TRAIN[k] for k in kw}
    cfg.TRAIN.update(kw)
    try:
        yield cfg
    finally:
        cfg.TRAIN.update(saved)


def test_learning_rate_schedule():
    from mv3d_tf_amd import optim
    with train_cfg(LEARNING_RATE=0.001, GAMMA=0.1, STEPSIZE=2, WARMUP_ITERS=0):
        assert optim.learning_rate(0) == 0.001 and optim.learning_rate(1) == 0.001                    # it = 0, STEPSIZE - 1
        assert optim.learning_rate(2) == 0.001 * 0.1 ** 1 and optim.learning_rate(4) == 0.001 * 0.1 ** 2   # STEPSIZE, 2 STEPSIZE
        assert optim.learning_rate(3) == optim.learning_rate(2)
    with train_cfg(LEARNING_RATE=0.001, GAMMA=0.1, STEPSIZE=2, WARMUP_ITERS=4):
        assert optim.learning_rate(0) == 0.001 * (1 / 4.0)
        assert optim.learning_rate(1) == 0.001 * (2 / 4.0)                                            # inside the warm-up
        assert optim.learning_rate(2) == 0.001 * 0.1 * (3 / 4.0)
        assert optim.learning_rate(3) == 0.001 * 0.1 * 1.0                                            # its end
        assert optim.learning_rate(4) == 0.001 * 0.1 ** 2
    from mv3d_tf_amd.fast_rcnn.config import AttrDict
    T = AttrDict(LEARNING_RATE=0.5, GAMMA=0.5, STEPSIZE=10, WARMUP_ITERS=0)
    assert optim.learning_rate(25, T) == 0.125                                                        # an explicit table


def test_solver_keys_defaults_and_yaml_merge():
    import copy
    from mv3d_tf_amd.fast_rcnn import config
    T = config.cfg.TRAIN
    assert (T.SOLVER, T.MOMENTUM, T.WEIGHT_DECAY, T.GAMMA, T.STEPSIZE, T.WARMUP_ITERS, T.CLIP_GRAD_NORM, T.SKIP_NON_FINITE, T.LEARNING_RATE) \
        == ('reference', 0.9, 0.0, 0.1, 50000, 0, 0.0, False, 0.001)
    c = copy.deepcopy(config.cfg)
    config._merge({"TRAIN": {"SOLVER": "sgd", "MOMENTUM": 0.8, "WEIGHT_DECAY": 0.0005, "GAMMA": 0.5, "STEPSIZE": 100000, "WARMUP_ITERS": 500,
                             "CLIP_GRAD_NORM": 10, "SKIP_NON_FINITE": True}}, c)
    assert (c.TRAIN.SOLVER, c.TRAIN.MOMENTUM, c.TRAIN.WEIGHT_DECAY, c.TRAIN.GAMMA, c.TRAIN.STEPSIZE, c.TRAIN.WARMUP_ITERS) \
        == ("sgd", 0.8, 0.0005, 0.5, 100000, 500)
    assert c.TRAIN.CLIP_GRAD_NORM == 10.0 and isinstance(c.TRAIN.CLIP_GRAD_NORM, float) and c.TRAIN.SKIP_NON_FINITE is True
    assert T.SOLVER == 'reference' and T.CLIP_GRAD_NORM == 0.0                                        # the copy took the merge
    for bad in ({"STEPSIZE": 2.5}, {"SKIP_NON_FINITE": 1}, {"SOLVER": 3}, {"CLIP_GRAD_NORM": "10"}, {"WARMUP_ITERS": "0"}):
        with pytest.raises(ValueError):
            config._merge({"TRAIN": bad}, copy.deepcopy(config.cfg))


class ToyNet:
    """the network face SolverWrapper uses (params dict, parameters(), forward(feed) -> layers, load()) on CPU tensors"""

    def __init__(self, seed):
        import torch
        g = torch.Generator().manual_seed(seed)
        mk = lambda *s: (torch.randn(*s, generator=g) * 0.3).requires_grad_(True)
        self.params = {"conv": [mk(4, 3, 3, 3), mk(4)], "fc": [mk(3, 4), mk(3)], "unused": [mk(2, 2), mk(2)]}
        self.poison = None                                           # iteration (0-based forward count) whose loss is NaN
        self.calls = 0

    def parameters(self):
        return [p for wb in self.params.values() for p in wb]

    def forward(self, feed):
        import torch
        import torch.nn.functional as Fn
        x = torch.as_tensor(np.asarray(feed["image_data"], np.float32)).permute(0, 3, 1, 2) / 255.0
        h = Fn.relu(Fn.conv2d(x, *self.params["conv"], padding=1)).mean(dim=(2, 3))
        out = Fn.linear(h, *self.params["fc"])
        if self.poison == self.calls:
            out = out * float("nan")
        self.calls += 1
        return {"logits": out}                                       # ("unused" never gets a gradient)

    def load(self, path, *a):                                        # a snapshot's .npy weight dict in the TF layouts (_tf_layout)
        import torch
        d = np.load(path, allow_pickle=True).item()
        with torch.no_grad():
            for name, (w, b) in self.params.items():
                a_ = d[name]["weights"]
                w.copy_(torch.as_tensor(a_.transpose(3, 2, 0, 1) if a_.ndim == 4 else a_.T))
                b.copy_(torch.as_tensor(d[name]["biases"]))


class ToyImdb:
    num_classes = 2


class ToyLayer:
    def __init__(self, roidb):
        self.roidb, self.i = roidb, 0

    def forward(self):
        e = self.roidb[self.i % len(self.roidb)]
        self.i += 1
        return {"image_data": e["image"][None].astype(np.float32), "lidar_bv_data": e["lidar_bv"][None], "calib": e["calib"],
                "im_info": np.array([[8, 8, 1]], np.float32), "gt_boxes_bv": np.zeros((1, 5), np.float32),
                "gt_boxes_3d": np.zeros((1, 7), np.float32), "gt_boxes_corners": np.zeros((1, 25), np.float32)}


def toy_roidb(n):
    rng = np.random.RandomState(0)
    return [{"image": rng.randint(0, 255, (6, 8, 3)).astype(np.uint8), "lidar_bv": np.zeros((8, 8, 9), np.float32),
             "calib": np.zeros((4, 12), np.float32), "boxes": np.zeros((1, 4)), "k": k, "max_overlaps": np.array([1.0])} for k in range(n)]


def toy_total_loss(layers, sigma=3.0):
    loss = (layers["logits"] ** 2).mean() * 50.0
    z = loss.detach() * 0
    return loss, (loss, z, z, z)


class ToyRun:
    """SolverWrapper.train_model on a ToyNet with the toy loss and the toy data layer (restarted from frame `start` on a resume)"""

    def __init__(self, monkeypatch, out_dir, seed=4, first_frame=0):
        from mv3d_tf_amd.fast_rcnn import train_mv
        self.train_mv = train_mv
        monkeypatch.setattr(train_mv, "total_loss", toy_total_loss)

        def layer(roidb, nc):
            l = ToyLayer(roidb)
            l.i = first_frame
            return l

        monkeypatch.setattr(train_mv, "get_data_layer", layer)
        self.net = ToyNet(seed)
        self.sw = train_mv.SolverWrapper(None, None, self.net, ToyImdb(), toy_roidb(5), str(out_dir))
        self.lines = []
        self.sw.log = self.lines.append

    def train(self, max_iters, **kw):
        return self.sw.train_model(None, max_iters, **kw)

    def lrs(self):
        return [l.split("lr: ")[1] for l in self.lines if l.startswith("iter: ")]

    def weights(self):
        return [p.detach().clone() for p in self.net.parameters()]


TOY_CLIP = 30.0                   # the toy's gradient norms are 22, 141, 14, 11 over four iterations: the clip is active in the second
SGD_KEYS = dict(SOLVER='sgd', LEARNING_RATE=0.05, GAMMA=0.1, STEPSIZE=2, MOMENTUM=0.9, WEIGHT_DECAY=5e-4, CLIP_GRAD_NORM=TOY_CLIP,
                SKIP_NON_FINITE=True, DISPLAY=1, SNAPSHOT_ITERS=1000, IMS_PER_BATCH=1, WARMUP_ITERS=0)


def hand_replay(seed, iters, poison=None):
    """the same gradients through torch.optim.SGD and clip_grad_norm_ by hand: two groups, decay on ndim >= 2"""
    import torch
    net, layer = ToyNet(seed), ToyLayer(toy_roidb(5))
    ps = net.parameters()
    opt = torch.optim.SGD([{"params": [p for p in ps if p.ndim >= 2], "weight_decay": 5e-4}, {"params": [p for p in ps if p.ndim < 2], "weight_decay": 0.0}],
                          lr=0.05, momentum=0.9)
    norms = []
    for it in range(iters):
        for p in ps:
            p.grad = None
        loss, _ = toy_total_loss(net.forward(layer.forward()))
        loss.backward()
        for g in opt.param_groups:
            g["lr"] = 0.05 * 0.1 ** (it // 2)
        norms.append(float(torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None], TOY_CLIP)))
        opt.step()
    return net, opt, norms


def test_solver_wrapper_reference_is_adam_at_1e_5(monkeypatch, tmp_path):
    import torch
    with train_cfg(DISPLAY=1, SNAPSHOT_ITERS=1000, IMS_PER_BATCH=1, LEARNING_RATE=0.05, CLIP_GRAD_NORM=TOY_CLIP, SKIP_NON_FINITE=True, STEPSIZE=1):
        run = ToyRun(monkeypatch, tmp_path)                           # SOLVER = 'reference': none of the other keys is read
        run.train(3)
    opt = run.sw.optimizer
    assert type(opt) is torch.optim.Adam and [g["lr"] for g in opt.param_groups] == [1e-5] and opt.param_groups[0]["weight_decay"] == 0
    assert run.lrs() == ["0.000010"] * 3 and not any("grad norm" in l for l in run.lines)
    state = torch.load(os.path.join(str(tmp_path), [f for f in os.listdir(str(tmp_path)) if f.endswith(".optim.pt")][0]))
    assert state["solver"] == "reference" and state["iter"] == 3


def test_solver_wrapper_sgd_equals_a_hand_replay(monkeypatch, tmp_path):
    import torch
    from mv3d_tf_amd import optim
    with train_cfg(**SGD_KEYS):
        run = ToyRun(monkeypatch, tmp_path)
        run.train(4)
    assert run.lrs() == ["0.050000", "0.050000", "0.005000", "0.005000"]
    ref, ref_opt, norms = hand_replay(4, 4)
    assert max(norms) > TOY_CLIP > min(norms), norms                      # the clip is active in some steps and idle in others
    for a, b in zip(run.net.parameters(), ref.parameters()):
        assert torch.equal(a.detach(), b.detach())
    opt = run.sw.optimizer
    assert isinstance(opt, optim.SGD) and isinstance(opt, torch.optim.SGD)
    assert [(g["weight_decay"], sorted(p.ndim for p in g["params"])) for g in opt.param_groups] == [(5e-4, [2, 2, 4]), (0.0, [1, 1, 1])]
    for p, q in zip(run.net.parameters(), ref.parameters()):         # the same state as torch's: momentum_buffer
        if q in ref_opt.state:
            assert torch.equal(opt.state[p]["momentum_buffer"], ref_opt.state[q]["momentum_buffer"])
    grad_lines = [l for l in run.lines if l.startswith("grad norm: ")]
    assert grad_lines == ["grad norm: %.4f, clip: %.4f, skipped: 0" % (n, min(1.0, TOY_CLIP / (n + 1e-6))) for n in norms]
    c = opt.control()
    assert c["calls_total"] == 4 and c["skipped_total"] == 0 and c["skip"] == 0 and c["norm"] == norms[-1]


def test_solver_wrapper_weight_decay_reaches_the_matrices_only(monkeypatch, tmp_path):
    """a decay large enough to see, a zero rate schedule apart: with gradients identical, biases move as without decay"""
    import torch
    res = {}
    for wd in (0.0, 0.1):
        with train_cfg(**dict(SGD_KEYS, WEIGHT_DECAY=wd, CLIP_GRAD_NORM=0.0, SKIP_NON_FINITE=False)):
            run = ToyRun(monkeypatch, tmp_path / ("wd%g" % wd))
            run.train(1)                                              # one step from the same weights: the same gradients
            res[wd] = run
    assert not any("grad norm" in l for l in res[0.1].lines)          # both keys off: no line, no norm
    for (name, a), b in zip([(n, p) for n, wb in res[0.0].net.params.items() for p in wb], res[0.1].net.parameters()):
        if a.ndim >= 2 and name != "unused":
            assert not torch.equal(a.detach(), b.detach()), name
        else:
            assert torch.equal(a.detach(), b.detach()), name          # biases, and the tensors without a gradient


def test_solver_wrapper_skips_a_non_finite_step(monkeypatch, tmp_path):
    import torch
    with train_cfg(**SGD_KEYS):
        run = ToyRun(monkeypatch, tmp_path)
        run.train(2)
        opt = run.sw.optimizer
        before = [p.detach().clone() for p in run.net.parameters()]
        bufs = [opt.state[p]["momentum_buffer"].clone() for p in run.net.parameters() if p in opt.state]
        run.net.poison = run.net.calls                                # the next forward, by hand on the run's optimizer: a NaN loss
        layers = run.net.forward(ToyLayer(toy_roidb(5)).forward())
        for p in run.net.parameters():
            p.grad = None
        toy_total_loss(layers)[0].backward()
        assert bool(torch.isnan(run.net.params["fc"][0].grad).all())
        opt.step()
    bits = lambda t: t.detach().view(torch.int32)
    for a, b in zip(run.net.parameters(), before):
        assert torch.equal(bits(a), bits(b))
    for a, b in zip([opt.state[p]["momentum_buffer"] for p in run.net.parameters() if p in opt.state], bufs):
        assert torch.equal(bits(a), bits(b))
    c = opt.control()
    assert c["skip"] == 1 and c["skipped_total"] == 1 and c["calls_total"] == 3 and c["coef"] == 0.0 and np.isnan(c["norm"])


def test_solver_wrapper_logs_a_skipped_step(monkeypatch, tmp_path):
    import torch
    with train_cfg(**SGD_KEYS):
        run = ToyRun(monkeypatch, tmp_path)
        run.net.poison = 1                                            # iteration 2's loss is NaN
        run.train(3)
    ref, _, _ = hand_replay(4, 1)                                     # iteration 1 alone ...
    skipped = [l for l in run.lines if l.startswith("grad norm: ")]
    assert skipped[1] == "grad norm: nan, clip: 0.0000, skipped: 1" and skipped[0].endswith("skipped: 0") and skipped[2].endswith("skipped: 1")
    assert all(torch.isfinite(p).all() for p in run.net.parameters())
    moved = [not torch.equal(a.detach(), b.detach()) for a, b in zip(run.net.parameters(), ref.parameters())]
    assert moved == [True, True, True, True, False, False]            # ... then iteration 3 moved on from iteration 1's weights


def test_solver_wrapper_sgd_resume_continues_bit_for_bit(monkeypatch, tmp_path):
    import torch
    with train_cfg(**dict(SGD_KEYS, SNAPSHOT_ITERS=2)):
        whole = ToyRun(monkeypatch, tmp_path / "whole")
        whole.train(4)
        first = ToyRun(monkeypatch, tmp_path / "parts")
        first.train(2)
        snap = first.train_mv.snapshot_filename(str(tmp_path / "parts"), 1)
        state = torch.load(snap + ".optim.pt")
        assert state["solver"] == "sgd" and state["iter"] == 2
        second = ToyRun(monkeypatch, tmp_path / "parts", seed=99, first_frame=2)      # other weights: the snapshot's must win
        second.train(4, resume=snap)
        assert second.lrs() == ["0.005000", "0.005000"]               # the schedule continues from the stored iteration
        for a, b in zip(whole.net.parameters()[:4], second.net.parameters()[:4]):
            assert torch.equal(a.detach(), b.detach())
        for a, b in zip(whole.net.parameters()[:4], second.net.parameters()[:4]):
            assert torch.equal(whole.sw.optimizer.state[a]["momentum_buffer"], second.sw.optimizer.state[b]["momentum_buffer"])
    with train_cfg(**dict(SGD_KEYS, SOLVER='adam')):                  # an 'sgd' state under 'adam', and the other way round
        with pytest.raises(ValueError, match="'sgd'.*'adam'"):
            ToyRun(monkeypatch, tmp_path / "parts").train(4, resume=snap)
    with train_cfg(**dict(SGD_KEYS, SOLVER='adam', SNAPSHOT_ITERS=2)):
        adam = ToyRun(monkeypatch, tmp_path / "adam")
        adam.train(2)
        assert isinstance(adam.sw.optimizer, torch.optim.Adam) and adam.lrs() == ["0.050000", "0.050000"]
        asnap = adam.train_mv.snapshot_filename(str(tmp_path / "adam"), 1)
    with train_cfg(**SGD_KEYS):
        with pytest.raises(ValueError, match="'adam'.*'sgd'"):
            ToyRun(monkeypatch, tmp_path / "adam").train(4, resume=asnap)


def test_solver_wrapper_refuses_an_unknown_solver(monkeypatch, tmp_path):
    with train_cfg(SOLVER='momentum'):
        run = ToyRun(monkeypatch, tmp_path)
        with pytest.raises(ValueError, match="SOLVER"):
            run.train(1)
    assert run.sw.optimizer is None and run.net.calls == 0            # at the top of train_model: nothing ran


# =================================================================== the device
@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import _lib, optim
    assert _lib.lib().mv3d_adam_chunk_elements() == CHUNK and C.sizeof(_lib.StepControl) == 32 and C.sizeof(_lib.SolverTensor) == 56
    return dict(torch=torch, lib=_lib, optim=optim)


def dev(torch, a):
    return torch.as_tensor(np.array(a, order="C")).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Flat:
    """a device buffer of n + 8 elements and the view of n elements at element offset `off` (0: the allocation's own 256-byte
    alignment; 1 .. 3: a view no vector access may touch); the elements outside the view hold a sentinel"""

    def __init__(self, torch, values, off, dtype=None, sentinel=777.0):
        values = np.asarray(values)
        self.n, self.off = values.size, off
        self.buf = torch.full((self.n + 8,), sentinel, dtype=dtype or torch.float32, device="cuda")
        self.view = self.buf[off:off + self.n]
        if dtype is None:
            self.view.copy_(torch.as_tensor(np.array(values.reshape(-1))))             # (a copy: a shared case table is read-only)
        self.sentinel = sentinel
        assert self.view.numel() == self.n and self.buf.data_ptr() % 256 == 0

    def get(self):
        return host(self.view)

    def untouched_outside(self):
        b = host(self.buf.float())
        return (b[:self.off] == self.sentinel).all() and (b[self.off + self.n:] == self.sentinel).all()


def tables(gpu, rows):
    """rows [(param, grad, state0, state1, lowp: device views or None, weight_decay)] -> (device table, chunk -> tensor, chunk -> first,
    num_chunks), built as optim.py builds them"""
    torch, L = gpu["torch"], gpu["lib"]
    ptr = lambda t: t.data_ptr() if t is not None else None
    arr = (L.SolverTensor * max(len(rows), 1))()
    ct, cf = [np.zeros(0, np.int32)], [np.zeros(0, np.int32)]
    for k, (p, g, s0, s1, lp, wd) in enumerate(rows):
        n = g.numel()
        assert all(a is None or (a.numel() == n and a.is_contiguous() and a.is_cuda) for a in (p, g, s0, s1, lp))
        arr[k] = L.SolverTensor(ptr(p), ptr(g), ptr(s0), ptr(s1), n, ptr(lp), wd, 0)
        c = (n + CHUNK - 1) // CHUNK
        ct.append(np.full(c, k, np.int32)); cf.append(np.arange(c, dtype=np.int32))
    ct, cf = np.concatenate(ct), np.concatenate(cf)
    pad = lambda a: np.concatenate([a, np.zeros(1, np.int32)])        # (never empty: a table of no chunks still has an address)
    return dev(torch, np.frombuffer(bytes(arr), np.uint8)), dev(torch, pad(ct)), dev(torch, pad(cf)), int(ct.size)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream(gpu):
    return C.c_void_p(gpu["torch"].cuda.current_stream().cuda_stream)


def control_record(gpu, coef=1.0, skip=0, sumsq=0.0, norm=0.0, skipped_total=0, calls_total=0):
    """a 32-byte device record written by the test (what mv3d_grad_norm would leave)"""
    return dev(gpu["torch"], np.frombuffer(bytes(gpu["lib"].StepControl(sumsq, norm, coef, skip, skipped_total, calls_total, 0)), np.uint8))


def read_control(gpu, rec):
    return gpu["lib"].StepControl.from_buffer_copy(host(rec).tobytes())


# ------------------------------------------------------------------- the norm
def norm_run(gpu, grads, max_norm=0.0, guard=0, off=0, rec=None):
    """one mv3d_grad_norm over sentinel-framed copies of `grads` at element offset `off`; the partials workspace is framed too
    -> the control record as the library's struct"""
    torch, L = gpu["torch"], gpu["lib"]
    flats = [Flat(torch, g, off) for g in grads]
    tab, ct, cf, n = tables(gpu, [(None, f.view, None, None, None, 0.0) for f in flats])
    parts = torch.full((n + 8,), -5.0, dtype=torch.float64, device="cuda")
    rec = control_record(gpu) if rec is None else rec
    st = L.lib().mv3d_grad_norm(P(tab), P(ct), P(cf), n, max_norm, guard, P(parts), P(rec), stream(gpu))
    torch.cuda.synchronize()
    assert st == 0
    assert all(f.untouched_outside() for f in flats), "wrote outside a gradient"
    assert all(np.array_equal(bits(f.get()), bits(g)) for f, g in zip(flats, grads)), "a gradient was written"
    assert (host(parts[n:]) == -5.0).all(), "wrote past the partials"
    return read_control(gpu, rec), host(parts[:n])


def u64(x):
    return np.array([x], F64).view(np.uint64)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name,sizes", [("sizes", SIZES), ("wrap", (WRAP_SIZE,))])
def test_grad_norm_against_fsum(gpu, name, sizes):
    """every size in one call, gradient scales 1e-6 .. 1e3 across the tensors; one tensor of 1026 chunks (the finishing loop wraps).
    Inside the derived bound of the correctly rounded sum -- and the very bits of the numpy statement of the kernel's order"""
    grads, ref = norm_case(name)
    c, parts = norm_run(gpu, grads, max_norm=1.0)
    use = abs(c.sumsq - ref) / ref / R.sumsq_bound(sizes)
    print("grad norm %s: use of the fsum bound %.4f" % (name, use))
    assert use <= 1.0, (c.sumsq, ref, use)
    assert np.array_equal(parts.view(np.uint64), np.concatenate([R.chunk_partials(g) for g in grads]).view(np.uint64))
    assert u64(c.sumsq) == u64(R.sumsq_restated(grads))
    norm, coef, skip = R.control_rule(c.sumsq, 1.0, 0)
    assert bits(F32(c.norm)) == bits(norm) and bits(F32(c.coef)) == bits(coef) and c.skip == 0 and c.calls_total == 1


@pytest.mark.gpu
def test_grad_norm_of_no_chunks(gpu):
    for max_norm, guard in ((0.0, 0), (1e-9, 1)):
        c, _ = norm_run(gpu, [], max_norm=max_norm, guard=guard, rec=control_record(gpu, coef=0.5, skip=1, sumsq=3.0, norm=2.0))
        assert (c.sumsq, c.norm, c.coef, c.skip, c.skipped_total, c.calls_total) == (0.0, 0.0, 1.0, 0, 0, 1)


@pytest.mark.gpu
def test_grad_norm_order_is_a_function_of_the_sizes_alone(gpu):
    """the same values at element offsets 0 .. 3 of their buffers (16-byte aligned: vector loads; 1 .. 3: scalar loads of the same
    elements by the same threads) and in two repeated calls: the same 64 bits of sumsq, the same bits of coef"""
    grads, _ = norm_case("sizes")
    seen = set()
    for off in (0, 0, 1, 2, 3):
        c, parts = norm_run(gpu, grads, max_norm=0.25, off=off)
        seen.add((int(u64(c.sumsq)), int(bits(F32(c.coef))[0]), int(bits(F32(c.norm))[0]), parts.tobytes()))
    assert len(seen) == 1
    assert 0.0 < c.coef < 1.0


@pytest.mark.gpu
def test_grad_norm_coefficient_and_skip_rules(gpu):
    r = np.random.RandomState(35)
    g = [r.normal(0, 1, CHUNK + 3).astype(F32), r.normal(0, 1, 5).astype(F32)]
    ref = R.sumsq_ref(g)
    nrm = float(np.sqrt(ref))
    for max_norm in (0.0, 2.0 * nrm, nrm, 0.5 * nrm):                 # none; above, at and below the norm
        for guard in (0, 1):
            c, _ = norm_run(gpu, g, max_norm=max_norm, guard=guard)
            assert abs(c.sumsq - ref) / ref <= R.sumsq_bound([a.size for a in g])
            norm, coef, skip = R.control_rule(c.sumsq, max_norm, guard)
            assert (bits(F32(c.norm)), bits(F32(c.coef)), c.skip) == (bits(norm), bits(coef), 0), (max_norm, guard)
    assert c.coef < 1.0
    z = [np.zeros(CHUNK + 3, F32), np.zeros(5, F32)]                  # a zero gradient: 1 / 1e-6 >= 1
    c, _ = norm_run(gpu, z, max_norm=1.0, guard=1)
    assert (c.sumsq, c.norm, c.coef, c.skip) == (0.0, 0.0, 1.0, 0)
    for bad, at in ((np.nan, (0, 7)), (np.inf, (1, 4)), (np.nan, (0, CHUNK + 2)), (-np.inf, (0, 4095))):
        h = [a.copy() for a in g]
        h[at[0]][at[1]] = bad
        for guard, max_norm in ((0, 1.0), (1, 1.0), (0, 0.0), (1, 0.0)):
            c, _ = norm_run(gpu, h, max_norm=max_norm, guard=guard)
            norm, coef, skip = R.control_rule(np.nan if np.isnan(bad) else np.inf, max_norm, guard)
            assert c.skip == skip == guard
            assert np.isnan(c.sumsq) if np.isnan(bad) else c.sumsq == np.inf
            assert np.array_equal(np.array([c.norm, c.coef], F32), np.array([norm, coef], F32), equal_nan=True), (bad, guard, max_norm, c.coef)
    rec = control_record(gpu)                                         # zeroed once; three calls, the second skipped
    h = [a.copy() for a in g]
    h[1][0] = np.inf
    seen = [norm_run(gpu, x, max_norm=1.0, guard=1, rec=rec)[0] for x in (g, h, g)]
    assert [(c.skip, c.skipped_total, c.calls_total) for c in seen] == [(0, 0, 1), (1, 1, 2), (0, 1, 3)]
    assert seen[2].coef == seen[0].coef and u64(seen[2].sumsq) == u64(seen[0].sumsq)


# ------------------------------------------------------------------- the SGD step
def sgd_run(gpu, state, h, offs=(0, 0, 0), wds=None, skip=0, lowp=0, lowp_off=None, use_control=True):
    """state [(p, g, buf)] numpy -> the step's (p, buf) per tensor (and the 16-bit copies' bits); offs: element offsets of p, g, buf"""
    torch, L = gpu["torch"], gpu["lib"]
    wds = [tensor_decay(k) for k in range(len(state))] if wds is None else wds
    flats = [[Flat(torch, a, o) for a, o in zip(st, offs)] for st in state]
    lps = None
    if lowp:
        lps = [Flat(torch, st[0], lowp_off, dtype=torch.float16 if lowp == 1 else torch.bfloat16, sentinel=3.0) for st in state]
    tab, ct, cf, n = tables(gpu, [(fl[0].view, fl[1].view, fl[2].view, None, lps[k].view if lps else None, wds[k]) for k, fl in enumerate(flats)])
    rec = control_record(gpu, coef=h["coef"], skip=skip) if use_control else None
    st = L.lib().mv3d_sgd_step(P(tab), P(ct), P(cf), n, h["lr"], h["momentum"], P(rec), lowp, stream(gpu))
    torch.cuda.synchronize()
    assert st == 0
    for k, fl in enumerate(flats):
        assert all(f.untouched_outside() for f in fl), "wrote outside a tensor"
        assert np.array_equal(bits(fl[1].get()), bits(state[k][1])), "the gradient was written"
        assert lps is None or lps[k].untouched_outside(), "wrote outside a 16-bit copy"
    out = [(fl[0].get(), fl[2].get()) for fl in flats]
    if lps:
        return out, [host(l.view.view(torch.int16)).view(np.uint16) for l in lps]
    return out


@pytest.mark.gpu
def test_sgd_every_size_and_hyper_parameter_against_f64(gpu):
    """all sizes in one launch (only full chunks, a tail of 1 / 17 / 4095, one chunk short by one, 1 and 3 elements), momentum x lr x
    coef, weight decay 0 and 5e-4 alternating over the tensors, gradient scales 1e-6 .. 1e3 across them"""
    worst = np.zeros(2)
    for i, h in enumerate(sgd_hypers()):
        state = sgd_state(SIZES, seed=2000 + i)
        for k, (st, got) in enumerate(zip(state, sgd_run(gpu, state, h))):
            w = sgd_worst(got, st, h, tensor_decay(k))
            assert max(w) <= 1.0, (h, st[0].size, w)
            worst = np.maximum(worst, w)
    print("sgd: worst use of the f64 bounds (p, buf):", worst)


@pytest.mark.gpu
def test_sgd_vector_body_and_scalar_loop_agree_bit_for_bit(gpu):
    h = dict(lr=1e-3, momentum=0.9, coef=0.37)
    state = sgd_state((2 * CHUNK + 17, CHUNK, 2 * CHUNK), seed=7)
    base = sgd_run(gpu, state, h)
    for k, (st, got) in enumerate(zip(state, base)):
        assert max(sgd_worst(got, st, h, tensor_decay(k))) <= 1.0
    for offs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        for k, (a, b) in enumerate(zip(base, sgd_run(gpu, state, h, offs=offs))):
            for name, x, y in zip(("p", "buf"), a, b):
                assert np.array_equal(bits(x), bits(y)), (offs, k, name, int((bits(x) != bits(y)).sum()))


@pytest.mark.gpu
def test_sgd_first_step_leaves_the_gradient_in_the_buffer(gpu):
    """a zeroed buffer, coef 1, decay 0: buf == g bit for bit (torch's first step clones the gradient), with and without a record"""
    state = [(p, np.where(g == 0, F32(0), g), np.zeros_like(b)) for p, g, b in sgd_state((2 * CHUNK + 17, 3), seed=8)]
    for use_control in (True, False):
        out = sgd_run(gpu, state, dict(lr=0.1, momentum=0.9, coef=1.0), wds=[0.0, 0.0], use_control=use_control)
        for (p, g, _), (gp, gb) in zip(state, out):
            assert np.array_equal(bits(gb), bits(g))
            assert np.array_equal(bits(gp), bits(p - F32(0.1) * g))


def torch_lowp_bits(a, kind):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(torch.float16 if kind == "f16" else torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_sgd_16_bit_copy_is_the_rounded_parameter(gpu, kind):
    """destination at element offsets 0 (8-byte stores) and 1 .. 3 (the 2-byte stores), full chunks and a tail, the parameter aligned
    (vector body) and not (scalar loop): the copy is the rounding of the parameter the kernel wrote, as torch casts it"""
    code = 1 if kind == "f16" else 2
    h = dict(lr=0.1, momentum=0.9, coef=0.37)
    state = sgd_state((2 * CHUNK + 37,), seed=9)
    state[0][0][:6] = [65519.996, 65520.0, 1 + 2.0 ** -11, 1 + 2.0 ** -8, 2.0 ** -25, -0.0]    # f16 overflow, ties, an f16 subnormal
    state[0][1][:6] = 0.0
    state[0][2][:6] = 0.0
    for lowp_off in (0, 1, 2, 3):
        for offs in ((0, 0, 0), (1, 0, 0)):
            out, lp = sgd_run(gpu, state, h, offs=offs, wds=[0.0], lowp=code, lowp_off=lowp_off)
            assert max(sgd_worst(out[0], state[0], h, 0.0)) <= 1.0
            assert np.array_equal(bits(out[0][0][:6]), bits(state[0][0][:6]))      # g = buf = 0: these parameters stay, their roundings are the test
            assert np.array_equal(lp[0], torch_lowp_bits(out[0][0], kind)) and np.array_equal(lp[0], R.lowp_bits(out[0][0], kind))


# ------------------------------------------------------------------- the controlled Adam step
def adam_run(gpu, state, h, coef=1.0, wds=None, skip=0, ctl=True, lowp=0):
    """state [(p, g, m, v)] -> (p, m, v) per tensor through mv3d_adam_step_ctl (ctl) or mv3d_adam_step on the same values"""
    torch, L = gpu["torch"], gpu["lib"]
    wds = [0.0] * len(state) if wds is None else wds
    flats = [[Flat(torch, a, 0) for a in st] for st in state]
    lps = [Flat(torch, st[0], 0, dtype=torch.bfloat16, sentinel=3.0) for st in state] if lowp else None
    lp = lambda k: lps[k].view if lps else None
    if ctl:
        tab, ct, cf, n = tables(gpu, [(fl[0].view, fl[1].view, fl[2].view, fl[3].view, lp(k), wds[k]) for k, fl in enumerate(flats)])
        rec = control_record(gpu, coef=coef, skip=skip)
        st = L.lib().mv3d_adam_step_ctl(P(tab), P(ct), P(cf), n, h["lr"], h["b1"], h["b2"], h["eps"], h["t"], P(rec), lowp, stream(gpu))
    else:
        arr = (L.AdamTensor * len(state))(*[L.AdamTensor(*[f.view.data_ptr() for f in fl], fl[0].n, None) for fl in flats])
        _, ct, cf, n = tables(gpu, [(fl[0].view, fl[1].view, fl[2].view, fl[3].view, None, 0.0) for fl in flats])
        tab = dev(torch, np.frombuffer(bytes(arr), np.uint8))
        st = L.lib().mv3d_adam_step(P(tab), P(ct), P(cf), n, h["lr"], h["b1"], h["b2"], h["eps"], h["t"], 0, stream(gpu))
    torch.cuda.synchronize()
    assert st == 0
    for k, fl in enumerate(flats):
        assert all(f.untouched_outside() for f in fl) and np.array_equal(bits(fl[1].get()), bits(state[k][1]))
    out = [(fl[0].get(), fl[2].get(), fl[3].get()) for fl in flats]
    return (out, [host(l.view.view(torch.int16)).view(np.uint16) for l in lps]) if lps else out


@pytest.mark.gpu
@pytest.mark.parametrize("t", [1, 1000])
def test_controlled_adam_with_nothing_to_control_is_adam_step(gpu, t):
    h = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, t=t)
    state = adam_state(SIZES, seed=3000 + t)
    for a, b in zip(adam_run(gpu, state, h, ctl=True), adam_run(gpu, state, h, ctl=False)):
        for name, x, y in zip("pmv", a, b):
            assert np.array_equal(bits(x), bits(y)), (name, x.size)


@pytest.mark.gpu
def test_controlled_adam_against_f64(gpu):
    worst = np.zeros(3)
    for t in (1, 1000):
        h = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, t=t)
        state = adam_state(SIZES, seed=3100 + t)
        for st, got in zip(state, adam_run(gpu, state, h, coef=0.37, wds=[5e-4] * len(state))):
            w = adam_worst(got, st, h, 0.37, 5e-4)
            assert max(w) <= 1.0, (t, st[0].size, w)
            worst = np.maximum(worst, w)
    print("controlled adam: worst use of the f64 bounds (p, m, v):", worst)


# ------------------------------------------------------------------- a skipped step
@pytest.mark.gpu
def test_a_skipped_step_keeps_every_bit(gpu):
    sizes = (2 * CHUNK + 17, 3)
    s = sgd_state(sizes, seed=12)
    out, lp = sgd_run(gpu, s, dict(lr=0.1, momentum=0.9, coef=0.0), skip=1, lowp=2, lowp_off=0)
    for (p, g, b), (gp, gb), l in zip(s, out, lp):
        assert np.array_equal(bits(gp), bits(p)) and np.array_equal(bits(gb), bits(b))
        assert (l == torch_lowp_bits(np.full(p.size, 3.0, F32), "bf16")).all()                # the copy keeps what it held
    a = adam_state(sizes, seed=13)
    out, lp = adam_run(gpu, a, dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, t=2), coef=0.0, wds=[5e-4, 0.0], skip=1, lowp=2)
    for st, got, l in zip(a, out, lp):
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(got, (st[0], st[2], st[3])))
        assert (l == torch_lowp_bits(np.full(st[0].size, 3.0, F32), "bf16")).all()


@pytest.mark.gpu
def test_an_infinite_parameter_without_decay_stays_infinite(gpu):
    """weight_decay == 0: the decay product is not evaluated, so 0 * inf never appears"""
    p = np.array([np.inf, -np.inf, 1.0, 2.0] * (CHUNK // 2), F32)    # two full chunks: the vector body
    g, z = np.zeros_like(p), np.zeros_like(p)
    for state in ([(p, g, z)], [(p[:7], g[:7], z[:7])]):
        (gp, gb), = sgd_run(gpu, state, dict(lr=0.1, momentum=0.9, coef=0.37), wds=[0.0])
        assert np.array_equal(bits(gp), bits(state[0][0])) and not gb.any()
    (gp, gm, gv), = adam_run(gpu, [(p, g, z, z)], dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, t=1), coef=0.37, wds=[0.0])
    assert np.array_equal(bits(gp), bits(p))


# ------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_solver_refusals_write_nothing(gpu):
    torch, L = gpu["torch"], gpu["lib"]
    ERR = L.ERR_INVALID_ARG
    t = [torch.ones(8, device="cuda") for _ in range(4)]
    tab, ct, cf, n = tables(gpu, [(t[0], t[1], t[2], t[3], None, 0.0)])
    parts = torch.full((4,), -5.0, dtype=torch.float64, device="cuda")
    rec = control_record(gpu, coef=0.25, calls_total=9)
    s = stream(gpu)
    norm = lambda a=tab, b=ct, c=cf, k=1, mx=1.0, pa=parts, r=rec: L.lib().mv3d_grad_norm(P(a), P(b), P(c), k, mx, 1, P(pa), P(r), s)
    assert norm(a=None) == ERR and norm(b=None) == ERR and norm(c=None) == ERR and norm(pa=None) == ERR and norm(r=None) == ERR
    assert norm(k=-1) == ERR and norm(mx=-1.0) == ERR and norm(mx=float("inf")) == ERR and norm(mx=float("nan")) == ERR
    sgd = lambda a=tab, b=ct, c=cf, k=1, lr=0.1, mu=0.9, lowp=0: L.lib().mv3d_sgd_step(P(a), P(b), P(c), k, lr, mu, None, lowp, s)
    assert sgd(a=None) == ERR and sgd(b=None) == ERR and sgd(c=None) == ERR and sgd(k=-1) == ERR
    assert sgd(mu=1.0) == ERR and sgd(mu=-0.1) == ERR and sgd(mu=float("nan")) == ERR
    assert sgd(lr=-1e-3) == ERR and sgd(lr=float("inf")) == ERR and sgd(lr=float("nan")) == ERR and sgd(lowp=3) == ERR and sgd(lowp=-1) == ERR
    adam = lambda a=tab, b=ct, c=cf, k=1, b1=0.9, b2=0.999, step=1, lowp=0: \
        L.lib().mv3d_adam_step_ctl(P(a), P(b), P(c), k, 1e-3, b1, b2, 1e-8, step, P(rec), lowp, s)
    assert adam(a=None) == ERR and adam(b=None) == ERR and adam(c=None) == ERR and adam(k=-1) == ERR
    assert adam(step=0) == ERR and adam(b1=1.0) == ERR and adam(b2=1.0) == ERR and adam(lowp=3) == ERR
    assert sgd(k=0) == L.OK and adam(k=0) == L.OK                     # no chunks: accepted, nothing to do
    torch.cuda.synchronize()
    assert all(bool((x == 1).all()) for x in t) and bool((parts == -5.0).all())
    c = read_control(gpu, rec)
    assert (c.coef, c.calls_total, c.skip) == (0.25, 9, 0)


# ------------------------------------------------------------------- optim.SGD / optim.Adam
OPT_SHAPES = [(3,), (64, 9, 3, 3), (4096 * 3 + 17,), (513, 257), (1,)]      # of test_adam_update_and_moments_against_f64
CLIP = 100.0                                                            # the global norm is ~3.6e3 (the (513, 257) tensor at scale 10)


def optimizer_steps(gpu, make, states, check):
    """six steps, the last tensor joining at the third; before every step the kernel's own f32 state is read back, after it `check`
    (tensor index, before, after, control record) bounds that one step against f64"""
    torch = gpu["torch"]
    gen = torch.Generator().manual_seed(0)
    ps = [torch.randn(s, generator=gen).cuda().requires_grad_(True) for s in OPT_SHAPES]
    opt = make(ps)
    for it in range(6):
        before = []
        for k, x in enumerate(ps):
            if k == 4 and it < 2:
                x.grad = None
                before.append(None)
                continue
            x.grad = torch.randn(x.shape, generator=gen).cuda() * (10.0 ** (k - 2))
            st = opt.state.get(x, {})
            z = np.zeros(x.numel(), F32)
            before.append((host(x).reshape(-1).copy(), host(x.grad).reshape(-1).copy()) +
                          tuple(host(st[n]).reshape(-1).copy() if st else z for n in states) + (int(float(st["step"])) if "step" in st else 0,))
        opt.step()
        rec = read_control(gpu, opt.__dict__["_control"])
        grads = [host(x.grad).reshape(-1) for g in opt.param_groups for x in g["params"] if x.grad is not None]     # the launch's order
        ref = R.sumsq_ref(grads)
        assert abs(rec.sumsq - ref) / ref <= R.sumsq_bound([g.size for g in grads]) and u64(rec.sumsq) == u64(R.sumsq_restated(grads))
        norm, coef, skip = R.control_rule(rec.sumsq, CLIP, 1)
        assert (bits(F32(rec.norm)), bits(F32(rec.coef)), rec.skip, rec.calls_total) == (bits(norm), bits(coef), 0, it + 1) and rec.coef < 1
        c = opt.control()
        assert c == dict(norm=rec.norm, coef=rec.coef, skip=0, skipped_total=0, calls_total=it + 1)
        for k, (x, b) in enumerate(zip(ps, before)):
            if b is not None:
                check(opt, x, b, float(rec.coef), it)
    return ps, opt


@pytest.mark.gpu
def test_optim_sgd_against_f64_and_torch_state(gpu):
    torch = gpu["torch"]
    worst = np.zeros(2)
    groups = lambda ps: [{"params": [p for p in ps if p.ndim >= 2], "weight_decay": 5e-4}, {"params": [p for p in ps if p.ndim < 2], "weight_decay": 0.0}]

    def check(opt, x, b, coef, it):
        nonlocal worst
        wd = 5e-4 if x.ndim >= 2 else 0.0
        h = dict(lr=1e-2, momentum=0.9, coef=coef)
        w = sgd_worst((host(x).reshape(-1), host(opt.state[x]["momentum_buffer"]).reshape(-1)), b[:3], h, wd)
        assert max(w) <= 1.0, (it, x.shape, w)
        worst = np.maximum(worst, w)

    ps, opt = optimizer_steps(gpu, lambda ps: gpu["optim"].SGD(groups(ps), lr=1e-2, momentum=0.9, clip_grad_norm=CLIP, skip_non_finite=True),
                              ("momentum_buffer",), check)
    print("optim.SGD: worst use of the f64 bounds (p, buf):", worst)
    assert set(opt.state[ps[0]].keys()) == {"momentum_buffer"}
    qs = [x.detach().clone().requires_grad_(True) for x in ps]       # the state round-trips into torch's own class, and steps on from it
    ref = torch.optim.SGD(groups(qs), lr=1e-2, momentum=0.9)
    ref.load_state_dict(opt.state_dict())
    for x, q in zip(ps, qs):
        assert torch.equal(ref.state[q]["momentum_buffer"], opt.state[x]["momentum_buffer"])
        q.grad = torch.ones_like(q)
    ref.step()
    back = gpu["optim"].SGD(groups([x.detach().clone().requires_grad_(True) for x in ps]), lr=1e-2, momentum=0.9)
    back.load_state_dict(ref.state_dict())
    assert all(torch.equal(back.state[a]["momentum_buffer"], ref.state[b]["momentum_buffer"])
               for ga, gb in zip(back.param_groups, ref.param_groups) for a, b in zip(ga["params"], gb["params"]))


@pytest.mark.gpu
def test_optim_adam_with_clip_guard_and_decay_against_f64(gpu):
    worst = np.zeros(3)

    def check(opt, x, b, coef, it):
        nonlocal worst
        st = opt.state[x]
        t = b[4] + 1
        assert int(float(st["step"])) == t
        h = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, t=t)
        w = adam_worst((host(x).reshape(-1), host(st["exp_avg"]).reshape(-1), host(st["exp_avg_sq"]).reshape(-1)), b[:4], h, coef, 5e-4)
        assert max(w) <= 1.0, (it, x.shape, w)
        worst = np.maximum(worst, w)

    optimizer_steps(gpu, lambda ps: gpu["optim"].Adam(ps, lr=1e-3, weight_decay=5e-4, clip_grad_norm=CLIP, skip_non_finite=True),
                    ("exp_avg", "exp_avg_sq"), check)
    print("optim.Adam(clip, guard, decay): worst use of the f64 bounds (p, m, v):", worst)


@pytest.mark.gpu
def test_optim_skips_a_non_finite_step_and_counts_it(gpu):
    torch = gpu["torch"]
    for make in (lambda ps: gpu["optim"].SGD(ps, lr=1e-2, momentum=0.9, skip_non_finite=True),
                 lambda ps: gpu["optim"].Adam(ps, lr=1e-2, skip_non_finite=True)):
        ps = [torch.randn(CHUNK + 9, device="cuda").requires_grad_(True), torch.randn(5, device="cuda").requires_grad_(True)]
        opt = make(ps)
        for x in ps:
            x.grad = torch.randn_like(x)
        opt.step()
        keep = [x.detach().clone() for x in ps] + [v.clone() for x in ps for v in opt.state[x].values() if v.ndim]
        ps[1].grad[2] = float("nan")
        opt.step()
        now = [x.detach() for x in ps] + [v for x in ps for v in opt.state[x].values() if v.ndim]
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(now, keep))
        c = opt.control()
        assert (c["skip"], c["skipped_total"], c["calls_total"], c["coef"]) == (1, 1, 2, 0.0) and np.isnan(c["norm"])
        ps[1].grad[2] = 0.0
        opt.step()
        assert not torch.equal(ps[0].detach(), keep[0]) and opt.control()["skipped_total"] == 1 and opt.control()["calls_total"] == 3


@pytest.mark.gpu
def test_optim_adam_with_the_options_off_launches_no_norm(gpu):
    torch = gpu["torch"]
    ps = [torch.randn(CHUNK + 9, device="cuda").requires_grad_(True), torch.randn(5, device="cuda").requires_grad_(True)]
    opt = gpu["optim"].Adam(ps, lr=1e-3)
    for _ in range(2):
        for x in ps:
            x.grad = torch.randn_like(x)
        opt.step()
    assert "_control" not in opt.__dict__ and "_host_control" not in opt.__dict__
    assert all(isinstance(k[0], int) for k in opt.__dict__["_cache"]) and len(opt.__dict__["_cache"]) == 1      # the plain entry's tables alone
    assert not any("partials" in e for e in opt.__dict__["_cache"].values())
    assert opt.control() == dict(norm=0.0, coef=1.0, skip=0, skipped_total=0, calls_total=0)
    dec = gpu["optim"].Adam(ps, lr=1e-3, weight_decay=5e-4)          # decay alone: the controlled entry without a record, still no norm
    dec.step()
    assert "_control" not in dec.__dict__ and [k[0] for k in dec.__dict__["_cache"]] == ["ctl"]


# ------------------------------------------------------------------- train_net
@pytest.mark.gpu
def test_train_net_three_iterations_under_sgd(gpu, tmp_path, capsys):
    """the synthetic roidb of test_train_entry.py::test_train_net_two_iterations_and_snapshot under the scheduled SGD solver"""
    torch = gpu["torch"]
    from mv3d_tf_amd import synth
    from mv3d_tf_amd.fast_rcnn import train_mv
    from mv3d_tf_amd.networks import get_network

    class Imdb:
        num_classes = 2
        name = "synthetic"

    rng = np.random.RandomState(0)
    roidb = []
    for i in range(3):
        _, _, _, calib, (gt_bv, gt_3d, gt_cnr) = synth.rpn_head(40 + i, 76, 76, "peaky", return_gt=True)
        roidb.append({"image": rng.randint(0, 255, (96, 320, 3)).astype(np.uint8),
                      "lidar_bv": (rng.random_sample((608, 608, 9)) < 0.02).astype(np.float32), "calib": calib.astype(np.float64),
                      "gt_classes": np.ones(len(gt_bv), np.int32), "boxes": np.zeros((len(gt_bv), 4), np.float32),
                      "boxes_bv": gt_bv[:, :4], "boxes_3D": gt_3d[:, :6], "boxes_corners": gt_cnr[:, :24],
                      "max_overlaps": np.ones(len(gt_bv))})
    with train_cfg(IMS_PER_BATCH=1, DISPLAY=1, SNAPSHOT_ITERS=2, SOLVER='sgd', STEPSIZE=2, CLIP_GRAD_NORM=10.0, SKIP_NON_FINITE=True,
                   WEIGHT_DECAY=5e-4) as cfg:
        np.random.seed(cfg.RNG_SEED)
        net = get_network("MV3D_train")
        before = net.params["rpn_bbox_pred"][0].detach().clone()
        hist = train_mv.train_net(net, Imdb(), roidb, str(tmp_path), max_iters=3)
        pref = cfg.TRAIN.SNAPSHOT_PREFIX
    assert len(hist) == 3 and all(np.isfinite(h[0]) for h in hist)
    assert not torch.equal(before, net.params["rpn_bbox_pred"][0].detach())
    assert all(bool(torch.isfinite(w).all()) for w, _ in net.params.values())
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("iter: ")]
    assert [l.split("lr: ")[1] for l in lines] == ["0.001000", "0.001000", "0.000100"]
    norms = [l for l in out.splitlines() if l.startswith("grad norm: ")]
    assert len(norms) == 3 and all(l.endswith("skipped: 0") for l in norms)
    state = torch.load(os.path.join(str(tmp_path), pref + "_iter_3.ckpt.optim.pt"))
    assert state["solver"] == "sgd" and state["iter"] == 3
    assert any("momentum_buffer" in s for s in state["optimizer"]["state"].values())
