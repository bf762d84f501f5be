"""The optimizer step of the training entry (lib/fast_rcnn/train_mv.py:138-146: tf.train.AdamOptimizer(lr)) on this library's kernel:
`Adam` is torch.optim.Adam -- same constructor, same state (`step`, `exp_avg`, `exp_avg_sq` per parameter, so state_dict / load_state_dict and
the `.optim.pt` files of SolverWrapper are interchangeable) -- whose `step()` updates every f32 device parameter that has a gradient with
ONE launch of mv3d_adam_step (csrc/adam.hip) instead of torch's multi-tensor kernels (2.07 ms -> the HBM time of 28 B per element for the
214 M parameters of the 3-view graph).  Anything the kernel does not cover (amsgrad, maximize, capturable, non-f32 or host
parameters, sparse gradients) goes to torch's own step.

The solver around it (not in the reference, which leaves its MomentumOptimizer, exponential_decay and WEIGHT_DECAY commented out or
unread): `SGD` is torch.optim.SGD (state `momentum_buffer`) on mv3d_sgd_step; both classes take
`clip_grad_norm` (the global L2 norm every gradient is scaled to, torch.nn.utils.clip_grad_norm_'s rule; 0 = off) and
`skip_non_finite` (a step whose global norm is inf or NaN changes nothing) as keyword-only arguments.  With either on, a step is one
mv3d_grad_norm over ALL parameters that have a gradient, then the update launches, which read the clip coefficient and the skip flag
from a 32-byte device record: the host never waits for the norm; `control()` is the one read-back.  `weight_decay` (L2, added to the
gradient) rides in the same launches.  `Adam` with all three off calls mv3d_adam_step exactly as before.  A skipped step still counts
as a step: `state['step']` advances (the host does not read the flag), so Adam's bias corrections move on.  `learning_rate(it)` is the
step schedule of cfg.TRAIN."""
import ctypes as C

import numpy as np
import torch

from ._lib import AdamTensor, SolverTensor, StepControl, check, lib


def learning_rate(it, T=None):
    """the rate of 0-based iteration `it`: LEARNING_RATE * GAMMA ** (it // STEPSIZE), times min(1, (it + 1) / WARMUP_ITERS) when
    WARMUP_ITERS > 0 (T = cfg.TRAIN); computed in doubles on the host, handed to the launch by value"""
    if T is None:
        from .fast_rcnn.config import cfg
        T = cfg.TRAIN
    lr = float(T.LEARNING_RATE) * float(T.GAMMA) ** (int(it) // int(T.STEPSIZE))
    if int(T.WARMUP_ITERS) > 0:
        lr *= min(1.0, (int(it) + 1) / float(T.WARMUP_ITERS))
    return lr


def _kernel_tensor(p):
    return p.is_cuda and p.dtype == torch.float32 and p.grad.dtype == torch.float32 and not p.grad.is_sparse and p.is_contiguous() \
        and p.grad.is_contiguous()


class _KernelStep:
    """what Adam and SGD share: the 16-bit copies, the staged tensor tables, the norm launch with its control record, the host path"""

    def _init_kernel_step(self, clip_grad_norm, skip_non_finite):
        if not (float(clip_grad_norm) >= 0.0 and np.isfinite(clip_grad_norm)):
            raise ValueError("clip_grad_norm: a finite norm >= 0 (0 = no clipping)")
        self.clip_grad_norm, self.skip_non_finite = float(clip_grad_norm), bool(skip_non_finite)
        self.lowp = {}                                                # id(param) -> (16-bit tensor of its shape, stamp callback): see register_lowp

    def register_lowp(self, param, dst, on_written=None):
        """`dst` (float16 / bfloat16, param's number of elements, contiguous) receives the updated `param` in every step of this
        optimizer, in the launch that updates it (the copy a cast at the top of the next step would make).  on_written(param) is called
        after each such step (the owner records that the copy is current)."""
        if dst.numel() != param.numel() or not dst.is_contiguous() or dst.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("register_lowp: a contiguous float16 / bfloat16 tensor with the parameter's number of elements")
        self.lowp[id(param)] = (dst, on_written)
        self.__dict__.pop("_cache", None)

    def _lowp_rows(self, params):
        """(16-bit destination pointer or 0 per parameter, the launch's lowp_dtype)"""
        lp = [self.lowp.get(id(p)) for p in params]
        kinds = {l[0].dtype for l in lp if l}
        if len(kinds) > 1:
            raise ValueError("register_lowp: one 16-bit type per optimizer")
        return [l[0].data_ptr() if l else 0 for l in lp], 0 if not kinds else (1 if kinds.pop() == torch.float16 else 2)

    def _written(self, params):
        for p in params:
            l = self.lowp.get(id(p))
            if l and l[1]:
                l[1](p)

    def _tables_for(self, key, sizes, rows, record, dev):
        """device tables of one launch: the chunk tables depend on the tensors' sizes only (built once per parameter list); the tensor
        table (`rows`: one tuple of `record`'s fields per tensor -- pointers) is refilled in a pinned staging buffer and copied
        asynchronously on the step's stream whenever a row changed -- gradients are fresh allocations in a single-process step
        (zero_grad drops them), usually at the same addresses.
        Two staging buffers alternate, each with an event recorded after its copy: the host waits for that event before it rewrites
        the buffer (a host that runs ahead of the stream would otherwise hand step n the pointers of step n + 1).  The event has
        normally completed: the wait costs something only when the host is two refills ahead of the device."""
        cache = self.__dict__.setdefault("_cache", {})
        ent = cache.get(key)
        if ent is None:
            chunk = lib().mv3d_adam_chunk_elements()
            ct, cf = [], []
            for k, numel in enumerate(sizes):
                n = (numel + chunk - 1) // chunk
                ct.append(np.full(n, k, np.int32)); cf.append(np.arange(n, dtype=np.int32))
            ct_dev = torch.from_numpy(np.concatenate(ct)).to(dev)
            cf_dev = torch.from_numpy(np.concatenate(cf)).to(dev)
            nbytes = C.sizeof(record) * len(sizes)
            ent = {"ct": ct_dev, "cf": cf_dev, "n": int(ct_dev.numel()),
                   "pin": [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(2)],
                   "copied": [torch.cuda.Event() for _ in range(2)], "fills": 0,
                   "dev": torch.empty(nbytes, dtype=torch.uint8, device=dev), "ptrs": None}
            cache[key] = ent
        if rows != ent["ptrs"]:
            slot = ent["fills"] & 1
            ent["fills"] += 1
            pin, copied = ent["pin"][slot], ent["copied"][slot]
            copied.synchronize()                                      # (this buffer's last copy has read it; at once if never recorded)
            arr = (record * len(sizes)).from_buffer(pin.numpy())
            for k, row in enumerate(rows):
                arr[k] = record(*row)
            ent["dev"].copy_(pin, non_blocking=True)                  # (stream-ordered before the launch below)
            copied.record(torch.cuda.current_stream(dev))
            ent["ptrs"] = rows
        return ent

    def _solver_tables(self, key, items, weight_decay, dev):
        """the mv3d_solver_tensor table of `items` = [(param, state0, state1 or None)] -> (table entry, lowp_dtype)"""
        lp, kind = self._lowp_rows([it[0] for it in items])
        rows = tuple((p.data_ptr(), p.grad.data_ptr(), s0.data_ptr(), s1.data_ptr() if s1 is not None else None, p.numel(), q or None,
                      float(weight_decay), 0) for (p, s0, s1), q in zip(items, lp))
        return self._tables_for(key, [it[0].numel() for it in items], rows, SolverTensor, dev), kind

    # ---------------------------------------------------------------------------------------------- norm, clip coefficient, guard
    def _controlled(self):
        return self.clip_grad_norm > 0.0 or self.skip_non_finite

    def _grad_norm(self, params, dev):
        """ONE mv3d_grad_norm over `params` (every parameter of the step that has a gradient): the control record's device pointer"""
        ctl = self.__dict__.get("_control")
        if ctl is None:
            ctl = self.__dict__["_control"] = torch.zeros(C.sizeof(StepControl), dtype=torch.uint8, device=dev)   # zeroed once
        rows = tuple((None, p.grad.data_ptr(), None, None, p.numel(), None, 0.0, 0) for p in params)
        ent = self._tables_for(("norm", tuple(id(p) for p in params)), [p.numel() for p in params], rows, SolverTensor, dev)
        if "partials" not in ent:
            ent["partials"] = torch.empty(max(ent["n"], 1), dtype=torch.float64, device=dev)
        check(lib().mv3d_grad_norm(C.c_void_p(ent["dev"].data_ptr()), C.c_void_p(ent["ct"].data_ptr()), C.c_void_p(ent["cf"].data_ptr()),
                                   ent["n"], self.clip_grad_norm, int(self.skip_non_finite), C.c_void_p(ent["partials"].data_ptr()),
                                   C.c_void_p(ctl.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "mv3d_grad_norm")
        return C.c_void_p(ctl.data_ptr())

    def control(self):
        """the one read-back of the control record (32 bytes; synchronises with the stream): what the LAST step's norm launch left --
        dict(norm, coef, skip, skipped_total, calls_total).  On the host path the same figures, kept on the host.  Before the first
        controlled step: zeros with coef 1."""
        ctl = self.__dict__.get("_control")
        if ctl is not None:
            c = StepControl.from_buffer_copy(ctl.cpu().numpy().tobytes())
            return dict(norm=float(c.norm), coef=float(c.coef), skip=int(c.skip), skipped_total=int(c.skipped_total),
                        calls_total=int(c.calls_total))
        return dict(self.__dict__.get("_host_control") or dict(norm=0.0, coef=1.0, skip=0, skipped_total=0, calls_total=0))

    def _host_step(self, torch_step):
        """the same rule through torch: clip_grad_norm_ over every parameter that has a gradient, a host isfinite test, torch's step"""
        if self._controlled():
            params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
            h = self.__dict__.setdefault("_host_control", dict(norm=0.0, coef=1.0, skip=0, skipped_total=0, calls_total=0))
            norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad.detach().float()) for p in params]))) \
                if params else 0.0
            skip = int(self.skip_non_finite and not np.isfinite(norm))
            coef = 0.0 if skip else 1.0
            if not skip and self.clip_grad_norm > 0.0 and params:
                norm = float(torch.nn.utils.clip_grad_norm_(params, self.clip_grad_norm))
                coef = float(min(1.0, self.clip_grad_norm / (norm + 1e-6)))
            h.update(norm=norm, coef=coef, skip=skip, skipped_total=h["skipped_total"] + skip, calls_total=h["calls_total"] + 1)
            if skip:
                return
        torch_step()

    def _device_of_step(self, covered):
        """the device of a kernel step, or None for the host path: every parameter that has a gradient is an f32 contiguous tensor on
        ONE device and every group is one the kernels cover (`covered(group)`)"""
        dev = None
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                if not (covered(g) and _kernel_tensor(p)) or (dev is not None and p.device != dev):
                    return None
                dev = p.device
        return dev


class Adam(_KernelStep, torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, *, clip_grad_norm=0.0, skip_non_finite=False, **kw):
        kw.pop("fused", None)                                        # (this class IS the fused step)
        super().__init__(params, lr=lr, betas=betas, eps=eps, **kw)
        self._init_kernel_step(clip_grad_norm, skip_non_finite)

    def _covered(self, g):
        return not (g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("differentiable"))

    def _state_of(self, p):
        st = self.state[p]
        if len(st) == 0:                                              # torch.optim.Adam's own lazy state
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._controlled() or any(g.get("weight_decay") for g in self.param_groups):
            self._step_controlled()
            return loss
        rest = []
        for gi, g in enumerate(self.param_groups):
            items = []
            for p in g["params"]:
                if p.grad is None:
                    continue
                if not (self._covered(g) and _kernel_tensor(p)):             # (no group has weight_decay on this path)
                    rest.append(gi)
                    items = None
                    break
                st = self._state_of(p)
                items.append((p, st["exp_avg"], st["exp_avg_sq"]))
            if not items:
                continue
            # one step count per launch: parameters that joined later (a gradient for the first time) keep their own count in `state`;
            # the launch is cut by count so that every tensor gets its own bias corrections
            by_step = {}
            for it in items:
                by_step.setdefault(int(float(self.state[it[0]]["step"])), []).append(it)
            for t0, its in by_step.items():
                dev = its[0][0].device
                lp, kind = self._lowp_rows([p for p, _, _ in its])
                rows = tuple((p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), q or None) for (p, m, v), q in zip(its, lp))
                ent = self._tables_for((gi, tuple(id(p) for p, _, _ in its)), [p.numel() for p, _, _ in its], rows, AdamTensor, dev)
                t_dev, ct_dev, cf_dev, n = ent["dev"], ent["ct"], ent["cf"], ent["n"]
                b1, b2 = g["betas"]
                check(lib().mv3d_adam_step(C.c_void_p(t_dev.data_ptr()), C.c_void_p(ct_dev.data_ptr()), C.c_void_p(cf_dev.data_ptr()), n,
                                           float(g["lr"]), float(b1), float(b2), float(g["eps"]), t0 + 1, kind,
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "mv3d_adam_step")
                for p, _, _ in its:
                    self.state[p]["step"] += 1
                self._written([p for p, _, _ in its])
        if rest:                                                      # whatever the kernel does not cover: torch's own update for those groups
            keep = self.param_groups
            try:
                self.param_groups = [keep[i] for i in sorted(set(rest))]
                super().step()
            finally:
                self.param_groups = keep
        return loss

    def _step_controlled(self):
        """clipping, the guard or weight decay: one norm launch over all gradients (clipping / guard only), then one
        mv3d_adam_step_ctl per (group, step count)"""
        dev = self._device_of_step(self._covered)
        if dev is None:
            return self._host_step(super().step)
        groups = [(gi, g, [p for p in g["params"] if p.grad is not None]) for gi, g in enumerate(self.param_groups)]
        every = [p for _, _, ps in groups for p in ps]
        if not every:
            return
        ctl = self._grad_norm(every, dev) if self._controlled() else None
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for gi, g, ps in groups:
            by_step = {}
            for p in ps:
                st = self._state_of(p)
                by_step.setdefault(int(float(st["step"])), []).append((p, st["exp_avg"], st["exp_avg_sq"]))
            for t0, its in by_step.items():
                ent, kind = self._solver_tables(("ctl", gi, tuple(id(p) for p, _, _ in its)), its, g.get("weight_decay") or 0.0, dev)
                b1, b2 = g["betas"]
                check(lib().mv3d_adam_step_ctl(C.c_void_p(ent["dev"].data_ptr()), C.c_void_p(ent["ct"].data_ptr()),
                                               C.c_void_p(ent["cf"].data_ptr()), ent["n"], float(g["lr"]), float(b1), float(b2),
                                               float(g["eps"]), t0 + 1, ctl, kind, stream), "mv3d_adam_step_ctl")
                for p, _, _ in its:
                    self.state[p]["step"] += 1                        # (also under skip: the host does not read the flag)
                self._written([p for p, _, _ in its])


class SGD(_KernelStep, torch.optim.SGD):
    """torch.optim.SGD -- same constructor, same state (`momentum_buffer`) -- whose step is one mv3d_sgd_step per group.  nesterov,
    dampening, maximize, momentum 0 (torch keeps no buffer then) or a host or non-f32 parameter go to torch's own step."""

    def __init__(self, params, lr=1e-3, momentum=0.0, *, clip_grad_norm=0.0, skip_non_finite=False, **kw):
        kw.pop("fused", None)
        super().__init__(params, lr=lr, momentum=momentum, **kw)
        self._init_kernel_step(clip_grad_norm, skip_non_finite)

    def _covered(self, g):
        return 0.0 < g["momentum"] < 1.0 and not (g.get("nesterov") or g.get("dampening") or g.get("maximize") or g.get("differentiable"))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        dev = self._device_of_step(self._covered)
        if dev is None:
            self._host_step(super().step)
            return loss
        groups = [(gi, g, [p for p in g["params"] if p.grad is not None]) for gi, g in enumerate(self.param_groups)]
        every = [p for _, _, ps in groups for p in ps]
        if not every:
            return loss
        ctl = self._grad_norm(every, dev) if self._controlled() else None
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for gi, g, ps in groups:
            if not ps:
                continue
            items = []
            for p in ps:
                st = self.state[p]
                if st.get("momentum_buffer") is None:                 # a zeroed buffer: the first step leaves torch's buf = g' in it
                    st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                items.append((p, st["momentum_buffer"], None))
            ent, kind = self._solver_tables((gi, tuple(id(p) for p in ps)), items, g.get("weight_decay") or 0.0, dev)
            check(lib().mv3d_sgd_step(C.c_void_p(ent["dev"].data_ptr()), C.c_void_p(ent["ct"].data_ptr()), C.c_void_p(ent["cf"].data_ptr()),
                                      ent["n"], float(g["lr"]), float(g["momentum"]), ctl, kind, stream), "mv3d_sgd_step")
            self._written(ps)
        return loss
