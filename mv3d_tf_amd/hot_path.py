"""Device-resident batches of the MV3D hot path (the path BASELINE.json's north_star names), bound once to the C-ABI
and replayed as plain kernel launches -- what bench.py times and what a training / serving loop drives.

    TrainPathBatch   BASELINE configs[2] path-only, B frames per batch:
        mv3d_proposal_3d (TRAIN cfg 12000 -> 2000)                          lib/rpn_msr/proposal_layer_tf.py:25-202
        per frame: mv3d_anchor_target_stage1 / stage2                       lib/rpn_msr/anchor_target_layer_tf.py:21-250
        per frame: mv3d_proposal_target_stage1 / stage2 (<= 128 sampled)    lib/rpn_msr/proposal_target_layer_tf.py:19-94
        mv3d_rois_3d_to_fv                                                  (third view; network.py:293-315 is a TODO)
        mv3d_roi_pool_forward_views_pair   BEV + RGB + FV, private 16-bit argmax plane  roi_pooling_op.cc:74-190 x 3 layers
        mv3d_roi_pool_backward_views_pair  BEV + RGB + FV: one launch of tiles          roi_pooling_op.cc:319-452 x 3 layers
    TestPathBatch    BASELINE configs[1] / configs[4] path: mv3d_proposal_3d (TEST cfg 6000 -> 300), FV ROIs,
        RoiPool forward on the three views.

The random subsamplings of the two target layers are ARGUMENTS of the C-ABI (index lists drawn by the caller from the
numpy global RNG): `setup()` runs the batch once with the host in the loop -- counts to the host,
`npr.permutation` draws exactly like the numpy-contract callables, index lists back to the device -- and keeps the lists
resident.  `run()` then replays the batch with NO host synchronisation: every launch reads device-resident inputs only.
(The dense layers between these calls -- VGG16 trunks, FC head, whose backward produces the RoiPool top_diff -- are not part
of the path; `top_diff` is a resident synthetic tensor.)
"""
import ctypes as C

import numpy as np
import torch

from . import ops
from ._lib import ProposalTargetParams, RoiGradView, RoiView, check, lib
from .rpn_msr.anchor_target_layer_tf import draw_subsamples
from .rpn_msr.proposal_target_layer_tf import draw_samples

TRAIN_CFG = dict(RPN_PRE_NMS_TOP_N=12000, RPN_POST_NMS_TOP_N=2000, RPN_NMS_THRESH=0.7, RPN_MIN_SIZE=5)   # config.py:126-148
TEST_CFG = dict(RPN_PRE_NMS_TOP_N=6000, RPN_POST_NMS_TOP_N=300, RPN_NMS_THRESH=0.7, RPN_MIN_SIZE=5)      # faster_rcnn_end2end.yml:15-20
# conv5_3 maps at stride 8 (no pool4): 608x608 BEV, 375x1242 RGB, 64x512 FV (BASELINE.json: "512x64 FV")
VIEW_MAPS = {"bev": (76, 76, 512), "rgb": (46, 155, 512), "fv": (8, 64, 512)}
VIEWS = ("bev", "rgb", "fv")


def _P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def synth_maps(batch, seed, device, views=VIEWS):
    """post-ReLU-like NHWC feature maps drawn on the device (~half zeros, rest U(0,2)), one per view"""
    g = torch.Generator(device=device).manual_seed(int(seed))
    out = {}
    for v in views:
        H, W, Cc = VIEW_MAPS[v]
        out[v] = torch.clamp(torch.rand((batch, H, W, Cc), generator=g, device=device) * 4.0 - 2.0, min=0.0)
    return out


class _Bound:
    """a list of (C function, prebuilt argument tuple): run() = the launches of one batch, nothing else"""

    def __init__(self):
        self.calls = []
        self.keep = []            # ctypes structs / tensors the argument tuples point into

    def add(self, fn, *args):
        self.calls.append((fn, args))

    def run(self):
        for fn, args in self.calls:
            rc = fn(*args)
            if rc:
                check(rc, fn.__name__)

    def run_marked(self, stream, marks):
        """run(), with a HIP event pair recorded on `stream` around every call whose C function name is a key of `marks`
        ({name: [(start, end), ...]} is appended to): the duration of a launch IN the batch's own launch sequence"""
        for fn, args in self.calls:
            pair = None
            if fn.__name__ in marks:
                pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                pair[0].record(stream)
            rc = fn(*args)
            if rc:
                check(rc, fn.__name__)
            if pair is not None:
                pair[1].record(stream)
                marks[fn.__name__].append(pair)


class TrainPathBatch:
    def __init__(self, frames, maps, stream=None, views=VIEWS, num_classes=2, top_diff_seed=0, cold_maps=True):
        """frames: list (len B) of synth.rpn_head(..., return_gt=True) tuples (host numpy); maps: {view: (B,H,W,C) device
        tensor}.  Everything is uploaded / allocated here; setup() must run once before run().  cold_maps: the maps are
        resident inputs that were written long before the batch runs (a ring of batches), not the output of a layer that
        just ran: the forward goes through mv3d_roi_pool_forward_views_cold (same results)."""
        self.cold_maps = bool(cold_maps)
        self.B = len(frames)
        self.views = tuple(views)
        self.stream = stream
        self.maps = maps
        dev = next(iter(maps.values())).device
        self.dev = dev
        t = lambda a, dt=np.float32: torch.as_tensor(np.ascontiguousarray(a, dt)).to(dev)
        self.prob = t(np.concatenate([f[0] for f in frames]))
        self.pred = t(np.concatenate([f[1] for f in frames]))
        self.info = t(np.concatenate([f[2] for f in frames]))
        self.calib = t(np.stack([f[3] for f in frames]))
        self.gt = [tuple(t(a) for a in f[4]) for f in frames]            # (gt_bv (G,5), gt_3d (G,7), gt_corners (G,25))
        self.H, self.W = int(self.prob.shape[1]), int(self.prob.shape[2])
        self.nc = int(num_classes)
        self.pparams = ops.proposal_params(TRAIN_CFG)
        from .fast_rcnn.config import cfg
        T = cfg.TRAIN
        self.aparams = ops.anchor_target_params(T)
        self.tparams = [ops.proposal_target_params(T, self.nc, b) for b in range(self.B)]
        self.anchor_cap = ops.anchor_debug_rows(T)
        self.top_diff_seed = top_diff_seed
        self.bound = None

    def _sid(self):
        return self.stream.cuda_stream if self.stream is not None else torch.cuda.current_stream().cuda_stream

    # ------------------------------------------------------------------ one pass with the host in the loop
    def setup(self):
        """Run the batch once, drawing the subsample index lists from the numpy global RNG (frame order, anchor targets
        before proposal targets within a frame), and bind the sync-free replay.  Returns self."""
        ctx = torch.cuda.stream(self.stream) if self.stream is not None else _Null()
        with ctx:
            self._setup()
        torch.cuda.synchronize()
        return self

    def _setup(self):
        dev, B, H, W, nc = self.dev, self.B, self.H, self.W, self.nc
        L = lib()
        N = H * W * 4
        bnd = _Bound()
        st = C.c_void_p(self._sid())
        # ---- proposal_layer_3d on the whole batch
        cap = L.mv3d_proposal_3d_capacity(H, W, C.byref(self.pparams))
        self.cap = cap
        _, self.prop = ops.proposal_3d_outputs(B, cap, dev)
        pws = torch.empty(max(L.mv3d_proposal_3d_workspace_bytes(B, H, W, C.byref(self.pparams)), 256), dtype=torch.uint8, device=dev)
        bv, img, b3, num, status = self.prop
        a = (_P(self.prob), _P(self.pred), B, H, W, _P(self.info), _P(self.calib), C.byref(self.pparams), _P(bv), _P(img),
             _P(b3), _P(num), _P(status), _P(pws), C.c_size_t(pws.numel()), st)
        check(L.mv3d_proposal_3d(*a), "mv3d_proposal_3d")
        bnd.add(L.mv3d_proposal_3d, *a)
        bnd.keep += [pws]
        nums = [int(v) for v in num.cpu().numpy()]
        if int(status.max().item()) & 1:
            raise ZeroDivisionError("float division")
        self.num_proposals = nums
        # ---- per frame: anchor targets, then proposal targets (the order of the reference's train graph is not
        # defined across the two py_funcs; this is the one the numpy-contract graph here uses)
        self.rpn_labels = torch.empty((B, N), dtype=torch.float32, device=dev)
        self.rpn_targets = torch.empty((B, N, 6), dtype=torch.float32, device=dev)
        self.anchors = torch.empty((B, self.anchor_cap, 5), dtype=torch.float32, device=dev)
        self.anchors_3d = torch.empty((B, self.anchor_cap, 7), dtype=torch.float32, device=dev)
        self.n_anchors = torch.empty((B,), dtype=torch.int32, device=dev)
        picks, self.S = [], []
        at_calls, pt_calls, at_frames, pt_frames = [], [], [], []
        for b in range(B):
            gt_bv, gt_3d, gt_cnr = self.gt[b]
            G = gt_bv.shape[0]
            info_b = self.info[b]
            # (one size for every frame of the batch: the batched entry takes a single workspace_bytes)
            aws = torch.empty(max(L.mv3d_anchor_target_workspace_bytes(H, W, max(g[0].shape[0] for g in self.gt)), 256),
                              dtype=torch.uint8, device=dev)
            cf = torch.empty((32 + N,), dtype=torch.uint8, device=dev)
            a1 = (H, W, _P(info_b), _P(gt_bv), _P(gt_3d), G, C.byref(self.aparams), _P(self.rpn_labels[b]),
                  _P(self.rpn_targets[b]), _P(cf[:32]), _P(cf[32:]), _P(aws), C.c_size_t(aws.numel()), st)
            check(L.mv3d_anchor_target_stage1(*a1), "mv3d_anchor_target_stage1")
            dis = draw_subsamples(cf, cf[32:], N)
            lists = [np.zeros(0, np.int32) if d is None else np.ascontiguousarray(d, np.int32) for d in dis]
            dl = ops.upload_packed(lists, dev) if sum(len(x) for x in lists) else [None, None, None]
            dl = [x if (x is not None and x.numel()) else None for x in dl]
            a2 = (H, W, C.byref(self.aparams), _P(dl[0]), len(lists[0]), _P(dl[1]), len(lists[1]), _P(dl[2]), len(lists[2]),
                  _P(self.rpn_labels[b]), _P(self.anchors[b]), _P(self.anchors_3d[b]), _P(self.n_anchors[b:b + 1]),
                  self.anchor_cap, _P(aws), C.c_size_t(aws.numel()), st)
            check(L.mv3d_anchor_target_stage2(*a2), "mv3d_anchor_target_stage2")
            at_calls += [(L.mv3d_anchor_target_stage1, a1), (L.mv3d_anchor_target_stage2, a2)]
            at_frames.append((gt_bv, gt_3d, G, cf, aws, dl, [len(x) for x in lists]))
            bnd.keep += [aws, cf, dl, info_b]
            # proposal targets of frame b on its num_proposals[b] rows
            R = nums[b]
            tws = torch.empty(max(L.mv3d_proposal_target_workspace_bytes(R, G), 256), dtype=torch.uint8, device=dev)
            counts = torch.empty((4,), dtype=torch.int32, device=dev)
            p1 = (_P(bv[b]), _P(b3[b]), R, _P(gt_bv), _P(gt_3d), G, C.byref(self.tparams[b]), _P(counts), _P(tws),
                  C.c_size_t(tws.numel()), st)
            check(L.mv3d_proposal_target_stage1(*p1), "mv3d_proposal_target_stage1")
            fg_pick, bg_pick = draw_samples(counts)
            pl = ops.upload_packed([np.ascontiguousarray(fg_pick, np.int32), np.ascontiguousarray(bg_pick, np.int32)], dev) \
                if len(fg_pick) + len(bg_pick) else [None, None]
            pl = [x if (x is not None and x.numel()) else None for x in pl]
            picks.append((p1, pl, len(fg_pick), len(bg_pick), tws, counts, gt_cnr))
            self.S.append(len(fg_pick) + len(bg_pick))
        # ---- sampled-ROI arrays of the whole batch (frame b's rows at [off_b, off_b + S_b), foreground first)
        St = sum(self.S)
        self.rois = {"bev": torch.empty((St, 5), dtype=torch.float32, device=dev),
                     "rgb": torch.empty((St, 5), dtype=torch.float32, device=dev),
                     "fv": torch.empty((St, 5), dtype=torch.float32, device=dev)}
        self.rois_3d = torch.empty((St, 7), dtype=torch.float32, device=dev)
        self.labels = torch.empty((St, 1), dtype=torch.int32, device=dev)
        self.bbox_targets = torch.empty((St, 24 * nc), dtype=torch.float32, device=dev)
        off = 0
        for b, (p1, pl, n_fg, n_bg, tws, counts, gt_cnr) in enumerate(picks):
            gt_bv, gt_3d, _ = self.gt[b]
            G = gt_bv.shape[0]
            S = n_fg + n_bg
            p2 = (_P(bv[b]), _P(b3[b]), nums[b], _P(gt_bv), _P(gt_3d), _P(gt_cnr), G, _P(self.calib[b]), C.byref(self.tparams[b]),
                  _P(pl[0]), n_fg, _P(pl[1]), n_bg, _P(self.rois["bev"][off:off + S]), _P(self.rois["rgb"][off:off + S]),
                  _P(self.labels[off:off + S]), _P(self.bbox_targets[off:off + S]), _P(self.rois_3d[off:off + S]), _P(tws),
                  C.c_size_t(tws.numel()), st)
            check(L.mv3d_proposal_target_stage2(*p2), "mv3d_proposal_target_stage2")
            pt_calls += [(L.mv3d_proposal_target_stage1, p1), (L.mv3d_proposal_target_stage2, p2)]
            pt_frames.append((gt_bv, gt_3d, gt_cnr, G, counts, tws, pl, n_fg, n_bg, off, S))
            bnd.keep += [pl, tws, counts]
            off += S
        # ---- the replay runs the target layers of ALL frames behind one launch of every kernel (mv3d_*_batch entries:
        # 3 + 2 launches for the anchor targets, 2 + 1 for the proposal targets, whatever the batch size)
        ptrs = lambda ts: (C.c_void_p * B)(*[0 if t is None else t.data_ptr() for t in ts])
        ints = lambda vs: (C.c_int * B)(*[int(v) for v in vs])
        A = at_frames
        a_gtbv, a_gt3d, a_G = ptrs([f[0] for f in A]), ptrs([f[1] for f in A]), ints([f[2] for f in A])
        a_cnt, a_fgh = ptrs([f[3][:32] for f in A]), ptrs([f[3][32:] for f in A])
        a_ws = ptrs([f[4] for f in A])
        a_wsz = min(f[4].numel() for f in A)
        a_d = [ptrs([f[5][k] for f in A]) for k in range(3)]
        a_n = [ints([f[6][k] for f in A]) for k in range(3)]
        bnd.add(L.mv3d_anchor_target_stage1_batch, B, H, W, _P(self.info), a_gtbv, a_gt3d, a_G, C.byref(self.aparams),
                _P(self.rpn_labels), _P(self.rpn_targets), a_cnt, a_fgh, a_ws, C.c_size_t(a_wsz), st)
        bnd.add(L.mv3d_anchor_target_stage2_batch, B, H, W, C.byref(self.aparams), a_d[0], a_n[0], a_d[1], a_n[1], a_d[2], a_n[2],
                _P(self.rpn_labels), _P(self.anchors), _P(self.anchors_3d), _P(self.n_anchors), self.anchor_cap, a_ws,
                C.c_size_t(a_wsz), st)
        P = pt_frames
        tpar = (ProposalTargetParams * B)(*self.tparams)
        p_bv, p_b3, p_nr = ptrs([bv[b] for b in range(B)]), ptrs([b3[b] for b in range(B)]), ints(nums)
        p_gtbv, p_gt3d, p_gtc = ptrs([f[0] for f in P]), ptrs([f[1] for f in P]), ptrs([f[2] for f in P])
        p_G, p_cnt, p_ws = ints([f[3] for f in P]), ptrs([f[4] for f in P]), ptrs([f[5] for f in P])
        p_wsz = (C.c_size_t * B)(*[f[5].numel() for f in P])
        p_cal = ptrs([self.calib[b] for b in range(B)])
        p_fg, p_bg = ptrs([f[6][0] for f in P]), ptrs([f[6][1] for f in P])
        p_nfg, p_nbg = ints([f[7] for f in P]), ints([f[8] for f in P])
        sl = lambda t: ptrs([t[f[9]:f[9] + f[10]] if f[10] else None for f in P])
        p_out = [sl(self.rois["bev"]), sl(self.rois["rgb"]), sl(self.labels), sl(self.bbox_targets), sl(self.rois_3d)]
        p_fv = sl(self.rois["fv"]) if "fv" in self.views else None         # third view's ROIs out of the same emit launch
        bnd.add(L.mv3d_proposal_target_stage1_batch, B, p_bv, p_b3, p_nr, p_gtbv, p_gt3d, p_G, tpar, p_cnt, p_ws, p_wsz, st)
        bnd.add(L.mv3d_proposal_target_stage2_batch, B, p_bv, p_b3, p_nr, p_gtbv, p_gt3d, p_gtc, p_G, p_cal, tpar, p_fg, p_nfg, p_bg,
                p_nbg, p_out[0], p_out[1], p_out[2], p_out[3], p_out[4], p_fv, p_ws, p_wsz, st)
        bnd.keep += [a_gtbv, a_gt3d, a_G, a_cnt, a_fgh, a_ws, a_d, a_n, tpar, p_bv, p_b3, p_nr, p_gtbv, p_gt3d, p_gtc, p_G, p_cnt,
                     p_ws, p_wsz, p_cal, p_fg, p_bg, p_nfg, p_nbg, p_out, p_fv]
        # ---- third view's ROIs, RoiPool forward + backward on every view
        self.tops, self.top_diff, self.bottom_diff = {}, {}, {}
        g = torch.Generator(device=dev).manual_seed(1000 + int(self.top_diff_seed))
        fwd = (RoiView * len(self.views))()
        bwd = (RoiGradView * len(self.views))()
        if "fv" in self.views:         # set-up pass: the stand-alone entry (the replay's emit launch writes the same rows)
            a = (_P(self.rois_3d), St, _P(self.rois["fv"]), st)
            check(L.mv3d_rois_3d_to_fv(*a), "mv3d_rois_3d_to_fv")
            self.rois_fv_setup = self.rois["fv"].clone()
        for k, v in enumerate(self.views):
            m = self.maps[v]
            Bm, Hm, Wm, Cm = m.shape
            top = torch.empty((St, 7, 7, Cm), dtype=torch.float32, device=dev)
            am = torch.empty((St, 7, 7, Cm), dtype=torch.int32, device=dev)
            td = torch.rand((St, 7, 7, Cm), generator=g, device=dev) * 2.0 - 1.0
            bd = torch.empty_like(m)
            self.tops[v], self.top_diff[v], self.bottom_diff[v] = (top, am), td, bd
            fwd[k] = RoiView(m.data_ptr(), self.rois[v].data_ptr(), top.data_ptr(), am.data_ptr(), 0.125, Bm, St, Hm, Wm, Cm)
            bwd[k] = RoiGradView(bd.data_ptr(), self.rois[v].data_ptr(), td.data_ptr(), am.data_ptr(), 0.125, Bm, St, Hm, Wm, Cm)
        # the RoiPool pair: forward with the private compact argmax plane, backward = one launch of LDS map tiles, no workspace
        # (mv3d_roi_pool_*_views_pair)
        af = (len(self.views), fwd, 7, 7, 1 if self.cold_maps else 0, st)
        ab = (len(self.views), bwd, 7, 7, None, C.c_size_t(0), st)
        self.fwd_fn = L.mv3d_roi_pool_forward_views_pair
        check(self.fwd_fn(*af), "mv3d_roi_pool_forward_views_pair")
        check(L.mv3d_roi_pool_backward_views_pair(*ab), "mv3d_roi_pool_backward_views_pair")
        bnd.add(self.fwd_fn, *af)
        bnd.add(L.mv3d_roi_pool_backward_views_pair, *ab)
        bnd.keep += [fwd, bwd]
        self.fwd_args, self.bwd_args = af, ab
        self.num_rois = St
        self.bound = bnd

    # ------------------------------------------------------------------ replay, no host sync
    def run(self):
        """Replay the batch as one in-order chain of launches on the batch's stream.  (Measured alternatives, all slower on
        this platform: per-frame side streams with event fork / join, 6.9 k vs 10.6 k frames/s -- a cross-queue hand-off costs
        tens of us; the anchor-target branch, which nothing on the path depends on, on a fourth stream without any event,
        176.7 vs 153.5 us per batch -- a fourth busy queue slows the other three down.)"""
        self.bound.run()

    def roi_forward(self):
        check(self.fwd_fn(*self.fwd_args), "mv3d_roi_pool_forward_views_pair")

    def roi_backward(self):
        check(lib().mv3d_roi_pool_backward_views_pair(*self.bwd_args), "mv3d_roi_pool_backward_views_pair")

    # algorithmic HBM bytes (the REFERENCE op's contract): maps once + rois + (top f32 + argmax i32) / (grad + argmax) +
    # map write -- 8 B per pooled value.  The pair itself moves 5: its argmax plane holds one-byte codes (roi_*_moved_bytes below)
    def roi_forward_bytes(self):
        return sum(self.maps[v].numel() * 4 + self.num_rois * 20 + self.num_rois * 49 * self.maps[v].shape[3] * 8 for v in self.views)

    def roi_backward_bytes(self):
        return sum(self.num_rois * 49 * self.maps[v].shape[3] * 8 + self.num_rois * 20 + self.maps[v].numel() * 4 for v in self.views)

    def roi_forward_moved_bytes(self):
        """what the pair's forward has to move at least: maps once + rois + top f32 + ONE code byte per pooled value"""
        return sum(self.maps[v].numel() * 4 + self.num_rois * 20 + self.num_rois * 49 * self.maps[v].shape[3] * 5 for v in self.views)

    def roi_backward_moved_bytes(self):
        """... and its backward: top_diff f32 + one code byte per pooled value + rois + the maps written once"""
        return sum(self.num_rois * 49 * self.maps[v].shape[3] * 5 + self.num_rois * 20 + self.maps[v].numel() * 4 for v in self.views)

    def snapshot(self):
        """host copies of every output of the batch (for replay == setup checks)"""
        ts = [*self.prop, self.rpn_labels, self.rpn_targets, self.n_anchors, self.rois_3d, self.labels, self.bbox_targets]
        ts += [self.rois[v] for v in ("bev", "rgb", "fv")]
        for v in self.views:
            ts += [self.tops[v][0], self.tops[v][1], self.bottom_diff[v]]
        return [x.cpu().numpy().copy() for x in ts]


class TestPathBatch:
    """proposal_layer_3d (TEST cfg) -> FV ROIs -> RoiPool forward on the views, B frames; R = B * 300 ROI rows
    (rows past a frame's count are zero boxes, as the fixed-shape serving graph pools them)."""

    def __init__(self, frames, maps, stream=None, views=VIEWS, cold_maps=False, want_argmax=True):
        """want_argmax=False: the inference graph's call (roi_pooling_op.roi_pool under no_grad: argmax_data = NULL -- the op's second
        output only feeds RoiPoolGrad, roi_pooling_op_grad.py:7-43); True: both outputs of the op, as the reference's kernel writes them"""
        self.B = len(frames)
        self.views = tuple(views)
        self.stream = stream
        self.maps = maps
        self.cold_maps = bool(cold_maps)
        self.want_argmax = bool(want_argmax)
        dev = next(iter(maps.values())).device
        self.dev = dev
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev)
        self.prob = t(np.concatenate([f[0] for f in frames]))
        self.pred = t(np.concatenate([f[1] for f in frames]))
        self.info = t(np.concatenate([f[2] for f in frames]))
        self.calib = t(np.stack([f[3] for f in frames]))
        self.pparams = ops.proposal_params(TEST_CFG)
        self.bound = None

    def setup(self):
        ctx = torch.cuda.stream(self.stream) if self.stream is not None else _Null()
        with ctx:
            dev, B = self.dev, self.B
            H, W = int(self.prob.shape[1]), int(self.prob.shape[2])
            L = lib()
            sid = self.stream.cuda_stream if self.stream is not None else torch.cuda.current_stream().cuda_stream
            st = C.c_void_p(sid)
            bnd = _Bound()
            cap = L.mv3d_proposal_3d_capacity(H, W, C.byref(self.pparams))
            _, self.prop = ops.proposal_3d_outputs(B, cap, dev)
            pws = torch.empty(max(L.mv3d_proposal_3d_workspace_bytes(B, H, W, C.byref(self.pparams)), 256), dtype=torch.uint8, device=dev)
            bv, img, b3, num, status = self.prop
            a = (_P(self.prob), _P(self.pred), B, H, W, _P(self.info), _P(self.calib), C.byref(self.pparams), _P(bv), _P(img),
                 _P(b3), _P(num), _P(status), _P(pws), C.c_size_t(pws.numel()), st)
            bnd.add(L.mv3d_proposal_3d, *a)
            R = B * cap
            self.rois = {"bev": bv.view(-1, 5), "rgb": img.view(-1, 5)}
            if "fv" in self.views:
                self.rois["fv"] = torch.empty((R, 5), dtype=torch.float32, device=dev)
                bnd.add(L.mv3d_rois_3d_to_fv, _P(b3.view(-1, 7)), R, _P(self.rois["fv"]), st)
            fwd = (RoiView * len(self.views))()
            self.tops = {}
            for k, v in enumerate(self.views):
                m = self.maps[v]
                Bm, Hm, Wm, Cm = m.shape
                top = torch.empty((R, 7, 7, Cm), dtype=torch.float32, device=dev)
                am = torch.empty((R, 7, 7, Cm), dtype=torch.int32, device=dev) if self.want_argmax else None
                self.tops[v] = (top, am)
                fwd[k] = RoiView(m.data_ptr(), self.rois[v].data_ptr(), top.data_ptr(), am.data_ptr() if am is not None else None, 0.125, Bm, R, Hm, Wm, Cm)
            self.fwd_args = (len(self.views), fwd, 7, 7, st)
            self.fwd_fn = L.mv3d_roi_pool_forward_views_cold if self.cold_maps else L.mv3d_roi_pool_forward_views
            bnd.add(self.fwd_fn, *self.fwd_args)
            bnd.keep += [pws, fwd]
            self.num_rois = R
            self.bound = bnd
            bnd.run()
        torch.cuda.synchronize()
        return self

    def run(self):
        self.bound.run()

    def roi_forward(self):
        check(self.fwd_fn(*self.fwd_args), "mv3d_roi_pool_forward_views")

    def roi_forward_bytes(self):
        per = 8 if self.want_argmax else 4                         # top f32 (+ argmax i32)
        return sum(self.maps[v].numel() * 4 + self.num_rois * 20 + self.num_rois * 49 * self.maps[v].shape[3] * per for v in self.views)


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False
