"""Tensor-level calls into libmv3d_hip.so.

torch CUDA(ROCm) tensors are used only as device buffers: every function passes
`tensor.data_ptr()` and the current stream handle through the C-ABI and returns tensors
holding the results.  Nothing here synchronises with the host unless it says so.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import AnchorTargetParams, ProposalParams, ProposalTargetParams, RoiGradView, RoiView, check, lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _dev(t, dtype=torch.float32, device=None):
    """numpy / tensor -> contiguous device tensor of dtype (the placeholder cast of the graph)."""
    if isinstance(t, torch.Tensor):
        return t.to(device=device or (t.device if t.is_cuda else "cuda"), dtype=dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(t), dtype=dtype).to(device or "cuda")


_ws_cache = {}


def upload_packed(arrays, device):
    """Several small host arrays (f32 / i32, any shape) -> ONE host-to-device copy; returns device views with the
    arrays' shapes (4-byte slots; an int32 array comes back as an int32 view)."""
    flat = [np.ascontiguousarray(a, np.int32 if np.issubdtype(np.asarray(a).dtype, np.integer) else np.float32) for a in arrays]
    sizes = [a.size for a in flat]
    host = np.empty((max(sum(sizes), 1),), np.float32)
    o = 0
    for a, n in zip(flat, sizes):
        host[o:o + n] = a.reshape(-1).view(np.float32)
        o += n
    devbuf = torch.from_numpy(host).to(device)
    views, o = [], 0
    for a, n in zip(flat, sizes):
        v = devbuf[o:o + n]
        if a.dtype == np.int32:
            v = v.view(torch.int32)
        views.append(v.view(a.shape))
        o += n
    return views


def packed_views(spec, device):
    """spec: [(shape, torch dtype of 4 bytes)] -> (pack f32 buffer, views): outputs that a host consumer fetches with
    ONE device-to-host copy (`unpack_host`)."""
    sizes = [int(np.prod(sh)) for sh, _ in spec]
    pack = torch.empty((max(sum(sizes), 1),), dtype=torch.float32, device=device)
    views, o = [], 0
    for (sh, dt), n in zip(spec, sizes):
        v = pack[o:o + n]
        if dt != torch.float32:
            v = v.view(dt)
        views.append(v.view(sh))
        o += n
    return pack, views


def unpack_host(pack, spec):
    host = pack.cpu().numpy()
    outs, o = [], 0
    for sh, dt in spec:
        n = int(np.prod(sh))
        a = host[o:o + n]
        if dt != torch.float32:
            a = a.view(np.int32)
        outs.append(a.reshape(sh))
        o += n
    return outs


def _workspace(nbytes, device, tag):
    """Reused per (device, stream, tag) so hot calls never allocate (buffers are 256-B aligned).  Uninitialised: every kernel
    that takes a workspace writes what it reads."""
    key = (str(device), torch.cuda.current_stream().cuda_stream, tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


# ------------------------------------------------------------------ proposal_layer_3d
def proposal_params(cfg_section, feat_stride=8, img_height=375, img_width=1242, img_padding=50, use_gpu_nms=None):
    """cfg[cfg_key] section (lib/rpn_msr/proposal_layer_tf.py:52-55) -> mv3d_proposal_params.  `use_gpu_nms` (default:
    cfg.USE_GPU_NMS) selects the rule of the NMS inside the layer the way nms_wrapper.py:13-21 does."""
    if use_gpu_nms is None:
        from .fast_rcnn.config import cfg
        use_gpu_nms = bool(cfg.USE_GPU_NMS)
    return ProposalParams(int(feat_stride), int(cfg_section["RPN_PRE_NMS_TOP_N"]),
                          int(cfg_section["RPN_POST_NMS_TOP_N"]), int(img_height), int(img_width),
                          int(img_padding), 1 if use_gpu_nms else 0, 0, float(cfg_section["RPN_NMS_THRESH"]),
                          float(cfg_section["RPN_MIN_SIZE"]))


def anchor_target_params(T, feat_stride=8):
    """cfg.TRAIN (anchor_target_layer_tf.py:125-143) -> mv3d_anchor_target_params"""
    return AnchorTargetParams(int(feat_stride), 1 if T["RPN_CLOBBER_POSITIVES"] else 0, float(T["RPN_NEGATIVE_OVERLAP"]),
                              float(T["RPN_POSITIVE_OVERLAP"]))


def anchor_debug_rows(T):
    """capacity of anchor_target_layer's debug outputs (anchors, anchors_3d): at most RPN_BATCHSIZE labelled anchors survive
    the draws of :146-159, and the relabel of :176 can add as many again before the last draw"""
    return max(int(T["RPN_BATCHSIZE"]), 1) * 2


def proposal_target_params(T, num_classes, frame_index=0):
    """cfg.TRAIN (proposal_target_layer_tf.py:246-260) -> mv3d_proposal_target_params; `frame_index` is the batch column of
    the ground-truth rows a batched caller appends to frame b's proposals (0 in the reference)"""
    return ProposalTargetParams(int(num_classes), int(frame_index), float(T["FG_THRESH"]), float(T["BG_THRESH_HI"]),
                                float(T["BG_THRESH_LO"]))


def proposal_3d_outputs(B, cap, dev):
    """The five outputs of proposal_3d as views of ONE buffer (bv | img | 3d | num | status, 4-byte slots), so that
    a host consumer fetches them with a single device-to-host copy.  Returns (pack, (bv, img, b3, num, status))."""
    n5, n7 = B * cap * 5, B * cap * 7
    pack = torch.empty((2 * n5 + n7 + 2 * B,), dtype=torch.float32, device=dev)
    bv = pack[:n5].view(B, cap, 5)
    img = pack[n5:2 * n5].view(B, cap, 5)
    b3 = pack[2 * n5:2 * n5 + n7].view(B, cap, 7)
    tail = pack[2 * n5 + n7:].view(torch.int32)
    return pack, (bv, img, b3, tail[:B], tail[B:])


def anchor_mask_tensor(anchor_mask, B, N, device):
    """An empty-anchor mask as the kernels take it: numpy / tensor, bool or uint8, (N,) or (B, N) -> contiguous (B, N) uint8
    device tensor (None stays None)."""
    if anchor_mask is None:
        return None
    if isinstance(anchor_mask, torch.Tensor):
        m = anchor_mask.to(device=device)
        m = (m if m.dtype == torch.uint8 else (m != 0).to(torch.uint8))
    else:
        m = torch.as_tensor(np.ascontiguousarray(np.asarray(anchor_mask) != 0).view(np.uint8)).to(device)
    if m.numel() != B * N:
        raise ValueError("anchor_mask: %d entries for %d frames of %d anchors" % (m.numel(), B, N))
    return m.reshape(B, N).contiguous()


def anchor_occupancy(bev, H, W, feat_stride=8, min_cells=1, want_counts=False, out=None):
    """The paper's empty-anchor rule (include/mv3d_hip.h: mv3d_anchor_occupancy; not in the reference).  bev (B,Hm,Wm,C) or
    (Hm,Wm,C) f32 device tensor, the RAW bird's-eye-view map; H, W the RPN head's grid.  Returns mask (B, 4 H W) u8 -- 1 = at
    least `min_cells` occupied cells under the anchor -- and, with want_counts, (mask, counts (B, 4 H W) i32).
    out = (mask, counts or None) reuses buffers.  Asynchronous, two launches."""
    if bev.dim() == 3:
        bev = bev.unsqueeze(0)
    if bev.dtype != torch.float32 or not bev.is_cuda:
        raise TypeError("anchor_occupancy: a float32 device tensor (B, Hm, Wm, C), got %s on %s" % (bev.dtype, bev.device))
    bev = bev.contiguous()
    B, Hm, Wm, Cc = (int(v) for v in bev.shape)
    N = 4 * int(H) * int(W)
    dev = bev.device
    if out is None:
        mask = torch.empty((B, N), dtype=torch.uint8, device=dev)
        counts = torch.empty((B, N), dtype=torch.int32, device=dev) if want_counts else None
    else:
        mask, counts = out
        for t, dt, what in ((mask, torch.uint8, "mask"), (counts, torch.int32, "counts")):
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == dt and t.device == dev and tuple(t.shape) == (B, N) and t.is_contiguous()):
                raise ValueError("anchor_occupancy: out %s must be a contiguous %s tensor of shape (%d, %d) on %s" % (what, dt, B, N, dev))
        if mask is None or (want_counts and counts is None):
            raise ValueError("anchor_occupancy: out = (mask, counts); counts may be None only without want_counts")
    nbytes = lib().mv3d_anchor_occupancy_workspace_bytes(B, Hm, Wm)
    if nbytes == 0:
        check(_lib.ERR_INVALID_ARG, "mv3d_anchor_occupancy_workspace_bytes")
    ws = _workspace(nbytes, dev, "anchor_occupancy")
    rc = lib().mv3d_anchor_occupancy(_ptr(bev), B, Hm, Wm, Cc, int(H), int(W), int(feat_stride), int(min_cells), _ptr(mask),
                                     _ptr(counts), _ptr(ws), ws.numel(), _stream())
    check(rc, "mv3d_anchor_occupancy")
    return (mask, counts) if want_counts else mask


def proposal_3d(prob, pred, im_info, calib, params, out=None, anchor_mask=None):
    """prob (B,H,W,8), pred (B,H,W,24), im_info (B,3), calib (B,4,12) device f32 tensors.
    Returns (blob_bv (B,cap,5), blob_img (B,cap,5), blob_3d (B,cap,7), num_out (B) i32,
    status (B) i32); rows >= num_out[b] are zero.  Asynchronous.  anchor_mask (B, 4 H W): anchors whose mask is 0 are no
    candidates (mv3d_proposal_3d_masked)."""
    B, H, W, _ = prob.shape
    dev = prob.device
    cap = lib().mv3d_proposal_3d_capacity(H, W, C.byref(params))
    if cap < 0:
        check(_lib.ERR_INVALID_ARG, "mv3d_proposal_3d_capacity")
    nbytes = lib().mv3d_proposal_3d_workspace_bytes(B, H, W, C.byref(params))
    ws = _workspace(nbytes, dev, "proposal")
    if out is None:
        out = proposal_3d_outputs(B, cap, dev)[1]
    bv, img, b3, num, status = out
    if anchor_mask is None:
        rc = lib().mv3d_proposal_3d(_ptr(prob), _ptr(pred), B, H, W, _ptr(im_info), _ptr(calib), C.byref(params),
                                    _ptr(bv), _ptr(img), _ptr(b3), _ptr(num), _ptr(status), _ptr(ws), ws.numel(),
                                    _stream())
        check(rc, "mv3d_proposal_3d")
        return out
    mask = anchor_mask_tensor(anchor_mask, B, 4 * H * W, dev)
    rc = lib().mv3d_proposal_3d_masked(_ptr(prob), _ptr(pred), B, H, W, _ptr(im_info), _ptr(calib), C.byref(params), _ptr(mask),
                                       _ptr(bv), _ptr(img), _ptr(b3), _ptr(num), _ptr(status), _ptr(ws), ws.numel(), _stream())
    check(rc, "mv3d_proposal_3d_masked")
    return out


# ------------------------------------------------------------------ NMS
def nms_device(dets, thresh, max_keep=0):
    """dets (n,5) device f32 in processing order -> (keep (n) i32, num_keep (1) i32, status (1) i32)."""
    n = dets.shape[0]
    dev = dets.device
    keep = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    cnt = torch.zeros((2,), dtype=torch.int32, device=dev)
    ws = _workspace(lib().mv3d_nms_workspace_bytes(n), dev, "nms")
    rc = lib().mv3d_nms_device(_ptr(dets), n, float(thresh), int(max_keep), _ptr(keep), _ptr(cnt[0:1]),
                               _ptr(cnt[1:2]), _ptr(ws), ws.numel(), _stream())
    check(rc, "mv3d_nms_device")
    return keep, cnt[0:1], cnt[1:2]


def nms_host(dets, thresh, device_id=0):
    """numpy (n,5) f32, unsorted -> list of kept indices (cpu_nms semantics, computed on the GPU)."""
    d = np.ascontiguousarray(dets, dtype=np.float32)
    n = d.shape[0]
    keep = np.zeros(max(n, 1), np.int32)
    num = C.c_int32(0)
    rc = lib().mv3d_nms_host(keep.ctypes.data_as(C.c_void_p), C.byref(num), d.ctypes.data_as(C.c_void_p), n,
                             float(thresh), int(device_id))
    check(rc, "mv3d_nms_host")
    return [int(i) for i in keep[:num.value]]


def nms_gpu_rule_host(sorted_dets, thresh, device_id=0):
    """_nms of lib/nms/gpu_nms.hpp: host pointers, pre-sorted boxes, IoU > thresh in f32."""
    d = np.ascontiguousarray(sorted_dets, dtype=np.float32)
    n = d.shape[0]
    keep = np.zeros(max(n, 1), np.int32)
    num = C.c_int(0)
    lib()._nms(keep.ctypes.data_as(C.c_void_p), C.byref(num), d.ctypes.data_as(C.c_void_p), n, d.shape[1],
               C.c_float(thresh), int(device_id))
    return keep[:num.value]


# ------------------------------------------------------------------ RoiPool
def roi_pool_forward(data, rois, pooled_height, pooled_width, spatial_scale, want_argmax=True):
    B, H, W, Cc = data.shape
    R = rois.shape[0]
    top = torch.empty((R, pooled_height, pooled_width, Cc), dtype=torch.float32, device=data.device)
    argmax = torch.empty((R, pooled_height, pooled_width, Cc), dtype=torch.int32, device=data.device) if want_argmax else None
    rc = lib().mv3d_roi_pool_forward(_ptr(data), C.c_float(spatial_scale), B, R, H, W, Cc, pooled_height,
                                     pooled_width, _ptr(rois), _ptr(top), _ptr(argmax), _stream())
    check(rc, "mv3d_roi_pool_forward")
    return top, argmax


def roi_pool_backward(top_diff, rois, argmax, data_shape, pooled_height, pooled_width, spatial_scale):
    B, H, W, Cc = data_shape
    R = rois.shape[0]
    out = torch.empty((B, H, W, Cc), dtype=torch.float32, device=top_diff.device)
    rc = lib().mv3d_roi_pool_backward(_ptr(top_diff), C.c_float(spatial_scale), B, R, H, W, Cc, pooled_height,
                                      pooled_width, _ptr(rois), _ptr(out), _ptr(argmax), _stream())
    check(rc, "mv3d_roi_pool_backward")
    return out


# ------------------------------------------------------------------ anchor_target_layer
def anchor_target_stage1(H, W, im_info, gt_bv, gt_3d, params, labels=None, targets=None, anchor_mask=None):
    """anchor_mask (N): anchors whose mask is 0 are treated as outside the image (the batched masked entry, batch = 1)"""
    dev = gt_bv.device
    N = H * W * 4
    G = gt_bv.shape[0]
    if labels is None:
        labels = torch.empty((N,), dtype=torch.float32, device=dev)
        targets = torch.empty((N, 6), dtype=torch.float32, device=dev)
    # counts (8 x i32) and the per-foreground flags in ONE buffer: the host reads both with one copy
    cf = torch.empty((32 + N,), dtype=torch.uint8, device=dev)
    counts = cf[:32].view(torch.int32)
    fg_hi = cf[32:]
    ws = _workspace(lib().mv3d_anchor_target_workspace_bytes(H, W, G), dev, "anchor_target")
    if anchor_mask is None:
        rc = lib().mv3d_anchor_target_stage1(H, W, _ptr(im_info), _ptr(gt_bv), _ptr(gt_3d), G, C.byref(params),
                                             _ptr(labels), _ptr(targets), _ptr(counts), _ptr(fg_hi), _ptr(ws),
                                             ws.numel(), _stream())
        check(rc, "mv3d_anchor_target_stage1")
        return labels, targets, counts, fg_hi, ws, cf
    mask = anchor_mask_tensor(anchor_mask, 1, N, dev)
    P1 = C.c_void_p * 1
    one = lambda t: P1(0 if t is None else t.data_ptr())
    rc = lib().mv3d_anchor_target_stage1_batch_masked(1, H, W, _ptr(im_info), one(gt_bv), one(gt_3d), (C.c_int * 1)(G), C.byref(params),
                                                      one(mask), _ptr(labels), _ptr(targets), one(counts), one(fg_hi), one(ws),
                                                      ws.numel(), _stream())
    check(rc, "mv3d_anchor_target_stage1_batch_masked")
    return labels, targets, counts, fg_hi, ws, cf


def anchor_target_stage2(H, W, params, dis_fg, dis_bg1, dis_bg2, labels, ws, anchors_cap, out=None):
    dev = labels.device
    lists = [np.zeros(0, np.int32) if a is None else np.ascontiguousarray(a, np.int32) for a in (dis_fg, dis_bg1, dis_bg2)]
    t_fg = t_b1 = t_b2 = None
    if sum(len(a) for a in lists):
        v = upload_packed(lists, dev)                          # the three index lists in one upload
        t_fg, t_b1, t_b2 = (x if x.numel() else None for x in v)
    if out is None:
        anchors = torch.empty((anchors_cap, 5), dtype=torch.float32, device=dev)
        anchors_3d = torch.empty((anchors_cap, 7), dtype=torch.float32, device=dev)
        n_anchors = torch.empty((1,), dtype=torch.int32, device=dev)
    else:
        anchors, anchors_3d, n_anchors = out
    rc = lib().mv3d_anchor_target_stage2(H, W, C.byref(params), _ptr(t_fg), 0 if t_fg is None else t_fg.numel(),
                                         _ptr(t_b1), 0 if t_b1 is None else t_b1.numel(),
                                         _ptr(t_b2), 0 if t_b2 is None else t_b2.numel(),
                                         _ptr(labels), _ptr(anchors), _ptr(anchors_3d), _ptr(n_anchors),
                                         anchors_cap, _ptr(ws), ws.numel(), _stream())
    check(rc, "mv3d_anchor_target_stage2")
    return anchors, anchors_3d, n_anchors


# ------------------------------------------------------------------ proposal_target_layer_3d
def proposal_target_stage1(rois_bv, rois_3d, gt_bv, gt_3d, params):
    dev = gt_bv.device
    R, G = rois_bv.shape[0], gt_bv.shape[0]
    counts = torch.empty((4,), dtype=torch.int32, device=dev)
    ws = _workspace(lib().mv3d_proposal_target_workspace_bytes(R, G), dev, "proposal_target")
    rc = lib().mv3d_proposal_target_stage1(_ptr(rois_bv), _ptr(rois_3d), R, _ptr(gt_bv), _ptr(gt_3d), G, C.byref(params),
                                           _ptr(counts), _ptr(ws), ws.numel(), _stream())
    check(rc, "mv3d_proposal_target_stage1")
    return counts, ws


def proposal_target_spec(S, nc):
    return [((S, 5), torch.float32), ((S, 5), torch.float32), ((S, 1), torch.int32), ((S, 24 * nc), torch.float32),
            ((S, 7), torch.float32)]


def proposal_target_stage2(rois_bv, rois_3d, gt_bv, gt_3d, gt_cnr, calib, params, fg_pick, bg_pick, ws, out=None):
    dev = gt_bv.device
    R, G = rois_bv.shape[0], gt_bv.shape[0]
    t_fg = t_bg = None
    if len(fg_pick) + len(bg_pick):
        v = upload_packed([np.ascontiguousarray(fg_pick, np.int32), np.ascontiguousarray(bg_pick, np.int32)], dev)
        t_fg, t_bg = (x if x.numel() else None for x in v)
    S = len(fg_pick) + len(bg_pick)
    nc = params.num_classes
    if out is None:
        out = tuple(torch.empty(sh, dtype=dt, device=dev) for sh, dt in proposal_target_spec(S, nc))
    rc = lib().mv3d_proposal_target_stage2(_ptr(rois_bv), _ptr(rois_3d), R, _ptr(gt_bv), _ptr(gt_3d), _ptr(gt_cnr), G,
                                           _ptr(calib), C.byref(params), _ptr(t_fg), len(fg_pick), _ptr(t_bg), len(bg_pick),
                                           _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), _ptr(out[4]),
                                           _ptr(ws), ws.numel(), _stream())
    check(rc, "mv3d_proposal_target_stage2")
    return out


# ------------------------------------------------------------------ SURVEY §8(f) next rows
def point_cloud_2_top(points, ranges=None):
    """points (P,4) f32 device tensor -> top f32 device tensor: (601,601,9) for the call MV3D makes (ranges=None), or the map of
    ranges = (res, zres, side_lo, side_hi, fwd_lo, fwd_hi, height_lo, height_hi) (lib/utils/read_lidar.py:10-16); that form reads
    one status word back and raises IndexError where numpy's fancy assignment would (a cell outside the map)."""
    pts = points.contiguous()
    if ranges is None:
        top = torch.empty((601, 601, 9), dtype=torch.float32, device=pts.device)
        check(lib().mv3d_point_cloud_2_top(_ptr(pts), pts.shape[0], _ptr(top), _stream()), "mv3d_point_cloud_2_top")
        return top
    r = [float(v) for v in ranges]
    dims = (C.c_int * 3)()
    check(lib().mv3d_point_cloud_2_top_shape(*r, dims), "mv3d_point_cloud_2_top_shape")
    top = torch.empty(tuple(dims), dtype=torch.float32, device=pts.device)
    status = torch.empty(1, dtype=torch.int32, device=pts.device)
    check(lib().mv3d_point_cloud_2_top_ranges(_ptr(pts), pts.shape[0], *r, _ptr(top), _ptr(status), _stream()), "mv3d_point_cloud_2_top_ranges")
    if int(status.item()):
        raise IndexError("point_cloud_2_top: a point's cell lies outside the map (numpy raises IndexError there)")
    return top


def box_detect_tail(rois_3d, bbox_pred, num_classes):
    R = rois_3d.shape[0]
    dev = rois_3d.device
    cnr = torch.empty((R, 24), dtype=torch.float32, device=dev)
    pr = torch.empty((R, 24 * num_classes), dtype=torch.float32, device=dev)
    bv = torch.empty((R, 4 * num_classes), dtype=torch.float32, device=dev)
    bvr = torch.empty((R, 4 * num_classes), dtype=torch.float32, device=dev)
    check(lib().mv3d_box_detect_tail(_ptr(rois_3d), _ptr(bbox_pred), R, num_classes, _ptr(cnr), _ptr(pr), _ptr(bv), _ptr(bvr),
                                     _stream()), "mv3d_box_detect_tail")
    return cnr, pr, bv, bvr


def detect_post_outputs(B, K, cap, dev, with_cnr_r=True):
    """Caller-owned outputs of detect_post: (det_bv (B,K,cap,5), det_cnr (B,K,cap,25), det_cnr_r (B,K,cap,25) | None, det_row (B,K,cap)
    i32, det_count (B,K) i32, status (B) i32).  det_count and status are views of ONE buffer (one small read-back)."""
    tail = torch.zeros((B * K + B,), dtype=torch.int32, device=dev)
    return (torch.empty((B, K, cap, 5), dtype=torch.float32, device=dev), torch.empty((B, K, cap, 25), dtype=torch.float32, device=dev),
            torch.empty((B, K, cap, 25), dtype=torch.float32, device=dev) if with_cnr_r else None,
            torch.empty((B, K, cap), dtype=torch.int32, device=dev), tail[:B * K].view(B, K), tail[B * K:])


def _detect_post_args(name, cls_prob, pred_bv, corners, pred_cnr_r, num_rois, rows_per_frame, num_classes, max_per_image, strict_gt,
                      score_thresh, nms_thresh):
    """what detect_post and detect_post_oriented (`name`, the prefix of the messages) do with their arguments: the row and shape
    checks, the widening to contiguous f32 and the parameter block -> (B, params, (cls_prob, pred_bv, corners, pred_cnr_r))"""
    K, cap = int(num_classes), int(rows_per_frame)
    if cap <= 0 or cls_prob.shape[0] % cap:
        check(_lib.ERR_INVALID_ARG, name + ": rows are not a multiple of rows_per_frame")
    B = cls_prob.shape[0] // cap
    cls_prob, pred_bv, corners = cls_prob.float().contiguous(), pred_bv.float().contiguous(), corners.float().contiguous()
    if pred_cnr_r is not None:
        pred_cnr_r = pred_cnr_r.float().contiguous()
    if (cls_prob.shape[1], pred_bv.shape, corners.shape) != (K, (B * cap, 4 * K), (B * cap, 24)) or \
            (pred_cnr_r is not None and pred_cnr_r.shape != (B * cap, 24 * K)) or \
            (num_rois is not None and (num_rois.dtype != torch.int32 or num_rois.numel() != B)):
        check(_lib.ERR_INVALID_ARG, name + ": input shapes")
    params = _lib.DetectPostParams(K, cap, int(max_per_image), 1 if strict_gt else 0, float(score_thresh), 0, float(nms_thresh))
    return B, params, (cls_prob, pred_bv, corners, pred_cnr_r)


def _detect_post_launch(fn, name, B, params, inputs, num_rois, extra, out, workspace):
    """the launch behind both: `out` (default: fresh detect_post_outputs) with its status zeroed (the kernels OR into it), then
    fn(*inputs, num_rois, B, params, *extra, *outputs, workspace, its bytes, stream)"""
    if out is None:
        out = detect_post_outputs(B, params.num_classes, params.rows_per_frame, inputs[0].device, inputs[3] is not None)
    det_bv, det_cnr, det_cnr_r, det_row, det_count, status = out
    status.zero_()
    rc = fn(*[_ptr(t) for t in inputs], _ptr(num_rois), B, C.byref(params), *extra, _ptr(det_bv), _ptr(det_cnr),
            _ptr(det_cnr_r if inputs[3] is not None else None), _ptr(det_row), _ptr(det_count), _ptr(status),
            _ptr(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size(), _stream())
    check(rc, name)
    return out


def detect_post(cls_prob, pred_bv, corners, pred_cnr_r, num_rois, rows_per_frame, num_classes, max_per_image, nms_thresh,
                score_thresh=0.05, use_gpu_nms=None, out=None):
    """The per-frame tail of test_net (score cut, NMS, cap over all classes; lib/fast_rcnn/test_mv.py:420-444, 491-501) for a batch
    of B = rows / rows_per_frame frames on the device: mv3d_detect_post.  cls_prob (B*cap, K) (16-bit is widened, exactly),
    pred_bv (B*cap, 4K), corners (B*cap, 24), pred_cnr_r (B*cap, 24K) or None, num_rois (B) i32 or None.  `use_gpu_nms`
    (default: cfg.USE_GPU_NMS) selects the NMS rule the way nms_wrapper.py:13-21 does.  Returns `out` =
    detect_post_outputs(...); status is zeroed here (the kernels OR into it).  Asynchronous: kernel launches only."""
    if use_gpu_nms is None:
        from .fast_rcnn.config import cfg
        use_gpu_nms = bool(cfg.USE_GPU_NMS)
    B, params, inputs = _detect_post_args("detect_post", cls_prob, pred_bv, corners, pred_cnr_r, num_rois, rows_per_frame, num_classes,
                                          max_per_image, use_gpu_nms, score_thresh, nms_thresh)
    return _detect_post_launch(lib().mv3d_detect_post, "mv3d_detect_post", B, params, inputs, num_rois, (), out, None)


_FOOTPRINTS = {"proposal": 0, "regressed": 1}


def detect_post_oriented_workspace(B, K, cap, dev):
    """A caller-owned workspace for detect_post_oriented (uint8; the kernels write before they read, so it is not initialised)."""
    params = _lib.DetectPostParams(int(K), int(cap), 0, 0, 0.0, 0, 0.0)
    return torch.empty((max(lib().mv3d_detect_post_oriented_workspace_bytes(int(B), C.byref(params)), 256),), dtype=torch.uint8, device=dev)


def detect_post_oriented(cls_prob, pred_bv, corners, pred_cnr_r, num_rois, rows_per_frame, num_classes, max_per_image, nms_thresh,
                         score_thresh=0.05, strict_gt=False, footprint="regressed", out=None, workspace=None):
    """detect_post with ORIENTED NMS (mv3d_detect_post_oriented): the same score cut, order, outputs and cap; a candidate is suppressed
    by an earlier kept one where the IoU of their BEV footprints, computed as the KITTI evaluator computes it, is >= nms_thresh
    (strict_gt: > nms_thresh), in f64.  footprint: 'regressed' = pred_cnr_r[r, 24j:24j+24] (required then), 'proposal' = corners[r].
    Returns the six-tuple of detect_post (`out` = detect_post_outputs(...)), for detect_post_lists as it is; status value 2
    (MV3D_DETECT_STATUS_NONFINITE) marks frames with a candidate whose footprint holds a non-finite value (kept, suppresses
    nothing).  `workspace`: detect_post_oriented_workspace(...), or the cached one of this stream.  Asynchronous: kernel launches only."""
    if footprint not in _FOOTPRINTS:
        raise ValueError("detect_post_oriented: footprint is 'regressed' or 'proposal', not %r" % (footprint,))
    B, params, inputs = _detect_post_args("detect_post_oriented", cls_prob, pred_bv, corners, pred_cnr_r, num_rois, rows_per_frame,
                                          num_classes, max_per_image, strict_gt, score_thresh, nms_thresh)
    need = lib().mv3d_detect_post_oriented_workspace_bytes(B, C.byref(params))
    if need == 0:
        check(_lib.ERR_INVALID_ARG, "detect_post_oriented: batch, num_classes or rows_per_frame out of range")
    if workspace is None:
        workspace = _workspace(need, inputs[0].device, "detect_post_oriented")
    return _detect_post_launch(lib().mv3d_detect_post_oriented, "mv3d_detect_post_oriented", B, params, inputs, num_rois,
                               (_FOOTPRINTS[footprint],), out, workspace)


def nms_oriented(corners, scores, thresh, strict_gt=False):
    """Greedy NMS of n <= 2048 oriented boxes by the IoU of their BEV footprints: corners (n, 24) [x0..7, y0..7, z0..7], scores (n)
    -> the kept indices (i64 device tensor) in keep order (descending score, equal scores by larger index).  One class of one frame
    of detect_post_oriented without score cut or cap (a NaN or -inf score is no candidate, as there).  Synchronises (one read of
    the count)."""
    corners = corners.float().reshape(-1, 24).contiguous()
    n = corners.shape[0]
    if n > 2048:
        raise ValueError("nms_oriented: %d boxes; at most 2048 (the rows of one frame of detect_post_oriented)" % n)
    if n == 0:
        return torch.empty((0,), dtype=torch.int64, device=corners.device)
    scores = scores.float().reshape(n)
    cls_prob = torch.stack([torch.zeros_like(scores), scores], 1)
    pred_bv = torch.zeros((n, 8), dtype=torch.float32, device=corners.device)
    out = detect_post_oriented(cls_prob, pred_bv, corners, None, None, n, 2, 0, thresh, score_thresh=float("-inf"), strict_gt=strict_gt,
                               footprint="proposal")
    return out[3][0, 1, :int(out[4][0, 1].item())].to(torch.int64)


def detect_post_lists(out, with_cnr_r=False):
    """The ONE read-back behind detect_post: synchronises, reads det_count | status, raises ZeroDivisionError where the reference's NMS
    does, copies the rows in front of the counts and returns per frame (dets, dets_cnr[, dets_cnr_r]) as class_detections +
    limit_detections build them: index 0 an empty list, class j (N,5) / (N,25) f32."""
    det_bv, det_cnr, det_cnr_r, _, det_count, status = out
    B, K, cap = det_count.shape[0], det_count.shape[1], det_bv.shape[2]
    cnt = det_count.cpu().numpy()
    st = status.cpu().numpy()
    if int(st.max()) & 1:
        raise ZeroDivisionError("float division")
    top = max(int(cnt.max()), 1)                              # rows behind the largest count never travel
    srcs = [det_bv, det_cnr] + ([det_cnr_r] if with_cnr_r else [])
    host = [t[:, :, :top].cpu().numpy() for t in srcs]
    return [tuple([[]] + [h[f, j, :cnt[f, j]].copy() for j in range(1, K)] for h in host) for f in range(B)]


def _roi_views(views, pooled_height, pooled_width, outs, top_dtype=torch.float32, want_argmax=True):
    """RoiView array of forward views [(data, rois, scale), ...] and their outputs [(top, argmax or None), ...]: `outs`, or fresh
    (R,PH,PW,C) tensors (top in top_dtype, argmax i32 when want_argmax)"""
    arr = (RoiView * len(views))()
    res = []
    for k, (data, rois, scale) in enumerate(views):
        B, H, W, Cc = data.shape
        R = rois.shape[0]
        if outs is not None:
            top, am = outs[k]
        else:
            top = torch.empty((R, pooled_height, pooled_width, Cc), dtype=top_dtype, device=data.device)
            am = torch.empty((R, pooled_height, pooled_width, Cc), dtype=torch.int32, device=data.device) if want_argmax else None
        arr[k] = RoiView(data.data_ptr(), rois.data_ptr(), top.data_ptr(), am.data_ptr() if am is not None else None, float(scale), B, R, H, W, Cc)
        res.append((top, am))
    return arr, res


def _roi_grad_views(views, outs):
    """RoiGradView array of backward views [(top_diff, rois, argmax, data_shape, scale), ...] and their bottom_diff outputs (`outs`
    or fresh (B,H,W,C) f32)"""
    arr = (RoiGradView * len(views))()
    res = []
    for k, (top_diff, rois, argmax, shape, scale) in enumerate(views):
        B, H, W, Cc = shape
        out = outs[k] if outs is not None else torch.empty((B, H, W, Cc), dtype=torch.float32, device=top_diff.device)
        arr[k] = RoiGradView(out.data_ptr(), rois.data_ptr(), top_diff.data_ptr(), argmax.data_ptr(), float(scale), B,
                             rois.shape[0], H, W, Cc)
        res.append(out)
    return arr, res


def roi_pool_forward_views(views, pooled_height, pooled_width, outs=None, cold_maps=False, want_argmax=True, top_dtype=None):
    """views: list of (data (B,H,W,C), rois (R,5), spatial_scale); one launch for all of them.
    Returns [(top, argmax), ...]; pass `outs` (same structure) to reuse output tensors.  cold_maps: the maps are not
    cache-resident (mv3d_roi_pool_forward_views_cold: same results, prefetch workgroups in front of the launch).
    want_argmax=False (inference): argmax_data = NULL, the entries are (top, None).  top_dtype = torch.float16 / bfloat16 (inference,
    want_argmax=False): `top` in that type (mv3d_roi_pool_forward_views_half: the values a cast of the f32 top gives)."""
    half = top_dtype in (torch.float16, torch.bfloat16)
    if half and want_argmax:
        raise ValueError("16-bit tops are an inference output: want_argmax=False")
    arr, res = _roi_views(views, pooled_height, pooled_width, outs, top_dtype if half else torch.float32, want_argmax)
    if half:
        check(lib().mv3d_roi_pool_forward_views_half(len(views), arr, pooled_height, pooled_width, 1 if top_dtype == torch.float16 else 2,
                                                     1 if cold_maps else 0, _stream()), "mv3d_roi_pool_forward_views_half")
        return res
    fn = lib().mv3d_roi_pool_forward_views_cold if cold_maps else lib().mv3d_roi_pool_forward_views
    check(fn(len(views), arr, pooled_height, pooled_width, _stream()), "mv3d_roi_pool_forward_views")
    return res


def roi_pool_backward_views(views, pooled_height, pooled_width, outs=None, workspace=None):
    """views: list of (top_diff (R,PH,PW,C), rois (R,5), argmax (R,PH,PW,C) i32, data_shape (B,H,W,C), spatial_scale);
    RoiPoolGrad of all of them behind one call.  Returns [bottom_diff, ...]; pass `outs` to reuse output tensors.
    workspace = None: the cached buffer of mv3d_roi_pool_backward_workspace_bytes bytes (index + gather for the shapes that take it);
    False: none (the sliced kernel for those shapes); a uint8 tensor: handed to the entry as is (same results every way)."""
    arr, res = _roi_grad_views(views, outs)
    if workspace is None:
        nbytes = lib().mv3d_roi_pool_backward_workspace_bytes(len(views), arr, pooled_height, pooled_width)
        workspace = _workspace(nbytes, views[0][0].device, "roi_bwd")
    wp, wn = (None, 0) if workspace is False else (_ptr(workspace), workspace.numel())
    check(lib().mv3d_roi_pool_backward_views(len(views), arr, pooled_height, pooled_width, wp, wn, _stream()),
          "mv3d_roi_pool_backward_views")
    return res


# ---- the RoiPool pair of a training step: private compact argmax plane, one launch forward, one launch backward
def roi_pool_forward_views_pair(views, pooled_height, pooled_width, outs=None, cold_maps=False):
    """views as roi_pool_forward_views; one launch.  Returns [(top, argmax_private), ...]: the second tensor is the pair's PRIVATE
    argmax plane (one-byte codes, 16-bit for bins of > 255 pixels, in an int32-shaped buffer for the shapes the pair's kernels take) -- hand it to
    roi_pool_backward_views_pair only; roi_pool_argmax_decode gives the reference's int32 plane."""
    arr, res = _roi_views(views, pooled_height, pooled_width, outs)
    check(lib().mv3d_roi_pool_forward_views_pair(len(views), arr, pooled_height, pooled_width, 1 if cold_maps else 0, _stream()),
          "mv3d_roi_pool_forward_views_pair")
    return res


def roi_pool_argmax_decode(views, res, pooled_height, pooled_width):
    """The reference's int32 argmax planes of a roi_pool_forward_views_pair call: views / res as given to / returned by it.  Tests and
    verification only."""
    arr, _ = _roi_views(views, pooled_height, pooled_width, res)
    outs = [torch.empty(tuple(top.shape), dtype=torch.int32, device=top.device) for top, _ in res]
    ptrs = (C.c_void_p * len(views))(*[o.data_ptr() for o in outs])
    check(lib().mv3d_roi_pool_argmax_decode(len(views), arr, pooled_height, pooled_width, ptrs, _stream()), "mv3d_roi_pool_argmax_decode")
    return outs


def roi_pool_backward_views_pair(views, pooled_height, pooled_width, outs=None, workspace=None):
    """views as roi_pool_backward_views, of a roi_pool_forward_views_pair call (the argmax tensors it returned): RoiPoolGrad of all of
    them behind one call -- ONE launch of LDS map tiles (csrc/roi_grad_tiles.hip) that needs no workspace.  workspace = None (or
    False, which callers written against the earlier signature pass): none; a uint8 tensor of mv3d_roi_pool_pair_workspace_bytes
    bytes: handed to the entry as is, which passes it on to the plain indexed RoiPoolGrad for shapes outside the pair's kernels (same
    results either way).  Returns [bottom_diff, ...]."""
    arr, res = _roi_grad_views(views, outs)
    wp, wn = (None, 0) if workspace is None or workspace is False else (_ptr(workspace), workspace.numel())
    check(lib().mv3d_roi_pool_backward_views_pair(len(views), arr, pooled_height, pooled_width, wp, wn, _stream()),
          "mv3d_roi_pool_backward_views_pair")
    return res


ROI_PAIR_MAX_PIXELS = 0xfffe         # roi_pair_shapes (csrc/roi_pool.hip): the pair's own kernels take maps of at most this many pixels


def roi_pool_pair_workspace(views, pooled_height, pooled_width):
    """The workspace roi_pool_backward_views_pair should be given for these backward views: None while every map fits the pair's own
    kernels, which use none (mv3d_roi_pool_pair_workspace_bytes cannot tell: it answers with the indexed RoiPoolGrad's size for every
    shape); for a larger map (a 4x upsampled 608 x 608 bird's-eye view) the reused buffer of roi_pool_backward_views, with which the
    hand-over takes the index + gather backward.  Should the C side's condition ever differ from this one, only the choice between
    two backward kernels with the same results differs: without a workspace the hand-over runs the unindexed RoiPoolGrad."""
    if all(shape[1] * shape[2] <= ROI_PAIR_MAX_PIXELS for _, _, _, shape, _ in views):
        return None
    arr = (RoiGradView * len(views))()
    for k, (_, rois, _, (B, H, W, Cc), scale) in enumerate(views):       # (the size query reads the shapes only)
        arr[k] = RoiGradView(None, None, None, None, float(scale), B, rois.shape[0], H, W, Cc)
    nbytes = lib().mv3d_roi_pool_pair_workspace_bytes(len(views), arr, pooled_height, pooled_width)
    return _workspace(nbytes, views[0][0].device, "roi_bwd")


def rois_3d_to_fv(rois_3d, out=None):
    """rois_3d (R,7) device f32 [b,x,y,z,l,w,h] -> rois_fv (R,5) [b,x1,y1,x2,y2] on the 64 x 512 front-view map."""
    r3 = rois_3d.contiguous()
    R = r3.shape[0]
    if out is None:
        out = torch.empty((R, 5), dtype=torch.float32, device=r3.device)
    check(lib().mv3d_rois_3d_to_fv(_ptr(r3), R, _ptr(out), _stream()), "mv3d_rois_3d_to_fv")
    return out


FV_SHAPE = (64, 512, 3)              # rows x columns x [height, distance, intensity] (csrc/front_view.h: FV_H, FV_W)
FV_MAX_FRAMES = 1024                 # MV3D_FV_MAX_FRAMES


def point_cloud_2_front_workspace_bytes(num_frames=1):
    return int(lib().mv3d_point_cloud_2_front_workspace(int(num_frames)))


def _scan_args(fn, points, offsets, frame, out, workspace=None, workspace_bytes=None, frame_rows=None, more=None):
    """The argument checks and uploads that the rasterisers of B clouds back to back share (point_cloud_2_front,
    point_cloud_2_top_batch; `fn` is the name the messages carry): points (P,4) f32, a device tensor or a numpy array; offsets None
    (one frame) or (B + 1) int32, whose VALUES are checked only when they come from the host (ascending within [0, P], at most
    `frame_rows` rows a frame where that is given); every tensor on one HIP device; out (optional) a contiguous f32 tensor of the
    result's shape; workspace (optional) contiguous uint8 of at least workspace_bytes(B) bytes.  `frame` is the shape of one frame
    of the result, or a function that gives it, called once the points have passed (the caller's own checks keep their place among
    these); None = the call has no such `out` (scan_crop_to_image, whose result is a batch of clouds).  more (optional) = the caller's
    checks of its further arguments, called as more(B, P, device) once all of these have passed.  TypeError for a wrong dtype,
    ValueError for a wrong shape, value or device, all before anything is uploaded or allocated.
    -> (points on the device, offsets on the device or None, B, P, out, device)"""
    if isinstance(points, torch.Tensor):
        if points.dtype != torch.float32:
            raise TypeError("{}: points must be float32, got {}".format(fn, points.dtype))
        if not points.is_cuda:
            raise ValueError("{}: a points tensor must live on the device (pass a numpy array to have it uploaded)".format(fn))
    else:
        points = np.asarray(points)
        if points.dtype != np.float32:
            raise TypeError("{}: points must be float32, got {}".format(fn, points.dtype))
    if points.ndim != 2 or points.shape[1] != 4:
        raise ValueError("{}: points must be (P, 4) [x, y, z, reflectance], got {}".format(fn, tuple(points.shape)))
    P = int(points.shape[0])
    if callable(frame):
        frame = frame()
    shape = frame
    if offsets is not None:
        if isinstance(offsets, torch.Tensor):
            if offsets.dtype != torch.int32:
                raise TypeError("{}: an offsets tensor must be int32, got {}".format(fn, offsets.dtype))
        else:
            offsets = np.asarray(offsets)
            if not np.issubdtype(offsets.dtype, np.integer):
                raise TypeError("{}: offsets must be integers, got {}".format(fn, offsets.dtype))
            if offsets.ndim == 1 and offsets.size and (np.any(np.diff(offsets) < 0) or offsets[0] < 0 or offsets[-1] > P):
                raise ValueError("{}: offsets must ascend within [0, {}], got {}".format(fn, P, offsets.tolist()))
            if frame_rows is not None and offsets.ndim == 1 and offsets.size > 1 and np.diff(offsets).max() > frame_rows:
                raise ValueError("{}: a frame holds at most {} rows".format(fn, frame_rows))
        if offsets.ndim != 1 or not 2 <= offsets.shape[0] <= FV_MAX_FRAMES + 1:
            raise ValueError("{}: offsets must be (B + 1,) with 1 <= B <= {}, got {}".format(fn, FV_MAX_FRAMES, tuple(offsets.shape)))
        shape = None if frame is None else (int(offsets.shape[0]) - 1,) + frame
    elif frame_rows is not None and P > frame_rows:
        raise ValueError("{}: a frame holds at most {} rows".format(fn, frame_rows))
    B = 1 if offsets is None else int(offsets.shape[0]) - 1
    for name, t, dtype in (("out", out, torch.float32), ("workspace", workspace, torch.uint8)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dtype):
            raise TypeError("{}: {} must be a {} tensor".format(fn, name, dtype))
    # one device for every tensor handed in (a numpy cloud goes where they are; with none of them, to the current device)
    tensors = [(n, t) for n, t in (("points", points), ("offsets", offsets), ("out", out), ("workspace", workspace)) if isinstance(t, torch.Tensor)]
    for name, t in tensors:
        if not t.is_cuda or t.device != tensors[0][1].device:
            raise ValueError("{}: {} on {}: every tensor must live on one HIP device".format(fn, name, t.device))
        if name in ("out", "workspace") and not t.is_contiguous():
            raise ValueError("{}: {} must be contiguous".format(fn, name))
    dev = tensors[0][1].device if tensors else "cuda"
    if out is not None and tuple(out.shape) != shape:
        raise ValueError("{}: out must be {}, got {}".format(fn, shape, tuple(out.shape)))
    if workspace is not None and workspace.numel() < workspace_bytes(B):
        raise ValueError("{}: workspace of {} bytes, {} needed".format(fn, workspace.numel(), workspace_bytes(B)))
    if more is not None:
        more(B, P, dev)
    pts = points.contiguous() if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points)).to(dev)
    off = None                                                # (one frame: the entries take NULL offsets, nothing to upload)
    if offsets is not None:
        off = offsets.contiguous() if isinstance(offsets, torch.Tensor) else torch.from_numpy(offsets.astype(np.int32)).to(dev)
    if out is None and shape is not None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    return pts, off, B, P, out, dev


def point_cloud_2_front(points, offsets=None, out=None, workspace=None):
    """points (P,4) f32 [x,y,z,reflectance] (a device tensor, or a numpy array, which is uploaded) -> the (64,512,3) f32 front-view
    map [height, distance, intensity] on the device (csrc/front_view_raster.hip, DESIGN.md section 3.21: nearest point per pixel,
    among equal distances the last; empty pixels 0).  offsets = (B + 1) ascending int32 row offsets (host sequence / array, or a device
    tensor): `points` is B clouds back to back, frame b owns rows offsets[b]:offsets[b + 1], the result is (B,64,512,3).
    out = a contiguous f32 device tensor of the result's shape to write into (a slice of a captured step's `lidar_fv_data`),
    workspace = a uint8 device tensor of point_cloud_2_front_workspace_bytes(B) bytes (default: the reused per-stream buffer); with
    both given and device inputs the call allocates nothing and can be captured.  Every argument is checked before anything is
    launched: TypeError for a wrong dtype, ValueError for a wrong shape or device (the kernels take what they are handed as f32 /
    int32 words on the device).  The VALUES of offsets are checked (ascending, within [0, P]) only when they come from the host:
    reading a device tensor would synchronise.  Under malformed device offsets the call stays inside its buffers and silently skips
    the rows no frame owns (include/mv3d_hip.h)."""
    pts, off, B, P, out, dev = _scan_args("point_cloud_2_front", points, offsets, FV_SHAPE, out, workspace, point_cloud_2_front_workspace_bytes)
    if workspace is None:
        workspace = _workspace(point_cloud_2_front_workspace_bytes(B), dev, "fv_raster")
    check(lib().mv3d_point_cloud_2_front(_ptr(pts), _ptr(off), B, P, _ptr(out), _ptr(workspace), _stream()), "mv3d_point_cloud_2_front")
    return out


BEV_SHAPE = (601, 601, 9)            # the map of the call MV3D makes (tools/read_lidar.py:121-133): rows x columns x (8 slices + reflectance)
BEV_MAX_FRAME_POINTS = (1 << 27) - 1  # rows per frame (the winner key holds the row's index within its frame in 27 bits)


def point_cloud_2_top_batch(points, offsets=None, ranges=None, out=None):
    """point_cloud_2_top for B clouds behind three launches (csrc/bev_raster.hip), argument for argument
    ops.point_cloud_2_front: points (P,4) f32 [x,y,z,reflectance] (a device tensor, or a numpy array, which is uploaded) is B clouds
    back to back, offsets = (B + 1) ascending int32 row offsets (host sequence / array, or a device tensor), frame b owns rows
    offsets[b]:offsets[b + 1]; the result is (B,601,601,9) f32 on the device -- (601,601,9) without offsets, one frame -- and frame b
    of it equals point_cloud_2_top(that frame's rows) bit for bit.  ranges = (res, zres, side_lo, side_hi, fwd_lo, fwd_hi, height_lo,
    height_hi): the frames' shape is mv3d_point_cloud_2_top_shape's, and ONE status word for the batch is read back (a
    synchronisation) to raise IndexError where numpy's fancy assignment would.  out = a contiguous f32 device tensor of the result's
    shape to write into; it may be any slice of frames of a larger batch buffer (4-byte alignment is all it needs).  With device
    inputs, out= and no ranges the call allocates nothing and can be captured.
    Every argument is checked before anything is launched: TypeError for a wrong dtype, ValueError for a wrong shape or device.  The
    VALUES of offsets are checked (ascending, within [0, P], at most 2^27 - 1 rows a frame) only when they come from the host:
    reading a device tensor would synchronise.  Under malformed device offsets the call stays inside its buffers and silently skips
    the rows no frame owns (include/mv3d_hip.h)."""
    r = None

    def frame():
        nonlocal r
        if ranges is None:
            return BEV_SHAPE
        r = (C.c_double * 8)(*[float(v) for v in ranges])     # (anything but 8 numbers: ctypes / float raise TypeError or ValueError here)
        dims = (C.c_int * 3)()
        if lib().mv3d_point_cloud_2_top_shape(*r, dims) != _lib.OK:
            raise ValueError("point_cloud_2_top_batch: ranges {} are empty, inverted or beyond 32767 cells / 31 slices".format(tuple(r)))
        return tuple(dims)

    pts, off, B, P, out, dev = _scan_args("point_cloud_2_top_batch", points, offsets, frame, out, frame_rows=BEV_MAX_FRAME_POINTS)
    status = None if r is None else torch.empty(1, dtype=torch.int32, device=dev)
    check(lib().mv3d_point_cloud_2_top_batch(_ptr(pts), _ptr(off), B, P, r, _ptr(out), _ptr(status), _stream()), "mv3d_point_cloud_2_top_batch")
    if status is not None and int(status.item()):
        raise IndexError("point_cloud_2_top_batch: a point's cell lies outside the map (numpy raises IndexError there)")
    return out


BEV_PAPER_SHAPE = (601, 601, 10)     # the paper's encoding of the same call: rows x columns x (8 slices + top intensity + density)


def _ranges8(fn, ranges):
    """ranges -> the (8) C doubles the BEV entries take, None for None (anything but 8 numbers: ctypes / float raise TypeError or
    ValueError here)"""
    return None if ranges is None else (C.c_double * 8)(*[float(v) for v in ranges])


def point_cloud_2_top_paper_workspace_bytes(num_frames=1, ranges=None):
    """bytes of workspace ops.point_cloud_2_top_paper needs for num_frames frames of these ranges: 8 per cell and frame"""
    return int(lib().mv3d_point_cloud_2_top_paper_workspace(int(num_frames), _ranges8("point_cloud_2_top_paper", ranges)))


def bev_density_table():
    """the 64 f32 density values T[n] = min(1, log(n + 1) / log 64) as the library computes them (mv3d_bev_density_table, host only)"""
    out = (C.c_float * 64)()
    check(lib().mv3d_bev_density_table(out), "mv3d_bev_density_table")
    return np.frombuffer(out, np.float32).copy()


def point_cloud_2_top_paper(points, offsets=None, ranges=None, out=None, workspace=None):
    """The MV3D paper's BEV encoding (csrc/bev_paper.hip; parity unpinned, the definition is
    tests/bev_paper_restatement.py) of B clouds behind three launches, argument for argument ops.point_cloud_2_top_batch and with its
    kept rows, cells and slices: the result is (B,601,601,10) f32 on the device -- (601,601,10) without offsets -- or (.., H, W, M + 2)
    for ranges = (res, zres, side_lo, side_hi, fwd_lo, fwd_hi, height_lo, height_hi), M = ceil((height_hi - height_lo) / zres):
    channels < M the maximal z - height_lo of each height slice, channel M the reflectance of the cell's highest point (among equal
    heights the last row), channel M + 1 the density min(1, log(N + 1) / log 64) of the cell's N kept points; an empty cell is 0.
    With ranges ONE status word is read back (a synchronisation) to raise IndexError where point_cloud_2_top_batch does.
    out = a contiguous f32 device tensor of the result's shape (any run of frames of a larger buffer: 4-byte alignment is all it
    needs), workspace = a uint8 device tensor of point_cloud_2_top_paper_workspace_bytes(B, ranges) bytes, 16-byte aligned (default: the
    reused per-stream buffer); with both given, device inputs and no ranges the call allocates nothing and can be captured.
    Every argument is checked before anything is launched, as ops.point_cloud_2_top_batch checks it."""
    fn = "point_cloud_2_top_paper"
    r = None

    def frame():
        nonlocal r
        if ranges is None:
            return BEV_PAPER_SHAPE
        r = _ranges8(fn, ranges)
        dims = (C.c_int * 3)()
        if lib().mv3d_point_cloud_2_top_paper_shape(*r, dims) != _lib.OK:
            raise ValueError("{}: ranges {} are empty, inverted or beyond 32767 cells / 31 slices".format(fn, tuple(r)))
        return tuple(dims)

    need = lambda B: int(lib().mv3d_point_cloud_2_top_paper_workspace(B, r))
    pts, off, B, P, out, dev = _scan_args(fn, points, offsets, frame, out, workspace, need, frame_rows=BEV_MAX_FRAME_POINTS)
    if workspace is None:
        workspace = _workspace(need(B), dev, "bev_paper")
    elif workspace.data_ptr() % 16:
        raise ValueError("{}: workspace must be 16-byte aligned".format(fn))
    status = None if r is None else torch.empty(1, dtype=torch.int32, device=dev)
    check(lib().mv3d_point_cloud_2_top_paper_batch(_ptr(pts), _ptr(off), B, P, r, _ptr(out), _ptr(workspace), _ptr(status), _stream()),
          "mv3d_point_cloud_2_top_paper_batch")
    if status is not None and int(status.item()):
        raise IndexError("{}: a point's cell lies outside the map (numpy raises IndexError there)".format(fn))
    return out


def bev_encoding():
    """cfg.LIDAR_BV_ENCODING checked: 'reference' or 'paper'; 'paper' without cfg.LIDAR_BV_FROM_SCAN raises ValueError (stored
    lidar_bv/*.npy maps are reference-encoded), as does any other value.  prepare_roidb and the detection loops call it before they
    load a frame."""
    from .fast_rcnn.config import cfg
    enc = cfg.LIDAR_BV_ENCODING
    if enc not in ("reference", "paper"):
        raise ValueError("cfg.LIDAR_BV_ENCODING must be 'reference' or 'paper', got %r" % (enc,))
    if enc == "paper" and not cfg.LIDAR_BV_FROM_SCAN:
        raise ValueError("cfg.LIDAR_BV_ENCODING = 'paper' needs cfg.LIDAR_BV_FROM_SCAN: stored bird's-eye-view maps are reference-encoded")
    return enc


def bev_channels():
    """channels of the network's `lidar_bv_data` under cfg.LIDAR_BV_ENCODING: 10 for 'paper', else 9"""
    return BEV_PAPER_SHAPE[2] if bev_encoding() == "paper" else BEV_SHAPE[2]


def scan_bev(points, offsets=None):
    """The network's `lidar_bv_data` from scans on the device, for every feed (get_minibatch, detect_batch.scan_feed): the raster
    cfg.LIDAR_BV_ENCODING names, on MV3D's ranges -- ops.point_cloud_2_top_batch ('reference') or ops.point_cloud_2_top_paper."""
    return (point_cloud_2_top_paper if bev_encoding() == "paper" else point_cloud_2_top_batch)(points, offsets=offsets)


def scan_crop():
    """cfg.LIDAR_CROP_TO_IMAGE checked: True where the feeds crop their scans to the image (scan_crop_to_image); on without
    cfg.LIDAR_BV_FROM_SCAN raises ValueError (stored lidar_bv/*.npy maps hold every point and cannot be cropped).  prepare_roidb and
    the detection loops call it before they load a frame."""
    from .fast_rcnn.config import cfg
    on = bool(cfg.LIDAR_CROP_TO_IMAGE)
    if on and not cfg.LIDAR_BV_FROM_SCAN:
        raise ValueError("cfg.LIDAR_CROP_TO_IMAGE needs cfg.LIDAR_BV_FROM_SCAN: stored bird's-eye-view maps hold every point and cannot be cropped")
    return on


def scan_crop_workspace_bytes(total_points):
    """bytes of workspace ops.scan_crop_to_image needs for a batch of total_points rows: one bit per row and 4 bytes per tile"""
    return int(lib().mv3d_scan_crop_workspace(int(total_points)))


def scan_crop_tile_rows():
    """the consecutive rows one workgroup of the crop compacts (mv3d_scan_crop_tile_rows, host only): the sizes its tests are built on"""
    return int(lib().mv3d_scan_crop_tile_rows())


def _crop_tables(fn, calib, image_hw, B):
    """calib -> (B,48) f32, image_hw -> (B,2) int32, each a device tensor that passed or a host array to upload; raises as
    scan_crop_to_image says"""
    if isinstance(calib, torch.Tensor):
        if calib.dtype != torch.float32:
            raise TypeError("{}: a calib tensor must be float32, got {}".format(fn, calib.dtype))
    else:
        calib = np.asarray(calib)
        if calib.dtype.kind != "f":
            raise TypeError("{}: calib must be floating point, got {}".format(fn, calib.dtype))
        calib = np.ascontiguousarray(calib, np.float32)          # (the feeds' cast of a frame's table)
    if tuple(calib.shape) not in ((B, 4, 12), (B, 48)):
        raise ValueError("{}: calib must be ({}, 4, 12) or ({}, 48), one table per frame, got {}".format(fn, B, B, tuple(calib.shape)))
    if isinstance(image_hw, torch.Tensor):
        if image_hw.dtype != torch.int32:
            raise TypeError("{}: an image_hw tensor must be int32, got {}".format(fn, image_hw.dtype))
        if tuple(image_hw.shape) != (B, 2):
            raise ValueError("{}: image_hw must be ({}, 2) [height, width], got {}".format(fn, B, tuple(image_hw.shape)))
    else:
        image_hw = np.asarray(image_hw)
        if not np.issubdtype(image_hw.dtype, np.integer):
            raise TypeError("{}: image_hw must be integers, got {}".format(fn, image_hw.dtype))
        if image_hw.ndim != 2 or image_hw.shape[0] != B or image_hw.shape[1] not in (2, 3):
            raise ValueError("{}: image_hw must be ({}, 2) [height, width] or the frames' image shapes, got {}".format(fn, B, image_hw.shape))
        if image_hw.size and (image_hw.min() < -2 ** 31 or image_hw.max() >= 2 ** 31):
            raise ValueError("{}: image_hw does not fit int32".format(fn))
        image_hw = np.ascontiguousarray(image_hw[:, :2], np.int32)
    return calib.reshape(B, 48), image_hw


def scan_crop_to_image(points, offsets, calib, image_hw, out=None, offsets_out=None, workspace=None):
    """The paper's crop to the camera image (csrc/scan_crop.hip; parity unpinned, the definition is
    tests/scan_crop_restatement.py): B clouds back to back -> (points_out, offsets_out), the batch of the rows whose projection by
    their frame's calibration table falls inside their frame's image, frames and rows in their order, every kept row bit for bit.
    Both results are device tensors and nothing is read back: points_out is (P,4) f32 of which rows offsets_out[0] = 0 ..
    offsets_out[B] are written, offsets_out (B + 1) int32 -- what ops.point_cloud_2_top_batch, ops.point_cloud_2_top_paper and
    ops.point_cloud_2_front take as (points, offsets); the rows behind offsets_out[B] belong to no frame.
    points, offsets as ops.point_cloud_2_front takes them (offsets None: one frame of every row).  calib = (B,4,12) or (B,48) f32, or
    a list of the frames' (4,12) tables (host values of any float type are cast to f32, as the feeds cast `calib`); image_hw = (B,2)
    integers [height, width], or a list of the frames' image shapes (h, w) / (h, w, 3); a frame whose height or width is <= 0 keeps
    nothing.  Numpy inputs are uploaded; tensors (calib f32, image_hw int32) must live on the points' device.
    out = a contiguous (P,4) f32 device tensor, 16-byte aligned and apart from `points`, offsets_out = a contiguous (B + 1) int32 device
    tensor, workspace = a uint8 device tensor of scan_crop_workspace_bytes(P) bytes, 16-byte aligned (default: the reused per-stream
    buffer); with all three and device inputs the call allocates nothing and can be captured, and a replay may find other clouds and
    other offsets in the same buffers.  Every argument is checked before anything is uploaded, allocated or launched: TypeError for
    a wrong dtype, ValueError for a wrong shape, value or device.  Under malformed device offsets the call stays inside its buffers
    and drops the rows no frame owns (include/mv3d_hip.h)."""
    fn = "scan_crop_to_image"
    tables = None

    def more(B, P, dev):
        nonlocal tables
        tables = _crop_tables(fn, calib, image_hw, B)
        for name, t, dtype, shape in (("out", out, torch.float32, (P, 4)), ("offsets_out", offsets_out, torch.int32, (B + 1,))):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dtype:
                raise TypeError("{}: {} must be a {} tensor".format(fn, name, dtype))
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("{}: {} must be contiguous {}, got {}".format(fn, name, shape, tuple(t.shape)))
        mine = [(n, t) for n, t in (("calib", tables[0]), ("image_hw", tables[1]), ("out", out), ("offsets_out", offsets_out))
                if isinstance(t, torch.Tensor)]
        for name, t in mine:                                     # (a numpy cloud with no tensor beside it goes to the current device)
            if not t.is_cuda or t.device != (dev if isinstance(dev, torch.device) else torch.device("cuda", torch.cuda.current_device())):
                raise ValueError("{}: {} on {}: every tensor must live on one HIP device".format(fn, name, t.device))
        if out is not None:
            if out.data_ptr() % 16:
                raise ValueError("{}: out must be 16-byte aligned".format(fn))
            if isinstance(points, torch.Tensor) and P and out.data_ptr() < points.data_ptr() + 16 * P and points.data_ptr() < out.data_ptr() + 16 * P:
                raise ValueError("{}: out must not overlap points".format(fn))
        if workspace is not None and workspace.data_ptr() % 16:
            raise ValueError("{}: workspace must be 16-byte aligned".format(fn))

    need = lambda B: scan_crop_workspace_bytes(points.shape[0])
    pts, off, B, P, _, dev = _scan_args(fn, points, offsets, None, None, workspace, need, more=more)
    cal, hw = ((t if isinstance(t, torch.Tensor) else torch.from_numpy(t).to(pts.device)).contiguous() for t in tables)
    if out is None:
        out = torch.empty((P, 4), dtype=torch.float32, device=pts.device)
    if offsets_out is None:
        offsets_out = torch.empty((B + 1,), dtype=torch.int32, device=pts.device)
    if workspace is None:
        workspace = _workspace(need(B), pts.device, "scan_crop")
    check(lib().mv3d_scan_crop_to_image(_ptr(pts), _ptr(off), B, P, _ptr(cal), _ptr(hw), _ptr(out), _ptr(offsets_out), _ptr(workspace),
                                        workspace.numel(), _stream()), "mv3d_scan_crop_to_image")
    return out, offsets_out


def scan_augment():
    """cfg.TRAIN.SCAN_AUGMENT checked: True where training transforms its scans (scan_transform, datasets/augment.py); on without
    cfg.LIDAR_BV_FROM_SCAN raises ValueError (a stored lidar_bv/*.npy map cannot be rotated), as does a scale bound <= 0 or any
    other range datasets.augment.check_config refuses.  prepare_roidb calls it before the first step."""
    from .datasets.augment import check_config
    return check_config()


def scan_transform(points, offsets, xform, out=None):
    """Scan augmentation's transform of the points (csrc/scan_transform.hip; parity unpinned, the definition
    is tests/scan_augment_restatement.py): B clouds back to back -> the (P,4) f32 device tensor of their rows, a row [x, y, z, r] of
    frame b with finite x, y, z taken to A_b . [x, y, z, 1] (one f64 fma chain per coordinate, rounded to f32 once) and r kept bit for
    bit.  A row with a non-finite coordinate and a row no frame owns come back as the same bits.
    points, offsets as ops.point_cloud_2_front takes them (offsets None: one frame of every row).  xform = (B,3,4) or (B,12) f64, per
    frame the matrix A of datasets.augment.transform_matrix (a numpy array, which is uploaded, or a device tensor).
    out = None allocates the result; out = points (the same device tensor) transforms in place; any other out must be a contiguous
    (P,4) f32 device tensor, 16-byte aligned, with no byte in common with points.  With device inputs and out given the call
    allocates nothing and can be captured, and a replay may find other clouds, offsets and matrices in the same buffers.  Every
    argument is checked before anything is uploaded, allocated or launched: TypeError for a wrong dtype, ValueError for a wrong
    shape, value or device.  Under malformed device offsets the call stays inside its buffers (include/mv3d_hip.h)."""
    fn = "scan_transform"
    table = None

    def more(B, P, dev):
        nonlocal table
        if isinstance(xform, torch.Tensor):
            if xform.dtype != torch.float64:
                raise TypeError("{}: an xform tensor must be float64, got {}".format(fn, xform.dtype))
            table = xform
        else:
            table = np.asarray(xform)
            if table.dtype != np.float64:
                raise TypeError("{}: xform must be float64, got {}".format(fn, table.dtype))
        if tuple(table.shape) not in ((B, 3, 4), (B, 12)):
            raise ValueError("{}: xform must be ({}, 3, 4) or ({}, 12), one matrix per frame, got {}".format(fn, B, B, tuple(table.shape)))
        # (a numpy cloud with no tensor beside it goes to the current device)
        here = lambda t: t.is_cuda and t.device == (dev if isinstance(dev, torch.device) else torch.device("cuda", torch.cuda.current_device()))
        if isinstance(table, torch.Tensor) and not here(table):
            raise ValueError("{}: xform on {}: every tensor must live on one HIP device".format(fn, table.device))
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.float32:
                raise TypeError("{}: out must be a {} tensor".format(fn, torch.float32))
            if tuple(out.shape) != (P, 4) or not out.is_contiguous():
                raise ValueError("{}: out must be contiguous {}, got {}".format(fn, (P, 4), tuple(out.shape)))
            if not here(out):
                raise ValueError("{}: out on {}: every tensor must live on one HIP device".format(fn, out.device))
            if out.data_ptr() % 16:
                raise ValueError("{}: out must be 16-byte aligned".format(fn))
            if isinstance(points, torch.Tensor) and P and out.data_ptr() != points.data_ptr() and \
                    out.data_ptr() < points.data_ptr() + 16 * P and points.data_ptr() < out.data_ptr() + 16 * P:
                raise ValueError("{}: out must be points itself or not overlap it".format(fn))
            if isinstance(points, torch.Tensor) and out.data_ptr() == points.data_ptr() and P and not points.is_contiguous():
                raise ValueError("{}: points must be contiguous to be transformed in place".format(fn))

    pts, off, B, P, _, dev = _scan_args(fn, points, offsets, None, None, more=more)
    if pts.data_ptr() % 16:
        raise ValueError("{}: points must be 16-byte aligned".format(fn))
    A = (table if isinstance(table, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(table)).to(pts.device)).contiguous()
    if out is None:
        out = torch.empty((P, 4), dtype=torch.float32, device=pts.device)
    check(lib().mv3d_scan_transform(_ptr(pts), _ptr(off), B, P, _ptr(A), _ptr(out), _stream()), "mv3d_scan_transform")
    return out


def gt_encode(box_cam, cos_sin, inv_rot, tr):
    """box_cam (G,6) f32, cos_sin (G,2) f64, inv_rot (9) f32, tr (12) f32 device tensors -> (corners_cam (G,24),
    corners_lidar (G,24), boxes_3d (G,6), boxes_bv (G,4)) f32 in ONE buffer (pack, views): a host caller fetches it with
    one copy."""
    G = box_cam.shape[0]
    spec = [((G, 24), torch.float32), ((G, 24), torch.float32), ((G, 6), torch.float32), ((G, 4), torch.float32)]
    pack, views = packed_views(spec, box_cam.device)
    check(lib().mv3d_gt_encode(_ptr(box_cam), _ptr(cos_sin), G, _ptr(inv_rot), _ptr(tr), _ptr(views[0]), _ptr(views[1]),
                               _ptr(views[2]), _ptr(views[3]), _stream()), "mv3d_gt_encode")
    return pack, spec, views


def mirror_columns(t):
    """Left/right mirror of a (..., W, C) f32 device tensor IN PLACE on the current stream (mv3d_mirror_columns): afterwards
    t[..., w, :] holds the old t[..., W - 1 - w, :].  Returns t.  The tensor must be contiguous (a slice along the leading axes
    is); anything else raises -- there is no torch path."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise TypeError("mirror_columns: a CUDA float32 tensor is required, got %s"
                        % ("%s on %s" % (t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t).__name__))
    if t.dim() < 3 or not t.is_contiguous() or t.shape[-1] < 1 or t.shape[-2] < 1:
        raise ValueError("mirror_columns: a contiguous (..., W, C) tensor with W, C >= 1 is required, got shape %s strides %s"
                         % (tuple(t.shape), tuple(t.stride())))
    W, Cn = int(t.shape[-2]), int(t.shape[-1])
    with torch.cuda.device(t.device):
        check(lib().mv3d_mirror_columns(_ptr(t), t.numel() // (W * Cn), W, Cn, _stream()), "mv3d_mirror_columns")
    return t


# ------------------------------------------------------------------ image input
IMAGE_MAX_FRAMES = 1024              # MV3D_IMAGE_MAX_FRAMES


def pack_image_frames(images):
    """A list of (h, w, 3) uint8 images -> (pixels, frames, (H, W)): ONE contiguous uint8 host buffer with the frames' pixels back to
    back, the (B, 4) int32 table [byte offset, h, w, flip = 0] that ops.image_blob takes, and the maximal height and width.
    TypeError for anything that is not a uint8 array, ValueError for another shape, an empty list or more than INT_MAX bytes."""
    images = list(images)
    if not images:
        raise ValueError("pack_image_frames: no image")
    for k, im in enumerate(images):
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8:
            raise TypeError("pack_image_frames: image {} must be a uint8 numpy array, got {}".format(
                k, im.dtype if isinstance(im, np.ndarray) else type(im).__name__))
        if im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
            raise ValueError("pack_image_frames: image {} must be (h, w, 3) with h, w >= 1, got {}".format(k, im.shape))
    frames = np.zeros((len(images), 4), np.int64)
    frames[:, 1] = [im.shape[0] for im in images]
    frames[:, 2] = [im.shape[1] for im in images]
    sizes = 3 * frames[:, 1] * frames[:, 2]
    frames[1:, 0] = np.cumsum(sizes)[:-1]
    total = int(sizes.sum())
    if total > 0x7fffffff:
        raise ValueError("pack_image_frames: {} bytes of pixels, at most 2^31 - 1 go into one call".format(total))
    pixels = np.empty((total,), np.uint8)
    for im, o, n in zip(images, frames[:, 0], sizes):
        pixels[o:o + n] = im.reshape(-1)
    return pixels, frames.astype(np.int32), (int(frames[:, 1].max()), int(frames[:, 2].max()))


def _pixel_means():
    from .fast_rcnn.config import cfg                         # (fast_rcnn imports ops)
    return cfg.PIXEL_MEANS


def image_blob(pixels, frames=None, canvas=None, means=None, flip=None, out=None):
    """uint8 BGR frames of their own sizes -> the (B, H, W, 3) f32 image blob on the device in ONE launch (csrc/image_blob.hip, DESIGN.md
    section 3.23): out[b, y, x, c] = float32(float64(frame_b[y, x', c]) - means[c]) at the top-left corner of a canvas of +0.0 (the
    reference's im_list_to_blob), x' = w_b - 1 - x for a frame whose flip flag is set (the mirror within its own width).
    pixels   a 1-D uint8 buffer with the frames' pixels back to back, a device tensor or a numpy array (uploaded); or a list of
             (h, w, 3) uint8 images, packed first (pack_image_frames; frames must then be None)
    frames   (B, 4) int32 [byte offset, h, w, flip], a device tensor or a host array / sequence (uploaded)
    canvas   (H, W); None = the frames' maximal height and width, which needs a host table
    means    three numbers; None = cfg.PIXEL_MEANS
    flip     a per-frame sequence of flags, folded into a host table's fourth column (a device table carries its own)
    out      a contiguous f32 device tensor of the result's shape to write into; it may be any slice of frames of a larger batch buffer
             (4-byte alignment is all it needs).  With device inputs and out= the call allocates nothing and can be captured.
    Every argument is checked before anything is uploaded or launched: TypeError for a dtype other than uint8 / int32 / f32,
    ValueError for shapes, devices, a frame larger than the canvas or a table that does not fit `pixels`.  The VALUES of the table are
    checked only when it comes from the host: reading a device tensor would synchronise.  Under a malformed device table the call stays
    inside its buffers and the frames it cannot use come out as zeros (include/mv3d_hip.h).  There is no torch path."""
    fn = "image_blob"
    if isinstance(pixels, (list, tuple)):
        if frames is not None:
            raise ValueError("{}: a list of images brings its own table, frames must be None".format(fn))
        pixels, frames, _ = pack_image_frames(pixels)
    if frames is None:
        raise ValueError("{}: frames, the (B, 4) int32 table [byte offset, h, w, flip], is required".format(fn))
    if isinstance(pixels, torch.Tensor):
        if pixels.dtype != torch.uint8:
            raise TypeError("{}: pixels must be uint8, got {}".format(fn, pixels.dtype))
        if not pixels.is_cuda:
            raise ValueError("{}: a pixels tensor must live on the device (pass a numpy array to have it uploaded)".format(fn))
    else:
        pixels = np.asarray(pixels)
        if pixels.dtype != np.uint8:
            raise TypeError("{}: pixels must be uint8, got {}".format(fn, pixels.dtype))
    if pixels.ndim != 1 or (isinstance(pixels, torch.Tensor) and not pixels.is_contiguous()):
        raise ValueError("{}: pixels must be one contiguous run of bytes, got shape {}".format(fn, tuple(pixels.shape)))
    total = int(pixels.shape[0])
    if total > 0x7fffffff:
        raise ValueError("{}: {} bytes of pixels, at most 2^31 - 1 go into one call".format(fn, total))
    host_table = not isinstance(frames, torch.Tensor)
    if host_table:
        frames = np.asarray(frames)
        if not np.issubdtype(frames.dtype, np.integer):
            raise TypeError("{}: frames must be integers, got {}".format(fn, frames.dtype))
    elif frames.dtype != torch.int32:
        raise TypeError("{}: a frames tensor must be int32, got {}".format(fn, frames.dtype))
    if frames.ndim != 2 or frames.shape[1] != 4 or not 1 <= frames.shape[0] <= IMAGE_MAX_FRAMES:
        raise ValueError("{}: frames must be (B, 4) with 1 <= B <= {}, got {}".format(fn, IMAGE_MAX_FRAMES, tuple(frames.shape)))
    B = int(frames.shape[0])
    if flip is not None:
        if not host_table:
            raise ValueError("{}: flip= is folded into a host table; a device table carries the flags in its fourth column".format(fn))
        flags = np.asarray(flip).reshape(-1)
        if flags.shape[0] != B:
            raise ValueError("{}: flip must have one flag per frame ({}), got {}".format(fn, B, flags.shape[0]))
        frames = frames.astype(np.int64)
        frames[:, 3] = flags != 0
    if canvas is None:
        if not host_table:
            raise ValueError("{}: canvas=None (the frames' maximal shape) needs a host table; give canvas=(H, W)".format(fn))
        canvas = (int(frames[:, 1].max()), int(frames[:, 2].max()))
    if len(canvas) != 2:
        raise ValueError("{}: canvas must be (H, W), got {}".format(fn, canvas))
    Hc, Wc = int(canvas[0]), int(canvas[1])
    if Hc < 1 or Wc < 1 or Hc * Wc * 3 > 0x7fffffff:
        raise ValueError("{}: a canvas has sides >= 1 and fewer than 2^31 elements, got {}".format(fn, (Hc, Wc)))
    if host_table:
        f = frames.astype(np.int64)
        if (f[:, 1:3] < 1).any() or (f[:, 0] < 0).any():
            raise ValueError("{}: a frame needs offset >= 0 and h, w >= 1, got {}".format(fn, f.tolist()))
        if (f[:, 1] > Hc).any() or (f[:, 2] > Wc).any():
            b = int(np.argmax((f[:, 1] > Hc) | (f[:, 2] > Wc)))
            raise ValueError("{}: frame {} is {} x {}, larger than the canvas {} x {}".format(fn, b, f[b, 1], f[b, 2], Hc, Wc))
        if (f[:, 0] + 3 * f[:, 1] * f[:, 2] > total).any():
            raise ValueError("{}: the table does not fit pixels: a frame ends behind its {} bytes".format(fn, total))
        if (np.abs(f) > 0x7fffffff).any():
            raise ValueError("{}: the table's values must fit int32".format(fn))
    m = np.asarray(_pixel_means() if means is None else means, np.float64).reshape(-1)
    if m.shape[0] != 3:
        raise ValueError("{}: means must be three numbers, got {}".format(fn, m.shape[0]))
    shape = (B, Hc, Wc, 3)
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32):
        raise TypeError("{}: out must be a {} tensor".format(fn, torch.float32))
    tensors = [(n, t) for n, t in (("pixels", pixels), ("frames", frames), ("out", out)) if isinstance(t, torch.Tensor)]
    for name, t in tensors:
        if not t.is_cuda or t.device != tensors[0][1].device:
            raise ValueError("{}: {} on {}: every tensor must live on one HIP device".format(fn, name, t.device))
        if name != "pixels" and not t.is_contiguous():
            raise ValueError("{}: {} must be contiguous".format(fn, name))
    dev = tensors[0][1].device if tensors else "cuda"
    if out is not None and tuple(out.shape) != shape:
        raise ValueError("{}: out must be {}, got {}".format(fn, shape, tuple(out.shape)))
    pix = pixels if isinstance(pixels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pixels)).to(dev)
    tab = torch.from_numpy(np.ascontiguousarray(frames, np.int32)).to(dev) if host_table else frames
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    with torch.cuda.device(out.device):
        check(lib().mv3d_image_blob(_ptr(pix), total, _ptr(tab), B, (C.c_double * 3)(*m), Hc, Wc, _ptr(out), _stream()), "mv3d_image_blob")
    return out


# ------------------------------------------------------------------ the deep-fusion join
_FJ_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _fusion_join_args(h, keep, drop, what):
    if not isinstance(h, torch.Tensor) or not h.is_cuda or h.dtype not in _FJ_DTYPES:
        raise TypeError("%s: a CUDA float32 / float16 / bfloat16 tensor is required, got %s"
                        % (what, "%s on %s" % (h.dtype, h.device) if isinstance(h, torch.Tensor) else type(h).__name__))
    if h.dim() != 4 or not h.is_contiguous():
        raise ValueError("%s: h must be a contiguous (sets_in, views, rows, channels) tensor, got shape %s strides %s"
                         % (what, tuple(h.shape), tuple(h.stride())))
    S, V, R, Cn = (int(n) for n in h.shape)
    k = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
    if k.ndim != 2 or k.shape[1] != V:
        raise ValueError("%s: keep must be (paths, %d views), got shape %s" % (what, V, k.shape))
    P = int(k.shape[0])
    if drop is not None:
        if not isinstance(drop, torch.Tensor) or drop.device != h.device or drop.dtype != torch.uint8 or not drop.is_contiguous() \
                or tuple(drop.shape) != (P, R, Cn):
            raise ValueError("%s: drop must be a contiguous uint8 tensor of shape %s on %s" % (what, (P, R, Cn), h.device))
    return S, P, V, R, Cn, k


def fusion_join(h, keep, drop=None, scale=1.0):
    """The deep-fusion join, forward (mv3d_fusion_join_forward): h (sets_in, views, rows, channels) pre-ReLU, keep (paths, views)
    host 0 / 1, drop None or (paths, rows, channels) uint8 on the device -> (paths, rows, channels) in h's type: the mean over each
    path's kept views of relu(h), dropout applied to the mean.  Device tensors only; there is no torch path."""
    S, P, V, R, Cn, k = _fusion_join_args(h, keep, drop, "fusion_join")
    out = torch.empty((P, R, Cn), dtype=h.dtype, device=h.device)
    with torch.cuda.device(h.device):
        check(lib().mv3d_fusion_join_forward(_ptr(h), _FJ_DTYPES[h.dtype], S, P, V, R, Cn, k.ctypes.data_as(C.c_void_p), _ptr(drop),
                                             C.c_float(scale), _ptr(out), _stream()), "mv3d_fusion_join_forward")
    return out


def fusion_join_backward(h, g_out, keep, drop=None, scale=1.0):
    """The join's gradient (mv3d_fusion_join_backward): g_out (paths, rows, channels) in h's type -> g_h of h's shape and type;
    with sets_in == 1 the paths' contributions are added in ascending path order.  Views a path dropped get zeros."""
    S, P, V, R, Cn, k = _fusion_join_args(h, keep, drop, "fusion_join_backward")
    if not isinstance(g_out, torch.Tensor) or g_out.device != h.device or g_out.dtype != h.dtype or not g_out.is_contiguous() \
            or tuple(g_out.shape) != (P, R, Cn):
        raise ValueError("fusion_join_backward: g_out must be a contiguous %s tensor of shape %s on %s" % (h.dtype, (P, R, Cn), h.device))
    g_h = torch.empty_like(h)
    with torch.cuda.device(h.device):
        check(lib().mv3d_fusion_join_backward(_ptr(h), _ptr(g_out), _FJ_DTYPES[h.dtype], S, P, V, R, Cn, k.ctypes.data_as(C.c_void_p),
                                              _ptr(drop), C.c_float(scale), _ptr(g_h), _stream()), "mv3d_fusion_join_backward")
    return g_h


class FusionJoin(torch.autograd.Function):
    """apply(h, keep, drop, scale) -> the joined activations; differentiable in h"""

    @staticmethod
    def forward(ctx, h, keep, drop, scale):
        h = h.detach().contiguous()
        ctx.keep, ctx.scale = np.array(keep, copy=True), float(scale)
        ctx.save_for_backward(h, drop)
        return fusion_join(h, keep, drop, scale)

    @staticmethod
    def backward(ctx, g_out):
        h, drop = ctx.saved_tensors
        return fusion_join_backward(h, g_out.contiguous(), ctx.keep, drop, ctx.scale), None, None, None


# ------------------------------------------------------------------ upsampled ROI features
def _upsample_view_checks(x, factor, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in _FJ_DTYPES:
        raise TypeError("%s: a CUDA float32 / float16 / bfloat16 tensor is required, got %s"
                        % (what, "%s on %s" % (x.dtype, x.device) if isinstance(x, torch.Tensor) else type(x).__name__))
    if x.dim() != 4 or x.shape[1] < 1 or x.shape[2] < 1 or x.shape[3] < 1:
        raise ValueError("%s: a (batch, height, width, channels) tensor with height, width, channels >= 1 is required, got shape %s"
                         % (what, tuple(x.shape)))
    if factor not in (2, 4):
        raise ValueError("%s: the factor must be 2 or 4, got %r" % (what, factor))


def _nhwc_strides(t):
    """element strides (frame, row, pixel, channel) of a 4-D tensor; an axis of one element may carry any stride (it is never stepped
    along), so it gets the stride a contiguous tensor would have"""
    B, H, W, Cn = t.shape
    if B == 0:
        return H * W * Cn, W * Cn, Cn, 1
    fs, rs, ps, cs = t.stride()
    cs = 1 if Cn == 1 else cs
    ps = Cn * cs if W == 1 else ps
    rs = W * ps if H == 1 else rs
    fs = H * rs if B <= 1 else fs
    return fs, rs, ps, cs


def _upsample_out(outs, k, shape, device):
    if outs is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    y = outs[k]
    if tuple(y.shape) != shape or y.dtype != torch.float32 or y.device != device or not y.is_contiguous():
        raise ValueError("outs[%d] must be a contiguous float32 tensor of shape %s on %s" % (k, shape, device))
    return y


def upsample_bilinear_views(views, outs=None):
    """views: [(x (B, H, W, C) device tensor f32 / f16 / bf16, factor 2 | 4), ...] -> [y (B, s H, s W, C) f32, ...]: the bilinear
    upsampling in front of RoiPool (mv3d_upsample_bilinear_views: up-pixel o at source coordinate o / s, so up-pixel s i is source pixel
    i), ONE launch for all views.  A strided x (unit channel stride, e.g. the interior y[:, 1:-1, 1:-1] of a framed map) is read where
    it lies; anything else is made contiguous first.  outs: contiguous f32 tensors to write into instead of fresh ones.  Device tensors
    only; there is no torch path."""
    if not 1 <= len(views) <= _lib.MAX_ROI_VIEWS:
        raise ValueError("upsample_bilinear_views: 1..%d views, got %d" % (_lib.MAX_ROI_VIEWS, len(views)))
    arr = (_lib.UpsampleView * len(views))()
    res, held = [], []
    for k, (x, s) in enumerate(views):
        _upsample_view_checks(x, s, "upsample_bilinear_views")
        B, H, W, Cn = (int(n) for n in x.shape)
        fs, rs, ps, cs = _nhwc_strides(x)
        if not (cs == 1 and ps >= Cn and rs >= W * ps and fs >= H * rs):
            x = x.contiguous()
            fs, rs, ps, cs = _nhwc_strides(x)
        held.append(x)
        y = _upsample_out(outs, k, (B, s * H, s * W, Cn), x.device)
        arr[k] = _lib.UpsampleView(x.data_ptr(), y.data_ptr(), fs, rs, ps, _FJ_DTYPES[x.dtype], B, H, W, Cn, s)
        res.append(y)
    with torch.cuda.device(res[0].device):
        check(lib().mv3d_upsample_bilinear_views(len(views), arr, _stream()), "mv3d_upsample_bilinear_views")
    return res


def upsample_bilinear(x, factor):
    """one view of upsample_bilinear_views"""
    return upsample_bilinear_views([(x, factor)])[0]


def upsample_bilinear_backward_views(views, outs=None):
    """views: [(g_y (B, s H, s W, C) f32 device tensor, factor), ...] -> [g_x (B, H, W, C) f32, ...]: the exact transpose of
    upsample_bilinear_views (mv3d_upsample_bilinear_backward_views), ONE launch, every element
    written by the one thread that owns it (outs: tensors to write into; they need no zeroing)."""
    if not 1 <= len(views) <= _lib.MAX_ROI_VIEWS:
        raise ValueError("upsample_bilinear_backward_views: 1..%d views, got %d" % (_lib.MAX_ROI_VIEWS, len(views)))
    arr = (_lib.UpsampleView * len(views))()
    res, held = [], []
    for k, (g, s) in enumerate(views):
        _upsample_view_checks(g, s, "upsample_bilinear_backward_views")
        if g.dtype != torch.float32 or g.shape[1] % s or g.shape[2] % s:
            raise ValueError("upsample_bilinear_backward_views: g_y must be float32 of shape (B, %d H, %d W, C), got %s %s"
                             % (s, s, g.dtype, tuple(g.shape)))
        g = g.contiguous()
        held.append(g)
        B, H, W, Cn = int(g.shape[0]), int(g.shape[1]) // s, int(g.shape[2]) // s, int(g.shape[3])
        gx = _upsample_out(outs, k, (B, H, W, Cn), g.device)
        arr[k] = _lib.UpsampleView(g.data_ptr(), gx.data_ptr(), 0, 0, 0, 0, B, H, W, Cn, s)
        res.append(gx)
    with torch.cuda.device(res[0].device):
        check(lib().mv3d_upsample_bilinear_backward_views(len(views), arr, _stream()), "mv3d_upsample_bilinear_backward_views")
    return res


class UpsampleBilinearViews(torch.autograd.Function):
    """apply(factors, x_0, x_1, ...) -> (y_0, y_1, ...): upsample_bilinear_views, differentiable in every x; forward and backward are
    ONE launch each for all views.  f32 gradients; a view whose output gets no gradient contributes zeros."""

    @staticmethod
    def forward(ctx, factors, *xs):
        ctx.factors = tuple(int(s) for s in factors)
        ctx.shapes = [tuple(x.shape) for x in xs]
        ctx.device = xs[0].device
        return tuple(upsample_bilinear_views([(x.detach(), s) for x, s in zip(xs, ctx.factors)]))

    @staticmethod
    def backward(ctx, *grads):
        views = []
        for g, s, (B, H, W, Cn) in zip(grads, ctx.factors, ctx.shapes):
            if g is None:
                g = torch.zeros((B, s * H, s * W, Cn), dtype=torch.float32, device=ctx.device)
            views.append((g.float(), s))
        return (None,) + tuple(upsample_bilinear_backward_views(views))


# ------------------------------------------------------------------ training losses
def _loss_call(fn, name, cls, labels, pred, tgt, extra, sigma, want_grad):
    dev = cls.device
    R = cls.shape[0]
    losses = torch.empty((2,), dtype=torch.float32, device=dev)
    d_cls = torch.empty_like(cls) if want_grad else None
    d_pred = torch.empty_like(pred) if want_grad else None
    ws = _workspace(lib().mv3d_loss_workspace_bytes(R), dev, "loss")
    check(fn(_ptr(cls), _ptr(labels), _ptr(pred), _ptr(tgt), R, *extra, C.c_float(sigma), _ptr(losses), _ptr(d_cls), _ptr(d_pred),
             _ptr(ws), ws.numel(), _stream()), name)
    return losses, d_cls, d_pred


def softmax_rows(logits):
    """softmax over the last axis of an f32 device tensor (any leading shape), forward only: mv3d_softmax_rows"""
    x = logits.detach().contiguous()
    y = torch.empty_like(x)
    K = int(x.shape[-1])
    check(lib().mv3d_softmax_rows(_ptr(x), _ptr(y), x.numel() // max(K, 1), K, _stream()), "mv3d_softmax_rows")
    return y


def rpn_loss(rpn_cls_score, rpn_labels, rpn_bbox_pred, rpn_bbox_targets, sigma=3.0, want_grad=True):
    """(N,2) logits, (N) f32 labels in {-1,0,1}, (N,6) pred / targets -> (losses[2] = [cross-entropy, box], d_cls, d_pred)."""
    return _loss_call(lib().mv3d_rpn_loss, "mv3d_rpn_loss", rpn_cls_score, rpn_labels, rpn_bbox_pred, rpn_bbox_targets, (),
                      sigma, want_grad)


def rcnn_loss(cls_score, labels, bbox_pred, bbox_targets, sigma=3.0, want_grad=True, ignore_label=None):
    """(S,K) logits, (S) i32 labels, (S,D) pred / targets -> (losses[2], d_cls, d_pred).  ignore_label=-1 (not in the reference,
    DESIGN.md section 3.26): rows with that label take no part in either term (mv3d_rcnn_loss_ignore: means over the other rows, NaN
    over none, zero gradient rows); None = the reference's every row, where a label of -1 poisons the loss."""
    if ignore_label is None:
        fn, name = lib().mv3d_rcnn_loss, "mv3d_rcnn_loss"
    elif int(ignore_label) == -1:
        fn, name = lib().mv3d_rcnn_loss_ignore, "mv3d_rcnn_loss_ignore"
    else:
        raise ValueError("rcnn_loss: ignore_label must be None or -1, got %r" % (ignore_label,))
    return _loss_call(fn, name, cls_score, labels, bbox_pred, bbox_targets, (cls_score.shape[1], bbox_pred.shape[1]), sigma, want_grad)


# ------------------------------------------------------------------ ignore regions in training
IGNORE_MAX_BOXES = 1024               # TARGET_MAX_GT: ignore boxes per frame and list


def pack_box_lists(frames):
    """per-frame (K_b, 4) host arrays -> (rows (sum K_b, 4) f32, offsets (B + 1) int32): the packed form ignore_relabel takes"""
    arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 4) for a in frames]
    off = np.zeros((len(arrs) + 1,), np.int32)
    off[1:] = np.cumsum([a.shape[0] for a in arrs])
    return (np.concatenate(arrs, 0) if arrs else np.zeros((0, 4), np.float32)), off


def _is_packed(v):
    if not (isinstance(v, tuple) and len(v) == 2):
        return False
    if isinstance(v[1], torch.Tensor):
        return v[1].dim() == 1 and v[1].dtype == torch.int32
    return np.ndim(v[1]) == 1 and np.issubdtype(np.asarray(v[1]).dtype, np.integer)


def ignore_relabel(rpn_labels, roi_labels, rois_bv, rois_img, calib, H, W, ignore_bv, ignore_img, overlap, feat_stride=8,
                   want_counts=False, out=None):
    """Sampled background anchors and ROIs on an ignore region get label -1 (mv3d_ignore_relabel, one launch, out of place).
    rpn_labels (B, 4 H W) f32 and roi_labels (S) or (S, 1) int32 device tensors, rois_bv / rois_img (S, 5) f32 with the frame in column
    0, calib (B, 4, 12) f32.  ignore_bv / ignore_img: a sequence of B per-frame (K_b, 4) arrays, or an already packed (rows, offsets)
    tuple -- rows (R, 4) f32, offsets (B + 1) int32; host lists cross in ONE copy, packed device tensors are used where they lie (no
    allocation beyond the outputs, capturable with out=).  overlap: the f64 threshold on the intersection over the candidate's area.
    Returns (rpn_labels_out, roi_labels_out, counts, status): the labels in the inputs' shapes, counts (B, 2) int32 [anchors, ROIs]
    relabelled per frame (None unless want_counts), status (B) int32 = _lib.ERR_INVALID_ARG for a frame whose offsets are out of
    order, out of the rows or span more than IGNORE_MAX_BOXES (its labels are written through); all on the device, nothing is read
    back.  out = that tuple from an earlier call (counts may be None) to write into."""
    name = "ignore_relabel"
    for nm, t, dt in (("rpn_labels", rpn_labels, torch.float32), ("roi_labels", roi_labels, torch.int32), ("rois_bv", rois_bv, torch.float32),
                      ("rois_img", rois_img, torch.float32), ("calib", calib, torch.float32)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("%s: %s must be a device tensor" % (name, nm))
        if t.dtype != dt:
            raise TypeError("%s: %s must be %s, got %s" % (name, nm, dt, t.dtype))
    dev = rpn_labels.device
    H, W = int(H), int(W)
    if rpn_labels.dim() != 2 or rpn_labels.shape[1] != 4 * H * W:
        raise ValueError("%s: rpn_labels must be (B, %d), got %s" % (name, 4 * H * W, tuple(rpn_labels.shape)))
    B, S = int(rpn_labels.shape[0]), int(roi_labels.numel())
    if tuple(calib.shape) != (B, 4, 12):
        raise ValueError("%s: calib must be (%d, 4, 12), got %s" % (name, B, tuple(calib.shape)))
    if tuple(rois_bv.shape) != (S, 5) or tuple(rois_img.shape) != (S, 5):
        raise ValueError("%s: rois_bv and rois_img must be (%d, 5), got %s and %s" % (name, S, tuple(rois_bv.shape), tuple(rois_img.shape)))
    lists, host = [], []
    for nm, v in (("ignore_bv", ignore_bv), ("ignore_img", ignore_img)):
        if not _is_packed(v):
            if len(v) != B:
                raise ValueError("%s: %s holds %d frames, rpn_labels %d" % (name, nm, len(v), B))
            if any(isinstance(a, torch.Tensor) for a in v):
                v = [a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a for a in v]
            v = pack_box_lists(v)
        rows, off = v
        if isinstance(rows, torch.Tensor) != isinstance(off, torch.Tensor):
            raise ValueError("%s: %s rows and offsets must both be host arrays or both device tensors" % (name, nm))
        if isinstance(rows, torch.Tensor):
            if not (rows.is_cuda and off.is_cuda and rows.dtype == torch.float32 and off.dtype == torch.int32):
                raise TypeError("%s: packed %s must be f32 rows and int32 offsets on the device" % (name, nm))
            rows, off = rows.contiguous(), off.contiguous()
        else:
            rows, off = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(off, np.int32)
            host += [len(lists)]
        if rows.ndim != 2 or rows.shape[1] != 4 or off.shape[0] != B + 1:
            raise ValueError("%s: %s must be (R, 4) rows and %d offsets, got %s and %s" % (name, nm, B + 1, tuple(rows.shape), tuple(off.shape)))
        lists.append([rows, off])
    if host:
        up = iter(upload_packed([a for k in host for a in lists[k]], dev))
        for k in host:
            lists[k] = [next(up), next(up)]
    rl, qb, qi, cal = rpn_labels.contiguous(), rois_bv.contiguous(), rois_img.contiguous(), calib.contiguous()
    ql = roi_labels.contiguous()
    if out is None:
        out = (torch.empty_like(rl), torch.empty_like(ql), torch.empty((B, 2), dtype=torch.int32, device=dev) if want_counts else None,
               torch.empty((B,), dtype=torch.int32, device=dev))
    o_rpn, o_roi, counts, status = out
    if o_rpn.shape != rl.shape or o_roi.shape != ql.shape or o_rpn.dtype != rl.dtype or o_roi.dtype != ql.dtype or \
            not (o_rpn.is_contiguous() and o_roi.is_contiguous()):
        raise ValueError("%s: out does not fit the labels" % name)
    (rb, ob), (ri, oi) = lists
    with torch.cuda.device(dev):
        check(lib().mv3d_ignore_relabel(_ptr(rl), _ptr(ql), _ptr(qb), _ptr(qi), S, _ptr(cal), B, H, W, int(feat_stride),
                                        _ptr(rb) if rb.shape[0] else None, _ptr(ob), int(rb.shape[0]),
                                        _ptr(ri) if ri.shape[0] else None, _ptr(oi), int(ri.shape[0]), C.c_double(float(overlap)),
                                        _ptr(o_rpn), _ptr(o_roi), _ptr(counts), _ptr(status), _stream()), "mv3d_ignore_relabel")
    return o_rpn, o_roi, counts, status



# ------------------------------------------------------------------ the serving trunk's contraction (f16 MFMA)
# (the `_f16` functions take float16, bfloat16 or float32 tensors and pick the C entry by the tensor's dtype: f16 = the serving trunk,
# bf16 = the training trunk, f32 = the serving trunk in the reference's precision)
def _half_entry(stem, dtype):
    if dtype == torch.float16:
        return getattr(lib(), stem + "_f16"), stem + "_f16"
    if dtype == torch.bfloat16:
        return getattr(lib(), stem + "_bf16"), stem + "_bf16"
    if dtype == torch.float32:
        return getattr(lib(), stem + "_f32"), stem + "_f32"
    raise TypeError("float16, bfloat16 or float32 tensors expected, got %s" % dtype)


def pack_conv3x3_weights(w_oihw, c_in_pad=None, dtype=torch.float16):
    """torch (O, I, 3, 3) f32 -> (O, 9 * I') f16 / bf16 with k = (ky * 3 + kx) * I' + c, I' = I zero-padded to c_in_pad."""
    O, I = w_oihw.shape[:2]
    Ip = c_in_pad or I
    w = torch.zeros((O, 3, 3, Ip), dtype=dtype, device=w_oihw.device)
    w[..., :I] = w_oihw.detach().permute(0, 2, 3, 1).to(dtype)
    return w.reshape(O, 9 * Ip).contiguous()


def pack_conv3x3_weights_input_layer(w_oihw, dtype=torch.float16):
    """the input layer's packing (c_in <= 16, see mv3d_conv3x3_f16): (O, I, 3, 3) f32 -> (O, 12 * 16), k = 16 * tap + c"""
    O, I = w_oihw.shape[:2]
    w = torch.zeros((O, 12, 16), dtype=dtype, device=w_oihw.device)
    w[:, :9, :I] = w_oihw.detach().permute(0, 2, 3, 1).reshape(O, 9, I).to(dtype)
    return w.reshape(O, 192).contiguous()


def framed_buffer(B, H, W, C, device, dtype=torch.float16):
    """zeroed (B, H + 2, W + 2, C): the kernels below only ever write its interior, so the SAME-padding frame stays 0"""
    return torch.zeros((B, H + 2, W + 2, C), dtype=dtype, device=device)


def frame_nhwc_f16(x_nhwc, out):
    """(B, H, W, C) f32 -> interior / first C channels of the framed f16 / bf16 buffer `out` (B, H + 2, W + 2, C' >= C)"""
    B, H, W, Cc = x_nhwc.shape
    fn, name = _half_entry("mv3d_frame_nhwc", out.dtype)
    check(fn(_ptr(x_nhwc), _ptr(out), B, H, W, Cc, out.shape[3], _stream()), name)
    return out


def conv3x3_f16(x_framed, w_packed, bias, out=None, out_framed=True, out_f32=False, relu=True):
    """x_framed (B, H + 2, W + 2, Cin) f16 / bf16, w_packed (Cout, 9 Cin) same type, bias (Cout) f32 -> framed map of that type
    (default), or the bare (B, H, W, Cout) map in that type / f32."""
    B, Hp, Wp, cin = x_framed.shape
    H, W, cout = Hp - 2, Wp - 2, w_packed.shape[0]
    if w_packed.dtype != x_framed.dtype:
        raise TypeError("activations %s, weights %s" % (x_framed.dtype, w_packed.dtype))
    fn, name = _half_entry("mv3d_conv3x3", x_framed.dtype)
    f32 = x_framed.dtype == torch.float32
    if f32:
        out_f32 = True                                            # f32 maps in, f32 maps out
    if out is None:
        if out_framed:
            out = framed_buffer(B, H, W, cout, x_framed.device, x_framed.dtype)
        else:
            out = torch.empty((B, H, W, cout), dtype=torch.float32 if out_f32 else x_framed.dtype, device=x_framed.device)
    # the kernel addresses each buffer with 32-bit offsets: frames are independent, so a larger batch goes in chunks
    per_frame = max(Hp * Wp * cin * x_framed.element_size(), out[0].numel() * out.element_size())
    step = max(1, min(B, (2 ** 31 - 1) // per_frame))
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        if f32:
            check(fn(_ptr(x_framed[b0:b0 + nb]), _ptr(w_packed), _ptr(bias), _ptr(out[b0:b0 + nb]), nb, H, W, cin, cout, int(out_framed), int(relu),
                     _stream()), name)
        else:
            check(fn(_ptr(x_framed[b0:b0 + nb]), _ptr(w_packed), _ptr(bias), _ptr(out[b0:b0 + nb]), nb, H, W, cin, cout, int(out_framed),
                     int(out_f32), int(relu), _stream()), name)
    return out


def maxpool2x2_f16(x_framed, out=None):
    B, Hp, Wp, Cc = x_framed.shape
    H, W = Hp - 2, Wp - 2
    if out is None:
        out = framed_buffer(B, H // 2, W // 2, Cc, x_framed.device, x_framed.dtype)
    fn, name = _half_entry("mv3d_maxpool2x2", x_framed.dtype)
    check(fn(_ptr(x_framed), _ptr(out), B, H, W, Cc, _stream()), name)
    return out



def maxpool2x2_bwd_bf16(y_framed, g_pooled_framed, out):
    """gradient of ReLU + 2x2 max pool into the zero-initialised framed buffer `out` (same shape / type as y_framed: bf16 or f32)"""
    B, Hp, Wp, Cc = y_framed.shape
    if y_framed.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("bfloat16 or float32 maps expected")
    fn, name = _half_entry("mv3d_maxpool2x2_bwd", y_framed.dtype)
    check(fn(_ptr(y_framed), _ptr(g_pooled_framed), _ptr(out), B, Hp - 2, Wp - 2, Cc, _stream()), name)
    return out


_WGRAD_CHUNK_BYTES = 2 ** 31 - 512          # what one weight-gradient launch may address per map


def conv3x3_wgrad_bf16(x_framed, dy_framed, c_in_real=None, want_bias=False):
    """x_framed (B, H + 2, W + 2, Cin), dy_framed (B, H + 2, W + 2, Cout) with a zero frame, both bf16 or both f32 -> the filter
    gradient (Cout, c_in_real, 3, 3) f32 (c_in_real <= Cin: the input layer's padding channels are dropped) [, the bias gradient
    (Cout) f32]"""
    B, Hp, Wp, cin = x_framed.shape
    cout = dy_framed.shape[3]
    if x_framed.dtype != dy_framed.dtype or x_framed.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("bfloat16 or float32 maps of one type expected, got %s / %s" % (x_framed.dtype, dy_framed.dtype))
    f32 = x_framed.dtype == torch.float32
    ws_fn = lib().mv3d_conv3x3_wgrad_f32_workspace_bytes if f32 else lib().mv3d_conv3x3_wgrad_workspace_bytes
    fn, name = (lib().mv3d_conv3x3_wgrad_f32, "mv3d_conv3x3_wgrad_f32") if f32 else (lib().mv3d_conv3x3_wgrad_bf16, "mv3d_conv3x3_wgrad_bf16")
    creal = cin if c_in_real is None else int(c_in_real)
    # the kernel addresses each map with 32-bit offsets: the gradient is a sum over the frames, so a larger batch goes in chunks
    per_frame = Hp * Wp * max(cin, cout) * x_framed.element_size()
    step = max(1, _WGRAD_CHUNK_BYTES // per_frame)
    if B > step:
        dw = db = None
        for b0 in range(0, B, step):
            r = conv3x3_wgrad_bf16(x_framed[b0:b0 + step], dy_framed[b0:b0 + step], creal, want_bias=want_bias)
            w_, b_ = r if want_bias else (r, None)
            dw = w_ if dw is None else dw.add_(w_)
            if want_bias:
                db = b_ if db is None else db.add_(b_)
        return (dw, db) if want_bias else dw
    need = ws_fn(B, Hp - 2, Wp - 2, cin, cout)
    if need == 0:
        raise _lib.Mv3dError(_lib.ERR_INVALID_ARG, name + "_workspace_bytes")
    ws = torch.empty(need, dtype=torch.uint8, device=x_framed.device)
    dw = torch.empty((cout, creal, 3, 3), dtype=torch.float32, device=x_framed.device)
    db = torch.empty((cout,), dtype=torch.float32, device=x_framed.device) if want_bias else None
    check(fn(_ptr(x_framed), _ptr(dy_framed), _ptr(dw), _ptr(db), B, Hp - 2, Wp - 2, cin, creal, cout, _ptr(ws), need, _stream()), name)
    return (dw, db) if want_bias else dw


def pack_conv3x3_train_bf16(w_oihw, c_in_pad=None, want_dgrad=True):
    """fp32 (O, I, 3, 3) -> (forward packing (O, 9 * I') bf16, data-gradient packing (I, 9 * O) bf16 | None) in one launch"""
    O, I = w_oihw.shape[:2]
    Ip = c_in_pad or I
    w = w_oihw.detach().contiguous()
    fwd = (torch.zeros if Ip > I else torch.empty)((O, 9 * Ip), dtype=torch.bfloat16, device=w.device)
    dg = torch.empty((I, 9 * O), dtype=torch.bfloat16, device=w.device) if want_dgrad else None
    check(lib().mv3d_conv3x3_pack_bf16(_ptr(w), _ptr(fwd), _ptr(dg), O, I, Ip, _stream()), "mv3d_conv3x3_pack_bf16")
    return fwd, dg


def conv3x3_gated_bf16(x_framed, w_packed, bias, gate_framed, out):
    """(conv3x3(x) + bias) gated by gate > 0 into the framed bf16 buffer `out` (the training trunk's data gradient + ReLU mask)"""
    B, Hp, Wp, cin = x_framed.shape
    cout = w_packed.shape[0]
    check(lib().mv3d_conv3x3_gated_bf16(_ptr(x_framed), _ptr(w_packed), _ptr(bias), _ptr(gate_framed), _ptr(out), B, Hp - 2, Wp - 2, cin, cout,
                                        _stream()), "mv3d_conv3x3_gated_bf16")
    return out


# ------------------------------------------------------------------ several views of one layer shape behind one launch
# (the BEV / image / front-view trunks at one VGG depth: lib/networks/MV3D_train.py:44-81 -- same channel counts, different map
# sizes; at a training batch one view's tiles do not fill the chip, together they do, on one stream)
_OFF32 = 2 ** 31 - 1


def conv3x3_views(views, out_framed=True, out_f32=False, relu=True):
    """views: list of (x_framed, w_packed, bias, gate_framed | None, out); the same (c_in, c_out) and type in every view.
    One launch (mv3d_conv3x3_views_*); `out` is written (framed of the operand type, or bare in that type / f32)."""
    x0, w0 = views[0][0], views[0][1]
    cin, cout, dt = x0.shape[3], w0.shape[0], x0.dtype
    f32 = dt == torch.float32
    big = False
    for x, w, b, g, out in views:
        if x.dtype != dt or w.dtype != dt or x.shape[3] != cin or w.shape[0] != cout:
            raise TypeError("views of one layer shape and type expected")
        big = big or x.numel() * x.element_size() > _OFF32 or out.numel() * out.element_size() > _OFF32
    if big or len(views) > 3:
        # beyond the kernel's 32-bit offsets (or its three view slots): view by view, each in batch chunks that fit, through the
        # one-view form of this same entry -- so the gated (data-gradient) views keep their own type (bf16 or f32: ADVICE r04)
        for x, w, b, g, out in views:
            per_frame = max(x[0].numel() * x.element_size(), out[0].numel() * out.element_size())
            step = _OFF32 // per_frame
            if step < 1:
                raise ValueError("one frame of %d bytes is beyond the convolution kernel's 32-bit offsets" % per_frame)
            for b0 in range(0, x.shape[0], step):
                conv3x3_views([(x[b0:b0 + step], w, b, None if g is None else g[b0:b0 + step], out[b0:b0 + step])],
                              out_framed=out_framed, out_f32=out_f32, relu=relu)
        return [v[4] for v in views]
    arr = (_lib.ConvView * len(views))()
    for k, (x, w, b, g, out) in enumerate(views):
        B, Hp, Wp, _ = x.shape
        arr[k] = _lib.ConvView(x.data_ptr(), w.data_ptr(), b.data_ptr(), g.data_ptr() if g is not None else None, out.data_ptr(),
                               B, Hp - 2, Wp - 2, 0)
    fn, name = _half_entry("mv3d_conv3x3_views", dt)
    if f32:
        check(fn(len(views), arr, cin, cout, int(out_framed), int(relu), _stream()), name)
    else:
        check(fn(len(views), arr, cin, cout, int(out_framed), int(out_f32), int(relu), _stream()), name)
    return [v[4] for v in views]


def conv3x3_pool_views(views):
    """views: list of (x_framed, w_packed, bias, out_pooled_framed): convolution + bias + ReLU + the 2x2 max pool behind it in one
    launch (mv3d_conv3x3_pool_views_*); `out` (B, H / 2 + 2, W / 2 + 2, Cout) is the POOLED framed map."""
    x0, w0 = views[0][0], views[0][1]
    cin, cout, dt = x0.shape[3], w0.shape[0], x0.dtype
    arr = (_lib.ConvView * len(views))()
    for k, (x, w, b, out) in enumerate(views):
        B, Hp, Wp, _ = x.shape
        if x.dtype != dt or w.dtype != dt or x.shape[3] != cin or w.shape[0] != cout or tuple(out.shape) != (B, (Hp - 2) // 2 + 2, (Wp - 2) // 2 + 2, cout):
            raise TypeError("views of one layer shape and type, pooled framed outputs expected")
        if x.numel() * x.element_size() > _OFF32:
            raise ValueError("map beyond the kernel's 32-bit offsets: pool separately")
        arr[k] = _lib.ConvView(x.data_ptr(), w.data_ptr(), b.data_ptr(), None, out.data_ptr(), B, Hp - 2, Wp - 2, 0)
    fn, name = _half_entry("mv3d_conv3x3_pool_views", dt)
    check(fn(len(views), arr, cin, cout, _stream()), name)
    return [v[3] for v in views]


def maxpool2x2_views(views):
    """views: list of (x_framed, out_framed): the 2x2 pools of several maps of one channel count in one launch"""
    arr = (_lib.PoolView * len(views))()
    for k, (x, out) in enumerate(views):
        B, Hp, Wp, _ = x.shape
        arr[k] = _lib.PoolView(x.data_ptr(), None, out.data_ptr(), B, Hp - 2, Wp - 2, 0)
    fn, name = _half_entry("mv3d_maxpool2x2_views", views[0][0].dtype)
    check(fn(len(views), arr, views[0][0].shape[3], _stream()), name)
    return [v[1] for v in views]


def maxpool2x2_bwd_views(views):
    """views: list of (y_framed, g_pooled_framed, out): gradient of ReLU + 2x2 max pool of several maps in one launch"""
    dt = views[0][0].dtype
    if dt not in (torch.bfloat16, torch.float32):
        raise TypeError("bfloat16 or float32 maps expected")
    arr = (_lib.PoolView * len(views))()
    for k, (y, g, out) in enumerate(views):
        B, Hp, Wp, _ = y.shape
        arr[k] = _lib.PoolView(y.data_ptr(), g.data_ptr(), out.data_ptr(), B, Hp - 2, Wp - 2, 0)
    fn, name = _half_entry("mv3d_maxpool2x2_bwd_views", dt)
    check(fn(len(views), arr, views[0][0].shape[3], _stream()), name)
    return [v[2] for v in views]


def conv3x3_wgrad_views(views, c_in_real=None, want_bias=False):
    """views: list of (x_framed, dy_framed) of one layer shape -> [(dw (Cout, c_in_real, 3, 3) f32, db (Cout) f32 | None), ...]:
    one weight-gradient launch + one reduce launch for all of them.  c_in_real: one number, or one per view (the input layers' 9 / 3
    real channels inside their 64-channel buffers)."""
    x0, dy0 = views[0]
    cin, cout, dt = x0.shape[3], dy0.shape[3], x0.dtype
    if dt not in (torch.bfloat16, torch.float32):
        raise TypeError("bfloat16 or float32 maps expected")
    reals = list(c_in_real) if isinstance(c_in_real, (list, tuple)) else [cin if c_in_real is None else int(c_in_real)] * len(views)
    creal = reals[0]
    if len(views) > 3 or any(x.numel() * x.element_size() > _OFF32 - 256 or dy.numel() * dy.element_size() > _OFF32 - 256 for x, dy in views):
        return [conv3x3_wgrad_bf16(x, dy, r, want_bias=True) if want_bias else (conv3x3_wgrad_bf16(x, dy, r), None) for (x, dy), r in zip(views, reals)]
    dev = x0.device
    arr = (_lib.WgradView * len(views))()
    res = []
    for k, (x, dy) in enumerate(views):
        if x.dtype != dt or dy.dtype != dt or x.shape[3] != cin or dy.shape[3] != cout:
            raise TypeError("views of one layer shape and type expected")
        B, Hp, Wp, _ = x.shape
        dw = torch.empty((cout, reals[k], 3, 3), dtype=torch.float32, device=dev)
        db = torch.empty((cout,), dtype=torch.float32, device=dev) if want_bias else None
        arr[k] = _lib.WgradView(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr() if db is not None else None, B, Hp - 2, Wp - 2, reals[k])
        res.append((dw, db))
    f32 = dt == torch.float32
    need = lib().mv3d_conv3x3_wgrad_views_workspace_bytes(len(views), arr, cin, cout, int(f32))
    if need == 0:
        raise _lib.Mv3dError(_lib.ERR_INVALID_ARG, "mv3d_conv3x3_wgrad_views_workspace_bytes")
    ws = _workspace(need, dev, "wgrad")
    fn, name = (lib().mv3d_conv3x3_wgrad_views_f32, "mv3d_conv3x3_wgrad_views_f32") if f32 else \
        (lib().mv3d_conv3x3_wgrad_views_bf16, "mv3d_conv3x3_wgrad_views_bf16")
    check(fn(len(views), arr, cin, creal, cout, _ptr(ws), ws.numel(), _stream()), name)
    return res


def pack_conv3x3_train_many(items, dtype=torch.bfloat16):
    """items: list of (w_oihw f32 (O, I, 3, 3), c_in_pad | None, want_dgrad) -> [(fwd (O, 9 I') of `dtype` (bf16 | f32), dgrad (I, 9 O)
    | None)]: every filter of a training step packed by ONE launch."""
    arr = (_lib.PackItem * len(items))()
    res, keep = [], []
    for k, (w_oihw, c_in_pad, want_dgrad) in enumerate(items):
        O, I = w_oihw.shape[:2]
        Ip = c_in_pad or I
        w = w_oihw.detach().contiguous()
        fwd = (torch.zeros if Ip > I else torch.empty)((O, 9 * Ip), dtype=dtype, device=w.device)
        dg = torch.empty((I, 9 * O), dtype=dtype, device=w.device) if want_dgrad else None
        arr[k] = _lib.PackItem(w.data_ptr(), fwd.data_ptr(), dg.data_ptr() if dg is not None else None, O, I, Ip, 0)
        keep.append(w)
        res.append((fwd, dg))
    fn, name = _half_entry("mv3d_conv3x3_pack_many", dtype)
    check(fn(len(items), arr, _stream()), name)
    return res


pack_conv3x3_train_many_bf16 = pack_conv3x3_train_many


# type-neutral names (the `_f16` / `_bf16` suffixes above are historical: each function picks the C entry by its tensors' dtype)
frame_nhwc = frame_nhwc_f16
conv3x3 = conv3x3_f16
maxpool2x2 = maxpool2x2_f16
maxpool2x2_bwd = maxpool2x2_bwd_bf16
conv3x3_wgrad = conv3x3_wgrad_bf16


# ------------------------------------------------------------------ KITTI evaluation (csrc/kitti_eval.hip, datasets/kitti_eval.py)
class KittiEvalSplit:
    """A split on the device for mv3d_kitti_eval_*: the packed CSR arrays of ONE upload and the C descriptor pointing at them."""

    def __init__(self, det_cnr, det_score, det_off, calib, gt_cnr, gt_off, gt_cls, gt_attr, device, img_height=375):
        det_off = np.ascontiguousarray(det_off, np.int32)
        gt_off = np.ascontiguousarray(gt_off, np.int32)
        F = det_off.size - 1
        D, G = np.diff(det_off).astype(np.int64), np.diff(gt_off).astype(np.int64)
        pair_off = np.concatenate([[0], np.cumsum(D * G)])
        self.num_pairs = int(pair_off[-1])
        if self.num_pairs > np.iinfo(np.int32).max:
            raise ValueError("KITTI evaluation: more than 2^31 - 1 (detection, object) pairs in one split")
        offsets = np.stack([det_off, gt_off, pair_off.astype(np.int32)])
        self.det_off, self.gt_off = det_off, gt_off        # host copies the C-ABI validates (kept alive with the descriptor)
        self.dev = upload_packed([offsets, np.reshape(det_cnr, (-1, 24)), np.reshape(det_score, (-1,)), np.reshape(calib, (F, 4, 12)),
                                  np.reshape(gt_cnr, (-1, 24)), np.asarray(gt_cls, np.int32), np.reshape(gt_attr, (-1, 4))], device)
        self.device = device
        self.F, self.N, self.G = F, int(det_off[-1]), int(gt_off[-1])
        v = self.dev
        self.split = _lib.KittiSplit(F, self.N, self.G, int(img_height), det_off.ctypes.data, gt_off.ctypes.data, v[0].data_ptr(),
                                     v[1].data_ptr(), v[2].data_ptr(), v[3].data_ptr(), v[4].data_ptr(), v[5].data_ptr(),
                                     v[6].data_ptr())


def kitti_eval_overlaps(sp):
    """-> iou (2, P) f64 (bev | 3d, frame f's D x G block at pair_off[f]), det_height (N) f64.  Asynchronous."""
    iou = torch.empty((2, max(sp.num_pairs, 1)), dtype=torch.float64, device=sp.device)
    height = torch.empty((max(sp.N, 1),), dtype=torch.float64, device=sp.device)
    check(lib().mv3d_kitti_eval_overlaps(C.byref(sp.split), sp.num_pairs, _ptr(iou), _ptr(height), _stream()),
          "mv3d_kitti_eval_overlaps")
    return iou[:, :sp.num_pairs], height[:sp.N]


def kitti_eval_match(sp, iou, height, eval_class, neighbor_class, min_overlap):
    """Pass 1 -> matched (2, 3, G) f32: the true-positive score of every object, -inf if none.  Asynchronous."""
    matched = torch.empty((2, 3, max(sp.G, 1)), dtype=torch.float32, device=sp.device)
    check(lib().mv3d_kitti_eval_match(C.byref(sp.split), sp.num_pairs, _ptr(iou.contiguous()), _ptr(height), int(eval_class),
                                      int(neighbor_class), float(min_overlap), _ptr(matched), _stream()), "mv3d_kitti_eval_match")
    return matched[:, :, :sp.G]


def kitti_eval_count(sp, iou, height, eval_class, neighbor_class, min_overlap, thresholds, num_thresholds):
    """Pass 2: thresholds (2, 3, 41) f32 and num_thresholds (2, 3) int32 device tensors -> counts (2, 3, 41, 3) int32
    (tp | fp | fn).  Asynchronous."""
    counts = torch.empty((2, 3, 41, 3), dtype=torch.int32, device=sp.device)
    check(lib().mv3d_kitti_eval_count(C.byref(sp.split), sp.num_pairs, _ptr(iou.contiguous()), _ptr(height), int(eval_class),
                                      int(neighbor_class), float(min_overlap), _ptr(thresholds), _ptr(num_thresholds), _ptr(counts),
                                      _stream()), "mv3d_kitti_eval_count")
    return counts


class KittiImageSplit:
    """The 2D side of a KittiEvalSplit for mv3d_kitti_eval_image_boxes / _match_2d / _count_2d: the label image boxes and
    alphas, the frames' DontCare boxes (CSR dc_off) and image shapes (H, W), in ONE upload, and the C descriptor."""

    def __init__(self, sp, gt_box, gt_alpha, dc_off, dc_box, image_shape):
        dc_off = np.ascontiguousarray(dc_off, np.int32)
        image_shape = np.ascontiguousarray(image_shape, np.int32).reshape(sp.F, 2)
        if dc_off.size != sp.F + 1:
            raise ValueError("KITTI evaluation: dc_off needs num_frames + 1 entries")
        if sp.F and image_shape.min() < 1:
            raise ValueError("KITTI evaluation: image shapes must be positive")
        self.dc_off = dc_off                               # host copy the C-ABI validates (kept alive with the descriptor)
        self.dev = upload_packed([dc_off, np.reshape(gt_box, (-1, 4)), np.reshape(gt_alpha, (-1,)), np.reshape(dc_box, (-1, 4)),
                                  image_shape], sp.device)
        self.K = int(dc_off[-1])
        v = self.dev
        self.image = _lib.KittiImageSplit(self.K, 0, dc_off.ctypes.data, v[0].data_ptr(), v[1].data_ptr(), v[2].data_ptr(),
                                          v[3].data_ptr(), v[4].data_ptr())


def kitti_eval_image_boxes(sp, im):
    """-> det_box (N, 4) f64 clipped image box x1 y1 x2 y2, det_cam (N, 8) f64 camera box h w l x y z ry alpha.  Asynchronous."""
    box = torch.empty((max(sp.N, 1), 4), dtype=torch.float64, device=sp.device)
    cam = torch.empty((max(sp.N, 1), 8), dtype=torch.float64, device=sp.device)
    check(lib().mv3d_kitti_eval_image_boxes(C.byref(sp.split), C.byref(im.image), _ptr(box), _ptr(cam), _stream()),
          "mv3d_kitti_eval_image_boxes")
    return box[:sp.N], cam[:sp.N]


def kitti_eval_match_2d(sp, im, det_box, eval_class, neighbor_class, min_overlap):
    """2D pass 1 -> matched (3, G) f32: the true-positive score of every object, -inf if none.  Asynchronous."""
    matched = torch.empty((3, max(sp.G, 1)), dtype=torch.float32, device=sp.device)
    check(lib().mv3d_kitti_eval_match_2d(C.byref(sp.split), C.byref(im.image), _ptr(det_box.contiguous()), int(eval_class),
                                         int(neighbor_class), float(min_overlap), _ptr(matched), _stream()), "mv3d_kitti_eval_match_2d")
    return matched[:, :sp.G]


def kitti_eval_count_2d(sp, im, det_box, det_cam, eval_class, neighbor_class, min_overlap, thresholds, num_thresholds):
    """2D pass 2: thresholds (3, 41) f32 and num_thresholds (3,) int32 device tensors -> counts (3, 41, 3) int32 (tp | fp | fn
    after the DontCare rule), similarity (F, 3, 41) f64 per-frame orientation similarity sums.  Asynchronous."""
    counts = torch.empty((3, 41, 3), dtype=torch.int32, device=sp.device)
    sim = torch.empty((max(sp.F, 1), 3, 41), dtype=torch.float64, device=sp.device)
    check(lib().mv3d_kitti_eval_count_2d(C.byref(sp.split), C.byref(im.image), _ptr(det_box.contiguous()), _ptr(det_cam.contiguous()),
                                         int(eval_class), int(neighbor_class), float(min_overlap), _ptr(thresholds),
                                         _ptr(num_thresholds), _ptr(counts), _ptr(sim), _stream()), "mv3d_kitti_eval_count_2d")
    return counts, sim[:sp.F]


# ------------------------------------------------------------------ proposal recall (csrc/proposal_recall.hip, datasets/proposal_recall.py)
def _exact_f32(a, what):
    """numpy array / tensor -> the same values in f32; another dtype only where the conversion loses nothing."""
    if isinstance(a, torch.Tensor):
        if a.dtype == torch.float32:
            return a
        b = a.to(torch.float32)
        same = (b.to(a.dtype) == a) | ((a != a) if a.dtype.is_floating_point else torch.zeros_like(b, dtype=torch.bool))
        if not bool(same.all()):
            raise ValueError(f"proposal recall: {what} of dtype {a.dtype} are not exactly representable in float32")
        return b
    a = np.asarray(a)
    if a.dtype == np.float32:
        return a
    if a.dtype.kind not in "fiub":
        raise ValueError(f"proposal recall: {what} of dtype {a.dtype}")
    b = a.astype(np.float32)
    if not np.array_equal(b.astype(a.dtype), a, equal_nan=a.dtype.kind == "f"):
        raise ValueError(f"proposal recall: {what} of dtype {a.dtype} are not exactly representable in float32")
    return b


def _recall_boxes(a, what):
    """(N, 4) f32 boxes from (N, 4) or (N, 5) rows (a `rois` blob carries the batch index in front)"""
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
    if a.ndim != 2 and a.shape[0] == 0:
        a = a.reshape(0, 4)
    if a.ndim != 2 or a.shape[1] not in (4, 5):
        raise ValueError(f"proposal recall: {what} must be (N, 4) or (N, 5), got {tuple(a.shape)}")
    return _exact_f32(a[:, 1:5] if a.shape[1] == 5 else a, what)


class _RecallSplitBase:
    """What RecallSplit and Recall3dSplit share: the offset checks, the int32 host copies of the offsets that the C-ABI
    validates, ONE packed upload of everything that comes from the host, and device tensors picked up as they are.  A subclass
    sets `what` (the prefix of its messages) and `_parse(boxes, gt) -> (boxes, gt)` f32; `_offsets` names the offset arrays."""
    what = None

    def __init__(self, boxes, box_off, gt, gt_off, device):
        box_off = np.ascontiguousarray(box_off, np.int64)
        gt_off = np.ascontiguousarray(gt_off, np.int64)
        if box_off.ndim != 1 or box_off.size < 1 or box_off.shape != gt_off.shape:
            raise ValueError(f"{self.what}: box_off and gt_off need num_frames + 1 entries each")
        offs = self._offsets(box_off, gt_off)
        boxes, gt = self._parse(boxes, gt)
        if boxes.shape[0] != box_off[-1] or gt.shape[0] != gt_off[-1]:
            raise ValueError(f"{self.what}: the offsets do not end at the number of boxes / objects")
        self.device = device
        self.F, self.N, self.G = box_off.size - 1, int(box_off[-1]), int(gt_off[-1])
        names = list(offs)
        for k in names:
            setattr(self, k, offs[k].astype(np.int32))          # host copies the C-ABI validates
        up = list(upload_packed([getattr(self, k) for k in names] + [a for a in (boxes, gt) if not isinstance(a, torch.Tensor)], device))
        for k in names:
            setattr(self, k + "_dev", up.pop(0))
        self.boxes, self.gt = (a.to(device).contiguous() if isinstance(a, torch.Tensor) else up.pop(0) for a in (boxes, gt))

    def _offsets(self, box_off, gt_off):
        if box_off[-1] > np.iinfo(np.int32).max:
            raise ValueError(f"{self.what}: more than 2^31 - 1 boxes in one split")
        return {"box_off": box_off, "gt_off": gt_off}


class RecallSplit(_RecallSplitBase):
    """A split on the device for mv3d_proposal_recall: frame f owns boxes box_off[f] .. box_off[f+1]-1 and objects gt_off[f] ..
    gt_off[f+1]-1.  boxes / gt: numpy arrays or device tensors, f32 (another dtype only if it converts exactly), boxes with or
    without the leading batch column of a `rois` blob.  Everything that comes from the host goes up in ONE packed upload."""
    what = "proposal recall"

    def _parse(self, boxes, gt):
        return _recall_boxes(boxes, "boxes"), _recall_boxes(gt, "objects")


def recall_limits(limits):
    """limits of evaluate_recall -> int32 array for the device, None -> 0 ("all of the frame's boxes")"""
    out = []
    for v in limits:
        if v is not None and (int(v) != v or int(v) < 1):
            raise ValueError(f"proposal recall: a limit is None or an integer >= 1, got {v!r}")
        out.append(0 if v is None else int(v))
    if not out:
        raise ValueError("proposal recall: no limit given")
    return np.array(out, np.int32)


def default_recall_thresholds():
    return np.arange(0.5, 0.95 + 1e-5, 0.05)              # lib/datasets/imdb.py:199-201


class _RecallOut(tuple):
    pack = None                                             # the one buffer the three tensors are views of
    keep = None


def _recall_prepare(what, split, limits, thresholds, on_short, planes):
    """-> (limits, thresholds on the device, short_mode, result): the packed (gt_overlaps, counts, status) of `planes` metric
    planes (1: (L, G) / (L, T); 2: (2, L, G) / (2, L, T)); `.keep` holds what a descriptor points to"""
    if on_short not in ('raise', 'zero'):
        raise ValueError(f"{what}: on_short is 'raise' or 'zero'")
    lim = recall_limits(limits)
    thr = np.ascontiguousarray(default_recall_thresholds() if thresholds is None else thresholds, np.float64).reshape(-1)
    L, T, dev = lim.size, thr.size, split.device
    d_lim = torch.from_numpy(lim).to(dev)
    d_thr = torch.from_numpy(thr).to(dev) if T else None
    lead = () if planes == 1 else (planes,)
    nb = [8 * planes * L * split.G, 4 * planes * L * T, 4 * split.F]
    pack = torch.empty((max(sum(nb), 8),), dtype=torch.uint8, device=dev)
    out = _RecallOut((pack[:nb[0]].view(torch.float64).view(*lead, L, split.G),
                      pack[nb[0]:nb[0] + nb[1]].view(torch.int32).view(*lead, L, T), pack[nb[0] + nb[1]:sum(nb)].view(torch.int32)))
    out.pack, out.keep = pack, (split, d_lim, d_thr)
    return d_lim, d_thr, 1 if on_short == 'zero' else 0, out


def proposal_recall(split, limits=(None,), thresholds=None, on_short='raise'):
    """-> (gt_overlaps (L, G) f64, counts (L, T) int32, status (F) int32), device tensors: the greedy matching of
    lib/datasets/imdb.py:162-196 for every frame and every limit in one launch (csrc/proposal_recall.hip).  on_short: frames with
    fewer boxes than objects, 'raise' = the reference's failing assert (status bit MV3D_RECALL_STATUS_SHORT, see
    `proposal_recall_host`), 'zero' = this library's definition, NOT the reference's: the objects left over record 0.0.
    Asynchronous."""
    d_lim, d_thr, mode, out = _recall_prepare("proposal recall", split, limits, thresholds, on_short, 1)
    ov, counts, status = out
    T = counts.shape[-1]
    desc = _lib.RecallSplit(split.F, split.G, d_lim.numel(), T, mode, 0, split.N, split.box_off.ctypes.data,
                            split.gt_off.ctypes.data, split.box_off_dev.data_ptr(), split.gt_off_dev.data_ptr(),
                            split.boxes.data_ptr() if split.N else None, split.gt.data_ptr() if split.G else None, d_lim.data_ptr(),
                            d_thr.data_ptr() if T else None)
    check(lib().mv3d_proposal_recall(C.byref(desc), _ptr(ov) if split.G else None, _ptr(counts) if T else None,
                                     _ptr(status) if split.F else None, _stream()), "mv3d_proposal_recall")
    return out


def proposal_recall_host(out):
    """The ONE read-back of proposal_recall's result -> numpy (gt_overlaps, counts, status).  Raises AssertionError if a frame
    had fewer boxes than objects under on_short='raise' (the reference's `assert(gt_ovr >= 0)`, imdb.py:186) and ValueError if
    a frame holds a non-finite coordinate."""
    ov, counts, status = out
    pack = getattr(out, "pack", None)
    if pack is None:
        h_ov, h_counts, h_status = ov.cpu().numpy(), counts.cpu().numpy(), status.cpu().numpy()
    else:
        host = pack.cpu().numpy()
        n0, n1 = 8 * ov.numel(), 4 * counts.numel()
        h_ov = host[:n0].view(np.float64).reshape(ov.shape)
        h_counts = host[n0:n0 + n1].view(np.int32).reshape(counts.shape)
        h_status = host[n0 + n1:n0 + n1 + 4 * status.numel()].view(np.int32)
    bad = np.flatnonzero(h_status & 2)
    if bad.size:
        raise ValueError(f"proposal recall: non-finite box or object coordinate in frame {int(bad[0])} ({bad.size} frames)")
    short = np.flatnonzero(h_status & 1)
    if short.size:
        raise AssertionError(f"proposal recall: frame {int(short[0])} has fewer boxes than objects ({short.size} frames): "
                             "lib/datasets/imdb.py:186 assert(gt_ovr >= 0); on_short='zero' counts the objects left over as misses")
    return h_ov, h_counts, h_status


# ------------------------------------------------------------------ proposal recall by oriented IoU (csrc/proposal_recall_3d.hip, datasets/proposal_recall_3d.py)
RECALL3D_METRICS = ('bev', '3d')                           # the planes of gt_overlaps / counts, in this order


def _recall3d_boxes(a, what):
    """(N, 6) x y z l w h (from (N, 6) or the (N, 7) rows of a `rois` blob with the batch index in front) or (N, 24) corners,
    f32 -> (array, format)"""
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
    if a.ndim != 2 and a.shape[0] == 0:
        a = a.reshape(0, 6)
    if a.ndim != 2 or a.shape[1] not in (6, 7, 24):
        raise ValueError(f"proposal recall 3d: {what} must be (N, 6), (N, 7) or (N, 24), got {tuple(a.shape)}")
    return _exact_f32(a[:, 1:7] if a.shape[1] == 7 else a, what), (1 if a.shape[1] == 24 else 0)


class Recall3dSplit(_RecallSplitBase):
    """A split on the device for mv3d_proposal_recall_3d: frame f owns proposals box_off[f] .. box_off[f+1]-1 and objects gt_off[f]
    .. gt_off[f+1]-1.  boxes: (N, 6) x y z l w h, (N, 7) with the batch column in front, or (N, 24) corners; gt: (G, 24) LIDAR
    corners; numpy arrays or device tensors, f32 (another dtype only if it converts exactly).  Everything that comes from the
    host goes up in ONE packed upload."""
    what = "proposal recall 3d"

    def _offsets(self, box_off, gt_off):
        pair_off = np.concatenate([[0], np.cumsum(np.diff(box_off) * np.diff(gt_off))]).astype(np.int64)
        if box_off[-1] > np.iinfo(np.int32).max or pair_off[-1] > np.iinfo(np.int32).max:
            raise ValueError("proposal recall 3d: more than 2^31 - 1 boxes or (box, object) pairs in one split")
        self.P = int(pair_off[-1])
        return {"box_off": box_off, "gt_off": gt_off, "pair_off": pair_off}

    def _parse(self, boxes, gt):
        boxes, self.box_format = _recall3d_boxes(boxes, "boxes")
        if not isinstance(gt, torch.Tensor):
            gt = np.asarray(gt)
        if gt.ndim != 2 and gt.shape[0] == 0:
            gt = gt.reshape(0, 24)
        if gt.ndim != 2 or gt.shape[1] != 24:
            raise ValueError(f"proposal recall 3d: objects must be (G, 24) corners, got {tuple(gt.shape)}")
        return boxes, _exact_f32(gt, "objects")


def proposal_recall_3d_workspace_bytes(num_pairs):
    return int(lib().mv3d_proposal_recall_3d_workspace_bytes(int(num_pairs)))


def recall3d_prepare(split, limits=(None,), thresholds=None, on_short='raise'):
    """-> (descriptor, workspace, result): the mv3d_recall3d_split of one call, its IoU workspace and the packed result tensors
    (gt_overlaps, counts, status; `.keep` holds the small device arrays the descriptor points to)"""
    d_lim, d_thr, mode, out = _recall_prepare("proposal recall 3d", split, limits, thresholds, on_short, 2)
    T = out[1].shape[-1]
    ws = torch.empty((max(proposal_recall_3d_workspace_bytes(split.P) // 8, 1),), dtype=torch.float64, device=split.device)
    desc = _lib.Recall3dSplit(split.F, split.G, d_lim.numel(), T, mode, split.box_format, split.N, split.P,
                              split.box_off.ctypes.data, split.gt_off.ctypes.data, split.pair_off.ctypes.data,
                              split.box_off_dev.data_ptr(), split.gt_off_dev.data_ptr(), split.pair_off_dev.data_ptr(),
                              split.boxes.data_ptr() if split.N else None, split.gt.data_ptr() if split.G else None, d_lim.data_ptr(),
                              d_thr.data_ptr() if T else None)
    return desc, ws, out


def proposal_recall_3d(split, limits=(None,), thresholds=None, on_short='raise'):
    """-> (gt_overlaps (2, L, G) f64, counts (2, L, T) int32, status (F) int32), device tensors, metric 0 = BEV IoU, 1 = 3D IoU
    (RECALL3D_METRICS): the greedy matching of lib/datasets/imdb.py:162-196 by oriented-box overlap for every frame, every limit
    and both metrics (csrc/proposal_recall_3d.hip).  on_short as in `proposal_recall`.  Asynchronous."""
    desc, ws, out = recall3d_prepare(split, limits, thresholds, on_short)
    ov, counts, status = out
    check(lib().mv3d_proposal_recall_3d(C.byref(desc), _ptr(ws) if split.P else None, _ptr(ov) if split.G else None,
                                        _ptr(counts) if counts.numel() else None, _ptr(status) if split.F else None, _stream()),
          "mv3d_proposal_recall_3d")
    return out


def proposal_recall_3d_host(out):
    """The ONE read-back of proposal_recall_3d's result -> numpy (gt_overlaps (2, L, G), counts (2, L, T), status (F)); raises as
    `proposal_recall_host` does."""
    return proposal_recall_host(out)
