"""Test-time entry points that end in FINAL detections on the device: the per-frame tail of test_net (lib/fast_rcnn/test_mv.py:420-444,
491-501: score cut at 0.05, NMS at cfg.TEST.NMS, cap of max_per_image) runs as ops.detect_post for a whole batch, so a batch costs one
small read-back instead of a host round trip per frame and class.

`ServeGraph(net, feed, warmup=2, post=None)`: fast_rcnn.test_mv.ServeGraph with `post=dict(max_per_image=...)` capturing ops.detect_post
behind the box tail in the same graph; `final_detections()` returns the lists.  post=None captures exactly test_mv.ServeGraph's graph.
`test_net(...)`: fast_rcnn.test_mv.test_net with the key cfg.TEST.BATCH_SIZE: 1 (the default) calls test_mv.test_net itself; n > 1
serves up to n consecutive frames of equal image / BEV shapes per forward and finishes them on the device.
cfg.TEST.NMS_ORIENTED (or `post=dict(..., oriented=True, footprint='regressed' | 'proposal')`) swaps the tail for
ops.detect_post_oriented: the same cut, order and cap with the NMS judged by the IoU of the oriented BEV footprints; with the
'regressed' footprint the corner lists carry the regressed corners, the boxes the NMS judged.  The key sends test_net down the
device route whatever BATCH_SIZE is.  The frame-by-frame loop has no oriented NMS: with the key on test_mv.test_net
raises ValueError where it asks for its output directory (config.get_output_dir), before it loads a frame.
fast_rcnn.test_mv keeps the reference's frame-by-frame entry points as they are: they feed two views.  The third view's input enters
here: `box_detect(sess, net, im, bv, calib, boxes=None, fv=None)` is test_mv.box_detect with the frame's (64,512,3) front-view map fed
as `lidar_fv_data`, and `test_net` rasterises the frames' Velodyne scans for a three-view network (`front_view_source`), which sends it
down the device route whatever BATCH_SIZE is.
The loops over an imdb (`test_net` here, rpn_msr.generate.imdb_proposals) share their pieces: `loop_scan_source` says whether the
frames' scans are needed, `iter_loaded_groups` loads and groups the frames, `group_feed` builds a group's feed (`image_feed`,
`scan_feed`) and `forward_fixed_rois` runs it; `launch_post` and `post_lists` are the tail of `test_net` and of `ServeGraph`."""
import time

import numpy as np
import torch

from .. import ops
from . import loop_parts, test_mv
from .config import cfg, get_output_dir
from ..networks.mv3d import n_classes


def post_settings(post):
    """a copy of `post` = dict(max_per_image=...) with `oriented` (default: cfg.TEST.NMS_ORIENTED) and `footprint` (default:
    cfg.TEST.NMS_ORIENTED_BOXES) filled in: what `launch_post` and `post_lists` read"""
    post = dict(post)
    post.setdefault("oriented", bool(cfg.TEST.get("NMS_ORIENTED", False)))
    post.setdefault("footprint", cfg.TEST.get("NMS_ORIENTED_BOXES", "regressed"))
    return post


def launch_post(post, cls_prob, pred_bv, corners, pred_cnr_r, num_rois, cap, K, plain_cnr_r=False, out=None, workspace=None):
    """the device tail `post` asks for behind a box tail: ops.detect_post_oriented, or ops.detect_post, which gets the regressed
    corners (and fills det_cnr_r) only with plain_cnr_r; asynchronous -> the tail's six-tuple"""
    mpi = int(post.get("max_per_image", 300))
    if post["oriented"]:
        return ops.detect_post_oriented(cls_prob, pred_bv, corners, pred_cnr_r, num_rois, cap, K, mpi, cfg.TEST.NMS,
                                        strict_gt=bool(cfg.USE_GPU_NMS), footprint=post["footprint"], out=out, workspace=workspace)
    return ops.detect_post(cls_prob, pred_bv, corners, pred_cnr_r if plain_cnr_r else None, num_rois, cap, K, mpi, cfg.TEST.NMS, out=out)


def post_lists(post, out):
    """the ONE read-back behind `launch_post`: per frame (dets, dets_cnr) exactly as class_detections + limit_detections return them
    (dets[0] == [], class j (N,5) / (N,25) f32).  Oriented NMS on the 'regressed' footprint: dets_cnr holds the regressed corners
    of the kept rows (the boxes the NMS judged)"""
    if post["oriented"] and post["footprint"] == "regressed":
        return [(dets, cnr_r) for dets, _, cnr_r in ops.detect_post_lists(out, with_cnr_r=True)]
    return ops.detect_post_lists(out)


class ServeGraph(test_mv.ServeGraph):
    """test_mv.ServeGraph whose captured step, with `post=dict(max_per_image=...)`, ends in ops.detect_post: the replay's outputs gain
    out["post"] = (det_bv, det_cnr, det_cnr_r, det_row, det_count, status), static tensors like the others.  `oriented` (default:
    cfg.TEST.NMS_ORIENTED) captures ops.detect_post_oriented with `footprint` (default: cfg.TEST.NMS_ORIENTED_BOXES) instead."""

    def __init__(self, net, feed, warmup=2, post=None):
        self.post = None if post is None else post_settings(post)
        self._post_out = self._post_ws = None
        super().__init__(net, feed, warmup)

    def _step(self):
        out = super()._step()
        if self.post is not None:
            cap = int(out["rois_per_frame"])
            if self._post_out is None:                          # (the graph's static outputs: allocated once, before the capture)
                B, dev = int(out["corners"].shape[0]) // cap, out["corners"].device
                self._post_out = ops.detect_post_outputs(B, n_classes, cap, dev)
                if self.post["oriented"]:
                    self._post_ws = ops.detect_post_oriented_workspace(B, n_classes, cap, dev)
            out["post"] = launch_post(self.post, out["cls_prob"], out["pred_bv"], out["corners"], out["pred_corners_r"], out["num_rois"],
                                      cap, n_classes, plain_cnr_r=True, out=self._post_out, workspace=self._post_ws)
        return out

    def final_detections(self):
        """after a replay of a graph built with `post`: `post_lists` of the tail that ran inside the graph; the ONE host round trip
        is the counts, the status words and the rows in front of the counts"""
        if self.post is None:
            raise ValueError("final_detections() needs ServeGraph(..., post=dict(max_per_image=...))")
        self.stream.synchronize()
        if int(self.out["status"].max().item()) & 1:
            raise ZeroDivisionError("float division")
        return post_lists(self.post, self.out["post"])


def front_view_source(net, imdb):
    """None for a two-view network; for a three-view one (net.views == 3) the function i -> (P,4) f32 scan of frame i that its
    `lidar_fv_data` is rasterised from: imdb.points_at(i) if the imdb has it, else the file imdb.velodyne_path_at(i) names.  An imdb
    with neither raises ValueError here, before a loop loads its first frame."""
    return scan_source(imdb, "a three-view network (`lidar_fv_data`)") if getattr(net, "views", 2) == 3 else None


def scan_source(imdb, needed_by):
    """The loops' one source of scans, for any network: the function i -> (P,4) f32 scan of frame i, imdb.points_at(i) if the imdb
    has it, else the file imdb.velodyne_path_at(i) names.  An imdb with neither raises ValueError here, before a loop loads its first frame;
    `needed_by` says in that message what asked for the scans."""
    if hasattr(imdb, "points_at"):
        return lambda i: np.ascontiguousarray(np.asarray(imdb.points_at(i), np.float32)[:, :4])
    if hasattr(imdb, "velodyne_path_at"):
        from ..utils.read_lidar import load_velodyne
        return lambda i: load_velodyne(imdb.velodyne_path_at(i))
    raise ValueError("{} needs the frames' Velodyne scans: the imdb has neither points_at(i) nor velodyne_path_at(i)".format(needed_by))


def loop_scan_source(net, imdb):
    """(i -> scan or None, maps_from_scans) for a detection loop: a three-view network needs the scans for `lidar_fv_data`,
    cfg.LIDAR_BV_FROM_SCAN for `lidar_bv_data` of any network; None when neither asks"""
    ops.bev_encoding()                                      # 'paper' without LIDAR_BV_FROM_SCAN, or an unknown value: ValueError here
    ops.scan_crop()                                         # cfg.LIDAR_CROP_TO_IMAGE without LIDAR_BV_FROM_SCAN: ValueError here
    from_scan = bool(cfg.LIDAR_BV_FROM_SCAN)
    points_of = front_view_source(net, imdb)
    return (scan_source(imdb, "cfg.LIDAR_BV_FROM_SCAN") if points_of is None and from_scan else points_of), from_scan


def scan_feed(clouds, bev, fv, calibs=None, image_shapes=None):
    """the feed entries a group of frames gets from its scans: the clouds are concatenated and uploaded ONCE, and `lidar_bv_data`
    (bev true: one ops.scan_bev call, the raster cfg.LIDAR_BV_ENCODING names) and `lidar_fv_data` (fv true: one ops.point_cloud_2_front call) are rasterised
    from that one device tensor.  Under cfg.LIDAR_CROP_TO_IMAGE that tensor is first cropped ONCE (ops.scan_crop_to_image) to the points
    each frame's table of `calibs` puts inside its own image, `image_shapes` = the frames' (h, w, ...), and both rasters read the crop."""
    feed = {}
    if bev or fv:
        pts = ops._dev(np.concatenate(clouds, 0))
        offsets = np.cumsum([0] + [len(c) for c in clouds])
        if ops.scan_crop():
            pts, offsets = ops.scan_crop_to_image(pts, offsets, calibs, image_shapes)
        if bev:
            feed["lidar_bv_data"] = ops.scan_bev(pts, offsets=offsets)
        if fv:
            feed["lidar_fv_data"] = ops.point_cloud_2_front(pts, offsets=offsets)
    return feed


def image_feed(ims, out=None):
    """`image_data` of a group of frames on the device (cfg.IMAGE_BLOB_ON_DEVICE): the (h, w, 3) uint8 BGR images are packed into ONE
    byte buffer, uploaded ONCE, and ONE ops.image_blob call subtracts cfg.PIXEL_MEANS and pads every frame at the top-left corner of a
    zero canvas (lib/utils/blob.py:14-27, im_list_to_blob) -> (B, H, W, 3) f32.  The canvas is cfg.IMAGE_CANVAS, or else the group's
    maximal height and width; with equally shaped frames and no fixed canvas the result is bit for bit the host expression's blob.
    out = a contiguous (B, H, W, 3) f32 device tensor to write into; its H and W are then the canvas.  That is the way into a captured
    ServeGraph, whose image shape is fixed: `image_feed(ims, out=graph.static["image_data"])` under `with torch.cuda.stream(graph.stream):`
    (the stream the replay runs on) in front of `graph.replay()` serves frames of any size up to the captured one.  TypeError for an image that is not a uint8 array, ValueError for one that is not (h, w, 3)
    or is larger than the canvas, before anything is uploaded."""
    canvas = cfg.IMAGE_CANVAS if out is None else tuple(out.shape[1:3])
    return ops.image_blob(list(ims), canvas=canvas, out=out)


def _image_key(im):
    """what a frame's image adds to its group key: its shape, or nothing under cfg.IMAGE_BLOB_ON_DEVICE (frames are padded to the
    group's canvas, `image_feed`, so a change of image shape no longer ends a group)"""
    return None if cfg.IMAGE_BLOB_ON_DEVICE else np.shape(im)


def host_image_blob(ims):
    """the (B, H, W, 3) f32 blob of equally shaped frames as the host builds it (lib/fast_rcnn/test_mv.py:162 per frame)"""
    return np.stack([(np.asarray(im, np.float64) - cfg.PIXEL_MEANS).astype(np.float32) for im in ims])


class _FeedsFrontView:
    """a network whose forward adds one frame's `lidar_fv_data` to the feed (what box_detect hands test_mv.box_detect, whose feed has
    two views)"""

    def __init__(self, net, fv):
        self.net, self.fv = net, fv

    def forward(self, feed):
        return self.net.forward(dict(feed, lidar_fv_data=self.fv))


def box_detect(sess, net, im, bv, calib, boxes=None, fv=None):
    """test_mv.box_detect (lib/fast_rcnn/test_mv.py:149-264) with `fv` (not in the reference), the frame's (64,512,3) front-view map
    as numpy or a device tensor (ops.point_cloud_2_front), fed as `lidar_fv_data`.  A three-view network needs it: ValueError without.
    fv=None on a two-view network is test_mv.box_detect itself."""
    if fv is None:
        if getattr(net, "views", 2) == 3:
            raise ValueError("a three-view network needs `lidar_fv_data`: pass fv=, the frame's (64, 512, 3) front-view map "
                             "(ops.point_cloud_2_front)")
        return test_mv.box_detect(sess, net, im, bv, calib, boxes)
    fv = fv.reshape((1,) + ops.FV_SHAPE) if isinstance(fv, torch.Tensor) else np.asarray(fv, np.float32).reshape((1,) + ops.FV_SHAPE)
    return test_mv.box_detect(sess, _FeedsFrontView(net, fv), im, bv, calib, boxes)


def iter_frame_groups(keys, batch_size):
    """Groups of CONSECUTIVE frame indices whose keys (the frames' image and BEV shapes) are equal, at most `batch_size` per group:
    frames are never padded or reordered, a change of shape just ends the group.  Lazy: `keys` may load the frames as it goes."""
    group, group_key = [], None
    for i, key in enumerate(keys):
        if group and (key != group_key or len(group) >= batch_size):
            yield group
            group = []
        group.append(i)
        group_key = key
    if group:
        yield group


def group_frames(keys, batch_size):
    return list(iter_frame_groups(keys, batch_size))


def iter_loaded_groups(imdb, points_of, from_scan, batch_size):
    """(group, (ims, bvs, calibs, clouds)) for every group of `iter_frame_groups` over the imdb's frames, whose key is `_image_key`
    of the image and the BEV shape (ops.BEV_SHAPE under from_scan, where `loop_parts.load_frame` opens no stored map).  Lazy: a frame
    (and its scan, points_of(i), if a source is given) is loaded when its key is asked for and let go of when its group is handed out"""
    pending = {}

    def keys():
        for i in range(len(imdb.image_index)):
            pending[i] = loop_parts.load_frame(imdb, i, not from_scan) + ((None if points_of is None else points_of(i)),)
            yield (_image_key(pending[i][0]), ops.BEV_SHAPE if from_scan else np.shape(pending[i][1]))

    for group in iter_frame_groups(keys(), batch_size):
        yield group, tuple(zip(*(pending.pop(i) for i in group)))


def group_feed(net, ims, bvs, calibs, clouds, from_scan):
    """the feed of one group of frames: `image_data` from `image_feed` (cfg.IMAGE_BLOB_ON_DEVICE) or `host_image_blob`, `lidar_bv_data`
    stacked from the stored maps or, under from_scan, rasterised with a three-view network's `lidar_fv_data` by `scan_feed` (the
    group's scans back to back: one upload, one call per view; under cfg.LIDAR_CROP_TO_IMAGE cropped with the group's tables and the
    frames' OWN image shapes, not the padded canvas), `calib`, and `im_info` = the BEV size, scale 1, per frame"""
    feed = {"image_data": image_feed(ims) if cfg.IMAGE_BLOB_ON_DEVICE else host_image_blob(ims),
            "calib": np.stack([np.asarray(c, np.float32).reshape(4, 12) for c in calibs]), "keep_prob": 1.0}
    if not from_scan:
        feed["lidar_bv_data"] = np.stack([np.asarray(bv, np.float32) for bv in bvs])
    feed.update(scan_feed(clouds, from_scan, getattr(net, "views", 2) == 3, calibs, [np.shape(im) for im in ims]))
    feed["im_info"] = np.array([[feed["lidar_bv_data"].shape[1], feed["lidar_bv_data"].shape[2], 1]] * len(ims), dtype=np.float32)
    return feed


def forward_fixed_rois(net, feed):
    """net.forward(feed) without gradients and with fixed ROI rows per frame (every frame owns `rois_per_frame` rows)"""
    net.fixed_rois = True
    try:
        with torch.no_grad():
            return net.forward(feed)
    finally:
        net.fixed_rois = False


def test_net(sess, net, imdb, weights_filename, max_per_image=300, thresh=0.05, vis=False):
    """test_mv.test_net with cfg.TEST.BATCH_SIZE (not in the reference).  1: test_mv.test_net, untouched.  n > 1: one eager forward
    with fixed ROI rows per group of equally shaped consecutive frames (`iter_loaded_groups`, `group_feed`), the box tail and
    `launch_post` on the device, ONE read-back of the final detections per group (`post_lists`).  A three-view network,
    cfg.LIDAR_BV_FROM_SCAN, cfg.TEST.NMS_ORIENTED and cfg.IMAGE_BLOB_ON_DEVICE each select the device route for any BATCH_SIZE.
    Pickles, the `im_detect: i/n` line (per frame, times averaged over the group) and the evaluate_detections call are
    test_mv.test_net's."""
    batch_size = int(cfg.TEST.get("BATCH_SIZE", 1))
    post = post_settings(dict(max_per_image=max_per_image))
    points_of, from_scan = loop_scan_source(net, imdb)
    if batch_size <= 1 and not post["oriented"] and points_of is None and not cfg.IMAGE_BLOB_ON_DEVICE:
        return test_mv.test_net(sess, net, imdb, weights_filename, max_per_image=max_per_image, thresh=thresh, vis=vis)
    loop_parts.apply_test_precision(net)
    num_images = len(imdb.image_index)
    all_boxes, all_boxes_cnr = loop_parts.detection_lists(imdb)
    output_dir = get_output_dir(imdb, weights_filename, oriented_nms=True)
    t_detect = t_misc = 0.0
    for group, frames in iter_loaded_groups(imdb, points_of, from_scan, max(batch_size, 1)):
        t0 = time.time()
        L = forward_fixed_rois(net, group_feed(net, *frames, from_scan))
        cnr, pr, pred_bv, _ = ops.box_detect_tail(L["rois"][2].contiguous(), L["bbox_pred"].contiguous(), n_classes)
        torch.cuda.synchronize()                                       # (for the timer only: one per group)
        t1 = time.time()
        out = launch_post(post, L["cls_prob"], pred_bv, cnr, pr, L["num_rois"], int(L["rois_per_frame"]), imdb.num_classes)
        if int(L["rois_status"].max().item()) & 1:
            raise ZeroDivisionError("float division")
        lists = post_lists(post, out)
        t2 = time.time()
        for i, (dets, dets_cnr) in zip(group, lists):
            for j in range(1, imdb.num_classes):
                all_boxes[j][i] = dets[j]
                all_boxes_cnr[j][i] = dets_cnr[j]
            t_detect += (t1 - t0) / len(group)
            t_misc += (t2 - t1) / len(group)
            print('im_detect: {:d}/{:d} {:.3f}s {:.3f}s'.format(i + 1, num_images, t_detect / (i + 1), t_misc / (i + 1)))
    return loop_parts.save_and_evaluate(imdb, all_boxes, all_boxes_cnr, output_dir)
