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
down the device route whatever BATCH_SIZE is."""
import os
import pickle
import time

import numpy as np
import torch

from .. import ops
from . import test_mv
from .config import cfg, get_output_dir
from ..networks.mv3d import n_classes


class ServeGraph(test_mv.ServeGraph):
    """test_mv.ServeGraph whose captured step, with `post=dict(max_per_image=...)`, ends in ops.detect_post: the replay's outputs gain
    out["post"] = (det_bv, det_cnr, det_cnr_r, det_row, det_count, status), static tensors like the others.  `oriented` (default:
    cfg.TEST.NMS_ORIENTED) captures ops.detect_post_oriented with `footprint` (default: cfg.TEST.NMS_ORIENTED_BOXES) instead."""

    def __init__(self, net, feed, warmup=2, post=None):
        self.post = None if post is None else dict(post)
        self._post_out = self._post_ws = None
        if self.post is not None:
            self.post.setdefault("oriented", bool(cfg.TEST.get("NMS_ORIENTED", False)))
            self.post.setdefault("footprint", cfg.TEST.get("NMS_ORIENTED_BOXES", "regressed"))
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
            if self.post["oriented"]:
                out["post"] = ops.detect_post_oriented(out["cls_prob"], out["pred_bv"], out["corners"], out["pred_corners_r"],
                                                       out["num_rois"], cap, n_classes, int(self.post.get("max_per_image", 300)),
                                                       cfg.TEST.NMS, strict_gt=bool(cfg.USE_GPU_NMS), footprint=self.post["footprint"],
                                                       out=self._post_out, workspace=self._post_ws)
            else:
                out["post"] = ops.detect_post(out["cls_prob"], out["pred_bv"], out["corners"], out["pred_corners_r"], out["num_rois"], cap,
                                              n_classes, int(self.post.get("max_per_image", 300)), cfg.TEST.NMS, out=self._post_out)
        return out

    def final_detections(self):
        """after a replay of a graph built with `post`: per frame (dets, dets_cnr) exactly as class_detections + limit_detections return
        them (dets[0] == [], class j (N,5) / (N,25) f32) -- the score cut, NMS and cap ran inside the graph; the ONE host round trip is the
        counts, the status words and the rows in front of the counts.  Oriented NMS on the 'regressed' footprint: dets_cnr holds the
        regressed corners of the kept rows (the boxes the NMS judged)"""
        if self.post is None:
            raise ValueError("final_detections() needs ServeGraph(..., post=dict(max_per_image=...))")
        self.stream.synchronize()
        if int(self.out["status"].max().item()) & 1:
            raise ZeroDivisionError("float division")
        if self.post["oriented"] and self.post["footprint"] == "regressed":
            return [(dets, cnr_r) for dets, _, cnr_r in ops.detect_post_lists(self.out["post"], with_cnr_r=True)]
        return ops.detect_post_lists(self.out["post"])


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
    from_scan = bool(cfg.LIDAR_BV_FROM_SCAN)
    points_of = front_view_source(net, imdb)
    return (scan_source(imdb, "cfg.LIDAR_BV_FROM_SCAN") if points_of is None and from_scan else points_of), from_scan


def scan_feed(clouds, bev, fv):
    """the feed entries a group of frames gets from its scans: the clouds are concatenated and uploaded ONCE, and `lidar_bv_data`
    (bev true: one ops.point_cloud_2_top_batch call) and `lidar_fv_data` (fv true: one ops.point_cloud_2_front call) are rasterised
    from that one device tensor"""
    feed = {}
    if bev or fv:
        pts = ops._dev(np.concatenate(clouds, 0))
        offsets = np.cumsum([0] + [len(c) for c in clouds])
        if bev:
            feed["lidar_bv_data"] = ops.point_cloud_2_top_batch(pts, offsets=offsets)
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


def _load_frame(imdb, i, stored_bv=True):
    """(image, BEV map, calib) of frame i of a duck-typed imdb (see test_mv.test_net); stored_bv=False (cfg.LIDAR_BV_FROM_SCAN): the
    map is None and neither imdb.bv_at nor imdb.lidar_path_at is touched"""
    if hasattr(imdb, "image_at"):
        im, bv = imdb.image_at(i), (imdb.bv_at(i) if stored_bv else None)
    else:
        bv = np.load(imdb.lidar_path_at(i)) if stored_bv else None
        path = imdb.image_path_at(i)
        if path.endswith(".npy"):
            im = np.load(path)
        else:
            from PIL import Image                               # (the reference uses cv2.imread: BGR)
            im = np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1]
    return im, bv, imdb.calib_at(i)


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


def test_net(sess, net, imdb, weights_filename, max_per_image=300, thresh=0.05, vis=False):
    """test_mv.test_net with cfg.TEST.BATCH_SIZE (not in the reference).  1: test_mv.test_net, untouched.  n > 1: one eager forward
    with fixed ROI rows per group of equally shaped consecutive frames (`iter_frame_groups`), the box tail and ops.detect_post on the
    device, ONE read-back of the final detections per group.  A three-view network takes the device route for any BATCH_SIZE and
    gets `lidar_fv_data` from the frames' scans (`front_view_source`), a group's frames rasterised by ONE batched
    ops.point_cloud_2_front call.  cfg.LIDAR_BV_FROM_SCAN: the device route for any BATCH_SIZE, no stored BEV map is opened (`_load_frame`
    touches neither imdb.bv_at nor imdb.lidar_path_at), frames group by image shape and ops.BEV_SHAPE, and a group's `lidar_bv_data` is
    ONE ops.point_cloud_2_top_batch call on the group's scans (`scan_feed`: one upload for both rasters).  cfg.TEST.NMS_ORIENTED: the device route for any BATCH_SIZE, with
    ops.detect_post_oriented on cfg.TEST.NMS_ORIENTED_BOXES; 'regressed' stores the regressed corners in all_boxes_cnr.
    cfg.IMAGE_BLOB_ON_DEVICE: the device route for any BATCH_SIZE; frames group by BEV shape only, and a group's `image_data` is ONE
    uint8 upload and ONE ops.image_blob call that pads the frames to cfg.IMAGE_CANVAS or the group's maximal image shape (`image_feed`;
    a frame larger than IMAGE_CANVAS raises ValueError before the forward).  Pickles, the `im_detect: i/n` line (per frame, times averaged over the
    group) and the evaluate_detections call are test_mv.test_net's."""
    batch_size = int(cfg.TEST.get("BATCH_SIZE", 1))
    oriented = bool(cfg.TEST.get("NMS_ORIENTED", False))
    footprint = cfg.TEST.get("NMS_ORIENTED_BOXES", "regressed")
    points_of, from_scan = loop_scan_source(net, imdb)
    three_views = getattr(net, "views", 2) == 3
    on_device = bool(cfg.IMAGE_BLOB_ON_DEVICE)
    if batch_size <= 1 and not oriented and points_of is None and not on_device:
        return test_mv.test_net(sess, net, imdb, weights_filename, max_per_image=max_per_image, thresh=thresh, vis=vis)
    if hasattr(net, "mfma_trunk") and (cfg.TEST.get("MFMA_TRUNK", False) or cfg.TEST.get("PRECISION", "fp32") != "fp32"):
        net.amp_dtype = {"fp32": None, "fp16": torch.float16, "bf16": torch.bfloat16}[cfg.TEST.get("PRECISION", "fp32")]
        net.mfma_trunk = bool(cfg.TEST.get("MFMA_TRUNK", False))
    num_images = len(imdb.image_index)
    all_boxes = [[[] for _ in range(num_images)] for _ in range(imdb.num_classes)]
    all_boxes_cnr = [[[] for _ in range(num_images)] for _ in range(imdb.num_classes)]
    output_dir = get_output_dir(imdb, weights_filename, oriented_nms=True)
    pending = {}

    def keys():
        for i in range(num_images):
            pending[i] = _load_frame(imdb, i, not from_scan) + ((None if points_of is None else points_of(i)),)
            yield (_image_key(pending[i][0]), ops.BEV_SHAPE if from_scan else np.shape(pending[i][1]))

    t_detect = t_misc = 0.0
    for group in iter_frame_groups(keys(), max(batch_size, 1)):
        ims, bvs, calibs, clouds = zip(*(pending.pop(i) for i in group))
        B = len(group)
        t0 = time.time()
        im_blob = image_feed(ims) if on_device else host_image_blob(ims)
        feed = {"image_data": im_blob, "calib": np.stack([np.asarray(c, np.float32).reshape(4, 12) for c in calibs]), "keep_prob": 1.0}
        if not from_scan:
            feed["lidar_bv_data"] = np.stack([np.asarray(bv, np.float32) for bv in bvs])
        feed.update(scan_feed(clouds, from_scan, three_views))         # the group's scans back to back: one upload, one call per view
        feed["im_info"] = np.array([[feed["lidar_bv_data"].shape[1], feed["lidar_bv_data"].shape[2], 1]] * B, dtype=np.float32)
        net.fixed_rois = True
        try:
            with torch.no_grad():
                L = net.forward(feed)
                cnr, pr, pred_bv, _ = ops.box_detect_tail(L["rois"][2].contiguous(), L["bbox_pred"].contiguous(), n_classes)
        finally:
            net.fixed_rois = False
        torch.cuda.synchronize()                                       # (for the timer only: one per group)
        t1 = time.time()
        if oriented:
            post = ops.detect_post_oriented(L["cls_prob"], pred_bv, cnr, pr, L["num_rois"], int(L["rois_per_frame"]), imdb.num_classes,
                                            max_per_image, cfg.TEST.NMS, strict_gt=bool(cfg.USE_GPU_NMS), footprint=footprint)
        else:
            post = ops.detect_post(L["cls_prob"], pred_bv, cnr, None, L["num_rois"], int(L["rois_per_frame"]), imdb.num_classes,
                                   max_per_image, cfg.TEST.NMS)
        if int(L["rois_status"].max().item()) & 1:
            raise ZeroDivisionError("float division")
        if oriented and footprint == "regressed":
            frames = [(dets, cnr_r) for dets, _, cnr_r in ops.detect_post_lists(post, with_cnr_r=True)]
        else:
            frames = ops.detect_post_lists(post)
        t2 = time.time()
        for i, (dets, dets_cnr) in zip(group, frames):
            for j in range(1, imdb.num_classes):
                all_boxes[j][i] = dets[j]
                all_boxes_cnr[j][i] = dets_cnr[j]
            t_detect += (t1 - t0) / B
            t_misc += (t2 - t1) / B
            print('im_detect: {:d}/{:d} {:.3f}s {:.3f}s'.format(i + 1, num_images, t_detect / (i + 1), t_misc / (i + 1)))
    with open(os.path.join(output_dir, 'detections.pkl'), 'wb') as f:
        pickle.dump(all_boxes, f, pickle.HIGHEST_PROTOCOL)
    with open(os.path.join(output_dir, 'detections_cnr.pkl'), 'wb') as f:
        pickle.dump(all_boxes_cnr, f, pickle.HIGHEST_PROTOCOL)
    print('Evaluating detections')
    imdb.evaluate_detections(all_boxes, all_boxes_cnr, output_dir)
    return all_boxes, all_boxes_cnr

