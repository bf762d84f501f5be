"""Collect a split's RPN proposals (lib/rpn_msr/generate.py:91 `imdb_proposals`, Caffe code in the reference: it runs `net.forward`
per image and keeps `rois[:, 1:]`).  Here the network runs over groups of equally shaped consecutive frames
(fast_rcnn.detect_batch.iter_frame_groups, cfg.TEST.BATCH_SIZE frames per forward, fixed ROI rows), every frame's first num_rois
rows of rois[0] (BEV) and rois[1] (image) stay on the device until the last forward is queued; only then are they read back.  The result feeds datasets.proposal_recall.evaluate_recall.
With `with_3d=True` the rows of rois[2] (the x, y, z, l, w, h LIDAR boxes) are kept as well, for
datasets.proposal_recall_3d.evaluate_recall_3d.
The frames' scans enter as in detect_batch.test_net: a three-view network gets `lidar_fv_data` rasterised from them, and with
cfg.LIDAR_BV_FROM_SCAN `lidar_bv_data` is rasterised from them too and no stored BEV map is opened (`detect_batch.scan_feed`).
With cfg.IMAGE_BLOB_ON_DEVICE frames group by BEV shape only and a group's `image_data` is one uint8 upload and one ops.image_blob call
that pads the frames to one canvas (`detect_batch.image_feed`)."""
import os
import pickle

import numpy as np
import torch

from .. import ops
from ..fast_rcnn.config import cfg, get_output_dir
from ..fast_rcnn.detect_batch import _image_key, _load_frame, host_image_blob, image_feed, iter_frame_groups, loop_scan_source, scan_feed


def imdb_proposals(sess, net, imdb, with_3d=False):
    """Generate RPN proposals on all frames of an imdb -> {'bv': [...], 'image': [...]}: per frame the (R, 4) f32 boxes in the
    proposal layer's order (descending score after NMS), also written to <get_output_dir(imdb)>/proposals.pkl.  `sess` is not
    used (the reference's TensorFlow session, kept for the call's shape).  with_3d: the result also has '3d', per frame the (R, 6) f32
    x, y, z, l, w, h rows of rois[2] in the same order, written to proposals_3d.pkl next to proposals.pkl (which stays as it is)."""
    batch_size = max(int(cfg.TEST.get("BATCH_SIZE", 1)), 1)
    if hasattr(net, "mfma_trunk") and (cfg.TEST.get("MFMA_TRUNK", False) or cfg.TEST.get("PRECISION", "fp32") != "fp32"):
        net.amp_dtype = {"fp32": None, "fp16": torch.float16, "bf16": torch.bfloat16}[cfg.TEST.get("PRECISION", "fp32")]
        net.mfma_trunk = bool(cfg.TEST.get("MFMA_TRUNK", False))
    num_images = len(imdb.image_index)
    points_of, from_scan = loop_scan_source(net, imdb)
    three_views = getattr(net, "views", 2) == 3
    pending = {}

    def keys():
        for i in range(num_images):
            pending[i] = _load_frame(imdb, i, not from_scan) + ((None if points_of is None else points_of(i)),)
            yield (_image_key(pending[i][0]), ops.BEV_SHAPE if from_scan else np.shape(pending[i][1]))

    kept = []                                                  # per group: (frames, cap, rois_bv, rois_img, num_rois, status, rois_3d), on the device
    for group in iter_frame_groups(keys(), batch_size):
        ims, bvs, calibs, clouds = zip(*(pending.pop(i) for i in group))
        B = len(group)
        im_blob = image_feed(ims) if cfg.IMAGE_BLOB_ON_DEVICE else host_image_blob(ims)
        feed = {"image_data": im_blob, "calib": np.stack([np.asarray(c, np.float32).reshape(4, 12) for c in calibs]), "keep_prob": 1.0}
        if not from_scan:
            feed["lidar_bv_data"] = np.stack([np.asarray(bv, np.float32) for bv in bvs])
        feed.update(scan_feed(clouds, from_scan, three_views))  # the group's scans back to back: one upload, one call per view
        feed["im_info"] = np.array([[feed["lidar_bv_data"].shape[1], feed["lidar_bv_data"].shape[2], 1]] * B, dtype=np.float32)
        net.fixed_rois = True
        try:
            with torch.no_grad():
                L = net.forward(feed)
        finally:
            net.fixed_rois = False
        kept.append((group, int(L["rois_per_frame"]), L["rois"][0][:, 1:5].clone(), L["rois"][1][:, 1:5].clone(), L["num_rois"].clone(),
                     L["rois_status"].clone(), L["rois"][2][:, 1:7].clone() if with_3d else None))
        print('im_proposals: {:d}/{:d}'.format(group[-1] + 1, num_images))
    out = {'bv': [None] * num_images, 'image': [None] * num_images}
    out_3d = [None] * num_images
    for group, cap, bv, img, num, status, r3d in kept:         # the read-back, after the last forward
        num, status = num.cpu().numpy(), status.cpu().numpy()
        if int(status.max(initial=0)) & 1:
            raise ZeroDivisionError("float division")
        bv, img = bv.cpu().numpy(), img.cpu().numpy()
        r3d = r3d.cpu().numpy() if with_3d else None
        for b, i in enumerate(group):
            n = min(max(int(num[b]), 0), cap)
            out['bv'][i] = np.ascontiguousarray(bv[b * cap:b * cap + n])
            out['image'][i] = np.ascontiguousarray(img[b * cap:b * cap + n])
            if with_3d:
                out_3d[i] = np.ascontiguousarray(r3d[b * cap:b * cap + n])
    with open(os.path.join(get_output_dir(imdb, None), 'proposals.pkl'), 'wb') as f:
        pickle.dump(out, f, pickle.HIGHEST_PROTOCOL)
    if with_3d:
        with open(os.path.join(get_output_dir(imdb, None), 'proposals_3d.pkl'), 'wb') as f:
            pickle.dump({'3d': out_3d}, f, pickle.HIGHEST_PROTOCOL)
        out = dict(out)
        out['3d'] = out_3d
    return out
