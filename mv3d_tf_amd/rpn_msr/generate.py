"""Collect a split's RPN proposals (lib/rpn_msr/generate.py:91 `imdb_proposals`, Caffe code in the reference: it runs `net.forward`
per image and keeps `rois[:, 1:]`).  Here the network runs over groups of equally shaped consecutive frames, loaded, fed and run as
fast_rcnn.detect_batch.test_net does (`iter_loaded_groups`, `group_feed`, `forward_fixed_rois`: cfg.TEST.BATCH_SIZE frames per forward,
fixed ROI rows, the same cfg keys for the inputs); every frame's first num_rois rows of rois[0] (BEV) and rois[1] (image) stay on the
device until the last forward is queued; only then are they read back.  The result feeds datasets.proposal_recall.evaluate_recall.
With `with_3d=True` the rows of rois[2] (the x, y, z, l, w, h LIDAR boxes) are kept as well, for
datasets.proposal_recall_3d.evaluate_recall_3d."""
import os
import pickle

import numpy as np

from ..fast_rcnn.config import cfg, get_output_dir
from ..fast_rcnn.detect_batch import forward_fixed_rois, group_feed, iter_loaded_groups, loop_scan_source
from ..fast_rcnn.loop_parts import apply_test_precision


def imdb_proposals(sess, net, imdb, with_3d=False):
    """Generate RPN proposals on all frames of an imdb -> {'bv': [...], 'image': [...]}: per frame the (R, 4) f32 boxes in the
    proposal layer's order (descending score after NMS), also written to <get_output_dir(imdb)>/proposals.pkl.  `sess` is not
    used (the reference's TensorFlow session, kept for the call's shape).  with_3d: the result also has '3d', per frame the (R, 6) f32
    x, y, z, l, w, h rows of rois[2] in the same order, written to proposals_3d.pkl next to proposals.pkl (which stays as it is)."""
    batch_size = max(int(cfg.TEST.get("BATCH_SIZE", 1)), 1)
    apply_test_precision(net)
    num_images = len(imdb.image_index)
    points_of, from_scan = loop_scan_source(net, imdb)
    kept = []                                                  # per group: (frames, cap, rois_bv, rois_img, num_rois, status, rois_3d), on the device
    for group, frames in iter_loaded_groups(imdb, points_of, from_scan, batch_size):
        L = forward_fixed_rois(net, group_feed(net, *frames, from_scan))
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
