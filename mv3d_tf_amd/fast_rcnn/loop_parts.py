"""What every test-time loop over an imdb does around the network (fast_rcnn.test_mv.test_net, fast_rcnn.detect_batch.test_net,
rpn_msr.generate.imdb_proposals): the precision keys, the frame read, and a detection loop's lists, pickles and evaluation."""
import os
import pickle

import numpy as np
import torch

from .config import cfg
from ..utils.read_image import read_image_bgr


def apply_test_precision(net):
    """cfg.TEST.MFMA_TRUNK / cfg.TEST.PRECISION onto a network that has the MFMA trunk (every test-time loop calls this first)"""
    if hasattr(net, "mfma_trunk") and (cfg.TEST.get("MFMA_TRUNK", False) or cfg.TEST.get("PRECISION", "fp32") != "fp32"):
        net.amp_dtype = {"fp32": None, "fp16": torch.float16, "bf16": torch.bfloat16}[cfg.TEST.get("PRECISION", "fp32")]
        net.mfma_trunk = bool(cfg.TEST.get("MFMA_TRUNK", False))


def load_frame(imdb, i, stored_bv=True):
    """(image, BEV map, calib) of frame i of a duck-typed imdb: calib_at(i) and either image_at(i) / bv_at(i) (arrays) or
    image_path_at(i) / lidar_path_at(i) (files: .npy for the BEV, an image utils.read_image.read_image_bgr reads).
    stored_bv=False (cfg.LIDAR_BV_FROM_SCAN): the map is None and neither imdb.bv_at nor imdb.lidar_path_at is touched"""
    if hasattr(imdb, "image_at"):
        im, bv = imdb.image_at(i), (imdb.bv_at(i) if stored_bv else None)
    else:
        bv = np.load(imdb.lidar_path_at(i)) if stored_bv else None
        im = read_image_bgr(imdb.image_path_at(i))
    return im, bv, imdb.calib_at(i)


def detection_lists(imdb):
    """the empty all_boxes[cls][image] and all_boxes_cnr[cls][image] of a detection loop"""
    n = len(imdb.image_index)
    return tuple([[[] for _ in range(n)] for _ in range(imdb.num_classes)] for _ in range(2))


def save_and_evaluate(imdb, all_boxes, all_boxes_cnr, output_dir):
    """the end of a detection loop (lib/fast_rcnn/test_mv.py:508-517): both pickles under output_dir, then imdb.evaluate_detections"""
    with open(os.path.join(output_dir, 'detections.pkl'), 'wb') as f:
        pickle.dump(all_boxes, f, pickle.HIGHEST_PROTOCOL)
    with open(os.path.join(output_dir, 'detections_cnr.pkl'), 'wb') as f:
        pickle.dump(all_boxes_cnr, f, pickle.HIGHEST_PROTOCOL)
    print('Evaluating detections')
    imdb.evaluate_detections(all_boxes, all_boxes_cnr, output_dir)
    return all_boxes, all_boxes_cnr
