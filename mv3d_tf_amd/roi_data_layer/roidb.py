"""`prepare_roidb(imdb)`: enrich a dataset's roidb with what training reads (interface of
lib/roi_data_layer/roidb.py:15-60): file paths, the (4,12) calibration table, and per-object max overlap / class taken from
the one-hot `gt_overlaps`.  cfg.LIDAR_BV_FROM_SCAN (not in the reference): no `lidar_bv_path` is recorded and imdb.lidar_path_at is not
called -- the data layer rasterises the map from `velodyne_path`, which the imdb must then be able to name.
cfg.LIDAR_BV_ENCODING, cfg.LIDAR_CROP_TO_IMAGE and cfg.TRAIN.SCAN_AUGMENT are checked first (ops.bev_encoding, ops.scan_crop,
ops.scan_augment): 'paper', the crop and the augmentation need LIDAR_BV_FROM_SCAN."""
import numpy as np

from .. import ops
from ..fast_rcnn.config import cfg


def prepare_roidb(imdb):
    ops.bev_encoding()                                         # cfg.LIDAR_BV_ENCODING: 'paper' without LIDAR_BV_FROM_SCAN, or an unknown value, raises
    ops.scan_crop()                                            # cfg.LIDAR_CROP_TO_IMAGE without LIDAR_BV_FROM_SCAN raises
    ops.scan_augment()                                         # cfg.TRAIN.SCAN_AUGMENT without LIDAR_BV_FROM_SCAN, or with a bad range, raises
    from_scan = bool(cfg.LIDAR_BV_FROM_SCAN)
    if from_scan and not hasattr(imdb, 'velodyne_path_at'):
        raise ValueError("cfg.LIDAR_BV_FROM_SCAN is on and the imdb has no velodyne_path_at(i) to name the scans the bird's-eye-view "
                         "maps are rasterised from")
    roidb = imdb.roidb
    for i, entry in enumerate(roidb):
        entry['image_path'] = imdb.image_path_at(i)
        if not from_scan:                                      # (with the key on no stored map is asked for: lidar_path_at asserts the file)
            entry['lidar_bv_path'] = imdb.lidar_path_at(i)
        entry['calib'] = imdb.calib_at(i)
        if hasattr(imdb, 'velodyne_path_at'):                  # (not in the reference) the scan cfg.FRONT_VIEW_INPUT rasterises
            entry['velodyne_path'] = imdb.velodyne_path_at(i)
        dense = entry['gt_overlaps'].toarray() if hasattr(entry['gt_overlaps'], 'toarray') else np.asarray(entry['gt_overlaps'])
        entry['max_overlaps'] = dense.max(axis=1) if dense.size else np.zeros((0,), dense.dtype)
        entry['max_classes'] = dense.argmax(axis=1) if dense.size else np.zeros((0,), np.int64)
        # background rows have class 0, foreground rows a positive class (roidb.py:52-58)
        assert all(entry['max_classes'][entry['max_overlaps'] == 0] == 0)
        assert all(entry['max_classes'][entry['max_overlaps'] > 0] != 0)
    return roidb
