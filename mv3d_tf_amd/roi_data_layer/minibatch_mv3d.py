"""`get_minibatch(roidb, num_classes)`: the blobs of one training frame (interface of
lib/roi_data_layer/minibatch_mv3d.py:17-76).

Keys and dtypes as the reference feeds them: image_data (1,H,W,3) f32 BGR minus PIXEL_MEANS,
lidar_bv_data (1,Hbv,Wbv,9), calib (4,12), gt_boxes / gt_boxes_bv (G,5), gt_boxes_3d (G,7), gt_boxes_corners (G,25),
im_info (1,3) = BEV size.  One numpy draw is kept for RNG-stream parity with the reference (`npr.randint` over
cfg.TRAIN.SCALES, :22-23, whose result the reference never uses either).  A roidb entry may carry the frame in memory
('image' (H,W,3) BGR array, 'lidar_bv' array) instead of 'image_path' / 'lidar_bv_path'; image files are read by
utils.read_image.read_image_bgr.  An entry with `flipped` true (cfg.TRAIN.USE_FLIPPED) returns its two maps as
device tensors, mirrored left/right by ops.mirror_columns; every other entry returns numpy as the reference does.

cfg.FRONT_VIEW_INPUT (not in the reference; default off = the blobs above exactly) adds `lidar_fv_data` (1,64,512,3), the third view's
input, as a device tensor: see `front_view_blob`.
cfg.LIDAR_BV_FROM_SCAN (not in the reference; default off) takes `lidar_bv_data` of an entry without an in-memory 'lidar_bv' from its
scan ('velodyne' array or 'velodyne_path' file) instead of 'lidar_bv_path': a (1,601,601,9) device tensor rasterised by
ops.scan_bev -- ops.point_cloud_2_top_batch, or under cfg.LIDAR_BV_ENCODING = 'paper' ops.point_cloud_2_top_paper and (1,601,601,10) --,
im_info = (601, 601, 1); with both keys on the scan is read and uploaded once for both rasters.
cfg.LIDAR_CROP_TO_IMAGE (not in the reference; default off; needs LIDAR_BV_FROM_SCAN) crops every scan uploaded here to the points
inside the frame's own image before either raster reads it: see `_device_cloud`.  In-memory 'lidar_bv' / 'lidar_fv' maps are the
caller's and stay as they are.
cfg.IMAGE_BLOB_ON_DEVICE (not in the reference; default off) builds `image_data` on the device: see `image_blob`.
cfg.TRAIN.IGNORE_TYPES (not in the reference; default () = the blobs above exactly) adds the frame's ignore regions, `ignore_boxes_bv`
(K,4) and `ignore_boxes_img` (M,4) f32 host arrays (datasets.kitti_mv3d.ignore_blobs); the roidb must have been parsed under the key.
cfg.TRAIN.SCAN_AUGMENT (not in the reference; default off = the blobs above exactly; needs LIDAR_BV_FROM_SCAN) draws a similarity
transform of the LIDAR frame at every call and returns the blobs of the transformed frame, plus `scan_transform`, its (3,4) f64
matrix: see `_augmented`."""
import numpy as np
import numpy.random as npr

from .. import ops
from ..datasets import augment
from ..datasets.kitti_mv3d import gt_blobs, ignore_blobs
from ..fast_rcnn.config import cfg
from ..utils.read_image import read_image_bgr


def _entry_cloud(entry, key, own_map):
    """the (P,4) f32 [x,y,z,reflectance] scan of a roidb entry as a contiguous host array: entry['velodyne'], an array in memory, else
    the file entry['velodyne_path'] names (a KITTI `.bin` scan or a `.npy`, utils.read_lidar.load_velodyne).  A `flipped` entry gets
    the cloud with y negated (the mirror of the scene, datasets/mirror.py), as a copy: the entry's own array stays."""
    if 'velodyne' in entry:
        pts = np.asarray(entry['velodyne'], np.float32)
    elif 'velodyne_path' in entry:
        from ..utils.read_lidar import load_velodyne
        pts = load_velodyne(entry['velodyne_path'])
    else:
        raise ValueError("cfg.{} is on and the roidb entry has none of '{}', 'velodyne', 'velodyne_path'".format(key, own_map))
    pts = np.ascontiguousarray(pts.reshape(-1, pts.shape[-1])[:, :4])
    if entry.get('flipped', False):
        pts = pts * np.array([1, -1, 1, 1], np.float32)
    return pts


def _device_cloud(entry, key, own_map, image, xform=None):
    """(points, offsets) of a roidb entry's scan on the device, what the rasterisers take: `_entry_cloud` uploaded once, offsets None
    = one frame of every row.  Under cfg.LIDAR_CROP_TO_IMAGE the upload is cropped (ops.scan_crop_to_image) to the points the entry's
    calibration table puts inside `image`, the frame's own (h, w, 3) pixels: offsets is then the crop's (2,) device tensor, and the
    rows of `points` behind offsets[1] belong to no frame.  A `flipped` entry's cloud, y negated, is cropped with the entry's own,
    mirrored table; at the image border that need not be the mirror of the source frame's crop.  xform = the (3,4) f64 matrix of
    cfg.TRAIN.SCAN_AUGMENT: the upload is transformed in place (ops.scan_transform) in front of the crop, which `entry`, the augmented
    one, then judges with its own table."""
    cloud = ops._dev(_entry_cloud(entry, key, own_map))
    if xform is not None:
        ops.scan_transform(cloud, None, np.asarray(xform, np.float64).reshape(1, 3, 4), out=cloud)
    if ops.scan_crop():
        return ops.scan_crop_to_image(cloud, None, [entry['calib']], [np.shape(image)])
    return cloud, None


def front_view_blob(entry, cloud=None, offsets=None):
    """`lidar_fv_data` (1,64,512,3) f32 on the device for one roidb entry, from the first of: entry['lidar_fv'], a (64,512,3) map in
    memory, used as is; entry['velodyne'], a (P,4) [x,y,z,reflectance] array; entry['velodyne_path'], a KITTI `.bin` scan or a `.npy`
    (utils.read_lidar.load_velodyne) -- a cloud is rasterised by ops.point_cloud_2_front.
    A `flipped` entry rasterises the cloud with y negated on the host (the mirror of the scene, datasets/mirror.py).  Its map is NOT
    the column-reversed map of the source frame: the column is floor((45 deg - azimuth) / d_theta), and floor makes the bin edges
    asymmetric -- a point exactly on an edge belongs to the bin on one fixed side of it before and after the mirror, and azimuth
    +45 deg is column 0 while -45 deg is column 512, outside the map -- so reversing the columns is not the mirrored scene's raster.
    An in-memory 'lidar_fv' is the caller's map for that entry and is not touched.
    cloud = the entry's scan already on the device, (P,4) f32 with y negated if the entry is `flipped` (what get_minibatch uploaded
    for the bird's-eye view under cfg.LIDAR_BV_FROM_SCAN): rasterised in place of a second read and upload of the scan.  offsets =
    that cloud's (2,) device offsets where it was cropped (`_device_cloud`): the one frame owns rows offsets[0]:offsets[1]."""
    if 'lidar_fv' in entry:
        fv = ops._dev(entry['lidar_fv'])
        if tuple(fv.shape) != ops.FV_SHAPE:
            raise ValueError("entry['lidar_fv'] must be {}, got {}".format(ops.FV_SHAPE, tuple(fv.shape)))
        return fv[None]
    cloud = _entry_cloud(entry, 'FRONT_VIEW_INPUT', 'lidar_fv') if cloud is None else cloud
    return ops.point_cloud_2_front(cloud, offsets=offsets).reshape((1,) + ops.FV_SHAPE)


def image_blob(entry, image):
    """`image_data` (1,H,W,3) f32 on the device under cfg.IMAGE_BLOB_ON_DEVICE: the frame's uint8 (h,w,3) BGR pixels are uploaded
    ONCE, as bytes, and ops.image_blob subtracts cfg.PIXEL_MEANS (bit for bit the host expression of the key-off path).  A `flipped`
    entry sets the call's flip flag, which gives the mirrored frame directly -- no f32 upload, no ops.mirror_columns.
    cfg.IMAGE_CANVAS = (H, W) pads the frame at the top-left corner of a zero canvas of that shape (im_list_to_blob's rule), so that
    a step's frames of different sizes stack; a larger frame raises ValueError.  None: (H, W) = (h, w), no padding.  An image that
    is not a uint8 (h,w,3) array raises TypeError."""
    if not isinstance(image, np.ndarray) or image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise TypeError("cfg.IMAGE_BLOB_ON_DEVICE needs the frame as a uint8 (h, w, 3) array, got {}".format(
            "{} {}".format(image.dtype, image.shape) if isinstance(image, np.ndarray) else type(image).__name__))
    return ops.image_blob([image], canvas=cfg.IMAGE_CANVAS, flip=[bool(entry.get('flipped', False))])


_FRAME_DATA = ('image', 'velodyne', 'lidar_bv', 'lidar_fv')        # a frame carried in memory: arrays that no annotation transform copies


def _augmented(entry):
    """(cfg.TRAIN.SCAN_AUGMENT) one draw of datasets.augment -> (the roidb entry of the transformed frame, A): the LIDAR-frame ground
    truth and ignore regions follow the (3,4) f64 matrix A, `calib` carries A^-1 in Tr_velo_to_cam, every other field -- the frame's
    files and in-memory arrays, the camera-frame fields, `flipped` -- is the entry's own.  `entry` is not modified.  The draw comes
    from the module's own generator, never from numpy's global one.  An entry that carries a 'lidar_bv' or 'lidar_fv' map raises
    ValueError: that map is the caller's and cannot be transformed."""
    for k in ('lidar_bv', 'lidar_fv'):
        if k in entry:
            raise ValueError("cfg.TRAIN.SCAN_AUGMENT is on and the roidb entry carries an in-memory '{}' map, which cannot be "
                             "transformed: give the frame's scan ('velodyne' or 'velodyne_path')".format(k))
    theta, scale, shift = augment.draw_scan_transform()
    A, A_inv = augment.transform_matrix(theta, scale, shift)
    out = dict(entry)
    out.update(augment.augment_annotation({k: v for k, v in entry.items() if k not in _FRAME_DATA}, A, scale))
    out['calib'] = augment.augment_calib(entry['calib'], A_inv)
    return out, A


def get_minibatch(roidb, num_classes):
    num_images = len(roidb)
    npr.randint(0, high=len(cfg.TRAIN.SCALES), size=num_images)          # RNG-stream parity (:22-23)
    assert cfg.TRAIN.BATCH_SIZE % num_images == 0, \
        'num_images ({}) must divide BATCH_SIZE ({})'.format(num_images, cfg.TRAIN.BATCH_SIZE)
    assert num_images == 1, "Single batch only"
    entry, xform = roidb[0], None
    if cfg.TRAIN.get('SCAN_AUGMENT', False) and ops.scan_augment():
        entry, xform = _augmented(entry)
    image = entry['image'] if 'image' in entry else read_image_bgr(entry['image_path'])
    on_device = bool(cfg.IMAGE_BLOB_ON_DEVICE)              # then image_data is final here: built, and mirrored, by ops.image_blob
    image_data = image_blob(entry, image) if on_device else (image.astype(np.float32, copy=True) - cfg.PIXEL_MEANS)[None].astype(np.float32)
    cloud = offsets = None
    if cfg.LIDAR_BV_FROM_SCAN and 'lidar_bv' not in entry:
        # no stored map: the scan is uploaded once (a mirrored frame's with y negated, whose raster IS the column-reversed map:
        # tests/test_mirror.py::test_bev_raster_commutes_with_the_mirror), cropped to the image under cfg.LIDAR_CROP_TO_IMAGE, and
        # rasterised on the device
        cloud, offsets = _device_cloud(entry, 'LIDAR_BV_FROM_SCAN', 'lidar_bv', image, xform)
        bev = ops.scan_bev(cloud, offsets)
        blobs = {'image_data': image_data, 'lidar_bv_data': bev.reshape((1,) + tuple(bev.shape[-3:])), 'calib': entry['calib']}
        blobs.update(gt_blobs(entry, ops.BEV_SHAPE))
        if entry.get('flipped', False) and not on_device:
            blobs['image_data'] = ops.mirror_columns(ops._dev(blobs['image_data']))
    else:
        bev = entry['lidar_bv'] if 'lidar_bv' in entry else np.load(entry['lidar_bv_path'])
        blobs = {'image_data': image_data, 'lidar_bv_data': np.asarray(bev)[None], 'calib': entry['calib']}
        blobs.update(gt_blobs(entry, np.asarray(bev).shape))
    if cloud is None and entry.get('flipped', False):
        # a mirrored frame (kitti_mv3d.append_flipped_images): the files are the source frame's, the entry's ground truth and
        # calibration are the mirror's already; the two maps are uploaded and mirrored on the device (ops.mirror_columns) and
        # go to the network as device tensors.  The BEV raster's mirror axis is its column 300 (datasets/mirror.py).
        if blobs['lidar_bv_data'].shape[2] != 601:
            raise ValueError("a mirrored frame needs the 601 columns wide BEV map of point_cloud_2_top (mirror axis = column "
                             "300), this one is {} wide".format(blobs['lidar_bv_data'].shape[2]))
        for k in ('lidar_bv_data',) if on_device else ('image_data', 'lidar_bv_data'):
            blobs[k] = ops.mirror_columns(ops._dev(blobs[k]))
    if cfg.FRONT_VIEW_INPUT:
        if cloud is None and 'lidar_fv' not in entry and ops.scan_crop():      # (an in-memory 'lidar_bv': the scan was not uploaded above)
            cloud, offsets = _device_cloud(entry, 'FRONT_VIEW_INPUT', 'lidar_fv', image)
        blobs['lidar_fv_data'] = front_view_blob(entry, cloud, offsets)
    if cfg.TRAIN.get('IGNORE_TYPES', ()):
        blobs.update(ignore_blobs(entry))
    if xform is not None:
        blobs['scan_transform'] = xform                      # for the record: nothing downstream reads it
    return blobs
