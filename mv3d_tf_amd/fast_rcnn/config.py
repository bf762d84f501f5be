"""Global configuration object `cfg` with the keys the hot path reads.

Mirror of the interface of lib/fast_rcnn/config.py (own implementation): attribute/dict
access, `cfg_from_file(yaml)`, `cfg_from_list([k, v, ...])` with the reference's type
checks.  Defaults are the reference's (config.py:26-243); `experiments/cfgs/
faster_rcnn_end2end.yml` values are available as `apply_end2end_yml()`.
"""
import ast

import os

import numpy as np


class AttrDict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


def _section(**kw):
    return AttrDict(**kw)


cfg = AttrDict()
cfg.TRAIN = _section(
    IMS_PER_BATCH=2, BATCH_SIZE=128, FG_FRACTION=0.25, FG_THRESH=0.5, BG_THRESH_HI=0.5, BG_THRESH_LO=0.1,
    RPN_POSITIVE_OVERLAP=0.7, RPN_NEGATIVE_OVERLAP=0.5, RPN_CLOBBER_POSITIVES=False, RPN_FG_FRACTION=0.25,
    RPN_BATCHSIZE=128, RPN_NMS_THRESH=0.7, RPN_PRE_NMS_TOP_N=12000, RPN_POST_NMS_TOP_N=2000, RPN_MIN_SIZE=5,
    HAS_RPN=False, BBOX_NORMALIZE_TARGETS_PRECOMPUTED=False, PROPOSAL_METHOD='selective_search',
    DISPLAY=10, SNAPSHOT_ITERS=5000, SNAPSHOT_PREFIX='VGGnet_fast_rcnn', SNAPSHOT_INFIX='', DEBUG_TIMELINE=False,
    SCALES=(600,), MAX_SIZE=2000, USE_FLIPPED=False, LEARNING_RATE=0.001,
    # (not in the reference) True: SolverWrapper trains in mixed precision -- the trunks' forward / data-gradient / weight-gradient
    # convolutions on the bf16 MFMA kernels (mv3d_tf_amd/trunk_train.py), the other dense layers under bf16 autocast, fp32 master
    # weights and Adam.  False = the reference's fp32 training.
    MIXED_PRECISION=False,
    # (not in the reference) True: the trunks' convolutions on this library's MFMA kernels in the precision MIXED_PRECISION selects --
    # with MIXED_PRECISION False that is the exact-f32 kernels (v_mfma_f32_32x32x2_f32): the reference's precision, 52.9 -> 47.6 ms
    # in a single process (under data parallelism the trunks share one stream and MIOpen's fp32 kernels are the faster choice).
    MFMA_TRUNK=False,
    # (not in the reference) True: the MV3D paper's empty-anchor removal (section 3.2) -- anchors with fewer than
    # RPN_EMPTY_ANCHOR_MIN_CELLS occupied cells of the bird's-eye-view map under them (ops.anchor_occupancy) get no RPN label and are
    # no proposal candidates.  False = the reference, which runs every anchor.
    RPN_SKIP_EMPTY_ANCHORS=False, RPN_EMPTY_ANCHOR_MIN_CELLS=1,
    # (not in the reference; cfg.FUSION = 'deep' only) the MV3D paper's training regularisers for the deep-fusion head (section 3.3):
    # DROP_PATH draws global or local drop-path for the two joins of every training forward from the network's own generator
    # (net.drop_path_rng, seeded with RNG_SEED); AUX_LOSSES adds one weight-sharing auxiliary path per view with its own
    # classification and box loss (weight 1), removed at inference.
    DROP_PATH=False, AUX_LOSSES=False,
    # (not in the reference, which drops every label row that is not a trained class, so a Van or the far traffic KITTI marks DontCare
    # is trained as background while the evaluator forgives detections there) IGNORE_TYPES: KITTI label types whose regions take no part
    # in training -- a SAMPLED background anchor or ROI whose intersection with such a region, over its OWN area, reaches IGNORE_OVERLAP
    # (in BEV for the types' 3D boxes, in the image for DontCare boxes) gets label -1 on the device after the target layers have drawn
    # (ops.ignore_relabel) and both stages' losses skip it.  The sample slot is spent, not redrawn; the numpy
    # RNG stream of the draws is the key-off stream.  () = the reference.  The documented KITTI setting is ('Van', 'DontCare').  A type
    # outside KITTI's vocabulary or a trained class raises ValueError (check_ignore_types below).  No accuracy claim.
    IGNORE_TYPES=(), IGNORE_OVERLAP=0.5,
    # (not in the reference, whose stored lidar_bv/*.npy maps cannot be rotated; needs cfg.LIDAR_BV_FROM_SCAN) SCAN_AUGMENT: every visit
    # of a training frame draws a similarity transform A of the LIDAR frame -- a rotation about the vertical axis by theta in
    # [-SCAN_AUGMENT_ROTATION, SCAN_AUGMENT_ROTATION) radians, a uniform scale in SCAN_AUGMENT_SCALE = (lo, hi), a shift by (dx, dy, dz)
    # with |d| below SCAN_AUGMENT_SHIFT metres per axis -- from a generator of datasets/augment.py's own (seeded RNG_SEED + rank; the
    # numpy RNG stream of the target layers' draws is the key-off stream).  The uploaded scan is transformed on the device in front of
    # the crop and the rasters (ops.scan_transform), Tr_velo_to_cam takes A^-1, so the image and every
    # camera-frame quantity stay as they are, and the LIDAR-frame ground truth and ignore regions follow A
    # (datasets.augment.augment_annotation).  The mirror (USE_FLIPPED) composes with it.  The test-time loops never augment.  The
    # default ranges (10 degrees, 5 % scale, no shift) are a guess that nothing here can validate: parity unpinned, no accuracy
    # claim.  On without LIDAR_BV_FROM_SCAN, or with a scale bound <= 0, prepare_roidb raises ValueError (ops.scan_augment).
    # False = every blob, launch and RNG stream as before.
    SCAN_AUGMENT=False, SCAN_AUGMENT_ROTATION=0.17453292519943295, SCAN_AUGMENT_SCALE=(0.95, 1.05),
    SCAN_AUGMENT_SHIFT=(0.0, 0.0, 0.0),
    # (not in the reference, whose one live solver line is AdamOptimizer(1e-5): its MomentumOptimizer, exponential_decay and WEIGHT_DECAY
    # sit commented out or unread, lib/fast_rcnn/train_mv.py:138-146, config.py:38-40) SOLVER: 'reference' = that line, Adam at
    # SolverWrapper.LEARNING_RATE, a constant rate, none of the keys below read; 'adam' or 'sgd' = optim.Adam / optim.SGD at the rate
    # optim.learning_rate(it) = LEARNING_RATE * GAMMA ** (it // STEPSIZE), times min(1, (it + 1) / WARMUP_ITERS) when WARMUP_ITERS > 0,
    # set before every step.  MOMENTUM: 'sgd' only (torch.optim.SGD's and TensorFlow's rule buf = momentum buf + g, p -= lr buf).
    # WEIGHT_DECAY: L2 decay added to the gradient of every tensor with ndim >= 2 (weights; biases get none).  Anything else in SOLVER
    # raises ValueError at the top of train_model.
    SOLVER='reference', MOMENTUM=0.9, WEIGHT_DECAY=0.0, GAMMA=0.1, STEPSIZE=50000, WARMUP_ITERS=0,
    # ('adam' / 'sgd' only) CLIP_GRAD_NORM: the global L2 norm the averaged gradients are scaled down to before the update
    # (torch.nn.utils.clip_grad_norm_'s rule; 0 = off).  SKIP_NON_FINITE: a step whose global gradient norm is inf or NaN changes no
    # weight and no optimizer buffer (it still counts as an iteration, and as a step of Adam's bias corrections).  Norm, coefficient
    # and flag stay on the device (ops of csrc/solver.hip); they are read and logged on DISPLAY steps only.
    # The paper's recipe is SOLVER='sgd', LEARNING_RATE=0.001, STEPSIZE=100000, GAMMA=0.1; nothing here can validate it: no accuracy claim.
    CLIP_GRAD_NORM=0.0, SKIP_NON_FINITE=False)
cfg.TEST = _section(
    NMS=0.5, HAS_RPN=True, RPN_NMS_THRESH=0.7, RPN_PRE_NMS_TOP_N=12000, RPN_POST_NMS_TOP_N=2000, RPN_MIN_SIZE=5,
    DEBUG_TIMELINE=False,
    # (not in the reference) test_net serves the 3x3 convolutions through this library's MFMA kernels: MFMA_TRUNK True with
    # PRECISION "fp32" (exact f32, the reference's precision), "fp16" or "bf16" (dense layers autocast as well)
    MFMA_TRUNK=False, PRECISION="fp32",
    # (not in the reference) what kitti_mv3d.evaluate_detections scores on the device: any of 'bev', '3d' (AP_BEV, AP_3D),
    # '2d' (AP_2D) and 'aos' (average orientation similarity); datasets/kitti_eval.py
    KITTI_EVAL_METRICS=('bev', '3d'),
    # (not in the reference) frames per forward of fast_rcnn.detect_batch.test_net: 1 = the reference's frame-by-frame loop
    # (test_mv.test_net); n > 1 groups up to n consecutive frames of equal image / BEV shapes and finishes them on the device
    # (ops.detect_post), one read-back per group
    BATCH_SIZE=1,
    # (not in the reference) True: fast_rcnn.detect_batch.test_net and ServeGraph run the final NMS on the ORIENTED BEV footprints
    # (ops.detect_post_oriented, the evaluator's IoU) instead of the axis-aligned pixel boxes; test_mv.test_net raises ValueError with
    # the key on (get_output_dir below refuses a detection loop without oriented NMS).
    # NMS_ORIENTED_BOXES: 'regressed' = the class's regressed corners, which are then also what all_boxes_cnr stores, or
    # 'proposal' = the proposal's own corners
    NMS_ORIENTED=False, NMS_ORIENTED_BOXES='regressed',
    # (not in the reference) the paper's empty-anchor removal at test time, as cfg.TRAIN.RPN_SKIP_EMPTY_ANCHORS: the proposal layer
    # (frame by frame, batched and in the captured ServeGraph step) ranks only the anchors over occupied cells
    RPN_SKIP_EMPTY_ANCHORS=False, RPN_EMPTY_ANCHOR_MIN_CELLS=1)
cfg.PIXEL_MEANS = np.array([[[95.8814, 98.7743, 93.8549]]])
# (not in the reference) how the views meet in the second stage: 'early' = the reference's head (every view runs fc6 -> fc7 alone, the
# towers are concatenated in front of cls_score / bbox_pred); 'deep' = the MV3D paper's deep fusion (the views' activations are joined
# by an element-wise mean after every layer, networks/mv3d.py)
cfg.FUSION = 'early'
# (not in the reference, which has the layers commented out: MV3D_train.py:117-120) the MV3D paper's upsampling of the feature maps in
# front of ROI pooling (section 3.2): bilinear factors for (bird's-eye view, image, front view), each 1, 2 or 4; the paper's setting is
# (4, 2, 4).  A view with factor s pools its conv5_3 upsampled s times at scale s / 8 (ops.upsample_bilinear_views, DESIGN.md section
# 3.20); (1, 1, 1) = the reference: nothing is upsampled.  No parameters, so every checkpoint loads under every setting.
cfg.ROI_UPSAMPLE = (1, 1, 1)
# (not in the reference, which has no front view) True: the data layer adds `lidar_fv_data` (1, 64, 512, 3), the third view's input,
# rasterised on the device from the frame's Velodyne scan (ops.point_cloud_2_front; the entry's 'lidar_fv' map,
# 'velodyne' array or 'velodyne_path' file).  False = the reference's blobs.  train_net refuses a 3-view network with the key off.
cfg.FRONT_VIEW_INPUT = False
# (not in the reference, which reads every frame's bird's-eye-view map from <kitti>/object/training/lidar_bv/*.npy, 13 MB a frame that
# KITTI does not ship) True: `lidar_bv_data` is rasterised on the device from the frame's Velodyne scan (ops.point_cloud_2_top_batch,
# DESIGN.md section 3.22; the entry's 'lidar_bv' map if it has one, else its 'velodyne' array or 'velodyne_path' file): prepare_roidb
# records no lidar_bv_path, and get_minibatch, detect_batch.test_net and rpn_msr.generate.imdb_proposals never open a stored map.  With
# FRONT_VIEW_INPUT also on, both rasters read one upload of the scan.  False = the stored maps, every blob and code path as before.
cfg.LIDAR_BV_FROM_SCAN = False
# (not in the reference) what the rasterised `lidar_bv_data` holds.  'reference' = point_cloud_2_top's map, (601, 601, 9): per height
# slice the LAST point written, and the reflectance of the last slice's last point.  'paper' = the MV3D paper's encoding (section 3.1;
# ops.point_cloud_2_top_paper), (601, 601, 10): per slice the MAXIMAL height, the reflectance of the cell's
# highest point, and the density min(1, log(N + 1) / log 64); it does not depend on the order of the points, and the network's BEV
# conv1_1 takes 10 channels (MV3D(bev_channels=None) follows this key).  Parity unpinned, no accuracy claim.  'paper' needs
# LIDAR_BV_FROM_SCAN, because stored lidar_bv/*.npy maps are reference-encoded: prepare_roidb and the detection loops raise
# ValueError otherwise, and for any other value (ops.bev_encoding).
cfg.LIDAR_BV_ENCODING = 'reference'
# (not in the reference, whose maps hold every return inside [0, 60] x [-30, 30] m) True: the paper's "we also remove points that are out
# of the image boundaries when projected to the image plane" (section 3.4): a frame's uploaded scan is compacted on the device to the
# points the frame's calibration table puts inside its own image (ops.scan_crop_to_image), in front of the
# bird's-eye-view and front-view rasters of get_minibatch, detect_batch.test_net and rpn_msr.generate.imdb_proposals.  KITTI labels
# only what the left colour image shows; with the crop the map is empty elsewhere, and RPN_SKIP_EMPTY_ANCHORS then drops those
# anchors.  Parity unpinned, no accuracy claim.  Needs LIDAR_BV_FROM_SCAN, because stored lidar_bv/*.npy maps hold every point:
# prepare_roidb and the detection loops raise ValueError otherwise (ops.scan_crop).  False = every blob and code path as before.
cfg.LIDAR_CROP_TO_IMAGE = False
# (not in the reference, which subtracts PIXEL_MEANS on the host, frame by frame, and uploads f32) True: `image_data` is built on the
# device from ONE upload of the frames' uint8 pixels (ops.image_blob) by get_minibatch, detect_batch.test_net
# and rpn_msr.generate.imdb_proposals; the two loops then group frames by BEV shape only and pad a group's frames to one canvas, the
# reference's im_list_to_blob (lib/utils/blob.py:14-27).  IMAGE_CANVAS: None = the group's maximal image shape (get_minibatch: the
# frame's own), or a fixed (H, W) such as (376, 1242) that every frame is padded to -- what a captured graph and the frames of one
# training step need; a larger frame raises ValueError.  False = the host expression, every blob and code path as before.
cfg.IMAGE_BLOB_ON_DEVICE = False
cfg.IMAGE_CANVAS = None
cfg.RNG_SEED = 3
cfg.EPS = 1e-14
cfg.EXP_DIR = 'default'
cfg.ROOT_DIR = os.path.abspath(os.path.join(os.path.dirname(__file__), '..', '..'))
# The reference sets this from `nvcc` being on PATH (config.py:235-242) and nms_wrapper.py:19-20 then picks gpu_nms, whose
# rule (IoU > thresh in f32) differs from cpu_nms ((double)IoU >= thresh) on boxes whose IoU rounds to the threshold.
# Both rules run on the MI355X here.  The parity target of this repository is the reference's CPU path (BASELINE.json), so
# the default is False = the cpu_nms rule everywhere (dispatcher and the NMS inside proposal_layer_3d); True selects the
# gpu_nms rule in both places, like a reference install with nvcc.  GPU_ID selects the HIP device.
cfg.USE_GPU_NMS = False
cfg.GPU_ID = 0


# KITTI's label vocabulary (devkit_object/readme.txt): what cfg.TRAIN.IGNORE_TYPES may list
KITTI_TYPES = ('Car', 'Van', 'Truck', 'Pedestrian', 'Person_sitting', 'Cyclist', 'Tram', 'Misc', 'DontCare')


def check_ignore_types(ignore_types, trained=('Car',)):
    """cfg.TRAIN.IGNORE_TYPES -> tuple of str; ValueError for a type outside KITTI's vocabulary or a trained class (`trained`: the
    dataset's class names; kitti_mv3d trains Car)"""
    if isinstance(ignore_types, str):
        raise ValueError("IGNORE_TYPES must be a sequence of KITTI label types, got the string %r" % (ignore_types,))
    types = tuple(ignore_types or ())
    for t in types:
        if t not in KITTI_TYPES:
            raise ValueError("IGNORE_TYPES: %r is not a KITTI label type %s" % (t, KITTI_TYPES))
        if t in trained:
            raise ValueError("IGNORE_TYPES: %r is a trained class" % (t,))
    return types


def _merge(a, b, path=""):
    for k, v in a.items():
        if k not in b:
            raise KeyError('{} is not a valid config key'.format(path + k))
        old = b[k]
        if isinstance(old, dict):
            if not isinstance(v, dict):
                raise ValueError('Type mismatch for config key: {}'.format(path + k))
            _merge(v, old, path + k + ".")
            continue
        if isinstance(old, np.ndarray):
            v = np.array(v, dtype=old.dtype)
        elif path + k == "ROI_UPSAMPLE" and isinstance(v, list):  # (YAML has no tuples: its sequence for this one key)
            v = tuple(v)
        elif path + k == "TRAIN.IGNORE_TYPES" and isinstance(v, (list, tuple)):   # a YAML sequence, as ROI_UPSAMPLE
            v = check_ignore_types(v)
        elif path + k == "IMAGE_CANVAS":                          # None or (H, W), a YAML sequence
            v = None if v is None else tuple(int(s) for s in v)
        elif type(old) is not type(v) and not (isinstance(old, float) and isinstance(v, int)):
            raise ValueError('Type mismatch ({} vs. {}) for config key: {}'.format(type(old), type(v), path + k))
        b[k] = type(old)(v) if isinstance(old, float) else v


def cfg_from_file(filename):
    """Merge a YAML file into `cfg` (lib/fast_rcnn/config.py:291-297)."""
    import yaml
    with open(filename) as f:
        _merge(yaml.safe_load(f) or {}, cfg)


def cfg_from_list(cfg_list):
    """`--set K V K V ...` overrides (lib/fast_rcnn/config.py:299-319)."""
    assert len(cfg_list) % 2 == 0
    for k, v in zip(cfg_list[0::2], cfg_list[1::2]):
        keys = k.split('.')
        d = cfg
        for sub in keys[:-1]:
            assert sub in d
            d = d[sub]
        assert keys[-1] in d
        try:
            value = ast.literal_eval(v)
        except Exception:
            value = v
        assert type(value) == type(d[keys[-1]]) or k == 'IMAGE_CANVAS', 'type {} does not match original type {}'.format(
            type(value), type(d[keys[-1]]))
        d[keys[-1]] = check_ignore_types(value) if k == 'TRAIN.IGNORE_TYPES' else value


def apply_end2end_yml():
    """experiments/cfgs/faster_rcnn_end2end.yml:1-20 (what experiments/scripts/mv3d.sh uses)."""
    _merge({"EXP_DIR": "faster_rcnn_end2end",
            "TRAIN": {"HAS_RPN": True, "IMS_PER_BATCH": 1, "BBOX_NORMALIZE_TARGETS_PRECOMPUTED": True,
                      "RPN_POSITIVE_OVERLAP": 0.7, "RPN_BATCHSIZE": 128, "PROPOSAL_METHOD": "gt",
                      "BG_THRESH_LO": 0.0, "BG_THRESH_HI": 0.5, "FG_THRESH": 0.7,
                      "RPN_PRE_NMS_TOP_N": 12000, "RPN_POST_NMS_TOP_N": 2000},
            "TEST": {"RPN_PRE_NMS_TOP_N": 6000, "RPN_POST_NMS_TOP_N": 300, "HAS_RPN": True, "NMS": 0.1}}, cfg)


def get_output_dir(imdb, weights_filename, oriented_nms=False):
    """Directory for the detections of `imdb` (lib/fast_rcnn/config.py:245-257): ROOT_DIR/output/EXP_DIR/<imdb.name>
    [/<weights_filename>]; created if missing.  A detection loop (weights_filename given) that has no oriented NMS
    (oriented_nms=False: the frame-by-frame test_mv.test_net) is refused here while cfg.TEST.NMS_ORIENTED is on, before anything
    is created or a frame is loaded: its detections would not be what the configuration says."""
    if weights_filename is not None and not oriented_nms and cfg.TEST.get("NMS_ORIENTED", False):
        raise ValueError("cfg.TEST.NMS_ORIENTED is set: the frame-by-frame reference loop (fast_rcnn.test_mv.test_net) has no oriented "
                         "NMS; use fast_rcnn.detect_batch.test_net")
    outdir = os.path.abspath(os.path.join(cfg.ROOT_DIR, 'output', cfg.EXP_DIR, imdb.name))
    if weights_filename is not None:
        outdir = os.path.join(outdir, weights_filename)
    if not os.path.exists(outdir):
        os.makedirs(outdir)
    return outdir

