"""KITTI object files -> MV3D ground truth, and the gt blobs of a training frame.

  <kitti>/object/{training,testing}/calib/000000.txt     P0..P3, R0_rect, Tr_velo_to_cam, Tr_imu_to_velo
  <kitti>/object/training/label_2/000000.txt             type trunc occ alpha x1 y1 x2 y2 h w l tx ty tz ry
  <kitti>/object/training/{image_2/*.png, lidar_bv/*.npy}, <kitti>/ImageSets/<set>.txt
  <kitti>/object/{training,testing}/velodyne/000000.bin  x y z reflectance, f32 (read only with cfg.FRONT_VIEW_INPUT / a 3-view net)

Interface kept from the reference (lib/datasets/kitti_mv3d.py): class `kitti_mv3d(image_set, kitti_path)` with
`image_index`, `num_classes`, `image_path_at`, `lidar_path_at`, `calib_at`, `gt_roidb`, and roidb entries with the same
keys / shapes / dtypes (:274-306); the (4,12) calibration table (:63-75); the gt blobs of
lib/roi_data_layer/minibatch_mv3d.py:47-75.

How it is done here: a frame's label file is parsed as ONE token table (no per-object Python loop); the numbers of the kept
objects go to the device in one upload, `mv3d_gt_encode` (csrc/gt_encode.hip) computes camera corners, LIDAR corners, LIDAR
box and BEV box for all objects at once, and one download brings the four arrays back.  Pinned bit for bit (values and
dtypes) by tests/golden/kitti_label.npz, which the reference's own loader produced.  `evaluate_detections` writes the
reference's result files and scores the detections on the device (datasets/kitti_eval.py); `evaluate_recall` is the base
class's proposal-recall statistics on the device (datasets/proposal_recall.py); `append_flipped_images` appends the
left/right mirror of every frame (datasets/mirror.py); caching is out of scope."""
import os

import numpy as np
import scipy.sparse
import torch

from .. import ops
from ..fast_rcnn.config import cfg, check_ignore_types
from .mirror import mirror_annotation, mirror_calib

# calibration file: the reference reads lines 2..5 by position (:158-168); KITTI writes them in this order
_CALIB_ROWS = ((2, 'P2', (3, 4)), (3, 'P3', (3, 4)), (4, 'R0', (3, 3)), (5, 'Tr_velo2cam', (3, 4)))


def load_kitti_calib(path):
    """{'P2' (3,4), 'P3' (3,4), 'R0' (3,3), 'Tr_velo2cam' (3,4)}, f32, from a KITTI calibration file."""
    with open(path) as f:
        text = f.read().splitlines()
    return {key: np.array(text[row].split()[1:], dtype=np.float32).reshape(shape) for row, key, shape in _CALIB_ROWS}


def pack_calib(c):
    """The (4, 12) table the layers take as `calib`: P2 | P3 | R0 (9 numbers + 3 zeros) | Tr_velo_to_cam, f64 holding the
    f32 file values (what `calib_at` returns in the reference)."""
    table = np.zeros((4, 12))
    for row, key in enumerate(('P2', 'P3', 'R0', 'Tr_velo2cam')):
        flat = c[key].ravel()
        table[row, :flat.size] = flat
    return table


def _device():
    return torch.device("cuda", cfg.GPU_ID)


def parse_kitti_labels(lines, Tr, class_to_ind, num_classes, ignore_types=None):
    """Annotation dict of one frame (roidb entry) from its label lines.  Objects whose type is not a key of `class_to_ind`
    are dropped.  Geometry on the device: `mv3d_gt_encode`.
    ignore_types (not in the reference; cfg.TRAIN.IGNORE_TYPES): a non-empty sequence of KITTI types adds the
    frame's ignore regions -- `ignore_boxes_bv` (K, 4) f32, the `boxes_bv` of the listed types' rows that have a 3D box (h, w, l all
    > 0, which DontCare rows have not), encoded by the same `mv3d_gt_encode` call as the objects; `ignore_boxes_3D` (K, 6), their
    LIDAR boxes (what the mirror needs); `ignore_boxes_img` (M, 4) f32, the image boxes of the listed 'DontCare' rows,
    float32(float64(text)).  None or empty: exactly the keys above."""
    every = [ln.split() for ln in lines if ln.strip()]
    table = [t for t in every if t[0] in class_to_ind]
    G = len(table)
    ign = check_ignore_types(ignore_types, trained=tuple(class_to_ind))
    ign3d = [t for t in every if t[0] in ign and all(float(v) > 0 for v in t[8:11])] if ign else []
    table = table + ign3d                                                             # (one encode call for both; split below)
    cls = np.array([class_to_ind[t[0]] for t in table[:G]], dtype=np.int32).reshape(G)
    # label columns 3..14 (KITTI devkit order: alpha | x1 y1 x2 y2 | h w l | tx ty tz | rotation_y) as the text's floats
    num = np.array([t[3:15] for t in table], dtype=np.float64).reshape(len(table), 12)
    alpha, box2d, hwl, xyz, ry = num[:, 0], num[:, 1:5], num[:, 5:8], num[:, 8:11], num[:, 11]
    lwh = hwl[:, ::-1]
    box_cam = np.ascontiguousarray(np.hstack([xyz, lwh]), dtype=np.float32)          # (tx, ty, tz, l, w, h) f32
    ann = {'ry': ry[:G].astype(np.float32), 'lwh': lwh[:G].astype(np.float32), 'boxes': box2d[:G].astype(np.float32),
           'boxes_3D_cam': box_cam[:G], 'gt_classes': cls, 'xyz': xyz[:G].astype(np.float32), 'alphas': alpha[:G].astype(np.float32),
           'flipped': False}
    onehot = np.zeros((G, num_classes), dtype=np.float32)
    onehot[np.arange(G), cls] = 1.0
    ann['gt_overlaps'] = scipy.sparse.csr_matrix(onehot)
    tr = np.ascontiguousarray(Tr, dtype=np.float32).reshape(3, 4)
    if len(table):
        dev = _device()
        cos_sin = np.stack([np.cos(ry), np.sin(ry)], axis=1)                          # f64, from the text's floats
        inv_rot = np.linalg.inv(tr[:, :3])                                            # f32 (LAPACK), once per frame
        d_box, d_inv, d_tr = ops.upload_packed([box_cam, inv_rot, tr], dev)
        d_cs = torch.from_numpy(np.ascontiguousarray(cos_sin)).to(dev)
        pack, spec, _ = ops.gt_encode(d_box, d_cs, d_inv.reshape(-1), d_tr.reshape(-1))
        cam, lid, box3d, bv = ops.unpack_host(pack, spec)
    else:
        cam, lid = np.zeros((0, 24), np.float32), np.zeros((0, 24), np.float32)
        box3d, bv = np.zeros((0, 6), np.float32), np.zeros((0, 4), np.float32)
    ann.update({'boxes3D_cam_corners': cam[:G], 'boxes_corners': lid[:G], 'boxes_3D': box3d[:G], 'boxes_bv': bv[:G]})
    if ign:
        dc = [t[4:8] for t in every if t[0] == 'DontCare'] if 'DontCare' in ign else []
        ann.update({'ignore_boxes_bv': bv[G:].copy(), 'ignore_boxes_3D': box3d[G:].copy(),
                    'ignore_boxes_img': np.array(dc, dtype=np.float64).reshape(len(dc), 4).astype(np.float32)})
    return ann


def ignore_blobs(entry):
    """(cfg.TRAIN.IGNORE_TYPES) the ignore regions of one roidb entry as blobs: `ignore_boxes_bv` (K, 4) and `ignore_boxes_img` (M, 4)
    f32, what MV3D.forward hands to ops.ignore_relabel.  An entry parsed without ignore_types raises KeyError."""
    return {'ignore_boxes_bv': np.ascontiguousarray(entry['ignore_boxes_bv'], np.float32).reshape(-1, 4),
            'ignore_boxes_img': np.ascontiguousarray(entry['ignore_boxes_img'], np.float32).reshape(-1, 4)}


def gt_blobs(entry, lidar_bv_shape):
    """Ground-truth blobs of one roidb entry: image / BEV / LIDAR boxes and LIDAR corners of the foreground objects, the
    class appended as last column, plus im_info = (BEV rows, BEV columns, 1)."""
    fg = np.flatnonzero(entry['gt_classes'] != 0)
    cls = entry['gt_classes'][fg].astype(np.float32)[:, None]
    blob = lambda key: np.hstack([np.asarray(entry[key], np.float32)[fg], cls]).astype(np.float32)
    return {'gt_boxes': blob('boxes'), 'gt_boxes_bv': blob('boxes_bv'), 'gt_boxes_3d': blob('boxes_3D'),
            'gt_boxes_corners': blob('boxes_corners'),
            'im_info': np.array([[lidar_bv_shape[0], lidar_bv_shape[1], 1]], dtype=np.float32)}


class kitti_mv3d(object):
    """Dataset accessor with the reference class's public face (what train_net / test_net touch)."""

    def __init__(self, image_set, kitti_path):
        self._image_set, self._kitti_path = image_set, kitti_path
        self._data_path = os.path.join(kitti_path, 'object')
        self._classes = ('__background__', 'Car')
        self._class_to_ind = {c: i for i, c in enumerate(self._classes)}
        self._image_ext, self._lidar_ext = '.png', '.npy'
        index_file = os.path.join(kitti_path, 'ImageSets', image_set + '.txt')
        for p, what in ((kitti_path, 'KITTI path'), (self._data_path, 'Path'), (index_file, 'Path')):
            assert os.path.exists(p), '{} does not exist: {}'.format(what, p)
        with open(index_file) as f:
            self._image_index = f.read().split()
        self.name = 'kitti_mv3d_' + image_set
        self._roidb = None
        self._widths = None                                        # image widths of the source frames once the mirrors are appended

    classes = property(lambda self: self._classes)
    num_classes = property(lambda self: len(self._classes))
    image_index = property(lambda self: self._image_index)
    num_images = property(lambda self: len(self._image_index))

    @property
    def roidb(self):
        if self._roidb is None:
            self._roidb = self.gt_roidb()
        return self._roidb

    def _dir(self, sub):
        return os.path.join(self._data_path, 'testing' if self._image_set == 'test' else 'training', sub)

    def _file(self, sub, i, ext):
        p = os.path.join(self._dir(sub), self._image_index[i] + ext)
        assert os.path.exists(p), 'Path does not exist: {}'.format(p)
        return p

    def image_path_at(self, i):
        return self._file('image_2', i, self._image_ext)

    def lidar_path_at(self, i):
        return self._file('lidar_bv', i, self._lidar_ext)

    def velodyne_path_at(self, i):
        """(not in the reference) the frame's raw scan, what the front-view map is rasterised from; a mirrored index names the source
        frame's file, like lidar_path_at.  The file is not looked for here: prepare_roidb records the path for every frame, and a
        tree without scans still serves the two-view model"""
        return os.path.join(self._dir('velodyne'), self._image_index[i] + '.bin')

    def _load_kitti_calib(self, index):
        return load_kitti_calib(os.path.join(self._dir('calib'), index + '.txt'))

    def calib_at(self, i):
        if self._widths is not None and i >= len(self._widths):    # the mirror of frame i - N (append_flipped_images)
            return mirror_calib(self.calib_at(i - len(self._widths)), self._widths[i - len(self._widths)])
        return pack_calib(self._load_kitti_calib('%06d' % i))      # by POSITION, like the reference (kitti_mv3d.py:67)

    def _load_kitti_annotation(self, index):
        with open(os.path.join(self._data_path, 'training', 'label_2', index + '.txt')) as f:
            lines = f.readlines()
        return parse_kitti_labels(lines, self._load_kitti_calib(index)['Tr_velo2cam'], self._class_to_ind, self.num_classes,
                                  ignore_types=cfg.TRAIN.get('IGNORE_TYPES', ()) or None)

    def gt_roidb(self):
        return [self._load_kitti_annotation(index) for index in self._image_index]

    def _write_kitti_results_file(self, all_boxes, path):
        """One <path>/<index>.txt per frame in the reference's line format (lib/datasets/kitti_mv3d.py:345-351): class name in
        lower case, alpha 0, the all_boxes box (the BEV pixel box, as the reference writes it), every other field -1."""
        os.makedirs(path, exist_ok=True)
        for im_ind, index in enumerate(self.image_index):
            with open(os.path.join(path, index + '.txt'), 'wt') as f:
                for cls_ind, cls in enumerate(self.classes):
                    if cls == '__background__':
                        continue
                    dets = all_boxes[cls_ind][im_ind]
                    for k in range(len(dets)):
                        f.write('{:s} -1 -1 {:.2f} {:.2f} {:.2f} {:.2f} {:.2f} -1 -1 -1 -1 -1 -1 -1 -1\n'
                                .format(cls.lower(), 0, dets[k, 0], dets[k, 1], dets[k, 2], dets[k, 3]))
        return path

    def evaluate_detections(self, all_boxes, all_boxes3D, output_dir):
        """Writes <output_dir>/results/data/<index>.txt (the reference writes under ROOT_DIR/kitti/results/<timestamp>
        instead), then scores all_boxes3D (test_net's all_boxes_cnr) against the split's label_2 files: AP_BEV and AP_3D in
        the three KITTI difficulties, printed, written to <output_dir>/kitti_ap.json and returned
        ({(class, 'bev' | '3d', 'easy' | 'moderate' | 'hard'): AP in percent}, datasets/kitti_eval.py); the metrics are
        cfg.TEST.KITTI_EVAL_METRICS ('2d' and 'aos' add AP_2D and AOS)."""
        from .kitti_eval import evaluate_split
        self._write_kitti_results_file(all_boxes, os.path.join(output_dir, 'results', 'data'))
        return evaluate_split(self, all_boxes3D, output_dir, metrics=cfg.TEST.KITTI_EVAL_METRICS)

    def evaluate_recall(self, candidate_boxes=None, thresholds=None, area='all', limit=None, space='bv'):
        """lib/datasets/imdb.py:121 on the device (datasets/proposal_recall.py): recall of `candidate_boxes` (per-frame boxes in
        proposal order, or what rpn_msr.generate.imdb_proposals returns) against this split's objects, in BEV ('bv') or in the
        image ('image').  candidate_boxes=None takes the roidb's own class-0 boxes as the reference does; this roidb has none."""
        from .proposal_recall import evaluate_recall
        return evaluate_recall(self.roidb, candidate_boxes, thresholds=thresholds, area=area, limit=limit, space=space)

    def evaluate_recall_3d(self, candidate_boxes, thresholds=None, area='all', limit=None, metric='3d', on_short='raise'):
        """Recall of 3D proposals by oriented BEV / 3D IoU against this split's `boxes_corners` (datasets/proposal_recall_3d.py):
        `candidate_boxes` are per-frame (R, 6) x y z l w h rows or (R, 24) corners in proposal order, or what
        rpn_msr.generate.imdb_proposals(..., with_3d=True) returns; the objects are those `evaluate_recall(space='bv')` selects."""
        from .proposal_recall_3d import evaluate_recall_3d
        return evaluate_recall_3d(self.roidb, candidate_boxes, thresholds=thresholds, area=area, limit=limit, metric=metric,
                                  on_short=on_short)

    def append_flipped_images(self):
        """cfg.TRAIN.USE_FLIPPED (lib/datasets/imdb.py:104-121): appends the left/right mirror of every frame -- roidb[N + i] =
        mirror_annotation(roidb[i], width of image i) (datasets/mirror.py: image boxes AND BEV / 3-D ground truth, where the
        reference mirrors the image boxes only) -- and doubles the image index, so that `image_path_at` / `lidar_path_at` of a
        mirror name the source frame's files and `calib_at` gives its mirrored table.  Only the image files' headers are read;
        the data layer mirrors the maps on the device when it loads them (`flipped` entries, roi_data_layer/minibatch_mv3d.py).
        The evaluators (`evaluate_detections`, `evaluate_recall*`) on a doubled imdb are out of scope, as in the reference: a
        doubled imdb is for training.  A second call raises."""
        if self._widths is not None:
            raise RuntimeError("append_flipped_images: the mirrored frames have been appended already")
        roidb = self.roidb
        n = self.num_images
        assert len(roidb) == n
        widths = [_image_width(self.image_path_at(i)) for i in range(n)]
        roidb.extend(mirror_annotation(roidb[i], widths[i]) for i in range(n))
        self._image_index = self._image_index * 2
        self._widths = widths


def _image_width(path):
    """width in pixels from the file's header (the pixel data is not read)"""
    if path.endswith('.npy'):
        return int(np.load(path, mmap_mode='r').shape[1])
    from PIL import Image
    with Image.open(path) as im:
        return int(im.size[0])
