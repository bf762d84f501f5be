"""cfg.TRAIN.USE_FLIPPED through the training entry chain: kitti_mv3d.append_flipped_images on a KITTI tree
with real PNG images of two widths and 601 x 601 x 9 BEV maps, the blobs get_minibatch returns for a mirrored frame, and
get_training_roidb -> filter_roidb -> train_net / train_model on the doubled roidb (a step whose two frames are a frame and its
mirror stacks a numpy map and a device tensor)."""
import os

import numpy as np
import pytest

from conftest import golden
from test_kitti_formats import ANN_KEYS, _same, _tree

pytestmark = pytest.mark.gpu

WIDTHS = (320, 308, 320)            # image widths of the tree's three frames
HEIGHT = 96


@pytest.fixture(scope="module")
def flipped_db(tmp_path_factory):
    """(imdb with the mirrors appended, its prepared roidb, n, the frames' (image BGR u8, BEV map) arrays)"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from PIL import Image
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd.datasets import kitti_mv3d
    from mv3d_tf_amd.fast_rcnn import train_mv
    from mv3d_tf_amd.fast_rcnn.config import cfg
    g = golden("kitti_label")
    root, n = _tree(tmp_path_factory.mktemp("flipped"), g)
    rng = np.random.RandomState(0)
    frames = []
    for i in range(n):
        rgb = rng.randint(0, 255, (HEIGHT, WIDTHS[i], 3)).astype(np.uint8)
        Image.fromarray(rgb).save(os.path.join(root, "object/training/image_2/%06d.png" % i))
        bev = ((rng.random_sample((601, 601, 9)) < 0.02) * rng.uniform(0.1, 2.4, (601, 601, 9))).astype(np.float32)
        np.save(os.path.join(root, "object/training/lidar_bv/%06d.npy" % i), bev)
        frames.append((rgb[:, :, ::-1], bev))
    db = kitti_mv3d("train", root)
    saved = cfg.TRAIN.USE_FLIPPED
    cfg.TRAIN.USE_FLIPPED = True
    try:
        roidb = train_mv.get_training_roidb(db)
    finally:
        cfg.TRAIN.USE_FLIPPED = saved
    return db, roidb, n, frames, root


def test_append_flipped_images_doubles_the_imdb(flipped_db):
    from mv3d_tf_amd.datasets import kitti_mv3d, mirror_annotation, mirror_calib
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    db, roidb, n, _, root = flipped_db
    assert db.num_images == 2 * n == len(roidb) == len(db.roidb) and db.image_index == ["%06d" % i for i in range(n)] * 2
    plain = kitti_mv3d("train", root)
    source = plain.gt_roidb()
    for i in range(n):
        want = mirror_annotation(source[i], WIDTHS[i])
        assert roidb[i]["flipped"] is False and roidb[n + i]["flipped"] is True
        for k in ANN_KEYS:
            a, b = (x[k].toarray() if k == "gt_overlaps" else x[k] for x in (roidb[n + i], want))
            assert _same(a, b), (i, k)
            assert _same(roidb[i][k].toarray() if k == "gt_overlaps" else roidb[i][k],
                         source[i][k].toarray() if k == "gt_overlaps" else source[i][k]), (i, k)      # the source entry stays
        assert _same(db.calib_at(n + i), mirror_calib(plain.calib_at(i), WIDTHS[i])) and _same(db.calib_at(i), plain.calib_at(i))
        assert _same(roidb[n + i]["calib"], db.calib_at(n + i))
        assert db.image_path_at(n + i) == db.image_path_at(i) == roidb[n + i]["image_path"]
        assert db.lidar_path_at(n + i) == db.lidar_path_at(i) == roidb[n + i]["lidar_bv_path"]
    assert not _same(db.calib_at(n), db.calib_at(n + 1))                                    # two widths, two mirrored P2
    with pytest.raises(RuntimeError):
        db.append_flipped_images()
    assert db.num_images == 2 * n and len(db.roidb) == 2 * n
    # a mirrored frame needs the 601 wide raster: 608 columns are refused by name
    wide = dict(roidb[n], lidar_bv=np.zeros((608, 608, 9), np.float32))
    with pytest.raises(ValueError, match="608"):
        get_minibatch([wide], db.num_classes)
    assert get_minibatch([dict(wide, flipped=False)], db.num_classes)["lidar_bv_data"].shape == (1, 608, 608, 9)


def test_blobs_of_a_mirrored_frame(flipped_db):
    import torch
    from mv3d_tf_amd.datasets import gt_blobs, mirror_calib
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    db, roidb, n, frames, _ = flipped_db
    bits = lambda a: (a.view(torch.int32).cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a).view(np.int32))
    for i in range(n):
        np.random.seed(7 + i)
        plain = get_minibatch([roidb[i]], db.num_classes)
        state_plain = np.random.get_state()
        np.random.seed(7 + i)
        flip = get_minibatch([roidb[n + i]], db.num_classes)
        state_flip = np.random.get_state()
        assert all(np.array_equal(a, b) for a, b in zip(state_plain[1:], state_flip[1:]))    # the same draw from the global RNG
        assert set(plain) == set(flip)
        for k in ("image_data", "lidar_bv_data"):
            assert isinstance(plain[k], np.ndarray) and plain[k].dtype == np.float32
            assert isinstance(flip[k], torch.Tensor) and flip[k].is_cuda and flip[k].dtype == torch.float32 and flip[k].is_contiguous()
            assert np.array_equal(bits(flip[k]), bits(plain[k][:, :, ::-1, :])), (i, k)
        img, bev = frames[i]
        assert _same(plain["image_data"][0], (img.astype(np.float32) - cfg.PIXEL_MEANS).astype(np.float32))
        assert _same(plain["lidar_bv_data"][0], bev)
        want = gt_blobs(roidb[n + i], (601, 601, 9))
        for k in ("gt_boxes", "gt_boxes_bv", "gt_boxes_3d", "gt_boxes_corners", "im_info"):
            assert _same(flip[k], want[k]), (i, k)
        assert _same(flip["calib"], mirror_calib(plain["calib"], WIDTHS[i]))
        if len(plain["gt_boxes_3d"]):
            assert np.array_equal(flip["gt_boxes_3d"][:, 1], -plain["gt_boxes_3d"][:, 1])


def test_stack_and_group_frames_with_device_maps(flipped_db):
    import torch
    from mv3d_tf_amd.fast_rcnn import train_mv
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    db, roidb, n, _, _ = flipped_db
    a, a_m, b = (get_minibatch([roidb[i]], db.num_classes) for i in (0, n, 1))
    groups = train_mv.group_frames_by_shape([a, b, a_m])
    assert [len(grp) for grp in groups] == [2, 1] and groups[0][0] is a and groups[0][1] is a_m      # by size, order kept
    feed = train_mv.stack_blobs(groups[0])
    for k in ("image_data", "lidar_bv_data"):
        assert isinstance(feed[k], torch.Tensor) and feed[k].is_cuda and feed[k].shape[0] == 2
        assert np.array_equal(feed[k][0].cpu().numpy(), a[k][0]) and torch.equal(feed[k][1], a_m[k][0])
    assert feed["calib"].shape == (2, 4, 12) and len(feed["gt_boxes_3d"]) == 2
    plain = train_mv.stack_blobs([a, a])                                                     # all numpy: numpy, as before
    assert isinstance(plain["image_data"], np.ndarray) and plain["image_data"].shape[0] == 2
    assert train_mv.stack_blobs([a_m])["image_data"] is a_m["image_data"]


def test_use_flipped_training_chain(flipped_db, tmp_path, monkeypatch):
    """get_training_roidb (USE_FLIPPED) -> filter_roidb -> train_net for two iterations, then ONE train_model step of two frames
    that are a frame and its mirror: a numpy map and a device tensor in one stack"""
    from mv3d_tf_amd.fast_rcnn import train_mv
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.networks import get_network
    db, roidb, n, _, _ = flipped_db
    assert len(roidb) == 2 * n
    kept = train_mv.filter_roidb(roidb)
    assert 0 < len(kept) < 2 * n and len(kept) % 2 == 0                 # the frame without a known class goes, with its mirror
    assert sum(e["flipped"] for e in kept) == len(kept) // 2
    saved = (cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.DISPLAY, cfg.TRAIN.MFMA_TRUNK)
    # (the trunks on this library's exact-f32 kernels: the vendor library's search for a convolution algorithm, run once per new
    # map size and batch, would be most of this test's time; snapshots have their own test)
    cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.DISPLAY, cfg.TRAIN.MFMA_TRUNK = 1, 1, True
    monkeypatch.setattr(train_mv.SolverWrapper, "snapshot", lambda self, sess, it: None)
    stacks = []
    stack_blobs = train_mv.stack_blobs
    monkeypatch.setattr(train_mv, "stack_blobs", lambda frames: stacks.append([type(f["image_data"]) for f in frames]) or stack_blobs(frames))
    try:
        net = get_network("MV3D_train")
        np.random.seed(cfg.RNG_SEED)
        hist = train_mv.train_net(net, db, roidb, str(tmp_path / "out"), max_iters=2)
        assert len(hist) == 2 and all(np.isfinite(h).all() for h in hist)
        # the data layer over [frame, mirror] shuffles before its second frame: a seed whose two draws differ
        pair = [roidb[0], roidb[n]]
        for seed in range(64):
            np.random.seed(seed)
            first = np.random.permutation(np.arange(2))[0]
            np.random.randint(0, high=len(cfg.TRAIN.SCALES), size=1)
            if np.random.permutation(np.arange(2))[0] != first:
                break
        del stacks[:]
        sw = train_mv.SolverWrapper(None, None, net, db, pair, str(tmp_path / "out2"))
        np.random.seed(seed)
        hist = sw.train_model(None, 1, frames_per_step=2)
        assert len(hist) == 1 and np.isfinite(hist[0]).all()
        assert len(stacks) == 1 and sorted(t.__name__ for t in stacks[0]) == ["Tensor", "ndarray"]
    finally:
        cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.DISPLAY, cfg.TRAIN.MFMA_TRUNK = saved
