"""Front-view input: ops.point_cloud_2_front / mv3d_point_cloud_2_front against the host restatement
(tests/front_view_raster_restatement.py), and the layers that feed `lidar_fv_data` from Velodyne scans.  PARITY UNPINNED: the reference
has no front view, the definition is this repository's.  Every comparison is np.array_equal; nothing has a tolerance."""
import os

import numpy as np
import pytest

import front_view_raster_restatement as R

F32 = np.float32
P_GROUP = 256                      # threads per workgroup of the point kernel (csrc/front_view_raster.hip)


def random_cloud(seed=0, P=4096):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-5, 70, P); y = rng.uniform(-40, 40, P); z = rng.uniform(-2.6, 1.0, P)
    return np.stack([x, y, z, rng.random_sample(P)], 1).astype(F32)


@pytest.fixture(scope="module")
def cloud(oracle):
    """the seeded random cloud, its projection and its map by the restatement: computed once, never written to"""
    pts = random_cloud()
    proj = R.project(pts, oracle)
    fv, win = R.raster(pts, oracle, proj)
    for a in (pts, fv, win) + proj:
        a.setflags(write=False)
    return {"pts": pts, "proj": proj, "fv": fv, "win": win}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops
    return {"torch": torch, "ops": ops}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def device_map(gpu, pts, **kw):
    out = gpu["ops"].point_cloud_2_front(gpu["torch"].from_numpy(np.array(pts, F32)).cuda(), **kw)
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- CPU
def test_restatement_pixels_are_the_roi_projections(cloud, oracle):
    """every in-window point of the random cloud: (col, row) of the restatement == oracle.rois_3d_to_fv of the zero-size box there"""
    pts, (keep, col, row, d) = cloud["pts"], cloud["proj"]
    assert 0.5 < keep.mean() < 0.8
    boxes = np.zeros((int(keep.sum()), 7), F32)
    boxes[:, 1:4] = pts[keep, :3]
    fv = oracle.rois_3d_to_fv(boxes)
    want = np.stack([np.zeros(len(boxes)), col[keep], row[keep], col[keep], row[keep]], 1).astype(F32)
    assert np.array_equal(fv, want)
    assert (d[keep] > 0).all()
    rng = np.random.RandomState(1)
    for a, b, c in np.concatenate([x_ * 10.0 ** rng.randint(-30, 30, (2000, 3)) for x_ in (rng.standard_normal((2000, 3)),)]).tolist() + \
            [(3.0, 1.0 / 3.0, -1.0), (1e308, 1.0, -1e308), (2.0 ** -600, 2.0 ** -600, 0.0), (0.1, 0.1, -0.010000000000000002)]:
        assert R.fma_ints(a, b, c) == R.fma(a, b, c)
    # for f32 inputs both products are exact in f64, so the two fma of the distance are plain f64 sums: the slow exact form agrees
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    assert np.array_equal(np.sqrt(z * z + (x * x + y * y)).astype(F32)[keep], d[keep])


def _entry(**extra):
    e = {"image": np.zeros((8, 12, 3), np.uint8), "lidar_bv": np.zeros((8, 601, 9), F32), "calib": np.zeros((4, 12)),
         "gt_classes": np.zeros((0,), np.int32), "boxes": np.zeros((0, 4), F32), "boxes_bv": np.zeros((0, 4), F32),
         "boxes_3D": np.zeros((0, 6), F32), "boxes_corners": np.zeros((0, 24), F32), "flipped": False}
    e.update(extra)
    return e


def test_key_defaults_off_and_blobs_are_unchanged():
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    assert cfg.FRONT_VIEW_INPUT is False
    blobs = get_minibatch([_entry(velodyne=random_cloud(1, 16))], 2)
    assert set(blobs) == {"image_data", "lidar_bv_data", "calib", "gt_boxes", "gt_boxes_bv", "gt_boxes_3d", "gt_boxes_corners", "im_info"}


def _kitti_tree(root, n=2):
    from PIL import Image
    for sub in ("ImageSets", "object/training/calib", "object/training/label_2", "object/training/image_2", "object/training/lidar_bv",
                "object/training/velodyne"):
        os.makedirs(os.path.join(root, sub))
    rows = ["P%d: " % k + " ".join(["1.0"] * 12) for k in range(4)] + ["R0_rect: " + " ".join(["1.0"] * 9)] + \
           [name + ": " + " ".join(["1.0"] * 12) for name in ("Tr_velo_to_cam", "Tr_imu_to_velo")]
    for i in range(n):
        idx = "%06d" % i
        with open(os.path.join(root, "object/training/calib", idx + ".txt"), "w") as f:
            f.write("\n".join(rows) + "\n")
        open(os.path.join(root, "object/training/label_2", idx + ".txt"), "w").close()            # no objects: nothing for the device
        Image.fromarray(np.zeros((4, 6 + i, 3), np.uint8)).save(os.path.join(root, "object/training/image_2", idx + ".png"))
        np.save(os.path.join(root, "object/training/lidar_bv", idx + ".npy"), np.zeros((2, 2, 9), F32))
    with open(os.path.join(root, "ImageSets", "train.txt"), "w") as f:
        f.write("\n".join("%06d" % i for i in range(n)) + "\n")
    return root


def test_velodyne_path_at_and_prepare_roidb(tmp_path):
    from mv3d_tf_amd.datasets.kitti_mv3d import kitti_mv3d
    from mv3d_tf_amd.roi_data_layer.roidb import prepare_roidb
    root = _kitti_tree(str(tmp_path / "kitti"))
    db = kitti_mv3d("train", root)
    want = [os.path.join(root, "object", "training", "velodyne", "%06d.bin" % i) for i in range(2)]
    assert [db.velodyne_path_at(i) for i in range(2)] == want
    db.append_flipped_images()
    assert [db.velodyne_path_at(i) for i in range(4)] == want * 2                  # a mirror names its source frame's scan
    roidb = prepare_roidb(db)
    assert [e["velodyne_path"] for e in roidb] == want * 2 and [e["flipped"] for e in roidb] == [False, False, True, True]

    class NoScans:                                                                   # an imdb without the method: no key
        roidb = [{"gt_overlaps": np.zeros((0, 2), F32)}]
        image_path_at = lidar_path_at = calib_at = staticmethod(lambda i: None)

    assert "velodyne_path" not in prepare_roidb(NoScans())[0]
    with open(os.path.join(root, "ImageSets", "test.txt"), "w") as f:
        f.write("000007\n")
    assert kitti_mv3d("test", root).velodyne_path_at(0) == os.path.join(root, "object", "testing", "velodyne", "000007.bin")


def test_point_cloud_2_front_refuses_bad_arguments_before_any_launch():
    import torch
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops
    good = np.zeros((3, 4), F32)
    for exc, args in ((TypeError, (np.zeros((3, 4)),)), (TypeError, (np.zeros((3, 4), np.int32),)), (TypeError, (torch.zeros(3, 4, dtype=torch.float16),)),
                      (ValueError, (np.zeros((3, 3), F32),)), (ValueError, (np.zeros((12,), F32),)), (ValueError, (torch.zeros(3, 4),)),
                      (TypeError, (good, [0.0, 3.0])), (TypeError, (good, torch.zeros(2, dtype=torch.int64))),
                      (ValueError, (good, [0, 2, 1])), (ValueError, (good, [0, 4])), (ValueError, (good, [-1, 3])), (ValueError, (good, [[0, 3]])),
                      (ValueError, (good, [0])), (ValueError, (good, np.zeros(ops.FV_MAX_FRAMES + 2, np.int32))),
                      (ValueError, (good, torch.zeros(2, dtype=torch.int32))),
                      (TypeError, (good, None, np.zeros(ops.FV_SHAPE, F32))), (TypeError, (good, None, torch.zeros(ops.FV_SHAPE, dtype=torch.float64))),
                      (ValueError, (good, None, torch.zeros(ops.FV_SHAPE))),
                      (TypeError, (good, None, None, torch.zeros(1 << 18))), (ValueError, (good, None, None, torch.zeros(1 << 18, dtype=torch.uint8)))):
        with pytest.raises(exc, match="point_cloud_2_front"):
            ops.point_cloud_2_front(*args)
    L, lib = ops.lib(), ops._lib
    A = 4096                                                                         # a non-NULL, aligned "pointer" (never dereferenced)
    assert L.mv3d_point_cloud_2_front_workspace(1) == 64 * 512 * 8 and L.mv3d_point_cloud_2_front_workspace(16) == 16 * 64 * 512 * 8
    assert L.mv3d_point_cloud_2_front_workspace(0) == 0 and L.mv3d_point_cloud_2_front_workspace(ops.FV_MAX_FRAMES + 1) == 0
    for args in ((A, A, -1, 4, A, A), (A, A, ops.FV_MAX_FRAMES + 1, 4, A, A), (A, A, 1, -1, A, A), (None, A, 1, 4, A, A),
                 (A, None, 2, 4, A, A), (A, A, 1, 4, None, A), (A, A, 1, 4, A, None), (A + 4, A, 1, 4, A, A), (A, A + 2, 1, 4, A, A),
                 (A, A, 1, 4, A + 8, A), (A, A, 1, 4, A, A + 8)):
        assert L.mv3d_point_cloud_2_front(*args, None) == lib.ERR_INVALID_ARG, args
    assert L.mv3d_point_cloud_2_front(None, None, 0, 0, None, None, None) == lib.OK  # no frame: nothing to do


class _ThreeViewStub:
    views = 3

    def forward(self, feed):
        raise AssertionError("no forward may run")


def test_three_view_paths_refuse_a_missing_front_view_before_any_work(tmp_path):
    from mv3d_tf_amd.fast_rcnn import detect_batch, train_mv
    from mv3d_tf_amd.fast_rcnn.config import cfg
    net = _ThreeViewStub()
    assert cfg.FRONT_VIEW_INPUT is False
    with pytest.raises(ValueError, match="FRONT_VIEW_INPUT"):
        train_mv.train_net(net, None, None, str(tmp_path / "out"), max_iters=1)

    class Imdb:                                                                      # neither points_at nor velodyne_path_at
        name, num_classes, image_index = "no_scans", 2, ["000000"]

        def image_at(self, i):
            raise AssertionError("no frame may be loaded")

    saved, root = dict(cfg.TEST), cfg.ROOT_DIR
    cfg.ROOT_DIR = str(tmp_path)
    try:
        for batch in (1, 4):
            cfg.TEST.BATCH_SIZE = batch
            with pytest.raises(ValueError, match="velodyne_path_at"):
                detect_batch.test_net(None, net, Imdb(), "w")
    finally:
        cfg.TEST.update(saved)
        cfg.ROOT_DIR = root
    assert not os.path.exists(str(tmp_path / "output")) and not os.path.exists(str(tmp_path / "out"))
    with pytest.raises(ValueError, match="fv="):
        detect_batch.box_detect(None, net, np.zeros((8, 12, 3), np.uint8), np.zeros((16, 24, 9), F32), np.zeros((4, 12)))
    assert detect_batch.front_view_source(object(), Imdb()) is None                      # a two-view network: no source is asked for


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("P", [0, 1, P_GROUP - 1, P_GROUP, P_GROUP + 1])
def test_counts(gpu, oracle, P):
    rng = np.random.RandomState(10 + P)
    pts = np.stack([rng.uniform(5, 60, P), rng.uniform(-4, 4, P), rng.uniform(-2, 0.1, P), rng.random_sample(P)], 1).astype(F32)
    if P:
        pts[-1, :3] = (3.0, 2.5, -0.25)                                               # the last point, nearer than any other: it must show
    got = device_map(gpu, pts)
    want, win = R.raster(pts, oracle)
    assert got.shape == (64, 512, 3) and got.dtype == F32
    assert np.array_equal(bits(got), bits(want))
    assert win.max() == P - 1 and (P > 0 or not got.any())


@pytest.mark.gpu
def test_random_cloud(gpu, cloud):
    keep, col, row, _ = cloud["proj"]
    hits = np.bincount(row[keep] * R.W + col[keep], minlength=R.H * R.W)
    assert (hits > 1).sum() >= 100, "the input must make points collide"
    got = device_map(gpu, cloud["pts"])
    assert np.array_equal(bits(got), bits(cloud["fv"]))
    assert np.array_equal(got[..., 1] == 0, cloud["win"] < 0)                         # distance 0 <=> empty, nothing else
    again = device_map(gpu, cloud["pts"])                                             # scheduling must not matter
    assert np.array_equal(bits(got), bits(again))


@pytest.mark.gpu
def test_winner_rules(gpu, oracle):
    rng = np.random.RandomState(3)
    # (a) 64 points along one ray at different ranges, shuffled: the nearest wins
    ray = R.point_at(200, 30)[None] * rng.uniform(5, 60, 64)[:, None]
    a = np.concatenate([ray, rng.random_sample((64, 1))], 1).astype(F32)
    keep, col, row, d = R.project(a, oracle)
    assert keep.all() and (col == 200).all() and (row == 30).all() and len(set(d.tolist())) == 64
    fv, win = R.raster(a, oracle, (keep, col, row, d))
    assert win[30, 200] == int(np.argmin(d)) and (win >= 0).sum() == 1
    assert np.array_equal(bits(device_map(gpu, a)), bits(fv))
    # (b) one point ten times with ten reflectances: the last wins
    b = np.repeat(a[:1], 10, 0)
    b[:, 3] = np.arange(10, dtype=F32) / 16
    fv, win = R.raster(b, oracle)
    assert win[30, 200] == 9
    got = device_map(gpu, b)
    assert np.array_equal(bits(got), bits(fv)) and got[30, 200, 2] == F32(9 / 16)
    # (c) radial scalings p (1 + k 2^-24): neighbours round to one f32 distance, the last of the nearest ones wins
    clouds = []
    for j in range(16):
        base = R.point_at(40 + 25 * j, 8 + 3 * j) * rng.uniform(5, 60)
        k = rng.permutation(16)
        clouds.append(np.concatenate([base[None] * (1.0 + k[:, None] * 2.0 ** -24), rng.random_sample((16, 1))], 1))
    c = np.concatenate(clouds).astype(F32)
    keep, col, row, d = R.project(c, oracle)
    fv, win = R.raster(c, oracle, (keep, col, row, d))
    assert keep.all()
    tied = 0
    for r_, c_ in zip(*np.nonzero(win >= 0)):
        same = np.flatnonzero((row == r_) & (col == c_))
        nearest = same[d[same] == d[same].min()]
        assert win[r_, c_] == nearest.max()
        tied += len(nearest) > 1 and len({tuple(p) for p in c[nearest, :3].tolist()}) > 1
    assert tied >= 1, "no pixel has two different points at its smallest distance: the tie rule is not exercised"
    assert np.array_equal(bits(device_map(gpu, c)), bits(fv))


def _edge_points():
    """(name, point, kept?) -- kept is what the definition says, asserted from the restatement before the device is asked"""
    f = F32
    up = lambda v: np.nextafter(f(v), f(np.inf))
    dn = lambda v: np.nextafter(f(v), f(-np.inf))
    top, bottom = f(10 * np.tan(np.radians(2.0))), f(10 * np.tan(np.radians(2.0 - 26.9)))
    pts = [("y = x: column 0", (12.5, 12.5, -1.0), True), ("y = -x: column 512", (12.5, -12.5, -1.0), False),
           ("just inside -45 deg", (12.5, up(-12.5), -1.0), True), ("just outside +45 deg", (12.5, up(12.5), -1.0), False),
           ("x < 0", (-10.0, 1.0, -1.0), False), ("x < 0 on the axis", (-10.0, 0.0, -1.0), False),
           ("x = 0, y > 0", (0.0, 5.0, -1.0), False), ("y = 0", (7.0, 0.0, -0.5), True), ("y = -0", (7.0, -0.0, -0.5), True)]
    for name, z in (("top", top), ("bottom", bottom)):
        pts += [("%s limit %s" % (name, s), (10.0, 0.0, v), None) for s, v in (("below", dn(z)), ("on", z), ("above", up(z)))]
    pts += [("(0, 0, %g)" % z, (0.0, 0.0, z), False) for z in (0.0, 1.0, -1.0)] + [("(-0, 0, 1)", (-0.0, 0.0, 1.0), False)]
    for k, axis in enumerate("xyz"):
        for bad in (np.nan, np.inf, -np.inf):
            p = [10.0, 1.0, -1.0]
            p[k] = bad
            pts.append(("%s = %s" % (axis, bad), tuple(p), False))
    return pts


@pytest.mark.gpu
def test_window_and_drop_rules(gpu, oracle):
    cases = _edge_points()
    pts = np.array([p + (0.25 + 0.01 * i,) for i, (_, p, _) in enumerate(cases)], F32)
    keep, col, row, d = R.project(pts, oracle)
    for i, (name, _, kept) in enumerate(cases):
        if kept is not None:
            assert keep[i] == kept, name
    names = [n for n, _, _ in cases]
    assert col[names.index("y = x: column 0")] == 0 and col[names.index("just inside -45 deg")] == 511
    lim = {n: keep[names.index(n)] for n in names if "limit" in n}
    assert lim["top limit below"] and not lim["top limit above"] and lim["bottom limit above"] and not lim["bottom limit below"]
    assert row[names.index("top limit below")] == 0 and row[names.index("bottom limit above")] == 63
    # every point as a frame of its own (nothing can hide behind a neighbour), then all of them as one cloud
    n = len(pts)
    got = device_map(gpu, pts, offsets=np.arange(n + 1))
    want = R.raster_batch(pts, np.arange(n + 1), oracle)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(got.reshape(n, -1).any(1), keep)
    assert not got[names.index("x = inf")][4, 256].any()                                # where +inf would land without the rule
    assert np.array_equal(bits(device_map(gpu, pts)), bits(R.raster(pts, oracle)[0]))
    # reflectance takes no part: a NaN (with a payload) on the winner is copied through
    nan = np.array([0x7FC12345], np.uint32).view(F32)[0]
    w = np.array([[20, 1, -1, 0.5], [10, 0.5, -0.5, nan], [30, 1.5, -1.5, 0.7]], F32)
    w[1, 2] = np.array([0xBF000001], np.uint32).view(F32)[0]
    want, win = R.raster(w, oracle)
    assert (win == 1).sum() == 1
    got = device_map(gpu, w)
    assert np.array_equal(bits(got), bits(want))
    r_, c_ = (int(v[0]) for v in np.nonzero(win == 1))
    assert bits(got[r_, c_, 2:3])[0] == 0x7FC12345 and bits(got[r_, c_, 0:1])[0] == 0xBF000001


@pytest.mark.gpu
def test_contention(gpu, oracle):
    """70 000 points on an 8 x 8 block of pixels (more than a thousand per pixel)"""
    rng = np.random.RandomState(5)
    P = 70000
    pc, pr = 300 + rng.randint(0, 8, P), 20 + rng.randint(0, 8, P)
    frac = rng.uniform(0.25, 0.75, P)
    theta = R.THETA_MAX - (pc + frac) * R.DTHETA
    phi = R.PHI_TOP - (pr + rng.uniform(0.25, 0.75, P)) * R.DPHI
    rr = rng.uniform(5, 60, P)
    pts = np.stack([rr * np.cos(phi) * np.cos(theta), rr * np.cos(phi) * np.sin(theta), rr * np.sin(phi), rng.random_sample(P)], 1).astype(F32)
    pts[P // 2:P // 2 + 2000, :3] = pts[:2000, :3]                                    # exact ties, later index
    pc[P // 2:P // 2 + 2000], pr[P // 2:P // 2 + 2000] = pc[:2000], pr[:2000]
    keep, col, row, d = R.project(pts, oracle, fma=R.fma_ints)
    assert keep.all() and np.array_equal(col, pc) and np.array_equal(row, pr)
    want, win = R.raster(pts, oracle, (keep, col, row, d))
    assert (win >= 0).sum() == 64 and np.bincount(row * R.W + col).max() > 1000
    got = device_map(gpu, pts)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.gpu
def test_batch_and_out(gpu, cloud, oracle):
    torch, ops = gpu["torch"], gpu["ops"]
    pts = cloud["pts"][:2500]
    offsets = np.array([0, 1000, 1000, 2500], np.int32)
    got = device_map(gpu, pts, offsets=offsets)
    assert got.shape == (3, 64, 512, 3)
    singles = [device_map(gpu, pts[offsets[b]:offsets[b + 1]]) for b in range(3)]
    assert np.array_equal(bits(got), bits(np.stack(singles))) and not got[1].any() and got[0].any() and got[2].any()
    assert np.array_equal(bits(got), bits(R.raster_batch(pts, offsets, oracle)))
    d_pts = torch.from_numpy(np.array(pts)).cuda()
    assert np.array_equal(bits(ops.point_cloud_2_front(d_pts, offsets=torch.from_numpy(offsets).cuda()).cpu().numpy()), bits(got))
    big = torch.full((5, 64, 512, 3), -7.0, device="cuda")
    ws = torch.empty(ops.point_cloud_2_front_workspace_bytes(3) + 64, dtype=torch.uint8, device="cuda")
    ws.fill_(0xAB)
    out = ops.point_cloud_2_front(d_pts, offsets=offsets, out=big[1:4], workspace=ws[:-64])
    assert out.data_ptr() == big[1:4].data_ptr()
    host = big.cpu().numpy()
    assert np.array_equal(bits(host[1:4]), bits(got)) and (host[0] == -7).all() and (host[4] == -7).all()
    assert (ws[-64:] == 0xAB).all()
    with pytest.raises(ValueError, match="out must be"):
        ops.point_cloud_2_front(d_pts, offsets=offsets, out=big[1:3])
    with pytest.raises(ValueError, match="contiguous"):
        ops.point_cloud_2_front(d_pts, out=torch.zeros((64, 3, 512), device="cuda").transpose(1, 2))
    with pytest.raises(ValueError, match="workspace of"):
        ops.point_cloud_2_front(d_pts, offsets=offsets, workspace=ws[:1 << 18])


@pytest.mark.gpu
def test_capture_and_replay(gpu, cloud):
    torch, ops = gpu["torch"], gpu["ops"]
    first, second = cloud["pts"][:2048], cloud["pts"][2048:]
    offsets = torch.tensor([0, 700, 2048], dtype=torch.int32, device="cuda")
    buf = torch.from_numpy(first).cuda()
    out, out2 = torch.zeros((64, 512, 3), device="cuda"), torch.zeros((2, 64, 512, 3), device="cuda")
    ws = torch.empty(ops.point_cloud_2_front_workspace_bytes(2), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.point_cloud_2_front(buf, out=out, workspace=ws)                           # (warm-up: the code object is loaded outside the capture)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.point_cloud_2_front(buf, out=out, workspace=ws)
        ops.point_cloud_2_front(buf, offsets=offsets, out=out2, workspace=ws)
    for pts in (first, second):
        buf.copy_(torch.from_numpy(pts))
        out.fill_(-1.0); out2.fill_(-1.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(device_map(gpu, pts)))
        assert np.array_equal(bits(out2.cpu().numpy()), bits(device_map(gpu, pts, offsets=np.array([0, 700, 2048]))))


@pytest.mark.gpu
def test_get_minibatch_feeds_the_front_view(gpu, cloud, oracle, tmp_path):
    torch = gpu["torch"]
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    from mv3d_tf_amd.utils import read_lidar
    pts = cloud["pts"]
    path = str(tmp_path / "000000.bin")
    pts.tofile(path)
    np.save(str(tmp_path / "000001.npy"), pts[:512])
    # a mirrored frame: the cloud plus a point ON the window's left edge (y = x, column 0), whose mirror (y = -x, column 512) is outside
    edged = np.concatenate([pts, np.array([[12.5, 12.5, -1.0, 0.5]], F32)])
    want_mirror = R.raster(edged * np.array([1, -1, 1, 1], F32), oracle)[0]
    assert not np.array_equal(want_mirror, R.raster(edged, oracle)[0][:, ::-1])       # the reversed map is NOT the mirrored scene's
    edged_path = str(tmp_path / "000002.bin")
    edged.tofile(edged_path)
    own = np.random.RandomState(2).random_sample((64, 512, 3)).astype(F32)
    saved = cfg.FRONT_VIEW_INPUT
    cfg.FRONT_VIEW_INPUT = True
    try:
        for entry, want in ((_entry(velodyne_path=path), cloud["fv"]), (_entry(velodyne=pts), cloud["fv"]),
                            (_entry(velodyne_path=str(tmp_path / "000001.npy")), R.raster(pts[:512], oracle)[0]),
                            (_entry(velodyne=pts, velodyne_path="/nowhere.bin"), cloud["fv"]),
                            (_entry(velodyne_path=edged_path, flipped=True), want_mirror), (_entry(velodyne=edged, flipped=True), want_mirror),
                            (_entry(lidar_fv=own, velodyne=pts), own), (_entry(lidar_fv=own, velodyne=pts, flipped=True), own)):
            blobs = get_minibatch([entry], 2)
            fv = blobs["lidar_fv_data"]
            assert isinstance(fv, torch.Tensor) and fv.is_cuda and tuple(fv.shape) == (1, 64, 512, 3) and fv.dtype == torch.float32
            assert np.array_equal(bits(fv.cpu().numpy()[0]), bits(want))
        assert edged[-1, 1] == 12.5                                                   # (the entry's own array is not mirrored in place)
        with pytest.raises(ValueError, match="velodyne"):
            get_minibatch([_entry()], 2)
    finally:
        cfg.FRONT_VIEW_INPUT = saved
    assert np.array_equal(bits(read_lidar.point_cloud_2_front(pts)), bits(cloud["fv"]))
    assert np.array_equal(read_lidar.load_velodyne(path), pts)


@pytest.mark.gpu
def test_detection_loops_feed_the_front_view(gpu, cloud, oracle, tmp_path):
    torch, ops = gpu["torch"], gpu["ops"]
    from mv3d_tf_amd.fast_rcnn import detect_batch
    from mv3d_tf_amd.fast_rcnn.config import cfg
    pts = cloud["pts"]
    clouds = [pts[:1500], pts[1500:1500], pts[1500:]]
    want = [R.raster(c, oracle)[0] for c in clouds]
    rois = np.array([[0, 20, 1, -1, 4, 1.6, 1.5], [0, 30, -3, -1, 4, 1.6, 1.5]], F32)
    scores = np.array([[0.2, 0.8], [0.9, 0.1]], F32)

    class Net:
        """a three-view stub: records the front-view input it is fed and answers with two fixed ROIs per frame (what box_detect reads,
        and what the batched loop reads on top of that: the ROI counts, the rows per frame, the status words)"""
        views = 3

        def __init__(self):
            self.fed = []

        def forward(self, feed):
            fv = feed["lidar_fv_data"]
            self.fed.append(fv)
            B = int(fv.shape[0])
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            return {"rois": (None, None, dev(np.tile(rois, (B, 1)))), "cls_prob": dev(np.tile(scores, (B, 1))),
                    "bbox_pred": dev(np.zeros((2 * B, 48), F32)), "num_rois": dev(np.full((B,), 2, np.int32)), "rois_per_frame": 2,
                    "rois_status": dev(np.zeros((B,), np.int32))}

    def host(t):
        return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    net = Net()
    args = (np.zeros((8, 12, 3), np.uint8), np.zeros((16, 24, 9), F32), np.zeros((4, 12)))
    a = detect_batch.box_detect(None, net, *args, fv=want[0])
    b = detect_batch.box_detect(None, net, *args, None, ops.point_cloud_2_front(clouds[0]))
    assert a[0].shape == (2, 2) and all(np.array_equal(x, y) for x, y in zip(a, b))
    for fed in net.fed:
        assert tuple(fed.shape) == (1, 64, 512, 3) and np.array_equal(bits(host(fed)[0]), bits(want[0]))

    class Imdb:
        name, num_classes, image_index = "three_scans", 2, ["000000", "000001", "000002"]

        def image_at(self, i): return args[0]
        def bv_at(self, i): return args[1]
        def calib_at(self, i): return args[2]
        def evaluate_detections(self, *a): self.evaluated = True

    class PointsImdb(Imdb):
        def points_at(self, i): return clouds[i]
        def velodyne_path_at(self, i): raise AssertionError("points_at comes first")

    class FilesImdb(Imdb):
        def velodyne_path_at(self, i):
            path = str(tmp_path / ("%06d.bin" % i))
            clouds[i].tofile(path)
            return path

    saved, root = dict(cfg.TEST), cfg.ROOT_DIR
    cfg.ROOT_DIR = str(tmp_path)
    try:
        for imdb in (PointsImdb(), FilesImdb()):
            for batch, groups in ((1, ([0], [1], [2])), (2, ([0, 1], [2])), (4, ([0, 1, 2],))):
                net, imdb.evaluated = Net(), False
                cfg.TEST.BATCH_SIZE = batch
                all_boxes, _ = detect_batch.test_net(None, net, imdb, "w")
                assert imdb.evaluated and len(all_boxes[1]) == 3 and all(len(d) >= 1 for d in all_boxes[1])
                assert [int(fed.shape[0]) for fed in net.fed] == [len(g) for g in groups]   # a group's frames from ONE batched call
                for fed, g in zip(net.fed, groups):
                    assert np.array_equal(bits(host(fed)), bits(np.stack([want[i] for i in g])))
    finally:
        cfg.TEST.update(saved)
        cfg.ROOT_DIR = root


@pytest.mark.gpu
def test_pixels_agree_with_the_roi_projection(gpu, cloud):
    """every non-empty pixel (r, c) of the random cloud's device map: the device's front-view ROI of the zero-size box at the winning
    point is [c, r, c, r]"""
    torch, ops = gpu["torch"], gpu["ops"]
    got = device_map(gpu, cloud["pts"])
    r, c = np.nonzero(got[..., 1] != 0)
    assert np.array_equal(got[..., 1] != 0, cloud["win"] >= 0) and len(r) > 2000
    boxes = np.zeros((len(r), 7), F32)
    boxes[:, 1:4] = cloud["pts"][cloud["win"][r, c], :3]
    assert np.array_equal(boxes[:, 3], got[r, c, 0])                                   # the map's height IS the winner's z
    fv = ops.rois_3d_to_fv(torch.from_numpy(boxes).cuda()).cpu().numpy()
    assert np.array_equal(fv[:, 1:], np.stack([c, r, c, r], 1).astype(F32))
