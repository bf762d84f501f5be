"""Crop of Velodyne scans to the camera image: ops.scan_crop_to_image / mv3d_scan_crop_to_image against
tests/scan_crop_restatement.py, the key cfg.LIDAR_CROP_TO_IMAGE and the feeds that crop under it.  PARITY UNPINNED: the reference has
no such code; the restatement is the definition.  Every comparison of device results is equality of bits (uint32 / int32 views: a NaN
reflectance keeps its payload); nothing has a tolerance.  The output buffer is pre-filled with a bit pattern, so a row written
behind the kept ones, or not written in front of them, cannot pass."""
import numpy as np
import pytest

import scan_crop_restatement as R
from conftest import golden
from mv3d_tf_amd import synth

F32 = np.float32
NAN, INF = float("nan"), float("inf")
FILL = 0xA5C3F00F                                   # the pattern every row of points_out holds before a call
# an exactly representable camera: u = 512 - 512 y / x, w = 128 - 512 z / x, depth x; image 256 x 1024
EXACT = np.array([[512, 0, 512, 0, 0, 512, 128, 0, 0, 0, 1, 0], [0] * 12, [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0],
                  [0, -1, 0, 0, 0, 0, -1, 0, 1, 0, 0, 0]], F32)
EXACT_HW = (256, 1024)
KEPT, DROPPED = (1.0, 0.0, 0.0, 0.5), (-1.0, 0.0, 0.0, 0.25)
KITTI_SIZES = ((370, 1224), (374, 1238), (376, 1241), (375, 1242))


def u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def tables():
    """five different calibration tables: the synthetic one, then those of kitti_label.npz and proj_matrix.npz that differ from it
    and from one another, in the files' order"""
    lab = golden("kitti_label")
    found = {}
    for c in [synth.KITTI_CALIB] + [lab["calib_%d" % i] for i in range(3)] + list(golden("proj_matrix")["calibs"]):
        found.setdefault(np.asarray(c, F32).tobytes(), np.asarray(c, F32).reshape(4, 12))
    return list(found.values())[:5]


@pytest.fixture(scope="module")
def lib_ops():
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops
    return ops


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops
    return {"torch": torch, "ops": ops}


def device_crop(gpu, pts, offsets, calibs, hw, device_offsets=False):
    """the op on a pre-filled output with 8 guard rows behind it -> (the whole (P,4) output as uint32, offsets_out); asserts that the
    guard rows and the input come back untouched"""
    torch, ops = gpu["torch"], gpu["ops"]
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 4)
    P = len(pts)
    d_pts = torch.from_numpy(pts).cuda()
    big = torch.from_numpy(np.full((P + 8, 4), FILL, np.uint32).view(F32)).cuda()
    if device_offsets:
        offsets = torch.from_numpy(np.asarray(offsets, np.int32)).cuda()
    out, offs = ops.scan_crop_to_image(d_pts, offsets, calibs, hw, out=big[:P])
    torch.cuda.synchronize()
    assert (P == 0 or out.data_ptr() == big.data_ptr()) and offs.dtype == torch.int32 and offs.is_cuda       # (an empty tensor has no address)
    host = big.cpu().numpy().view(np.uint32)
    assert (host[P:] == FILL).all(), "rows behind the output were written"
    assert np.array_equal(u32(d_pts.cpu().numpy()), u32(pts)), "the input was written"
    return host[:P], offs.cpu().numpy()


def check_against_restatement(gpu, pts, offsets, calibs, hw, device_offsets=False):
    want, want_off = R.crop(pts, offsets, calibs, hw)
    got, got_off = device_crop(gpu, pts, offsets, calibs, hw, device_offsets)
    K = len(want)
    assert np.array_equal(got_off, want_off), (got_off, want_off)
    assert np.array_equal(got[:K], u32(want)), "kept rows differ"
    assert (got[K:] == FILL).all(), "a row at or behind offsets_out[B] was written"
    return want, want_off


def pattern(name, P, T):
    i = np.arange(P)
    return {"all": i >= 0, "none": i < 0, "alternating": i % 2 == 0, "last row": i == P - 1, "first of each tile": i % T == 0,
            "last of each tile": (i % T == T - 1) | (i == P - 1)}[name]


PATTERNS = ("all", "none", "alternating", "last row", "first of each tile", "last of each tile")


def template_cloud(keep):
    """rows of the two template points, each with its own reflectance (so that a row copied from the wrong place shows)"""
    pts = np.where(keep[:, None], F32(KEPT), F32(DROPPED)).astype(F32)
    pts[:, 3] = np.arange(len(pts), dtype=F32) + F32(0.5)
    return pts


# ---------------------------------------------------------------------------------------------------- CPU
def test_restatement_on_the_exact_camera():
    M = R.proj_matrix(EXACT)
    assert M.tolist() == [512, -512, 0, 0, 128, 0, -512, 0, 1, 0, 0, 0]
    h, w = EXACT_HW
    keep = lambda *row: R.keep_row(M, F32(row + (0.0,) * (4 - len(row))), h, w)
    assert R.image_vector(M, 1.0, 1.0, 0.0)[0] == 0.0 and keep(1, 1, 0)                       # u = 0: the first column
    assert R.image_vector(M, 1.0, -1.0, 0.0)[0] == 1024.0 and not keep(1, -1, 0)              # u = width
    assert R.image_vector(M, 1.0, 0.0, 0.25)[1] == 0.0 and keep(1, 0, 0.25)                   # w = 0: the first row
    assert R.image_vector(M, 1.0, 0.0, -0.25)[1] == 256.0 and not keep(1, 0, -0.25)           # w = height
    assert keep(*KEPT[:3]) and not keep(*DROPPED[:3])                                         # in front of / behind the camera
    assert R.image_vector(M, 0.0, 0.0, 0.0)[2] == 0.0 and not keep(0, 0, 0)                   # v[2] == 0
    for bad in (NAN, INF, -INF):
        for axis in range(3):
            row = list(KEPT)
            row[axis] = bad
            assert not keep(*row), row
    assert keep(1, 0, 0, NAN)                                                                  # the reflectance is never looked at
    assert not R.keep_row(M, F32(KEPT), 0, w) and not R.keep_row(M, F32(KEPT), h, 0) and not R.keep_row(M, F32(KEPT), -1, w)
    pts = F32([KEPT, DROPPED, (1, 0, 0, NAN), (NAN, 0, 0, 1)])
    got, off = R.crop(pts, [0, 1, 4], [EXACT, EXACT], [EXACT_HW, EXACT_HW])
    assert np.array_equal(u32(got), u32(pts[[0, 2]])) and off.tolist() == [0, 1, 2] and off.dtype == np.int32
    assert R.crop(pts, [1, 3], [EXACT], [EXACT_HW])[1].tolist() == [0, 1]                      # rows no frame owns are dropped


def test_restatement_is_homogeneous_w_1():
    """a table with a translation along the camera axis: (-1, 0, 0) is one metre in FRONT of the camera (v[2] = -1 + 2), which the
    w = 0 form of image_point (v[2] = -1) would put behind it"""
    moved = EXACT.copy()
    moved[3, 11] = 2.0                                                                         # Tr[2][3]
    M = R.proj_matrix(moved)
    assert M[11] == 2.0 and R.image_vector(M, -1.0, 0.0, 0.0) == [512.0, 128.0, 1.0]
    assert R.keep_row(M, F32(DROPPED), *EXACT_HW) and not R.keep_row(R.proj_matrix(EXACT), F32(DROPPED), *EXACT_HW)


def test_the_checked_key(lib_ops):
    ops = lib_ops
    from mv3d_tf_amd.fast_rcnn import detect_batch
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.roi_data_layer.roidb import prepare_roidb
    from mv3d_tf_amd.rpn_msr.generate import imdb_proposals
    assert cfg.LIDAR_CROP_TO_IMAGE is False and ops.scan_crop() is False

    class NothingLoaded:
        name, num_classes, image_index = "none", 2, ["000000"]

        def __getattr__(self, name):
            raise AssertionError("the imdb was asked for %s" % name)

    cfg.LIDAR_CROP_TO_IMAGE = True
    try:
        for call in (ops.scan_crop, lambda: prepare_roidb(NothingLoaded()), lambda: imdb_proposals(None, object(), NothingLoaded()),
                     lambda: detect_batch.test_net(None, object(), NothingLoaded(), "w")):
            with pytest.raises(ValueError, match="LIDAR_CROP_TO_IMAGE needs cfg.LIDAR_BV_FROM_SCAN"):
                call()
        cfg.LIDAR_BV_FROM_SCAN = True
        assert ops.scan_crop() is True
    finally:
        cfg.LIDAR_CROP_TO_IMAGE, cfg.LIDAR_BV_FROM_SCAN = False, False


def _entry(**extra):
    e = {"image": np.arange(8 * 12 * 3, dtype=np.uint8).reshape(8, 12, 3), "calib": synth.KITTI_CALIB,
         "gt_classes": np.array([1, 0], np.int32), "boxes": np.arange(8, dtype=F32).reshape(2, 4), "boxes_bv": np.arange(8, dtype=F32).reshape(2, 4) + 1,
         "boxes_3D": np.arange(12, dtype=F32).reshape(2, 6), "boxes_corners": np.arange(48, dtype=F32).reshape(2, 24), "flipped": False}
    e.update(extra)
    return e


class _Net:
    def __init__(self, views):
        self.views = views


def _never(*a, **kw):
    raise AssertionError("ops.scan_crop_to_image was called with cfg.LIDAR_CROP_TO_IMAGE off")


def test_key_off_means_no_call(lib_ops, monkeypatch):
    from mv3d_tf_amd.fast_rcnn import detect_batch
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    monkeypatch.setattr(lib_ops, "scan_crop_to_image", _never)
    bev = np.zeros((5, 601, 2), F32)
    blobs = get_minibatch([_entry(lidar_bv=bev, velodyne=np.zeros((3, 4), F32))], 2)
    assert blobs["lidar_bv_data"].shape == (1, 5, 601, 2) and "lidar_fv_data" not in blobs
    ims = [np.zeros((8, 12, 3), np.uint8)] * 2
    feed = detect_batch.group_feed(_Net(2), ims, [bev, bev], [synth.KITTI_CALIB] * 2, [None, None], False)
    assert feed["lidar_bv_data"].shape == (2, 5, 601, 2) and "lidar_fv_data" not in feed
    assert detect_batch.scan_feed([np.zeros((3, 4), F32)], False, False) == {}


def test_bad_arguments_are_refused_before_any_upload(lib_ops, monkeypatch):
    import torch
    ops = lib_ops
    monkeypatch.setattr(ops, "_workspace", lambda *a, **kw: pytest.fail("a workspace was asked for"))
    good, cal, hw = np.zeros((3, 4), F32), EXACT[None], [EXACT_HW]
    for exc, args in ((TypeError, (np.zeros((3, 4)), None, cal, hw)), (ValueError, (np.zeros((3, 3), F32), None, cal, hw)),
                      (ValueError, (torch.zeros(3, 4), None, cal, hw)),                                  # a points tensor on the host
                      (TypeError, (good, [0.0, 3.0], cal, hw)), (ValueError, (good, [0, 2, 1], np.stack([EXACT] * 2), [EXACT_HW] * 2)),
                      (ValueError, (good, [0, 4], cal, hw)),
                      (TypeError, (good, None, EXACT[None].astype(np.int32), hw)), (TypeError, (good, None, torch.zeros((1, 48), dtype=torch.float64), hw)),
                      (ValueError, (good, None, EXACT, hw)), (ValueError, (good, None, np.zeros((1, 47), F32), hw)),
                      (ValueError, (good, [0, 1, 3], cal, [EXACT_HW] * 2)), (ValueError, (good, None, [EXACT, EXACT], hw)),
                      (ValueError, (good, None, torch.zeros((1, 48)), hw)),                              # a calib tensor on the host
                      (TypeError, (good, None, cal, [(256.0, 1024.0)])), (TypeError, (good, None, cal, torch.zeros((1, 2), dtype=torch.int64))),
                      (ValueError, (good, None, cal, [EXACT_HW] * 2)), (ValueError, (good, None, cal, [(256,)])), (ValueError, (good, None, cal, EXACT_HW)),
                      (ValueError, (good, None, cal, [(256, 2 ** 31)])), (ValueError, (good, None, cal, torch.zeros((1, 2), dtype=torch.int32))),
                      (TypeError, (good, None, cal, hw, np.zeros((3, 4), F32))), (TypeError, (good, None, cal, hw, torch.zeros((3, 4), dtype=torch.float16))),
                      (ValueError, (good, None, cal, hw, torch.zeros((2, 4)))), (ValueError, (good, None, cal, hw, torch.zeros((3, 4)))),
                      (ValueError, (good, None, cal, hw, torch.zeros((4, 3)).t())),
                      (TypeError, (good, None, cal, hw, None, torch.zeros(2, dtype=torch.int64))), (ValueError, (good, None, cal, hw, None, torch.zeros(3, dtype=torch.int32))),
                      (ValueError, (good, None, cal, hw, None, torch.zeros(2, dtype=torch.int32))),      # (on the host)
                      (TypeError, (good, None, cal, hw, None, None, torch.zeros(4096))), (ValueError, (good, None, cal, hw, None, None, torch.zeros(4096, dtype=torch.uint8)))):
        with pytest.raises(exc, match="scan_crop_to_image"):
            ops.scan_crop_to_image(*args)
    # image shapes (h, w, 3) and float64 tables from the host pass the table checks
    cal48, hw2 = ops._crop_tables("scan_crop_to_image", [EXACT.astype(np.float64)] * 2, [(375, 1242, 3), (370, 1224, 3)], 2)
    assert cal48.dtype == F32 and cal48.shape == (2, 48) and hw2.dtype == np.int32 and hw2.tolist() == [[375, 1242], [370, 1224]]


def test_c_entry_refuses_invalid_arguments_before_any_launch(lib_ops):
    ops, L, lib = lib_ops, lib_ops.lib(), lib_ops._lib
    T = L.mv3d_scan_crop_tile_rows()
    assert T == ops.scan_crop_tile_rows() and T >= 256 and T % 64 == 0
    ws = L.mv3d_scan_crop_workspace
    assert ws(-1) == 0 and ws(0) == 0 and ws(1) > 0 and ws(2 * T + 3) >= (2 * T + 3 + 63) // 64 * 8 + 3 * 4 and ws(2 ** 31 - 1) > 2 ** 28 // 8
    assert ops.scan_crop_workspace_bytes(120000) == ws(120000)
    A, fn, big = 1 << 20, L.mv3d_scan_crop_to_image, 1 << 30                         # non-NULL, aligned "pointers" (never dereferenced)
    P = 100
    IN, OUT, WS, OFF, CAL, HW, OOUT = A, 2 * A, 3 * A, 4 * A, 5 * A, 6 * A, 7 * A
    for args in ((IN, OFF, 1025, P, CAL, HW, OUT, OOUT, WS, big), (IN, OFF, -1, P, CAL, HW, OUT, OOUT, WS, big), (IN, OFF, 1, -1, CAL, HW, OUT, OOUT, WS, big),
                 (IN, None, 2, P, CAL, HW, OUT, OOUT, WS, big),                       # no offsets, two frames
                 (None, OFF, 1, P, CAL, HW, OUT, OOUT, WS, big), (IN, OFF, 1, P, None, HW, OUT, OOUT, WS, big), (IN, OFF, 1, P, CAL, None, OUT, OOUT, WS, big),
                 (IN, OFF, 1, P, CAL, HW, None, OOUT, WS, big), (IN, OFF, 1, P, CAL, HW, OUT, None, WS, big), (IN, OFF, 1, P, CAL, HW, OUT, OOUT, None, big),
                 (IN + 4, OFF, 1, P, CAL, HW, OUT, OOUT, WS, big), (IN, OFF + 2, 1, P, CAL, HW, OUT, OOUT, WS, big), (IN, OFF, 1, P, CAL + 2, HW, OUT, OOUT, WS, big),
                 (IN, OFF, 1, P, CAL, HW + 1, OUT, OOUT, WS, big), (IN, OFF, 1, P, CAL, HW, OUT + 8, OOUT, WS, big), (IN, OFF, 1, P, CAL, HW, OUT, OOUT + 2, WS, big),
                 (IN, OFF, 1, P, CAL, HW, OUT, OOUT, WS + 8, big),                    # misaligned, one by one
                 (IN, OFF, 1, P, CAL, HW, OUT, OOUT, WS, ws(P) - 1), (IN, OFF, 1, P, CAL, HW, OUT, OOUT, WS, 0),      # a short workspace
                 (IN, OFF, 1, P, CAL, HW, IN, OOUT, WS, big), (IN, OFF, 1, P, CAL, HW, IN + 16 * (P - 1), OOUT, WS, big),
                 (IN + 16 * (P - 1), OFF, 1, P, CAL, HW, IN, OOUT, WS, big)):         # output over input: the same, one row shared at either end
        assert fn(*args, None) == lib.ERR_INVALID_ARG, args
    assert fn(None, None, 0, 0, None, None, None, None, None, 0, None) == lib.OK       # no frame: nothing to do


# ---------------------------------------------------------------------------------------------------- GPU
def _sizes(T):
    return (0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 3)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(12))
def test_one_frame_sizes_and_patterns(gpu, which):
    T = gpu["ops"].scan_crop_tile_rows()
    P = _sizes(T)[which]
    for name in PATTERNS:
        keep = pattern(name, P, T)
        pts = template_cloud(keep)
        want, off = check_against_restatement(gpu, pts, None, [EXACT], [EXACT_HW])
        assert len(want) == int(keep.sum()) == off[1], (name, P)                    # the templates are what they are meant to be


def _batch(T):
    sizes = (0, 1, T + 1, 0, 300)
    offsets = np.cumsum((7,) + sizes).astype(np.int32)
    pts = synth.point_cloud(81, int(offsets[-1]) + 11)
    return pts, offsets, tables(), list(KITTI_SIZES) + [KITTI_SIZES[0]]


@pytest.mark.gpu
def test_batch_of_five_frames(gpu):
    T = gpu["ops"].scan_crop_tile_rows()
    pts, offsets, calibs, hw = _batch(T)
    assert len({c.tobytes() for c in calibs}) == 5
    want, want_off = check_against_restatement(gpu, pts, offsets, calibs, hw)
    kept = np.diff(want_off)
    assert kept[0] == kept[3] == 0 and 0 < kept[2] < T + 1 and 0 < kept[4] < 300       # the crop does crop, and does keep
    check_against_restatement(gpu, pts, offsets, calibs, hw, device_offsets=True)
    for b in range(5):                                                                   # frame b alone: the same rows
        rows = pts[offsets[b]:offsets[b + 1]]
        got, off = device_crop(gpu, rows, None, [calibs[b]], [hw[b]])
        assert off.tolist() == [0, kept[b]] and np.array_equal(got[:kept[b]], u32(want[want_off[b]:want_off[b + 1]])), b


@pytest.mark.gpu
@pytest.mark.parametrize("offsets", [(0, 900, 400, 1200, 1100, 5000), (1300, 900, 600, 300, 100, 0), (-5, -5, 40, 40, 2 ** 31 - 1, 2 ** 31 - 1),
                                     (2000, 2001, 2002, 2003, 2004, 2005), (0, 0, 0, 0, 0, 0)])
def test_malformed_device_offsets_stay_in_bounds(gpu, offsets):
    """descending offsets and offsets beyond P: the rows no frame owns are dropped, the rest is the restatement's, nothing else is written"""
    T = gpu["ops"].scan_crop_tile_rows()
    pts, _, calibs, hw = _batch(T)
    assert max(offsets) > len(pts) or min(np.diff(offsets)) <= 0
    check_against_restatement(gpu, pts, np.array(offsets, np.int64).astype(np.int32), calibs, hw, device_offsets=True)


@pytest.mark.gpu
def test_special_values(gpu):
    sub = float(np.float32(1e-42))
    rows = [KEPT, DROPPED, (1, 1, 0, 1), (1, -1, 0, 2), (1, 0, 0.25, 3), (1, 0, -0.25, 4), (0, 0, 0, 5), (-0.0, -0.0, -0.0, 6),
            (1, -0.0, -0.0, 7), (sub, 0, 0, 8), (sub, sub, -sub, 9), (sub, -sub, 0, 10), (-sub, 0, 0, 11), (1, sub, sub, 12),
            (3e38, 0, 0, 13), (3e38, 3e38, 0, 14), (3e38, -3e38, 3e38, 15), (1, 0, 0, NAN), (1, 0, 0, INF), (2, 1, 0.25, -0.0)]
    for bad in (NAN, INF, -INF):
        for axis in range(3):
            row = list(KEPT)
            row[axis] = bad
            rows.append(tuple(row))
    pts = np.array(rows * 3, F32)
    nan_rows = np.flatnonzero(np.isnan(pts[:, 3]))
    pts.view(np.uint32)[nan_rows, 3] = 0x7FC12345 + np.arange(len(nan_rows), dtype=np.uint32)       # NaN reflectances with payloads
    n = len(rows)
    offsets = [0, n, 2 * n, 3 * n]
    want, off = check_against_restatement(gpu, pts, offsets, [EXACT] * 3, [EXACT_HW, (0, 1024), (256, 0)])
    assert off[1] > 4 and off[1] == off[2] == off[3]                                   # a frame of height 0 or width 0 keeps nothing
    assert np.isnan(want[:, 3]).sum() == 1 and (u32(want)[:, 3] == 0x7FC12345).sum() == 1
    want, off = check_against_restatement(gpu, pts, offsets, [EXACT] * 3, [EXACT_HW, (1, 1024), (256, 1)])
    assert off[1] < off[2] < off[3] < 2 * off[1]


def _frustum_clouds():
    clouds = [synth.point_cloud(seed, 4096) for seed in (90, 91)]
    masks = [R.keep_mask(c, None, [synth.KITTI_CALIB], [(375, 1242)]) for c in clouds]
    return clouds, masks


@pytest.fixture(scope="module")
def frustum_clouds():
    """two synthetic scans and the rows of each the restatement keeps under KITTI_CALIB and a 375 x 1242 image: computed once"""
    clouds, masks = _frustum_clouds()
    for c, m in zip(clouds, masks):
        c.setflags(write=False)
        m.setflags(write=False)
    return clouds, masks


def test_the_synthetic_scans_straddle_the_frustum(frustum_clouds):
    for mask in frustum_clouds[1]:
        share = mask.mean()
        print("kept share of the synthetic scan: %.3f" % share)
        assert 0.10 <= share <= 0.90


@pytest.mark.gpu
def test_through_the_rasters(gpu, frustum_clouds):
    torch, ops = gpu["torch"], gpu["ops"]
    clouds, masks = frustum_clouds
    for mask in masks:
        assert 0.10 <= mask.mean() <= 0.90
    pts = np.concatenate(clouds, 0)
    offsets = np.array([0, 4096, 8192], np.int32)
    cropped, off = ops.scan_crop_to_image(torch.from_numpy(pts).cuda(), offsets, [synth.KITTI_CALIB] * 2, [(375, 1242)] * 2)
    host = [c[m] for c, m in zip(clouds, masks)]
    h_pts = torch.from_numpy(np.concatenate(host, 0)).cuda()
    h_off = np.cumsum([0] + [len(c) for c in host]).astype(np.int32)
    assert off.cpu().numpy().tolist() == h_off.tolist()
    for raster in (ops.point_cloud_2_top_batch, ops.point_cloud_2_top_paper, ops.point_cloud_2_front):
        got, want = raster(cropped, off), raster(h_pts, h_off)
        full = raster(torch.from_numpy(pts).cuda(), offsets)
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), raster.__name__
        assert bool(want.any()) and not torch.equal(full.view(torch.int32), want.view(torch.int32)), raster.__name__     # (the crop shows in the map)


@pytest.mark.gpu
def test_occupancy_outside_the_frustum(gpu):
    """returns at x = 5, y = +-20 lie inside the BEV range and outside KITTI_CALIB's image: uncropped they occupy anchors, cropped the
    map is empty and the existing mask drops every anchor"""
    torch, ops = gpu["torch"], gpu["ops"]
    rng = np.random.RandomState(5)
    pts = np.stack([np.full(200, 5.0), np.where(np.arange(200) % 2, 20.0, -20.0), rng.uniform(-1.5, 0.0, 200), rng.uniform(0.1, 1.0, 200)], 1).astype(F32)
    d = torch.from_numpy(pts).cuda()
    full = ops.point_cloud_2_top_batch(d)
    assert bool(full.any()) and int(ops.anchor_occupancy(full, 75, 75).sum()) > 0
    cropped, off = ops.scan_crop_to_image(d, None, [synth.KITTI_CALIB], [(375, 1242)])
    assert off.cpu().numpy().tolist() == [0, 0]
    top = ops.point_cloud_2_top_batch(cropped, off)
    assert tuple(top.shape) == (1, 601, 601, 9) and not bool(top.any()) and int(ops.anchor_occupancy(top, 75, 75).sum()) == 0


@pytest.mark.gpu
def test_capture_and_replay(gpu):
    """ONE graph with out=, offsets_out= and workspace= given, replayed after the cloud's contents and the device offsets change (the
    total, the buffers' capacity, stays); each replay equals the eager call on fresh buffers"""
    torch, ops = gpu["torch"], gpu["ops"]
    cap = 3000
    calibs, hw = tables()[:2], [KITTI_SIZES[3], KITTI_SIZES[0]]
    fillings = [(synth.point_cloud(seed, cap), np.cumsum((0,) + sizes).astype(np.int32)) for seed, sizes in ((95, (1200, 1500)), (96, (2900, 100)), (97, (0, 3)))]
    buf = torch.from_numpy(fillings[0][0]).cuda()
    d_off = torch.from_numpy(fillings[0][1]).cuda()
    d_cal, d_hw = torch.from_numpy(np.stack(calibs).reshape(2, 48)).cuda(), torch.tensor(hw, dtype=torch.int32, device="cuda")
    out = torch.empty((cap, 4), device="cuda")
    off_out = torch.empty(3, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.scan_crop_workspace_bytes(cap), dtype=torch.uint8, device="cuda")
    call = lambda: ops.scan_crop_to_image(buf, d_off, d_cal, d_hw, out=out, offsets_out=off_out, workspace=ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                                          # (warm-up: the code object is loaded outside the capture)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res = call()
    assert res[0] is out and res[1] is off_out
    for pts, offsets in reversed(fillings):
        buf.copy_(torch.from_numpy(pts))
        d_off.copy_(torch.from_numpy(offsets))
        out.view(torch.int32).fill_(0x5A5A5A5A)
        off_out.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_off = ops.scan_crop_to_image(torch.from_numpy(pts).cuda(), torch.from_numpy(offsets).cuda(), d_cal, d_hw)
        K = int(eager_off[2])
        assert torch.equal(off_out, eager_off) and torch.equal(out[:K].view(torch.int32), eager[:K].view(torch.int32))
        assert bool((out[K:].view(torch.int32) == 0x5A5A5A5A).all())
        want, want_off = R.crop(pts, offsets, calibs, hw)
        assert want_off.tolist() == off_out.cpu().numpy().tolist() and np.array_equal(u32(out[:K].cpu().numpy()), u32(want))


def _host_rasters(ops, torch, cloud, keep):
    d = torch.from_numpy(np.ascontiguousarray(cloud[keep])).cuda()
    return ops.point_cloud_2_top_batch(d), ops.point_cloud_2_front(d)


@pytest.mark.gpu
def test_get_minibatch_crops_under_the_key(gpu, frustum_clouds, monkeypatch):
    torch, ops = gpu["torch"], gpu["ops"]
    from mv3d_tf_amd.datasets.mirror import mirror_calib
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    pts = np.array(frustum_clouds[0][0])
    image = np.random.RandomState(1).randint(0, 255, (375, 1242, 3)).astype(np.uint8)
    mirrored = np.asarray(mirror_calib(synth.KITTI_CALIB, 1242), F32)
    entries = (_entry(image=image, velodyne=pts), _entry(image=image, velodyne=pts, flipped=True, calib=mirrored))
    cfg.LIDAR_BV_FROM_SCAN = cfg.FRONT_VIEW_INPUT = True
    try:
        # key off: what the existing rasters give, called directly
        monkeypatch.setattr(ops, "scan_crop_to_image", _never)
        for entry in entries:
            cloud = pts * F32([1, -1, 1, 1]) if entry["flipped"] else pts
            blobs = get_minibatch([entry], 2)
            d = torch.from_numpy(cloud).cuda()
            assert tuple(blobs["lidar_bv_data"].shape) == (1, 601, 601, 9) and tuple(blobs["lidar_fv_data"].shape) == (1, 64, 512, 3)
            assert torch.equal(blobs["lidar_bv_data"][0].view(torch.int32), ops.point_cloud_2_top_batch(d).view(torch.int32))
            assert torch.equal(blobs["lidar_fv_data"][0].view(torch.int32), ops.point_cloud_2_front(d).view(torch.int32))
        monkeypatch.undo()
        cfg.LIDAR_CROP_TO_IMAGE = True
        for entry in entries:
            cloud = pts * F32([1, -1, 1, 1]) if entry["flipped"] else pts
            keep = R.keep_mask(cloud, None, [entry["calib"]], [(375, 1242)])
            assert 0.10 <= keep.mean() <= 0.90
            blobs = get_minibatch([entry], 2)
            bev, fv = _host_rasters(ops, torch, cloud, keep)
            assert tuple(blobs["lidar_bv_data"].shape) == (1, 601, 601, 9) and tuple(blobs["lidar_fv_data"].shape) == (1, 64, 512, 3)
            assert np.array_equal(blobs["im_info"], [[601, 601, 1]])
            assert bool(bev.any()) and torch.equal(blobs["lidar_bv_data"][0].view(torch.int32), bev.view(torch.int32))
            assert bool(fv.any()) and torch.equal(blobs["lidar_fv_data"][0].view(torch.int32), fv.view(torch.int32))
    finally:
        cfg.LIDAR_BV_FROM_SCAN = cfg.FRONT_VIEW_INPUT = cfg.LIDAR_CROP_TO_IMAGE = False


@pytest.mark.gpu
def test_group_feed_crops_under_the_key(gpu, frustum_clouds, monkeypatch):
    """three frames of different image sizes under cfg.IMAGE_BLOB_ON_DEVICE: each frame is cropped to its OWN image, not the canvas"""
    torch, ops = gpu["torch"], gpu["ops"]
    from mv3d_tf_amd.fast_rcnn import detect_batch
    from mv3d_tf_amd.fast_rcnn.config import cfg
    clouds = [np.array(frustum_clouds[0][0][:2000]), np.array(frustum_clouds[0][1][:1500]), np.array(frustum_clouds[0][0][2000:])]
    shapes = [(370, 1224, 3), (376, 1241, 3), (200, 600, 3)]
    ims = [np.random.RandomState(i).randint(0, 255, s).astype(np.uint8) for i, s in enumerate(shapes)]
    calibs = [c.astype(np.float64) for c in tables()[:3]]
    cfg.LIDAR_BV_FROM_SCAN = cfg.IMAGE_BLOB_ON_DEVICE = True
    try:
        monkeypatch.setattr(ops, "scan_crop_to_image", _never)
        feed = detect_batch.group_feed(_Net(3), ims, [None] * 3, calibs, clouds, True)
        for b, cloud in enumerate(clouds):                                             # key off: the existing rasters, called directly
            bev, fv = _host_rasters(ops, torch, cloud, slice(None))
            assert torch.equal(feed["lidar_bv_data"][b].view(torch.int32), bev.view(torch.int32))
            assert torch.equal(feed["lidar_fv_data"][b].view(torch.int32), fv.view(torch.int32))
        monkeypatch.undo()
        cfg.LIDAR_CROP_TO_IMAGE = True
        feed = detect_batch.group_feed(_Net(3), ims, [None] * 3, calibs, clouds, True)
        assert tuple(feed["image_data"].shape) == (3, 376, 1241, 3) and tuple(feed["lidar_bv_data"].shape) == (3, 601, 601, 9)
        assert tuple(feed["lidar_fv_data"].shape) == (3, 64, 512, 3) and np.array_equal(feed["im_info"], [[601, 601, 1]] * 3)
        for b, cloud in enumerate(clouds):
            keep = R.keep_mask(cloud, None, [calibs[b]], [shapes[b][:2]])
            assert 0 < keep.sum() < len(cloud)
            bev, fv = _host_rasters(ops, torch, cloud, keep)
            assert bool(bev.any()) and torch.equal(feed["lidar_bv_data"][b].view(torch.int32), bev.view(torch.int32)), b
            assert bool(fv.any()) and torch.equal(feed["lidar_fv_data"][b].view(torch.int32), fv.view(torch.int32)), b
        on_canvas = R.keep_mask(clouds[2], None, [calibs[2]], [(376, 1241)])
        assert on_canvas.sum() > R.keep_mask(clouds[2], None, [calibs[2]], [shapes[2][:2]]).sum()       # (the canvas would keep more)
    finally:
        cfg.LIDAR_BV_FROM_SCAN = cfg.IMAGE_BLOB_ON_DEVICE = cfg.LIDAR_CROP_TO_IMAGE = False
