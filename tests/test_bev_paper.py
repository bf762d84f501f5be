"""The MV3D paper's bird's-eye-view encoding from raw scans: ops.point_cloud_2_top_paper /
mv3d_point_cloud_2_top_paper_batch against tests/bev_paper_restatement.py, and the layers that feed a 10-channel `lidar_bv_data`
under cfg.LIDAR_BV_ENCODING = 'paper'.  PARITY UNPINNED: the reference has no such raster; the restatement is tied to pinned code
where the two encodings agree (test_restatement_agrees_with_the_oracle_where_the_encodings_meet).  Every raster comparison is
equality of the int32 views; nothing has a tolerance except the convolution's input layer, whose bound is tests/test_conv_mfma.py's.
Every non-empty expected map is asserted to have non-zero entries, so an all-zero output cannot pass."""
import ctypes as C
import math

import numpy as np
import pytest

import bev_paper_restatement as R
from mv3d_tf_amd import synth

F32 = np.float32
P_GROUP = 256                      # threads per workgroup of the scatter kernel (csrc/bev_paper.hip)
NAN, INF = float("nan"), float("inf")
# 33 x 33 x 10 = 10 890 floats a frame = 8 mod 16 bytes: odd frames of a batch start off a 16-byte boundary
SMALL = (0.1, 0.3, -1.6, 1.6, 0.0, 3.2, -2.0, 0.4)
# ranges whose corner cells a point can reach (tests/test_bev_batch.py: CORNER_CASE): (81, 39, 7), 22 113 floats = 4 mod 16 bytes
CORNER = (0.2, 0.5, 0.3, 8.0, 2.0, 18.1, -1.0, 1.25)
# y_max = int(3.15 / 0.1) = 31, but a point with 0.05 < x < 0.1 lands on row int(-x / 0.1) + 32 = 32: outside the map
OUTSIDE = (0.1, 0.3, -1.6, 1.6, 0.05, 3.2, -2.0, 0.4)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def small_rows(seed, P):
    """P rows that SMALL keeps, z over all eight slices"""
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(0.05, 3.15, P), rng.uniform(-1.55, 1.55, P), rng.uniform(-2.0, 0.39, P), rng.uniform(0.05, 1.0, P)], 1).astype(F32)


def small_cell(x, y):
    """(row, column) of SMALL's map a kept point falls into"""
    return int(F32(-x) / F32(0.1)) + 32, int(F32(-y) / F32(0.1)) + 16


def expected(pts, offsets, ranges=R.MV3D_RANGES):
    want = R.raster_batch(pts, offsets, ranges)
    for b in range(len(offsets) - 1):
        assert want[b].any() == (offsets[b + 1] > offsets[b]), "frame %d: a non-empty frame's expected map must have non-zero entries" % b
    return want


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


def device_map(gpu, pts, offsets=None, **kw):
    return gpu["ops"].point_cloud_2_top_paper(gpu["torch"].from_numpy(np.array(pts, F32)).cuda(), offsets, **kw).cpu().numpy()


# ---------------------------------------------------------------------------------------------------- CPU
def test_density_table(lib_ops):
    T = lib_ops.bev_density_table()
    assert T.dtype == F32 and T.shape == (64,)
    want = np.array([F32(min(1.0, math.log(n + 1) / math.log(64))) for n in range(64)], F32)
    assert np.array_equal(bits(T), bits(want)) and np.array_equal(bits(T), bits(R.density_table()))
    assert T[0] == 0 and T[63] == 1.0 and (np.diff(T) > 0).all()
    assert lib_ops.lib().mv3d_bev_density_table(None) == lib_ops._lib.ERR_INVALID_ARG


def test_shape_and_workspace_functions(lib_ops):
    ops, L, lib = lib_ops, lib_ops.lib(), lib_ops._lib
    assert ops.BEV_PAPER_SHAPE == (601, 601, 10) == R.shape()[0]
    dims = (C.c_int * 3)()
    for ranges, want in ((R.MV3D_RANGES, (601, 601, 10)), (SMALL, (33, 33, 10)), (CORNER, (81, 39, 7)), (OUTSIDE, (32, 33, 10)),
                         ((0.1, 0.35, -1.6, 1.6, 0.0, 3.2, -2.0, 0.4), (33, 33, 9))):
        assert L.mv3d_point_cloud_2_top_paper_shape(*ranges, dims) == lib.OK and tuple(dims) == want == R.shape(ranges)[0]
        ref = (C.c_int * 3)()
        assert L.mv3d_point_cloud_2_top_shape(*ranges, ref) == lib.OK and tuple(ref)[:2] == want[:2]       # the same cells
        r8 = (C.c_double * 8)(*ranges)
        assert L.mv3d_point_cloud_2_top_paper_workspace(3, r8) == 3 * want[0] * want[1] * 8 == ops.point_cloud_2_top_paper_workspace_bytes(3, ranges)
    assert ops.point_cloud_2_top_paper_workspace_bytes() == L.mv3d_point_cloud_2_top_paper_workspace(1, None) == 601 * 601 * 8
    assert 10890 * 4 % 16 == 8 and 601 * 601 * 10 * 4 % 16 == 8
    # refused as the existing shape entry refuses them: inverted, empty, too many cells, too many slices, no dims
    for bad in ((0.1, 0.3, 30., -30., 0., 60., -2., 0.4), (0.1, 0.001, -30., 30., 0., 60., -2., 0.4), (0.0, 0.3, -30., 30., 0., 60., -2., 0.4),
                (0.1, 0.3, -30., 30., 0., 60., 0.4, -2.), (0.001, 0.3, -30., 30., 0., 60., -2., 0.4), (NAN, 0.3, -30., 30., 0., 60., -2., 0.4)):
        assert L.mv3d_point_cloud_2_top_paper_shape(*bad, dims) == lib.ERR_INVALID_ARG == L.mv3d_point_cloud_2_top_shape(*bad, dims), bad
        assert L.mv3d_point_cloud_2_top_paper_workspace(1, (C.c_double * 8)(*bad)) == 0
    assert L.mv3d_point_cloud_2_top_paper_shape(*SMALL, None) == lib.ERR_INVALID_ARG
    assert L.mv3d_point_cloud_2_top_paper_workspace(0, None) == 0 and L.mv3d_point_cloud_2_top_paper_workspace(ops.FV_MAX_FRAMES + 1, None) == 0


def test_bad_arguments_are_refused_before_any_launch(lib_ops):
    import torch
    ops = lib_ops
    good = np.zeros((3, 4), F32)
    for exc, args in ((TypeError, (np.zeros((3, 4)),)), (TypeError, (np.zeros((3, 4), np.int32),)), (TypeError, (torch.zeros(3, 4, dtype=torch.float16),)),
                      (ValueError, (np.zeros((3, 3), F32),)), (ValueError, (np.zeros((12,), F32),)), (ValueError, (torch.zeros(3, 4),)),
                      (TypeError, (good, [0.0, 3.0])), (TypeError, (good, torch.zeros(2, dtype=torch.int64))),
                      (ValueError, (good, [0, 2, 1])), (ValueError, (good, [0, 4])), (ValueError, (good, [-1, 3])), (ValueError, (good, [[0, 3]])),
                      (ValueError, (good, [0])), (ValueError, (good, np.zeros(ops.FV_MAX_FRAMES + 2, np.int32))),
                      (ValueError, (good, None, (0.1, 0.3, 30., -30., 0., 60., -2., 0.4))), (ValueError, (good, None, (0.1, 0.001, -30., 30., 0., 60., -2., 0.4))),
                      (TypeError, (good, None, None, np.zeros(ops.BEV_PAPER_SHAPE, F32))), (TypeError, (good, None, SMALL, torch.zeros((33, 33, 10), dtype=torch.float16))),
                      (ValueError, (good, None, None, torch.zeros((601, 601, 9)))), (ValueError, (good, [0, 1, 3], SMALL, torch.zeros((1, 33, 33, 10)))),
                      (ValueError, (good, None, SMALL, torch.zeros((33, 33, 9)))),
                      (TypeError, (good, None, None, None, np.zeros(1 << 22, np.uint8))), (TypeError, (good, None, None, None, torch.zeros(1 << 22))),
                      (ValueError, (good, None, SMALL, None, torch.zeros(33 * 33 * 8 - 1, dtype=torch.uint8)))):     # (a host tensor, and too small)
        with pytest.raises(exc, match="point_cloud_2_top_paper"):
            ops.point_cloud_2_top_paper(*args)
    L, lib = ops.lib(), ops._lib
    A = 4096                                                                         # a non-NULL, aligned "pointer" (never dereferenced)
    r8 = (C.c_double * 8)(*SMALL)
    bad = (C.c_double * 8)(0.1, 0.3, 30.0, -30.0, 0.0, 60.0, -2.0, 0.4)
    fn = L.mv3d_point_cloud_2_top_paper_batch
    for args in ((A, A, -1, 4, None, A, A, None), (A, A, ops.FV_MAX_FRAMES + 1, 4, None, A, A, None), (A, A, 1, -1, None, A, A, None),
                 (None, A, 1, 4, None, A, A, None), (A, None, 2, 4, None, A, A, None), (A, A, 1, 4, None, None, A, None),
                 (A, A, 1, 4, None, A, None, None), (A, A, 1, 4, None, A, A + 8, None),                   # no workspace; a misaligned one
                 (A + 4, A, 1, 4, None, A, A, None), (A, A + 2, 1, 4, None, A, A, None), (A, A, 1, 4, None, A + 2, A, None),
                 (A, A, 1, 4, r8, A, A, None), (A, A, 1, 4, r8, A, A, A + 2), (A, A, 1, 4, bad, A, A, A)):
        assert fn(*args, None) == lib.ERR_INVALID_ARG, args
    assert fn(None, None, 0, 0, None, None, None, None, None) == lib.OK              # no frame: nothing to do


class _Imdb:
    """what prepare_roidb asks of a dataset"""

    def __init__(self):
        self.roidb = [{"gt_overlaps": np.array([[0, 1.0], [0, 0]], F32)} for _ in range(2)]

    def image_path_at(self, i): return "/images/%06d.png" % i
    def lidar_path_at(self, i): return "/lidar_bv/%06d.npy" % i
    def calib_at(self, i): return np.full((4, 12), i, F32)
    def velodyne_path_at(self, i): return "/velodyne/%06d.bin" % i


class _NothingLoaded:
    """an imdb whose every access fails: the loops must refuse the configuration before they load a frame"""
    name, num_classes, image_index = "none", 2, ["000000"]

    def __getattr__(self, name):
        raise AssertionError("the imdb was asked for %s" % name)


def test_config_rules(lib_ops, tmp_path):
    ops = lib_ops
    from mv3d_tf_amd.fast_rcnn import detect_batch
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.roi_data_layer.roidb import prepare_roidb
    from mv3d_tf_amd.rpn_msr.generate import imdb_proposals
    assert cfg.LIDAR_BV_ENCODING == "reference" and cfg.LIDAR_BV_FROM_SCAN is False
    assert ops.bev_encoding() == "reference" and ops.bev_channels() == 9
    plain = prepare_roidb(_Imdb())
    for i, e in enumerate(plain):                                                   # the default: what prepare_roidb gave before the key
        assert set(e) == {"gt_overlaps", "image_path", "lidar_bv_path", "calib", "velodyne_path", "max_overlaps", "max_classes"}
        assert e["lidar_bv_path"] == "/lidar_bv/%06d.npy" % i and np.array_equal(e["max_classes"], [1, 0])
    root = cfg.ROOT_DIR
    cfg.ROOT_DIR = str(tmp_path)
    try:
        for enc, from_scan, match in (("paper", False, "LIDAR_BV_FROM_SCAN"), ("Paper", True, "'reference' or 'paper'"), (None, False, "'reference' or 'paper'")):
            cfg.LIDAR_BV_ENCODING, cfg.LIDAR_BV_FROM_SCAN = enc, from_scan
            with pytest.raises(ValueError, match=match):
                prepare_roidb(_NothingLoaded())
            with pytest.raises(ValueError, match=match):
                detect_batch.test_net(None, object(), _NothingLoaded(), "w")
            with pytest.raises(ValueError, match=match):
                imdb_proposals(None, object(), _NothingLoaded())
            with pytest.raises(ValueError, match=match):
                ops.bev_channels()
        cfg.LIDAR_BV_ENCODING, cfg.LIDAR_BV_FROM_SCAN = "paper", True
        assert ops.bev_encoding() == "paper" and ops.bev_channels() == 10
        on = prepare_roidb(_Imdb())
        assert all("lidar_bv_path" not in e and e["velodyne_path"] for e in on)
    finally:
        cfg.LIDAR_BV_ENCODING, cfg.LIDAR_BV_FROM_SCAN, cfg.ROOT_DIR = "reference", False, root


def test_network_variable_for_ten_channels(tmp_path, capsys):
    import torch
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.networks import factory
    from mv3d_tf_amd.networks.mv3d import MV3D
    nine, ten, default = (MV3D(phase="TEST", device="cpu", bev_channels=c) for c in (9, 10, None))
    assert default.bev_channels == nine.bev_channels == 9 and ten.bev_channels == 10
    assert ten.params["conv1_1"][0].shape == (64, 10, 3, 3) and nine.params["conv1_1"][0].shape == default.params["conv1_1"][0].shape == (64, 9, 3, 3)
    assert list(nine.params) == list(ten.params)
    for k in nine.params:
        assert nine.params[k][1].shape == ten.params[k][1].shape
        assert k == "conv1_1" or nine.params[k][0].shape == ten.params[k][0].shape, k
    assert all(torch.equal(a, b) for k in nine.params for a, b in zip(nine.params[k], default.params[k]))       # None under 'reference' IS 9
    for bad in (0, -1, 9.0, True, "10"):
        with pytest.raises(ValueError, match="bev_channels"):
            MV3D(phase="TEST", device="cpu", bev_channels=bad)
    cfg.LIDAR_BV_ENCODING, cfg.LIDAR_BV_FROM_SCAN = "paper", True
    try:
        assert MV3D(phase="TEST", device="cpu").params["conv1_1"][0].shape == (64, 10, 3, 3)
        assert MV3D(phase="TEST", device="cpu", bev_channels=9).params["conv1_1"][0].shape == (64, 9, 3, 3)
    finally:
        cfg.LIDAR_BV_ENCODING, cfg.LIDAR_BV_FROM_SCAN = "reference", False
    seen = []
    real = factory.MV3D
    factory.MV3D = lambda **kw: seen.append(kw) or kw
    try:
        factory.get_network("MV3D_test", bev_channels=10)
        factory.get_network("MV3D_train_3view")
    finally:
        factory.MV3D = real
    assert seen == [dict(phase="TEST", views=2, fusion=None, bev_channels=10), dict(phase="TRAIN", views=3, fusion=None)]
    # a 9-channel checkpoint: everything but conv1_1's filter loads under ignore_missing ("ignore conv1_1"), an error otherwise
    rng = np.random.RandomState(0)
    ckpt = {"conv1_1": {"weights": rng.randn(3, 3, 9, 64).astype(F32), "biases": rng.randn(64).astype(F32)},
            "conv1_2": {"weights": rng.randn(3, 3, 64, 64).astype(F32), "biases": rng.randn(64).astype(F32)}}
    path = str(tmp_path / "nine.npy")
    np.save(path, ckpt, allow_pickle=True)
    before = ten.params["conv1_1"][0].detach().clone()
    ten.load(path, ignore_missing=True)
    out = capsys.readouterr().out
    assert "ignore conv1_1" in out and "ignore conv1_2" not in out
    assert torch.equal(ten.params["conv1_1"][0].detach(), before) and torch.equal(ten.params["conv1_1"][1].detach(), torch.as_tensor(ckpt["conv1_1"]["biases"]))
    assert torch.equal(ten.params["conv1_2"][0].detach(), torch.as_tensor(ckpt["conv1_2"]["weights"]).permute(3, 2, 0, 1))
    with pytest.raises(ValueError):
        ten.load(path, ignore_missing=False)
    nine.load(path, ignore_missing=False)
    assert torch.equal(nine.params["conv1_1"][0].detach(), torch.as_tensor(ckpt["conv1_1"]["weights"]).permute(3, 2, 0, 1))


def test_restatement_agrees_with_the_oracle_where_the_encodings_meet(oracle):
    """with at most one point per cell and an integer slice count, "the last point" IS "the highest point": the restatement's height
    channels and top-intensity channel equal the oracle's reference-encoding map (itself pinned to the reference's output), so the
    restatement's range tests, cell index, slice tests and z - height_lo are the pinned ones"""
    for ranges, case in ((R.MV3D_RANGES, None), (SMALL, (0.1, 0.3, (-1.6, 1.6), (0.0, 3.2), (-2.0, 0.4))),
                         ((0.2, 0.5, -8.0, 8.0, 2.0, 18.0, -1.0, 1.0), (0.2, 0.5, (-8.0, 8.0), (2.0, 18.0), (-1.0, 1.0)))):
        (H, W, Cc), M = R.shape(ranges)
        res, _, s0, s1, f0, f1, h0, h1 = ranges
        assert (h1 - h0) / ranges[1] == M                                           # an integer slice count
        rng = np.random.RandomState(M)
        n = 1500
        pts = np.stack([rng.uniform(f0 - 1, f1 + 1, n), rng.uniform(-s1 - 1, -s0 + 1, n), rng.uniform(h0 - 0.3, h1 + 0.3, n), rng.uniform(0.05, 1, n)], 1).astype(F32)
        pts[:16, 2] = np.arange(h0, h1 + 1e-9, ranges[1]).astype(F32)[np.arange(16) % (M + 1)]      # z ON the slice limits
        pts[16:20, 2] = [NAN, INF, -INF, -0.0]
        got_all = R.raster(pts, ranges)
        occupied = got_all[..., M + 1] > 0
        # keep one row per cell: the first that the paper map counts there
        seen, keep = set(), []
        for k, p in enumerate(pts):
            one = R.raster(p[None], ranges)
            cells = np.argwhere(one[..., M + 1] > 0)
            if len(cells) and tuple(cells[0]) not in seen:
                seen.add(tuple(cells[0]))
                keep.append(k)
            elif not len(cells):
                keep.append(k)                                                       # (dropped rows stay: they must leave no trace in either)
        pts = pts[keep]
        assert len(seen) > 200 and len(seen) == occupied.sum()
        got = R.raster(pts, ranges)
        want = oracle.point_cloud_2_top(pts) if case is None else oracle.point_cloud_2_top(pts, *case)
        assert want.shape == (H, W, M + 1) and got.shape == (H, W, M + 2) and want.any()
        assert np.array_equal(bits(got[..., :M + 1]), bits(want))
        assert np.array_equal(got[..., M + 1] > 0, want.any(axis=2) | (got[..., M + 1] > 0)) and (got[..., M + 1][got[..., M + 1] > 0] == R.density_table()[1]).all()


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("P", [0, 1, P_GROUP - 1, P_GROUP, P_GROUP + 1])
def test_counts(gpu, P):
    torch, ops = gpu["torch"], gpu["ops"]
    pts = small_rows(10 + P, P)
    want = expected(pts, [0, P], SMALL)[0]
    got = ops.point_cloud_2_top_paper(torch.from_numpy(pts).cuda(), ranges=SMALL)
    assert tuple(got.shape) == (33, 33, 10) and got.dtype == torch.float32
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert P == 0 or np.count_nonzero(want) >= 3


@pytest.mark.gpu
def test_winner_rules(gpu):
    """in single cells: equal z -> the last row's reflectance; -0.0 against +0.0 (one height, the later row wins whichever zero it
    holds); a higher point in a lower-numbered row; the highest point in the top slice while lower slices are hit"""
    base = small_rows(40, 100)
    base = base[[small_cell(x, y) not in ((12, 10), (12, 11), (12, 12), (12, 13), (12, 14)) for x, y in base[:, :2]]]
    rows = np.concatenate([
        base,
        F32([[2.05, 0.65, -0.6, 0.25], [2.05, 0.65, -0.6, 0.75], [2.05, 0.65, -0.6, 0.5]]),            # cell (12, 10): equal z
        F32([[2.05, 0.55, 0.0, 0.3], [2.05, 0.55, -0.0, 0.6]]),                                       # (12, 11): +0.0 then -0.0
        F32([[2.05, 0.45, -0.0, 0.7], [2.05, 0.45, 0.0, 0.2]]),                                       # (12, 12): -0.0 then +0.0
        F32([[2.05, 0.35, 0.2, 0.9], [2.05, 0.35, 0.15, 0.1], [2.05, 0.35, -1.0, 0.4]]),              # (12, 13): the first row is the highest
        F32([[2.05, 0.25, -1.9, 0.15], [2.05, 0.25, 0.35, 0.85], [2.05, 0.25, -0.7, 0.35], [2.05, 0.25, 0.3, 0.45]]),      # (12, 14): top slice
    ])
    assert [small_cell(x, y) for x, y in rows[len(base)::3, :2]][:1] == [(12, 10)]
    want = R.raster(rows, SMALL)
    T = R.density_table()
    assert want[12, 10, 8] == F32(0.5) and want[12, 10, 4] == F32(-0.6) + F32(2.0) and want[12, 10, 9] == T[3]
    assert want[12, 11, 8] == F32(0.6) and want[12, 12, 8] == F32(0.2)
    assert bits(want[12, 11, 6]) == bits(want[12, 12, 6]) == bits(F32(0.0) - F32(-2.0))
    assert want[12, 13, 8] == F32(0.9) and want[12, 13, 7] == F32(0.2) + F32(2.0) and want[12, 13, 3] == F32(-1.0) + F32(2.0)
    assert want[12, 14, 8] == F32(0.85) and want[12, 14, 7] == F32(0.35) + F32(2.0) and want[12, 14, 0] == F32(-1.9) + F32(2.0) and want[12, 14, 4] != 0
    got = device_map(gpu, rows, ranges=SMALL)
    assert np.array_equal(bits(got), bits(want))
    # a height range spanning 0 with height_lo = 0 below it: the zeros' slice is slice 0 and the stored height is +0.0
    spans = (0.1, 0.3, -1.6, 1.6, 0.0, 3.2, 0.0, 0.6)
    zeros = F32([[2.05, 0.55, 0.0, 0.3], [2.05, 0.55, -0.0, 0.6], [1.05, 0.45, -0.0, 0.7], [1.05, 0.45, 0.0, 0.2], [1.05, 0.45, 0.31, -0.0]])
    want = R.raster(zeros, spans)
    assert want[12, 11, 2] == F32(0.6) and bits(want[12, 11, 0]) == 0 and want[12, 11, 3] == T[2] and bits(want[22, 12, 2]) == bits(F32(-0.0))
    assert np.array_equal(bits(device_map(gpu, zeros, ranges=spans)), bits(want))


@pytest.mark.gpu
def test_density_counts_and_clamp(gpu):
    counts = (1, 62, 63, 64, 300)
    rng = np.random.RandomState(3)
    rows = []
    for k, n in enumerate(counts):
        r = np.tile(F32([0.55 + 0.5 * k, 0.25, 0, 0]), (n, 1))
        r[:, 2], r[:, 3] = rng.uniform(-2, 0.39, n), rng.uniform(0.1, 1, n)
        rows.append(r)
    rows = np.concatenate(rows)[rng.permutation(sum(counts))]
    want = R.raster(rows, SMALL)
    T = R.density_table()
    for k, n in enumerate(counts):
        r, c = small_cell(0.55 + 0.5 * k, 0.25)
        assert want[r, c, 9] == T[min(n, 63)] and (n < 63) == (want[r, c, 9] < 1)
    assert np.count_nonzero(want[..., 9]) == len(counts)                            # a count of 0: every other cell, density 0
    assert np.array_equal(bits(device_map(gpu, rows, ranges=SMALL)), bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("zres", [0.3, 0.35])
def test_slice_edges(gpu, zres):
    """z exactly on height_i (rounded to f32) and its f32 neighbours, which include one ulp below height_i + zres; z == height_hi, which
    is in no slice: dropped and not counted; zres = 0.35: 6.86 slices, M = 7, where neighbouring slices meet within an ulp"""
    ranges = SMALL[:1] + (zres,) + SMALL[2:]
    (H, W, Cc), M = R.shape(ranges)
    assert (Cc, M) == ((10, 8) if zres == 0.3 else (9, 7))
    lim = np.array(R.slice_heights(ranges, M) + [R.slice_heights(ranges, M)[-1] + zres, 0.4], np.float64)
    z = np.concatenate([lim.astype(F32), np.nextafter(lim.astype(F32), F32(-9)), np.nextafter(lim.astype(F32), F32(9))])
    rows = np.zeros((len(z), 4), F32)
    rows[:, 0] = 0.15 + 0.1 * (np.arange(len(z)) % 30)                              # one cell each
    rows[:, 1] = -1.05 + 0.1 * (np.arange(len(z)) // 30)
    rows[:, 2], rows[:, 3] = z, 0.5
    assert len({small_cell(x, y) for x, y in rows[:, :2]}) == len(z)
    want = R.raster(rows, ranges)
    hi = rows[z == F32(0.4)][0]
    # z == height_hi: nothing, not even a count -- unless the last of np.arange's slices reaches past it (zres = 0.35: [0.1, 0.45))
    assert want[small_cell(hi[0], hi[1])].any() == (zres == 0.35)
    hit = np.count_nonzero(want[..., :M], axis=2)
    dens = want[..., M + 1] > 0
    assert hit.max() <= 2 and 0 < np.count_nonzero(dens) < len(z) and not (hit > 0)[~dens].any()
    lo = rows[z == F32(-2.0)][0]                                                     # z == height_lo: kept, its height channel holds 0.0
    assert (hit == 0)[dens].sum() == 1 and dens[small_cell(lo[0], lo[1])] and hit[small_cell(lo[0], lo[1])] == 0
    assert np.array_equal(bits(device_map(gpu, rows, ranges=ranges)), bits(want))
    # a pile of points on one slice limit in ONE cell: counted once each, even where a point falls into two slices
    pile = np.tile(F32([1.05, 0.05, 0, 0.5]), (len(z), 1))
    pile[:, 2] = z
    want = R.raster(pile, ranges)
    assert np.array_equal(bits(device_map(gpu, pile, ranges=ranges)), bits(want))


@pytest.mark.gpu
def test_dropped_rows_and_cells_outside_the_map(gpu):
    base = small_rows(50, 200)
    base = base[base[:, 0] > 0.2]
    dropped = F32([[NAN, 1, -1, .5], [1, NAN, -1, .5], [1, 1, NAN, .5], [INF, 1, -1, .5], [-INF, 1, -1, .5], [1, INF, -1, .5], [1, -INF, -1, .5],
                   [1, 1, INF, .5], [1, 1, -INF, .5], [0, 1, -1, .5], [3.2, 1, -1, .5], [1, 1.6, -1, .5], [1, -1.6, -1, .5], [1, 1, 0.4, .5], [1, 1, -2.1, .5]])
    want = R.raster(base, SMALL)
    assert np.array_equal(bits(R.raster(np.concatenate([base, dropped]), SMALL)), bits(want))
    assert np.array_equal(bits(device_map(gpu, np.concatenate([dropped[:7], base, dropped[7:]]), ranges=SMALL)),
                          bits(R.raster(np.concatenate([dropped[:7], base, dropped[7:]]), SMALL)))
    # a reflectance of NaN / inf is data: copied bit for bit
    odd = F32([[1.05, 0.05, -1, NAN], [2.05, 0.05, -1, INF], [2.55, 0.05, -1, -0.0]])
    got = device_map(gpu, odd, ranges=SMALL)
    assert np.array_equal(bits(got), bits(R.raster(odd, SMALL))) and np.isnan(got[..., 8]).sum() == 1
    # the cell outside the map: no error while the row is in no slice, IndexError once it is
    quiet = np.concatenate([base, F32([[0.07, 1.0, 5.0, 0.5], [0.07, 1.0, NAN, 0.5]])])
    want = R.raster(quiet, OUTSIDE)
    assert want.shape == (32, 33, 10) and want.any()
    assert np.array_equal(bits(device_map(gpu, quiet, ranges=OUTSIDE)), bits(want))
    loud = np.concatenate([base, F32([[0.07, 1.0, -1.0, 0.5]])])
    with pytest.raises(IndexError):
        R.raster(loud, OUTSIDE)
    with pytest.raises(IndexError, match="point_cloud_2_top_paper"):
        device_map(gpu, loud, ranges=OUTSIDE)
    assert np.array_equal(bits(device_map(gpu, quiet, ranges=OUTSIDE)), bits(want))  # (the status word is cleared by every call)


@pytest.mark.gpu
def test_batch_frames_offsets_and_out(gpu):
    torch, ops = gpu["torch"], gpu["ops"]
    sizes = (257, 0, 300)
    offsets = np.cumsum((0,) + sizes).astype(np.int32)
    pts = small_rows(60, int(offsets[-1]))
    pts[256], pts[257] = [2.05, 0.65, -0.95, 0.125], [2.05, 0.65, -0.95, 0.875]     # neighbours in the buffer, in different frames
    want = expected(pts, offsets, SMALL)
    assert want[0][12, 10, 8] == F32(0.125) and want[2][12, 10, 8] == F32(0.875) and not want[1].any()
    d_pts = torch.from_numpy(pts).cuda()
    got = ops.point_cloud_2_top_paper(d_pts, offsets, ranges=SMALL)
    assert tuple(got.shape) == (3, 33, 33, 10) and np.array_equal(bits(got.cpu().numpy()), bits(want))
    for b in (0, 2):                                                                 # frame b == the single-frame call on its rows
        one = ops.point_cloud_2_top_paper(d_pts[offsets[b]:offsets[b + 1]], ranges=SMALL)
        assert torch.equal(one.view(torch.int32), got[b].view(torch.int32))
    d_off = torch.from_numpy(offsets).cuda()                                         # device offsets
    assert np.array_equal(bits(ops.point_cloud_2_top_paper(d_pts, d_off, ranges=SMALL).cpu().numpy()), bits(want))
    d_off = torch.tensor([257, 557], dtype=torch.int32, device="cuda")              # unchecked: rows in front of offsets[0] belong to no frame
    assert np.array_equal(bits(ops.point_cloud_2_top_paper(d_pts, d_off, ranges=SMALL).cpu().numpy()), bits(want[2:]))
    # out = a run of frames that starts at an odd element of a larger buffer; sentinels on either side
    n = 33 * 33 * 10
    for lead, frames in ((1, slice(0, 3)), (3, slice(2, 3)), (2, slice(0, 1))):
        nb = frames.stop - frames.start
        flat = torch.full((lead + nb * n + 5,), -7.0, device="cuda")
        out = flat[lead:lead + nb * n].view(nb, 33, 33, 10)
        assert out.data_ptr() % 16 == 4 * lead
        lo, hi = offsets[frames.start], offsets[frames.stop]
        ws = torch.empty(ops.point_cloud_2_top_paper_workspace_bytes(nb, SMALL) + 64, dtype=torch.uint8, device="cuda").fill_(255)
        res = ops.point_cloud_2_top_paper(d_pts[lo:hi], offsets[frames.start:frames.stop + 1] - lo, ranges=SMALL, out=out, workspace=ws[:-64])
        assert res.data_ptr() == out.data_ptr()
        host = flat.cpu().numpy()
        assert np.array_equal(bits(host[lead:lead + nb * n].reshape(nb, 33, 33, 10)), bits(want[frames]))
        assert (host[:lead] == -7).all() and (host[lead + nb * n:] == -7).all() and (ws[-64:] == 255).all()
    with pytest.raises(ValueError, match="out must be"):
        ops.point_cloud_2_top_paper(d_pts, offsets, ranges=SMALL, out=torch.zeros((2, 33, 33, 10), device="cuda"))
    with pytest.raises(ValueError, match="workspace of"):
        ops.point_cloud_2_top_paper(d_pts, offsets, ranges=SMALL, workspace=torch.zeros(3 * 33 * 33 * 8 - 8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="16-byte"):
        ops.point_cloud_2_top_paper(d_pts, offsets, ranges=SMALL, workspace=torch.zeros(3 * 33 * 33 * 8 + 8, dtype=torch.uint8, device="cuda")[8:])


def corner_frame(seed):
    """200 random rows inside CORNER's ranges, then rows into the first cell (slices 0, 1, 2) and the last cell (slices 2, 4)"""
    rng = np.random.RandomState(seed)
    body = np.stack([rng.uniform(2.3, 17.9, 200), rng.uniform(-7.7, -0.5, 200), rng.uniform(-1, 1.2, 200), rng.uniform(0.1, 1, 200)], 1)
    first = [[18.05, -0.35, z, 0.3 + 0.1 * k] for k, z in enumerate((-0.9, -0.4, 0.1))]
    last = [[2.1, -7.9, z, 0.6 + 0.1 * k] for k, z in enumerate((0.1, 1.1))]
    return np.concatenate([body, first, last]).astype(F32)


@pytest.mark.gpu
def test_keys_in_the_scalar_head_and_tail(gpu):
    """runs of frames that start 12, 4, 8 and 0 mod 16 bytes into a batch buffer (one frame is 4 mod 16 bytes here): the resolve's
    scalar head and tail hold keys -- heights of the first cell; the top slice, winner and count of the last -- and are resolved"""
    torch, ops = gpu["torch"], gpu["ops"]
    frames = [corner_frame(90 + b) for b in range(4)]
    want = np.stack([R.raster(f, CORNER) for f in frames])
    assert want.shape == (4, 81, 39, 7)
    flat = want.reshape(4, -1)
    assert (flat[:, :3] != 0).all() and (flat[:, -3:] != 0).all()                   # the head and tail elements of every frame hold values
    for lo, hi, head, tail in ((3, 4, 1, 0), (1, 3, 3, 3), (2, 3, 2, 3), (0, 1, 0, 1)):
        pts = np.concatenate(frames[lo:hi])
        offsets = np.cumsum([0] + [len(f) for f in frames[lo:hi]]).astype(np.int32)
        buf = torch.full((4, 81, 39, 7), -7.0, device="cuda")
        ops.point_cloud_2_top_paper(torch.from_numpy(pts).cuda(), torch.from_numpy(offsets).cuda(), ranges=CORNER, out=buf[lo:hi])
        n_head = (-buf[lo:hi].data_ptr() % 16) // 4
        assert (n_head, ((hi - lo) * 81 * 39 * 7 - n_head) % 4) == (head, tail)
        host = buf.cpu().numpy()
        assert np.array_equal(bits(host[lo:hi]), bits(want[lo:hi])) and (host[:lo] == -7).all() and (host[hi:] == -7).all()


@pytest.mark.gpu
def test_contention_is_deterministic(gpu):
    """5 000 rows on 4 cells, many with equal heights: run twice, bit-equal, and equal to the restatement"""
    rng = np.random.RandomState(7)
    rows = np.zeros((5000, 4), F32)
    rows[:, 0] = 1.05 + 0.1 * rng.randint(0, 2, 5000)
    rows[:, 1] = 0.05 + 0.1 * rng.randint(0, 2, 5000)
    rows[:, 2] = rng.choice(np.linspace(-2, 0.39, 40).astype(F32), 5000)            # 40 heights: ties everywhere
    rows[:, 3] = rng.uniform(0.1, 1, 5000)
    want = R.raster(rows, SMALL)
    assert np.count_nonzero(want[..., 9]) == 4 and (want[..., 9][want[..., 9] > 0] == 1).all()
    a, b = device_map(gpu, rows, ranges=SMALL), device_map(gpu, rows, ranges=SMALL)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(want))
    assert np.array_equal(bits(device_map(gpu, rows[::-1].copy(), ranges=SMALL))[..., :8], bits(want)[..., :8])      # heights: no order at all


@pytest.fixture(scope="module")
def default_cloud():
    """3 000 rows of a synthetic scan and their (601, 601, 10) map: computed once, never written to"""
    pts = synth.point_cloud(70, 3000)
    want = expected(pts, [0, len(pts)])[0]
    pts.setflags(write=False)
    want.setflags(write=False)
    return pts, want


@pytest.mark.gpu
def test_default_ranges(gpu, default_cloud):
    torch, ops = gpu["torch"], gpu["ops"]
    pts, want = default_cloud
    got = ops.point_cloud_2_top_paper(torch.from_numpy(np.array(pts)).cuda())
    assert tuple(got.shape) == ops.BEV_PAPER_SHAPE == want.shape and np.count_nonzero(want) > 3000
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    from mv3d_tf_amd.utils.read_lidar import point_cloud_2_top_paper
    assert np.array_equal(bits(point_cloud_2_top_paper(np.array(pts))), bits(want))                  # the numpy-in form
    small = point_cloud_2_top_paper(small_rows(1, 50), side_range=(-1.6, 1.6), fwd_range=(0.0, 3.2))
    assert np.array_equal(bits(small), bits(R.raster(small_rows(1, 50), SMALL)))


@pytest.mark.gpu
def test_raster_commutes_with_the_mirror(gpu):
    """the paper map of the cloud with y negated == mirror_columns of the cloud's map, bit for bit (the column is int(-y / res), odd in
    y; the side filter is the open (-30, 30)); points as tests/test_mirror.py::test_bev_raster_commutes_with_the_mirror chooses them"""
    torch, ops = gpu["torch"], gpu["ops"]
    pts = synth.point_cloud(0, P=20000)
    ys = F32([0, 0.05, -0.05, 0.1, -0.1, 29.99, -29.99, 30, -30])
    pts[5000:5000 + len(ys), 1] = ys
    pts[5000:5000 + len(ys), 0] = F32(10.0) + np.arange(len(ys), dtype=F32)
    pts[5000:5000 + len(ys), 2] = F32(-1.0)
    pts[6000:6040, :2] = F32([33.33, 4.21])
    pts[6040:6080, :2] = F32([33.33, -4.21])
    top = ops.point_cloud_2_top_paper(torch.from_numpy(pts).cuda())
    top_neg = ops.point_cloud_2_top_paper(torch.from_numpy(pts * F32([1, -1, 1, 1])).cuda())
    assert torch.count_nonzero(top).item() > 1000 and not torch.equal(top, top_neg)
    assert torch.equal(ops.mirror_columns(top.clone()).view(torch.int32), top_neg.view(torch.int32))


@pytest.mark.gpu
def test_capture_and_replay(gpu):
    """ONE linear graph with out= and workspace= given, replayed after the cloud's contents and row counts change"""
    torch, ops = gpu["torch"], gpu["ops"]
    cap = 2048
    fillings = []
    for seed, sizes in ((60, (500, 700)), (61, (900, 1100)), (62, (0, 3))):
        pts = synth.point_cloud(seed, cap)                                          # the whole buffer is refilled: the rows behind offsets[B] are stale points
        offsets = np.cumsum((0,) + sizes).astype(np.int32)
        fillings.append((pts, offsets, expected(pts, offsets)))
    buf = torch.from_numpy(fillings[0][0]).cuda()
    d_off = torch.from_numpy(fillings[0][1]).cuda()
    big = torch.zeros((4, 601, 601, 10), device="cuda")
    out = big[1:3]                                                                  # 8 mod 16 bytes
    ws = torch.empty(ops.point_cloud_2_top_paper_workspace_bytes(2), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.point_cloud_2_top_paper(buf, d_off, out=out, workspace=ws)              # (warm-up: the code object is loaded outside the capture)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.point_cloud_2_top_paper(buf, d_off, out=out, workspace=ws)
    for pts, offsets, want in reversed(fillings):
        buf.copy_(torch.from_numpy(pts))
        d_off.copy_(torch.from_numpy(offsets))
        big.fill_(-1.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        host = big.cpu().numpy()
        assert out.data_ptr() % 16 == 8
        assert np.array_equal(bits(host[1:3]), bits(want)) and (host[0] == -1).all() and (host[3] == -1).all()


@pytest.mark.gpu
def test_occupancy_means_a_kept_point(gpu, default_cloud):
    """with every reflectance > 0 the two maps mark the same anchors; a cell whose only return sits at z == height_lo with reflectance 0
    is all zeros in the reference map and holds a density in the paper map"""
    torch, ops = gpu["torch"], gpu["ops"]
    pts = np.array(default_cloud[0])
    pts[:, 3] = np.maximum(pts[:, 3], F32(0.01))
    d = torch.from_numpy(pts).cuda()
    ref, paper = ops.point_cloud_2_top_batch(d), ops.point_cloud_2_top_paper(d)
    m_ref, m_paper = ops.anchor_occupancy(ref, 75, 75), ops.anchor_occupancy(paper, 75, 75)
    assert torch.equal(m_ref, m_paper) and 0 < int(m_ref.sum()) < m_ref.numel()
    lone = torch.tensor([[45.05, 20.05, -2.0, 0.0]], device="cuda")
    ref, paper = ops.point_cloud_2_top_batch(lone), ops.point_cloud_2_top_paper(lone)
    assert not ref.any() and int(torch.count_nonzero(paper)) == 1 and float(paper.max()) == float(R.density_table()[1])
    assert int(ops.anchor_occupancy(ref, 75, 75).sum()) == 0 and int(ops.anchor_occupancy(paper, 75, 75).sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_input_layer_at_ten_channels(gpu, dtype):
    """conv1_1 of the MFMA trunks at c_in = 10, as trunk.MfmaTrunks runs it (channels zero-padded to 16 for 16-bit maps, to one
    32-channel K step for f32), against torch's f32 convolution of the rounded operands; tolerance as tests/test_conv_mfma.py states it:
    2e-3 * max|want| for 16-bit maps, 2e-5 * max|want| for f32 maps"""
    torch, ops = gpu["torch"], gpu["ops"]
    import torch.nn.functional as F
    T = getattr(torch, dtype)
    B, H, W, cin, cout = 2, 40, 52, 10, 64
    g = torch.Generator(device="cuda").manual_seed(10)
    x = torch.randn((B, H, W, cin), device="cuda", generator=g)
    w = torch.randn((cout, cin, 3, 3), device="cuda", generator=g) * 0.3
    b = torch.randn((cout,), device="cuda", generator=g)
    want = F.relu(F.conv2d(x.to(T).float().permute(0, 3, 1, 2), w.to(T).float(), b, padding=1)).permute(0, 2, 3, 1)
    if T == torch.float32:
        xf = ops.frame_nhwc_f16(x, ops.framed_buffer(B, H, W, 32, x.device, T))
        got = ops.conv3x3_f16(xf, ops.pack_conv3x3_weights(w, 32, dtype=T), b)[:, 1:-1, 1:-1]
    else:
        xf = ops.frame_nhwc_f16(x, ops.framed_buffer(B, H, W, 16, x.device, T))
        got = ops.conv3x3_f16(xf, ops.pack_conv3x3_weights_input_layer(w, T), b)[:, 1:-1, 1:-1]
    torch.cuda.synchronize()
    err, scale = float((got.float() - want).abs().max()), float(want.abs().max())
    print("c_in = 10 input layer, %s: max error %.3e, max|want| %.3e" % (dtype, err, scale))
    assert err <= (2e-5 if T == torch.float32 else 2e-3) * scale, (err, scale)
    # the channel the paper's map adds does reach the output
    x2 = x.clone()
    x2[..., 9] += 1.0
    xf2 = ops.frame_nhwc_f16(x2, ops.framed_buffer(B, H, W, xf.shape[3], x.device, T))
    packed = ops.pack_conv3x3_weights(w, 32, dtype=T) if T == torch.float32 else ops.pack_conv3x3_weights_input_layer(w, T)
    assert not torch.equal(ops.conv3x3_f16(xf2, packed, b), ops.conv3x3_f16(xf, packed, b))


def _entry(**extra):
    e = {"image": np.arange(8 * 12 * 3, dtype=np.uint8).reshape(8, 12, 3), "calib": np.arange(48, dtype=np.float64).reshape(4, 12),
         "gt_classes": np.array([1, 0], np.int32), "boxes": np.arange(8, dtype=F32).reshape(2, 4), "boxes_bv": np.arange(8, dtype=F32).reshape(2, 4) + 1,
         "boxes_3D": np.arange(12, dtype=F32).reshape(2, 6), "boxes_corners": np.arange(48, dtype=F32).reshape(2, 24), "flipped": False}
    e.update(extra)
    return e


@pytest.mark.gpu
def test_feeds_and_network_under_the_key(gpu, default_cloud, tmp_path, monkeypatch):
    torch, ops = gpu["torch"], gpu["ops"]
    from mv3d_tf_amd.fast_rcnn import detect_batch
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.networks import get_network
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    pts, want = np.array(default_cloud[0]), default_cloud[1]
    d_pts = torch.from_numpy(pts).cuda()
    want_dev = ops.point_cloud_2_top_paper(d_pts)
    want_mirror = ops.point_cloud_2_top_paper(torch.from_numpy(pts * F32([1, -1, 1, 1])).cuda())
    assert np.array_equal(bits(want_dev.cpu().numpy()), bits(want))
    path = str(tmp_path / "000000.bin")
    pts.tofile(path)
    uploads = []
    real_dev = ops._dev
    monkeypatch.setattr(ops, "_dev", lambda t, *a, **kw: (uploads.append(np.shape(t)) if not isinstance(t, torch.Tensor) else None) or real_dev(t, *a, **kw))
    saved = dict(cfg.TEST)
    cfg.LIDAR_BV_FROM_SCAN, cfg.LIDAR_BV_ENCODING = True, "paper"
    try:
        for fv_on in (False, True):
            cfg.FRONT_VIEW_INPUT = fv_on
            for entry in (_entry(velodyne_path=path), _entry(velodyne=pts, flipped=True)):
                del uploads[:]
                blobs = get_minibatch([entry], 2)
                bev = blobs["lidar_bv_data"]
                assert isinstance(bev, torch.Tensor) and bev.is_cuda and tuple(bev.shape) == (1, 601, 601, 10) and bev.dtype == torch.float32
                assert torch.equal(bev[0].view(torch.int32), (want_mirror if entry["flipped"] else want_dev).view(torch.int32))
                assert np.array_equal(blobs["im_info"], [[601, 601, 1]]) and ("lidar_fv_data" in blobs) == fv_on
                assert [s for s in uploads if len(s) == 2 and s[1] == 4] == [(3000, 4)]                  # ONE upload of the scan
                if fv_on:
                    cloud = torch.from_numpy(pts * F32([1, -1, 1, 1])).cuda() if entry["flipped"] else d_pts
                    assert torch.equal(blobs["lidar_fv_data"][0], ops.point_cloud_2_front(cloud))
        cfg.FRONT_VIEW_INPUT = False
        clouds = [pts[:1000], pts[1000:]]
        del uploads[:]
        feed = detect_batch.scan_feed(clouds, True, True)
        two = ops.point_cloud_2_top_paper(d_pts, [0, 1000, 3000])
        assert tuple(feed["lidar_bv_data"].shape) == (2, 601, 601, 10) and torch.equal(feed["lidar_bv_data"].view(torch.int32), two.view(torch.int32))
        assert tuple(feed["lidar_fv_data"].shape) == (2, 64, 512, 3) and uploads == [(3000, 4)]
        # the network: ten channels by the key, ROIs from the paper map, a nine-channel map refused
        net = get_network("MV3D_test")
        assert net.bev_channels == 10 and net.params["conv1_1"][0].shape == (64, 10, 3, 3)
        net10 = get_network("MV3D_test", bev_channels=10)
        with torch.no_grad():
            net10.params["rpn_cls_score"][0].mul_(40.0)
            net10.params["rpn_bbox_pred"][0].mul_(5.0)
        cfg.TEST.update(RPN_PRE_NMS_TOP_N=600, RPN_POST_NMS_TOP_N=50)
        im = np.random.RandomState(0).randint(0, 255, (1, 48, 160, 3)).astype(F32)
        base = {"image_data": im, "im_info": np.array([[601, 601, 1]], F32), "calib": synth.KITTI_CALIB}
        with torch.no_grad():
            L = net10.forward(dict(base, lidar_bv_data=want_dev[None]))
            rois = L["rois"]
            assert isinstance(rois, tuple) and 0 < rois[0].shape[0] <= 50 and rois[2].shape[1] == 7 and bool(torch.isfinite(L["cls_prob"]).all())
            assert tuple(L["conv1_1"].shape) == (1, 601, 601, 64)
            with pytest.raises(ValueError, match="lidar_bv_data has 9 channels"):
                net10.forward(dict(base, lidar_bv_data=ops.point_cloud_2_top_batch(d_pts)[None]))
    finally:
        cfg.LIDAR_BV_FROM_SCAN, cfg.LIDAR_BV_ENCODING, cfg.FRONT_VIEW_INPUT = False, "reference", False
        cfg.TEST.clear()
        cfg.TEST.update(saved)
