"""Bird's-eye-view input from raw scans: ops.point_cloud_2_top_batch / mv3d_point_cloud_2_top_batch against
oracle.point_cloud_2_top of each frame's rows (pinned to the reference's own output by the point_cloud_top_* fixtures), and the
layers that feed `lidar_bv_data` from Velodyne scans under cfg.LIDAR_BV_FROM_SCAN.  Every comparison is equality of the int32 views;
nothing has a tolerance.  Every non-empty frame's expected map is asserted to have non-zero entries, so an all-zero output cannot pass."""
import ctypes as C

import numpy as np
import pytest

import front_view_raster_restatement as R
from mv3d_tf_amd import synth

F32 = np.float32
P_GROUP = 256                      # threads per workgroup of the scatter kernel (csrc/bev_raster.hip)
NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def kept_rows(seed, P):
    """P rows of synth.point_cloud(seed) that the MV3D ranges keep (inside the open x / y limits, inside a height slice)"""
    c = synth.point_cloud(seed, 4 * P + 64)
    c = c[(c[:, 0] > 0) & (c[:, 0] < 60) & (c[:, 1] > -30) & (c[:, 1] < 30) & (c[:, 2] >= -2) & (c[:, 2] < 0.39)]
    assert len(c) >= P
    return np.ascontiguousarray(c[:P])


def ranges_args(case):
    res, zres, side, fwd, hr = case
    return (res, zres, side[0], side[1], fwd[0], fwd[1], hr[0], hr[1])


def expected(oracle, pts, offsets, case=None):
    """(B, H, W, C) from the oracle, frame by frame on the frame's rows alone; a non-empty frame must leave something in its map"""
    maps = []
    for b in range(len(offsets) - 1):
        rows = pts[offsets[b]:offsets[b + 1]]
        maps.append(oracle.point_cloud_2_top(rows) if case is None else oracle.point_cloud_2_top(rows, *case))
        assert maps[-1].any() == (len(rows) > 0), "frame %d: a non-empty frame's expected map must have non-zero entries" % b
    return np.stack(maps)


def cell(x, y):
    """(row, column) of the MV3D map a kept point falls into (read_lidar.py:96-103)"""
    return int(F32(-x) / F32(0.1)) + 600, int(F32(-y) / F32(0.1)) + 300


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops
    return {"torch": torch, "ops": ops}


def device_maps(gpu, pts, offsets=None, **kw):
    return gpu["ops"].point_cloud_2_top_batch(gpu["torch"].from_numpy(np.array(pts, F32)).cuda(), offsets, **kw).cpu().numpy()


@pytest.fixture(scope="module")
def four(oracle):
    """four random clouds of 5 000 rows back to back and their maps: computed once, never written to"""
    pts = np.concatenate([synth.point_cloud(20 + b, 5000) for b in range(4)])
    offsets = np.arange(5, dtype=np.int32) * 5000
    want = expected(oracle, pts, offsets)
    for a in (pts, offsets, want):
        a.setflags(write=False)
    return {"pts": pts, "offsets": offsets, "want": want}


# ---------------------------------------------------------------------------------------------------- CPU
def _entry(**extra):
    e = {"image": np.arange(8 * 12 * 3, dtype=np.uint8).reshape(8, 12, 3), "calib": np.arange(48, dtype=np.float64).reshape(4, 12),
         "gt_classes": np.array([1, 0], np.int32), "boxes": np.arange(8, dtype=F32).reshape(2, 4), "boxes_bv": np.arange(8, dtype=F32).reshape(2, 4) + 1,
         "boxes_3D": np.arange(12, dtype=F32).reshape(2, 6), "boxes_corners": np.arange(48, dtype=F32).reshape(2, 24), "flipped": False}
    e.update(extra)
    return e


class _Imdb:
    """what prepare_roidb asks of a dataset"""

    def __init__(self):
        self.roidb = [{"gt_overlaps": np.array([[0, 1.0], [0, 0]], F32)} for _ in range(2)]
        self.asked = []

    def image_path_at(self, i): return "/images/%06d.png" % i
    def lidar_path_at(self, i): self.asked.append(i); return "/lidar_bv/%06d.npy" % i
    def calib_at(self, i): return np.full((4, 12), i, F32)
    def velodyne_path_at(self, i): return "/velodyne/%06d.bin" % i


def test_key_defaults_off_and_nothing_changes(tmp_path):
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    from mv3d_tf_amd.roi_data_layer.roidb import prepare_roidb
    assert cfg.LIDAR_BV_FROM_SCAN is False
    bev = np.random.RandomState(0).random_sample((8, 601, 9)).astype(F32)
    np.save(str(tmp_path / "bev.npy"), bev)
    for entry in (_entry(lidar_bv=bev, velodyne=synth.point_cloud(1, 64)),
                  _entry(lidar_bv_path=str(tmp_path / "bev.npy"), velodyne_path=str(tmp_path / "no_such_scan.bin"))):
        blobs = get_minibatch([entry], 2)
        assert set(blobs) == {"image_data", "lidar_bv_data", "calib", "gt_boxes", "gt_boxes_bv", "gt_boxes_3d", "gt_boxes_corners", "im_info"}
        assert all(isinstance(v, np.ndarray) for v in blobs.values())
        assert blobs["lidar_bv_data"].dtype == F32 and np.array_equal(blobs["lidar_bv_data"], bev[None])
        assert blobs["image_data"].dtype == F32 and np.array_equal(blobs["image_data"], (entry["image"].astype(F32) - cfg.PIXEL_MEANS).astype(F32)[None])
        assert blobs["im_info"].dtype == F32 and np.array_equal(blobs["im_info"], [[8, 601, 1]])
        assert blobs["calib"] is entry["calib"]
        assert blobs["gt_boxes"].dtype == F32 and np.array_equal(blobs["gt_boxes"], [[0, 1, 2, 3, 1]])
        assert np.array_equal(blobs["gt_boxes_bv"], [[1, 2, 3, 4, 1]]) and blobs["gt_boxes_3d"].shape == (1, 7) and blobs["gt_boxes_corners"].shape == (1, 25)
    imdb = _Imdb()
    roidb = prepare_roidb(imdb)
    assert imdb.asked == [0, 1]
    for i, e in enumerate(roidb):
        assert set(e) == {"gt_overlaps", "image_path", "lidar_bv_path", "calib", "velodyne_path", "max_overlaps", "max_classes"}
        assert e["lidar_bv_path"] == "/lidar_bv/%06d.npy" % i and e["velodyne_path"] == "/velodyne/%06d.bin" % i
        assert np.array_equal(e["max_overlaps"], [1, 0]) and np.array_equal(e["max_classes"], [1, 0])


def test_prepare_roidb_with_the_key_on():
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.roi_data_layer.roidb import prepare_roidb

    class NoMaps(_Imdb):
        def lidar_path_at(self, i): raise AssertionError("no stored map may be asked for")

    class NoScans:
        image_path_at = lidar_path_at = calib_at = staticmethod(lambda i: None)

        @property
        def roidb(self): raise AssertionError("refused before the loop")

    cfg.LIDAR_BV_FROM_SCAN = True
    try:
        roidb = prepare_roidb(NoMaps())
        assert [e["velodyne_path"] for e in roidb] == ["/velodyne/000000.bin", "/velodyne/000001.bin"]
        assert all("lidar_bv_path" not in e and e["image_path"] and "max_classes" in e for e in roidb)
        with pytest.raises(ValueError, match="velodyne_path_at"):
            prepare_roidb(NoScans())
    finally:
        cfg.LIDAR_BV_FROM_SCAN = False


def test_point_cloud_2_top_batch_refuses_bad_arguments_before_any_launch():
    import torch
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops
    assert ops.BEV_SHAPE == (601, 601, 9)
    good = np.zeros((3, 4), F32)
    odd = ranges_args(synth.BEV_RANGE_CASES["odd"])
    for exc, args in ((TypeError, (np.zeros((3, 4)),)), (TypeError, (np.zeros((3, 4), np.int32),)), (TypeError, (torch.zeros(3, 4, dtype=torch.float16),)),
                      (ValueError, (np.zeros((3, 3), F32),)), (ValueError, (np.zeros((12,), F32),)), (ValueError, (np.zeros((1, 3, 4), F32),)),
                      (ValueError, (torch.zeros(3, 4),)),
                      (TypeError, (good, [0.0, 3.0])), (TypeError, (good, torch.zeros(2, dtype=torch.int64))),
                      (ValueError, (good, [0, 2, 1])), (ValueError, (good, [0, 4])), (ValueError, (good, [-1, 3])), (ValueError, (good, [[0, 3]])),
                      (ValueError, (good, [0])), (ValueError, (good, np.zeros(ops.FV_MAX_FRAMES + 2, np.int32))),      # B = 0, B = 1025
                      (ValueError, (good, torch.zeros(2, dtype=torch.int32))),
                      (ValueError, (good, None, (0.1, 0.3, 30., -30., 0., 60., -2., 0.4))), (ValueError, (good, None, (0.1, 0.001, -30., 30., 0., 60., -2., 0.4))),
                      (TypeError, (good, None, None, np.zeros(ops.BEV_SHAPE, F32))), (TypeError, (good, None, None, torch.zeros((2, 2, 9), dtype=torch.float64))),
                      (TypeError, (good, None, odd, torch.zeros((243, 203, 12), dtype=torch.float16))),
                      (ValueError, (good, None, None, torch.zeros((600, 601, 9)))), (ValueError, (good, [0, 1, 3], None, torch.zeros((1, 601, 601, 9)))),
                      (ValueError, (good, None, odd, torch.zeros(ops.BEV_SHAPE)))):
        with pytest.raises(exc, match="point_cloud_2_top_batch"):
            ops.point_cloud_2_top_batch(*args)
    L, lib = ops.lib(), ops._lib
    A = 4096                                                                         # a non-NULL, aligned "pointer" (never dereferenced)
    r8 = (C.c_double * 8)(*odd)
    bad = (C.c_double * 8)(0.1, 0.3, 30.0, -30.0, 0.0, 60.0, -2.0, 0.4)
    for fn in (L.mv3d_point_cloud_2_top_batch, L.mv3d_point_cloud_2_top_batch_dense):
        for args in ((A, A, -1, 4, None, A, None), (A, A, ops.FV_MAX_FRAMES + 1, 4, None, A, None), (A, A, 1, -1, None, A, None),
                     (None, A, 1, 4, None, A, None), (A, None, 2, 4, None, A, None), (A, A, 1, 4, None, None, None),
                     (A + 4, A, 1, 4, None, A, None), (A, A + 2, 1, 4, None, A, None), (A, A, 1, 4, None, A + 2, None),
                     (A, A, 1, 4, r8, A, None), (A, A, 1, 4, r8, A, A + 2), (A, A, 1, 4, bad, A, A)):
            assert fn(*args, None) == lib.ERR_INVALID_ARG, args
        assert fn(None, None, 0, 0, None, None, None, None) == lib.OK                # no frame: nothing to do


def test_single_cloud_entries_refuse_bad_arguments_before_any_launch():
    """mv3d_point_cloud_2_top / _ranges are the batched body on one frame and keep their own refusals (include/mv3d_hip.h): 2^27 rows
    or more, and a map that is not 16-byte aligned, which the batched entry takes"""
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops
    L, lib = ops.lib(), ops._lib
    A = 4096                                                                         # a non-NULL, aligned "pointer" (never dereferenced)
    odd = ranges_args(synth.BEV_RANGE_CASES["odd"])
    cases = ((A, -1, A), (A, 1 << 27, A), (None, 4, A), (A, 4, None), (A + 4, 4, A), (A, 4, A + 4))
    for pts, P, top in cases:
        assert L.mv3d_point_cloud_2_top(pts, P, top, None) == lib.ERR_INVALID_ARG, (pts, P, top)
        assert L.mv3d_point_cloud_2_top_ranges(pts, P, *odd, top, A, None) == lib.ERR_INVALID_ARG, (pts, P, top)
    assert L.mv3d_point_cloud_2_top_ranges(A, 4, *odd, A, None, None) == lib.ERR_INVALID_ARG             # no status word
    for bad in ((0.1, 0.3, 30., -30., 0., 60., -2., 0.4), (0.1, 0.001, -30., 30., 0., 60., -2., 0.4)):   # inverted; 2400 slices
        assert L.mv3d_point_cloud_2_top_ranges(A, 4, *bad, A, A, None) == lib.ERR_INVALID_ARG, bad


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("P", [0, 1, P_GROUP - 1, P_GROUP, P_GROUP + 1])
def test_counts(gpu, oracle, P):
    torch, ops = gpu["torch"], gpu["ops"]
    pts = kept_rows(10 + P, P) if P else np.zeros((0, 4), F32)
    want = expected(oracle, pts, [0, P])[0]
    d_pts = torch.from_numpy(pts).cuda()
    got = ops.point_cloud_2_top_batch(d_pts)
    assert tuple(got.shape) == ops.BEV_SHAPE and got.dtype == torch.float32
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert np.array_equal(bits(ops.point_cloud_2_top(d_pts).cpu().numpy()), bits(want))
    assert P == 0 or np.count_nonzero(want) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(257, 0, 300), (256, 1, 255)])
def test_frame_boundaries(gpu, oracle, sizes):
    offsets = np.cumsum((0,) + sizes).astype(np.int32)
    pts = synth.point_cloud(3, 2000)[:offsets[-1]].copy()
    last0, first_next = offsets[1] - 1, offsets[1] if sizes[1] else offsets[2]     # two neighbours in the buffer, in different frames
    nxt = 1 if sizes[1] else 2
    pts[last0] = [55.55, -25.55, -0.95, 0.125]
    pts[first_next] = [55.55, -25.55, -0.95, 0.875]
    want = expected(oracle, pts, offsets)
    r, c = cell(55.55, -25.55)
    assert want[0][r, c, 8] == F32(0.125) and want[nxt][r, c, 8] == F32(0.875) and want[0][r, c, 3] == want[nxt][r, c, 3] == F32(-0.95) + F32(2.0)
    got = device_maps(gpu, pts, offsets)
    assert got.shape == (3, 601, 601, 9)
    assert np.array_equal(bits(got), bits(want))
    assert sizes[1] or not got[1].any()                                             # the empty frame shows nobody's points
    assert not np.array_equal(got[0], got[2])


@pytest.mark.gpu
def test_winner_rules_per_frame(gpu, oracle):
    """frame 1 of a batch (the index within the frame is not the row of the buffer): forty rows into one cell and slice; an earlier row
    in a higher slice and a later one in a lower slice of one cell; rows ON the slice limits; rows ON the x / y limits and rows with
    NaN / infinite coordinates, which are dropped"""
    f0 = kept_rows(40, 300)
    base = kept_rows(41, 100)
    pile = np.tile(F32([33.33, 4.21, 0, 0]), (40, 1))
    pile[:, 2] = np.linspace(-1.39, -1.11, 40, dtype=F32)                           # all in slice 2 = [-1.4, -1.1)
    pile[:, 3] = np.linspace(0.1, 0.9, 40, dtype=F32)
    two = F32([[44.44, -7.77, 0.2, 0.25], [44.44, -7.77, -1.9, 0.75]])              # slice 7 first, then slice 0
    dropped = F32([[0, 1, -1, .5], [60, 1, -1, .5], [30, 30, -1, .5], [30, -30, -1, .5], [NAN, 1, -1, .5], [30, NAN, -1, .5], [30, 1, NAN, .5],
                   [INF, 1, -1, .5], [-INF, 1, -1, .5], [30, INF, -1, .5], [30, -INF, -1, .5], [30, 1, INF, .5], [30, 1, -INF, .5]])
    f1 = np.concatenate([base, pile, two, dropped])
    f2 = synth.point_cloud_ranges(5, 400, "mv3d_edges")                             # z exactly on numpy's slice limits and their f32 neighbours
    pts = np.concatenate([f0, f1, f2])
    offsets = np.cumsum([0, len(f0), len(f1), len(f2)]).astype(np.int32)
    want = expected(oracle, pts, offsets)
    r, c = cell(33.33, 4.21)
    assert want[1][r, c, 2] == pile[-1, 2] + F32(2.0) and want[1][r, c, 8] == pile[-1, 3]          # the last of the forty
    r, c = cell(44.44, -7.77)
    assert want[1][r, c, 8] == F32(0.25) and want[1][r, c, 7] == F32(0.2) + F32(2.0) and want[1][r, c, 0] == F32(-1.9) + F32(2.0)
    assert np.array_equal(bits(want[1]), bits(oracle.point_cloud_2_top(f1[:-len(dropped)])))       # the dropped rows leave no trace
    got = device_maps(gpu, pts, offsets)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.gpu
def test_odd_frame_bases_and_out(gpu, four):
    """B = 4: inside an aligned batch the frames start at 0, 4, 8 and 12 mod 16 bytes; out = buf[1:3] starts 4 mod 16"""
    torch, ops = gpu["torch"], gpu["ops"]
    pts, offsets, want = four["pts"], four["offsets"], four["want"]
    d_pts = torch.from_numpy(np.array(pts)).cuda()
    got = ops.point_cloud_2_top_batch(d_pts, offsets)
    assert got.data_ptr() % 16 == 0 and np.array_equal(bits(got.cpu().numpy()), bits(want))
    buf = torch.full((4, 601, 601, 9), -7.0, device="cuda")
    out = ops.point_cloud_2_top_batch(d_pts[5000:15000], offsets[1:4] - 5000, out=buf[1:3])
    assert out.data_ptr() == buf[1:3].data_ptr() and out.data_ptr() % 16 == 4
    host = buf.cpu().numpy()
    assert np.array_equal(bits(host[1:3]), bits(want[1:3])) and (host[0] == -7).all() and (host[3] == -7).all()
    buf = torch.full((4, 601, 601, 9), -7.0, device="cuda")
    ops.point_cloud_2_top_batch(d_pts[:0], out=buf[3])                              # no rows: the clear alone, on a frame 12 mod 16
    host = buf.cpu().numpy()
    assert not host[3].any() and (host[:3] == -7).all()
    with pytest.raises(ValueError, match="out must be"):
        ops.point_cloud_2_top_batch(d_pts, offsets, out=buf[1:3])
    with pytest.raises(ValueError, match="contiguous"):
        ops.point_cloud_2_top_batch(d_pts[:5000], out=torch.zeros((601, 9, 601), device="cuda").transpose(1, 2))


# Ranges whose corner cells a point can reach.  Under MV3D's ranges it cannot: int() truncates toward zero and the limits are open, so
# row 0 and column 0 (the head elements of a misaligned run) and column 600 (its tail) never hold a key.  Here floor(fwd_hi / res) *
# res < fwd_hi puts x in [18.0, 18.1) on row 0 and side_lo > 0 puts -y in (0.3, 0.4) on column 0; the map is (81, 39, 5), 63 180
# bytes a frame = 12 mod 16.
CORNER_CASE = (0.2, 0.5, (0.3, 8.0), (2.0, 18.1), (-1.0, 1.25))


def corner_frame(seed):
    """200 random rows inside CORNER_CASE's ranges, then rows into the first cell (slices 0, 1, 2) and the last cell (slices 2, 3)"""
    rng = np.random.RandomState(seed)
    body = np.stack([rng.uniform(2.3, 17.9, 200), rng.uniform(-7.7, -0.5, 200), rng.uniform(-1, 1.2, 200), rng.random_sample(200)], 1)
    first = [[18.05, -0.35, z, 0.3 + 0.1 * k] for k, z in enumerate((-0.9, -0.4, 0.1))]
    last = [[2.1, -7.9, z, 0.6 + 0.1 * k] for k, z in enumerate((0.1, 0.6))]
    return np.concatenate([body, first, last]).astype(F32)


@pytest.mark.gpu
def test_keys_in_the_scalar_head_and_tail(gpu, oracle):
    """runs of frames that start 12, 4 and 0 mod 16 bytes into a batch buffer: the resolve's scalar head (1, 3, 0 elements) and tail
    (1, 0, 3 elements) hold keys -- channels 0-2 of the first cell, channels 2-4 of the last -- and are resolved, not only cleared;
    the dense export writes the same bits"""
    torch, ops = gpu["torch"], gpu["ops"]
    frames = [corner_frame(90 + b) for b in range(4)]
    want = np.stack([oracle.point_cloud_2_top(f, *CORNER_CASE) for f in frames])
    assert want.shape == (4, 81, 39, 5)
    flat = want.reshape(4, -1)
    assert (flat[:, :3] != 0).all() and (flat[:, -3:] != 0).all()                   # the head and tail elements of every frame hold values
    r8 = (C.c_double * 8)(*ranges_args(CORNER_CASE))
    for lo, hi, head, tail in ((1, 3, 1, 1), (3, 4, 3, 0), (0, 1, 0, 3)):
        pts = np.concatenate(frames[lo:hi])
        offsets = np.cumsum([0] + [len(f) for f in frames[lo:hi]]).astype(np.int32)
        d_pts, d_off = torch.from_numpy(pts).cuda(), torch.from_numpy(offsets).cuda()
        buf = torch.full((4, 81, 39, 5), -7.0, device="cuda")
        ops.point_cloud_2_top_batch(d_pts, d_off, ranges=ranges_args(CORNER_CASE), out=buf[lo:hi])
        n_head = (-buf[lo:hi].data_ptr() % 16) // 4
        assert (n_head, ((hi - lo) * 81 * 39 * 5 - n_head) % 4) == (head, tail)
        host = buf.cpu().numpy()
        assert np.array_equal(bits(host[lo:hi]), bits(want[lo:hi])) and (host[:lo] == -7).all() and (host[hi:] == -7).all()
        buf.fill_(-7.0)
        status = torch.full((1,), 5, dtype=torch.int32, device="cuda")
        rc = ops.lib().mv3d_point_cloud_2_top_batch_dense(d_pts.data_ptr(), d_off.data_ptr(), hi - lo, len(pts), r8, buf[lo:hi].data_ptr(),
                                                           status.data_ptr(), torch.cuda.current_stream().cuda_stream)
        host = buf.cpu().numpy()
        assert rc == 0 and int(status.item()) == 0
        assert np.array_equal(bits(host[lo:hi]), bits(want[lo:hi])) and (host[:lo] == -7).all() and (host[hi:] == -7).all()


def outside_case(oracle):
    """(ranges, a handful of rows inside them, the same rows and one whose cell lies outside the map: numpy's IndexError)"""
    # fwd_range = (0.05, 10): y_max = int(9.95 / 0.1) = 99, but a point with 0.05 < x < 0.1 lands on row int(-x / 0.1) + 100 = 100
    case = (0.1, 0.3, (-10., 10.), (0.05, 10.), (-2., 0.4))
    inside = kept_rows(9, 400)
    inside = inside[(inside[:, 0] > 0.2) & (inside[:, 0] < 10) & (np.abs(inside[:, 1]) < 10)]
    assert len(inside) >= 8
    outside = np.concatenate([inside, F32([[0.07, 1.0, -1.0, 0.5]])])
    assert oracle.point_cloud_2_top(inside, *case).any()
    with pytest.raises(IndexError):
        oracle.point_cloud_2_top(outside, *case)
    return case, inside, outside


@pytest.mark.gpu
def test_single_ranges_entry_resolves_the_scalar_tail(gpu, oracle):
    """ops.point_cloud_2_top(ranges=...) into its own 16-byte aligned (81, 39, 5) map: 15 795 elements = no head, 3 948 vectors and a
    tail of 3, which holds keys (channels 2-4 of the last cell) that are resolved, not only cleared"""
    torch, ops = gpu["torch"], gpu["ops"]
    pts = corner_frame(90)
    want = oracle.point_cloud_2_top(pts, *CORNER_CASE)
    assert want.shape == (81, 39, 5) and want.size % 4 == 3
    assert (want.reshape(-1)[:3] != 0).all() and (want.reshape(-1)[-3:] != 0).all()
    got = ops.point_cloud_2_top(torch.from_numpy(pts).cuda(), ranges=ranges_args(CORNER_CASE))
    assert got.data_ptr() % 16 == 0 and tuple(got.shape) == (81, 39, 5)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))


@pytest.mark.gpu
def test_ranges(gpu, oracle):
    torch, ops = gpu["torch"], gpu["ops"]
    case = synth.BEV_RANGE_CASES["odd"]                                             # (h1 - h0) / zres = 11.72: twelve slices, the last one cut
    f = [synth.point_cloud_ranges(7, 3000, "odd"), synth.point_cloud_ranges(8, 2001, "odd")]
    pts, offsets = np.concatenate(f), np.array([0, 3000, 5001], np.int32)
    want = expected(oracle, pts, offsets, case)
    assert want.shape[-1] == 12
    got = device_maps(gpu, pts, offsets, ranges=ranges_args(case))
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    case, inside, outside = outside_case(oracle)
    pts, offsets = np.concatenate([inside, outside]), np.array([0, len(inside), 2 * len(inside) + 1], np.int32)
    got = device_maps(gpu, inside, ranges=ranges_args(case))                        # (the status word is cleared by every call)
    assert np.array_equal(bits(got), bits(oracle.point_cloud_2_top(inside, *case)))
    with pytest.raises(IndexError, match="point_cloud_2_top_batch"):
        device_maps(gpu, pts, offsets, ranges=ranges_args(case))
    assert np.array_equal(bits(device_maps(gpu, inside, ranges=ranges_args(case))), bits(got))


@pytest.mark.gpu
def test_single_ranges_entry_raises_index_error(gpu, oracle):
    """ops.point_cloud_2_top(ranges=...) is the batched body on one frame: the status word raises, and every call clears it"""
    torch, ops = gpu["torch"], gpu["ops"]
    case, inside, outside = outside_case(oracle)
    with pytest.raises(IndexError, match="point_cloud_2_top:"):
        ops.point_cloud_2_top(torch.from_numpy(outside).cuda(), ranges=ranges_args(case))
    got = ops.point_cloud_2_top(torch.from_numpy(inside).cuda(), ranges=ranges_args(case)).cpu().numpy()
    assert np.array_equal(bits(got), bits(oracle.point_cloud_2_top(inside, *case)))


@pytest.mark.gpu
def test_device_offsets_and_repeat(gpu, four):
    torch, ops = gpu["torch"], gpu["ops"]
    d_pts = torch.from_numpy(np.array(four["pts"])).cuda()
    d_off = torch.from_numpy(np.array(four["offsets"])).cuda()
    for _ in range(2):                                                              # scatter order must not matter
        assert np.array_equal(bits(ops.point_cloud_2_top_batch(d_pts, d_off).cpu().numpy()), bits(four["want"]))
    # device offsets are not checked: rows in front of offsets[0] and behind offsets[B] belong to no frame
    d_off = torch.tensor([5000, 10000, 15000], dtype=torch.int32, device="cuda")
    assert np.array_equal(bits(ops.point_cloud_2_top_batch(d_pts, d_off).cpu().numpy()), bits(four["want"][1:3]))


@pytest.mark.gpu
def test_capture_and_replay(gpu, oracle):
    torch, ops = gpu["torch"], gpu["ops"]
    cap = 4096
    fillings = []
    for seed, sizes in ((60, (1000, 1500)), (61, (700, 2000))):
        pts = synth.point_cloud(seed, cap)                                          # the whole buffer is refilled: the rows behind offsets[B] are stale points
        offsets = np.cumsum((0,) + sizes).astype(np.int32)
        fillings.append((pts, offsets, expected(oracle, pts, offsets)))
    buf = torch.from_numpy(fillings[0][0]).cuda()
    d_off = torch.from_numpy(fillings[0][1]).cuda()
    big = torch.zeros((4, 601, 601, 9), device="cuda")
    out = big[1:3]                                                                  # 4 mod 16 bytes
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.point_cloud_2_top_batch(buf, d_off, out=out)                            # (warm-up: the code object is loaded outside the capture)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.point_cloud_2_top_batch(buf, d_off, out=out)
    for pts, offsets, want in reversed(fillings):
        buf.copy_(torch.from_numpy(pts))
        d_off.copy_(torch.from_numpy(offsets))
        big.fill_(-1.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        host = big.cpu().numpy()
        assert np.array_equal(bits(host[1:3]), bits(want)) and (host[0] == -1).all() and (host[3] == -1).all()


@pytest.mark.gpu
def test_get_minibatch_rasterises_the_scan(gpu, oracle, tmp_path):
    torch, ops = gpu["torch"], gpu["ops"]
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    pts = synth.point_cloud(70, 6000)
    want = expected(oracle, pts, [0, len(pts)])[0]
    want_fv = R.raster(pts, oracle)[0]
    want_fv_mirror = R.raster(pts * F32([1, -1, 1, 1]), oracle)[0]
    path = str(tmp_path / "000000.bin")
    pts.tofile(path)
    own = np.random.RandomState(2).random_sample((16, 601, 9)).astype(F32)
    cfg.LIDAR_BV_FROM_SCAN = True
    try:
        for fv_on in (False, True):
            cfg.FRONT_VIEW_INPUT = fv_on
            for entry in (_entry(velodyne_path=path), _entry(velodyne=pts), _entry(velodyne_path=path, lidar_bv_path=str(tmp_path / "no_such_map.npy"))):
                blobs = get_minibatch([entry], 2)
                bev = blobs["lidar_bv_data"]
                assert isinstance(bev, torch.Tensor) and bev.is_cuda and tuple(bev.shape) == (1, 601, 601, 9) and bev.dtype == torch.float32
                assert np.array_equal(bits(bev.cpu().numpy()[0]), bits(want))
                assert blobs["im_info"].dtype == F32 and np.array_equal(blobs["im_info"], [[601, 601, 1]])
                assert isinstance(blobs["image_data"], np.ndarray) and ("lidar_fv_data" in blobs) == fv_on
                if fv_on:
                    assert np.array_equal(bits(blobs["lidar_fv_data"].cpu().numpy()[0]), bits(want_fv))
                flipped = get_minibatch([dict(entry, flipped=True)], 2)
                assert torch.equal(flipped["lidar_bv_data"].view(torch.int32), ops.mirror_columns(bev.clone()).view(torch.int32))
                assert torch.equal(flipped["image_data"], ops.mirror_columns(ops._dev(blobs["image_data"])))
                if fv_on:
                    assert np.array_equal(bits(flipped["lidar_fv_data"].cpu().numpy()[0]), bits(want_fv_mirror))
            # an in-memory map is the caller's, used as is, as with the key off
            blobs = get_minibatch([_entry(lidar_bv=own, velodyne=pts)], 2)
            assert isinstance(blobs["lidar_bv_data"], np.ndarray) and np.array_equal(blobs["lidar_bv_data"], own[None])
            assert np.array_equal(blobs["im_info"], [[16, 601, 1]])
        assert pts[0, 1] == synth.point_cloud(70, 6000)[0, 1]                       # (the entry's own array is not mirrored in place)
        cfg.FRONT_VIEW_INPUT = False
        with pytest.raises(ValueError, match="velodyne"):
            get_minibatch([_entry()], 2)
    finally:
        cfg.LIDAR_BV_FROM_SCAN = False
        cfg.FRONT_VIEW_INPUT = False


@pytest.mark.gpu
def test_detection_loops_rasterise_the_scans(gpu, oracle, tmp_path):
    torch, ops = gpu["torch"], gpu["ops"]
    from mv3d_tf_amd.fast_rcnn import detect_batch
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.rpn_msr.generate import imdb_proposals
    clouds = [synth.point_cloud(80, 3000), synth.point_cloud(81, 2000), synth.point_cloud(82, 2500)]
    want = [oracle.point_cloud_2_top(c) for c in clouds]
    want_fv = [R.raster(c, oracle)[0] for c in clouds]
    assert all(w.any() for w in want)
    rois = np.array([[0, 20, 1, -1, 4, 1.6, 1.5], [0, 30, -3, -1, 4, 1.6, 1.5]], F32)
    image = np.zeros((8, 12, 3), np.uint8)

    def host(t):
        return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    class Net:
        """a stub that records what it is fed and answers with two fixed ROIs per frame whose scores depend on the frame's BEV map"""

        def __init__(self, views):
            self.views, self.fed, self.fed_fv = views, [], []

        def forward(self, feed):
            bev = host(feed["lidar_bv_data"])
            self.fed.append(bev)
            if self.views == 3:
                self.fed_fv.append(host(feed["lidar_fv_data"]))
            B = bev.shape[0]
            assert np.array_equal(feed["im_info"], [[601, 601, 1]] * B)
            p = np.array([0.3 + 0.4 * ((float(bev[b].sum(dtype=np.float64)) * 0.37) % 1.0) for b in range(B)], F32)
            scores = np.stack([np.stack([1 - p, p], 1), np.stack([p, 1 - p], 1)], 1).reshape(2 * B, 2)
            r3, r4 = np.tile(rois, (B, 1)), np.tile(rois[:, :5], (B, 1))
            r3[:, 0] = r4[:, 0] = np.repeat(np.arange(B), 2)
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            return {"rois": (dev(r4), dev(r4 + 1), dev(r3)), "cls_prob": dev(scores), "bbox_pred": dev(np.zeros((2 * B, 48), F32)),
                    "num_rois": dev(np.full((B,), 2, np.int32)), "rois_per_frame": 2, "rois_status": dev(np.zeros((B,), np.int32))}

    class Imdb:
        name, num_classes, image_index = "three_scans", 2, ["000000", "000001", "000002"]

        def image_at(self, i): return image
        def calib_at(self, i): return np.zeros((4, 12))
        def evaluate_detections(self, *a): self.evaluated = True

    class ScanImdb(Imdb):
        def points_at(self, i): return clouds[i]
        def bv_at(self, i): raise AssertionError("no stored map may be asked for")
        def lidar_path_at(self, i): raise AssertionError("no stored map may be asked for")

    class MapImdb(Imdb):
        def points_at(self, i): return clouds[i]
        def bv_at(self, i): return want[i]

    saved, root = dict(cfg.TEST), cfg.ROOT_DIR
    cfg.ROOT_DIR = str(tmp_path)
    try:
        for batch, groups in ((1, ([0], [1], [2])), (2, ([0, 1], [2]))):
            cfg.TEST.BATCH_SIZE = batch
            cfg.LIDAR_BV_FROM_SCAN = False
            stored = detect_batch.test_net(None, Net(2), MapImdb(), "w")
            stored_props = imdb_proposals(None, Net(2), MapImdb())
            cfg.LIDAR_BV_FROM_SCAN = True
            for views in (2, 3):
                for loop in ("test_net", "imdb_proposals"):
                    net, imdb = Net(views), ScanImdb()
                    if loop == "test_net":
                        got = detect_batch.test_net(None, net, imdb, "w")
                        assert imdb.evaluated
                        for a, b in zip(got, stored):                               # (all_boxes, all_boxes_cnr)[class][frame]
                            assert all(len(a[1][i]) >= 1 and np.array_equal(a[1][i], b[1][i]) for i in range(3))
                    else:
                        got = imdb_proposals(None, net, imdb)
                        assert all(np.array_equal(got[k][i], stored_props[k][i]) and len(got[k][i]) == 2 for k in ("bv", "image") for i in range(3))
                    assert [fed.shape[0] for fed in net.fed] == [len(g) for g in groups]          # a group's frames from ONE batched call
                    for fed, g in zip(net.fed, groups):
                        assert np.array_equal(bits(fed), bits(np.stack([want[i] for i in g])))
                    for fed, g in zip(net.fed_fv, groups):
                        assert np.array_equal(bits(fed), bits(np.stack([want_fv[i] for i in g])))
                    assert len(net.fed_fv) == (len(groups) if views == 3 else 0)
        # the scores do depend on the map: the frames' detections differ
        assert not np.array_equal(stored[0][1][0][:, -1], stored[0][1][1][:, -1])
    finally:
        cfg.LIDAR_BV_FROM_SCAN = False
        cfg.TEST.clear()
        cfg.TEST.update(saved)
        cfg.ROOT_DIR = root
