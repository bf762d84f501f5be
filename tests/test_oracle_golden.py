"""CPU oracle (oracle/mv3d_oracle.c) pinned against golden vectors captured from the
reference itself (tests/golden/make_golden.py).  Runs without a GPU."""
import numpy as np
import pytest

from conftest import golden
from mv3d_tf_amd import synth

# Tolerance for float regressions stated by BASELINE.json north_star: 1e-4 (fp32).
TOL = 1e-4


def test_anchors_bv(oracle):
    g = golden("anchors_bv")
    assert np.array_equal(oracle.generate_anchors_bv(), g["base"])
    assert int(g["Xn"]) == 600 and int(g["Yn"]) == 600
    # known answer
    assert oracle.generate_anchors_bv().tolist() == [[-19, -8, 20, 8], [-5, -2, 5, 3], [-8, -19, 8, 20], [-2, -5, 3, 5]]


def test_floor_divide_matches_numpy(oracle):
    g = golden("floor_divide")
    assert np.array_equal(oracle.floor_divide(g["a"], 0.1), g["q"])


def test_defined_exp_log(oracle):
    g = golden("exp_log")
    e = oracle.expf(g["x32"])
    assert np.array_equal(e, g["exp32"])          # numpy's f32 exp restated bit-for-bit
    lg = oracle.log(g["x64"])
    assert np.all(np.abs(lg - g["log64"]) <= 4e-16 * np.maximum(1.0, np.abs(g["log64"])))


def exp_edge_arguments():
    """22 015 f32 arguments around the two cut-offs of numpy's f32 exp and through the zone where its result is subnormal"""
    hi, lo = np.float32(88.72283935546875), np.float32(-103.97208404541015625)
    up, down = np.float32(np.inf), np.float32(-np.inf)
    hand = [hi, np.nextafter(hi, up), np.nextafter(hi, down), lo, np.nextafter(lo, up), np.nextafter(lo, down),
            0.0, -0.0, np.inf, -np.inf, np.nan, 88.5, 89.0, -100.0, 88.0]
    return np.concatenate([np.linspace(-104.5, -87, 20000), np.linspace(88, 89, 2000), hand]).astype(np.float32)


def test_defined_exp_edges_against_numpy(oracle):
    """the restated exp against numpy ITSELF where exp_log.npz (arguments in [-80, 80], 88 and -100) does not reach: overflow,
    underflow and subnormal results.  numpy's f32 exp is one SIMD kernel on AVX512F and on AVX2 + FMA3 hosts (the same bits on
    both, the oracle's) and the C library's expf elsewhere, whose subnormal results differ in the last bits: the comparison is
    made for the numpy version of the fixtures on a host that dispatches to the SIMD kernel."""
    recorded = str(golden("exp_log")["numpy_version"])
    if np.__version__ != recorded:
        pytest.skip("numpy %s here; the f32 exp is pinned for numpy %s, the fixtures' version" % (np.__version__, recorded))
    # (a private name of numpy: safe to import only because the version check above has let nothing but numpy 2.2.x through)
    from numpy._core._multiarray_umath import __cpu_features__ as have
    if not (have.get("AVX512F") or (have.get("AVX2") and have.get("FMA3"))):
        pytest.skip("numpy's f32 exp falls back to the C library on this host (no AVX512F, no AVX2 + FMA3)")
    x = exp_edge_arguments()
    assert x.size == 22015
    with np.errstate(all="ignore"):
        want = np.exp(x)
    got = oracle.expf(x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    tiny = (want > 0) & (want < np.float32(2.0 ** -126))
    assert tiny.sum() > 5000 and np.isposinf(want).sum() > 500 and (want == 0).sum() > 100


@pytest.mark.parametrize("name", ["bbox_overlaps_int", "bbox_overlaps_frac"])
def test_bbox_overlaps(oracle, name):
    g = golden(name)
    assert np.array_equal(oracle.bbox_overlaps(g["boxes"], g["query"]), g["overlaps"])


NMS_CASES = ["nms_6000_rand", "nms_6000_clustered", "nms_12000_rand", "nms_12000_clustered", "nms_300_clustered",
             "nms_300_rand", "nms_1000_clustered", "nms_65_clustered", "nms_1_rand"]


def nms_case(name):
    g = golden(name)
    n = int(name.split("_")[1])
    dets = synth.nms_dets(int(g["seed"]), n, str(g["variant"]), integer=bool(g["integer"]))
    assert synth.sha256(dets) == str(g["sha"])
    return g, dets


@pytest.mark.parametrize("name", NMS_CASES)
def test_cpu_nms(oracle, name):
    g, dets = nms_case(name)
    assert oracle.cpu_nms(dets, float(g["thresh"])) == g["keep"].tolist()
    order = np.argsort(-dets[:, 4], kind="stable")
    assert oracle.cpu_nms(dets[order], float(g["thresh"]), presorted=True) == g["keep_presorted"].tolist()


def test_cpu_nms_exact_iou_and_degenerate(oracle):
    g = golden("nms_exact_iou")
    for i in range(4):
        assert oracle.cpu_nms(g[f"dets{i}"], float(g[f"thresh{i}"])) == g[f"keep{i}"].tolist()
    # the pair that separates a double compare from a float compare: IoU = 0.7f < 0.7
    assert g["keep0"].tolist() == [0, 1]
    d = golden("nms_degenerate")
    assert int(d["raises_zero_division"]) == 1
    with pytest.raises(ZeroDivisionError):
        oracle.cpu_nms(d["dets"], float(d["thresh"]))
    assert oracle.cpu_nms(np.zeros((0, 5), np.float32), 0.7) == []


def test_projection_matrix_and_edges(oracle):
    g = golden("project_edge")
    cn = oracle.lidar_3d_to_corners(g["boxes3d"])
    assert np.array_equal(cn, g["corners"], equal_nan=True)
    assert np.array_equal(oracle.lidar_cnr_to_img(cn, g["calib"]), g["img"])


PROPOSAL_CASES = ["proposal3d_76_TRAIN_rand", "proposal3d_76_TEST_peaky", "proposal3d_76_TRAIN_peaky",
                  "proposal3d_75_TEST_peaky", "proposal3d_75_TRAIN_rand", "proposal3d_76_TEST_rand",
                  "proposal3d_20_TRAIN_peaky", "proposal3d_75_TRAIN_peaky", "proposal3d_75_TEST_rand"]


def proposal_case(name):
    g = golden(name)
    H = int(g["H"])
    prob, pred, im_info, calib = synth.rpn_head(int(g["seed"]), H, H, str(g["variant"]))
    assert synth.sha256(prob, pred, im_info, calib) == str(g["sha"])
    cfg = {str(g["cfg_key"]): dict(RPN_PRE_NMS_TOP_N=int(g["pre"]), RPN_POST_NMS_TOP_N=int(g["post"]),
                                   RPN_NMS_THRESH=float(g["thresh"]), RPN_MIN_SIZE=int(g["min_size"]))}
    return g, (prob, pred, im_info, calib), cfg


def check_proposal_blobs(got, g):
    """All three blobs bit-exact (north_star asks 1e-4 on the regressions; we get equality)."""
    bv, img, b3 = got
    assert bv.shape == g["blob_bv"].shape and img.shape == g["blob_img"].shape and b3.shape == g["blob_3d"].shape
    assert np.array_equal(bv, g["blob_bv"])
    assert np.array_equal(img, g["blob_img"])
    assert np.array_equal(b3, g["blob_3d"])


@pytest.mark.parametrize("name", PROPOSAL_CASES)
def test_proposal_layer_3d(oracle, name):
    g, inp, cfg = proposal_case(name)
    out = oracle.proposal_layer_3d(*inp, str(g["cfg_key"]), [8, ], [1.0, 1.0], cfg=cfg, debug=True)
    check_proposal_blobs(out[:3], g)
    if "props3d" in g.files:
        d = out[3]
        assert np.array_equal(d["anchors3d"], g["anchors3d"])
        assert np.array_equal(d["props3d"], g["props3d"])
        assert bool(g["bv_raw_is_integral"])
        # integer BEV coordinates: equal everywhere (exp ulp differences would show as +-1 flips)
        assert np.array_equal(d["bv_raw"].astype(np.int64), g["bv_raw"].astype(np.int64))
        assert np.array_equal(d["img"], g["img"])


AT_CASES = ["anchor_target_76_normal", "anchor_target_76_gt_outside", "anchor_target_76_many_gt",
            "anchor_target_75_normal", "anchor_target_75_gt_outside", "anchor_target_75_many_gt",
            "anchor_target_76_tiny_gt", "anchor_target_76_no_gt_overlap"]


@pytest.mark.parametrize("name", AT_CASES)
def test_anchor_target_layer(oracle, name):
    g = golden(name)
    H = int(g["H"])
    np.random.seed(int(g["np_seed"]))
    lab, tg, anc, anc3 = oracle.anchor_target_layer(np.zeros((1, H, H, 8), np.float32), g["gt_bv"], g["gt_3d"],
                                                    g["im_info"], [8, ], [1.0, 1.0])
    assert np.array_equal(lab.astype(np.int8), g["labels"])            # bit-exact anchor indices
    rows = g["target_rows"]
    assert np.array_equal(tg[rows], g["targets"])       # north_star asks 1e-4; equal on these vectors
    assert np.array_equal(np.where(np.any(tg != 0, 1))[0], g["targets_nonzero_rows"])
    assert np.array_equal(anc, g["anchors"])
    assert np.array_equal(anc3, g["anchors_3d"])
    if "gt_outside" in name:   # the flood ends with 0 positives
        assert (lab == 1).sum() == 0 and (lab == 0).sum() == 128


@pytest.mark.parametrize("name", ["proposal_target_few", "proposal_target_many"])
def test_proposal_target_layer_3d(oracle, name):
    g = golden(name)
    np.random.seed(int(g["np_seed"]))
    out = oracle.proposal_target_layer_3d(g["rois_bv_in"], g["rois_3d_in"], g["gt_bv"], g["gt_3d"], g["gt_cnr"],
                                          g["calib"], 2)
    assert np.array_equal(out[0], g["rois_bv"])
    assert np.array_equal(out[1], g["rois_img"])
    assert np.array_equal(out[2], g["labels"])
    assert np.array_equal(out[3], g["bbox_targets"])
    assert np.array_equal(out[4], g["rois_3d"])


def test_box_tail(oracle):
    g = golden("box_tail")
    r3 = np.hstack([np.zeros((len(g["boxes_3d"]), 1), np.float32), g["boxes_3d"]])
    cnr, pred, pred_r, bv, bv_r = oracle.box_tail(r3, g["deltas"], 2)
    assert np.array_equal(cnr, g["corners"])
    assert np.array_equal(pred_r, g["pred_cnr_r"])
    assert np.array_equal(bv, g["pred_bv"]) and bv.dtype == g["pred_bv"].dtype
    assert np.array_equal(bv_r, g["pred_bv_r"])


@pytest.mark.parametrize("case", sorted(synth.BEV_RANGE_CASES))
def test_point_cloud_2_top_with_its_own_parameters(oracle, case):
    """lib/utils/read_lidar.py:10-16's parameters (reference-generated): the function's defaults, unrepresentable limits, a slice
    count that is not an integer, and points exactly ON numpy's slice limits for the MV3D ranges (np.arange's values are
    h0 + i * ((h0 + zres) - h0), not h0 + i * zres: z = -0.5 lands one slice lower than the naive restatement puts it)"""
    g = golden("point_cloud_top_ranges_" + case)
    res, zres, side, fwd, hr = synth.BEV_RANGE_CASES[case]
    pts = synth.point_cloud_ranges(int(g["seed"]), int(g["P"]), case)
    assert synth.sha256(pts) == str(g["sha_points"])
    top = oracle.point_cloud_2_top(pts, res, zres, side, fwd, hr)
    assert tuple(g["shape"]) == top.shape
    nz = np.flatnonzero(top)
    assert np.array_equal(nz, g["nz_index"]) and np.array_equal(top.ravel()[nz], g["nz_value"])
    assert synth.sha256(top) == str(g["sha_top"])


@pytest.mark.parametrize("name", ["point_cloud_top_small", "point_cloud_top_kitti"])
def test_point_cloud_2_top(oracle, name):
    g = golden(name)
    pts = synth.point_cloud(int(g["seed"]), int(g["P"]))
    assert synth.sha256(pts) == str(g["sha_points"])
    top = oracle.point_cloud_2_top(pts)
    assert tuple(g["shape"]) == top.shape == (601, 601, 9)
    nz = np.flatnonzero(top)
    assert np.array_equal(nz, g["nz_index"]) and np.array_equal(top.ravel()[nz], g["nz_value"])
    assert synth.sha256(top) == str(g["sha_top"])
