"""Scan augmentation in training (cfg.TRAIN.SCAN_AUGMENT): ops.scan_transform / mv3d_scan_transform and
mv3d_tf_amd/datasets/augment.py against tests/scan_augment_restatement.py, the checked key, the draw stream and the data layer under
the key.  PARITY UNPINNED: the reference trains from stored maps and has no such code; the restatement is the definition.  Every
comparison of device results and of annotations is equality of bits (uint32 views: a NaN reflectance keeps its payload); the one
tolerance, of the projection's consistency, is derived where it is used."""
import numpy as np
import pytest

import scan_augment_restatement as R
import scan_crop_restatement as C
from conftest import golden
from mv3d_tf_amd import synth
from mv3d_tf_amd.datasets import augment
from mv3d_tf_amd.datasets.mirror import lidar_box_to_bv, mirror_annotation, mirror_calib

F32 = np.float32
NAN, INF = float("nan"), float("inf")
FILL = 0xA5C3F00F                                   # the pattern every guard row holds before a call
EPS = 2.0 ** -24                                    # half an ulp of f32, relative: one rounding to nearest
DRAWS = ((0.15, 1.04, (1.5, -2.0, 0.25)), (-0.17453292519943295, 0.95, (0.0, 0.0, 0.0)), (3.0, 2.5, (-40.0, 7.0, 1.0)))
HW = (375, 1242)


def u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def annotation(G, ignore=False):
    """a roidb entry as parse_kitti_labels + prepare_roidb leave it: the first G of the 7 objects of tests/golden/kitti_label.npz's
    frame 0 under that frame's table, with two ignore regions where asked"""
    lab = golden("kitti_label")
    keys = ("ry", "boxes", "boxes_bv", "boxes_3D_cam", "boxes_3D", "boxes3D_cam_corners", "boxes_corners", "gt_classes", "gt_overlaps",
            "xyz", "alphas")
    e = {k: np.array(lab["ann0_" + k][:G]) for k in keys}
    e["flipped"] = False
    e["calib"] = np.array(lab["calib_0"])
    e["max_overlaps"] = e["gt_overlaps"].max(axis=1) if G else np.zeros((0,), F32)
    e["max_classes"] = e["gt_overlaps"].argmax(axis=1) if G else np.zeros((0,), np.int64)
    e["image_path"] = "000000.png"
    if ignore:
        e["ignore_boxes_3D"] = F32([[31.25, -7.5, -0.9, 5.1, 1.9, 2.2], [12.0, 9.75, -1.1, 4.4, 1.8, 1.9]])
        e["ignore_boxes_bv"] = lidar_box_to_bv(e["ignore_boxes_3D"])
        e["ignore_boxes_img"] = F32([[100.5, 150.25, 180.0, 190.75]])
    return e


def frozen(entry):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in entry.items()}


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


@pytest.fixture
def key():
    """cfg with the augmentation's keys as they are, restored afterwards"""
    from mv3d_tf_amd.fast_rcnn.config import cfg
    top = {k: cfg[k] for k in ("LIDAR_BV_FROM_SCAN", "FRONT_VIEW_INPUT", "LIDAR_CROP_TO_IMAGE", "LIDAR_BV_ENCODING")}
    train = {k: cfg.TRAIN[k] for k in ("SCAN_AUGMENT", "SCAN_AUGMENT_ROTATION", "SCAN_AUGMENT_SCALE", "SCAN_AUGMENT_SHIFT", "IGNORE_TYPES")}
    try:
        yield cfg
    finally:
        for k, v in top.items():
            cfg[k] = v
        for k, v in train.items():
            cfg.TRAIN[k] = v


# ---------------------------------------------------------------------------------------------------- CPU
def test_config_defaults():
    from mv3d_tf_amd.fast_rcnn.config import cfg
    T = cfg.TRAIN
    assert T.SCAN_AUGMENT is False and T.SCAN_AUGMENT_ROTATION == 0.17453292519943295 == np.deg2rad(10.0)
    assert T.SCAN_AUGMENT_SCALE == (0.95, 1.05) and T.SCAN_AUGMENT_SHIFT == (0.0, 0.0, 0.0)


def test_matrix_and_its_inverse():
    for theta, s, t in DRAWS:
        A, Ai = augment.transform_matrix(theta, s, t)
        RA, RAi = R.transform_matrix(theta, s, t)
        assert same_bits(A, RA) and same_bits(Ai, RAi) and A.shape == (3, 4) and A.dtype == np.float64
        assert A[0, 0] == s * np.cos(theta) and A[0, 1] == -(s * np.sin(theta)) and A[1, 0] == s * np.sin(theta) and A[2, 2] == s
        assert A[:, 3].tolist() == list(t) and A[2, :2].tolist() == [0, 0] and A[:2, 2].tolist() == [0, 0]
        full = lambda M: np.vstack([M, [0, 0, 0, 1.0]])
        for prod in (full(A) @ full(Ai), full(Ai) @ full(A)):
            # entries are sums of <= 3 products of magnitude <= max|A| max|Ai| (1 + |t|): a few f64 roundings of that
            scale = np.abs(full(A)).max() * np.abs(full(Ai)).max() * (1.0 + np.abs(t).max())
            assert np.abs(prod - np.eye(4)).max() <= 8 * 2.0 ** -53 * scale
    for bad in ((NAN, 1.0, (0, 0, 0)), (0.1, 0.0, (0, 0, 0)), (0.1, -1.0, (0, 0, 0)), (0.1, 1.0, (0, INF, 0)), (0.1, 1.0, (0, 0))):
        with pytest.raises(ValueError, match="transform_matrix"):
            augment.transform_matrix(*bad)


def test_identity_changes_no_value():
    A, Ai = augment.transform_matrix(0.0, 1.0, (0.0, 0.0, 0.0))
    assert np.array_equal(A, np.eye(3, 4)) and np.array_equal(Ai, np.eye(3, 4))
    for G, ign in ((0, False), (3, True), (7, False)):
        e = annotation(G, ign)
        out = augment.augment_annotation(e, A, 1.0)
        assert set(out) == set(e)
        for k, v in e.items():                                # values: a -0.0 may come back as +0.0
            assert np.array_equal(out[k], v) and np.asarray(out[k]).dtype == np.asarray(v).dtype, k
        assert np.array_equal(augment.augment_calib(e["calib"], Ai), e["calib"])


@pytest.mark.parametrize("G,ign", [(0, False), (0, True), (1, False), (1, True), (3, False), (3, True)])
def test_annotation_and_table_equal_the_restatement(G, ign):
    e = annotation(G, ign)
    if G == 3:
        e["boxes_corners"][1, 5] = NAN                      # a corner that is no point: copied, and the centre's mean follows numpy
    before = frozen(e)
    lidar = {"boxes_corners", "boxes_3D", "boxes_bv", "ignore_boxes_3D", "ignore_boxes_bv"}
    for theta, s, t in DRAWS:
        A, Ai = augment.transform_matrix(theta, s, t)
        out, want = augment.augment_annotation(e, A, s), R.augment_annotation(e, A, s)
        assert frozen(e) == before, "the input entry was modified"
        assert set(out) == set(want) == set(e)
        for k in e:
            if isinstance(e[k], np.ndarray):
                assert same_bits(out[k], want[k]), k
                assert out[k] is not e[k] and not np.shares_memory(out[k], e[k]), k
                if k not in lidar:
                    assert same_bits(out[k], e[k]), k       # the camera-frame fields, `boxes`, the classes: the same bits
                elif out[k].size and k != "boxes_bv":
                    assert not same_bits(out[k], e[k]), k
            else:
                assert out[k] == e[k], k
        if G:
            assert same_bits(out["boxes_bv"], lidar_box_to_bv(out["boxes_3D"]))
            assert same_bits(out["boxes_3D"][:, 3:], (e["boxes_3D"][:, 3:].astype(np.float64) * s).astype(F32))
        table, want_table = augment.augment_calib(e["calib"], Ai), R.augment_calib(e["calib"], Ai)
        assert same_bits(table, want_table) and table.dtype == np.float64 and table.shape == (4, 12)
        assert same_bits(table[:3], e["calib"][:3]) and same_bits(table[3].astype(F32).astype(np.float64), table[3])
        assert not same_bits(table[3], e["calib"][3])
    with pytest.raises(ValueError, match="augment_calib"):
        augment.augment_calib(np.zeros((3, 12)), Ai)


def test_a_mirrored_entry_is_augmented_like_any_other():
    e = mirror_annotation(annotation(3, True), 1242)
    A, _ = augment.transform_matrix(*DRAWS[0])
    out, want = augment.augment_annotation(e, A, DRAWS[0][1]), R.augment_annotation(e, A, DRAWS[0][1])
    assert out["flipped"] is True and set(out) == set(e)
    for k in e:
        if isinstance(e[k], np.ndarray):
            assert same_bits(out[k], want[k]), k


def _fixture_points():
    """LIDAR points whose camera depth under kitti_label's frame-0 table lies in [2, 70] m and whose pixel lies inside the image"""
    rng = np.random.RandomState(11)
    x = np.concatenate([np.linspace(2.3, 70.0, 200), rng.uniform(2.3, 70.0, 800)])
    y = x * rng.uniform(-0.6, 0.6, x.size)
    z = x * rng.uniform(-0.15, 0.2, x.size)
    return np.stack([x, y, z], 1).astype(F32)


def test_projection_consistency():
    """The pixel of A . X under proj_matrix(calib') against the pixel of X under proj_matrix(calib).  Both are held to ONE f64
    evaluation, u_ref = pixel of (P2 . R0 . (Tr . A^-1), all f64 and unrounded) . (A . X in f64).

    The bound, from f32's eps = 2^-24 (one rounding to nearest) and the fixture's magnitudes.  With v = M . [X; 1] and u = v_0 / v_2
    (the column; v_1 / v_2 the row), a perturbation of M and X moves v_i by at most
        d_i <= sum_j |dM_ij| |X_j| + sum_{j<3} |M_ij| |dX_j|.
    dX_j <= eps |X_j|: the transformed coordinates are rounded to f32 once.  dM: the twelve entries of Tr' are rounded to f32
    (eps each), proj_matrix's f32 chain m1 = P2 . R0 rounds four partial sums (<= 4 eps of sum |P2||R0|) and M = m1 . Tr' three
    (<= 3 eps): |dM_ij| <= 8 eps S_ij with S = |P2| |R0| |Tr'| (products of the absolute values), and |M_ij| <= S_ij.  So
        d_i <= 9 eps T_i,   T_i = (S . |[X; 1]|)_i,
    and the pixel moves by at most (d_0 + |u| d_2) / (v_2 - d_2) <= 9 eps (max T_0 + max|u| max T_2) / (min depth), the maxima over
    the fixture and max(T_0) read as max(T_0, T_1), max|u| over columns and rows.  The f64 evaluation's own roundings (2^-53) and the
    second-order terms are covered by a factor 1.01.  The untransformed side has no rounded table and no rounded coordinates; the same
    expression on its own magnitudes bounds it a fortiori.  Nothing here was tuned to the observed value, which is printed."""
    X = _fixture_points()
    calib = np.array(golden("kitti_label")["calib_0"])
    P2, R0, Tr = calib[0].reshape(3, 4), calib[2, :9].reshape(3, 3), calib[3].reshape(3, 4)
    hom = lambda M34: np.vstack([M34, [0, 0, 0, 1.0]])
    worst = 0.0
    for theta, s, t in DRAWS[:2]:
        A, Ai = augment.transform_matrix(theta, s, t)
        calib2 = augment.augment_calib(calib, Ai)
        Tr2 = Tr @ hom(Ai)                                                           # f64, unrounded
        M_ref = (P2[:, :3] @ R0) @ Tr2
        AX = X.astype(np.float64) @ A[:, :3].T + A[:, 3]
        v_ref = AX @ M_ref[:, :3].T + M_ref[:, 3]
        assert v_ref[:, 2].min() >= 2.0 and v_ref[:, 2].max() <= 70.0
        pix_ref = v_ref[:, :2] / v_ref[:, 2:]
        assert (pix_ref >= 0).all() and (pix_ref[:, 0] < HW[1]).all() and (pix_ref[:, 1] < HW[0]).all()
        X2 = R.transform_rows(np.hstack([X, np.zeros((len(X), 1), F32)]), None, [A])[:, :3]
        for pts, table, Tr_abs in ((X2, calib2, np.abs(Tr2)), (X, calib, np.abs(Tr))):
            M = C.proj_matrix(table)
            v = np.array([C.image_vector(M, *row) for row in pts])
            pix = v[:, :2] / v[:, 2:]
            S = (np.abs(P2[:, :3]) @ np.abs(R0)) @ Tr_abs
            T = np.hstack([np.abs(pts.astype(np.float64)), np.ones((len(pts), 1))]) @ S.T
            bound = 1.01 * 9 * EPS * (T[:, :2].max() + np.abs(pix_ref).max() * T[:, 2].max()) / v_ref[:, 2].min()
            err = np.abs(pix - pix_ref).max()
            worst = max(worst, err)
            print("projection consistency: max |pixel - f64 pixel| = %.3e px, bound %.3e px" % (err, bound))
            assert bound < 0.25, "the bound says nothing"
            assert err <= bound
    print("projection consistency: observed maximum %.3e px" % worst)


def test_draws(key):
    cfg = key
    rot, (lo, hi) = cfg.TRAIN.SCAN_AUGMENT_ROTATION, cfg.TRAIN.SCAN_AUGMENT_SCALE
    cfg.TRAIN.SCAN_AUGMENT_SHIFT = (1.0, 2.0, 0.25)
    runs = []
    for _ in range(2):
        augment.seed(cfg.RNG_SEED + 1)
        runs.append([augment.draw_scan_transform() for _ in range(4)])
    assert runs[0] == runs[1] and len({d[0] for d in runs[0]}) == 4
    ref = np.random.RandomState(cfg.RNG_SEED + 1)
    for theta, s, shift in runs[0]:
        want = [ref.uniform(-rot, rot), ref.uniform(lo, hi), ref.uniform(-1.0, 1.0), ref.uniform(-2.0, 2.0), ref.uniform(-0.25, 0.25)]
        assert [theta, s] + list(shift) == want                 # five uniforms, in this order
        assert -rot <= theta < rot and lo <= s < hi and all(abs(d) <= b for d, b in zip(shift, (1.0, 2.0, 0.25)))
    # degenerate ranges still consume five draws
    cfg.TRAIN.SCAN_AUGMENT_ROTATION, cfg.TRAIN.SCAN_AUGMENT_SCALE, cfg.TRAIN.SCAN_AUGMENT_SHIFT = 0.0, (1.0, 1.0), (0.0, 0.0, 0.0)
    rng, ref = np.random.RandomState(9), np.random.RandomState(9)
    assert augment.draw_scan_transform(rng) == (0.0, 1.0, (0.0, 0.0, 0.0))
    ref.uniform(size=5)
    assert rng.uniform() == ref.uniform()
    # an explicit generator leaves the module's own alone, and neither touches numpy's global stream
    augment.seed(5)
    np.random.seed(123)
    state = np.random.get_state()
    augment.draw_scan_transform(np.random.RandomState(1))
    first = augment.draw_scan_transform()
    augment.seed(5)
    assert augment.draw_scan_transform() == first
    now = np.random.get_state()
    assert now[0] == state[0] and np.array_equal(now[1], state[1]) and now[2:] == state[2:]


def test_the_checked_key(lib_ops, key):
    ops, cfg = lib_ops, key
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    from mv3d_tf_amd.roi_data_layer.roidb import prepare_roidb
    assert ops.scan_augment() is False

    class NothingLoaded:
        name, num_classes, image_index = "none", 2, ["000000"]

        def __getattr__(self, name):
            raise AssertionError("the imdb was asked for %s" % name)

    cfg.TRAIN.SCAN_AUGMENT = True
    entry = dict(annotation(1), image=np.zeros((8, 12, 3), np.uint8), velodyne=np.zeros((3, 4), F32))
    for call in (ops.scan_augment, lambda: prepare_roidb(NothingLoaded()), lambda: get_minibatch([entry], 2)):
        with pytest.raises(ValueError, match="SCAN_AUGMENT needs cfg.LIDAR_BV_FROM_SCAN"):
            call()
    cfg.LIDAR_BV_FROM_SCAN = True
    assert ops.scan_augment() is True
    for scale in ((0.0, 1.05), (-0.5, 1.0), (0.95, 0.0), (1.05, 0.95), (0.95, INF)):
        cfg.TRAIN.SCAN_AUGMENT_SCALE = scale
        for call in (ops.scan_augment, lambda: prepare_roidb(NothingLoaded())):
            with pytest.raises(ValueError, match="SCAN_AUGMENT_SCALE"):
                call()
    cfg.TRAIN.SCAN_AUGMENT_SCALE = (0.95, 1.05)
    for k, bad in (("SCAN_AUGMENT_ROTATION", -0.1), ("SCAN_AUGMENT_ROTATION", NAN), ("SCAN_AUGMENT_SHIFT", (0.0, 0.0)), ("SCAN_AUGMENT_SHIFT", (0.0, -1.0, 0.0))):
        good = cfg.TRAIN[k]
        cfg.TRAIN[k] = bad
        with pytest.raises(ValueError, match=k):
            ops.scan_augment()
        cfg.TRAIN[k] = good
    # an in-memory map is the caller's and cannot be transformed: refused before anything is drawn, uploaded or launched
    augment.seed(2)
    first = augment.draw_scan_transform()
    augment.seed(2)
    for k, shape in (("lidar_bv", (601, 601, 9)), ("lidar_fv", (64, 512, 3))):
        with pytest.raises(ValueError, match="in-memory '%s'" % k):
            get_minibatch([dict(entry, **{k: np.zeros(shape, F32)})], 2)
    assert augment.draw_scan_transform() == first


def _mock_device(monkeypatch, ops, calls):
    """the data layer's device calls replaced by host stand-ins that record them"""
    monkeypatch.setattr(ops, "_dev", lambda t, *a, **kw: np.array(t, copy=True))
    monkeypatch.setattr(ops, "scan_transform", lambda pts, off, A, out=None: calls.append(("scan_transform", np.array(A))) or out)
    monkeypatch.setattr(ops, "scan_bev", lambda pts, off=None: calls.append(("scan_bev",)) or np.zeros(ops.BEV_SHAPE, F32))


def test_global_rng_stream_is_the_key_off_stream(lib_ops, key, monkeypatch):
    """numpy's global generator after get_minibatch with the key on is where it is after the same call with the key off; the data
    layer hands the drawn matrix to ops.scan_transform, in place, and to the blobs"""
    ops, cfg = lib_ops, key
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    calls = []
    _mock_device(monkeypatch, ops, calls)
    cfg.LIDAR_BV_FROM_SCAN = True
    cfg.TRAIN.SCAN_AUGMENT_SHIFT = (1.0, 1.0, 0.2)
    entry = dict(annotation(3), image=np.zeros((8, 12, 3), np.uint8), velodyne=synth.point_cloud(90, 64))
    before = frozen(entry)
    states, blobs = [], []
    for on in (False, True):
        cfg.TRAIN.SCAN_AUGMENT = on
        np.random.seed(77)
        augment.seed(4)
        blobs.append(get_minibatch([entry], 2))
        states.append(np.random.get_state())
    assert states[0][0] == states[1][0] and np.array_equal(states[0][1], states[1][1]) and states[0][2:] == states[1][2:]
    assert frozen(entry) == before
    assert [c[0] for c in calls] == ["scan_bev", "scan_transform", "scan_bev"]          # key off: no transform
    assert "scan_transform" not in blobs[0] and blobs[0]["calib"] is entry["calib"]
    augment.seed(4)
    theta, s, shift = augment.draw_scan_transform()
    A, Ai = R.transform_matrix(theta, s, shift)
    got = blobs[1]["scan_transform"]
    assert same_bits(got, A) and same_bits(calls[1][1].reshape(3, 4), A)
    assert same_bits(blobs[1]["calib"], R.augment_calib(entry["calib"], Ai))
    from mv3d_tf_amd.datasets.kitti_mv3d import gt_blobs
    want = gt_blobs(R.augment_annotation(entry, A, s), ops.BEV_SHAPE)
    for k in ("gt_boxes", "gt_boxes_bv", "gt_boxes_3d", "gt_boxes_corners", "im_info"):
        assert same_bits(blobs[1][k], want[k]), k
    assert same_bits(blobs[1]["gt_boxes"], blobs[0]["gt_boxes"]) and not same_bits(blobs[1]["gt_boxes_3d"], blobs[0]["gt_boxes_3d"])


def test_ignore_blobs_follow_and_unknown_blob_is_ignored_by_the_stack(lib_ops, key, monkeypatch):
    ops, cfg = lib_ops, key
    from mv3d_tf_amd.fast_rcnn.train_mv import stack_blobs
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    _mock_device(monkeypatch, ops, [])
    cfg.LIDAR_BV_FROM_SCAN = cfg.TRAIN.SCAN_AUGMENT = True
    cfg.TRAIN.IGNORE_TYPES = ("Van", "DontCare")
    entry = dict(annotation(3, True), image=np.zeros((8, 12, 3), np.uint8), velodyne=synth.point_cloud(90, 64))
    augment.seed(6)
    theta, s, shift = augment.draw_scan_transform()
    augment.seed(6)
    frames = [get_minibatch([entry], 2) for _ in range(2)]
    want = R.augment_annotation(entry, R.transform_matrix(theta, s, shift)[0], s)
    assert same_bits(frames[0]["ignore_boxes_bv"], want["ignore_boxes_bv"]) and not same_bits(want["ignore_boxes_bv"], entry["ignore_boxes_bv"])
    assert same_bits(frames[0]["ignore_boxes_img"], entry["ignore_boxes_img"])
    assert not same_bits(frames[0]["scan_transform"], frames[1]["scan_transform"])      # a new sample at every visit
    feed = stack_blobs(frames)
    assert "scan_transform" not in feed and feed["calib"].shape == (2, 4, 12)
    assert same_bits(feed["calib"][1], np.asarray(frames[1]["calib"], F32))


def test_bad_arguments_are_refused_before_any_upload(lib_ops):
    import torch
    ops = lib_ops
    good, A = np.zeros((3, 4), F32), np.zeros((1, 3, 4))
    for exc, args in ((TypeError, (np.zeros((3, 4)), None, A)), (ValueError, (np.zeros((3, 3), F32), None, A)),
                      (ValueError, (torch.zeros(3, 4), None, A)),                                        # a points tensor on the host
                      (TypeError, (good, [0.0, 3.0], A)), (ValueError, (good, [0, 2, 1], np.zeros((2, 12)))), (ValueError, (good, [0, 4], A)),
                      (TypeError, (good, None, A.astype(F32))), (TypeError, (good, None, torch.zeros((1, 12)))),
                      (ValueError, (good, None, np.zeros((3, 4)))), (ValueError, (good, None, np.zeros((1, 11)))),
                      (ValueError, (good, [0, 1, 3], A)), (ValueError, (good, None, np.zeros((2, 3, 4)))),
                      (ValueError, (good, None, torch.zeros((1, 12), dtype=torch.float64))),             # an xform tensor on the host
                      (TypeError, (good, None, A, np.zeros((3, 4), F32))), (TypeError, (good, None, A, torch.zeros((3, 4), dtype=torch.float16))),
                      (ValueError, (good, None, A, torch.zeros((2, 4)))), (ValueError, (good, None, A, torch.zeros((3, 4)))),
                      (ValueError, (good, None, A, torch.zeros((4, 3)).t()))):
        with pytest.raises(exc, match="scan_transform"):
            ops.scan_transform(*args)


def test_c_entry_refuses_invalid_arguments_before_any_launch(lib_ops):
    L, lib = lib_ops.lib(), lib_ops._lib
    fn, U, P = L.mv3d_scan_transform, 1 << 20, 100                                  # non-NULL, aligned "pointers" (never dereferenced)
    IN, OUT, OFF, XF = U, 2 * U, 3 * U, 4 * U
    for args in ((IN, OFF, 1025, P, XF, OUT), (IN, OFF, -1, P, XF, OUT), (IN, OFF, 1, -1, XF, OUT),
                 (IN, None, 2, P, XF, OUT),                                          # no offsets, two frames
                 (None, OFF, 1, P, XF, OUT), (IN, OFF, 1, P, None, OUT), (IN, OFF, 1, P, XF, None), (IN, OFF, 1, 0, None, OUT),
                 (IN + 4, OFF, 1, P, XF, OUT), (IN, OFF + 2, 1, P, XF, OUT), (IN, OFF, 1, P, XF + 4, OUT), (IN, OFF, 1, P, XF, OUT + 8),
                 (IN, OFF, 1, P, XF, IN + 16), (IN, OFF, 1, P, XF, IN + 16 * (P - 1)), (IN + 16 * (P - 1), OFF, 1, P, XF, IN)):
        assert fn(*args, None) == lib.ERR_INVALID_ARG, args
    assert fn(None, None, 0, 0, None, None, None) == lib.OK                           # no frame: nothing to do
    assert fn(None, None, 1, 0, XF, None, None) == lib.OK and fn(IN, OFF, 3, 0, XF, IN, None) == lib.OK        # no row: no launch


# ---------------------------------------------------------------------------------------------------- GPU
def matrices(B):
    return np.stack([R.transform_matrix(*DRAWS[b % 3])[0] for b in range(B)])


def cloud(P, seed=3):
    """P rows around the scan's magnitudes, each with its own reflectance (a row copied from the wrong place shows)"""
    rng = np.random.RandomState(seed)
    pts = np.stack([rng.uniform(-5, 70, P), rng.uniform(-40, 40, P), rng.uniform(-3, 2, P), np.arange(P) + 0.5], 1).astype(F32)
    return pts


def device_transform(gpu, pts, offsets, A, device_offsets=False):
    """the op out of place (on a pre-filled output with 8 guard rows behind it) and in place (8 guard rows behind the cloud) -> the
    (P,4) result as uint32; asserts that both agree, that the guard rows come back untouched and that out of place leaves the input"""
    torch, ops = gpu["torch"], gpu["ops"]
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 4)
    P = len(pts)
    if device_offsets:
        offsets = torch.from_numpy(np.asarray(offsets, np.int32)).cuda()
    d_pts = torch.from_numpy(pts).cuda()
    big = torch.from_numpy(np.full((P + 8, 4), FILL, np.uint32).view(F32)).cuda()
    out = ops.scan_transform(d_pts, offsets, A, out=big[:P])
    fresh = ops.scan_transform(d_pts, offsets, A)
    torch.cuda.synchronize()
    assert (P == 0 or out.data_ptr() == big.data_ptr()) and tuple(fresh.shape) == (P, 4) and fresh.dtype == torch.float32
    host = big.cpu().numpy().view(np.uint32)
    assert (host[P:] == FILL).all(), "rows behind the output were written"
    assert np.array_equal(u32(d_pts.cpu().numpy()), u32(pts)), "the input was written"
    assert np.array_equal(u32(fresh.cpu().numpy()), host[:P])
    place = torch.from_numpy(np.full((P + 8, 4), FILL, np.uint32).view(F32)).cuda()
    place[:P] = d_pts
    view = place[:P]
    same = ops.scan_transform(view, offsets, A, out=view)
    torch.cuda.synchronize()
    assert same is view
    inplace = place.cpu().numpy().view(np.uint32)
    assert (inplace[P:] == FILL).all(), "rows behind the cloud were written"
    assert np.array_equal(inplace[:P], host[:P]), "in place differs from out of place"
    return host[:P]


def check_against_restatement(gpu, pts, offsets, A, device_offsets=False):
    want = R.transform_rows(pts, offsets, A)
    got = device_transform(gpu, pts, offsets, A, device_offsets)
    assert np.array_equal(got, u32(want)), np.flatnonzero((got != u32(want)).any(1))[:8]
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("P", [0, 1, 255, 256, 257, 3 * 256 + 5])
def test_one_frame_sizes(gpu, P):
    pts = cloud(P)
    want = check_against_restatement(gpu, pts, None, matrices(1))
    assert P == 0 or not np.array_equal(u32(want)[:, :3], u32(pts)[:, :3])
    assert np.array_equal(u32(want)[:, 3], u32(pts)[:, 3])
    check_against_restatement(gpu, pts, None, matrices(1).reshape(1, 12))              # the (B, 12) form


@pytest.mark.gpu
def test_three_frames_with_an_empty_one_and_unowned_rows(gpu):
    """offsets start at 7 and end 9 rows before P; frame 1 is empty; every frame has its own matrix"""
    P = 2 * 256 + 77
    pts = cloud(P, 4)
    offsets = np.array([7, 300, 300, P - 9], np.int32)
    A = matrices(3)
    for dev in (False, True):
        want = check_against_restatement(gpu, pts, offsets, A, device_offsets=dev)
    assert np.array_equal(u32(want)[:7], u32(pts)[:7]) and np.array_equal(u32(want)[P - 9:], u32(pts)[P - 9:])      # unowned: the same bits
    assert np.array_equal(u32(want[7:300]), u32(R.transform_rows(pts[7:300], None, A[0:1])))
    assert np.array_equal(u32(want[300:P - 9]), u32(R.transform_rows(pts[300:P - 9], None, A[2:3])))
    assert not np.array_equal(u32(want[300:P - 9]), u32(R.transform_rows(pts[300:P - 9], None, A[0:1])))


@pytest.mark.gpu
def test_more_frames_in_a_workgroup_than_it_stages(gpu):
    """frames of 5 rows: 256 consecutive rows touch 52 frames, more than a workgroup keeps in LDS"""
    B = 120
    P = 5 * B + 3
    rng = np.random.RandomState(8)
    A = np.stack([R.transform_matrix(rng.uniform(-3, 3), rng.uniform(0.5, 2), rng.uniform(-5, 5, 3))[0] for _ in range(B)])
    check_against_restatement(gpu, cloud(P, 5), np.arange(0, 5 * B + 1, 5, dtype=np.int32), A)


@pytest.mark.gpu
@pytest.mark.parametrize("offsets", [[400, 300, 200, 100], [0, 500, 100, 600], [-5, 100, 10 ** 6, 2 * 10 ** 6], [700, 800, 900, 2 ** 31 - 1],
                                     [0, 0, 0, 0], [-2 ** 31, -1, 600, 600]])
def test_malformed_device_offsets_stay_in_bounds(gpu, offsets):
    P = 600
    pts = cloud(P, 6)
    want = check_against_restatement(gpu, pts, offsets, matrices(3), device_offsets=True)
    owned = np.array([C.frame_of_row(offsets, p) is not None for p in range(P)])
    assert np.array_equal(u32(want)[~owned], u32(pts)[~owned])


@pytest.mark.gpu
def test_special_values(gpu):
    sub = 1e-42
    rows = [(1, 2, 3, 0.5), (0, 0, 0, 1), (-0.0, -0.0, -0.0, -0.0), (sub, -sub, sub, sub), (3e38, 3e38, -3e38, 2), (1e-30, 70, -2, 3),
            (1, 0, 0, NAN), (1, 0, 0, INF), (1, 0, 0, -INF)]
    for bad in (NAN, INF, -INF):
        for axis in range(3):
            row = [1.5, -2.5, 0.75, 4.0]
            row[axis] = bad
            rows.append(tuple(row))
    rows.append((NAN, INF, -INF, NAN))
    pts = np.array(rows * 2, F32)
    nan_cells = np.argwhere(np.isnan(pts))
    pts.view(np.uint32)[nan_cells[:, 0], nan_cells[:, 1]] = 0x7FC12345 + np.arange(len(nan_cells), dtype=np.uint32)      # NaNs with payloads
    n = len(rows)
    want = check_against_restatement(gpu, pts, [0, n, 2 * n], matrices(2))
    passed = ~np.isfinite(pts[:, :3]).all(1)
    assert passed.sum() == 20 and np.array_equal(u32(want)[passed], u32(pts)[passed])          # all 16 bytes
    assert np.array_equal(u32(want)[:, 3], u32(pts)[:, 3])                                      # the reflectance bits, NaN payloads included
    assert np.isinf(want[4, :3]).any()                                                          # (an overflow of the f32 rounding is what it is)


@pytest.mark.gpu
def test_capture_and_replay(gpu):
    """ONE graph of the call with out= given, replayed after the cloud, the device offsets and the matrices have been overwritten in
    their buffers (the capacity stays)"""
    torch, ops = gpu["torch"], gpu["ops"]
    cap = 1000
    fillings = [(cloud(cap, seed), np.cumsum((0,) + sizes).astype(np.int32), matrices(3)[list(order)])
                for seed, sizes, order in ((21, (400, 500), (0, 1)), (22, (990, 10), (2, 0)), (23, (0, 3), (1, 2)))]
    buf = torch.from_numpy(fillings[0][0]).cuda()
    d_off = torch.from_numpy(fillings[0][1]).cuda()
    d_A = torch.from_numpy(fillings[0][2]).cuda()
    out = torch.empty((cap, 4), device="cuda")
    call = lambda: ops.scan_transform(buf, d_off, d_A, out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                                          # (warm-up: the code object is loaded outside the capture)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res = call()
    assert res is out
    for pts, offsets, A in reversed(fillings):
        buf.copy_(torch.from_numpy(pts))
        d_off.copy_(torch.from_numpy(offsets))
        d_A.copy_(torch.from_numpy(A))
        out.view(torch.int32).fill_(0x5A5A5A5A)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(u32(out.cpu().numpy()), u32(R.transform_rows(pts, offsets, A)))


@pytest.mark.gpu
def test_the_corners_through_the_kernel_are_the_annotation_s(gpu):
    torch, ops = gpu["torch"], gpu["ops"]
    e = annotation(7)
    cnr = e["boxes_corners"].reshape(7, 3, 8)
    pts = np.zeros((56, 4), F32)
    pts[:, :3] = cnr.transpose(0, 2, 1).reshape(56, 3)
    for theta, s, t in DRAWS:
        A, _ = augment.transform_matrix(theta, s, t)
        got = ops.scan_transform(pts, None, A[None]).cpu().numpy()
        back = got[:, :3].reshape(7, 8, 3).transpose(0, 2, 1).reshape(7, 24)
        assert same_bits(back, augment.augment_annotation(e, A, s)["boxes_corners"])


@pytest.fixture(scope="module")
def frame():
    """a synthetic scan, the image and the three-object annotation of the end-to-end tests, and what the restatement makes of the
    scan (plain and mirrored) under the draw the tests' seed gives: computed once"""
    from mv3d_tf_amd.fast_rcnn.config import cfg
    pts = synth.point_cloud(90, 4096)
    image = np.random.RandomState(1).randint(0, 255, HW + (3,)).astype(np.uint8)
    plain = dict(annotation(3, True), image=image, velodyne=pts)
    flipped = mirror_annotation(annotation(3, True), HW[1])
    flipped.update(image=image, velodyne=pts, calib=mirror_calib(plain["calib"], HW[1]))
    shift = (1.0, 1.0, 0.2)
    rng = np.random.RandomState(41)
    rot, (lo, hi) = cfg.TRAIN.SCAN_AUGMENT_ROTATION, cfg.TRAIN.SCAN_AUGMENT_SCALE
    theta, s = rng.uniform(-rot, rot), rng.uniform(lo, hi)
    t = tuple(rng.uniform(-b, b) for b in shift)
    A, Ai = R.transform_matrix(theta, s, t)
    out = {"shift": shift, "seed": 41, "A": A, "Ai": Ai, "scale": s}
    for name, entry in (("plain", plain), ("flipped", flipped)):
        host = pts * F32([1, -1, 1, 1]) if entry["flipped"] else pts.copy()
        moved = R.transform_rows(host, None, [A])
        table = R.augment_calib(entry["calib"], Ai)
        keep = C.keep_mask(moved, None, [table], [HW])
        for a in (host, moved, keep):
            a.setflags(write=False)
        out[name] = {"entry": entry, "host": host, "moved": moved, "calib": table, "keep": keep, "annotation": R.augment_annotation(entry, A, s)}
    return out


def test_the_end_to_end_fixture_is_what_it_is_meant_to_be(frame):
    for name in ("plain", "flipped"):
        f = frame[name]
        assert 0.10 <= f["keep"].mean() <= 0.90 and not np.array_equal(f["moved"][:, :3], f["host"][:, :3])
        assert (f["entry"]["gt_classes"] != 0).sum() == 3 and bool(f["entry"]["flipped"]) == (name == "flipped")


@pytest.mark.gpu
@pytest.mark.parametrize("which,crop,encoding", [("plain", False, "reference"), ("flipped", False, "reference"), ("plain", True, "reference"),
                                                 ("flipped", True, "reference"), ("plain", False, "paper"), ("plain", True, "paper")])
def test_get_minibatch_under_the_key(gpu, frame, key, which, crop, encoding):
    torch, ops, cfg = gpu["torch"], gpu["ops"], key
    from mv3d_tf_amd.datasets.kitti_mv3d import gt_blobs, ignore_blobs
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    f = frame[which]
    cfg.LIDAR_BV_FROM_SCAN = cfg.FRONT_VIEW_INPUT = cfg.TRAIN.SCAN_AUGMENT = True
    cfg.LIDAR_CROP_TO_IMAGE, cfg.LIDAR_BV_ENCODING = crop, encoding
    cfg.TRAIN.SCAN_AUGMENT_SHIFT, cfg.TRAIN.IGNORE_TYPES = frame["shift"], ("Van", "DontCare")
    before = frozen(f["entry"])
    augment.seed(frame["seed"])
    np.random.seed(55)
    blobs = get_minibatch([f["entry"]], 2)
    on_state = np.random.get_state()
    assert frozen(f["entry"]) == before
    want_pts = f["moved"][f["keep"]] if crop else f["moved"]
    d = torch.from_numpy(np.ascontiguousarray(want_pts)).cuda()
    raster = ops.point_cloud_2_top_paper if encoding == "paper" else ops.point_cloud_2_top_batch
    bev, fv = raster(d), ops.point_cloud_2_front(d)
    chans = 10 if encoding == "paper" else 9
    assert tuple(blobs["lidar_bv_data"].shape) == (1, 601, 601, chans) and tuple(blobs["lidar_fv_data"].shape) == (1, 64, 512, 3)
    assert bool(bev.any()) and torch.equal(blobs["lidar_bv_data"][0].view(torch.int32), bev.view(torch.int32))
    assert bool(fv.any()) and torch.equal(blobs["lidar_fv_data"][0].view(torch.int32), fv.view(torch.int32))
    untouched = raster(torch.from_numpy(np.ascontiguousarray(f["host"])).cuda())
    assert not torch.equal(untouched.view(torch.int32), bev.view(torch.int32))          # (the transform shows in the map)
    assert same_bits(blobs["scan_transform"], frame["A"]) and same_bits(blobs["calib"], f["calib"])
    want = gt_blobs(f["annotation"], ops.BEV_SHAPE)
    for k in ("gt_boxes", "gt_boxes_bv", "gt_boxes_3d", "gt_boxes_corners", "im_info"):
        assert same_bits(blobs[k], want[k]), k
    for k, v in ignore_blobs(f["annotation"]).items():
        assert same_bits(blobs[k], v), k
    # the image is the key-off image, and numpy's global stream is where the key-off call leaves it
    cfg.TRAIN.SCAN_AUGMENT = False
    np.random.seed(55)
    off = get_minibatch([f["entry"]], 2)
    state = np.random.get_state()
    assert state[0] == on_state[0] and np.array_equal(state[1], on_state[1]) and state[2:] == on_state[2:]
    img_on, img_off = (b["image_data"] for b in (blobs, off))
    assert torch.equal(ops._dev(img_on), ops._dev(img_off))
    assert same_bits(blobs["gt_boxes"], off["gt_boxes"])


@pytest.mark.gpu
def test_key_off_is_the_parent_s_code_path(gpu, frame, key, monkeypatch):
    torch, ops, cfg = gpu["torch"], gpu["ops"], key
    from mv3d_tf_amd.datasets.kitti_mv3d import gt_blobs
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch

    def never(*a, **kw):
        raise AssertionError("called with cfg.TRAIN.SCAN_AUGMENT off")

    monkeypatch.setattr(ops, "scan_transform", never)
    monkeypatch.setattr(augment, "draw_scan_transform", never)
    cfg.LIDAR_BV_FROM_SCAN = cfg.FRONT_VIEW_INPUT = True
    for which in ("plain", "flipped"):
        f = frame[which]
        blobs = get_minibatch([f["entry"]], 2)
        d = torch.from_numpy(np.ascontiguousarray(f["host"])).cuda()
        assert "scan_transform" not in blobs and blobs["calib"] is f["entry"]["calib"]
        assert torch.equal(blobs["lidar_bv_data"][0].view(torch.int32), ops.point_cloud_2_top_batch(d).view(torch.int32))
        assert torch.equal(blobs["lidar_fv_data"][0].view(torch.int32), ops.point_cloud_2_front(d).view(torch.int32))
        want = gt_blobs(f["entry"], ops.BEV_SHAPE)
        for k in ("gt_boxes", "gt_boxes_bv", "gt_boxes_3d", "gt_boxes_corners", "im_info"):
            assert same_bits(blobs[k], want[k]), k
