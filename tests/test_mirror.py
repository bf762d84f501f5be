"""Mirrored training frames (cfg.TRAIN.USE_FLIPPED): the left/right mirror of a frame's annotation and
calibration (mv3d_tf_amd/datasets/mirror.py, host numpy) and of its maps (mv3d_mirror_columns, csrc/mirror.hip).

CPU tests: the BEV box rule against the reference-generated fixture and the oracle; the mirror of an annotation against the
oracle's encoding of the MIRRORED LABEL (tx -> -tx, ry -> pi - ry, Tr -> Tr'), which is what makes the mirror more than a
convention; the calibration's projection identity.  `gpu` tests: the kernel bit for bit, the BEV raster commuting with it, and
the product's encoder on mirrored label lines."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from test_kitti_formats import ANN_KEYS, _same

from mv3d_tf_amd.datasets.mirror import lidar_box_to_bv, mirror_annotation, mirror_calib

WIDTHS = (1242, 1224, 7)
SWAP = [1, 0, 3, 2, 5, 4, 7, 6]


def _entry(g, i):
    e = {k: np.array(g["ann%d_%s" % (i, k)]) for k in ANN_KEYS}
    e["flipped"] = False
    return e


def _population():
    """the 3 000 objects of tests/test_kitti_formats.py:100-107 (yaw at +-pi, 0, pi/2 among them)"""
    rng = np.random.RandomState(4)
    G = 3000
    box = np.stack([rng.uniform(-40, 40, G), rng.uniform(0.5, 2.5, G), rng.uniform(0.5, 80, G), rng.uniform(0.3, 12, G),
                    rng.uniform(0.3, 3, G), rng.uniform(0.5, 4, G)], 1).astype(np.float32)
    ry = rng.uniform(-np.pi, np.pi, G); ry[:4] = [np.pi, -np.pi, 0.0, np.pi / 2]
    return box, ry


def _wrap(a):
    """pi - a brought back into (-pi, pi], f64: the yaw / alpha of the mirrored label"""
    m = np.pi - np.asarray(a, np.float64)
    return np.where(m > np.pi, m - 2 * np.pi, m)


def _encoded_entry(oracle, box, ry, tr, rng):
    """a roidb entry of the oracle's encodings (every field mirror_annotation reads)"""
    cam, lid, b3, bv = oracle.gt_encode(box, ry, tr)
    G = len(box)
    x1 = rng.randint(0, 4000, G) / 4.0
    boxes = np.stack([x1, rng.randint(0, 1400, G) / 4.0, x1 + rng.randint(4, 800, G) / 4.0, rng.randint(1400, 1500, G) / 4.0], 1)
    return {"ry": ry.astype(np.float32), "alphas": rng.uniform(-np.pi, np.pi, G).astype(np.float32), "lwh": box[:, 3:].copy(),
            "boxes": boxes.astype(np.float32), "boxes_3D_cam": box.copy(), "xyz": box[:, :3].copy(), "boxes3D_cam_corners": cam,
            "boxes_corners": lid, "boxes_3D": b3, "boxes_bv": bv, "gt_classes": np.ones(G, np.int32),
            "gt_overlaps": np.tile(np.float32([0, 1]), (G, 1)), "flipped": False}


def _mirrored_label(box, ry, table, W):
    """what a label file of the mirrored scene holds: tx negated, yaw pi - ry, and Tr' of the mirrored calibration"""
    box_m = box.copy()
    box_m[:, 0] = -box_m[:, 0]
    return box_m, _wrap(ry), mirror_calib(table, W)[3].reshape(3, 4).astype(np.float32)


def _assert_encodings_agree(got, want, what):
    """got / want: dicts with the four encodings.  Corners and LIDAR box within 1e-4 m (ten times the f32 spacing at 80 m, plus a
    one-ulp difference of the inverted rotation times 80 m); BEV boxes within one pixel, no more than 1 % of the boxes differing."""
    for k in ("boxes3D_cam_corners", "boxes_corners", "boxes_3D"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        d = np.abs(got[k].astype(np.float64) - want[k]).max()
        print(what, k, "max difference", d)
        assert d <= 1e-4, (what, k, d)
    assert got["boxes_bv"].shape == want["boxes_bv"].shape and got["boxes_bv"].dtype == want["boxes_bv"].dtype
    d = np.abs(got["boxes_bv"].astype(np.float64) - want["boxes_bv"])
    differing = np.count_nonzero(d.max(axis=1))
    print(what, "boxes_bv max difference", d.max(), "boxes differing", differing, "of", len(d))
    assert d.max() <= 1.0 and differing <= 0.01 * len(d), (what, d.max(), differing)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_bev_box_rule_matches_fixture_and_oracle(oracle):
    g = golden("kitti_label")
    seen = 0
    for i in range(int(g["n_frames"])):
        if len(g["ann%d_boxes_3D" % i]):
            assert _same(lidar_box_to_bv(g["ann%d_boxes_3D" % i]), g["ann%d_boxes_bv" % i]), i
            seen += 1
    assert seen >= 2
    box, ry = _population()
    _, _, b3, bv = oracle.gt_encode(box, ry, g["calib_0"][3].reshape(3, 4).astype(np.float32))
    assert _same(lidar_box_to_bv(b3), bv)
    assert _same(lidar_box_to_bv(np.zeros((0, 6), np.float32)), np.zeros((0, 4), np.float32))


@pytest.mark.parametrize("W", WIDTHS)
def test_mirror_annotation_copies_and_is_an_involution(W):
    """the input entry stays bit-identical; mirrored twice, every array field comes back bit-identical -- ry / alphas as
    (cos, sin) within 1e-6 (two f32 roundings at magnitude <= pi, 2.4e-7 each; +-pi may come back as the other sign)."""
    g = golden("kitti_label")
    for i in range(int(g["n_frames"])):
        e = _entry(g, i)
        keep = {k: np.array(v, copy=True) for k, v in e.items()}
        m = mirror_annotation(e, W)
        assert all(_same(e[k], keep[k]) for k in keep) and e["flipped"] is False
        assert m["flipped"] is True and set(m) == set(e) | {"boxes_residual"}
        assert m["boxes_residual"].dtype == np.float32 and m["boxes_residual"].shape == e["boxes"].shape
        assert np.abs(m["boxes_residual"]).max(initial=0) <= 2.0 ** -14                       # half the f32 spacing below 2048
        assert all(m[k] is not e[k] and not np.shares_memory(m[k], e[k]) for k in ANN_KEYS)
        assert all(m[k].shape == e[k].shape and m[k].dtype == e[k].dtype for k in ANN_KEYS), i
        for k in ("lwh", "gt_classes", "gt_overlaps"):
            assert _same(m[k], e[k])
        mm = mirror_annotation(m, W)
        for k in ANN_KEYS:
            if k in ("ry", "alphas"):
                assert np.abs(np.cos(mm[k].astype(np.float64)) - np.cos(e[k].astype(np.float64))).max(initial=0) <= 1e-6
                assert np.abs(np.sin(mm[k].astype(np.float64)) - np.sin(e[k].astype(np.float64))).max(initial=0) <= 1e-6
            else:
                assert _same(mm[k], e[k]), (i, k)
        assert not mm["boxes_residual"].any()
    # the empty frame: well-formed empty arrays
    m = mirror_annotation(_entry(g, 2), W)
    assert m["boxes"].shape == (0, 4) and m["boxes_corners"].shape == (0, 24) and m["boxes_bv"].shape == (0, 4)
    assert m["ry"].shape == (0,) and m["gt_overlaps"].shape == (0, 2)


@pytest.mark.parametrize("W", WIDTHS)
def test_mirror_annotation_twice_restores_the_image_boxes_bit_for_bit(W):
    """`boxes` of the involution above: bit-identical after two mirrors.  x -> (W - 1) - x stored as f32 alone cannot be undone
    when the mirrored value lies in a higher binade than x (on this fixture 5 of 56 coordinates would come back changed at
    W = 1242 and 1224, by up to 5.9e-5 px); mirror_annotation carries the dropped part in `boxes_residual`, which makes it exact."""
    g = golden("kitti_label")
    worst, changed, total = 0.0, 0, 0
    for i in range(int(g["n_frames"])):
        e = _entry(g, i)
        mm = mirror_annotation(mirror_annotation(e, W), W)
        d = np.abs(mm["boxes"].astype(np.float64) - e["boxes"])
        worst, changed, total = max(worst, d.max(initial=0)), changed + np.count_nonzero(d), total + d.size
    print("W", W, "coordinates changed", changed, "of", total, "max difference", worst)
    assert changed == 0, (W, changed, total, worst)
    # and on label-like coordinates anywhere in the image, not only the fixture's
    e = _entry(g, 0)
    x = np.round(np.random.RandomState(W).uniform(0.0, 1300.0, (2000, 4)), 2).astype(np.float32)
    e.update({k: np.resize(e[k], (2000,) + e[k].shape[1:]) for k in ANN_KEYS}, boxes=x.copy())
    m = mirror_annotation(e, W)
    assert np.array_equal(m["boxes"][:, [2, 1, 0, 3]], ((W - 1) * np.float64([1, 0, 1, 0]) + x * np.float64([-1, 1, -1, 1])).astype(np.float32))
    assert _same(mirror_annotation(m, W)["boxes"], x)


def test_mirror_annotation_is_the_encoding_of_the_mirrored_label(oracle):
    """oracle.gt_encode(tx negated, wrap(pi - ry), Tr') against the mirror of oracle.gt_encode(box, ry, Tr)"""
    g = golden("kitti_label")
    table = g["calib_0"]
    tr = table[3].reshape(3, 4).astype(np.float32)
    box, ry = _population()
    rng = np.random.RandomState(11)
    for W in WIDTHS[:2]:
        e = _encoded_entry(oracle, box, ry, tr, rng)
        m = mirror_annotation(e, W)
        box_m, ry_m, tr_m = _mirrored_label(box, ry, table, W)
        cam, lid, b3, bv = oracle.gt_encode(box_m, ry_m, tr_m)
        want = {"boxes3D_cam_corners": cam, "boxes_corners": lid, "boxes_3D": b3, "boxes_bv": bv}
        _assert_encodings_agree(m, want, "W=%d" % W)
        assert _same(m["boxes_3D_cam"], box_m) and _same(m["xyz"], box_m[:, :3])
        assert np.abs(np.cos(m["ry"].astype(np.float64)) - np.cos(ry_m)).max() <= 1e-6
        assert np.abs(np.sin(m["ry"].astype(np.float64)) - np.sin(ry_m)).max() <= 1e-6
        x = e["boxes"].astype(np.float64)                          # quarter pixels: the rule is exact
        assert _same(m["boxes"], np.stack([W - x[:, 2] - 1, x[:, 1], W - x[:, 0] - 1, x[:, 3]], 1).astype(np.float32))
        # guard of this test: WITHOUT the j <-> j ^ 1 exchange the corners are far off
        plain = e["boxes_corners"].reshape(-1, 3, 8).copy()
        plain[:, 1] = -plain[:, 1]
        assert np.abs(plain.reshape(-1, 24) - lid).max() > 0.1
        assert _same(m["boxes_corners"], plain[:, :, SWAP].reshape(-1, 24))


def _project(table, X):
    """pixels (u, v) of LIDAR points X (N, 3) through a (4, 12) calibration table, f64"""
    P2, R0, Tr = table[0].reshape(3, 4), table[2, :9].reshape(3, 3), table[3].reshape(3, 4)
    cam = R0 @ (Tr @ np.hstack([X, np.ones((len(X), 1))]).T)
    uvw = P2 @ np.vstack([cam, np.ones((1, len(X)))])
    return uvw[0] / uvw[2], uvw[1] / uvw[2]


@pytest.mark.parametrize("W", WIDTHS)
def test_mirror_calib_signs_and_projection_identity(W):
    g = golden("kitti_label")
    rng = np.random.RandomState(5)
    X = np.stack([rng.uniform(2, 70, 1000), rng.uniform(-30, 30, 1000), rng.uniform(-2.5, 1.0, 1000)], 1)
    for i in range(int(g["n_frames"])):
        t = g["calib_%d" % i]
        keep = t.copy()
        m = mirror_calib(t, W)
        assert _same(t, keep) and m.dtype == np.float64 and m.shape == (4, 12)
        assert np.array_equal(m.astype(np.float32).astype(np.float64), m)                   # f64 holding f32 values
        R0, Tr = t[2, :9].reshape(3, 3), t[3].reshape(3, 4)
        sr = np.outer([-1, 1, 1], [-1, 1, 1])                                               # Mc R0 Mc
        st = np.outer([-1, 1, 1], [1, -1, 1, 1])                                            # Mc Tr M
        assert np.array_equal(m[2, :9].reshape(3, 3), sr * R0) and np.array_equal(m[2, 9:], np.zeros(3))
        assert np.array_equal(m[3].reshape(3, 4), st * Tr)
        F = np.array([[-1.0, 0, W - 1], [0, 1, 0], [0, 0, 1]])
        for row in (0, 1):                                                                  # P2' = F P2 Mc, P3 the same way
            want = (F @ t[row].reshape(3, 4) @ np.diag([-1.0, 1, 1, 1])).ravel()
            assert np.array_equal(m[row], want.astype(np.float32).astype(np.float64)), (i, row)
            assert np.array_equal(m[row, 4:], t[row, 4:] * ([-1, 1, 1, 1] * 2))             # rows 1 and 2: signs only
        u, v = _project(t, X)
        Xm = X * [1, -1, 1]
        um, vm = _project(m, Xm)
        d = max(np.abs(um - (W - 1 - u)).max(), np.abs(vm - v).max())
        print("frame", i, "W", W, "projection identity: max difference", d, "px")
        assert d <= 1e-3, (i, W, d)
    with pytest.raises(ValueError):
        mirror_calib(np.zeros((3, 4)), W)


# ------------------------------------------------------------------------------------------------------------ GPU
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    return torch


def _payload(rng, shape):
    """f32 data with NaN payloads, -0.0 and +-inf among it, as uint32 bit patterns"""
    bits = rng.randint(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = bits.reshape(-1)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001], np.uint32)
    n = min(len(special), flat.size)
    flat[rng.permutation(flat.size)[:n]] = special[:n]
    return bits


KERNEL_SHAPES = [(1, 1, 1), (3, 1, 3), (1, 2, 1), (2, 2, 3), (5, 3, 9), (7, 64, 1), (3, 65, 3), (2, 601, 9), (4, 1242, 3),
                 (1, 255, 16), (129, 7, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_mirror_columns_bit_for_bit(shape):
    torch = _gpu()
    from mv3d_tf_amd import ops
    bits = _payload(np.random.RandomState(sum(shape)), shape)
    t = torch.from_numpy(bits.view(np.int32)).cuda().view(torch.float32)
    out = ops.mirror_columns(t)
    assert out is t
    got = t.view(torch.int32).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, bits[:, ::-1, :])
    ops.mirror_columns(t)                                                                   # twice: the bytes are back
    assert np.array_equal(t.view(torch.int32).cpu().numpy().view(np.uint32), bits)


@pytest.mark.gpu
def test_mirror_columns_shapes_slices_and_bad_arguments():
    torch = _gpu()
    from mv3d_tf_amd import _lib, ops
    rng = np.random.RandomState(3)
    as_dev = lambda bits: torch.from_numpy(bits.view(np.int32)).cuda().view(torch.float32)
    as_bits = lambda t: t.view(torch.int32).cpu().numpy().view(np.uint32)
    for shape in ((2, 3, 5, 3), (2, 2, 3, 6, 9)):                                           # 4-D and 5-D through the op
        bits = _payload(rng, shape)
        assert np.array_equal(as_bits(ops.mirror_columns(as_dev(bits))), bits[..., ::-1, :])
    # frame 1 of a batch through its slice: the neighbours stay
    bits = _payload(rng, (3, 4, 601, 9))
    t = as_dev(bits)
    ops.mirror_columns(t[1])
    got = as_bits(t)
    assert np.array_equal(got[0], bits[0]) and np.array_equal(got[2], bits[2]) and np.array_equal(got[1], bits[1][:, ::-1, :])
    # rows = 0: OK, nothing written (a NULL pointer is fine there); an empty tensor through the op
    L = _lib.lib()
    assert L.mv3d_mirror_columns(None, 0, 601, 9, None) == _lib.OK
    guard = as_dev(bits[0])
    assert L.mv3d_mirror_columns(C.c_void_p(guard.data_ptr()), 0, 601, 9, ops._stream()) == _lib.OK
    torch.cuda.synchronize()
    assert np.array_equal(as_bits(guard), bits[0])
    assert ops.mirror_columns(torch.empty((0, 5, 3), device="cuda")).shape == (0, 5, 3)
    # bad arguments at the C entry: the status code only, nothing is launched
    A = C.c_void_p(4096)
    for args in ((None, 1, 4, 3), (A, -1, 4, 3), (A, 1, 0, 3), (A, 1, 4, 0), (A, 1, -2, 3), (A, 1, 1 << 20, 1 << 12)):
        assert L.mv3d_mirror_columns(args[0], args[1], args[2], args[3], None) == _lib.ERR_INVALID_ARG, args[1:]
    # bad tensors at the op
    good = torch.zeros((2, 4, 3), device="cuda")
    for bad in (good.cpu(), good.double(), good.half(), good.int(), np.zeros((2, 4, 3), np.float32)):
        with pytest.raises(TypeError):
            ops.mirror_columns(bad)
    for bad in (good[0], good.permute(1, 0, 2), good[:, ::2], good[:, :, :2], torch.zeros((2, 0, 3), device="cuda")):
        with pytest.raises(ValueError):
            ops.mirror_columns(bad)
    assert torch.count_nonzero(good).item() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
def test_bev_raster_commutes_with_the_mirror(seed):
    """point_cloud_2_top of the cloud with y negated == mirror_columns of the cloud's raster, bit for bit: the column is
    int(-y / res), odd in y; the side filter is the open (-30, 30); the last writer wins in point order"""
    torch = _gpu()
    from mv3d_tf_amd import ops, synth
    pts = synth.point_cloud(seed, P=20000)
    ys = np.float32([0, 0.05, -0.05, 0.1, -0.1, 29.99, -29.99, 30, -30])
    pts[5000:5000 + len(ys), 1] = ys
    pts[5000:5000 + len(ys), 0] = np.float32(10.0) + np.arange(len(ys), dtype=np.float32)
    pts[5000:5000 + len(ys), 2] = np.float32(-1.0)
    pts[6000:6040, :2] = np.float32([33.33, 4.21])                                          # forty points in one cell, z as drawn
    pts[6040:6080, :2] = np.float32([33.33, -4.21])                                         # and in its mirror cell
    top = ops.point_cloud_2_top(torch.from_numpy(pts).cuda())
    neg = pts.copy()
    neg[:, 1] = -neg[:, 1]
    top_neg = ops.point_cloud_2_top(torch.from_numpy(neg).cuda())
    assert torch.count_nonzero(top).item() > 1000 and not torch.equal(top, top_neg)
    mirrored = ops.mirror_columns(top.clone())
    assert torch.equal(mirrored.view(torch.int32), top_neg.view(torch.int32))


@pytest.mark.gpu
def test_parse_kitti_labels_of_the_mirrored_lines(oracle):
    """the product's encoder on the label lines of the mirrored scene with Tr', against the mirror of its encoding of the scene"""
    _gpu()
    from mv3d_tf_amd.datasets import parse_kitti_labels
    g = golden("kitti_label")
    table = g["calib_0"]
    tr = table[3].reshape(3, 4).astype(np.float32)
    box, ry = _population()
    rng = np.random.RandomState(12)
    G = len(box)
    alpha = rng.uniform(-np.pi, np.pi, G)
    x1 = rng.randint(0, 4000, G) / 4.0
    b2 = np.stack([x1, rng.randint(0, 1400, G) / 4.0, x1 + rng.randint(4, 800, G) / 4.0, rng.randint(1400, 1500, G) / 4.0], 1)
    line = "Car 0 0 %r %r %r %r %r %r %r %r %r %r %r %r"
    fmt = lambda al, b2, box, ry: [line % (float(a), float(q[0]), float(q[1]), float(q[2]), float(q[3]), float(b[5]), float(b[4]),
                                           float(b[3]), float(b[0]), float(b[1]), float(b[2]), float(r))
                                   for a, q, b, r in zip(al, b2, box, ry)]
    cls = {"__background__": 0, "Car": 1}
    ann = parse_kitti_labels(fmt(alpha, b2, box, ry), tr, cls, 2)
    for W in WIDTHS[:2]:
        box_m, ry_m, tr_m = _mirrored_label(box, ry, table, W)
        b2_m = np.stack([W - b2[:, 2] - 1, b2[:, 1], W - b2[:, 0] - 1, b2[:, 3]], 1)
        want = parse_kitti_labels(fmt(_wrap(alpha), b2_m, box_m, ry_m), tr_m, cls, 2)
        got = mirror_annotation(ann, W)
        _assert_encodings_agree(got, want, "W=%d" % W)
        for k in ("boxes", "boxes_3D_cam", "xyz", "lwh", "gt_classes"):
            assert _same(got[k], want[k]), k
        assert _same(got["gt_overlaps"].toarray(), want["gt_overlaps"].toarray())
        for k in ("ry", "alphas"):
            a, b = got[k].astype(np.float64), want[k].astype(np.float64)
            assert max(np.abs(np.cos(a) - np.cos(b)).max(), np.abs(np.sin(a) - np.sin(b)).max()) <= 1e-6, k
