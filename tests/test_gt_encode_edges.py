"""KITTI label rows -> ground-truth encodings at their edges: `mv3d_gt_encode` (csrc/gt_encode.hip) behind
`datasets.parse_kitti_labels` / `kitti_mv3d`, which restates lib/datasets/kitti_mv3d.py:240-272 = computeCorners3D,
camera_to_lidar_cnr, lidar_cnr_to_3d and lidar_3d_to_bv.

One case table (`cases`: KITTI label / calib TEXT, the product's input) feeds three descriptions of the same thing:
  1. a recording of the reference's own loader on those files (tests/golden/gt_encode_edges.npz, written by
     tests/golden/make_gt_encode_edge_golden.py, which imports this table),
  2. the CPU oracle (oracle.gt_encode) on the numbers parsed here from the text,
  3. the device, under `-m gpu`: the loader on a KITTI tree of the cases, and the C entry with guarded outputs.
Every comparison is on bit patterns (f32 as u32, f64 as u64), except that any NaN matches any NaN.  No tolerances.

The BEV box is 600 - (corner - origin) // 0.1 in f64, the corner an f32 sum.  An f32 corner is never a multiple of the f64
0.1; what a label can put "on a cell edge" is the f32 nearest to k / 10 (x axis) or to k / 10 - 30 (y axis), where the quotient
is within 1e-7 of an integer, and for k a multiple of 5 the corner IS k / 10: there numpy's floor-division differs from
floor(a / 0.1) (0.5 // 0.1 = 4).  `grid_axis` reaches these values exactly: under the axis-aligned calibration, with a yaw of 0
or +-pi and the extent across the targeted axis zero, the LIDAR centre is the label's translation bit for bit, so the corner
is f32(centre + extent / 2) of two numbers chosen here.  The other yaws and `grid_kitti` put the same objects next to the
edges.
"""
import os

import numpy as np
import pytest

from conftest import golden
from mv3d_tf_amd import synth
from mv3d_tf_amd.datasets import load_kitti_calib, pack_calib
from test_box_tail_edges import assert_same, place, same, sha_of, step

FIXTURE = "gt_encode_edges"
F32 = np.float32
WG = 64                           # objects per workgroup of gt_encode_kernel
RECORD_ARRAY_BYTES = 16384        # larger outputs are stored as test_box_tail_edges.sha_of
ANN_KEYS = ("ry", "lwh", "boxes", "boxes_bv", "boxes_3D_cam", "boxes_3D", "boxes3D_cam_corners", "boxes_corners",
            "gt_classes", "gt_overlaps", "xyz", "alphas", "flipped")
GEOMETRY = ("boxes3D_cam_corners", "boxes_corners", "boxes_3D", "boxes_bv")          # mv3d_gt_encode's four outputs, in order

# Cases the reference itself cannot run: name -> the exception type it raised (recorded in the fixture under exc__<name>).
REFERENCE_RAISES = {}

K_LO, K_HI = -8, 609              # cell edges -8 .. 608: the 0 .. 600 map and a margin of 8 either side
SIZES_G = (1, 63, 64, 65)
AXIS_TR = "Tr_velo_to_cam: 0 -1 0 0 0 0 -1 0 1 0 0 0"
PI, HALF_PI = repr(np.pi), repr(np.pi / 2)
YAWS = ("0", HALF_PI, PI, "-" + HALF_PI, "-" + PI, "3.14", "0", "-3.14", PI, "1.57", "-" + PI, "-1.57")          # 0 and +-pi: exact corners


# ------------------------------------------------------------------ the case table
def txt(v):
    """a label field: text as given, a number as the shortest text that parses back to it"""
    return v if isinstance(v, str) else repr(float(v))


def label(kind, i, h, w, l, tx, ty, tz, ry):
    x1, y1 = 10 + (37 * i) % 1100, 100 + (13 * i) % 200
    return " ".join([kind, "0.00", str(i % 3), "-1.57", "%d.00" % x1, "%d.00" % y1, "%d.50" % (x1 + 20 + i % 90), "%d.25" % (y1 + 15 + i % 50)] +
                    [txt(v) for v in (h, w, l, tx, ty, tz, ry)])


def kitti_calib_txt():
    return str(golden("kitti_label")["calib_txt_0"])


def axis_calib_txt():
    rows = kitti_calib_txt().strip().split("\n")
    assert rows[5].startswith("Tr_velo_to_cam: ")
    rows[5] = AXIS_TR
    return "\n".join(rows) + "\n"


def grid_labels():
    ks = [k for k in range(K_LO, K_HI) if k % 5 == 0 or k % 7 == 0]
    lines = []
    for j, k in enumerate(ks):
        for d in (-1, 0, 1):
            side, i = (1 if j % 4 < 2 else -1), len(lines)
            if (j // 3) % 2 == 0:                                # LIDAR x = camera z: corner = f32(tz +- l / 2), w = 0
                ctr, size = place(step(F32(k / 10.0), d), side, 0)
                lines.append(label("Car", i, 1.5, 0, size, F32(((37 * j) % 500) / 10.0 - 25), 1.65, ctr, YAWS[j % 12]))
            else:                                                # LIDAR y = -camera x: corner = f32(-tx +- w / 2), l = 0
                ctr, size = place(step(F32(k / 10.0 - 30.0), d), side, 0)
                lines.append(label("Car", i, 1.5, size, 0, -ctr, 1.65, F32(((53 * j) % 560) / 10.0 + 2), YAWS[j % 12]))
    return "\n".join(lines) + "\n"


def off_map_labels():
    r = np.random.RandomState(702)
    lines = []
    for i in range(48):
        tz = r.uniform(60, 200) if i % 4 == 0 else (r.uniform(-50, 0) if i % 4 == 1 else r.uniform(-20, 90))
        tx = r.uniform(30, 120) if i % 3 == 0 else (r.uniform(-120, -30) if i % 3 == 1 else r.uniform(-50, 50))
        lines.append(label("Car", i, "%.2f" % r.uniform(1.3, 1.9), "%.2f" % r.uniform(1.4, 1.9), "%.2f" % r.uniform(3, 4.8), "%.2f" % tx,
                           "%.2f" % r.uniform(1.2, 2), "%.2f" % tz, "%.2f" % r.uniform(-3.14, 3.14)))
    lines += [label("Car", 48, "1.50", "1.60", "3.90", "0.00", "1.65", "6000.00", "0.3"), label("Car", 49, "1.50", "1.60", "3.90", "-4000.25", "1.65", "-0.05", "-2")]
    return "\n".join(lines) + "\n"


def extent_labels():
    hwl = (("0", "0", "0"), ("1.5", "1.6", "1000000"), ("1.5", "1000000", "3.9"), ("1000000", "1.6", "3.9"), ("1e-42", "1e-42", "1e-42"),
           ("1e30", "1e30", "1e30"), ("-1.5", "-1.6", "-3.9"), ("1.5", "1.6", "1e-42"), ("0", "1.6", "0"))
    lines = []
    for s in hwl:
        for t, ry in ((("10.25", "1.65", "30.5"), "0"), (("-3.7", "1.5", "22.13"), "-1.23"), (("0", "0", "0"), HALF_PI)):
            lines.append(label("Car", len(lines), *s, *t, ry))
    lines.append("Car -1 -1 -10 0.00 0.00 10.00 10.00 -1 -1 -1 -1000 -1000 -1000 -10")            # DontCare's values on a Car
    for ry in ("1000000", "-1000000", "1e300", "1e-300", "-0.0", "6.283185307179586", "100"):
        lines.append(label("Car", len(lines), "1.5", "1.6", "3.9", "4.5", "1.65", "25.05", ry))
    return "\n".join(lines) + "\n"


def nonfinite_labels():
    base = ["1.5", "1.6", "3.9", "4.5", "1.65", "25.05", "0.5"]                  # h w l tx ty tz ry
    lines = []
    for field in range(7):
        for v in ("nan", "inf", "-inf", "1e39"):                                # 1e39 is finite text and an infinite f32
            vals = list(base)
            vals[field] = v
            lines.append(label("Car", len(lines), *vals))
    return "\n".join(lines) + "\n"


def size_labels(G):
    r = np.random.RandomState(800 + G)
    lines, cars = [], 0
    others = ("Van", "DontCare", "Pedestrian", "Misc")
    while cars < G:
        kind = "Car" if r.random_sample() < 0.8 else others[r.randint(4)]
        cars += kind == "Car"
        vals = ["%.2f" % v for v in (r.uniform(1.3, 1.9), r.uniform(1.4, 1.9), r.uniform(3, 4.8), r.uniform(-20, 20), r.uniform(1.2, 2),
                                     r.uniform(4, 58), r.uniform(-3.14, 3.14))]
        if kind == "DontCare":
            vals = ["-1", "-1", "-1", "-1000", "-1000", "-1000", "-10"]
        lines.append(label(kind, len(lines), *vals))
    return "\n".join(lines) + "\n"


_CASES = None


def cases():
    """name -> dict(labels_txt, calib_txt): one frame each; built once"""
    global _CASES
    if _CASES is None:
        kitti, axis, grid = kitti_calib_txt(), axis_calib_txt(), grid_labels()
        out = dict(grid_axis=dict(labels_txt=grid, calib_txt=axis), grid_kitti=dict(labels_txt=grid, calib_txt=kitti),
                   off_map=dict(labels_txt=off_map_labels(), calib_txt=kitti), extents=dict(labels_txt=extent_labels(), calib_txt=kitti),
                   extents_axis=dict(labels_txt=extent_labels(), calib_txt=axis),
                   nonfinite=dict(labels_txt=nonfinite_labels(), calib_txt=kitti), nonfinite_axis=dict(labels_txt=nonfinite_labels(), calib_txt=axis))
        for G in SIZES_G:
            out["sizes_G%d" % G] = dict(labels_txt=size_labels(G), calib_txt=kitti if G != 64 else axis)
        out["sizes_none"] = dict(labels_txt=label("DontCare", 0, "-1", "-1", "-1", "-1000", "-1000", "-1000", "-10") + "\n" +
                                 label("Van", 1, "2.1", "1.9", "5.2", "3.5", "1.7", "20.1", "0.1") + "\n", calib_txt=kitti)
        _CASES = out
    return _CASES


ALL_NAMES = ["grid_axis", "grid_kitti", "off_map", "extents", "extents_axis", "nonfinite", "nonfinite_axis"] + ["sizes_G%d" % G for G in SIZES_G] + \
            ["sizes_none"]


def case_inputs_sha(c):
    return synth.sha256(np.frombuffer(c["labels_txt"].encode(), np.uint8), np.frombuffer(c["calib_txt"].encode(), np.uint8))


def write_tree(root, table, dirs=("ImageSets", "object/training/calib", "object/training/label_2", "object/training/image_2",
                                  "object/training/lidar_bv")):
    """the cases as frames 000000 ... of a KITTI tree (frame i = case i of the table), split `train`"""
    for sub in dirs:
        os.makedirs(os.path.join(root, sub))
    for i, c in enumerate(table.values()):
        idx = "%06d" % i
        with open(os.path.join(root, "object/training/label_2", idx + ".txt"), "w") as f:
            f.write(c["labels_txt"])
        with open(os.path.join(root, "object/training/calib", idx + ".txt"), "w") as f:
            f.write(c["calib_txt"])
        open(os.path.join(root, "object/training/image_2", idx + ".png"), "w").close()
        np.save(os.path.join(root, "object/training/lidar_bv", idx + ".npy"), np.zeros((8, 9, 9), F32))
    with open(os.path.join(root, "ImageSets", "train.txt"), "w") as f:
        f.write("".join("%06d\n" % i for i in range(len(table))))
    return root


def host_inputs(c):
    """(box_cam (G,6) f32 [tx ty tz l w h], ry (G,) f64, Tr (3,4) f32) of a case's cars, parsed from its text"""
    rows = [ln.split(" ") for ln in c["labels_txt"].splitlines() if ln.split(" ")[0] == "Car"]
    with np.errstate(all="ignore"):
        num = np.array([[float(v) for v in t[8:15]] for t in rows], np.float64).reshape(len(rows), 7)
        box = np.ascontiguousarray(num[:, [3, 4, 5, 2, 1, 0]], F32)
    tr = np.array(c["calib_txt"].splitlines()[5].split(" ")[1:], F32).reshape(3, 4)
    return box, num[:, 6].copy(), tr


_MEMO = {}


def described(name, oracle):
    """the oracle's four geometry arrays of a case: computed once, never modified"""
    if name not in _MEMO:
        box, ry, tr = host_inputs(cases()[name])
        with np.errstate(all="ignore"):
            out = oracle.gt_encode(box, ry, tr)
        for a in out:
            a.setflags(write=False)
        _MEMO[name] = out
    return _MEMO[name]


def assert_matches_recording(g, name, key, a, what):
    a = np.asarray(a)
    if "%s__%s" % (name, key) in g.files:
        assert_same(a, g["%s__%s" % (name, key)], "%s: %s of %s against the reference" % (name, key, what))
    else:
        want = g["%s__%s__sha" % (name, key)]
        assert [str(v) for v in want[:2]] == [str(a.dtype), str(a.shape)] and sha_of(a) == str(want[2]), \
            "%s: %s of %s differs from the reference" % (name, key, what)


# ------------------------------------------------------------------ tests that need no GPU
def test_case_table_is_what_the_names_say():
    cs = cases()
    assert list(cs) == ALL_NAMES
    for G in SIZES_G:
        assert host_inputs(cs["sizes_G%d" % G])[0].shape == (G, 6) and WG == 64
        assert len(cs["sizes_G%d" % G]["labels_txt"].splitlines()) > G or G == 1
    assert host_inputs(cs["sizes_none"])[0].shape == (0, 6)
    assert np.array_equal(host_inputs(cs["grid_axis"])[2], np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0]], F32))
    assert cs["grid_axis"]["labels_txt"] == cs["grid_kitti"]["labels_txt"] and cs["grid_axis"]["calib_txt"] != cs["grid_kitti"]["calib_txt"]
    assert "Car -1 -1 -10 0.00 0.00 10.00 10.00 -1 -1 -1 -1000 -1000 -1000 -10" in cs["extents"]["labels_txt"].splitlines()
    box, ry, _ = host_inputs(cs["nonfinite"])
    for col in range(6):                                                  # one non-finite field per object, every field
        others = [k for k in range(6) if k != col]
        assert (~np.isfinite(box[:, col]) & np.isfinite(box[:, others]).all(1) & np.isfinite(ry)).sum() == 4
    assert (~np.isfinite(ry)).sum() == 3 and np.isfinite(box[~np.isfinite(ry)]).all()
    box, ry, _ = host_inputs(cs["off_map"])
    assert (box[:, 2] > 60).sum() >= 5 and (box[:, 2] < 0).sum() >= 5 and (np.abs(box[:, 0]) > 30).sum() >= 10
    yaws = set(ln.split(" ")[14] for ln in cs["grid_axis"]["labels_txt"].splitlines())
    assert yaws == set(YAWS) and repr(float(PI)) == PI


def test_every_case_is_in_the_fixture_or_listed():
    g = golden(FIXTURE)
    assert [str(n) for n in g["case_names"]] == ALL_NAMES
    raised = {}
    for name, c in cases().items():
        assert str(g["%s__inputs_sha" % name]) == case_inputs_sha(c), name
        assert str(g["%s__labels_txt" % name]) == c["labels_txt"] and str(g["%s__calib_txt" % name]) == c["calib_txt"], name
        if "exc__" + name in g.files:
            raised[name] = str(g["exc__" + name])
        else:
            for k in ANN_KEYS + ("calib",):
                assert "%s__%s" % (name, k) in g.files or "%s__%s__sha" % (name, k) in g.files, (name, k)
    assert raised == REFERENCE_RAISES


@pytest.mark.parametrize("name", ALL_NAMES)
def test_oracle_matches_the_recording(oracle, name, tmp_path):
    g = golden(FIXTURE)
    if name in REFERENCE_RAISES:
        assert str(g["exc__" + name]) == REFERENCE_RAISES[name]
        return
    c = cases()[name]
    box, ry, tr = host_inputs(c)
    assert_matches_recording(g, name, "boxes_3D_cam", box, "the parsed text")
    with np.errstate(all="ignore"):
        assert_matches_recording(g, name, "ry", ry.astype(F32), "the parsed text")
    out = described(name, oracle)
    assert [a.shape for a in out] == [(len(box), 24), (len(box), 24), (len(box), 6), (len(box), 4)] and all(a.dtype == F32 for a in out)
    for key, a in zip(GEOMETRY, out):
        assert_matches_recording(g, name, key, a, "the oracle")
    p = tmp_path / "calib.txt"
    p.write_text(c["calib_txt"])
    table = pack_calib(load_kitti_calib(str(p)))
    assert_matches_recording(g, name, "calib", table, "pack_calib")
    assert same(table[3].reshape(3, 4).astype(F32), tr)


def bev_corners(b3):
    """(x1, y1, x2, y2) f32 of lidar_3d_to_bv from the LIDAR boxes: the f32 sums whose f64 copies are divided"""
    b3 = np.asarray(b3, F32)
    with np.errstate(all="ignore"):
        return (b3[:, 0] + b3[:, 3] * F32(0.5), b3[:, 1] + b3[:, 4] * F32(0.5), b3[:, 0] - b3[:, 3] * F32(0.5), b3[:, 1] - b3[:, 4] * F32(0.5))


def test_cases_reach_the_cell_edges(oracle):
    """the four BEV numerators of the table sit on / just below / just above cell edges at least 50 times each, at every edge of
    the map and its margin that the table names; negative numerators occur; on multiples of 0.5 m numpy's floor-division is not
    floor(a / 0.1)"""
    x_edges = {float(F32(k / 10.0)): k for k in range(K_LO, K_HI)}
    y_edges = {float(F32(k / 10.0 - 30.0)): k for k in range(K_LO, K_HI)}
    hits = {"on": set(), "below": set(), "above": set()}
    n_hits = {"on": [0, 0], "below": [0, 0], "above": [0, 0]}
    negative = differs = 0
    for name in ALL_NAMES:
        _, _, b3, bv = described(name, oracle)
        x1, y1, x2, y2 = bev_corners(b3)
        with np.errstate(all="ignore"):
            for col, (v, origin, n) in enumerate(((y1, -30.0, 600.0), (x1, 0.0, 600.0), (y2, -30.0, 600.0), (x2, 0.0, 600.0))):
                a = v.astype(np.float64) - origin
                q = np.floor_divide(a, 0.1)
                assert same((n - q).astype(F32), bv[:, col]), (name, col)          # numpy's own f64 floor-division gives the oracle's pixels
                negative += int((a < 0).sum())
                differs += int((np.isfinite(a) & (q != np.floor(a / 0.1))).sum())
        if name == "grid_axis":
            for axis, (edges, vals) in enumerate(((x_edges, np.concatenate([x1, x2])), (y_edges, np.concatenate([y1, y2])))):
                for tag, d in (("on", 0), ("below", 1), ("above", -1)):  # below an edge: the f32 neighbour above is the edge
                    moved = vals if d == 0 else np.nextafter(vals, F32(d * np.inf))
                    for v in moved:
                        if float(v) in edges:
                            hits[tag].add(edges[float(v)])
                            n_hits[tag][axis] += 1
    named = set(k for k in range(K_LO, K_HI) if k % 5 == 0 or k % 7 == 0)
    for tag in hits:
        assert sum(n_hits[tag]) >= 50 and min(n_hits[tag]) >= 10, (tag, n_hits[tag])
        assert min(hits[tag]) <= K_LO + 3 and max(hits[tag]) >= K_HI - 4 and len(hits[tag] & named) >= 50, (tag, sorted(hits[tag]))
    assert negative >= 50 and differs >= 10, (negative, differs)


def test_special_values_reach_the_outputs(oracle):
    cam, lid, b3, bv = described("nonfinite", oracle)
    assert np.isnan(bv).any() and np.isnan(cam).any() and np.isinf(cam).any() and np.isinf(b3[:, 3:]).any()
    # one non-finite coordinate poisons the whole object (0 * inf in the matrix products); a yaw of 1e39 is a finite f64
    assert np.isnan(bv).all(1).sum() >= 20 and np.isfinite(bv).all(1).sum() == 1
    cam, lid, b3, bv = described("extents", oracle)
    assert np.isfinite(bv).all() and np.abs(bv).max() > 1e6 and bv.min() < 0
    zero = np.where(~b3[:, 3:].any(1))[0]
    assert len(zero) and np.array_equal(bv[zero, :2], bv[zero, 2:])
    cam, lid, b3, bv = described("off_map", oracle)
    assert (bv < 0).any() and (bv > 600).any()


# ------------------------------------------------------------------ the device
SENTINEL = 0xC0DEFACE


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import _lib, ops
    return dict(torch=torch, ops=ops, lib=_lib)


@pytest.fixture(scope="module")
def roidb(gpu, tmp_path_factory):
    """the loader's roidb of the cases' KITTI tree, read once"""
    from mv3d_tf_amd.datasets import kitti_mv3d
    root = write_tree(str(tmp_path_factory.mktemp("gt_edges") / "KITTI"), cases())
    db = kitti_mv3d("train", root)
    with np.errstate(all="ignore"):
        return db, db.gt_roidb()


def value_of(ann, key):
    return ann[key].toarray() if key == "gt_overlaps" else np.asarray(ann[key])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_NAMES)
def test_loader_on_the_device(gpu, roidb, oracle, name):
    from mv3d_tf_amd.datasets import parse_kitti_labels
    db, entries = roidb
    i = ALL_NAMES.index(name)
    c, g = cases()[name], golden(FIXTURE)
    with np.errstate(all="ignore"):
        direct = parse_kitti_labels(c["labels_txt"].splitlines(True), host_inputs(c)[2], {"__background__": 0, "Car": 1}, 2)
    for what, ann in (("gt_roidb", entries[i]), ("parse_kitti_labels", direct)):
        assert set(ann) == set(ANN_KEYS) and ann["flipped"] is False
        for key, want in zip(GEOMETRY, described(name, oracle)):
            assert_same(ann[key], want, "%s: %s of %s against the oracle" % (name, key, what))
        if name not in REFERENCE_RAISES:
            for key in ANN_KEYS:
                assert_matches_recording(g, name, key, value_of(ann, key), what)
    if name not in REFERENCE_RAISES:
        assert_matches_recording(g, name, "calib", db.calib_at(i), "calib_at")


def guarded(torch, rows, width):
    return torch.full(((rows + WG) * width,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda").view(torch.float32).view(rows + WG, width)


def words(t):
    return t.cpu().numpy().view(np.uint32)


def raw_encode(gpu, box, ry, tr, G=None, missing=None):
    """mv3d_gt_encode through ctypes into outputs 64 objects longer than needed -> (status, the four buffers)"""
    torch, P = gpu["torch"], gpu["ops"]._ptr
    G = len(box) if G is None else G
    with np.errstate(all="ignore"):
        cs = np.ascontiguousarray(np.stack([np.cos(ry), np.sin(ry)], 1), np.float64).reshape(-1, 2)
        inv = np.ascontiguousarray(np.linalg.inv(tr[:, :3]), F32)
    ins = [torch.as_tensor(np.array(a, order="C")).cuda() for a in (box, cs, inv.reshape(-1), tr.reshape(-1))]
    outs = [guarded(torch, max(G, 0), w) for w in (24, 24, 6, 4)]
    args = [ins[0], ins[1], ins[2], ins[3]] + outs
    if missing is not None:
        args[missing] = None
    rc = gpu["lib"].lib().mv3d_gt_encode(P(args[0]), P(args[1]), G, *[P(a) for a in args[2:]], gpu["ops"]._stream())
    torch.cuda.synchronize()
    return rc, outs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_NAMES)
def test_gt_encode_entry_on_the_device(gpu, oracle, name):
    box, ry, tr = host_inputs(cases()[name])
    G = len(box)
    rc, outs = raw_encode(gpu, box, ry, tr)
    assert rc == gpu["lib"].OK
    for o in outs:
        assert (words(o[G:]) == SENTINEL).all(), "%s: objects beyond G were written" % name
    g = golden(FIXTURE)
    for key, o, want in zip(GEOMETRY, outs, described(name, oracle)):
        got = o[:G].cpu().numpy()
        assert_same(got, want, "%s: %s of the device against the oracle" % (name, key))
        if name not in REFERENCE_RAISES:
            assert_matches_recording(g, name, key, got, "the device")


@pytest.mark.gpu
def test_empty_and_refused_calls_write_nothing(gpu):
    lib = gpu["lib"]
    box, ry, tr = host_inputs(cases()["sizes_G1"])
    rc, outs = raw_encode(gpu, box, ry, tr, G=0)
    assert rc == lib.OK and all((words(o) == SENTINEL).all() for o in outs)
    assert lib.lib().mv3d_gt_encode(None, None, 0, None, None, None, None, None, None, gpu["ops"]._stream()) == lib.OK
    rc, outs = raw_encode(gpu, box, ry, tr, G=-1)
    assert rc == lib.ERR_INVALID_ARG and all((words(o) == SENTINEL).all() for o in outs)
    for missing in range(8):                                              # every pointer, one at a time
        rc, outs = raw_encode(gpu, box, ry, tr, missing=missing)
        assert rc == lib.ERR_INVALID_ARG, missing
        assert all((words(o) == SENTINEL).all() for o in outs), missing
