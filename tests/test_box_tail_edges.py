"""The test-time tail of box_detect at its edges: `mv3d_box_detect_tail` (csrc/box_tail.hip), which restates
lib/fast_rcnn/test_mv.py:240-261 = lidar_3d_to_corners, bbox_transform_inv_cnr and corners_to_bv.

One case table (`cases`) feeds three descriptions of the same thing:
  1. a recording of the reference's three functions (tests/golden/box_tail_edges.npz, written by
     tests/golden/make_box_tail_edge_golden.py, which imports this table),
  2. the CPU oracle (oracle.box_tail),
  3. the device, under `-m gpu`.
Every comparison is on bit patterns (f32 as u32, f64 as u64), except that any NaN matches any NaN.  No tolerances.

corners_to_bv is the one place where numpy's f32 floor-division (npy_divmodf) runs on the device; `divmodf_branches` restates
its branches and `test_cases_reach_the_floor_division_branches` counts how often the table's numerators take each.  With
b = f32(0.1) = 13421773 * 2^-27 (an odd mantissa) a numerator a = k * b is an f32 only when k * 13421773 fits 24 bits, that is
for k = 0 and the powers of two, so `fmodf(a, b) == 0` is rare.  A cell edge in f32 is the rounded product f32(k) * f32(0.1):
"on" a multiple means equal to that product, "below" / "above" one ulp either side of it.  On the y axis the numerator is
f32(corner + 30); where that sum cannot give the wanted value (small k: the sum is exact on the corner's coarser grid) the row
gets an ordinary y instead, so the y axis contributes fewer exact hits than the x axis.
All of npy_divmodf's branches are reachable with this b and are asserted: `mod != 0` with differing signs (every negative
numerator that is no multiple), `div - floor(div) > 0.5` (a numerator just below k * b whose (a - mod) / b rounds below the
integer), `div == 0` with a / b positive (0 <= a < b) and negative (a = -0.0 only: a negative non-zero a takes the sign branch
and leaves with div = -1), and a NaN `mod` (infinite or NaN numerator).
"""

import numpy as np
import pytest

from conftest import golden
from mv3d_tf_amd import synth

FIXTURE = "box_tail_edges"
F32 = np.float32
RES32 = F32(0.1)
WG = 128                          # rows per workgroup of box_tail_kernel
RECORD_ARRAY_BYTES = 65536        # larger outputs are stored as `sha_of`
FIELDS = ("corners", "pred_cnr_r", "pred_bv", "pred_bv_r")

# Cases the reference itself cannot run: name -> the exception type it raised (recorded in the fixture under exc__<name>).
REFERENCE_RAISES = {}

K_LO, K_HI = -8, 609              # cells -8 .. 608: the 0 .. 600 map and a margin of 8 either side
SIZES_R = (0, 1, 127, 128, 129)
SERVE_FRAMES, SERVE_ROWS, SERVE_REAL = 3, 100, (100, 37, 0)


# ------------------------------------------------------------------ the case table
def step(v, d):
    """v, or its f32 neighbour below (d = -1) / above (d = +1)"""
    v = F32(v)
    return v if d == 0 else np.nextafter(v, F32(d * np.inf))


def _near(v, n=3):
    out, lo, hi = [F32(v)], F32(v), F32(v)
    for _ in range(n):
        lo, hi = step(lo, -1), step(hi, 1)
        out += [lo, hi]
    return out


HALVES = tuple(F32(2.0 ** e) for e in range(1, -12, -1)) + (F32(0),)


def place(target, side, origin):
    """(centre, size) f32 of an extent whose upper (side > 0) or lower corner c = f32(+-size / 2 + centre) makes the
    floor-division's numerator f32(c - origin) equal to `target`; None where no f32 corner gives it."""
    target, origin = F32(target), F32(origin)
    wanted = [c for c in _near(target + origin) if F32(c - origin) == target]
    for half in HALVES:
        s = half if side > 0 else -half
        for c in wanted:
            for ctr in _near(c - s):
                if F32(s + ctr) == c:
                    return ctr, F32(half * 2)
    return None


def ordinary(r, R):
    """boxes as the product meets them (the shape of box_tail.npz), with a zero batch column"""
    b = np.stack([np.zeros(R), r.uniform(0, 60, R), r.uniform(-30, 30, R), r.uniform(-1.5, 0, R), r.uniform(1, 5, R),
                  r.uniform(0.5, 2, R), r.uniform(1, 2, R)], 1)
    return b.astype(F32).reshape(R, 7)


def cell_case(nc):
    ks = [k for k in range(K_LO, K_HI) if k % 4 == nc - 1 or k < K_LO + 17 or k >= K_HI - 17]
    r = np.random.RandomState(100 + nc)
    rows = []
    for i in range(3 * len(ks)):
        kx, ky, d, side = ks[i // 3], ks[len(ks) - 1 - i // 3], i % 3 - 1, 1 if (i // 3) % 2 else -1
        x, l = place(step(F32(kx) * RES32, d), side, 0)
        py = place(step(F32(ky) * RES32, d), -side, -30)
        y, w = py if py is not None else (F32(ky * 0.1 - 30 + 0.05), F32(1.6))
        rows.append([0, x, y, -1, l, w, 1.5])
    rois = np.array(rows, F32)
    return dict(rois_3d=rois, deltas=r.uniform(-0.05, 0.05, (len(rois), 24 * nc)).astype(F32), nc=nc)


def off_map_case():
    tiny, norm = F32(1e-45), F32(1.2e-38)
    xs = [0.0, -0.0, tiny, -tiny, norm, -norm, -0.05, -RES32, -0.25, -1, -7.3, -29.95, -100.05, -1e4, -1e6, 0.05, 59.95, 60, 60.05,
          61, 100, 1e3, 1e5, 1e7, step(RES32, -1), step(-RES32, 1), step(-RES32, -1), 2.0, -2.0, 0.8]
    ys = [-30, step(-30, 1), step(-30, -1), -30.05, -31, -100, -1e4, -29.95, 29.95, 30, 30.05, 31, 1e3, 1e6, 0.0, -0.0]
    sizes = ((0, 0, 0), (4, 1.6, 1.5), (0.5, 0.25, 1))
    rows = [[0, x, y, -1] + list(sizes[(i + j) % 3]) for i, x in enumerate(xs) for j, y in enumerate(ys)]
    r = np.random.RandomState(201)
    return dict(rois_3d=np.array(rows, F32), deltas=r.uniform(-0.2, 0.2, (len(rows), 48)).astype(F32), nc=2)


def wild_case():
    r = np.random.RandomState(301)
    R, nan, inf = 400, np.nan, np.inf
    rois = ordinary(r, R)
    # magnitudes 1e-3 ... 1e38 in row order: with diagonals of a few metres the products overflow from about 6e37 on
    mag = 10.0 ** (-3 + 41 * (np.arange(R)[:, None] + r.uniform(0, 1, (R, 48))) / R)
    deltas = (np.minimum(mag, 3.4e38) * r.choice([-1.0, 1.0], (R, 48))).astype(F32)
    for i in range(72):              # one non-finite delta per row: class i % 2, axis i % 3 (x, y, z), corner i % 8
        deltas[i, 24 * (i % 2) + 8 * (i % 3) + i % 8] = (inf, -inf, nan)[(i // 6) % 3]
    special = [(0, 0, 0), (1e30, 1.6, 1.5), (4, 1e30, 1.5), (4, 1.6, 1e30), (1e30, 1e30, 1e30), (1e-42, 1e-42, 1e-42), (1e-42, 1.6, 1e-42),
               (-4, -1.6, -1.5), (-4, 1.6, 1.5), (4, -1.6, 1.5), (nan, 1.6, 1.5), (4, nan, 1.5), (4, 1.6, nan), (inf, 1.6, 1.5),
               (4, inf, 1.5), (4, 1.6, inf), (3e38, 3e38, 3e38), (2e19, 2e19, 1.5)]
    row = 80
    for s in special:                # every special size with small, zero, huge and non-finite deltas
        for v in range(6):
            rois[row, 4:7] = s
            if v == 1:
                rois[row, 1:4] = 0
            if v == 2:
                deltas[row] = r.uniform(-0.2, 0.2, 48)
            if v == 3:
                deltas[row, ::5] = 0
            if v == 4:
                deltas[row, 3::7] = (inf, -inf, nan, inf, -inf, nan, inf)
            if v == 5:
                deltas[row] = r.uniform(-0.2, 0.2, 48)
                deltas[row, [1, 9, 17, 25, 33, 41]] = (inf, -inf, nan, nan, inf, -inf)
            row += 1
    for axis in range(3):            # a non-finite centre on one axis only, with ordinary and with wild deltas
        for v in (nan, inf, -inf, 3e38, -3e38):
            for wild in (False, True):
                rois[row, 1 + axis] = v
                if not wild:
                    deltas[row] = r.uniform(-0.2, 0.2, 48)
                row += 1
    assert row <= R
    return dict(rois_3d=rois, deltas=deltas, nc=2)


def huge_case():
    r = np.random.RandomState(401)
    R = 300
    rois = ordinary(r, R)
    v = (10.0 ** np.linspace(3, np.log10(3e38), R) * np.where(np.arange(R) % 4 < 2, 1, -1)).astype(F32)
    v[-4:] = [np.finfo(F32).max, -np.finfo(F32).max, F32(2.0 ** 24) * RES32, F32(2.0 ** 100)]
    rois[0::2, 1], rois[1::2, 2] = v[0::2], v[1::2]
    rois[0::3, 4:7] = 0
    return dict(rois_3d=rois, deltas=r.uniform(-0.2, 0.2, (R, 72)).astype(F32), nc=3)


def serve_case():
    """what ServeGraph feeds: frames of SERVE_ROWS rows, the rows behind a frame's proposal count all-zero ROIs, the head's
    deltas there whatever it computed"""
    r = np.random.RandomState(601)
    rois = np.zeros((SERVE_FRAMES * SERVE_ROWS, 7), F32)
    for f, n in enumerate(SERVE_REAL):
        rois[f * SERVE_ROWS:f * SERVE_ROWS + n] = ordinary(r, n)
        rois[f * SERVE_ROWS:f * SERVE_ROWS + n, 0] = f
    return dict(rois_3d=rois, deltas=r.uniform(-2, 2, (len(rois), 48)).astype(F32), nc=2)


_CASES = None


def cases():
    """name -> dict(rois_3d (R,7) f32, deltas (R,24*nc) f32, nc); built once, read-only"""
    global _CASES
    if _CASES is None:
        with np.errstate(all="ignore"):
            out = {"cells_nc%d" % nc: cell_case(nc) for nc in (1, 2, 3, 4)}
            out.update(off_map=off_map_case(), wild=wild_case(), huge_quotient=huge_case())
            for R in SIZES_R:
                r = np.random.RandomState(500 + R)
                out["sizes_R%d" % R] = dict(rois_3d=ordinary(r, R), deltas=r.uniform(-0.2, 0.2, (R, 48)).astype(F32), nc=2)
            out["serve_padding"] = serve_case()
        for c in out.values():
            assert c["rois_3d"].dtype == F32 and c["deltas"].dtype == F32 and c["rois_3d"].shape[0] <= 600
            assert c["deltas"].shape == (c["rois_3d"].shape[0], 24 * c["nc"])
            c["rois_3d"].setflags(write=False)
            c["deltas"].setflags(write=False)
        _CASES = out
    return _CASES


ALL_NAMES = ["cells_nc%d" % nc for nc in (1, 2, 3, 4)] + ["off_map", "wild", "huge_quotient"] + ["sizes_R%d" % R for R in SIZES_R] + \
            ["serve_padding"]


def case_inputs_sha(c):
    return synth.sha256(c["rois_3d"], c["deltas"], np.int32(c["nc"]))


# ------------------------------------------------------------------ comparing
def bits(a):
    """the array's bit patterns, every NaN replaced by one pattern"""
    a = np.asarray(a)
    a = a if a.flags.c_contiguous else np.ascontiguousarray(a)
    u = a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()
    if a.dtype.kind == "f":
        u[np.isnan(a)] = np.iinfo(u.dtype).max
    return u


def sha_of(a):
    """what the fixture stores of an output above RECORD_ARRAY_BYTES: the hash of its bit patterns, NaNs made one"""
    return synth.sha256(bits(a))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert not len(bad), "%s: %d entries differ, first at %s: %r against %r" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])],
                                                                               want[tuple(bad[0])])


_MEMO = {}


def described(name, oracle):
    """the oracle's (corners, pred_cnr_r, pred_bv f64, pred_bv_r f64) of a case: computed once, never modified"""
    if name not in _MEMO:
        c = cases()[name]
        cnr, _, pr, bv, bvr = oracle.box_tail(c["rois_3d"], c["deltas"], c["nc"])
        out = (cnr, pr, bv, bvr)
        for a in out:
            a.setflags(write=False)
        _MEMO[name] = out
    return _MEMO[name]


def assert_matches_recording(g, name, out, what):
    for f, a in zip(FIELDS, out):
        a = np.ascontiguousarray(a)
        if "%s__%s" % (name, f) in g.files:
            assert_same(a, g["%s__%s" % (name, f)], "%s: %s of %s against the reference" % (name, f, what))
        else:
            assert sha_of(a) == str(g["%s__%s__sha" % (name, f)]), "%s: %s of %s differs from the reference" % (name, f, what)


# ------------------------------------------------------------------ npy_divmodf, restated to count its branches
def numerators(nc, cnr, pr):
    """every numerator corners_to_bv divides for a case, (xmax, xmin, ymax, ymin) blocks of R: the min / max of the plain and of
    each class's regressed corners' x, and of their y minus f32(-30)"""
    with np.errstate(all="ignore"):
        sets = [cnr] + [pr[:, 24 * k:24 * k + 24] for k in range(nc)]
        out = []
        for s in sets:
            out += [s[:, :8].max(1), s[:, :8].min(1), s[:, 8:16].max(1) - F32(-30), s[:, 8:16].min(1) - F32(-30)]
    return np.concatenate(out).astype(F32)


def divmodf_branches(a, b=RES32):
    """numpy/core/src/npymath/npy_math_internal.h.src: npy_divmod@c@ on f32, branch by branch.  Returns (floor-division, flags)."""
    a = np.asarray(a, F32)
    with np.errstate(all="ignore"):
        mod = np.fmod(a, b)
        div = ((a - mod) / b).astype(F32)
        signs = (mod != 0) & ((b < 0) != (mod < 0))
        div = np.where(signs, div - F32(1), div).astype(F32)
        fl = np.floor(div)
        up = (div != 0) & (div - fl > F32(0.5))
        zero = div == 0
        q = (a / b).astype(F32)
        fd = np.where(zero, np.copysign(F32(0), q), np.where(up, fl + F32(1), fl)).astype(F32)
    return fd, dict(signs_differ=signs, rounds_up=up, zero_pos=zero & ~np.signbit(q), zero_neg=zero & np.signbit(q), mod_nan=np.isnan(mod),
                    mod_zero=(mod == 0) & (a != 0))


# ------------------------------------------------------------------ tests that need no GPU
def test_case_table_is_what_the_names_say():
    cs = cases()
    assert list(cs) == ALL_NAMES
    assert [cs["cells_nc%d" % n]["nc"] for n in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert [cs["sizes_R%d" % R]["rois_3d"].shape[0] for R in SIZES_R] == list(SIZES_R) and WG == 128
    sp = cs["serve_padding"]["rois_3d"].reshape(SERVE_FRAMES, SERVE_ROWS, 7)
    for f, n in enumerate(SERVE_REAL):
        assert not sp[f, n:].any() and (n == 0 or sp[f, :n, 4:].all())
    assert cs["serve_padding"]["deltas"].all()
    w = cs["wild"]
    assert np.isnan(w["deltas"]).any() and np.isinf(w["deltas"]).any() and np.abs(w["deltas"][np.isfinite(w["deltas"])]).max() > 1e37
    for axis in (1, 2, 3):           # a centre that is non-finite on this axis only
        others = [a for a in (1, 2, 3) if a != axis]
        assert (~np.isfinite(w["rois_3d"][:, axis]) & np.isfinite(w["rois_3d"][:, others]).all(1)).sum() >= 6
    assert np.abs(cs["huge_quotient"]["rois_3d"][:, 1:3]).max() == np.finfo(F32).max


def test_every_case_is_in_the_fixture_or_listed():
    g = golden(FIXTURE)
    assert [str(n) for n in g["case_names"]] == ALL_NAMES
    raised = {}
    for name, c in cases().items():
        assert str(g["%s__inputs_sha" % name]) == case_inputs_sha(c), name
        if "exc__" + name in g.files:
            raised[name] = str(g["exc__" + name])
        else:
            for f in FIELDS:
                assert "%s__%s" % (name, f) in g.files or "%s__%s__sha" % (name, f) in g.files, (name, f)
    assert raised == REFERENCE_RAISES


@pytest.mark.parametrize("name", ALL_NAMES)
def test_oracle_matches_the_recording(oracle, name):
    g = golden(FIXTURE)
    if name in REFERENCE_RAISES:
        assert str(g["exc__" + name]) == REFERENCE_RAISES[name]
        return
    c = cases()[name]
    out = described(name, oracle)
    R, nc = c["rois_3d"].shape[0], c["nc"]
    assert [a.shape for a in out] == [(R, 24), (R, 24 * nc), (R, 4 * nc), (R, 4 * nc)]
    assert [a.dtype for a in out] == [F32, F32, np.float64, np.float64]
    assert_matches_recording(g, name, out, "the oracle")


def test_cases_reach_the_floor_division_branches(oracle):
    """the table's numerators take every branch of npy_divmodf, and sit on / one ulp below / one ulp above cell edges"""
    cs = cases()
    count = dict(signs_differ=0, rounds_up=0, zero_pos=0, zero_neg=0, mod_nan=0, mod_zero=0)
    edges = {float(F32(k) * RES32): k for k in range(K_LO, K_HI)}
    hits = {"on": {}, "below": {}, "above": {}}
    y_hits = 0
    for name in ALL_NAMES:
        out = described(name, oracle)
        a = numerators(cs[name]["nc"], out[0], out[1])
        fd, flags = divmodf_branches(a)
        for k, v in flags.items():
            count[k] += int(v.sum())
        # the restatement is the oracle's arithmetic: Xn - fd = 600 - fd is what the oracle put out
        R, nc = cs[name]["rois_3d"].shape[0], cs[name]["nc"]
        want = np.concatenate([out[2][:, 1], out[2][:, 3], out[2][:, 0], out[2][:, 2]] +
                              [out[3][:, 4 * k + j] for k in range(nc) for j in (1, 3, 0, 2)]) if R else np.zeros(0)
        assert same((F32(600) - fd).astype(np.float64), want), name
        if name.startswith("cells"):
            plain = a[:4 * R]
            for tag, d in (("on", 0), ("below", 1), ("above", -1)):      # a is below an edge when its neighbour above is the edge
                moved = plain if d == 0 else np.nextafter(plain, F32(d * np.inf))
                for i, v in enumerate(moved):
                    if float(v) in edges:
                        hits[tag][edges[float(v)]] = hits[tag].get(edges[float(v)], 0) + 1
                        y_hits += int(i >= 2 * R)
    assert all(v > 0 for v in count.values()), count
    for tag in hits:
        n = sum(hits[tag].values())
        assert n >= 50, (tag, n)
        assert set(range(K_LO, K_HI)) == set(hits[tag]), (tag, sorted(set(range(K_LO, K_HI)) - set(hits[tag])))      # every cell of the map and margin
    assert y_hits >= 50


def test_wild_case_poisons_each_axis_alone(oracle):
    """min / max with a NaN is NaN per axis: rows whose BEV x pair is NaN and y pair is not, and the other way round, and rows with
    NaN only among the z corners (BEV untouched)"""
    cnr, pr, bv, bvr = described("wild", oracle)
    b, p = bvr.reshape(-1, 4), pr.reshape(-1, 24)                         # one row per (ROI, class)
    nx, ny = np.isnan(b[:, [1, 3]]).all(1), np.isnan(b[:, [0, 2]]).all(1)
    assert (nx & ~ny).sum() >= 5 and (ny & ~nx).sum() >= 5 and (nx & ny).sum() >= 5
    assert (np.isnan(p[:, :8]).any(1) & ~np.isnan(p[:, :8]).all(1)).sum() >= 5      # one NaN among finite x corners poisons the pair
    nz = np.isnan(p[:, 16:24]).any(1) & ~np.isnan(p[:, :16]).any(1)
    assert (nz & ~np.isnan(b).any(1)).sum() >= 5
    assert np.isinf(bvr).any() and np.isinf(described("huge_quotient", oracle)[2]).any()
    z = cases()["wild"]["rois_3d"]
    zero = np.where(~z[:, 4:7].any(1))[0]
    assert len(zero) and np.isnan(pr[zero]).any()                         # inf * (diag = 0)


# ------------------------------------------------------------------ the device
SENTINEL = 0xC0DEFACE             # a bit pattern no output takes (as f32: -6.9677...; the outputs here are corners in metres or pixels)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import _lib, ops
    return dict(torch=torch, ops=ops, lib=_lib)


def dev(torch, a):
    return torch.as_tensor(np.array(a, order="C")).cuda()                 # a copy: the table's arrays are read-only


def guarded(torch, rows, width):
    """(rows + WG, width) f32 on the device, every word the sentinel"""
    return torch.full(((rows + WG) * width,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda").view(torch.float32).view(rows + WG, width)


def words(t):
    return t.cpu().numpy().view(np.uint32)


def raw_tail(gpu, rois, deltas, nc, R=None):
    """mv3d_box_detect_tail through ctypes into guarded buffers -> (status, the four buffers)"""
    torch, P = gpu["torch"], gpu["ops"]._ptr
    R = rois.shape[0] if R is None else R
    outs = [guarded(torch, max(R, 0), w) for w in (24, 24 * max(nc, 1), 4 * max(nc, 1), 4 * max(nc, 1))]
    d_r, d_d = dev(torch, rois), dev(torch, deltas)
    rc = gpu["lib"].lib().mv3d_box_detect_tail(P(d_r), P(d_d), R, nc, *[P(o) for o in outs], gpu["ops"]._stream())
    torch.cuda.synchronize()
    return rc, outs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_NAMES)
def test_box_detect_tail_on_the_device(gpu, oracle, name):
    c = cases()[name]
    R, nc = c["rois_3d"].shape[0], c["nc"]
    rc, outs = raw_tail(gpu, c["rois_3d"], c["deltas"], nc)
    assert rc == gpu["lib"].OK
    for o in outs:
        assert (words(o[R:]) == SENTINEL).all(), "%s: rows beyond R were written" % name
    got = [o[:R].cpu().numpy() for o in outs]
    got = (got[0], got[1], got[2].astype(np.float64), got[3].astype(np.float64))
    for f, a, w in zip(FIELDS, got, described(name, oracle)):
        assert_same(a, w, "%s: %s of the device against the oracle" % (name, f))
    if name not in REFERENCE_RAISES:
        assert_matches_recording(golden(FIXTURE), name, got, "the device")


@pytest.mark.gpu
def test_ops_and_box_detect_return_the_same_arrays(gpu, oracle, monkeypatch):
    """ops.box_detect_tail allocates and returns what the raw entry wrote; test_mv.box_detect adds the f64 cast of pred_bv and
    the n_classes copies of the corners"""
    torch, ops = gpu["torch"], gpu["ops"]
    from mv3d_tf_amd.fast_rcnn import test_mv
    c = cases()["off_map"]
    R, nc = c["rois_3d"].shape[0], c["nc"]
    assert nc == test_mv.n_classes
    want = described("off_map", oracle)
    got = [t.cpu().numpy() for t in ops.box_detect_tail(dev(torch, c["rois_3d"]), dev(torch, c["deltas"]), nc)]
    for f, a, w in zip(FIELDS, got, want):
        assert_same(a, w.astype(F32), "ops.box_detect_tail: " + f)
    scores = np.random.RandomState(3).random_sample((R, nc)).astype(F32)

    class Net:
        def forward(self, feed):
            assert feed["image_data"].dtype == F32 and feed["lidar_bv_data"].shape == (1, 16, 24, 9)
            return {"rois": (None, None, dev(torch, c["rois_3d"])), "cls_prob": dev(torch, scores), "bbox_pred": dev(torch, c["deltas"])}

    sc, bv, cnr, pr = test_mv.box_detect(None, Net(), np.zeros((8, 12, 3), np.uint8), np.zeros((16, 24, 9), F32), np.zeros((4, 12)))
    assert_same(sc, scores, "box_detect: scores")
    assert_same(bv, want[2], "box_detect: pred_boxes_bv")
    assert_same(cnr, np.hstack([want[0]] * nc), "box_detect: pred_boxes_cnr")
    assert_same(pr, want[1], "box_detect: pred_boxes_cnr_r")
    g = golden(FIXTURE)
    if "off_map__pred_bv" in g.files:
        assert_same(bv, g["off_map__pred_bv"], "box_detect: pred_boxes_bv against the reference")


@pytest.mark.gpu
def test_empty_and_refused_calls_write_nothing(gpu):
    torch, lib, P = gpu["torch"], gpu["lib"], gpu["ops"]._ptr
    c = cases()["sizes_R1"]
    rc, outs = raw_tail(gpu, c["rois_3d"], c["deltas"], 2, R=0)           # R = 0 with valid pointers
    assert rc == lib.OK and all((words(o) == SENTINEL).all() for o in outs)
    assert lib.lib().mv3d_box_detect_tail(None, None, 0, 2, None, None, None, None, gpu["ops"]._stream()) == lib.OK
    for nc in (0, -1):
        rc, outs = raw_tail(gpu, c["rois_3d"], c["deltas"], nc)
        assert rc == lib.ERR_INVALID_ARG and all((words(o) == SENTINEL).all() for o in outs)
    rc, outs = raw_tail(gpu, c["rois_3d"], c["deltas"], 2, R=-1)
    assert rc == lib.ERR_INVALID_ARG and all((words(o) == SENTINEL).all() for o in outs)
    d_r, d_d = dev(torch, c["rois_3d"]), dev(torch, c["deltas"])
    outs = [guarded(torch, 1, w) for w in (24, 48, 8, 8)]
    for missing in range(6):                                              # every pointer, one at a time
        args = [d_r, d_d] + outs
        args[missing] = None
        rc = lib.lib().mv3d_box_detect_tail(P(args[0]), P(args[1]), 1, 2, *[P(a) for a in args[2:]], gpu["ops"]._stream())
        torch.cuda.synchronize()
        assert rc == lib.ERR_INVALID_ARG, missing
        assert all((words(o) == SENTINEL).all() for o in outs), missing


@pytest.mark.gpu
def test_wild_tail_through_detect_post(gpu, oracle):
    """the NaN / inf BEV boxes the tail really produces, through the cut / NMS / cap of mv3d_detect_post, against
    oracle.test_net_frame on the same arrays"""
    import test_detect_post as DP
    torch, ops = gpu["torch"], gpu["ops"]
    c = cases()["wild"]
    R, K = c["rois_3d"].shape[0], c["nc"]
    cnr, pr, bv, _ = [t.cpu().numpy() for t in ops.box_detect_tail(dev(torch, c["rois_3d"]), dev(torch, c["deltas"]), K)]
    want = described("wild", oracle)
    assert_same(bv, want[2].astype(F32), "pred_bv")
    assert_same(cnr, want[0], "corners")
    assert np.isnan(bv).any() and np.isinf(bv).any()
    scores = np.random.RandomState(77).random_sample((R, K)).astype(F32)
    scores[:, 0] = 1 - scores[:, 1:].max(1)
    arrays = (scores, bv, cnr, pr)
    for mpi in (0, 50):
        got = DP.run(ops, torch, arrays, None, K, R, mpi, 0.1)
        totals = DP.compare(oracle, got, arrays, None, K, R, mpi, 0.1, equal_nan=True)
        assert totals[0] > 0
