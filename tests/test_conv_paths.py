"""Every tile path of the trunks' convolutions (csrc/conv3x3_mfma.hip, conv3x3_wgrad.hip, conv_input.hip), each at the shapes that
select it, against a float64 reference that cannot share the kernels' bugs.

The host code picks a kernel by the launch's tile count.  `select_path` below restates those rules and constants; every case of the
table names the path it is meant to reach and asserts that the restatement sends it there.  The library answers for itself:
`mv3d_conv3x3_path` (host only) returns the selection the launch entries call, and `test_the_library_selects_what_the_rules_say`
(no GPU) compares it with the restatement for every case and from both sides of every threshold, so that a retuned threshold cannot
silently move a case to another path; every GPU case asks it again before it launches.  Only the weight gradient's constants, whose
plan depends on the device, are still read out of its .hip source (`test_selection_constants_match_the_sources`).

Two kinds of operands:
  * exact integers: x in {0..7} (non-negative, as after a ReLU), w in {-1..3} (positively biased), integer biases, dy in {-1..2},
    gates in {-1, 0, 1}.  All are exact in f16, bf16 and f32, every product and partial sum is an integer below 2^24 -- so the f32
    accumulation is exact in ANY order -- and the sums regularly pass 2048, where a 16-bit accumulator would drop bits.  The f32
    results must then EQUAL the float64 reference, and the 16-bit outputs must equal its round-to-nearest-even (ties included: at
    ~20 000 an f16 step is 16).
  * random normals (He-scaled, rounded to the operand type) with a per-element float64 bound
    |got - ref| <= 2^-p |ref| + 1.01 L 2^-24 S,  S = |x| (*) |w| + |b|  (the same GEMMs on absolute values),
    p = 11 (f16) / 8 (bf16) / no term (f32 out), L = the kernel's real summation length: 9 Cin + 1 for the forward, pixels per K split
    + number of splits for the weight gradient (the split count is read from the workspace size the planner asks for).

The reference (tests/conv_float64_reference.py) is nine shifted float64 GEMMs (rocBLAS dgemm on the device, not MIOpen), a frame
chunk at a time.  Every output's
interior is NaN before the launch (a skipped tile stays NaN), and its frame must stay zero (the next layer reads it as padding)."""
import ctypes as C
import os
import re
import zlib
from collections import namedtuple

import pytest

from conv_float64_reference import _bound_check, _conv_ref, _wgrad_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mv3d_tf_amd", "csrc")
gpu_mark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ the selection rules, restated
FIRST_CIN = 16                 # c_in == 16: the input layer's packing (conv3x3_views_entry)
INPUT_KERNEL_COUT = 64         # ... and with 64 couts, 16-bit out, no gate: conv_input.hip
SMALL_MAX = 512                # 16-bit: tiles128 < SMALL_MAX -> 64 x 128 ("few tiles")
BIG_MIN = 640                  # 16-bit: tiles256 >= BIG_MIN, c_out % 256 == 0, 16-bit out -> conv3x3_pp_kernel
F32_SMALL_MAX = 1024           # f32: tiles128 < F32_SMALL_MAX -> 64 x 128, else 128 x 128
RED_G = 4                      # conv3x3_wgrad_reduce_kernel: thread groups per piece, each an 8-way unrolled run of its splits
WG_PIX, WGF_PIX = 64, 32       # weight gradient: pixels per K step (bf16 / f32)


def _tiles(Ms, cout, bm, bn):
    return sum((M + bm - 1) // bm for M in Ms) * (cout // bn)


def select_path(dt, Ms, cin, cout, out_f32=False, gated=False, pool=False):
    """the kernel mv3d_conv3x3[_views|_pool_views]_{f16,bf16,f32} launches for views of Ms pixels each"""
    if dt == "f32":
        if cout % 128 == 0:
            return "f32_64x128" if _tiles(Ms, cout, 128, 128) < F32_SMALL_MAX else "f32_128x128"
        return "f32_128x64"
    if pool:
        return "pool_128x128" if cout % 128 == 0 else "pool_256x64"
    tag = ("_f32out" if out_f32 else "") + ("_gated" if gated else "")
    if cin == FIRST_CIN:
        if cout == INPUT_KERNEL_COUT and not out_f32 and not gated:
            return "conv_input"
        return ("first_128x128" if cout % 128 == 0 else "first_256x64") + tag
    if cout % 128 == 0:
        if _tiles(Ms, cout, 128, 128) < SMALL_MAX:
            return "64x128" + tag
        if not out_f32 and cout % 256 == 0 and _tiles(Ms, cout, 256, 256) >= BIG_MIN:
            return "pp" + tag
        return "128x128" + tag
    return "256x64" + tag


# every path the table of the issue names; each must be reached by a case below
PATHS = ["64x128", "64x128_f32out", "128x128", "128x128_f32out", "128x128_gated", "pp", "pp_gated", "256x64", "256x64_f32out",
         "conv_input", "first_128x128", "first_256x64_f32out", "pool_128x128", "pool_256x64", "f32_64x128", "f32_128x128", "f32_128x64"]

Case = namedtuple("Case", "name path dts views cin cout framed out_f32 relu gated pool")
H16 = ("f16", "bf16")


def _c(name, path, dts, views, cin, cout, framed=True, out_f32=False, relu=True, gated=False, pool=False):
    return Case(name, path, dts, views, cin, cout, framed, out_f32, relu, gated, pool)


# (views: [(B, H, W)]; one view = the single-view entry, several = one grouped *_views_* launch)
CASES = [
    # conv3x3_pp_kernel: the batch-16 serving shapes (5776-pixel frames: tiles span two frames), c_in 64 (9 K tiles, an odd
    # number) and 128, a partial last M tile, bare output, and the gated data-gradient form at a large batch
    _c("pp_serving_conv4", "pp", H16, [(16, 76, 76)], 512, 512),
    _c("pp_serving_conv3", "pp", H16, [(16, 152, 152)], 256, 256, relu=False),
    _c("pp_cin64_bare", "pp", H16, [(2, 304, 304)], 64, 256, framed=False),
    _c("pp_cin128_partial_tile", "pp", H16, [(5, 181, 183)], 128, 256),
    _c("pp_gated", "pp_gated", ("bf16",), [(16, 76, 76)], 512, 512, relu=False, gated=True),
    # 128 x 128: training shapes, framed and bare; f32 output (conv5_3 of a serving batch: the pp tile has no f32 form)
    _c("t128_train_conv2", "128x128", H16, [(2, 304, 304)], 64, 128),
    _c("t128_train_conv3_bare", "128x128", H16, [(2, 152, 152)], 128, 256, framed=False, relu=False),
    _c("t128_partial_tile", "128x128", H16, [(3, 157, 151)], 192, 128),
    _c("t128_f32out_serving", "128x128_f32out", H16, [(16, 76, 76)], 512, 512, framed=False, out_f32=True),
    _c("t128_f32out_odd", "128x128_f32out", H16, [(2, 153, 149)], 128, 256, framed=False, out_f32=True, relu=False),
    _c("t128_gated_dgrad", "128x128_gated", ("bf16",), [(2, 304, 304)], 128, 128, relu=False, gated=True),
    # few tiles
    _c("t64_conv4_batch2", "64x128", H16, [(2, 76, 76)], 512, 512),
    _c("t64_f32out_rgb", "64x128_f32out", H16, [(1, 46, 155)], 512, 512, framed=False, out_f32=True),
    # 64-cout layers
    _c("t256x64_conv1_2", "256x64", H16, [(2, 608, 608)], 64, 64),
    _c("t256x64_odd", "256x64", H16, [(3, 37, 53)], 192, 64, relu=False),
    _c("t256x64_f32out", "256x64_f32out", H16, [(1, 45, 77)], 128, 64, framed=False, out_f32=True),
    # input layer (9 real channels of 16)
    _c("input_kernel_bev", "conv_input", H16, [(2, 608, 608)], 16, 64),
    _c("input_kernel_odd", "conv_input", H16, [(3, 33, 71)], 16, 64, framed=False, relu=False),
    _c("first_128x128", "first_128x128", H16, [(2, 152, 153)], 16, 128),
    _c("first_256x64_f32out", "first_256x64_f32out", H16, [(1, 97, 311)], 16, 64, framed=False, out_f32=True),
    # convolution + pool epilogue at 608-wide maps (odd height: the VALID pool drops the last row)
    _c("pool_256x64_bev", "pool_256x64", H16, [(2, 608, 608)], 64, 64, pool=True),
    _c("pool_128x128_608w", "pool_128x128", H16, [(1, 41, 608)], 128, 128, pool=True),
    # exact f32
    _c("f32_128x128_train", "f32_128x128", ("f32",), [(2, 304, 304)], 64, 128),
    _c("f32_64x128_bare", "f32_64x128", ("f32",), [(2, 38, 50)], 128, 256, framed=False, relu=False),
    _c("f32_128x64", "f32_128x64", ("f32",), [(2, 152, 152)], 128, 64),
    # grouped launches, BEV / RGB / FV sizes: no view alone crosses the threshold, their sum does
    _c("views_pp", "pp", H16, [(4, 152, 152), (4, 94, 311), (4, 16, 128)], 256, 256),
    _c("views_128x128", "128x128", H16, [(2, 76, 76), (2, 47, 156), (2, 8, 64)], 512, 512),
    _c("views_f32_128x128", "f32_128x128", ("f32",), [(2, 152, 152), (2, 94, 311), (2, 64, 512)], 128, 128),
    _c("views_pool", "pool_256x64", H16, [(2, 608, 608), (2, 96, 320), (2, 64, 512)], 64, 64, pool=True),
]
_CASE_PARAMS = [pytest.param(c, dt, id="%s-%s" % (c.name, dt)) for c in CASES for dt in c.dts]


def _seed(name):
    return zlib.crc32(name.encode()) % 100003


def _Ms(views):
    return [B * H * W for B, H, W in views]


def test_every_case_selects_the_path_it_names():
    """no GPU: the restated rules send every case to the path it names, and every path of the table has a case"""
    for c in CASES:
        for dt in c.dts:
            assert select_path(dt, _Ms(c.views), c.cin, c.cout, c.out_f32, c.gated, c.pool) == c.path, (c.name, dt)
        if len(c.views) > 1 and c.path in ("pp", "128x128", "f32_128x128"):
            alone = {select_path(c.dts[0], [M], c.cin, c.cout, c.out_f32, c.gated, c.pool) for M in _Ms(c.views)}
            assert c.path not in alone, (c.name, alone)          # only the sum of the views crosses the threshold
    assert set(PATHS) == {c.path for c in CASES}


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def refused(dt, cin, cout, out_f32=False, gated=False, pool=False):
    """the channel counts and flag combinations the launch entries answer with MV3D_ERR_INVALID_ARG"""
    if cin <= 0 or cout <= 0 or cout % 64:
        return True
    if dt == "f32":
        return cin % 32 != 0 or pool                            # (no f32 pool entry; f32 maps out whatever out_f32 says)
    if pool:
        return cin % 64 != 0 or out_f32 or gated
    return (cin % 64 != 0 and cin != FIRST_CIN) or (gated and out_f32)


@pytest.fixture(scope="module")
def hiplib():
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import _lib
    return _lib.lib()


def library_path(L, dt, Ms, cin, cout, out_f32=False, gated=False, pool=False):
    """what the library decides for such a launch: mv3d_conv3x3_path (host only; the selection the launch entries themselves call)
    plus this file's output tag; None = refused"""
    name = L.mv3d_conv3x3_path(4 if dt == "f32" else 2, len(Ms), (C.c_int32 * max(1, len(Ms)))(*Ms), cin, cout, int(out_f32), int(gated), int(pool))
    if name is None:
        return None
    tagged = dt != "f32" and not pool                           # (as select_path tags)
    return name.decode() + (("_f32out" if out_f32 else "") + ("_gated" if gated else "") if tagged else "")


def _edge_views(cout):
    """[(Ms, threshold, tile, side)]: view sizes one tile below (side 0) and at (side 1) each threshold of the selection, in one
    view and in three views of which only the sum crosses; plus sizes far from every threshold"""
    out = [([1], None, None, None), ([5000], None, None, None), ([2 * 608 * 608, 2 * 96 * 320, 2 * 64 * 512], None, None, None)]
    for T, b in ((SMALL_MAX, 128), (F32_SMALL_MAX, 128), (BIG_MIN, 256)):
        f = cout // b
        if f:
            m = (T - 1) // f                                    # m-tiles: m * f < T <= (m + 1) * f
            for side in (0, 1):
                out.append(([b * m + side], T, b, side))
                out.append(([b * (m // 3), b * (m // 3), b * (m - 2 * (m // 3)) + side], T, b, side))
    return out


def test_the_library_selects_what_the_rules_say(hiplib):
    """no GPU: mv3d_conv3x3_path -- the selection the launch entries call -- equals select_path for every case of the table, and on
    a sweep that stands one tile below and exactly at every threshold (in one view, and in three views whose sum alone crosses),
    for every channel class, output type, gate and pool flag; what the entries refuse is NULL"""
    L = hiplib
    for c in CASES:
        for dt in c.dts:
            assert library_path(L, dt, _Ms(c.views), c.cin, c.cout, c.out_f32, c.gated, c.pool) == c.path, (c.name, dt)
    seen = set()
    for dt, cins in (("f16", (16, 64, 48)), ("bf16", (16, 64, 48)), ("f32", (32, 64, 16))):
        for cin in cins:
            for cout in (64, 128, 256, 512, 96):
                for Ms, T, b, side in _edge_views(cout):
                    if T is not None:                            # the sizes are where they claim to be
                        lo = _tiles(Ms, cout, b, b) - side * (cout // b)
                        assert lo < T <= lo + cout // b, (Ms, cout, T)
                        assert len(Ms) == 1 or all(_tiles([M], cout, b, b) < T for M in Ms)
                    for out_f32 in (False, True):
                        for gated in (False, True):
                            for pool in (False, True):
                                want = None if refused(dt, cin, cout, out_f32, gated, pool) else select_path(dt, Ms, cin, cout, out_f32, gated, pool)
                                got = library_path(L, dt, Ms, cin, cout, out_f32, gated, pool)
                                assert got == want, (dt, Ms, cin, cout, out_f32, gated, pool, got, want)
                                seen.add(got)
    assert set(PATHS) | {None} <= seen
    # the thresholds in plain numbers, from both sides
    P = lambda dt, Ms, cin, cout, **kw: library_path(L, dt, Ms, cin, cout, **kw)
    assert P("f16", [128 * 511], 64, 128) == "64x128" and P("f16", [128 * 511 + 1], 64, 128) == "128x128"
    assert P("bf16", [128 * 170, 128 * 170, 128 * 171], 64, 128) == "64x128" and P("bf16", [128 * 170, 128 * 170, 128 * 171 + 1], 64, 128) == "128x128"
    assert P("f16", [256 * 639], 64, 256) == "128x128" and P("f16", [256 * 639 + 1], 64, 256) == "pp"
    assert P("bf16", [256 * 213, 256 * 213, 256 * 213], 64, 256) == "128x128" and P("bf16", [256 * 213, 256 * 213, 256 * 213 + 1], 64, 256) == "pp"
    assert P("f16", [256 * 639 + 1], 64, 256, out_f32=True) == "128x128_f32out"          # the pp tile has no f32 form
    assert P("bf16", [256 * 639 + 1], 64, 256, gated=True) == "pp_gated"
    assert P("f32", [128 * 1023], 32, 128) == "f32_64x128" and P("f32", [128 * 1023 + 1], 32, 128) == "f32_128x128"
    assert P("f32", [128 * 341, 128 * 341, 128 * 341], 32, 128) == "f32_64x128" and P("f32", [128 * 341, 128 * 341, 128 * 341 + 1], 32, 128) == "f32_128x128"
    assert P("f16", [10 ** 6], 16, 64) == "conv_input" and P("f16", [10 ** 6], 16, 64, out_f32=True) == "first_256x64_f32out"
    assert P("bf16", [10 ** 6], 16, 64, gated=True) == "first_256x64_gated" and P("f16", [10 ** 6], 16, 128) == "first_128x128"
    # refused: channel counts, pool on the input layer's packing, a gate with f32 maps out, a gated or f32 pool, view counts, empty views
    assert P("f16", [5000], 64, 96) is None and P("f16", [5000], 48, 64) is None and P("f32", [5000], 16, 64) is None
    assert P("f16", [5000], 16, 64, pool=True) is None and P("bf16", [5000], 64, 64, out_f32=True, gated=True) is None
    assert P("bf16", [5000], 64, 64, gated=True, pool=True) is None and P("f32", [5000], 32, 64, pool=True) is None
    assert P("f16", [], 64, 64) is None and P("f16", [5000] * 4, 64, 64) is None and P("f16", [5000, 0], 64, 64) is None
    assert L.mv3d_conv3x3_path(2, 1, None, 64, 64, 0, 0, 0) is None and L.mv3d_conv3x3_path(3, 1, (C.c_int32 * 1)(5000), 64, 64, 0, 0, 0) is None


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_selection_constants_match_the_sources():
    """no GPU: the weight gradient's constants and conditions restated above are the ones compiled into the product (its plan depends
    on the device's occupancy and is not a pure function; the forward selection is asked of the library, above)"""
    wg = _source("conv3x3_wgrad.hip")
    checks = [
        (wg, r"#define RED_G {n}", RED_G),
        (wg, r"#define WG_PIX {n}", WG_PIX),
        (wg, r"#define WGF_PIX {n}", WGF_PIX),
        (wg, r"P\.bmc = c_out % 128 == 0 \? 128 : 64;", None),
        (wg, r"o \+= \(size_t\)P\.splits\[k\] \* c_out \* 9 \* c_in \* 4; P\.bpart_off\[k\] = o; "
             r"o \+= \(\(size_t\)P\.splits\[k\] \* c_out \* 4 \+ 15\) / 16 \* 16;", None),
        (wg, r"const int per = \(splits \+ RED_G - 1\) / RED_G, k0 = grp \* per, k1 = min\(splits, k0 \+ per\);", None),
    ]
    for src, pat, want in checks:
        m = re.search(pat.replace("{n}", r"(\d+)"), src)
        assert m, pat
        if want is not None:
            assert int(m.group(1)) == want, (pat, m.group(1), want)


# ---------------------------------------------------------------------------------------------------------------- GPU side
@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    return torch


def _dtype(torch, dt):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[dt]


def _nan_output(torch, B, H, W, cout, framed, T):
    """the output buffer: framed = zero frame + NaN interior, bare = all NaN"""
    if framed:
        y = torch.zeros((B, H + 2, W + 2, cout), dtype=T, device="cuda")
        y[:, 1:-1, 1:-1] = float("nan")
        return y
    return torch.full((B, H, W, cout), float("nan"), dtype=T, device="cuda")


def _assert_frame_zero(torch, y):
    fr = y.clone()
    fr[:, 1:-1, 1:-1] = 0
    assert not bool(torch.isnan(fr).any()) and float(fr.abs().max()) == 0.0, "the frame was written"


def _operands(torch, c, dt, exact, seed):
    """per view: (xp f64 framed, w f64 (Cout, Cin, 3, 3), b f64, gate f64 framed | None), values exact in the operand type"""
    T = _dtype(torch, dt)
    g = torch.Generator(device="cuda").manual_seed(seed)
    creal = 9 if c.cin == FIRST_CIN else c.cin
    K = 9 * creal
    out = []
    for B, H, W in c.views:
        xp = torch.zeros((B, H + 2, W + 2, c.cin), dtype=torch.float64, device="cuda")
        if exact:
            xp[:, 1:-1, 1:-1, :creal] = torch.randint(0, 8, (B, H, W, creal), device="cuda", generator=g).double()
            w = torch.zeros((c.cout, c.cin, 3, 3), dtype=torch.float64, device="cuda")
            w[:, :creal] = torch.randint(-1, 4, (c.cout, creal, 3, 3), device="cuda", generator=g).double()
            b = torch.randint(-4 * K, 2 * K, (c.cout,), device="cuda", generator=g).double()
        else:
            xp[:, 1:-1, 1:-1, :creal] = torch.randn((B, H, W, creal), device="cuda", generator=g).to(T).double()
            w = torch.zeros((c.cout, c.cin, 3, 3), dtype=torch.float64, device="cuda")
            w[:, :creal] = (torch.randn((c.cout, creal, 3, 3), device="cuda", generator=g) * (2.0 / K) ** 0.5).to(T).double()
            b = (torch.randn((c.cout,), device="cuda", generator=g) * 0.5).double()
        gate = None
        if c.gated:
            gate = torch.zeros((B, H + 2, W + 2, c.cout), dtype=torch.float64, device="cuda")
            gate[:, 1:-1, 1:-1] = torch.randint(-1, 2, (B, H, W, c.cout), device="cuda", generator=g).double()
        out.append((xp, w, b, gate))
    return out


def _launch(torch, c, dt, ops_views):
    """runs the case's entry on NaN-filled outputs -> the outputs"""
    from mv3d_tf_amd import ops
    T = _dtype(torch, dt)
    OT = torch.float32 if (c.out_f32 or dt == "f32") else T
    args, outs = [], []
    for (B, H, W), (xp, w, b, gate) in zip(c.views, ops_views):
        x16 = xp.to(T)
        if c.cin == FIRST_CIN:
            wp = ops.pack_conv3x3_weights_input_layer(w[:, :9].float(), dtype=T)
        else:
            wp = ops.pack_conv3x3_weights(w.float(), dtype=T)
        if c.pool:
            y = _nan_output(torch, B, H // 2, W // 2, c.cout, True, T)
        else:
            y = _nan_output(torch, B, H, W, c.cout, c.framed, OT)
        args.append((x16, wp, b.float(), None if gate is None else gate.to(T), y))
        outs.append(y)
    if c.pool:
        ops.conv3x3_pool_views([(x, w, b, y) for x, w, b, _, y in args])
    elif len(args) == 1 and c.gated:
        x, w, b, gate, y = args[0]
        ops.conv3x3_gated_bf16(x, w, b, gate, y)
    elif len(args) == 1:
        x, w, b, _, y = args[0]
        ops.conv3x3_f16(x, w, b, out=y, out_framed=c.framed, out_f32=c.out_f32, relu=c.relu)
    else:
        ops.conv3x3_views(args, out_framed=c.framed, out_f32=c.out_f32, relu=c.relu)
    torch.cuda.synchronize()
    return outs


def _interior(y, framed):
    return y[:, 1:-1, 1:-1] if framed else y


@gpu_mark
@pytest.mark.parametrize("c,dt", _CASE_PARAMS)
def test_forward_path_exact_on_integer_operands(gpu, hiplib, c, dt):
    """integer operands: f32 outputs EQUAL the float64 reference, 16-bit outputs equal its round-to-nearest-even"""
    torch = gpu
    assert select_path(dt, _Ms(c.views), c.cin, c.cout, c.out_f32, c.gated, c.pool) == c.path
    assert library_path(hiplib, dt, _Ms(c.views), c.cin, c.cout, c.out_f32, c.gated, c.pool) == c.path
    ops_views = _operands(torch, c, dt, True, seed=_seed(c.name))
    outs = _launch(torch, c, dt, ops_views)
    framed = c.framed or c.pool
    OT = outs[0].dtype
    big = 0
    for (xp, w, b, gate), y in zip(ops_views, outs):
        if framed:
            _assert_frame_zero(torch, y)
        got = _interior(y, framed)
        assert not bool(torch.isnan(got).any()), "an output tile was never written"
        for b0, ref in _conv_ref(torch, xp, w, b, relu=c.relu, gate=gate, pool=c.pool):
            part = got[b0:b0 + ref.shape[0]]
            want = ref.to(OT)
            if not torch.equal(part, want):
                bad = (part.double() != want.double()).nonzero()
                i = tuple(bad[0].tolist())
                raise AssertionError("%s/%s: %d elements differ, first at %s: got %r, want %r (float64 %r)" % (
                    c.name, dt, bad.shape[0], i, float(part[i]), float(want[i]), float(ref[i])))
            big = max(big, float(ref.abs().max()))
    if c.cin != FIRST_CIN:
        assert big > 2048, big                                  # the sums leave the range a 16-bit accumulator would hold


@gpu_mark
@pytest.mark.parametrize("c,dt", _CASE_PARAMS)
def test_forward_path_within_float64_bound_on_random_operands(gpu, hiplib, c, dt):
    """He-scaled random operands rounded to the operand type: per element |got - ref| <= 2^-p |ref| + 1.01 (9 Cin + 1) 2^-24 S"""
    torch = gpu
    assert library_path(hiplib, dt, _Ms(c.views), c.cin, c.cout, c.out_f32, c.gated, c.pool) == c.path
    ops_views = _operands(torch, c, dt, False, seed=_seed(c.name) + 1)
    outs = _launch(torch, c, dt, ops_views)
    framed = c.framed or c.pool
    out_dt = "f32" if (c.out_f32 or dt == "f32") else dt
    L = 9 * (9 if c.cin == FIRST_CIN else c.cin) + 1
    for (xp, w, b, gate), y in zip(ops_views, outs):
        if framed:
            _assert_frame_zero(torch, y)
        got = _interior(y, framed)
        assert not bool(torch.isnan(got).any())
        refs = _conv_ref(torch, xp, w, b, relu=c.relu, gate=gate, pool=False)
        Ss = _conv_ref(torch, xp, w, b, absval=True)
        for (b0, ref), (_, S) in zip(refs, Ss):
            if c.pool:                                          # |max a - max b| <= max |a - b|: the pooled bound is the window's largest
                pool = lambda t: torch.nn.functional.max_pool2d(t.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
                bound = pool(1.01 * L * 2.0 ** -24 * S + 2.0 ** -{"f16": 11, "bf16": 8}[out_dt] * ref.abs())
                ref = pool(ref)
                err = (got[b0:b0 + ref.shape[0]].double() - ref).abs()
                assert bool((err <= bound).all()), (c.name, dt, float((err - bound).max()))
            else:
                _bound_check(torch, got[b0:b0 + ref.shape[0]], ref, S, L, out_dt, "%s/%s" % (c.name, dt))


@gpu_mark
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_batch_invariance_across_paths(gpu, hiplib, dt):
    """A frame's result does not depend on the path its launch takes: frame 5 of a batch-16 launch (conv3x3_pp_kernel), of a
    batch-4 launch (128 x 128, 2 stages) and alone (64 x 128, few tiles), random operands -- bit for bit, as the pp kernel's header
    claims (the three tiles walk a pixel's K steps in the same order through the same MFMA fragments)."""
    torch = gpu
    from mv3d_tf_amd import ops
    T = _dtype(torch, dt)
    g = torch.Generator(device="cuda").manual_seed(16)
    B, H, W, C = 16, 76, 76, 512
    assert select_path(dt, [B * H * W], C, C) == "pp" and select_path(dt, [4 * H * W], C, C) == "128x128"
    assert select_path(dt, [H * W], C, C) == "64x128"
    assert [library_path(hiplib, dt, [b * H * W], C, C) for b in (B, 4, 1)] == ["pp", "128x128", "64x128"]
    x = ops.frame_nhwc_f16(torch.randn((B, H, W, C), device="cuda", generator=g), ops.framed_buffer(B, H, W, C, "cuda", T))
    w = ops.pack_conv3x3_weights(torch.randn((C, C, 3, 3), device="cuda", generator=g) * (2.0 / (9 * C)) ** 0.5, dtype=T)
    b = torch.randn(C, device="cuda", generator=g) * 0.5
    for framed, relu in ((True, True), (False, False)):
        full = ops.conv3x3_f16(x, w, b, out_framed=framed, relu=relu)
        four = ops.conv3x3_f16(x[2:6], w, b, out_framed=framed, relu=relu)
        one = ops.conv3x3_f16(x[5:6], w, b, out_framed=framed, relu=relu)
        torch.cuda.synchronize()
        assert torch.equal(full[5:6], one), "pp vs 64 x 128"
        assert torch.equal(four[3:4], one), "128 x 128 vs 64 x 128"
        assert torch.equal(full[2:6], four), "pp vs 128 x 128"


# ------------------------------------------------------------------------------------------------------------ weight gradient
WCase = namedtuple("WCase", "name dt views cin cout creal fold")
WCASES = [
    WCase("bf16_bmc64_bev_conv1", "bf16", [(2, 608, 608)], 64, 64, None, True),     # ~170 splits: every RED_G group >= 8, remainders
    WCase("bf16_bmc128_bev", "bf16", [(2, 608, 608)], 64, 128, None, True),
    WCase("bf16_input_layer", "bf16", [(2, 608, 608)], 64, 64, 9, False),
    WCase("bf16_bmc128_conv3", "bf16", [(2, 152, 152)], 128, 256, None, False),
    WCase("bf16_small_odd", "bf16", [(1, 21, 33)], 64, 128, 9, False),
    WCase("f32_bmc64_input_layer", "f32", [(2, 304, 304)], 64, 64, 9, True),
    WCase("f32_bmc128", "f32", [(2, 152, 152)], 128, 128, None, False),
    WCase("f32_bmc64_odd", "f32", [(3, 37, 53)], 256, 64, None, False),
    WCase("views_bf16", "bf16", [(2, 152, 152), (2, 94, 311), (2, 16, 128)], 128, 128, None, False),
    WCase("views_f32_input", "f32", [(1, 304, 304), (1, 96, 320), (1, 64, 512)], 64, 64, [9, 3, 3], False),
]


def _plan(views, cin, cout, dt):
    """-> (splits per view, largest pixels per split) of a weight-gradient launch, from the workspace size its planner asks for
    (mv3d_conv3x3_wgrad[_f32 | _views]_workspace_bytes = all views' splits x (Cout 9 Cin 4 + Cout 4)): the views share one number
    of K steps per split; the largest one that gives this split count bounds the summation length"""
    from mv3d_tf_amd import _lib, ops
    L = ops.lib()
    if len(views) == 1:
        B, H, W = views[0]
        need = (L.mv3d_conv3x3_wgrad_f32_workspace_bytes if dt == "f32" else L.mv3d_conv3x3_wgrad_workspace_bytes)(B, H, W, cin, cout)
    else:
        arr = (_lib.WgradView * len(views))()
        for k, (B, H, W) in enumerate(views):
            arr[k] = _lib.WgradView(None, None, None, None, B, H, W, 0)
        need = L.mv3d_conv3x3_wgrad_views_workspace_bytes(len(views), arr, cin, cout, int(dt == "f32"))
    per = cout * 9 * cin * 4 + (cout * 4 + 15) // 16 * 16
    assert need > 0 and need % per == 0, (need, per)
    pix = WGF_PIX if dt == "f32" else WG_PIX
    steps = [(B * (H + 2) * (W + 2) + pix - 1) // pix for B, H, W in views]
    fits = [s for s in range(1, max(steps) + 1) if sum((st + s - 1) // s for st in steps) == need // per]
    assert fits, (need, per, steps)
    sps = max(fits)
    return [(st + sps - 1) // sps for st in steps], sps * pix, need


def _group_sizes(splits):
    per = (splits + RED_G - 1) // RED_G
    return [max(0, min(splits, (k + 1) * per) - k * per) for k in range(RED_G)]


def _wgrad_launch(torch, xq, dyq, creal, dt, need):
    """mv3d_conv3x3_wgrad_{bf16,f32} into NaN-filled dw / db followed by NaN guards (a write past c_in_real's channels shows)"""
    from mv3d_tf_amd import _lib, ops
    B, Hp, Wp, cin = xq.shape
    cout = dyq.shape[3]
    n = cout * creal * 9
    dwbuf = torch.full((n + 64,), float("nan"), dtype=torch.float32, device="cuda")
    dbbuf = torch.full((cout + 64,), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")       # (NaN bytes: every partial sum must be written)
    fn = ops.lib().mv3d_conv3x3_wgrad_f32 if dt == "f32" else ops.lib().mv3d_conv3x3_wgrad_bf16
    _lib.check(fn(xq.data_ptr(), dyq.data_ptr(), dwbuf.data_ptr(), dbbuf.data_ptr(), B, Hp - 2, Wp - 2, cin, creal, cout,
                  ws.data_ptr(), need, ops._stream()), "wgrad")
    torch.cuda.synchronize()
    assert bool(torch.isnan(dwbuf[n:]).all()) and bool(torch.isnan(dbbuf[cout:]).all()), "written past the gradient"
    return dwbuf[:n].view(cout, creal, 3, 3), dbbuf[:cout]


def _wgrad_operands(torch, wc, exact, seed):
    T = _dtype(torch, wc.dt)
    g = torch.Generator(device="cuda").manual_seed(seed)
    reals = wc.creal if isinstance(wc.creal, list) else [wc.creal or wc.cin] * len(wc.views)
    res = []
    for (B, H, W), cr in zip(wc.views, reals):
        xp = torch.zeros((B, H + 2, W + 2, wc.cin), dtype=torch.float64, device="cuda")
        dyp = torch.zeros((B, H + 2, W + 2, wc.cout), dtype=torch.float64, device="cuda")
        if exact:
            xp[:, 1:-1, 1:-1, :cr] = torch.randint(0, 4, (B, H, W, cr), device="cuda", generator=g).double()
            dyp[:, 1:-1, 1:-1] = torch.randint(-1, 3, (B, H, W, wc.cout), device="cuda", generator=g).double()
        else:
            xp[:, 1:-1, 1:-1, :cr] = torch.randn((B, H, W, cr), device="cuda", generator=g).to(T).double()
            dyp[:, 1:-1, 1:-1] = torch.randn((B, H, W, wc.cout), device="cuda", generator=g).to(T).double()
        res.append((xp, dyp, cr))
    return res


@gpu_mark
@pytest.mark.parametrize("exact", [True, False], ids=["integers", "random"])
@pytest.mark.parametrize("wc", WCASES, ids=[w.name for w in WCASES])
def test_weight_gradient_against_float64(gpu, wc, exact):
    """mv3d_conv3x3_wgrad[_views]_{bf16,f32}: integer operands -> dW and db EQUAL the float64 reference (every partial sum of
    every split an exact integer below 2^24); random operands -> |got - ref| <= 1.01 (pixels per split + splits) 2^-24 S.
    The split count comes from the planner's workspace size; the fold cases assert that every RED_G group of the reduce kernel
    runs its 8-way unrolled loop and that some group ends in a remainder."""
    torch = gpu
    from mv3d_tf_amd import ops
    T = _dtype(torch, wc.dt)
    data = _wgrad_operands(torch, wc, exact, seed=_seed(wc.name) + exact)
    splits, pps, need = _plan(wc.views, wc.cin, wc.cout, wc.dt)
    if wc.fold:
        sizes = _group_sizes(splits[0])
        assert min(sizes) >= 8 and any(s % 8 for s in sizes), (splits, sizes)
    if len(wc.views) == 1:
        (xp, dyp, cr), = data
        got = [_wgrad_launch(torch, xp.to(T), dyp.to(T), cr, wc.dt, need)]
    else:
        got = ops.conv3x3_wgrad_views([(xp.to(T), dyp.to(T)) for xp, dyp, _ in data], c_in_real=[cr for _, _, cr in data], want_bias=True)
        torch.cuda.synchronize()
    Ls = [pps + n for n in splits]
    for (xp, dyp, cr), (dw, db), L in zip(data, got, Ls):
        ref_w, ref_b = _wgrad_ref(torch, xp, dyp)
        ref_w = ref_w[:, :cr]
        assert dw.shape == ref_w.shape and not bool(torch.isnan(dw).any()) and not bool(torch.isnan(db).any())
        if exact:
            assert torch.equal(dw, ref_w.float()), (wc.name, int((dw.double() != ref_w).sum()), float((dw.double() - ref_w).abs().max()))
            assert torch.equal(db, ref_b.float()), (wc.name, float((db.double() - ref_b).abs().max()))
            if xp.shape[0] * xp.shape[1] * xp.shape[2] > 20000:
                assert float(ref_w.abs().max()) > 2048            # beyond what a 16-bit accumulator would hold
        else:
            S_w, S_b = _wgrad_ref(torch, xp, dyp, absval=True)
            _bound_check(torch, dw, ref_w, S_w[:, :cr], L, "f32", wc.name + " dW")
            _bound_check(torch, db, ref_b, S_b, L, "f32", wc.name + " db")
