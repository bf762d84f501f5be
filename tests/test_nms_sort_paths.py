"""Every path of the score sort (csrc/rank.hip) and of the NMS rounds (csrc/nms.hip), each at the sizes that select it, up to
the library's limit of 32768 boxes per frame, against references that cannot share the kernels' bugs.

The host code picks the sort by the key stride and the round layout by the box count and the cap.  `sort_path` and `rounds`
below restate those rules; every case names what it must reach.  The round layout is asked of the library: `mv3d_nms_round_plan`
(host only) returns the plan the launcher walks, and `test_the_library_plans_the_rounds_the_rules_say` (no GPU) compares it with
`rounds` for every frame size and both layouts; `test_selection_constants_match_the_sources` (no GPU) reads the remaining constants
out of the .hip sources, so that a retuned limit cannot silently move a case to another path.

  * the sort: `nms_host` with a threshold that suppresses nothing returns the whole processing order.  It must equal a numpy
    `lexsort` (descending score, NaN largest, -0.0 == +0.0, ties by descending index) over tied, NaN, infinite, signed-zero,
    subnormal and negative scores, at the sizes around every run count of the merge sort and on the counting sort.
  * the rounds: keep lists of `nms_device` (presorted, capped) and `nms_host` (unsorted) must equal the CPU oracle's.  Frames
    built from clusters of near-duplicates make the greedy stop in a chosen block, so that every round of both layouts runs
    with its frame still unfinished, at every kernel width.
  * the compare: IoUs that round onto the threshold (or onto its predecessor) while the exact quotient lies on the other side,
    thresholds at the fast path's edges under both rules, huge / infinite / NaN coordinates and unions below 2^-20, each in a
    diagonal tile, an off-diagonal tile of round 1, a tile of round 2 and a tile reduced through `rem`.
  * proposal_3d over 24576 anchors: the 24-run merge and the counting sort with the record gather, batched frames that finish
    in different rounds, against the oracle's ROI blobs bit for bit."""
import ctypes as C
import functools
import os
import re
import zlib
from collections import namedtuple
from fractions import Fraction

import numpy as np
import pytest

from mv3d_tf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mv3d_tf_amd", "csrc")
gpu_mark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ the selection rules, restated
RANK_SEG = 1024                # keys per run / counting segment
RANK_LDS_KEYS = 24576          # merge sort while key_stride <= this (all runs staged in LDS), counting sort above
NMS_MAX_WORDS = 512            # blocks of 64 boxes per frame: 32768 boxes
MAX_BOXES = 64 * NMS_MAX_WORDS
SMALL_CAP_MAX = 512            # 0 < max_keep <= 512: the "cap" round layout, else the "nocap" layout
CHL_ARENA = 231                # round 1's chain streams its tiles in epochs of at most this many tiles
FAST_TF_MIN, FAST_TF_MAX = 2.0 ** -10, 2.0 ** 10   # tile_fast() only for tf in [2^-10, 2^10]
TAME_LIMIT = 2.0 ** 18         # ... and only for boxes with every |coordinate| < 2^18
MIN_DEN = 2.0 ** -20           # ... and every union >= 2^-20; otherwise the tile runs the exact path
NOCAP_BOUNDS = (0, 32, 64, 128, 256, 384, None)    # None = nbw
CAP_BOUNDS = (0, 32, 128, 256, 384, None)
CAP_SMALL_NBW = 128            # the cap layout is (0, 32, nbw) up to this many blocks


def key_stride(n):
    return (n + RANK_SEG - 1) // RANK_SEG * RANK_SEG


def sort_path(n):
    """("merge", runs) or ("counting", segments) for a frame of n keys"""
    ks = key_stride(n)
    return ("merge" if ks <= RANK_LDS_KEYS else "counting", ks // RANK_SEG)


def layout(max_keep):
    return "nocap" if max_keep <= 0 or max_keep > SMALL_CAP_MAX else "cap"


def kernel_width(w):
    return 32 if w <= 32 else 64 if w <= 64 else 128


def rounds(n, max_keep):
    """[(b0, b1, kernel)] of mv3d_launch_nms: round 1 is nms_tiles_kernel + nms_chain_lds_kernel ("chain_lds"), a later round
    nms_round_kernel<32|64|128>"""
    nbw = (n + 63) // 64
    if layout(max_keep) == "nocap":
        b = [nbw if x is None else x for x in NOCAP_BOUNDS]
    elif nbw > CAP_SMALL_NBW:
        b = [nbw if x is None else x for x in CAP_BOUNDS]
    else:
        b = [0, 32, nbw]
    out = []
    for r in range(len(b) - 1):
        b0, b1 = min(b[r], nbw), min(b[r + 1], nbw)
        if r > 0 and b0 >= b1:
            break
        out.append((b0, b1, "chain_lds" if r == 0 else kernel_width(b1 - b0)))
    return out


def chain_epochs(cols):
    """chl_epoch_end(): round 1's columns cut into epochs of whole columns of at most CHL_ARENA tiles"""
    out, c0 = [], 0
    while c0 < cols:
        c1 = c0
        while c1 < cols and (c1 + 1) * (c1 + 2) // 2 - c0 * (c0 + 1) // 2 <= CHL_ARENA:
            c1 += 1
        out.append((c0, c1))
        c0 = c1
    return out


def finishing_block(n, max_keep, keep_positions):
    """the block in which the greedy pass stops: the one holding the max_keep-th kept box, else the last block"""
    if max_keep > 0 and len(keep_positions) >= max_keep:
        return keep_positions[max_keep - 1] // 64
    return max(0, (n + 63) // 64 - 1)


def finishing_round(n, max_keep, keep_positions, n_cap=None):
    """1-based index of the round that finishes a frame of n boxes (the layout follows the capacity n_cap, default n)"""
    b = finishing_block(n, max_keep, keep_positions)
    for r, (b0, b1, _) in enumerate(rounds(n if n_cap is None else n_cap, max_keep)):
        if b0 <= b < max(b1, 1):
            return r + 1
    raise AssertionError((n, max_keep, b))


def reached(n, max_keep, keep_positions):
    """{(layout, round, kernel)} of the rounds that run with the frame still unfinished"""
    fin = finishing_round(n, max_keep, keep_positions)
    return {(layout(max_keep), r + 1, k) for r, (_, _, k) in enumerate(rounds(n, max_keep)) if r + 1 <= fin}


def all_round_combos():
    return {(layout(c), r + 1, k) for n in range(1, MAX_BOXES + 1, 64) for c in (0, 300)
            for r, (_, _, k) in enumerate(rounds(n, c))}


def ceil_f32(t):
    """mv3d_ceil_f32: the smallest f32 >= t"""
    f = np.float32(t)
    if float(f) < t:
        f = np.nextafter(f, np.float32(np.inf))
    return f


def fast_ok(tf):
    return FAST_TF_MIN <= float(tf) <= FAST_TF_MAX


# ------------------------------------------------------------------------------------------------ constants vs the sources
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(src, name):
    m = re.search(r"#define %s (\d+)" % name, src)
    assert m, name
    return int(m.group(1))


@functools.lru_cache(maxsize=None)
def _hiplib():
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import _lib
    return _lib.lib()


def library_rounds(n, max_keep):
    """what the library decides: mv3d_nms_round_plan (host only; the plan function mv3d_launch_nms itself walks), in the form of
    `rounds`; None = refused"""
    out = (C.c_int32 * 21)(*([-1] * 21))
    nr = _hiplib().mv3d_nms_round_plan(n, max_keep, out)
    assert 0 <= nr <= 7 and all(v == -1 for v in out[3 * nr:])
    return [(out[3 * r], out[3 * r + 1], out[3 * r + 2] or "chain_lds") for r in range(nr)] or None


def test_the_library_plans_the_rounds_the_rules_say():
    """no GPU: the library's round plan equals the restated one, kernel widths included, for every frame size in blocks and on both
    sides of the cap that switches the layout; an empty frame, box counts that fill no whole block, and counts it refuses"""
    for nbw in range(1, NMS_MAX_WORDS + 1):
        for cap in (0, 1, SMALL_CAP_MAX, SMALL_CAP_MAX + 1):
            assert library_rounds(64 * nbw, cap) == rounds(64 * nbw, cap), (nbw, cap)
    assert library_rounds(0, 0) == library_rounds(0, 300) == [(0, 0, "chain_lds")] == rounds(0, 0)
    for n in (1, 63, 65, 2049, 64 * CAP_SMALL_NBW + 1, 13000, 16385, MAX_BOXES - 63, MAX_BOXES - 1):
        for cap in (-1, 0, 300, SMALL_CAP_MAX, SMALL_CAP_MAX + 1, 2000):
            assert library_rounds(n, cap) == rounds(n, cap), (n, cap)
    # the layouts in plain numbers, at the edges of the cap and of the small cap layout
    assert library_rounds(64 * 128, 512) == [(0, 32, "chain_lds"), (32, 128, 128)]
    assert library_rounds(64 * 128 + 1, 512) == [(0, 32, "chain_lds"), (32, 128, 128), (128, 129, 32)]
    assert library_rounds(64 * 128, 513) == [(0, 32, "chain_lds"), (32, 64, 32), (64, 128, 64)]
    assert library_rounds(32768, 0) == [(0, 32, "chain_lds"), (32, 64, 32), (64, 128, 64), (128, 256, 128), (256, 384, 128), (384, 512, 128)]
    assert library_rounds(64 * 97, 300) == [(0, 32, "chain_lds"), (32, 97, 128)] and library_rounds(64 * 96, 300)[1] == (32, 96, 64)
    assert library_rounds(64 * 65, 0)[2] == (64, 65, 32) and library_rounds(64 * 64, 300)[1] == (32, 64, 32)
    assert library_rounds(MAX_BOXES + 1, 0) is None and library_rounds(-1, 0) is None and library_rounds(10 ** 6, 300) is None


def test_selection_constants_match_the_sources():
    """no GPU: the constants restated above are the ones rank.hip / nms.hip compile (the round layout is asked of the library,
    above)"""
    rank, nms = _src("rank.hip"), _src("nms.hip")
    assert _define(rank, "RANK_LDS_KEYS") == RANK_LDS_KEYS and _define(rank, "RANK_SEG") == RANK_SEG
    assert _define(rank, "RANK_RUN") == RANK_SEG
    assert re.search(r"if \(key_stride <= RANK_LDS_KEYS\)", rank)
    assert re.search(r"return \(N \+ RANK_SEG - 1\) / RANK_SEG \* RANK_SEG;", rank)
    assert _define(nms, "NMS_MAX_WORDS") == NMS_MAX_WORDS and _define(nms, "CHL_ARENA") == CHL_ARENA
    # the fast path's gates
    m = re.search(r"d\.fast_ok = \(d\.tf >= (0x1p-?\d+f) && d\.tf <= (0x1p-?\d+f)\)", nms)
    assert m and float.fromhex(m.group(1)[:-1]) == FAST_TF_MIN and float.fromhex(m.group(2)[:-1]) == FAST_TF_MAX
    m = re.search(r"const float L = (0x1p\d+f);", nms)
    assert m and float.fromhex(m.group(1)[:-1]) == TAME_LIMIT
    m = re.search(r"min_den >= (0x1p-\d+f)", nms)
    assert m and float.fromhex(m.group(1)[:-1]) == MIN_DEN
    assert "d.neg_h = d.fast_ok ? -0.5f * (d.tf - nextafterf(d.tf, 0.0f))" in nms
    # round 1's chain at its full 32 columns: three epochs, columns [0, 21), [21, 29) and [29, 32)
    assert re.search(r"while \(c1 < cols && \(c1 \+ 1\) \* \(c1 \+ 2\) / 2 - T0 <= CHL_ARENA\) \+\+c1;", nms)
    assert chain_epochs(32) == [(0, 21), (21, 29), (29, 32)]


def test_sort_and_round_restatement_at_the_named_sizes():
    """no GPU: the sizes of the issue land where the tables say"""
    assert sort_path(24576) == ("merge", 24) and sort_path(23553) == ("merge", 24) and sort_path(23552) == ("merge", 23)
    assert sort_path(24577) == ("counting", 25) and sort_path(25600) == ("counting", 25) and sort_path(32768) == ("counting", 32)
    assert rounds(32768, 0)[4:] == [(256, 384, 128), (384, 512, 128)]
    assert rounds(32768, 300) == [(0, 32, "chain_lds"), (32, 128, 128), (128, 256, 128), (256, 384, 128), (384, 512, 128)]
    assert rounds(16385, 2000)[-1] == (256, 257, 32)
    assert rounds(13000, 0)[-1] == (128, 204, 128)


# ------------------------------------------------------------------------------------------------ frames with controlled suppression
GRID, PITCH, SIDE = 182, 40, 16     # 182^2 >= 32768 cluster cells, 40 apart: boxes of different clusters never overlap


def cluster_frame(n, seed, news, integer=True, exclusive=None):
    """(n,5) dets in processing order (score descending, all distinct).  Position p starts a new cluster if p is in `news`,
    else it joins a random earlier cluster as a near-duplicate (IoU >= 0.78 with every member: suppressed at thresh <= 0.78 by
    the cluster's first box, which is kept).  `exclusive` {start: [members]} pins clusters that no other position joins."""
    rng = np.random.RandomState(seed)
    exclusive = exclusive or {}
    is_new = np.zeros(n, bool)
    is_new[sorted(news)] = True
    is_new[0] = True
    fixed = {}
    for start, members in exclusive.items():
        is_new[start] = True
        for m in members:
            fixed[m] = start
            is_new[m] = False
    cid = np.full(n, -1, np.int64)
    starts, nc = [], 0
    pinned = set(exclusive)
    open_ids = []
    for p in range(n):
        if is_new[p]:
            cid[p] = nc
            if p not in pinned:
                open_ids.append(nc)
            starts.append(p)
            nc += 1
    starts, open_ids = np.asarray(starts), np.asarray(open_ids, np.int64)
    for p in range(n):
        if cid[p] < 0 and p not in fixed:
            k = int(np.searchsorted(starts, p))                        # clusters started before p
            m = int(np.searchsorted(open_ids, k))
            cid[p] = open_ids[rng.randint(m)] if m else 0
    for m, start in fixed.items():
        cid[m] = cid[start]
    cx = (cid % GRID) * PITCH + 64.0
    cy = (cid // GRID) * PITCH + 64.0
    j = rng.randint(0, 2, (n, 2)).astype(np.float64) if integer else rng.uniform(0, 1, (n, 2))
    x1, y1 = cx + j[:, 0], cy + j[:, 1]
    score = (n - np.arange(n)) * 2.0 ** -15
    d = np.stack([x1, y1, x1 + SIDE - 1, y1 + SIDE - 1, score], 1).astype(np.float32)
    return d


def _news(n, seed, cap, fin_block, tail_every=0):
    """new-cluster positions: cap - 1 of them spread over blocks [0, fin_block), the cap-th in block fin_block, then one
    every `tail_every` positions (0: none)"""
    rng = np.random.RandomState(seed + 1)
    pre = fin_block * 64
    news = {0}
    if cap > 1:
        news |= set(int(v) for v in rng.choice(np.arange(1, pre), cap - 2, replace=False)) if cap > 2 else set()
        news.add(int(min(n - 1, pre + rng.randint(0, 64))))
    if tail_every:
        news |= set(range(min(n - 1, pre + 64), n, tail_every))
    return sorted(news)


NmsCase = namedtuple("NmsCase", "name n cap thresh gen seed fin")
# gen: ("synth", variant, integer) | ("ctl", fin_block, tail_every, integer) | ("ctl_rem",) ; fin = expected finishing round
NMS_CASES = [
    # nocap layout, frames that run to their last block: every (round, width) of the layout
    NmsCase("nocap_r2w32_3000", 3000, 0, 0.7, ("ctl", 0, 3, True), 1, 2),
    NmsCase("nocap_r3w32_5000", 5000, 0, 0.7, ("ctl", 0, 5, False), 2, 3),
    NmsCase("nocap_r3w64_7000", 7000, 0, 0.7, ("synth", "clustered", True), 3, 3),
    NmsCase("nocap_r4w32_9000", 9000, 0, 0.5, ("synth", "rand", False), 4, 4),
    NmsCase("nocap_r4w64_11000", 11000, 0, 0.7, ("ctl", 0, 9, True), 5, 4),
    NmsCase("nocap_r4w128_16384", 16384, 0, 0.7, ("synth", "clustered", False), 6, 4),
    NmsCase("nocap_r5w32_16385", 16385, 0, 0.7, ("ctl", 0, 11, False), 7, 5),
    NmsCase("nocap_r5w64_19000", 19000, 0, 0.6, ("synth", "rand", True), 8, 5),
    NmsCase("nocap_r5w128_24576", 24576, 0, 0.7, ("ctl", 0, 17, True), 9, 5),
    NmsCase("nocap_r6w32_24577", 24577, 0, 0.7, ("synth", "clustered", True), 10, 6),
    NmsCase("nocap_r6w32_24640", 24640, 0, 0.5, ("ctl", 0, 13, False), 11, 6),
    NmsCase("nocap_r6w32_25600", 25600, 0, 0.7, ("synth", "rand", False), 12, 6),
    NmsCase("nocap_r6w64_27500", 27500, 0, 0.7, ("ctl", 0, 19, True), 13, 6),
    NmsCase("nocap_r6w128_32767", 32767, 0, 0.7, ("synth", "clustered", False), 14, 6),
    NmsCase("nocap_rem_32768", 32768, 0, 0.7, ("ctl_rem",), 15, 6),
    # caps above 512: the nocap layout, stopping in a chosen round
    NmsCase("cap513_r2_16385", 16385, 513, 0.7, ("ctl", 40, 7, True), 16, 2),
    NmsCase("cap2000_r3_24577", 24577, 2000, 0.7, ("ctl", 100, 5, False), 17, 3),
    NmsCase("cap2000_r6_32768", 32768, 2000, 0.7, ("ctl", 500, 0, True), 18, 6),
    NmsCase("cap5000_r5_25600", 25600, 5000, 0.7, ("ctl", 300, 0, False), 19, 5),
    NmsCase("cap5000_runs_out_32767", 32767, 5000, 0.7, ("ctl", 0, 23, True), 20, 6),
    NmsCase("cap2000_synth_32768", 32768, 2000, 0.7, ("synth", "rand", True), 21, None),
    # the cap layout (0 < cap <= 512): every (round, width), the frame finishing in the round it names
    NmsCase("cap300_r2w32_3000", 3000, 300, 0.7, ("ctl", 40, 0, True), 22, 2),
    NmsCase("cap512_r2w64_5000", 5000, 512, 0.7, ("ctl", 70, 0, False), 23, 2),
    NmsCase("cap300_r3w32_9000", 9000, 300, 0.7, ("ctl", 135, 0, True), 24, 3),
    NmsCase("cap50_r3w64_11000", 11000, 50, 0.7, ("ctl", 170, 0, False), 25, 3),
    NmsCase("cap300_r3w128_16384", 16384, 300, 0.7, ("ctl", 250, 0, True), 26, 3),
    NmsCase("cap512_r4w32_16385", 16385, 512, 0.7, ("ctl", 256, 0, False), 27, 4),
    NmsCase("cap300_r4w64_19000", 19000, 300, 0.7, ("ctl", 290, 0, True), 28, 4),
    NmsCase("cap300_r4w128_24576", 24576, 300, 0.7, ("ctl", 383, 0, False), 29, 4),
    NmsCase("cap512_r5w32_24577", 24577, 512, 0.7, ("ctl", 384, 0, True), 30, 5),
    NmsCase("cap300_r5w32_25600", 25600, 300, 0.7, ("ctl", 399, 0, False), 31, 5),
    NmsCase("cap300_r5w64_27500", 27500, 300, 0.7, ("ctl", 420, 0, True), 32, 5),
    NmsCase("cap300_r5w128_32768", 32768, 300, 0.7, ("ctl", 460, 0, False), 33, 5),
    NmsCase("cap512_runs_out_32767", 32767, 512, 0.7, ("ctl", 0, 0, True), 34, 5),
    # stopping in round 1 at the largest sizes
    NmsCase("cap1_32768", 32768, 1, 0.7, ("synth", "rand", False), 35, 1),
    NmsCase("cap300_r1_32768", 32768, 300, 0.7, ("synth", "clustered", True), 36, None),
    NmsCase("cap300_r1_24577", 24577, 300, 0.5, ("synth", "rand", True), 37, None),
]
NMS_IDS = [c.name for c in NMS_CASES]
REM_SUPPRESSOR, REM_VICTIMS = 3 * 64 + 5, (40 * 64 + 7, 300 * 64 + 9, 500 * 64 + 11)


def nms_frame(case):
    """(n,5) f32 dets in processing order"""
    g = case.gen
    if g[0] == "synth":
        d = synth.nms_dets(1000 + case.seed, case.n, g[1], integer=g[2])
        return np.ascontiguousarray(d[np.argsort(-d[:, 4], kind="stable")])
    if g[0] == "ctl_rem":
        # one kept box of block 3 is the only suppressor of boxes in blocks 40, 300 and 500 (rounds 2, 5 and 6: the last two
        # see it only through rem, reduced from tiles of a row block finished in round 1)
        news = set(range(0, case.n, 29))
        return cluster_frame(case.n, case.seed, news, True, exclusive={REM_SUPPRESSOR: list(REM_VICTIMS)})
    _, fin_block, tail, integer = g
    if case.cap <= 0 or fin_block == 0:
        news = set(range(0, case.n, tail)) if tail else set(range(0, case.n, 97))
        if case.cap > 0:                         # a frame that runs out before cap kept boxes
            news = set(range(0, case.n, max(1, case.n // (case.cap - 1))))
    else:
        news = _news(case.n, case.seed, case.cap, fin_block, tail)
    return cluster_frame(case.n, case.seed, news, integer)


@functools.lru_cache(maxsize=None)
def _oracle_keep(name):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    oracle.build()
    case = NMS_CASES[NMS_IDS.index(name)]
    return oracle.cpu_nms(nms_frame(case), case.thresh, presorted=True)


def test_case_table_covers_every_path():
    """no GPU (runs the CPU oracle): each case finishes in the round it names, and the table reaches every (layout, round,
    kernel width) the launcher can produce, frames finishing in each of rounds 1-6, both sort paths at their edges, the sizes
    and caps of the issue, and the rem frame's structure"""
    got = set()
    fins = set()
    for c in NMS_CASES:
        keep = _oracle_keep(c.name)
        fin = finishing_round(c.n, c.cap, keep)
        if c.fin is not None:
            assert fin == c.fin, (c.name, fin, c.fin)
        got |= reached(c.n, c.cap, keep)
        fins.add(fin)
    missing = all_round_combos() - got
    assert not missing, sorted(missing)
    assert fins == {1, 2, 3, 4, 5, 6}
    sizes = {c.n for c in NMS_CASES} | set(SORT_SIZES)
    assert {16384, 16385, 24576, 24577, 24640, 25600, 32767, 32768} <= sizes
    assert {0, 1, 300, 512, 513, 2000, 5000} <= {c.cap for c in NMS_CASES}
    paths = {sort_path(n) for n in sizes}
    assert {("merge", 23), ("merge", 24), ("counting", 25), ("counting", 32)} <= paths
    assert {g for c in NMS_CASES if c.gen[0] == "synth" for g in [(c.gen[1], c.gen[2])]} == \
        {("rand", True), ("rand", False), ("clustered", True), ("clustered", False)}
    keep = set(_oracle_keep("nocap_rem_32768"))
    d = nms_frame(NMS_CASES[NMS_IDS.index("nocap_rem_32768")])
    assert REM_SUPPRESSOR in keep and not keep & set(REM_VICTIMS)
    same = np.all(np.abs(d[:, :2] - d[REM_SUPPRESSOR, :2]) <= 1, axis=1)
    assert sorted(np.nonzero(same)[0].tolist()) == sorted([REM_SUPPRESSOR, *REM_VICTIMS])   # no other box overlaps them


# ------------------------------------------------------------------------------------------------ near-threshold pairs
# Pairs of integer boxes whose f32 IoU (inter and union exact in f32: areas and their sum below 2^24) rounds ONTO tf while the
# exact quotient lies below it ("up": suppressed only because of the rounding), or onto tf's predecessor while the exact quotient
# lies above that ("down": kept although the quotient exceeds the predecessor).  Found by a numpy search over boxes
# [0, 0, iw+a-1, ih-1] / [a, 0, a+iw-1, ih+b-1] (overlap iw x ih); `test_near_threshold_pairs_are_what_they_claim` re-derives
# every claim.  One-pixel-high pairs give the decimal IoUs exactly (IoU = width ratio).
NEAR_PAIRS = [  # (thresh, kind, box1, box2)
    (0.3, "up", (0, 0, 899, 1036), (225, 0, 899, 3110)),
    (0.3, "up", (0, 0, 700, 1049), (0, 0, 700, 3499)),
    (0.3, "down", (0, 0, 2390, 1486), (1172, 0, 2390, 3526)),
    (0.3, "down", (0, 0, 2772, 1158), (1277, 0, 2772, 2873)),
    (0.7, "up", (0, 0, 1709, 1405), (287, 0, 1709, 1724)),
    (0.7, "up", (0, 0, 2064, 1418), (608, 0, 2064, 1434)),
    (0.7, "down", (0, 0, 792, 993), (0, 0, 792, 1419)),
    (0.7, "down", (0, 0, 912, 531), (0, 0, 912, 759)),
    (0.9, "down", (0, 0, 1639, 760), (164, 0, 1639, 760)),
    (0.9, "down", (0, 0, 819, 1366), (82, 0, 819, 1366)),
    (0.3, "up", (0, 0, 4099, 0), (0, 0, 1229, 0)),       # IoU 1230/4100 = 0.3: f32 rounds it up to tf
    (0.7, "down", (0, 0, 4099, 0), (0, 0, 2869, 0)),     # 2870/4100 = 0.7: rounds down to tf's predecessor
    (0.9, "down", (0, 0, 4099, 0), (0, 0, 3689, 0)),     # 3690/4100 = 0.9
]


def iou_f32(p, q):
    """pair_suppresses()'s IoU, operation for operation in f32 (coordinates as given), and the exact quotient"""
    f = np.float32
    ar = lambda r: f(f(f(r[2]) - f(r[0])) + f(1)) * f(f(f(r[3]) - f(r[1])) + f(1))
    w = max(f(0), f(f(f(min(p[2], q[2])) - f(max(p[0], q[0]))) + f(1)))
    h = max(f(0), f(f(f(min(p[3], q[3])) - f(max(p[1], q[1]))) + f(1)))
    inter = f(w * h)
    den = f(f(ar(p) + ar(q)) - inter)
    return f(inter / den), Fraction(float(inter)) / Fraction(float(den)), float(inter), float(den)


def test_near_threshold_pairs_are_what_they_claim():
    """no GPU: every committed pair rounds across tf (or its predecessor) as its kind says, with exact f32 operands"""
    for t, kind, p, q in NEAR_PAIRS:
        tf = ceil_f32(t)
        pred = np.nextafter(tf, np.float32(0))
        v, exact, inter, den = iou_f32(p, q)
        assert inter < 2 ** 24 and den < 2 ** 24 and Fraction(inter) / Fraction(den) == exact
        assert (p[2] + 1) * (p[3] + 1) + (q[2] - q[0] + 1) * (q[3] - q[1] + 1) < 2 ** 24
        if kind == "up":
            assert v == tf and exact < Fraction(float(tf)), (t, p, q)
        else:
            assert v == pred and exact > Fraction(float(pred)), (t, p, q)
        assert fast_ok(tf)
    assert {(t, k) for t, k, _, _ in NEAR_PAIRS} == {(0.3, "up"), (0.3, "down"), (0.7, "up"), (0.7, "down"), (0.9, "down")}


# tile positions of a 70-block frame (nocap layout: rounds [0,32), [32,64), [64,70)): (first box, second box)
EDGE_N = 70 * 64
TILE_POSITIONS = {
    "diagonal": (10 * 64 + 5, 10 * 64 + 40),
    "offdiag_round1": (2 * 64 + 5, 20 * 64 + 40),
    "round2": (40 * 64 + 5, 50 * 64 + 40),
    "round3_via_rem": (5 * 64 + 5, 66 * 64 + 7),
}


def edge_frame(first, second, pos, extra=()):
    """EDGE_N tame, far-apart 4x4 boxes in processing order, with `first` and `second` at the positions `pos`, and
    (position, box) pairs of `extra`"""
    k = np.arange(EDGE_N)
    x = 20000.0 + (k % 67) * 12
    y = 20000.0 + (k // 67) * 12
    d = np.stack([x, y, x + 3, y + 3, (EDGE_N - k) * 2.0 ** -13], 1)
    for p, b in ((pos[0], first), (pos[1], second)) + tuple(extra):
        d[p, :4] = b
    return d.astype(np.float32)


def _shift(b, dx=1000, dy=1000):
    return (b[0] + dx, b[1] + dy, b[2] + dx, b[3] + dy)


EDGE_THRESHOLDS = [2.0 ** -10, float(np.nextafter(np.float32(2.0 ** -10), np.float32(0))), 0.0, 1.0, 2.0 ** 10,
                   float(np.nextafter(np.float32(2.0 ** 10), np.float32(np.inf)))]
EDGE_PAIRS = {  # name -> (first, second)
    "iou_2^-10": ((0, 0, 1023, 0), (1023, 0, 1023, 0)),          # inter 1, union 1024
    "iou_below_2^-10": ((0, 0, 1023, 0), (1023, 0, 1024, 0)),    # 1 / 1025
    "iou_above_2^-10": ((0, 0, 1023, 0), (1022, 0, 1023, 0)),    # 2 / 1024
    "disjoint": ((0, 0, 9, 9), (100, 100, 109, 109)),
    "touching": ((0, 0, 9, 9), (9, 0, 18, 9)),                   # one column shared
    "identical": ((0, 0, 9, 9), (0, 0, 9, 9)),
    "half": ((0, 0, 9, 9), (0, 0, 9, 4)),
}
UNTAME = {  # name -> (first, second): one box of the tile is not tame, the rest are
    "2^18-1_vs_2^18": ((2 ** 18 - 21, 0, 2 ** 18 - 1, 20), (2 ** 18 - 20, 0, 2 ** 18, 20)),
    "2^18-1_both": ((2 ** 18 - 21, 0, 2 ** 18 - 1, 20), (2 ** 18 - 20, 0, 2 ** 18 - 1, 20)),
    "1e30": ((0, 0, 100, 10), (0, 0, 1e30, 10)),
    "1e30_first": ((0, 0, 1e30, 10), (0, 0, 100, 10)),
    "inf_span": ((0, 0, 100, 10), (-np.inf, 0, np.inf, 10)),
    "inf_corner": ((0, 0, 100, 10), (0, 0, np.inf, 10)),
    "nan_first": ((np.nan, 0, 100, 10), (0, 0, 100, 10)),
    "nan_second": ((0, 0, 100, 10), (0, 0, 100, np.nan)),
    "tiny_union_identical": ((5, 5, 4 + 2 ** -12, 4 + 2 ** -12), (5, 5, 4 + 2 ** -12, 4 + 2 ** -12)),   # union 2^-24
    "tiny_union_half": ((5, 5, 4 + 2 ** -12, 4 + 2 ** -12), (5, 5, 4 + 2 ** -13, 4 + 2 ** -12)),        # IoU 0.5
}


def test_edge_constructions_select_the_paths_they_claim():
    """no GPU: the untame boxes break `tame`, the tiny unions fall below MIN_DEN, the edge thresholds sit on both sides of
    the fast path's range under both rules, and the tile positions are the tiles they name"""
    tame = lambda b: all(abs(v) < TAME_LIMIT for v in np.float32(b))
    assert tame(UNTAME["2^18-1_both"][1]) and not tame(UNTAME["2^18-1_vs_2^18"][1])
    for k in ("1e30", "inf_span", "inf_corner", "nan_second"):
        assert not tame(UNTAME[k][1])
    for k in ("tiny_union_identical", "tiny_union_half"):
        assert 0 < iou_f32(*UNTAME[k])[3] < MIN_DEN
    assert float(iou_f32(*UNTAME["tiny_union_half"])[0]) == 0.5
    cpu = [fast_ok(ceil_f32(t)) for t in EDGE_THRESHOLDS]
    cuda = [fast_ok(np.nextafter(np.float32(t), np.float32(np.inf))) for t in EDGE_THRESHOLDS]
    assert cpu == [True, False, False, True, True, False] and cuda == [True, True, False, True, False, False]
    r = rounds(EDGE_N, 0)
    assert [(b0, b1) for b0, b1, _ in r] == [(0, 32), (32, 64), (64, 70)]
    blk = {k: (a // 64, b // 64) for k, (a, b) in TILE_POSITIONS.items()}
    assert blk["diagonal"][0] == blk["diagonal"][1] < 32
    assert blk["offdiag_round1"][0] < blk["offdiag_round1"][1] < 32
    assert 32 <= blk["round2"][0] < blk["round2"][1] < 64
    assert blk["round3_via_rem"][0] < 32 <= 64 <= blk["round3_via_rem"][1]


# ------------------------------------------------------------------------------------------------ the sort, exactly (GPU)
SORT_SIZES = [1, 1023, 1024, 1025, 23552, 23553, 24576, 24577, 32767, 32768]
POPULATIONS = ["ties", "nan", "inf", "signed_zero", "subnormal", "negative"]


def scores(pop, n, seed):
    rng = np.random.RandomState(seed)
    if pop == "ties":                            # 8 values, every run holds every value: ties cross runs both ways
        s = rng.choice(np.float32([0.9, 0.5, 0.25, 0.1, 0.05, 1e-3, 0.75, 0.3]), n)
    elif pop == "nan":
        s = rng.standard_normal(n).astype(np.float32)
        s[rng.random_sample(n) < 0.2] = np.nan
        neg_nan = rng.random_sample(n) < 0.05
        s[neg_nan] = np.frombuffer(np.uint32(0xFFC00001).tobytes(), np.float32)[0]   # a negative NaN with a payload
    elif pop == "inf":
        s = rng.choice(np.float32([np.inf, -np.inf, 1.0, -1.0, 0.5]), n)
    elif pop == "signed_zero":
        s = rng.choice(np.float32([0.0, -0.0, 1e-30, -1e-30]), n, p=[0.4, 0.4, 0.1, 0.1])
    elif pop == "subnormal":
        bits = rng.randint(1, 1 << 23, n).astype(np.uint32) | (rng.randint(0, 2, n).astype(np.uint32) << 31)
        s = bits.view(np.float32).copy()
        s[rng.random_sample(n) < 0.1] = np.float32(np.finfo(np.float32).tiny)
        s[rng.random_sample(n) < 0.1] = rng.choice(np.float32([0.0, -0.0]))
        s[rng.random_sample(n) < 0.1] = s[0]                                    # ties among subnormals
    else:                                        # all negative, with ties
        s = -np.abs(rng.standard_normal(n)).astype(np.float32) - np.float32(1e-3)
        s[rng.random_sample(n) < 0.3] = np.float32(-0.5)
    return s.astype(np.float32)


def processing_order(s):
    """descending score, NaN largest, -0.0 == +0.0, ties by descending index"""
    s = np.asarray(s, np.float32).astype(np.float64)
    nan = np.isnan(s)
    v = np.where(nan, 0.0, s) + 0.0              # + 0.0 turns -0.0 into +0.0
    idx = np.arange(len(s))
    return np.lexsort((-idx, -v, ~nan))


def test_processing_order_reference():
    """no GPU: the lexsort reference on hand-checked cases"""
    assert processing_order(np.float32([0.0, -0.0])).tolist() == [1, 0]
    assert processing_order(np.float32([-0.0, 0.0])).tolist() == [1, 0]
    assert processing_order(np.float32([1, np.nan, 2, np.nan, -np.inf, np.inf])).tolist() == [3, 1, 5, 2, 0, 4]
    assert processing_order(np.float32([0.5, 0.5, 0.25, 0.5])).tolist() == [3, 1, 0, 2]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops
    return torch, ops


@pytest.fixture(scope="module")
def sort_boxes():
    return synth.nms_dets(77, MAX_BOXES, "rand", integer=True)[:, :4]


@gpu_mark
@pytest.mark.parametrize("tf", [1.5, 4096.0], ids=["fast_tiles", "exact_tiles"])
@pytest.mark.parametrize("pop", POPULATIONS)
@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_order_exact(gpu, sort_boxes, n, pop, tf):
    """nms_host at a threshold nothing reaches: keep = the processing order, equal to the lexsort reference"""
    _, ops = gpu
    path = sort_path(n)
    assert fast_ok(ceil_f32(tf)) == (tf == 1.5)
    s = scores(pop, n, zlib.crc32(("%s-%d" % (pop, n)).encode()) % 100003)
    dets = np.concatenate([sort_boxes[:n], s[:, None]], 1).astype(np.float32)
    got = ops.nms_host(dets, tf)
    want = processing_order(s).tolist()
    assert len(got) == n, (path, len(got))
    if got != want:
        bad = next(i for i in range(n) if got[i] != want[i])
        pytest.fail("%s n=%d %s: first difference at rank %d: got index %d (score %r), want %d (score %r)" %
                    (path, n, pop, bad, got[bad], s[got[bad]], want[bad], s[want[bad]]))


@gpu_mark
def test_signed_zero_scores_are_equal(gpu):
    """+0.0 and -0.0 are one score: ties by descending index, as numpy and the oracle order them"""
    _, ops = gpu
    dets = np.float32([[0, 0, 9, 9, 0.0], [100, 100, 109, 109, -0.0]])
    assert ops.nms_host(dets, 0.5) == [1, 0]
    dets[:, 4] = [-0.0, 0.0]
    assert ops.nms_host(dets, 0.5) == [1, 0]


@gpu_mark
def test_more_than_32768_boxes_is_refused(gpu):
    torch, ops = gpu
    from mv3d_tf_amd._lib import Mv3dError
    dets = np.concatenate([synth.nms_dets(5, MAX_BOXES + 1, "rand")], 0)
    with pytest.raises(Mv3dError):
        ops.nms_host(dets, 0.7)
    with pytest.raises(Mv3dError):
        ops.nms_device(torch.as_tensor(dets).cuda(), 0.7)


# ------------------------------------------------------------------------------------------------ keep lists (GPU)
@gpu_mark
@pytest.mark.parametrize("name", NMS_IDS)
def test_nms_keep_lists_vs_oracle(gpu, name):
    """nms_device (presorted, capped) and nms_host (shuffled rows, uncapped: the sort runs first) equal the oracle's keep list"""
    torch, ops = gpu
    case = NMS_CASES[NMS_IDS.index(name)]
    d = nms_frame(case)
    want = _oracle_keep(name)
    cap_want = want[:case.cap] if case.cap > 0 else want
    keep, num, status = ops.nms_device(torch.as_tensor(d).cuda(), case.thresh, max_keep=case.cap)
    m = int(num.item())
    assert m == len(cap_want) == (min(case.cap, len(want)) if case.cap > 0 else len(want)), (m, len(cap_want))
    got = keep[:m].cpu().numpy().tolist()
    assert got == cap_want, (name, rounds(case.n, case.cap), finishing_round(case.n, case.cap, want))
    assert int(status.item()) == 0
    perm = np.random.RandomState(case.seed).permutation(case.n)
    got = ops.nms_host(np.ascontiguousarray(d[perm]), case.thresh)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(case.n)
    assert got == inv[want].tolist(), name


# ------------------------------------------------------------------------------------------------ the compare at its edges (GPU)
def _run_cpu_rule(torch, ops, oracle, d, thresh):
    want = oracle.cpu_nms(d, thresh, presorted=True)
    keep, num, status = ops.nms_device(torch.as_tensor(d).cuda(), thresh)
    m = int(num.item())
    assert keep[:m].cpu().numpy().tolist() == want
    assert int(status.item()) == 0
    perm = np.random.RandomState(len(d)).permutation(len(d))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(d))
    assert ops.nms_host(np.ascontiguousarray(d[perm]), thresh) == inv[want].tolist()
    return want


@gpu_mark
@pytest.mark.parametrize("where", list(TILE_POSITIONS))
@pytest.mark.parametrize("k", range(len(NEAR_PAIRS)), ids=["%s_%s_%d" % (p[0], p[1], i) for i, p in enumerate(NEAR_PAIRS)])
def test_near_threshold_pairs_in_every_tile(gpu, oracle, k, where):
    """the second box is suppressed exactly when the ROUNDED quotient reaches tf ("up": yes, "down": no)"""
    torch, ops = gpu
    t, kind, p, q = NEAR_PAIRS[k]
    pos = TILE_POSITIONS[where]
    for a, b in ((p, q), (q, p)):
        d = edge_frame(_shift(a), _shift(b), pos)
        want = _run_cpu_rule(torch, ops, oracle, d, t)
        assert (pos[1] in want) == (kind == "down")


@gpu_mark
@pytest.mark.parametrize("where", list(TILE_POSITIONS))
@pytest.mark.parametrize("thresh", EDGE_THRESHOLDS, ids=["2^-10", "below_2^-10", "0", "1", "2^10", "above_2^10"])
def test_fast_path_threshold_edges_both_rules(gpu, oracle, thresh, where):
    """thresholds on both sides of [2^-10, 2^10] under the cpu rule (>= ceil_f32(t)) and the CUDA rule (> f32(t))"""
    torch, ops = gpu
    pos = TILE_POSITIONS[where]
    for name, (a, b) in EDGE_PAIRS.items():
        d = edge_frame(_shift(a), _shift(b), pos)
        want = _run_cpu_rule(torch, ops, oracle, d, thresh)
        if thresh == 0.0:
            assert want == [0], name                 # the first box suppresses every later box (IoU 0 >= 0)
        got = ops.nms_gpu_rule_host(d, np.float32(thresh)).tolist()
        want_gpu = oracle.gpu_nms_rule(d, np.float32(thresh))
        assert got == want_gpu, name
        if thresh == 0.0:
            assert (pos[1] in want_gpu) == (name in ("disjoint",)), name
        if thresh == 1.0:
            assert len(want_gpu) == EDGE_N and (pos[1] in want) == (name != "identical"), name


@gpu_mark
@pytest.mark.parametrize("where", list(TILE_POSITIONS))
@pytest.mark.parametrize("name", list(UNTAME))
def test_untame_boxes_and_tiny_unions_in_a_tame_tile(gpu, oracle, name, where):
    """a non-tame box or a union below 2^-20 sends its tile to the exact path; a near-duplicate of the second box sits in the
    same tile, so that a wrong fast-path verdict would show"""
    torch, ops = gpu
    pos = TILE_POSITIONS[where]
    a, b = UNTAME[name]
    for thresh in (0.5, 0.7):
        k = pos[0] + 1                           # a tame neighbour of the first box, in its row block: IoU 0.6 with ...
        x, y = 20000.0 + (k % 67) * 12, 20000.0 + (k // 67) * 12
        d = edge_frame(a, b, pos, extra=((pos[1] + 3, (x + 1, y, x + 4, y + 3)),))   # ... a box in the second box's block
        _run_cpu_rule(torch, ops, oracle, d, thresh)


# ------------------------------------------------------------------------------------------------ proposal_3d over 24576 anchors (GPU)
PROPOSAL_GRIDS = [((64, 96), ("merge", 24)), ((64, 97), ("counting", 25)), ((64, 128), ("counting", 32))]


def _proposal_frames(torch, frames):
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    return (dev(np.concatenate([f[0] for f in frames])), dev(np.concatenate([f[1] for f in frames])),
            dev(np.concatenate([f[2] for f in frames])), dev(np.stack([f[3] for f in frames])))


def _check_proposals(oracle, frames, sec, out):
    bv, img, b3, num, status = [t.cpu().numpy() for t in out]
    fins = []
    for b, f in enumerate(frames):
        o_bv, o_img, o_3d, dbg = oracle.proposal_layer_3d(*f, "TRAIN", [8, ], cfg={"TRAIN": sec}, debug=True)
        r = o_bv.shape[0]
        assert num[b] == r, (b, num[b], r)
        o_bv[:, 0] = b; o_img[:, 0] = b; o_3d[:, 0] = b
        assert np.array_equal(bv[b, :r], o_bv) and np.array_equal(img[b, :r], o_img) and np.array_equal(b3[b, :r], o_3d)
        assert not bv[b, r:].any() and not img[b, r:].any() and not b3[b, r:].any()
        assert status[b] == 0
        N = f[0].shape[1] * f[0].shape[2] * 4
        pre, post = sec["RPN_PRE_NMS_TOP_N"], sec["RPN_POST_NMS_TOP_N"]
        order_cap = pre if 0 < pre < N else N
        cap = post if 0 < post < order_cap else order_cap
        fins.append(finishing_round(min(len(dbg["order"]), order_cap), cap, dbg["nms_keep"].tolist(), order_cap))
    return fins


@gpu_mark
@pytest.mark.parametrize("post", [0, 2000, 300])
@pytest.mark.parametrize("pre", [0, 12000])
@pytest.mark.parametrize("grid", [g for g, _ in PROPOSAL_GRIDS], ids=["%dx%d" % g for g, _ in PROPOSAL_GRIDS])
def test_proposal_3d_large_grids_vs_oracle(gpu, oracle, grid, pre, post):
    """the 24-run merge and the counting sort, both with the record gather, feeding up to 32768 boxes to the NMS"""
    torch, ops = gpu
    H, W = grid
    assert sort_path(H * W * 4) == dict(PROPOSAL_GRIDS)[grid]
    sec = dict(RPN_PRE_NMS_TOP_N=pre, RPN_POST_NMS_TOP_N=post, RPN_NMS_THRESH=0.7, RPN_MIN_SIZE=5)
    frame = synth.rpn_head(600 + W + pre // 1000 + post, H, W, "peaky" if (pre + post) % 3 else "rand")
    out = ops.proposal_3d(*_proposal_frames(torch, [frame]), ops.proposal_params(sec, use_gpu_nms=False))
    _check_proposals(oracle, [frame], sec, out)


@gpu_mark
def test_proposal_3d_over_32768_anchors(gpu, oracle):
    """64 x 129 (33024 anchors): refused without a pre-NMS cap (more than 32768 NMS boxes), run with one"""
    torch, ops = gpu
    from mv3d_tf_amd._lib import Mv3dError
    frame = synth.rpn_head(700, 64, 129, "rand")
    sec = dict(RPN_PRE_NMS_TOP_N=0, RPN_POST_NMS_TOP_N=2000, RPN_NMS_THRESH=0.7, RPN_MIN_SIZE=5)
    with pytest.raises(Mv3dError):
        ops.proposal_3d(*_proposal_frames(torch, [frame]), ops.proposal_params(sec, use_gpu_nms=False))
    sec["RPN_PRE_NMS_TOP_N"] = 12000
    out = ops.proposal_3d(*_proposal_frames(torch, [frame]), ops.proposal_params(sec, use_gpu_nms=False))
    _check_proposals(oracle, [frame], sec, out)


@gpu_mark
def test_proposal_3d_batch_frames_finish_in_different_rounds(gpu, oracle):
    """one batch on the counting sort under a TRAIN-like cap (nocap layout): a rand frame, a peaky frame and a frame whose
    min-size filter (scaled by its im_info) leaves few boxes -- each must finish where the oracle's keep list says, alone"""
    torch, ops = gpu
    frames = [synth.rpn_head(801, 64, 97, "rand"), synth.rpn_head(802, 64, 97, "peaky"), synth.rpn_head(803, 64, 97, "rand")]
    frames[2] = (frames[2][0], frames[2][1], frames[2][2].copy(), frames[2][3])
    frames[2][2][0, 2] = 6.0                     # min_size x scale = 30 pixels: almost every box is filtered
    sec = dict(RPN_PRE_NMS_TOP_N=0, RPN_POST_NMS_TOP_N=2000, RPN_NMS_THRESH=0.7, RPN_MIN_SIZE=5)
    out = ops.proposal_3d(*_proposal_frames(torch, frames), ops.proposal_params(sec, use_gpu_nms=False))
    fins = _check_proposals(oracle, frames, sec, out)
    assert len(set(fins)) >= 2, fins
