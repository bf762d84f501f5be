#!/usr/bin/env python3
"""Generate tests/golden/recall_*.npz by calling the REFERENCE's own imdb.evaluate_recall (lib/datasets/imdb.py:121-209).

Runs only in the build container (needs /root/reference, Cython, gcc), like make_golden.py, whose scratch copy it reuses:
`build_scratch` (lib2to3 + the cythonized bbox_overlaps), plus lib/datasets/imdb.py through the same lib2to3 pass inside the stub
`datasets` package gen_kitti uses (the real package drags in every dataset).  The reference runs on hand-built roidbs inside a
minimal `imdb` subclass; every fixture holds the inputs and what the reference returned (or that it raised AssertionError).
The files are written with fixed zip time stamps, so a second run reproduces them byte for byte:

    python tests/golden/make_recall_golden.py            # write the fixtures
    python tests/golden/make_recall_golden.py --check    # regenerate in memory and compare with the committed bytes
"""
import argparse
import io
import os
import shutil
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

REF = make_golden.REF


def add_imdb(d):
    L = os.path.join(d, "lib")
    os.makedirs(f"{L}/datasets", exist_ok=True)
    open(f"{L}/datasets/__init__.py", "w").write("import os.path as osp\nROOT_DIR = osp.dirname(__file__)\nfrom .imdb import imdb\n")
    shutil.copy(f"{REF}/datasets/imdb.py", f"{L}/datasets/imdb.py")
    subprocess.check_call([sys.executable, "-m", "lib2to3", "-w", "-n", f"{L}/datasets/imdb.py"], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)


def npz_bytes(**kw):
    """an .npz (deflated) whose bytes depend on the arrays only"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(kw):
            a = io.BytesIO()
            np.lib.format.write_array(a, np.asanyarray(kw[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, a.getvalue())
    return buf.getvalue()


def int_boxes(rng, n, lo=0, hi=300, wmax=140):
    xy = np.floor(rng.uniform(lo, hi, (n, 2)))
    return np.hstack([xy, xy + np.floor(rng.uniform(4, wmax, (n, 2)))]).astype(np.float32)


def frac_boxes(rng, n):
    xy = rng.uniform(0, 300, (n, 2))
    return np.hstack([xy, xy + rng.uniform(2, 120, (n, 2))]).astype(np.float32)


def make_split(seed, make, frames, nbg=1):
    """frames: per frame (objects G, candidate boxes R).  Every frame's roidb rows: the G objects (class 1, overlap 1), then a
    crowd-style row (class 1, overlap 0.6) and `nbg` background rows (class 0) in the frames with an odd index.  Candidates: random
    boxes, jittered copies of the objects, an exact copy of object 0 (overlap 1.0), duplicated candidates (ties in argmax(axis=0))
    and, in the frames with G >= 3, object 2 == object 1 (ties in max_overlaps.argmax()); the last object of every third frame lies
    far away from every candidate (overlap 0, matched to the first unused box)."""
    rng = np.random.RandomState(seed)
    roidb, cands = [], []
    for fi, (G, R) in enumerate(frames):
        gt = make(rng, G)
        if G >= 3:
            gt[2] = gt[1]
        if G and fi % 3 == 0:
            gt[G - 1] = gt[G - 1] + np.float32(5000)
        extra = 1 + nbg if fi % 2 else 0
        rows = np.vstack([gt, make(rng, extra)]).astype(np.float32)
        cls = np.array([1] * G + ([1] + [0] * nbg)[:extra], np.int32)
        ov = np.zeros((G + extra, 2), np.float32)
        ov[:G, 1] = 1.0
        if extra:
            ov[G, 1], ov[G + 1:, 0] = 0.6, 1.0
            for k in range(min(nbg, G)):                       # background rows near the objects (the candidates of candidate_boxes=None)
                rows[G + 1 + k] = gt[k] + np.floor(rng.uniform(-6, 7, 4)).astype(np.float32)
        areas = ((rows[:, 2].astype(np.float64) - rows[:, 0] + 1) * (rows[:, 3].astype(np.float64) - rows[:, 1] + 1)).astype(np.float32)
        roidb.append(dict(boxes=rows, gt_classes=cls, gt_overlaps=ov, seg_areas=areas))
        c = make(rng, R)
        for k in range(min(R, 2 * G)):
            c[k] = gt[k % G] + np.floor(rng.uniform(-6, 7, 4)).astype(np.float32)
        if R > 3 and G:
            c[3] = gt[0]
        if R > 8:
            c[7] = c[1]
            c[8] = c[1]
        cands.append(c.astype(np.float32))
    return roidb, cands


FRAMES = ((4, 40), (3, 0), (0, 12), (2, 9), (5, 64), (1, 1), (0, 0), (4, 7), (3, 30), (6, 100))

# name: (seed, coordinates, frames, use candidates, area, limit, thresholds[, background rows])
CASES = {
    "recall_int_all": (101, int_boxes, FRAMES, True, "all", None, None),
    "recall_int_limit_below": (101, int_boxes, FRAMES, True, "all", 6, None),
    "recall_int_limit_above": (101, int_boxes, FRAMES, True, "all", 1000, None),
    "recall_int_small": (102, lambda r, n: int_boxes(r, n, wmax=40), FRAMES, True, "small", None, None),
    "recall_int_96_128": (103, lambda r, n: int_boxes(r, n, wmax=160), FRAMES, True, "96-128", 20, None),
    "recall_frac_thresholds": (104, frac_boxes, FRAMES, True, "all", None, np.array([0.25, 0.5, 0.7, 1.0])),
    "recall_own_boxes": (105, int_boxes, FRAMES, False, "all", None, None, 8),     # candidate_boxes=None: the roidb's class-0 rows
    "recall_short_raises": (106, int_boxes, ((2, 9), (3, 2), (1, 4)), True, "all", None, None),
}


def run_case(imdb_cls, bbox_overlaps, name):
    import scipy.sparse
    seed, make, frames, use_cands, area, limit, thresholds = CASES[name][:7]
    roidb, cands = make_split(seed, make, frames, *CASES[name][7:])

    class hand_imdb(imdb_cls):
        def __init__(self, entries):
            imdb_cls.__init__(self, "hand_built")
            self._image_index = list(range(len(entries)))
            self._roidb = entries

        def default_roidb(self):
            return self._roidb

    entries = [dict(e, gt_overlaps=scipy.sparse.csr_matrix(e["gt_overlaps"])) for e in roidb]
    db = hand_imdb(entries)
    kw = dict(numpy_version=np.__version__, scratch_patches=make_golden.PATCH_NOTE + "; lib/datasets/imdb.py through lib2to3",
              area=np.array(area), limit=np.int64(-1 if limit is None else limit), use_candidates=np.int64(use_cands),
              has_thresholds=np.int64(thresholds is not None), thresholds_in=np.zeros(0) if thresholds is None else thresholds,
              roidb_off=np.concatenate([[0], np.cumsum([len(e["boxes"]) for e in roidb])]).astype(np.int32),
              roidb_boxes=np.vstack([e["boxes"] for e in roidb]), gt_classes=np.concatenate([e["gt_classes"] for e in roidb]),
              roidb_gt_overlaps=np.vstack([e["gt_overlaps"] for e in roidb]), seg_areas=np.concatenate([e["seg_areas"] for e in roidb]),
              cand_off=np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int32), cand_boxes=np.vstack(cands))
    try:
        res = db.evaluate_recall(candidate_boxes=cands if use_cands else None, thresholds=thresholds, area=area, limit=limit)
        kw.update(raises_assertion=np.int64(0), ar=np.float64(res["ar"]), recalls=res["recalls"], thresholds=res["thresholds"],
                  gt_overlaps=res["gt_overlaps"])
    except AssertionError:
        kw.update(raises_assertion=np.int64(1))
    assert kw["raises_assertion"] == (name == "recall_short_raises"), name
    return npz_bytes(**kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    d = tempfile.mkdtemp(prefix="mv3d_ref_")
    try:
        make_golden.build_scratch(d)
        add_imdb(d)
        from datasets.imdb import imdb
        from utils.cython_bbox import bbox_overlaps
        for name in CASES:
            data = run_case(imdb, bbox_overlaps, name)
            path = os.path.join(HERE, name + ".npz")
            if args.check:
                assert open(path, "rb").read() == data, name + ": the committed fixture differs"
                print(f"{name:28s} identical")
            else:
                open(path, "wb").write(data)
                print(f"{name:28s} {len(data) / 1024:6.1f} KB")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
