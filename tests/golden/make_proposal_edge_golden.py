#!/usr/bin/env python3
"""Record the REFERENCE's proposal_layer_3d (and, for the target cases, proposal_target_layer_3d) on the cases of
tests/test_proposal_edges.py -> tests/golden/proposal_edges.npz (no other fixture is touched).

Same scratch build of the reference as make_golden.py (its `build_scratch`); the case table is imported from the test module,
so the recording and the tests cannot drift apart (each case's inputs are hashed into the fixture; only outputs are stored).
Per proposal case: the three blobs under the case's cfg section; per target case: the five outputs under the case's numpy
seed and the value np.random.randint(1 << 30) gives right afterwards.  Everything runs under np.errstate(all="ignore").
Outputs above RECORD_ARRAY_BYTES are stored as synth.sha256.  Where the reference raises, the exception's type is stored
under exc__<case> instead.  numpy's version, the scratch patches and numpy's CPU dispatch features are stored as well: numpy's
f32 exp depends on the dispatched kernel where its result is subnormal (the AVX512F and AVX2 + FMA3 kernels agree with one
another and with the oracle, the scalar fall-back does not).  The archive is written with fixed member dates: running the
script again gives the same bytes.

Usage:  python tests/golden/make_proposal_edge_golden.py  [--keep-scratch]
        python tests/golden/make_proposal_edge_golden.py  --find-graze     (prints test_proposal_edges.GRAZE_ROWS again; writes nothing)
"""
import argparse
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
from make_golden import PATCH_NOTE, build_scratch  # noqa: E402
from make_target_edge_golden import write_npz  # noqa: E402
from mv3d_tf_amd import synth  # noqa: E402
import test_proposal_edges as E  # noqa: E402


def cpu_features():
    from numpy._core._multiarray_umath import __cpu_features__ as f
    return " ".join(sorted(k for k, v in f.items() if v))


def find_graze_rows(anchors=(0, 404, 808, 1020)):
    """The search behind test_proposal_edges.GRAZE_ROWS, with the oracle alone.  For an anchor of the first shape the box is put
    at y < 0 and z = -4 (every corner left of and below the camera axis, so every projection is positive once every depth is),
    with its near face a few centimetres in front of the camera.  dl[0] is bisected to the first value at which every depth is
    positive (xmin, ymin sane); dl[1], which moves the smallest depth by about 1e-10 per f32 step, is bisected likewise.  The
    result is the third f32 above that boundary: there and at its neighbours the image box is (xmin, ymin, INT32_MIN, INT32_MIN)."""
    import oracle
    F32 = np.float32
    A = E.anchors_3d(oracle, 16, 16)
    prob, pred, info, calib = E.plane_graze_case()
    sec = dict(E.ALL_VISIBLE, RPN_PRE_NMS_TOP_N=1, RPN_POST_NMS_TOP_N=1)
    rows = {}
    for n in anchors:
        a = A[n]
        dl = np.zeros((1024, 6), F32)
        dl[n, 1], dl[n, 2] = F32((-a[4] / 2 - 0.5 - a[1]) / a[4]), F32((-4.0 - a[2]) / a[5])

        def box(col, v):
            dl[n, col] = v
            with np.errstate(all="ignore"):
                d = oracle.proposal_layer_3d(prob, dl.reshape(pred.shape), info, calib, "TEST", [8, ], cfg={"TEST": sec}, debug=True)[3]
            return d["img"][n], int(d["valid"][n])

        def boundary(col, bad, good):
            """the smallest f32 in (bad, good] at which xmin and ymin are sane"""
            while np.nextafter(bad, F32(np.inf)) < good:
                mid = F32((np.float64(bad) + np.float64(good)) / 2)
                img, _ = box(col, mid)
                bad, good = (bad, mid) if img[0] > -50 and img[1] > -50 else (mid, good)
            return good

        near = lambda delta: F32((a[3] / 2 + delta - a[0]) / a[3])            # dl[0] that puts the near face `delta` metres ahead
        box(0, boundary(0, near(0.0), near(0.2)))
        good = boundary(1, F32(dl[n, 1] - F32(0.2)), dl[n, 1].copy())
        for _ in range(2):
            good = np.nextafter(good, F32(np.inf))
        img, valid = box(1, good)
        assert valid and img[2] == img[3] == E.INT32_MIN, (n, img, valid)
        rows[n] = tuple(float(v) for v in dl[n, :3])
        print("%d: %r,   # image box %s" % (n, rows[n], img.tolist()))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep-scratch", action="store_true")
    ap.add_argument("--find-graze", action="store_true")
    args = ap.parse_args()
    if args.find_graze:
        assert find_graze_rows() == E.GRAZE_ROWS, "the search no longer gives test_proposal_edges.GRAZE_ROWS: paste the rows printed above"
        return
    d = tempfile.mkdtemp(prefix="mv3d_ref_")
    build_scratch(d)
    import oracle
    oracle.build()
    from fast_rcnn.config import cfg
    cfg.USE_GPU_NMS = False
    from rpn_msr.proposal_layer_tf import proposal_layer_3d
    from rpn_msr.proposal_target_layer_tf import proposal_target_layer_3d
    table = E.cases(oracle)
    assert {k: cfg.TRAIN[k] for k in E.TRAIN_SEC} == E.TRAIN_SEC and {k: cfg.TRAIN[k] for k in E.TRAIN_DEFAULTS} == E.TRAIN_DEFAULTS
    kw = dict(case_names=np.array(list(table)), numpy_version=np.__version__, scratch_patches=PATCH_NOTE,
              numpy_cpu_features=cpu_features())
    raised = {}
    for name, c in table.items():
        kw[name + "__inputs_sha"] = np.array(E.case_inputs_sha(c))
        saved = {}
        try:
            with np.errstate(all="ignore"):
                if c["kind"] == "proposal":
                    saved = {k: cfg[c["key"]][k] for k in c["section"]}
                    for k, v in c["section"].items():
                        cfg[c["key"]][k] = v
                    out = proposal_layer_3d(c["prob"], c["pred"], c["im_info"], c["calib"], c["key"], [8, ], [1.0, 1.0])
                    pos = None
                else:
                    saved = {k: cfg.TRAIN[k] for k in c["train"]}
                    for k, v in c["train"].items():
                        cfg.TRAIN[k] = v
                    np.random.seed(c["seed"])
                    out = proposal_target_layer_3d(c["rois_bv"], c["rois_3d"], c["gt_bv"], c["gt_3d"], c["gt_corners"], c["calib"],
                                                   c["num_classes"])
                    pos = int(np.random.randint(1 << 30))
        except Exception as e:  # noqa: BLE001  (whatever the reference raises is the record)
            raised[name] = type(e).__name__
            kw["exc__" + name] = np.array(type(e).__name__)
            print("%-28s raises %s: %s" % (name, type(e).__name__, e))
            continue
        finally:
            for k, v in saved.items():
                cfg[c.get("key", "TRAIN")][k] = v
        if pos is not None:
            kw[name + "__rng"] = np.int64(pos)
        for f, a in zip(E.fields_of(c), out):
            a = np.ascontiguousarray(a)
            if a.nbytes > E.RECORD_ARRAY_BYTES:
                kw["%s__%s__sha" % (name, f)] = np.array(synth.sha256(a))
            else:
                kw["%s__%s" % (name, f)] = a
        print("%-28s %s" % (name, " ".join(str(np.shape(a)) for a in out)))
    assert 4 * len(raised) <= len(table), "the reference raises on more than a quarter of the cases: choose the inputs again"
    path = os.path.join(HERE, E.FIXTURE + ".npz")
    write_npz(path, kw)
    print("%s %.1f KB, %d cases, %d raised: %s" % (os.path.basename(path), os.path.getsize(path) / 1024, len(table), len(raised), raised))
    if args.keep_scratch:
        print("scratch kept at", d)
    else:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
