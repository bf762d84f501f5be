#!/usr/bin/env python3
"""Record the REFERENCE's test-time tail of box_detect (lib/fast_rcnn/test_mv.py:240-261) on the edge cases of
tests/test_box_tail_edges.py -> tests/golden/box_tail_edges.npz (no other fixture is touched).

Same scratch build of the reference as make_golden.py (its `build_scratch`); the case table is imported from the test module,
so the recording and the tests cannot drift apart (each case's inputs are hashed into the fixture as well).  Per case, what
make_golden.py stores for box_tail.npz: `corners` = lidar_3d_to_corners(rois_3d[:, 1:7]), `pred_cnr_r` =
bbox_transform_inv_cnr(corners, deltas), `pred_bv` = corners_to_bv(np.hstack([corners] * nc)) and `pred_bv_r` =
corners_to_bv(pred_cnr_r), all under np.errstate(all="ignore").  box_detect itself hard-codes two classes
(`np.hstack((boxes_cnr, boxes_cnr))`, test_mv.py:255): for nc = 2 the script asserts that this is the array it projects; for
any other nc the recording is of the three functions, not of box_detect.  Outputs above RECORD_ARRAY_BYTES are stored as the
test module's `sha_of`.  Where the reference raises, the exception's type is stored under exc__<case> instead.  The archive is
written with fixed member dates: running the script again gives the same bytes.

Usage:  python tests/golden/make_box_tail_edge_golden.py  [--keep-scratch]
"""
import argparse
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
from make_golden import PATCH_NOTE, build_scratch  # noqa: E402
from make_target_edge_golden import write_npz  # noqa: E402
import test_box_tail_edges as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep-scratch", action="store_true")
    args = ap.parse_args()
    d = tempfile.mkdtemp(prefix="mv3d_ref_")
    build_scratch(d)
    import utils.transform as T
    import fast_rcnn.bbox_transform as BT
    table = E.cases()
    kw = dict(case_names=np.array(list(table)), numpy_version=np.__version__, scratch_patches=PATCH_NOTE)
    raised = {}
    for name, c in table.items():
        kw[name + "__inputs_sha"] = np.array(E.case_inputs_sha(c))
        nc = c["nc"]
        try:
            with np.errstate(all="ignore"):
                cnr = T.lidar_3d_to_corners(c["rois_3d"][:, 1:7])
                pred_cnr = np.hstack([cnr] * nc)
                if nc == 2:
                    assert np.array_equal(pred_cnr, np.hstack((cnr, cnr)), equal_nan=True)        # test_mv.py:255
                pred_r = BT.bbox_transform_inv_cnr(cnr, c["deltas"])
                out = (cnr, pred_r, T.corners_to_bv(pred_cnr), T.corners_to_bv(pred_r))
        except Exception as e:  # noqa: BLE001  (whatever the reference raises is the record)
            raised[name] = type(e).__name__
            kw["exc__" + name] = np.array(type(e).__name__)
            print("%-16s raises %s: %s" % (name, type(e).__name__, e))
            continue
        for f, a in zip(E.FIELDS, out):
            a = np.ascontiguousarray(a)
            if a.nbytes > E.RECORD_ARRAY_BYTES:
                kw["%s__%s__sha" % (name, f)] = np.array(E.sha_of(a))
            else:
                kw["%s__%s" % (name, f)] = a
        print("%-16s %s" % (name, " ".join("%s%s" % (a.dtype, np.shape(a)) for a in out)))
    path = os.path.join(HERE, E.FIXTURE + ".npz")
    write_npz(path, kw)
    print("%s %.1f KB, %d cases, %d raised: %s" % (os.path.basename(path), os.path.getsize(path) / 1024, len(table), len(raised), raised))
    if args.keep_scratch:
        print("scratch kept at", d)
    else:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
