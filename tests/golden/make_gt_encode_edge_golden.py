#!/usr/bin/env python3
"""Record the REFERENCE's KITTI loader (lib/datasets/kitti_mv3d.py: _load_kitti_annotation, calib_at) on the edge cases of
tests/test_gt_encode_edges.py -> tests/golden/gt_encode_edges.npz (no other fixture is touched).

Same scratch build of the reference as make_golden.py (its `build_scratch` and `kitti_loader`); the case table is imported
from the test module, so the recording and the tests cannot drift apart (each case's text is stored in the fixture and hashed
into it as well).  The cases' label / calib text is written into a KITTI tree, frame i = case i; per case every key of the
annotation the reference's loader returns (gt_overlaps as a dense array) and `calib` = calib_at(i), all under
np.errstate(all="ignore").  Arrays above RECORD_ARRAY_BYTES are stored as (dtype, shape, the test module's `sha_of`).  Where the
reference raises, the exception's type is stored under exc__<case> instead.  The archive is written with fixed member dates:
running the script again gives the same bytes.

Usage:  python tests/golden/make_gt_encode_edge_golden.py  [--keep-scratch]
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
from make_golden import KITTI_TREE_DIRS, PATCH_NOTE, build_scratch, kitti_loader  # noqa: E402
from make_target_edge_golden import write_npz  # noqa: E402
import test_gt_encode_edges as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep-scratch", action="store_true")
    args = ap.parse_args()
    d = tempfile.mkdtemp(prefix="mv3d_ref_")
    build_scratch(d)
    kitti_mv3d, _ = kitti_loader(d)
    table = E.cases()
    root = E.write_tree(os.path.join(d, "KITTI"), table, KITTI_TREE_DIRS)
    db = kitti_mv3d("train", root)
    kw = dict(case_names=np.array(list(table)), numpy_version=np.__version__, scratch_patches=PATCH_NOTE)
    raised = {}
    for i, (name, c) in enumerate(table.items()):
        kw[name + "__inputs_sha"] = np.array(E.case_inputs_sha(c))
        kw[name + "__labels_txt"] = np.array(c["labels_txt"])
        kw[name + "__calib_txt"] = np.array(c["calib_txt"])
        try:
            with np.errstate(all="ignore"):
                ann = db._load_kitti_annotation("%06d" % i)
                out = dict(ann, gt_overlaps=ann["gt_overlaps"].toarray(), calib=db.calib_at(i))
        except Exception as e:  # noqa: BLE001  (whatever the reference raises is the record)
            raised[name] = type(e).__name__
            kw["exc__" + name] = np.array(type(e).__name__)
            print("%-16s raises %s: %s" % (name, type(e).__name__, e))
            continue
        assert set(out) == set(E.ANN_KEYS + ("calib",)), sorted(out)
        for k, a in out.items():
            a = np.asarray(a)
            if a.nbytes > E.RECORD_ARRAY_BYTES:
                kw["%s__%s__sha" % (name, k)] = np.array([str(a.dtype), str(a.shape), E.sha_of(a)])
            else:
                kw["%s__%s" % (name, k)] = a
        print("%-16s %d objects" % (name, len(out["gt_classes"])))
    path = os.path.join(HERE, E.FIXTURE + ".npz")
    write_npz(path, kw)
    print("%s %.1f KB, %d cases, %d raised: %s" % (os.path.basename(path), os.path.getsize(path) / 1024, len(table), len(raised), raised))
    if args.keep_scratch:
        print("scratch kept at", d)
    else:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
