"""Writes tests/golden/tail_kloop_parent.npz: the logits of the cases of tests/test_gpu_tail_kloop.py as the library
under ``LPF_HIP_LIB`` (or the installed one) computes them, with the commit that library was built from.  Run once on a GPU
box with the PARENT commit's build, before tail_chain.hip changes:

    LPF_HIP_LIB=<parent build>/lpformer_amd/liblpformer_hip.so python tools/tail_kloop_record.py --commit <hash> [--out FILE]

The test then asks the current build for the same bits.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "tail_kloop_parent.npz"))
    a = ap.parse_args()
    from lpformer_amd import _lib
    from tests import scoring_harness as H
    from tests import test_gpu_tail_kloop as T
    case = T.KLoop()
    out = {"parent_commit": np.array(a.commit), "library": np.array(os.path.basename(os.path.dirname(_lib.HIP_LIB_PATH)))}
    for form, _kernel in T.FORMS:
        for bs, n_full in T.CASES:
            batch = case.batch_of(bs, n_full)
            case.scores(batch, form, True)
            out[T.key(form, bs, n_full)] = H._np(case.scores(batch, form, True)).copy()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("wrote %s: %d cases from commit %s (%s)" % (a.out, len(out) - 2, a.commit, _lib.HIP_LIB_PATH))


if __name__ == "__main__":
    sys.exit(main())
