"""Golden vectors of the collar DER (tests/golden/der_*.npz).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_der.py

The reference scores with pyannote.metrics (LS-EEND/metrics.py:41-108), which is not installed where this project is built, so
the goldens come from the interval restatement of pyannote's algorithm in tests/der_ref.py (segments, collars as intervals, gaps
of the union extent, cropping, matching per elementary segment, all in fractions.Fraction).  Inputs are regenerated from the
seeds in tests/der_ref.py CASES, so each file holds only the case with its figures in `meta`, the eight counters, the 16 x 16
co-occurrence counts and the value of the optimal mapping.  `meta` also records what the non-degeneracy test reads: the share
of frames kept, whether an optimal mapping is the identity, and the counters of the same inputs at collar 0.
"""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np

from tests import der_ref as R

OUT = os.path.join(ROOT, "tests", "golden")


def golden(case):
    ref, hyp = R.inputs(case)
    skip = case.get("skip_overlap", False)
    res = R.interval(ref, hyp, case["sub"], case["collar"], skip)
    res0 = R.interval(ref, hyp, case["sub"], 0, skip)
    T = max(ref.shape[0], hyp.shape[0] * case["sub"])
    meta = dict(case, Th=int(hyp.shape[0]), Ch=int(hyp.shape[1]), T=T, kept_share=res["counters"][5] / T,
                identity=all(j == i for j, i in res["mapping"].items()), counters0=res0["counters"])
    return meta, res


def main():
    for c in R.CASES:
        meta, res = golden(c)
        np.savez_compressed(os.path.join(OUT, c["name"] + ".npz"), meta=np.array(repr(meta)),
                            counters=np.array(res["counters"], np.int64), cooc=res["cooc"], best=np.int64(res["best"]))
        print(c["name"], "counters", res["counters"], f"kept {meta['kept_share']:.2f}", "identity" if meta["identity"] else "permuted")


if __name__ == "__main__":
    main()
