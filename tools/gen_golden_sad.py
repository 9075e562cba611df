"""Golden vectors of the speech-activity-mask post-processing (runs ONLY where the reference tree exists).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_sad.py /path/to/reference

LS-EEND/sad_post_process.py imports hyperpyyaml and h5py at module level, which `sad_func` does not use.  So, like
oracle/gen_golden_post.py, this parses the file, takes the definition of `sad_func` as it stands and evaluates only that, then
the reference's own `make_rttm` body (scipy.signal.medfilt and the change-point scan) on the fused decisions, which is how
LS-EEND/metrics.py:59-69 reads them.  Inputs are seeded (tests/sad_ref.py); each tests/golden/sad_*.npz holds the case (seeds
included) with the number of gated and recovered rows in `meta`, the flag vector, the fused (T, S) map and the RTTM lines.
"""
import ast
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np
import torch

from oracle import gen_golden_post as G
from tests import sad_ref as R

OUT = os.path.join(ROOT, "tests", "golden")


def reference_sad_func(path):
    """The reference's `sad_func` definition alone, with the names it uses (torch, Tensor) bound to the installed torch."""
    ns = {"torch": torch, "Tensor": torch.Tensor}
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name == "sad_func":
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["sad_func"]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else G.REF
    sad_func = reference_sad_func(f"{ref}/LS-EEND/sad_post_process.py")
    (make_rttm,) = G.reference_functions(f"{ref}/LS-EEND/train/utils/make_rttm.py", ["make_rttm"])
    for c in R.CASES:
        pred, flags = R.inputs(c)
        sad = torch.from_numpy(flags).float().unsqueeze(-1)           # (T, 1) float, as label.max(dim=-1, keepdim=True) gives
        decision = torch.where(pred > c["threshold"], 1, 0)
        fused = sad_func(decision, sad, pred)
        assert fused.dtype == torch.float32 and fused.shape == pred.shape
        rttm = make_rttm(rec="rec0", pred=fused, threshold=0.5, median=c["median"])
        lines = [f"{k}\t{l}" for k in sorted(rttm, key=int) for l in rttm[k]]
        raw = decision.sum(-1) > 0
        on = sad.squeeze(-1) == 1
        meta = dict(c, gated=int((raw & ~on).sum()), recovered=int((on & ~raw & (fused.sum(-1) > 0)).sum()))
        np.savez_compressed(os.path.join(OUT, c["name"] + ".npz"), meta=np.array(repr(meta)), flags=flags,
                            fused=fused.numpy().astype(np.uint8), lines=np.array(lines, dtype=object).astype(str))
        print(c["name"], meta["gated"], "gated", meta["recovered"], "recovered", len(lines), "segments")


if __name__ == "__main__":
    main()
