"""Test helper (not a test module): a CPU restatement of the reference's fusion of thresholded decisions with an external
speech-activity mask, LS-EEND/sad_post_process.py:23-33 `sad_func`, and of make_rttm behind it (LS-EEND/metrics.py:59-69 reads
the fused decisions as T_hat: threshold 0.5, median, change points), with the seeded inputs of tests/golden/sad_*.npz.

Pinned: the goldens hold the outputs of the reference's own `sad_func` and `make_rttm` bodies on these inputs (written by
tools/gen_golden_sad.py where the reference tree exists); tests/test_sad_ref.py holds this restatement to them.  Where the
reference is silent the rules are the product's (include/eend_hip.h eend_sad_fuse_f32): a flag is speech iff non-zero; NaN is
never active and never the largest; a speech row of NaN only recovers nobody; -inf and 0 are ordinary values; ties go to the
lowest index (torch.argmax).  Integer work: everything is exact.
"""
import numpy as np
import torch

from oracle import postproc_ref as P

CASES = [dict(name="sad_noise137", seed=21, T=137, S=3, kind="noise", median=11, threshold=0.5, flags="runs"),
         dict(name="sad_smooth500", seed=22, T=500, S=5, kind="smooth", median=11, threshold=0.7, flags="runs"),
         dict(name="sad_T1", seed=23, T=1, S=3, kind="noise", median=11, threshold=0.99, flags="ones"),
         dict(name="sad_short7", seed=24, T=7, S=2, kind="noise", median=11, threshold=0.4, flags="runs"),
         dict(name="sad_flags0", seed=25, T=60, S=3, kind="noise", median=11, threshold=0.5, flags="zeros"),
         dict(name="sad_flags1_rec", seed=26, T=90, S=3, kind="noise", median=11, threshold=0.5, flags="ones"),
         dict(name="sad_flags1_full", seed=27, T=90, S=4, kind="noise", median=11, threshold=0.02, flags="ones"),
         dict(name="sad_ties", seed=28, T=150, S=4, kind="ties", median=11, threshold=0.45, flags="runs"),
         dict(name="sad_med1", seed=29, T=90, S=4, kind="noise", median=1, threshold=0.7, flags="runs"),
         dict(name="sad_med5", seed=30, T=333, S=9, kind="smooth", median=5, threshold=0.7, flags="runs"),
         dict(name="sad_S11", seed=31, T=200, S=11, kind="smooth", median=11, threshold=0.7, flags="runs")]
# cases in which both effects must occur (at least 5 gated and 5 recovered rows, asserted from the goldens' meta)
NON_DEGENERATE = ("sad_noise137", "sad_smooth500", "sad_ties", "sad_med1", "sad_med5", "sad_S11")


def run_flags(seed, T, longest=12):
    """uint8 (T,): alternating runs of 0 and 1 of random lengths 1..longest, so that the median meets gaps it bridges and
    gaps it does not."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, longest + 1, (T + 1,), generator=g).tolist()
    on = int(torch.randint(0, 2, (1,), generator=g))
    out = []
    for n in lens:
        out += [on] * n
        on ^= 1
        if len(out) >= T:
            break
    return np.array(out[:T], dtype=np.uint8)


def inputs(case):
    """-> (posterior float32 (T, S) tensor, flags uint8 (T,) array) of a golden case."""
    T, S = case["T"], case["S"]
    if case["kind"] == "ties":                  # few distinct values: every row has repeated maxima, some rows an active one
        g = torch.Generator().manual_seed(case["seed"])
        pred = torch.randint(0, 6, (T, S), generator=g).float() / 10
        pred[torch.rand(T, generator=g) < 0.6] *= 0.8
    else:
        from oracle import gen_golden_post as G
        pred = G.post_inputs(case["seed"], T, S, case["kind"])
    flags = {"runs": lambda: run_flags(case["seed"] + 1000, T), "ones": lambda: np.ones(T, np.uint8),
             "zeros": lambda: np.zeros(T, np.uint8)}[case["flags"]]()
    return pred, flags


def sad_fuse(posterior, sad, threshold=0.5):
    """Steps 1-3: float32 (T, S) array of 0 / 1."""
    p = posterior.detach().cpu().numpy() if torch.is_tensor(posterior) else np.asarray(posterior)
    p = p.astype(np.float32)
    g = (np.asarray(sad.detach().cpu() if torch.is_tensor(sad) else sad).reshape(-1) != 0)
    with np.errstate(invalid="ignore"):
        d = (p > np.float32(threshold)) & g[:, None]
        cand = ~np.isnan(p)
        top = np.where(cand, p, -np.inf).max(axis=1, keepdims=True)
        win = cand & (p == top)
    rec = g & ~d.any(axis=1) & win.any(axis=1)
    d[rec, win.argmax(axis=1)[rec]] = True      # argmax of a bool row: its first True, the lowest index among the largest
    return d.astype(np.float32)


def counts(posterior, sad, threshold=0.5):
    """-> (gated rows: non-speech rows that had a decision, recovered rows: speech rows that had none and got one)"""
    p = posterior.detach().cpu().numpy() if torch.is_tensor(posterior) else np.asarray(posterior)
    g = (np.asarray(sad.detach().cpu() if torch.is_tensor(sad) else sad).reshape(-1) != 0)
    with np.errstate(invalid="ignore"):
        raw = (p > np.float32(threshold)).any(axis=1)
    fused = sad_fuse(posterior, sad, threshold).any(axis=1)
    return int((raw & ~g).sum()), int((g & ~raw & fused).sum())


def make_rttm(rec, posterior, sad, threshold=0.5, median=11, **kw):
    """make_rttm's dict of the fused decisions (the median comes after the fusion, as in the reference)."""
    fused = torch.from_numpy(sad_fuse(posterior, sad, threshold))
    return P.make_rttm(rec, fused, threshold=0.5, median=median, **kw)


def flat(rttm):
    return [f"{k}\t{l}" for k in sorted(rttm, key=int) for l in rttm[k]]
