"""CPU: tests/sad_ref.py (the restatement of the reference's sad_func and of make_rttm behind it) against the goldens the
reference's own function bodies wrote (tests/golden/sad_*.npz, tools/gen_golden_sad.py): the fused map and the RTTM lines,
exactly; and the rules the reference leaves open."""
import ast
import os

import numpy as np
import pytest
import torch

from tests import sad_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAN, INF = float("nan"), float("inf")


def load(case):
    z = np.load(os.path.join(GOLD, case["name"] + ".npz"), allow_pickle=False)
    return ast.literal_eval(str(z["meta"])), z["flags"], z["fused"], [str(l) for l in z["lines"]]


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_restatement_equals_golden(case):
    meta, flags, fused, lines = load(case)
    assert {k: meta[k] for k in case} == case
    pred, f = R.inputs(case)
    assert f.dtype == np.uint8 and np.array_equal(f, flags)
    got = R.sad_fuse(pred, f, case["threshold"])
    assert got.dtype == np.float32 and got.shape == (case["T"], case["S"])
    assert np.array_equal(got.astype(np.uint8), fused)
    assert R.flat(R.make_rttm("rec0", pred, f, case["threshold"], case["median"])) == lines
    assert R.counts(pred, f, case["threshold"]) == (meta["gated"], meta["recovered"])
    for shape in ((-1, 1), (-1,)):                                  # (T, 1) as the reference passes it, and (T,)
        assert np.array_equal(R.sad_fuse(pred, torch.from_numpy(f).float().reshape(shape), case["threshold"]), got)


def test_goldens_cover_both_effects():
    names = [c["name"] for c in R.CASES]
    assert set(R.NON_DEGENERATE) <= set(names)
    for case in R.CASES:
        meta, flags, fused, lines = load(case)
        if case["name"] in R.NON_DEGENERATE:
            assert meta["gated"] >= 5 and meta["recovered"] >= 5, meta
    by = {c["name"]: load(c) for c in R.CASES}
    assert not by["sad_flags0"][2].any() and by["sad_flags0"][3] == [] and by["sad_flags0"][0]["gated"] >= 5
    assert by["sad_flags1_rec"][0]["recovered"] >= 5 and by["sad_flags1_rec"][2].any(axis=1).all()
    assert by["sad_flags1_full"][0]["recovered"] == 0 and by["sad_flags1_full"][0]["gated"] == 0
    assert by["sad_T1"][2].sum() == 1 and by["sad_T1"][0]["recovered"] == 1


def test_ties_go_to_the_lowest_index():
    case = next(c for c in R.CASES if c["name"] == "sad_ties")
    pred, f = R.inputs(case)
    _, _, fused, _ = load(case)
    p = pred.numpy()
    raw = p > np.float32(case["threshold"])
    rec = (f != 0) & ~raw.any(axis=1)
    tied = rec & ((p == p.max(axis=1, keepdims=True)).sum(axis=1) > 1)
    assert tied.sum() >= 5                                           # the case does hold repeated maxima in recovered rows
    for t in np.nonzero(tied)[0]:
        assert fused[t].sum() == 1 and fused[t].argmax() == int(np.nonzero(p[t] == p[t].max())[0][0])


def test_rules_the_reference_leaves_open():
    p = torch.tensor([[0.9, 0.1, 0.2],          # speech, one active: as thresholded
                      [0.9, 0.1, 0.2],          # non-speech: cleared
                      [0.1, 0.3, 0.3],          # speech, none active: the largest, lowest index of the tie
                      [NAN, 0.2, 0.1],          # NaN never wins
                      [NAN, NAN, NAN],          # nobody to recover
                      [NAN, -INF, NAN],         # -inf is an ordinary candidate
                      [0.0, 0.0, 0.0],          # an all-zero row recovers track 0
                      [0.2, NAN, 0.9],          # NaN is never active
                      [0.1, 0.2, 0.3]])         # non-speech, none active: stays empty
    flags = [1, 0, 1, 1, 1, 7, 1, 2.5, 0]                              # any non-zero flag is speech
    want = [[1, 0, 0], [0, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 0, 0]]
    assert R.sad_fuse(p, np.array(flags), 0.5).tolist() == want
    assert R.sad_fuse(p[:0], np.zeros(0), 0.5).shape == (0, 3)


def test_median_runs_after_the_gate():
    """A non-speech gap shorter than the median's half width is bridged, as in the reference."""
    T = 40
    p = torch.full((T, 1), 0.9)
    flags = np.ones(T, np.uint8)
    flags[18:21] = 0
    assert R.sad_fuse(p, flags)[18:21].sum() == 0
    assert len(R.flat(R.make_rttm("r", p, flags, 0.5, 11))) == 1
    assert len(R.flat(R.make_rttm("r", p, flags, 0.5, 1))) == 2
