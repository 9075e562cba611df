"""CPU: the two restatements of the collar DER in tests/der_ref.py (frame grid with numpy / scipy, and pyannote's interval
arithmetic with fractions.Fraction) against each other, against tests/golden/der_*.npz and against the hand-sized cases of
include/eend_hip.h's contract.  Everything is exact."""
import ast
import os

import numpy as np
import pytest

from tests import der_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return ast.literal_eval(str(z["meta"])), z["counters"].tolist(), z["cooc"], int(z["best"])


def same(a, b):
    return a["counters"] == b["counters"] and np.array_equal(a["cooc"], b["cooc"]) and a["best"] == b["best"]


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_goldens_and_both_restatements(case):
    meta, counters, cooc, best = load_golden(case["name"])
    assert {k: meta[k] for k in case} == case                                   # the file was written for this case
    ref, hyp = R.inputs(case)
    assert hyp.shape == (meta["Th"], meta["Ch"])
    skip = case.get("skip_overlap", False)
    for res in (R.grid(ref, hyp, case["sub"], case["collar"], skip), R.interval(ref, hyp, case["sub"], case["collar"], skip)):
        assert res["counters"] == counters and np.array_equal(res["cooc"], cooc) and res["best"] == best
        assert R.valid_mapping(res["mapping"], cooc, best)
        total, miss, fa, conf, correct, kept, removed, both = res["counters"]
        assert correct == best and conf == both - best and kept + removed == meta["T"]
    assert R.grid(ref, hyp, case["sub"], 0, skip)["counters"] == meta["counters0"]


def check(got, total, miss, fa, conf, correct, kept=None, cooc=None):
    assert got["counters"][:5] == [total, miss, fa, conf, correct]
    if kept is not None:
        assert got["counters"][5] == kept
    if cooc is not None:
        assert got["cooc"][:len(cooc), :len(cooc[0])].tolist() == cooc and got["cooc"].sum() == sum(map(sum, cooc))


@pytest.mark.parametrize("fn", [R.grid, R.interval], ids=["grid", "interval"])
def test_hand_cases(fn):
    ref, hyp, sub = R.HAND_A
    check(fn(ref, hyp, sub, 0), 10, 2, 2, 0, 8, kept=20)
    check(fn(ref, hyp, sub, 4), 6, 0, 0, 0, 6, kept=12)
    ref, hyp, sub = R.HAND_B
    got = fn(ref, hyp, sub, 0)
    check(got, 14, 0, 6, 0, 14, cooc=[[2, 6, 0], [8, 2, 0]])
    assert got["mapping"] == {0: 1, 1: 0}                                      # h0 -> r1, h1 -> r0, h2 unmapped
    check(fn(ref, hyp, sub, 2), 6, 0, 5, 0, 6, kept=9, cooc=[[0, 2, 0], [4, 0, 0]])
    check(fn(ref, hyp, sub, 0, True), 10, 0, 6, 0, 10, kept=14, cooc=[[0, 4, 0], [6, 0, 0]])


def test_random_sweep():
    rng = np.random.default_rng(2024)
    seen = set()
    for k in range(300):
        ref, hyp, sub, collar, skip = R.random_small(rng)
        g, i = R.grid(ref, hyp, sub, collar, skip), R.interval(ref, hyp, sub, collar, skip)
        assert same(g, i), (k, ref.shape, hyp.shape, sub, collar, skip, g["counters"], i["counters"])
        assert R.valid_mapping(g["mapping"], g["cooc"], g["best"]) and R.valid_mapping(i["mapping"], i["cooc"], i["best"])
        seen.add((sub, collar, skip))
    assert len(seen) == 3 * 5 * 2                                              # every combination came up


def test_empty_sides_and_total_zero():
    z = np.zeros((0, 2), np.uint8)
    ref, hyp, sub = R.HAND_A
    for fn in (R.grid, R.interval):
        assert fn(z, z, 10, 50)["counters"] == [0] * 8
        assert fn(ref, z, 1, 0)["counters"] == [10, 10, 0, 0, 0, 20, 0, 0]      # an empty hypothesis: all missed
        assert fn(z, hyp, 1, 0)["counters"] == [0, 0, 10, 0, 0, 20, 0, 0]       # an empty reference: all false alarm


@pytest.mark.parametrize("name", R.NON_DEGENERATE)
def test_non_degenerate(name):
    meta, counters, _, _ = load_golden(name)
    total, miss, fa, conf, correct = counters[:5]
    assert 0.1 <= meta["kept_share"] <= 0.9 and abs(meta["kept_share"] - counters[5] / meta["T"]) < 1e-12
    assert min(miss, fa, conf, correct) >= 5
    assert meta["identity"] is False
    assert meta["collar"] > 0 and meta["counters0"] != counters
