"""CPU: the sweep's reference (tests/sweep_ref.py) against its brute-force form on random small cases, and the seeded cases of
tests/test_sweep_gpu.py shown to be non-degenerate, so that a kernel ignoring a part of the grid cannot pass them."""
import numpy as np
import pytest

from tests import sweep_ref as W


def same(a, b):
    return a["counters"] == b["counters"] and np.array_equal(a["cooc"], b["cooc"]) and a["best"] == b["best"]


def test_reference_equals_the_brute_force_form():
    rng = np.random.default_rng(2024)
    seen_sad = seen_nan = scored = 0
    for _ in range(60):
        ref, pred, flags, ths, meds, sub, collar, skip = W.random_small(rng)
        got = W.sweep(ref, pred, ths, meds, flags, sub, collar, skip)
        assert len(got) == 4
        for g, (th, k) in enumerate((th, k) for th in ths for k in meds):
            assert same(got[g], W.brute(ref, pred, th, k, flags, sub, collar, skip)), (th, k, sub, collar, skip)
        seen_sad += flags is not None
        seen_nan += bool(np.isnan(pred).any())
        scored += got[0]["counters"][0] > 0
    assert seen_sad >= 10 and seen_nan >= 5 and scored >= 30


def test_float32_comparison_is_explicit():
    """0.3 rounds down to float32: a posterior of float32(0.3) is not above the threshold 0.3, though it is above the double."""
    p = np.full((4, 1), np.float32(0.3), np.float32)
    assert float(p[0, 0]) > 0.3 or float(p[0, 0]) < 0.3
    assert not W.decisions(p, 0.3).any()
    assert W.decisions(np.nextafter(p, np.float32(1)), 0.3).all()
    assert not W.decisions(np.full((2, 2), np.nan, np.float32), -1.0).any()
    assert W.decisions(np.array([[np.inf, -np.inf]], np.float32), 0.5).tolist() == [[True, False]]


@pytest.fixture(scope="module")
def cases():
    out = []
    for c in W.CASES:
        ref, pred, flags = W.inputs(c)
        out.append((c, ref, pred, flags, W.sweep(ref, pred, c["thresholds"], c["medians"], flags, c["sub"], c["collar"],
                                                   c.get("skip_overlap", False))))
    return out


def test_points_of_a_case_differ(cases):
    for c, ref, pred, flags, _ in cases:
        ths, meds = c["thresholds"], c["medians"]
        maps = {(th, k): W.activity(pred, th, k, flags) for th in ths for k in meds}
        for k in meds:
            for a in ths:
                for b in ths:
                    if np.float32(a) != np.float32(b):
                        assert (maps[a, k] != maps[b, k]).any(), (c["name"], a, b, k)
        for th in ths:
            for a in meds:
                for b in meds:
                    if a != b:
                        assert (maps[th, a] != maps[th, b]).any(), (c["name"], th, a, b)


def test_rates_differ_and_the_best_point_moves(cases):
    best = []
    for c, _, _, _, res in cases:
        rates = [W.rate(p["counters"]) for p in res]
        assert len(set(rates)) >= 3, (c["name"], rates)
        assert all(p["counters"][0] > 100 for p in res)
        g = min(range(len(rates)), key=lambda i: (rates[i], i))
        best.append((c["thresholds"][g // len(c["medians"])], c["medians"][g % len(c["medians"])]))
    assert any(b != (0.5, 11) for b in best), best


def test_the_mask_recovers_at_a_high_threshold_only(cases):
    masked = [x for x in cases if x[3] is not None]
    assert masked
    for c, _, pred, flags, _ in masked:
        lo, hi = min(c["thresholds"]), max(c["thresholds"])
        with np.errstate(invalid="ignore"):
            none_hi = ~(pred > np.float32(hi)).any(axis=1)
            none_lo = ~(pred > np.float32(lo)).any(axis=1)
        speech = flags != 0
        recovered_hi = speech & none_hi & W.decisions(pred, hi, flags).any(axis=1)
        recovered_lo = speech & none_lo & W.decisions(pred, lo, flags).any(axis=1)
        assert (recovered_hi & ~recovered_lo).any(), c["name"]
        assert (~speech & ~none_lo).any(), c["name"]               # and the gate takes decisions away
