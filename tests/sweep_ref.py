"""Test helper (not a test module): the CPU reference of the threshold x median sweep of the collar DER (include/eend_hip.h
eend_collar_der_sweep_u64), composed of restatements that are pinned elsewhere and changed by nothing here:

    threshold + zero-padded median   oracle/postproc_ref.py median_binary (pinned to make_rttm's body by tests/golden/post_*.npz)
    the speech-activity gate         tests/sad_ref.py sad_fuse (pinned to sad_func's body by tests/golden/sad_*.npz)
    the scoring                      tests/der_ref.py grid (held to its interval form and to tests/golden/der_*.npz)

float32 posteriors are compared against np.float32(threshold) explicitly.  `brute` is the second form that tests/test_sweep_ref.py
holds `sweep` to: a literal scipy.signal.medfilt on the 0 / 1 map, then der_ref.interval.  Also the seeded inputs of the GPU
tests: speaker tracks as der_ref.run_track makes them, turned into posteriors by a per-frame offset plus noise, so that many
frames land between the thresholds of a grid and the points differ.  Integer work after the comparison: everything is exact.
"""
import numpy as np

from oracle import postproc_ref as P
from tests import der_ref as R
from tests import sad_ref as S

THRESHOLDS = (0.3, 0.4, 0.5, 0.6, 0.7)
MEDIANS = (1, 11)

# The seeded cases of tests/test_sweep_gpu.py; tests/test_sweep_ref.py asserts on the CPU that none of them is degenerate.
CASES = [
    dict(name="c3_sub10", seed=301, Tr=3000, Cr=3, Ch=4, sub=10, collar=50, on=400, off=500, thresholds=THRESHOLDS, medians=MEDIANS),
    dict(name="c2_sub1", seed=302, Tr=700, Cr=2, Ch=2, sub=1, collar=10, on=90, off=110, thresholds=THRESHOLDS, medians=(1, 3, 11, 127)),
    dict(name="c5_sub3_sad", seed=303, Tr=2500, Cr=5, Ch=5, sub=3, collar=20, on=200, off=500, thresholds=(0.7, 0.3, 0.5, 0.45),
         medians=(11, 1, 3), sad=True),
    dict(name="c8_sub10_sad", seed=304, Tr=6000, Cr=8, Ch=7, sub=10, collar=50, on=600, off=3000, thresholds=THRESHOLDS, medians=MEDIANS,
         sad=True, skip_overlap=True),
    dict(name="c16_sub10", seed=305, Tr=4000, Cr=16, Ch=16, sub=10, collar=50, on=500, off=6000, thresholds=(0.35, 0.5, 0.65),
         medians=(1, 5, 11, 127)),
]


def posteriors(rng, base, spread=0.14, noise=0.2):
    """0 / 1 (Th, Ch) -> float32 posteriors: 0.27 / 0.73 plus an offset per frame (one value for the whole row, uniform in
    +-spread) plus noise per value (uniform in +-noise), clipped to [0, 1]."""
    Th, Ch = base.shape
    off = rng.uniform(-spread, spread, size=(Th, 1))
    p = 0.27 + 0.46 * base + off + rng.uniform(-noise, noise, size=(Th, Ch))
    return np.clip(p, 0.0, 1.0).astype(np.float32)


def make(seed, Tr, Cr, Ch, sub, on, off, th_delta=0, sad=False):
    """-> (ref uint8 (Tr, Cr), pred float32 (Th, Ch), flags uint8 (Th,) or None).  The hypothesis tracks are the reference's,
    every sub-th frame, rotated by one column (so the best mapping is not the identity); columns beyond Cr are tracks of their own."""
    rng = np.random.default_rng(seed)
    ref = np.stack([R.run_track(rng, Tr, on, off) for _ in range(Cr)], axis=1) if Tr else np.zeros((0, Cr), np.uint8)
    Th = max(0, -(-Tr // sub) + th_delta)
    base = np.zeros((Th, Ch), np.uint8)
    sampled = np.roll(ref[::sub][:Th], 1, axis=1)
    w = min(Cr, Ch)
    base[:len(sampled), :w] = sampled[:, :w]
    for c in range(w, Ch):
        base[:, c] = R.run_track(rng, Th, max(1, on // sub), max(1, 4 * off // sub))
    pred = posteriors(rng, base)
    flags = S.run_flags(seed + 1000, Th, longest=14) if sad else None
    return np.ascontiguousarray(ref), pred, flags


def inputs(case):
    return make(case["seed"], case["Tr"], case["Cr"], case["Ch"], case["sub"], case["on"], case["off"], case.get("th_delta", 0),
                case.get("sad", False))


def decisions(pred, threshold, sad=None):
    """float32 (Th, Ch) -> bool (Th, Ch): pred > float32(threshold), strict, NaN never; with flags, the gate of sad_ref."""
    p = np.asarray(pred, dtype=np.float32)
    if sad is not None:
        return S.sad_fuse(p, sad, threshold) != 0 if p.shape[0] else np.zeros(p.shape, bool)
    with np.errstate(invalid="ignore"):
        return p > np.float32(threshold)


def activity(pred, threshold, median, sad=None):
    """-> uint8 (Th, Ch): decisions, then the zero-padded median of `median` frames along time."""
    d = decisions(pred, threshold, sad)
    if not d.shape[0]:
        return d.astype(np.uint8)
    return P.median_binary(d.astype(np.int64), int(median)).astype(np.uint8)


def sweep(ref, pred, thresholds, medians, sad=None, sub=10, collar=50, skip_overlap=False):
    """-> [der_ref.grid(...) of point g], g = i_threshold * len(medians) + i_median."""
    return [R.grid(ref, activity(pred, th, k, sad), sub, collar, skip_overlap) for th in thresholds for k in medians]


def brute(ref, pred, threshold, median, sad=None, sub=10, collar=50, skip_overlap=False):
    """One point, the long way: scipy's medfilt on the 0 / 1 map, pyannote's interval arithmetic on the runs."""
    from scipy.signal import medfilt
    d = decisions(pred, threshold, sad).astype(np.float64)
    if d.shape[0] and median > 1:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)            # "kernel_size exceeds volume extent": zero padding is the point
            d = medfilt(d, (int(median), 1))
    return R.interval(ref, d != 0, sub, collar, skip_overlap)


def aggregate(points):
    """[grid result per recording] -> (summed counters, rate as gen_ref forms it)."""
    c = np.sum([p["counters"] for p in points], axis=0).tolist()
    return c, rate(c)


def rate(c):
    err = c[1] + c[2] + c[3]
    return err / c[0] if c[0] else (0.0 if err == 0 else 1.0)


def random_small(rng):
    """A small random case for the CPU cross-check: (ref, pred, flags or None, thresholds, medians, sub, collar, skip_overlap)."""
    sub = int(rng.choice([1, 2, 3, 10]))
    collar = int(rng.choice([0, 2, 4, 10, 50]))
    Cr, Ch = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    Tr = int(rng.integers(0, 90))
    ref, pred, flags = make(int(rng.integers(0, 2 ** 31)), Tr, Cr, Ch, sub, 20, 25, int(rng.integers(-3, 4)), bool(rng.integers(0, 2)))
    if pred.size and rng.random() < 0.3:
        pred[rng.integers(0, pred.shape[0]), rng.integers(0, Ch)] = np.nan
    ths = [float(v) for v in rng.choice([0.2, 0.35, 0.5, 0.65, 0.8], size=2, replace=False)]
    meds = [int(v) for v in rng.choice([1, 3, 5, 11, 127], size=2, replace=False)]
    return ref, pred, flags, ths, meds, sub, collar, bool(rng.integers(0, 2))
