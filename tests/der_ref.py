"""Test helper (not a test module): two independent CPU restatements of the collar DER that include/eend_hip.h states at
eend_collar_der_u64 (LS-EEND/metrics.py:41-108 scores with pyannote.metrics DiarizationErrorRate(collar=50); pyannote is not
needed and never imported here), with the seeded inputs of tests/golden/der_*.npz.

    grid(ref, hyp, ...)       the frame-grid rule, vectorised numpy, scipy.optimize.linear_sum_assignment
    interval(ref, hyp, ...)   pyannote's algorithm on segments with fractions.Fraction: every maximal run is a segment, every
                              reference boundary b gives a collar [b - collar/2, b + collar/2), the evaluated region is the union
                              extent minus the collars (minus the reference's overlap regions with skip_overlap), both sides are
                              cropped to it, the co-occurrence durations give the mapping, and the components are summed per
                              elementary segment WITH that mapping -- a true second pass, so `correct == best` is checked, not
                              assumed

Both return the same dict: counters (8 ints: total, miss, false alarm, confusion, correct, frames kept, frames removed in
[0, T), sum of min(nr, nh)), cooc (16 x 16 int64), best (value of the optimal mapping) and mapping {hyp: ref}.  The mapping may
differ between implementations where ties exist; nothing else may.  Integer work: everything is exact.
"""
from fractions import Fraction

import numpy as np
from scipy.optimize import linear_sum_assignment

CMAX = 16

# Reference: per speaker alternating silent / active runs, lengths uniform in 1 .. off / 1 .. on (`on` is the case's longest
# run).  Hypothesis: every sub-th reference frame, Th = Tr // sub + th_delta frames (zeros beyond the reference), the columns
# rotated by one (so the optimal mapping is not the identity), `extra` more columns (negative: columns dropped), then `flips`
# runs of up to `flip_len` frames inverted at seeded places and `swaps` runs in which two columns trade places.
CASES = [
    dict(name="der_c3_T3000", seed=101, Tr=3000, Cr=3, sub=10, collar=50, on=400, off=500, th_delta=0, extra=1, flips=30, flip_len=12),
    dict(name="der_c2_T700_sub1", seed=102, Tr=700, Cr=2, sub=1, collar=10, on=90, off=110, th_delta=0, extra=0, flips=24, flip_len=25, swaps=12),
    dict(name="der_c8_sparse", seed=103, Tr=12000, Cr=8, sub=10, collar=50, on=600, off=6000, th_delta=0, extra=2, flips=60, flip_len=20),
    dict(name="der_c16_sparse", seed=104, Tr=16000, Cr=16, sub=10, collar=50, on=500, off=12000, th_delta=0, extra=0, flips=80, flip_len=20),
    dict(name="der_sub2_c4", seed=105, Tr=1501, Cr=4, sub=2, collar=4, on=60, off=150, th_delta=0, extra=1, flips=40, flip_len=15),
    dict(name="der_hyp_long", seed=106, Tr=1203, Cr=3, sub=10, collar=50, on=300, off=300, th_delta=9, extra=0, flips=12, flip_len=10),
    dict(name="der_hyp_short", seed=107, Tr=1297, Cr=3, sub=10, collar=50, on=300, off=300, th_delta=-31, extra=0, flips=12, flip_len=10),
    dict(name="der_collar0", seed=108, Tr=900, Cr=4, sub=10, collar=0, on=120, off=200, th_delta=1, extra=2, flips=20, flip_len=8),
    dict(name="der_skip_overlap", seed=109, Tr=2400, Cr=3, sub=10, collar=20, on=300, off=300, th_delta=0, extra=0, flips=25, flip_len=10,
         skip_overlap=True),
    dict(name="der_fewer_hyp", seed=110, Tr=2000, Cr=5, sub=10, collar=10, on=200, off=500, th_delta=0, extra=-2, flips=20, flip_len=10),
    dict(name="der_c16_h2", seed=111, Tr=5000, Cr=16, sub=1, collar=50, on=400, off=9000, th_delta=0, extra=-14, flips=20, flip_len=40),
]
# cases that must show every effect (asserted from the goldens' meta): between 10 % and 90 % of the frames kept; miss, false
# alarm, confusion and correct all >= 5; an optimal mapping that is not the identity; other counters than at collar 0
NON_DEGENERATE = ("der_c3_T3000", "der_c2_T700_sub1", "der_c8_sparse", "der_c16_sparse", "der_sub2_c4")


def run_track(rng, T, on, off):
    out = np.zeros(T, np.uint8)
    t, active = 0, bool(rng.integers(0, 2))
    while t < T:
        n = int(rng.integers(1, (on if active else off) + 1))
        out[t:t + n] = active
        t += n
        active = not active
    return out


def inputs(case):
    """-> (ref uint8 (Tr, Cr), hyp uint8 (Th, Ch)) of a case."""
    rng = np.random.default_rng(case["seed"])
    Tr, Cr, sub = case["Tr"], case["Cr"], case["sub"]
    ref = np.stack([run_track(rng, Tr, case["on"], case["off"]) for _ in range(Cr)], axis=1)
    Th = max(0, Tr // sub + case["th_delta"])
    hyp = np.zeros((Th, Cr), np.uint8)
    sampled = ref[::sub][:Th]
    hyp[:len(sampled)] = sampled
    hyp = np.roll(hyp, 1, axis=1)
    extra = case["extra"]
    if extra > 0:
        hyp = np.concatenate([hyp, np.zeros((Th, extra), np.uint8)], axis=1)
    elif extra < 0:
        hyp = hyp[:, :extra]
    for _ in range(case["flips"] if Th else 0):
        c, s, n = int(rng.integers(0, hyp.shape[1])), int(rng.integers(0, Th)), int(rng.integers(1, case["flip_len"] + 1))
        hyp[s:s + n, c] ^= 1
    for _ in range(case.get("swaps", 0) if Th and hyp.shape[1] > 1 else 0):
        a, b = (int(v) for v in rng.choice(hyp.shape[1], 2, replace=False))
        s, n = int(rng.integers(0, Th)), int(rng.integers(1, case["flip_len"] + 1))
        hyp[s:s + n, [a, b]] = hyp[s:s + n, [b, a]]
    return np.ascontiguousarray(ref), np.ascontiguousarray(hyp)


def _bool2d(x):
    x = np.asarray(x)
    assert x.ndim == 2
    return x != 0


def _assign(cooc):
    """Optimal one-to-one partial mapping on an integer (Cr, Ch) matrix -> (best value, {hyp: ref})."""
    if cooc.size == 0:
        return 0, {}
    ri, hj = linear_sum_assignment(cooc, maximize=True)
    mapping = {int(j): int(i) for i, j in zip(ri, hj) if cooc[i, j] > 0}
    return int(sum(cooc[i, j] for j, i in mapping.items())), mapping


def _result(total, miss, fa, conf, correct, kept, removed, both, cooc, best, mapping):
    full = np.zeros((CMAX, CMAX), np.int64)
    full[:cooc.shape[0], :cooc.shape[1]] = cooc
    return dict(counters=[int(total), int(miss), int(fa), int(conf), int(correct), int(kept), int(removed), int(both)], cooc=full,
                best=int(best), mapping=mapping)


def grid(ref, hyp, sub=10, collar=50, skip_overlap=False):
    ref, hyp = _bool2d(ref), _bool2d(hyp)
    assert collar % 2 == 0 and collar >= 0 and sub >= 1
    (Tr, Cr), (Th, Ch), h = ref.shape, hyp.shape, collar // 2
    T = max(Tr, Th * sub)
    R = np.zeros((T, Cr), bool)
    R[:Tr] = ref
    H = np.zeros((T, Ch), bool)
    H[:Th * sub] = np.repeat(hyp, sub, axis=0)
    pad = np.zeros((Tr + 2, Cr), bool)
    pad[1:-1] = ref
    D = (pad[1:] != pad[:-1]).any(axis=1)                     # D[b]: some speaker has a boundary at b, b in 0 .. Tr
    before = np.concatenate([[0], np.cumsum(D)])              # before[x]: boundaries at positions < x
    t = np.arange(T)
    lo, hi = np.clip(t - h + 1, 0, Tr + 1), np.clip(t + h + 1, 0, Tr + 1)
    removed = before[hi] - before[lo] > 0                     # a boundary b with t - h < b <= t + h
    nr, nh = R.sum(axis=1), H.sum(axis=1)
    keep = ~removed & ~(bool(skip_overlap) & (nr >= 2))
    cooc = R[keep].T.astype(np.int64) @ H[keep].astype(np.int64)
    best, mapping = _assign(cooc)
    nr, nh = nr[keep].astype(np.int64), nh[keep].astype(np.int64)
    both = np.minimum(nr, nh).sum()
    return _result(nr.sum(), np.maximum(nr - nh, 0).sum(), np.maximum(nh - nr, 0).sum(), both - best, best, keep.sum(),
                   T - keep.sum(), both, cooc, best, mapping)


def segments(act, scale=1):
    """bool (T, C) -> [(start, end, speaker), ...] of the maximal runs, as Fractions times `scale`."""
    out = []
    for c in range(act.shape[1]):
        col = np.concatenate([[0], act[:, c].astype(np.int8), [0]])
        ch = np.flatnonzero(np.diff(col))
        out += [(Fraction(int(s) * scale), Fraction(int(e) * scale), c) for s, e in zip(ch[::2], ch[1::2])]
    return out


def union(ivs):
    """Half-open intervals -> their union as sorted, disjoint, non-empty intervals."""
    out = []
    for a, b in sorted(iv for iv in ivs if iv[0] < iv[1]):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [tuple(iv) for iv in out]


def gaps(ivs, lo, hi):
    """[lo, hi) minus a union of intervals."""
    out, at = [], lo
    for a, b in ivs:
        if a > at:
            out.append((at, min(a, hi)))
        at = max(at, b)
        if at >= hi:
            break
    if at < hi:
        out.append((at, hi))
    return [iv for iv in out if iv[0] < iv[1]]


def crop(segs, region):
    return [(max(s, a), min(e, b), c) for s, e, c in segs for a, b in region if max(s, a) < min(e, b)]


def sweep(rsegs, hsegs):
    """Elementary segments of two labelled segment lists -> [(duration, reference labels, hypothesis labels), ...]."""
    cuts = sorted({x for s, e, _ in rsegs + hsegs for x in (s, e)})
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        r = frozenset(c for s, e, c in rsegs if s <= a and b <= e)
        hh = frozenset(c for s, e, c in hsegs if s <= a and b <= e)
        if r or hh:
            out.append((b - a, r, hh))
    return out


def measure(ivs):
    return sum((b - a for a, b in ivs), Fraction(0))


def interval(ref, hyp, sub=10, collar=50, skip_overlap=False):
    ref, hyp = _bool2d(ref), _bool2d(hyp)
    (Tr, Cr), (Th, Ch) = ref.shape, hyp.shape
    T = max(Tr, Th * sub)
    rsegs, hsegs = segments(ref), segments(hyp, sub)
    half = Fraction(collar, 2)
    taken = union([(b - half, b + half) for s, e, _ in rsegs for b in (s, e)])
    if skip_overlap:
        taken = union(taken + [(a, a + d) for a, d in _overlaps(rsegs)])
    both_sides = rsegs + hsegs
    region = gaps(taken, min(s for s, _, _ in both_sides), max(e for _, e, _ in both_sides)) if both_sides else []
    elementary = sweep(crop(rsegs, region), crop(hsegs, region))
    cooc = np.zeros((Cr, Ch), object)
    cooc[:] = Fraction(0)
    for d, r, hh in elementary:
        for i in r:
            for j in hh:
                cooc[i, j] += d
    assert all(v.denominator == 1 for v in cooc.flat)
    cooc = np.array([[int(v) for v in row] for row in cooc], np.int64).reshape(Cr, Ch)
    best, mapping = _assign(cooc)
    total = miss = fa = conf = correct = both = Fraction(0)
    for d, r, hh in elementary:                                # matching per elementary segment, with the mapping
        nr, nh = len(r), len(hh)
        hit = sum(1 for j in hh if mapping.get(j, -1) in r)
        total += d * nr
        miss += d * max(0, nr - nh)
        fa += d * max(0, nh - nr)
        correct += d * hit
        conf += d * (min(nr, nh) - hit)
        both += d * min(nr, nh)
    removed = measure([(max(a, Fraction(0)), min(b, Fraction(T))) for a, b in taken if max(a, 0) < min(b, T)])
    vals = (total, miss, fa, conf, correct, T - removed, removed, both)
    assert all(Fraction(v).denominator == 1 for v in vals)
    return _result(*vals, cooc, best, mapping)


def _overlaps(rsegs):
    """(start, duration) of the stretches with two or more reference speakers."""
    cuts = sorted({x for s, e, _ in rsegs for x in (s, e)})
    return [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:]) if sum(1 for s, e, _ in rsegs if s <= a and b <= e) >= 2]


def valid_mapping(mapping, cooc, best):
    """One-to-one, every mapped pair co-occurs, and the pairs add up to the optimal value."""
    refs = list(mapping.values())
    return (len(set(refs)) == len(refs) and all(cooc[i][j] > 0 for j, i in mapping.items())
            and sum(int(cooc[i][j]) for j, i in mapping.items()) == best)


def from_runs(T, runs_per_speaker):
    """[[(start, end), ...] per speaker] -> uint8 (T, C)."""
    out = np.zeros((T, len(runs_per_speaker)), np.uint8)
    for c, runs in enumerate(runs_per_speaker):
        for s, e in runs:
            out[s:e, c] = 1
    return out


# the two hand-sized cases: (ref, hyp, sub)
HAND_A = (from_runs(20, [[(5, 15)]]), from_runs(20, [[(7, 17)]]), 1)
HAND_B = (from_runs(12, [[(0, 6)], [(4, 12)]]), from_runs(8, [[(2, 8)], [(0, 3)], [(7, 8)]]), 2)


def random_small(rng):
    """A small random case for the sweep: (ref, hyp, sub, collar, skip_overlap)."""
    sub = int(rng.choice([1, 2, 10]))
    collar = int(rng.choice([0, 2, 4, 10, 50]))
    Cr, Ch = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    Tr = int(rng.integers(0, 90))
    Th = max(0, Tr // sub + int(rng.integers(-3, 4)))
    ref = np.stack([run_track(rng, Tr, 20, 25) for _ in range(Cr)], axis=1) if Tr else np.zeros((0, Cr), np.uint8)
    hyp = np.stack([run_track(rng, Th, max(1, 20 // sub), max(1, 25 // sub)) for _ in range(Ch)], axis=1) if Th else np.zeros((0, Ch), np.uint8)
    if rng.random() < 0.1:
        ref[:] = 0
    if rng.random() < 0.1:
        hyp[:] = 0
    return ref, hyp, sub, collar, bool(rng.integers(0, 2))
