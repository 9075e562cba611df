"""Test helper (not a test module): a frame-by-frame integer restatement of what include/eend_hip.h states at
eend_collar_der_regions_u64, eend_jer_assign_f64 and eend_segments_raster_u8 -- scoring regions (UEM), the two marginal times and
the Jaccard error rate -- with the seeded cases the GPU tests use and the RTTM / UEM parsing expectations as literal tables.

    region(ref, hyp, uem, ...)   one Python loop over the frames of [0, T): in a region? clear of every collar of the uncropped
                                 reference? fewer than two reference speakers (skip_overlap)?  Then the counts of that frame.
                                 Nothing of the rule is vectorised; tests/der_ref.py supplies the assignment and the result form.
    jer(cooc, ref_time, hyp_time)   the per-speaker integers, the float64 cost matrix and scipy's linear_sum_assignment on it
    pairing_gap(...)             all assignments enumerated: the best total against the best total of any other reported pairing

pyannote and dscore are not needed and never imported; no equality with either tool is claimed.
"""
import itertools

import numpy as np
from scipy.optimize import linear_sum_assignment

from tests import der_ref as R

CMAX = R.CMAX


def in_regions(t, uem):
    """uem None: everywhere; else half-open (s, e) pairs in any order."""
    if uem is None:
        return True
    for s, e in uem:
        if s <= t < e:
            return True
    return False


def region(ref, hyp, uem=None, sub=10, collar=50, skip_overlap=False):
    """-> der_ref's result dict (counters, cooc, best, mapping) plus ref_time and hyp_time (lists of 16)."""
    ref, hyp = np.asarray(ref) != 0, np.asarray(hyp) != 0
    (Tr, Cr), (Th, Ch), h = ref.shape, hyp.shape, collar // 2
    T = max(Tr, Th * sub)
    boundary = [False] * (Tr + 2)                                  # boundary[b], b in 0 .. Tr, of the uncropped reference
    for b in range(Tr + 1):
        for s in range(Cr):
            before = bool(ref[b - 1, s]) if b >= 1 else False
            after = bool(ref[b, s]) if b < Tr else False
            if before != after:
                boundary[b] = True
    below = [0]                                                    # below[x]: boundaries at positions < x
    for b in range(Tr + 1):
        below.append(below[-1] + (1 if boundary[b] else 0))
    clip = lambda x: min(max(x, 0), Tr + 1)
    total = miss = fa = both = kept = 0
    cooc = np.zeros((Cr, Ch), np.int64)
    ref_time, hyp_time = [0] * CMAX, [0] * CMAX
    for t in range(T):
        if not in_regions(t, uem):
            continue
        if below[clip(t + h + 1)] - below[clip(t - h + 1)] > 0:   # a boundary b with t - h < b <= t + h
            continue
        rs = [s for s in range(Cr) if t < Tr and ref[t, s]]
        if skip_overlap and len(rs) >= 2:
            continue
        k = t // sub
        hs = [j for j in range(Ch) if k < Th and hyp[k, j]]
        kept += 1
        total += len(rs)
        miss += max(0, len(rs) - len(hs))
        fa += max(0, len(hs) - len(rs))
        both += min(len(rs), len(hs))
        for i in rs:
            ref_time[i] += 1
            for j in hs:
                cooc[i, j] += 1
        for j in hs:
            hyp_time[j] += 1
    best, mapping = R._assign(cooc)
    out = R._result(total, miss, fa, both - best, best, kept, T - kept, both, cooc, best, mapping)
    out["ref_time"], out["hyp_time"] = ref_time, hyp_time
    return out


def masked(ref, uem):
    """The wrong substitute: the activity zeroed outside the regions."""
    out = np.array(ref, copy=True)
    for t in range(out.shape[0]):
        if not in_regions(t, uem):
            out[t] = 0
    return out


# ---- Jaccard error rate

def jer_costs(cooc, ref_time, hyp_time):
    """-> (reference speakers with kept time, hypothesis speakers with kept time, float64 cost matrix over them)."""
    rs = [i for i in range(CMAX) if ref_time[i] > 0]
    hs = [j for j in range(CMAX) if hyp_time[j] > 0]
    cost = np.ones((len(rs), len(hs)), np.float64)
    for a, i in enumerate(rs):
        for b, j in enumerate(hs):
            inter = int(cooc[i][j])
            cost[a, b] = 1.0 - inter / (ref_time[i] + hyp_time[j] - inter)
    return rs, hs, cost


def jer(cooc, ref_time, hyp_time):
    """-> dict: speakers {ref: (ref_time, paired hyp_time or 0, inter)}, pairing {ref: hyp} (pairs with inter = 0 left out), total
    (the minimal sum of costs, an unpaired reference speaker costing 1), rate (per the convention of metrics.rate)."""
    rs, hs, cost = jer_costs(cooc, ref_time, hyp_time)
    speakers = {i: (int(ref_time[i]), 0, 0) for i in rs}
    pairing, total = {}, float(len(rs))
    if rs and hs:
        ai, bj = linear_sum_assignment(cost)
        total = float(cost[ai, bj].sum()) + (len(rs) - len(ai))
        for a, b in zip(ai, bj):
            i, j = rs[a], hs[b]
            if cooc[i][j] > 0:
                pairing[i] = j
                speakers[i] = (int(ref_time[i]), int(hyp_time[j]), int(cooc[i][j]))
    rates = {}
    for i, (rt, ht, inter) in speakers.items():
        union = rt + ht - inter
        rates[i] = (union - inter) / union
    rate = sum(rates.values()) / len(rs) if rs else (1.0 if hs else 0.0)
    return dict(speakers=speakers, pairing=pairing, total=total, rates=rates, rate=rate)


def pairing_gap(cooc, ref_time, hyp_time):
    """Every one-to-one assignment of the padded square enumerated -> (best total, the best total among the assignments that
    report another pairing) ; the second is inf if every assignment reports the same pairing.  Reported: pairs of existing
    speakers with inter > 0."""
    rs, hs, cost = jer_costs(cooc, ref_time, hyp_time)
    n = max(len(rs), len(hs))
    assert n <= 7, "enumeration is for small speaker counts"
    by_pairing = {}
    for perm in itertools.permutations(range(n)):
        total, rep = 0.0, []
        for a in range(len(rs)):
            b = perm[a]
            if b < len(hs):
                total += cost[a, b]
                if cooc[rs[a]][hs[b]] > 0:
                    rep.append((rs[a], hs[b]))
            else:
                total += 1.0
        key = tuple(rep)
        by_pairing[key] = min(by_pairing.get(key, np.inf), total)
    totals = sorted(by_pairing.values())
    return totals[0], (totals[1] if len(totals) > 1 else np.inf)


def tracks(seed, T, C, on=40, off=60):
    rng = np.random.default_rng(seed)
    return np.stack([R.run_track(rng, T, on, off) for _ in range(C)], axis=1) if T else np.zeros((0, C), np.uint8)


# Seeded JER cases, small enough to enumerate: reference tracks, the hypothesis = every sub-th reference frame with the columns
# rotated, `extra` silent-or-noisy columns more (negative: fewer), and runs flipped at seeded places.  `uem`: regions or None.
JER_CASES = [
    dict(name="jer_c3", seed=301, Tr=900, Cr=3, sub=10, collar=0, extra=1, flips=25, uem=None),
    dict(name="jer_c4_regions", seed=302, Tr=1500, Cr=4, sub=10, collar=0, extra=0, flips=30, uem=[(100, 700), (800, 1450)]),
    dict(name="jer_c2_collar", seed=303, Tr=700, Cr=2, sub=1, collar=10, extra=2, flips=20, uem=None),
    dict(name="jer_c5_fewer_hyp", seed=304, Tr=1200, Cr=5, sub=10, collar=0, extra=-2, flips=20, uem=[(0, 1100)]),
    dict(name="jer_c3_skip", seed=305, Tr=1100, Cr=3, sub=2, collar=4, extra=1, flips=30, uem=[(50, 1000)], skip_overlap=True),
]
MIN_GAP = 1e-9


def jer_inputs(case):
    rng = np.random.default_rng(case["seed"])
    Tr, Cr, sub = case["Tr"], case["Cr"], case["sub"]
    ref = np.stack([R.run_track(rng, Tr, 90, 120) for _ in range(Cr)], axis=1)
    hyp = np.roll(ref[::sub], 1, axis=1).copy()
    Th = hyp.shape[0]
    if case["extra"] > 0:
        hyp = np.concatenate([hyp, np.zeros((Th, case["extra"]), np.uint8)], axis=1)
    elif case["extra"] < 0:
        hyp = hyp[:, :case["extra"]].copy()
    for _ in range(case["flips"]):
        c, s, n = int(rng.integers(0, hyp.shape[1])), int(rng.integers(0, Th)), int(rng.integers(1, max(2, 60 // sub)))
        hyp[s:s + n, c] ^= 1
    return np.ascontiguousarray(ref), np.ascontiguousarray(hyp)


def jer_case_reference(case):
    ref, hyp = jer_inputs(case)
    want = region(ref, hyp, case["uem"], case["sub"], case["collar"], case.get("skip_overlap", False))
    return ref, hyp, want


# ---- the rasteriser

def raster(table, length, C):
    """[(speaker, start, end), ...] -> uint8 (length, C), one store per segment and frame."""
    out = np.zeros((length, C), np.uint8)
    for spk, s, e in table:
        for t in range(s, e):
            out[t, spk] = 1
    return out


# ---- RTTM and UEM text with what the parsers must make of it, at 100 frames per second

RTTM_TEXT = """\
SPEAKER rec1 1 0.00 1.00 <NA> <NA> bob <NA> <NA>
SPEAKER rec1 1 0.50 1.25 <NA> <NA> alice <NA> <NA>
SPKR-INFO rec1 1 <NA> <NA> <NA> unknown bob <NA> <NA>
SPEAKER rec2 1 2.005 0.010 <NA> <NA> zed <NA> <NA>
SPEAKER rec1 1 3.015 0.020 <NA> <NA> bob <NA> <NA>
SPEAKER rec2 1 0.125 0.000 <NA> <NA> amy <NA> <NA>
""".splitlines()
# in float64 2.005 * 100 = 200.5 -> 200 and 3.015 * 100 = 301.5 -> 302 (half to even), (2.005 + 0.010) * 100 = 201.49999999999997
# -> 201, 3.035 * 100 = 303.5 -> 304; 0.125 * 100 = 12.5 -> 12 at both ends, an empty segment that still names amy
RTTM_WANT = {
    "rec1": {"speakers": ["bob", "alice"], "segments": [(0, 0, 100), (1, 50, 175), (0, 302, 304)]},
    "rec2": {"speakers": ["zed", "amy"], "segments": [(0, 200, 201), (1, 12, 12)]},
}
HALF_FRAMES = [(0.005, 0), (0.015, 2), (0.025, 2), (0.035, 4), (0.125, 12), (0.135, 14)]   # np.rint(t * 100.0): half to even

UEM_TEXT = """\
rec1 1 0.000 1.000
rec1 1 2.500 3.000
rec1 1 1.000 1.500
rec2 1 0.125 0.135
rec2 1 0.200 0.204
""".splitlines()
UEM_WANT = {"rec1": [(0, 150), (250, 300)], "rec2": [(12, 14)]}   # touching intervals merge; (20, 20) is empty and dropped

RTTM_REFUSED = [
    "SPEAKER rec1 1 0.00",                                         # too few fields
    "SPEAKER rec1 1 zero 1.00 <NA> <NA> bob <NA>",                 # not a number
    "SPEAKER rec1 1 nan 1.00 <NA> <NA> bob <NA>",                  # not finite
    "SPEAKER rec1 1 -0.10 1.00 <NA> <NA> bob <NA>",                # negative start
    "SPEAKER rec1 1 0.10 -1.00 <NA> <NA> bob <NA>",                # negative duration
    "SPEAKER rec1 1 30000000.0 1.00 <NA> <NA> bob <NA>",           # a frame beyond MAX_FRAMES
    "hello",                                                       # not a record at all
]
UEM_REFUSED = [
    "rec1 1 0.0",                                                  # too few fields
    "rec1 1 0.0 x",                                                # not a number
    "rec1 1 -1.0 2.0",                                             # negative time
    "rec1 1 2.0 1.0",                                              # end before start
    "rec1 1 0.0 30000000.0",                                       # a frame beyond MAX_FRAMES
]
