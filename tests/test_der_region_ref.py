"""CPU: the restatement of tests/der_region_ref.py against hand-worked cases, the RTTM / UEM parsers of fs_eend_amd.metrics against
literal tables, the argument checks of the new keywords (no device needed), and the assignment gap of every seeded JER case that
tests/test_der_region_gpu.py compares pairings on."""
import io

import numpy as np
import pytest
import torch

from tests import der_ref as R
from tests import der_region_ref as Q


@pytest.fixture(scope="module")
def M():
    from fs_eend_amd import metrics
    return metrics


def one(T, runs):
    return R.from_runs(T, [runs])


# ---- the region rule, by hand

def test_boundary_outside_a_region_reaches_in():
    """ref active in [10, 20): boundaries at 10 and 20.  Region [21, 30), half collar 2: the boundary at 20 lies outside the
    region and still removes frame 21 (21 - 2 < 20); the region's own edges at 21 and 30 remove nothing."""
    ref, hyp = one(40, [(10, 20)]), one(40, [(0, 40)])
    got = Q.region(ref, hyp, [(21, 30)], sub=1, collar=4)
    assert got["counters"] == [0, 0, 8, 0, 0, 8, 32, 0]             # frames 22 .. 29: false alarm only
    assert got["ref_time"][0] == 0 and got["hyp_time"][0] == 8
    assert Q.region(ref, hyp, [(21, 30)], sub=1, collar=0)["counters"][5] == 9


def test_region_edge_is_not_a_boundary_and_masking_is_no_substitute():
    """ref active throughout: boundaries at 0 and 40 only.  Region [10, 30), half collar 2: all 20 frames are kept.  Zeroing the
    activity outside the region instead puts boundaries at 10 and 30, loses 2 frames inside at each, and calls 32 frames kept."""
    ref, hyp = one(40, [(0, 40)]), one(40, [(0, 40)])
    uem = [(10, 30)]
    got = Q.region(ref, hyp, uem, sub=1, collar=4)
    assert got["counters"] == [20, 0, 0, 0, 20, 20, 20, 20] and got["ref_time"][0] == 20 and got["hyp_time"][0] == 20
    wrong = R.grid(Q.masked(ref, uem), Q.masked(hyp, uem), 1, 4)
    assert wrong["counters"][0] == 16 and wrong["counters"][5] == 32
    assert wrong["counters"] != got["counters"]


def test_skip_overlap_with_regions():
    ref = R.from_runs(30, [[(0, 20)], [(10, 30)]])
    hyp = R.from_runs(30, [[(0, 30)]])
    got = Q.region(ref, hyp, [(5, 25)], sub=1, collar=0, skip_overlap=True)
    # frames 5 .. 9 (speaker 0) and 20 .. 24 (speaker 1); the one hypothesis speaker maps to one of them: 5 correct, 5 confused
    assert got["counters"] == [10, 0, 0, 5, 5, 10, 20, 10]
    assert got["ref_time"][:2] == [5, 5] and got["hyp_time"][0] == 10
    assert got["cooc"][:2, 0].tolist() == [5, 5] and got["best"] == 5
    keep_all = Q.region(ref, hyp, [(5, 25)], sub=1, collar=0)
    assert keep_all["counters"][:3] == [30, 10, 0] and keep_all["counters"][5] == 20


def test_empty_uem_and_uem_past_the_end():
    ref, hyp = one(40, [(5, 35)]), one(4, [(0, 4)])
    got = Q.region(ref, hyp, [], sub=10, collar=0)
    assert got["counters"] == [0, 0, 0, 0, 0, 0, 40, 0] and sum(got["ref_time"]) == 0 and sum(got["hyp_time"]) == 0
    got = Q.region(ref, hyp, [(10, 1000)], sub=10, collar=0)
    assert got["counters"][:3] == [25, 0, 5] and got["counters"][5:7] == [30, 10]
    assert Q.region(ref, hyp, [(0, 1000)], sub=10, collar=4)["counters"] == Q.region(ref, hyp, None, sub=10, collar=4)["counters"]


def test_without_regions_the_restatement_is_the_grid():
    rng = np.random.default_rng(2024)
    for _ in range(60):
        ref, hyp, sub, collar, skip = R.random_small(rng)
        want = R.grid(ref, hyp, sub, collar, skip)
        T = max(ref.shape[0], hyp.shape[0] * sub)
        for uem in (None, [(0, max(T, 1))]):
            got = Q.region(ref, hyp, uem, sub, collar, skip)
            assert got["counters"] == want["counters"] and np.array_equal(got["cooc"], want["cooc"])
            assert sum(got["ref_time"]) == want["counters"][0]                          # the sum of nr over the kept frames
            assert sum(got["hyp_time"]) == want["counters"][2] + want["counters"][7]   # ... and of nh: false alarm + sum of min
        lo, hi = sorted(int(v) for v in rng.integers(0, T + 2, 2))
        if lo < hi:                                                  # kept frames of a region are kept frames without it
            part = Q.region(ref, hyp, [(lo, hi)], sub, collar, skip)
            assert part["counters"][5] <= min(want["counters"][5], hi - lo) and part["counters"][5] + part["counters"][6] == T


def test_marginals_by_hand():
    ref = R.from_runs(12, [[(0, 6)], [(4, 12)]])
    hyp = R.from_runs(6, [[(1, 4)], [(0, 6)]])                       # sub 2
    got = Q.region(ref, hyp, [(2, 10)], sub=2, collar=0)
    assert got["ref_time"][:2] == [4, 6] and got["hyp_time"][:2] == [6, 8]
    assert got["cooc"][:2, :2].tolist() == [[4, 4], [4, 6]]


# ---- JER by hand, and the gaps of the seeded cases

def test_jer_by_hand():
    cooc = np.zeros((16, 16), np.int64)
    cooc[0, 1], cooc[1, 0], cooc[0, 0] = 8, 5, 2
    rt, ht = [10, 10, 4] + [0] * 13, [6, 9] + [0] * 14
    j = Q.jer(cooc, rt, ht)
    assert j["pairing"] == {0: 1, 1: 0}
    assert j["speakers"] == {0: (10, 9, 8), 1: (10, 6, 5), 2: (4, 0, 0)}
    assert j["rates"] == {0: 3 / 11, 1: 6 / 11, 2: 1.0}
    assert abs(j["total"] - (3 / 11 + 6 / 11 + 1.0)) < 1e-15 and abs(j["rate"] - j["total"] / 3) < 1e-15
    best, second = Q.pairing_gap(cooc, rt, ht)
    assert abs(best - j["total"]) < 1e-15 and second > best + 0.1
    # no reference speaker: 0.0 without hypothesis time, 1.0 with; a zero-intersection pair is not reported
    assert Q.jer(cooc * 0, [0] * 16, [0] * 16)["rate"] == 0.0 and Q.jer(cooc * 0, [0] * 16, [3] + [0] * 15)["rate"] == 1.0
    lone = Q.jer(cooc * 0, [5] + [0] * 15, [3] + [0] * 15)
    assert lone["pairing"] == {} and lone["speakers"] == {0: (5, 0, 0)} and lone["rate"] == 1.0


@pytest.mark.parametrize("case", Q.JER_CASES, ids=[c["name"] for c in Q.JER_CASES])
def test_every_seeded_jer_case_has_a_unique_pairing(case):
    """The GPU test compares pairings on all of Q.JER_CASES, so all of them must have the gap: none is left out."""
    _, _, want = Q.jer_case_reference(case)
    best, second = Q.pairing_gap(want["cooc"], want["ref_time"], want["hyp_time"])
    j = Q.jer(want["cooc"], want["ref_time"], want["hyp_time"])
    assert abs(best - j["total"]) <= 1e-12 * max(1, len(j["speakers"]))
    assert second - best >= Q.MIN_GAP
    assert len(j["speakers"]) >= 2 and 0.0 < j["rate"] < 1.0 and want["counters"][5] > 100


# ---- the parsers

def test_read_rttm_and_uem_tables(M, tmp_path):
    assert M.read_rttm(Q.RTTM_TEXT) == Q.RTTM_WANT
    assert M.read_uem(Q.UEM_TEXT) == Q.UEM_WANT
    assert M.read_rttm(io.StringIO("\n".join(Q.RTTM_TEXT) + "\n")) == Q.RTTM_WANT
    p = tmp_path / "ref.rttm"
    p.write_text("\n".join(Q.RTTM_TEXT) + "\n")
    assert M.read_rttm(str(p)) == Q.RTTM_WANT and M.read_rttm(p) == Q.RTTM_WANT
    u = tmp_path / "all.uem"
    u.write_text("\n".join(Q.UEM_TEXT) + "\n")
    assert M.read_uem(u) == Q.UEM_WANT
    first = M.read_rttm(Q.RTTM_TEXT)["rec1"]["speakers"]
    assert first == ["bob", "alice"]                                 # first appearance, not sorted


def test_rounding_at_half_a_frame(M):
    for t, want in Q.HALF_FRAMES:
        assert int(np.rint(t * 100.0)) == want
        got = M.read_rttm([f"SPEAKER r 1 {t!r} 1.0 <NA> <NA> s <NA>"])["r"]["segments"][0]
        assert got[1] == want and got[2] == int(np.rint((t + 1.0) * 100.0))
    # another rate: the model's 10 frames per second
    assert M.read_rttm(["SPEAKER r 1 0.25 0.5 <NA> <NA> s <NA>"], frame_rate=10.0)["r"]["segments"] == [(0, 2, 8)]


def test_parser_refusals(M):
    for line in Q.RTTM_REFUSED:
        with pytest.raises(ValueError, match="RTTM line 2"):
            M.read_rttm([Q.RTTM_TEXT[0], line])
    for line in Q.UEM_REFUSED:
        with pytest.raises(ValueError, match="UEM line 3"):
            M.read_uem(Q.UEM_TEXT[:2] + [line])
    many = [f"SPEAKER r 1 {i}.0 0.5 <NA> <NA> spk{i} <NA>" for i in range(17)]
    assert len(M.read_rttm(many[:16])["r"]["speakers"]) == 16
    with pytest.raises(ValueError, match="RTTM line 17"):
        M.read_rttm(many)
    assert M.read_rttm(many[:16] + ["SPEAKER other 1 0.0 0.5 <NA> <NA> spk16 <NA>"])["other"]["speakers"] == ["spk16"]


def test_round_trip_through_rttm_lines(M):
    from fs_eend_amd import postproc
    segs = [[(3, 17), (40, 41), (1234, 5678)], [], [(0, 5), (17, 40)]]
    lines = [ln for spk in postproc.rttm_lines("rec", segs).values() for ln in spk]
    got = M.read_rttm(lines, frame_rate=10.0)["rec"]                 # rttm_lines writes model frames of 0.1 s
    assert got["speakers"] == ["rec_0", "rec_2"]
    assert got["segments"] == [(0, 3, 17), (0, 40, 41), (0, 1234, 5678), (1, 0, 5), (1, 17, 40)]
    at_label_rate = M.read_rttm(lines)["rec"]["segments"]
    assert at_label_rate == [(c, 10 * s, 10 * e) for c, s, e in got["segments"]]
    assert M.rttm_lengths(["rec", "absent"], {"rec": got}, {"rec": [(0, 9000)]}, [7000, 3]) == [9000, 3]
    assert np.array_equal(Q.raster(got["segments"][:2], 50, 2)[:, 0].nonzero()[0], list(range(3, 17)) + [40])


# ---- the argument checks of the new keywords: refused before any device is needed

BAD_UEMS = [[(-1, 5)], [(5, 5)], [(7, 3)], [(1.5, 3)], [(0, 4, 5)], [3], torch.tensor([[0.0, 4.0]]), torch.tensor([1, 2, 3]), [(True, 2)]]


@pytest.mark.parametrize("uem", BAD_UEMS, ids=[str(i) for i in range(len(BAD_UEMS))])
def test_uem_is_checked_on_the_host(M, uem):
    ref, hyp, pred = torch.zeros(50, 2), torch.zeros(5, 2), torch.rand(5, 2)
    calls = [lambda: M.collar_der(ref, hyp, uem=uem), lambda: M.collar_der_counters([ref], [hyp], uem=[uem]),
             lambda: M.collar_der_counters(ref, hyp, uem=uem), lambda: M.score_predictions(ref, pred, uem=uem),
             lambda: M.sweep_counters([ref], [pred], [0.5], [1], uem=[uem]), lambda: M.sweep_predictions(ref, pred, uem=uem),
             lambda: M.DerSweep().add([ref], [pred], uem=[uem]), lambda: M.jaccard_error(ref, hyp, uem=uem),
             lambda: M.jaccard_error_counters([ref], [hyp], uem=[uem]), lambda: M.CollarDER()(ref, hyp, uem=uem),
             lambda: M.CollarDER().score_batch([ref], [hyp], uems=[uem]), lambda: M.JaccardER()(ref, hyp, uem=uem),
             lambda: M.JaccardER().score_batch([ref], [hyp], uems=[uem]), lambda: M.pack_uem([uem], torch.device("cpu"))]
    for call in calls:
        with pytest.raises(ValueError):
            call()


def test_uem_list_must_match_the_batch(M):
    ref, hyp = torch.zeros(50, 2), torch.zeros(5, 2)
    for bad in ([[(0, 5)]], [None, None, None], (0, 5)):
        with pytest.raises(ValueError):
            M.collar_der_counters([ref, ref], [hyp, hyp], uem=bad)
    with pytest.raises(ValueError):
        M.jaccard_error(ref, hyp, collar=3)
    with pytest.raises(ValueError):
        M.JaccardER(subsampling=0)


def test_uem_is_sorted_and_merged_on_the_host(M):
    table, off = M.pack_uem([None, [(30, 40), (0, 10), (10, 20), (35, 50)], [], torch.tensor([[5, 6]], dtype=torch.int64)],
                            torch.device("cpu"))
    assert off.tolist() == [0, 1, 3, 3, 4] and table.dtype == torch.int32
    assert table.tolist() == [[0, 2 ** 31 - 1], [0, 20], [30, 50], [5, 6]]
    empty, off = M.pack_uem([[]], torch.device("cpu"))
    assert off.tolist() == [0, 0] and empty.shape == (1, 2)          # never an empty allocation


def test_segments_raster_refusals(M):
    for tables, lengths in (([[(0, 0, 5)]], [4]), ([[(16, 0, 2)]], [4]), ([[(0, -1, 2)]], [4]), ([[]], [-1]), ([[]], [1, 2])):
        with pytest.raises(ValueError):
            M.segments_raster(tables, lengths)
