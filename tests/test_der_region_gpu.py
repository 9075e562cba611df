"""GPU: scoring regions, marginal times, the Jaccard error rate and the RTTM rasteriser (csrc/der_tile.h region_fill,
csrc/der_collar.hip, csrc/der_sweep.hip, csrc/segraster.hip behind fs_eend_amd.metrics) against the frame-by-frame restatement of
tests/der_region_ref.py.  Integer work: every comparison of counts is exact.  DER mappings are checked for validity, never
against scipy's choice; JER pairings are compared because tests/test_der_region_ref.py shows every seeded case has one optimum."""
import numpy as np
import pytest
import torch

from tests import der_ref as R
from tests import der_region_ref as Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(hip_lib, dev):
    from fs_eend_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def lim(M):
    return M.limits()                                                # (TILE, HMAX)


def tt(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def run(M, dev, refs, hyps, uems, sub, collar, skip=False):
    """-> per recording (counters, cooc, mapping {hyp: ref}, ref_time, hyp_time) through eend_collar_der_regions_u64"""
    batch = M.pack([tt(r) for r in refs], [tt(h) for h in hyps], sub)
    table = M.pack_uem(uems, dev) if uems is not None else None
    out = M.collar_der_regions_packed(batch, table, collar, sub, skip)
    assert all(t.is_cuda for t in out) and out[3].dtype == torch.int64 and out[3].shape == (len(refs), 16) == out[4].shape
    counters, cooc, mapping, rt, ht = (t.cpu() for t in out)
    return [(counters[b].tolist(), cooc[b].numpy(), {j: i for j, i in enumerate(mapping[b].tolist()) if i >= 0}, rt[b].tolist(),
             ht[b].tolist()) for b in range(len(refs))]


def agrees(got, want, Ch):
    counters, cooc, mapping, rt, ht = got
    assert counters == want["counters"]
    assert np.array_equal(cooc, want["cooc"])
    assert rt == want["ref_time"] and ht == want["hyp_time"]
    assert all(j < Ch for j in mapping) and R.valid_mapping(mapping, cooc, want["best"])


def check(M, dev, refs, hyps, uems, sub, collar, skip=False):
    got = run(M, dev, refs, hyps, uems, sub, collar, skip)
    for g, r, h, u in zip(got, refs, hyps, uems if uems is not None else [None] * len(refs)):
        agrees(g, Q.region(r, h, u, sub, collar, skip), h.shape[1])
    return got


# ---- regions at the pass's edges

def edge_uems(TILE, T):
    return [
        [(TILE - 1, TILE)], [(TILE, TILE + 1)], [(TILE - 1, TILE + 1)], [(0, TILE - 1), (TILE + 1, 2 * TILE)], [(5, TILE)],   # tile edges
        [(63, 64)], [(64, 65)], [(10, 63)], [(10, 64)], [(10, 65)], [(63, 129), (TILE + 64, TILE + 128)],                    # ballot words
        [(100, 2 * TILE + 20)],                                                                                            # three tiles
        [(TILE + 10 + 2 * k, TILE + 11 + 2 * k) for k in range(300)],                                                      # 300 in a tile
        [(2 * TILE - 3, T + 1000)],                                                                                        # past T
        [],
        None,
    ]


@pytest.mark.parametrize("sub,half,skip", [(1, 0, False), (10, 25, True), (1, 25, False), (10, "tile", False)])
def test_regions_at_tile_and_word_edges(M, dev, lim, sub, half, skip):
    TILE, HMAX = lim
    half = min(TILE + 3, HMAX) if half == "tile" else half
    T = 2 * TILE + 40
    # a collar wider than a tile leaves frames only far from every boundary: one speaker who never stops has them at 0 and T
    ref = Q.tracks(11, T, 3, on=70, off=90) if half <= 25 else R.from_runs(T, [[], [(0, T)], []])
    hyp = Q.tracks(12, -(-T // sub), 2, on=max(2, 70 // sub), off=max(2, 90 // sub))
    uems = edge_uems(TILE, T)
    got = check(M, dev, [ref] * len(uems), [hyp] * len(uems), uems, sub, 2 * half, skip)
    Tall = max(T, hyp.shape[0] * sub)                              # the hypothesis's last frame may reach beyond the reference
    assert got[-2][0] == [0, 0, 0, 0, 0, 0, Tall, 0] and sum(got[-2][3]) == 0 and sum(got[-2][4]) == 0   # the empty list
    if half == 0 and not skip:
        assert got[12][0][5] == 300 and got[0][0][5] == 1 and got[11][0][5] == 2 * TILE - 80
    assert any(g[0][0] > 0 for g in got) and any(sum(g[4]) > 0 for g in got) and 0 < got[-1][0][5] <= Tall


def test_ragged_batch_with_every_kind_of_uem(M, dev, lim):
    TILE, _ = lim
    lens = [1, TILE - 1, 2 * TILE + 1, 5]
    refs = [Q.tracks(20 + i, n, 2 + i, on=30, off=40) for i, n in enumerate(lens)]
    many = [(3 * k, 3 * k + 2) for k in range(0, (2 * TILE + 1) // 3, 2)]
    for sub in (1, 10):
        hyps = [Q.tracks(30 + i, -(-n // sub) + (i == 3), 5 - i, on=max(2, 30 // sub), off=max(2, 40 // sub)) for i, n in enumerate(lens)]
        for uems in ([None, [], many, [(1, 4)]], [[(0, 1)], [(TILE - 2, TILE + 5)], None, []]):
            for collar in (0, 50):
                check(M, dev, refs, hyps, uems, sub, collar)
    check(M, dev, refs, hyps, [None, [], many, [(1, 4)]], 10, 50, True)


def test_widths_with_regions(M, dev):
    wide, one = Q.tracks(40, 300, 16, on=20, off=200), Q.tracks(41, 300, 1, on=50, off=50)
    uem = [(7, 130), (150, 290)]
    check(M, dev, [wide, one], [one[::10], wide[::10]], [uem, uem], 10, 10)      # 16 x 1 and 1 x 16 in one batch
    check(M, dev, [wide], [one[::10]], [uem], 10, 0)
    check(M, dev, [one], [wide], [uem], 1, 4, True)


def test_region_rule_by_hand(M, dev):
    """The two hand cases of tests/test_der_region_ref.py, on the device, and the wrong substitute next to them."""
    ref, hyp = R.from_runs(40, [[(10, 20)]]), R.from_runs(40, [[(0, 40)]])
    assert run(M, dev, [ref], [hyp], [[(21, 30)]], 1, 4)[0][0] == [0, 0, 8, 0, 0, 8, 32, 0]
    full = R.from_runs(40, [[(0, 40)]])
    assert run(M, dev, [full], [full], [[(10, 30)]], 1, 4)[0][0] == [20, 0, 0, 0, 20, 20, 20, 20]
    d = M.collar_der(tt(full), tt(full), collar=4, subsampling=1, uem=[(10, 30)])
    assert d["total"] == 20 and d["frames kept"] == 20 and d["frames removed"] == 20 and d["diarization error rate"] == 0.0
    wrong = M.collar_der(tt(Q.masked(full, [(10, 30)])), tt(Q.masked(full, [(10, 30)])), collar=4, subsampling=1)
    assert wrong["total"] == 16 and wrong["frames kept"] == 32
    metric = M.CollarDER(collar=4, subsampling=1)
    assert metric(tt(full), tt(full), uem=torch.tensor([[10, 30]])) == 0.0
    assert [r["total"] for r in metric.score_batch([tt(full), tt(ref)], [tt(full), tt(hyp)], uems=[None, [(21, 30)]])] == [36, 0]
    assert metric.report()["total"] == 56 and metric.report()["false alarm"] == 8


# ---- the unchanged path

def test_no_regions_is_the_existing_entry(M, dev, lim):
    TILE, _ = lim
    refs = [tt(Q.tracks(50 + i, n, 3, on=60, off=80)) for i, n in enumerate((TILE + 5, 700, 2 * TILE))]
    hyps = [tt(Q.tracks(60 + i, -(-r.shape[0] // 10), 4, on=6, off=8)) for i, r in enumerate(refs)]
    batch = M.pack(refs, hyps, 10)
    for collar, skip in ((50, False), (0, True)):
        old = M.collar_der_packed(batch, collar, 10, skip)
        whole = [[(0, max(r.shape[0], h.shape[0] * 10))] for r, h in zip(refs, hyps)]        # exactly [0, T), T = max(Tr, Th sub)
        for uem in (None, M.pack_uem([None] * 3, dev), M.pack_uem(whole, dev)):
            new = M.collar_der_regions_packed(batch, uem, collar, 10, skip)
            assert all(torch.equal(a, b) for a, b in zip(old, new[:3]))
            assert new[3].sum().item() == old[0][:, 0].sum().item()
            via = M.collar_der_packed(batch, collar, 10, skip, uem=uem)
            assert all(torch.equal(a, b) for a, b in zip(old, via))
        counters = M.collar_der_counters(refs, hyps, collar, 10, skip, uem=None)
        assert all(torch.equal(a, b) for a, b in zip(old, counters))
    g = torch.Generator().manual_seed(3)
    preds = [(h.float() * 0.5 + torch.rand(h.shape, generator=g) * 0.5) for h in hyps]
    old = M.sweep_counters(refs, preds, [0.4, 0.6], [1, 5])
    new = M.sweep_counters(refs, preds, [0.4, 0.6], [1, 5], times=True)
    assert len(new) == 5 and all(torch.equal(a, b) for a, b in zip(old, new[:3]))
    assert torch.equal(new[3][0], new[3][3]) and new[3][0].sum().item() == old[0][0, :, 0].sum().item()
    again = M.sweep_counters(refs, preds, [0.4, 0.6], [1, 5], uem=whole)
    assert all(torch.equal(a, b) for a, b in zip(old, again))


# ---- the sweep with regions

def test_sweep_with_regions_equals_score_predictions(M, dev, lim):
    from fs_eend_amd import postproc
    TILE, _ = lim
    g = torch.Generator().manual_seed(7)
    ref = Q.tracks(70, TILE + 300, 3, on=80, off=120)
    pred = (tt(ref[::10]).float().roll(1, 1) * 0.55 + torch.rand(ref[::10].shape, generator=g) * 0.5).clamp(0, 1)
    uem = [(40, 64), (100, TILE - 1), (TILE + 1, TILE + 250)]
    ths, meds = [0.35, 0.5, 0.65], [1, 7]
    res = M.sweep_predictions(tt(ref), pred, ths, meds, collar=10, uem=uem, jaccard=True)
    out = M.sweep_counters(tt(ref), pred, ths, meds, collar=10, uem=uem, times=True)
    rt, ht = out[3].cpu().tolist(), out[4].cpu().tolist()
    for i, th in enumerate(ths):
        for k, med in enumerate(meds):
            gi = i * len(meds) + k
            want = M.score_predictions(tt(ref), pred, threshold=res.thresholds[i], median=med, collar=10, uem=uem, jaccard=True)
            assert {k2: v for k2, v in want.items() if k2 not in ("mapping", "jaccard error rate", "pairing")} == \
                {k2: v for k2, v in res.details[gi][0].items() if k2 != "mapping"}
            hyp = postproc.activity(pred.to(dev), res.thresholds[i], med).cpu().numpy()
            grid = Q.region(ref, hyp, uem, 10, 10)
            assert out[0][gi, 0].cpu().tolist() == grid["counters"] and np.array_equal(out[1][gi, 0].cpu().numpy(), grid["cooc"])
            assert rt[gi][0] == grid["ref_time"] and ht[gi][0] == grid["hyp_time"]
            assert R.valid_mapping(res.details[gi][0]["mapping"], grid["cooc"], grid["best"])
            j = Q.jer(grid["cooc"], grid["ref_time"], grid["hyp_time"])
            assert abs(res.jaccard[gi] - j["rate"]) <= 1e-12 and abs(want["jaccard error rate"] - j["rate"]) <= 1e-12
            assert res.table[gi]["jaccard error rate"] == res.jaccard[gi]
    assert len({tuple(c) for c in out[0][:, 0].cpu().tolist()}) > 1 and res.table[0]["total"] > 0
    sweep = M.DerSweep(ths, meds, collar=10)
    sweep.add([tt(ref)], [pred], uem=[uem])
    assert [r["total"] for r in sweep.report().table] == [r["total"] for r in res.table]
    assert [r["diarization error rate"] for r in sweep.report().table] == [r["diarization error rate"] for r in res.table]


# ---- the Jaccard error rate

@pytest.fixture(scope="module")
def jer_refs():
    return {c["name"]: Q.jer_case_reference(c) for c in Q.JER_CASES}


@pytest.mark.parametrize("case", Q.JER_CASES, ids=[c["name"] for c in Q.JER_CASES])
def test_jer_cases(M, dev, jer_refs, case):
    ref, hyp, want = jer_refs[case["name"]]
    j = Q.jer(want["cooc"], want["ref_time"], want["hyp_time"])
    kw = dict(collar=case["collar"], subsampling=case["sub"], skip_overlap=case.get("skip_overlap", False))
    pairing, speakers, hyp_time = M.jaccard_error_counters([tt(ref)], [tt(hyp)], [case["uem"]], **kw)
    assert pairing.shape == (1, 16) and pairing.dtype == torch.int32 and speakers.shape == (1, 16, 3) and speakers.dtype == torch.int64
    speakers, pairing = speakers[0].cpu().tolist(), pairing[0].cpu().tolist()
    assert hyp_time[0].cpu().tolist() == want["hyp_time"]
    # the integers
    assert {i: tuple(s) for i, s in enumerate(speakers) if s[0] > 0} == j["speakers"]
    assert all(s == [0, 0, 0] for i, s in enumerate(speakers) if i not in j["speakers"])
    # the total, from the integers, against scipy's optimum
    total = sum((rt + ht - 2 * inter) / (rt + ht - inter) for rt, ht, inter in speakers if rt > 0)
    print(case["name"], "total", total, "scipy", j["total"])
    assert abs(total - j["total"]) <= 1e-12 * len(j["speakers"])
    # the pairing: every seeded case has a gap >= Q.MIN_GAP (tests/test_der_region_ref.py), so it is unique
    assert {i: p for i, p in enumerate(pairing) if p >= 0} == j["pairing"]
    d = M.jaccard_error(tt(ref), tt(hyp), uem=case["uem"], **kw)
    assert abs(d["jaccard error rate"] - j["rate"]) <= 1e-12 and d["pairing"] == j["pairing"] and not d["spurious"]
    assert {i: (v["ref time"], v["hyp time"], v["intersection"]) for i, v in d["speakers"].items()} == j["speakers"]
    assert {i: v["jaccard error rate"] for i, v in d["speakers"].items()} == j["rates"]


def test_jer_accumulator(M, jer_refs):
    picks = [c for c in Q.JER_CASES if c["sub"] == 10 and c["collar"] == 0]
    assert len(picks) >= 3
    js = [Q.jer(jer_refs[c["name"]][2]["cooc"], jer_refs[c["name"]][2]["ref_time"], jer_refs[c["name"]][2]["hyp_time"]) for c in picks]
    metric = M.JaccardER(collar=0, subsampling=10)
    first = metric(tt(jer_refs[picks[0]["name"]][0]), tt(jer_refs[picks[0]["name"]][1]), uem=picks[0]["uem"])
    assert abs(first - js[0]["rate"]) <= 1e-12
    rest = metric.score_batch([tt(jer_refs[c["name"]][0]) for c in picks[1:]], [tt(jer_refs[c["name"]][1]) for c in picks[1:]],
                              uems=[c["uem"] for c in picks[1:]])
    assert [r["pairing"] for r in rest] == [j["pairing"] for j in js[1:]]
    n = sum(len(j["speakers"]) for j in js)
    assert metric.report()["speakers"] == n and metric.report()["recordings"] == len(picks)
    assert abs(abs(metric) - sum(j["total"] for j in js) / n) <= 1e-12            # not the mean of the recordings' means
    metric.reset()
    assert abs(metric) == 0.0


def test_jer_degenerate_cases(M, dev):
    ref = R.from_runs(60, [[(0, 20)], [(30, 50)]])
    silent, none = np.zeros((60, 2), np.uint8), np.zeros((60, 1), np.uint8)
    d = M.jaccard_error(tt(ref), tt(silent), subsampling=1)                       # no hypothesis speaker
    assert d["jaccard error rate"] == 1.0 and d["pairing"] == {} and {i: v["hyp time"] for i, v in d["speakers"].items()} == {0: 0, 1: 0}
    d = M.jaccard_error(tt(none), tt(ref), subsampling=1)                          # no reference speaker, hypothesis activity
    assert d["jaccard error rate"] == 1.0 and d["speakers"] == {} and d["spurious"]
    d = M.jaccard_error(tt(none), tt(silent), subsampling=1)                       # ... and none
    assert d["jaccard error rate"] == 0.0 and d["speakers"] == {} and not d["spurious"]
    d = M.jaccard_error(tt(ref), tt(ref), uem=[(0, 25)], subsampling=1)            # speaker 1 has no kept time: not a speaker
    assert list(d["speakers"]) == [0] and d["jaccard error rate"] == 0.0 and d["pairing"] == {0: 0}
    apart = M.jaccard_error(tt(R.from_runs(60, [[(0, 10)]])), tt(R.from_runs(60, [[(20, 30)]])), subsampling=1)
    assert apart["pairing"] == {} and apart["jaccard error rate"] == 1.0          # the pair has no intersection: reported unpaired
    assert apart["speakers"][0] == {"ref time": 10, "hyp time": 0, "intersection": 0, "jaccard error rate": 1.0}
    pairing, speakers, _ = M.jaccard_error_counters([tt(ref), tt(none), tt(ref)], [tt(silent), tt(ref), tt(ref)], subsampling=1)
    assert pairing.cpu().tolist() == [[-1] * 16, [-1] * 16, [0, 1] + [-1] * 14]
    assert speakers[2, :2].cpu().tolist() == [[20, 20, 20], [20, 20, 20]] and speakers[1].sum().item() == 0
    agg = M.JaccardER(subsampling=1)
    agg.score_batch([tt(none)], [tt(ref)])
    assert abs(agg) == 1.0 and agg.report()["speakers"] == 0


# ---- the rasteriser

RASTER_TABLES = [
    [(0, 5, 20), (0, 10, 30), (1, 0, 3), (0, 29, 31)],               # overlapping segments of one speaker
    [(0, 7, 7), (1, 12, 12), (1, 3, 4)],                              # zero-length segments write nothing
    [(2, 90, 100), (0, 0, 100)],                                      # ends exactly at the recording's length
    [(s, 3 * s, 3 * s + 10 + s) for s in range(16)],                  # 16 speakers
    [],                                                               # no segments
    [(0, 0, 1)],
]
RASTER_LENGTHS = [40, 20, 100, 80, 33, 1]


def test_rasteriser(M, dev):
    want = [Q.raster(t, n, 16) for t, n in zip(RASTER_TABLES, RASTER_LENGTHS)]
    rows, off = M.segments_raster(RASTER_TABLES, RASTER_LENGTHS)
    wrows, woff = M.pack_references([tt(w) for w in want])
    assert rows.dtype == torch.uint8 and torch.equal(rows, wrows) and torch.equal(off, woff)
    for t, n, w in zip(RASTER_TABLES[:3], RASTER_LENGTHS, want):     # alone, narrower, and odd widths
        C = max(s[0] for s in t) + 1
        rows, off = M.segments_raster([t], [n])
        assert torch.equal(rows.cpu(), tt(w[:, :C])) and off.tolist() == [0, n]
    rows, off = M.segments_raster([[]], [0])
    assert rows.shape == (1, 1) and off.tolist() == [0, 0]


def test_pack_rttm_equals_pack_of_the_matrices(M, dev):
    rttm = M.read_rttm(Q.RTTM_TEXT)
    uem = M.read_uem(Q.UEM_TEXT)
    recs = ["rec2", "missing", "rec1"]
    (rows, off), table = M.pack_rttm(recs, rttm, uem, lengths={"rec2": 150, "missing": 9, "rec1": 10})
    lens = [201, 9, 304]                                              # last segment end; the caller's; last segment end (> UEM's 300)
    mats = [Q.raster(Q.RTTM_WANT["rec2"]["segments"], 201, 2), np.zeros((9, 2), np.uint8), Q.raster(Q.RTTM_WANT["rec1"]["segments"], 304, 2)]
    wrows, woff = M.pack_references([tt(m) for m in mats])
    assert off.tolist() == [0, 201, 210, 514] and torch.equal(rows, wrows) and torch.equal(off, woff)
    wt, wo = M.pack_uem([Q.UEM_WANT["rec2"], None, Q.UEM_WANT["rec1"]], dev)
    assert torch.equal(table[0], wt) and torch.equal(table[1], wo)
    (rows2, off2), none = M.pack_rttm(["rec1"], rttm, None, [400])
    assert none is None and off2.tolist() == [0, 400] and torch.equal(rows2[:304].cpu(), tt(mats[2])) and rows2[304:].sum().item() == 0
    # scored straight from the text: the reference is itself, inside the UEM
    hyp = tt(mats[2][::10])
    batch = (rows2, off2) + M.pack([tt(mats[2])], [hyp], 10)[2:]
    got = M.collar_der_regions_packed(batch, M.pack_uem([Q.UEM_WANT["rec1"]], dev), 0, 10)
    want = Q.region(np.concatenate([mats[2], np.zeros((96, 2), np.uint8)]), mats[2][::10], Q.UEM_WANT["rec1"], 10, 0)
    assert got[0][0].cpu().tolist() == want["counters"] and got[3][0].cpu().tolist() == want["ref_time"]


# ---- graph capture

def test_graph_capture_and_replay_with_regions(M, dev, lim):
    TILE, _ = lim
    T = TILE + 200
    data = [(Q.tracks(80 + i, T, 3, on=90, off=110), Q.tracks(90 + i, T // 10, 4, on=9, off=11), u)
            for i, u in enumerate(([(10, 500), (TILE - 5, TILE + 100)], [(0, 64), (700, T)], [(10, 500), (TILE - 5, TILE + 100)]))]
    batch = M.pack([tt(data[0][0])], [tt(data[0][1])])
    table = M.pack_uem([data[0][2]], dev)
    der_out = tuple(torch.full_like(t, -1) for t in M.collar_der_regions_packed(batch, table, 10, 10))
    jer_out = tuple(torch.full_like(t, -1) for t in M.jaccard_error_counters(batch, None, table, 10, 10)[:2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        M.collar_der_packed(batch, 10, 10, out=der_out, uem=table)
        M.jaccard_error_counters(batch, None, table, 10, 10, out=(der_out, jer_out))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        M.collar_der_packed(batch, 10, 10, out=der_out, uem=table)
        M.jaccard_error_counters(batch, None, table, 10, 10, out=(der_out, jer_out))
    for ref, hyp, uem in data:
        batch[0].copy_(tt(ref))
        batch[2].copy_(tt(hyp))
        table[0].copy_(torch.tensor(uem, dtype=torch.int32))
        for t in der_out + jer_out:
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        want = Q.region(ref, hyp, uem, 10, 10)
        j = Q.jer(want["cooc"], want["ref_time"], want["hyp_time"])
        assert want["counters"][0] > 100 and want["counters"][6] > 100
        mapping = {k: i for k, i in enumerate(der_out[2][0].cpu().tolist()) if i >= 0}
        agrees((der_out[0][0].cpu().tolist(), der_out[1][0].cpu().numpy(), mapping, der_out[3][0].cpu().tolist(),
                der_out[4][0].cpu().tolist()), want, 4)
        assert {i: tuple(s) for i, s in enumerate(jer_out[1][0].cpu().tolist()) if s[0] > 0} == j["speakers"]
