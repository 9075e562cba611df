"""GPU: the collar DER kernels (csrc/der_collar.hip behind eend_collar_der_u64, fs_eend_amd.metrics) against the goldens and
against the frame-grid restatement of tests/der_ref.py, at the tile, collar, recording and width edges.  Integer work: every
comparison is exact.  Mappings are checked for validity (one-to-one, every pair co-occurs, optimal value), never against
scipy's choice, because ties are free."""
import ast
import os

import numpy as np
import pytest
import torch

from tests import der_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL = -1


@pytest.fixture(scope="module")
def M(hip_lib, dev):
    from fs_eend_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def lim(M):
    return M.limits()                                                # (TILE, HMAX)


@pytest.fixture(scope="module")
def golden_inputs():
    return [R.inputs(c) for c in R.CASES]


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return ast.literal_eval(str(z["meta"])), z["counters"].tolist(), z["cooc"], int(z["best"])


def run(M, refs, hyps, sub, collar, skip=False):
    """-> per recording (counters list, cooc array, mapping {hyp: ref})"""
    counters, cooc, mapping = M.collar_der_counters([torch.from_numpy(np.ascontiguousarray(r)) for r in refs],
                                                    [torch.from_numpy(np.ascontiguousarray(h)) for h in hyps], collar, sub, skip)
    assert counters.is_cuda and counters.dtype == torch.int64 and cooc.shape[1:] == (16, 16) and mapping.dtype == torch.int32
    counters, cooc, mapping = counters.cpu().tolist(), cooc.cpu().numpy(), mapping.cpu().tolist()
    return [(c, k, {j: i for j, i in enumerate(m) if i >= 0}) for c, k, m in zip(counters, cooc, mapping)]


def agrees(got, want, Ch):
    counters, cooc, mapping = got
    assert counters == want["counters"]
    assert np.array_equal(cooc, want["cooc"])
    assert all(j < Ch for j in mapping) and R.valid_mapping(mapping, cooc, want["best"])


def check(M, refs, hyps, sub, collar, skip=False):
    got = run(M, refs, hyps, sub, collar, skip)
    for g, r, h in zip(got, refs, hyps):
        agrees(g, R.grid(r, h, sub, collar, skip), h.shape[1])
    return got


def tracks(seed, T, C, on=40, off=60):
    rng = np.random.default_rng(seed)
    return np.stack([R.run_track(rng, T, on, off) for _ in range(C)], axis=1) if T else np.zeros((0, C), np.uint8)


# ---- goldens and hand cases

@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_golden_alone(M, case):
    meta, counters, cooc, best = load_golden(case["name"])
    ref, hyp = R.inputs(case)
    got, = run(M, [ref], [hyp], case["sub"], case["collar"], case.get("skip_overlap", False))
    agrees(got, dict(counters=counters, cooc=cooc, best=best), hyp.shape[1])


def test_goldens_in_one_ragged_batch(M, golden_inputs):
    """All eleven recordings in one launch, once per parameter set of the cases: the cases written with that set equal their
    goldens, the others the grid restatement."""
    refs, hyps = [r for r, _ in golden_inputs], [h for _, h in golden_inputs]
    for sub, collar, skip in sorted({(c["sub"], c["collar"], c.get("skip_overlap", False)) for c in R.CASES}):
        got = check(M, refs, hyps, sub, collar, skip)
        for c, g, h in zip(R.CASES, got, hyps):
            if (c["sub"], c["collar"], c.get("skip_overlap", False)) == (sub, collar, skip):
                _, counters, cooc, best = load_golden(c["name"])
                agrees(g, dict(counters=counters, cooc=cooc, best=best), h.shape[1])


def test_hand_cases(M):
    ref, hyp, sub = R.HAND_A
    assert run(M, [ref], [hyp], sub, 0)[0][0] == [10, 2, 2, 0, 8, 20, 0, 8]
    assert run(M, [ref], [hyp], sub, 4)[0][0] == [6, 0, 0, 0, 6, 12, 8, 6]
    ref, hyp, sub = R.HAND_B
    c, cooc, mapping = run(M, [ref], [hyp], sub, 0)[0]
    assert c[:5] == [14, 0, 6, 0, 14] and cooc[:2, :3].tolist() == [[2, 6, 0], [8, 2, 0]] and mapping == {0: 1, 1: 0}
    c, cooc, _ = run(M, [ref], [hyp], sub, 2)[0]
    assert c[:6] == [6, 0, 5, 0, 6, 9] and cooc[:2, :3].tolist() == [[0, 2, 0], [4, 0, 0]]
    c, cooc, _ = run(M, [ref], [hyp], sub, 0, True)[0]
    assert c[:6] == [10, 0, 6, 0, 10, 14] and cooc[:2, :3].tolist() == [[0, 4, 0], [6, 0, 0]]
    d = M.collar_der(torch.from_numpy(ref), torch.from_numpy(hyp), collar=0, subsampling=sub)
    assert d == {"total": 14, "correct": 14, "confusion": 0, "false alarm": 6, "missed detection": 0,
                 "diarization error rate": 6 / 14, "mapping": {0: 1, 1: 0}, "frames kept": 16, "frames removed": 0}


# ---- tile edges

def test_boundary_at_the_tile_edge(M, lim):
    TILE, HMAX = lim
    Tr = 3 * TILE
    refs = []
    for p in (TILE - 1, TILE, TILE + 1):
        r = np.zeros((Tr, 1), np.uint8)
        r[p:] = 1                                                    # one boundary at p (and the one at Tr, far away)
        refs.append(r)
    hyps = [tracks(40 + i, Tr, 2) for i in range(3)]
    for h in (0, 1, 25):
        got = check(M, refs, hyps, 1, 2 * h)
        assert [g[0][6] for g in got] == [3 * h] * 3                # 2 h frames around p, h in front of the boundary at Tr = T
    if TILE + 3 <= HMAX:                                             # a collar that spans a whole tile
        check(M, refs, hyps, 1, 2 * (TILE + 3))
        long_ref = np.zeros((6 * TILE, 1), np.uint8)
        long_ref[3 * TILE + 5:] = 1
        check(M, [long_ref], [tracks(44, 6 * TILE, 2)], 1, 2 * (TILE + 3))


def test_lengths_around_the_tile(M, lim):
    TILE, _ = lim
    lens = [TILE, TILE - 1, TILE + 1, 2 * TILE + 1]
    refs = [tracks(50 + i, n, 3) for i, n in enumerate(lens)]
    for sub in (1, 10):
        hyps = [tracks(60 + i, -(-n // sub), 4, on=max(2, 40 // sub), off=max(2, 60 // sub)) for i, n in enumerate(lens)]
        for collar in (0, 50):
            check(M, refs, hyps, sub, collar)


def test_hypothesis_frame_straddles_the_tile_edge(M, lim):
    TILE, _ = lim
    sub = 10
    assert TILE % sub, "the tile is a multiple of the subsampling: pick another one here"
    k = TILE // sub                                                  # covers [k sub, (k + 1) sub), the tile edge inside
    Tr = 2 * TILE + 1
    ref = np.ones((Tr, 2), np.uint8)
    ref[:, 1] = 0
    hyp = np.zeros((-(-Tr // sub), 2), np.uint8)
    hyp[k, 1] = 1
    got, = check(M, [ref], [hyp], sub, 0)
    assert got[1][0, 1] == sub and got[0][:3] == [Tr, Tr - sub, 0]
    hyp[k - 3:k + 3, 0] = 1
    check(M, [ref], [hyp], sub, 4)


def test_more_tiles_than_tile_groups(M, lim):
    """eend_collar_der_u64 launches at most 512 tile groups per recording: with more tiles a workgroup loops, keeps its sums on
    chip and adds once."""
    TILE, _ = lim
    Tr = (512 + 2) * TILE + 7
    ref, hyp = tracks(70, Tr, 2, on=3000, off=4000), tracks(71, Tr // 10 + 3, 3, on=300, off=500)
    check(M, [ref], [hyp], 10, 50)
    # and in a batch, where a recording gets fewer groups
    small = [tracks(80 + i, 300 + i, 2) for i in range(63)]
    mid = tracks(72, 70 * TILE + 3, 2, on=500, off=700)
    got = check(M, small[:31] + [mid] + small[31:], [tracks(90 + i, 31 + i % 5, 2, on=5, off=6) for i in range(31)]
                + [tracks(73, 7 * TILE, 2, on=50, off=70)] + [tracks(130 + i, 29 + i % 5, 2, on=5, off=6) for i in range(32)], 10, 50)
    assert len(got) == 64


# ---- recording edges

def test_recording_edges(M):
    on = lambda T, C, runs: R.from_runs(T, runs + [[]] * (C - len(runs)))
    cases = [
        (on(300, 2, [[(0, 120)], [(200, 300)]]), tracks(1, 30, 2, 8, 8), 10),          # active in frame 0 and in frame Tr - 1
        (on(300, 1, [[(100, 300)]]), np.ones((40, 1), np.uint8), 10),                  # Th sub > Tr: the tail behind the boundary at Tr
        (on(300, 2, [[(0, 300)], [(50, 250)]]), tracks(2, 17, 3, 5, 5), 10),           # Th sub < Tr
        (np.ones((1, 1), np.uint8), np.ones((1, 2), np.uint8), 1),                     # Tr = 1
        (np.ones((1, 1), np.uint8), np.ones((3, 1), np.uint8), 10),
        (tracks(3, 200, 3), np.zeros((20, 2), np.uint8), 10),                          # an all-zero hypothesis
        (tracks(4, 200, 3), np.zeros((0, 2), np.uint8), 10),                           # an empty hypothesis
        (np.zeros((0, 2), np.uint8), tracks(5, 20, 2, 5, 5), 10),                      # an empty reference
        (np.zeros((0, 1), np.uint8), np.zeros((0, 1), np.uint8), 10),                  # nothing at all
    ]
    for collar in (0, 2, 50):
        for ref, hyp, sub in cases:
            check(M, [ref], [hyp], sub, collar)
        by_sub = {}
        for ref, hyp, sub in cases:
            by_sub.setdefault(sub, []).append((ref, hyp))
        for sub, pairs in by_sub.items():
            check(M, [p[0] for p in pairs], [p[1] for p in pairs], sub, collar)
    # the collar of the boundary at Tr removes tail frames that would otherwise be false alarms
    ref, hyp, sub = cases[1]
    assert run(M, [ref], [hyp], sub, 0)[0][0][2] == 100 + 100 and run(M, [ref], [hyp], sub, 50)[0][0][2] == 200 - 25 - 25


def test_all_zero_reference(M):
    ref = torch.zeros(120, 2)
    silent = M.collar_der(ref, torch.zeros(12, 3), collar=50, subsampling=10)
    assert silent["total"] == 0 and silent["diarization error rate"] == 0.0 and silent["mapping"] == {} and silent["frames kept"] == 120
    hyp = torch.zeros(12, 3)
    hyp[2:7, 1] = 1
    active = M.collar_der(ref, hyp, collar=50, subsampling=10)
    assert active["total"] == 0 and active["false alarm"] == 50 and active["diarization error rate"] == 1.0 and active["mapping"] == {}


# ---- widths and the collar cap

def test_widths(M):
    pairs = [(tracks(10, 500, 1), tracks(11, 50, 3, 6, 6)), (tracks(12, 900, 16, 60, 700), tracks(13, 90, 16, 6, 60)),
             (tracks(14, 900, 16, 60, 700), tracks(15, 90, 2, 6, 10))]
    for ref, hyp in pairs:
        check(M, [ref], [hyp], 10, 10)
    check(M, [p[0] for p in pairs], [p[1] for p in pairs], 10, 10)   # mixed widths in one batch: silent columns are added
    ref16 = tracks(16, 900, 16, 60, 120)                             # every speaker talks; the hypothesis is the reference, rotated
    got, = check(M, [ref16], [np.roll(ref16[::10], 3, axis=1)], 10, 0)
    assert got[2] == {j: (j - 3) % 16 for j in range(16)}


def raw_call(M, ref, hyp, Cr, Ch, h, sub=10):
    dev = ref.device
    roff = torch.tensor([0, ref.shape[0]], dtype=torch.int32, device=dev)
    hoff = torch.tensor([0, hyp.shape[0]], dtype=torch.int32, device=dev)
    counters = torch.full((1, 8), -7, dtype=torch.int64, device=dev)
    cooc = torch.zeros(1, 16, 16, dtype=torch.int64, device=dev)
    mapping = torch.zeros(1, 16, dtype=torch.int32, device=dev)
    from fs_eend_amd import lib
    rc = lib.load().eend_collar_der_u64(ref.data_ptr(), roff.data_ptr(), Cr, hyp.data_ptr(), hoff.data_ptr(), Ch, 1, sub, h, 0,
                                        counters.data_ptr(), cooc.data_ptr(), mapping.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, counters.cpu().tolist()[0]


def test_c_entry_refusals_and_collar_cap(M, lim, dev):
    TILE, HMAX = lim
    assert HMAX >= 512
    Tr = 3 * HMAX + 100                                              # boundaries at 0, 40, Tr - 40 and Tr: the middle survives h = HMAX
    ref_np, hyp_np = R.from_runs(Tr, [[(0, 40)], [(Tr - 40, Tr)]]), tracks(21, Tr // 10 + 10, 2, 90, 90)
    ref, hyp = torch.from_numpy(ref_np).to(dev), torch.from_numpy(hyp_np).to(dev)
    wide = torch.zeros(64, 17, dtype=torch.uint8, device=dev)
    for Cr, Ch in ((17, 2), (2, 17), (17, 17), (0, 2)):
        rc, counters = raw_call(M, wide, wide, Cr, Ch, 25)
        assert rc == EINVAL and counters == [-7] * 8                 # refused before anything was written
    rc, counters = raw_call(M, ref, hyp, 2, 2, HMAX + 1)
    assert rc == EINVAL and counters == [-7] * 8
    rc, counters = raw_call(M, ref, hyp, 2, 2, HMAX)
    assert rc == 0 and counters == R.grid(ref_np, hyp_np, 10, 2 * HMAX)["counters"]
    assert 0 < counters[5] < ref_np.shape[0]                         # the widest collar still leaves frames to score
    check(M, [ref_np], [hyp_np], 10, 2 * HMAX)
    with pytest.raises(ValueError):
        M.collar_der(ref, hyp, collar=2 * HMAX + 2)
    # frame indices beyond 2^31 are out of scope: the Python layer refuses, and the C entry, which cannot see the lengths on the
    # host, leaves the recording unread and marks it (every counter ~0, no mapping)
    with pytest.raises(ValueError):
        M.collar_der(ref, hyp, subsampling=2 ** 30)
    rc, counters = raw_call(M, ref, hyp, 2, 2, 25, sub=2 ** 30)
    assert rc == 0 and counters == [-1] * 8


def test_skip_overlap_changes_every_counter(M):
    case = next(c for c in R.CASES if c["name"] == "der_skip_overlap")
    ref, hyp = R.inputs(case)
    off, = check(M, [ref], [hyp], case["sub"], case["collar"], False)
    on, = check(M, [ref], [hyp], case["sub"], case["collar"], True)
    assert all(a != b for a, b in zip(off[0], on[0])), (off[0], on[0])


# ---- batch independence, input forms, the Python layer

def test_batch_independence(M):
    ref, hyp = tracks(30, 2500, 4, 100, 200), tracks(31, 251, 5, 10, 20)
    a, b, c = (tracks(32, 17, 2), tracks(33, 1, 1, 3, 3)), (tracks(34, 5000, 6, 100, 300), tracks(35, 480, 3, 10, 20)), \
        (np.zeros((0, 1), np.uint8), tracks(36, 9, 2, 3, 3))
    alone = run(M, [ref], [hyp], 10, 50)[0]
    agrees(alone, R.grid(ref, hyp, 10, 50), hyp.shape[1])
    again = run(M, [ref], [hyp], 10, 50)[0]
    assert again[0] == alone[0] and np.array_equal(again[1], alone[1]) and again[2] == alone[2]
    for order, at in (([(ref, hyp), a, b, c], 0), ([a, b, c, (ref, hyp)], 3), ([b, (ref, hyp), a], 1), ([(ref, hyp)], 0),
                      ([c, (ref, hyp), c, b], 1)):
        got = run(M, [p[0] for p in order], [p[1] for p in order], 10, 50)[at]
        assert got[0] == alone[0] and np.array_equal(got[1], alone[1]) and got[2] == alone[2]


def test_input_forms(M, dev):
    ref, hyp = tracks(37, 800, 3, 60, 90), tracks(38, 83, 4, 6, 9)
    want = R.grid(ref, hyp, 10, 10)["counters"]
    r8, h8 = torch.from_numpy(ref), torch.from_numpy(hyp)
    forms = [(r8, h8), (r8.to(dev), h8.to(dev)), (r8.float() * 0.25, h8.double() * 7), (r8.bool(), h8.bool().to(dev)),
             (r8.long().to(dev) * -3, h8.to(torch.float16)), (r8.to(dev).t().contiguous().t(), h8.to(dev)[:, :])]
    for r, h in forms:
        counters, _, _ = M.collar_der_counters(r, h, 10, 10)
        assert counters.cpu().tolist() == [want]
    counters, _, _ = M.collar_der_counters([r8, r8.to(dev)], (h8.bool(), h8.float()), 10, 10)
    assert counters.cpu().tolist() == [want, want]


def test_score_predictions(M, dev):
    from fs_eend_amd import postproc
    g = torch.Generator().manual_seed(5)
    ref = torch.from_numpy(tracks(39, 1200, 3, 100, 150))
    pred = (ref[::10].float().roll(1, 1) * 0.6 + torch.rand(120, 3, generator=g) * 0.5).clamp(0, 1)
    sad = (torch.rand(120, generator=g) > 0.2)
    for kw in (dict(), dict(threshold=0.7, median=5), dict(sad=sad), dict(median=1, collar=10, skip_overlap=True)):
        post = {k: v for k, v in kw.items() if k in ("threshold", "median", "sad")}
        score = {k: v for k, v in kw.items() if k in ("collar", "skip_overlap")}
        hyp = postproc.activity(pred.to(dev), **post)
        want = M.collar_der(ref, hyp, **score)
        assert M.score_predictions(ref, pred, **kw) == want
        assert want["total"] > 0 and want == M.score_predictions(ref.to(dev), pred.to(dev), **kw)
        g = R.grid(ref.numpy(), hyp.cpu().numpy(), 10, score.get("collar", 50), score.get("skip_overlap", False))
        assert [want[k] for k in ("total", "missed detection", "false alarm", "confusion", "correct")] == g["counters"][:5]
        assert R.valid_mapping(want["mapping"], g["cooc"], g["best"])


def test_collar_der_metric_aggregates(M, golden_inputs):
    picks = [(r, h) for c, (r, h) in zip(R.CASES, golden_inputs) if c["sub"] == 10][:5]
    want = [R.grid(r, h, 10, 50)["counters"] for r, h in picks]
    sums = np.sum(want, axis=0).tolist()
    metric = M.CollarDER(collar=50, subsampling=10)
    one = metric(torch.from_numpy(picks[0][0]), torch.from_numpy(picks[0][1]))
    assert one == (want[0][1] + want[0][2] + want[0][3]) / want[0][0]
    det = metric(torch.from_numpy(picks[1][0]), torch.from_numpy(picks[1][1]), detailed=True)
    assert [det[k] for k in ("total", "missed detection", "false alarm", "confusion", "correct")] == want[1][:5]
    rest = metric.score_batch([torch.from_numpy(r) for r, _ in picks[2:]], [torch.from_numpy(h) for _, h in picks[2:]])
    assert [[d[k] for k in ("total", "missed detection", "false alarm", "confusion", "correct")] for d in rest] == [w[:5] for w in want[2:]]
    rep = metric.report()
    assert [rep[k] for k in ("total", "missed detection", "false alarm", "confusion", "correct")] == sums[:5] and rep["recordings"] == 5
    assert abs(metric) == (sums[1] + sums[2] + sums[3]) / sums[0] == rep["diarization error rate"]
    metric.reset()
    assert abs(metric) == 0.0 and metric.report()["total"] == 0


def test_graph_capture_and_replay(M, dev):
    ref, hyp = tracks(41, 3000, 4, 600, 900), tracks(42, 300, 5, 60, 90)
    ref2, hyp2 = tracks(43, 3000, 4, 500, 700), tracks(44, 300, 5, 50, 70)
    batch = M.pack([torch.from_numpy(ref)], [torch.from_numpy(hyp)])
    out = tuple(torch.full_like(t, -1) for t in M.collar_der_packed(batch, 50, 10))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        M.collar_der_packed(batch, 50, 10, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        M.collar_der_packed(batch, 50, 10, out=out)
    for r, h in ((ref, hyp), (ref2, hyp2), (ref, hyp)):
        batch[0].copy_(torch.from_numpy(r))
        batch[2].copy_(torch.from_numpy(h))
        for t in out:
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        want = R.grid(r, h, 10, 50)
        assert want["counters"][0] > 100 and want["best"] > 0
        mapping = {j: i for j, i in enumerate(out[2].cpu().tolist()[0]) if i >= 0}
        agrees((out[0].cpu().tolist()[0], out[1].cpu().numpy()[0], mapping), want, 5)


def test_one_hour_of_eight_speakers(M):
    """Tr = 360 000, sub = 10, twice in one batch: the grid over 352 tiles of each and the 64-bit sums."""
    ref, hyp = tracks(45, 360000, 8, 600, 9000), tracks(46, 36000, 8, 60, 900)
    hyp[:, :6] |= np.roll(ref[::10], 2, axis=1)[:, :6]
    want = R.grid(ref, hyp, 10, 50)
    assert want["counters"][0] > 100000 and want["counters"][3] > 0
    a, b = run(M, [ref, ref], [hyp, hyp], 10, 50)
    agrees(a, want, 8)
    agrees(b, want, 8)
    assert a[2] == b[2]
