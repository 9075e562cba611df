"""GPU: the collar DER sweep (csrc/der_sweep.hip behind eend_collar_der_sweep_u64, the sweep functions of fs_eend_amd.metrics).
For every point of a grid the counters and co-occurrence counts must equal the CPU reference (tests/sweep_ref.py) and the
two-step device path that existed before, collar_der_counters over postproc.activity.  Every comparison is exact; mappings are
checked for validity only (ties are free), as in tests/test_der_gpu.py."""
import ast
import os

import numpy as np
import pytest
import torch

from tests import der_ref as R
from tests import sweep_ref as W

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def M(hip_lib, dev):
    from fs_eend_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def TILE(M):
    return M.limits()[0]


def t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x))


def run(M, refs, preds, ths, meds, sads=None, sub=10, collar=50, skip=False):
    """-> got[g][b] = (counters list, cooc array, mapping {hyp: ref})"""
    counters, cooc, mapping = M.sweep_counters([t(r) for r in refs], [t(p) for p in preds], ths, meds,
                                               None if sads is None else [t(s) for s in sads], collar, sub, skip)
    G, B = len(ths) * len(meds), len(refs)
    assert counters.is_cuda and counters.dtype == torch.int64 and counters.shape == (G, B, 8)
    assert cooc.shape == (G, B, 16, 16) and cooc.dtype == torch.int64 and mapping.shape == (G, B, 16) and mapping.dtype == torch.int32
    counters, cooc, mapping = counters.cpu().tolist(), cooc.cpu().numpy(), mapping.cpu().tolist()
    return [[(counters[g][b], cooc[g][b], {j: i for j, i in enumerate(mapping[g][b]) if i >= 0}) for b in range(B)] for g in range(G)]


def two_step(M, dev, refs, preds, th, k, sads, sub, collar, skip):
    """The path the sweep replaces, per recording: activity on the device (an empty recording has an empty map), then the scorer."""
    from fs_eend_amd import postproc
    hyps = [postproc.activity(t(p).to(dev), th, k, None if sads is None else t(sads[b])) if p.shape[0]
            else torch.zeros(0, p.shape[1], dtype=torch.uint8) for b, p in enumerate(preds)]
    counters, cooc, _ = M.collar_der_counters([t(r) for r in refs], hyps, collar, sub, skip)
    return counters.cpu().tolist(), cooc.cpu().numpy()


def check(M, dev, refs, preds, ths, meds, sads=None, sub=10, collar=50, skip=False, device_path=True):
    got = run(M, refs, preds, ths, meds, sads, sub, collar, skip)
    for g, (th, k) in enumerate((th, k) for th in ths for k in meds):
        if device_path:
            counters, cooc = two_step(M, dev, refs, preds, th, k, sads, sub, collar, skip)
        for b, (ref, pred) in enumerate(zip(refs, preds)):
            want = R.grid(ref, W.activity(pred, th, k, None if sads is None else sads[b]), sub, collar, skip)
            c, co, mapping = got[g][b]
            assert c == want["counters"], (g, b, th, k)
            assert np.array_equal(co, want["cooc"]), (g, b, th, k)
            assert all(j < pred.shape[1] for j in mapping) and R.valid_mapping(mapping, co, want["best"]), (g, b, th, k)
            if device_path:
                assert c == counters[b] and np.array_equal(co, cooc[b]), (g, b, th, k)
    return got


def tracks(seed, T, C, on=40, off=60):
    rng = np.random.default_rng(seed)
    return np.stack([R.run_track(rng, T, on, off) for _ in range(C)], axis=1) if T else np.zeros((0, C), np.uint8)


def post(seed, base):
    return W.posteriors(np.random.default_rng(seed), base)


# ---- the seeded cases (shown to be non-degenerate by tests/test_sweep_ref.py)

@pytest.mark.parametrize("case", W.CASES, ids=[c["name"] for c in W.CASES])
def test_seeded_cases(M, dev, case):
    ref, pred, flags = W.inputs(case)
    check(M, dev, [ref], [pred], case["thresholds"], case["medians"], None if flags is None else [flags], case["sub"], case["collar"],
          case.get("skip_overlap", False))


def test_seeded_cases_in_one_ragged_batch(M, dev):
    ins = [W.inputs(c) for c in W.CASES if not c.get("sad")]
    check(M, dev, [i[0] for i in ins], [i[1] for i in ins], W.THRESHOLDS, W.MEDIANS, None, 10, 50)
    ins = [W.inputs(c) for c in W.CASES if c.get("sad")]
    check(M, dev, [i[0] for i in ins], [i[1] for i in ins], (0.6, 0.4), (11, 3), [i[2] for i in ins], 3, 20, device_path=False)


# ---- tile edges

@pytest.mark.parametrize("sub", [1, 3, 10])
def test_activity_changes_next_to_a_tile_edge(M, dev, TILE, sub):
    """Decisions that flip within k / 2 hypothesis frames of the frame under the tile edge, on both sides of it: the filtered
    value there needs the halo of the staged rows.  sub = 3 does not divide the tile."""
    Tr = 2 * TILE + 5
    Th = -(-Tr // sub)
    ref = tracks(400 + sub, Tr, 2, 300, 400)
    base = tracks(410 + sub, Th, 3, 5, 6)                            # runs of 1 .. 5 on, 1 .. 6 off: flips everywhere
    pred = post(420 + sub, base)
    for edge in (TILE // sub, 2 * TILE // sub):
        pred[edge - 1, 0], pred[edge, 0], pred[edge + 1, 0] = 0.9, 0.1, 0.9
        pred[edge - 2:edge, 1], pred[edge:edge + 2, 1] = 0.05, 0.95
    meds = (1, 3, 11, 127)
    for th in (0.4, 0.6):
        d = W.decisions(pred, th)
        for edge in (TILE // sub, 2 * TILE // sub):
            assert d[edge - 1, 0] and not d[edge, 0] and d[edge + 1, 0] and not d[edge - 1, 1] and d[edge, 1]
    check(M, dev, [ref], [pred], (0.4, 0.6), meds, None, sub, 10)
    flags = W.S.run_flags(430 + sub, Th, longest=9)
    check(M, dev, [ref], [pred], (0.4, 0.6), meds, [flags], sub, 10, device_path=False)


def test_lengths_around_the_tile(M, dev, TILE):
    for sub in (1, 3):
        ths_len = [-(-n // sub) for n in (TILE - 1, TILE, TILE + 1)] if sub > 1 else [TILE - 1, TILE, TILE + 1]
        preds = [post(440 + i, tracks(450 + i, n, 2, 7, 9)) for i, n in enumerate(ths_len)]
        refs = [tracks(460 + i, max(0, n * sub - 7 * i), 3, 50, 70) for i, n in enumerate(ths_len)]   # T = Th sub for i > 0
        check(M, dev, refs, preds, (0.5,), (1, 11), None, sub, 10)
    refs = [tracks(470 + i, n, 2, 50, 70) for i, n in enumerate((TILE - 1, TILE, TILE + 1))]            # and T = Tr
    preds = [post(480 + i, tracks(490 + i, n // 10, 2, 7, 9)) for i, n in enumerate((TILE - 1, TILE, TILE + 1))]
    check(M, dev, refs, preds, (0.5,), (1, 11), None, 10, 10)


def test_more_tiles_than_tile_groups(M, dev, TILE):
    """The launch gives a recording at most 512 tile groups: with more tiles a workgroup loops, keeps its sums on chip and adds
    once per point."""
    Tr = (512 + 2) * TILE + 7
    ref = tracks(500, Tr, 2, 3000, 4000)
    pred = post(501, tracks(502, Tr // 10 + 3, 2, 300, 500))
    got = check(M, dev, [ref], [pred], (0.5,), (1, 11), None, 10, 50)
    assert got[0][0][0] != got[1][0][0] and got[0][0][0][0] > 100000


# ---- recording edges

def test_short_and_empty_recordings(M, dev):
    ref = tracks(510, 60, 2, 20, 20)
    pairs = [(ref, post(511, tracks(512, 5, 2, 3, 2))),               # Th < k
             (ref, np.full((1, 2), 0.9, np.float32)),                 # Th = 1
             (ref, np.zeros((0, 2), np.float32)),                     # Th = 0
             (np.zeros((0, 2), np.uint8), post(513, tracks(514, 9, 2, 4, 3))),   # Tr = 0
             (np.zeros((0, 1), np.uint8), np.zeros((0, 1), np.float32))]        # nothing at all
    meds = (1, 3, 11, 127)
    for r, p in pairs:
        check(M, dev, [r], [p], (0.5, 0.3), meds, None, 10, 4)
    check(M, dev, [p[0] for p in pairs], [p[1] for p in pairs], (0.5, 0.3), meds, None, 10, 4)
    flags = [np.ones(p.shape[0], np.uint8) for _, p in pairs]
    check(M, dev, [p[0] for p in pairs], [p[1] for p in pairs], (0.5, 0.95), meds, flags, 10, 4, device_path=False)
    # one active frame in five survives no median of 11 and a lone frame no median of 3
    got = run(M, [ref], [np.full((1, 2), 0.9, np.float32)], (0.5,), (1, 3), None, 10, 0)
    assert got[0][0][0][2] + got[0][0][0][4] + got[0][0][0][3] > 0 and got[1][0][0][2] == 0 and got[1][0][0][4] == 0


def test_median_window_over_both_ends(M, dev):
    Th = 40
    pred = np.full((Th, 2), 0.1, np.float32)
    pred[:4, 0] = 0.9                                                # 4 of the 7 frames a window of 7 sees at frame 0 .. are zeros outside
    pred[-6:, 1] = 0.9
    ref = tracks(520, Th * 10, 2, 150, 100)
    meds = (3, 7, 11, 127)
    acts = [W.activity(pred, 0.5, k) for k in meds]
    assert acts[0][0, 0] and acts[0][-1, 1] and acts[1][0, 0] and not acts[2][0, 0] and acts[2][-1, 1] and not acts[3].any()
    check(M, dev, [ref], [pred], (0.5,), meds, None, 10, 0)


def test_neighbours_in_the_packed_buffer_do_not_leak(M, dev):
    """The first ends active and the second starts silent, and the other way round: the median window of a recording sees zeros
    beyond its ends, not the rows next to it."""
    a = np.full((30, 2), 0.1, np.float32)
    a[-4:] = 0.9                                                     # ends active: 4 frames, which no median of 11 keeps
    b = np.full((30, 2), 0.1, np.float32)
    b[12:20] = 0.9                                                   # starts and ends silent
    c = np.full((30, 2), 0.1, np.float32)
    c[:4] = 0.9                                                      # starts active
    ref = tracks(530, 300, 2, 80, 60)
    meds = (1, 11, 127)
    alone = {k: run(M, [ref], [p], (0.5,), meds, None, 10, 0) for k, p in (("a", a), ("b", b), ("c", c))}
    for order in ("ab", "ba", "bc", "cb", "ac", "ca", "abc"):
        ps = [dict(a=a, b=b, c=c)[k] for k in order]
        got = check(M, dev, [ref] * len(ps), ps, (0.5,), meds, None, 10, 0, device_path=False)
        for g in range(len(meds)):
            for i, k in enumerate(order):
                assert got[g][i][0] == alone[k][g][0][0] and np.array_equal(got[g][i][1], alone[k][g][0][1]), (order, g, k)
    # the leak would show: filtered as one buffer, the 4 + 4 active rows around the seam keep each other alive
    assert not W.activity(a, 0.5, 11).any() and not W.activity(c, 0.5, 11).any() and W.activity(np.concatenate([a, c]), 0.5, 11).any()


# ---- widths

@pytest.mark.parametrize("Cr,Ch", [(2, 1), (1, 3), (4, 5), (16, 16), (3, 16), (16, 2)])
def test_widths(M, dev, Cr, Ch):
    ref, pred, flags = W.make(540 + Cr * 17 + Ch, 1500, Cr, Ch, 10, 200, 300 if Cr < 16 else 2500, sad=True)
    check(M, dev, [ref], [pred], (0.4, 0.6), (1, 11), None, 10, 10)
    check(M, dev, [ref], [pred], (0.4, 0.6), (1, 11), [flags], 10, 10)


def test_ragged_batch_equals_each_recording_alone(M, dev):
    ins = [W.make(560, 2500, 4, 5, 10, 100, 200), W.make(561, 17, 2, 1, 10, 5, 5, th_delta=1), W.make(562, 5000, 6, 3, 10, 100, 300, th_delta=-20),
           (np.zeros((0, 1), np.uint8), np.zeros((0, 2), np.float32), None)]
    ths, meds = (0.45, 0.55), (1, 11)
    alone = [run(M, [r], [p], ths, meds, None, 10, 50) for r, p, _ in ins]
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0], [2, 0]):
        got = check(M, dev, [ins[i][0] for i in order], [ins[i][1] for i in order], ths, meds, None, 10, 50, device_path=order == [0, 1, 2, 3])
        for g in range(4):
            for at, i in enumerate(order):
                assert got[g][at][0] == alone[i][g][0][0] and np.array_equal(got[g][at][1], alone[i][g][0][1]), (order, g, i)
    again = run(M, [ins[0][0]], [ins[0][1]], ths, meds, None, 10, 50)
    for g in range(4):
        assert again[g][0][0] == alone[0][g][0][0] and np.array_equal(again[g][0][1], alone[0][g][0][1]) and again[g][0][2] == alone[0][g][0][2]


# ---- values

def test_special_values(M, dev):
    """Posteriors exactly at a threshold (not above it), NaN (never active, never the largest), +-inf (ordinary values), and a
    speech row of NaN only (recovers nobody)."""
    ref, pred, flags = W.make(570, 800, 3, 3, 10, 60, 90, sad=True)
    ths = (0.5, 0.3, 0.75)
    f32 = [np.float32(v) for v in ths]
    pred[5:9, 0], pred[5:9, 1], pred[5:9, 2] = f32[0], f32[1], f32[2]          # equal to the thresholds
    pred[12:16] = [np.nan, np.inf, -np.inf]
    pred[20:24] = np.nan                                                       # a row of NaN only
    pred[28:32] = [np.nan, 0.1, 0.1]                                           # the winner is not the NaN, lowest index on the tie
    pred[36:40] = [-np.inf, -np.inf, np.nan]                                   # -inf wins over NaN
    pred[44:48] = [np.nextafter(f32[1], np.float32(1)), np.nextafter(f32[1], np.float32(0)), 0.0]
    flags[4:50] = 1
    d = W.decisions(pred, 0.3)
    assert not d[5, 1] and d[5, 0] and d[12].tolist() == [False, True, False] and not d[20].any() and d[44].tolist() == [True, False, False]
    s = W.decisions(pred, 0.3, flags)
    assert not s[20].any() and s[28].tolist() == [False, True, False] and s[36].tolist() == [True, False, False]
    for sads in (None, [flags]):
        check(M, dev, [ref], [pred], ths, (1, 3, 11), sads, 10, 10)


def test_thresholds_out_of_order_and_repeated(M, dev):
    ref, pred, flags = W.make(580, 1500, 3, 4, 10, 150, 200, sad=True)
    ths = (0.7, 0.3, 0.5, 0.3, 0.7)
    got = check(M, dev, [ref], [pred], ths, (11, 1), [flags], 10, 50)
    for i, j in ((0, 4), (1, 3)):
        for k in range(2):
            a, b = got[i * 2 + k][0], got[j * 2 + k][0]
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert got[0][0][0] != got[2][0][0] and got[2][0][0] != got[3][0][0]


def test_one_point_equals_score_predictions(M, dev):
    ref, pred, flags = W.make(590, 1200, 3, 3, 10, 100, 150, sad=True)
    for kw in (dict(), dict(threshold=0.7, median=5), dict(sad=t(flags)), dict(median=1, collar=10, skip_overlap=True)):
        want = M.score_predictions(t(ref), t(pred), **kw)
        res = M.sweep_predictions(t(ref), t(pred), (kw.get("threshold", 0.5),), (kw.get("median", 11),), None if "sad" not in kw else [kw["sad"]],
                                  kw.get("collar", 50), 10, kw.get("skip_overlap", False))
        assert want["total"] > 0 and res.details == [[want]]
        assert res.best == (float(np.float32(kw.get("threshold", 0.5))), kw.get("median", 11), want["diarization error rate"])
        assert {k: v for k, v in res.table[0].items() if k not in ("threshold", "median")} == {k: want[k] for k in (
            "total", "correct", "confusion", "false alarm", "missed detection", "diarization error rate")}


@pytest.mark.parametrize("nth,meds", [(16, (1, 11)), (8, (1, 3, 11, 127))])
def test_grid_at_the_limit(M, dev, nth, meds):
    ref, pred, flags = W.make(600 + nth, 1500, 3, 4, 10, 150, 200, sad=True)
    ths = [round(0.2 + 0.6 * i / (nth - 1), 4) for i in range(nth)]
    got = check(M, dev, [ref, ref[:700]], [pred, pred[:75]], ths, meds, [flags, flags[:75]], 10, 50)
    assert len(got) == 32 and len({tuple(p[0][0]) for p in got}) >= 16


# ---- masks

def test_masks(M, dev):
    """A non-speech gap shorter than the median is bridged (the median comes after the gate), a speech row with nobody above the
    highest threshold recovers its largest speaker, and no mask at all is the plain path."""
    Th = 80
    pred = np.full((Th, 2), 0.1, np.float32)
    pred[:60, 0] = 0.9
    pred[62:70] = [0.2, 0.25]                                        # nobody above any threshold: speaker 1 is recovered
    flags = np.ones(Th, np.uint8)
    flags[20:24] = 0                                                 # a gap of 4 frames inside the speech of speaker 0
    flags[70:] = 0
    ref = np.repeat((pred > 0.5).astype(np.uint8), 10, axis=0)
    ths, meds = (0.5, 0.8), (1, 11)
    gated, bridged = W.activity(pred, 0.8, 1, flags), W.activity(pred, 0.8, 11, flags)
    assert not gated[20:24].any() and bridged[20:24, 0].all() and gated[62:70, 1].all() and not gated[62:70, 0].any() and not gated[70:].any()
    with_mask = check(M, dev, [ref], [pred], ths, meds, [flags], 10, 0)
    without = check(M, dev, [ref], [pred], ths, meds, None, 10, 0)
    assert with_mask[2][0][0] != without[2][0][0] and with_mask[2][0][0] != with_mask[3][0][0]
    assert without[3][0][0][1:4] == [0, 0, 0]                         # the reference is the plain decision: no error without a mask


# ---- totals, the metric object, graphs

def test_totals_accumulate_and_der_sweep_reports(M, dev):
    a = [W.make(610 + i, 900 + 100 * i, 3, 3, 10, 100, 150, sad=True) for i in range(3)]
    b = [W.make(620 + i, 700 + 50 * i, 2, 4, 10, 100, 150, sad=True) for i in range(2)]
    ths, meds = (0.35, 0.5, 0.65), (1, 11)
    totals = torch.zeros(6, 8, dtype=torch.int64, device=dev)
    sums = torch.zeros(6, 8, dtype=torch.int64, device=dev)
    for part in (a, b):
        counters, _, _ = M.sweep_counters([t(x[0]) for x in part], [t(x[1]) for x in part], ths, meds, [t(x[2]) for x in part], totals=totals)
        sums += counters.sum(dim=1)
    assert torch.equal(totals, sums) and int(totals[:, 0].min()) > 0
    metric = M.DerSweep(ths, meds)
    for part in (a, b):
        metric.add([t(x[0]) for x in part], [t(x[1]) for x in part], [t(x[2]) for x in part])
    rep = metric.report()
    assert torch.equal(metric.totals, totals) and rep.recordings == 5 and rep.details is None
    whole = M.sweep_predictions([t(x[0]) for x in a + b], [t(x[1]) for x in a + b], ths, meds, [t(x[2]) for x in a + b])
    assert rep.table == whole.table and rep.best == whole.best and rep.rates() == whole.rates()
    assert len(whole.details) == 6 and len(whole.details[0]) == 5
    want = [W.aggregate([W.sweep(x[0], x[1], [th], [k], x[2])[0] for x in a + b]) for th in ths for k in meds]
    assert [[r[k] for k in ("total", "missed detection", "false alarm", "confusion", "correct")] for r in rep.table] == [w[0][:5] for w in want]
    assert [r["diarization error rate"] for r in rep.table] == [w[1] for w in want]
    g = min(range(6), key=lambda i: (want[i][1], i))
    assert rep.best == (float(np.float32(ths[g // 2])), meds[g % 2], want[g][1])
    assert len({w[1] for w in want}) >= 3
    metric.reset()
    assert metric.report().table[0]["total"] == 0


def test_a_bad_median_on_the_device_marks_its_points_only(M, dev):
    """Device-tensor grids are used as they are: a median the kernel does not take is not scored (counters -1, no mapping,
    nothing added to the totals), the other points are."""
    ref, pred, _ = W.make(630, 900, 2, 2, 10, 100, 150)
    ths = torch.tensor([0.5], dtype=torch.float32, device=dev)
    meds = torch.tensor([11, 4, 129, 1], dtype=torch.int32, device=dev)
    totals = torch.zeros(4, 8, dtype=torch.int64, device=dev)
    counters, cooc, mapping = M.collar_der_sweep_packed(M.pack_references([t(ref)]), M.pack_predictions([t(pred)]), ths, meds, totals=totals)
    counters, mapping = counters.cpu().tolist(), mapping.cpu().tolist()
    want = W.sweep(ref, pred, [0.5], [11, 1])
    assert counters[0][0] == want[0]["counters"] and counters[3][0] == want[1]["counters"]
    assert counters[1][0] == [-1] * 8 and counters[2][0] == [-1] * 8 and mapping[1][0] == [-1] * 16
    assert totals.cpu().tolist() == [want[0]["counters"], [0] * 8, [0] * 8, want[1]["counters"]]


def test_graph_capture_and_replay(M, dev):
    ins = [W.make(640 + i, 3000, 4, 5, 10, 600, 900, sad=True) for i in range(3)]
    ths, meds = (0.4, 0.6), (1, 11)
    ref_batch = M.pack_references([t(ins[0][0])])
    pred_batch = M.pack_predictions([t(ins[0][1])], [t(ins[0][2])])
    th_dev = torch.tensor(ths, dtype=torch.float32, device=dev)
    med_dev = torch.tensor(meds, dtype=torch.int32, device=dev)
    out = tuple(torch.full_like(x, -1) for x in M.collar_der_sweep_packed(ref_batch, pred_batch, th_dev, med_dev))
    totals = torch.zeros(4, 8, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        M.collar_der_sweep_packed(ref_batch, pred_batch, th_dev, med_dev, out=out, totals=totals)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        M.collar_der_sweep_packed(ref_batch, pred_batch, th_dev, med_dev, out=out, totals=totals)
    totals.zero_()
    sums = np.zeros((4, 8), np.int64)
    for ref, pred, flags in (ins[1], ins[2], ins[1]):
        ref_batch[0].copy_(t(ref))
        pred_batch[0].copy_(t(pred))
        pred_batch[2].copy_(t(flags))
        for x in out:
            x.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        want = W.sweep(ref, pred, ths, meds, flags)
        for g in range(4):
            assert want[g]["counters"][0] > 100 and want[g]["best"] > 0
            assert out[0][g, 0].cpu().tolist() == want[g]["counters"] and np.array_equal(out[1][g, 0].cpu().numpy(), want[g]["cooc"])
            mapping = {j: i for j, i in enumerate(out[2][g, 0].cpu().tolist()) if i >= 0}
            assert R.valid_mapping(mapping, want[g]["cooc"], want[g]["best"])
        sums += np.array([w["counters"] for w in want])
    assert np.array_equal(totals.cpu().numpy(), sums)


# ---- the entry points that were there before

def test_existing_collar_der_entry_points_are_unchanged(M, dev):
    """The assignment kernel now serves both entries: a golden through the three existing ones."""
    for name in ("der_c3_T3000", "der_c16_sparse"):
        case = next(c for c in R.CASES if c["name"] == name)
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        meta = ast.literal_eval(str(z["meta"]))
        ref, hyp = R.inputs(case)
        counters, cooc, mapping = M.collar_der_counters(t(ref), t(hyp), case["collar"], case["sub"])
        assert counters.cpu().tolist() == [z["counters"].tolist()] and np.array_equal(cooc.cpu().numpy()[0], z["cooc"])
        m = {j: i for j, i in enumerate(mapping.cpu().tolist()[0]) if i >= 0}
        assert R.valid_mapping(m, z["cooc"], int(z["best"]))
        d = M.collar_der(t(ref), t(hyp), case["collar"], case["sub"])
        assert [d[k] for k in ("total", "missed detection", "false alarm", "confusion", "correct")] == z["counters"].tolist()[:5]
        assert d["mapping"] == m and meta is not None
        metric = M.CollarDER(case["collar"], case["sub"])
        two = metric.score_batch([t(ref), t(ref)], [t(hyp), t(hyp)])
        assert two == [d, d] and metric.report()["total"] == 2 * d["total"]
