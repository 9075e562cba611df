"""CPU: the host side of the live segment tracker (live_rttm.py) -- the RTTM formatting shared with make_rttm, a model of the
kernel's incremental state machine (csrc/segtrack.hip) against the reference's make_rttm for many chunkings, the poll
bookkeeping, and the parameter domain of the Python API and of the C ABI."""
import random

import numpy as np
import pytest
import torch

from oracle import postproc_ref as P

EINVAL = -1


def lines(rttm):
    return [(k, l) for k in rttm for l in rttm[k]]


def pred_from_segments(segs, T):
    x = torch.zeros(T, len(segs))
    for s, ss in enumerate(segs):
        for a, b in ss:
            x[a:b, s] = 1.0
    return x


def random_segments(rng, T, S):
    segs = []
    for _ in range(S):
        cut = sorted(rng.sample(range(T + 1), 2 * rng.randrange(0, min(8, (T + 1) // 2) + 1)))
        segs.append([(cut[i], cut[i + 1]) for i in range(0, len(cut), 2) if cut[i] < cut[i + 1]])
    return segs


@pytest.mark.parametrize("shift,sub,rate", [(80, 10, 8000), (160, 1, 16000), (80, 10, 16000), (10, 3, 8000)])
def test_shared_formatting_matches_reference(shift, sub, rate):
    from fs_eend_amd.postproc import rttm_lines
    rng = random.Random(shift + sub)
    for T, S in ((1, 1), (7, 3), (500, 5), (36000, 4), (137, 11)):
        segs = random_segments(rng, T, S)
        want = P.make_rttm("rec7", pred_from_segments(segs, T), frame_shift=shift, subsampling=sub, sampling_rate=rate, median=1)
        got = rttm_lines("rec7", segs, frame_shift=shift, subsampling=sub, sampling_rate=rate)
        assert list(got) == list(want)
        assert lines(got) == lines(want)


class Model:
    """One slot of csrc/segtrack.hip in Python: per track the last k - 1 raw decisions (bit word, oldest at bit 0) and the start
    of the open segment; closes appended by end frame, then track."""

    def __init__(self, S, k):
        self.S, self.k, self.h = S, k, k // 2
        self.hist = [0] * S
        self.st = [-1] * S
        self.n = 0
        self.ring = []

    def _settle(self, f, u):
        for s in range(self.S):
            if f[s] and self.st[s] < 0:
                self.st[s] = u
            elif not f[s] and self.st[s] >= 0:
                self.ring.append((s, self.st[s], u))
                self.st[s] = -1

    def feed(self, dec, end=False):
        k, h, keep = self.k, self.h, (1 << (self.k - 1)) - 1
        for row in dec:
            t = self.n
            w = [self.hist[s] | (int(row[s]) << (k - 1)) for s in range(self.S)]
            if t >= h:
                self._settle([bin(x).count("1") >= h + 1 for x in w], t - h)
            self.hist = [(x >> 1) & keep for x in w]
            self.n += 1
        if end:
            for t in range(self.n, self.n + h):
                if t >= h:
                    self._settle([bin(x).count("1") >= h + 1 for x in self.hist], t - h)
                self.hist = [x >> 1 for x in self.hist]
            self._settle([False] * self.S, self.n)


def tracks(rng, T, S, kind):
    noise = np.random.default_rng(rng.randrange(1 << 30)).random((T, S))
    if kind == "noise":
        return noise < 0.5
    runs = np.zeros((T, S), dtype=bool)
    for s in range(S):
        t, on = 0, rng.random() < 0.5
        while t < T:
            n = rng.randrange(1, 30)
            runs[t:t + n, s] = on
            on, t = not on, t + n
    return runs ^ (noise < 0.05)


@pytest.mark.parametrize("k", [1, 5, 11, 63])
def test_incremental_model_matches_make_rttm(k):
    rng = random.Random(k)
    for T in (0, 1, 2, k // 2, k - 1, k, k + 1, 97, 400):
        for kind in ("noise", "runs"):
            S = rng.randrange(1, 7)
            dec = tracks(rng, T, S, kind)
            pred = torch.from_numpy(dec.astype(np.float32))
            want = [[(a, b) for a, b in ss] for ss in P.segments(P.activity(pred, 0.5, k) if T else np.zeros((0, S), np.int64))]
            for _ in range(4):
                m = Model(S, k)
                t, ring = 0, []
                while t < T:
                    n = rng.choice([1, 1, 7, rng.randrange(0, T + 1)])
                    m.feed(dec[t:t + n])
                    t += n
                    if rng.random() < 0.3:
                        ring += m.ring
                        m.ring = []
                m.feed(dec[T:], end=True)
                ring += m.ring
                assert [(u, s) for s, _, u in ring] == sorted((u, s) for s, _, u in ring)     # by end frame, then track
                got = [[(a, b) for s2, a, b in ring if s2 == s] for s in range(S)]
                assert got == want, (k, T, kind)


def box_of(rows, cap):
    from fs_eend_amd import live_rttm as LR
    b = torch.zeros(len(rows), LR.HDR + 3 * cap, dtype=torch.int32)
    for s, (frames, segs, ovf) in enumerate(rows):
        b[s, 0], b[s, 1], b[s, 2] = frames, len(segs), ovf
        for i, seg in enumerate(segs):
            b[s, LR.HDR + 3 * i:LR.HDR + 3 * i + 3] = torch.tensor(seg)
    return b


def test_poll_bookkeeping():
    from fs_eend_amd import live_rttm as LR
    log = LR.SegmentLog(4, ntracks=3, capacity=4)
    log.take(box_of([(0, [], 0)] * 4, 4))
    assert log.pop_pending() == {}
    log.take(box_of([(9, [(1, 0, 4), (0, 2, 5)], 0), (3, [], 0), (20, [(2, 3, 7)], 0), (0, [], 0)], 4))
    assert log.pop_pending() == {0: [(1, 0, 4), (0, 2, 5)], 2: [(2, 3, 7)]}
    assert log.pop_pending() == {}
    log.take(box_of([(30, [(1, 6, 12), (1, 13, 20)], 0), (3, [], 0), (40, [(0, 1, 2)] * 4, 1), (0, [], 0)], 4))
    assert log.pending[0] == [(1, 6, 12), (1, 13, 20)] and log.unreported == {2} and log.overflowed[2] and not log.overflowed[0]
    assert log.by_track(0) == [[(2, 5)], [(0, 4), (6, 12), (13, 20)], []]
    log.reset(2)
    assert log.segs[2] == [] and not log.overflowed[2] and log.unreported == set() and 2 not in log.pending
    assert log.pop_pending() == {0: [(1, 6, 12), (1, 13, 20)]}
    log.close(0)
    log.take(box_of([(30, [(1, 0, 1)], 0)] + [(0, [], 0)] * 3, 4))          # a closed slot's leftovers are ignored
    assert log.pop_pending() == {}
    assert log.state[0] == LR.FREE and log.segs[0] == []
    log.ended([1])
    with pytest.raises(LR.SlotError):
        log.check_feed([1], [])
    with pytest.raises(LR.SlotError):
        log.check_feed([0], [])
    with pytest.raises(LR.SlotError):
        log.check_feed([2], [2, 2])
    with pytest.raises(LR.SlotError):
        log.check_feed([7], [])
    log.check_feed([2], [2, 3])


def test_segments_read_between_polls_stay_pending():
    """rttm() reads every slot's ring from the device between two polls: those segments are still returned by the next poll,
    exactly once, while a reset or close of one slot drops its own pending segments only."""
    from fs_eend_amd import live_rttm as LR
    log = LR.SegmentLog(3, ntracks=2, capacity=8)
    log.take(box_of([(5, [(0, 0, 3)], 0), (5, [(1, 1, 4)], 0), (5, [(0, 2, 5)], 0)], 8))     # as rttm(0) does
    assert log.by_track(0) == [[(0, 3)], []]
    log.take(box_of([(9, [(1, 4, 8)], 0), (9, [], 0), (9, [(1, 0, 9)], 0)], 8))               # as rttm(1) does
    log.reset(2)
    assert log.pop_pending() == {0: [(0, 0, 3), (1, 4, 8)], 1: [(1, 1, 4)]}
    assert log.pop_pending() == {}
    assert log.segs[0] == [(0, 0, 3), (1, 4, 8)] and log.segs[1] == [(1, 1, 4)]


def test_bad_parameters_rejected():
    from fs_eend_amd import live_rttm as LR
    from fs_eend_amd.lib import EendHipError
    for kw in (dict(median=0), dict(median=2), dict(median=65), dict(median=11.0), dict(ntracks=0), dict(ntracks=65),
               dict(col0=-1), dict(capacity=0), dict(threshold=float("nan"))):
        args = dict(ntracks=3, col0=1, threshold=0.5, median=11, capacity=8)
        args.update(kw)
        with pytest.raises(ValueError):
            LR.check_params(**args)
        with pytest.raises(ValueError):
            LR.SegmentTracker(2, **args)
    LR.check_params(64, 0, 0.5, 63, 1)
    with pytest.raises(LR.SlotError):
        LR.SegmentLog(0, 3, 8)
    with pytest.raises(EendHipError):
        LR.SegmentTracker(2, 3, device="cpu")                       # no CPU fallback


def test_cabi_domain(hip_lib):
    """Arguments outside the domain return EEND_EINVAL before any launch (the pointers are never touched)."""
    from fs_eend_amd import lib as L
    f = L.load().eend_segtrack_feed_f32
    p = 64                                                          # never dereferenced: every call below is rejected or empty
    ok = dict(desc=p, counts=p, ends=None, n=2, ld=11, col0=1, ntracks=10, thr=0.5, k=11, is_prob=0, hist=p, open=p, box=p,
              S=4, cap=16)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return f(a["desc"], a["counts"], a["ends"], a["n"], a["ld"], a["col0"], a["ntracks"], a["thr"], a["k"], a["is_prob"],
                 a["hist"], a["open"], a["box"], a["S"], a["cap"], None)

    for kw in (dict(k=0), dict(k=2), dict(k=63 + 2), dict(k=-1), dict(ntracks=0), dict(ntracks=65, ld=80), dict(ld=10),
               dict(col0=-1), dict(n=-1), dict(n=5), dict(S=0), dict(cap=0), dict(desc=None), dict(counts=None),
               dict(hist=None), dict(open=None), dict(box=None), dict(S=1 << 20, cap=1 << 12, n=0)):
        assert call(**kw) == EINVAL, kw
    assert call(n=0) == 0                                           # nothing to do: no launch
