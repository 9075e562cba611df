"""GPU: live RTTM segments (live_rttm.SegmentTracker on csrc/segtrack.hip, SegmentSession) against make_rttm, exactly: the
reference's own golden lines under every chunking, slot placement, neighbours and poll cadence; random logits up to one hour;
the logits decision bit for bit against torch.sigmoid at the threshold; both multi-stream sessions and the audio session end to
end; and ring overflow confined to its slot."""
import ast
import math
import os
import random

import numpy as np
import pytest
import torch

from fs_eend_amd.postproc import rttm_lines
from oracle import fixtures as FX
from oracle import gen_golden_post as G
from tests.helpers import build_fs_mirror, build_ls_mirror
from tests.test_feature_gpu import wave

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAN = float("nan")


def flat(rttm):
    return [f"{k}\t{l}" for k in sorted(rttm, key=int) for l in rttm[k]]


def same_rttm(got, want):
    assert list(got) == list(want)
    assert flat(got) == flat(want)


def same_bits(a, b):
    """torch.equal with NaN equal to NaN (the NaN-fed streams)"""
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())


def cuts(rng, T, how):
    """Row counts of one chunking of T rows."""
    if how == "one":
        return [1] * T
    if how == "seven":
        return [7] * (T // 7) + ([T % 7] if T % 7 else [])
    if how == "whole":
        return [T]
    out, t = [], 0
    while t < T:
        n = rng.choice([0, 1, 2, 3, 5, 11, 40, rng.randrange(1, T + 1)])
        out.append(min(n, T - t))
        t += out[-1]
    return out


def by_track(segs, ntracks):
    per = [[] for _ in range(ntracks)]
    for spk, a, b in segs:
        per[spk].append((a, b))
    return per


def drive(tr, streams, rng, poll_p=0.2, rttm_p=0.2):
    """streams: {slot: (rows tensor, [row counts])}: every call feeds the next chunk of every slot that still has one (a slot
    ends with its last chunk or in a call of its own), with polls and rttm() reads of random slots at random points.
    -> {slot: its segments as the polls returned them, concatenated}; each slot's equal its rttm() lines."""
    polled = {s: [] for s in streams}

    def poll():
        for s, segs in tr.poll().items():
            assert [(u, spk) for spk, _, u in segs] == sorted((u, spk) for spk, _, u in segs)   # by end frame, then track
            polled[s] += segs

    pos = {s: 0 for s in streams}
    k = {s: 0 for s in streams}
    while any(k[s] <= len(c) for s, (_, c) in streams.items()):
        rows, end = {}, []
        for s, (x, c) in streams.items():
            if k[s] > len(c):
                continue
            if k[s] == len(c):
                end.append(s)
            else:
                rows[s] = x[pos[s]:pos[s] + c[k[s]]]
                pos[s] += c[k[s]]
                if k[s] == len(c) - 1 and rng.random() < 0.5:
                    end.append(s)
                    k[s] += 1
            k[s] += 1
        tr.feed(rows, end=end)
        if rng.random() < rttm_p:
            tr.rttm(rng.choice(sorted(streams)), "any")                # reads every slot's ring; the next poll still returns them
        if rng.random() < poll_p:
            poll()
    poll()
    for s in streams:
        same_rttm(rttm_lines("p", by_track(polled[s], tr.ntracks)), tr.rttm(s, "p"))
    return polled


@pytest.mark.parametrize("case", [c["name"] for c in G.RTTM_CASES])
def test_golden_lines_under_any_chunking(hip_lib, dev, case):
    from fs_eend_amd.live_rttm import SegmentTracker
    z = np.load(os.path.join(GOLD, case + ".npz"), allow_pickle=False)
    meta = ast.literal_eval(str(z["meta"]))
    want = [str(l) for l in z["lines"]]
    pred = G.post_inputs(meta["seed"], meta["T"], meta["S"], meta["kind"]).to(dev)
    T, S = pred.shape
    rng = random.Random(case)
    g = torch.Generator().manual_seed(3)
    noise = lambda n: torch.rand(n, S, generator=g).to(dev)
    for layout in range(2):
        tr = SegmentTracker(7, S, col0=0, threshold=meta["threshold"], median=meta["median"], is_prob=True, capacity=4096, device=dev)
        hows = ["one", "seven", "random", "whole", "random"]
        slots = [1, 3, 4, 5, 6] if layout == 0 else [6, 0, 2, 1, 5]
        streams = {s: (pred, cuts(rng, T, h)) for s, h in zip(slots, hows)}
        for s in range(7):
            if s not in streams:
                n = rng.randrange(0, 300)
                streams[s] = (noise(n), cuts(rng, n, "random"))
        if layout == 1:
            tr.feed({0: noise(50)}, end=[0])                      # slot 0 reused: a NaN-fed stream first
            tr.reset(0)
            tr.feed({0: torch.full((30, S), NAN, device=dev)})
            tr.reset(0)
        drive(tr, streams, rng)
        for s, h in zip(slots, hows):
            assert flat(tr.rttm(s, "rec0")) == want, (case, s, h)


def smooth_logits(T, C, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T + 41, C, generator=g)
    x = torch.nn.functional.avg_pool1d(x.t().unsqueeze(0), 41, 1).squeeze(0).t()[:T] * 8
    return (x + 0.8 * torch.randn(T, C, generator=g)).to(dev)


@pytest.mark.parametrize("k", [1, 5, 11])
def test_random_logits_up_to_one_hour(hip_lib, dev, k):
    from fs_eend_amd import postproc
    from fs_eend_amd.live_rttm import SegmentTracker
    C, col0 = 12, 1
    rng = random.Random(k)
    for thr in (0.4, 0.5, 0.7):
        lens = [36000 if thr == 0.5 else 3000, 5000, 1, 0, 777]
        L = [smooth_logits(T, C, 100 * k + i, dev) for i, T in enumerate(lens)]
        tr = SegmentTracker(len(lens), C - col0, col0=col0, threshold=thr, median=k, capacity=1 << 16, device=dev)
        streams = {s: (x, cuts(rng, x.shape[0], "whole" if s == 0 else "random")) for s, x in enumerate(L)}
        drive(tr, streams, rng, poll_p=0.5)
        for s, x in enumerate(L):
            want = postproc.make_rttm("r", torch.sigmoid(x[:, col0:]), threshold=thr, median=k) if x.shape[0] else {}
            same_rttm(tr.rttm(s, "r"), want)
        assert len(flat(tr.rttm(0, "r"))) > 100


def test_sigmoid_decision_bit_exact(hip_lib, dev):
    """k = 1, one frame per track: the tracker's decisions equal torch.sigmoid(x) > threshold for a dense sweep of float32
    logits around logit(threshold) and the special values."""
    from fs_eend_amd.live_rttm import SegmentTracker
    specials = [0.0, -0.0, math.inf, -math.inf, NAN, 1e-45, -1e-45, 1e-38, -1e-38, 88.7, -88.7, 103.9, -103.9, 3.4e38, -3.4e38,
                17.0, -17.0, 1e-7, -1e-7]
    for thr in (0.4, 0.5, 0.7, 0.25, 0.9):
        x0 = np.float32(math.log(thr / (1 - thr)))
        bits = np.array([x0], dtype=np.float32).view(np.int32)[0]
        sweep = np.concatenate([(np.arange(-6000, 6001, dtype=np.int64) + bits).astype(np.int32).view(np.float32),
                                np.array(specials, dtype=np.float32)])
        xs = torch.from_numpy(sweep.copy())
        n = xs.numel()
        S = (n + 63) // 64
        grid = torch.full((S * 64,), -math.inf)
        grid[:n] = xs
        grid = grid.view(S, 1, 64).to(dev)
        tr = SegmentTracker(S, 64, col0=0, threshold=thr, median=1, capacity=64, device=dev)
        tr.feed({s: grid[s] for s in range(S)}, end=range(S))
        got = torch.zeros(S, 64, dtype=torch.bool)
        for s, segs in tr.poll().items():
            for spk, a, b in segs:
                assert (a, b) == (0, 1)
                got[s, spk] = True
        want = (torch.sigmoid(grid.view(S, 64)) > thr).cpu()
        bad = (got != want).view(-1)[:n].nonzero().view(-1)
        assert bad.numel() == 0, [(float(xs[i]), bool(want.view(-1)[i])) for i in bad[:8]]


# ---------------------------------------------------------------------------------------------- sessions
def _fs(dev):
    from fs_eend_amd.fs_stream import StreamingTransformerEDADiarization, copy_params_from_masked_to_streaming
    meta, _ = FX.load_case("fs_stream_T60")
    m = build_fs_mirror(meta).to(dev)
    sm = StreamingTransformerEDADiarization(in_size=meta["in_size"], **meta["cfg"]).eval().to(dev)
    copy_params_from_masked_to_streaming(m, sm)
    src = FX.make_src([meta["T"]], meta["in_size"], meta["xseed"])[0].to(dev)
    return sm, meta["C"], src


def _ls(dev):
    meta, _ = FX.load_case("ls_stream_T120")
    m = build_ls_mirror(meta).to(dev)
    src = FX.make_src([meta["T"]], meta["in_size"], meta["xseed"])[0].to(dev)
    return m, meta["C"], src


class Driver:
    """streams[name] = (frames, start step): a stream takes a slot at its start step, pushes its frames (skipping the steps in
    pauses[name]), flushes and is closed once done -- after its lines are read when the session is a SegmentSession."""

    def __init__(self, ses, rng=None):
        self.ses, self.rng = ses, rng
        self.out, self.lines, self.slot, self.where, self.polled = {}, {}, {}, {}, {}

    def poll(self):
        by_slot = {s: n for n, s in self.slot.items()}
        for s, segs in self.ses.poll().items():
            self.polled[by_slot[s]] += segs

    def run(self, streams, pauses=None):
        pauses = pauses or {}
        pos = {n: 0 for n in streams}
        step = 0
        while True:
            for n, (_, start) in streams.items():
                if start == step:
                    self.slot[n] = self.where[n] = self.ses.open()
                    self.out[n], self.polled[n] = [], []
            push, flush = {}, []
            for n, s in self.slot.items():
                fr = streams[n][0]
                if self.ses.state(s) != "open" or step in pauses.get(n, ()):
                    continue
                if pos[n] < len(fr):
                    push[s] = fr[pos[n]]
                    pos[n] += 1
                else:
                    flush.append(s)
            y = self.ses.step(push=push, flush=flush)
            by_slot = {s: n for n, s in self.slot.items()}
            for s, v in y.items():
                self.out[by_slot[s]].append(v.reshape(1, -1))
            if self.rng is not None and self.slot and self.rng.random() < 0.15:
                self.ses.rttm(self.rng.choice(sorted(self.slot.values())), "any")     # a live slot's lines between polls
            if self.rng is not None and self.rng.random() < 0.15:
                self.poll()
            for n, s in list(self.slot.items()):
                if self.ses.state(s) == "done":
                    if self.rng is not None:
                        self.poll()
                        self.lines[n] = self.ses.rttm(s, "rec")
                        same_rttm(rttm_lines("rec", by_track(self.polled[n], self.ses.tracker.ntracks)), self.lines[n])
                    self.ses.close(s)
                    del self.slot[n]
            step += 1
            if not self.slot and all(start < step for _, start in streams.values()):
                return {n: torch.cat(v) if v else None for n, v in self.out.items()}


def _scenario(src, C_in, dev, seed):
    g = torch.Generator().manual_seed(seed)
    other = lambda n: (torch.randn(n, C_in, generator=g) * 2 - 3).to(dev)
    nan = other(30)
    nan[8:] = NAN
    streams = {"x": (src, 0), "nan": (nan, 0), "late": (src[:40], 9), "empty": ([], 2), "o1": (other(25), 1), "short": (src[:3], 4),
               "re": (src, 45)}                                     # "re" takes a slot that an earlier stream left
    pauses = {"x": [5, 6, 7, 30], "late": [12, 13, 20]}
    return streams, pauses


@pytest.mark.parametrize("kind", ["fs", "ls"])
def test_segment_session_exact(hip_lib, dev, kind):
    from fs_eend_amd import postproc
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    from fs_eend_amd.live_rttm import SegmentSession
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    if kind == "fs":
        sm, C, src = _fs(dev)
        mk = lambda g: FsMultiStreamSession(sm, 6, C, cap=16, use_graph=g)
    else:
        sm, C, src = _ls(dev)
        src = src[:70].contiguous()
        mk = lambda g: LsMultiStreamSession(sm, 6, C, use_graph=g)
    streams, pauses = _scenario(src, src.shape[1], dev, seed=7)
    bare = Driver(mk(True)).run(streams, pauses)
    allp = torch.sigmoid(torch.cat([v for v in bare.values() if v is not None])[:, 1:])
    allp = allp[~allp.isnan()]
    thr = float(allp.median())                                      # both decisions occur whatever the random weights give
    results = []
    for graph, seed in ((True, 1), (True, 2), (False, 3)):
        d = Driver(SegmentSession(mk(graph), threshold=thr, median=5), random.Random(seed))
        got = d.run(streams, pauses)
        for n, v in bare.items():
            assert (v is None and got[n] is None) or same_bits(got[n], v), (n, graph)
        for n, v in got.items():
            want = postproc.make_rttm("rec", torch.sigmoid(v[:, 1:]), threshold=thr, median=5) if v is not None else {}
            same_rttm(d.lines[n], want)
        results.append({n: flat(l) for n, l in d.lines.items()})
    assert results[0] == results[1] == results[2]
    assert results[0]["x"] == results[0]["re"]                      # the same stream later, in a slot another stream left
    assert sum(len(v) for v in results[0].values()) > 10


def test_audio_session_through_wrapper(hip_lib, dev):
    from fs_eend_amd import postproc
    from fs_eend_amd.audio_stream import AudioStreamSession
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    from fs_eend_amd.live_rttm import SegmentSession
    sm, C, _ = _fs(dev)
    waves = [wave(8000 * 3 + 4321, 1), wave(8000 * 5 + 79, 3)]
    runs = []
    for seed in (0, 1):
        rng = random.Random(seed)
        ases = AudioStreamSession(SegmentSession(FsMultiStreamSession(sm, 3, C, cap=64), threshold=0.5, median=11))
        assert ases.fe.input_transform == "logmel23"
        slots = [ases.open() for _ in waves]
        pos = [0] * len(waves)
        logits = [[] for _ in waves]
        while any(p < y.size for p, y in zip(pos, waves)):
            push = {}
            for i, (s, y) in enumerate(zip(slots, waves)):
                if pos[i] < y.size and rng.random() < 0.8:
                    m = rng.randrange(0, 5000)
                    push[s] = torch.from_numpy(y[pos[i]:pos[i] + m])
                    pos[i] += m
            for s, v in ases.push(push).items():
                logits[slots.index(s)].append(v)
            if rng.random() < 0.3:
                ases.ses.poll()
        for s, v in ases.end(slots).items():
            logits[slots.index(s)].append(v)
        out = []
        for i, s in enumerate(slots):
            L = torch.cat(logits[i])
            got = ases.ses.rttm(s, f"w{i}")
            same_rttm(got, postproc.make_rttm(f"w{i}", torch.sigmoid(L[:, 1:])))
            out.append((flat(got), L))
            ases.close(s)
        runs.append(out)
    for (la, La), (lb, Lb) in zip(*runs):
        assert la == lb and torch.equal(La, Lb)


def test_ring_overflow_confined_to_its_slot(hip_lib, dev):
    from fs_eend_amd import postproc
    from fs_eend_amd.lib import EendHipError
    from fs_eend_amd.live_rttm import SegmentTracker
    C = 4
    good = [smooth_logits(300, C, 40 + i, dev) for i in range(2)]
    noisy = torch.randn(400, C, generator=torch.Generator().manual_seed(9)).to(dev)
    tr = SegmentTracker(3, C - 1, col0=1, median=1, capacity=4, device=dev)
    raised = []
    for t in range(300):
        rows = {0: good[0][t:t + 1], 2: good[1][t:t + 1]}
        if t == 10:
            rows[1] = noisy
        tr.feed(rows, end=[0, 2] if t == 299 else [])
        try:
            tr.poll()
        except EendHipError as e:
            assert "slot(s) [1]" in str(e) and e.slots == [1]
            raised.append(t)
    assert raised == [10]
    for s, x in ((0, good[0]), (2, good[1])):
        same_rttm(tr.rttm(s, "r"), postproc.make_rttm("r", torch.sigmoid(x[:, 1:]), median=1))
    with pytest.raises(EendHipError, match="slot 1"):
        tr.rttm(1, "r")
    tr.reset(1)                                                     # the slot serves a new stream again
    for t in range(300):
        tr.feed({1: good[0][t:t + 1]}, end=[1] if t == 299 else [])
        tr.poll()
    same_rttm(tr.rttm(1, "r"), postproc.make_rttm("r", torch.sigmoid(good[0][:, 1:]), median=1))
