"""GPU: the external speech-activity mask, exactly (integers and strings, no tolerance): postproc.sad_func / activity /
make_rttm(sad=) on csrc/postproc.hip sad_fuse_kernel against the goldens of the reference's own sad_func; the live tracker's
SAD instantiation (csrc/segtrack.hip) against the same goldens under every chunking, at the 16-row batch edge, at 1 / 11 / 64
tracks, beside larger untracked columns, on NaN and -inf rows and in logits mode; both multi-stream sessions through step,
step_frames and prefill; a snapshot taken while flags wait for their rows; and the audio wrapper's refusal."""
import ast
import os
import random

import numpy as np
import pytest
import torch

from tests import sad_ref as R
from tests.test_live_rttm import NAN, _fs, _ls, _scenario, by_track, cuts, flat, same_bits, same_rttm, smooth_logits

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = float("inf")
IDS = [c["name"] for c in R.CASES]


def golden(case):
    z = np.load(os.path.join(GOLD, case["name"] + ".npz"), allow_pickle=False)
    return ast.literal_eval(str(z["meta"])), z["flags"], z["fused"], [str(l) for l in z["lines"]]


# ---------------------------------------------------------------------------------------------- whole files
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_batch_against_golden(hip_lib, dev, case):
    from fs_eend_amd import postproc
    _, flags, fused, lines = golden(case)
    pred, f = R.inputs(case)
    thr, k, T, S = case["threshold"], case["median"], case["T"], case["S"]
    sad = torch.from_numpy(f).float().unsqueeze(-1)                   # (T, 1) float, as the reference's caller passes it
    decision = torch.where(pred > thr, 1, 0)
    got = postproc.sad_func(decision, sad, pred, threshold=thr)       # CPU inputs are moved to the GPU
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (T, S)
    assert np.array_equal(got.cpu().numpy().astype(np.uint8), fused)
    p = pred.to(dev)
    assert torch.equal(postproc.sad_func(decision.to(dev), sad.to(dev), p, threshold=thr), got)
    wide = torch.cat([torch.full((T, 1), 9.0), pred, torch.full((T, 2), 7.0)], dim=1).to(dev)
    view = wide[:, 1:1 + S]                                           # a strided view beside larger columns
    assert view.stride(0) == S + 3 and torch.equal(postproc.sad_fuse(view, f, thr), got)
    for x in (p, view):
        for m in (torch.from_numpy(f), torch.from_numpy(f).to(dev).unsqueeze(-1), sad, f.astype(bool), (f * 3).tolist()):
            assert flat(postproc.make_rttm("rec0", x, threshold=thr, median=k, sad=m)) == lines
    act = postproc.activity(p, thr, k, sad=f)
    assert act.dtype == torch.uint8
    assert np.array_equal(act.cpu().numpy(), R.P.median_binary(fused.astype(np.int64), k))


def test_batch_without_mask_unchanged_and_rules(hip_lib, dev):
    from fs_eend_amd import postproc
    pred, f = R.inputs(R.CASES[0])
    p = pred.to(dev)
    assert torch.equal(postproc.activity(p, 0.5, 11), postproc.activity(p, 0.5, 11, sad=None))
    same_rttm(postproc.make_rttm("r", p, sad=None), postproc.make_rttm("r", p))
    assert flat(postproc.make_rttm("r", p)) != flat(postproc.make_rttm("r", p, sad=f))
    for bad in (f[:-1], np.stack([f, f], axis=1), f.reshape(1, -1)):
        with pytest.raises(ValueError):
            postproc.make_rttm("r", p, sad=bad)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(400, 5, generator=g)                               # the rules the reference leaves open
    x[torch.rand(400, 5, generator=g) < 0.2] = NAN
    x[torch.rand(400, 5, generator=g) < 0.1] = -INF
    x[torch.rand(400, 5, generator=g) < 0.1] = 0.0
    x[10:20] = NAN
    x[30:35] = -INF
    x[40:45] = 0.0
    fl = R.run_flags(77, 400, longest=4) * 5                          # any non-zero flag is speech
    fl[10:20:2] = 1
    for thr in (0.5, 0.9, 1.5):
        want = R.sad_fuse(x, fl, thr)
        assert np.array_equal(postproc.sad_fuse(x.to(dev), fl, thr).cpu().numpy(), want)
        assert want[10:20].sum() == 0 and want[30:35, 0].sum() == int((fl[30:35] != 0).sum())
    one = postproc.sad_fuse(torch.rand(70000, 1, generator=g).to(dev), np.ones(70000, np.uint8), 2.0)     # more than one block
    assert float(one.sum()) == 70000


# ---------------------------------------------------------------------------------------------- the tracker
def chunks(rng, T, how):
    if isinstance(how, int):
        return [how] * (T // how) + ([T % how] if T % how else [])
    return cuts(rng, T, how)


def drive(tr, streams, rng):
    """streams: {slot: (rows, flags, [row counts])}: every call feeds the next chunk of every slot that still has one, flags as
    a list, an array or a tensor; a stream ends with its last chunk or in a call of its own.  -> the polled segments per slot."""
    polled = {s: [] for s in streams}
    pos = {s: 0 for s in streams}
    k = {s: 0 for s in streams}
    while any(k[s] <= len(c) for s, (_, _, c) in streams.items()):
        rows, end, sad = {}, [], {}
        for s, (x, f, c) in streams.items():
            if k[s] > len(c):
                continue
            if k[s] == len(c):
                end.append(s)
            else:
                n = c[k[s]]
                rows[s] = x[pos[s]:pos[s] + n]
                piece = f[pos[s]:pos[s] + n]
                if n or rng.random() < 0.5:                           # a slot that brings no rows may leave its flags out
                    sad[s] = [piece.tolist(), piece, torch.from_numpy(piece.copy())][rng.randrange(3)]
                pos[s] += n
                if k[s] == len(c) - 1 and rng.random() < 0.5:
                    end.append(s)
                    k[s] += 1
            k[s] += 1
        tr.feed(rows, end=end, sad=sad)
        if rng.random() < 0.2:
            for s, segs in tr.poll().items():
                polled[s] += segs
    for s, segs in tr.poll().items():
        polled[s] += segs
    return polled


HOWS = ["one", "seven", "random", "whole", 15, 16, 17, 33]


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_tracker_against_golden_under_any_chunking(hip_lib, dev, case):
    from fs_eend_amd.live_rttm import SegmentTracker
    from fs_eend_amd.postproc import rttm_lines
    _, _, _, lines = golden(case)
    pred, f = R.inputs(case)
    pred = pred.to(dev)
    T, S = pred.shape
    rng = random.Random(case["name"])
    g = torch.Generator().manual_seed(3)
    slots = list(range(len(HOWS) + 2))
    rng.shuffle(slots)
    tr = SegmentTracker(len(slots), S, col0=0, threshold=case["threshold"], median=case["median"], is_prob=True, capacity=4096,
                        device=dev, sad=True)
    streams = {s: (pred, f, chunks(rng, T, h)) for s, h in zip(slots, HOWS)}
    for s in slots[len(HOWS):]:                                       # noise in the slots between them
        n = rng.randrange(0, 200)
        streams[s] = (torch.rand(n, S, generator=g).to(dev), R.run_flags(s, n, longest=5), chunks(rng, n, "random"))
    polled = drive(tr, streams, rng)
    for s, h in zip(slots, HOWS):
        assert flat(tr.rttm(s, "rec0")) == lines, (case["name"], s, h)
        assert flat(rttm_lines("rec0", by_track(polled[s], S))) == lines
    for s in slots[len(HOWS):]:
        x, fl, _ = streams[s]
        want = R.make_rttm("n", x, fl, case["threshold"], case["median"]) if x.shape[0] else {}
        same_rttm(tr.rttm(s, "n"), want)


@pytest.mark.parametrize("ntracks,col0", [(1, 0), (1, 3), (11, 1), (64, 0), (64, 3)])
def test_tracker_lanes_and_untracked_columns(hip_lib, dev, ntracks, col0):
    """median 1, so every raw decision shows in the lines: the recovered track is the largest of the tracked columns only
    (the columns before and behind them hold the row's largest values), on the first lane and on the last."""
    from fs_eend_amd import postproc
    from fs_eend_amd.live_rttm import SegmentTracker
    T, thr = 150, 0.9
    g = torch.Generator().manual_seed(ntracks + col0)
    x = torch.rand(T, ntracks, generator=g) * (1.0 if ntracks < 64 else 0.905)      # 64 tracks: few rows pass 0.9 by themselves
    x[5:25, 0] = 0.8995                                               # recoveries on the first lane ...
    x[5:25, 1:] *= 0.85
    x[40:60, -1] = 0.8995                                             # ... and on the last
    x[40:60, :-1] *= 0.85
    x[70:80] = x[70:71]                                               # repeated rows
    x[80:90, :] = 0.3                                                 # a full tie: track 0
    fl = R.run_flags(9, T, longest=6)
    fl[5:25:2] = fl[40:60:2] = fl[80:90:3] = 1
    fused = R.sad_fuse(x, fl, thr)
    raw = (x > thr).any(dim=1).numpy()
    rec = (fl != 0) & ~raw
    assert rec.sum() >= 20 and ((fl == 0) & raw).sum() >= (5 if ntracks > 1 else 1)
    assert fused[rec][:, 0].sum() >= 5 and fused[rec][:, -1].sum() >= 5              # both edge lanes take recoveries
    wide = torch.full((T, col0 + ntracks + 2), 5.0)
    wide[:, col0:col0 + ntracks] = x
    wide = wide.to(dev)
    want = R.make_rttm("r", x, fl, thr, 1)
    same_rttm(postproc.make_rttm("r", wide[:, col0:col0 + ntracks], threshold=thr, median=1, sad=fl), want)
    rng = random.Random(ntracks)
    tr = SegmentTracker(3, ntracks, col0=col0, threshold=thr, median=1, is_prob=True, capacity=1 << 14, device=dev, sad=True)
    drive(tr, {0: (wide, fl, chunks(rng, T, "random")), 1: (wide, fl, chunks(rng, T, 16)), 2: (wide, fl, [T])}, rng)
    for s in range(3):
        same_rttm(tr.rttm(s, "r"), want)


@pytest.mark.parametrize("is_prob", [True, False])
def test_tracker_nan_and_inf_rows(hip_lib, dev, is_prob):
    from fs_eend_amd.live_rttm import SegmentTracker
    T, S = 200, 6
    g = torch.Generator().manual_seed(11)
    x = torch.rand(T, S, generator=g) if is_prob else torch.randn(T, S, generator=g) * 2 - 2
    x[torch.rand(T, S, generator=g) < 0.25] = NAN                    # NaN is never active and never the largest
    x[20:40] = NAN                                                    # speech rows of NaN only recover nobody
    x[60:70] = -INF                                                   # -inf is an ordinary value: track 0
    x[80:90, 1:] = -INF
    x[80:90, 0] = NAN                                                 # ... and wins over NaN: track 1
    fl = R.run_flags(12, T, longest=5)
    fl[20:40:2] = fl[60:70:2] = fl[80:90:2] = 1
    thr = 0.8
    post = x if is_prob else torch.sigmoid(x)
    fused = R.sad_fuse(post, fl, thr)
    assert fused[20:40].sum() == 0 and fused[60:70, 0].sum() >= 5 and fused[80:90, 1].sum() >= 5 and fused[80:90, 0].sum() == 0
    want = R.make_rttm("r", post, fl, thr, 1)
    want3 = R.make_rttm("r", post, fl, thr, 3)
    rng = random.Random(4)
    xd = x.to(dev)
    for k, w in ((1, want), (3, want3)):
        tr = SegmentTracker(2, S, col0=0, threshold=thr, median=k, is_prob=is_prob, capacity=4096, device=dev, sad=True)
        drive(tr, {0: (xd, fl, chunks(rng, T, "random")), 1: (xd, fl, chunks(rng, T, 17))}, rng)
        same_rttm(tr.rttm(0, "r"), w)
        same_rttm(tr.rttm(1, "r"), w)


def test_tracker_logits_mode(hip_lib, dev):
    """Logits: the decision is sigmoid(x) > threshold and the largest value is taken over the raw logits, which is the
    posterior's wherever the two largest differ -- a condition on the inputs, checked here on the reference alone."""
    from fs_eend_amd.live_rttm import SegmentTracker
    T, C, thr, seed = 300, 8, 0.7, 3
    L = smooth_logits(T, C, seed, "cpu")
    fl = R.run_flags(seed + 500, T)
    post = torch.sigmoid(L[:, 1:])
    gated, recovered = R.counts(post, fl, thr)
    rec = torch.from_numpy((fl != 0) & ~(post > thr).any(dim=1).numpy())
    top = torch.topk(L[:, 1:], 2, dim=1).values[rec]
    ptop = torch.topk(post, 2, dim=1).values[rec]
    assert gated >= 10 and recovered >= 10 and int(rec.sum()) == recovered
    assert float((top[:, 0] - top[:, 1]).min()) > 1e-3 and bool((ptop[:, 0] > ptop[:, 1]).all())
    rng = random.Random(6)
    Ld = L.to(dev)
    for k in (1, 5, 11):
        want = R.make_rttm("r", post, fl, thr, k)
        tr = SegmentTracker(3, C - 1, col0=1, threshold=thr, median=k, capacity=4096, device=dev, sad=True)
        drive(tr, {0: (Ld, fl, chunks(rng, T, "random")), 1: (Ld, fl, [T]), 2: (Ld, fl, chunks(rng, T, 16))}, rng)
        for s in range(3):
            same_rttm(tr.rttm(s, "r"), want)


def test_tracker_refuses_bad_flags_before_launching(hip_lib, dev):
    from fs_eend_amd.live_rttm import SegmentTracker, SlotError
    x = torch.rand(5, 3).to(dev)
    plain = SegmentTracker(2, 3, col0=0, is_prob=True, device=dev)
    with pytest.raises(SlotError):
        plain.feed({0: x}, sad={0: [1] * 5})
    with pytest.raises(SlotError):
        plain.feed_rows(x[:2].contiguous(), torch.ones(2, dtype=torch.int32, device=dev), sad=torch.ones(2, 1, dtype=torch.uint8, device=dev))
    tr = SegmentTracker(2, 3, col0=0, is_prob=True, device=dev, sad=True)
    for sad in (None, {0: [1] * 4}, {0: [1] * 5, 1: [1]}, {1: [1] * 5}):
        with pytest.raises(SlotError):
            tr.feed({0: x}, sad=sad)
    with pytest.raises(SlotError):
        tr.feed_rows(x[:2].contiguous(), torch.ones(2, dtype=torch.int32, device=dev))
    with pytest.raises(SlotError):
        tr.feed_rows(x[:2].contiguous(), torch.ones(2, dtype=torch.int32, device=dev), sad=torch.ones(3, dtype=torch.uint8, device=dev))
    assert plain.poll() == {} and tr.poll() == {}
    assert int(tr.box[:, 0].sum()) == 0 and int(plain.box[:, 0].sum()) == 0          # nothing was launched
    assert "sad" not in plain.export(0)["config"] and "fifo" not in plain.export(0)
    tr.feed({0: x}, sad={0: [1] * 5}, end=[0])
    tr.feed({1: x[:0]}, end=[1])                                      # no rows: no flags wanted
    assert int(tr.box[0, 0]) == 5 and int(tr.box[1, 0]) == 0


# ---------------------------------------------------------------------------------------------- sessions
class Driver:
    """test_live_rttm's scenario (late / paused / empty / short / reopened streams) with a flag per frame.  mode "step": one
    frame per step; "frames": up to 8 per step_frames call; "prefill": a stream's first frames go in by prefill (in two
    pieces), the rest by step.  The schedule depends on `seed` alone, so a bare session driven with the same seed takes the
    same calls."""

    def __init__(self, ses, mode, seed, sad, read=None):
        self.ses, self.mode, self.rng, self.sad = ses, mode, random.Random(seed), sad
        self.read = sad if read is None else read                     # poll and read the lines (a SegmentSession)
        self.out, self.lines, self.polled, self.slot = {}, {}, {}, {}

    def _take(self, y):
        by_slot = {s: n for n, s in self.slot.items()}
        for s, v in y.items():
            if v.shape[1]:
                self.out[by_slot[s]].append(v.reshape(-1, v.shape[-1]))

    def run(self, streams, pauses, flags):
        kw = (lambda f: {"sad": f}) if self.sad else (lambda f: {})
        pos = {n: 0 for n in streams}
        step = 0
        while True:
            for n, (fr, start) in streams.items():
                if start == step:
                    s = self.slot[n] = self.ses.open()
                    self.out[n], self.polled[n] = [], []
                    if self.mode == "prefill" and n in ("x", "late", "re"):
                        for m in (5, 7 + self.rng.randrange(8)):      # the first shorter than the delay, the second emits
                            self._take({s: self.ses.prefill(s, fr[pos[n]:pos[n] + m], **kw(flags[n][pos[n]:pos[n] + m]))})
                            pos[n] += m
            push, flush, sad = {}, [], {}
            for n, s in self.slot.items():
                fr = streams[n][0]
                if self.ses.state(s) != "open" or step in pauses.get(n, ()):
                    continue
                if self.mode == "frames":
                    m = min(self.rng.choice([0, 1, 2, 5, 8]), len(fr) - pos[n])
                    push[s] = fr[pos[n]:pos[n] + m] if m else torch.zeros(0, streams["x"][0].shape[1], device=streams["x"][0].device)
                    sad[s] = flags[n][pos[n]:pos[n] + m]
                    pos[n] += m
                    if pos[n] == len(fr):
                        flush.append(s)
                elif pos[n] < len(fr):
                    push[s] = fr[pos[n]]
                    sad[s] = int(flags[n][pos[n]])
                    pos[n] += 1
                else:
                    flush.append(s)
            fn = self.ses.step_frames if self.mode == "frames" else self.ses.step
            self._take(fn(push=push, flush=flush, **kw(sad)))
            if self.read and step % 7 == 3:
                self.poll()
            for n, s in list(self.slot.items()):
                if self.ses.state(s) == "done":
                    if self.read:
                        self.poll()
                        self.lines[n] = self.ses.rttm(s, "rec")
                    self.ses.close(s)
                    del self.slot[n]
            step += 1
            if not self.slot and all(start < step for _, start in streams.values()):
                return {n: torch.cat(v) if v else None for n, v in self.out.items()}

    def poll(self):
        by_slot = {s: n for n, s in self.slot.items()}
        for s, segs in self.ses.poll().items():
            self.polled[by_slot[s]] += segs


@pytest.mark.parametrize("mode", ["step", "frames", "prefill"])
@pytest.mark.parametrize("kind", ["fs", "ls"])
def test_sessions_exact(hip_lib, dev, kind, mode):
    from fs_eend_amd import postproc
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    from fs_eend_amd.live_rttm import SegmentSession
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    from fs_eend_amd.postproc import rttm_lines
    nmax = 1 if mode == "step" else 8
    if kind == "fs":
        sm, C, src = _fs(dev)
        mk = lambda g: FsMultiStreamSession(sm, 6, C, cap=16, use_graph=g, max_frames=nmax)
    else:
        sm, C, src = _ls(dev)
        src = src[:70].contiguous()
        mk = lambda g: LsMultiStreamSession(sm, 6, C, use_graph=g, max_frames=nmax)
    streams, pauses = _scenario(src, src.shape[1], dev, seed=7)
    flags = {n: R.run_flags(100 + i, len(fr), longest=6) for i, (n, (fr, _)) in enumerate(streams.items())}
    flags["re"] = flags["x"]                                          # the same stream and mask again, later
    bare = Driver(mk(True), mode, 5, sad=False).run(streams, pauses, flags)
    allp = torch.sigmoid(torch.cat([v for v in bare.values() if v is not None])[:, 1:])
    thr = float(torch.quantile(allp.max(dim=1).values.nan_to_num(0.0), 0.6))        # four rows in ten have nobody above it
    gated = recovered = 0
    for n, v in bare.items():                                         # both effects occur, by the bare logits alone
        if v is not None:
            assert v.shape[0] == len(flags[n])                        # output row u belongs to input frame u
            a, b = R.counts(torch.sigmoid(v[:, 1:]).cpu(), flags[n], thr)
            gated, recovered = gated + a, recovered + b
    assert gated >= 10 and recovered >= 10, (gated, recovered)
    results = []
    for graph in (True, False):
        d = Driver(SegmentSession(mk(graph), sad=True, threshold=thr, median=5), mode, 5, sad=True)
        got = d.run(streams, pauses, flags)
        for n, v in bare.items():
            assert (v is None and got[n] is None) or same_bits(got[n], v), (n, graph)
        for n, v in got.items():
            want = postproc.make_rttm("rec", torch.sigmoid(v[:, 1:]), threshold=thr, median=5, sad=flags[n]) if v is not None else {}
            same_rttm(d.lines[n], want)
            same_rttm(rttm_lines("rec", by_track(d.polled[n], C - 1)), want)
            if v is not None:
                same_rttm(want, R.make_rttm("rec", torch.sigmoid(v[:, 1:]).cpu(), flags[n], thr, 5))
        results.append({n: flat(l) for n, l in d.lines.items()})
        assert all(q == [] for q in d.ses.tracker.fifo.q)
    assert results[0] == results[1]
    assert results[0]["x"] == results[0]["re"]                      # the same stream later, in a slot another stream left
    assert sum(len(v) for v in results[0].values()) > 10
    plain = Driver(SegmentSession(mk(True), threshold=thr, median=5), mode, 5, sad=False, read=True)
    plain.run(streams, pauses, flags)
    assert {n: flat(l) for n, l in plain.lines.items()} != results[0]                # the mask does change the lines


@pytest.mark.parametrize("kind", ["fs", "ls"])
def test_snapshot_with_flags_waiting(hip_lib, dev, kind):
    """Suspended while flags wait for their rows, through the host, into a session of another slot count and max_frames: the
    lines and the concatenated polls are the uninterrupted stream's.  A plain tracker's snapshot and a masked one's do not mix."""
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    from fs_eend_amd.live_rttm import SegmentSession, SlotError
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    if kind == "fs":
        sm, C, src = _fs(dev)
        base = lambda slots, **kw: FsMultiStreamSession(sm, slots, C, cap=64, **kw)
    else:
        sm, C, src = _ls(dev)
        src = src[:60].contiguous()
        base = lambda slots, **kw: LsMultiStreamSession(sm, slots, C, **kw)
    T = src.shape[0]
    fl = R.run_flags(31, T, longest=6).tolist()
    bare = base(1)
    s = bare.open()
    ref = [bare.step({s: src[i]}) for i in range(T)]
    ref = torch.cat([y[s].reshape(1, -1) for y in ref if s in y])
    thr = float(torch.quantile(torch.sigmoid(ref[:, 1:]).max(dim=1).values, 0.6))
    mk = lambda slots, **kw: SegmentSession(base(slots, **kw), sad=True, threshold=thr, median=5)

    def run(cut):
        A = mk(3)
        s, polled, snap = A.open(), [], None
        for i in range(T):
            A.step({s: src[i]}, sad={s: fl[i]})
            if i in (15, 33, 44):
                polled += A.poll().get(s, [])
            if i == cut:
                snap = A.suspend(s)
                waiting = snap.parts["tracker"]["fifo"]
                assert len(waiting) == A.ses.center > 0 and waiting == fl[i + 1 - len(waiting):i + 1]
                assert snap.parts["tracker"]["config"]["sad"] is True
                A = mk(4, use_graph=False, max_frames=4)
                A.open()
                s = A.resume(snap.to("cpu"))
                assert s == 1 and A.tracker.fifo.q[s] == waiting
        A.step(flush=[s])
        while A.state(s) != "done":
            A.step()
        polled += A.poll().get(s, [])
        return A.rttm(s, "rec"), polled, snap

    whole = run(None)
    assert sum(len(v) for v in whole[0].values()) > 2
    got = run(29)
    assert got[0] == whole[0] and got[1] == whole[1]
    snap = got[2]
    plain = SegmentSession(base(1), threshold=thr, median=5)
    with pytest.raises(SlotError, match="tracker"):
        plain.resume(snap)                                            # a masked stream does not go on without its mask
    assert plain.state(0) == "free"
    a = plain.open()
    plain.step({a: src[0]})
    masked = mk(1)
    with pytest.raises(SlotError, match="tracker"):
        masked.resume(plain.snapshot(a))                              # ... nor a plain one with one
    assert masked.state(0) == "free" and masked.tracker.fifo.q == [[]]
    with pytest.raises(SlotError):
        masked.seek(0, 3)


def test_audio_session_refuses_a_masked_session(hip_lib, dev):
    from fs_eend_amd.audio_stream import AudioStreamSession
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    from fs_eend_amd.live_rttm import SegmentSession
    sm, C, _ = _fs(dev)
    with pytest.raises(ValueError, match="speech-activity"):
        AudioStreamSession(SegmentSession(FsMultiStreamSession(sm, 2, C, cap=16), sad=True))
