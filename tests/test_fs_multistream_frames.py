"""GPU: many frames per slot in one FS-EEND multi-stream step (FsMultiStreamSession.step_frames) -- the chunk attention and the
chunk window kernels against exact references, the session against the reference's own streaming logits and against the
per-frame session, and the slot invariance of the multi-frame step: a stream's logits, for one chunk schedule, do not depend
on its slot, its neighbours, what the slot held before, the cache capacity or the graph."""
import pytest
import torch

from tests.helpers import max_abs
from tests.test_fs_multistream import _models

pytestmark = pytest.mark.gpu
F16, F32, I32 = torch.float16, torch.float32, torch.int32
H, D = 4, 256


def _chunk_ref(qkv, kc, vc, q, nmax, t, c):
    """fp32 attention of the c chunk rows of sequence q over its t cached keys and the chunk's keys 0..j, (c, D)"""
    x = qkv[q * nmax:q * nmax + c].float()
    Q = x[:, :D].view(c, H, 64).transpose(0, 1)
    K = torch.cat([kc[q, :, :t].float(), x[:, D:2 * D].view(c, H, 64).transpose(0, 1)], dim=1)
    V = torch.cat([vc[q, :, :t].float(), x[:, 2 * D:].view(c, H, 64).transpose(0, 1)], dim=1)
    s = Q @ K.transpose(-1, -2) / 8.0
    mask = torch.ones(c, t + c, dtype=torch.bool, device=qkv.device).triu(t + 1)
    s = s.masked_fill(mask, float("-inf"))
    return (torch.softmax(s, -1) @ V).transpose(0, 1).reshape(c, D)


def _chunk(rps, cap, nmax, lens, cnts, seed, kc=None, vc=None, qkv=None):
    from fs_eend_amd import ops
    dev = torch.device("cuda:0")
    S = len(lens)
    N = S * rps
    g = torch.Generator().manual_seed(seed)
    if kc is None:
        kc = (torch.randn(N, H, cap, 64, generator=g) * 0.7).to(F16).to(dev)
        vc = torch.randn(N, H, cap, 64, generator=g).to(F16).to(dev)
        qkv = torch.randn(N * nmax, 3 * D, generator=g).to(F16).to(dev)
    ln = torch.tensor(lens, dtype=I32, device=dev)
    ct = torch.tensor(cnts, dtype=I32, device=dev)
    k2, v2 = kc.clone(), vc.clone()
    out = torch.full((N * nmax, D), float("nan"), dtype=F16, device=dev)
    ws = torch.full((ops.attn_chunk_ragged_ws(N, H, cap, nmax),), float("nan"), dtype=F32, device=dev)
    ops.attn_chunk_ragged(qkv, k2, v2, out, ws, N, H, cap, nmax, rps, ln, ct)
    torch.cuda.synchronize()
    assert torch.equal(ln.cpu(), torch.tensor(lens, dtype=I32))          # lengths are not advanced here
    return kc, vc, qkv, k2, v2, out


LENS = [0, 1, 63, 64, 65, 511, 512, 513, 1500]
CNTS = [0, 1, 2, 7, 16, 33, 64]


@pytest.mark.parametrize("rps", [1, 6])
def test_chunk_attention_matches_reference(hip_lib, dev, rps):
    cap, nmax = 2048, 64
    lens, cnts = [], []
    for c in CNTS:
        for t in LENS + [cap - c]:
            lens.append(t)
            cnts.append(c)
    lens += [cap - 3, cap, cap + 5, 1000]                                 # past the capacity (no-ops), and a negative-free extra
    cnts += [4, 1, 2, 0]
    kc, vc, qkv, k2, v2, out = _chunk(rps, cap, nmax, lens, cnts, seed=rps)
    want_k, want_v = kc.clone(), vc.clone()
    worst = 0.0
    zero = torch.zeros(D, dtype=F16, device=dev)
    for s, (t, c) in enumerate(zip(lens, cnts)):
        live = c > 0 and t + c <= cap
        for q in range(s * rps, (s + 1) * rps):
            if live:
                x = qkv[q * nmax:q * nmax + c]
                want_k[q, :, t:t + c] = x[:, D:2 * D].view(c, H, 64).transpose(0, 1)
                want_v[q, :, t:t + c] = x[:, 2 * D:].view(c, H, 64).transpose(0, 1)
                ref = _chunk_ref(qkv, kc, vc, q, nmax, t, c)
                err = float((out[q * nmax:q * nmax + c].float() - ref).abs().max())
                worst = max(worst, err)
                assert err < 2e-3, (s, t, c, err)
            for j in range(c if live else 0, nmax):
                assert torch.equal(out[q * nmax + j], zero), (s, t, c, j)
    print(f"chunk attention rps={rps}: max |err| {worst:.2e}")
    assert torch.equal(k2, want_k) and torch.equal(v2, want_v)           # appends bit-equal to qkv, nothing else touched


@pytest.mark.parametrize("rps", [1, 6])
def test_chunk_attention_independent_of_capacity_and_stale_rows(hip_lib, dev, rps):
    """The same histories in cap = 2048 and cap = 4096 buffers give bit-identical outputs and appends; NaN in every cache row at
    or beyond the length is never read."""
    nmax = 16
    lens = [0, 1, 63, 64, 65, 511, 512, 513, 1500, 2032]
    cnts = [16, 1, 7, 16, 2, 9, 16, 3, 16, 16]
    kc, vc, qkv, k_small, v_small, o_small = _chunk(rps, 2048, nmax, lens, cnts, seed=10 + rps)
    N = kc.shape[0]
    kb = torch.full((N, H, 4096, 64), float("nan"), dtype=F16, device=dev)
    vb = torch.full((N, H, 4096, 64), float("nan"), dtype=F16, device=dev)
    for i, t in enumerate(lens):
        for q in range(i * rps, (i + 1) * rps):
            kb[q, :, :t], vb[q, :, :t] = kc[q, :, :t], vc[q, :, :t]
    _, _, _, k_big, v_big, o_big = _chunk(rps, 4096, nmax, lens, cnts, 0, kb, vb, qkv)
    assert torch.isfinite(o_big).all()
    assert torch.equal(o_small, o_big)
    for i, (t, c) in enumerate(zip(lens, cnts)):
        for q in range(i * rps, (i + 1) * rps):
            assert torch.equal(k_big[q, :, :t + c], k_small[q, :, :t + c]) and torch.equal(v_big[q, :, :t + c], v_small[q, :, :t + c])


def test_counter_add_count_and_window_chunk_exact(hip_lib, dev):
    from fs_eend_amd import ops
    S, k, nmax = 23, 19, 8
    g = torch.Generator().manual_seed(4)
    ln = torch.randint(0, 5000, (S,), generator=g, dtype=I32)
    ct = torch.randint(0, nmax + 1, (S,), generator=g, dtype=I32)
    ld = ln.to(dev)
    ops.counter_add_count(ld, ct.to(dev))
    assert torch.equal(ld.cpu(), ln + ct)

    win = torch.randn(S, k * D, generator=g).to(F16)
    x = torch.randn(S * nmax, D, generator=g) * 3
    npush, ndummy, ndec = [], [], []
    for s in range(S):
        p = int(torch.randint(0, nmax + 1, (1,), generator=g))
        d = int(torch.randint(0, nmax - p + 1, (1,), generator=g))
        e = int(torch.randint(0, p + d + 1, (1,), generator=g))
        npush.append(p), ndummy.append(d), ndec.append(e)
    npush[0], ndummy[0], ndec[0] = nmax, 0, nmax                           # a full chunk that emits every window
    npush[1], ndummy[1], ndec[1] = 0, 0, 0                                 # an idle slot
    npush[2], ndummy[2], ndec[2] = 0, nmax, 3                              # flushing only
    wd = win.to(dev)
    cols = torch.full((S * nmax, k * D), float("nan"), dtype=F16, device=dev)
    t = lambda v: torch.tensor(v, dtype=I32, device=dev)
    ops.window_chunk(wd, x.to(dev), cols, t(npush), t(ndummy), t(ndec), nmax)
    # reference: npush + ndummy calls of ops.window_push, im2col of the windows after each push
    ref_win = win.to(dev)
    hist = [[] for _ in range(S)]
    for f in range(nmax):
        mode = [1 if f < npush[s] else 2 if f < npush[s] + ndummy[s] else 0 for s in range(S)]
        xf = torch.stack([x[s * nmax + f] if f < npush[s] else torch.zeros(D) for s in range(S)]).to(dev)
        ops.window_push(ref_win, xf, t(mode))
        for s in range(S):
            if mode[s]:
                hist[s].append(ref_win[s].clone())
    want = torch.zeros(S * nmax, k * D, dtype=F16, device=dev)
    for s in range(S):
        P = npush[s] + ndummy[s]
        for i in range(ndec[s]):
            want[s * nmax + i] = hist[s][P - ndec[s] + i]
    torch.cuda.synchronize()
    assert torch.equal(wd, ref_win)
    assert torch.equal(cols, want)


# ---------------------------------------------------------------------------------------------- the session
class _ChunkDriver:
    """Feeds scripted streams through a session with step_frames: streams[name] = (frames, start step, chunk sizes); a stream
    takes a slot at its start step and pushes its frames in the given chunk sizes (0 = a pause), cycling; its last chunk goes
    with the flush.  closes[name] = step at which the stream's slot is closed early."""

    def __init__(self, ses):
        self.ses, self.out, self.slot = ses, {}, {}

    def run(self, streams, closes=None, want_slot=None, per_frame=()):
        closes, want_slot = closes or {}, want_slot or {}
        pos = {n: 0 for n in streams}
        k = {n: 0 for n in streams}
        step = 0
        while True:
            for n, (_, start, _) in streams.items():
                if start == step:
                    self.slot[n] = self.ses.open()
                    self.out[n] = []
                    if n in want_slot:
                        assert self.slot[n] == want_slot[n], (n, self.slot[n])
            for n, at in closes.items():
                if at == step and n in self.slot:
                    self.ses.close(self.slot.pop(n))
            push, flush, single = {}, [], {}
            for n, s in self.slot.items():
                fr, _, sizes = streams[n]
                if self.ses.state(s) != "open":
                    continue
                m = sizes[k[n] % len(sizes)]
                k[n] += 1
                if n in per_frame and step % 3 == 1 and pos[n] < len(fr):       # mix in a one-frame step
                    single[s] = fr[pos[n]]
                    pos[n] += 1
                    continue
                m = min(m, len(fr) - pos[n])
                if m:
                    push[s] = fr[pos[n]:pos[n] + m]
                    pos[n] += m
                if pos[n] >= len(fr):
                    flush.append(s)
            if single:
                y = self.ses.step(push=single)
                by_slot = {s: n for n, s in self.slot.items()}
                for s, v in y.items():
                    self.out[by_slot[s]].append(v)
            y = self.ses.step_frames(push=push, flush=flush)
            by_slot = {s: n for n, s in self.slot.items()}
            for s, v in y.items():
                self.out[by_slot[s]].append(v)
            for n, s in list(self.slot.items()):
                if self.ses.state(s) == "done":
                    self.ses.close(s)
                    del self.slot[n]
            step += 1
            if not self.slot and all(start < step for _, start, _ in streams.values()):
                return {n: torch.cat(v, dim=1) for n, v in self.out.items() if v}


def _sizes(seed, nmax, n=23):
    g = torch.Generator().manual_seed(seed)
    return [int(v) for v in torch.randint(0, nmax + 1, (n,), generator=g)]


@pytest.mark.parametrize("nmax", [4, 16])
def test_session_frames_vs_reference_and_per_frame(hip_lib, dev, nmax):
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    from tests.test_fs_multistream import _Driver
    meta, arr, sm, src = _models("fs_stream_T60", dev)
    T, C = meta["T"], meta["C"]
    g = torch.Generator().manual_seed(22)
    pert = lambda n: (src[:n] + 0.3 * torch.randn(n, src.shape[1], generator=g).to(dev)).contiguous()
    ses = FsMultiStreamSession(sm, 4, C, cap=16, max_frames=nmax)
    sz = _sizes(nmax, nmax)
    streams = {"gold0": (src, 0, sz), "p1": (pert(T), 0, _sizes(1, nmax)), "hold2": ([], 0, [1]), "p3": (pert(45), 0, _sizes(3, nmax)),
               "gold2": (src, 5, sz)}
    out = _ChunkDriver(ses).run(streams, closes={"hold2": 1, "p1": 4}, want_slot={"gold0": 0, "p1": 1, "hold2": 2, "p3": 3, "gold2": 1})
    a, b = out["gold0"], out["gold2"]
    assert a.shape == (1, T, C) and b.shape == (1, T, C)
    assert torch.equal(a, b), f"slot 0 vs slot 1: {float((a - b).abs().max()):.3e}"
    err = max_abs(a[0], arr["stream_logits"])
    ref = _Driver(FsMultiStreamSession(sm, 4, C, cap=16)).run({"x": (src, 0)})["x"]
    gap = float((a - ref).abs().max())
    print(f"multi-frame session nmax={nmax}: vs reference streaming {err:.2e}, vs per-frame session {gap:.2e}")
    assert err < 1e-3 and gap < 1e-3


@pytest.mark.parametrize("use_graph", [True, False])
def test_session_frames_slot_invariance_bit_exact(hip_lib, dev, use_graph):
    """One chunk schedule, bit for bit: alone in slot 0; in slot 5 amid other streams that join and leave; in a slot whose
    previous stream left NaN behind -- caches starting at 16 rows and growing on the way; and graph on vs off."""
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    meta, arr, sm, src = _models("fs_stream_T60", dev)
    C, nmax = meta["C"], 8
    g = torch.Generator().manual_seed(6)
    other = lambda n: (torch.randn(n, src.shape[1], generator=g) * 2 - 3).to(dev)
    mk = lambda: FsMultiStreamSession(sm, 6, C, cap=16, use_graph=use_graph, max_frames=nmax)
    sz = _sizes(40, nmax)

    alone = _ChunkDriver(mk()).run({"x": (src, 0, sz)})["x"]
    crowd = {f"o{i}": (other(20 + 9 * i), 0, _sizes(50 + i, nmax)) for i in range(5)}
    crowd.update({"x": (src, 1, sz), "o5": (other(30), 6, [nmax])})
    amid = _ChunkDriver(mk()).run(crowd, closes={"o3": 5}, want_slot={"x": 5})["x"]
    ses = mk()
    dr = _ChunkDriver(ses)
    nan = torch.full((90, src.shape[1]), float("nan"), device=dev)
    dr.run({"long": (nan, 0, [nmax, 3, 7])})
    assert ses.cap == 128
    reopened = dr.run({"x": (src, 0, sz)}, want_slot={"x": 0})["x"]
    for name, got in (("amid traffic in slot 5", amid), ("after a NaN stream", reopened)):
        assert got.shape == alone.shape, name
        assert torch.equal(got, alone), f"{name}: max diff {float((got - alone).abs().max()):.3e}"
    assert max_abs(alone[0], arr["stream_logits"]) < 1e-3
    if use_graph:
        eager = _ChunkDriver(FsMultiStreamSession(sm, 6, C, cap=16, use_graph=False, max_frames=nmax)).run({"x": (src, 0, sz)})["x"]
        assert torch.equal(eager, alone)


def test_session_mixes_step_and_step_frames(hip_lib, dev):
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    meta, arr, sm, src = _models("fs_stream_T60", dev)
    T, C = meta["T"], meta["C"]
    ses = FsMultiStreamSession(sm, 3, C, cap=16, max_frames=8)
    out = _ChunkDriver(ses).run({"x": (src, 0, _sizes(7, 8)), "o": (src.flip(0).contiguous(), 0, [5])}, per_frame=("x",))["x"]
    assert out.shape == (1, T, C)
    err = max_abs(out[0], arr["stream_logits"])
    print(f"step / step_frames mixed: vs reference streaming {err:.2e}")
    assert err < 1e-3


def test_long_stream_frames_among_other_streams(hip_lib, dev):
    """fs_stream_T5000 in chunks of 16 in slot 0 of an 8-slot session while the other slots open and close; the caches grow
    from 1024 past 4096."""
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    meta, arr, sm, src = _models("fs_stream_T5000", dev)
    T, C, n = meta["T"], meta["C"], 16
    ses = FsMultiStreamSession(sm, 8, C, cap=1024, max_frames=n)
    s0 = ses.open()
    keep = {int(r): i for i, r in enumerate(arr["rows"])}
    got = torch.zeros(len(keep), C, device=dev)
    done = 0
    life = {}
    step = 0
    pos = 0
    while ses.state(s0) != "done":
        if step % 13 == 0 and len(life) < 7:
            s = ses.open()
            life[s] = [(step * 31) % (T - 800), 40 + (step * 13) % 300]
        push, flush = {}, []
        if pos < T:
            push[s0] = src[pos:pos + n]
            pos += n
            if pos >= T:
                flush.append(s0)
        for s, (i0, left) in life.items():
            if ses.state(s) != "open" or (step + s) % 11 == 0:
                continue
            m = min(left, 1 + (step + s) % n)
            if m:
                push[s] = src[i0:i0 + m]
                life[s] = [i0 + m, left - m]
            if left - m <= 0:
                flush.append(s)
        y = ses.step_frames(push=push, flush=flush)
        if s0 in y:
            for r in range(y[s0].shape[1]):
                if done in keep:
                    got[keep[done]] = y[s0][0, r]
                done += 1
        for s in [s for s in life if ses.state(s) == "done"]:
            ses.close(s)
            del life[s]
        step += 1
    torch.cuda.synchronize()
    assert done == T and ses.cap == 8192
    d = (got - torch.as_tensor(arr["stream_logits"], device=dev)).abs()
    print(f"multi-frame session to t={T}: vs reference streaming max |d logit| {float(d.max()):.2e}")
    assert float(d.max()) < 1e-3


# ---------------------------------------------------------------------------------------------- the layers above
@pytest.mark.parametrize("max_chunk", [6000, 20000])
def test_audio_session_over_frames_session(hip_lib, dev, max_chunk):
    """AudioStreamSession over a max_frames = 8 session against the per-frame session, for two chunkings of the audio."""
    from fs_eend_amd.audio_stream import AudioStreamSession
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    from tests.test_audio_stream import _fs_model, audio_path, wave
    sm, C = _fs_model(dev)
    waves = [wave(8000 * 3 + 4321, 1), wave(8000 * 8, 2), wave(8000 * 5 + 79, 3)]
    want = audio_path(AudioStreamSession(FsMultiStreamSession(sm, 3, C, cap=256)), waves, seed=7, max_chunk=max_chunk)
    ases = AudioStreamSession(FsMultiStreamSession(sm, 3, C, cap=256, max_frames=8))
    got = audio_path(ases, waves, seed=7, max_chunk=max_chunk)
    worst = 0.0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (i, g.shape, w.shape)
        worst = max(worst, float((g - w).abs().max()))
    print(f"audio session, max_frames 8 vs per frame (chunks < {max_chunk}): {worst:.2e}")
    assert worst < 1e-3


def test_segment_session_over_frames_session(hip_lib, dev):
    """SegmentSession over a max_frames session: each slot's rttm lines are make_rttm of its own returned logits, and the
    polled segments add up to those lines."""
    import random

    from fs_eend_amd import postproc
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    from fs_eend_amd.live_rttm import SegmentSession
    meta, arr, sm, src = _models("fs_stream_T60", dev)
    C, nmax = meta["C"], 8
    g = torch.Generator().manual_seed(9)
    streams = [torch.cat([src, src.flip(0), src * 1.1]).contiguous(), (src + 0.5 * torch.randn(src.shape, generator=g).to(dev)),
               torch.cat([src.flip(0), src]).contiguous()]
    ses = SegmentSession(FsMultiStreamSession(sm, 4, C, cap=32, max_frames=nmax), threshold=0.5, median=5)
    assert ses.max_frames == nmax
    slots = [ses.open() for _ in streams]
    pos, logits = [0] * len(streams), [[] for _ in streams]
    polled = {s: [] for s in slots}
    rng = random.Random(3)
    while any(ses.state(s) != "done" for s in slots):
        push, flush = {}, []
        for i, s in enumerate(slots):
            if ses.state(s) != "open" or rng.random() < 0.2:
                continue
            m = min(rng.randrange(0, nmax + 1), streams[i].shape[0] - pos[i])
            if m:
                push[s] = streams[i][pos[i]:pos[i] + m]
                pos[i] += m
            if pos[i] >= streams[i].shape[0]:
                flush.append(s)
        for s, v in ses.step_frames(push=push, flush=flush).items():
            logits[slots.index(s)].append(v[0])
        if rng.random() < 0.3:
            for s, segs in ses.poll().items():
                polled[s] += segs
    for s, segs in ses.poll().items():
        polled[s] += segs
    for i, s in enumerate(slots):
        L = torch.cat(logits[i])
        assert L.shape == (streams[i].shape[0], C)
        want = postproc.make_rttm("rec", torch.sigmoid(L[:, 1:]), threshold=0.5, median=5)
        assert ses.rttm(s, "rec") == want, i
        per = [[] for _ in range(C - 1)]
        for spk, a, b in polled[s]:
            per[spk].append((a, b))
        assert postproc.rttm_lines("rec", per) == want, i
