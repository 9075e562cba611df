"""GPU: the audio ingest (csrc/resample.hip behind eend_audio_ingest, audio_ingest.AudioIngest) against the float64 restatement
(tests/resample_ref.py) within the worst-case bound of an f32 accumulation, bit for bit against itself across cuttings, slots
and neighbours, and through every layer above it: AudioFrontEnd, extract_fbank_wave, snapshots and AudioStreamSession.

Shapes: at most three tiles of output (775 samples at 8 kHz, under 5000 input samples at 48 kHz)."""
import random

import numpy as np
import pytest
import torch

from tests import resample_ref as R

pytestmark = pytest.mark.gpu
OUTS = [255, 256, 257, 3 * 256 + 7]                     # output counts whose smallest input length is a test length
TODAY_KEYS = {"config", "tail", "ring", "sums", "state", "recv", "frames", "mframes"}


def lengths(rate):
    L, M, _, _ = R.params(rate)
    return [0, 1, M - 1, M] + [R.smallest_input(n, rate) for n in OUTS]


def raw(n, encoding, seed):
    return torch.from_numpy(R.raw_stream(n, encoding, seed))


def one_shot(ing, streams):
    """streams: [raw CPU tensor], one per slot, fed whole with their end in one call -> [f32 8 kHz samples]."""
    for s in range(len(streams)):
        ing.reset(s)
    got = ing.feed(dict(enumerate(streams)), end=list(range(len(streams))))
    return [got[s] for s in range(len(streams))]


def run_cut(ing, s, x, bounds):
    """Stream x through slot s cut at `bounds` (a non-decreasing list from 0 to len(x)), then its end alone."""
    ing.reset(s)
    out = [ing.feed({s: x[a:b]})[s] for a, b in zip(bounds, bounds[1:])]
    out.append(ing.feed({}, end=[s])[s])
    return torch.cat(out)


def cuttings(n_in, rate, rng):
    """Cut points of a stream of 3 tiles + 7 outputs: an empty chunk, one-sample chunks, a chunk that completes no output, a cut on
    each side of the sample that makes output 256 ready, a chunk longer than the history row plus a tile's span, and seeded
    random cuts in the rest."""
    L, M, H, P = R.params(rate)
    r = next(v for v in range(n_in + 1) if R.n_ready(v, rate) >= 257)            # with r samples output 256 is ready, with r - 1 not
    big = 256 + (256 * M + L - 1) // L + 1
    assert r + big <= n_in and (H == 0 or R.n_ready(2, rate) == 0)               # (at 8000 Hz only the empty chunk completes nothing)
    fixed = [0, 0, 1, 2, r - 1, r, r + big, n_in]
    free = [v for v in range(3, n_in) if not r - 1 <= v <= r + big]
    return sorted(fixed + rng.sample(free, 6))


# ------------------------------------------------------------------------------------------------ the kernel against float64
@pytest.fixture(scope="module")
def worst():
    """{(rate, encoding): worst observed error as a fraction of the bound}, printed at the end of the module."""
    seen = {}
    yield seen
    if seen:
        k = max(seen, key=seen.get)
        print(f"\n[audio ingest] worst |error| / bound over {len(seen)} rate x encoding cases: {seen[k]:.4f} at {k}")


@pytest.mark.parametrize("encoding", R.ENCODINGS)
@pytest.mark.parametrize("rate", R.RATES)
def test_accuracy_and_cut_independence(hip_lib, dev, worst, rate, encoding):
    """One feed with end, eight lengths in eight slots: every sample within P 2^-24 sum |h32[.] x[k]| of the float64 sum over
    the same f32 table and decoded samples (the worst case of an f32 fma chain of P terms; derived, not measured).  Then the
    longest stream cut at the edges and at random: the same bits."""
    from fs_eend_amd import audio_ingest as I
    L, M, H, P = R.params(rate)
    h32 = R.prototype(rate).astype(np.float32)
    ns = lengths(rate)
    streams = [raw(n, encoding, 1000 * rate + n) for n in ns]
    ing = I.AudioIngest(len(ns), rate, encoding, device=dev)
    got = one_shot(ing, streams)
    frac = 0.0
    for n_in, x, g in zip(ns, streams, got):
        xd = R.decode(x.numpy(), encoding)
        want = R.resample(xd, h32, rate)
        bound = P * 2.0 ** -24 * R.resample(xd, h32, rate, absolute=True)
        g = g.cpu().numpy().astype(np.float64)
        assert g.shape == want.shape == (R.n_total(n_in, rate),), (n_in, g.shape, want.shape)
        err = np.abs(g - want)
        assert np.all(err <= bound), (n_in, float(err.max()), float(bound[err.argmax()]))
        if n_in:
            frac = max(frac, float((err / np.maximum(bound, 1e-300)).max()))
    worst[(rate, encoding)] = frac
    assert all(ing.state(s) == "ended" for s in range(len(ns)))
    rng = random.Random(rate + len(encoding))
    x, whole = streams[-1], got[-1]
    for slot in (0, 5):
        cut = run_cut(ing, slot, x, cuttings(ns[-1], rate, rng))
        assert torch.equal(cut, whole), (slot, float((cut - whole).abs().max()))


def test_eight_slots_at_their_own_pace(hip_lib, dev):
    """Eight streams of different lengths and chunk sizes in one ingest, each pausing at random: each equals its solo run."""
    from fs_eend_amd import audio_ingest as I
    rate, encoding = 44100, "s16"
    rng = random.Random(8)
    ns = [4270, 0, 1, 441, 1411, 3000, 2999, 777]
    streams = [raw(n, encoding, 80 + s) for s, n in enumerate(ns)]
    solo = I.AudioIngest(1, rate, encoding, device=dev)
    want = [one_shot(solo, [x])[0] for x in streams]
    ing = I.AudioIngest(8, rate, encoding, device=dev)
    for s in range(8):
        ing.reset(s)
    pos, out, live = [0] * 8, [[] for _ in range(8)], set(range(8))
    calls = 0
    while live:
        waves, end = {}, []
        for s in sorted(live):
            if rng.random() < 0.35:
                continue                                              # not named: the slot pauses
            if pos[s] < ns[s]:
                m = rng.choice([1, 7, 100 * (s + 1), 1500])
                w = streams[s][pos[s]:pos[s] + m]
                waves[s] = w.to(dev) if (calls + s) % 2 else w
                pos[s] += m
            else:
                end.append(s)
        for s, v in ing.feed(waves, end=end).items():
            out[s].append(v)
        live -= set(end)
        calls += 1
    for s in range(8):
        g = torch.cat(out[s])
        assert g.shape == want[s].shape and torch.equal(g, want[s]), (s, g.shape, want[s].shape)


# ------------------------------------------------------------------------------------------------ the front-end on top
def fe_run(fe, s, x, sizes):
    """Stream x through slot s of front-end fe in chunks of `sizes`, ended with the last chunk -> its model frames."""
    fe.reset(s)
    out, a = [], 0
    for i, m in enumerate(sizes):
        out.append(fe.feed({s: x[a:a + m]}, end=[s] if i == len(sizes) - 1 else [])[s])
        a += m
    assert a == x.numel()
    return torch.cat(out)


def uneven(n, rng, k=7):
    cuts = sorted(rng.randrange(n + 1) for _ in range(k))
    return [b - a for a, b in zip([0] + cuts, cuts + [n])]


@pytest.mark.parametrize("tr", ["logmel23", "logmel23_cummn"])
def test_pass_through_at_8000(hip_lib, dev, tr):
    from fs_eend_amd import audio_ingest as I
    from fs_eend_amd.audio_stream import AudioFrontEnd
    x = raw(2345, "s16", 5)
    y = one_shot(I.AudioIngest(1, 8000, "s16", device=dev), [x])[0]
    assert torch.equal(y.cpu(), x.to(torch.float32) / 32768)
    sizes = uneven(x.numel(), random.Random(1))
    a = AudioFrontEnd(2, tr, device=dev, sample_rate=8000, encoding="s16")
    b = AudioFrontEnd(2, tr, device=dev)
    assert a.ingest is not None and b.ingest is None
    got, want = fe_run(a, 1, x, sizes), fe_run(b, 1, x.to(torch.float32) / 32768, sizes)
    assert got.shape == want.shape == (3, 345) and torch.equal(got, want)
    assert a.table.frames == b.table.frames and a.table.mframes == b.table.mframes


@pytest.mark.parametrize("tr", ["logmel23", "logmel23_cummn"])
@pytest.mark.parametrize("rate,encoding", [(16000, "s16"), (44100, "f32")])
def test_front_end_plumbing(hip_lib, dev, rate, encoding, tr):
    """The front-end with an ingest, fed uneven chunks and ended, against a default front-end fed the ingest's own 8 kHz output:
    the same frames, the zero-padded last ones included, and the same counters."""
    from fs_eend_amd import audio_ingest as I
    from fs_eend_amd.audio_stream import AudioFrontEnd
    rng = random.Random(rate)
    n_in = R.smallest_input(8 * 800 + 123, rate)
    x = raw(n_in, encoding, 9)
    x8 = one_shot(I.AudioIngest(1, rate, encoding, device=dev), [x])[0]
    a = AudioFrontEnd(3, tr, device=dev, sample_rate=rate, encoding=encoding)
    b = AudioFrontEnd(3, tr, device=dev)
    got = fe_run(a, 2, x, uneven(n_in, rng) + [0])
    want = fe_run(b, 2, x8, uneven(x8.numel(), rng))
    assert got.shape == want.shape == (9, 345) and torch.equal(got, want)
    assert (a.table.recv[2], a.table.frames[2], a.table.mframes[2]) == (b.table.recv[2], b.table.frames[2], b.table.mframes[2])
    assert a.table.recv[2] == x8.numel() == a.ingest.table.outs[2] and a.ingest.table.recv[2] == n_in
    assert a.state(2) == a.ingest.state(2) == "ended"
    from fs_eend_amd.multistream import SlotError
    with pytest.raises(SlotError):
        a.feed({2: x[:10]})                                           # audio after the end
    with pytest.raises(TypeError):
        a.feed({0: torch.zeros(4, dtype=torch.uint8)})


def test_batch_equals_streamed(hip_lib, dev):
    from fs_eend_amd import audio_ingest as I, feature
    from fs_eend_amd.audio_stream import AudioFrontEnd
    rate, encoding = 48000, "s16"
    x = raw(R.smallest_input(3 * 256 + 7, rate) * 6, encoding, 21)                      # about 0.6 s
    x8 = I.convert(x.to(dev), rate, encoding)
    assert torch.equal(x8, one_shot(I.AudioIngest(1, rate, encoding, device=dev), [x])[0])
    for tr, tol in (("logmel23", 0.0), ("logmel23_cummn", 4e-6)):
        want = feature.extract_fbank_wave(x.to(dev), input_transform=tr, sample_rate=rate, encoding=encoding)
        assert torch.equal(want, feature.extract_fbank_wave(x8, input_transform=tr))
        got = fe_run(AudioFrontEnd(1, tr, device=dev, sample_rate=rate, encoding=encoding), 0, x, uneven(x.numel(), random.Random(3)))
        assert got.shape == want.shape and float((got - want).abs().max()) <= tol, (tr, float((got - want).abs().max()))
    with pytest.raises(TypeError):
        feature.extract_fbank_wave(x.to(dev).float(), input_transform="logmel23", sample_rate=rate, encoding=encoding)


# ------------------------------------------------------------------------------------------------ sessions and snapshots
def _sessions(kind, dev):
    from tests.test_audio_stream import _fs_model, _ls_model
    if kind == "fs":
        from fs_eend_amd.fs_multistream import FsMultiStreamSession
        sm, C = _fs_model(dev)
        return (lambda slots, **kw: FsMultiStreamSession(sm, slots, C, cap=64, **kw)), C
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    m, C = _ls_model(dev)
    return (lambda slots, **kw: LsMultiStreamSession(m, slots, C, **kw)), C


@pytest.mark.parametrize("kind", ["fs", "ls"])
def test_session_takes_16k_mulaw(hip_lib, dev, kind):
    """push / prefill / end with 16 kHz mu-law against the same session pushed the ingest's own 8 kHz floats, call for call."""
    from fs_eend_amd import audio_ingest as I
    from fs_eend_amd.audio_stream import AudioStreamSession
    mk, C = _sessions(kind, dev)
    rate, encoding = 16000, "mulaw"
    x = raw(2 * 8000 * 2 + 1234, encoding, 33)                                          # about 2 s
    ing = I.AudioIngest(1, rate, encoding, device=dev)
    ing.reset(0)
    A = AudioStreamSession(mk(2), sample_rate=rate, encoding=encoding)
    B = AudioStreamSession(mk(2))
    assert A.fe.sample_rate == rate and A.fe.encoding == encoding and B.fe.ingest is None
    A.open(), B.open()
    a, b = A.open(), B.open()
    cuts = [0, 9000, 9001, 9001, 20000, 27777, x.numel()]
    got, want = [], []
    for i, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        chunk = x[lo:hi]
        x8 = ing.feed({0: chunk})[0]
        if i == 0:
            got.append(A.prefill(a, chunk)), want.append(B.prefill(b, x8))
        else:
            got.append(A.push({a: chunk})[a]), want.append(B.push({b: x8})[b])
    x8 = ing.feed({}, end=[0])[0]
    assert x8.numel() == R.Z                                                            # the filter's latency comes out at the end
    got.append(A.end([a])[a]), want.append(B.end([b], {b: x8})[b])
    got, want = torch.cat(got), torch.cat(want)
    assert got.shape == want.shape == (21, C) and torch.equal(got, want)
    assert A.state(a) == B.state(b) == "done"


def test_front_end_snapshot_mid_history(hip_lib, dev):
    """A slot exported with samples in the ingest's history and adopted by a front-end with another slot count goes on bit for bit."""
    from fs_eend_amd.audio_stream import AudioFrontEnd
    rate, encoding = 44100, "s16"
    x = raw(44100 + 321, encoding, 45)
    cuts = [0, 20000, 30001, x.numel()]

    def run(cut, tr):
        fe, s, out = AudioFrontEnd(2, tr, device=dev, sample_rate=rate, encoding=encoding), 0, []
        fe.reset(s)
        for lo, hi in zip(cuts, cuts[1:]):
            out.append(fe.feed({s: x[lo:hi]})[s])
            if hi == cut:
                part = fe.export(s)
                assert 0 < hi - R.oldest(part["ingest"]["outs"], rate) < 256 and part["ingest"]["recv"] == hi       # mid-history
                fe.close(s)
                fe, s = AudioFrontEnd(3, tr, device=dev, sample_rate=rate, encoding=encoding), 1
                fe.reset(0)
                fe.check_part(part)
                fe.adopt(s, part)
                assert fe.ingest.state(s) == "open" and fe.ingest.table.recv[s] == hi
        out.append(fe.feed({}, end=[s])[s])
        return torch.cat(out)

    for tr in ("logmel23", "logmel23_cummn"):
        whole, got = run(None, tr), run(30001, tr)
        assert whole.shape == (11, 345) and torch.equal(got, whole), tr


def test_snapshot_with_ingest(hip_lib, dev, tmp_path):
    """A stream suspended with samples in the ingest's history, taken to the host, saved, loaded and resumed in a stack with
    another slot count goes on bit for bit (the stacks of tests/test_ls_suspend.py's audio test); a front-end at another rate
    or encoding, or without an ingest, refuses it and stays as it was."""
    from fs_eend_amd.audio_stream import AudioFrontEnd, AudioStreamSession
    from fs_eend_amd.multistream import SlotError, StreamSnapshot
    mk, C = _sessions("ls", dev)
    rate, encoding = 44100, "s16"
    x = raw(2 * 44100 + 321, encoding, 44)
    cuts = [0, 30000, 50001, 70000, x.numel()]

    def run(suspend_at):
        A = AudioStreamSession(mk(3), sample_rate=rate, encoding=encoding)
        s, out = A.open(), []
        for lo, hi in zip(cuts, cuts[1:]):
            out.append(A.push({s: x[lo:hi]})[s])
            if hi == suspend_at:
                snap = A.suspend(s)
                ing = snap.parts["frontend"]["ingest"]
                assert set(snap.parts["frontend"]) == TODAY_KEYS | {"ingest"}
                assert set(ing) == {"config", "hist", "recv", "outs"} and ing["recv"] == hi
                assert ing["config"] == {"rate": rate, "encoding": encoding, "zeros": 16, "beta": 9.0, "rolloff": 0.9}
                assert 0 < hi - R.oldest(ing["outs"], rate) < 256 and bool(ing["hist"].abs().sum() > 0)    # mid-history
                cpu = snap.to("cpu")
                assert cpu.parts["frontend"]["ingest"]["hist"].device.type == "cpu"
                assert torch.equal(cpu.parts["frontend"]["ingest"]["hist"], ing["hist"].cpu())
                path = str(tmp_path / "call.snap")
                cpu.save(path)
                snap = StreamSnapshot.load(path)
                for kw in (dict(sample_rate=48000, encoding=encoding), dict(sample_rate=rate, encoding="f32"), dict()):
                    other = AudioStreamSession(mk(2), **kw)
                    with pytest.raises(SlotError, match="ingest"):
                        other.resume(snap)
                    assert other.state(0) == "free" and other.fe.state(0) == "free"
                A = AudioStreamSession(mk(4, use_graph=False), sample_rate=rate, encoding=encoding)
                A.open()
                s = A.resume(snap)
                assert s == 1 and A.fe.ingest.table.recv[s] == hi and A.fe.ingest.state(s) == "open"
        out.append(A.end([s])[s])
        return torch.cat(out)

    whole, got = run(None), run(50001)
    assert whole.shape == (21, C)
    assert torch.equal(got, whole), f"max diff {float((got - whole).abs().max()):.3e}"
    plain = AudioFrontEnd(2, "logmel23", device=dev)
    plain.reset(0)
    assert set(plain.export(0)) == TODAY_KEYS
    with_ingest = AudioFrontEnd(2, "logmel23", device=dev, sample_rate=rate, encoding=encoding)
    with_ingest.reset(0)
    with pytest.raises(SlotError, match="ingest"):
        with_ingest.check_part(plain.export(0))                       # a snapshot of 8 kHz float audio into an ingesting front-end
