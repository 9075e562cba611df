"""GPU: the incremental audio front-end (audio_stream.AudioFrontEnd) against the batch front-end on the same whole waveform --
bit-identical for logmel23, within an ulp of the running mean for logmel23_cummn, and bit-identical to itself across
chunkings, slot placement, neighbours, pauses and NaN left behind by an earlier stream -- and AudioStreamSession end to end
over both multi-stream sessions."""
import random

import numpy as np
import pytest
import torch

from oracle import feature_ref as R
from oracle import fixtures as FX
from tests.helpers import build_fs_mirror, build_ls_mirror
from tests.test_feature_gpu import wave

pytestmark = pytest.mark.gpu
LENGTHS = [0, 1, 79, 80, 81, 99, 100, 659, 660, 661, 8000, 23456]


def sizes_of(n, kind, rng):
    if kind == "whole":
        return [n]
    if kind == "ones":
        return [1] * min(n, 700) + ([n - 700] if n > 700 else [])
    if kind in (79, 80, 81, 800):
        return [kind] * (n // kind) + ([n % kind] if n % kind else [])
    cuts = sorted(rng.randrange(n + 1) for _ in range(rng.randrange(1, 10)))
    return [b - a for a, b in zip([0] + cuts, cuts + [n])]


def drive(fe, streams, seed, pause=0.3):
    """streams: [(slot, waveform np.float32, chunk sizes)] fed together, each ending after its last chunk; a stream skips a
    call with probability `pause`; chunks alternate between CPU and GPU tensors.  -> [its model frames]"""
    rng = random.Random(seed)
    dev = fe.dev
    for s, _, _ in streams:
        fe.reset(s)
    pos, k = [0] * len(streams), [0] * len(streams)
    out = [[] for _ in streams]
    active = set(range(len(streams)))
    calls = 0
    while active:
        waves, end, who = {}, [], {}
        for i in sorted(active):
            if rng.random() < pause:
                continue
            s, y, sizes = streams[i]
            who[s] = i
            if k[i] < len(sizes):
                m = sizes[k[i]]
                w = torch.from_numpy(y[pos[i]:pos[i] + m])
                waves[s] = w.to(dev) if (calls + i) % 2 else w
                pos[i] += m
                k[i] += 1
            else:
                end.append(s)
        got = fe.feed(waves, end=end)
        assert set(got) == set(who)
        for s, v in got.items():
            assert v.shape[1] == fe.width and v.dtype == torch.float32 and v.is_cuda
            out[who[s]].append(v)
        for s in end:
            active.discard(who[s])
        calls += 1
    return [torch.cat(v) for v in out]


def batch(y, tr, dev, ctx=7, sub=10):
    from fs_eend_amd import feature
    if y.size == 0:
        return torch.zeros(0, 23 * (2 * ctx + 1), device=dev)
    return feature.extract_fbank_wave(torch.from_numpy(y).to(dev), context_size=ctx, subsampling=sub, input_transform=tr)


@pytest.mark.parametrize("ctx,sub", [(7, 10), (0, 1), (2, 4)])
def test_logmel23_bit_identical_to_batch(hip_lib, dev, ctx, sub):
    from fs_eend_amd.audio_stream import AudioFrontEnd
    rng = random.Random(ctx + 100 * sub)
    fe = AudioFrontEnd(6, "logmel23", ctx, sub, device=dev)
    kinds = ["whole", "ones", 79, 80, 81, 800, "random"]
    cases = [(n, kind) for n in LENGTHS for kind in kinds]
    for r in range(0, len(cases), 6):                                   # six streams of different lengths per front-end call
        group = cases[r:r + 6]
        streams = [(s, wave(n, n + s), sizes_of(n, kind, rng)) for s, (n, kind) in enumerate(group)]
        got = drive(fe, streams, seed=r)
        for (s, y, _), g, (n, kind) in zip(streams, got, group):
            want = batch(y, "logmel23", dev, ctx, sub)
            assert g.shape == want.shape, (n, kind, g.shape, want.shape)
            assert torch.equal(g, want), (n, kind, float((g - want).abs().max()))


def test_cummn_matches_batch_and_oracle(hip_lib, dev):
    from fs_eend_amd.audio_stream import AudioFrontEnd
    rng = random.Random(7)
    fe = AudioFrontEnd(4, "logmel23_cummn", device=dev)
    for n in [1, 80, 661, 8000, 16123, 160000]:
        y = wave(n, n)
        variants = []
        for slot, kind in [(0, "whole"), (3, "ones"), (1, 81), (2, "random"), (0, 800)]:
            neighbours = [(s, wave(5000 + 37 * s, s), sizes_of(5000 + 37 * s, "random", rng)) for s in range(4) if s != slot]
            got = drive(fe, [(slot, y, sizes_of(n, kind, rng))] + neighbours, seed=n + slot)[0]
            variants.append(got)
        want = batch(y, "logmel23_cummn", dev)
        ref = R.extract_fbank_wave(y, input_transform="logmel23_cummn")
        for g in variants:
            assert torch.equal(g, variants[0])                          # the chunking, slot and neighbours do not matter
        g = variants[0]
        assert g.shape == want.shape == ref.shape
        assert float((g - want).abs().max()) <= 4e-6, float((g - want).abs().max())
        assert np.abs(g.cpu().numpy() - ref).max() <= 2e-4


def test_cummn_ten_minutes(hip_lib, dev):
    from fs_eend_amd.audio_stream import AudioFrontEnd
    y = wave(4_800_000, 3)
    rng = random.Random(3)
    fe = AudioFrontEnd(2, "logmel23_cummn", device=dev)
    sizes, left = [], y.size
    while left:
        sizes.append(min(left, rng.randrange(1, 120_000)))
        left -= sizes[-1]
    got = drive(fe, [(1, y, sizes)], seed=0, pause=0.0)[0]
    lm = R.transform(R.stft(y), "logmel23_cummn")
    want = R.splice(lm, 7)[::10]
    assert got.shape == want.shape == (6000, 345)
    assert np.abs(got.cpu().numpy() - want).max() < 5e-4


@pytest.mark.parametrize("tr", ["logmel23", "logmel23_cummn"])
def test_slot_reused_after_nan_stream(hip_lib, dev, tr):
    from fs_eend_amd.audio_stream import AudioFrontEnd
    y = wave(9001, 11)
    fresh = drive(AudioFrontEnd(3, tr, device=dev), [(0, y, [1234, 4000, 3767])], seed=1, pause=0.0)[0]
    fe = AudioFrontEnd(3, tr, device=dev)
    bad = np.full(7777, np.nan, dtype=np.float32)
    drive(fe, [(2, bad, [100, 5000, 2677])], seed=2, pause=0.0)
    assert bool(fe.tail[2].isnan().any())
    fe.tail[2], fe.ring[2], fe.sums[2] = float("nan"), float("nan"), float("nan")   # whatever an earlier stream could leave
    fe.reset(2)
    fe.feed({2: torch.from_numpy(bad[:3000])})                          # reset in the middle of another NaN stream
    again = drive(fe, [(2, y, [1234, 4000, 3767])], seed=3, pause=0.0)[0]
    assert torch.equal(again, fresh)


def test_front_end_errors(hip_lib, dev):
    from fs_eend_amd.audio_stream import AudioFrontEnd
    from fs_eend_amd.multistream import SlotError
    fe = AudioFrontEnd(2, "logmel23", device=dev)
    with pytest.raises(SlotError):
        fe.feed({0: torch.zeros(100)})                                  # not reset
    fe.reset(0)
    with pytest.raises(SlotError):
        fe.feed({5: torch.zeros(100)})
    with pytest.raises(TypeError):
        fe.feed({0: torch.zeros(100, dtype=torch.int16)})
    out = fe.feed({0: torch.zeros(100, device=dev)}, end=[0])
    assert out[0].shape == (1, 345)
    with pytest.raises(SlotError):
        fe.feed({0: torch.zeros(10)})
    assert fe.feed({}) == {}


@pytest.mark.parametrize("rate,encoding", [(8000, "f32"), (16000, "s16")])
def test_cpu_chunks_of_odd_length_in_one_staging_block(hip_lib, dev, rate, encoding):
    """Three slots fed together: per call 81 samples for slot 0 and 1 sample for slot 1 as CPU tensors (an odd-length chunk
    followed by another CPU chunk, each placed on its own 8-byte boundary of the staging block) and 160 samples for slot 2
    as a GPU tensor, until slot 0 has passed 900 samples.  Bit for bit the batch front-end of each whole waveform."""
    from fs_eend_amd import feature
    from fs_eend_amd.audio_stream import AudioFrontEnd
    fe = AudioFrontEnd(3, "logmel23", 2, 4, device=dev, sample_rate=rate, encoding=encoding)
    per_call, calls = [81, 1, 160], 900 // 81 + 1
    whole = [wave(m * calls, 50 + s) for s, m in enumerate(per_call)]
    if encoding == "s16":
        whole = [(y * 16384).astype(np.int16) for y in whole]
    whole = [torch.from_numpy(y) for y in whole]
    for s in range(3):
        fe.reset(s)
    out = [[] for _ in whole]
    for k in range(calls + 1):
        cut = [y[m * k:m * (k + 1)] for y, m in zip(whole, per_call)]
        got = fe.feed({0: cut[0], 1: cut[1], 2: cut[2].to(dev)}) if k < calls else fe.feed({}, end=[0, 1, 2])
        for s in range(3):
            out[s].append(got[s])
    assert (fe.table if fe.ingest is None else fe.ingest.table).recv[0] == 81 * calls > 900
    for s, y in enumerate(whole):
        want = feature.extract_fbank_wave(y.to(dev), context_size=2, subsampling=4, input_transform="logmel23", sample_rate=rate,
                                          encoding=encoding)
        g = torch.cat(out[s])
        assert g.shape == want.shape and want.shape[0] > 0, (s, g.shape, want.shape)
        assert torch.equal(g, want), (s, float((g - want).abs().max()))


# ---------------------------------------------------------------------------------------------- end to end
def _fs_model(dev):
    from fs_eend_amd.fs_stream import StreamingTransformerEDADiarization, copy_params_from_masked_to_streaming
    meta, _ = FX.load_case("fs_stream_T60")
    m = build_fs_mirror(meta).to(dev)
    sm = StreamingTransformerEDADiarization(in_size=meta["in_size"], **meta["cfg"]).eval().to(dev)
    copy_params_from_masked_to_streaming(m, sm)
    return sm, meta["C"]


def _ls_model(dev):
    meta, _ = FX.load_case("ls_stream_T120")
    return build_ls_mirror(meta).to(dev), meta["C"]


def feature_path(ses, feats):
    """Each stream's features pushed frame by frame through the session on its own, then flushed -> (T, C) logits."""
    out = []
    for f in feats:
        s = ses.open()
        ys = [ses.step(push={s: f[t]}) for t in range(f.shape[0])]
        ys.append(ses.step(flush=[s]))
        while ses.state(s) == "flushing":
            ys.append(ses.step())
        ses.close(s)
        out.append(torch.cat([y[s].reshape(1, -1) for y in ys if s in y]))
    return out


def audio_path(ases, waves, seed, max_chunk=6000):
    """The streams open at staggered rounds, push random chunks with random pauses and end when their audio runs out."""
    rng = random.Random(seed)
    start = [3 * i for i in range(len(waves))]
    slot, pos, out = {}, [0] * len(waves), [[] for _ in waves]
    rnd = 0
    while rnd <= start[-1] or slot:
        for i, st in enumerate(start):
            if st == rnd:
                slot[i] = ases.open()
        push, end = {}, []
        for i, s in slot.items():
            if rng.random() < 0.25:
                continue
            y = waves[i]
            if pos[i] < y.size:
                m = rng.randrange(0, max_chunk)
                push[s] = torch.from_numpy(y[pos[i]:pos[i] + m])
                pos[i] += m
            else:
                end.append(s)
        by = {s: i for i, s in slot.items()}
        for s, v in ases.push(push).items():
            assert v.shape[1] == ases.C
            out[by[s]].append(v)
        if end:
            for s, v in ases.end(end).items():
                out[by[s]].append(v)
                assert ases.state(s) == "done"
                ases.close(s)
                del slot[by[s]]
        rnd += 1
    return [torch.cat(v) for v in out]


@pytest.mark.parametrize("use_graph", [True, False])
def test_fs_audio_session_bit_identical_to_feature_path(hip_lib, dev, use_graph):
    from fs_eend_amd import postproc
    from fs_eend_amd.audio_stream import AudioStreamSession
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    sm, C = _fs_model(dev)
    waves = [wave(8000 * 3 + 4321, 1), wave(8000 * 8, 2), wave(8000 * 5 + 79, 3), wave(8000 * 4 + 1, 4)]
    feats = [batch(y, "logmel23", dev) for y in waves]
    want = feature_path(FsMultiStreamSession(sm, 4, C, cap=256, use_graph=use_graph), feats)
    ases = AudioStreamSession(FsMultiStreamSession(sm, 4, C, cap=256, use_graph=use_graph))
    assert ases.fe.input_transform == "logmel23"
    got = audio_path(ases, waves, seed=int(use_graph))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape == (feats[i].shape[0], C), (i, g.shape, w.shape)
        assert torch.equal(g, w), (i, float((g - w).abs().max()))
        assert postproc.make_rttm("utt", torch.sigmoid(g[:, 1:])) == postproc.make_rttm("utt", torch.sigmoid(w[:, 1:]))


def test_ls_audio_session_matches_feature_path(hip_lib, dev):
    from fs_eend_amd.audio_stream import AudioStreamSession
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    m, C = _ls_model(dev)
    waves = [wave(8000 * 3 + 555, 5), wave(8000 * 6, 6), wave(8000 * 4 + 80, 7)]
    feats = [batch(y, "logmel23_cummn", dev) for y in waves]
    want = feature_path(LsMultiStreamSession(m, 4, C), feats)
    runs = []
    for seed, max_chunk in [(0, 6000), (1, 900)]:
        ases = AudioStreamSession(LsMultiStreamSession(m, 4, C))
        assert ases.fe.input_transform == "logmel23_cummn"
        runs.append(audio_path(ases, waves, seed=seed, max_chunk=max_chunk))
    for i, w in enumerate(want):
        a, b = runs[0][i], runs[1][i]
        assert a.shape == b.shape == w.shape
        assert torch.equal(a, b), (i, float((a - b).abs().max()))     # two chunkings of the same audio
        assert float((a - w).abs().max()) <= 1e-4, float((a - w).abs().max())


def test_audio_session_zero_length_and_errors(hip_lib, dev):
    from fs_eend_amd.audio_stream import AudioStreamSession
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    from fs_eend_amd.multistream import SlotError
    sm, C = _fs_model(dev)
    ases = AudioStreamSession(FsMultiStreamSession(sm, 2, C, cap=64))
    a = ases.open()
    assert ases.push({a: torch.zeros(0)})[a].shape == (0, C)
    assert ases.end([a])[a].shape == (0, C)
    assert ases.state(a) == "done"
    with pytest.raises(SlotError):
        ases.push({a: torch.zeros(10)})
    ases.close(a)
    with pytest.raises(ValueError):
        AudioStreamSession(FsMultiStreamSession(sm, 2, C, cap=64), context_size=3)     # 161 features for a 345-input model
