"""GPU: labelled training batches built on the device (fs_eend_amd/device_data.py, eend_chunk_batch_f32).  Every comparison is
exact: the features against the single-waveform path `feature.extract_fbank_wave` on the chunk's slice (itself pinned to the oracle
by test_feature_gpu.py), the labels against the numpy restatement of the reference's rule (tests/chunk_label_ref.py, pinned to the
reference by tests/golden/chunk_labels.json)."""
import numpy as np
import pytest
import torch

import chunk_label_ref as R

CASES = R.load_golden()

pytestmark = pytest.mark.gpu

LENS = {"r0": 10400, "r1": 20013, "r2": 5120}
TRANSFORMS = ("logmel23", "logmel23_mn", "logmel23_cummn")
# frame counts 1 (clipped, 13 samples), 1, 9, 10, 11, 63, 64, 65, 129 (clipped), 64 (a whole file), 0 (at the file's end), 51 (clipped, an
# odd tail), 20 (all-zero audio); r0, r1 and r2 all appear more than once
ROWS = [("r1", 250, 251), ("r0", 5, 6), ("r0", 0, 9), ("r0", 20, 30), ("r1", 3, 14), ("r1", 100, 163), ("r0", 10, 74), ("r1", 100, 165),
        ("r0", 1, 200), ("r2", 0, 64), ("r1", 251, 300), ("r1", 200, 300), ("r2", 20, 40)]
FRAMES = [1, 1, 9, 10, 11, 63, 64, 65, 129, 64, 0, 51, 20]


def _segments():
    rng = np.random.default_rng(5)
    seg, utt2spk = {}, {}
    st = rng.uniform(0.0, 2.4, 40)
    seg["r1"] = [(f"u{i}", float(st[i]), float(st[i] + rng.uniform(0.02, 0.8))) for i in range(40)]      # 40 segments over 4 speakers
    utt2spk.update({f"u{i}": f"spk{i % 4}" for i in range(40)})
    seg["r0"] = [("a0", 0.0, 0.31), ("a1", 0.25, 0.8), ("a2", 0.74, 1.3), ("a3", 0.055, 0.065)]
    utt2spk.update({"a0": "B", "a1": "A", "a2": "B", "a3": "A"})
    seg["r2"] = [("c0", 0.1, 0.5)]
    utt2spk["c0"] = "C"
    return seg, utt2spk


@pytest.fixture(scope="module")
def world(hip_lib, dev):
    """The three recordings, an f32 and an s16 corpus of them, and the single-waveform features of every chunk (computed once)."""
    from fs_eend_amd import device_data as DD, feature
    g = torch.Generator().manual_seed(11)
    s16 = {r: torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int32).to(torch.int16) for r, n in LENS.items()}
    f32 = {r: torch.randn(n, generator=g) * 0.1 for r, n in LENS.items()}
    f32["r2"][1600:3200] = 0.0                              # chunk ("r2", 20, 40) is all-zero audio
    seg, utt2spk = _segments()
    corp = {}
    for storage, waves in (("f32", f32), ("s16", s16)):
        c = DD.DeviceCorpus(dev, storage=storage)
        for r in LENS:
            c.add(r, waves[r], seg[r], utt2spk)
        corp[storage] = c.finalize()
    want = {}
    for storage, waves in (("f32", f32), ("s16", {r: w.float() / 32768 for r, w in s16.items()})):
        for tr in TRANSFORMS:
            for ctx, sub in ((7, 10), (0, 1)):
                want[storage, tr, ctx, sub] = [feature.extract_fbank_wave(waves[r][st * 80:ed * 80].to(dev), ctx, 200, 80, tr, sub)
                                               for r, st, ed in ROWS]
    torch.cuda.synchronize()
    return {"corpus": corp, "want": want, "seg": seg, "utt2spk": utt2spk, "f32": f32}


def test_chunk_frame_counts(world):
    feats, labels, recs = world["corpus"]["f32"].batch(ROWS, context_size=0, subsampling=1, input_transform="logmel23")
    assert [f.shape[0] for f in feats] == FRAMES and recs == [r[0] for r in ROWS]
    assert all(f.shape[1] == 23 and f.dtype == torch.float32 for f in feats)


@pytest.mark.parametrize("storage", ["f32", "s16"])
@pytest.mark.parametrize("ctx,sub", [(7, 10), (0, 1)])
@pytest.mark.parametrize("transform", TRANSFORMS)
def test_features_are_the_single_waveform_path_bit_for_bit(world, transform, ctx, sub, storage):
    feats, _, _ = world["corpus"][storage].batch(ROWS, context_size=ctx, subsampling=sub, input_transform=transform)
    want = world["want"][storage, transform, ctx, sub]
    assert len(feats) == len(ROWS)
    for row, n, got, ref in zip(ROWS, FRAMES, feats, want):
        assert got.shape == ref.shape == (-(-n // sub), 23 * (2 * ctx + 1)), row
        assert torch.equal(got, ref), (row, transform)


def test_all_zero_audio_reaches_the_floor(world):
    b = ROWS.index(("r2", 20, 40))
    feats, _, _ = world["corpus"]["f32"].batch(ROWS, context_size=0, subsampling=1, input_transform="logmel23")
    # every element is the floor itself, log10f(1e-10f): one value, finite, -10 to within an ulp of the device's log10f
    floor = feats[b][0, 0].item()
    assert feats[b].shape == (20, 23) and torch.equal(feats[b], torch.full_like(feats[b], floor))
    assert abs(floor + 10.0) <= 2 * 2.0 ** -20, floor        # ulp(10) in float32 is 2^-20
    assert torch.equal(feats[b], world["want"]["f32", "logmel23", 0, 1][b])
    mn, _, _ = world["corpus"]["f32"].batch(ROWS, context_size=0, subsampling=1, input_transform="logmel23_mn")
    assert torch.equal(mn[b], torch.zeros_like(mn[b]))


@pytest.mark.parametrize("sub", [10, 1])
@pytest.mark.parametrize("n_speakers", [None, 5])
def test_labels_follow_the_reference_rule(world, sub, n_speakers):
    _, labels, _ = world["corpus"]["f32"].batch(ROWS, subsampling=sub, n_speakers=n_speakers)
    for (r, st, ed), n, got in zip(ROWS, FRAMES, labels):
        T = R.chunk_labels(world["seg"][r], world["utt2spk"], LENS[r], st, ed, n_speakers)
        assert T.shape[0] == n
        ref = R.subsampled(T, sub)
        assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape == (-(-n // sub), n_speakers or {"r0": 2, "r1": 4, "r2": 1}[r])
        assert np.array_equal(got.cpu().numpy(), ref), (r, st, ed)
        assert set(np.unique(got.cpu().numpy()).tolist()) <= {0.0, 1.0}
    active = sum(float(l.sum()) for l in labels)
    assert active > 0                                       # the table is not vacuous


@pytest.mark.parametrize("n_speakers", [None, 4])
def test_labels_on_the_golden_segment_sets(hip_lib, dev, n_speakers):
    """One recording per golden case; the expected matrices are the reference's own where the case's n_speakers is the batch's."""
    from fs_eend_amd import device_data as DD
    c = DD.DeviceCorpus(dev)
    for case in CASES:
        c.add(case["name"], torch.zeros(case["file_len"]), case["segments"], case["utt2spk"])
    c.finalize()
    rows = [(case["name"], case["start"], case["end"]) for case in CASES]
    for sub in (1, 10):
        _, labels, _ = c.batch(rows, context_size=0, subsampling=sub, input_transform="logmel23", n_speakers=n_speakers)
        for case, got in zip(CASES, labels):
            T = R.chunk_labels(case["segments"], case["utt2spk"], case["file_len"], case["start"], case["end"], n_speakers)
            if case["n_speakers"] == n_speakers:
                assert np.array_equal(T, case["T"])
            assert np.array_equal(got.cpu().numpy(), R.subsampled(T, sub)), case["name"]


def test_a_chunk_does_not_depend_on_its_batch(world):
    c = world["corpus"]["f32"]
    x = ("r1", 100, 165)
    others = [("r0", 1, 200), ("r1", 250, 251), ("r1", 100, 165), ("r2", 0, 64), ("r1", 251, 300), ("r0", 0, 9)]
    def run(rows, b):
        f, l, _ = c.batch(rows, input_transform="logmel23_cummn")
        return f[b].clone(), l[b].clone()                   # the pool is overwritten by the next call
    alone = run([x], 0)
    assert alone[0].shape == (7, 345) and alone[1].shape == (7, 4)
    for rows, b in ((([x] + others), 0), ((others + [x]), 6), ((others[:3] + [x] + others[3:]), 3)):
        assert len(rows) == 7
        got = run(rows, b)
        assert torch.equal(got[0], alone[0]) and torch.equal(got[1], alone[1]), b
    c.batch(ROWS * 3, context_size=0, subsampling=1)        # grows and dirties every buffer of the pool
    again = run([x], 0)
    assert torch.equal(again[0], alone[0]) and torch.equal(again[1], alone[1])


def test_a_repeated_batch_shape_allocates_nothing(world):
    c = world["corpus"]["f32"]
    c.batch(ROWS)
    ptrs = {k: v.data_ptr() for k, v in c._pool.items()}
    a = [f.clone() for f in c.batch(ROWS)[0]]
    b = c.batch(ROWS)[0]
    assert {k: v.data_ptr() for k, v in c._pool.items()} == ptrs
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_training_step_on_a_collated_batch(hip_lib, dev):
    """SpeakerDiarization.training_step on corpus.collate's batch gives, bit for bit, the loss of the same chunks built one by one
    with extract_fbank_wave and the CPU restatement of the labels (a small FS config, T = 40 model frames)."""
    from fs_eend_amd import device_data as DD, feature
    from fs_eend_amd.fs_model import OnlineTransformerDADiarization
    from fs_eend_amd.trainer import SpeakerDiarization
    g = torch.Generator().manual_seed(23)
    wave = torch.randn(40000, generator=g) * 0.1
    seg = [("a", 0.2, 1.9), ("b", 1.5, 3.6), ("c", 3.2, 4.4), ("d", 0.0, 0.4)]
    utt2spk = {"a": "s0", "b": "s1", "c": "s0", "d": "s1"}
    corpus = DD.DeviceCorpus(dev)
    corpus.add("rec", wave, seg, utt2spk)
    corpus.finalize()
    ds = DD.ChunkDataset(corpus, [("rec", 0, 400), ("rec", 90, 490)])
    rows = [ds[0], ds[1]]

    def module(collate):
        torch.manual_seed(3)
        m = OnlineTransformerDADiarization(n_speakers=None, in_size=345, n_units=256, n_heads=4, enc_n_layers=1, dec_n_layers=1,
                                           dropout=0.0, has_mask=True, max_seqlen=500, dec_dim_feedforward=256,
                                           mask_delay=0).to(dev).train()
        hp = dict(data=dict(max_speakers=3, label_delay=0),
                  training=dict(lr=1.0, warm_steps=50, schedule_scale=1.0, grad_clip=5.0, batch_size=2, shuffle=False, seed=5))
        return SpeakerDiarization(hp, m, {"train": ds}, dict(lr=1.0, betas=(0.9, 0.98), eps=1e-9), dict(warmup_steps=50, scale=1.0), collate)

    a = module(corpus.collate(7, 10, "logmel23_mn"))
    batch = next(iter(a.train_dataloader()))                # the module's own loader: ChunkDataset rows -> corpus.collate
    assert [f.shape for f in batch[0]] == [(40, 345)] * 2 and [l.shape for l in batch[1]] == [(40, 2)] * 2 and batch[2] == ["rec"] * 2
    loss_a = a.training_step(batch, 0)
    feats = [feature.extract_fbank_wave(wave[st * 80:ed * 80].to(dev), 7, 200, 80, "logmel23_mn", 10) for _, st, ed in rows]
    labels = [torch.from_numpy(R.subsampled(R.chunk_labels(seg, utt2spk, 40000, st, ed), 10)) for _, st, ed in rows]
    b = module(None)
    loss_b = b.training_step((feats, labels, ["rec"] * 2), 0)
    torch.cuda.synchronize()
    assert torch.isfinite(torch.as_tensor(loss_a)).all()
    assert torch.equal(torch.as_tensor(loss_a), torch.as_tensor(loss_b))
