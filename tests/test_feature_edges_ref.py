"""CPU: the references and probes of tests/feature_edge_ref.py really pin the feature front-end kernels -- `ref_logmel` restates what
oracle/feature_ref.py computes, every probe the GPU tests use passes the exactness guard, each one-step indexing mistake (a window tap
dropped at a slice boundary, a frame one hop late at the block boundary, Re / Im paired one column off, a mel row too many, `len`
taken inclusive, `first` off by one) moves an output of the GPU cases by more than 64 times the bar it is compared under, the
normalisation reference equals the oracle's, and the project's own planners tile the cut lists of the GPU walk exactly once within
the ring, STFT-tile and splice-tile limits."""
import numpy as np
import pytest

from oracle import feature_ref as R
from tests import feature_edge_ref as E
from tests import test_feature_edges as G


# ---------------------------------------------------------------------------------------------------- log-mel reference
def test_ref_logmel_restates_the_oracle():
    """float64 tables by the header's formula: ref_logmel equals the oracle's chain run without its float32 casts to float64 accuracy,
    and the oracle as it stands (float32 window, complex64 spectrum: 2^-24 relative per bin, far below every mel power here) to 2e-6."""
    n = 16123
    y = E.speechlike(n, 1)
    T = E.stft_frames(n)
    dft, melT = E.header_tables()
    got = E.ref_logmel(y, n, -100, T, dft, melT)
    yp = np.pad(y.astype(np.float64), 128)
    fr = yp[np.arange(256)[None, :] + 80 * np.arange(T)[:, None]] * R.hann_padded(200, 256)[None, :]
    want64 = np.log10(np.maximum((np.abs(np.fft.rfft(fr, axis=1)) ** 2) @ R.mel_filterbank(8000, 256, 23).astype(np.float64).T, 1e-10))
    e64 = np.abs(got - want64).max()
    want = R.transform(R.stft(y), "logmel23", dtype=np.float64)
    e32 = np.abs(got - want).max()
    print(f"ref_logmel vs float64 oracle chain {e64:.3e}, vs oracle/feature_ref as it stands {e32:.3e}")
    assert want.shape == got.shape == (T, 23) and e64 < 1e-11 and e32 < 2e-6
    # pre-padded host (first = 28) and a length that is a multiple of the hop (the excess frame dropped)
    n2 = 8000
    y2 = E.speechlike(n2, 2)
    got2 = E.ref_logmel(np.pad(y2, 128, mode="reflect"), n2 + 256, 28, E.stft_frames(n2), dft, melT)
    want2 = R.transform(R.stft(y2, pad_mode="reflect"), "logmel23", dtype=np.float64)
    assert got2.shape == want2.shape == (100, 23) and np.abs(got2 - want2).max() < 2e-6


def test_production_tables_are_the_headers():
    """feature._tables is the header's table rounded to float32, zero in every column the production path leaves unused; with it
    ref_logmel stays within the table's rounding (2^-24 per entry) of the oracle"""
    from fs_eend_amd import feature
    dft32, melT32 = (t.numpy() for t in feature._tables("cpu"))
    dft, melT = E.header_tables()
    assert dft32.dtype == melT32.dtype == np.float32 and np.array_equal(melT32, melT.astype(np.float32))
    assert np.abs(dft32.astype(np.float64) - dft).max() <= 2.0 ** -24                 # |entries| <= 1: half an ulp, libm differences included
    assert not dft32[:, 129:144].any() and not dft32[:, 273:].any() and not melT32[129:].any() and not melT32[:, 23:].any()
    n = 8123
    y = E.speechlike(n, 3)
    got = E.ref_logmel(y, n, -100, E.stft_frames(n), dft32, melT32)
    want = R.transform(R.stft(y), "logmel23", dtype=np.float64)
    err = np.abs(got - want).max()
    print(f"ref_logmel with the production tables vs oracle: {err:.3e}")
    assert err < 1e-5


def test_ignored_columns_do_not_show_and_read_ones_do():
    n = 80 * 20 + 199
    for name in E.PROBES:
        y, dft, melT = E.probe(name, n)
        base = E.ref_melpower(y, n, 0, 20, dft, melT)
        d2, m2 = dft.copy(), melT.copy()
        d2[:, E.IGNORED_DFT] = 0
        m2[:, E.NMEL:] = 0
        assert np.array_equal(base, E.ref_melpower(y, n, 0, 20, d2, m2))
        d3, m3 = dft.copy(), melT.copy()
        d3[:, [129, 130, 131, 273, 274, 275]] = 0
        m3[129:] = 0
        assert not np.array_equal(base, E.ref_melpower(y, n, 0, 20, d3, m3)), name     # bins 129..131 carry weight in every probe


# ---------------------------------------------------------------------------------------------------- probes
@pytest.mark.parametrize("name", E.PROBES)
def test_probes_are_exact(name):
    y, dft, melT = E.probe(name, 12000)
    worst = E.assert_exact(y, dft, melT)
    print(f"{name}: largest partial-sum bound {worst:.0f} of {E.LIMIT}")
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y) and np.array_equal(y.astype(np.int16).astype(np.float64), y)
    if name == "dense":                                                                # every tap feeds a used column, every used column has taps
        assert np.abs(dft[:, E.USED_DFT]).sum(1).min() > 0 and np.abs(dft[:, E.USED_DFT]).sum(0).min() > 0 and (np.abs(y) >= 1).all()
    assert E.assert_exact(y / 32768.0, dft, melT, unit=2.0 ** -15) == worst           # the s16 decoding only scales by a power of two
    with pytest.raises(AssertionError):
        E.assert_exact(y * 4096.0, dft, melT)
    with pytest.raises(AssertionError):
        E.assert_exact(y + 0.5, dft, melT)


def test_pick_probe_outputs_are_single_samples():
    n = 12000
    for v in (0, 1):
        y, dft, melT = E.probe(f"pick{v}", n)
        L = E.ref_logmel(y, n, -100, 129, dft, melT)
        for t in (0, 1, 63, 64, 128):
            for m in range(E.NMEL):
                i = -100 + 80 * t + E.PICK_TAPS[v][m]
                assert L[t, m] == (np.log10(y[i] ** 2) if i >= 0 else -10.0)
        vals = np.unique(L[L > -10.0])
        assert np.diff(vals).min() >= E.PICK_STEP * (1 - 1e-9) and 64 * G.BARS["logmel probe abs"] < E.PICK_STEP
    for w in range(0, 11000, 997):                                                     # distinct within any 1000 consecutive samples
        assert len(set(E.pick_samples(n)[w:w + 1000])) == 1000
    assert sorted(set(E.PICK_TAPS[0]) & {19, 20, 99, 100, 199}) == [19, 20, 99, 100, 199]


@pytest.mark.parametrize("name", E.PROBES)
@pytest.mark.parametrize("mutation", E.MUTATIONS)
def test_mutations_show(name, mutation):
    """each seeded mistake moves at least one output of the (first = -100, 129 frames) GPU case by more than 64 bars; the two that act
    on `len` at the cases whose length ends inside the launch"""
    first, nf = -100, 129
    last = first + 80 * (nf - 1) + 199
    y, dft, melT = E.probe(name, last + 400)
    shown = 0.0
    for length in E.stft_lengths(first, nf) + [last - 57]:
        want = E.ref_logmel(y, length, first, nf, dft, melT)
        shown = max(shown, np.abs(E.ref_logmel(y, length, first, nf, dft, melT, mutation) - want).max())
    print(f"{name} {mutation}: moves an output by {shown:.3e} (64 bars = {64 * G.BARS['logmel probe abs']:.3e})")
    if name == "pick1" and mutation.startswith("drop_tap"):
        assert shown == 0.0                       # pick1 reads none of those taps: pick0 carries them
        return
    assert shown > 64 * G.BARS["logmel probe abs"]


def test_mutations_show_with_the_production_tables():
    """the real-table cases see them too, each far beyond 64 times their own bar"""
    from fs_eend_amd import feature
    dft, melT = (t.numpy() for t in feature._tables("cpu"))
    first, nf = -100, 129
    last = first + 80 * (nf - 1) + 199
    y = E.speechlike(last + 400, 7)
    for mutation in E.MUTATIONS:
        if mutation in ("mel_row_132", "drop_tap_199"):
            continue                              # bin 132 has no power and tap 199 a Hann weight of 2.5e-4 there: the probes carry these
        shown = max(np.abs(E.ref_logmel(y, length, first, nf, dft, melT, mutation) - E.ref_logmel(y, length, first, nf, dft, melT)).max()
                    for length in (last + 1, last - 57))
        print(f"production tables, {mutation}: {shown:.3e}")
        assert shown > 64 * G.BARS["logmel real abs"], mutation


def test_stft_lengths_hit_the_edges():
    for first in E.FIRSTS:
        for nf in E.N_FRAMES:
            lens = E.stft_lengths(first, nf)
            last = first + 80 * (nf - 1) + 199
            assert all(v >= 1 for v in lens) and (last < 0 or last + 1 in lens) and 1 in lens
            if last >= 1:
                assert last in lens
            b = (nf - 1) // 64
            if first + 5120 * b >= 0:
                assert first + 5120 * b + 1 in lens
    assert E.stft_grid(1) == (1, 64, 1) and E.stft_grid(64) == (1, 64, 4) and E.stft_grid(65) == (2, 64, 1) and E.stft_grid(129) == (3, 64, 1)
    # first = -200: frame 0 lies wholly before sample 0; -5240: every frame of a one-block launch; -5239: all but the last tap of frame 63
    one = np.ones(20000)
    assert (E.ref_melpower(one, 20000, -200, 1, *E.dense_tables()) == 0).all() and (E.ref_melpower(one, 20000, -199, 1, *E.dense_tables()) != 0).any()
    assert (E.ref_melpower(one, 20000, -5240, 64, *E.dense_tables()) == 0).all()
    p = E.ref_melpower(one, 20000, -5239, 64, *E.dense_tables())
    assert (p[:63] == 0).all() and (p[63] != 0).any()


# ---------------------------------------------------------------------------------------------------- normalisation, splice
@pytest.mark.parametrize("mode,name", [(1, "logmel23_mn"), (2, "logmel23_cummn")])
def test_ref_meannorm_equals_the_oracle(mode, name):
    g = np.random.default_rng(mode)
    Y = (g.standard_normal((777, 23)) + 5.0).astype(np.float32)
    Y64 = Y.astype(np.float64)
    got = E.ref_meannorm(Y, mode)
    want = Y64 - (Y64.mean(0) if mode == 1 else np.cumsum(Y64, 0) / np.arange(1, 778)[:, None])
    assert got.dtype == np.float32 and np.abs(got - want).max() < 1e-6
    # and the oracle's own transform: its mean, taken from its float64 output, subtracted from the float32 rows ref_meannorm is given
    S = R.stft(E.speechlike(8123, 5)).astype(np.complex128)                           # float64 in: the oracle then works in float64 throughout
    lm = R.transform(S, "logmel23", dtype=np.float64)
    mean = lm - R.transform(S, name, dtype=np.float64)
    lm32 = lm.astype(np.float32)
    err = np.abs(E.ref_meannorm(lm32, mode) - (lm32.astype(np.float64) - mean)).max()
    print(f"ref_meannorm mode {mode} vs oracle transform: {err:.3e}")
    assert err < 1e-6


@pytest.mark.parametrize("T", E.NORM_T)
def test_quantised_sums_do_not_depend_on_the_order(T):
    for F in E.NORM_F:
        Y = E.quantised(T, F, T + F)
        assert np.array_equal(Y * 1024, np.round(Y * 1024)) and np.abs(Y).max() <= 16
        seq = np.cumsum(Y.astype(np.float64), axis=0)[-1]
        assert np.array_equal(seq.view(np.int64), E.pairwise_sum(Y).view(np.int64))
        assert np.array_equal(seq.view(np.int64), np.cumsum(Y[::-1].astype(np.float64), axis=0)[-1].view(np.int64))
        if T > 1:                                                                       # the means matter: a dropped row shows
            assert np.abs(E.ref_meannorm(Y, 1) - E.ref_meannorm(np.vstack([Y[:-1], Y[:1]]), 1)).max() > 0 or np.array_equal(Y[-1], Y[0])


def test_ref_splice_equals_the_oracle():
    g = np.random.default_rng(0)
    for T, F, ctx, sub in E.SPLICE_CASES:
        Y = g.standard_normal((T, F)).astype(np.float32)
        assert np.array_equal(E.ref_splice(Y, ctx, sub), R.splice(Y, ctx)[::sub]), (T, F, ctx, sub)
    counts = {E.splice_grid(*c)[0] for c in E.SPLICE_CASES}
    assert {255, 256, 257, 511, 513} <= counts
    assert any(sub > T for T, F, ctx, sub in E.SPLICE_CASES) and any(ctx >= T for T, F, ctx, sub in E.SPLICE_CASES)


# ---------------------------------------------------------------------------------------------------- the planners
@pytest.mark.parametrize("ctx,sub", E.STREAM_PAIRS)
def test_feed_planner_tiles_the_walk_exactly_once(ctx, sub):
    """audio_stream.FrontEndTable / feed_words on the schedule of the GPU walk: ring length <= 32, STFT tiles <= 64 frames, splice tiles
    <= 16 rows, the tiles cover the new frames and rows exactly once, and the row counts are those of ref_stream's independent rule"""
    from fs_eend_amd.audio_stream import FrontEndTable, feed_words
    table = FrontEndTable(4, ctx, sub)
    for s in range(4):
        table.reset(s)
    cuts = {s: [[]] for s in range(4)}
    seen = dict(stft64=0, stft2=0, stft3=0, spl1=0, spl2=0, spl3=0, noframe=0, ring=0)
    for c, feed, end, reset in E.stream_schedule():
        for s in reset:
            table.reset(s)
            cuts[s].append([])
        plan = table.plan(feed, end)
        desc, stft, splice, rows, y_rows, o_rows = feed_words(plan, [0] * len(plan))
        assert [d[8] for d in desc] == sorted(set(feed) | set(end))
        for i, p in enumerate(plan):
            cuts[p.slot][-1].append((p.recv1 - p.recv0, p.ended))
            assert 0 <= p.f0 - p.rb0 <= E.RING and 0 <= p.f1 - p.rb1 <= E.RING and p.rb0 <= p.rb1
            seen["ring"] = max(seen["ring"], p.f1 - p.rb1)
            mine = [t for t in stft if t[0] == i]
            assert all(1 <= t[2] <= E.FB for t in mine)
            assert sorted(f for t in mine for f in range(t[1], t[1] + t[2])) == list(range(p.f0, p.f1))
            ours = [t for t in splice if t[0] == i]
            assert all(1 <= t[2] <= E.SPL_ROWS for t in ours)
            assert sorted(j for t in ours for j in range(t[1], t[1] + t[2])) == list(range(p.j0, p.j1))
            assert sorted(r for t in ours for r in range(t[3], t[3] + t[2])) == list(range(rows[p.slot][0], rows[p.slot][0] + rows[p.slot][1]))
            assert desc[i][7] + (p.f1 - p.rb0) <= y_rows
            k = p.f1 - p.f0
            seen["stft64"] += k == 64
            seen["stft2"] += k == 65
            seen["stft3"] += k == 129
            seen["noframe"] += k == 0 and p.recv1 > p.recv0
            if sub == 1:
                seen["spl1"] += p.j1 - p.j0 == 16
                seen["spl2"] += p.j1 - p.j0 == 17
                seen["spl3"] += p.j1 - p.j0 == 33
        assert sorted(r for o, k in rows.values() for r in range(o, o + k)) == list(range(o_rows))
        table.commit(plan)
    assert seen["stft64"] and seen["stft2"] and seen["stft3"] and seen["noframe"], seen
    assert sub != 1 or (seen["spl1"] and seen["spl2"] and seen["spl3"]), seen
    assert seen["ring"] == 2 * ctx                                                     # ctx = 15 fills 30 of the 32 ring rows
    for s, streams in cuts.items():
        for stream in streams:
            n = sum(m for m, _ in stream)
            _rows, counts = E.ref_stream(np.zeros(n), stream, ctx, sub, 0, None, logmel=np.zeros((E.stft_frames(n), 23), np.float32))
            assert sum(counts) == _rows.shape[0] and all(k >= 0 for k in counts)
            assert stream[-1][1] and not any(e for _, e in stream[:-1])
    assert sum(m for m, _ in cuts[3][0]) == 57 and cuts[0][0][-1] == (0, True) and cuts[2][0][-1] == (37, True)
    assert [m for m, _ in cuts[0][0][:300]] == [1] * 300


def test_chunk_planner_tiles_the_batch_exactly_once():
    from fs_eend_amd import device_data as DD
    lens, rows = E.CHUNK_LENS, E.CHUNK_ROWS
    total = sum(lens.values())
    off_of = dict(zip(lens, np.cumsum([0] + list(lens.values()))[:-1].tolist()))
    for sub in (1, 10, 16):
        cols = [[], [], [], [], [], []]
        for rec, st, ed in rows:
            a, length = DD.chunk_samples(lens[rec], st, ed)
            for cc, v in zip(cols, (off_of[rec] + a, length, st, ed, 0, 1)):
                cc.append(v)
        p = DD.plan_batch(*cols, sub)
        assert p["frames"].tolist() == list(E.CHUNK_FRAMES) == [int(E.stft_frames(n)) for n in cols[1]]
        assert {1, 63, 64, 65, 4097} <= set(E.CHUNK_FRAMES)
        assert any(n % 80 == 0 and o + n == total and (ed - st) * 80 == n for o, n, (_, st, ed) in zip(cols[0], cols[1], rows))   # ends at the corpus end
        assert any(n % 80 == 0 and (ed - st) * 80 > n for n, (_, st, ed) in zip(cols[1], rows))                                   # clipped to a multiple
        assert any(n % 80 for n in cols[1]) and 0 in cols[0]
        for b in range(len(rows)):
            mine = p["stft"][p["stft"][:, 0] == b]
            assert (mine[:, 2] >= 1).all() and (mine[:, 2] <= E.FB).all()
            assert sorted(f for t in mine for f in range(t[1], t[1] + t[2])) == list(range(p["frames"][b]))
            ours = p["splice"][p["splice"][:, 0] == b]
            assert (ours[:, 2] >= 1).all() and (ours[:, 2] <= E.SPL_ROWS).all()
            assert sorted(j for t in ours for j in range(t[1], t[1] + t[2])) == list(range(p["rows"][b]))
            assert sorted(r for t in ours for r in range(t[3], t[3] + t[2])) == list(range(p["obase"][b], p["obase"][b] + p["rows"][b]))
        assert p["y_rows"] == p["frames"].sum() and p["o_rows"] == p["rows"].sum()
        assert p["frames"].max() > E.SCAN                                              # the colnorm chunk goes into a second scan pass
    cover = E.chunk_cover()
    for rec, st, ed in rows:                                                           # poison on both sides of every chunk but at the corpus ends
        a, length = DD.chunk_samples(lens[rec], st, ed)
        a += off_of[rec]
        assert a == 0 or not cover[a - 1]
        assert a + length == total or not cover[a + length]


def test_chunk_segments_hit_every_branch_of_the_label_rule():
    from tests import chunk_label_ref as C
    for S in (1, 5, 64):
        segs = E.chunk_segments(S)
        for rec, (segments, utt2spk) in segs.items():
            assert len(C.speakers_of(segments, utt2spk)) == (S if rec == "A" else min(S, 3))
        segments, utt2spk = segs["A"]
        fr = {u: (C.segment_frames(st), C.segment_frames(et)) for u, st, et in segments}
        assert fr["u0"] == (66, 80) and fr["u1"] == (100, 130) and fr["u2"] == (50, 66) and fr["u3"] == (130, 140) and fr["u4"] == (0, 5000)
        T = C.chunk_labels(segments, utt2spk, E.CHUNK_LENS["A"], 66, 130, S)
        assert T.shape == (64, S) and T[:, S - 1].any() and T[0, 0] == 1
        if S > 2:
            assert T[:, 1].tolist() == [0] * 4 + [1] * 50 + [0] * 10                   # u6 and u7 overlap; u4 covers the chunk and is skipped
