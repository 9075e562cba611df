"""GPU: simulated mixtures on the device (fs_eend_amd/simulate.py, eend_sim_mix_f32) against the float64 restatement of the
contract (tests/simulate_ref.py), against themselves bit for bit where the contract says so, and end to end through
DeviceCorpus.batch.  Shapes are a few tiles at most (a tile is 2048 outputs, a tap slice 1024 steps of the product, which a
track of K taps crosses at K + 15 > 1024)."""
import numpy as np
import pytest
import torch

import chunk_label_ref as L
import simulate_ref as R

pytestmark = pytest.mark.gpu

TILE, SLICE = 2048, 1024
U24 = 2.0 ** -24


def mix_call(dev, mixes, utt_storage="f32", noise_storage="f32", storage="f32"):
    """Run one simulate() over `mixes` given as arrays: [{"N", "tracks": [{"gain", "rir" (array or None), "placements": [(wave,
    start)]}], "noise" (array or None), "noise_offset", "snr_db"}].  -> (corpus, stats, [y of each mixture], [out of each mixture])
    as numpy."""
    from fs_eend_amd import simulate as S
    utts, rirs, noises = S.SourcePool(dev, utt_storage), S.SourcePool(dev), S.SourcePool(dev, noise_storage)
    recipes = []
    for mi, m in enumerate(mixes):
        tracks = []
        for si, t in enumerate(m["tracks"]):
            pl = []
            for pi, (w, start) in enumerate(t["placements"]):
                utts.add(f"u{mi}_{si}_{pi}", w)
                pl.append((f"u{mi}_{si}_{pi}", start))
            rn = None
            if t.get("rir") is not None:
                rn = f"h{mi}_{si}"
                rirs.add(rn, t["rir"])
            tracks.append({"speaker": t.get("speaker", f"spk{si}"), "rir": rn, "gain": t["gain"], "placements": pl})
        nn = None
        if m.get("noise") is not None:
            nn = f"n{mi}"
            noises.add(nn, m["noise"])
        recipes.append({"name": f"m{mi}", "length": m["N"], "tracks": tracks, "noise": nn, "noise_offset": m.get("noise_offset", 0),
                        "snr_db": m.get("snr_db")})
    for p in (utts, rirs, noises):
        p.finalize()
    corpus, stats = S.simulate(utts, rirs, noises, recipes, storage)
    torch.cuda.synchronize()
    edges = np.cumsum([0] + [m["N"] for m in mixes])
    y, out = stats["y"].cpu().numpy(), corpus.samples.cpu().numpy()
    return (corpus, {k: v.cpu().numpy() for k, v in stats.items()}, [y[a:b] for a, b in zip(edges[:-1], edges[1:])],
            [out[a:b] for a, b in zip(edges[:-1], edges[1:])])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def rnd(rng, n, s16=False):
    if s16:
        return rng.integers(-20000, 20000, n).astype(np.int16)
    return (rng.standard_normal(n) * 0.1).astype(np.float32)


def rir_of(rng, K):
    return (rng.standard_normal(K) * np.exp(-np.arange(K) / max(K / 4, 1.0))).astype(np.float32)


def edge_mixture(rng, N, K, s16=False):
    """Three tracks.  One with a response of K taps and an utterance starting at sample 0, one shorter than 16 samples, one
    straddling the tile edge and one ending at N - 1 (as far as N allows); one without a response whose utterance is clipped by
    N; one with a response and no placement."""
    pl = [(rnd(rng, min(50, N), s16), 0)]
    if N >= 120:
        pl.append((rnd(rng, 10, s16), 100))
    if N >= TILE + 500:
        pl.append((rnd(rng, 100, s16), TILE - 40))
    if N >= 700:
        pl.append((rnd(rng, 300, s16), N - 300))
    return {"N": N, "tracks": [{"gain": 0.8, "rir": rir_of(rng, K), "placements": pl},
                               {"gain": 1.25, "rir": None, "placements": [(rnd(rng, 200, s16), max(N - 100, 0))]},
                               {"gain": 1.0, "rir": rir_of(rng, 7), "placements": []}]}


def check_bound(mixes, ys, what):
    """Every output against float64: |y - ref| <= (n + 1) 2^-24 sum |a d|, n = sum_s (K_s + 15): the worst case of any float32
    accumulation of that many terms.  -> the worst observed fraction of the bound."""
    worst = 0.0
    for i, (m, y) in enumerate(zip(mixes, ys)):
        ref, mag, n = R.wet_mix(m["N"], m["tracks"])
        assert y.shape == ref.shape and np.isfinite(y).all()
        bound = (n + 1) * U24 * mag
        err = np.abs(y.astype(np.float64) - ref)
        bad = np.nonzero(err > bound)[0]
        assert bad.size == 0, (what, i, m["N"], bad[:8].tolist(), err[bad[:8]].tolist(), bound[bad[:8]].tolist())
        assert np.array_equal(y[mag == 0], np.zeros(int((mag == 0).sum()), dtype=np.float32))
        nz = bound > 0
        if nz.any():
            worst = max(worst, float((err[nz] / bound[nz]).max()))
    print(f"{what}: worst |y - ref| / bound = {worst:.3e}")
    return worst


KS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 33, SLICE - 16, SLICE - 15, SLICE - 14, SLICE - 1, SLICE, SLICE + 1]
NS = [1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 3]


@pytest.mark.parametrize("s16", [False, True])
def test_rounding_bound_over_tap_counts(hip_lib, dev, s16):
    """K around the MFMA step (4), the block row (16) and the tap slice (K + 15 = 1024 and K = 1024, each +- 1) at N = 2 tiles + 3,
    and K = 8192 at N = 300: f32 and s16 sources, responses and none mixed, a track with no placement."""
    rng = np.random.default_rng(10 + s16)
    mixes = [edge_mixture(rng, 2 * TILE + 3, K, s16) for K in KS] + [edge_mixture(rng, 300, 8192, s16)]
    _, _, ys, outs = mix_call(dev, mixes, utt_storage="s16" if s16 else "f32")
    assert check_bound(mixes, ys, f"K sweep, s16={s16}") > 0
    assert all(np.array_equal(bits(y), bits(o)) for y, o in zip(ys, outs))             # no noise: the call returns y itself


def test_rounding_bound_over_lengths_and_track_counts(hip_lib, dev):
    rng = np.random.default_rng(12)
    mixes = [edge_mixture(rng, N, 33) for N in NS] + [edge_mixture(rng, N, 1) for N in NS]
    for S_ in (1, 2, 5):
        mixes.append({"N": 600, "tracks": [{"gain": 0.5 + 0.1 * s, "rir": rir_of(rng, 20 + 13 * s) if s % 2 == 0 else None,
                                            "placements": [(rnd(rng, 150), 40 * s), (rnd(rng, 9), 300 + 50 * s)]} for s in range(S_)]})
    _, _, ys, _ = mix_call(dev, mixes)
    assert check_bound(mixes, ys, "N sweep") > 0


def test_identity_and_pure_delays_are_exact(hip_lib, dev):
    """h = [1], g = 1 gives the dry track itself; h = e_d the dry track d samples later: every product is the sample or zero."""
    rng = np.random.default_rng(13)
    N = TILE + 300
    for s16 in (False, True):
        pl = [(rnd(rng, 500, s16), 0), (rnd(rng, 11, s16), 700), (rnd(rng, 400, s16), TILE - 200), (rnd(rng, 100, s16), N - 50)]
        dry = R.dry_track(N, pl).astype(np.float32)
        mixes = [{"N": N, "tracks": [{"gain": 1.0, "rir": np.ones(1, dtype=np.float32), "placements": pl}]},
                 {"N": N, "tracks": [{"gain": 1.0, "rir": None, "placements": pl}]}]
        delays = [1, 15, 16, 17, 100]
        for d in delays:
            h = np.zeros(d + 1, dtype=np.float32)
            h[d] = 1.0
            mixes.append({"N": N, "tracks": [{"gain": 1.0, "rir": h, "placements": pl}]})
        _, _, ys, _ = mix_call(dev, mixes, utt_storage="s16" if s16 else "f32")
        assert np.abs(dry).max() > 0
        assert np.array_equal(bits(ys[0]), bits(dry)) and np.array_equal(bits(ys[1]), bits(dry))
        for d, y in zip(delays, ys[2:]):
            assert np.array_equal(bits(y), bits(np.concatenate([np.zeros(d, dtype=np.float32), dry[:N - d]]))), d


def noisy_mixture(rng, N, K=100, L=333, snr=15.0, offset=77):
    m = edge_mixture(rng, N, K)
    m.update(noise=rnd(rng, L), noise_offset=offset, snr_db=snr)
    return m


def test_alone_equals_among_others(hip_lib, dev):
    rng = np.random.default_rng(14)
    m = noisy_mixture(rng, 2 * TILE + 3, K=SLICE + 77)
    others = [noisy_mixture(rng, N, K) for N, K in ((1, 3), (17, 40), (TILE, 300), (TILE + 1, 5), (3 * TILE - 1, 2000), (900, 16))]
    others.append(edge_mixture(rng, 5000, 64))
    _, sa, ya, oa = mix_call(dev, [m])
    _, sb, yb, ob = mix_call(dev, others[:3] + [m] + others[3:])
    assert len(others) == 7 and np.abs(ya[0]).max() > 0 and sa["scale"][0] > 0
    assert np.array_equal(bits(ya[0]), bits(yb[3])) and np.array_equal(bits(oa[0]), bits(ob[3]))
    assert (sa["Ps"][0], sa["Pn"][0], sa["scale"][0]) == (sb["Ps"][3], sb["Pn"][3], sb["scale"][3])


@pytest.mark.parametrize("shift", [1, TILE])
def test_shifting_the_placements_shifts_the_output(hip_lib, dev, shift):
    """The same sources `shift` samples later, compared at the shifted position: other tiles, other lanes, other slices of the
    staged span, the same bits."""
    rng = np.random.default_rng(15)
    N = TILE + 700
    tracks = [{"gain": 0.9, "rir": rir_of(rng, SLICE + 300), "placements": [(rnd(rng, 300), 0), (rnd(rng, 12), 900), (rnd(rng, 500), N - 500)]},
              {"gain": 1.1, "rir": None, "placements": [(rnd(rng, 100), TILE - 50)]},
              {"gain": 0.7, "rir": rir_of(rng, 5), "placements": [(rnd(rng, 64), 17)]}]
    moved = [dict(t, placements=[(w, s + shift) for w, s in t["placements"]]) for t in tracks]
    _, _, ys, _ = mix_call(dev, [{"N": N, "tracks": tracks}, {"N": N + shift, "tracks": moved}])
    assert np.abs(ys[0]).max() > 0 and not ys[1][:shift].any()
    assert np.array_equal(bits(ys[0]), bits(ys[1][shift:]))


def test_noise_powers_and_scale(hip_lib, dev):
    rng = np.random.default_rng(16)
    mixes = [noisy_mixture(rng, 2 * TILE + 3, snr=10.0), noisy_mixture(rng, 600, L=7, snr=20.0, offset=7 * 9 + 4),
             noisy_mixture(rng, TILE, L=5000, snr=-5.0, offset=4999), dict(noisy_mixture(rng, 500), snr_db=None),
             dict(noisy_mixture(rng, 500), noise=np.zeros(50, dtype=np.float32)),                  # silent noise
             {"N": 400, "tracks": [{"gain": 1.0, "rir": None, "placements": []}], "noise": rnd(rng, 90), "snr_db": 10.0}]   # silent speech
    _, st, ys, outs = mix_call(dev, mixes)
    for i, (m, y, out) in enumerate(zip(mixes, ys, outs)):
        N = m["N"]
        Ps = float(np.sum(y.astype(np.float64) ** 2))
        assert abs(st["Ps"][i] - Ps) <= N * 2.0 ** -52 * Ps, i
        if i == 3:                                          # snr_db None: the noise is not read
            assert st["Pn"][i] == 0 and st["scale"][i] == 0 and np.array_equal(bits(out), bits(y))
            continue
        noise = R.noise_at(m["noise"], m.get("noise_offset", 0), N)
        Pn = float(np.sum(noise ** 2))
        assert abs(st["Pn"][i] - Pn) <= N * 2.0 ** -52 * Pn, i
        if i >= 4:
            assert st["scale"][i] == 0 and np.array_equal(bits(out), bits(y)), i
            continue
        want = np.float32(np.sqrt(R.snr_constant(m["snr_db"]) * st["Ps"][i] / st["Pn"][i]))
        assert st["scale"][i] > 0 and abs(float(st["scale"][i]) - float(want)) <= float(np.spacing(want)), i
        # the noise that was added has the requested SNR (scale is a float32: 2^-23 in power, and out is rounded to float32)
        added = out.astype(np.float64) - y
        assert abs(10 * np.log10(Ps / np.sum(added ** 2)) - m["snr_db"]) < 1e-3, i
    assert st["clipped"].tolist() == [0] * len(mixes)


def test_noise_add_is_one_fused_multiply_add(hip_lib, dev):
    """out = fmaf(scale, noise, y) exactly.  y is made exact (no response, gain 1: the dry track itself) and y and the noise are
    multiples of 2^-10 below 1 in magnitude; with scale a float32 of at least 2^-16 the product has its last bit at 2^-50 or
    above and the sum stays below 2, so the float64 sum of the (exact) float64 product and y is exact, and its one rounding to
    float32 is the fused result.  A noise of 7 samples with an offset that wraps it several times, and a long one."""
    rng = np.random.default_rng(17)
    grid = lambda n: (rng.integers(-1023, 1024, n) / 1024.0).astype(np.float32)
    mixes = []
    for N, L, o, snr in ((TILE + 50, 7, 7 * 5 + 3, 10.0), (700, 1000, 650, 3.0), (50, 7, 6, 20.0)):
        mixes.append({"N": N, "tracks": [{"gain": 1.0, "rir": None, "placements": [(grid(N - 10), 5)]}], "noise": grid(L), "noise_offset": o,
                      "snr_db": snr})
    _, st, ys, outs = mix_call(dev, mixes)
    for i, (m, y, out) in enumerate(zip(mixes, ys, outs)):
        assert np.array_equal(bits(y), bits(R.dry_track(m["N"], m["tracks"][0]["placements"]).astype(np.float32)))
        noise = R.noise_at(m["noise"], m["noise_offset"], m["N"])
        assert 2.0 ** -16 <= st["scale"][i] < 1.0
        want = R.add_noise(y, noise, st["scale"][i])
        assert np.array_equal(bits(out), bits(want)), i
        assert not np.array_equal(out, y)


def test_s16_storage(hip_lib, dev):
    """Half to even at +-0.5 LSB and saturation at both ends on exact values (no response, gain 1, no noise), then a noisy
    reverberant mixture loud enough to clamp: the s16 call stores what the f32 call returns, rounded."""
    lsb = 2.0 ** -15
    v = np.array([0.5 * lsb, 1.5 * lsb, 2.5 * lsb, -0.5 * lsb, -1.5 * lsb, -2.5 * lsb, 0.49 * lsb, 1.0, -1.0, 1.0 - 0.5 * lsb, 1.0 - 0.75 * lsb,
                  -1.0 - 0.5 * lsb, -1.0 - lsb, 3.0, -3.0, 0.0], dtype=np.float32)
    exact = {"N": 20, "tracks": [{"gain": 1.0, "rir": None, "placements": [(v, 2)]}]}
    rng = np.random.default_rng(18)
    loud = noisy_mixture(rng, TILE + 99, K=50, snr=5.0)
    for t in loud["tracks"]:
        t["gain"] *= 6.0
    _, _, _, of = mix_call(dev, [exact, loud], storage="f32")
    _, st, _, os_ = mix_call(dev, [exact, loud], storage="s16")
    assert os_[0].dtype == np.int16
    assert os_[0].tolist() == [0, 0, 0, 2, 2, 0, -2, -2, 0, 32767, -32768, 32767, 32767, -32768, -32768, 32767, -32768, 0, 0, 0]
    assert st["clipped"][0] == 5                             # 1.0, 1 - LSB / 2 (rounds to 32768), -1 - LSB, 3, -3
    for i in range(2):
        want, clipped = R.store_s16(of[i])
        assert np.array_equal(os_[i], want) and st["clipped"][i] == clipped, i
    assert st["clipped"][1] > 0 and (os_[1] == 32767).any() and (os_[1] == -32768).any()


@pytest.mark.parametrize("storage", ["f32", "s16"])
def test_end_to_end_batches(hip_lib, dev, storage):
    """draw_recipes -> simulate -> corpus.batch: the features are the single-waveform path on the downloaded slice bit for bit,
    the labels the reference's rule on the recipe's segments, and a corpus built by add() from the downloaded waves gives the
    same batch."""
    from fs_eend_amd import device_data as DD, feature, simulate as S
    rng = np.random.default_rng(19)
    utts, rirs, noises = S.SourcePool(dev, "s16"), S.SourcePool(dev), S.SourcePool(dev, "f32")
    spk2utt = {}
    for s in range(4):
        for i in range(3):
            utts.add(f"s{s}_u{i}", rnd(rng, int(rng.integers(1500, 5000)), s16=True))
            spk2utt.setdefault(f"s{s}", []).append(f"s{s}_u{i}")
    for i in range(3):
        rirs.add(f"h{i}", rir_of(rng, 400 + 300 * i))
    noises.add("n0", rnd(rng, 3001))
    for p in (utts, rirs, noises):
        p.finalize()
    recipes = S.draw_recipes(5, spk2utt, utts, rirs, noises, n_mixtures=3, n_speakers=(2, 3), n_utts=(1, 3), beta=0.2)
    corpus, stats = S.simulate(utts, rirs, noises, recipes, storage=storage)
    assert isinstance(corpus, DD.DeviceCorpus) and corpus.storage == storage and corpus.samples is not None
    assert [r for r, _ in corpus.recordings()] == [r["name"] for r in recipes]
    assert (stats["scale"] > 0).all() and stats["Ps"].dtype == torch.float64 and stats["clipped"].dtype == torch.int32
    p = S.plan(recipes, utts, rirs, noises)
    rows, waves = [], {}
    for r, off in zip(recipes, p["offsets"].tolist()):
        n = r["length"]
        waves[r["name"]] = corpus.samples[off:off + n].cpu()
        frames = n // 80
        rows += [(r["name"], 0, min(frames, 120)), (r["name"], frames // 3, frames // 3 + 57), (r["name"], max(frames - 30, 0), frames + 5)]
    feats, labels, recs = corpus.batch(rows, context_size=7, subsampling=10, input_transform="logmel23_mn")
    feats, labels = [f.clone() for f in feats], [l.clone() for l in labels]
    assert recs == [r[0] for r in rows]
    segs = dict(zip(p["names"], zip(p["segments"], p["utt2spk"])))
    active = 0.0
    for (rec, st, ed), f, l in zip(rows, feats, labels):
        w = waves[rec].float() / 32768 if storage == "s16" else waves[rec]
        ref = feature.extract_fbank_wave(w[st * 80:ed * 80].to(dev), 7, 200, 80, "logmel23_mn", 10)
        assert torch.equal(f, ref), (rec, st, ed)
        T = L.chunk_labels(segs[rec][0], segs[rec][1], len(w), st, ed)
        assert np.array_equal(l.cpu().numpy(), L.subsampled(T, 10)), (rec, st, ed)
        active += float(l.sum())
    assert active > 0
    again = DD.DeviceCorpus(dev, storage=storage)
    for name in p["names"]:
        again.add(name, waves[name], *segs[name])
    f2, l2, _ = again.finalize().batch(rows, context_size=7, subsampling=10, input_transform="logmel23_mn")
    assert all(torch.equal(a, b) for a, b in zip(feats, f2)) and all(torch.equal(a, b) for a, b in zip(labels, l2))
