"""CPU: the float64 restatement of simulated mixtures (tests/simulate_ref.py) against scipy and against its own contract, the
recipe generator (fs_eend_amd/simulate.py `draw_recipes`), and the segment rows of a simulated mixture against those
DeviceCorpus.add computes from the same seconds.  No device."""
import numpy as np
import pytest
from scipy.signal import fftconvolve

import simulate_ref as R
from fs_eend_amd import device_data as DD
from fs_eend_amd import simulate as S


def _case(seed=0, N=3000):
    rng = np.random.default_rng(seed)
    u = [rng.standard_normal(n).astype(np.float32) * 0.1 for n in (700, 40, 1200)]
    s = (rng.integers(-20000, 20000, 900)).astype(np.int16)
    h = [rng.standard_normal(k).astype(np.float32) * np.exp(-np.arange(k) / (k / 4)).astype(np.float32) for k in (257, 1000)]
    tracks = [{"gain": 0.7, "rir": h[0], "placements": [(u[0], 0), (u[1], 900), (s, 2500)]},       # the last one is clipped at N
              {"gain": 1.3, "rir": h[1], "placements": [(u[2], 1500)]},
              {"gain": 0.5, "rir": None, "placements": [(u[1], N - 40)]}]                         # ends at N - 1
    return N, tracks


def test_wet_mix_agrees_with_fftconvolve():
    """Both sides are float64.  The direct sum of K terms is off by at most K 2^-53 sum |a d| <= K 2^-53 |a|_2 |d|_2 per output;
    an FFT convolution of length n (two forward transforms, a product, one inverse) is off by c 2^-53 log2(n) |a|_2 |d|_2 with
    a constant of a few units per transform (Higham, Accuracy and Stability, 24.2: eta log2 n per transform, eta the error of a
    butterfly), taken as 4 for each of the three.  The margin is their sum."""
    N, tracks = _case()
    y, mag, n = R.wet_mix(N, tracks)
    assert n == 257 + 1000 + 1 + 45 and y.shape == mag.shape == (N,) and (mag >= np.abs(y)).all()
    want, margin = np.zeros(N), 0.0
    for t in tracks:
        a, d = R.taps(t["gain"], t["rir"]).astype(np.float64), R.dry_track(N, t["placements"])
        full = fftconvolve(d, a)
        want += full[:N]
        margin += (len(a) + 12 * np.log2(len(full))) * 2.0 ** -53 * np.linalg.norm(a) * np.linalg.norm(d)
    worst = np.abs(y - want).max()
    print(f"worst |direct - fft| = {worst:.3e}, margin {margin:.3e}")
    assert 0 < margin < 1e-9 * np.abs(y).max() and worst <= margin          # the margin is far below the signal: not vacuous


def test_clipping_at_the_end_and_the_dropped_tail():
    N = 100
    w = np.arange(1, 61, dtype=np.float32)
    d = R.dry_track(N, [(w, 70)])                           # 60 samples from 70 on: 30 of them fit
    assert d[:70].tolist() == [0.0] * 70 and d[70:].tolist() == w[:30].tolist()
    h = np.zeros(50, dtype=np.float32)
    h[49] = 1.0                                             # a delay of 49: the utterance's first sample lands on 119 > N - 1
    y, _, _ = R.wet_mix(N, [{"gain": 1.0, "rir": h, "placements": [(w, 70)]}])
    assert y.shape == (N,) and not y.any()
    y, _, _ = R.wet_mix(N, [{"gain": 1.0, "rir": h, "placements": [(w, 40)]}])
    assert y[:89].tolist() == [0.0] * 89 and y[89:].tolist() == w[:11].tolist()
    # int16 sources decode as v / 32768, and taps are one float32 product
    assert R.dry_track(3, [(np.array([-32768, 16384, 1], dtype=np.int16), 0)]).tolist() == [-1.0, 0.5, 2.0 ** -15]
    a = R.taps(0.1, np.array([0.3, 1.0], dtype=np.float32))
    assert a.dtype == np.float32 and a.tolist() == [float(np.float32(0.1) * np.float32(0.3)), float(np.float32(0.1))]
    assert R.taps(0.1, None).tolist() == [float(np.float32(0.1))]
    with pytest.raises(AssertionError):
        R.dry_track(N, [(w, 0), (w, 59)])


def test_noise_wraps_modulo_its_length():
    noise = np.arange(7, dtype=np.float32)
    assert R.noise_at(noise, 5, 10).tolist() == [5, 6, 0, 1, 2, 3, 4, 5, 6, 0]
    assert R.noise_at(noise, 7 * 1000 + 3, 4).tolist() == [3, 4, 5, 6]
    assert R.noise_at(np.array([16384], dtype=np.int16), 9, 3).tolist() == [0.5] * 3


def test_scale_is_zero_without_noise_power_or_speech():
    y = np.array([0.5, -0.25, 0.0], dtype=np.float32)
    n = np.array([0.1, 0.2, -0.3], dtype=np.float32)
    assert R.noise_scale(y, n, 10.0)[2] > 0
    assert R.noise_scale(y, np.zeros(3, dtype=np.float32), 10.0) == (0.3125, 0.0, 0.0)         # silent noise
    assert R.noise_scale(np.zeros(3, dtype=np.float32), n, 10.0)[::2] == (0.0, 0.0)              # silent speech
    assert R.noise_scale(y, None, 10.0) == (0.3125, 0.0, 0.0) and R.noise_scale(y, n, None)[2] == 0.0
    assert R.add_noise(y, n, 0.0).tolist() == y.tolist()


@pytest.mark.parametrize("snr_db", [0.0, 10.0, 15.0, 20.0, -5.0])
def test_the_added_noise_has_the_requested_snr(snr_db):
    """scale is a float32: its relative error of 2^-24 moves the power ratio by 2^-23, 5.2e-7 dB."""
    N, tracks = _case(1)
    y = R.wet_mix(N, tracks)[0].astype(np.float32)
    noise = R.noise_at(np.random.default_rng(2).standard_normal(333).astype(np.float32), 1000, N)
    Ps, Pn, scale = R.noise_scale(y, noise, snr_db)
    assert scale.dtype == np.float32
    added = np.float64(scale) * noise                       # out - y before out is rounded
    got = 10 * np.log10(Ps / np.sum(added ** 2))
    assert abs(got - snr_db) <= 1e-6
    out = R.add_noise(y, noise, scale)
    assert out.dtype == np.float32 and np.abs(out.astype(np.float64) - (y + added)).max() <= 2.0 ** -24 * np.abs(out).max()


def test_s16_storage_rounds_half_to_even_and_counts_the_clamped():
    lsb = 2.0 ** -15
    v = np.array([0.5 * lsb, 1.5 * lsb, 2.5 * lsb, -0.5 * lsb, -1.5 * lsb, 1.0, -1.0, 1.0 - 0.5 * lsb, 1.0 - 0.75 * lsb, -1.0 - 0.5 * lsb,
                  -1.0 - lsb, 3.0], dtype=np.float32)
    s, clipped = R.store_s16(v)
    assert s.tolist() == [0, 2, 2, 0, -2, 32767, -32768, 32767, 32767, -32768, -32768, 32767] and clipped == 4


UTTS = {f"s{s}_u{i}": (1000 * (3 * s + i), 400 + 150 * i + 37 * s) for s in range(5) for i in range(3)}
SPK2UTT = {f"s{s}": [f"s{s}_u{i}" for i in range(3)] for s in range(5)}
RIRS = {f"h{i}": (100 * i, 100) for i in range(4)}
NOISES = {"n0": (0, 7), "n1": (7, 5000)}


def test_draw_recipes_is_deterministic_in_the_seed():
    a = S.draw_recipes(7, SPK2UTT, UTTS, RIRS, NOISES, n_mixtures=6)
    assert a == S.draw_recipes(7, SPK2UTT, UTTS, RIRS, NOISES, n_mixtures=6)
    assert a != S.draw_recipes(8, SPK2UTT, UTTS, RIRS, NOISES, n_mixtures=6)
    assert len(a) == 6 and len({r["name"] for r in a}) == 6
    dry = S.draw_recipes(7, SPK2UTT, UTTS, n_mixtures=2)
    assert all(r["noise"] is None and r["snr_db"] is None and all(t["rir"] is None for t in r["tracks"]) for r in dry)
    with pytest.raises(ValueError):
        S.draw_recipes(7, SPK2UTT, UTTS, n_speakers=(1, 6))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_drawn_placements_are_sorted_disjoint_and_inside(seed):
    recipes = S.draw_recipes(seed, SPK2UTT, UTTS, RIRS, NOISES, n_mixtures=20, n_speakers=(1, 4), n_utts=(1, 4), beta=0.05)
    silences = []
    for r in recipes:
        assert 1 <= len(r["tracks"]) <= 4 and len({t["speaker"] for t in r["tracks"]}) == len(r["tracks"])
        ends = []
        for t in r["tracks"]:
            assert 1 <= len(t["placements"]) <= 4 and t["rir"] in RIRS and 10 ** (-3 / 20) <= t["gain"] <= 10 ** (3 / 20)
            end = 0
            for utt, start in t["placements"]:
                assert utt in SPK2UTT[t["speaker"]] and start >= end
                silences.append(start - end)
                end = start + UTTS[utt][1]
                assert end <= r["length"]
            ends.append(end)
        assert r["length"] == max(ends)
        assert r["noise"] in NOISES and 0 <= r["noise_offset"] < NOISES[r["noise"]][1] and r["snr_db"] in (10.0, 15.0, 20.0)
    S.plan(recipes, UTTS, RIRS, NOISES)                     # and the planner takes them
    assert 0.5 * 400 < np.mean(silences) < 1.5 * 400        # an exponential with mean 0.05 s is 400 samples


def test_segment_rows_are_those_of_device_corpus_add():
    recipes = S.draw_recipes(3, SPK2UTT, UTTS, RIRS, NOISES, n_mixtures=5, beta=0.3)
    recipes[0]["length"] -= 55                              # the longest track is clipped
    p = S.plan(recipes, UTTS, RIRS, NOISES)
    lengths = {u: n for u, (_, n) in UTTS.items()}
    c = DD.DeviceCorpus("cuda:0")                           # add() does not touch the device
    want_rows, seen = [], 0
    for r, segs, u2s in zip(recipes, p["segments"], p["utt2spk"]):
        ref_segs, ref_u2s = R.segments(r["name"], r["length"], r["tracks"], lengths)
        assert segs == ref_segs and u2s == ref_u2s
        assert all(0 <= st <= et <= r["length"] / 8000 for _, st, et in segs)
        c.add(r["name"], np.zeros(r["length"], dtype=np.float32), segs, u2s)
        spk, rows = R.segment_rows(segs, u2s)
        assert c.speakers[r["name"]] == spk == sorted({t["speaker"] for t in r["tracks"]})
        want_rows += rows
        seen += len(segs)
        assert c._seg[r["name"]] == (seen - len(segs), seen)
    assert c._segrows == want_rows and seen > 10
    clipped_end = max(et for _, _, et in p["segments"][0])
    assert clipped_end == recipes[0]["length"] / 8000
