"""Float64 numpy restatement of the arithmetic contract of simulated mixtures (include/eend_hip.h at eend_sim_mix_f32, DESIGN
10d), independent of fs_eend_amd/simulate.py: it works on plain arrays.  A track is a dict {"gain", "rir" (1-D float array or
None), "placements": [(wave, start)]} with `wave` float (already decoded: int16 / 32768); a mixture is (N, [track])."""
import numpy as np

RATE = 8000


def decode(wave):
    """Source samples as the device decodes them: int16 / 32768, floats as they are (float32)."""
    w = np.asarray(wave)
    return w.astype(np.float64) / 32768.0 if w.dtype == np.int16 else w.astype(np.float32).astype(np.float64)


def dry_track(N, placements):
    """d[t], 0 <= t < N: the utterance sample where a placement covers t, 0 elsewhere; an utterance past N is clipped."""
    d = np.zeros(N, dtype=np.float64)
    end = 0
    for wave, start in placements:
        assert start >= end, "placements are sorted by start and disjoint"
        w = decode(wave)
        end = start + len(w)
        n = min(end, N) - start
        if n > 0:
            d[start:start + n] = w[:n]
    return d


def taps(gain, rir):
    """a[k] = f32(g h[k]), one float32 multiply; without a response a = [f32(g)]."""
    g = np.float32(gain)
    if rir is None:
        return np.array([g], dtype=np.float32)
    return (g * np.asarray(rir).astype(np.float32)).astype(np.float32)


def wet_mix(N, tracks):
    """-> (y, mag, n): y[t] = sum_s sum_k a_s[k] d_s[t - k] in float64 with the tail past N dropped, mag[t] the same sum of
    absolute values, n = sum_s (K_s + 15) the terms an accumulator of the device sees at most."""
    y, mag, n = np.zeros(N), np.zeros(N), 0
    for t in tracks:
        a = taps(t["gain"], t.get("rir")).astype(np.float64)
        d = dry_track(N, t["placements"])
        y += np.convolve(d, a)[:N]
        mag += np.convolve(np.abs(d), np.abs(a))[:N]
        n += len(a) + 15
    return y, mag, n


def noise_at(noise, offset, N):
    """n[(o + t) mod L] for t < N, decoded."""
    w = decode(noise)
    return w[(offset + np.arange(N)) % len(w)]


def snr_constant(snr_db):
    return 10.0 ** (-float(snr_db) / 10.0)


def noise_scale(y, noise, snr_db):
    """(Ps, Pn, scale): float64 powers of y and of the aligned noise (an array of len(y), or None); scale =
    f32(sqrt(c Ps / Pn)), 0 without noise or when either power is 0."""
    Ps = float(np.sum(np.asarray(y, dtype=np.float64) ** 2))
    if noise is None or snr_db is None:
        return Ps, 0.0, np.float32(0.0)
    Pn = float(np.sum(np.asarray(noise, dtype=np.float64) ** 2))
    if Ps == 0.0 or Pn == 0.0:
        return Ps, Pn, np.float32(0.0)
    return Ps, Pn, np.float32(np.sqrt(snr_constant(snr_db) * Ps / Pn))


def add_noise(y, noise, scale):
    """out[t] = fmaf(scale, n[t], y[t]) for float32 y, n and scale: the product of two float32 is exact in float64, so one
    float64 sum rounded to float32 is the fused result whenever that sum is exact in float64 (double rounding aside)."""
    y32, n32 = np.asarray(y, dtype=np.float32), np.asarray(noise, dtype=np.float32)
    return (np.float64(np.float32(scale)) * n32.astype(np.float64) + y32.astype(np.float64)).astype(np.float32)


def store_s16(out):
    """(int16 samples, clamped count): rint(out 32768), half to even, clamped to [-32768, 32767]."""
    r = np.rint(np.asarray(out, dtype=np.float32).astype(np.float64) * 32768.0)
    clipped = int(np.sum((r > 32767) | (r < -32768)))
    return np.clip(r, -32768, 32767).astype(np.int16), clipped


def segments(name, N, tracks, lengths):
    """One (utt, st_seconds, et_seconds) per placement and {utt: speaker}: tracks [{"speaker", "placements": [(utterance
    name, start)]}], lengths {utterance name: samples}."""
    segs, utt2spk = [], {}
    for si, t in enumerate(tracks):
        for pi, (utt, start) in enumerate(t["placements"]):
            seg = f"{name}_{si}_{pi}"
            segs.append((seg, start / RATE, min(start + lengths[utt], N) / RATE))
            utt2spk[seg] = t["speaker"]
    return segs, utt2spk


def segment_rows(segs, utt2spk, rate=RATE, frame_shift=80):
    """(speakers as np.unique orders them, [(start frame, end frame, speaker index)]) by the rint(. rate / frame_shift) rule."""
    spk = np.unique([utt2spk[u] for u, _, _ in segs]).tolist()
    return spk, [(int(np.rint(st * rate / frame_shift)), int(np.rint(et * rate / frame_shift)), spk.index(utt2spk[u])) for u, st, et in segs]
