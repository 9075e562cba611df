"""The arithmetic of the audio ingest (fs-eend_amd/audio_ingest.py, csrc/resample.hip) restated in float64 numpy: rate
conversion to 8000 Hz with a Kaiser-windowed sinc, the counters, and the G.711 expansions.  No package import.

    g = gcd(rate, 8000), L = 8000 / g, M = rate / g, H = Z M, P = 2 H // L + 1       (L == M == 1: H = 0, h = [1])
    h[i] = L (rho / M) sinc(rho i / M) kaiser(2 H + 1, beta)[i + H], i = -H .. H, rescaled so that sum(h) == L
    y[n] = sum over k = ceil((n M - H) / L) .. floor((n M + H) / L) of h[n M - k L] x[k], x zero outside [0, n_in)
"""
import math

import numpy as np

RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000]
ENCODINGS = ["f32", "s16", "mulaw", "alaw"]
Z, BETA, RHO = 16, 9.0, 0.9


def cdiv(a, b):
    return -((-a) // b)


def params(rate, zeros=Z):
    """-> L, M, H, P"""
    g = math.gcd(rate, 8000)
    L, M = 8000 // g, rate // g
    if L == M:
        return 1, 1, 0, 1
    H = zeros * M
    return L, M, H, 2 * H // L + 1


def prototype(rate, zeros=Z, beta=BETA, rho=RHO):
    """float64 h[-H .. H] as an array of 2 H + 1 (h[i] at index i + H)."""
    L, M, H, _ = params(rate, zeros)
    if H == 0:
        return np.ones(1)
    i = np.arange(-H, H + 1, dtype=np.float64)
    h = L * (rho / M) * np.sinc(rho * i / M) * np.kaiser(2 * H + 1, beta)
    return h * (L / h.sum())


def phase_table(h, rate, zeros=Z):
    """The device table, float64 [L][P]: row (n M) mod L holds h[n M - k L] for k = ceil((n M - H) / L) .. in order, zero-padded."""
    L, M, H, P = params(rate, zeros)
    t = np.zeros((L, P))
    for p in range(L):
        k = cdiv(p - H, L)
        for j in range(P):
            i = p - (k + j) * L
            if i >= -H:
                t[p, j] = h[i + H]
    return t


def n_ready(recv, rate, zeros=Z):
    L, M, H, _ = params(rate, zeros)
    return max(0, cdiv(recv * L - H, M))


def n_total(n_in, rate):
    L, M, _, _ = params(rate)
    return cdiv(n_in * L, M)


def oldest(n, rate, zeros=Z):
    L, M, H, _ = params(rate, zeros)
    return max(0, cdiv(n * M - H, L))


def smallest_input(n_out, rate):
    """The fewest input samples whose stream has n_out outputs."""
    L, M, _, _ = params(rate)
    return 0 if n_out == 0 else (n_out - 1) * M // L + 1


def resample(x, h, rate, zeros=Z, absolute=False):
    """All ceil(n_in L / M) outputs of stream x (float64) under prototype h (2 H + 1 values, any dtype): the defining sum, or with
    absolute=True the sum of |h[.] x[k]| that bounds its rounding error."""
    L, M, H, P = params(rate, zeros)
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    n_in = x.size
    n_out = cdiv(n_in * L, M)
    if n_out == 0:
        return np.zeros(0)
    n = np.arange(n_out, dtype=np.int64)[:, None]
    k = -((-(n * M - H)) // L) + np.arange(P + 1, dtype=np.int64)[None, :]
    i = n * M - k * L + H
    ok = (i >= 0) & (i <= 2 * H) & (k >= 0) & (k < n_in)
    terms = np.where(ok, h[np.clip(i, 0, 2 * H)] * x[np.clip(k, 0, n_in - 1)], 0.0)
    return np.abs(terms).sum(axis=1) if absolute else terms.sum(axis=1)


def mulaw_table():
    """int [256]: ITU-T G.711 mu-law expansion to 16-bit linear."""
    out = []
    for b in range(256):
        u = ~b & 0xFF
        mag = ((((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)) - 0x84
        out.append(-mag if u & 0x80 else mag)
    return np.array(out, dtype=np.int64)


def alaw_table():
    """int [256]: ITU-T G.711 A-law expansion to 16-bit linear."""
    out = []
    for b in range(256):
        a = b ^ 0x55
        seg, mag = (a & 0x70) >> 4, (a & 0x0F) << 4
        mag = mag + 8 if seg == 0 else (mag + 0x108) << (seg - 1)
        out.append(mag if a & 0x80 else -mag)
    return np.array(out, dtype=np.int64)


def decode(raw, encoding):
    """The decoded samples of a raw chunk (numpy array of the encoding's dtype), float64 (exact: every value is a float32)."""
    raw = np.asarray(raw)
    if encoding == "f32":
        return raw.astype(np.float32).astype(np.float64)
    if encoding == "s16":
        return raw.astype(np.float64) / 32768.0
    table = mulaw_table() if encoding == "mulaw" else alaw_table()
    return table[raw.astype(np.int64)].astype(np.float64) / 32768.0


def raw_stream(n, encoding, seed):
    """n seeded raw samples in the encoding's dtype: 0.3-sigma noise as float or 16-bit PCM, uniform bytes for G.711."""
    rng = np.random.default_rng(seed)
    if encoding == "f32":
        return (0.3 * rng.standard_normal(n)).astype(np.float32)
    if encoding == "s16":
        return np.clip(np.round(0.3 * 32768 * rng.standard_normal(n)), -32768, 32767).astype(np.int16)
    return rng.integers(0, 256, n, dtype=np.uint8)
