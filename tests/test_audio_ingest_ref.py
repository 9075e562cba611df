"""CPU: the audio ingest's arithmetic.  The float64 restatement (tests/resample_ref.py) against scipy's polyphase resampler and
against the filter's frequency-response conditions, the G.711 tables against their pins and audioop, `IngestTable`'s counters
over random cuttings, the refusals, and `audio_ingest.design` against the restatement bit for bit."""
import random

import numpy as np
import pytest
import torch

from tests import resample_ref as R


@pytest.mark.parametrize("rate", R.RATES)
def test_restatement_matches_upfirdn(rate):
    from scipy.signal import upfirdn
    L, M, H, P = R.params(rate)
    h = R.prototype(rate)
    assert abs(h.sum() - L) < 1e-12 and h.size == 2 * H + 1 and np.array_equal(h, h[::-1])
    rng = np.random.default_rng(rate)
    for n_in in (1, M, 5 * M + 3, 2000):
        x = 0.3 * rng.standard_normal(n_in)
        got = R.resample(x, h, rate)
        n_out = R.n_total(n_in, rate)
        assert got.shape == (n_out,)
        lat = R.Z if H else 0                                       # the filter's delay in output samples
        want = upfirdn(h, x, L, M)[lat:lat + n_out]
        assert want.shape == got.shape
        assert np.abs(got - want).max() <= 1e-15, (rate, n_in, np.abs(got - want).max())


def test_supported_rates_and_taps():
    taps = {rate: R.params(rate)[3] for rate in R.RATES}
    assert taps == {8000: 1, 11025: 45, 12000: 49, 16000: 65, 22050: 89, 24000: 97, 32000: 129, 44100: 177, 48000: 193}
    assert R.params(96000)[3] == 385
    for rate in R.RATES:
        L, M, H, P = R.params(rate)
        assert 255 * M // L + P + 2 <= 2048                         # the kernel's LDS span


@pytest.mark.parametrize("rate", R.RATES[1:])
def test_frequency_response(rate):
    """Ripple below 0.05 dB up to 3 kHz, everything from 5 kHz up (to the Nyquist frequency of the rate * L grid) below -90 dB."""
    L, M, H, P = R.params(rate)
    h = R.prototype(rate) / L
    fs = float(rate * L)
    i = np.arange(-H, H + 1, dtype=np.float64)

    def gain_db(f):
        g = np.concatenate([np.cos(2 * np.pi * np.outer(f[a:a + 100], i) / fs) @ h for a in range(0, f.size, 100)])   # h is symmetric
        return 20 * np.log10(np.maximum(np.abs(g), 1e-300))

    assert np.abs(gain_db(np.linspace(0.0, 3000.0, 301))).max() < 0.05
    nyq = fs / 2
    stop = np.linspace(5000.0, min(nyq, 12000.0), 701)              # the highest side lobes, finely, then the rest of the band
    if nyq > 12000.0:
        stop = np.concatenate([stop, np.linspace(12000.0, nyq, 800)])
    assert gain_db(stop).max() < -90.0
    assert -29.0 < gain_db(np.array([4000.0]))[0] < -25.0


def test_g711_tables():
    from fs_eend_amd import audio_ingest as I
    mu, al = R.mulaw_table(), R.alaw_table()
    assert (mu[0x00], mu[0x80], mu[0xFF], mu[0x7F]) == (-32124, 32124, 0, 0)
    assert (al[0x55], al[0xD5], al[0x2A], al[0xAA]) == (-8, 8, -32256, 32256)
    assert np.array_equal(I.mulaw_table(), mu) and np.array_equal(I.alaw_table(), al)
    dec = I.decode_table()
    assert dec.dtype == np.float32 and dec.shape == (2, 256)
    assert np.array_equal(dec.astype(np.float64) * 32768, np.stack([mu, al]))         # every value is exact in f32
    try:
        import audioop
    except ImportError:
        return
    every = bytes(range(256))
    assert np.array_equal(np.frombuffer(audioop.ulaw2lin(every, 2), dtype="<i2"), mu)
    assert np.array_equal(np.frombuffer(audioop.alaw2lin(every, 2), dtype="<i2"), al)


@pytest.mark.parametrize("rate", R.RATES)
def test_design_equals_restatement(rate):
    from fs_eend_amd import audio_ingest as I
    d = I.design(rate)
    assert (d.L, d.M, d.H, d.P) == R.params(rate) and (d.zeros, d.beta, d.rolloff) == (R.Z, R.BETA, R.RHO)
    want = R.phase_table(R.prototype(rate), rate).astype(np.float32)
    assert d.table.dtype == np.float32 and d.table.shape == want.shape
    assert np.array_equal(d.table.view(np.uint32), want.view(np.uint32))
    for recv in (0, 1, 95, 96, 97, 1000, 12345):
        assert d.ready(recv) == R.n_ready(recv, rate) and d.ready(recv, True) == R.n_total(recv, rate)
        assert d.oldest(recv) == R.oldest(recv, rate)


@pytest.mark.parametrize("rate", R.RATES)
def test_ingest_table_counters(rate):
    """200 random cuttings: the outputs per call add up to ceil(n_in L / M), the ready count never decreases and matches the
    restatement, the history (oldest sample still needed .. last received) is never longer than P."""
    from fs_eend_amd import audio_ingest as I
    L, M, H, P = R.params(rate)
    rng = random.Random(rate)
    d = I.design(rate)
    t = I.IngestTable(3, d)
    for it in range(200):
        s = it % 3
        n_in = rng.choice([0, 1, M - 1, M, rng.randrange(0, 40 * M), rng.randrange(0, 6000)])
        cuts = sorted(rng.randrange(n_in + 1) for _ in range(rng.randrange(0, 12)))
        sizes = [b - a for a, b in zip([0] + cuts, cuts + [n_in])]
        t.reset(s)
        total = 0
        for i, m in enumerate(sizes):
            last = i == len(sizes) - 1 and rng.random() < 0.5
            (p,) = t.plan({s: m}, end=[s] if last else [])
            assert p.out1 >= p.out0 == t.outs[s] and p.recv0 == t.recv[s] and p.recv1 == p.recv0 + m
            if not last:
                assert p.out1 == R.n_ready(p.recv1, rate)
                hist = p.recv1 - R.oldest(p.out1, rate)
                assert 0 <= hist < P <= 255, (rate, p.recv1, p.out1, hist)
            total += p.out1 - p.out0
            t.commit([p])
        if t.state[s] != "ended":
            (p,) = t.plan({}, end=[s])
            total += p.out1 - p.out0
            t.commit([p])
        assert total == t.outs[s] == R.n_total(n_in, rate) and t.state[s] == "ended"


def test_refusals():
    from fs_eend_amd import audio_ingest as I
    from fs_eend_amd.audio_stream import AudioFrontEnd
    from fs_eend_amd.multistream import SlotError
    with pytest.raises(ValueError, match="8000"):
        I.design(7999)
    with pytest.raises(ValueError, match="385 taps.*255"):
        I.design(96000)
    for bad in (dict(sample_rate=7999), dict(sample_rate=96000), dict(encoding="opus")):
        with pytest.raises(ValueError):
            AudioFrontEnd(2, "logmel23", device="cpu", **bad)
        with pytest.raises(ValueError):
            I.AudioIngest(2, **{"sample_rate": 16000, **bad}, device="cpu")
    with pytest.raises(TypeError, match="mulaw.*uint8.*int16"):
        I.samples("mulaw", "slot 0", torch.zeros(10, dtype=torch.int16))
    with pytest.raises(TypeError):
        I.samples("s16", "slot 0", torch.zeros(10))
    with pytest.raises(TypeError):
        I.samples("f32", "slot 0", torch.zeros(10, dtype=torch.int16))
    assert I.samples("f32", "slot 0", torch.zeros(10, dtype=torch.float64)).dtype == torch.float64
    with pytest.raises(ValueError, match="1-D"):
        I.samples("alaw", "slot 0", torch.zeros(2, 5, dtype=torch.uint8))
    t = I.IngestTable(2, I.design(16000))
    with pytest.raises(SlotError, match="not open"):
        t.plan({0: 10})
    t.reset(0)
    t.commit(t.plan({0: 100}, end=[0]))
    with pytest.raises(SlotError, match="fed its end"):
        t.plan({0: 1})                                              # audio after the end
    with pytest.raises(SlotError):
        t.plan({2: 1})
    t.reset(1)
    with pytest.raises(ValueError):
        t.plan({1: -1})


def test_entry_is_declared_and_bound():
    from fs_eend_amd import lib as L
    from tests.test_cabi import _header_protos
    assert _header_protos()["eend_audio_ingest"] == len(L.PROTOTYPES["eend_audio_ingest"]) == 14
    assert L.ABI_VERSION == 5
