"""Live audio at its own sample rate and encoding -> f32 samples at 8 kHz on the device (csrc/resample.hip
`eend_audio_ingest`), for many streams per call: the stage in front of `audio_stream.AudioFrontEnd`.

Decoding (`ENCODINGS`): "f32" any float tensor, the value itself; "s16" int16, v / 32768; "mulaw" / "alaw" uint8, the ITU-T
G.711 expansion to 16-bit linear, / 32768 (256-entry tables built here from the G.711 formula).

Rate conversion from `rate` to 8000 Hz: g = gcd(rate, 8000), L = 8000 / g, M = rate / g, H = zeros M, P = 2 H // L + 1 taps per
output.  The prototype, for i = -H .. H on the rate * L grid,

    h[i] = L (rolloff / M) sinc(rolloff i / M) kaiser(2 H + 1, beta)[i + H],   rescaled so that sum(h) == L,

is computed in float64 and rounded to f32; L == M == 1 has no filter (H = 0, h = [1]).  Output n of a stream of n_in samples is

    y[n] = sum over k = ceil((n M - H) / L) .. floor((n M + H) / L) of h[n M - k L] x[k],   x zero outside [0, n_in)

accumulated in f32 with fmaf from zero in ascending k, so a sample's bits do not depend on how the audio was cut.  The
counters are host integers (`IngestTable`, an `audio_plan.SlotTable`): while a stream is open, recv samples make
max(0, ceil((recv L - H) / M)) outputs ready; at its end all ceil(n_in L / M) exist; after n outputs the oldest sample still needed is max(0, ceil((n M - H) / L)),
so a slot's history is fewer than P <= 255 samples.  The latency is `zeros` output samples (2 ms with the default 16).
Supported: rate >= 8000 with P <= 255 (with the defaults 8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000 Hz).
"""
import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from . import lib as _lib
from .audio_plan import DESC_N, F32, HIST, OPEN, TILE, SlotTable, Staging, there
from .multistream import SlotError

OUT_RATE = 8000
MAX_TAPS = 255
ENCODINGS = {"f32": 0, "s16": 1, "mulaw": 2, "alaw": 3}     # enum ENC_* of csrc/resample.hip
DTYPES = {"f32": torch.float32, "s16": torch.int16, "mulaw": torch.uint8, "alaw": torch.uint8}


def _cdiv(a: int, b: int) -> int:
    return -((-a) // b)


def ratio(rate: int, zeros: int = 16):
    """-> (L, M, H, P) of the conversion rate -> 8000 Hz; ValueError for a rate the kernel does not take."""
    if not isinstance(rate, int) or isinstance(rate, bool):
        raise ValueError(f"sample_rate must be an int, got {rate!r}")
    if not isinstance(zeros, int) or zeros < 1:
        raise ValueError(f"zeros must be a positive int, got {zeros!r}")
    if rate < OUT_RATE:
        raise ValueError(f"sample_rate {rate} Hz is below {OUT_RATE} Hz: the ingest converts down to {OUT_RATE} Hz only")
    g = math.gcd(rate, OUT_RATE)
    L, M = OUT_RATE // g, rate // g
    if L == M:
        return 1, 1, 0, 1
    H = zeros * M
    P = 2 * H // L + 1
    if P > MAX_TAPS:
        raise ValueError(f"sample_rate {rate} Hz with zeros={zeros} needs {P} taps per output, the limit is {MAX_TAPS}")
    return L, M, H, P


class Design:
    """A conversion filter: rate, zeros, beta, rolloff, L, M, H, P and `table`, the f32 [L][P] phase-major coefficients."""

    __slots__ = ("rate", "zeros", "beta", "rolloff", "L", "M", "H", "P", "table")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def ready(self, recv: int, ended: bool = False) -> int:
        """Outputs computable from recv input samples: all of them at the end of the stream."""
        if ended:
            return _cdiv(recv * self.L, self.M)
        return max(0, _cdiv(recv * self.L - self.H, self.M))

    def oldest(self, n: int) -> int:
        """The oldest input sample an output from n on still reads."""
        return max(0, _cdiv(n * self.M - self.H, self.L))


@lru_cache(maxsize=None)
def design(rate: int, zeros: int = 16, beta: float = 9.0, rolloff: float = 0.9) -> Design:
    L, M, H, P = ratio(rate, zeros)
    if not 0.0 < rolloff <= 1.0:
        raise ValueError(f"rolloff must be in (0, 1], got {rolloff!r}")
    table = np.zeros((L, P), dtype=np.float32)
    if H == 0:
        table[0, 0] = 1.0
    else:
        i = np.arange(-H, H + 1, dtype=np.float64)
        h = L * (rolloff / M) * np.sinc(rolloff * i / M) * np.kaiser(2 * H + 1, beta)
        h *= L / h.sum()
        for p in range(L):                                   # output n with (n M) mod L == p: taps h[p - (c + j) L], j = 0 ..
            idx = p - (_cdiv(p - H, L) + np.arange(P)) * L
            ok = idx >= -H
            table[p, ok] = h[idx[ok] + H].astype(np.float32)
    table.setflags(write=False)
    return Design(rate=rate, zeros=zeros, beta=float(beta), rolloff=float(rolloff), L=L, M=M, H=H, P=P, table=table)


def mulaw_table() -> np.ndarray:
    """int32 [256]: G.711 mu-law byte -> 16-bit linear."""
    out = np.zeros(256, dtype=np.int32)
    for b in range(256):
        u = ~b & 0xFF
        t = ((((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84
        out[b] = -t if u & 0x80 else t
    return out


def alaw_table() -> np.ndarray:
    """int32 [256]: G.711 A-law byte -> 16-bit linear."""
    out = np.zeros(256, dtype=np.int32)
    for b in range(256):
        a = b ^ 0x55
        t, seg = (a & 0x0F) << 4, (a & 0x70) >> 4
        t = t + 8 if seg == 0 else (t + 0x108) << (seg - 1)
        out[b] = t if a & 0x80 else -t
    return out


def decode_table() -> np.ndarray:
    """f32 [2][256]: the value of every mu-law byte, then of every A-law byte."""
    return (np.stack([mulaw_table(), alaw_table()]).astype(np.float64) / 32768.0).astype(np.float32)


def check_encoding(encoding: str):
    if encoding not in ENCODINGS:
        raise ValueError(f"unknown encoding {encoding!r} (supported: {sorted(ENCODINGS)})")


def samples(encoding: str, what, w):
    """A chunk as a 1-D tensor of the encoding's dtype; TypeError when its dtype does not match the encoding."""
    if not isinstance(w, torch.Tensor):
        w = torch.as_tensor(w)
    if not (w.is_floating_point() if encoding == "f32" else w.dtype == DTYPES[encoding]):
        want = "a float dtype" if encoding == "f32" else str(DTYPES[encoding])
        raise TypeError(f"{what}: encoding {encoding!r} takes {want}, got {w.dtype}")
    if w.dim() != 1:
        raise ValueError(f"{what}: expected a 1-D waveform, got shape {tuple(w.shape)}")
    return w


_DEVICE_TABLES = {}


def _device_tables(d: Design, dev):
    key = (d.rate, d.zeros, d.beta, d.rolloff, str(dev))
    if key not in _DEVICE_TABLES:
        _DEVICE_TABLES[key] = (torch.from_numpy(d.table.copy()).to(dev), torch.from_numpy(decode_table()).to(dev))
    return _DEVICE_TABLES[key]


def launch(d: Design, encoding: str, desc, n_desc, tiles, n_tiles, hist, out, dev):
    """eend_audio_ingest on the current stream of `dev`; desc and tiles are device addresses."""
    table, dec = _device_tables(d, dev)
    _lib.check(_lib.load().eend_audio_ingest(desc, n_desc, tiles, n_tiles, hist.data_ptr(), table.data_ptr(), dec.data_ptr(), d.L, d.M,
                                             d.H, d.P, ENCODINGS[encoding], out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               "eend_audio_ingest")


@dataclass(slots=True)
class SlotIngest:
    """What one feed does to one slot: input samples recv0 -> recv1, outputs out0 -> out1."""
    slot: int
    recv0: int
    recv1: int
    out0: int
    out1: int
    ended: bool


class IngestTable(SlotTable):
    """Host bookkeeping of the ingest (`audio_plan.SlotTable`, like `audio_stream.FrontEndTable`): per slot the input samples
    received and the 8 kHz samples made."""

    counters = {"recv": "recv1", "outs": "out1"}

    def __init__(self, slots: int, d: Design):
        super().__init__(slots, "an ingest")
        self.d = d

    def advance(self, s, recv1, ended):
        return SlotIngest(s, self.recv[s], recv1, self.outs[s], self.d.ready(recv1, ended), ended)


def stage(plan, waves, staging):
    """The ingest's words for `plan` (chunks placed through `staging`): -> (words, indices of the chunk addresses in it,
    number of tiles, {slot: (first index in the packed output, new outputs)}, outputs in all)."""
    desc, tiles, rows = [], [], {}
    n_out = 0
    for i, p in enumerate(plan):
        desc.append([staging.place(waves.get(p.slot)), p.recv0, p.recv1, p.out0, p.out1, n_out, int(p.ended), p.slot])
        tiles += [[i, n, min(TILE, p.out1 - n)] for n in range(p.out0, p.out1, TILE)]
        rows[p.slot] = (n_out, p.out1 - p.out0)
        n_out += p.out1 - p.out0
    words = [v for d in desc for v in d] + [v for t in tiles for v in t]
    return words, [DESC_N * i for i in range(len(desc))], len(tiles), rows, n_out


def convert(data, sample_rate: int, encoding: str = "f32", zeros: int = 16, beta: float = 9.0, rolloff: float = 0.9):
    """A whole recording (1-D GPU tensor of the encoding's dtype) -> its f32 samples at 8 kHz, the bits a stream of it gives:
    one slot fed the recording and its end in one call."""
    check_encoding(encoding)
    d = design(sample_rate, zeros, beta, rolloff)
    data = samples(encoding, "convert", data)
    if not data.is_cuda:
        raise _lib.EendHipError("audio_ingest.convert: expected a GPU tensor (the HIP path has no CPU fallback)")
    dev = data.device
    table = IngestTable(1, d)
    table.reset(0)
    staging = Staging(dev, DTYPES[encoding])
    words, chunk_at, n_tiles, _rows, n_out = stage(table.plan({0: data.numel()}, end=[0]), {0: data}, staging)
    out = torch.empty(n_out, dtype=F32, device=dev)
    if n_out:
        _dbuf, base = staging.upload(words, chunk_at)
        launch(d, encoding, base, 1, base + 8 * DESC_N, n_tiles, torch.zeros(1, HIST, dtype=F32, device=dev), out, dev)
    return out


class AudioIngest:
    """Decoding and rate conversion for `slots` concurrent streams of one sample rate and encoding:

        ing = AudioIngest(64, 48000, "s16")
        ing.reset(s)
        x = ing.feed({s: chunk, t: other_chunk})      # {slot: 1-D f32 device tensor}: its new samples at 8 kHz
        last = ing.feed({s: final_chunk}, end=[s])    # the rest of the stream: ceil(n_in 8000 / rate) samples in all

    Slots not named in a call pause.  One feed costs two launches and one host-to-device copy and never waits for the device.
    `AudioFrontEnd(sample_rate=, encoding=)` puts one in front of its own feed, in the same staging block."""

    def __init__(self, slots: int, sample_rate: int, encoding: str = "f32", zeros: int = 16, beta: float = 9.0, rolloff: float = 0.9,
                 device=None):
        check_encoding(encoding)
        self.d = design(sample_rate, zeros, beta, rolloff)
        self.encoding, self.dtype = encoding, DTYPES[encoding]
        self.table = IngestTable(slots, self.d)
        self.S = slots
        self.dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.dev.type != "cuda":
            raise _lib.EendHipError("AudioIngest runs on the GPU (no CPU fallback)")
        self.hist = torch.zeros(slots, HIST, dtype=F32, device=self.dev)
        _device_tables(self.d, self.dev)

    def reset(self, s: int):
        """Start an empty stream in slot s (any state): its history row is ignored until overwritten."""
        self.table.reset(s)

    def close(self, s: int):
        self.table.close(s)

    def state(self, s: int) -> str:
        return self.table.state[s]

    def samples(self, s, w):
        return samples(self.encoding, f"slot {s}", w)

    # ---- a slot's stream leaves / comes back (the "ingest" entry of the front-end's snapshot part)
    def _config(self):
        d = self.d
        return {"rate": d.rate, "encoding": self.encoding, "zeros": d.zeros, "beta": d.beta, "rolloff": d.rolloff}

    def export(self, s: int) -> dict:
        return self.table.export(s, self._config(), {"hist": self.hist})

    def check_part(self, part):
        """SlotError unless `part` is an export of an ingest configured like this one."""
        if not self.table.fits(part, self._config(), {"hist": self.hist}):
            raise SlotError("resume: the snapshot's ingest does not fit this front-end "
                            f"(here {self._config()}, there {there(part)!r})")

    def adopt(self, s: int, part, state: str = OPEN):
        """Slot s goes on from an exported `part` (checked by check_part) in `state`: a row copy on the current stream."""
        self.table.adopt(s, part, {"hist": self.hist}, state)

    def launch(self, desc, n_desc, n_tiles, out):
        launch(self.d, self.encoding, desc, n_desc, desc + 8 * DESC_N * n_desc, n_tiles, self.hist, out, self.dev)

    @torch.no_grad()
    def feed(self, waves=None, end=()):
        """waves: {slot: 1-D tensor (CPU or GPU) of its next raw samples}; end: slots whose audio ends here.
        -> {slot: 1-D f32 device tensor of its new samples at 8 kHz} for every slot named."""
        waves = {s: self.samples(s, w) for s, w in dict(waves or {}).items()}
        plan = self.table.plan({s: int(w.numel()) for s, w in waves.items()}, end)
        if not plan:
            return {}
        staging = Staging(self.dev, self.dtype)
        words, chunk_at, n_tiles, rows, n_out = stage(plan, waves, staging)
        _dbuf, base = staging.upload(words, chunk_at)
        out = torch.empty(max(n_out, 1), dtype=F32, device=self.dev)
        self.launch(base, len(plan), n_tiles, out)
        self.table.commit(plan)
        return {s: out[o:o + n] for s, (o, n) in rows.items()}
