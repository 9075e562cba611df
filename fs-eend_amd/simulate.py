"""Reverberant, noisy training mixtures simulated on the device from resident dry sources (csrc/simulate.hip `eend_sim_mix_f32`).

FS-EEND and LS-EEND train on simulated mixtures (`data_simu_*`, both shipped configs are `*_simu.yaml`): single-speaker
utterances laid out with random silences, convolved with a room impulse response per speaker, summed, with a noise added at a
chosen SNR.  The reference takes them as files made elsewhere.  Here utterances, impulse responses and noises live on the GPU
and one call turns a list of recipes into a finalized `device_data.DeviceCorpus`, so the mixtures can be redrawn every epoch:

    utts, rirs, noises = SourcePool("cuda:0", "s16"), SourcePool("cuda:0"), SourcePool("cuda:0", "s16")
    utts.add(name, wave) ...; utts.finalize()            # likewise rirs (always "f32") and noises
    rirs = rooms.room_responses(rows, taps)              # or: responses of drawn rooms made on the device (rooms.py), none loaded
    recipes = draw_recipes(seed, spk2utt, utts, rirs=rirs, noises=noises, n_mixtures=64)
    corpus, stats = simulate(utts, rirs, noises, recipes, storage="f32")
    feats, labels, recs = corpus.batch(rows)             # as with a corpus built by add / finalize

A recipe is a dict: {"name", "length" (samples), "tracks": [{"speaker", "rir" (name or None), "gain", "placements": [(utterance
name, start sample)]}], "noise" (name or None), "noise_offset", "snr_db" (or None)}.  The arithmetic contract (dry track, taps,
wet mix, noise scale, storage) is written down at eend_sim_mix_f32 in include/eend_hip.h and in DESIGN 10d; tests/simulate_ref.py
restates it in float64.  `plan` does everything the host decides, with every refusal, in numpy and without a device; the tables
travel in one pinned block with one asynchronous copy, and the device runs four launches whatever the call holds.

Impulse responses no longer have to be loaded: `rooms.room_responses` generates them on the device by the image method and
returns the pool `simulate` takes as `rirs` (`SourcePool.from_device` adopts any device tensor), and `draw_recipes(...,
rir_groups=groups)` keeps the speakers of a mixture in one room.

Out of scope: reading audio or Kaldi files, rates other than 8 kHz (convert with `audio_ingest.convert` first), FFT or
overlap-save convolution, sharding across ranks, equality with any particular external mixing script.
"""
import numpy as np
import torch

from . import lib as _lib
from .device_data import MAX_CHUNKS, MAX_ROWS, MAX_SPEAKERS, STORAGES, DeviceCorpus, _tiles

# csrc/kernels.h SIM_*: outputs per tile, FIR steps per tap slice, the most taps of a track, words per descriptor row
TILE, SLICE, MAX_TAPS = 2048, 1024, 8192
MIX_WORDS, TRACK_WORDS, PLACE_WORDS = 10, 5, 3
MAX_MIXTURES, MAX_TRACKS, MAX_SAMPLES = MAX_CHUNKS, MAX_SPEAKERS, MAX_ROWS
RATE = 8000


class SourcePool:
    """A ragged resident buffer of named waves, back to back on one GPU: `add(name, wave)` (numpy or torch, 1-D; float for
    storage "f32", int16 for "s16"), then `finalize()` uploads them once.  `table` is {name: (first sample, samples)}."""

    def __init__(self, device=None, storage: str = "f32"):
        if storage not in STORAGES:
            raise ValueError(f"storage must be one of {sorted(STORAGES)}, got {storage!r}")
        self.dev = torch.device(device) if device is not None else torch.device("cuda")
        if self.dev.type != "cuda":
            raise _lib.EendHipError("SourcePool lives on the GPU (no CPU fallback)")
        self.storage, self.table = storage, {}
        self._waves, self._n = [], 0
        self.samples = None

    def add(self, name, wave):
        if self.samples is not None:
            raise RuntimeError("the pool is finalized; add every wave before finalize()")
        if name in self.table:
            raise ValueError(f"{name!r} is already in the pool")
        w = wave if isinstance(wave, torch.Tensor) else torch.as_tensor(np.asarray(wave))
        if w.dim() != 1:
            raise ValueError(f"{name}: expected a 1-D wave, got shape {tuple(w.shape)}")
        if self.storage == "s16" and w.dtype != torch.int16:
            raise TypeError(f"{name}: an s16 pool takes int16 samples, got {w.dtype}")
        if self.storage == "f32" and not w.is_floating_point():
            raise TypeError(f"{name}: an f32 pool takes float samples, got {w.dtype}")
        self._waves.append(w.detach().to(STORAGES[self.storage][1]))
        self.table[name] = (self._n, int(w.numel()))
        self._n += int(w.numel())

    def finalize(self):
        if self.samples is not None:
            return self
        self.samples = torch.empty(max(self._n, 1), dtype=STORAGES[self.storage][1], device=self.dev)
        at = 0
        for w in self._waves:
            self.samples[at:at + w.numel()].copy_(w, non_blocking=True)
            at += w.numel()
        torch.cuda.current_stream(self.dev).synchronize()       # the host copies may go once the upload is done
        self._waves = []
        return self

    @classmethod
    def from_device(cls, samples, table, storage: str = "f32"):
        """A finalized pool that adopts `samples`, a 1-D device tensor (float32 for storage "f32", int16 for "s16") holding the
        waves named by `table` {name: (first sample, samples)}, e.g. as rooms.room_responses wrote them: the counterpart of
        DeviceCorpus.from_device.  The tensor is kept, not copied, and whoever wrote it is not waited for."""
        if storage not in STORAGES:
            raise ValueError(f"storage must be one of {sorted(STORAGES)}, got {storage!r}")
        if not isinstance(samples, torch.Tensor) or samples.dtype != STORAGES[storage][1] or samples.dim() != 1:
            raise TypeError(f"a {storage} pool adopts a 1-D {STORAGES[storage][1]} tensor, got "
                            f"{getattr(samples, 'dtype', type(samples))} {tuple(getattr(samples, 'shape', ()))}")
        table = {name: (int(first), int(n)) for name, (first, n) in dict(table).items()}
        for name, (first, n) in table.items():
            if first < 0 or n < 0 or first + n > samples.numel():
                raise ValueError(f"{name!r}: samples {first} .. {first + n} lie outside the tensor's {samples.numel()}")
        if not samples.is_cuda:
            raise _lib.EendHipError("SourcePool lives on the GPU (no CPU fallback)")
        self = cls(samples.device, storage)
        self.table, self._n, self.samples = table, int(samples.numel()), samples
        return self


def _table(pool):
    """{name: (first sample, samples)} of a SourcePool, of such a dict itself, or of nothing."""
    if pool is None:
        return {}
    return pool.table if isinstance(pool, SourcePool) else pool


def plan(recipes, utts, rirs=None, noises=None):
    """Everything `simulate` decides on the host, with every refusal (numpy only, no device touched).  utts, rirs, noises: a
    SourcePool or its table {name: (first sample, samples)}.  -> dict(mix (M, 10), tracks (T, 5), places (P, 3), tiles (n, 2)
    int64 arrays as eend_sim_mix_f32 takes them, names, lengths (M,), offsets (M,), total, and per mixture `segments`
    [(utt, st_seconds, et_seconds)] with `utt2spk`, as DeviceCorpus.add takes them)."""
    utts, rirs, noises = _table(utts), _table(rirs), _table(noises)
    recipes = list(recipes)
    if len(recipes) > MAX_MIXTURES:
        raise ValueError(f"a call takes at most {MAX_MIXTURES} mixtures, got {len(recipes)}")
    mix, tracks, places, names, segments, utt2spk = [], [], [], [], [], []
    total = 0
    for r in recipes:
        name, N = r["name"], int(r["length"])
        if name in names:
            raise ValueError(f"mixture {name!r} is named twice")
        if N < 1:
            raise ValueError(f"{name}: a mixture has at least one sample, got length {N}")
        if len(r["tracks"]) > MAX_TRACKS:
            raise ValueError(f"{name}: {len(r['tracks'])} tracks, at most {MAX_TRACKS} are supported")
        segs, u2s = [], {}
        track0 = len(tracks)
        for si, t in enumerate(r["tracks"]):
            rir = t.get("rir")
            if rir is not None and rir not in rirs:
                raise KeyError(f"{name}: unknown impulse response {rir!r}")
            roff, K = rirs[rir] if rir is not None else (-1, 1)
            if not 1 <= K <= MAX_TAPS:
                raise ValueError(f"{name}: impulse response {rir!r} has {K} taps, 1 .. {MAX_TAPS} are supported")
            gain = np.float32(t.get("gain", 1.0))
            place0, end = len(places), 0
            for pi, (utt, start) in enumerate(t["placements"]):
                if utt not in utts:
                    raise KeyError(f"{name}: unknown utterance {utt!r}")
                start = int(start)
                src, n = utts[utt]
                if start < 0:
                    raise ValueError(f"{name}: utterance {utt!r} starts at {start}, before the mixture")
                if start < end:
                    raise ValueError(f"{name}: the placements of track {si} must be sorted by start and must not overlap "
                                     f"({utt!r} starts at {start}, the one before it ends at {end})")
                if start >= N:
                    raise ValueError(f"{name}: utterance {utt!r} starts at {start}, past the mixture's {N} samples")
                end = start + n
                clipped = min(end, N) - start
                if clipped > 0:
                    places.append((start, src, clipped))
                seg = f"{name}_{si}_{pi}"
                segs.append((seg, start / RATE, min(end, N) / RATE))
                u2s[seg] = t["speaker"]
            tracks.append((roff, K, int(gain.view(np.uint32)), place0, len(places) - place0))
        noise, snr = r.get("noise"), r.get("snr_db")
        noff = nlen = o = 0
        c = 0.0
        if noise is not None and snr is not None:
            if noise not in noises:
                raise KeyError(f"{name}: unknown noise {noise!r}")
            noff, nlen = noises[noise]
            o = int(r.get("noise_offset", 0))
            if o < 0:
                raise ValueError(f"{name}: noise_offset must not be negative, got {o}")
            c = 10.0 ** (-float(snr) / 10.0)
        mix.append([N, total, track0, len(tracks) - track0, noff, nlen, o, int(np.float64(c).view(np.int64)), 0, 0])
        names.append(name)
        segments.append(segs)
        utt2spk.append(u2s)
        total += N
        if total > MAX_SAMPLES:
            raise ValueError(f"a call takes at most 2^31 - 1 samples, got {total} by mixture {name!r}")
    mix = np.asarray(mix, dtype=np.int64).reshape(-1, MIX_WORDS)
    lengths = mix[:, 0].copy()
    idx, first, _ = _tiles(lengths, TILE)
    nt = -(-lengths // TILE)
    mix[:, 8], mix[:, 9] = np.cumsum(nt) - nt, nt
    return {"mix": mix, "tracks": np.asarray(tracks, dtype=np.int64).reshape(-1, TRACK_WORDS),
            "places": np.asarray(places, dtype=np.int64).reshape(-1, PLACE_WORDS), "tiles": np.stack([idx, first], axis=1),
            "names": names, "lengths": lengths, "offsets": mix[:, 1].copy(), "total": total, "segments": segments,
            "utt2spk": utt2spk}


def _check_pool(pool, what, dev):
    if pool is None:
        return None
    if not isinstance(pool, SourcePool) or pool.samples is None:
        raise RuntimeError(f"{what} must be a finalized SourcePool")
    if pool.samples.device != dev:
        raise ValueError(f"{what} lives on {pool.samples.device}, the utterances on {dev}")
    return pool


@torch.no_grad()
def simulate(utts, rirs, noises, recipes, storage: str = "f32"):
    """Mix `recipes` from the resident pools.  -> (corpus, stats): `corpus` a finalized DeviceCorpus of storage "f32" or "s16"
    whose recordings are the mixtures (named and ordered as the recipes) and whose samples the kernel wrote; `stats` device
    tensors Ps, Pn float64 [M], scale float32 [M], clipped int32 [M], and `y`, the wet mix before the noise, float32 [total]."""
    if storage not in STORAGES:
        raise ValueError(f"storage must be one of {sorted(STORAGES)}, got {storage!r}")
    if not isinstance(utts, SourcePool) or utts.samples is None:
        raise RuntimeError("utts must be a finalized SourcePool")
    dev = utts.samples.device
    rirs, noises = _check_pool(rirs, "rirs", dev), _check_pool(noises, "noises", dev)
    if rirs is not None and rirs.storage != "f32":
        raise ValueError("impulse responses are kept as f32")
    p = plan(recipes, utts, rirs, noises)
    M, n_tiles, total = len(p["names"]), len(p["tiles"]), p["total"]
    out = torch.empty(max(total, 1), dtype=STORAGES[storage][1], device=dev)
    y = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
    part = torch.empty(max(2 * n_tiles, 1), dtype=torch.float64, device=dev)
    stats = {"Ps": torch.zeros(M, dtype=torch.float64, device=dev), "Pn": torch.zeros(M, dtype=torch.float64, device=dev),
             "scale": torch.zeros(M, dtype=torch.float32, device=dev), "clipped": torch.zeros(M, dtype=torch.int32, device=dev),
             "y": y[:total]}
    if M:
        parts = (p["mix"], p["tracks"], p["places"], p["tiles"])
        n_words = sum(a.size for a in parts)
        stage = torch.empty(n_words, dtype=torch.int64, pin_memory=True)      # a fresh pinned block per call (copied asynchronously)
        words, at, addr = stage.numpy(), 0, []
        for a in parts:
            words[at:at + a.size] = a.reshape(-1)
            addr.append(8 * at)
            at += a.size
        dbuf = torch.empty(n_words, dtype=torch.int64, device=dev)
        empty = torch.zeros(1, dtype=torch.float32, device=dev)              # stands in for a pool the call does not have
        stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            dbuf.copy_(stage, non_blocking=True)
            base = dbuf.data_ptr()
            L = _lib.load()
            _lib.check(L.eend_sim_mix_f32(
                utts.samples.data_ptr(), STORAGES[utts.storage][0], (rirs.samples if rirs is not None else empty).data_ptr(),
                (noises.samples if noises is not None else empty).data_ptr(), STORAGES[noises.storage][0] if noises is not None else 0,
                base + addr[0], M, base + addr[1], base + addr[2], base + addr[3], n_tiles, y.data_ptr(), part.data_ptr(),
                out.data_ptr(), STORAGES[storage][0], stats["Ps"].data_ptr(), stats["Pn"].data_ptr(), stats["scale"].data_ptr(),
                stats["clipped"].data_ptr(), stream.cuda_stream), "eend_sim_mix_f32")
    corpus = DeviceCorpus.from_device(out, [(n, int(k), s, u) for n, k, s, u in zip(p["names"], p["lengths"], p["segments"], p["utt2spk"])],
                                      storage=storage, device=dev)
    return corpus, stats


def _length(utts, name):
    return _table(utts)[name][1]


def draw_recipes(seed, spk2utt, utts, rirs=None, noises=None, n_mixtures=1, n_speakers=(1, 4), n_utts=(2, 5), beta=2.0,
                 gain_db=(-3.0, 3.0), snr_db=(10.0, 15.0, 20.0), prefix="mix", rir_groups=None):
    """The usual generator of simulated mixtures (host only, deterministic in the seed).  spk2utt: {speaker: [utterance name]};
    utts, rirs, noises: a SourcePool or its table (rirs / noises None or empty: dry / clean mixtures).  Per mixture: a number of
    speakers in n_speakers (inclusive, drawn without replacement); per speaker a number of utterances in n_utts (inclusive),
    each preceded by a silence drawn from an exponential with mean `beta` seconds, one impulse response and one gain (uniform
    in dB over gain_db); per mixture one noise, an offset into it and an SNR from snr_db.  The mixture's length is the end of
    its longest track.  Every draw comes from numpy.random.Generator(PCG64(seed)) in a fixed order.

    rir_groups {room: [response names]} (rooms.draw_rooms makes one) puts a mixture in one room: after its speakers the mixture
    draws a room, then one response per speaker from that room without replacement, so all its speakers share a room and a
    microphone; the per-speaker response draw is left out.  A room with fewer responses than the mixture has speakers is
    refused.  With None every draw and the result are what they are without the argument."""
    rng = np.random.Generator(np.random.PCG64(seed))
    speakers = sorted(spk2utt)
    rir_names, noise_names = sorted(_table(rirs)), sorted(_table(noises))
    rooms = None
    if rir_groups is not None:
        rooms = sorted(rir_groups)
        if not rooms:
            raise ValueError("rir_groups names no room")
        for room in rooms:
            for h in rir_groups[room]:
                if h not in _table(rirs):
                    raise KeyError(f"room {room!r}: unknown impulse response {h!r}")
    lo, hi = n_speakers
    if not 1 <= lo <= hi <= min(len(speakers), MAX_TRACKS):
        raise ValueError(f"n_speakers {n_speakers} must lie in 1 .. {min(len(speakers), MAX_TRACKS)}")
    recipes = []
    for i in range(n_mixtures):
        chosen = rng.choice(len(speakers), size=int(rng.integers(lo, hi + 1)), replace=False)
        tracks, length = [], 1
        shared = None
        if rooms is not None:
            room = rooms[int(rng.integers(len(rooms)))]
            if len(rir_groups[room]) < len(chosen):
                raise ValueError(f"room {room!r} has {len(rir_groups[room])} responses, the mixture {len(chosen)} speakers")
            shared = [rir_groups[room][j] for j in rng.choice(len(rir_groups[room]), size=len(chosen), replace=False).tolist()]
        for si in chosen.tolist():
            spk, pos, placements = speakers[si], 0, []
            for _ in range(int(rng.integers(n_utts[0], n_utts[1] + 1))):
                utt = spk2utt[spk][int(rng.integers(len(spk2utt[spk])))]
                pos += int(np.rint(rng.exponential(beta) * RATE))
                placements.append((utt, pos))
                pos += _length(utts, utt)
            if shared is not None:
                rir = shared[len(tracks)]
            else:
                rir = rir_names[int(rng.integers(len(rir_names)))] if rir_names else None
            gain = float(10.0 ** (rng.uniform(*gain_db) / 20.0))
            tracks.append({"speaker": spk, "rir": rir, "gain": gain, "placements": placements})
            length = max(length, pos)
        r = {"name": f"{prefix}_{seed}_{i:05d}", "length": length, "tracks": tracks, "noise": None, "noise_offset": 0, "snr_db": None}
        if noise_names:
            r["noise"] = noise_names[int(rng.integers(len(noise_names)))]
            r["noise_offset"] = int(rng.integers(_length(noises, r["noise"])))
            r["snr_db"] = float(snr_db[int(rng.integers(len(snr_db)))])
        recipes.append(r)
    return recipes
