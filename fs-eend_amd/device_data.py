"""Labelled training batches built on the device from resident audio (csrc/feature.hip `eend_chunk_batch_f32`).

The reference builds every item of a batch on one CPU core: `get_labeledSTFT -> transform -> splice -> subsample`
(LS-EEND/datasets/diarization_dataset_on_the_fly.py:87-131, datasets/feature.py:255-322).  Here the decoded corpus and its
Kaldi `segments` table live on the GPU, and one call turns a list of chunk rows `(rec, st, ed)` (STFT frames, as
`data.chunk_table` / `data.on_the_fly_chunk` make them) into the features and labels of the whole batch in three launches:

    corpus = DeviceCorpus("cuda:0", storage="s16")
    corpus.add(rec, wave, segments, utt2spk)          # segments: [(utt, st_seconds, et_seconds)], once per recording
    corpus.finalize()                                 # one upload of the samples and of the segment table
    feats, labels, recs = corpus.batch(rows)          # what SpeakerDiarization.training_step takes

Every chunk is treated as a file of its own, so `feats[b]` is `feature.extract_fbank_wave(wave[st * 80:ed * 80], ...)` bit for
bit (the same STFT tile body, the same order of the fp64 sums) and `labels[b]` is the reference's label matrix, subsampled.
The host builds per-chunk descriptors and two tile tables (`plan_batch`, numpy only; the frame count and the layout constants
are `audio_plan`'s), which travel in one pinned block with one asynchronous copy.  Scratch and outputs come from a pool that grows on demand: a repeated batch shape allocates nothing, and
the tensors a call returns are views of the pool that the next `batch` call of the same corpus overwrites (clone what must
outlive it; the training step consumes them before the next batch is built).

Out of scope: reading Kaldi directories or audio files, `use_speaker_id`, the datasets' frame `shuffle`, reflect padding, other
sample rates (convert once with `audio_ingest.convert` before `add`), sharding a corpus across ranks.
"""
import numpy as np
import torch

from . import data as _data
from . import feature
from . import lib as _lib
from .audio_plan import CHUNK_N, F32, FB, HOP, NMEL, SPL_ROWS, WIN, stft_frames

MODES = {"logmel23": 0, "logmel23_mn": 1, "logmel23_cummn": 2}
STORAGES = {"f32": (0, torch.float32), "s16": (1, torch.int16)}
MAX_ROWS, MAX_CHUNKS, MAX_SPEAKERS = 2 ** 31 - 1, 65535, 64
MAX_CONTEXT, MAX_SUBSAMPLING = 64, 4096


def chunk_samples(n_samples: int, st: int, ed: int, frame_shift: int = HOP):
    """(first sample, samples) of chunk [st, ed) frames of a recording of n_samples, clipped as sf.read(start, stop) clips."""
    a = min(st * frame_shift, n_samples)
    return a, min(ed * frame_shift, n_samples) - a


chunk_frames = stft_frames                 # STFT frames of a chunk of `length` samples: a chunk is a file of its own


def _tiles(n, step):
    """Rows (chunk, first, count <= step) that cover n[b] items of every chunk b in pieces of `step`."""
    nt = -(-n // step)
    idx = np.repeat(np.arange(len(n), dtype=np.int64), nt)
    first = (np.arange(int(nt.sum()), dtype=np.int64) - np.repeat(np.cumsum(nt) - nt, nt)) * step
    return idx, first, np.minimum(step, n[idx] - first)


def plan_batch(off, length, start, end, seg0, seg1, subsampling: int):
    """Descriptor and tile tables of one eend_chunk_batch_f32 call (host arithmetic only).  Per chunk: `off` / `length` its
    samples in the corpus (clipped), `start` / `end` its frames as the row names them, `seg0` / `seg1` its recording's segment
    rows.  -> dict(desc (B, 8), stft (n, 3), splice (m, 4) int64 arrays, frames (B,), rows (B,), obase (B,), y_rows, o_rows)."""
    off, length, start, end, seg0, seg1 = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (off, length, start, end, seg0, seg1))
    B = len(off)
    if B > MAX_CHUNKS:
        raise ValueError(f"a batch takes at most {MAX_CHUNKS} chunks, got {B}")
    n = stft_frames(length)
    T = -(-n // subsampling)
    y_rows, o_rows = int(n.sum()), int(T.sum())
    if y_rows > MAX_ROWS or o_rows > MAX_ROWS:
        raise ValueError(f"a batch takes at most 2^31 - 1 frames and rows, got {y_rows} frames and {o_rows} rows")
    ybase, obase = np.cumsum(n) - n, np.cumsum(T) - T
    desc = np.stack([off, length, n, ybase, start, end, seg0, seg1], axis=1) if B else np.zeros((0, CHUNK_N), dtype=np.int64)
    ci, first, cnt = _tiles(n, FB)
    stft = np.stack([ci, first, cnt], axis=1)
    ci, first, cnt = _tiles(T, SPL_ROWS)
    splice = np.stack([ci, first, cnt, obase[ci] + first], axis=1)
    return {"desc": desc, "stft": stft, "splice": splice, "frames": n, "rows": T, "obase": obase, "y_rows": y_rows, "o_rows": o_rows}


class DeviceCorpus:
    """Decoded recordings and their segments, resident on one GPU; see the module's text."""

    def __init__(self, device=None, storage: str = "f32", rate: int = 8000, frame_shift: int = 80, frame_size: int = 200):
        if frame_size != WIN or frame_shift != HOP:
            raise NotImplementedError("the HIP feature front-end is specialised for frame_size=200, frame_shift=80 (all shipped configs)")
        if rate != 8000:
            raise ValueError(f"a corpus holds 8 kHz audio, got rate={rate}: convert once with audio_ingest.convert before add")
        if storage not in STORAGES:
            raise ValueError(f"storage must be one of {sorted(STORAGES)}, got {storage!r}")
        self.dev = torch.device(device) if device is not None else torch.device("cuda")
        if self.dev.type != "cuda":
            raise _lib.EendHipError("DeviceCorpus lives on the GPU (no CPU fallback)")
        self.storage, self.rate, self.frame_shift, self.frame_size = storage, rate, frame_shift, frame_size
        self.reco2dur = {}                      # rec -> seconds, as Kaldi's reco2dur: feeds data.chunk_table as it is
        self.speakers = {}                      # rec -> sorted unique speaker ids (np.unique)
        self._len, self._off, self._seg = {}, {}, {}       # rec -> samples, first sample, (first, last + 1) segment row
        self._waves, self._segrows = [], []
        self._n_samples = 0
        self.samples = self.segments = None      # device tensors after finalize()
        self._pool, self._stage_event = {}, None

    # ---- building the corpus
    def add(self, rec, wave, segments, utt2spk):
        """Append recording `rec`: `wave` its 1-D samples (float for storage "f32", int16 for "s16"; numpy or torch),
        `segments` [(utt, st_seconds, et_seconds)], `utt2spk` {utt: speaker id}."""
        if self.samples is not None:
            raise RuntimeError("the corpus is finalized; add every recording before finalize()")
        if rec in self._len:
            raise ValueError(f"recording {rec!r} is already in the corpus")
        w = wave if isinstance(wave, torch.Tensor) else torch.as_tensor(np.asarray(wave))
        if w.dim() != 1:
            raise ValueError(f"{rec}: expected a 1-D waveform, got shape {tuple(w.shape)}")
        dtype = STORAGES[self.storage][1]
        if self.storage == "s16" and w.dtype != torch.int16:
            raise TypeError(f"{rec}: an s16 corpus takes int16 samples, got {w.dtype}")
        if self.storage == "f32" and not w.is_floating_point():
            raise TypeError(f"{rec}: an f32 corpus takes float samples, got {w.dtype}")
        spk, rows = self._segment_rows(rec, segments, utt2spk)
        n = int(w.numel())
        self._waves.append(w.detach().to(dtype))
        self._enter(rec, n, spk, rows)

    def _segment_rows(self, rec, segments, utt2spk):
        """(the recording's speakers as np.unique orders them, its segment rows (start frame, end frame, speaker index))."""
        segments = list(segments)
        spk = np.unique([utt2spk[utt] for utt, _, _ in segments]).tolist()      # feature.py:290-292
        rows = []
        for utt, st, et in segments:
            sf = int(np.rint(st * self.rate / self.frame_shift).astype(int))       # feature.py:305-308: half to even, in float64
            ef = int(np.rint(et * self.rate / self.frame_shift).astype(int))
            if not (-2 ** 31 <= sf < 2 ** 31 and -2 ** 31 <= ef < 2 ** 31):
                raise ValueError(f"{rec}: segment {utt} is outside the int32 frame range")
            rows.append((sf, ef, spk.index(utt2spk[utt])))
        if len(spk) > MAX_SPEAKERS:
            raise ValueError(f"{rec}: {len(spk)} speakers, at most {MAX_SPEAKERS} are supported")
        return spk, rows

    def _enter(self, rec, n, spk, rows):
        self._len[rec], self._off[rec] = n, self._n_samples
        self._seg[rec] = (len(self._segrows), len(self._segrows) + len(rows))
        self._segrows += rows
        self._n_samples += n
        self.speakers[rec] = spk
        self.reco2dur[rec] = n / self.rate

    def recordings(self):
        """[(rec, seconds)] in the order added: the `recordings` argument of data.chunk_table."""
        return list(self.reco2dur.items())

    def finalize(self):
        """Upload the concatenated samples and the segment table, once."""
        if self.samples is not None:
            return self
        dtype = STORAGES[self.storage][1]
        self.samples = torch.empty(max(self._n_samples, 1), dtype=dtype, device=self.dev)
        at = 0
        for w in self._waves:
            self.samples[at:at + w.numel()].copy_(w, non_blocking=True)
            at += w.numel()
        return self._finish()

    def _finish(self, wait=True):
        seg = np.asarray(self._segrows if self._segrows else [(0, 0, 0)], dtype=np.int32).reshape(-1, 3)
        self.segments = torch.from_numpy(seg).to(self.dev)
        if wait:
            torch.cuda.current_stream(self.dev).synchronize()   # the host copies may go once the upload is done
        self._waves = []
        self.dft, self.melT = feature._tables(self.dev)
        return self

    @classmethod
    def from_device(cls, samples, records, storage: str = "f32", device=None, **kw):
        """A finalized corpus that adopts `samples`, a 1-D device tensor (float32 for storage "f32", int16 for "s16") holding
        the recordings back to back, e.g. as simulate.simulate wrote them.  records: [(rec, samples, segments, utt2spk)] in that
        order, segments and utt2spk as `add` takes them.  The tensor is kept, not copied."""
        self = cls(samples.device if device is None else device, storage, **kw)
        if not samples.is_cuda or self.dev.index not in (None, samples.device.index) or samples.dim() != 1 or samples.dtype != STORAGES[storage][1]:
            raise TypeError(f"a {storage} corpus on {self.dev} adopts a 1-D {STORAGES[storage][1]} tensor there, got "
                            f"{samples.dtype} {tuple(samples.shape)} on {samples.device}")
        for rec, n, segments, utt2spk in records:
            if rec in self._len:
                raise ValueError(f"recording {rec!r} is already in the corpus")
            if n < 0:
                raise ValueError(f"{rec}: {n} samples")
            spk, rows = self._segment_rows(rec, segments, utt2spk)
            self._enter(rec, int(n), spk, rows)
        if self._n_samples > samples.numel():
            raise ValueError(f"the records name {self._n_samples} samples, the tensor holds {samples.numel()}")
        self.samples = samples
        return self._finish(wait=False)                         # no host copy of samples: whoever wrote them is not waited for

    # ---- one batch
    def plan(self, rows, context_size=7, subsampling=10, input_transform="logmel23_mn", n_speakers=None):
        """Everything `batch` decides on the host, with every refusal (no device touched): -> (plan_batch's dict, S per chunk,
        S_max, recs)."""
        if input_transform not in MODES:
            raise ValueError(f"Unknown transform_type: {input_transform} (on the device: {sorted(MODES)})")
        if not isinstance(context_size, int) or not 0 <= context_size <= MAX_CONTEXT:
            raise ValueError(f"context_size must be in 0..{MAX_CONTEXT}, got {context_size!r}")
        if not isinstance(subsampling, int) or not 1 <= subsampling <= MAX_SUBSAMPLING:
            raise ValueError(f"subsampling must be in 1..{MAX_SUBSAMPLING}, got {subsampling!r}")
        if n_speakers is not None and not 1 <= n_speakers <= MAX_SPEAKERS:
            raise ValueError(f"n_speakers must be in 1..{MAX_SPEAKERS}, got {n_speakers!r}")
        cols = [[] for _ in range(6)]
        S, recs = [], []
        for rec, st, ed in rows:
            if rec not in self._len:
                raise KeyError(f"unknown recording {rec!r}")
            st, ed = int(st), int(ed)
            if st < 0 or ed < st:
                raise ValueError(f"{rec}: chunk [{st}, {ed}) must have 0 <= st <= ed")
            n_spk = len(self.speakers[rec])
            if n_speakers is not None and n_speakers < n_spk:
                raise IndexError(f"{rec} has {n_spk} speakers, n_speakers={n_speakers} is too small")       # as feature.py:315
            a, length = chunk_samples(self._len[rec], st, ed)
            for c, v in zip(cols, (self._off[rec] + a, length, st, ed) + self._seg[rec]):
                c.append(v)
            S.append(n_spk if n_speakers is None else n_speakers)
            recs.append(rec)
        p = plan_batch(*cols, subsampling)
        return p, S, max(S + [1]), recs

    def _buf(self, name, numel, dtype, **kw):
        t = self._pool.get(name)
        if t is None or t.numel() < numel:
            t = self._pool[name] = torch.empty(max(numel, 1), dtype=dtype, **kw)
        return t

    @torch.no_grad()
    def batch(self, rows, context_size=7, subsampling=10, input_transform="logmel23_mn", n_speakers=None):
        """rows: [(rec, st, ed)] in STFT frames -> (feats, labels, recs): feats[b] (T_b, 23 (2 ctx + 1)) and labels[b]
        (T_b, S_b) float32 views of the pool's packed outputs, T_b = ceil(n_b / subsampling), S_b = n_speakers or the
        recording's speaker count."""
        p, S, S_max, recs = self.plan(rows, context_size, subsampling, input_transform, n_speakers)
        if self.samples is None:
            raise RuntimeError("finalize() the corpus before batch()")
        dev, W = self.dev, NMEL * (2 * context_size + 1)
        mode = MODES[input_transform]
        B, n_stft, n_splice = len(recs), len(p["stft"]), len(p["splice"])
        n_words = CHUNK_N * B + 3 * n_stft + 4 * n_splice
        L = _lib.load()
        feats_all = self._buf("feats", p["o_rows"] * W, F32, device=dev)
        labels_all = self._buf("labels", p["o_rows"] * S_max, F32, device=dev)
        if B:
            Y = self._buf("Y", p["y_rows"] * NMEL, F32, device=dev)
            Yn = self._buf("Yn", p["y_rows"] * NMEL if mode else 0, F32, device=dev)
            dbuf = self._buf("tables", n_words, torch.int64, device=dev)
            stage = self._buf("stage", n_words, torch.int64, pin_memory=True)
            if self._stage_event is not None:
                self._stage_event.synchronize()         # the previous call's copy has read the block (long done, as a rule)
            words = stage.numpy()
            at = 0
            for part in (p["desc"], p["stft"], p["splice"]):
                words[at:at + part.size] = part.reshape(-1)
                at += part.size
            stream = torch.cuda.current_stream(dev)
            with torch.cuda.device(dev):
                dbuf[:n_words].copy_(stage[:n_words], non_blocking=True)
                if self._stage_event is None:
                    self._stage_event = torch.cuda.Event()
                self._stage_event.record(stream)
                base = dbuf.data_ptr()
                _lib.check(L.eend_chunk_batch_f32(self.samples.data_ptr(), STORAGES[self.storage][0], self.segments.data_ptr(), base, B,
                                                  base + 8 * CHUNK_N * B, n_stft, base + 8 * (CHUNK_N * B + 3 * n_stft), n_splice,
                                                  Y.data_ptr(), Yn.data_ptr(), feats_all.data_ptr(), labels_all.data_ptr(), S_max,
                                                  mode, context_size, subsampling, self.dft.data_ptr(), self.melT.data_ptr(),
                                                  stream.cuda_stream), "eend_chunk_batch_f32")
        fv = feats_all[:p["o_rows"] * W].view(p["o_rows"], W)
        lv = labels_all[:p["o_rows"] * S_max].view(p["o_rows"], S_max)
        feats = [fv[o:o + t] for o, t in zip(p["obase"].tolist(), p["rows"].tolist())]
        labels = [lv[o:o + t, :s] for o, t, s in zip(p["obase"].tolist(), p["rows"].tolist(), S)]
        return feats, labels, recs

    def collate(self, context_size=7, subsampling=10, input_transform="logmel23_mn", n_speakers=None):
        """A `collate_func` for trainer.SpeakerDiarization / a DataLoader over a ChunkDataset (n_workers = 0): the list of
        row descriptors of a batch -> one batch(...) call."""
        def collate_func(rows):
            return list(self.batch(list(rows), context_size, subsampling, input_transform, n_speakers))
        return collate_func


class ChunkDataset:
    """The dataset side of the device path: `rows` are data.chunk_table's, `__getitem__` returns only the row descriptor
    (rec, st, ed) of an item, and corpus.collate(...) builds the tensors of a whole batch.  An item is named by its index, or by
    the (index, seed) pair of data.MyDistributedSampler, which draws the chunk start as data.on_the_fly_chunk does (rows of
    chunk_table(..., on_the_fly=True): (rec, data_len, st, ed))."""

    def __init__(self, corpus, rows, chunk_size=2000, subsampling=1, data_type="train"):
        self.corpus, self.rows = corpus, list(rows)
        self.chunk_size, self.subsampling, self.data_type = chunk_size, subsampling, data_type
        for row in self.rows:
            if row[0] not in corpus.reco2dur:
                raise KeyError(f"unknown recording {row[0]!r}")

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, item):
        if isinstance(item, (tuple, list)):
            index, seed = item
            row = self.rows[index]
            if len(row) != 4:
                raise ValueError("an (index, seed) item needs on-the-fly rows (rec, data_len, st, ed): chunk_table(..., on_the_fly=True)")
            return _data.on_the_fly_chunk(row, int(seed), self.chunk_size, self.subsampling, self.data_type)
        row = self.rows[item]
        return (row[0], row[-2], row[-1])
