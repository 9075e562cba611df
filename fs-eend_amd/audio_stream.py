"""Audio in, logits out for live streams: an incremental feature front-end for many streams (csrc/feature.hip
`eend_audio_feed_f32`) and `AudioStreamSession`, which puts it in front of `FsMultiStreamSession` / `LsMultiStreamSession`.

`feature.extract_fbank_wave` needs the whole recording: its frame count and right-edge padding depend on the final length,
the splice pads with zeros past the last frame and `logmel23_cummn` normalises by the running mean of every earlier frame.
Both shipped transforms are causal, so they can be computed as the audio arrives.  Per slot the device keeps the sample tail
(fewer than 200 samples), the fp64 column sums of the running mean and a ring of the last normalised log-mel frames that the
splice of the next model frame reads; the host keeps the counters, which depend on sample counts only
(`FrontEndTable`).  With pad_mode "constant" (first sample of frame f at 80 f - 100, as `feature.logmel`):

    log-mel frame f is ready once 80 f + 100 samples are in;
    model frame j (frames sub j - ctx .. sub j + ctx) once log-mel frame sub j + ctx exists;
    at the end of a stream of n samples the rest follow the batch rules: n_frames = 1 + n // 80 - (n % 80 == 0) log-mel
    frames (zero samples past n) and ceil(n_frames / sub) model frames (zero frames past n_frames).

`logmel23` frames are bit-identical to the batch front-end (the same STFT tile body); `logmel23_cummn` adds the fp64 running
sum strictly in frame order, so its features do not depend on how the audio was cut, and differ from the batch path (which
sums in another order) by about one float ulp of the mean.  One `feed` costs three launches and one host-to-device copy,
whatever the number of slots or the chunk sizes, and never waits for the device.

Audio that is not 8 kHz float goes through `audio_ingest.AudioIngest` first (`sample_rate=`, `encoding=`: G.711 mu-law / A-law,
16-bit PCM or float at 8 .. 48 kHz): the raw chunks travel at their own width in the same staging block, two more launches
decode and convert them on the device into a packed f32 buffer, and the feed descriptors point at that buffer.  The converted
samples do not depend on how the audio was cut either, so the contract above starts at the wire.
"""
import torch

from . import audio_ingest, feature
from . import lib as _lib
from .multistream import SlotError, check_parts

F32 = torch.float32
HOP, WIN_END = 80, 100                   # frame f reads samples 80 f - 100 .. 80 f + 99
TAIL, RING, NMEL = 200, 32, 23             # per-slot device state of csrc/feature.hip
FB, SPL_ROWS, FEED_N = 64, 16, 9           # log-mel frames per STFT tile, model frames per splice tile, descriptor fields
MODES = {"logmel23": 0, "logmel23_cummn": 2}

FREE, OPEN, ENDED = "free", "open", "ended"


def logmel_frames(n: int, ended: bool) -> int:
    """Log-mel frames computable from n samples: all of them at the end of the stream (feature.logmel's count)."""
    if ended:
        return 1 + n // HOP - (1 if n % HOP == 0 else 0)
    return (n - WIN_END) // HOP + 1 if n >= WIN_END else 0


def model_frames(T: int, ended: bool, ctx: int, sub: int) -> int:
    """Model frames computable from T log-mel frames."""
    if ended:
        return (T + sub - 1) // sub
    return (T - 1 - ctx) // sub + 1 if T - 1 - ctx >= 0 else 0


def ring_start(T: int, j: int, ctx: int, sub: int) -> int:
    """First log-mel frame a later splice still reads, given T frames and j model frames emitted."""
    return max(0, min(T, sub * j - ctx))


class SlotFeed:
    """What one feed does to one slot: samples recv0 -> recv1, log-mel frames f0 -> f1, model frames j0 -> j1, the ring holding
    frames rb0 .. f0 - 1 before and rb1 .. f1 - 1 after."""

    __slots__ = ("slot", "recv0", "recv1", "f0", "f1", "j0", "j1", "rb0", "rb1", "ended")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


class FrontEndTable:
    """Host bookkeeping of the incremental front-end (pure Python, no device): per slot its state free / open / ended and the
    samples received, log-mel frames and model frames emitted.  reset(s) starts an empty stream in any slot; a slot fed its
    end accepts no more audio until the next reset."""

    def __init__(self, slots: int, context_size: int = 7, subsampling: int = 10):
        if slots <= 0:
            raise SlotError("a front-end needs at least one slot")
        if not 0 <= context_size <= 15:
            raise ValueError(f"context_size must be in 0..15, got {context_size}")
        if not 1 <= subsampling <= 16:
            raise ValueError(f"subsampling must be in 1..16, got {subsampling}")
        self.S, self.ctx, self.sub = slots, context_size, subsampling
        self.state = [FREE] * slots
        self.recv = [0] * slots
        self.frames = [0] * slots
        self.mframes = [0] * slots

    def _check(self, s):
        if not isinstance(s, int) or not 0 <= s < self.S:
            raise SlotError(f"slot {s!r} out of range 0..{self.S - 1}")

    def reset(self, s):
        self._check(s)
        self.state[s] = OPEN
        self.recv[s] = self.frames[s] = self.mframes[s] = 0

    def close(self, s):
        self._check(s)
        self.state[s] = FREE

    def plan(self, counts, end=()):
        """counts: {slot: new samples}; end: slots whose audio ends with this call.  -> [SlotFeed] in slot order."""
        counts, end = dict(counts), list(end)
        if len(set(end)) != len(end):
            raise SlotError("a slot is named twice in end")
        for s in list(counts) + end:
            self._check(s)
            if self.state[s] == FREE:
                raise SlotError(f"slot {s} is not open (reset it first)")
            if self.state[s] == ENDED:
                raise SlotError(f"slot {s} was fed its end; reset it to start a new stream")
        for s, n in counts.items():
            if not isinstance(n, int) or n < 0:
                raise ValueError(f"slot {s}: sample count must be a non-negative int, got {n!r}")
        ctx, sub = self.ctx, self.sub
        out = []
        for s in sorted(set(counts) | set(end)):
            ended = s in end
            recv0, f0, j0 = self.recv[s], self.frames[s], self.mframes[s]
            recv1 = recv0 + counts.get(s, 0)
            f1 = logmel_frames(recv1, ended)
            j1 = model_frames(f1, ended, ctx, sub)
            out.append(SlotFeed(slot=s, recv0=recv0, recv1=recv1, f0=f0, f1=f1, j0=j0, j1=j1,
                                rb0=ring_start(f0, j0, ctx, sub), rb1=ring_start(f1, j1, ctx, sub), ended=ended))
        return out

    def commit(self, plan):
        for p in plan:
            self.recv[p.slot], self.frames[p.slot], self.mframes[p.slot] = p.recv1, p.f1, p.j1
            if p.ended:
                self.state[p.slot] = ENDED


class AudioFrontEnd:
    """Incremental `extract_fbank_wave` for `slots` concurrent streams (8 kHz float, or any `sample_rate` / `encoding` of
    `audio_ingest`, decoded and converted on the device):

        fe = AudioFrontEnd(64, "logmel23_cummn")
        fe.reset(s)                                   # an empty stream in slot s
        feats = fe.feed({s: chunk, t: other_chunk})   # {slot: (n, 23 (2 ctx + 1)) f32 device tensor}: its new model frames
        last = fe.feed({s: final_chunk}, end=[s])     # the remaining frames, zero-padded as the batch front-end does

    Slots not named in a call pause.  The concatenated frames of a stream equal extract_fbank_wave of its whole waveform (bit
    for bit with logmel23), however the audio was cut."""

    def __init__(self, slots: int, input_transform: str, context_size: int = 7, subsampling: int = 10, device=None,
                 pad_mode: str = "constant", sample_rate: int = 8000, encoding: str = "f32"):
        if input_transform == "logmel23_mn":
            raise ValueError("logmel23_mn normalises by the mean of the whole recording and cannot be computed incrementally; "
                             "use logmel23 or logmel23_cummn")
        if input_transform not in MODES:
            raise ValueError(f"unsupported input_transform {input_transform!r} (incremental: {sorted(MODES)})")
        if pad_mode != "constant":
            raise ValueError("the incremental front-end supports pad_mode='constant' only (reflect padding needs the samples past "
                             "the end of the stream)")
        audio_ingest.check_encoding(encoding)
        audio_ingest.ratio(sample_rate)
        self.table = FrontEndTable(slots, context_size, subsampling)
        self.S, self.ctx, self.sub = slots, context_size, subsampling
        self.mode = MODES[input_transform]
        self.input_transform = input_transform
        self.width = NMEL * (2 * context_size + 1)
        self.dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.dev.type != "cuda":
            raise _lib.EendHipError("AudioFrontEnd runs on the GPU (no CPU fallback)")
        z = lambda *s_, dt=F32: torch.zeros(*s_, dtype=dt, device=self.dev)
        self.tail = z(slots, TAIL)
        self.ring = z(slots, RING, NMEL)
        self.sums = z(slots, NMEL, dt=torch.float64)
        self.dft, self.melT = feature._tables(self.dev)
        self.sample_rate, self.encoding = sample_rate, encoding
        self.ingest = None                      # 8 kHz float needs none: feed is the three launches alone
        if (sample_rate, encoding) != (audio_ingest.OUT_RATE, "f32"):
            self.ingest = audio_ingest.AudioIngest(slots, sample_rate, encoding, device=self.dev)

    def reset(self, s: int):
        """Start an empty stream in slot s (any state): its device state is ignored until overwritten."""
        self.table.reset(s)
        if self.ingest is not None:
            self.ingest.reset(s)

    def close(self, s: int):
        self.table.close(s)
        if self.ingest is not None:
            self.ingest.close(s)

    def state(self, s: int) -> str:
        return self.table.state[s]

    # ---- a slot's stream leaves / comes back (the "frontend" part of a multistream.StreamSnapshot)
    def _config(self):
        return {"mode": self.mode, "context_size": self.ctx, "subsampling": self.sub}

    def export(self, s: int) -> dict:
        """Slot s's front-end state as plain values and tensors: its device rows (copies) and its table fields."""
        self.table._check(s)
        if self.table.state[s] == FREE:
            raise SlotError(f"slot {s} is not open (reset it first)")
        t = self.table
        part = {"config": self._config(), "tail": self.tail[s].clone(), "ring": self.ring[s].clone(), "sums": self.sums[s].clone(),
                "state": t.state[s], "recv": t.recv[s], "frames": t.frames[s], "mframes": t.mframes[s]}
        if self.ingest is not None:             # config, history row and counters of the stage in front
            part["ingest"] = self.ingest.export(s)
        return part

    def check_part(self, part):
        """SlotError unless `part` is an export of a front-end configured like this one."""
        ok = (isinstance(part, dict) and part.get("config") == self._config() and part.get("state") in (OPEN, ENDED)
              and all(isinstance(part.get(k), int) and part[k] >= 0 for k in ("recv", "frames", "mframes"))
              and all(torch.is_tensor(part.get(k)) and part[k].shape == row.shape[1:] and part[k].dtype == row.dtype
                      for k, row in (("tail", self.tail), ("ring", self.ring), ("sums", self.sums))))
        if not ok:
            raise SlotError("resume: the snapshot's front-end part does not fit this front-end "
                            f"(here {self._config()}, there {part.get('config') if isinstance(part, dict) else part!r})")
        if self.ingest is not None:
            self.ingest.check_part(part.get("ingest"))
        elif "ingest" in part:
            raise SlotError("resume: the snapshot's audio was ingested as "
                            f"{part['ingest'].get('config') if isinstance(part['ingest'], dict) else part['ingest']!r}, this "
                            "front-end takes 8 kHz float samples")

    def adopt(self, s: int, part):
        """Slot s goes on from an exported `part` (checked by check_part): ordinary row copies on the current stream."""
        self.table._check(s)
        for k, rows in (("tail", self.tail), ("ring", self.ring), ("sums", self.sums)):
            rows[s].copy_(part[k], non_blocking=True)
        t = self.table
        t.state[s], t.recv[s], t.frames[s], t.mframes[s] = part["state"], part["recv"], part["frames"], part["mframes"]
        if self.ingest is not None:
            self.ingest.adopt(s, part["ingest"], part["state"])

    @staticmethod
    def _samples(s, w):
        if not isinstance(w, torch.Tensor):
            w = torch.as_tensor(w)
        if not w.is_floating_point():
            raise TypeError(f"slot {s}: expected float samples at 8 kHz, got {w.dtype}")
        if w.dim() != 1:
            raise ValueError(f"slot {s}: expected a 1-D waveform, got shape {tuple(w.shape)}")
        return w

    @torch.no_grad()
    def feed(self, waves=None, end=()):
        """waves: {slot: 1-D tensor (CPU or GPU) of its next samples, float at 8 kHz or as sample_rate / encoding say}; end: slots
        whose audio ends here.  -> {slot: (n, width) f32 device tensor of its new model frames} for every slot named."""
        if self.ingest is not None:
            return self._feed_ingest(waves, end)
        waves = {s: self._samples(s, w) for s, w in dict(waves or {}).items()}
        plan = self.table.plan({s: int(w.numel()) for s, w in waves.items()}, end)
        if not plan:
            return {}
        dev, W = self.dev, self.width
        desc, stft, splice = [], [], []
        keep, host = [], []                     # device chunks to keep alive; (sample offset, CPU chunk) for the staging block
        n_host = y_rows = o_rows = 0
        rows = {}
        for i, p in enumerate(plan):
            w = waves.get(p.slot)
            ptr = 0
            if w is not None and w.numel():
                if w.is_cuda:
                    w = w.to(device=dev, dtype=F32).contiguous()
                    keep.append(w)
                    ptr = w.data_ptr()
                else:
                    host.append((n_host, w.to(F32).contiguous()))
                    ptr = -1 - n_host           # patched to the device address below
                    n_host += w.numel()
            desc.append([ptr, p.recv0, p.recv1, p.f0, p.f1, p.rb0, p.rb1, y_rows, p.slot])
            stft += [[i, f, min(FB, p.f1 - f)] for f in range(p.f0, p.f1, FB)]
            splice += [[i, j, min(SPL_ROWS, p.j1 - j), o_rows + j - p.j0] for j in range(p.j0, p.j1, SPL_ROWS)]
            rows[p.slot] = (o_rows, p.j1 - p.j0)
            y_rows += p.f1 - p.rb0
            o_rows += p.j1 - p.j0
        n_words = FEED_N * len(desc) + 3 * len(stft) + 4 * len(splice)
        nbytes = 8 * n_words + 4 * n_host
        dbuf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        base = dbuf.data_ptr()
        for d in desc:
            if d[0] < 0:
                d[0] = base + 8 * n_words + 4 * (-1 - d[0])
        words = [v for d in desc for v in d] + [v for t in stft for v in t] + [v for t in splice for v in t]
        stage = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)   # a fresh pinned block per call (copied asynchronously)
        stage[:8 * n_words].view(torch.int64).copy_(torch.tensor(words, dtype=torch.int64))
        if n_host:
            samples = stage[8 * n_words:].view(F32)
            for off, w in host:
                samples[off:off + w.numel()].copy_(w)
        dbuf.copy_(stage, non_blocking=True)
        Y = torch.empty(max(y_rows, 1), NMEL, dtype=F32, device=dev)
        out = torch.empty(o_rows, W, dtype=F32, device=dev)
        L = _lib.load()
        _lib.check(L.eend_audio_feed_f32(base, len(desc), base + 8 * FEED_N * len(desc), len(stft),
                                         base + 8 * (FEED_N * len(desc) + 3 * len(stft)), len(splice),
                                         self.tail.data_ptr(), self.ring.data_ptr(), self.sums.data_ptr(), Y.data_ptr(),
                                         out.data_ptr() if o_rows else None, self.mode, self.ctx, self.sub, self.dft.data_ptr(),
                                         self.melT.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "eend_audio_feed_f32")
        self.table.commit(plan)
        del keep
        return {s: out[o:o + n] for s, (o, n) in rows.items()}

    def _feed_ingest(self, waves, end):
        """feed with the ingest in front: both tables planned, the raw chunks at their own width behind both descriptor sets in
        one staging block, the ingest launched into a packed f32 buffer that the feed descriptors point at, both tables
        committed after both calls returned."""
        ing = self.ingest
        waves = {s: ing.samples(s, w) for s, w in dict(waves or {}).items()}
        iplan = ing.table.plan({s: int(w.numel()) for s, w in waves.items()}, end)
        plan = self.table.plan({p.slot: p.out1 - p.out0 for p in iplan}, end)      # the front-end is fed what the ingest makes
        if not plan:
            return {}
        dev, W = self.dev, self.width
        staging = audio_ingest.Staging(dev, ing.dtype, ing.every)
        iwords, ichunk_at, n_itiles, x_at, n_x = ing.stage(iplan, waves, staging)
        x8 = torch.empty(max(n_x, 1), dtype=F32, device=dev)
        desc, stft, splice = [], [], []
        y_rows = o_rows = 0
        rows = {}
        for i, p in enumerate(plan):
            desc.append([x8.data_ptr() + 4 * x_at[p.slot][0], p.recv0, p.recv1, p.f0, p.f1, p.rb0, p.rb1, y_rows, p.slot])
            stft += [[i, f, min(FB, p.f1 - f)] for f in range(p.f0, p.f1, FB)]
            splice += [[i, j, min(SPL_ROWS, p.j1 - j), o_rows + j - p.j0] for j in range(p.j0, p.j1, SPL_ROWS)]
            rows[p.slot] = (o_rows, p.j1 - p.j0)
            y_rows += p.f1 - p.rb0
            o_rows += p.j1 - p.j0
        words = [v for d in desc for v in d] + [v for t in stft for v in t] + [v for t in splice for v in t]
        n_words = len(words)
        _dbuf, base = staging.upload(words + iwords, [n_words + i for i in ichunk_at])
        Y = torch.empty(max(y_rows, 1), NMEL, dtype=F32, device=dev)
        out = torch.empty(o_rows, W, dtype=F32, device=dev)
        ing.launch(base + 8 * n_words, len(iplan), n_itiles, x8)
        _lib.check(_lib.load().eend_audio_feed_f32(base, len(desc), base + 8 * FEED_N * len(desc), len(stft),
                                                   base + 8 * (FEED_N * len(desc) + 3 * len(stft)), len(splice),
                                                   self.tail.data_ptr(), self.ring.data_ptr(), self.sums.data_ptr(), Y.data_ptr(),
                                                   out.data_ptr() if o_rows else None, self.mode, self.ctx, self.sub,
                                                   self.dft.data_ptr(), self.melT.data_ptr(),
                                                   torch.cuda.current_stream(dev).cuda_stream), "eend_audio_feed_f32")
        self.table.commit(plan)
        ing.table.commit(iplan)
        return {s: out[o:o + n] for s, (o, n) in rows.items()}


class AudioStreamSession:
    """Audio in, logits out: an `AudioFrontEnd` in front of an `FsMultiStreamSession` or `LsMultiStreamSession`, slot for slot.

        ses = AudioStreamSession(FsMultiStreamSession(model, slots=64))
        a = ses.open()
        y = ses.push({a: chunk})          # {slot: (k, C) logits} of the frames this audio completed
        y = ses.end([a])                  # the rest of the stream: remaining frames, flush -> {slot: (k, C) logits}
        ses.close(a)

    A `live_rttm.SegmentSession` around either session is served the same way (its segments then follow the audio).
    `push` runs the front-end once for all slots named, then steps the session with step_frames, each step pushing the next
    max_frames feature frames of every slot that still has some (the other slots pause); `end` flushes with the last of
    them; `prefill` gives one slot a backlog of audio through the session's prefill.  `input_transform` defaults to the session's (the reference configs': logmel23 for FS-EEND, logmel23_cummn for
    LS-EEND).  `sample_rate` / `encoding` say how the audio of push, prefill and end arrives (`audio_ingest`): by default float
    samples at 8 kHz, else e.g. 8000 / "mulaw" from a telephone trunk or 48000 / "s16" from a meeting client."""

    def __init__(self, session, input_transform=None, context_size: int = 7, subsampling: int = 10, sample_rate: int = 8000,
                 encoding: str = "f32"):
        self.ses, self.C = session, session.C
        if getattr(session, "sad", False):
            raise ValueError("AudioStreamSession over a SegmentSession with sad=True: the session wants one speech-activity flag "
                             "per model frame, and this wrapper cuts audio into frames itself, so a sample-rate mask has no way "
                             "through it yet; push features and flags to the SegmentSession directly")
        if input_transform is None:
            input_transform = session.input_transform
        self.fe = AudioFrontEnd(session.S, input_transform, context_size, subsampling, device=session.dev, sample_rate=sample_rate,
                                encoding=encoding)
        in_size = session.m._in_size
        if in_size != self.fe.width:
            raise ValueError(f"the model takes {in_size} features per frame, the front-end makes {self.fe.width} "
                             f"(23 x (2 x {context_size} + 1))")

    def open(self) -> int:
        s = self.ses.open()
        self.fe.reset(s)
        return s

    def close(self, s: int):
        self.ses.close(s)
        self.fe.close(s)

    def state(self, s: int) -> str:
        return self.ses.state(s)

    # ---- snapshot / suspend / resume: the wrapped session's, plus the front-end's part for the same slot
    @property
    def parts(self):
        return tuple(self.ses.parts) + ("frontend",)

    def snapshot(self, s: int):
        """The wrapped session's snapshot of slot s with the front-end's state of that slot (sample tail, log-mel ring, running
        sums, counters) as its "frontend" part.  The slot goes on."""
        snap = self.ses.snapshot(s)
        snap.parts["frontend"] = self.fe.export(s)
        return snap

    def suspend(self, s: int):
        snap = self.snapshot(s)
        self.close(s)
        return snap

    def resume(self, snap) -> int:
        """A suspended stream into a free slot -> the slot; the audio goes on at the sample it stopped at.  SlotError, with
        nothing changed, when the snapshot's parts are not this stack's or a part does not fit."""
        check_parts(snap, self.parts)
        return self._resume(snap)

    def _resume(self, snap):
        self.fe.check_part(snap.parts["frontend"])
        s = self.ses._resume(snap)
        self.fe.adopt(s, snap.parts["frontend"])
        return s

    def _collect(self, out, y):
        for s, v in y.items():
            out[s].append(v.reshape(-1, self.C))

    def _run_frames(self, feats, out, flush=()):
        """step_frames in pieces of max_frames; `flush` goes with the last piece (alone when there are no frames)."""
        m = self.ses.max_frames
        n = max([f.shape[0] for f in feats.values()] + [0])
        k = 0
        while True:
            last = k + m >= n
            self._collect(out, self.ses.step_frames(push={s: f[k:k + m] for s, f in feats.items() if k < f.shape[0]},
                                                    flush=flush if last else ()))
            k += m
            if last:
                return

    def _result(self, out):
        z = lambda: torch.zeros(0, self.C, dtype=F32, device=self.ses.dev)
        return {s: torch.cat(v) if v else z() for s, v in out.items()}

    def _check_open(self, slots, what):
        for s in slots:
            self.fe.table._check(s)
            if self.ses.state(s) != "open":
                raise SlotError(f"{what} slot {s}, which is {self.ses.state(s)}")

    @torch.no_grad()
    def push(self, waves):
        """waves: {slot: 1-D tensor of its next samples (float at 8 kHz, or as sample_rate / encoding say)} -> {slot: (k, C)
        logits} of the frames completed."""
        waves = dict(waves)
        self._check_open(waves, "push to")
        feats = self.fe.feed(waves)
        out = {s: [] for s in waves}
        if any(f.shape[0] for f in feats.values()):
            self._run_frames(feats, out)
        return self._result(out)

    @torch.no_grad()
    def prefill(self, s: int, wave):
        """A backlog of audio for open slot s: the front-end once, then the session's prefill with the frames it completed
        (one pass instead of a step_frames loop).  -> (k, C) logits; the slot goes on with push / end."""
        self._check_open([s], "prefill of")
        feats = self.fe.feed({s: wave})[s]
        return self.ses.prefill(s, feats).reshape(-1, self.C)

    @torch.no_grad()
    def end(self, slots, waves=None):
        """The audio of `slots` ends (after the optional last samples in `waves`): their remaining feature frames are pushed,
        then they flush until done.  -> {slot: (k, C) logits} of their last frames."""
        slots = list(slots)
        self._check_open(slots, "end of")
        if waves and not set(waves) <= set(slots):
            raise SlotError("end(slots, waves): every slot in waves must be among the slots that end")
        feats = self.fe.feed(waves, end=slots)
        out = {s: [] for s in slots}
        self._run_frames(feats, out, flush=slots)
        while any(self.ses.state(s) == "flushing" for s in slots):
            self._collect(out, self.ses.step_frames())
        return self._result(out)
