"""Audio in, logits out for live streams: an incremental feature front-end for many streams (csrc/feature.hip
`eend_audio_feed_f32`) and `AudioStreamSession`, which puts it in front of `FsMultiStreamSession` / `LsMultiStreamSession`.

`feature.extract_fbank_wave` needs the whole recording: its frame count and right-edge padding depend on the final length,
the splice pads with zeros past the last frame and `logmel23_cummn` normalises by the running mean of every earlier frame.
Both shipped transforms are causal, so they can be computed as the audio arrives.  Per slot the device keeps the sample tail
(fewer than 200 samples), the fp64 column sums of the running mean and a ring of the last normalised log-mel frames that the
splice of the next model frame reads; the host keeps the counters, which depend on sample counts only (`FrontEndTable`, an
`audio_plan.SlotTable`).  With pad_mode "constant" (first sample of frame f at 80 f - 100, as `feature.logmel`):

    log-mel frame f is ready once 80 f + 100 samples are in;
    model frame j (frames sub j - ctx .. sub j + ctx) once log-mel frame sub j + ctx exists;
    at the end of a stream of n samples the rest follow the batch rules: `audio_plan.stft_frames(n)` log-mel frames, 1 + n // 80
    less the excess last one (zero samples past n), and ceil(n_frames / sub) model frames (zero frames past n_frames).

`logmel23` frames are bit-identical to the batch front-end (the same STFT tile body); `logmel23_cummn` adds the fp64 running
sum strictly in frame order, so its features do not depend on how the audio was cut, and differ from the batch path (which
sums in another order) by about one float ulp of the mean.  One `feed` costs three launches and one host-to-device copy
(`audio_plan.Staging`: the words that `feed_words` builds, then the CPU chunks), whatever the number of slots or the chunk
sizes, and never waits for the device.

Audio that is not 8 kHz float goes through `audio_ingest.AudioIngest` first (`sample_rate=`, `encoding=`: G.711 mu-law / A-law,
16-bit PCM or float at 8 .. 48 kHz): the raw chunks travel at their own width in the same staging block, two more launches
decode and convert them on the device into a packed f32 buffer, and the feed descriptors point at that buffer.  The converted
samples do not depend on how the audio was cut either, so the contract above starts at the wire.
"""
from dataclasses import dataclass

import torch

from . import audio_ingest, feature
from . import lib as _lib
from .audio_plan import ENDED, F32, FB, FEED_N, FREE, HOP, NMEL, OPEN, RING, SPL_ROWS, TAIL, SlotTable, Staging, stft_frames, there
from .multistream import SlotError, check_parts

WIN_END = 100                              # frame f reads samples 80 f - 100 .. 80 f + 99
MODES = {"logmel23": 0, "logmel23_cummn": 2}


def logmel_frames(n: int, ended: bool) -> int:
    """Log-mel frames computable from n samples: all of them at the end of the stream (feature.logmel's count)."""
    if ended:
        return stft_frames(n)
    return (n - WIN_END) // HOP + 1 if n >= WIN_END else 0


def model_frames(T: int, ended: bool, ctx: int, sub: int) -> int:
    """Model frames computable from T log-mel frames."""
    if ended:
        return (T + sub - 1) // sub
    return (T - 1 - ctx) // sub + 1 if T - 1 - ctx >= 0 else 0


def ring_start(T: int, j: int, ctx: int, sub: int) -> int:
    """First log-mel frame a later splice still reads, given T frames and j model frames emitted."""
    return max(0, min(T, sub * j - ctx))


@dataclass(slots=True)
class SlotFeed:
    """What one feed does to one slot: samples recv0 -> recv1, log-mel frames f0 -> f1, model frames j0 -> j1, the ring holding
    frames rb0 .. f0 - 1 before and rb1 .. f1 - 1 after."""
    slot: int
    recv0: int
    recv1: int
    f0: int
    f1: int
    j0: int
    j1: int
    rb0: int
    rb1: int
    ended: bool


class FrontEndTable(SlotTable):
    """Host bookkeeping of the incremental front-end (`audio_plan.SlotTable`): per slot the samples received, log-mel frames
    and model frames emitted."""

    counters = {"recv": "recv1", "frames": "f1", "mframes": "j1"}

    def __init__(self, slots: int, context_size: int = 7, subsampling: int = 10):
        super().__init__(slots, "a front-end")
        if not 0 <= context_size <= 15:
            raise ValueError(f"context_size must be in 0..15, got {context_size}")
        if not 1 <= subsampling <= 16:
            raise ValueError(f"subsampling must be in 1..16, got {subsampling}")
        self.ctx, self.sub = context_size, subsampling

    def advance(self, s, recv1, ended):
        ctx, sub = self.ctx, self.sub
        f0, j0 = self.frames[s], self.mframes[s]
        f1 = logmel_frames(recv1, ended)
        j1 = model_frames(f1, ended, ctx, sub)
        return SlotFeed(s, self.recv[s], recv1, f0, f1, j0, j1, ring_start(f0, j0, ctx, sub), ring_start(f1, j1, ctx, sub), ended)


def feed_words(plan, chunks):
    """The words of one eend_audio_feed_f32 call (host arithmetic only): `plan` a FrontEndTable's, `chunks` the address of each
    planned slot's new samples, in the plan's order.  -> (desc rows of FEED_N, stft tiles {descriptor, first frame, frames <=
    FB}, splice tiles {descriptor, first model frame, rows <= SPL_ROWS, output row}, {slot: (first output row, rows)}, y_rows,
    o_rows).  A slot's region of the scratch Y starts at its y row with its ring frames rb0 .. f0 - 1, then its new frames."""
    desc, stft, splice, rows = [], [], [], {}
    y_rows = o_rows = 0
    for i, (p, ptr) in enumerate(zip(plan, chunks)):
        desc.append([ptr, p.recv0, p.recv1, p.f0, p.f1, p.rb0, p.rb1, y_rows, p.slot])
        stft += [[i, f, min(FB, p.f1 - f)] for f in range(p.f0, p.f1, FB)]
        splice += [[i, j, min(SPL_ROWS, p.j1 - j), o_rows + j - p.j0] for j in range(p.j0, p.j1, SPL_ROWS)]
        rows[p.slot] = (o_rows, p.j1 - p.j0)
        y_rows += p.f1 - p.rb0
        o_rows += p.j1 - p.j0
    return desc, stft, splice, rows, y_rows, o_rows


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

    def _rows(self):
        return {"tail": self.tail, "ring": self.ring, "sums": self.sums}

    def export(self, s: int) -> dict:
        """Slot s's front-end state as plain values and tensors: its device rows (copies) and its table fields."""
        part = self.table.export(s, self._config(), self._rows())
        part["state"] = self.table.state[s]
        if self.ingest is not None:             # config, history row and counters of the stage in front
            part["ingest"] = self.ingest.export(s)
        return part

    def check_part(self, part):
        """SlotError unless `part` is an export of a front-end configured like this one."""
        if not (self.table.fits(part, self._config(), self._rows()) and part.get("state") in (OPEN, ENDED)):
            raise SlotError(f"resume: the snapshot's front-end part does not fit this front-end (here {self._config()}, "
                            f"there {there(part)!r})")
        if self.ingest is not None:
            self.ingest.check_part(part.get("ingest"))
        elif "ingest" in part:
            raise SlotError(f"resume: the snapshot's audio was ingested as {there(part['ingest'])!r}, this front-end takes 8 kHz "
                            "float samples")

    def adopt(self, s: int, part):
        """Slot s goes on from an exported `part` (checked by check_part): ordinary row copies on the current stream."""
        self.table.adopt(s, part, self._rows(), part["state"])
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
        whose audio ends here.  -> {slot: (n, width) f32 device tensor of its new model frames} for every slot named.

        With an ingest in front both tables are planned, the raw chunks travel at their own width behind both sets of words in
        the one staging block, the ingest is launched into a packed f32 buffer that the feed descriptors point at, and both
        tables are committed after both calls returned."""
        ing, dev = self.ingest, self.dev
        waves = {s: (self._samples if ing is None else ing.samples)(s, w) for s, w in dict(waves or {}).items()}
        counts = {s: int(w.numel()) for s, w in waves.items()}
        if ing is not None:
            iplan = ing.table.plan(counts, end)
            counts = {p.slot: p.out1 - p.out0 for p in iplan}      # the front-end is fed what the ingest makes
        plan = self.table.plan(counts, end)
        if not plan:
            return {}
        if ing is None:
            staging = Staging(dev, F32)
            chunks, iwords, ichunk_at = [staging.place(waves.get(p.slot)) for p in plan], [], []
        else:
            staging = Staging(dev, ing.dtype)
            iwords, ichunk_at, n_itiles, x_at, n_x = audio_ingest.stage(iplan, waves, staging)
            x8 = torch.empty(max(n_x, 1), dtype=F32, device=dev)
            chunks = [x8.data_ptr() + 4 * x_at[p.slot][0] for p in plan]
        desc, stft, splice, rows, y_rows, o_rows = feed_words(plan, chunks)
        words = [v for part in (desc, stft, splice) for row in part for v in row]
        n_words = len(words)
        chunk_at = list(range(0, FEED_N * len(desc), FEED_N)) + [n_words + i for i in ichunk_at]
        _dbuf, base = staging.upload(words + iwords, chunk_at)
        Y = torch.empty(max(y_rows, 1), NMEL, dtype=F32, device=dev)
        out = torch.empty(o_rows, self.width, dtype=F32, device=dev)
        if ing is not None:
            ing.launch(base + 8 * n_words, len(iplan), n_itiles, x8)
        _lib.check(_lib.load().eend_audio_feed_f32(base, len(desc), base + 8 * FEED_N * len(desc), len(stft),
                                                   base + 8 * (FEED_N * len(desc) + 3 * len(stft)), len(splice),
                                                   self.tail.data_ptr(), self.ring.data_ptr(), self.sums.data_ptr(), Y.data_ptr(),
                                                   out.data_ptr() if o_rows else None, self.mode, self.ctx, self.sub,
                                                   self.dft.data_ptr(), self.melT.data_ptr(),
                                                   torch.cuda.current_stream(dev).cuda_stream), "eend_audio_feed_f32")
        self.table.commit(plan)
        if ing is not None:
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
