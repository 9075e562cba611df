"""Live RTTM segments for many streams: `SegmentTracker` (csrc/segtrack.hip `eend_segtrack_feed_f32`) and `SegmentSession`,
which runs it behind an `FsMultiStreamSession` / `LsMultiStreamSession` frame step.

`postproc.make_rttm` needs the whole recording, but its three steps are causal up to a fixed look-ahead: the threshold is per
frame, the zero-padded median of k frames reads h = k // 2 frames ahead, and a change point of a speaker track at frame u
depends on the filtered decisions of u - 1 and u only.  So the filtered decision of frame u, and a segment start or end at u,
is final once frame u + h has arrived, or once the stream has ended (zeros past the end).  Per (slot, track) the device keeps
the last k - 1 raw decisions as a bit word and the start of the open segment; per slot a frame counter and a bounded ring of
closed segments (track, start, end).  The segments of a stream, collected by `poll` and fed its end, are exactly make_rttm's
over the concatenated rows, however the rows were cut and whatever the other slots did.

One `feed` is one launch (and one small descriptor copy for the ragged form); `feed_rows` reads the per-slot row counts from
device memory, so a session's own decoder-append mask drives it with no host work.  `poll` is one device-to-host copy.

With `sad=True` the raw decisions are first fused with an external speech-activity mask, one flag per row, as
`postproc.sad_func` / `make_rttm(sad=)` do for a whole file (LS-EEND/sad_post_process.py:23-33): rows the mask calls non-speech
are cleared, and a speech row in which no track passed the threshold gets the track with the largest value.  The flags of a
`feed` travel in its descriptor block; a `SegmentSession` keeps, per slot, the flags of the frames pushed but not yet emitted.
"""

import torch

from . import lib as _lib
from . import ops
from .multistream import SlotError, check_parts
from .postproc import rttm_lines

F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8
HDR = ops.SEGTRACK_HDR                          # box row: frames, count, overflow, 0, then cap x (track, start, end)
MAX_MEDIAN, MAX_TRACKS = 63, 64

FREE, OPEN, ENDED = "free", "open", "ended"


def check_params(ntracks, col0, threshold, median, capacity):
    """The tracker's parameter domain (also checked by the C ABI): odd 1 <= median <= 63, 1 <= ntracks <= 64, col0 >= 0."""
    if not isinstance(median, int) or median < 1 or median > MAX_MEDIAN or median % 2 == 0:
        raise ValueError(f"median must be odd and in 1..{MAX_MEDIAN}, got {median!r}")
    if not isinstance(ntracks, int) or not 1 <= ntracks <= MAX_TRACKS:
        raise ValueError(f"ntracks must be in 1..{MAX_TRACKS}, got {ntracks!r}")
    if not isinstance(col0, int) or col0 < 0:
        raise ValueError(f"col0 must be a non-negative int, got {col0!r}")
    if not isinstance(capacity, int) or capacity < 1:
        raise ValueError(f"capacity must be a positive int, got {capacity!r}")
    if not isinstance(threshold, (int, float)) or threshold != threshold:
        raise ValueError(f"threshold must be a number, got {threshold!r}")


def host_flags(flags, n, what):
    """Speech-activity flags given as a host sequence, a scalar (n = 1) or a tensor -> a list of n ints 0 / 1 (non-zero:
    speech); SlotError when there are not exactly n."""
    if torch.is_tensor(flags):
        flags = flags.reshape(-1).tolist()
    elif isinstance(flags, (bool, int, float)):
        flags = [flags]
    try:
        out = [1 if f != 0 else 0 for f in flags]
    except TypeError:
        raise SlotError(f"{what}: expected {n} speech-activity flag(s), got {flags!r}") from None
    if len(out) != n:
        raise SlotError(f"{what}: {n} row(s) need {n} speech-activity flag(s), got {len(out)}")
    return out


def tracker_config(ntracks, col0, threshold, median, is_prob, capacity, sad=False):
    """The "config" of a tracker's snapshot part.  A plain tracker's keeps the keys it always had, so parts saved before the
    speech-activity mask existed still fit; a tracker with the mask adds "sad": True, and neither resumes the other's."""
    cfg = {"ntracks": ntracks, "col0": col0, "threshold": threshold, "median": median, "is_prob": is_prob, "capacity": capacity}
    if sad:
        cfg["sad"] = True
    return cfg


class FlagFifo:
    """Host side of a SegmentSession with a speech-activity mask (pure Python, no device): per slot, the flags of the frames
    pushed whose output rows the session has not emitted yet, oldest first.  `check` validates a step's flags without changing
    anything; `push` and `pop` run after the wrapped step has."""

    def __init__(self, slots):
        self.S = slots
        self.q = [[] for _ in range(slots)]

    def clear(self, s):
        self.q[s] = []

    def check(self, frames, sad):
        """frames: {slot: frames it pushes in this step}, sad: {slot: their flags} -> {slot: flags as a list of 0 / 1}.
        SlotError unless every slot that pushes frames has one flag per frame and no other slot has any."""
        sad = dict(sad or {})
        extra = sorted(s for s in sad if s not in frames)
        if extra:
            raise SlotError(f"speech-activity flags for slot(s) {extra}, which bring no frames in this call")
        out = {}
        for s, n in frames.items():
            if s not in sad:
                if n:
                    raise SlotError(f"slot {s}: {n} frame(s) without speech-activity flags")
                continue
            out[s] = host_flags(sad[s], n, f"slot {s}")
        return out

    def push(self, flags):
        for s, f in flags.items():
            self.q[s] += f

    def pop(self, emitted):
        """emitted: {slot: rows it emitted} -> {slot: the flags of those rows}, which leave the queue."""
        for s, m in emitted.items():
            assert len(self.q[s]) >= m, f"slot {s} emitted {m} row(s) with {len(self.q[s])} flag(s) waiting"
        out = {}
        for s, m in emitted.items():
            out[s] = self.q[s][:m]
            del self.q[s][:m]
        return out

    def export(self, s):
        return list(self.q[s])

    @staticmethod
    def fits(v):
        return isinstance(v, (list, tuple)) and all(isinstance(f, int) and f in (0, 1) for f in v)

    def adopt(self, s, v):
        self.q[s] = [int(f) for f in v]


class SegmentLog:
    """Host side of a tracker (pure Python, no device): slot states free / open / ended, the segments each stream has closed so
    far, the segments no poll has returned yet, and the decoding of a copied box (int32 rows of HDR + 3 cap words)."""

    def __init__(self, slots, ntracks, capacity):
        if slots <= 0:
            raise SlotError("a tracker needs at least one slot")
        self.S, self.ntracks, self.cap = slots, ntracks, capacity
        self.state = [OPEN] * slots
        self.segs = [[] for _ in range(slots)]
        self.overflowed = [False] * slots
        self.unreported = set()                 # overflowed slots that poll has not raised for yet
        self.pending = {}                       # slot -> segments taken from the device that poll has not returned yet

    def check(self, s):
        if not isinstance(s, int) or not 0 <= s < self.S:
            raise SlotError(f"slot {s!r} out of range 0..{self.S - 1}")

    def reset(self, s):
        self.check(s)
        self.state[s], self.segs[s], self.overflowed[s] = OPEN, [], False
        self.unreported.discard(s)
        self.pending.pop(s, None)

    def close(self, s):
        self.check(s)
        self.state[s], self.segs[s], self.overflowed[s] = FREE, [], False
        self.unreported.discard(s)
        self.pending.pop(s, None)

    def export(self, s):
        """Slot s's host fields, as plain values."""
        self.check(s)
        if self.state[s] == FREE:
            raise SlotError(f"slot {s} is not open")
        return {"state": self.state[s], "segs": list(self.segs[s]), "pending": list(self.pending.get(s, [])),
                "overflowed": self.overflowed[s], "unreported": s in self.unreported}

    def adopt(self, s, f):
        self.reset(s)
        triples = lambda v: [tuple(int(x) for x in seg) for seg in v]
        self.state[s], self.segs[s], self.overflowed[s] = f["state"], triples(f["segs"]), bool(f["overflowed"])
        if f["pending"]:
            self.pending[s] = triples(f["pending"])
        if f["unreported"]:
            self.unreported.add(s)

    def check_feed(self, slots, end):
        slots, end = list(slots), list(end)
        if len(set(slots)) != len(slots) or len(set(end)) != len(end):
            raise SlotError("a slot is named twice")
        for s in slots + end:
            self.check(s)
            if self.state[s] != OPEN:
                raise SlotError(f"feed to slot {s}, which is {self.state[s]} (reset it to start a new stream)")

    def ended(self, slots):
        for s in slots:
            self.state[s] = ENDED

    def take(self, box):
        """box: int32 (S, HDR + 3 cap) as copied from the device (whose counts are then zeroed): the new segments of every slot
        join its stream's segments and its pending ones; slots whose ring overflowed are marked (overflowed, unreported)."""
        counts = box[:, 1].tolist()
        flags = box[:, 2].tolist()
        for s in range(self.S):
            if self.state[s] == FREE:
                continue
            c = counts[s]
            if c:
                v = box[s, HDR:HDR + 3 * c].tolist()
                new = [(v[i], v[i + 1], v[i + 2]) for i in range(0, 3 * c, 3)]
                self.segs[s].extend(new)
                self.pending.setdefault(s, []).extend(new)
            if flags[s]:
                self.overflowed[s] = True
                self.unreported.add(s)

    def pop_pending(self):
        """-> {slot: [(spk, start, end), ...]} taken since the last call, in slot order; none are returned twice."""
        out = {s: self.pending[s] for s in sorted(self.pending)}
        self.pending = {}
        return out

    def by_track(self, s):
        """Slot s's segments so far, per track in frame order (the ring is ordered by end frame)."""
        per = [[] for _ in range(self.ntracks)]
        for spk, a, b in self.segs[s]:
            per[spk].append((a, b))
        return per


class SegmentTracker:
    """Incremental make_rttm for `slots` concurrent streams of model outputs:

        tr = SegmentTracker(64, ntracks=10)            # columns 1..10 of the logits, median 11, threshold 0.5
        tr.reset(s)                                    # an empty stream in slot s
        tr.feed({s: L_new, t: L_other})                # (n, C) logits rows (device), any number per call
        tr.feed({s: L_last}, end=[s])                  # the stream ends: the last median // 2 frames are finalised
        new = tr.poll()                                # {slot: [(spk, start, end), ...]} closed since the last poll
        tr.rttm(s, "rec")                              # make_rttm's dict of every line of the stream so far

    Slots start open and empty.  `threshold` and `is_prob` follow make_rttm(rec, sigmoid(L[:, col0:col0 + ntracks])):
    logits are thresholded as torch.sigmoid(x) > threshold, probabilities (is_prob) as x > threshold.

    With sad=True every row comes with a flag of an external speech-activity mask (non-zero: speech), and the stream's segments
    are those of make_rttm(..., sad=flags): `feed(rows, end, sad={slot: flags})`, one flag per row of every slot that brings
    rows (a host sequence or a tensor), or `feed_rows(..., sad=flags_dev)`.  In logits mode the largest value of a row is taken
    over the raw logits of the tracked columns."""

    def __init__(self, slots: int, ntracks: int, col0: int = 1, threshold: float = 0.5, median: int = 11, capacity: int = 256,
                 is_prob: bool = False, device=None, sad: bool = False):
        check_params(ntracks, col0, threshold, median, capacity)
        self.sad = bool(sad)
        self.fifo = FlagFifo(slots) if self.sad else None               # a SegmentSession's flags pushed but not yet emitted
        self.log = SegmentLog(slots, ntracks, capacity)
        self.S, self.ntracks, self.col0, self.cap = slots, ntracks, col0, capacity
        self.threshold, self.median, self.is_prob = float(threshold), median, bool(is_prob)
        self.dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.dev.type != "cuda":
            raise _lib.EendHipError("SegmentTracker runs on the GPU (no CPU fallback)")
        self.hist = torch.zeros(slots, 64, dtype=I64, device=self.dev)
        self.open_ = torch.full((slots, 64), -1, dtype=I32, device=self.dev)
        self.box = torch.zeros(slots, HDR + 3 * capacity, dtype=I32, device=self.dev)
        self._rows = None                       # (data_ptr, ld, desc) of the last feed_rows matrix
        self._sad_rows = None                   # (data_ptr, rows_per_slot, desc) of the last feed_rows flags

    @property
    def lookahead(self) -> int:
        """Frames of look-ahead before a decision is final (median // 2)."""
        return self.median // 2

    # ---- slots
    def reset(self, s: int):
        """Start an empty stream in slot s (any state); its unpolled segments are dropped."""
        self.log.reset(s)
        self.box[s, :3] = 0
        if self.sad:
            self.fifo.clear(s)

    def close(self, s: int):
        """Drop slot s's stream: its device state, its unpolled segments and the lines collected so far."""
        self.log.close(s)
        self.box[s, :3] = 0
        if self.sad:
            self.fifo.clear(s)

    def state(self, s: int) -> str:
        return self.log.state[s]

    # ---- a slot's stream leaves / comes back (the "tracker" part of a multistream.StreamSnapshot)
    def _config(self):
        return tracker_config(self.ntracks, self.col0, self.threshold, self.median, self.is_prob, self.cap, self.sad)

    def export(self, s: int) -> dict:
        """Slot s's tracker state as plain values and tensors: its device rows (copies; the segments no poll has taken yet
        travel in the box row) and its host fields; with sad, also the flags pushed but not yet emitted ("fifo")."""
        part = self.log.export(s)
        part.update(config=self._config(), hist=self.hist[s].clone(), open=self.open_[s].clone(), box=self.box[s].clone())
        if self.sad:
            part["fifo"] = self.fifo.export(s)
        return part

    def check_part(self, part):
        """SlotError unless `part` is an export of a tracker configured like this one."""
        ok = (isinstance(part, dict) and part.get("config") == self._config() and part.get("state") in (OPEN, ENDED)
              and all(isinstance(part.get(k), (list, tuple)) for k in ("segs", "pending"))
              and all(torch.is_tensor(part.get(k)) and part[k].shape == row.shape[1:] and part[k].dtype == row.dtype
                      for k, row in (("hist", self.hist), ("open", self.open_), ("box", self.box))))
        if ok and self.sad:
            ok = FlagFifo.fits(part.get("fifo"))
        if not ok:
            raise SlotError("resume: the snapshot's tracker part does not fit this tracker "
                            f"(here {self._config()}, there {part.get('config') if isinstance(part, dict) else part!r})")

    def adopt(self, s: int, part):
        """Slot s goes on from an exported `part` (checked by check_part): ordinary row copies on the current stream."""
        self.log.adopt(s, part)
        for k, rows in (("hist", self.hist), ("open", self.open_), ("box", self.box)):
            rows[s].copy_(part[k], non_blocking=True)
        if self.sad:
            self.fifo.adopt(s, part["fifo"])

    # ---- feeding
    def _launch(self, desc, counts, ends, n, ld, sad_desc=None):
        ops.segtrack_feed(desc, counts, ends, n, ld, self.col0, self.ntracks, self.threshold, self.median, self.is_prob, self.hist,
                          self.open_, self.box, self.cap, sad_desc)

    def _check_sad(self, rows, sad):
        """The flags of a feed: {slot: n flags as a list} for every slot that brings n > 0 rows; SlotError otherwise."""
        if not self.sad:
            if sad is not None:
                raise SlotError("speech-activity flags given to a tracker built without sad=True")
            return None
        return self.fifo.check({s: x.shape[0] for s, x in rows.items()}, sad)

    def _rows_f32(self, s, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise _lib.EendHipError(f"slot {s}: expected a GPU tensor (the HIP path has no CPU fallback)")
        if x.dim() == 3 and x.shape[0] == 1:
            x = x[0]
        if x.dim() != 2:
            raise ValueError(f"slot {s}: expected (n, C) rows, got shape {tuple(x.shape)}")
        return x.to(F32).contiguous()

    @torch.no_grad()
    def feed(self, rows=None, end=(), sad=None):
        """rows: {slot: (n, C) device tensor of its next rows}; end: slots whose stream ends after these rows.  Every tensor of a
        call has the same C >= col0 + ntracks.  One descriptor copy, one launch; nothing waits for the device.  A tracker built
        with sad=True also takes sad: {slot: n flags} for every slot that brings rows; they travel in the descriptor block."""
        rows = {s: self._rows_f32(s, x) for s, x in dict(rows or {}).items()}
        end = list(end)
        self.log.check_feed(rows.keys(), end)
        sad = self._check_sad(rows, sad)
        slots = sorted(set(rows) | set(end))
        if not slots:
            return
        cols = {x.shape[1] for x in rows.values()}
        if len(cols) > 1:
            raise ValueError(f"every tensor of a feed needs the same number of columns, got {sorted(cols)}")
        if cols and min(cols) < self.col0 + self.ntracks:
            raise ValueError(f"rows have {min(cols)} columns, the tracker reads columns {self.col0}..{self.col0 + self.ntracks - 1}")
        ld = next(iter(cols)) if cols else self.col0 + self.ntracks
        n = len(slots)
        desc = [[rows[s].data_ptr() if s in rows and rows[s].shape[0] else self.box.data_ptr(), s] for s in slots]
        if self.sad:
            self._feed_sad(rows, end, sad, slots, desc, ld)
            return
        stage = torch.empty(4 * n + 2 * n, dtype=I32, pin_memory=True)   # a fresh pinned block per call (copied asynchronously)
        stage[:4 * n].view(I64).copy_(torch.tensor(desc, dtype=I64).reshape(-1))
        stage[4 * n:5 * n].copy_(torch.tensor([rows[s].shape[0] if s in rows else 0 for s in slots], dtype=I32))
        stage[5 * n:].copy_(torch.tensor([1 if s in end else 0 for s in slots], dtype=I32))
        dbuf = torch.empty(6 * n, dtype=I32, device=self.dev)
        dbuf.copy_(stage, non_blocking=True)
        self._launch(dbuf[:4 * n].view(I64), dbuf[4 * n:5 * n], dbuf[5 * n:], n, ld)
        self.log.ended(end)

    def _feed_sad(self, rows, end, sad, slots, desc, ld):
        """feed's block with the flags behind it: int32 words [desc 4n | flag addresses 2n | counts n | ends n | flags, one byte
        per row, each slot's run after the other].  Still one copy and one launch."""
        n = len(slots)
        flags, off = [], []
        for s in slots:
            off.append(len(flags))
            flags += sad.get(s, [])
        words = 8 * n + (len(flags) + 3) // 4
        dbuf = torch.empty(words, dtype=I32, device=self.dev)
        base = dbuf.data_ptr() + 32 * n
        stage = torch.zeros(words, dtype=I32, pin_memory=True)
        stage[:4 * n].view(I64).copy_(torch.tensor(desc, dtype=I64).reshape(-1))
        stage[4 * n:6 * n].view(I64).copy_(torch.tensor([base + o for o in off], dtype=I64))
        stage[6 * n:7 * n].copy_(torch.tensor([rows[s].shape[0] if s in rows else 0 for s in slots], dtype=I32))
        stage[7 * n:8 * n].copy_(torch.tensor([1 if s in end else 0 for s in slots], dtype=I32))
        if flags:
            stage[8 * n:].view(U8)[:len(flags)].copy_(torch.tensor(flags, dtype=U8))
        dbuf.copy_(stage, non_blocking=True)
        self._launch(dbuf[:4 * n].view(I64), dbuf[6 * n:7 * n], dbuf[7 * n:8 * n], n, ld, dbuf[4 * n:6 * n].view(I64))
        self.log.ended(end)

    @torch.no_grad()
    def feed_rows(self, x, counts_dev, rows_per_slot=1, sad=None):
        """The session form: row s of x ((S, C) or (S, 1, C) f32 device tensor, rows contiguous) is slot s's next row when
        counts_dev[s] (device int32 [S]) is 1.  With rows_per_slot = n, x is (S, n, C) and slot s takes its first counts_dev[s]
        (0..n) rows.  No host data, one launch; the host does not check slot states here.  A tracker built with sad=True also
        takes sad: a contiguous uint8 (S, rows_per_slot) device tensor, the flag of row j of slot s at [s, j]."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != F32 or not x.is_contiguous():
            raise _lib.EendHipError("feed_rows: expected a contiguous f32 GPU tensor")
        if not isinstance(rows_per_slot, int) or rows_per_slot < 1:
            raise ValueError(f"feed_rows: rows_per_slot must be a positive int, got {rows_per_slot!r}")
        if self.sad != (sad is not None):
            raise SlotError("feed_rows: speech-activity flags go with a tracker built with sad=True, and only with it")
        if self.sad and (not isinstance(sad, torch.Tensor) or not sad.is_cuda or sad.dtype != U8 or not sad.is_contiguous()
                         or sad.numel() != self.S * rows_per_slot):
            raise SlotError(f"feed_rows: sad must be a contiguous uint8 GPU tensor of {self.S} x {rows_per_slot} flags")
        x2 = x.reshape(x.shape[0] * rows_per_slot, -1) if x.shape[0] == self.S else x.reshape(x.shape[0], -1)
        if x2.shape[0] != self.S * rows_per_slot:
            raise ValueError(f"feed_rows: {rows_per_slot} row(s) per slot ({self.S}), got {x2.shape[0]}")
        ld = x2.shape[1]
        if ld < self.col0 + self.ntracks:
            raise ValueError(f"rows have {ld} columns, the tracker reads columns {self.col0}..{self.col0 + self.ntracks - 1}")
        key = (x2.data_ptr(), ld, rows_per_slot)
        if self._rows is None or self._rows[0] != key:
            desc = torch.tensor([[key[0] + 4 * rows_per_slot * ld * s, s] for s in range(self.S)], dtype=I64).to(self.dev)
            self._rows = (key, desc)
        if self.sad:
            skey = (sad.data_ptr(), rows_per_slot)
            if self._sad_rows is None or self._sad_rows[0] != skey:
                self._sad_rows = (skey, torch.tensor([skey[0] + rows_per_slot * s for s in range(self.S)], dtype=I64).to(self.dev))
            self._launch(self._rows[1], counts_dev, None, self.S, ld, self._sad_rows[1])
            return
        self._launch(self._rows[1], counts_dev, None, self.S, ld)

    def end(self, slots):
        """The streams of `slots` end (no more rows): their last median // 2 decisions are finalised, open segments close."""
        self.feed(end=slots)

    # ---- reading
    def _drain(self):
        box = self.box.cpu()                    # one device-to-host copy (waits for the work queued before it)
        self.box[:, 1:3] = 0
        self.log.take(box)

    def poll(self):
        """-> {slot: [(spk, start, end), ...]} of the segments closed since the last poll, by end frame then track (frames of
        the model's output rate, end exclusive).  A slot whose ring overflowed raises EendHipError naming it; the segments of
        the other slots are kept (rttm) and attached to the exception as `.segments`.  rttm() reads the device rings too; what it
        takes is still returned by the next poll."""
        self._drain()
        out = self.log.pop_pending()
        bad = sorted(self.log.unreported)
        self.log.unreported.clear()
        if bad:
            err = _lib.EendHipError(f"segment ring overflowed in slot(s) {bad}: more than {self.cap} segments closed between polls "
                                    "(poll more often or raise capacity); their lines are incomplete")
            err.segments, err.slots = out, bad
            raise err
        return out

    def active(self, s: int):
        """{spk: start frame} of slot s's segments whose start is final and whose end is not."""
        self.log.check(s)
        st = self.open_[s, :self.ntracks].cpu().tolist()
        if int(self.box[s, 0]) == 0:
            return {}
        return {k: v for k, v in enumerate(st) if v >= 0}

    def rttm(self, s: int, rec: str, frame_shift=80, subsampling=10, sampling_rate=8000):
        """Every line of slot s's stream so far, as make_rttm's dict: the same keys, order and strings.  The segments it copies
        from the device (of every slot) stay pending for the next poll."""
        self.log.check(s)
        self._drain()
        if self.log.overflowed[s]:
            raise _lib.EendHipError(f"segment ring of slot {s} overflowed: its lines are incomplete")
        return rttm_lines(rec, self.log.by_track(s), frame_shift, subsampling, sampling_rate)


class SegmentSession:
    """An FsMultiStreamSession / LsMultiStreamSession with live segments: the session's interface unchanged, plus poll / active
    / rttm per slot.

        ses = SegmentSession(FsMultiStreamSession(model, slots=64))    # tracker over logits columns 1..C-1
        a = ses.open()
        ses.step(push={a: x_t})                 # the session's own result; the tracker reads the rows it emitted
        ses.poll()                              # {slot: [(spk, start, end), ...]} closed since the last poll
        ses.rttm(a, "rec")                      # make_rttm's lines of the stream so far

    After a step that emitted logits, one tracker launch reads the rows the session emitted (`emitted()`: its logits rows
    with the per-slot emitted row counts on the device, no host work); slots that turned done in a step are ended.
    tracker_kw go to SegmentTracker (col0 = 1 and ntracks = C - col0 by default).

    With sad=True every pushed frame comes with a flag of an external speech-activity mask: `step(push, flush, sad={slot:
    flag})`, `step_frames(push, flush, sad={slot: flags of its pushed frames})`, `prefill(s, feats, sad=flags)`.  Output row u
    of a slot belongs to its input frame u and is emitted conv_delay pushes later, so the flags wait in a per-slot host FIFO;
    after a step each slot's emitted rows take the oldest flags (one asynchronous copy of an (S, n) uint8 block, then the
    tracker's launch).  The stream's lines are make_rttm(rec, sigmoid(L[:, 1:]), sad=flags) over its logits L."""

    def __init__(self, session, sad: bool = False, **tracker_kw):
        self.ses = session
        self.sad = bool(sad)
        self._flags = {}                        # rows per slot -> the (S, n) uint8 device block the tracker reads
        self.S, self.C, self.dev, self.m = session.S, session.C, session.dev, session.m
        self.max_frames, self.input_transform = session.max_frames, session.input_transform
        kw = dict(tracker_kw)
        col0 = kw.setdefault("col0", 1)
        kw.setdefault("ntracks", self.C - col0)
        self.tracker = SegmentTracker(self.S, device=self.dev, sad=self.sad, **kw)

    def open(self) -> int:
        s = self.ses.open()
        self.tracker.reset(s)
        return s

    def close(self, s: int):
        self.ses.close(s)
        self.tracker.close(s)

    def state(self, s: int) -> str:
        return self.ses.state(s)

    # ---- snapshot / suspend / resume: the wrapped session's, plus the tracker's part for the same slot
    @property
    def parts(self):
        return tuple(self.ses.parts) + ("tracker",)

    def snapshot(self, s: int):
        """The wrapped session's snapshot of slot s with the tracker's state of that slot (decision history, open segments,
        segment ring, the lines collected so far and the segments no poll has returned) as its "tracker" part.  The slot goes on."""
        snap = self.ses.snapshot(s)
        snap.parts["tracker"] = self.tracker.export(s)
        return snap

    def suspend(self, s: int):
        snap = self.snapshot(s)
        self.close(s)
        return snap

    def resume(self, snap) -> int:
        """A suspended stream into a free slot -> the slot; its segments go on across the cut (an open one included), and
        rttm / poll return what the uninterrupted stream's would.  SlotError, with nothing changed, when the snapshot's parts
        are not this stack's or a part does not fit."""
        check_parts(snap, self.parts)
        return self._resume(snap)

    def _resume(self, snap):
        self.tracker.check_part(snap.parts["tracker"])
        s = self.ses._resume(snap)
        self.tracker.adopt(s, snap.parts["tracker"])
        return s

    def _pushed_flags(self, frames, sad):
        """frames: {slot: frames it pushes in this step}; -> {slot: their flags as a list}.  SlotError, before anything ran,
        unless every pushing slot has one flag per frame and no other slot has any (a plain session takes none at all)."""
        if not self.sad:
            if sad is not None:
                raise SlotError("speech-activity flags given to a session built without sad=True")
            return None
        return self.tracker.fifo.check(frames, sad)

    def _emitted_flags(self, out, n):
        """The flags of the rows a step emitted (out: its result), oldest first per slot, as the (S, n) uint8 device block of
        that row count: one asynchronous copy from a fresh pinned block."""
        rows = [[0] * n for _ in range(self.S)]
        for s, f in self.tracker.fifo.pop({s: v.shape[1] for s, v in out.items()}).items():
            rows[s][:len(f)] = f
        stage = torch.empty(self.S, n, dtype=U8, pin_memory=self.dev.type == "cuda")
        stage.copy_(torch.tensor(rows, dtype=U8))
        if n not in self._flags:
            self._flags[n] = torch.zeros(self.S, n, dtype=U8, device=self.dev)
        self._flags[n].copy_(stage, non_blocking=True)
        return self._flags[n]

    def _step(self, step, push, flush, flags=None):
        before = [self.ses.state(s) for s in range(self.S)]
        out = step(push=push, flush=flush)
        if self.sad:
            self.tracker.fifo.push(flags)
        if out:                                 # a replay happened: the tracker reads its emitted rows
            logits, counts, n = self.ses.emitted()
            if self.sad:
                self.tracker.feed_rows(logits, counts, rows_per_slot=n, sad=self._emitted_flags(out, n))
            else:
                self.tracker.feed_rows(logits, counts, rows_per_slot=n)
        done = [s for s in range(self.S) if before[s] != "done" and self.ses.state(s) == "done"]
        if done:
            if self.sad:
                assert not any(self.tracker.fifo.q[s] for s in done), "a finished stream has flags left"
            self.tracker.end(done)
        return out

    @torch.no_grad()
    def step(self, push=None, flush=(), sad=None):
        flags = self._pushed_flags({s: 1 for s in dict(push or {})}, sad)
        return self._step(self.ses.step, push, flush, flags)

    @torch.no_grad()
    def step_frames(self, push=None, flush=(), sad=None):
        frames = {}
        if self.sad:
            for s, x in dict(push or {}).items():
                if not torch.is_tensor(x):
                    raise SlotError(f"push to slot {s}: expected a tensor of features")
                frames[s] = x.numel() // self.m._in_size
        flags = self._pushed_flags(frames, sad)
        return self._step(self.ses.step_frames, push, flush, flags)

    @torch.no_grad()
    def prefill(self, s: int, feats, sad=None):
        """The session's prefill of slot s; the rows it emitted go to the slot's tracker in one feed.  With sad=True, `sad` holds
        one flag per frame of feats."""
        flags = None
        if self.sad or sad is not None:
            if not torch.is_tensor(feats):
                raise SlotError(f"prefill of slot {s}: expected a tensor of features")
            flags = self._pushed_flags({s: feats.numel() // self.m._in_size}, None if sad is None else {s: sad})
        out = self.ses.prefill(s, feats)
        m = out.shape[1]
        if self.sad:
            self.tracker.fifo.push(flags)
            f = self.tracker.fifo.pop({s: m})[s]
            if m:
                self.tracker.feed({s: out[0]}, sad={s: f})
        elif m:
            self.tracker.feed({s: out[0]})
        return out

    def seek(self, s: int, t: int):
        """The session's benchmarking aid (FsMultiStreamSession.seek).  The tracker is not moved: the slot's segment frames keep
        counting the rows the session emits, from 0 at open().  Not with sad=True: the flags waiting for their rows would no
        longer belong to them."""
        if self.sad:
            raise SlotError("seek on a session with a speech-activity mask would misalign its flags")
        self.ses.seek(s, t)

    def poll(self):
        return self.tracker.poll()

    def active(self, s: int):
        return self.tracker.active(s)

    def rttm(self, s: int, rec: str, **kw):
        return self.tracker.rttm(s, rec, **kw)
