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
"""

import torch

from . import lib as _lib
from . import ops
from .multistream import SlotError, check_parts
from .postproc import rttm_lines

F32, I32, I64 = torch.float32, torch.int32, torch.int64
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
    logits are thresholded as torch.sigmoid(x) > threshold, probabilities (is_prob) as x > threshold."""

    def __init__(self, slots: int, ntracks: int, col0: int = 1, threshold: float = 0.5, median: int = 11, capacity: int = 256,
                 is_prob: bool = False, device=None):
        check_params(ntracks, col0, threshold, median, capacity)
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

    @property
    def lookahead(self) -> int:
        """Frames of look-ahead before a decision is final (median // 2)."""
        return self.median // 2

    # ---- slots
    def reset(self, s: int):
        """Start an empty stream in slot s (any state); its unpolled segments are dropped."""
        self.log.reset(s)
        self.box[s, :3] = 0

    def close(self, s: int):
        """Drop slot s's stream: its device state, its unpolled segments and the lines collected so far."""
        self.log.close(s)
        self.box[s, :3] = 0

    def state(self, s: int) -> str:
        return self.log.state[s]

    # ---- a slot's stream leaves / comes back (the "tracker" part of a multistream.StreamSnapshot)
    def _config(self):
        return {"ntracks": self.ntracks, "col0": self.col0, "threshold": self.threshold, "median": self.median,
                "is_prob": self.is_prob, "capacity": self.cap}

    def export(self, s: int) -> dict:
        """Slot s's tracker state as plain values and tensors: its device rows (copies; the segments no poll has taken yet
        travel in the box row) and its host fields."""
        part = self.log.export(s)
        part.update(config=self._config(), hist=self.hist[s].clone(), open=self.open_[s].clone(), box=self.box[s].clone())
        return part

    def check_part(self, part):
        """SlotError unless `part` is an export of a tracker configured like this one."""
        ok = (isinstance(part, dict) and part.get("config") == self._config() and part.get("state") in (OPEN, ENDED)
              and all(isinstance(part.get(k), (list, tuple)) for k in ("segs", "pending"))
              and all(torch.is_tensor(part.get(k)) and part[k].shape == row.shape[1:] and part[k].dtype == row.dtype
                      for k, row in (("hist", self.hist), ("open", self.open_), ("box", self.box))))
        if not ok:
            raise SlotError("resume: the snapshot's tracker part does not fit this tracker "
                            f"(here {self._config()}, there {part.get('config') if isinstance(part, dict) else part!r})")

    def adopt(self, s: int, part):
        """Slot s goes on from an exported `part` (checked by check_part): ordinary row copies on the current stream."""
        self.log.adopt(s, part)
        for k, rows in (("hist", self.hist), ("open", self.open_), ("box", self.box)):
            rows[s].copy_(part[k], non_blocking=True)

    # ---- feeding
    def _launch(self, desc, counts, ends, n, ld):
        ops.segtrack_feed(desc, counts, ends, n, ld, self.col0, self.ntracks, self.threshold, self.median, self.is_prob, self.hist,
                          self.open_, self.box, self.cap)

    def _rows_f32(self, s, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise _lib.EendHipError(f"slot {s}: expected a GPU tensor (the HIP path has no CPU fallback)")
        if x.dim() == 3 and x.shape[0] == 1:
            x = x[0]
        if x.dim() != 2:
            raise ValueError(f"slot {s}: expected (n, C) rows, got shape {tuple(x.shape)}")
        return x.to(F32).contiguous()

    @torch.no_grad()
    def feed(self, rows=None, end=()):
        """rows: {slot: (n, C) device tensor of its next rows}; end: slots whose stream ends after these rows.  Every tensor of a
        call has the same C >= col0 + ntracks.  One descriptor copy, one launch; nothing waits for the device."""
        rows = {s: self._rows_f32(s, x) for s, x in dict(rows or {}).items()}
        end = list(end)
        self.log.check_feed(rows.keys(), end)
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
        stage = torch.empty(4 * n + 2 * n, dtype=I32, pin_memory=True)   # a fresh pinned block per call (copied asynchronously)
        stage[:4 * n].view(I64).copy_(torch.tensor(desc, dtype=I64).reshape(-1))
        stage[4 * n:5 * n].copy_(torch.tensor([rows[s].shape[0] if s in rows else 0 for s in slots], dtype=I32))
        stage[5 * n:].copy_(torch.tensor([1 if s in end else 0 for s in slots], dtype=I32))
        dbuf = torch.empty(6 * n, dtype=I32, device=self.dev)
        dbuf.copy_(stage, non_blocking=True)
        self._launch(dbuf[:4 * n].view(I64), dbuf[4 * n:5 * n], dbuf[5 * n:], n, ld)
        self.log.ended(end)

    @torch.no_grad()
    def feed_rows(self, x, counts_dev, rows_per_slot=1):
        """The session form: row s of x ((S, C) or (S, 1, C) f32 device tensor, rows contiguous) is slot s's next row when
        counts_dev[s] (device int32 [S]) is 1.  With rows_per_slot = n, x is (S, n, C) and slot s takes its first counts_dev[s]
        (0..n) rows.  No host data, one launch; the host does not check slot states here."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != F32 or not x.is_contiguous():
            raise _lib.EendHipError("feed_rows: expected a contiguous f32 GPU tensor")
        if not isinstance(rows_per_slot, int) or rows_per_slot < 1:
            raise ValueError(f"feed_rows: rows_per_slot must be a positive int, got {rows_per_slot!r}")
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
    tracker_kw go to SegmentTracker (col0 = 1 and ntracks = C - col0 by default)."""

    def __init__(self, session, **tracker_kw):
        self.ses = session
        self.S, self.C, self.dev, self.m = session.S, session.C, session.dev, session.m
        self.max_frames, self.input_transform = session.max_frames, session.input_transform
        kw = dict(tracker_kw)
        col0 = kw.setdefault("col0", 1)
        kw.setdefault("ntracks", self.C - col0)
        self.tracker = SegmentTracker(self.S, device=self.dev, **kw)

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

    def _step(self, step, push, flush):
        before = [self.ses.state(s) for s in range(self.S)]
        out = step(push=push, flush=flush)
        if out:                                 # a replay happened: the tracker reads its emitted rows
            logits, counts, n = self.ses.emitted()
            self.tracker.feed_rows(logits, counts, rows_per_slot=n)
        done = [s for s in range(self.S) if before[s] != "done" and self.ses.state(s) == "done"]
        if done:
            self.tracker.end(done)
        return out

    @torch.no_grad()
    def step(self, push=None, flush=()):
        return self._step(self.ses.step, push, flush)

    @torch.no_grad()
    def step_frames(self, push=None, flush=()):
        return self._step(self.ses.step_frames, push, flush)

    @torch.no_grad()
    def prefill(self, s: int, feats):
        """The session's prefill of slot s; the rows it emitted go to the slot's tracker in one feed."""
        out = self.ses.prefill(s, feats)
        if out.shape[1]:
            self.tracker.feed({s: out[0]})
        return out

    def seek(self, s: int, t: int):
        """The session's benchmarking aid (FsMultiStreamSession.seek).  The tracker is not moved: the slot's segment frames keep
        counting the rows the session emits, from 0 at open()."""
        self.ses.seek(s, t)

    def poll(self):
        return self.tracker.poll()

    def active(self, s: int):
        return self.tracker.active(s)

    def rttm(self, s: int, rec: str, **kw):
        return self.tracker.rttm(s, rec, **kw)
