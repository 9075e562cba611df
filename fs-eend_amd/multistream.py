"""The slot model and the step core shared by the multi-stream sessions (`FsMultiStreamSession`, `LsMultiStreamSession`).

A session holds S slots, each carrying its own stream with its own lifetime.  `SlotTable` is the host bookkeeping (pure
Python, no device): per slot its state and the frames it has taken, and per step a `SlotPlan` that says how many frames each
slot pushes, how many dummy frames a flushing slot takes and how many frames of logits it emits.  `MultiStreamSession` runs
such a plan: it stages the pushed features, writes the plan's int32 control rows to the device with one copy and replays
the captured graph of the step (or runs its eager body), then commits the plan.  A session has one set of rows and one graph
per frame count Tp per slot and step: Tp = 1 (`step`), and Tp = max_frames (`step_frames`) when that is larger.

A slot can leave its session: `snapshot(s)` packs its state into a `StreamSnapshot` (one batched copy launch into one blob),
`suspend(s)` = snapshot + close, and `resume(snap)` puts it into a free slot of any session of the same model configuration --
another slot count, cache capacity, max_frames or graph setting, another GPU, or another process after `save` / `load`.
"""
import torch

from . import ops

F32, I32 = torch.float32, torch.int32

FREE, OPEN, FLUSHING, DONE = "free", "open", "flushing", "done"


def capture_graphs(*fns):
    """Run every fn once on a side stream (warm-up: workspaces, operand caches, lazy allocations), then record each into a graph
    of its own -> the graphs, in order.  The caller keeps whatever state the warm-up run may disturb."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for fn in fns:
            fn()
    torch.cuda.current_stream().wait_stream(s)
    graphs = []
    for fn in fns:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        graphs.append(g)
    return graphs


class SlotError(ValueError):
    pass


class SlotPlan:
    """What one step does to each slot: enc[s] frames appended to the encoder history (the pushed frames, npush[s]), then
    ndummy[s] zero frames through the look-ahead window, dec[s] of those npush + ndummy windows emitting a frame of logits
    (the last dec[s]); `flush` = slots that start flushing with this step, after their pushed frames."""

    def __init__(self, npush, ndummy, dec, flush):
        self.enc = self.npush = npush                 # the encoder appends the pushed frames
        self.ndummy, self.dec, self.flush = ndummy, dec, flush

    @property
    def win(self):
        """Per slot the look-ahead window mode of a one-frame plan: ops.WIN_PUSH / WIN_FLUSH (a dummy frame) / WIN_KEEP."""
        return [ops.WIN_PUSH if p else ops.WIN_FLUSH if d else ops.WIN_KEEP for p, d in zip(self.npush, self.ndummy)]

    def modes(self):
        """The (3, S) int32 rows the one-frame graph reads: [encoder append, window mode, decoder append]."""
        return [self.enc, self.win, self.dec]

    def counts(self):
        """The (4, S) int32 rows the multi-frame graph reads: [encoder frames, window pushes, window dummies, decoder frames]."""
        return [self.enc, self.npush, self.ndummy, self.dec]

    @property
    def emit(self):
        return [s for s, d in enumerate(self.dec) if d]

    @property
    def idle(self):
        return not any(self.npush) and not any(self.ndummy)


class SlotTable:
    """Host bookkeeping of the S slots: state free / open / flushing / done, and per slot the frames through the look-ahead
    window (`t`), the encoder and decoder history lengths and the dummy frames left to flush.

    A slot's lifetime: open() -> pushes (a step that leaves an open slot out pauses it) -> flush: conv_delay dummy frames,
    up to nmax per step, alongside the other slots -> done -> close().  close() is allowed in any state but free."""

    def __init__(self, slots: int, center: int):
        if slots <= 0:
            raise SlotError("a session needs at least one slot")
        self.S, self.center = slots, center
        self.state = [FREE] * slots
        self.t = [0] * slots
        self.n_enc = [0] * slots
        self.n_dec = [0] * slots
        self.flush_left = [0] * slots

    def _check(self, s):
        if not isinstance(s, int) or not 0 <= s < self.S:
            raise SlotError(f"slot {s!r} out of range 0..{self.S - 1}")

    def open(self) -> int:
        for s, st in enumerate(self.state):
            if st == FREE:
                self.state[s] = OPEN
                self.t[s] = self.n_enc[s] = self.n_dec[s] = self.flush_left[s] = 0
                return s
        raise SlotError(f"all {self.S} slots are in use")

    def close(self, s):
        self._check(s)
        if self.state[s] == FREE:
            raise SlotError(f"slot {s} is not open")
        self.state[s] = FREE

    def export(self, s) -> dict:
        """The fields of slot s (any state but free), as plain values: what `adopt` of any table of the same center takes."""
        self._check(s)
        if self.state[s] == FREE:
            raise SlotError(f"slot {s} is not open")
        return {"state": self.state[s], "t": self.t[s], "n_enc": self.n_enc[s], "n_dec": self.n_dec[s],
                "flush_left": self.flush_left[s]}

    @staticmethod
    def check_fields(f):
        """Raise SlotError unless f is what `export` makes."""
        ok = (isinstance(f, dict) and f.get("state") in (OPEN, FLUSHING, DONE)
              and all(isinstance(f.get(k), int) and not isinstance(f.get(k), bool) and f[k] >= 0
                      for k in ("t", "n_enc", "n_dec", "flush_left")))
        if not ok:
            raise SlotError(f"not the fields of a slot: {f!r}")

    def free_slot(self) -> int:
        """The slot the next open() or adopt() takes (the lowest free one); SlotError when all are in use."""
        for s, st in enumerate(self.state):
            if st == FREE:
                return s
        raise SlotError(f"all {self.S} slots are in use")

    def adopt(self, fields) -> int:
        """Claim a free slot, the lowest as open() does, for a stream that goes on from exported `fields`."""
        self.check_fields(fields)
        s = self.free_slot()
        self.state[s] = fields["state"]
        self.t[s], self.n_enc[s], self.n_dec[s] = fields["t"], fields["n_enc"], fields["n_dec"]
        self.flush_left[s] = fields["flush_left"]
        return s

    def plan(self, push=(), flush=()) -> SlotPlan:
        """One frame per slot.  push: slots that push a frame; flush: slots whose stream ended (not pushed in the same call)."""
        push, flush = list(push), list(flush)
        for s in push + flush:
            self._check(s)
        if len(set(push)) != len(push) or len(set(flush)) != len(flush):
            raise SlotError("a slot is named twice")
        for s in push:
            if self.state[s] != OPEN:
                raise SlotError(f"push to slot {s}, which is {self.state[s]}")
        for s in flush:
            if self.state[s] != OPEN:
                raise SlotError(f"flush of slot {s}, which is {self.state[s]}")
            if s in push:
                raise SlotError(f"slot {s} is pushed and flushed in the same step")
        return self._plan(dict.fromkeys(push, 1), flush, 1)

    def plan_frames(self, push=None, flush=(), nmax=1) -> SlotPlan:
        """One step of up to nmax frames per slot.  push: {slot: frames n (0..nmax)}; flush: slots whose stream ends after
        this step's pushed frames.  A flushing slot takes up to nmax dummy frames per step: a slot flushed in this call takes
        min(conv_delay, nmax - n) of them now, the rest follow in later calls (alongside the other slots); open slots named
        in neither pause."""
        push, flush = dict(push or {}), list(flush)
        for s in list(push) + flush:
            self._check(s)
        if len(set(flush)) != len(flush):
            raise SlotError("a slot is named twice")
        if nmax < 1:
            raise SlotError("nmax must be at least 1")
        for s, n in push.items():
            if self.state[s] != OPEN:
                raise SlotError(f"push to slot {s}, which is {self.state[s]}")
            if not isinstance(n, int) or not 0 <= n <= nmax:
                raise SlotError(f"push of {n!r} frames to slot {s}: 0..{nmax} per step")
        for s in flush:
            if self.state[s] != OPEN:
                raise SlotError(f"flush of slot {s}, which is {self.state[s]}")
        return self._plan(push, flush, nmax)

    def plan_prefill(self, s, T) -> SlotPlan:
        """Slot s alone pushes T >= 0 frames (a plan_frames-shaped plan with nmax = T): every other slot, flushing ones
        included, stands still.  Committing it leaves slot s where T committed one-frame pushes leave it."""
        self._check(s)
        if self.state[s] != OPEN:
            raise SlotError(f"prefill of slot {s}, which is {self.state[s]}")
        if not isinstance(T, int) or T < 0:
            raise SlotError(f"prefill of {T!r} frames to slot {s}")
        npush, ndummy, dec = [0] * self.S, [0] * self.S, [0] * self.S
        npush[s] = T
        dec[s] = max(0, min(T, self.t[s] + T - self.center))
        return SlotPlan(npush, ndummy, dec, [])

    def _plan(self, push, flush, nmax):
        S, c = self.S, self.center
        npush, ndummy, dec = [0] * S, [0] * S, [0] * S
        for s, n in push.items():
            npush[s] = n
        for s in flush:
            ndummy[s] = min(c, nmax - npush[s])
        for s in range(S):
            if self.state[s] == FLUSHING:
                ndummy[s] = min(self.flush_left[s], nmax)
            w = npush[s] + ndummy[s]
            if w:
                dec[s] = max(0, min(w, self.t[s] + w - c))             # windows after push m emit once t0 + m > center
        return SlotPlan(npush, ndummy, dec, flush)

    def commit(self, plan: SlotPlan):
        for s in plan.flush:
            self.state[s], self.flush_left[s] = FLUSHING, self.center
        for s in range(self.S):
            self.n_enc[s] += plan.enc[s]
            self.n_dec[s] += plan.dec[s]
            self.t[s] += plan.npush[s] + plan.ndummy[s]
            if self.state[s] == FLUSHING:
                self.flush_left[s] -= plan.ndummy[s]
                if self.flush_left[s] <= 0:
                    self.state[s] = DONE

    def max_len(self):
        """The longest K/V history of any slot in use."""
        return max([max(self.n_enc[s], self.n_dec[s]) for s in range(self.S) if self.state[s] != FREE] + [0])

SNAPSHOT_FORMAT = 1
SECTION_ALIGN = 256                             # every section of a snapshot's blob starts on this boundary


def _map_tensors(v, fn):
    """v with every tensor in it (dicts, lists and tuples searched) replaced by fn(tensor)."""
    if torch.is_tensor(v):
        return fn(v)
    if isinstance(v, dict):
        return {k: _map_tensors(x, fn) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_map_tensors(x, fn) for x in v)
    return v


def _tensors(v):
    out = []
    _map_tensors(v, out.append)
    return out


class StreamSnapshot:
    """One stream taken out of a session: a plain container, no device work of its own.

        kind        "fs" or "ls"
        signature   the model configuration the state belongs to: kind, D, H, C, window taps k, encoder and decoder layer counts,
                    in_size and the state dtypes.  `resume` refuses a session with another one.
        table       the slot's SlotTable fields: state, t, n_enc, n_dec, flush_left
        parts       {"model": ..., and one part per wrapper around the session ("frontend", "tracker")}: each a dict of plain
                    Python values and tensors.  parts["model"] = {"blob": one contiguous uint8 tensor, "sections": [(name,
                    offset, bytes), ...]}: the slot's state pieces packed back to back, each on a SECTION_ALIGN boundary (the
                    bytes between sections are unspecified).

    The weights are NOT part of a snapshot and are not identified by it: resuming under other weights than the stream ran
    with is the caller's error and goes undetected.

    `to("cpu")` returns a copy in pinned host memory, complete on return; `to(device)` a copy on that device.  `save` /
    `load` go through torch.save / torch.load(weights_only=True) of a dict of plain values and CPU tensors."""

    def __init__(self, kind, signature, table, parts):
        self.kind, self.signature, self.table, self.parts = kind, dict(signature), dict(table), dict(parts)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in _tensors(self.parts))

    @property
    def device(self):
        return self.parts["model"]["blob"].device

    def mismatch(self, signature):
        """-> the fields in which this snapshot's signature differs from `signature`, as {field: (snapshot's, other)}."""
        keys = sorted(set(self.signature) | set(signature))
        return {k: (self.signature.get(k), signature.get(k)) for k in keys if self.signature.get(k) != signature.get(k)}

    def to(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device.type == "cpu":
            pin = torch.cuda.is_available()

            def move(t):
                out = torch.empty(t.shape, dtype=t.dtype, pin_memory=pin)
                out.copy_(t, non_blocking=True)
                return out
        else:
            def move(t):
                return t.clone() if t.device == device else t.to(device, non_blocking=True)
        src = {t.device for t in _tensors(self.parts) if t.is_cuda}
        out = StreamSnapshot(self.kind, self.signature, self.table, _map_tensors(self.parts, move))
        if device.type == "cpu":
            for d in src:
                torch.cuda.synchronize(d)                             # the host copy is complete on return
        return out

    def _as_dict(self):
        return {"format": SNAPSHOT_FORMAT, "kind": self.kind, "signature": self.signature, "table": self.table,
                "parts": self.parts}

    def save(self, path):
        snap = self if not any(t.is_cuda for t in _tensors(self.parts)) else self.to("cpu")
        torch.save(snap._as_dict(), path)

    @classmethod
    def load(cls, path):
        d = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(d, dict) or d.get("format") != SNAPSHOT_FORMAT:
            raise SlotError(f"{path}: not a stream snapshot of format {SNAPSHOT_FORMAT}")
        parts = {name: dict(p) for name, p in d["parts"].items()}
        parts["model"]["sections"] = [tuple(sec) for sec in parts["model"]["sections"]]
        return cls(d["kind"], d["signature"], d["table"], parts)


def check_parts(snap, parts):
    """SlotError unless `snap` is a StreamSnapshot that carries exactly the parts `parts` of a session stack."""
    if not isinstance(snap, StreamSnapshot):
        raise SlotError(f"resume: expected a StreamSnapshot, got {type(snap).__name__}")
    if sorted(snap.parts) != sorted(parts):
        raise SlotError(f"resume: the snapshot carries the parts {sorted(snap.parts)}, this session stack {sorted(parts)}")


def _layout(pieces):
    """pieces: [(name, address, nblocks, block_bytes, stride)] -> ([(name, offset, bytes)], total bytes) of the packed blob."""
    sections, off = [], 0
    for name, _, nblocks, block_bytes, _ in pieces:
        size = nblocks * block_bytes
        sections.append((name, off, size))
        off += (size + SECTION_ALIGN - 1) // SECTION_ALIGN * SECTION_ALIGN
    return sections, off


class MultiStreamSession:
    """What the multi-stream sessions share: the slots' lifetimes, the step core and the protocol of the wrappers
    (`audio_stream.AudioStreamSession`, `live_rttm.SegmentSession`).  A subclass calls __init__, then sets

        self._rows      {Tp: row set}: Tp = 1, and Tp = max_frames when that is larger.  A row set (a SimpleNamespace) holds
                        Tp, x_in (S, Tp, in) f32 input features, ctl: the int32 control rows of a plan (plan.modes() at
                        Tp = 1, plan.counts() above; the last row is each slot's emitted frame count), logits (S, Tp, C)
                        f32, and whatever else the session's step needs
        self.len_enc, self.len_dec   int32 (S,) device history lengths, zeroed by open()

    and provides _body(rows), the eager step over one row set (captured once into a graph per row set), and
    _clear_window(s); a session whose caches grow overrides _room(need), which is called before every step that runs.  For
    snapshot / resume it sets `kind` and provides _signature() and _pieces(s, n_enc, n_dec): the state pieces of slot s at
    those history lengths as [(name, device address, nblocks, block_bytes, stride)] (the session's side of ops.copy_blocks)."""

    max_frames = 1
    kind = None
    parts = ("model",)                          # the parts of this stack's snapshots; a wrapper adds its own
    input_transform = None                      # the feature transform of the model's reference config

    def __init__(self, model, slots: int, max_nspks: int, use_graph: bool, center: int, dev):
        self.m, self.S, self.C, self.use_graph, self.center, self.dev = model, slots, max_nspks, use_graph, center, dev
        self.table = SlotTable(slots, center)
        self.frames = 0                         # steps run
        self._graph = {}                        # Tp -> captured graph of that row set; a new table once they go stale
        self._P_captured = None
        self._last = 1                          # Tp of the last step run

    def _room(self, need):
        pass

    def _check_weights(self):
        """The graphs hold raw pointers into model._prepare()'s operand copies: capture again when they were refreshed.  The
        streaming state lives in the session's own buffers and is kept."""
        P = self.m._prep
        if P is None or (self.frames & 255) == 0:
            P = self.m._prepare()
        if P is not self._P_captured:
            self._P_captured = P
            self._graph = {}

    def _capture(self, r):
        r.ctl.zero_()                           # warm-up and capture with every mask / count off: no slot state changes
        return capture_graphs(lambda: self._body(r))[0]

    # ---- public API
    def open(self) -> int:
        """Claim a free slot for a new stream: its history lengths start at 0 and its look-ahead window at zeros."""
        s = self.table.open()
        self.len_enc[s] = 0
        self.len_dec[s] = 0
        self._clear_window(s)
        return s

    def close(self, s: int):
        self.table.close(s)

    def state(self, s: int) -> str:
        return self.table.state[s]

    # ---- a slot leaves the session, a snapshot comes back
    @torch.no_grad()
    def snapshot(self, s: int) -> StreamSnapshot:
        """Slot s (open, flushing or done) as a StreamSnapshot on this session's device: one ops.copy_blocks launch on the
        current stream packs its state pieces into an exactly sized blob.  The slot is untouched and goes on; the snapshot is
        a fork of it."""
        fields = self.table.export(s)
        pieces = self._pieces(s, fields["n_enc"], fields["n_dec"])
        sections, total = _layout(pieces)
        with torch.cuda.device(self.dev):
            blob = torch.empty(total, dtype=torch.uint8, device=self.dev)
            base = blob.data_ptr()
            ops.copy_blocks([(ptr, base + off, nb, bb, stride, bb) for (_, ptr, nb, bb, stride), (_, off, _) in zip(pieces, sections)])
        return StreamSnapshot(self.kind, self._signature(), fields, {"model": {"blob": blob, "sections": sections}})

    def suspend(self, s: int) -> StreamSnapshot:
        """snapshot(s), then close(s): the stream leaves the session and its slot is free."""
        snap = self.snapshot(s)
        self.close(s)
        return snap

    def resume(self, snap: StreamSnapshot) -> int:
        """Put a suspended stream into a free slot (the lowest, as open() does) -> the slot; it goes on, bit for bit, as the
        stream it was taken from.  The snapshot may come from any session of the same signature -- other slots, cap, max_frames,
        use_graph or prefill_rows -- and from the host (staged to the device first).  SlotError, with nothing changed, when no
        slot is free or the signature differs.  The slot's rows at or beyond the snapshot's lengths keep whatever they held."""
        check_parts(snap, self.parts)
        return self._resume(snap)

    @torch.no_grad()
    def _resume(self, snap):
        diff = snap.mismatch(self._signature())
        if diff:
            raise SlotError("resume: the snapshot belongs to another model configuration: "
                            + ", ".join(f"{k} {a!r} (here {b!r})" for k, (a, b) in diff.items()))
        f, part = snap.table, snap.parts["model"]
        SlotTable.check_fields(f)
        s = self.table.free_slot()
        sections, total = _layout(self._pieces(s, f["n_enc"], f["n_dec"]))
        blob = part["blob"]
        if [tuple(x) for x in part["sections"]] != sections or blob.dtype != torch.uint8 or blob.numel() != total:
            raise SlotError("resume: the snapshot's sections are not this session's state pieces")
        self._room(max(f["n_enc"], f["n_dec"]))                       # caches grow (and graphs go) as before a step
        pieces = self._pieces(s, f["n_enc"], f["n_dec"])              # ... so the addresses are taken after it
        with torch.cuda.device(self.dev):
            blob = blob.to(self.dev, non_blocking=True).contiguous()
            base = blob.data_ptr()
            ops.copy_blocks([(base + off, ptr, nb, bb, bb, stride) for (_, ptr, nb, bb, stride), (_, off, _) in zip(pieces, sections)])
            self.table.adopt(f)                                       # takes slot s, the lowest free one
            self.len_enc[s] = f["n_enc"]
            self.len_dec[s] = f["n_dec"]
        return s

    @torch.no_grad()
    def step(self, push=None, flush=()):
        """One frame for every slot in use.  push: {slot: features of its next frame ((1,1,in) / (1,in) / (in,))}; flush: slots
        whose stream ended (each then takes conv_delay dummy frames, one per step); open slots named in neither pause.
        -> {slot: logits (1,1,C)} for the slots that emitted a frame (frame t - conv_delay of that stream)."""
        push = dict(push or {})
        plan = self.table.plan(push.keys(), flush)
        return self._step(plan, {s: x.reshape(1, -1) for s, x in push.items()}, 1)

    @torch.no_grad()
    def step_frames(self, push=None, flush=()):
        """Up to max_frames frames for every slot in use, in one replay.  push: {slot: features (n, in) / (1, n, in), n <=
        max_frames}; flush: slots whose stream ends after this step's frames (a slot may be pushed and flushed in one call; its
        dummy frames, up to max_frames per step, follow its pushed ones); open slots named in neither pause.
        -> {slot: logits (1, m, C)}: the m frames the slot emitted in this step, in order.

        Every step computes all S * max_frames rows (fixed shapes: one graph per cache capacity, and a slot's results
        independent of the others'), so max_frames should match the rate at which frames arrive: a session whose steps carry
        far fewer frames than max_frames pays for the idle rows."""
        feats = {}
        for s, x in dict(push or {}).items():
            if not torch.is_tensor(x):
                raise SlotError(f"push to slot {s}: expected a tensor of features")
            feats[s] = x.reshape(-1, self.m._in_size)
        plan = self.table.plan_frames({s: int(x.shape[0]) for s, x in feats.items()}, flush, self.max_frames)
        return self._step(plan, feats, self.max_frames)

    def _step(self, plan, feats, Tp):
        """Run `plan` on the Tp row set; feats: {slot: (n, in) features of its n pushed frames}."""
        if plan.idle:
            self.table.commit(plan)
            return {}
        self._check_weights()
        self._room(self.table.max_len() + Tp)
        r = self._rows[Tp]
        if self.use_graph and Tp not in self._graph:
            self._graph[Tp] = self._capture(r)
        slots = sorted(s for s, x in feats.items() if x.shape[0])
        if slots:                               # frame j of slot s -> input row s*Tp + j; the rows beyond a slot's count are
            src = torch.cat([feats[s] for s in slots]).to(device=self.dev, dtype=F32)   # never read for its results
            x = r.x_in.view(self.S * Tp, -1)
            if src.shape[0] == self.S * Tp:
                x.copy_(src)
            else:
                rows = slots if Tp == 1 else [s * Tp + j for s in slots for j in range(feats[s].shape[0])]
                idx = torch.tensor(rows, dtype=torch.int64, pin_memory=True).to(self.dev, non_blocking=True)
                x.index_copy_(0, idx, src)
        ctl = torch.tensor(plan.modes() if Tp == 1 else plan.counts(), dtype=I32, pin_memory=True)   # a fresh pinned block
        r.ctl.copy_(ctl, non_blocking=True)                                                          # per step (async copy)
        if self.use_graph:
            self._graph[Tp].replay()
        else:
            self._body(r)
        self.table.commit(plan)
        self.frames += 1
        self._last = Tp
        emit = plan.emit
        if not emit:
            return {}
        y = r.logits.clone()
        if Tp == 1:
            return {s: y[s:s + 1] for s in emit}
        return {s: y[s:s + 1, :plan.dec[s]] for s in emit}

    def emitted(self):
        """The rows of the last step that ran: (logits (S, n, C) f32 device tensor, int32 (S,) device tensor of each slot's
        emitted row count -- its first rows, n).  Valid until the next step."""
        r = self._rows[self._last]
        return r.logits, r.ctl[-1], self._last
