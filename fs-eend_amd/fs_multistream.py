"""Many FS-EEND streams in one session: S slots, each carrying its own stream with its own lifetime and K/V history length,
all advanced by one graph replay per frame.

`FsStreamSession` (fs_stream.py) serves one stream; its frame step sits at the per-launch floor (~60 launches)
whatever the row count, so S streams pushed one after another cost S times that floor.  Here every buffer has S rows on
the encoder side and S*C on the decoder side, every stage computes all rows every frame (fixed shapes: one capture per
cache capacity), and a per-slot int32 mode vector, written to the device with one copy before each replay, decides which
state changes: the encoder K/V append, the look-ahead window push (or a dummy zero frame while flushing) and the decoder
K/V append.  The decode attention reads each slot's history length from device memory (`ops.attn_decode_ragged`), so
slots open, pause, flush and close at arbitrary frames and a slot's logits depend on its own stream alone.

The per-frame procedure of one slot is FS-EEND/streaming_infer_dia.py:77-95, as in `FsStreamSession`.
"""
import torch

from . import ops
from .lib import EendHipError

F16, F32, I32 = torch.float16, torch.float32, torch.int32

FREE, OPEN, FLUSHING, DONE = "free", "open", "flushing", "done"


class SlotError(ValueError):
    pass


class SlotPlan:
    """What one frame step does to each slot: enc[s] / dec[s] = append to the encoder / decoder K/V histories, win[s] = the
    look-ahead window mode (ops.WIN_KEEP / WIN_PUSH / WIN_FLUSH); `flush` = slots that start flushing with this step."""

    def __init__(self, enc, win, dec, flush):
        self.enc, self.win, self.dec, self.flush = enc, win, dec, flush

    def modes(self):
        """The (3, S) int32 mode rows the device reads: [encoder append, window mode, decoder append]."""
        return [list(self.enc), list(self.win), list(self.dec)]

    @property
    def emit(self):
        return [s for s, d in enumerate(self.dec) if d]

    @property
    def idle(self):
        return not any(self.win)


class SlotFramesPlan:
    """What one multi-frame step (FsMultiStreamSession.step_frames) does to each slot: enc[s] frames appended to the encoder
    history (the pushed frames, npush[s]), then ndummy[s] zero frames through the look-ahead window, dec[s] of those
    npush + ndummy windows emitting a frame of logits (the last dec[s]); `flush` = slots that start flushing with this step,
    after their pushed frames.  t0[s] = the slot's frame count through the window before the step."""

    def __init__(self, enc, npush, ndummy, dec, flush, t0, center):
        self.enc, self.npush, self.ndummy, self.dec, self.flush = enc, npush, ndummy, dec, flush
        self.t0, self.center = t0, center

    def counts(self):
        """The (4, S) int32 count rows the device reads: [encoder frames, window pushes, window dummies, decoder frames]."""
        return [list(self.enc), list(self.npush), list(self.ndummy), list(self.dec)]

    @property
    def emit(self):
        return [s for s, d in enumerate(self.dec) if d]

    @property
    def idle(self):
        return not any(p + d for p, d in zip(self.npush, self.ndummy))

    def frames(self):
        """The same step as one-frame SlotPlans, in order (each slot's frames are independent of the others')."""
        S, flush = len(self.npush), set(self.flush)
        F = max([self.npush[s] + self.ndummy[s] for s in range(S)] + [self.npush[s] + 1 for s in flush] + [0])
        for f in range(F):
            enc, win, dec = [0] * S, [0] * S, [0] * S
            fl = [s for s in flush if self.npush[s] == f]
            for s in range(S):
                if f < self.npush[s]:
                    enc[s], win[s] = 1, ops.WIN_PUSH
                elif f < self.npush[s] + self.ndummy[s]:
                    win[s] = ops.WIN_FLUSH
                else:
                    continue
                dec[s] = 1 if self.t0[s] + f >= self.center else 0
            yield SlotPlan(enc, win, dec, fl)


class SlotTable:
    """Host bookkeeping of the S slots (pure Python, no device): state free / open / flushing / done, and per slot the frames
    through the look-ahead window (`t`), the encoder and decoder history lengths and the dummy frames left to flush.

    A slot's lifetime: open() -> pushes (a step that leaves an open slot out pauses it) -> flush: conv_delay dummy frames,
    one per step, alongside the other slots -> done -> close().  close() is allowed in any state but free."""

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

    def plan(self, push=(), flush=()) -> SlotPlan:
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
        S = self.S
        enc, win, dec = [0] * S, [0] * S, [0] * S
        for s in range(S):
            if s in push:
                enc[s], win[s] = 1, ops.WIN_PUSH
            elif (s in flush and self.center > 0) or (self.state[s] == FLUSHING and self.flush_left[s] > 0):
                win[s] = ops.WIN_FLUSH
            else:
                continue
            dec[s] = 1 if self.t[s] + 1 >= self.center + 1 else 0       # the look-ahead is full: a frame of logits
        return SlotPlan(enc, win, dec, flush)

    def plan_frames(self, push=None, flush=(), nmax=1) -> SlotFramesPlan:
        """One step of up to nmax frames per slot.  push: {slot: frames n (0..nmax)}; flush: slots whose stream ends after
        this step's pushed frames.  A flushing slot takes up to nmax dummy frames per step: a slot flushed in this call takes
        min(conv_delay, nmax - n) of them now, the rest follow in later calls (alongside the other slots); open slots named
        in neither pause.  commit() of the plan leaves the table as the same frames pushed through plan() / commit() would."""
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
        S = self.S
        npush, ndummy, dec = [0] * S, [0] * S, [0] * S
        for s in range(S):
            n = push.get(s, 0)
            if s in flush:
                d = min(self.center, nmax - n)
            elif self.state[s] == FLUSHING:
                d = min(self.flush_left[s], nmax)
            else:
                d = 0
            npush[s], ndummy[s] = n, d
            dec[s] = max(0, min(n + d, self.t[s] + n + d - self.center))     # windows after push m emit once t0 + m > center
        return SlotFramesPlan(list(npush), npush, ndummy, dec, flush, list(self.t), self.center)

    def commit(self, plan: SlotPlan):
        if isinstance(plan, SlotFramesPlan):
            for p in plan.frames():
                self.commit(p)
            return
        for s in plan.flush:
            self.state[s], self.flush_left[s] = FLUSHING, self.center
        for s in range(self.S):
            self.n_enc[s] += plan.enc[s]
            self.n_dec[s] += plan.dec[s]
            if plan.win[s]:
                self.t[s] += 1
            if plan.win[s] == ops.WIN_FLUSH:
                self.flush_left[s] -= 1
            if self.state[s] == FLUSHING and self.flush_left[s] <= 0:
                self.state[s] = DONE

    def max_len(self):
        """The longest K/V history of any slot in use."""
        return max([max(self.n_enc[s], self.n_dec[s]) for s in range(self.S) if self.state[s] != FREE] + [0])


class FsMultiStreamSession:
    """S concurrent FS-EEND streams on one `StreamingTransformerEDADiarization`, one captured hipGraph per frame step:

        encoder : BatchNorm + input projection + the incremental encoder layers, S rows (per-slot K/V appends)
        window  : per-slot look-ahead window push / dummy frame / keep, Conv1d, L2 norm, S rows
        decoder : `convert` fan-out, incremental decoder layers (S*C rows, per-slot K/V appends), speaker attention, head

        ses = FsMultiStreamSession(model, slots=64)
        a = ses.open()
        out = ses.step(push={a: x_t})          # {slot: logits (1,1,C)} for the slots that emitted a frame
        ses.step(flush=[a])                    # then conv_delay dummy frames, one per step, beside the other slots
        ses.close(a)

    K/V caches are f16 (S, H, cap, 64) per encoder layer and (S*C, H, cap, 64) per decoder layer; when a slot's history would
    reach `cap` they all double (contents kept) and the graph is captured again.  Caches are never cleared: the lengths gate
    every read, so a reopened slot computes exactly what a fresh one does."""

    def __init__(self, streaming_model, slots: int, max_nspks: int = 6, cap: int = 1024, use_graph: bool = True,
                 max_frames: int = 1):
        m = streaming_model
        self.m, self.S, self.C, self.use_graph = m, slots, max_nspks, use_graph
        if not isinstance(max_frames, int) or not 1 <= max_frames <= 64:
            raise EendHipError("max_frames must be in 1..64")
        self.nmax = self.max_frames = max_frames
        P = m._prepare()
        dev = m.cnn.conv.weight.device
        self.dev, self.D, self.H = dev, m.n_units, m._H
        S, C, D = slots, max_nspks, self.D
        if C <= 0:
            raise EendHipError("max_nspks must be positive")
        self.k, self.center = m.cnn.kernel_size, m.cnn.center
        self.table = SlotTable(S, self.center)
        Fmax = max([l["w1"].shape[0] for l in P["enc"] + P["dec"]] + [1])
        z = lambda *s_, dt=F16: torch.zeros(*s_, dtype=dt, device=dev)
        R = S * C
        self.x_in = z(S, 1, m._in_size, dt=F32)
        self.xin16 = z(S, P["Fin_pad"])
        self.h32, self.h16 = z(S, D, dt=F32), z(S, D)                 # encoder rows; h32 is the window's input
        self.a32, self.a16 = z(R, D, dt=F32), z(R, D)                 # decoder rows
        self.qkv, self.o16, self.ff = z(R, 3 * D), z(R, D), z(R * Fmax)
        self.win16 = z(S, self.k * D)                                 # [tap*D + c], oldest tap first
        self.conv32, self.e32, self.e16 = z(S, D, dt=F32), z(S, D, dt=F32), z(S, D)
        self.attr = z(S, 1, C, D, dt=F32)
        self.logits = z(S, 1, C, dt=F32)
        self.len_enc = z(S, dt=I32)
        self.len_dec = z(S, dt=I32)
        self.modes = z(3, S, dt=I32)                                  # [encoder append, window mode, decoder append]
        self.frames = 0
        if max_frames > 1:                                            # the multi-frame step's own rows: Tp = nmax per slot
            n, Rn = max_frames, R * max_frames
            self.c_x_in = z(S, n, m._in_size, dt=F32)
            self.c_xin16 = z(S * n, P["Fin_pad"])
            self.c_h32, self.c_h16 = z(S * n, D, dt=F32), z(S * n, D)
            self.c_a32, self.c_a16 = z(Rn, D, dt=F32), z(Rn, D)
            self.c_qkv, self.c_o16, self.c_ff = z(Rn, 3 * D), z(Rn, D), z(Rn * Fmax)
            self.c_cols = z(S * n, self.k * D)                        # the Conv1d's im2col rows of the emitting windows
            self.c_conv32, self.c_e32, self.c_e16 = z(S * n, D, dt=F32), z(S * n, D, dt=F32), z(S * n, D)
            self.c_attr = z(S, n, C, D, dt=F32)
            self.c_logits = z(S, n, C, dt=F32)
            self.counts = z(4, S, dt=I32)                             # [encoder frames, window pushes, dummies, decoder frames]
        self.cap = 0
        self._alloc_caches(cap, keep=False)

    # ---- state
    def _alloc_caches(self, cap, keep):
        P = self.m._prepare()
        old_enc, old_dec, old_cap = getattr(self, "enc_kv", []), getattr(self, "dec_kv", []), self.cap
        mk = lambda N: tuple(torch.zeros(N, self.H, cap, 64, dtype=F16, device=self.dev) for _ in range(2))
        self.enc_kv = [mk(self.S) for _ in P["enc"]]
        self.dec_kv = [mk(self.S * self.C) for _ in P["dec"]]
        if keep:
            for new, prev in zip(self.enc_kv + self.dec_kv, old_enc + old_dec):
                for a, b in zip(new, prev):
                    a[:, :, :old_cap] = b
        del old_enc, old_dec
        self.cap = cap
        self.ws = torch.empty(ops.attn_decode_ragged_ws(self.S * self.C, self.H, cap), dtype=F32, device=self.dev)
        self._graph = None
        if self.nmax > 1:
            self.c_ws = None                                          # let the old one go first
            self.c_ws = torch.empty(ops.attn_chunk_ragged_ws(self.S * self.C, self.H, cap, self.nmax), dtype=F32, device=self.dev)
            self._c_graph = None

    def _room(self, need):
        while need >= self.cap:                                       # next capacity bucket: bigger caches, a new capture
            self._alloc_caches(2 * self.cap, keep=True)

    def _check_weights(self):
        """As FsStreamSession._check_weights: the graph holds raw pointers into model._prepare()'s operand copies -- capture
        again when they were refreshed."""
        P = self.m._prep
        if P is None or (self.frames & 255) == 0:
            P = self.m._prepare()
        if P is not getattr(self, "_P_captured", None):
            self._P_captured = P
            self._graph = None
            self._c_graph = None

    # ---- the frame step (eager body; captured once per cache capacity)
    def _frame(self):
        P, H, S, C, D = self.m._prepare(), self.H, self.S, self.C, self.D
        enc_m, win_m, dec_m = self.modes[0], self.modes[1], self.modes[2]
        # encoder, S rows
        qkv, o16 = self.qkv[:S], self.o16[:S]
        ops.bn_cast_pad(self.x_in, P["bn"], self.xin16, 1, 1, True, P["bn.eps"])
        ops.linear_res_ln(self.xin16, P["in.w"], P["in.b"], None, P["in.g"], P["in.beta"], self.h32, self.h16, P["in.eps"])
        for L, (kc, vc) in zip(P["enc"], self.enc_kv):
            Fi = L["w1"].shape[0]
            ff = self.ff[:S * Fi].view(S, Fi)
            ops.linear(self.h16, L["att"][0], L["att"][1], qkv)
            ops.attn_decode_ragged(qkv, kc, vc, o16, self.ws, S, H, self.cap, 1, self.len_enc, enc_m)
            ops.linear_res_ln(o16, L["att"][2], L["att"][3], self.h32, L["n1"][0], L["n1"][1], self.h32, self.h16, L["n1"][2])
            ops.linear(self.h16, L["w1"], L["b1"], ff, relu=True)
            ops.linear_res_ln(ff, L["w2"], L["b2"], self.h32, L["n2"][0], L["n2"][1], self.h32, self.h16, L["n2"][2])
        ops.counter_add_masked(self.len_enc, enc_m)
        # look-ahead window, Conv1d, L2 norm (reference :42-50)
        ops.window_push(self.win16, self.h32, win_m)
        wr, bias = self.m.cnn._weights()[:2]
        ops.linear_res_scale(self.win16, wr, bias, None, 1.0, self.conv32, None)
        ops.l2norm_rows_f32(self.conv32, self.e32)
        self.e16.copy_(self.e32)
        # decoder, S*C rows
        R = S * C
        qkv, o16 = self.qkv[:R], self.o16[:R]
        ops.convert_fanout(self.e16, P["convert.w1"], self.m._convert_const(C), self.a32, self.a16, S, 1, C)
        for L, (kc, vc) in zip(P["dec"], self.dec_kv):
            Fi = L["w1"].shape[0]
            ff = self.ff[:R * Fi].view(R, Fi)
            ops.linear(self.a16, L["att"][0], L["att"][1], qkv)
            ops.attn_decode_ragged(qkv, kc, vc, o16, self.ws, R, H, self.cap, C, self.len_dec, dec_m)
            ops.linear_res_ln(o16, L["att"][2], L["att"][3], self.a32, L["n1"][0], L["n1"][1], self.a32, self.a16, L["n1"][2])
            ops.linear(self.a16, L["spk"][0], L["spk"][1], qkv)
            ops.spk_attn(qkv, o16, S, C, 1, H)
            ops.linear_res_ln(o16, L["spk"][2], L["spk"][3], self.a32, L["n2"][0], L["n2"][1], self.a32, self.a16, L["n2"][2])
            ops.linear(self.a16, L["w1"], L["b1"], ff, relu=True)
            ops.linear_res_ln(ff, L["w2"], L["b2"], self.a32, L["n3"][0], L["n3"][1], self.a32, self.a16, L["n3"][2])
        ops.counter_add_masked(self.len_dec, dec_m)
        ops.head_l2dot(self.e32, self.a32, self.attr, self.logits, S, 1, 1, C, D)

    # ---- the multi-frame step: the _frame body at Tp = nmax (eager body; captured once per cache capacity)
    def _frames(self):
        P, H, S, C, D, n = self.m._prepare(), self.H, self.S, self.C, self.D, self.nmax
        enc_c, push_c, dummy_c, dec_c = self.counts[0], self.counts[1], self.counts[2], self.counts[3]
        # encoder, S*n rows (slot s: rows s*n .. s*n + enc[s] - 1 are its new frames)
        Se = S * n
        qkv, o16 = self.c_qkv[:Se], self.c_o16[:Se]
        ops.bn_cast_pad(self.c_x_in, P["bn"], self.c_xin16, n, n, True, P["bn.eps"])
        ops.linear_res_ln(self.c_xin16, P["in.w"], P["in.b"], None, P["in.g"], P["in.beta"], self.c_h32, self.c_h16, P["in.eps"])
        for L, (kc, vc) in zip(P["enc"], self.enc_kv):
            Fi = L["w1"].shape[0]
            ff = self.c_ff[:Se * Fi].view(Se, Fi)
            ops.linear(self.c_h16, L["att"][0], L["att"][1], qkv)
            ops.attn_chunk_ragged(qkv, kc, vc, o16, self.c_ws, S, H, self.cap, n, 1, self.len_enc, enc_c)
            ops.linear_res_ln(o16, L["att"][2], L["att"][3], self.c_h32, L["n1"][0], L["n1"][1], self.c_h32, self.c_h16, L["n1"][2])
            ops.linear(self.c_h16, L["w1"], L["b1"], ff, relu=True)
            ops.linear_res_ln(ff, L["w2"], L["b2"], self.c_h32, L["n2"][0], L["n2"][1], self.c_h32, self.c_h16, L["n2"][2])
        ops.counter_add_count(self.len_enc, enc_c)
        # look-ahead window over the chunk (pushes, then dummies), Conv1d on the emitting windows, L2 norm
        ops.window_chunk(self.win16, self.c_h32, self.c_cols, push_c, dummy_c, dec_c, n)
        wr, bias = self.m.cnn._weights()[:2]
        ops.linear_res_scale(self.c_cols, wr, bias, None, 1.0, self.c_conv32, None)
        ops.l2norm_rows_f32(self.c_conv32, self.c_e32)
        self.c_e16.copy_(self.c_e32)
        # decoder, (B = S, C, Tp = n) slabs
        R = S * C * n
        qkv, o16 = self.c_qkv[:R], self.c_o16[:R]
        ops.convert_fanout(self.c_e16, P["convert.w1"], self.m._convert_const(C), self.c_a32, self.c_a16, S, n, C)
        for L, (kc, vc) in zip(P["dec"], self.dec_kv):
            Fi = L["w1"].shape[0]
            ff = self.c_ff[:R * Fi].view(R, Fi)
            ops.linear(self.c_a16, L["att"][0], L["att"][1], qkv)
            ops.attn_chunk_ragged(qkv, kc, vc, o16, self.c_ws, S * C, H, self.cap, n, C, self.len_dec, dec_c)
            ops.linear_res_ln(o16, L["att"][2], L["att"][3], self.c_a32, L["n1"][0], L["n1"][1], self.c_a32, self.c_a16, L["n1"][2])
            ops.linear(self.c_a16, L["spk"][0], L["spk"][1], qkv)
            ops.spk_attn(qkv, o16, S, C, n, H)
            ops.linear_res_ln(o16, L["spk"][2], L["spk"][3], self.c_a32, L["n2"][0], L["n2"][1], self.c_a32, self.c_a16, L["n2"][2])
            ops.linear(self.c_a16, L["w1"], L["b1"], ff, relu=True)
            ops.linear_res_ln(ff, L["w2"], L["b2"], self.c_a32, L["n3"][0], L["n3"][1], self.c_a32, self.c_a16, L["n3"][2])
        ops.counter_add_count(self.len_dec, dec_c)
        ops.head_l2dot(self.c_e32, self.c_a32, self.c_attr, self.c_logits, S, n, n, C, D)

    def _graph_of(self, body, state):
        state.zero_()                           # warm-up and capture with every mask / count off: no slot state changes
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                    # warm-up: workspaces, operand caches
            body()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            body()
        return g

    def _capture(self):
        self._graph = self._graph_of(self._frame, self.modes)

    # ---- public API
    def open(self) -> int:
        """Claim a free slot for a new stream: its history lengths and look-ahead window start empty."""
        s = self.table.open()
        self.len_enc[s] = 0
        self.len_dec[s] = 0
        self.win16[s].zero_()
        return s

    def close(self, s: int):
        self.table.close(s)

    def state(self, s: int) -> str:
        return self.table.state[s]

    @torch.no_grad()
    def step(self, push=None, flush=()):
        """One frame for every slot in use.  push: {slot: features of its next frame ((1,1,in) / (1,in) / (in,))}; flush: slots
        whose stream ended (each then takes conv_delay dummy frames, one per step); open slots named in neither pause.
        -> {slot: logits (1,1,C)} for the slots that emitted a frame (frame t - conv_delay of that stream)."""
        push = dict(push or {})
        plan = self.table.plan(push.keys(), flush)
        if plan.idle:
            self.table.commit(plan)
            return {}
        self._check_weights()
        self._room(self.table.max_len() + 1)
        if self.use_graph and self._graph is None:
            self._capture()
        if push:
            slots = sorted(push)
            src = torch.stack([push[s].reshape(-1) for s in slots]).to(device=self.dev, dtype=F32)
            x = self.x_in.view(self.S, -1)
            if slots == list(range(self.S)):
                x.copy_(src)
            else:
                idx = torch.tensor(slots, dtype=torch.int64, pin_memory=True).to(self.dev, non_blocking=True)
                x.index_copy_(0, idx, src)
        modes = torch.tensor(plan.modes(), dtype=I32, pin_memory=True)   # a fresh pinned block per step (copied asynchronously)
        self.modes.copy_(modes, non_blocking=True)
        if self.use_graph:
            self._graph.replay()
        else:
            self._frame()
        self.table.commit(plan)
        self.frames += 1
        emit = plan.emit
        if not emit:
            return {}
        y = self.logits.clone()
        return {s: y[s:s + 1] for s in emit}

    @torch.no_grad()
    def step_frames(self, push=None, flush=()):
        """Up to max_frames frames for every slot in use, in one replay.  push: {slot: features (n, in) / (1, n, in), n <=
        max_frames}; flush: slots whose stream ends after this step's frames (a slot may be pushed and flushed in one call; its
        dummy frames, up to max_frames per step, follow its pushed ones); open slots named in neither pause.
        -> {slot: logits (1, m, C)}: the m frames the slot emitted in this step, in order.

        Every step computes all S * max_frames rows (fixed shapes: one graph per cache capacity, and a slot's results
        independent of the others'), so max_frames should match the rate at which frames arrive: a session whose steps carry
        far fewer frames than max_frames pays for the idle rows."""
        if self.nmax == 1:
            raise SlotError("step_frames needs a session built with max_frames > 1")
        feats = {}
        for s, x in dict(push or {}).items():
            if not torch.is_tensor(x):
                raise SlotError(f"push to slot {s}: expected a tensor of features")
            feats[s] = x.reshape(-1, self.m._in_size)
        plan = self.table.plan_frames({s: int(x.shape[0]) for s, x in feats.items()}, flush, self.nmax)
        if plan.idle:
            self.table.commit(plan)
            return {}
        self._check_weights()
        self._room(self.table.max_len() + self.nmax)
        if self.use_graph and self._c_graph is None:
            self._c_graph = self._graph_of(self._frames, self.counts)
        slots = sorted(s for s, x in feats.items() if x.shape[0])
        if slots:                               # frame j of slot s -> input row s*nmax + j; the rows beyond a slot's count are
            n = self.nmax                       # never read for its results, whatever they hold
            src = torch.cat([feats[s] for s in slots]).to(device=self.dev, dtype=F32)
            x = self.c_x_in.view(self.S * n, -1)
            if src.shape[0] == self.S * n:
                x.copy_(src)
            else:
                rows = [s * n + j for s in slots for j in range(feats[s].shape[0])]
                idx = torch.tensor(rows, dtype=torch.int64, pin_memory=True).to(self.dev, non_blocking=True)
                x.index_copy_(0, idx, src)
        counts = torch.tensor(plan.counts(), dtype=I32, pin_memory=True)   # a fresh pinned block per step (copied asynchronously)
        self.counts.copy_(counts, non_blocking=True)
        if self.use_graph:
            self._c_graph.replay()
        else:
            self._frames()
        self.table.commit(plan)
        self.frames += 1
        emit = plan.emit
        if not emit:
            return {}
        y = self.c_logits.clone()
        return {s: y[s:s + 1, :plan.dec[s]] for s in emit}

    def seek(self, s: int, t: int):
        """Benchmarking aid: let open slot `s` continue as if `t` frames had been pushed -- its cache rows keep whatever they
        hold, only the history counters move (FsStreamSession.seek for one slot)."""
        if self.table.state[s] != OPEN:
            raise SlotError(f"seek on slot {s}, which is {self.table.state[s]}")
        n_dec = max(0, t - self.center)
        self._room(max(t, n_dec) + 1)
        self.table.t[s], self.table.n_enc[s], self.table.n_dec[s] = t, t, n_dec
        self.len_enc[s] = t
        self.len_dec[s] = n_dec
