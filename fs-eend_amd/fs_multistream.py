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
from types import SimpleNamespace

import torch

from . import ops
from .fs_stream import dec_layers, enc_layers, front_end
from .lib import EendHipError
from .weights import convert_const
# the slot model lives in multistream.py; its names stay importable from here for existing callers
from .multistream import DONE, FLUSHING, FREE, OPEN, MultiStreamSession, SlotError, SlotTable  # noqa: F401

F16, F32, I32 = torch.float16, torch.float32, torch.int32


class FsMultiStreamSession(MultiStreamSession):
    """S concurrent FS-EEND streams on one `StreamingTransformerEDADiarization`, one captured hipGraph per frame step:

        encoder : BatchNorm + input projection + the incremental encoder layers, S rows (per-slot K/V appends)
        window  : per-slot look-ahead window push / dummy frame / keep, Conv1d, L2 norm, S rows
        decoder : `convert` fan-out, incremental decoder layers (S*C rows, per-slot K/V appends), speaker attention, head

        ses = FsMultiStreamSession(model, slots=64)
        a = ses.open()
        out = ses.step(push={a: x_t})          # {slot: logits (1,1,C)} for the slots that emitted a frame
        ses.step(flush=[a])                    # then conv_delay dummy frames, one per step, beside the other slots
        ses.close(a)

    prefill(slot, feats) takes one open slot forward by a backlog of any length in one eager pass (the batch-rate kernels and
    the causal prefill attention over the slot's own cache sequences); the slot then streams on frame by frame.

    With max_frames = n > 1, step_frames runs the same step at Tp = n rows per slot in a second graph: the chunk attention
    over the K/V histories, the window pushes then dummies of the chunk, the decoder over (B = S, C, Tp = n) slabs.

    K/V caches are f16 (S, H, cap, 64) per encoder layer and (S*C, H, cap, 64) per decoder layer; when a slot's history would
    reach `cap` they all double (contents kept) and the graphs are captured again.  Caches are never cleared: the lengths gate
    every read, so a reopened slot computes exactly what a fresh one does."""

    input_transform = "logmel23"
    kind = "fs"

    def __init__(self, streaming_model, slots: int, max_nspks: int = 6, cap: int = 1024, use_graph: bool = True,
                 max_frames: int = 1, prefill_rows: int = 4096):
        m = streaming_model
        if not isinstance(max_frames, int) or not 1 <= max_frames <= 64:
            raise EendHipError("max_frames must be in 1..64")
        if not isinstance(prefill_rows, int) or prefill_rows < 1:
            raise EendHipError("prefill_rows must be a positive int")
        P = m._prepare()
        if max_nspks <= 0:
            raise EendHipError("max_nspks must be positive")
        super().__init__(m, slots, max_nspks, use_graph, m.cnn.center, m.cnn.conv.weight.device)
        self.max_frames, self.D, self.H, self.k = max_frames, m.n_units, m._H, m.cnn.kernel_size
        self.win16 = torch.zeros(slots, self.k * self.D, dtype=F16, device=self.dev)   # [tap*D + c], oldest tap first
        self.len_enc = torch.zeros(slots, dtype=I32, device=self.dev)
        self.len_dec = torch.zeros(slots, dtype=I32, device=self.dev)
        self._rows = {n: self._alloc_rows(n, P) for n in sorted({1, max_frames})}
        self.prefill_rows, self._pre = prefill_rows, None             # prefill's row set: allocated on first use and kept
        self.cap = 0
        self._alloc_caches(cap, keep=False)

    def _zeros(self, *shape, dt=F16):
        return torch.zeros(*shape, dtype=dt, device=self.dev)

    def _alloc_row_set(self, N, P, **own):
        """What every row set holds: the scratch of N encoder rows and C*N decoder rows."""
        D, R, z = self.D, self.C * N, self._zeros
        r = SimpleNamespace(**own)
        r.xin16 = z(N, P["Fin_pad"])
        r.h32, r.h16 = z(N, D, dt=F32), z(N, D)                       # encoder rows; h32 is the window's input
        r.conv32, r.e32, r.e16 = z(N, D, dt=F32), z(N, D, dt=F32), z(N, D)   # the Conv1d's output, its L2 norm
        r.a32, r.a16 = z(R, D, dt=F32), z(R, D)                       # decoder rows
        r.qkv, r.o16, r.ff = z(R, 3 * D), z(R, D), z(R * P["Fmax"])
        return r

    def _alloc_rows(self, n, P):
        """The rows of a step of Tp = n frames per slot: S*n encoder rows, S*C*n decoder rows."""
        S, C, D, z = self.S, self.C, self.D, self._zeros
        r = self._alloc_row_set(S * n, P, Tp=n)
        r.x_in = z(S, n, self.m._in_size, dt=F32)
        r.cols = self.win16 if n == 1 else z(S * n, self.k * D)       # the Conv1d's rows: the windows, or the im2col rows of
        r.attr = z(S, n, C, D, dt=F32)                                # a chunk's emitting windows
        r.logits = z(S, n, C, dt=F32)
        r.ctl = z(3 if n == 1 else 4, S, dt=I32)                      # SlotPlan.modes() / counts()
        return r

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
        N = self.S * self.C
        for n, r in self._rows.items():
            r.ws = None                                               # let the old one go first
            size = ops.attn_decode_ragged_ws(N, self.H, cap) if n == 1 else ops.attn_chunk_ragged_ws(N, self.H, cap, n)
            r.ws = torch.empty(size, dtype=F32, device=self.dev)
        self._graph = {}

    def _room(self, need):
        while need >= self.cap:                                       # next capacity bucket: bigger caches, new captures
            self._alloc_caches(2 * self.cap, keep=True)

    def _clear_window(self, s):
        self.win16[s].zero_()

    # ---- snapshot / resume (multistream.py): what a slot's state is
    def _signature(self):
        return {"kind": self.kind, "D": self.D, "H": self.H, "C": self.C, "k": self.k, "enc_layers": len(self.enc_kv),
                "dec_layers": len(self.dec_kv), "in_size": self.m._in_size, "dtypes": "kv float16, window float16"}

    def _pieces(self, s, n_enc, n_dec):
        """Slot s's state: rows [0, n_enc) of its sequence in every encoder layer's K and V, rows [0, n_dec) of its C sequences
        in every decoder layer's, and its window row.  A K (or V) piece is nseq * H blocks of n * 128 bytes, cap * 128 apart."""
        H, C, row = self.H, self.C, 64 * 2
        out = []
        for side, caches, seq0, nseq, n in (("enc", self.enc_kv, s, 1, n_enc), ("dec", self.dec_kv, s * C, C, n_dec)):
            for i, kv in enumerate(caches):
                for name, t in zip("kv", kv):
                    out.append((f"{side}{i}.{name}", t.data_ptr() + seq0 * H * self.cap * row, nseq * H, n * row, self.cap * row))
        out.append(("win", self.win16[s].data_ptr(), 1, self.win16.shape[1] * 2, 0))
        return out

    # ---- the step of r.Tp frames per slot (eager body; captured once per cache capacity and row set)
    def _attn(self, r, qkv, kc, vc, o16, N, per_slot, lens, cnt):
        """Ragged attention of N sequences (per_slot of them per slot): the per-frame decode at Tp = 1, else the chunk form."""
        if r.Tp == 1:
            ops.attn_decode_ragged(qkv, kc, vc, o16, r.ws, N, self.H, self.cap, per_slot, lens, cnt)
        else:
            ops.attn_chunk_ragged(qkv, kc, vc, o16, r.ws, N, self.H, self.cap, r.Tp, per_slot, lens, cnt)

    def _conv_l2(self, cols, conv32, e32, e16):
        """Conv1d over the window rows `cols`, L2 norm (reference :42-50), and the f16 copy the decoder's fan-out reads."""
        wr, bias = self.m.cnn._weights()[:2]
        ops.linear_res_scale(cols, wr, bias, None, 1.0, conv32, None)
        ops.l2norm_rows_f32(conv32, e32)
        e16.copy_(e32)

    def _body(self, r):
        """The frame procedure (fs_stream.enc_layers / dec_layers) with the ragged attention `_attn` over every slot's history."""
        P, S, C, D, n = self.m._prepare(), self.S, self.C, self.D, r.Tp
        enc_c, dec_c = r.ctl[0], r.ctl[-1]
        advance = ops.counter_add_masked if n == 1 else ops.counter_add_count
        # encoder, S*n rows (slot s: rows s*n .. s*n + enc[s] - 1 are its new frames)
        N = S * n
        front_end(P, r.x_in, r.xin16, r.h32, r.h16, n)
        enc_layers(P, r.h32, r.h16, r.qkv[:N], r.o16[:N], r.ff,
                   lambda i, qkv, o16: self._attn(r, qkv, *self.enc_kv[i], o16, S, 1, self.len_enc, enc_c))
        advance(self.len_enc, enc_c)
        # look-ahead window: push / dummy / keep per slot, or a chunk's pushes then dummies into the im2col rows of its
        # emitting windows
        if n == 1:
            ops.window_push(self.win16, r.h32, r.ctl[1])
        else:
            ops.window_chunk(self.win16, r.h32, r.cols, r.ctl[1], r.ctl[2], r.ctl[3], n)
        self._conv_l2(r.cols, r.conv32, r.e32, r.e16)
        # decoder, (B = S, C, Tp = n) slabs
        ops.convert_fanout(r.e16, P["convert.w1"], convert_const(self.m, C), r.a32, r.a16, S, n, C)
        dec_layers(P, r.a32, r.a16, r.qkv, r.o16, r.ff,
                   lambda i, qkv, o16: self._attn(r, qkv, *self.dec_kv[i], o16, S * C, C, self.len_dec, dec_c), S, C, n, self.H)
        advance(self.len_dec, dec_c)
        ops.head_l2dot(r.e32, r.a32, r.attr, r.logits, S, n, n, C, D)

    # ---- prefill: one slot taken forward by a backlog of any length (eager, no graph)
    def _alloc_prefill(self, P):
        """The rows of one prefill piece: prefill_rows encoder rows (after the k window taps in z), C * prefill_rows decoder rows."""
        n, C, D, z = self.prefill_rows, self.C, self.D, self._zeros
        r = self._alloc_row_set(n, P)
        r.z = z(self.k + n, D)                                        # the slot's k stored taps, then the piece's encoder rows
        r.attr, r.logits = z(n * C * D, dt=F32), z(n * C, dt=F32)
        return r

    def _prefill_piece(self, r, s, x, t_enc, t_dec, ne):
        """Slot s takes the N frames x (1, N, in) f32 at encoder history t_enc; the last ne of the N windows emit, at decoder
        history t_dec.  -> logits (1, ne, C), a view of the row set.  The frame procedure with B = 1, the prefill attention over
        the slot's own cache sequences and the Conv1d reading the emitting windows as overlapping rows of z."""
        P, C, D, k, N = self.m._prepare(), self.C, self.D, self.k, x.shape[1]
        h32, h16 = r.h32[:N], r.h16[:N]
        front_end(P, x, r.xin16[:N], h32, h16, N)
        enc_layers(P, h32, h16, r.qkv[:N], r.o16[:N], r.ff,
                   lambda i, qkv, o16: ops.attn_prefill(qkv, *self.enc_kv[i], o16, s, 1, self.H, t_enc, N))
        # look-ahead window: z = the stored taps, then the new frames; the window after push m is z[m .. m + k - 1]
        r.z[:k].copy_(self.win16[s].view(k, D))
        r.z[k:k + N].copy_(h32)
        self.win16[s].copy_(r.z[N:N + k].reshape(-1))
        if not ne:
            return r.logits[:0].view(1, 0, C)
        cols = r.z.as_strided((ne, k * D), (D, 1), r.z.storage_offset() + (N - ne + 1) * D)
        e32, e16 = r.e32[:ne], r.e16[:ne]
        self._conv_l2(cols, r.conv32[:ne], e32, e16)
        R = C * ne
        a32, a16 = r.a32[:R], r.a16[:R]
        ops.convert_fanout(e16, P["convert.w1"], convert_const(self.m, C), a32, a16, 1, ne, C)
        dec_layers(P, a32, a16, r.qkv[:R], r.o16[:R], r.ff,
                   lambda i, qkv, o16: ops.attn_prefill(qkv, *self.dec_kv[i], o16, s * C, C, self.H, t_dec, ne), 1, C, ne, self.H)
        logits = r.logits[:ne * C].view(1, ne, C)
        ops.head_l2dot(e32, a32, r.attr[:ne * C * D].view(1, ne, C, D), logits, 1, ne, ne, C, D)
        return logits

    @torch.no_grad()
    def prefill(self, s: int, feats):
        """Take open slot `s`, at any position, forward by the T >= 0 frames feats ((T, in) or (1, T, in)) in one pass at batch
        rate: the slot's K/V caches, look-ahead window, counters and accounting end as after T pushes through `step`, and the
        slot streams on from there.  -> logits (1, m, C), m = max(0, min(T, t + T - conv_delay)): the frames it emitted, in order.
        No other slot is touched; flushing stays with step / step_frames.  Runs eagerly on the current stream in pieces of at
        most prefill_rows frames.  A few frames over a long history are step_frames' case, not this one's: the prefill
        attention has one work item per (sequence, head, 128 queries)."""
        self.table._check(s)
        if self.table.state[s] != OPEN:
            raise SlotError(f"prefill of slot {s}, which is {self.table.state[s]}")
        if not torch.is_tensor(feats):
            raise SlotError(f"prefill of slot {s}: expected a tensor of features")
        x = feats.reshape(-1, self.m._in_size)
        T = int(x.shape[0])
        out = []
        if T:
            self._check_weights()
            self._room(self.table.n_enc[s] + T)
            if self._pre is None:
                self._pre = self._alloc_prefill(self.m._prepare())
            x = x.to(device=self.dev, dtype=F32).contiguous()
            for a in range(0, T, self.prefill_rows):
                xp = x[a:a + self.prefill_rows].unsqueeze(0)
                plan = self.table.plan_prefill(s, int(xp.shape[1]))
                y = self._prefill_piece(self._pre, s, xp, self.table.n_enc[s], self.table.n_dec[s], plan.dec[s])
                self.table.commit(plan)
                self.len_enc[s] = self.table.n_enc[s]
                self.len_dec[s] = self.table.n_dec[s]
                if plan.dec[s]:
                    out.append(y.clone())
        if not out:
            return torch.zeros(1, 0, self.C, dtype=F32, device=self.dev)
        return out[0] if len(out) == 1 else torch.cat(out, dim=1)

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
