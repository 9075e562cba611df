"""Many LS-EEND streams in one session: S slots, each carrying its own stream with its own lifetime and stream position, all
advanced by one graph replay per frame.

`LsStreamSession(batch=S)` (ls_stream.py) runs S streams in lockstep: one retention scale for the whole batch, one reset for
all.  Here every buffer has S rows on the encoder side and S*C on the decoder side, every stage computes all rows every frame
with the all-f32 frame step of ls_stream.py (`enc_step` / `dec_step` run it too), and the three state touches of that step take
their stream position from per-slot int32 lengths in device memory: the retention recurrence (`ops.retention_step_ragged`,
scale = the slot's own frame count), the Conformer depthwise-conv cache (`ops.dwconv_step_ragged`) and the f32 look-ahead window
(`ops.window_push_f32`).  A per-slot mode vector, written with one copy before each replay, decides which state changes.
LS state is O(1) per stream, so one capture serves the whole session (again only when the weights are refreshed).

The per-frame procedure of one slot is LS-EEND/streaming_infer_dia.py:52-97, as in `LsStreamSession`; the slot bookkeeping is
FsMultiStreamSession's (multistream.py): encoder on push, window push or flush, decoder once the look-ahead is full.
"""
from types import SimpleNamespace

import torch

from . import ops
from .lib import EendHipError
from .ls_stream import f32_blocks, f32_dec_layers, f32_input
from .multistream import OPEN, MultiStreamSession, SlotError
from .weights import convert_const

F16, F32, I32 = torch.float16, torch.float32, torch.int32


class LsMultiStreamSession(MultiStreamSession):
    """S concurrent LS-EEND streams on one `OnlineConformerRetentionDADiarization`, one captured hipGraph per frame step:

        encoder : input projection + Conformer-retention blocks, S rows (per-slot retention scale and conv cache)
        window  : per-slot look-ahead window push / zero frame / keep (f32), Conv1d, L2 norm, S rows
        decoder : `convert` fan-out, retention decoder layers (S*C rows, per-slot scale), speaker attention, head

        ses = LsMultiStreamSession(model, slots=64, max_nspks=10)
        a = ses.open()
        out = ses.step(push={a: x_t})          # {slot: logits (1,1,C)} for the slots that emitted a frame
        ses.step(flush=[a])                    # then conv_delay zero embeddings, one per step, beside the other slots
        ses.close(a)

    prefill(slot, feats) takes one open slot forward by a backlog of any length in one eager pass (the same all-f32 step at
    B = 1 over the backlog's rows, the chunk-parallel f32 retention `ops.retention_prefill` and the frame-parallel conv cache
    `ops.dwconv_prefill` on the slot's own state); the slot then streams on frame by frame.

    State: retention kv f32 (S, H, 64, 64) per encoder block and (S*C, H, 64, 64) per decoder layer, conv caches f32 (S, D, k-1)
    per block, the window f32 (S, k*D) and two int32 length vectors.  States are never cleared: a length of 0 means "empty" to
    every kernel that reads them, so a reopened slot computes exactly what a fresh one does.

    With max_frames = n > 1, step_frames runs the same step at Tp = n rows per slot in a second graph: the chunk forms of the
    three state touches (`ops.retention_chunk_ragged`, `ops.dwconv_chunk_ragged`, `ops.window_chunk_f32`: each slot advances
    by its own 0..n frames, its state read and written once, bit for bit what n per-frame calls leave) and the decoder over
    (B = S, C, Tp = n) slabs.  Without it step_frames takes one frame per slot and step."""

    input_transform = "logmel23_cummn"
    kind = "ls"

    def __init__(self, model, slots: int, max_nspks: int = 10, use_graph: bool = True, max_frames: int = 1,
                 prefill_rows: int = 1024):
        m = model
        if not isinstance(max_frames, int) or isinstance(max_frames, bool) or not 1 <= max_frames <= 64:
            raise EendHipError("max_frames must be in 1..64")
        if not isinstance(prefill_rows, int) or isinstance(prefill_rows, bool) or prefill_rows < 1:
            raise EendHipError("prefill_rows must be a positive int")
        P = m._prepare()
        if max_nspks <= 0 or max_nspks > 16:
            raise EendHipError("max_nspks must be in 1..16 (the f32 speaker attention of the frame step)")
        dev = m.cnn.weight.device
        super().__init__(m, slots, max_nspks, use_graph, P["cnn.k"] // 2, dev)
        self.max_frames, self.D, self.H, self.k = max_frames, m.n_units, m._n_heads, P["cnn.k"]
        S, C, D, H = slots, max_nspks, self.D, self.H
        R = S * C
        K1 = m.enc.encoder._conv_kernel_size - 1
        z = lambda *s_, dt=F32: torch.zeros(*s_, dtype=dt, device=dev)
        self.win32 = z(S, self.k * D)                                 # [tap*D + c], oldest tap first
        self.enc_kv = [z(S, H, 64, 64) for _ in P["blocks"]]
        self.caches = [z(S, D, K1) for _ in P["blocks"]]
        self.dec_kv = [z(R, H, 64, 64) for _ in P["dec.layers"]]
        self.len_enc = z(S, dt=I32)
        self.len_dec = z(S, dt=I32)
        self._rows = {n: self._alloc_rows(n, P) for n in sorted({1, max_frames})}
        r = self._rows[1]                                             # the per-frame rows under their long-standing names
        self.x_in, self.logits, self.modes, self.attr = r.x_in, r.logits, r.ctl, r.attr
        self.prefill_rows, self._pre = prefill_rows, None             # prefill's row set: allocated on first use and kept

    def _alloc_rows(self, n, P):
        """The rows of a step of Tp = n frames per slot: S*n encoder rows, S*C*n decoder rows (slabs: row (s*C + c)*n + j)."""
        S, C, D, m = self.S, self.C, self.D, self.m
        Fmax = max([Bk["w1a32"].shape[0] for Bk in P["blocks"]] + [Ld["w1_32"].shape[0] for Ld in P["dec.layers"]] + [1])
        z = lambda *s_, dt=F32: torch.zeros(*s_, dtype=dt, device=self.dev)
        N, R = S * n, S * C * n
        r = SimpleNamespace(Tp=n)
        r.x_in = z(S, m._in_size) if n == 1 else z(S, n, m._in_size)
        r.xin32 = z(N, P["Fin_pad"])                                  # zero-padded input rows of the f32 input projection
        r.h32, r.h16, r.x16, r.xn32 = z(N, D), z(N, D, dt=F16), z(N, D, dt=F16), z(N, D)    # encoder rows
        r.o16, r.glu16, r.dw16 = z(N, D, dt=F16), z(N, D, dt=F16), z(N, D, dt=F16)
        r.q32 = z(R, 4 * D)                                           # retention projections (encoder: the first N rows)
        r.ff32 = z(R * Fmax)
        r.cols = self.win32 if n == 1 else z(N, self.k * D)           # the Conv1d's rows: the windows, or the im2col rows of
        r.y32, r.e32 = z(N, D), z(N, D)                               # a chunk's emitting windows
        r.a32, r.a16, r.o32, r.qkv32 = z(R, D), z(R, D, dt=F16), z(R, D), z(R, 3 * D)    # decoder rows
        r.attr = z(S, n, C, D)
        r.logits = z(S, n, C)
        r.ctl = z(3 if n == 1 else 4, S, dt=I32)                      # SlotPlan.modes() / counts()
        return r

    def _clear_window(self, s):
        self.win32[s].zero_()

    # ---- snapshot / resume (multistream.py): what a slot's state is
    def _signature(self):
        return {"kind": self.kind, "D": self.D, "H": self.H, "C": self.C, "k": self.k, "enc_layers": len(self.enc_kv),
                "dec_layers": len(self.dec_kv), "in_size": self.m._in_size, "dtypes": "kv float32, conv cache float32, window float32"}

    def _pieces(self, s, n_enc, n_dec):
        """Slot s's state, O(1) whatever its position: its retention state and conv cache in every encoder block, the
        retention states of its C sequences in every decoder layer and its window row -- one block each."""
        C = self.C
        one = lambda name, t, a, n: (name, t[a].data_ptr(), 1, n * t[a].numel() * t.element_size(), 0)
        out = []
        for i, (kv, cache) in enumerate(zip(self.enc_kv, self.caches)):
            out += [one(f"enc{i}.kv", kv, s, 1), one(f"enc{i}.conv", cache, s, 1)]
        out += [one(f"dec{i}.kv", kv, s * C, C) for i, kv in enumerate(self.dec_kv)]
        out.append(one("win", self.win32, s, 1))
        return out

    # ---- the step of r.Tp frames per slot (eager body; captured once per row set)
    def _ret(self, r, q32, kv, lens, ctl, per_slot, Nseq, eps, out16=None, out32=None):
        """The retention recurrence of Nseq sequences (per_slot of them per slot): the frame step at Tp = 1, else the chunk."""
        if r.Tp == 1:
            ops.retention_step_ragged(q32, kv, lens, ctl, per_slot, Nseq, self.H, eps, out16=out16, out32=out32)
        else:
            ops.retention_chunk_ragged(q32, kv, lens, ctl, per_slot, Nseq, self.H, r.Tp, eps, out16=out16, out32=out32)

    def _body(self, r):
        """ls_stream's all-f32 frame step with the retention state, conv cache and look-ahead window per slot."""
        P, S, C, n = self.m._prepare(), self.S, self.C, r.Tp
        enc_c, dec_c = r.ctl[0], r.ctl[-1]                            # modes at Tp = 1, frame counts above
        advance = ops.counter_add_masked if n == 1 else ops.counter_add_count
        # encoder, S*n rows (slot s: rows s*n .. s*n + enc[s] - 1 are its new frames)
        N = S * n

        def dwconv(i, Bk, glu16, dw16):
            if n == 1:
                ops.dwconv_step_ragged(glu16, self.caches[i], self.len_enc, enc_c, Bk["dw"], Bk["bn"], dw16, Bk["bn_eps"])
            else:
                ops.dwconv_chunk_ragged(glu16, self.caches[i], self.len_enc, enc_c, Bk["dw"], Bk["bn"], dw16, n, Bk["bn_eps"])

        ret = lambda i, Bk, q32, **out: self._ret(r, q32, self.enc_kv[i], self.len_enc, enc_c, 1, S, Bk["gn_eps"], **out)
        f32_input(P, r.x_in.view(N, -1), r.xin32, r.h32, r.h16)
        f32_blocks(P, r.h32, r.h16, r.x16, r.xn32, r.q32[:N], r.o16, r.glu16, r.dw16, r.ff32, ret, dwconv)
        advance(self.len_enc, enc_c)
        # look-ahead window (f32): push / zero frame / keep per slot, or a chunk's pushes then dummies into the im2col rows of
        # its emitting windows; Conv1d, L2 norm (LsStreamSession._conv per slot)
        if n == 1:
            ops.window_push_f32(self.win32, r.h32, r.ctl[1])
        else:
            ops.window_chunk_f32(self.win32, r.h32, r.cols, r.ctl[1], r.ctl[2], r.ctl[3], n)
        ops.linear_step_f32(r.cols, P["cnn.w32"], P["cnn.b"], r.y32)
        ops.l2norm_rows_f32(r.y32, r.e32)
        # decoder, S*C*n rows in (B = S, C, Tp = n) slabs
        if n == 1:
            ops.convert_fanout_step_f32(r.e32, P["convert.w32"], convert_const(self.m, C), r.a32, r.a16, S, C)
        else:
            ops.convert_fanout_f32(r.e32, P["convert.w32"], convert_const(self.m, C), r.a32, r.a16, S, n, C)
        ret = lambda i, Ld, q32, **out: self._ret(r, q32, self.dec_kv[i], self.len_dec, dec_c, C, S * C, Ld["gn_eps"], **out)
        f32_dec_layers(P, r.a32, r.q32, r.o32, r.qkv32, r.ff32, ret, S, C, n)
        advance(self.len_dec, dec_c)
        ops.head_l2dot(r.e32, r.a32, r.attr, r.logits, S, n, n, C, self.D)

    # ---- prefill: one slot taken forward by a backlog of any length (eager, no graph)
    def _alloc_prefill(self, P):
        """The rows of one prefill piece: prefill_rows encoder rows (after the k window taps in z), C * prefill_rows decoder rows
        (about 17.5 KB of f32 scratch each), and the retention prefill's workspace."""
        n, C, D = self.prefill_rows, self.C, self.D
        Fmax = max([Bk["w1a32"].shape[0] for Bk in P["blocks"]] + [Ld["w1_32"].shape[0] for Ld in P["dec.layers"]] + [1])
        z = lambda *s_, dt=F32: torch.zeros(*s_, dtype=dt, device=self.dev)
        R = C * n
        r = SimpleNamespace()
        r.xin32 = z(n, P["Fin_pad"])
        r.h32, r.h16, r.x16, r.xn32 = z(n, D), z(n, D, dt=F16), z(n, D, dt=F16), z(n, D)
        r.o16, r.glu16, r.dw16 = z(n, D, dt=F16), z(n, D, dt=F16), z(n, D, dt=F16)
        r.q32 = z(R, 4 * D)
        r.ff32 = z(R * Fmax)
        r.z = z(self.k + n, D)                                        # the slot's k stored taps, then the piece's encoder rows
        r.y32, r.e32 = z(n, D), z(n, D)
        r.a32, r.a16, r.o32, r.qkv32 = z(R, D), z(R, D, dt=F16), z(R, D), z(R, 3 * D)
        r.attr, r.logits = z(R * D), z(R)
        r.ws = z(ops.retention_prefill_ws(C, self.H, n))
        return r

    def _prefill_piece(self, r, s, x, t_enc, t_dec, ne):
        """Slot s takes the N frames x (N, in) f32 at encoder position t_enc; the last ne of the N windows emit, at decoder
        position t_dec.  -> logits (1, ne, C), a view of the row set.  `_body` with B = 1 and Tp = N: the retention prefill on
        the slot's own state sequences, the conv prefill on its cache rows, and the Conv1d reading the emitting windows as
        overlapping rows of z."""
        P, C, D, H, k, N = self.m._prepare(), self.C, self.D, self.H, self.k, x.shape[0]
        h32, h16 = r.h32[:N], r.h16[:N]
        ret = lambda i, Bk, q32, **out: ops.retention_prefill(q32, self.enc_kv[i], r.ws, s, 1, H, t_enc, N, Bk["gn_eps"], **out)
        dwconv = lambda i, Bk, glu16, dw16: ops.dwconv_prefill(glu16, self.caches[i], s, t_enc, Bk["dw"], Bk["bn"], dw16, Bk["bn_eps"])
        f32_input(P, x, r.xin32[:N], h32, h16)
        f32_blocks(P, h32, h16, r.x16[:N], r.xn32[:N], r.q32[:N], r.o16[:N], r.glu16[:N], r.dw16[:N], r.ff32, ret, dwconv)
        # look-ahead window (f32): z = the stored taps, then the new frames; the window after push m is z[m .. m + k - 1]
        r.z[:k].copy_(self.win32[s].view(k, D))
        r.z[k:k + N].copy_(h32)
        self.win32[s].copy_(r.z[N:N + k].reshape(-1))
        if not ne:
            return r.logits[:0].view(1, 0, C)
        cols = r.z.as_strided((ne, k * D), (D, 1), r.z.storage_offset() + (N - ne + 1) * D)
        e32 = r.e32[:ne]
        ops.linear_step_f32(cols, P["cnn.w32"], P["cnn.b"], r.y32[:ne])
        ops.l2norm_rows_f32(r.y32[:ne], e32)
        R = C * ne
        a32 = r.a32[:R]
        ops.convert_fanout_f32(e32, P["convert.w32"], convert_const(self.m, C), a32, r.a16[:R], 1, ne, C)
        ret = lambda i, Ld, q32, **out: ops.retention_prefill(q32, self.dec_kv[i], r.ws, s * C, C, H, t_dec, ne, Ld["gn_eps"], **out)
        f32_dec_layers(P, a32, r.q32[:R], r.o32[:R], r.qkv32[:R], r.ff32, ret, 1, C, ne)
        logits = r.logits[:R].view(1, ne, C)
        ops.head_l2dot(e32, a32, r.attr[:R * D].view(1, ne, C, D), logits, 1, ne, ne, C, D)
        return logits

    @torch.no_grad()
    def prefill(self, s: int, feats):
        """Take open slot `s`, at any position, forward by the T >= 0 frames feats ((T, in) or (1, T, in)) in one pass at batch
        rate: the slot's retention states, conv caches, look-ahead window, counters and accounting end as after T pushes through
        `step`, and the slot streams on from there.  -> logits (1, m, C), m = max(0, min(T, t + T - conv_delay)): the frames it
        emitted, in order.  No other slot is touched; flushing stays with step / step_frames.  Runs eagerly on the current stream
        in pieces of at most prefill_rows frames.  The retention prefill has one work item per (sequence, head, 64 frames): a
        few frames are step_frames' case, not this one's."""
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
            if self._pre is None:
                self._pre = self._alloc_prefill(self.m._prepare())
            x = x.to(device=self.dev, dtype=F32).contiguous()
            for a in range(0, T, self.prefill_rows):
                xp = x[a:a + self.prefill_rows]
                plan = self.table.plan_prefill(s, int(xp.shape[0]))
                y = self._prefill_piece(self._pre, s, xp, self.table.n_enc[s], self.table.n_dec[s], plan.dec[s])
                self.table.commit(plan)
                self.len_enc[s] = self.table.n_enc[s]
                self.len_dec[s] = self.table.n_dec[s]
                if plan.dec[s]:
                    out.append(y.clone())
        if not out:
            return torch.zeros(1, 0, self.C, dtype=F32, device=self.dev)
        return out[0] if len(out) == 1 else torch.cat(out, dim=1)
