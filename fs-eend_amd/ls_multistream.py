"""Many LS-EEND streams in one session: S slots, each carrying its own stream with its own lifetime and stream position, all
advanced by one graph replay per frame.

`LsStreamSession(batch=S)` (ls_stream.py) runs S streams in lockstep: one retention scale for the whole batch, one reset for
all.  Here every buffer has S rows on the encoder side and S*C on the decoder side, every stage computes all rows every frame
with the all-f32 frame step of `ls_stream.enc_step` / `dec_step`, and the three state touches of that step take their stream
position from per-slot int32 lengths in device memory: the retention recurrence (`ops.retention_step_ragged`, scale = the
slot's own frame count), the Conformer depthwise-conv cache (`ops.dwconv_step_ragged`) and the f32 look-ahead window
(`ops.window_push_f32`).  A per-slot mode vector, written with one copy before each replay, decides which state changes.
LS state is O(1) per stream, so one capture serves the whole session (again only when the weights are refreshed).

The per-frame procedure of one slot is LS-EEND/streaming_infer_dia.py:52-97, as in `LsStreamSession`; the slot bookkeeping is
FsMultiStreamSession's (multistream.py): encoder on push, window push or flush, decoder once the look-ahead is full.
"""
from types import SimpleNamespace

import torch

from . import ops
from .lib import EendHipError
from .multistream import MultiStreamSession

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

    State: retention kv f32 (S, H, 64, 64) per encoder block and (S*C, H, 64, 64) per decoder layer, conv caches f32 (S, D, k-1)
    per block, the window f32 (S, k*D) and two int32 length vectors.  States are never cleared: a length of 0 means "empty" to
    every kernel that reads them, so a reopened slot computes exactly what a fresh one does.  step_frames takes one frame per
    slot and step (max_frames = 1)."""

    input_transform = "logmel23_cummn"

    def __init__(self, model, slots: int, max_nspks: int = 10, use_graph: bool = True):
        m = model
        P = m._prepare()
        if max_nspks <= 0 or max_nspks > 16:
            raise EendHipError("max_nspks must be in 1..16 (the f32 speaker attention of the frame step)")
        dev = m.cnn.weight.device
        super().__init__(m, slots, max_nspks, use_graph, P["cnn.k"] // 2, dev)
        self.D, self.H, self.k = m.n_units, m._n_heads, P["cnn.k"]
        S, C, D, H = slots, max_nspks, self.D, self.H
        R = S * C
        K1 = m.enc.encoder._conv_kernel_size - 1
        Fmax = max([Bk["w1a32"].shape[0] for Bk in P["blocks"]] + [Ld["w1_32"].shape[0] for Ld in P["dec.layers"]] + [1])
        z = lambda *s_, dt=F32: torch.zeros(*s_, dtype=dt, device=dev)
        self.x_in = z(S, m._in_size)
        self.xin32 = z(S, P["Fin_pad"])                               # zero-padded input row of the f32 input projection
        self.h32, self.h16, self.x16, self.xn32 = z(S, D), z(S, D, dt=F16), z(S, D, dt=F16), z(S, D)    # encoder rows
        self.o16, self.glu16, self.dw16 = z(S, D, dt=F16), z(S, D, dt=F16), z(S, D, dt=F16)
        self.q32 = z(R, 4 * D)                                        # retention projections (encoder: the first S rows)
        self.ff32 = z(R * Fmax)
        self.win32 = z(S, self.k * D)                                 # [tap*D + c], oldest tap first
        self.y32, self.e32 = z(S, D), z(S, D)
        self.a32, self.a16, self.o32, self.qkv32 = z(R, D), z(R, D, dt=F16), z(R, D), z(R, 3 * D)    # decoder rows
        self.attr = z(S, 1, C, D)
        self.logits = z(S, 1, C)
        self.enc_kv = [z(S, H, 64, 64) for _ in P["blocks"]]
        self.caches = [z(S, D, K1) for _ in P["blocks"]]
        self.dec_kv = [z(R, H, 64, 64) for _ in P["dec.layers"]]
        self.len_enc = z(S, dt=I32)
        self.len_dec = z(S, dt=I32)
        self.modes = z(3, S, dt=I32)                                  # [encoder step, window mode, decoder step]
        self._rows = {1: SimpleNamespace(Tp=1, x_in=self.x_in, ctl=self.modes, logits=self.logits)}

    def _clear_window(self, s):
        self.win32[s].zero_()

    # ---- the frame step (eager body; captured once)
    def _body(self, r):
        P, H, S, C = self.m._prepare(), self.H, self.S, self.C
        enc_m, win_m, dec_m = self.modes[0], self.modes[1], self.modes[2]
        # encoder, S rows: ls_stream.enc_step's all-f32 form, the retention state and conv cache per slot
        h32, h16, x16, xn32 = self.h32, self.h16, self.x16, self.xn32
        self.xin32[:, :self.x_in.shape[1]].copy_(self.x_in)
        ops.linear_res_ln_step_f32(self.xin32, P["in.w32"], P["in.b"], None, P["in.g"], P["in.beta"], h32, P["in.eps"], out16=h16)
        nb = len(P["blocks"])
        q32 = self.q32[:S]
        for i, (Bk, kv, cache) in enumerate(zip(P["blocks"], self.enc_kv, self.caches)):
            ff32 = self.ff32[:S * Bk["w1a32"].shape[0]].view(S, -1)
            if i == 0:
                ops.layernorm_rows_f32(h32, Bk["lna"][0], Bk["lna"][1], xn32, Bk["lna"][2])
            ops.linear_step_f32(xn32, Bk["w1a32"], Bk["b1a"], ff32, act=ops.ACT_SWISH)
            ops.linear_res_scale_ln_step_f32(ff32, Bk["w2a32"], Bk["b2a"], h32, Bk["fa"], Bk["lnb"][0], Bk["lnb"][1], h32,
                                             ln_out16=x16, eps=Bk["lnb"][2])
            ops.retention_proj_step(h32, Bk["lnb"], Bk["wqkvg32"], Bk["bqkvg"], q32, S)
            ops.retention_step_ragged(q32, kv, self.len_enc, enc_m, 1, S, H, Bk["gn_eps"], out16=self.o16)
            ops.linear_res_scale_ln16(self.o16, Bk["wo"], Bk["bo"], h32, 1.0, Bk["lnc"][0], Bk["lnc"][1], h32, x16, Bk["lnc"][2])
            ops.linear_glu(x16, Bk["pw1"], Bk["pb1"], self.glu16)
            ops.dwconv_step_ragged(self.glu16, cache, self.len_enc, enc_m, Bk["dw"], Bk["bn"], self.dw16, Bk["bn_eps"])
            ops.linear_res_scale_ln16(self.dw16, Bk["pw2"], Bk["pb2"], h32, 1.0, Bk["lnd"][0], Bk["lnd"][1], h32, x16, Bk["lnd"][2])
            ops.layernorm_rows_f32(h32, Bk["lnd"][0], Bk["lnd"][1], xn32, Bk["lnd"][2])
            ops.linear_step_f32(xn32, Bk["w1b32"], Bk["b1b"], ff32, act=ops.ACT_SWISH)
            ops.linear_res_ln_step_f32(ff32, Bk["w2b32"], Bk["b2b"], h32, Bk["lne"][0], Bk["lne"][1], h32, Bk["lne"][2], alpha=Bk["fb"],
                                       out16=h16)
            if i + 1 < nb:
                nx = P["blocks"][i + 1]["lna"]
                ops.layernorm_rows_f32(h32, nx[0], nx[1], xn32, nx[2])
        ops.counter_add_masked(self.len_enc, enc_m)
        # look-ahead window (f32), Conv1d, L2 norm: LsStreamSession._conv per slot
        ops.window_push_f32(self.win32, h32, win_m)
        ops.linear_step_f32(self.win32, P["cnn.w32"], P["cnn.b"], self.y32)
        ops.l2norm_rows_f32(self.y32, self.e32)
        # decoder, S*C rows: ls_stream.dec_step's all-f32 form, the retention state per slot
        R = S * C
        a32, o32 = self.a32, self.o32
        ops.convert_fanout_step_f32(self.e32, P["convert.w32"], self.m._convert_const(C), a32, self.a16, S, C)
        for Ld, kv in zip(P["dec.layers"], self.dec_kv):
            ff32 = self.ff32[:R * Ld["w1_32"].shape[0]].view(R, -1)
            ops.retention_proj_step(a32, None, Ld["wqkvg32"], Ld["bqkvg"], self.q32, R)
            ops.retention_step_ragged(self.q32, kv, self.len_dec, dec_m, C, R, H, Ld["gn_eps"], out32=o32)
            ops.linear_res_ln_step_f32(o32, Ld["out1_w32"], Ld["out1_b"], a32, Ld["g11"], Ld["be11"], a32, Ld["eps11"])
            ops.linear_step_f32(a32, Ld["in2_w32"], Ld["in2_b"], self.qkv32)
            ops.spk_attn_step_f32(self.qkv32, o32, S, C)
            ops.linear_res_ln_step_f32(o32, Ld["out2_w32"], Ld["out2_b"], a32, Ld["g21"], Ld["be21"], a32, Ld["eps21"])
            ops.linear_step_f32(a32, Ld["w1_32"], Ld["b1"], ff32, act=ops.ACT_RELU)
            ops.linear_res_ln_step_f32(ff32, Ld["w2_32"], Ld["b2"], a32, Ld["g22"], Ld["be22"], a32, Ld["eps22"])
        ops.counter_add_masked(self.len_dec, dec_m)
        ops.head_l2dot(self.e32, a32, self.attr, self.logits, S, 1, 1, C, self.D)
