"""Host-side mirror of the reference's FS-EEND batch ("masked") model.

Drop-in for ``nnet.model.onl_tfm_enc_1dcnn_enc_linear_non_autoreg_pos_enc_l2norm``
(reference FS-EEND/nnet/model/...l2norm.py): same class names, constructor
arguments, attribute tree (what utils/copy_params.py:7-57 walks) and
``state_dict`` keys (106 entries incl. the dead ``dec.encoder*`` / ``norm12``
tensors and the ``dec.pos_enc.pe`` buffer), so reference checkpoints load with
``load_state_dict`` and default initialisation under a given
``torch.manual_seed`` is bit-identical (modules are created in the reference's
order with the same torch.nn initialisers).

The torch.nn modules here are *parameter containers only*: ``forward`` /
``test`` never call them.  All arithmetic runs in libeend_hip.so (ops.py).
"""
import copy
import math
from typing import List, Optional, Sequence

import torch
import torch.nn as nn
from torch import Tensor

from . import ops
from .weights import (PreparedOperands, _f16, _f32, _qscaled, convert_const, encoder_layer_operands, input_operands,
                      need_gpu_params)

_D_SUPPORTED = 256
_H_SUPPORTED = 4
# One fast form + one general fallback per operator, selected by SHAPE (round 6: the A/B environment switches of rounds 1 - 5 are gone;
# their questions are answered in profiles/OPTIMISATION_LOG.md):
#   encoder input      encin.hip (320 < in_size <= 384)              | gather + BatchNorm + linear_res_ln
#   time-axis MHA      attn_stream.hip (Tp <= 512, packed weights)   | in-projection + attn.hip (longer chunks)
#   decoder layer      dec_stream.hip (C = 3 / 6, F % 64 == 0, F <= 2048: head and tail in one launch) | the two launches below
#   layer head         spk_stream.hip (C <= 12: the limit of every speaker-axis kernel)
#   layer tail         ffn_stream.hip (F % 64 == 0)                  | attnout_ffn_fused_res16 (ffn.hip)
#   look-ahead conv    conv_stream.hip (256 channels)                | implicit-GEMM epilogue (gemm.hip)
# The stacks are post-norm, so the residual of every sub-layer is the previous LayerNorm's output: its f16 copy (the next MFMA operand
# anyway) IS the residual stream; no f32 stream exists between the layers (oracle emulation: max |d logit| 2.4e-4 -> 2.6e-4).


class PositionalEncoding(nn.Module):
    """Sinusoid table, rows indexed by *speaker slot* (reference model :190-224)."""

    def __init__(self, d_model, dropout=0.1, max_len=5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe.unsqueeze(0))


class TransformerEncoder(nn.Module):
    """Layer-stack container (reference modules/merge_tfm_encoder.py:17-43): N deep copies."""

    def __init__(self, encoder_layer, num_layers, norm=None):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(encoder_layer) for _ in range(num_layers)])
        self.num_layers = num_layers
        self.norm = norm


class TransformerEncoderFusionLayer(nn.Module):
    """Parameters of the time x speaker fusion layer (merge_tfm_encoder.py:197-233)."""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, layer_norm_eps=1e-5,
                 batch_first=True):
        super().__init__()
        self.self_attn1 = nn.MultiheadAttention(d_model, nhead, dropout=dropout, batch_first=batch_first)
        self.self_attn2 = nn.MultiheadAttention(d_model, nhead, dropout=dropout, batch_first=batch_first)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm11 = nn.LayerNorm(d_model, eps=layer_norm_eps)
        self.norm12 = nn.LayerNorm(d_model, eps=layer_norm_eps)      # unused by the reference too (:361)
        self.norm21 = nn.LayerNorm(d_model, eps=layer_norm_eps)
        self.norm22 = nn.LayerNorm(d_model, eps=layer_norm_eps)
        self.dropout11 = nn.Dropout(dropout)
        self.dropout21 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)


class MaskedTransformerEncoderModel(nn.Module):
    """Parameters of the embedding encoder (reference model :120-160)."""

    def __init__(self, in_size, n_heads, n_units, n_layers, dim_feedforward=2048, dropout=0.5,
                 has_mask=False, max_seqlen=500, has_pos=False, mask_delay=0):
        super().__init__()
        self.in_size, self.n_heads, self.n_units, self.n_layers = in_size, n_heads, n_units, n_layers
        self.has_pos, self.has_mask, self.max_seqlen, self.mask_delay = has_pos, has_mask, max_seqlen, mask_delay
        if has_pos:
            raise NotImplementedError("has_pos=True is not used by any reference config")
        self.bn = nn.BatchNorm1d(in_size)
        self.encoder = nn.Linear(in_size, n_units)
        self.encoder_norm = nn.LayerNorm(n_units)
        encoder_layers = nn.TransformerEncoderLayer(n_units, n_heads, dim_feedforward, dropout)
        self.transformer_encoder = TransformerEncoder(encoder_layers, n_layers)
        self.init_weights()

    def init_weights(self):
        initrange = 0.1
        self.encoder.bias.data.zero_()
        self.encoder.weight.data.uniform_(-initrange, initrange)


class MaskedTransformerDecoderModel(nn.Module):
    """Parameters of the attractor decoder (reference model :87-105)."""

    def __init__(self, in_size, n_heads, n_units, n_layers, dim_feedforward, dropout=0.5, has_mask=False,
                 max_seqlen=500, has_pos=False, mask_delay=0):
        super().__init__()
        self.in_size, self.n_heads, self.n_units, self.n_layers = in_size, n_heads, n_units, n_layers
        self.has_pos, self.has_mask, self.max_seqlen, self.mask_delay = has_pos, has_mask, max_seqlen, mask_delay
        self.encoder = nn.Linear(in_size, n_units)          # dead in the reference, kept for checkpoints
        self.encoder_norm = nn.LayerNorm(n_units)           # dead
        self.pos_enc = PositionalEncoding(n_units, dropout)
        self.convert = nn.Linear(n_units * 2, n_units)
        decoder_layers = TransformerEncoderFusionLayer(n_units, n_heads, dim_feedforward, dropout, batch_first=True)
        self.attractor_decoder = TransformerEncoder(decoder_layers, n_layers)


class _Workspace:
    """Device buffers for one (B, Tp, C) problem shape (allocated once, reused)."""

    def __init__(self, dev, B, Tp, C, D, F_enc, F_dec, Fin_pad, H):
        f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32
        Me, Md = B * Tp, B * C * Tp
        Mx = max(Me, Md)
        e = lambda *s, dt: torch.empty(*s, dtype=dt, device=dev)
        self.xin16 = torch.zeros(Me, Fin_pad, dtype=f16, device=dev)
        self.h16 = e(Me, D, dt=f16)
        # windows of more than 512 frames: partial rows + softmax denominators of the grouped form (attn_stream.hip), or -- where that form
        # does not cover the shape -- bf16 Q / K / V^T of the un-packed path; both allocated at first use (grow-only)
        self.q = self.k = self.vt = None
        self.attn_part, self.attn_lse = e(0, dt=f16), e(0, dt=f32)
        self.o16 = e(Mx, D, dt=f16)
        self.emb16 = e(Me, D, dt=f16)
        self.a16 = e(Md, D, dt=f16)


class WorkspaceCache:
    """Activation workspaces keyed by shape, least-recently-used eviction under a byte budget (EEND_WS_BUDGET_GB, default
    24): ragged real-world inference walks through many (B, Tp, C) shapes, and dropping every workspace whenever a count is
    exceeded re-allocates multi-GB slabs per call.  The entry in use is never evicted."""

    def __init__(self, budget_bytes: Optional[int] = None, max_entries: int = 32):
        import os
        from collections import OrderedDict
        self._d = OrderedDict()
        self.budget = int(float(os.environ.get("EEND_WS_BUDGET_GB", "24")) * 2 ** 30) if budget_bytes is None else budget_bytes
        self.max_entries = max_entries

    @staticmethod
    def nbytes(ws) -> int:
        return sum(t.numel() * t.element_size() for t in vars(ws).values() if isinstance(t, Tensor))

    def get(self, key):
        ws = self._d.get(key)
        if ws is not None:
            self._d.move_to_end(key)
        return ws

    def put(self, key, ws):
        self._d[key] = ws
        total = sum(self.nbytes(w) for w in self._d.values())
        while len(self._d) > 1 and (total > self.budget or len(self._d) > self.max_entries):
            _, old = self._d.popitem(last=False)
            total -= self.nbytes(old)

    def clear(self):
        self._d.clear()

    def __len__(self):
        return len(self._d)


def time_attention(ws, x16, Ly, nseq, H, Tp, delay, kv, key="in", slots=None, slot_delta=None):
    """in-projection + causal MHA over the frames of `nseq` sequences of the rows x16 -> ws.o16 rows (merge_tfm_encoder.py:379-385).
    Ly[key + "_w" / "_wp" / "_b"] are the layer's q-scaled in-projection operands; delay >= Tp switches the causal mask off, kv is
    the number of real frames.  The form is chosen by Tp (and `slots`) alone."""
    o = ws.o16[:nseq * Tp]
    wp, b = Ly[key + "_wp"], Ly[key + "_b"]
    if slots is not None and Tp == 512:
        # the sequences are the fan-out's speaker slots: K / V projected once per utterance, from the rows of slot 0 (slot form)
        ops.inproj_attn_causal_packed(x16, wp, b, o, nseq, H, Tp, delay, kv, slots=slots, slot_delta=slot_delta)
        return o
    if Tp <= 512:            # token-owning waves, packed weights, Q in registers, K / V never leave the CU (attn_stream.hip)
        ops.inproj_attn_causal_packed(x16, wp, b, o, nseq, H, Tp, delay, kv)
        return o
    # (same-box A/B, 163840 frames: Tp 1024 326 vs 454 us, 2048 586 vs 664 us, 4096 1098 vs 1090 us -- an item re-projects its key
    #  group's K / V, so the grouped form stops paying at about six groups)
    need = ops.inproj_attn_long_scratch(nseq, Tp, delay, kv) if Tp <= 3072 else None
    if need is not None:     # the same kernel on (query group, key group) items of 512 frames + a combine pass over the partial rows
        if ws.attn_part.numel() < need[0]:
            ws.attn_part = torch.empty(need[0], dtype=torch.float16, device=o.device)
        if ws.attn_lse.numel() < need[1]:
            ws.attn_lse = torch.empty(need[1], dtype=torch.float32, device=o.device)
        ops.inproj_attn_causal_long(x16, wp, b, o, ws.attn_part, ws.attn_lse, nseq, H, Tp, delay, kv)
    else:                    # bf16 Q / K / V^T through HBM, tiled attention kernel; the scratch, made at first use, covers every o16 row
        n = nseq * Tp * o.shape[1]
        if ws.q is None:
            ws.q, ws.k, ws.vt = (torch.empty(ws.o16.numel(), dtype=torch.bfloat16, device=o.device) for _ in range(3))
        ops.inproj_heads(x16, Ly[key + "_w"], b, ws.q[:n], ws.k[:n], ws.vt[:n], nseq, Tp, H)
        ops.attn_causal(ws.q[:n], ws.k[:n], ws.vt[:n], o, nseq, H, Tp, delay, kv, scale=ops.LN2)
    return o


def encoder_layer(ws, L, nseq, H, Tp, delay, kv, out32=None):
    """One post-norm encoder layer (operands: weights.encoder_layer_operands) on the rows ws.h16, in place; out32: the rows in f32 too."""
    o16 = time_attention(ws, ws.h16, L, nseq, H, Tp, delay, kv)
    if "ws" in L:            # out-projection + norm1 + FFN + norm2 in one launch on the packed weight stream (ffn_stream.hip)
        ops.attnout_ffn_stream(o16, L["ws"], L["out_b"], None, ws.h16, L["g1"], L["be1"], L["eps1"], L["b1"], L["b2"], L["g2"],
                               L["be2"], L["eps2"], out32, ws.h16)
    else:                    # hidden sizes the packed stream does not take (ffn.hip)
        ops.attnout_ffn_fused_res16(o16, L["out_w"], L["out_b"], ws.h16, L["g1"], L["be1"], L["eps1"], L["w1"], L["b1"],
                                    L["w2"], L["b2"], L["g2"], L["be2"], L["eps2"], out32, ws.h16)


class OnlineTransformerDADiarization(PreparedOperands, nn.Module):
    """FS-EEND batch model on MI355X (reference model :10-84)."""

    def __init__(self, n_speakers, in_size, n_units, n_heads, enc_n_layers, dec_n_layers, dropout, has_mask,
                 max_seqlen, dec_dim_feedforward, conv_delay=9, mask_delay=0, decom_kernel_size=64):
        super().__init__()
        if n_units != _D_SUPPORTED or n_heads != _H_SUPPORTED:
            raise NotImplementedError("HIP kernels are specialised for n_units=256, n_heads=4 (all reference configs)")
        self.n_speakers = n_speakers
        self.delay = conv_delay
        self.enc = MaskedTransformerEncoderModel(in_size, n_heads, n_units, enc_n_layers, dropout=dropout,
                                                 has_mask=has_mask, max_seqlen=max_seqlen, mask_delay=mask_delay)
        self.dec = MaskedTransformerDecoderModel(in_size, n_heads, n_units, dec_n_layers,
                                                 dim_feedforward=dec_dim_feedforward, dropout=dropout,
                                                 has_mask=has_mask, max_seqlen=max_seqlen, mask_delay=mask_delay)
        # NB padding is hard-coded 9 in the reference (model :30), whatever conv_delay is
        self.cnn = nn.Conv1d(n_units, n_units, kernel_size=2 * conv_delay + 1, padding=9)
        self._ws = WorkspaceCache()

    # ------------------------------------------------------------------ weight preparation (the cache: weights.PreparedOperands)
    def _build_operands(self):
        """f16 MFMA-operand copies of the weights in kernel layouts."""
        need_gpu_params(self.cnn.weight)
        P = {}
        enc = self.enc
        (P["enc.in.w"], P["enc.in.b"], P["enc.in.g"], P["enc.in.beta"], P["enc.in.eps"], P["Fin_pad"],
         P["bn"]) = input_operands(enc.encoder, enc.encoder_norm, enc.in_size, enc.bn)
        P["bn.eps"] = enc.bn.eps
        P["enc.layers"] = [encoder_layer_operands(l, keep_unpacked=True) for l in enc.transformer_encoder.layers]
        cw = self.cnn.weight.detach()                       # (Dout, Din, k)
        P["cnn.w"] = cw.permute(0, 2, 1).reshape(cw.shape[0], -1).to(torch.float16).contiguous()
        P["cnn.b"] = _f32(self.cnn.bias)
        P["cnn.k"], P["cnn.pad"] = cw.shape[2], self.cnn.padding[0]
        if ops.conv_stream_ok(cw.shape[1], cw.shape[2], self.cnn.padding[0]) and cw.shape[0] == 256:
            P["cnn.ws"] = ops.conv_stream_pack(P["cnn.w"], cw.shape[2])
        D = enc.n_units
        P["convert.w1"] = _f16(self.dec.convert.weight[:, :D])
        dl = []
        for l in self.dec.attractor_decoder.layers:
            dl.append(dict(
                in1_w=_f16(_qscaled(l.self_attn1.in_proj_weight)), in1_b=_f32(_qscaled(l.self_attn1.in_proj_bias)),
                out1_w=_f16(l.self_attn1.out_proj.weight), out1_b=_f32(l.self_attn1.out_proj.bias),
                in2_w=_f16(l.self_attn2.in_proj_weight), in2_b=_f32(l.self_attn2.in_proj_bias),
                out2_w=_f16(l.self_attn2.out_proj.weight), out2_b=_f32(l.self_attn2.out_proj.bias),
                w1=_f16(l.linear1.weight), b1=_f32(l.linear1.bias), w2=_f16(l.linear2.weight), b2=_f32(l.linear2.bias),
                g11=_f32(l.norm11.weight), be11=_f32(l.norm11.bias), eps11=l.norm11.eps,
                g21=_f32(l.norm21.weight), be21=_f32(l.norm21.bias), eps21=l.norm21.eps,
                g22=_f32(l.norm22.weight), be22=_f32(l.norm22.bias), eps22=l.norm22.eps))
        for L in dl:
            if ops.stream_ok(L["w1"].shape[0]):
                L["ws"] = ops.ffn_stream_pack(L["out2_w"], L["w1"], L["w2"])
            L["ws1"] = ops.spk_stream_pack(L["out1_w"], L["in2_w"])
            if ops.stream_ok(L["w1"].shape[0]):
                L["wsd"] = ops.dec_stream_pack(L["out1_w"], L["in2_w"], L["out2_w"], L["w1"], L["w2"])
            L["in1_wp"] = ops.inproj_attn_pack(L["in1_w"])
        P["dec.layers"] = dl
        return P

    def _slot_delta(self, C):
        """slot_delta[c] = (W_q d_c | W_v d_c), d_c = pc[c] - pc[0]  (a (C, 512) f32 constant of the weights): what the slot constants of
        the fan-out become behind the first fusion layer's time-axis in-projection.  W is the f16 operand copy the kernel multiplies
        with (q rows pre-scaled), the products are summed in f32; cached like convert_const, per parameter version and slot count."""
        def build():
            W = self._prep["dec.layers"][0]["in1_w"].to(torch.float32)
            pc = convert_const(self, C)
            d = pc - pc[:1]
            sd = (d[:, None, :] * torch.cat([W[:256], W[512:]])[None]).sum(-1)
            sd[0] = 0.0
            return sd.contiguous()

        return self._derived(("sd", C), build)

    @property
    def _sd(self):
        """{C: slot delta} of the present operand set: a read-only view of the derived cache."""
        return {k[1]: v for k, v in self._consts.items() if k[0] == "sd"}

    def _workspace(self, dev, B, Tp, C):
        key = (str(dev), B, Tp, C)
        ws = self._ws.get(key)
        if ws is None:
            P = self._prep
            F_enc = P["enc.layers"][0]["w1"].shape[0] if P["enc.layers"] else 0
            F_dec = P["dec.layers"][0]["w1"].shape[0] if P["dec.layers"] else 0
            ws = _Workspace(dev, B, Tp, C, self.enc.n_units, F_enc, F_dec, P["Fin_pad"], self.enc.n_heads)
            self._ws.put(key, ws)
        return ws

    # ------------------------------------------------------------------ the hot path
    def _run(self, src: Sequence[Tensor], ilens: Sequence[int], C: int):
        """encoder -> look-ahead conv + L2 -> attractor decoder -> head, all in HIP.
        Returns (logits (B,T,C), emb slab (B,Tp,D) f32, attractors (B,T,C,D), T, Tp)."""
        P = self._prepare()
        dev = self.cnn.weight.device
        D, H = self.enc.n_units, self.enc.n_heads
        srcs = [s.to(device=dev, dtype=torch.float32).contiguous() for s in src]
        B, T = len(srcs), max(int(s.shape[0]) for s in srcs)
        Tp = ops.frames_pad(T)
        ws = self._workspace(dev, B, Tp, C)
        il_key = tuple(min(int(l), T) for l in ilens)
        if getattr(ws, "il_key", None) != il_key:           # cached: no H2D copy inside a captured step
            ws.il = torch.tensor(il_key, dtype=torch.int32, device=dev)
            ws.il_key = il_key
        il = ws.il
        Me, Md = B * Tp, B * C * Tp
        delay_e = self.enc.mask_delay if self.enc.has_mask else Tp
        kv_e = T          # keys are the T real frames of the padded batch (the reference's mask is (T, T)), never slab padding

        # ---- embedding encoder (model :162-188)
        if ops.encoder_input_ok(srcs, Tp, P["enc.in.w"]):
            # pad_sequence(-1) (model :165) + BatchNorm + input projection + LayerNorm in one launch, the f32 features read once (encin.hip)
            ops.encoder_input(srcs, P["bn"], P["enc.in.w"], P["enc.in.b"], P["enc.in.g"], P["enc.in.beta"], None, ws.h16, T, Tp, -1.0,
                              P["bn.eps"], P["enc.in.eps"])
        else:
            ops.gather_bn_cast_pad(srcs, P["bn"], ws.xin16, T, Tp, -1.0, True, P["bn.eps"])
            ops.linear_res_ln(ws.xin16, P["enc.in.w"], P["enc.in.b"], None, P["enc.in.g"], P["enc.in.beta"], None, ws.h16, P["enc.in.eps"])
        for L in P["enc.layers"]:
            encoder_layer(ws, L, B, H, Tp, delay_e, kv_e)

        # ---- truncate to ilen / zero re-pad, look-ahead conv, L2 norm (model :38-41)
        emb32 = torch.empty(Me, D, dtype=torch.float32, device=dev)       # returned to the caller (views, no copies)
        if "cnn.ws" in P:        # packed weight stream (conv_stream.hip)
            ops.conv1d_l2norm_stream(ws.h16, P["cnn.ws"], P["cnn.b"], il, emb32, ws.emb16, B, Tp, P["cnn.k"], P["cnn.pad"])
        else:
            ops.conv1d_l2norm(ws.h16, P["cnn.w"], P["cnn.b"], il, emb32, ws.emb16, B, Tp, D, P["cnn.k"], P["cnn.pad"])

        # ---- attractor decoder (model :112-118, merge_tfm_encoder.py:356-376)
        ops.convert_fanout(ws.emb16, P["convert.w1"], convert_const(self, C), None, ws.a16, B, Tp, C)
        o16 = ws.o16[:Md]
        for li, L in enumerate(P["dec.layers"]):
            # (the first layer reads the fan-out itself: its rows differ by pc[c] between the slots of an utterance)
            slots = C if li == 0 and C <= 12 and Tp == 512 else None
            time_attention(ws, ws.a16, L, B * C, H, Tp, self.dec.mask_delay, T, key="in1", slots=slots,
                           slot_delta=None if slots is None else self._slot_delta(C))
            # out-projection + norm11 + speaker-axis in-projection + C x C attention in one launch (spk_stream.hip; any slot count the
            # speaker-axis kernels take, C <= 12).  It takes no T_valid: the slab's padded frames [T, Tp) are computed too (finite
            # don't-care rows, masked as keys and dropped by the head) -- 2.4 % of the rows at T = 500 / Tp = 512; a per-tile T_valid test
            # would cost the kernel its tile-uniform control flow
            if "wsd" in L and ops.dec_stream_ok(C, Tp):
                # ... and the rest of the layer in the same launch: x1 and O never leave the chip (dec_stream.hip)
                ops.attnout_spk_ffn_stream(o16, L["wsd"], L["out1_b"], ws.a16, L["g11"], L["be11"], L["eps11"], L["in2_b"], L["out2_b"],
                                           L["g21"], L["be21"], L["eps21"], L["b1"], L["b2"], L["g22"], L["be22"], L["eps22"], ws.a16, B, C, Tp)
                continue
            ops.attnout_spk_stream(o16, L["ws1"], L["out1_b"], ws.a16, L["g11"], L["be11"], L["eps11"], ws.a16, L["in2_b"], o16, B, C, Tp)
            if "ws" in L:
                ops.attnout_ffn_stream(o16, L["ws"], L["out2_b"], None, ws.a16, L["g21"], L["be21"], L["eps21"], L["b1"], L["b2"],
                                       L["g22"], L["be22"], L["eps22"], None, ws.a16)
            else:
                ops.attnout_ffn_fused_res16(o16, L["out2_w"], L["out2_b"], ws.a16, L["g21"], L["be21"], L["eps21"], L["w1"], L["b1"],
                                            L["w2"], L["b2"], L["g22"], L["be22"], L["eps22"], None, ws.a16)

        # ---- attractor L2 norm + embedding . attractor head (model :43,:60)
        attr = torch.empty(B, T, C, D, dtype=torch.float32, device=dev)
        logits = torch.empty(B, T, C, dtype=torch.float32, device=dev)
        ops.head_l2dot(emb32, ws.a16, attr, logits, B, T, Tp, C, D)
        emb = emb32.view(B, Tp, D)
        return logits, emb, attr, T, Tp

    @torch.no_grad()
    def test(self, src, ilens, max_nspks=6):
        """reference model :67-84 -> (logits [ (T_i,C) ], emb [ (T_i,D) ], attractors [ (T_i,C,D) ])."""
        logits, emb, attr, T, Tp = self._run(src, ilens, max_nspks)
        output = [logits[b, :l] for b, l in enumerate(ilens)]
        embs = [emb[b, :l] for b, l in enumerate(ilens)]
        attractors = [attr[b, :l] for b, l in enumerate(ilens)]
        return output, embs, attractors

    def forward(self, src, tgt, ilens):
        """reference model :32-65.  Under torch.no_grad(): values only (eval-mode numerics).  With gradients enabled
        (the reference's training_step, FS-EEND/train/oln_tfm_enc_dec.py:49): the HIP forward runs inside a
        torch.autograd.Function whose backward is the hand-written HIP backward (autograd.py) -- `loss.backward()`
        fills `.grad` of every parameter, so the reference's LightningModule / any torch optimiser trains this model."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            from .autograd import fs_forward_with_grad
            return fs_forward_with_grad(self, src, tgt, ilens)
        n_speakers = [t.shape[1] for t in tgt]
        C = max(n_speakers)
        logits, emb, attr, T, Tp = self._run(src, ilens, C)
        dev = logits.device
        # embedding-consistency loss (model :46-57); (B,T,T) cosine maps, training-time diagnostic
        tgt_pad = [nn.functional.pad(t.to(dev, torch.float32), (0, C - t.shape[1])) for t in tgt]
        tgt_pad = nn.utils.rnn.pad_sequence(tgt_pad, padding_value=0.0, batch_first=True).contiguous()
        emb_consis_loss = ops.emb_consistency(emb, tgt_pad, tgt_pad.shape[1])
        output = [logits[b, :l, :n] for b, (l, n) in enumerate(zip(ilens, n_speakers))]
        embs = [emb[b, :l] for b, l in enumerate(ilens)]
        attractors = [attr[b, :l, 1:n] for b, (l, n) in enumerate(zip(ilens, n_speakers))]
        return output, emb_consis_loss, embs, attractors
