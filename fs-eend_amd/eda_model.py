"""Host-side mirror of the reference's offline EEND-EDA baseline, inference only.

Public face of ``nnet.model.offl_tfm_enc_lstm_enc_dec`` (reference FS-EEND/nnet/model/offl_tfm_enc_lstm_enc_dec.py): the same class
names, constructor arguments, attribute tree and ``state_dict`` keys (``enc.encoder.*``, ``enc.encoder_norm.*``,
``enc.transformer_encoder.layers.N.*``, ``eda.encoder.*``, ``eda.decoder.*``, ``eda.counter.*``), so a reference checkpoint loads
with ``load_state_dict`` and default initialisation under a given ``torch.manual_seed`` is the reference's.

The torch.nn modules are parameter containers only; all arithmetic runs in libeend_hip.so:

  encoder      the FS-EEND encoder path without BatchNorm and without a mask (fs_model.encoder_layer): pad_sequence(-1), Linear, LayerNorm,
               then the post-norm layers on the packed stream kernels with unmasked attention over the T rows of the padded batch.
               The reference has no key-padding mask, so in a ragged batch a shorter sequence sees its -1 padding, here as there.
               The last layer also writes its rows in f32: the embeddings are not L2-normalised in this model, and both the LSTM
               and the head read them.
  attractors   the input projection of the encoder LSTM (eend_linear_step_f32), the two recurrences (eend_lstm_f32: the shuffle of
               model :62-65 is an index into the projected rows, the decoder's zero input needs no GEMM), the counter with the
               speaker count (eend_eda_count_f32) and the head (eend_eda_head_f32).

Two quirks of the reference's ``test`` are deliberately not reproduced: with B > 1 it applies the first item's
count to every later item (here every sequence keeps the columns before its own first p < th), and it raises on a recording where
no probability is below ``th`` (here all 15 columns are kept).  ``forward``, the attractor loss and the LSTM backward are out of
scope, as is the Lightning module train/offl_tfm_lstm.py.  The block-online use of this model with a speaker-tracing buffer
(train/tfm_STB.py) is ``fs_eend_amd.stb.StbSession``: it runs ``_encode`` and ``eda._attractors`` on many streams at once, every
stream with its own frame order (a (B, T) ``order``).
"""
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor

from . import ops
from .fs_model import TransformerEncoder, WorkspaceCache, encoder_layer
from .lib import EendHipError
from .weights import PreparedOperands, _f32, encoder_layer_operands, input_operands, need_gpu_params

_D_SUPPORTED = 256
_H_SUPPORTED = 4
MAX_N_SPEAKERS = 15


def _need_gpu(t: Tensor, name: str):
    if not isinstance(t, Tensor) or not t.is_cuda:
        raise EendHipError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")


def check_order(order, T: int) -> np.ndarray:
    """A permutation of 0 .. T-1 as an int32 array, or ValueError."""
    o = np.asarray(order.detach().cpu() if isinstance(order, Tensor) else order)
    if o.ndim != 1 or o.shape[0] != T:
        raise ValueError(f"order must be a 1-D permutation of the {T} frames, got shape {o.shape}")
    if o.dtype == np.bool_ or not np.issubdtype(o.dtype, np.integer):
        raise ValueError(f"order must hold integers, got {o.dtype}")
    o = o.astype(np.int64)
    if o.min() < 0 or o.max() >= T or np.unique(o).shape[0] != T:
        raise ValueError("order is not a permutation of 0 .. T-1")
    return o.astype(np.int32)


class TransformerModel(nn.Module):
    """Parameters of the embedding encoder (reference model :130-167)."""

    def __init__(self, in_size, n_heads, n_units, n_layers, dim_feedforward=2048, dropout=0.5, has_pos=False):
        super().__init__()
        self.in_size, self.n_heads, self.n_units, self.n_layers, self.has_pos = in_size, n_heads, n_units, n_layers, has_pos
        if has_pos:
            raise NotImplementedError("has_pos=True is not used by any reference config")
        self.src_mask = None
        self.encoder = nn.Linear(in_size, n_units)
        self.encoder_norm = nn.LayerNorm(n_units)
        encoder_layers = nn.TransformerEncoderLayer(n_units, n_heads, dim_feedforward, dropout)
        self.transformer_encoder = TransformerEncoder(encoder_layers, n_layers)
        self.init_weights()

    def init_weights(self):
        initrange = 0.1
        self.encoder.bias.data.zero_()
        self.encoder.weight.data.uniform_(-initrange, initrange)


class _EdaWorkspace:
    def __init__(self, dev, B, Tp, D, Fin_pad):
        Me = B * Tp
        self.xin16 = torch.zeros(Me, Fin_pad, dtype=torch.float16, device=dev)
        self.h16 = torch.empty(Me, D, dtype=torch.float16, device=dev)
        self.o16 = torch.empty(Me, D, dtype=torch.float16, device=dev)
        self.attn_part = torch.empty(0, dtype=torch.float16, device=dev)
        self.attn_lse = torch.empty(0, dtype=torch.float32, device=dev)
        self.q = self.k = self.vt = None


class EncoderDecoderAttractor(PreparedOperands, nn.Module):
    """LSTM encoder-decoder attractor calculation (reference model :79-107), inference only."""

    def __init__(self, n_units, encoder_dropout=0.1, decoder_dropout=0.1):
        super().__init__()
        if n_units != _D_SUPPORTED:
            raise NotImplementedError("the LSTM kernel is specialised for n_units=256 (all reference configs)")
        # (single-layer nn.LSTM ignores its dropout and warns about it; the values are kept as attributes only)
        self.encoder_dropout, self.decoder_dropout = encoder_dropout, decoder_dropout
        self.encoder = nn.LSTM(n_units, n_units, 1, batch_first=True)
        self.decoder = nn.LSTM(n_units, n_units, 1, batch_first=True)
        self.counter = nn.Linear(n_units, 1)
        self.n_units = n_units

    def _fingerprint_tensors(self):
        return list(self.parameters())

    def _build_operands(self):
        """f32 operand copies of the two LSTMs and the counter."""
        need_gpu_params(self.counter.weight)
        e, d = self.encoder, self.decoder
        P = dict(enc_wih=_f32(e.weight_ih_l0), enc_whh=_f32(e.weight_hh_l0),
                 enc_b=(_f32(e.bias_ih_l0) + _f32(e.bias_hh_l0)).contiguous(),
                 dec_whh=_f32(d.weight_hh_l0), dec_b=(_f32(d.bias_ih_l0) + _f32(d.bias_hh_l0)).contiguous(),
                 cnt_w=_f32(self.counter.weight).view(-1), cnt_b=_f32(self.counter.bias).view(-1))
        return P

    def _attractors(self, rows32: Tensor, T: int, order: Optional[Tensor], max_n_speakers: int, th: Optional[float]):
        """rows32 f32 (B, rows >= T, D) -> attractors (B, C, D), probs (B, C), count i32 (B,) or None.  Step t of the encoder LSTM
        reads row order[t]; order i32 (T,) for the batch or (B, T), one per sequence."""
        P = self._prepare()
        B, rows, D = rows32.shape
        dev = rows32.device
        C = int(max_n_speakers)
        if not ops.lstm_ok(B, T, D) or not 1 <= C <= 16:
            raise EendHipError(f"EDA attractors: unsupported shape B={B}, T={T}, D={D}, C={C}")
        f32 = dict(dtype=torch.float32, device=dev)
        G = torch.empty(B, rows, 4 * D, **f32)
        ops.linear_step_f32(rows32.view(B * rows, D), P["enc_wih"], P["enc_b"], G.view(B * rows, 4 * D))
        hT, cT, hD, cD = (torch.empty(B, D, **f32) for _ in range(4))
        ops.lstm(G, order, None, P["enc_whh"], None, None, hT, cT, None, B, T)
        attractors = torch.empty(B, C, D, **f32)
        ops.lstm(None, None, P["dec_b"], P["dec_whh"], hT, cT, hD, cD, attractors, B, C)       # zero input: no GEMM
        probs = torch.empty(B, C, **f32)
        count = torch.empty(B, dtype=torch.int32, device=dev) if th is not None else None
        ops.eda_count(attractors, P["cnt_w"], P["cnt_b"], 0.0 if th is None else th, probs, count)
        return attractors, probs, count

    @torch.no_grad()
    def estimate(self, xs: Tensor, max_n_speakers: int = MAX_N_SPEAKERS):
        """Attractors from embedding sequences without prior knowledge of the number of speakers (reference model :94-107):
        xs (B, T, E) in the order the LSTM is to read them -> (attractors (B, C, E), probs (B, C))."""
        _need_gpu(xs, "xs")
        if xs.dim() != 3:
            raise EendHipError("estimate: xs must be (B, T, E)")
        xs = xs.detach().to(torch.float32).contiguous()
        attractors, probs, _ = self._attractors(xs, xs.shape[1], None, max_n_speakers, None)
        return attractors, probs


class TransformerEDADiarization(PreparedOperands, nn.Module):
    """Offline EEND-EDA on MI355X (reference model :10-76), inference only."""

    def __init__(self, n_speakers, in_size, n_units, n_heads, n_layers, dropout, attractor_loss_ratio=1.0,
                 attractor_encoder_dropout=0.1, attractor_decoder_dropout=0.1):
        super().__init__()
        if n_units != _D_SUPPORTED or n_heads != _H_SUPPORTED:
            raise NotImplementedError("HIP kernels are specialised for n_units=256, n_heads=4 (all reference configs)")
        self.n_speakers = n_speakers
        self.enc = TransformerModel(in_size, n_heads, n_units, n_layers, dropout=dropout)
        self.eda = EncoderDecoderAttractor(n_units, encoder_dropout=attractor_encoder_dropout,
                                           decoder_dropout=attractor_decoder_dropout)
        self.attractor_loss_ratio = attractor_loss_ratio
        self._ws = WorkspaceCache()

    def refresh_weights(self):
        super().refresh_weights()
        self.eda.refresh_weights()

    def _fingerprint_tensors(self):
        return list(self.enc.parameters())

    def _build_operands(self):
        """f16 MFMA-operand copies of the encoder weights in the layouts of the packed stream kernels."""
        enc = self.enc
        need_gpu_params(enc.encoder.weight)
        P = {}
        P["in.w"], P["in.b"], P["in.g"], P["in.beta"], P["in.eps"], P["Fin_pad"] = input_operands(enc.encoder, enc.encoder_norm,
                                                                                                  enc.in_size)
        for l in enc.transformer_encoder.layers:
            if not ops.stream_ok(l.linear1.weight.shape[0]):
                raise EendHipError("EEND-EDA encoder: the packed stream kernels take hidden widths that are multiples of 64 up to 2048")
        P["layers"] = [encoder_layer_operands(l, keep_unpacked=False) for l in enc.transformer_encoder.layers]
        return P

    def _encode(self, src: Sequence[Tensor]):
        """pad_sequence(-1) + Linear + LayerNorm + the layer stack (reference model :169-193) -> f32 slab (B, Tp, D), T."""
        P = self._prepare()
        enc = self.enc
        dev = enc.encoder.weight.device
        D, H = enc.n_units, enc.n_heads
        for s in src:
            _need_gpu(s, "src[i]")
        srcs = [s.detach().to(device=dev, dtype=torch.float32).contiguous() for s in src]
        B, T = len(srcs), max(int(s.shape[0]) for s in srcs)
        Tp = ops.frames_pad(T)
        key = (str(dev), B, Tp)
        ws = self._ws.get(key)
        if ws is None:
            ws = _EdaWorkspace(dev, B, Tp, D, P["Fin_pad"])
            self._ws.put(key, ws)
        Me = B * Tp
        emb32 = torch.empty(Me, D, dtype=torch.float32, device=dev)       # returned to the caller
        n_layers = len(P["layers"])
        ops.gather_bn_cast_pad(srcs, None, ws.xin16, T, Tp, -1.0, False)
        ops.linear_res_ln(ws.xin16, P["in.w"], P["in.b"], None, P["in.g"], P["in.beta"], emb32 if n_layers == 0 else None, ws.h16,
                          P["in.eps"])
        for li, L in enumerate(P["layers"]):
            # unmasked MHA over the T rows of the padded batch (delay >= Tp switches the causal mask off, kv_len = T keeps the slab's
            # own padding out); the last layer's rows also in f32
            encoder_layer(ws, L, B, H, Tp, Tp, T, out32=emb32 if li == n_layers - 1 else None)
        return emb32.view(B, Tp, D), T

    @torch.no_grad()
    def test(self, src, ilens, n_spk=None, th=None, order=None):
        """reference model :54-76 -> (output_active [ (ilen_i, n_i) ], emb (B, T, E), attractors[:, :-1, :] (B, 14, E)).
        With `n_spk` the first n_spk columns are kept; with `th` every sequence keeps the columns before its own first p < th (all
        15 if there is none).  `order` is the permutation in which the encoder LSTM reads the T frames: None draws it the way the
        reference does (np.arange(T), np.random.shuffle -- the same numpy seed gives the same order).
        The call's full tensors stay readable afterwards: `last_logits` (B, T, 15), `last_probs` (B, 15), `last_counts` [B]."""
        if n_spk is None and th is None:
            raise ValueError("test() needs n_spk or th to choose the speaker columns")
        if len(src) != len(ilens) or len(src) == 0:
            raise ValueError("src and ilens must be non-empty lists of one length")
        T = max(int(s.shape[0]) for s in src)
        if order is None:
            order = np.arange(T)
            np.random.shuffle(order)
        order = check_order(order, T)
        emb_slab, T = self._encode(src)
        dev = emb_slab.device
        B = emb_slab.shape[0]
        order_dev = torch.from_numpy(order).to(dev)
        attractors, probs, count = self.eda._attractors(emb_slab, T, order_dev, MAX_N_SPEAKERS, None if n_spk is not None else float(th))
        logits = torch.empty(B, T, MAX_N_SPEAKERS, dtype=torch.float32, device=dev)
        ops.eda_head(emb_slab, attractors, logits, T)
        counts = [int(n_spk)] * B if n_spk is not None else count.tolist()
        self.last_probs, self.last_counts, self.last_logits = probs, counts, logits
        output_active = [logits[b, :int(l), :counts[b]] for b, l in enumerate(ilens)]
        return output_active, emb_slab[:, :T], attractors[:, :-1, :]

    def forward(self, src, tgt, ilens):
        raise NotImplementedError("EEND-EDA training (forward, the attractor loss, the LSTM backward) is out of scope: inference only")
