"""Host-side mirror of the reference's offline EEND-EDA baseline: inference, and a differentiable attractor path.

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
  attractors   one pass for inference and training (``_attractor_pass``): the input projection of the encoder LSTM
               (eend_linear_step_f32) and the two recurrences (eend_lstm_train_f32, which keeps nothing and runs the inference
               kernel unless the backward's buffers are given: the shuffle of model :62-65 is an index into the projected rows, the
               decoder's zero input needs no GEMM); then the counter with the speaker count (eend_eda_count_f32) and the head
               (eend_eda_head_f32).

Two quirks of the reference's ``test`` are deliberately not reproduced: with B > 1 it applies the first item's
count to every later item (here every sequence keeps the columns before its own first p < th), and it raises on a recording where
no probability is below ``th`` (here all 15 columns are kept).

Training.  The attractor path is differentiable end to end: ``EncoderDecoderAttractor.forward(xs, n_speakers, order=None)`` is the
reference's (model :109-127) as a ``torch.autograd.Function`` over eend_lstm_train_f32 (the inference recurrence that also keeps
gates, cell states and the entering hidden states), eend_eda_count_loss_f32 (the attractor-existence loss and its gradients),
eend_lstm_bwd_f32 (the recurrence backwards, decoder then encoder) and eend_wgrad_f32 (exact-f32 weight and bias gradients);
gradients reach ``xs`` and every ``eda.*`` parameter.  ``TransformerEDADiarization.forward(src, tgt, ilens)`` (model :39-52) runs
it for a FROZEN encoder -- embeddings from the inference kernels, so without dropout, and without a gradient -- with the logits
behind a second Function (eend_eda_head_f32 / eend_eda_head_bwd_f32).  Not built: the encoder backward of this model (``forward``
raises NotImplementedError while any ``enc.*`` parameter requires grad), the Lightning module train/offl_tfm_lstm.py, and STB
training.  The block-online use of this model with a speaker-tracing buffer
(train/tfm_STB.py) is ``fs_eend_amd.stb.StbSession``: it runs ``_encode`` and ``eda._attractors`` on many streams at once, every
stream with its own frame order (a (B, T) ``order``).
"""
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor
from torch.autograd.function import once_differentiable

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


def check_n_speakers(n_speakers, B: int) -> list:
    """The speaker counts of a batch as a list of B ints in 0 .. MAX_N_SPEAKERS, or ValueError."""
    try:
        n = [int(v) for v in n_speakers]
    except TypeError as e:
        raise ValueError("n_speakers must be a sequence of integers") from e
    if len(n) != B or any(v != w for v, w in zip(n, n_speakers)):
        raise ValueError(f"n_speakers must hold one integer per sequence ({B}), got {list(n_speakers)}")
    if min(n) < 0 or max(n) > MAX_N_SPEAKERS:
        raise ValueError(f"n_speakers must lie in 0 .. {MAX_N_SPEAKERS}, got {n}")
    return n


_EDA_PARAMS = ("encoder.weight_ih_l0", "encoder.weight_hh_l0", "encoder.bias_ih_l0", "encoder.bias_hh_l0", "decoder.weight_ih_l0",
               "decoder.weight_hh_l0", "decoder.bias_ih_l0", "decoder.bias_hh_l0", "counter.weight", "counter.bias")


def _slab_logits(emb32: Tensor, attractors: Tensor, T: int) -> Tensor:
    """logits (B, T, C) f32 = emb32 (B, rows >= T, D) attractors (B, C, D)^T (eend_eda_head_f32)."""
    B, C, _ = attractors.shape
    logits = torch.empty(B, T, C, dtype=torch.float32, device=emb32.device)
    ops.eda_head(emb32, attractors, logits, T)
    return logits


def _pad_rows(grad: Tensor, rows: int) -> Tensor:
    """A gradient over the T rows the steps read, back to the slab's `rows` rows: zeros for the rows no step read."""
    B, T, D = grad.shape
    return grad if rows <= T else torch.cat([grad, grad.new_zeros(B, rows - T, D)], dim=1)


class _AttractorLoss(torch.autograd.Function):
    """rows32 (B, rows >= T, D) -> (attractor loss, attractors (B, C, D)) on the kernels of csrc/lstm.hip; the backward fills the
    gradients of rows32 and of the ten `eda.*` tensors (_EDA_PARAMS order; the two biases of an LSTM receive the same gradient, the
    decoder's weight_ih, whose input is zero, receives zeros)."""

    @staticmethod
    def forward(ctx, holder, rows32, *params):
        eda, T, order, n_spk = holder["eda"], holder["T"], holder["order"], holder["n_speakers"]
        P = eda._prepare()
        B, rows, D = rows32.shape
        C = max(n_spk) + 1
        dev = rows32.device
        f32 = dict(dtype=torch.float32, device=dev)
        # grad mode is always off in here and needs_input_grad ignores it: the caller read it (holder["save"])
        save = holder["save"] and any(ctx.needs_input_grad)
        # what the backward reads is T rows tall whatever the slab: its GEMMs never meet a padding row
        ge, ce, pe = (torch.empty(B, T, 4 * D, **f32), torch.empty(B, T, D, **f32), torch.empty(B, T, D, **f32)) if save else (None,) * 3
        gd, cd, pd = (torch.empty(B, C, 4 * D, **f32), torch.empty(B, C, D, **f32), torch.empty(B, C, D, **f32)) if save else (None,) * 3
        dattr, dw, db = (torch.empty(B, C, D, **f32), torch.empty(D, **f32), torch.empty(1, **f32)) if save else (None,) * 3
        attractors, cT = eda._attractor_pass(P, rows32, T, order, C, (ge, ce, pe), (gd, cd, pd))
        loss = torch.empty(1, **f32)
        ops.eda_count_loss(attractors, P["cnt_w"], P["cnt_b"], torch.tensor(n_spk, dtype=torch.int32, device=dev), loss, dattr, dw, db)
        if save:
            xs = rows32 if rows == T else rows32[:, :T].contiguous()
            # through save_for_backward, so that an in-place write to xs or a parameter before the backward raises (the operand
            # copies share the parameters' version counters where they alias them)
            ctx.save_for_backward(xs, order, ge, ce, pe, gd, cd, pd, cT, dattr, dw, db, P["enc_whh"], P["dec_whh"], P["enc_wih_t"])
            ctx.rows = rows
        return loss.view(()), attractors

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss, dattractors):
        xs, order, ge, ce, pe, gd, cd, pd, cT, dattr, dw, db, enc_whh, dec_whh, enc_wih_t = ctx.saved_tensors
        B, T, D = xs.shape
        C = gd.shape[1]
        f32 = dict(dtype=torch.float32, device=xs.device)
        scale = torch.zeros((), **f32) if dloss is None else dloss.to(torch.float32)
        dA = dattr * scale
        if dattractors is not None:
            dA = dA + dattractors
        # decoder: every step's h is an attractor
        dGd, dh0, dc0 = torch.empty(B, C, 4 * D, **f32), torch.empty(B, D, **f32), torch.empty(B, D, **f32)
        ops.lstm_bwd(gd, cd, cT, dec_whh, dA.contiguous(), None, None, None, dGd, dh0, dc0, B, C)
        ws = torch.empty(ops.wgrad_f32_workspace_bytes(4 * D, D, True) // 4, **f32)
        dWd, dbd = torch.empty(4 * D, D, **f32), torch.empty(4 * D, **f32)
        ops.wgrad_f32(dGd.view(B * C, 4 * D), pd.view(B * C, D), ws, dWd, dbd)
        # encoder: fed by the decoder's initial-state gradients
        dGe, dhe, dce = torch.empty(B, T, 4 * D, **f32), torch.empty(B, D, **f32), torch.empty(B, D, **f32)
        ops.lstm_bwd(ge, ce, None, enc_whh, None, dh0, dc0, order, dGe, dhe, dce, B, T)
        dWhh, dWih, dbe = torch.empty(4 * D, D, **f32), torch.empty(4 * D, D, **f32), torch.empty(4 * D, **f32)
        ops.wgrad_f32(dGe.view(B * T, 4 * D), pe.view(B * T, D), ws, dWhh, dbe)
        ops.wgrad_f32(dGe.view(B * T, 4 * D), xs.view(B * T, D), ws, dWih, None)
        dxs = None
        if ctx.needs_input_grad[1]:
            dxs = torch.empty(B, T, D, **f32)
            ops.linear_step_f32(dGe.view(B * T, 4 * D), enc_wih_t, None, dxs.view(B * T, D))
            dxs = _pad_rows(dxs, ctx.rows)
        grads = (dWih, dWhh, dbe, dbe.clone(), torch.zeros(4 * D, D, **f32), dWd, dbd, dbd.clone(), (dw * scale).view(1, D),
                 (db * scale).view(1))
        return (None, dxs) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))


class _HeadLogits(torch.autograd.Function):
    """logits (B, T, C) = emb (B, rows >= T, D) attractors (B, C, D)^T (eend_eda_head_f32) with eend_eda_head_bwd_f32 behind it."""

    @staticmethod
    def forward(ctx, emb32, attractors, T):
        ctx.save_for_backward(emb32, attractors)
        ctx.T = T
        return _slab_logits(emb32, attractors, T)

    @staticmethod
    @once_differentiable
    def backward(ctx, dlogits):
        emb32, attractors = ctx.saved_tensors
        B, rows, D = emb32.shape
        T = ctx.T
        need_emb, need_attr = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dattr = torch.empty_like(attractors) if need_attr else None
        demb = torch.empty(B, T, D, dtype=torch.float32, device=emb32.device) if need_emb else None
        ops.eda_head_bwd(dlogits.contiguous(), emb32, attractors, dattr, demb, T)
        return _pad_rows(demb, rows) if need_emb else None, dattr, None


class EncoderDecoderAttractor(PreparedOperands, nn.Module):
    """LSTM encoder-decoder attractor calculation (reference model :79-127): `estimate` for inference, `forward` with the attractor
    loss under autograd (the LSTM backward of csrc/lstm.hip)."""

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
        P["enc_wih_t"] = P["enc_wih"].t().contiguous()            # the backward's d xs = dG W_ih as a linear layer over W_ih^T
        return P

    @staticmethod
    def _attractor_pass(P, rows32: Tensor, T: int, order: Optional[Tensor], C: int, enc_keep=(None,) * 3, dec_keep=(None,) * 3):
        """The one encoder-LSTM-then-decoder-LSTM pass: rows32 f32 (B, rows >= T, D) -> attractors (B, C, D) and the encoder's final
        cell state.  The input projection runs over all slab rows; step t of the encoder LSTM reads row order[t] (order i32 (T,) for
        the batch, (B, T) one per sequence, or None); the decoder reads C zero vectors from the encoder's (hT, cT).  enc_keep /
        dec_keep: (gates, c_all, h_prev) for the backward; with None everywhere the recurrence runs its inference instance.  P: the
        operands of _prepare()."""
        B, rows, D = rows32.shape
        f32 = dict(dtype=torch.float32, device=rows32.device)
        G = torch.empty(B, rows, 4 * D, **f32)
        ops.linear_step_f32(rows32.view(B * rows, D), P["enc_wih"], P["enc_b"], G.view(B * rows, 4 * D))
        hT, cT, hD, cD = (torch.empty(B, D, **f32) for _ in range(4))
        ops.lstm_train(G, order, None, P["enc_whh"], None, None, hT, cT, None, *enc_keep, B, T)
        attractors = torch.empty(B, C, D, **f32)
        ops.lstm_train(None, None, P["dec_b"], P["dec_whh"], hT, cT, hD, cD, attractors, *dec_keep, B, C)    # zero input: no GEMM
        return attractors, cT

    def _attractors(self, rows32: Tensor, T: int, order: Optional[Tensor], max_n_speakers: int, th: Optional[float]):
        """rows32 f32 (B, rows >= T, D) -> attractors (B, C, D), probs (B, C), count i32 (B,) or None (_attractor_pass, then the
        counter)."""
        P = self._prepare()
        B, _, D = rows32.shape
        C = int(max_n_speakers)
        if not ops.lstm_ok(B, T, D) or not 1 <= C <= 16:
            raise EendHipError(f"EDA attractors: unsupported shape B={B}, T={T}, D={D}, C={C}")
        attractors, _ = self._attractor_pass(P, rows32, T, order, C)
        probs = torch.empty(B, C, dtype=torch.float32, device=rows32.device)
        count = torch.empty(B, dtype=torch.int32, device=rows32.device) if th is not None else None
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

    def _loss_and_attractors(self, rows32: Tensor, T: int, n_speakers: list, order: Optional[Tensor]):
        """rows32 f32 (B, rows >= T, D), contiguous -> (loss, attractors (B, max(n_speakers) + 1, D)) under autograd."""
        B, _, D = rows32.shape
        if not ops.lstm_ok(B, T, D):
            raise EendHipError(f"EDA attractors: unsupported shape B={B}, T={T}, D={D}")
        params = [self.get_parameter(n) for n in _EDA_PARAMS]
        holder = dict(eda=self, T=T, order=order, n_speakers=n_speakers, save=torch.is_grad_enabled())
        return _AttractorLoss.apply(holder, rows32, *params)

    def forward(self, xs: Tensor, n_speakers, order=None):
        """Attractors from embedding sequences with the number of speakers given, and the attractor-existence loss (reference model
        :109-127): xs (B, T, E), n_speakers a list of B counts -> (loss, attractors (B, max(n_speakers) + 1, E)).  `loss.backward()`
        reaches xs (if it requires grad) and every parameter of this module; without grad mode nothing is kept for it.
        `order` (ours): None reads the frames as they lie, as the reference's forward does; a permutation of 0 .. T-1 reads frame
        order[t] at step t, as `test` does."""
        if not isinstance(xs, Tensor) or xs.dim() != 3:
            raise EendHipError("forward: xs must be a (B, T, E) tensor")
        n = check_n_speakers(n_speakers, xs.shape[0])
        o = None if order is None else check_order(order, xs.shape[1])
        _need_gpu(xs, "xs")
        if xs.dtype != torch.float32 or not xs.is_contiguous():
            xs = xs.to(torch.float32).contiguous()
        return self._loss_and_attractors(xs, xs.shape[1], n, None if o is None else torch.from_numpy(o).to(xs.device))


class TransformerEDADiarization(PreparedOperands, nn.Module):
    """Offline EEND-EDA on MI355X (reference model :10-76): `test` for inference, `forward` for training with a frozen encoder."""

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
        order_dev = torch.from_numpy(order).to(emb_slab.device)
        attractors, probs, count = self.eda._attractors(emb_slab, T, order_dev, MAX_N_SPEAKERS, None if n_spk is not None else float(th))
        logits = _slab_logits(emb_slab, attractors, T)
        counts = [int(n_spk)] * len(src) if n_spk is not None else count.tolist()
        self.last_probs, self.last_counts, self.last_logits = probs, counts, logits
        output_active = [logits[b, :int(l), :counts[b]] for b, l in enumerate(ilens)]
        return output_active, emb_slab[:, :T], attractors[:, :-1, :]

    def forward(self, src, tgt, ilens):
        """reference model :39-52 for a FROZEN encoder -> ([logits (ilen_i, n_i)], attractor_loss_ratio * attractor loss, emb (B, T, E),
        attractors[:, :-1, :]) with n_i = tgt[i].shape[1].  The embeddings come from the inference kernels (no dropout, no gradient);
        the attractor loss and the logits carry gradients to every `eda.*` parameter.  The caller's PIT / BCE loss on the slices is
        ordinary torch."""
        if any(p.requires_grad for p in self.enc.parameters()):
            raise NotImplementedError("the encoder backward of EEND-EDA is not built: freeze the encoder "
                                      "(model.enc.requires_grad_(False)) to train the attractor path")
        if tgt is None or len(src) == 0 or len(src) != len(tgt) or len(src) != len(ilens):
            raise ValueError("src, tgt and ilens must be non-empty lists of one length")
        n_speakers = check_n_speakers([t.shape[1] for t in tgt], len(src))
        with torch.no_grad():
            emb_slab, T = self._encode(src)
        loss, attractors = self.eda._loss_and_attractors(emb_slab, T, n_speakers, None)
        logits = _HeadLogits.apply(emb_slab, attractors, T)
        output = [logits[b, :int(l), :n] for b, (l, n) in enumerate(zip(ilens, n_speakers))]
        return output, self.attractor_loss_ratio * loss, emb_slab[:, :T], attractors[:, :-1, :]
