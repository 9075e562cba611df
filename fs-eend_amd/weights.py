"""The operand cache every model shares, and the operand blocks more than one model builds.

The kernels read the weights as copies in their own layouts (f16 / f32, packed streams).  `PreparedOperands` keeps one set of
copies per model and rebuilds it when the parameters change: `_prepare()` compares a fingerprint -- (data_ptr, _version) of the
tensors the class names -- with the one the copies were built under.  That sees optimiser steps, `load_state_dict` and `.to()`;
a write through `.data` does NOT bump `_version`: call `refresh_weights()` after one.

A rebuild makes a NEW dict: the streaming sessions compare `model._prep` by identity to learn that the copies their captured
graphs point into are gone.  Constants derived from the weights for one call shape (`_derived`) live until the next rebuild.
Nothing here touches a device: the class's `_build_operands()` does (and raises through `need_gpu_params` on the CPU).
"""
import torch
from torch import Tensor

from . import lib as _lib, ops
from .lib import EendHipError


def _f16(t: Tensor) -> Tensor:
    return t.detach().to(torch.float16).contiguous()


def _f32(t: Tensor) -> Tensor:
    return t.detach().to(torch.float32).contiguous()


def _qscaled(t: Tensor) -> Tensor:
    """Packed in-projection (3D x D weight or 3D bias) with the q rows pre-multiplied by
    1/sqrt(dh) * log2(e) in fp32 (ops.QSCALE_LOG2): the attention kernel then needs no per-score scale."""
    t = t.detach().to(torch.float32).clone()
    t[: t.shape[0] // 3] *= ops.QSCALE_LOG2
    return t


def need_gpu_params(t: Tensor):
    """-> the device of parameter t; the HIP path has no CPU fallback."""
    if t.device.type != "cuda":
        raise EendHipError("model parameters must live on the GPU: the HIP path has no CPU fallback")
    return t.device


class PreparedOperands:
    """Mixin of an nn.Module (listed before it).  The class gives `_build_operands()` -> the operand dict and, unless it is
    parameters plus buffers, `_fingerprint_tensors()`: the tensors whose change rebuilds the operands."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._prep = self._prep_key = None
        self._consts = {}
        self.register_load_state_dict_post_hook(lambda module, incompatible_keys: module.refresh_weights())

    def refresh_weights(self):
        """Drop the cached operand copies (needed after a write through `.data`, which does not bump _version)."""
        self._prep = None

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        self._prep = None
        return out

    def _fingerprint_tensors(self):
        return list(self.parameters()) + list(self.buffers())

    def _prepare(self):
        """The operand copies in kernel layouts, rebuilt when the fingerprinted tensors changed."""
        key = tuple((t.data_ptr(), t._version) for t in self._fingerprint_tensors())
        if self._prep is None or key != self._prep_key:
            self._prep, self._prep_key = self._build_operands(), key
            self._consts = {}
        return self._prep

    def _derived(self, key, build):
        """build() once per key and operand set: a constant of the weights for one call shape."""
        if key not in self._consts:
            self._consts[key] = build()
        return self._consts[key]


def convert_const(m, C):
    """pc[c] = convert.weight[:, D:] pe[c] + convert.bias of model m's decoder (a (C, D) constant of the weights, made by
    eend_convert_const_f32), cached with m's operands."""
    def build():
        dec = m.dec
        dev = dec.convert.weight.device
        W, b = _f32(dec.convert.weight), _f32(dec.convert.bias)
        pe = dec.pos_enc.pe[0, :C].to(device=dev, dtype=torch.float32).contiguous()
        pc = torch.empty(C, W.shape[0], dtype=torch.float32, device=dev)
        _lib.check(_lib.load().eend_convert_const_f32(0, W.data_ptr(), b.data_ptr(), pe.data_ptr(), pc.data_ptr(), None, None, None, C,
                                                      torch.cuda.current_stream().cuda_stream), "eend_convert_const_f32")
        return pc

    return m._derived(("pc", C), build)


def input_operands(linear, norm, in_size, bn=None):
    """The input projection's operands: (f16 weight zero-padded to Fin_pad columns, bias, LayerNorm gamma, beta, eps, Fin_pad) and,
    with `bn`, the BatchNorm tuple (weight, bias, running mean, running variance) as a seventh element."""
    Fin_pad = (in_size + 63) // 64 * 64
    w = torch.zeros(linear.weight.shape[0], Fin_pad, dtype=torch.float16, device=linear.weight.device)
    w[:, :in_size] = linear.weight.detach().to(torch.float16)
    out = (w, _f32(linear.bias), _f32(norm.weight), _f32(norm.bias), norm.eps, Fin_pad)
    if bn is not None:
        out += (tuple(_f32(t) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)),)
    return out


def encoder_layer_operands(l, keep_unpacked):
    """Operands of one nn.TransformerEncoderLayer-shaped layer: q-scaled in-projection (`in_w`, packed `in_wp`, `in_b`), the biases
    and LayerNorms, and `ws`, the out-projection + FFN weights on the packed stream.  keep_unpacked (FS-EEND): `out_w` / `w1` /
    `w2` stay for the ffn.hip fallback and `ws` exists only where the stream takes the hidden width; otherwise (EEND-EDA) the
    caller has made sure that it does.  Each model keeps the order of its two pack launches."""
    a = l.self_attn
    L = dict(in_w=_f16(_qscaled(a.in_proj_weight)), in_b=_f32(_qscaled(a.in_proj_bias)), out_b=_f32(a.out_proj.bias),
             b1=_f32(l.linear1.bias), b2=_f32(l.linear2.bias),
             g1=_f32(l.norm1.weight), be1=_f32(l.norm1.bias), eps1=l.norm1.eps,
             g2=_f32(l.norm2.weight), be2=_f32(l.norm2.bias), eps2=l.norm2.eps)
    wo, w1, w2 = _f16(a.out_proj.weight), _f16(l.linear1.weight), _f16(l.linear2.weight)
    if keep_unpacked:
        L.update(out_w=wo, w1=w1, w2=w2)
        if ops.stream_ok(w1.shape[0]):
            L["ws"] = ops.ffn_stream_pack(wo, w1, w2)
        L["in_wp"] = ops.inproj_attn_pack(L["in_w"])
    else:
        L["in_wp"] = ops.inproj_attn_pack(L["in_w"])
        L["ws"] = ops.ffn_stream_pack(wo, w1, w2)
    return L
