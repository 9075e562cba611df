"""Tensor-level wrappers over the C-ABI (include/eend_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every
arithmetic op of the hot path is one call into libeend_hip.so.  All wrappers
require CUDA(ROCm) tensors and raise on anything else -- there is no eager or
CPU fallback.
"""
import math

import torch

from . import lib as _lib

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _chk(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise _lib.EendHipError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise _lib.EendHipError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.EendHipError(f"{name}: expected a contiguous tensor")


def frames_pad(T: int) -> int:
    """Frames per sequence slab: T rounded up to a multiple of 64."""
    return (T + 63) // 64 * 64


def bn_cast_pad(x, bn, out16, T, Tp, apply_bn=True, eps=1e-5):
    """x f32 (B,T,Fin) -> out16 f16 (B*Tp, Fpad).  bn = (weight, bias, mean, var) or None."""
    L = _lib.load()
    _chk(x, F32, "x"); _chk(out16, F16, "out16")
    B, Fin = x.shape[0], x.shape[2]
    Fpad = out16.shape[-1]
    w = b = m = v = None
    if apply_bn:
        w, b, m, v = bn
        for t, n in ((w, "bn.weight"), (b, "bn.bias"), (m, "bn.mean"), (v, "bn.var")):
            _chk(t, F32, n)
    _lib.check(L.eend_bn_cast_pad_f16(_p(x), _p(w), _p(b), _p(m), _p(v), eps, _p(out16), B, T, Tp, Fin, Fpad,
                                      1 if apply_bn else 0, _stream()), "eend_bn_cast_pad_f16")
    return out16


ACT_NONE, ACT_RELU, ACT_SWISH = 0, 1, 2


def linear(a16, w16, bias, out16, relu=False, act=None):
    """out16 = act(a16 @ w16.T + bias); a16 (M,K) f16, w16 (N,K) f16."""
    if act is None:
        act = ACT_RELU if relu else ACT_NONE
    L = _lib.load()
    _chk(a16, F16, "a16"); _chk(w16, F16, "w16"); _chk(bias, F32, "bias"); _chk(out16, F16, "out16")
    M, K = a16.shape
    N = w16.shape[0]
    _lib.check(L.eend_linear_f16(_p(a16), a16.stride(0), _p(w16), w16.stride(0), _p(bias), _p(out16),
                                 out16.stride(0), M, N, K, act, _stream()), "eend_linear_f16")
    return out16


def inproj_heads(a16, w16, bias, q, k, vt, nseq, Tp, H):
    L = _lib.load()
    _chk(a16, F16, "a16"); _chk(w16, F16, "w16"); _chk(bias, F32, "bias")
    _chk(q, BF16, "q"); _chk(k, BF16, "k"); _chk(vt, BF16, "vt")
    K = a16.shape[1]
    _lib.check(L.eend_inproj_heads_bf16(_p(a16), a16.stride(0), _p(w16), w16.stride(0), _p(bias), _p(q), _p(k),
                                        _p(vt), nseq, Tp, H, 64, K, _stream()), "eend_inproj_heads_bf16")


def linear_glu(a16, wi16, bias_i, out16):
    """GLU(a16 @ W.T + b) with value/gate rows interleaved in wi16 (2N, K); out16 (M, N)."""
    L = _lib.load()
    _chk(a16, F16, "a16"); _chk(wi16, F16, "wi16"); _chk(bias_i, F32, "bias_i"); _chk(out16, F16, "out16")
    M, K = a16.shape
    _lib.check(L.eend_linear_glu_f16(_p(a16), a16.stride(0), _p(wi16), wi16.stride(0), _p(bias_i), _p(out16),
                                     out16.stride(0), M, wi16.shape[0], K, _stream()), "eend_linear_glu_f16")


def linear_res_scale_ln16(a16, w16, bias, res, alpha, gamma, beta, out32, out16, eps=1e-5):
    """out32 = (a16 @ w16.T + bias) * alpha + res ; out16 = f16(LN(out32) * gamma + beta)."""
    L = _lib.load()
    _chk(a16, F16, "a16"); _chk(w16, F16, "w16"); _chk(bias, F32, "bias"); _chk(res, F32, "res")
    _chk(gamma, F32, "gamma"); _chk(beta, F32, "beta"); _chk(out32, F32, "out32"); _chk(out16, F16, "out16")
    M, K = a16.shape
    _lib.check(L.eend_linear_res_scale_ln16_f16(_p(a16), a16.stride(0), _p(w16), w16.stride(0), _p(bias), _p(res),
                                                float(alpha), _p(gamma), _p(beta), eps, _p(out32), _p(out16), M, K,
                                                _stream()), "eend_linear_res_scale_ln16_f16")


def retention_proj(a16, wqkvg16, bias, q, k, kt, vt, g, nseq, Tp, H):
    L = _lib.load()
    _chk(a16, F16, "a16"); _chk(wqkvg16, F16, "wqkvg"); _chk(bias, F32, "bias")
    for t, n in ((q, "q"), (k, "k"), (kt, "kt"), (vt, "vt"), (g, "g")):
        _chk(t, F16, n)
    _lib.check(L.eend_retention_proj_f16(_p(a16), a16.stride(0), _p(wqkvg16), wqkvg16.stride(0), _p(bias), _p(q),
                                         _p(k), _p(kt), _p(vt), _p(g), nseq, Tp, H, 64, a16.shape[1], _stream()),
               "eend_retention_proj_f16")


_KV_WS = {}


def retention_chunk(q, k, kt, vt, g, o16, st_ws, cscale_ws, sexp_ws, nseq, H, Tp, chunk, gn_eps=1e-6, t_valid=0,
                    state_in=None, state_out=None):
    L = _lib.load()
    for t, n in ((q, "q"), (k, "k"), (kt, "kt"), (vt, "vt"), (g, "g"), (o16, "o16"), (st_ws, "st_ws")):
        _chk(t, F16, n)
    _chk(cscale_ws, F32, "cscale_ws"); _chk(sexp_ws, F32, "sexp_ws"); _chk(state_in, F32, "state_in"); _chk(state_out, F32, "state_out")
    for st_ in (state_in, state_out):
        if st_ is not None and st_.numel() < nseq * H * 4096:
            raise _lib.EendHipError("retention_chunk: carried state must be (nseq, H, 64, 64) f32")
    nc = (Tp + chunk - 1) // chunk
    if st_ws.numel() < nseq * H * nc * 2 * 4096 or cscale_ws.numel() < nseq * H * nc or sexp_ws.numel() < nseq * H * nc:
        raise _lib.EendHipError("retention_chunk: workspace too small")
    need = nseq * H * nc * 4096
    kv_ws = _KV_WS.get(str(q.device))
    if kv_ws is None or kv_ws.numel() < need:                  # f32 per-chunk K^T V workspace, grown on demand
        kv_ws = torch.empty(need, dtype=F32, device=q.device)
        _KV_WS[str(q.device)] = kv_ws
    _lib.check(L.eend_retention_chunk_f16(_p(q), _p(k), _p(kt), _p(vt), _p(g), _p(o16), _p(st_ws), _p(kv_ws),
                                          _p(cscale_ws), _p(sexp_ws), nseq, H, Tp, chunk, o16.stride(0), g.stride(0),
                                          gn_eps, int(t_valid), _p(state_in), _p(state_out), _stream()), "eend_retention_chunk_f16")


def retention_stream_ok(L, Tp, ldx=256, ldo=256):
    return bool(_lib.load().eend_retention_stream_ok(int(L), int(Tp), int(ldx), int(ldo)))


def retention_stream_pack(wqkvg32):
    """Pack the f32 [q; k * dk^-0.5; v; g] rows (1024, 256) into the weight stream of retention_stream (hi / lo parts of the q rows)."""
    L = _lib.load()
    _chk(wqkvg32, F32, "wqkvg32")
    if wqkvg32.shape != (1024, 256):
        raise _lib.EendHipError("retention_stream_pack: expected the packed projection [1024][256]")
    out = torch.empty(L.eend_retention_stream_elems(), dtype=F16, device=wqkvg32.device)
    _lib.check(L.eend_retention_stream_pack_f16(_p(wqkvg32), _p(out), _stream()), "eend_retention_stream_pack_f16")
    return out


def retention_stream(x16, xlo16, wstream, bias, o16, st_ws, cscale_ws, sexp_ws, nseq, Tp, chunk, gn_eps=1e-6, t_valid=0,
                     state_in=None, state_out=None):
    """o16 = swish(g) * LN_head(retention(q, k, v)) with q / k / v / g projected on chip from the rows x16 (ret_stream.hip); xlo16
    (optional): the f16 remainder of the f32 stream behind x16 (query path precision).  H = 4."""
    L = _lib.load()
    _chk(x16, F16, "x16"); _chk(xlo16, F16, "xlo16"); _chk(wstream, F16, "wstream"); _chk(bias, F32, "bias"); _chk(o16, F16, "o16")
    _chk(st_ws, F16, "st_ws"); _chk(cscale_ws, F32, "cscale_ws"); _chk(sexp_ws, F32, "sexp_ws")
    _chk(state_in, F32, "state_in"); _chk(state_out, F32, "state_out")
    H = 4
    if x16.shape != (nseq * Tp, 256) or o16.shape[0] < nseq * Tp or bias.numel() != 1024 or wstream.numel() != L.eend_retention_stream_elems() or \
            (xlo16 is not None and (xlo16.shape != x16.shape or xlo16.stride(0) != x16.stride(0))):
        raise _lib.EendHipError("retention_stream: shape mismatch")
    for st_ in (state_in, state_out):
        if st_ is not None and st_.numel() < nseq * H * 4096:
            raise _lib.EendHipError("retention_stream: carried state must be (nseq, H, 64, 64) f32")
    nc = (Tp + chunk - 1) // chunk
    if st_ws.numel() < nseq * H * nc * 2 * 4096 or cscale_ws.numel() < nseq * H * nc or sexp_ws.numel() < nseq * H * nc:
        raise _lib.EendHipError("retention_stream: workspace too small")
    need = nseq * H * nc * 4096
    kv_ws = _KV_WS.get(str(x16.device))
    if kv_ws is None or kv_ws.numel() < need:                  # f32 per-chunk K^T V workspace, grown on demand
        kv_ws = torch.empty(need, dtype=F32, device=x16.device)
        _KV_WS[str(x16.device)] = kv_ws
    _lib.check(L.eend_retention_stream_f16(_p(x16), x16.stride(0), _p(xlo16), _p(wstream), _p(bias), _p(o16), o16.stride(0), _p(st_ws),
                                           _p(kv_ws), _p(cscale_ws), _p(sexp_ws), nseq, Tp, chunk, gn_eps, int(t_valid), _p(state_in),
                                           _p(state_out), _stream()), "eend_retention_stream_f16")


def layernorm_f16(x32, gamma, beta, out16, eps=1e-5):
    L = _lib.load()
    _chk(x32, F32, "x32"); _chk(gamma, F32, "gamma"); _chk(beta, F32, "beta"); _chk(out16, F16, "out16")
    M, D = x32.shape
    _lib.check(L.eend_layernorm_f16(_p(x32), _p(gamma), _p(beta), eps, _p(out16), M, D, _stream()), "eend_layernorm_f16")


def dwconv_bn_swish(x16, w, bn, out16, nseq, Tp, eps=1e-5, halo16=None):
    """x16/out16 f16 (nseq*Tp, D); w f32 (D, k); bn = (weight, bias, mean, var); halo16 f16 (nseq, k-1, D) or None."""
    L = _lib.load()
    _chk(x16, F16, "x16"); _chk(w, F32, "w"); _chk(out16, F16, "out16")
    for t in bn:
        _chk(t, F32, "bn")
    D, k = w.shape
    _chk(halo16, F16, "halo16")
    if halo16 is not None and tuple(halo16.shape) != (nseq, k - 1, D):
        raise _lib.EendHipError("dwconv_bn_swish: halo must be (nseq, k-1, D)")
    _lib.check(L.eend_dwconv_bn_swish_f16(_p(x16), _p(w), _p(bn[0]), _p(bn[1]), _p(bn[2]), _p(bn[3]), eps, _p(out16),
                                          nseq, Tp, D, k, _p(halo16), _stream()), "eend_dwconv_bn_swish_f16")


def linear_res_ln(a16, w16, bias, res, gamma, beta, out32, out16, eps=1e-5, alpha=1.0):
    L = _lib.load()
    _chk(a16, F16, "a16"); _chk(w16, F16, "w16"); _chk(bias, F32, "bias"); _chk(res, F32, "res")
    _chk(gamma, F32, "gamma"); _chk(beta, F32, "beta"); _chk(out32, F32, "out32"); _chk(out16, F16, "out16")
    M, K = a16.shape
    if w16.shape[0] != 256:
        raise _lib.EendHipError("linear_res_ln: N must be 256")
    _lib.check(L.eend_linear_res_ln_f16(_p(a16), a16.stride(0), _p(w16), w16.stride(0), _p(bias), _p(res),
                                        float(alpha), _p(gamma), _p(beta), eps, _p(out32), _p(out16), M, K, _stream()),
               "eend_linear_res_ln_f16")


def linear_res_scale(a16, w16, bias, res, alpha, out32, out16):
    """a16 (M, K) f16 rows at any row stride that is a multiple of 8 halves (rows may overlap: a Conv1d's windows as a strided
    view of its input frames)."""
    L = _lib.load()
    if a16.is_contiguous() or a16.dim() != 2 or a16.stride(1) != 1 or a16.stride(0) % 8:
        _chk(a16, F16, "a16")
    elif not a16.is_cuda or a16.dtype != F16:
        raise _lib.EendHipError("a16: expected an f16 GPU tensor")
    _chk(w16, F16, "w16"); _chk(bias, F32, "bias"); _chk(res, F32, "res")
    _chk(out32, F32, "out32"); _chk(out16, F16, "out16")
    M, K = a16.shape
    if w16.shape[0] != 256:
        raise _lib.EendHipError("linear_res_scale: N must be 256")
    _lib.check(L.eend_linear_res_scale_f16(_p(a16), a16.stride(0), _p(w16), w16.stride(0), _p(bias), _p(res),
                                           float(alpha), _p(out32), _p(out16), M, K, _stream()),
               "eend_linear_res_scale_f16")


def conv1d_l2norm(x16, wr16, bias, ilens_i32, out32, out16, nseq, Tp, cin, ktaps, pad):
    L = _lib.load()
    _chk(x16, F16, "x16"); _chk(wr16, F16, "wr16"); _chk(bias, F32, "bias"); _chk(ilens_i32, torch.int32, "ilens")
    _chk(out32, F32, "out32"); _chk(out16, F16, "out16")
    _lib.check(L.eend_conv1d_l2norm_f16(_p(x16), _p(wr16), _p(bias), _p(ilens_i32), _p(out32), _p(out16), nseq,
                                        Tp, cin, ktaps, pad, _stream()), "eend_conv1d_l2norm_f16")


def conv_stream_ok(cin, ktaps, pad):
    return bool(_lib.load().eend_conv_stream_ok(int(cin), int(ktaps), int(pad)))


def conv_stream_pack(wr16, ktaps):
    """Pack the tap-major conv weight Wr f16 [256][ktaps*256] into the weight stream of conv1d_l2norm_stream."""
    L = _lib.load()
    _chk(wr16, F16, "wr16")
    if wr16.shape != (256, ktaps * 256):
        raise _lib.EendHipError("conv_stream_pack: expected Wr [256][ktaps*256]")
    out = torch.empty(L.eend_conv_stream_elems(int(ktaps)), dtype=F16, device=wr16.device)
    _lib.check(L.eend_conv_stream_pack_f16(_p(wr16), _p(out), int(ktaps), _stream()), "eend_conv_stream_pack_f16")
    return out


def conv1d_l2norm_stream(x16, wstream, bias, ilens_i32, out32, out16, nseq, Tp, ktaps, pad):
    """conv1d_l2norm on the packed weight stream (conv_stream.hip; cin = 256)."""
    L = _lib.load()
    _chk(x16, F16, "x16"); _chk(wstream, F16, "wstream"); _chk(bias, F32, "bias"); _chk(ilens_i32, torch.int32, "ilens")
    _chk(out32, F32, "out32"); _chk(out16, F16, "out16")
    if x16.shape != (nseq * Tp, 256) or out32.shape != (nseq * Tp, 256) or out16.shape != (nseq * Tp, 256) or \
            wstream.numel() != L.eend_conv_stream_elems(int(ktaps)):
        raise _lib.EendHipError("conv1d_l2norm_stream: shape mismatch")
    _lib.check(L.eend_conv1d_l2norm_stream_f16(_p(x16), _p(wstream), _p(bias), _p(ilens_i32), _p(out32), _p(out16), nseq, Tp, ktaps, pad,
                                               _stream()), "eend_conv1d_l2norm_stream_f16")


def convert_fanout(e16, w1_16, pc, out32, out16, B, Tp, C):
    L = _lib.load()
    _chk(e16, F16, "e16"); _chk(w1_16, F16, "w1"); _chk(pc, F32, "pc"); _chk(out32, F32, "out32"); _chk(out16, F16, "out16")
    _lib.check(L.eend_convert_fanout_f16(_p(e16), _p(w1_16), _p(pc), _p(out32), _p(out16), B, Tp, C, _stream()),
               "eend_convert_fanout_f16")


def convert_fanout_f32(e32, w32, pc, out32, out16, B, Tp, C, out16lo=None):
    """convert_fanout with f32 operands (exact-f32 MFMA): e32 (B*Tp, 256) f32, w32 the (256, >= 256) f32 convert.weight; out16lo
    (optional): the f16 remainder of the f32 rows."""
    L = _lib.load()
    _chk(e32, F32, "e32"); _chk(w32, F32, "w32"); _chk(pc, F32, "pc"); _chk(out32, F32, "out32"); _chk(out16, F16, "out16"); _chk(out16lo, F16, "out16lo")
    _lib.check(L.eend_convert_fanout_f32(_p(e32), _p(w32), w32.stride(0), _p(pc), _p(out32), _p(out16), _p(out16lo), B, Tp, C, _stream()),
               "eend_convert_fanout_f32")


LN2 = math.log(2.0)
# Multiply the q rows of an in-projection (weight and bias) by QSCALE_LOG2 and call attn_causal with
# scale=LN2: the scores then leave the QK^T MFMA already scaled and in the log2 domain, which is what the
# whole-sequence attention kernel's cheap softmax path needs (attn_full.hip, LAZY).
QSCALE_LOG2 = (1.0 / math.sqrt(64.0)) * math.log2(math.e)


def attn_causal(q, k, vt, o16, nseq, H, Tp, mask_delay=0, kv_len=None, scale=1.0 / math.sqrt(64.0)):
    L = _lib.load()
    _chk(q, BF16, "q"); _chk(k, BF16, "k"); _chk(vt, BF16, "vt"); _chk(o16, F16, "o16")
    _lib.check(L.eend_attn_causal_bf16(_p(q), _p(k), _p(vt), _p(o16), nseq, H, Tp, o16.stride(0), mask_delay,
                                       Tp if kv_len is None else kv_len, scale, _stream()), "eend_attn_causal_bf16")


def inproj_attn_pack(w_in):
    """Pack in_proj_weight f16 [768][256] (q rows pre-scaled by QSCALE_LOG2) for inproj_attn_causal_packed."""
    L = _lib.load()
    _chk(w_in, F16, "w_in")
    if w_in.shape != (768, 256):
        raise _lib.EendHipError("inproj_attn_pack: expected in_proj_weight [768][256]")
    out = torch.empty(L.eend_inproj_attn_packed_elems(), dtype=F16, device=w_in.device)
    _lib.check(L.eend_inproj_attn_pack_f16(_p(w_in), _p(out), _stream()), "eend_inproj_attn_pack_f16")
    return out


def inproj_attn_slots_choice(n_utt, C, workgroups):
    """Slots per item the slot form of inproj_attn_causal_packed takes for n_utt utterances of C slots on `workgroups` workgroups."""
    S = _lib.load().eend_inproj_attn_slots_choice(n_utt, C, workgroups)
    if S < 1:
        _lib.check(S, "eend_inproj_attn_slots_choice")
    return S


def inproj_attn_causal_packed(x16, w_packed, b_in, o16, nseq, H, Tp, mask_delay=0, kv_len=None, *, slots=None, slot_delta=None,
                              slots_per_item=0):
    """Packed in-projection + causal attention in one launch (attn_stream.hip; Tp = 64 m <= 512, H = 4): Q, K, V never reach HBM.
    slots = C (Tp = 512 only): the nseq = B C sequences are the C speaker slots of B utterances whose rows differ from slot 0's by a
    constant per slot; only slot 0's rows are read, K / V are projected once per utterance and head, and slot_delta f32 [C][512]
    (dq | dv per slot, row 0 zero) carries the constants through the projection.  slots_per_item: slots an item covers (0: chosen)."""
    L = _lib.load()
    _chk(x16, F16, "x16"); _chk(w_packed, F16, "w_packed"); _chk(b_in, F32, "b_in"); _chk(o16, F16, "o16")
    if w_packed.numel() != L.eend_inproj_attn_packed_elems() or b_in.numel() != 768 or x16.shape[0] < nseq * Tp or o16.shape[0] < nseq * Tp:
        raise _lib.EendHipError("inproj_attn_causal_packed: shape mismatch")
    if slots is not None:
        if slot_delta is not None:
            _chk(slot_delta, F32, "slot_delta")
            if slot_delta.numel() < slots * 512:
                raise _lib.EendHipError("inproj_attn_causal_packed: slot_delta must hold [slots][512]")
        _lib.check(L.eend_inproj_attn_causal_slots_f16(_p(x16), x16.stride(0), _p(w_packed), _p(b_in), _p(o16), nseq, H, Tp,
                                                       o16.stride(0), mask_delay, Tp if kv_len is None else kv_len, slots,
                                                       _p(slot_delta), slots_per_item, _stream()),
                   "eend_inproj_attn_causal_slots_f16")
        return
    _lib.check(L.eend_inproj_attn_causal_packed_f16(_p(x16), x16.stride(0), _p(w_packed), _p(b_in), _p(o16), nseq, H, Tp,
                                                    o16.stride(0), mask_delay, Tp if kv_len is None else kv_len, _stream()),
               "eend_inproj_attn_causal_packed_f16")


def inproj_attn_long_scratch(nseq, Tp, mask_delay=0, kv_len=None):
    """(partial-row f16 elements, lse f32 elements) eend_inproj_attn_causal_long_f16 needs for this shape, or None if it does not cover it."""
    import ctypes
    L = _lib.load()
    a, b = ctypes.c_longlong(0), ctypes.c_longlong(0)
    rc = L.eend_inproj_attn_long_scratch_elems(nseq, Tp, mask_delay, Tp if kv_len is None else kv_len, ctypes.byref(a), ctypes.byref(b))
    return None if rc != 0 else (a.value, b.value)


def inproj_attn_causal_long(x16, w_packed, b_in, o16, part16, lse32, nseq, H, Tp, mask_delay=0, kv_len=None):
    """Packed in-projection + causal attention for windows of more than 512 frames (attn_stream.hip, groups of 512 frames + combine)."""
    L = _lib.load()
    _chk(x16, F16, "x16"); _chk(w_packed, F16, "w_packed"); _chk(b_in, F32, "b_in"); _chk(o16, F16, "o16"); _chk(part16, F16, "part16"); _chk(lse32, F32, "lse32")
    kv = Tp if kv_len is None else kv_len
    need = inproj_attn_long_scratch(nseq, Tp, mask_delay, kv)
    if need is None:
        raise _lib.EendHipError("inproj_attn_causal_long: shape not covered")
    if (w_packed.numel() != L.eend_inproj_attn_packed_elems() or b_in.numel() != 768 or x16.shape[0] < nseq * Tp or o16.shape[0] < nseq * Tp
            or part16.numel() < need[0] or lse32.numel() < need[1]):
        raise _lib.EendHipError("inproj_attn_causal_long: shape mismatch")
    _lib.check(L.eend_inproj_attn_causal_long_f16(_p(x16), x16.stride(0), _p(w_packed), _p(b_in), _p(o16), _p(part16), _p(lse32), nseq, H, Tp,
                                                  o16.stride(0), mask_delay, kv, _stream()),
               "eend_inproj_attn_causal_long_f16")


def proj_stream_pack(w16, out=None):
    """Re-order W f16 [N][256] (N = 256 n <= 1024) into the packed weight stream of proj_stream; None if the shape has no stream form."""
    L = _lib.load()
    _chk(w16, F16, "w16")
    n = L.eend_proj_stream_elems(int(w16.shape[0])) if (w16.dim() == 2 and w16.shape[1] == 256) else 0
    if n <= 0:
        return None
    if out is None:
        out = torch.empty(n, dtype=F16, device=w16.device)
    _lib.check(L.eend_proj_stream_pack_f16(_p(w16), _p(out), int(w16.shape[0]), _stream()), "eend_proj_stream_pack_f16")
    return out


def _proj_groups(groups):
    arr = (_lib.ProjGroup * len(groups))()
    for a, gd in zip(arr, groups):
        rows, kind, t = gd.get("rows"), gd.get("kind", 0), gd.get("heads_t")
        a.rows = _p(rows); a.rows_kind = kind if rows is not None else 0
        a.rows_bf16 = 1 if (rows is not None and rows.dtype == BF16) else 0
        a.rows_ld = int(gd.get("ld", 0))
        a.rows2_bf16_heads = _p(gd.get("rows2"))
        a.heads_t = _p(t); a.heads_t_bf16 = 1 if (t is not None and t.dtype == BF16) else 0
    return arr


def proj_stream_ok(ldx, M, N, Tp, H, groups):
    return bool(_lib.load().eend_proj_stream_ok(int(ldx), int(M), int(N), int(Tp), int(H), _proj_groups(groups)))


def proj_stream(x16, wstream, bias, M, N, Tp, H, groups):
    """Y = x16 W^T + bias on the packed stream; groups: one dict per 256 output features with rows (+ kind 1 row-major / 2 head rows, ld),
    rows2 (bf16 head rows), heads_t (transposed head rows) -- see eend_proj_stream_f16."""
    L = _lib.load()
    _chk(x16, F16, "x16"); _chk(wstream, F16, "wstream"); _chk(bias, F32, "bias")
    if wstream.numel() != L.eend_proj_stream_elems(N) or bias.numel() != N or len(groups) != N // 256 or x16.shape[0] < M:
        raise _lib.EendHipError("proj_stream: shape mismatch")
    for gd in groups:
        for k in ("rows2",):
            if gd.get(k) is not None:
                _chk(gd[k], BF16, k)
    _lib.check(L.eend_proj_stream_f16(_p(x16), x16.stride(0), _p(wstream), _p(bias), M, N, Tp, H, _proj_groups(groups), _stream()),
               "eend_proj_stream_f16")


def spk_stream_pack(wo16, win16):
    """Pack Wo1 [256][256] + in_proj_weight [768][256] (f16) into the weight stream of attnout_spk_stream."""
    L = _lib.load()
    _chk(wo16, F16, "wo16"); _chk(win16, F16, "win16")
    if wo16.shape != (256, 256) or win16.shape != (768, 256):
        raise _lib.EendHipError("spk_stream_pack: expected Wo [256][256] and W_in [768][256]")
    out = torch.empty(L.eend_spk_stream_elems(), dtype=F16, device=wo16.device)
    _lib.check(L.eend_spk_stream_pack_f16(_p(wo16), _p(win16), _p(out), _stream()), "eend_spk_stream_pack_f16")
    return out


def spk_stream_ok(C, Tp):
    return bool(_lib.load().eend_spk_stream_ok(int(C), int(Tp)))


def attnout_spk_stream(a16, wstream, bo, res16, g1, be1, eps1, x16, b_in, out16, B, C, Tp):
    """x16 = LN11(a16 @ Wo1.T + bo + res16); out16 = MHA over the C slots of (x16 @ W_in.T + b_in), one launch.
    x16 may be res16 and out16 may be a16."""
    L = _lib.load()
    _chk(a16, F16, "a16"); _chk(wstream, F16, "wstream"); _chk(res16, F16, "res16"); _chk(x16, F16, "x16"); _chk(out16, F16, "out16")
    for n, t in (("bo", bo), ("g1", g1), ("be1", be1), ("b_in", b_in)):
        _chk(t, F32, n)
    M = B * C * Tp
    if a16.shape != (M, 256) or res16.shape != (M, 256) or x16.shape != (M, 256) or out16.shape != (M, 256) or b_in.numel() != 768:
        raise _lib.EendHipError("attnout_spk_stream: shape mismatch")
    if wstream.numel() != L.eend_spk_stream_elems():
        raise _lib.EendHipError("attnout_spk_stream: weight stream has the wrong size")
    _lib.check(L.eend_attnout_spk_stream_f16(_p(a16), a16.stride(0), _p(wstream), _p(bo), _p(res16), _p(g1), _p(be1), eps1, _p(x16),
                                             _p(b_in), _p(out16), B, C, Tp, 0.125, _stream()), "eend_attnout_spk_stream_f16")


def attnout_spk_stream_res32(a16, wstream, bo, res32, g1, be1, eps1, x32, b_in, out16, B, C, Tp):
    """attnout_spk_stream on an f32 residual stream: x32 = LN11(a16 @ Wo1.T + bo + res32) (f32 rows; x32 may be res32), out16 as above."""
    L = _lib.load()
    _chk(a16, F16, "a16"); _chk(wstream, F16, "wstream"); _chk(res32, F32, "res32"); _chk(x32, F32, "x32"); _chk(out16, F16, "out16")
    for n, t in (("bo", bo), ("g1", g1), ("be1", be1), ("b_in", b_in)):
        _chk(t, F32, n)
    M = B * C * Tp
    if a16.shape != (M, 256) or res32.shape != (M, 256) or x32.shape != (M, 256) or out16.shape != (M, 256) or b_in.numel() != 768:
        raise _lib.EendHipError("attnout_spk_stream_res32: shape mismatch")
    if wstream.numel() != L.eend_spk_stream_elems():
        raise _lib.EendHipError("attnout_spk_stream_res32: weight stream has the wrong size")
    _lib.check(L.eend_attnout_spk_stream_res32_f16(_p(a16), a16.stride(0), _p(wstream), _p(bo), _p(res32), _p(g1), _p(be1), eps1, _p(x32),
                                                   _p(b_in), _p(out16), B, C, Tp, 0.125, _stream()), "eend_attnout_spk_stream_res32_f16")


def dec_stream_pack(wo1, win, wo2, w1, w2):
    """Pack Wo1, in_proj_weight [768][256], Wo2 [256][256], W1 [F][256], W2 [256][F] (f16) into the weight stream of attnout_spk_ffn_stream."""
    L = _lib.load()
    for n, t in (("wo1", wo1), ("win", win), ("wo2", wo2), ("w1", w1), ("w2", w2)):
        _chk(t, F16, n)
    Fh = w1.shape[0]
    n = L.eend_dec_stream_elems(Fh)
    if (wo1.shape != (256, 256) or win.shape != (768, 256) or wo2.shape != (256, 256) or w1.shape[1] != 256 or w2.shape != (256, Fh)
            or n <= 0 or not all(t.is_contiguous() for t in (wo1, win, wo2, w1, w2))):
        raise _lib.EendHipError("dec_stream_pack: expected contiguous Wo1 / Wo2 [256][256], W_in [768][256], W1 [F][256], W2 [256][F], "
                                "F a multiple of 64 up to 2048")
    out = torch.empty(n, dtype=F16, device=wo1.device)
    _lib.check(L.eend_dec_stream_pack_f16(_p(wo1), _p(win), _p(wo2), _p(w1), _p(w2), _p(out), Fh, _stream()), "eend_dec_stream_pack_f16")
    return out


def dec_stream_ok(C, Tp):
    return bool(_lib.load().eend_dec_stream_ok(int(C), int(Tp)))


def attnout_spk_ffn_stream(a16, wstream, bo1, res16, g11, be11, eps11, b_in, bo2, g21, be21, eps21, b1, b2, g22, be22, eps22, out16,
                           B, C, Tp):
    """attnout_spk_stream followed by attnout_ffn_stream (res16 form) in one launch, x1 and O kept on chip:
    out16 = the decoder layer's output rows.  out16 may be res16."""
    L = _lib.load()
    _chk(a16, F16, "a16"); _chk(wstream, F16, "wstream"); _chk(res16, F16, "res16"); _chk(out16, F16, "out16")
    for n, t in (("bo1", bo1), ("g11", g11), ("be11", be11), ("b_in", b_in), ("bo2", bo2), ("g21", g21), ("be21", be21), ("b1", b1),
                 ("b2", b2), ("g22", g22), ("be22", be22)):
        _chk(t, F32, n)
    M = B * C * Tp
    Fh = b1.numel()
    if a16.shape != (M, 256) or res16.shape != (M, 256) or out16.shape != (M, 256) or b_in.numel() != 768:
        raise _lib.EendHipError("attnout_spk_ffn_stream: shape mismatch")
    if wstream.numel() != L.eend_dec_stream_elems(Fh):
        raise _lib.EendHipError("attnout_spk_ffn_stream: weight stream has the wrong size")
    _lib.check(L.eend_attnout_spk_ffn_stream_f16(_p(a16), a16.stride(0), _p(wstream), _p(bo1), _p(res16), _p(g11), _p(be11), eps11,
                                                 _p(b_in), _p(bo2), _p(g21), _p(be21), eps21, _p(b1), _p(b2), _p(g22), _p(be22), eps22,
                                                 _p(out16), B, C, Tp, Fh, 0.125, _stream()), "eend_attnout_spk_ffn_stream_f16")


def spk_attn(qkv16, o16, B, C, Tp, H):
    L = _lib.load()
    _chk(qkv16, F16, "qkv16"); _chk(o16, F16, "o16")
    _lib.check(L.eend_spk_attn_f16(_p(qkv16), _p(o16), B, C, Tp, H, 1.0 / math.sqrt(64.0), _stream()),
               "eend_spk_attn_f16")


def emb_consistency(emb32, labels, T, lens=None, inv_count=0.0):
    """MSE between the cosine-similarity maps of the embeddings and of the labels (FS model :46-57).
    emb32 f32 (B, Tp, D) (frames >= T ignored), labels f32 (B, T, C) zero-padded -> 0-dim f32 tensor.
    lens (int32 device tensor, B) zeroes the embeddings beyond each length and inv_count overrides the
    1/(B*T*T) normalisation (LS model :92-113)."""
    L = _lib.load()
    _chk(emb32, F32, "emb32"); _chk(labels, F32, "labels"); _chk(lens, torch.int32, "lens")
    B, Tp, D = emb32.shape
    if labels.shape[0] != B or labels.shape[1] != T or Tp < T:
        raise _lib.EendHipError("emb_consistency: shape mismatch")
    nt = (T + 63) // 64
    ws = torch.empty(B * nt * nt, dtype=F32, device=emb32.device)
    out = torch.empty(1, dtype=F32, device=emb32.device)
    _lib.check(L.eend_emb_consistency_f32(_p(emb32), _p(labels), _p(lens) if lens is not None else None, float(inv_count),
                                          _p(ws), _p(out), B, T, Tp, D, labels.shape[2], _stream()),
               "eend_emb_consistency_f32")
    return out[0]


def head_l2dot(emb32, attr, attr_out, logits, B, T, Tp, C, D):
    """attr: the un-normalised attractor rows, f32 or f16 (B*C*Tp, D)."""
    L = _lib.load()
    _chk(emb32, F32, "emb32"); _chk(attr_out, F32, "attr_out"); _chk(logits, F32, "logits")
    if attr.dtype == F16:
        _chk(attr, F16, "attr")
        _lib.check(L.eend_head_l2dot_a16_f32(_p(emb32), _p(attr), _p(attr_out), _p(logits), B, T, Tp, C, D, _stream()),
                   "eend_head_l2dot_a16_f32")
        return
    _chk(attr, F32, "attr")
    _lib.check(L.eend_head_l2dot_f32(_p(emb32), _p(attr), _p(attr_out), _p(logits), B, T, Tp, C, D, _stream()),
               "eend_head_l2dot_f32")


def lstm_ok(B, T, hidden):
    """Whether lstm() takes the shape (hidden 256, T >= 1, B >= 1)."""
    return bool(_lib.load().eend_lstm_ok(int(B), int(T), int(hidden)))


def _order_stride(order, B, T, what):
    if order is None:
        return 0
    _chk(order, torch.int32, "order")
    if order.dim() == 2:
        if tuple(order.shape) != (B, T):
            raise _lib.EendHipError(f"{what}: an order per sequence must be (B, T)")
        return T
    if order.numel() != T:
        raise _lib.EendHipError(f"{what}: order must have T entries, or be (B, T)")
    return 0


def _lstm_args(what, w_hh, g_name, G, bias, order, B, T, sized):
    """What lstm, lstm_train and lstm_bwd check alike -> (hidden, g_rows, order_stride).  w_hh f32 (4 * hidden, hidden); G (the
    backward's dG) f32 (B, g_rows, 4 * hidden), or None = zero input, which needs the bias sum (4 * hidden,); the order by
    _order_stride; sized = (name, tensor or None, elements per sequence in units of hidden)."""
    for n, t in ((g_name, G), ("bias", bias), ("w_hh", w_hh)) + tuple(s[:2] for s in sized):
        _chk(t, F32, n)
    if w_hh.dim() != 2 or w_hh.shape[0] != 4 * w_hh.shape[1]:
        raise _lib.EendHipError(f"{what}: w_hh must be (4 * hidden, hidden)")
    hidden = w_hh.shape[1]
    if G is None:
        if bias is None or bias.numel() != 4 * hidden:            # lstm_bwd has no bias: its dG is not optional
            raise _lib.EendHipError(f"{what}: needs {g_name} (B, g_rows, 4 * hidden), or for a zero input the bias sum (4 * hidden,)")
    elif G.dim() != 3 or G.shape[0] != B or G.shape[2] != 4 * hidden:
        raise _lib.EendHipError(f"{what}: {g_name} must be (B, g_rows, 4 * hidden)")
    stride = _order_stride(order, B, T, what)
    for n, t, per_seq in sized:
        if t is not None and t.numel() != B * per_seq * hidden:
            raise _lib.EendHipError(f"{what}: {n} has {t.numel()} elements, expected {B * per_seq * hidden}")
    return hidden, 0 if G is None else G.shape[1], stride


def lstm(G, order, bias, w_hh, h0, c0, hT, cT, h_all, B, T):
    """Single-layer LSTM recurrence (lstm.hip).  G f32 (B, g_rows, 1024) input pre-activations, read at row order[t] in step t, or None
    = zero input (pre-activation = bias f32 (1024,) = b_ih + b_hh); order i32 (T,) shared by the batch, (B, T) one per sequence
    (eend_lstm_orders_f32, the same kernel), or None = identity; w_hh f32 (1024, 256); h0 / c0
    f32 (B, 256), both or neither; hT / cT f32 (B, 256); h_all f32 (B, T, 256) or None."""
    L = _lib.load()
    hidden, g_rows, stride = _lstm_args("lstm", w_hh, "G", G, bias, order, B, T,
                                        (("h0", h0, 1), ("c0", c0, 1), ("hT", hT, 1), ("cT", cT, 1), ("h_all", h_all, T)))
    if stride:
        if G is None:
            raise _lib.EendHipError("lstm: an order per sequence needs G")
        _lib.check(L.eend_lstm_orders_f32(_p(G), g_rows, _p(order), _p(w_hh), _p(h0), _p(c0), _p(hT), _p(cT), _p(h_all), B, T, hidden,
                                          _stream()), "eend_lstm_orders_f32")
        return
    _lib.check(L.eend_lstm_f32(_p(G), g_rows, _p(order), _p(bias), _p(w_hh), _p(h0), _p(c0), _p(hT), _p(cT), _p(h_all), B, T, hidden,
                               _stream()), "eend_lstm_f32")


def eda_count(attractors, w, bias, th, probs, count):
    """probs (B, C) = sigmoid(attractors (B, C, 256) . w (256,) + bias (1,)); count i32 (B,) or None = first c with probs < th, else C."""
    L = _lib.load()
    _chk(attractors, F32, "attractors"); _chk(w, F32, "w"); _chk(bias, F32, "bias"); _chk(probs, F32, "probs")
    _chk(count, torch.int32, "count")
    B, C, D = attractors.shape
    if D != 256 or w.numel() != 256 or bias.numel() != 1 or probs.numel() != B * C or (count is not None and count.numel() != B):
        raise _lib.EendHipError("eda_count: attractors (B, C, 256), w (256,), bias (1,), probs (B, C), count (B,)")
    _lib.check(L.eend_eda_count_f32(_p(attractors), _p(w), _p(bias), float(th), _p(probs), _p(count), B, C, _stream()),
               "eend_eda_count_f32")


def eda_head(emb32, attractors, logits, T):
    """logits (B, T, C) = emb32 (B, emb_rows >= T, 256) . attractors (B, C, 256)^T."""
    L = _lib.load()
    _chk(emb32, F32, "emb32"); _chk(attractors, F32, "attractors"); _chk(logits, F32, "logits")
    B, C, D = attractors.shape
    if emb32.dim() != 3 or emb32.shape[0] != B or emb32.shape[2] != 256 or D != 256 or logits.numel() != B * T * C:
        raise _lib.EendHipError("eda_head: emb (B, rows, 256), attractors (B, C, 256), logits (B, T, C)")
    _lib.check(L.eend_eda_head_f32(_p(emb32), emb32.shape[1], _p(attractors), _p(logits), B, T, C, _stream()), "eend_eda_head_f32")


def lstm_train(G, order, bias, w_hh, h0, c0, hT, cT, h_all, gates, c_all, h_prev, B, T):
    """lstm() that also keeps what lstm_bwd() reads (eend_lstm_train_f32; hT, cT, h_all have lstm()'s bits): gates f32 (B, T, 1024)
    after their functions, c_all f32 (B, T, 256), h_prev f32 (B, rows >= T, 256) = the hidden state entering step t at row order[t]
    (row t without an order; its row count is its own, not G's); each of the three may be None."""
    L = _lib.load()
    _chk(h_prev, F32, "h_prev")
    hidden, g_rows, stride = _lstm_args("lstm_train", w_hh, "G", G, bias, order, B, T,
                                        (("h0", h0, 1), ("c0", c0, 1), ("hT", hT, 1), ("cT", cT, 1), ("h_all", h_all, T),
                                         ("gates", gates, 4 * T), ("c_all", c_all, T)))
    if G is None and order is not None:
        raise _lib.EendHipError("lstm_train: a zero input takes no order")
    hp_rows = 0
    if h_prev is not None:
        if h_prev.dim() != 3 or h_prev.shape[0] != B or h_prev.shape[1] < T or h_prev.shape[2] != hidden:
            raise _lib.EendHipError("lstm_train: h_prev must be (B, rows >= T, hidden)")
        hp_rows = h_prev.shape[1]
    _lib.check(L.eend_lstm_train_f32(_p(G), g_rows, _p(order), stride, _p(bias), _p(w_hh), _p(h0), _p(c0), _p(hT), _p(cT), _p(h_all),
                                     _p(gates), _p(c_all), _p(h_prev), hp_rows, B, T, hidden, _stream()), "eend_lstm_train_f32")


def lstm_bwd(gates, c_all, c0, w_hh, dh_all, dhT, dcT, order, dG, dh0, dc0, B, T):
    """Backward of lstm_train (eend_lstm_bwd_f32): upstream dh_all f32 (B, T, 256) and / or dhT, dcT f32 (B, 256) -> dG f32
    (B, g_rows >= T, 1024) with step t's pre-activation gradients at row order[t] (other rows are left as they are), dh0, dc0 (B, 256)."""
    L = _lib.load()
    hidden, g_rows, stride = _lstm_args("lstm_bwd", w_hh, "dG", dG, None, order, B, T,
                                        (("gates", gates, 4 * T), ("c_all", c_all, T), ("c0", c0, 1), ("dh_all", dh_all, T),
                                         ("dhT", dhT, 1), ("dcT", dcT, 1), ("dh0", dh0, 1), ("dc0", dc0, 1)))
    _lib.check(L.eend_lstm_bwd_f32(_p(gates), _p(c_all), _p(c0), _p(w_hh), _p(dh_all), _p(dhT), _p(dcT), _p(order), stride, _p(dG),
                                   g_rows, _p(dh0), _p(dc0), B, T, hidden, _stream()), "eend_lstm_bwd_f32")


def wgrad_f32_workspace_bytes(N, K, with_bias=False):
    """Bytes of workspace wgrad_f32 needs; 0 where it refuses the sizes (N, K multiples of 64)."""
    return int(_lib.load().eend_wgrad_f32_workspace_bytes(int(N), int(K), 1 if with_bias else 0))


def wgrad_f32(dy, x, ws, dw, db=None):
    """dw (N, K) = dy (M, N)^T x (M, K), db (N,) = column sums of dy; all f32, exact-f32 MFMA, fixed row slices summed in order
    (wgrad_f32.hip).  ws: f32 workspace of wgrad_f32_workspace_bytes(N, K, db is not None) bytes."""
    L = _lib.load()
    for n, t in (("dy", dy), ("x", x), ("ws", ws), ("dw", dw), ("db", db)):
        _chk(t, F32, n)
    if dy.dim() != 2 or x.dim() != 2 or dy.shape[0] != x.shape[0]:
        raise _lib.EendHipError("wgrad_f32: dy (M, N) and x (M, K)")
    M, N = dy.shape
    K = x.shape[1]
    if tuple(dw.shape) != (N, K) or (db is not None and db.numel() != N):
        raise _lib.EendHipError("wgrad_f32: dw (N, K), db (N,)")
    _lib.check(L.eend_wgrad_f32(_p(dy), dy.stride(0), _p(x), x.stride(0), M, N, K, _p(ws), ws.numel() * 4, _p(dw), _p(db), _stream()),
               "eend_wgrad_f32")


def eda_count_loss(attractors, w, bias, n_spk, loss, dattractors, dw, dbias):
    """The attractor-existence loss (eend_eda_count_loss_f32): mean BCE-with-logits of attractors[b, :n_b + 1] . w + bias against
    [1] * n_b + [0], and for a unit loss gradient dattractors (B, C, 256), dw (256,), dbias (1,): all three, or all three None for the
    loss alone.  n_spk i32 (B,), 0 <= n_b < C."""
    L = _lib.load()
    for n, t in (("attractors", attractors), ("w", w), ("bias", bias), ("loss", loss), ("dattractors", dattractors), ("dw", dw),
                 ("dbias", dbias)):
        _chk(t, F32, n)
    _chk(n_spk, torch.int32, "n_spk")
    B, C, D = attractors.shape
    grads = (dattractors, dw, dbias)
    if any(g is None for g in grads) != all(g is None for g in grads):
        raise _lib.EendHipError("eda_count_loss: dattractors, dw and dbias together, or none of them")
    if D != 256 or w.numel() != 256 or bias.numel() != 1 or n_spk.numel() != B or loss.numel() != 1 or (dw is not None and (
            dattractors.numel() != B * C * D or dw.numel() != 256 or dbias.numel() != 1)):
        raise _lib.EendHipError("eda_count_loss: attractors (B, C, 256), w (256,), bias (1,), n_spk (B,), loss (1,), dattractors "
                                "(B, C, 256), dw (256,), dbias (1,)")
    nbytes = int(L.eend_eda_count_loss_workspace_bytes(B))
    ws = torch.empty(nbytes // 4, dtype=F32, device=attractors.device)
    _lib.check(L.eend_eda_count_loss_f32(_p(attractors), _p(w), _p(bias), _p(n_spk), _p(loss), _p(dattractors), _p(dw), _p(dbias),
                                         _p(ws), nbytes, B, C, _stream()), "eend_eda_count_loss_f32")


def eda_head_bwd(dlogits, emb32, attractors, dattractors, demb, T):
    """Backward of eda_head (eend_eda_head_bwd_f32): dlogits (B, T, C) -> dattractors (B, C, 256) and / or demb (B, T, 256)."""
    L = _lib.load()
    for n, t in (("dlogits", dlogits), ("emb32", emb32), ("attractors", attractors), ("dattractors", dattractors), ("demb", demb)):
        _chk(t, F32, n)
    B, C, D = attractors.shape
    if emb32.dim() != 3 or emb32.shape[0] != B or emb32.shape[2] != 256 or D != 256 or dlogits.numel() != B * T * C or \
            (dattractors is not None and dattractors.numel() != B * C * D) or (demb is not None and demb.numel() != B * T * D):
        raise _lib.EendHipError("eda_head_bwd: dlogits (B, T, C), emb (B, rows, 256), attractors (B, C, 256), demb (B, T, 256)")
    ws, nbytes = None, 0
    if dattractors is not None:
        nbytes = int(L.eend_eda_head_bwd_workspace_bytes(B, T, C))
        ws = torch.empty(max(nbytes // 4, 1), dtype=F32, device=attractors.device)
    _lib.check(L.eend_eda_head_bwd_f32(_p(dlogits), _p(emb32), emb32.shape[1], _p(attractors), _p(dattractors), _p(demb), _p(ws), nbytes,
                                       B, T, C, _stream()), "eend_eda_head_bwd_f32")


STB_DESC_WORDS, STB_MAX_ROWS, STB_MAX_FEATURES = 12, 4096, 512
STB_POLICIES = {"kld": 0, "fifo": 1}


def _stb_args(desc, B, T, F):
    _chk(desc, torch.int64, "desc")
    if tuple(desc.shape) != (B, STB_DESC_WORDS):
        raise _lib.EendHipError(f"stb: desc must be i64 (B, {STB_DESC_WORDS})")


def stb_center(desc, out, buf_size, blk_size):
    """out f32 (B, T, F) = the rows [x_buf; x_i] of each descriptor minus their column mean (stb.hip, eend_stb_center_f32)."""
    L = _lib.load()
    _chk(out, F32, "out")
    B, T, F = out.shape
    _stb_args(desc, B, T, F)
    _lib.check(L.eend_stb_center_f32(_p(desc), _p(out), B, T, F, int(buf_size), int(blk_size), _stream()), "eend_stb_center_f32")


def stb_track(logits, count, xc, desc, perm_out, sel_out, buf_size, blk_size, policy):
    """Everything of an STB block after the head (stb.hip, eend_stb_track_f32): logits f32 (B, T, 15), count i32 (B,), xc f32 (B, T, F),
    desc i64 (B, 12); perm_out i32 (B, 15) / sel_out i32 (B, buf_size) or None; policy 0 = kld, 1 = fifo."""
    L = _lib.load()
    _chk(logits, F32, "logits"); _chk(count, torch.int32, "count"); _chk(xc, F32, "xc")
    _chk(perm_out, torch.int32, "perm_out"); _chk(sel_out, torch.int32, "sel_out")
    B, T, F = xc.shape
    _stb_args(desc, B, T, F)
    if tuple(logits.shape) != (B, T, 15) or count.numel() != B or (perm_out is not None and perm_out.numel() != B * 15) or \
            (sel_out is not None and sel_out.numel() != B * int(buf_size)):
        raise _lib.EendHipError("stb_track: logits (B, T, 15), count (B,), perm_out (B, 15), sel_out (B, buf_size)")
    _lib.check(L.eend_stb_track_f32(_p(logits), _p(count), _p(xc), _p(desc), _p(perm_out), _p(sel_out), B, T, F, int(buf_size),
                                    int(blk_size), int(policy), _stream()), "eend_stb_track_f32")


def retention_step(qkvg16, kv_state, scale_in, scale_out, out16, N, H, gn_eps=1e-6):
    L = _lib.load()
    _chk(qkvg16, F16, "qkvg16"); _chk(kv_state, F32, "kv_state"); _chk(scale_in, F32, "scale_in")
    _chk(scale_out, F32, "scale_out"); _chk(out16, F16, "out16")
    _lib.check(L.eend_retention_step_f16(_p(qkvg16), _p(kv_state), _p(scale_in), _p(scale_out), _p(out16), N, H, gn_eps,
                                         _stream()), "eend_retention_step_f16")


def retention_proj_step(x32, ln, w32, b32, qkvg32, N):
    """qkvg32 (N, 1024) f32 = LayerNorm(x32 (N, 256)) @ w32.T + b32, all f32 (ln = (gamma, beta, eps) or None)."""
    L = _lib.load()
    _chk(x32, F32, "x32"); _chk(w32, F32, "w32"); _chk(b32, F32, "b32"); _chk(qkvg32, F32, "qkvg32")
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    _lib.check(L.eend_retention_proj_step_f32(_p(x32), _p(g), _p(b), float(eps), _p(w32), _p(b32), _p(qkvg32), N, _stream()),
               "eend_retention_proj_step_f32")


def retention_step_f32(qkvg32, kv_state, scale_in, scale_out, out16, N, H, gn_eps=1e-6, out32=None):
    L = _lib.load()
    _chk(qkvg32, F32, "qkvg32"); _chk(kv_state, F32, "kv_state"); _chk(scale_in, F32, "scale_in")
    _chk(scale_out, F32, "scale_out"); _chk(out16, F16, "out16"); _chk(out32, F32, "out32")
    _lib.check(L.eend_retention_step_f32(_p(qkvg32), _p(kv_state), _p(scale_in), _p(scale_out), _p(out16), _p(out32), N, H, gn_eps,
                                         _stream()), "eend_retention_step_f32")


# The f32 frame-step linears (skinny.hip) serve any number of rows in groups of 16 (round 4: multi-stream sessions take the
# all-f32 step too -- their f16 step drifted past the 1e-3 bar within an hour): no row limit.
STEP_F32_MAX_ROWS = 1 << 30


def linear_step_f32(a32, w32, bias, out32, act=ACT_NONE):
    """out32 = act(a32 w32^T + bias), everything f32 (the all-f32 LS decoder frame step)."""
    L = _lib.load()
    if a32.is_contiguous() or a32.dim() != 2 or a32.stride(1) != 1 or a32.stride(0) % 4:
        _chk(a32, F32, "a32")
    elif not a32.is_cuda or a32.dtype != F32:         # rows at any stride that is a multiple of 4 floats; they may overlap (a
        raise _lib.EendHipError("a32: expected an f32 GPU tensor")     # Conv1d's windows as a strided view of its input frames)
    _chk(w32, F32, "w32"); _chk(bias, F32, "bias"); _chk(out32, F32, "out32")
    M, K = a32.shape
    _lib.check(L.eend_linear_step_f32(_p(a32), a32.stride(0), _p(w32), w32.stride(0), _p(bias), _p(out32), out32.stride(0), M,
                                      w32.shape[0], K, act, _stream()), "eend_linear_step_f32")


def linear_res_ln_step_f32(a32, w32, bias, res, gamma, beta, out32, eps=1e-5, alpha=1.0, out16=None):
    """out32 = LayerNorm((a32 w32^T + bias) * alpha + res), f32 operands; out32 may alias res."""
    L = _lib.load()
    _chk(a32, F32, "a32"); _chk(w32, F32, "w32"); _chk(bias, F32, "bias"); _chk(res, F32, "res"); _chk(gamma, F32, "gamma")
    _chk(beta, F32, "beta"); _chk(out32, F32, "out32"); _chk(out16, F16, "out16")
    M, K = a32.shape
    if w32.shape[0] != 256:
        raise _lib.EendHipError("linear_res_ln_step_f32: N must be 256")
    _lib.check(L.eend_linear_res_ln_step_f32(_p(a32), a32.stride(0), _p(w32), w32.stride(0), _p(bias), _p(res), float(alpha), _p(gamma),
                                             _p(beta), eps, _p(out32), _p(out16), M, K, _stream()), "eend_linear_res_ln_step_f32")


def linear_res_scale_ln_step_f32(a32, w32, bias, res, alpha, gamma, beta, out32, ln_out32=None, ln_out16=None, eps=1e-5):
    """out32 = (a32 w32^T + bias) * alpha + res (un-normalised stream, may alias res); ln_out32 / ln_out16 = LayerNorm(out32)."""
    L = _lib.load()
    for n, t in (("a32", a32), ("w32", w32), ("bias", bias), ("res", res), ("gamma", gamma), ("beta", beta), ("out32", out32), ("ln_out32", ln_out32)):
        _chk(t, F32, n)
    _chk(ln_out16, F16, "ln_out16")
    M, K = a32.shape
    if w32.shape[0] != 256:
        raise _lib.EendHipError("linear_res_scale_ln_step_f32: N must be 256")
    _lib.check(L.eend_linear_res_scale_ln_step_f32(_p(a32), a32.stride(0), _p(w32), w32.stride(0), _p(bias), _p(res), float(alpha),
                                                   _p(gamma), _p(beta), eps, _p(out32), _p(ln_out32), _p(ln_out16), M, K, _stream()),
               "eend_linear_res_scale_ln_step_f32")


def layernorm_rows_f32(x32, gamma, beta, out32, eps=1e-5):
    L = _lib.load()
    _chk(x32, F32, "x32"); _chk(gamma, F32, "gamma"); _chk(beta, F32, "beta"); _chk(out32, F32, "out32")
    if x32.shape[-1] != 256:
        raise _lib.EendHipError("layernorm_rows_f32: rows of 256 features")
    _lib.check(L.eend_layernorm_rows_f32(_p(x32), _p(gamma), _p(beta), eps, _p(out32), x32.numel() // 256, _stream()),
               "eend_layernorm_rows_f32")


def l2norm_rows_f32(x32, y32):
    L = _lib.load()
    _chk(x32, F32, "x32"); _chk(y32, F32, "y32")
    if x32.shape[-1] != 256:
        raise _lib.EendHipError("l2norm_rows_f32: rows of 256 features")
    _lib.check(L.eend_l2norm_rows_f32(_p(x32), _p(y32), x32.numel() // 256, _stream()), "eend_l2norm_rows_f32")


def spk_attn_step_f32(qkv32, out32, B, C):
    L = _lib.load()
    _chk(qkv32, F32, "qkv32"); _chk(out32, F32, "out32")
    _lib.check(L.eend_spk_attn_step_f32(_p(qkv32), _p(out32), B, C, 1.0 / math.sqrt(64.0), _stream()), "eend_spk_attn_step_f32")


def convert_fanout_step_f32(emb32, w32, pc, out32, out16, B, C):
    """One frame of `convert(cat(emb, pe_c))` in f32: emb32 (B, 256), w32 the (256, 512) convert.weight, pc (C, 256)."""
    L = _lib.load()
    _chk(emb32, F32, "emb32"); _chk(w32, F32, "w32"); _chk(pc, F32, "pc"); _chk(out32, F32, "out32"); _chk(out16, F16, "out16")
    _lib.check(L.eend_convert_fanout_step_f32(_p(emb32), _p(w32), w32.stride(0), _p(pc), _p(out32), _p(out16), B, C, _stream()),
               "eend_convert_fanout_step_f32")


def dwconv_step(x16, cache, w, bn, out16, eps=1e-5):
    """x16/out16 f16 (B, D); cache f32 (B, D, k-1) shifted in place; w f32 (D, k)."""
    L = _lib.load()
    _chk(x16, F16, "x16"); _chk(cache, F32, "cache"); _chk(w, F32, "w"); _chk(out16, F16, "out16")
    for t in bn:
        _chk(t, F32, "bn")
    B, D = x16.shape
    _lib.check(L.eend_dwconv_step_f16(_p(x16), _p(cache), _p(w), _p(bn[0]), _p(bn[1]), _p(bn[2]), _p(bn[3]), eps,
                                      _p(out16), B, D, w.shape[1], _stream()), "eend_dwconv_step_f16")


def attn_decode(qkv16, k_cache, v_cache, out16, N, H, cap, t):
    """Append the new token's k/v (row t) to the caches (N,H,cap,64) f16 and attend over t+1 tokens."""
    L = _lib.load()
    _chk(qkv16, F16, "qkv16"); _chk(k_cache, F16, "k_cache"); _chk(v_cache, F16, "v_cache"); _chk(out16, F16, "out16")
    _lib.check(L.eend_attn_decode_f16(_p(qkv16), _p(k_cache), _p(v_cache), _p(out16), N, H, cap, t,
                                      1.0 / math.sqrt(64.0), _stream()), "eend_attn_decode_f16")


def attn_decode_dev(qkv16, k_cache, v_cache, out16, N, H, cap, t_dev):
    """attn_decode with the token count in device memory (int32 tensor of one element): graph-capturable."""
    L = _lib.load()
    _chk(qkv16, F16, "qkv16"); _chk(k_cache, F16, "k_cache"); _chk(v_cache, F16, "v_cache"); _chk(out16, F16, "out16")
    _chk(t_dev, torch.int32, "t_dev")
    _lib.check(L.eend_attn_decode_dev_f16(_p(qkv16), _p(k_cache), _p(v_cache), _p(out16), N, H, cap, _p(t_dev),
                                          1.0 / math.sqrt(64.0), _stream()), "eend_attn_decode_dev_f16")


SPLIT_DECODE_MIN_CAP = 4096      # cache capacities from here on take the key-split decode kernel


def attn_decode_split_ws(N, H, cap):
    return N * H * ((cap + 511) // 512) * 66


def attn_decode_split(qkv16, k_cache, v_cache, out16, ws, N, H, cap, t_dev):
    """attn_decode_dev with the history split over cap/512 workgroups per (n, h) + a merge kernel (long streams)."""
    L = _lib.load()
    _chk(qkv16, F16, "qkv16"); _chk(k_cache, F16, "k_cache"); _chk(v_cache, F16, "v_cache"); _chk(out16, F16, "out16")
    _chk(t_dev, torch.int32, "t_dev"); _chk(ws, F32, "ws")
    _lib.check(L.eend_attn_decode_split_f16(_p(qkv16), _p(k_cache), _p(v_cache), _p(out16), _p(ws), ws.numel(), N, H, cap, _p(t_dev),
                                            1.0 / math.sqrt(64.0), _stream()), "eend_attn_decode_split_f16")


def counter_add(counter_i32, inc=1):
    L = _lib.load()
    _chk(counter_i32, torch.int32, "counter")
    _lib.check(L.eend_counter_add_i32(_p(counter_i32), inc, _stream()), "eend_counter_add_i32")


def attn_decode_ragged_ws(N, H, cap):
    return N * H * ((cap + 511) // 512) * 66


def attn_decode_ragged(qkv16, k_cache, v_cache, out16, ws, N, H, cap, rows_per_seq, len_dev, mask_dev):
    """Key-split decode over ragged histories: row n belongs to sequence n // rows_per_seq, whose history length is len_dev[s]
    (int32); rows with mask_dev[s] != 0 append their k / v at row len and attend over len + 1 tokens, the others leave the
    caches alone and get a zero output row.  The lengths are not advanced (counter_add_masked)."""
    L = _lib.load()
    _chk(qkv16, F16, "qkv16"); _chk(k_cache, F16, "k_cache"); _chk(v_cache, F16, "v_cache"); _chk(out16, F16, "out16")
    _chk(len_dev, torch.int32, "len_dev"); _chk(mask_dev, torch.int32, "mask_dev"); _chk(ws, F32, "ws")
    if N % rows_per_seq or len_dev.numel() < N // rows_per_seq or mask_dev.numel() < N // rows_per_seq:
        raise _lib.EendHipError("attn_decode_ragged: one length and one mask per sequence of rows_per_seq rows")
    if k_cache.shape != (N, H, cap, 64) or v_cache.shape != (N, H, cap, 64) or qkv16.shape[0] < N or out16.shape[0] < N:
        raise _lib.EendHipError("attn_decode_ragged: shape mismatch")
    _lib.check(L.eend_attn_decode_ragged_f16(_p(qkv16), _p(k_cache), _p(v_cache), _p(out16), _p(ws), ws.numel(), N, H, cap,
                                             rows_per_seq, _p(len_dev), _p(mask_dev), 1.0 / math.sqrt(64.0), _stream()),
               "eend_attn_decode_ragged_f16")


def counter_add_masked(len_i32, mask_i32):
    """len[s] += (mask[s] != 0) for every s, in one launch."""
    L = _lib.load()
    _chk(len_i32, torch.int32, "len"); _chk(mask_i32, torch.int32, "mask")
    if mask_i32.numel() < len_i32.numel():
        raise _lib.EendHipError("counter_add_masked: one mask per counter")
    _lib.check(L.eend_counter_add_masked_i32(_p(len_i32), _p(mask_i32), len_i32.numel(), _stream()), "eend_counter_add_masked_i32")


SEGTRACK_HDR = 4                                  # per-slot header of the segment box: frames, count, overflow, 0


def segtrack_feed(desc_i64, counts_i32, ends_i32, n, ld, col0, ntracks, threshold, median, is_prob, hist, open_i32, box, cap,
                  sad_desc_i64=None):
    """Advance n slots of a segment tracker in one launch: entry e feeds counts[e] rows from the address desc[e][0] (row stride
    ld floats) to slot desc[e][1]; ends[e] != 0 (ends may be None) ends that stream.  State: hist int64 (S, 64), open int32
    (S, 64), box int32 (S, SEGTRACK_HDR + 3 cap) (include/eend_hip.h eend_segtrack_feed_f32).  sad_desc_i64 (n addresses of
    uint8 flags, one per row of the entry) gates the decisions with a speech-activity mask (eend_segtrack_feed_sad_f32)."""
    L = _lib.load()
    _chk(desc_i64, torch.int64, "desc"); _chk(counts_i32, torch.int32, "counts"); _chk(ends_i32, torch.int32, "ends")
    _chk(hist, torch.int64, "hist"); _chk(open_i32, torch.int32, "open"); _chk(box, torch.int32, "box")
    S = box.shape[0]
    if (desc_i64.numel() < 2 * n or counts_i32.numel() < n or (ends_i32 is not None and ends_i32.numel() < n) or hist.shape != (S, 64)
            or open_i32.shape != (S, 64) or box.shape[1] != SEGTRACK_HDR + 3 * cap):
        raise _lib.EendHipError("segtrack_feed: shape mismatch")
    if sad_desc_i64 is not None:
        _chk(sad_desc_i64, torch.int64, "sad_desc")
        if sad_desc_i64.numel() < n:
            raise _lib.EendHipError("segtrack_feed: one flag address per entry")
        _lib.check(L.eend_segtrack_feed_sad_f32(_p(desc_i64), _p(counts_i32), _p(ends_i32), _p(sad_desc_i64), n, ld, col0, ntracks,
                                                float(threshold), median, int(bool(is_prob)), _p(hist), _p(open_i32), _p(box), S, cap,
                                                _stream()), "eend_segtrack_feed_sad_f32")
        return
    _lib.check(L.eend_segtrack_feed_f32(_p(desc_i64), _p(counts_i32), _p(ends_i32), n, ld, col0, ntracks, float(threshold), median,
                                        int(bool(is_prob)), _p(hist), _p(open_i32), _p(box), S, cap, _stream()), "eend_segtrack_feed_f32")


COPY_BLOCKS_MAX = 64                             # EEND_COPY_BLOCKS_MAX: entries of one eend_copy_blocks launch


def copy_blocks(entries):
    """Batched strided block copy between device buffers on the current stream: entries = [(src, dst, nblocks, block_bytes,
    src_stride, dst_stride), ...], device addresses and byte counts, every one a multiple of 16 (include/eend_hip.h
    eend_copy_blocks).  One launch per COPY_BLOCKS_MAX entries; entries that move nothing are skipped by the library.  The
    entries travel in the kernel arguments, so nothing has to outlive the call but the buffers themselves."""
    L = _lib.load()
    entries = list(entries)
    for a in range(0, len(entries), COPY_BLOCKS_MAX):
        part = entries[a:a + COPY_BLOCKS_MAX]
        arr = (_lib.BlockCopy * len(part))(*[_lib.BlockCopy(*(int(v) for v in e)) for e in part])
        _lib.check(L.eend_copy_blocks(arr, len(part), _stream()), "eend_copy_blocks")


def copy_blocks_tile_bytes() -> int:
    """Bytes one workgroup of eend_copy_blocks moves per tile."""
    return int(_lib.load().eend_copy_blocks_tile_bytes())


WIN_KEEP, WIN_PUSH, WIN_FLUSH = 0, 1, 2


def window_push(win16, x32, mode_i32):
    """Look-ahead windows f16 (S, k*D) of S slots: per slot keep / shift + append x32[s] (f32 -> f16) / shift + append zeros."""
    L = _lib.load()
    _chk(win16, F16, "win16"); _chk(x32, F32, "x32"); _chk(mode_i32, torch.int32, "mode")
    S, D = x32.shape
    if win16.shape[0] != S or win16.shape[1] % D or mode_i32.numel() < S:
        raise _lib.EendHipError("window_push: shape mismatch")
    _lib.check(L.eend_window_push_f16(_p(win16), _p(x32), _p(mode_i32), S, win16.shape[1] // D, D, _stream()), "eend_window_push_f16")


def attn_chunk_ragged_ws(Nseq, H, cap, nmax):
    return Nseq * H * ((cap + 511) // 512) * nmax * 66


def attn_chunk_ragged(qkv16, k_cache, v_cache, out16, ws, Nseq, H, cap, nmax, rows_per_seq, len_dev, cnt_dev):
    """Chunk attention over ragged histories: rows q*nmax + j of qkv16 are frames j of sequence q, which belongs to slot
    q // rows_per_seq with history length len_dev[s] and cnt_dev[s] (0..nmax) new frames (int32).  Frame j < cnt attends over
    its len cached keys and the chunk's keys 0..j and appends its k / v at row len + j; rows j >= cnt, and every row of a slot
    with cnt == 0 or len + cnt > cap, are zero and leave the caches alone.  The lengths are not advanced (counter_add_count)."""
    L = _lib.load()
    _chk(qkv16, F16, "qkv16"); _chk(k_cache, F16, "k_cache"); _chk(v_cache, F16, "v_cache"); _chk(out16, F16, "out16")
    _chk(len_dev, torch.int32, "len_dev"); _chk(cnt_dev, torch.int32, "cnt_dev"); _chk(ws, F32, "ws")
    if not 1 <= nmax <= 64:
        raise _lib.EendHipError("attn_chunk_ragged: nmax must be in 1..64")
    if Nseq % rows_per_seq or len_dev.numel() < Nseq // rows_per_seq or cnt_dev.numel() < Nseq // rows_per_seq:
        raise _lib.EendHipError("attn_chunk_ragged: one length and one count per slot of rows_per_seq sequences")
    if (k_cache.shape != (Nseq, H, cap, 64) or v_cache.shape != (Nseq, H, cap, 64) or qkv16.shape[0] < Nseq * nmax
            or qkv16.shape[-1] != 3 * H * 64 or out16.shape[0] < Nseq * nmax or out16.shape[-1] != H * 64):
        raise _lib.EendHipError("attn_chunk_ragged: shape mismatch")
    if ws.numel() < attn_chunk_ragged_ws(Nseq, H, cap, nmax):
        raise _lib.EendHipError("attn_chunk_ragged: workspace too small (attn_chunk_ragged_ws)")
    _lib.check(L.eend_attn_chunk_ragged_f16(_p(qkv16), _p(k_cache), _p(v_cache), _p(out16), _p(ws), ws.numel(), Nseq, H, cap, nmax,
                                            rows_per_seq, _p(len_dev), _p(cnt_dev), 1.0 / math.sqrt(64.0), _stream()),
               "eend_attn_chunk_ragged_f16")


def attn_prefill(qkv16, k_cache, v_cache, out16, seq0, Nseq, H, t0, Tq):
    """Causal prefill attention over K/V caches f16 (Ncache, H, cap, 64): rows i*Tq + j of qkv16 (rows of 3*H*64 halves, any row
    stride that is a multiple of 8) are the Tq >= 1 new frames j of cache sequence seq0 + i, i < Nseq, which all have history
    length t0.  Frame j's k / v are copied to cache row t0 + j and out16 (Nseq*Tq, H*64) row i*Tq + j is the attention of query
    j over cache keys [0, t0 + j]; cache rows at or beyond t0 + Tq and other sequences are neither read nor written.  Work items
    are (sequence, head, 128-query tile): few queries over a long history are the case of attn_chunk_ragged, not of this kernel."""
    L = _lib.load()
    _chk(k_cache, F16, "k_cache"); _chk(v_cache, F16, "v_cache"); _chk(out16, F16, "out16")
    if not qkv16.is_cuda or qkv16.dtype != F16 or qkv16.dim() != 2 or qkv16.stride(1) != 1:
        raise _lib.EendHipError("attn_prefill: qkv16 must be f16 GPU rows with unit column stride")
    if Tq < 1 or Nseq < 1 or t0 < 0 or seq0 < 0:
        raise _lib.EendHipError("attn_prefill: Nseq >= 1 sequences from seq0 >= 0, Tq >= 1 frames at t0 >= 0")
    if (k_cache.dim() != 4 or k_cache.shape[1] != H or k_cache.shape[3] != 64 or v_cache.shape != k_cache.shape
            or qkv16.shape != (Nseq * Tq, 3 * H * 64) or out16.shape != (Nseq * Tq, H * 64)):
        raise _lib.EendHipError("attn_prefill: shape mismatch")
    Ncache, cap = k_cache.shape[0], k_cache.shape[2]
    if seq0 + Nseq > Ncache:
        raise _lib.EendHipError(f"attn_prefill: sequences {seq0}..{seq0 + Nseq - 1} outside a cache of {Ncache}")
    if t0 + Tq > cap:
        raise _lib.EendHipError(f"attn_prefill: {t0} + {Tq} frames exceed the cache capacity {cap}")
    _lib.check(L.eend_attn_prefill_f16(_p(qkv16), qkv16.stride(0), _p(k_cache), _p(v_cache), _p(out16), Ncache, seq0, Nseq, H, cap, t0,
                                       Tq, 1.0 / math.sqrt(64.0), _stream()), "eend_attn_prefill_f16")


def counter_add_count(len_i32, cnt_i32):
    """len[s] += cnt[s] for every s, in one launch."""
    L = _lib.load()
    _chk(len_i32, torch.int32, "len"); _chk(cnt_i32, torch.int32, "cnt")
    if cnt_i32.numel() < len_i32.numel():
        raise _lib.EendHipError("counter_add_count: one count per counter")
    _lib.check(L.eend_counter_add_count_i32(_p(len_i32), _p(cnt_i32), len_i32.numel(), _stream()), "eend_counter_add_count_i32")


def window_chunk(win16, x32, cols16, npush_i32, ndummy_i32, ndec_i32, nmax):
    """Look-ahead windows f16 (S, k*D) over a chunk: slot s takes npush[s] frames x32[s*nmax + j] (f32 (S*nmax, D)) and then
    ndummy[s] zero frames; cols16 f16 (S*nmax, k*D) gets the ndec[s] emitting windows of the slot, in order, then zero rows."""
    L = _lib.load()
    _chk(win16, F16, "win16"); _chk(x32, F32, "x32"); _chk(cols16, F16, "cols16")
    for t, n in ((npush_i32, "npush"), (ndummy_i32, "ndummy"), (ndec_i32, "ndec")):
        _chk(t, torch.int32, n)
    S = win16.shape[0]
    D = x32.shape[-1]
    if (nmax < 1 or x32.numel() != S * nmax * D or win16.shape[1] % D or cols16.shape != (S * nmax, win16.shape[1])
            or min(npush_i32.numel(), ndummy_i32.numel(), ndec_i32.numel()) < S):
        raise _lib.EendHipError("window_chunk: shape mismatch")
    _lib.check(L.eend_window_chunk_f16(_p(win16), _p(x32), _p(cols16), _p(npush_i32), _p(ndummy_i32), _p(ndec_i32), S, nmax,
                                       win16.shape[1] // D, D, _stream()), "eend_window_chunk_f16")


def retention_step_ragged(qkvg32, kv_state, len_dev, mask_dev, rows_per_seq, N, H, gn_eps=1e-6, out16=None, out32=None):
    """retention_step_f32 over slots at different positions: row n belongs to sequence n // rows_per_seq, whose scale is its own
    length len_dev[s] (int32; 0 = empty state, never read).  mask_dev[s] == 0 leaves the state untouched and zeroes the output
    rows.  The lengths are not advanced (counter_add_masked)."""
    L = _lib.load()
    _chk(qkvg32, F32, "qkvg32"); _chk(kv_state, F32, "kv_state"); _chk(out16, F16, "out16"); _chk(out32, F32, "out32")
    _chk(len_dev, torch.int32, "len_dev"); _chk(mask_dev, torch.int32, "mask_dev")
    if out16 is None and out32 is None:
        raise _lib.EendHipError("retention_step_ragged: out16 and / or out32")
    if rows_per_seq <= 0 or N % rows_per_seq or len_dev.numel() < N // rows_per_seq or mask_dev.numel() < N // rows_per_seq:
        raise _lib.EendHipError("retention_step_ragged: one length and one mask per sequence of rows_per_seq rows")
    D = H * 64
    if (kv_state.numel() < N * H * 64 * 64 or qkvg32.numel() < N * 4 * D or (out16 is not None and out16.numel() < N * D)
            or (out32 is not None and out32.numel() < N * D)):
        raise _lib.EendHipError("retention_step_ragged: shape mismatch")
    _lib.check(L.eend_retention_step_ragged_f32(_p(qkvg32), _p(kv_state), _p(len_dev), _p(mask_dev), rows_per_seq, _p(out16), _p(out32),
                                                N, H, gn_eps, _stream()), "eend_retention_step_ragged_f32")


def dwconv_step_ragged(x16, cache, len_dev, mask_dev, w, bn, out16, eps=1e-5):
    """dwconv_step per slot: mask_dev[b] != 0 shifts slot b's cache f32 (B, D, k-1) in place (len_dev[b] == 0: the cache is read
    as zeros), mask_dev[b] == 0 leaves it as it is and zeroes the output row."""
    L = _lib.load()
    _chk(x16, F16, "x16"); _chk(cache, F32, "cache"); _chk(w, F32, "w"); _chk(out16, F16, "out16")
    _chk(len_dev, torch.int32, "len_dev"); _chk(mask_dev, torch.int32, "mask_dev")
    for t in bn:
        _chk(t, F32, "bn")
    B, D = x16.shape
    k = w.shape[1]
    if (cache.shape != (B, D, k - 1) or out16.shape != (B, D) or w.shape[0] != D or len_dev.numel() < B or mask_dev.numel() < B
            or any(t.numel() < D for t in bn)):
        raise _lib.EendHipError("dwconv_step_ragged: shape mismatch")
    _lib.check(L.eend_dwconv_step_ragged_f16(_p(x16), _p(cache), _p(len_dev), _p(mask_dev), _p(w), _p(bn[0]), _p(bn[1]), _p(bn[2]),
                                             _p(bn[3]), eps, _p(out16), B, D, k, _stream()), "eend_dwconv_step_ragged_f16")


def window_push_f32(win32, x32, mode_i32):
    """window_push on f32 windows (S, k*D): per slot keep / shift + append x32[s] / shift + append zeros."""
    L = _lib.load()
    _chk(win32, F32, "win32"); _chk(x32, F32, "x32"); _chk(mode_i32, torch.int32, "mode")
    S, D = x32.shape
    if win32.shape[0] != S or win32.shape[1] % D or mode_i32.numel() < S:
        raise _lib.EendHipError("window_push_f32: shape mismatch")
    _lib.check(L.eend_window_push_f32(_p(win32), _p(x32), _p(mode_i32), S, win32.shape[1] // D, D, _stream()), "eend_window_push_f32")


def retention_chunk_ragged(qkvg32, kv_state, len_dev, cnt_dev, seq_per_slot, Nseq, H, nmax, gn_eps=1e-6, out16=None, out32=None):
    """retention_step_ragged over a chunk: rows q*nmax + j of qkvg32 are frames j of sequence q, which belongs to slot
    q // seq_per_slot; the slot takes cnt_dev[s] (0..nmax) frames at position len_dev[s].  The state is read and written once;
    outputs and state are bit for bit those of cnt successive retention_step_ragged calls.  Rows beyond a slot's count are
    zero.  The lengths are not advanced (counter_add_count)."""
    L = _lib.load()
    _chk(qkvg32, F32, "qkvg32"); _chk(kv_state, F32, "kv_state"); _chk(out16, F16, "out16"); _chk(out32, F32, "out32")
    _chk(len_dev, torch.int32, "len_dev"); _chk(cnt_dev, torch.int32, "cnt_dev")
    if out16 is None and out32 is None:
        raise _lib.EendHipError("retention_chunk_ragged: out16 and / or out32")
    if not 1 <= nmax <= 64:
        raise _lib.EendHipError("retention_chunk_ragged: nmax must be in 1..64")
    if seq_per_slot <= 0 or Nseq <= 0 or Nseq % seq_per_slot or len_dev.numel() < Nseq // seq_per_slot or cnt_dev.numel() < Nseq // seq_per_slot:
        raise _lib.EendHipError("retention_chunk_ragged: one length and one count per slot of seq_per_slot sequences")
    D, R = H * 64, Nseq * nmax
    if (kv_state.numel() < Nseq * H * 64 * 64 or qkvg32.numel() < R * 4 * D or (out16 is not None and out16.numel() < R * D)
            or (out32 is not None and out32.numel() < R * D)):
        raise _lib.EendHipError("retention_chunk_ragged: shape mismatch")
    _lib.check(L.eend_retention_chunk_ragged_f32(_p(qkvg32), _p(kv_state), _p(len_dev), _p(cnt_dev), seq_per_slot, nmax, _p(out16),
                                                 _p(out32), Nseq, H, gn_eps, _stream()), "eend_retention_chunk_ragged_f32")


def dwconv_chunk_ragged(x16, cache, len_dev, cnt_dev, w, bn, out16, nmax, eps=1e-5):
    """dwconv_step_ragged over a chunk: x16 / out16 (B*nmax, D), slot b's frames are rows b*nmax + j, j < cnt_dev[b]; the cache
    f32 (B, D, k-1) ends as after cnt one-frame calls (bit-identical, as are the outputs); rows beyond the count are zero."""
    L = _lib.load()
    _chk(x16, F16, "x16"); _chk(cache, F32, "cache"); _chk(w, F32, "w"); _chk(out16, F16, "out16")
    _chk(len_dev, torch.int32, "len_dev"); _chk(cnt_dev, torch.int32, "cnt_dev")
    for t in bn:
        _chk(t, F32, "bn")
    if not 1 <= nmax <= 64:
        raise _lib.EendHipError("dwconv_chunk_ragged: nmax must be in 1..64")
    B, D = cache.shape[0], cache.shape[1]
    k = w.shape[1]
    if (x16.shape != (B * nmax, D) or cache.shape != (B, D, k - 1) or out16.shape != (B * nmax, D) or w.shape[0] != D
            or len_dev.numel() < B or cnt_dev.numel() < B or any(t.numel() < D for t in bn)):
        raise _lib.EendHipError("dwconv_chunk_ragged: shape mismatch")
    _lib.check(L.eend_dwconv_chunk_ragged_f16(_p(x16), _p(cache), _p(len_dev), _p(cnt_dev), nmax, _p(w), _p(bn[0]), _p(bn[1]), _p(bn[2]),
                                              _p(bn[3]), eps, _p(out16), B, D, k, _stream()), "eend_dwconv_chunk_ragged_f16")


def retention_prefill_ws(Nseq, H, T):
    """Floats of workspace retention_prefill needs: one 64 x 64 tile per (sequence, head, chunk of 64 frames)."""
    return Nseq * H * ((T + 63) // 64) * 4096


def retention_prefill(qkvg32, kv_state, ws, seq0, Nseq, H, t0, T, gn_eps=1e-6, out16=None, out32=None):
    """The retention recurrence over a backlog in chunk-parallel f32 form: rows i*T + j of qkvg32 (Nseq*T, 4*H*64) are frames
    t0 + j of state sequence seq0 + i of kv_state f32 (Ncache, H, 64, 64), i < Nseq, which all stand at position t0 >= 0 (0: the
    state is not read).  out16 / out32 (Nseq*T, H*64) get the frames' outputs and the state ends as after T per-frame updates;
    no other sequence or row is touched.  ws: f32 scratch of retention_prefill_ws(Nseq, H, T) floats."""
    L = _lib.load()
    _chk(qkvg32, F32, "qkvg32"); _chk(kv_state, F32, "kv_state"); _chk(out16, F16, "out16"); _chk(out32, F32, "out32")
    _chk(ws, F32, "ws")
    if out16 is None and out32 is None:
        raise _lib.EendHipError("retention_prefill: out16 and / or out32")
    if T < 1 or Nseq < 1 or t0 < 0 or seq0 < 0:
        raise _lib.EendHipError("retention_prefill: Nseq >= 1 sequences from seq0 >= 0, T >= 1 frames at t0 >= 0")
    D = H * 64
    if (kv_state.dim() != 4 or kv_state.shape[1:] != (H, 64, 64) or qkvg32.shape != (Nseq * T, 4 * D)
            or (out16 is not None and out16.shape != (Nseq * T, D)) or (out32 is not None and out32.shape != (Nseq * T, D))):
        raise _lib.EendHipError("retention_prefill: shape mismatch")
    if seq0 + Nseq > kv_state.shape[0]:
        raise _lib.EendHipError(f"retention_prefill: sequences {seq0}..{seq0 + Nseq - 1} outside a state of {kv_state.shape[0]}")
    if ws.numel() < retention_prefill_ws(Nseq, H, T):
        raise _lib.EendHipError("retention_prefill: workspace too small (retention_prefill_ws)")
    _lib.check(L.eend_retention_prefill_f32(_p(qkvg32), _p(kv_state), _p(out16), _p(out32), _p(ws), ws.numel(), kv_state.shape[0],
                                            seq0, Nseq, H, t0, T, gn_eps, _stream()), "eend_retention_prefill_f32")


def dwconv_prefill(x16, cache, b, t0, w, bn, out16, eps=1e-5):
    """dwconv_step_ragged for slot b alone over the T frames x16 / out16 (T, D), frame-parallel: outputs and the slot's row of
    cache f32 (B, D, k-1) end bit for bit as after T one-frame calls from position t0 (0: the row is read as zeros)."""
    L = _lib.load()
    _chk(x16, F16, "x16"); _chk(cache, F32, "cache"); _chk(w, F32, "w"); _chk(out16, F16, "out16")
    for t in bn:
        _chk(t, F32, "bn")
    if x16.dim() != 2 or cache.dim() != 3:
        raise _lib.EendHipError("dwconv_prefill: x16 (T, D), cache (B, D, k-1)")
    T, D = x16.shape
    B, k = cache.shape[0], w.shape[1]
    if (T < 1 or t0 < 0 or not 0 <= b < B or cache.shape != (B, D, k - 1) or out16.shape != (T, D) or w.shape[0] != D
            or any(t.numel() < D for t in bn)):
        raise _lib.EendHipError("dwconv_prefill: shape mismatch")
    _lib.check(L.eend_dwconv_prefill_f16(_p(x16), _p(cache), b, t0, _p(w), _p(bn[0]), _p(bn[1]), _p(bn[2]), _p(bn[3]), eps, _p(out16),
                                         T, B, D, k, _stream()), "eend_dwconv_prefill_f16")


def window_chunk_f32(win32, x32, cols32, npush_i32, ndummy_i32, ndec_i32, nmax):
    """window_chunk on f32 windows (S, k*D): x32 (S*nmax, D), cols32 (S*nmax, k*D) the im2col rows of the emitting windows,
    compacted to each slot's first rows; the stored window ends as after the same pushes and dummies through window_push_f32."""
    L = _lib.load()
    _chk(win32, F32, "win32"); _chk(x32, F32, "x32"); _chk(cols32, F32, "cols32")
    for t in (npush_i32, ndummy_i32, ndec_i32):
        _chk(t, torch.int32, "counts")
    if not 1 <= nmax <= 64:
        raise _lib.EendHipError("window_chunk_f32: nmax must be in 1..64")
    S, D = win32.shape[0], x32.shape[1]
    if (x32.shape[0] != S * nmax or win32.shape[1] % D or cols32.shape != (S * nmax, win32.shape[1])
            or any(t.numel() < S for t in (npush_i32, ndummy_i32, ndec_i32))):
        raise _lib.EendHipError("window_chunk_f32: shape mismatch")
    _lib.check(L.eend_window_chunk_f32(_p(win32), _p(x32), _p(cols32), _p(npush_i32), _p(ndummy_i32), _p(ndec_i32), S, nmax,
                                       win32.shape[1] // D, D, _stream()), "eend_window_chunk_f32")


def spk_attn_rows_f32(qkv32, out32, B, C, Tp):
    """spk_attn_step_f32 on decoder slabs: rows (b*C + c)*Tp + t; the C rows of frame (b, t) attend to each other."""
    L = _lib.load()
    _chk(qkv32, F32, "qkv32"); _chk(out32, F32, "out32")
    if B <= 0 or Tp <= 0 or not 1 <= C <= 16 or qkv32.numel() < B * C * Tp * 768 or out32.numel() < B * C * Tp * 256:
        raise _lib.EendHipError("spk_attn_rows_f32: shape mismatch")
    _lib.check(L.eend_spk_attn_rows_f32(_p(qkv32), _p(out32), B, C, Tp, 1.0 / math.sqrt(64.0), _stream()), "eend_spk_attn_rows_f32")


_PTR_TABLES = {}


def gather_bn_cast_pad(src, bn, out16, T, Tp, pad_value, apply_bn=True, eps=1e-5):
    """src: list of B f32 GPU tensors (T_i, Fin) -> out16 f16 (B*Tp, Fpad) in one launch (pointer table)."""
    L = _lib.load()
    _chk(out16, F16, "out16")
    for s_ in src:
        _chk(s_, F32, "src[i]")
    B, Fin, Fpad = len(src), src[0].shape[1], out16.shape[-1]
    if Fpad > 512:
        raise _lib.EendHipError(f"gather_bn_cast_pad: padded feature width {Fpad} > 512 (in_size {Fin}): the gather kernel holds "
                                "four feature pairs per lane; the shipped configs use in_size 345")
    tab = _ptr_table(src, T, out16.device)
    w = b = m = v = None
    if apply_bn:
        w, b, m, v = bn
    _lib.check(L.eend_gather_bn_cast_pad_f16(_p(tab[0]), _p(tab[1]), float(pad_value), _p(w), _p(b), _p(m), _p(v), eps,
                                             _p(out16), B, T, Tp, Fin, Fpad, 1 if apply_bn else 0, _stream()),
               "eend_gather_bn_cast_pad_f16")
    return out16


def _ptr_table(src, T, dev):
    key = tuple((s_.data_ptr(), s_.shape[0]) for s_ in src)
    tab = _PTR_TABLES.get(key)
    if tab is None:                                            # tiny H2D upload, cached per (pointers, lengths)
        if len(_PTR_TABLES) > 64:
            _PTR_TABLES.clear()
        tab = (torch.tensor([k[0] for k in key], dtype=torch.int64, device=dev),
               torch.tensor([min(k[1], T) for k in key], dtype=torch.int32, device=dev))
        _PTR_TABLES[key] = tab
    return tab


def encoder_input_ok(src, Tp, w16):
    """True where encoder_input covers the shapes (else the caller runs gather_bn_cast_pad + linear_res_ln)."""
    Fin = src[0].shape[1]
    return (bool(_lib.load().eend_encoder_input_ok(int(Fin), int(Tp), int(w16.stride(0)))) and w16.shape[0] == 256
            and all(s_.is_contiguous() and s_.data_ptr() % 16 == 0 and s_.shape[1] == Fin for s_ in src))


def encoder_input(src, bn, w16, bias, gamma, beta, out32, out16, T, Tp, pad_value, bn_eps=1e-5, eps=1e-5):
    """out = LayerNorm(BN(pad_sequence(src, pad_value)) @ w16.T + bias) in one launch (encin.hip): src list of B f32 GPU tensors
    (T_i, Fin); w16 f16 (256, >= ceil32(Fin)) zero-padded; out16 f16 (B*Tp, 256), out32 optional."""
    L = _lib.load()
    _chk(w16, F16, "w16"); _chk(out16, F16, "out16"); _chk(out32, F32, "out32")
    for n, t in (("bias", bias), ("gamma", gamma), ("beta", beta)) + tuple(("bn", t) for t in bn):
        _chk(t, F32, n)
    for s_ in src:
        _chk(s_, F32, "src[i]")
    B, Fin = len(src), src[0].shape[1]
    if out16.shape != (B * Tp, 256) or not encoder_input_ok(src, Tp, w16):
        raise _lib.EendHipError("encoder_input: unsupported shapes (see eend_encoder_input_ok)")
    tab = _ptr_table(src, T, out16.device)
    w, b, m, v = bn
    _lib.check(L.eend_encoder_input_f16(_p(tab[0]), _p(tab[1]), float(pad_value), _p(w), _p(b), _p(m), _p(v), bn_eps, _p(w16), w16.stride(0),
                                        _p(bias), _p(gamma), _p(beta), eps, _p(out32), _p(out16), B, T, Tp, Fin, _stream()),
               "eend_encoder_input_f16")


def linear_res16_ln(a16, w16, bias, res16, gamma, beta, out32, out16, eps=1e-5, alpha=1.0):
    """out = LayerNorm((a16 @ w16.T + bias) * alpha + res16) with the residual read from the f16 stream; out32 may be None."""
    L = _lib.load()
    _chk(a16, F16, "a16"); _chk(w16, F16, "w16"); _chk(bias, F32, "bias"); _chk(res16, F16, "res16")
    _chk(gamma, F32, "gamma"); _chk(beta, F32, "beta"); _chk(out32, F32, "out32"); _chk(out16, F16, "out16")
    M, K = a16.shape
    if w16.shape[0] != 256:
        raise _lib.EendHipError("linear_res16_ln: N must be 256")
    _lib.check(L.eend_linear_res16_ln_f16(_p(a16), a16.stride(0), _p(w16), w16.stride(0), _p(bias), _p(res16), float(alpha), _p(gamma),
                                          _p(beta), eps, _p(out32), _p(out16), M, K, _stream()), "eend_linear_res16_ln_f16")


def attnout_ffn_fused_res16(a16, wo, bo, res16, g1, be1, eps1, w1, b1, w2, b2, g2, be2, eps2, out32, out16):
    """attnout_ffn_fused with the out-projection's residual read from the f16 stream; out32 may be None."""
    L = _lib.load()
    _chk(a16, F16, "a16"); _chk(wo, F16, "wo"); _chk(w1, F16, "w1"); _chk(w2, F16, "w2"); _chk(res16, F16, "res16")
    for n, t in (("bo", bo), ("g1", g1), ("be1", be1), ("b1", b1), ("b2", b2), ("g2", g2), ("be2", be2), ("out32", out32)):
        _chk(t, F32, n)
    _chk(out16, F16, "out16")
    M, K = a16.shape
    Fh = w1.shape[0]
    if K != 256 or wo.shape != (256, 256) or w1.shape[1] != 256 or w2.shape != (256, Fh):
        raise _lib.EendHipError("attnout_ffn_fused_res16: expected d_model 256")
    _lib.check(L.eend_attnout_ffn_fused_res16_f16(_p(a16), a16.stride(0), _p(wo), _p(bo), _p(res16), _p(g1), _p(be1), eps1, _p(w1),
                                                  _p(b1), _p(w2), _p(b2), _p(g2), _p(be2), eps2, _p(out32), _p(out16), M, Fh,
                                                  _stream()), "eend_attnout_ffn_fused_res16_f16")


def attnout_ffn_fused(a16, wo, bo, res, g1, be1, eps1, w1, b1, w2, b2, g2, be2, eps2, out32, out16, out16lo=None, wo_lo=None):
    """x = LN1(a16 @ wo.T + bo + res); out = LN2(relu(x @ w1.T + b1) @ w2.T + b2 + x): the attention
    out-projection, both residual adds, both LayerNorms and the FFN of a post-LN layer in one launch."""
    L = _lib.load()
    _chk(a16, F16, "a16"); _chk(wo, F16, "wo"); _chk(w1, F16, "w1"); _chk(w2, F16, "w2")
    for n, t in (("bo", bo), ("res", res), ("g1", g1), ("be1", be1), ("b1", b1), ("b2", b2), ("g2", g2), ("be2", be2), ("out32", out32)):
        _chk(t, F32, n)
    _chk(out16, F16, "out16"); _chk(out16lo, F16, "out16lo"); _chk(wo_lo, F16, "wo_lo")
    M, K = a16.shape
    Fh = w1.shape[0]
    if K != 256 or wo.shape != (256, 256) or w1.shape[1] != 256 or w2.shape != (256, Fh) or (wo_lo is not None and wo_lo.shape != (256, 256)):
        raise _lib.EendHipError("attnout_ffn_fused: expected d_model 256")
    _lib.check(L.eend_attnout_ffn_fused_f16(_p(a16), a16.stride(0), _p(wo), _p(bo), _p(res), _p(g1), _p(be1), eps1, _p(w1), _p(b1),
                                            _p(w2), _p(b2), _p(g2), _p(be2), eps2, _p(out32), _p(out16), _p(out16lo), _p(wo_lo), M, Fh, _stream()),
               "eend_attnout_ffn_fused_f16")


def ffn_stream_pack(wo, w1, w2):
    """Pack Wo (or None), W1 [F][256], W2 [256][F] into the MFMA-fragment stream of the stream kernels (once per
    parameter version).  With wo the stream serves attnout_ffn_stream, without it ffn_stream."""
    L = _lib.load()
    _chk(w1, F16, "w1"); _chk(w2, F16, "w2")
    Fh = w1.shape[0]
    if w1.shape[1] != 256 or w2.shape != (256, Fh) or Fh % 64 or Fh < 64 or not w1.is_contiguous() or not w2.is_contiguous():
        raise _lib.EendHipError("ffn_stream_pack: expected contiguous W1 [F][256], W2 [256][F], F a multiple of 64")
    if wo is not None:
        _chk(wo, F16, "wo")
        if wo.shape != (256, 256) or not wo.is_contiguous():
            raise _lib.EendHipError("ffn_stream_pack: expected contiguous Wo [256][256]")
    n = L.eend_ffn_stream_elems(Fh, 1 if wo is not None else 0)
    out = torch.empty(n, dtype=F16, device=w1.device)
    _lib.check(L.eend_ffn_stream_pack_f16(_p(wo), _p(w1), _p(w2), _p(out), Fh, _stream()), "eend_ffn_stream_pack_f16")
    return out


def ffn_stream_pack_lo(wo, wo_lo, w1, w2):
    """ffn_stream_pack with the out-projection weight as an f16 hi / lo pair: the stream of attnout_ffn_stream_lo."""
    L = _lib.load()
    for n, t in (("wo", wo), ("wo_lo", wo_lo), ("w1", w1), ("w2", w2)):
        _chk(t, F16, n)
    Fh = w1.shape[0]
    if (w1.shape[1] != 256 or w2.shape != (256, Fh) or Fh % 64 or Fh < 64 or wo.shape != (256, 256) or wo_lo.shape != (256, 256)
            or not all(t.is_contiguous() for t in (wo, wo_lo, w1, w2))):
        raise _lib.EendHipError("ffn_stream_pack_lo: expected contiguous Wo / Wo_lo [256][256], W1 [F][256], W2 [256][F], F a multiple of 64")
    out = torch.empty(L.eend_ffn_stream_elems(Fh, 2), dtype=F16, device=w1.device)
    _lib.check(L.eend_ffn_stream_pack_lo_f16(_p(wo), _p(wo_lo), _p(w1), _p(w2), _p(out), Fh, _stream()), "eend_ffn_stream_pack_lo_f16")
    return out


def attnout_ffn_stream_lo(a16, wstream, bo, res, g1, be1, eps1, b1, b2, g2, be2, eps2, out32, out16, out16lo):
    """attnout_ffn_fused(..., out16lo, wo_lo) on a packed weight stream (ffn_stream_pack_lo): f32 residual rows in, f32 + f16 hi / lo out."""
    L = _lib.load()
    _chk(a16, F16, "a16"); _chk(wstream, F16, "wstream"); _chk(out16, F16, "out16"); _chk(out16lo, F16, "out16lo")
    for n, t in (("bo", bo), ("res", res), ("g1", g1), ("be1", be1), ("b1", b1), ("b2", b2), ("g2", g2), ("be2", be2), ("out32", out32)):
        _chk(t, F32, n)
    M, K = a16.shape
    Fh = b1.shape[0]
    if K != 256 or wstream.numel() != L.eend_ffn_stream_elems(Fh, 2) or res is None:
        raise _lib.EendHipError("attnout_ffn_stream_lo: expected d_model 256 and a stream packed with Wo / Wo_lo for this F")
    _lib.check(L.eend_attnout_ffn_stream_lo_f16(_p(a16), a16.stride(0), _p(wstream), _p(bo), _p(res), _p(g1), _p(be1), eps1, _p(b1), _p(b2),
                                                _p(g2), _p(be2), eps2, _p(out32), _p(out16), _p(out16lo), M, Fh, _stream()),
               "eend_attnout_ffn_stream_lo_f16")


def ffn_stream_max_rows(lda=256):
    """Rows one launch of the packed-stream layer-tail kernels takes; larger M is served in several launches inside the C ABI."""
    return int(_lib.load().eend_ffn_stream_max_rows(int(lda)))


def debug_ffn_stream_set(tile_fragments=0, max_rows_per_launch=0):
    """Test hook: force the tile size (2 / 3 fragments) / cap the rows per launch of the packed-stream layer-tail kernels (0 = default)."""
    _lib.check(_lib.load().eend_debug_ffn_stream_set(int(tile_fragments), int(max_rows_per_launch)), "eend_debug_ffn_stream_set")


def stream_ok(Fh):
    """Whether the packed-stream kernels take this hidden width."""
    return Fh % 64 == 0 and 64 <= Fh <= 2048


def attnout_ffn_stream(a16, wstream, bo, res, res16, g1, be1, eps1, b1, b2, g2, be2, eps2, out32, out16):
    """attnout_ffn_fused[_res16] on a packed weight stream (ffn_stream_pack(wo, w1, w2)); exactly one of res (f32) / res16."""
    L = _lib.load()
    _chk(a16, F16, "a16"); _chk(wstream, F16, "wstream"); _chk(res, F32, "res"); _chk(res16, F16, "res16")
    for n, t in (("bo", bo), ("g1", g1), ("be1", be1), ("b1", b1), ("b2", b2), ("g2", g2), ("be2", be2), ("out32", out32)):
        _chk(t, F32, n)
    _chk(out16, F16, "out16")
    M, K = a16.shape
    Fh = b1.shape[0]
    if K != 256 or wstream.numel() != L.eend_ffn_stream_elems(Fh, 1):
        raise _lib.EendHipError("attnout_ffn_stream: expected d_model 256 and a stream packed with Wo for this F")
    _lib.check(L.eend_attnout_ffn_stream_f16(_p(a16), a16.stride(0), _p(wstream), _p(bo), _p(res), _p(res16), _p(g1), _p(be1), eps1,
                                             _p(b1), _p(b2), _p(g2), _p(be2), eps2, _p(out32), _p(out16), M, Fh, _stream()),
               "eend_attnout_ffn_stream_f16")


def ffn_stream(x16, wstream, b1, b2, res, gamma, beta, out32, out16, act=ACT_RELU, alpha=1.0, eps=1e-5,
               residual_unnormalised=False):
    """ffn_fused on a packed weight stream (ffn_stream_pack(None, w1, w2))."""
    L = _lib.load()
    _chk(x16, F16, "x16"); _chk(wstream, F16, "wstream"); _chk(b1, F32, "b1"); _chk(b2, F32, "b2")
    _chk(res, F32, "res"); _chk(gamma, F32, "gamma"); _chk(beta, F32, "beta"); _chk(out32, F32, "out32"); _chk(out16, F16, "out16")
    M, K = x16.shape
    Fh = b1.shape[0]
    if K != 256 or wstream.numel() != L.eend_ffn_stream_elems(Fh, 0):
        raise _lib.EendHipError("ffn_stream: expected d_model 256 and a stream packed without Wo for this F")
    _lib.check(L.eend_ffn_stream_f16(_p(x16), x16.stride(0), _p(wstream), _p(b1), _p(b2), _p(res), float(alpha),
                                     _p(gamma), _p(beta), eps, _p(out32), _p(out16), M, Fh, act,
                                     1 if residual_unnormalised else 0, _stream()), "eend_ffn_stream_f16")


def ffn_fused(x16, w1, b1, w2, b2, res, gamma, beta, out32, out16, act=ACT_RELU, alpha=1.0, eps=1e-5,
              residual_unnormalised=False):
    """out = LN((act(x16 @ w1.T + b1) @ w2.T + b2) * alpha + res); hidden activations stay on chip."""
    L = _lib.load()
    _chk(x16, F16, "x16"); _chk(w1, F16, "w1"); _chk(w2, F16, "w2"); _chk(b1, F32, "b1"); _chk(b2, F32, "b2")
    _chk(res, F32, "res"); _chk(gamma, F32, "gamma"); _chk(beta, F32, "beta"); _chk(out32, F32, "out32"); _chk(out16, F16, "out16")
    M, K = x16.shape
    Fh = w1.shape[0]
    if K != 256 or w1.shape[1] != 256 or w2.shape != (256, Fh):
        raise _lib.EendHipError("ffn_fused: expected d_model 256")
    _lib.check(L.eend_ffn_fused_f16(_p(x16), x16.stride(0), _p(w1), _p(b1), _p(w2), _p(b2), _p(res), float(alpha),
                                    _p(gamma), _p(beta), eps, _p(out32), _p(out16), M, Fh, act,
                                    1 if residual_unnormalised else 0, _stream()), "eend_ffn_fused_f16")
