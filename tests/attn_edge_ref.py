"""Test helper (not a test module): an exact float64 reference of the causal time-axis attention and input constructions that
turn a mask error of one key into an O(1) error of the output.

Mask of every attention entry (include/eend_hip.h): key j is visible to query i iff  j - i <= delay  and  j < kv_len; the
backward also drops the queries i >= q_len.

Constructions:
  * staircase: K[j] = (j >> 6, j & 63, 0, ...), Q = (64 s, s, 0, ...) with s a power of two, so the score of key j is s * j
    (exact in f16 / bf16 and fp32 for j < 4096) and adjacent keys differ by s in the log2 domain.  The softmax is one-hot on the
    last visible key: row i's output is V[min(i + delay, kv_len - 1)].  The reverse staircase (Q negated) puts every row on V[0].
  * stair values: V rows that differ from their neighbours by >= 0.5 in every feature but two, whose other two features tell rows
    32 and 1024 apart; every value a multiple of 0.5 in [-8, 7.5] (exact in f16 and bf16).
  * poison: rows a kernel must not read (keys at or beyond kv_len, cache rows beyond t, dO rows at or beyond q_len) hold finite
    values of about 1e3 whose keys would win the softmax: a leak is a gross error, never a near miss.
"""
import math

import torch

LN2 = math.log(2.0)
QSCALE_LOG2 = 0.125 * math.log2(math.e)     # fs_eend_amd.ops.QSCALE_LOG2: the q-row pre-scaling of the packed kernels
POISON = 1000.0                             # exact in f16 and bf16
STAIR_S = 32.0                              # score step per key (log2 domain) of the staircase on the ln2-scaled entries
STAIR_BAR = 1.0 / 32                        # staircase bar: the rounding of |V| <= 10 (2^-8 |V|); a mask error costs >= 0.5


def visible(Tq, Tk, delay, kv_len, q_len=None, device=None):
    """bool (Tq, Tk): the index predicate of the attention entries."""
    i = torch.arange(Tq, device=device)[:, None]
    j = torch.arange(Tk, device=device)[None, :]
    ok = ((j - i) <= delay) & (j < kv_len)
    if q_len is not None:
        ok = ok & (i < q_len)
    return ok


def ref_attn(q, k, v, delay, kv_len, scale, keep=None, drop_scale=1.0, mask=None):
    """q, k, v (n, H, Tq / Tk, 64) -- the operands the kernel consumes, any float dtype -- in float64.
    Returns (o (n, H, Tq, 64), lse2 (n, H, Tq)): softmax(mask(q k^T * scale)) v, and the log2-domain log-sum-exp of the masked
    scores (un-dropped, as the kernels save it).  keep (broadcastable to (n, H, Tq, Tk), bool): dropout keep mask of the
    probabilities, kept ones scaled by drop_scale.  mask: an explicit (Tq, Tk) visibility (mutation checks) instead of the
    predicate."""
    q, k, v = q.double(), k.double(), v.double()
    ok = visible(q.shape[-2], k.shape[-2], delay, kv_len, device=q.device) if mask is None else mask
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~ok, float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    if keep is not None:
        p = p * keep.double() * drop_scale
    return p @ v, lse / LN2


def ref_attn_bwd(q, k, v, dO, delay, kv_len, q_len, scale, keep=None, drop_scale=1.0, mask=None):
    """float64 autograd of ref_attn with the backward's q_len cut (queries i >= q_len contribute nothing: their dO is ignored).
    dO (n, H, Tq, 64).  Returns (dq, dk, dv)."""
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    o, _ = ref_attn(q, k, v, delay, kv_len, scale, keep, drop_scale, mask)
    w = dO.double().clone()
    w[..., q_len:, :] = 0
    (o * w).sum().backward()
    return q.grad, k.grad, v.grad


def row_err(got, want):
    """per-row error: max |got - want| over a row's 64 features / RMS of that row of want; (..., T, 64) -> (..., T)"""
    got, want = got.double(), want.double()
    rms = want.pow(2).mean(-1).sqrt().clamp_min(1e-6)
    return (got - want).abs().amax(-1) / rms


def last_visible(Tq, delay, kv_len):
    """index of the last key row i sees: the staircase answer"""
    i = torch.arange(Tq)
    return torch.clamp(i + delay, max=kv_len - 1).clamp(min=0)


def stair_values(T, ncols=64, shift=0):
    """(T, ncols) float: features 0 / 1 = (j >> 5) & 31 and (j >> 10) & 31, feature d >= 2 = (j (2d' + 1) + 5 d') mod 32 with
    d' = d + shift; every value halved and shifted to [-8, 7.5]"""
    j = torch.arange(T)[:, None]
    d = torch.arange(ncols)[None, :] + shift
    v = (j * (2 * d + 1) + 5 * d) % 32
    v[:, 0] = (torch.arange(T) >> 5) & 31
    v[:, 1] = (torch.arange(T) >> 10) & 31
    return v.double() / 2 - 8


def poison_rows(n, ncols, gen=None):
    """(n, ncols) of +-POISON in a fixed sign pattern"""
    sgn = torch.where((torch.arange(n)[:, None] + torch.arange(ncols)[None, :]) % 3 == 0, -1.0, 1.0)
    return sgn.double() * POISON


def stair_qkv(nseq, H, Tp, kv_len, s=STAIR_S, reverse=False, poison=True):
    """float64 Q, K, V (nseq, H, Tp, 64) of the (reverse) staircase for the entries that take Q / K / V head rows; with `poison`
    the key and value rows at or beyond kv_len are poison whose keys would win the softmax."""
    sign = -1.0 if reverse else 1.0
    j = torch.arange(Tp)
    K = torch.zeros(nseq, H, Tp, 64, dtype=torch.float64)
    K[..., 0] = (j >> 6).double()
    K[..., 1] = (j & 63).double()
    Q = torch.zeros_like(K)
    Q[..., 0] = sign * 64 * s
    Q[..., 1] = sign * s
    V = torch.stack([stair_values(Tp, 64, 7 * h) for h in range(H)])[None].expand(nseq, H, Tp, 64).clone()
    if poison and kv_len < Tp:
        K[..., kv_len:, 0:2] = sign * POISON
        V[..., kv_len:, :] = poison_rows(Tp - kv_len, 64)
    return Q, K, V


def stair_x(nseq, Tp, kv_len, reverse=False, poison=True):
    """f16-exact x (nseq * Tp, 256) of the staircase for the fused in-projection entries (stair_inproj gives the weights):
    column 0 = j >> 6, column 1 = j & 63, columns 2 .. 255 the stair values; rows at or beyond kv_len poison (columns 0 / 1
    signed so that their keys win)."""
    sign = -1.0 if reverse else 1.0
    j = torch.arange(Tp)
    x = torch.zeros(Tp, 256, dtype=torch.float64)
    x[:, 0] = (j >> 6).double()
    x[:, 1] = (j & 63).double()
    x[:, 2:] = stair_values(Tp, 254)
    if poison and kv_len < Tp:
        x[kv_len:, 0:2] = sign * POISON
        x[kv_len:, 2:] = poison_rows(Tp - kv_len, 254)
    return x.repeat(nseq, 1)


def stair_vcols(h):
    """x column of each of head h's 64 value features (stair_x / stair_inproj)"""
    return [2, 3] + [4 + (d - 2 + 62 * h) % 252 for d in range(2, 64)]


def stair_inproj(s=STAIR_S, reverse=False):
    """(W [768][256], b [768]) float64, 0 / 1 weights: q = bias (64 s, s) per head (the already pre-scaled q the packed kernels
    consume, scale ln 2), k = (x[0], x[1]) per head, v = the head's stair_vcols columns of x."""
    sign = -1.0 if reverse else 1.0
    W = torch.zeros(768, 256, dtype=torch.float64)
    b = torch.zeros(768, dtype=torch.float64)
    for h in range(4):
        b[h * 64 + 0] = sign * 64 * s
        b[h * 64 + 1] = sign * s
        W[256 + h * 64 + 0, 0] = 1
        W[256 + h * 64 + 1, 1] = 1
        for d, c in enumerate(stair_vcols(h)):
            W[512 + h * 64 + d, c] = 1
    return W, b


def inproj_heads(x, W, b, nseq, Tp):
    """float64 in-projection of x (nseq * Tp, 256) -> q, k, v (nseq, 4, Tp, 64)"""
    y = x.double() @ W.double().t() + b.double()
    return tuple(y[:, i * 256:(i + 1) * 256].reshape(nseq, Tp, 4, 64).transpose(1, 2) for i in range(3))


def inproj_heads_bf16(x, W, b, nseq, Tp, key_bias=True):
    """inproj_heads rounded to bf16 as the fused kernels round their projections before the attention (the packed inference
    kernels drop the key bias, which cancels in the softmax): the operands their attention phase consumes, in float64"""
    bk = b.double().clone()
    if not key_bias:
        bk[256:512] = 0
    return tuple(t.to(torch.bfloat16).double() for t in inproj_heads(x, W, bk, nseq, Tp))


def heads_to_rows(o):
    """(n, H, T, 64) -> (n, T, H * 64): the concatenated head rows the kernels write"""
    n, H, T, _ = o.shape
    return o.transpose(1, 2).reshape(n, T, H * 64)


def rows_to_heads(r, H=4):
    """(n, T, H * 64) -> (n, H, T, 64)"""
    n, T, _ = r.shape
    return r.reshape(n, T, H, 64).transpose(1, 2)


def drop_spec(p_drop, Tp, site=3):
    """(seed, thresh24, scale) of the attention dropout spec tests/test_train_kernels.py::_drop_spec builds"""
    from oracle import dropout_ref as DR
    d = DR.HashDropout(p_drop, 42, 7, Tp)
    return DR.site_seed(d.base, site), d.thresh24, d.scale


def drop_keep(seed, thresh24, nseq, H, Tp, Tq=None, Tk=None, device=None):
    """bool (nseq, H, Tq, Tk) keep mask of the attention probabilities: element ((seq*H + head)*Tp + query, key)"""
    from oracle import dropout_ref as DR
    Tq = Tp if Tq is None else Tq
    Tk = Tp if Tk is None else Tk
    a = ((torch.arange(nseq, device=device)[:, None, None] * H + torch.arange(H, device=device)[None, :, None]) * Tp
         + torch.arange(Tq, device=device)[None, None, :])
    return DR.keep_mask(a[..., None].to(torch.int64), torch.arange(Tk, device=device, dtype=torch.int64), seed, thresh24)
