"""Test helper (not a test module): a float64 reference of the LS-EEND retention operator as the kernels implement it, and input
constructions that turn a chunk, mask or scale error into an error far above the bar of the GPU test.

Operator (LS-EEND/nnet/modules/retention.py:146-194, 222-224, decay 1; i = index of frame t inside its chunk of L frames):
    raw_t       = sum_{s <= t} (q_t . k_s) v_s                           all earlier frames, earlier chunks through the 64 x 64 state
    inner_raw_t = sum_{s <= t, same chunk} |q_t . k_s| / sqrt(i + 1)     inner_scale = max(inner_raw, 1)
    cross_raw_c = max_dv sum_dk |sum_{s in chunks < c} k_s (x) v_s| / sqrt(L)        cross_scale = max(cross_raw, 1)
    all_scale   = max(inner_scale, cross_scale) = max(inner_raw, cross_raw, 1)       (detached: no gradient)
    out_t  = raw_t / (sqrt(i + 1) all_scale);   rhat = LN_head(out), eps 1e-6, no affine;   ctx = swish(g) rhat
    c_t    = 1 / (sqrt(i + 1) all_scale) = d out_t / d raw_t;   rc = rstd c_t   (what eend_retention_chunk_train_f16 saves)
Away from the eps floor the LayerNorm divides all_scale out again (rhat and rc = 1 / std(raw) do not depend on it): only rows whose
var_head(out) is near or under 1e-6 see the scales, which is why the regime inputs below are built at that floor.

Constructions (every value a small integer times a power of two: exact in f16 and bf16):
  * impulse: K is zero except on the probe frames -- first and last frame of every chunk and the frames on either side of every
    16-frame edge counted from the start of the recording and from the start of each chunk (so every 16 / 32 / 64 / 128 tile edge of
    either kind) -- probe number r carrying the one-hot key feature r mod 64.  Q_t is 1 on the features of the three probes at or before
    t, of the two after it and of the first probe of the previous chunk, V the stair values of attn_edge_ref (rows >= 0.5 apart in
    most features), so every row is the sum of a few V rows: admitting or losing ONE probe (diagonal <= vs <, chunk start / end off by one, a state that includes its own chunk or
    lags one chunk behind) moves the normalised row by O(0.1 .. 1).  The scores are 0 / 1 and every sum is a multiple of 0.5 under
    2^11: P = f16(S), the f32 accumulators and the hi / lo state pairs hold them exactly, so the only roundings are the f32
    LayerNorm / gate arithmetic (~2^-20) and the f16 store of the result (2^-11 |x|).  IMPULSE_BAR = 2^-9 max(1, |want|) is four
    times that store rounding.  Backward: o~ is the kernel's own bf16 tensor, v and k are exact, so A = o~ . v is exact in f32 and
    is rounded to bf16 once (unit roundoff 2^-8) before A k / A^T q, the result once more: |err| <= 2^-7 sum |terms|; the bar is
    2^-6 sum |terms| elementwise (bwd_core(..., bound=True) returns the sums of |terms|).
  * regimes: q, k, v = integers in [-8, 8] / 8 times 2^e.  `clamped` (inner_raw < 1 and cross_raw < 1: all_scale == 1), `inner`
    (inner_raw the largest), `cross` (cross_raw the largest from chunk 1 on), `mixed` (rows pass inner_raw = 1 inside every chunk,
    cross_raw passes 1 between chunk 1 and chunk 2).  The V exponents put var_head(out) at or under the 1e-6 floor;
    branch_shares() and floor_share() report what share of the rows sits where, and the tests assert them.
  * poison: frames at or beyond T_valid hold +-1000 (products up to 6.4e7: finite in f32, saturating but finite in f16).
"""
import math
from collections import namedtuple

import torch

from tests.attn_edge_ref import POISON, heads_to_rows, poison_rows, rows_to_heads, stair_values  # noqa: F401  (re-exported)

GN_EPS = 1e-6
F64 = torch.float64

# ---- bars: the contract between tests/test_ret_edges_ref.py (CPU mutation table) and tests/test_ret_edges.py (GPU)
GAP = 4.0                     # every mutation must move the asserted quantity past GAP x the bar of the GPU test
IMPULSE_BAR = 2.0 ** -9       # |got - want| <= IMPULSE_BAR * max(1, |want|): 4 x the f16 store rounding (see above), no stray allowance
IMPULSE_BWD = 2.0 ** -6       # |got - want| <= IMPULSE_BWD * sum |terms| elementwise: 2 x the two bf16 roundings of 2^-8 (measured: 7.6e-3)
IMPULSE_RC = 5e-7             # relative, impulse inputs: f32 arithmetic on exact operands (about ten roundings of 2^-24: 6e-7); worst
                              # measured on MI355X 2.4e-7, bar = 2 x that, one digit
FWD_ATOL, FWD_RTOL, FWD_STRAY, FWD_CAP = 2e-2, 1e-2, 1e-5, 5.0        # the project's forward bar (test_hip_ret_stream._close)
BWD_L2, BWD_WORST = 6e-3, 3e-2                                         # the project's retention-backward bars (test_train_step_ls)
# measured on MI355X against this reference (tests/test_ret_edges.py prints every figure), bar = 2 x the worst, rounded up to one digit:
RC_BAR = 5e-7                 # |rc - want| / want per (row, head), regime inputs at the eps floor: worst measured 2.2e-7 (f32 arithmetic;
                              # the scores of these inputs are short enough for P = f16(S) to be nearly exact)
OT_BAR = 8e-3                 # max |o~ - want| / max |want|, non-zero rhat: worst measured 3.7e-3 (one bf16 store, unit roundoff 2^-8)
DG_BAR = 8e-3                 # max |d_g - want| / max |want|: worst measured 3.7e-3 (likewise)


Core = namedtuple("Core", "out inner_scale cross_scale all_scale inner_raw cross_raw")


def swish(x):
    return x * torch.sigmoid(x)


def dswish(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def pad_chunks(x, L):
    """(N, H, T, 64) zero-padded along T to a multiple of L (what a partial last chunk sees)"""
    T = x.shape[2]
    return torch.nn.functional.pad(x, (0, 0, 0, (-T) % L))


def ref_core(q, k, v, L, *, mask=None, kv_range=None, prefix_shift=0, cscale_shift=0, all_scale_fn=None, state_in=None):
    """q, k, v (N, H, T, 64), T a multiple of L -> Core(out (N, H, T, 64), inner_scale (N, H, T), cross_scale (N, H, nc),
    all_scale (N, H, T), and the two raw sums).  The scales are detached as in the reference.  state_in (N, H, 64, 64): the chunk
    state carried in (sum of k (x) v over earlier frames).  Mutation hooks (tests/test_ret_edges_ref.py only): mask (L, L) bool instead
    of tril; kv_range (lo, hi): local frames that enter a chunk's state contribution; prefix_shift +1: the state of chunk c includes
    chunk c, -1: it lags one chunk; cscale_shift +-1: chunk c uses the cross scale of chunk c +- 1; all_scale_fn(inner_raw,
    cross_raw) instead of max(inner_raw, cross_raw, 1)."""
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    N, H, T, D = q.shape
    assert T % L == 0
    nc = T // L
    rs = torch.sqrt(torch.arange(L, dtype=F64) + 1.0)
    m = torch.tril(torch.ones(L, L, dtype=F64)) if mask is None else mask.to(F64)
    qc, kc, vc = (x.reshape(N, H, nc, L, D) for x in (q, k, v))
    S = (qc @ kc.transpose(-1, -2)) * m
    inner_raw = S.detach().abs().sum(-1) / rs                                    # (N, H, nc, L)
    lo, hi = kv_range or (0, L)
    kv = kc[..., lo:hi, :].transpose(-1, -2) @ vc[..., lo:hi, :]                 # (N, H, nc, 64, 64)
    incl = torch.cumsum(kv, 2)
    z = torch.zeros_like(kv[:, :, :1])
    if prefix_shift == 0:
        P = incl - kv
    elif prefix_shift > 0:
        P = incl
    else:
        P = torch.cat([z, z, incl[:, :, :-2]], 2)[:, :, :nc]
    if state_in is not None:
        P = P + state_in.to(F64)[:, :, None]
    cross_raw = P.detach().abs().sum(-2).amax(-1) / math.sqrt(L)                 # (N, H, nc)
    if cscale_shift:
        idx = (torch.arange(nc) + cscale_shift).clamp(0, nc - 1)
        cross_raw = cross_raw[:, :, idx]
    cr = cross_raw[..., None].expand_as(inner_raw)
    if all_scale_fn is None:
        all_scale = torch.maximum(torch.maximum(inner_raw, cr), torch.ones_like(cr))
    else:
        all_scale = all_scale_fn(inner_raw, cr)
    out = (S @ vc + qc @ P) / (rs[:, None] * all_scale[..., None])
    return Core(out.reshape(N, H, T, D), inner_raw.clamp(min=1).reshape(N, H, T), cross_raw.clamp(min=1),
                all_scale.reshape(N, H, T), inner_raw.reshape(N, H, T), cross_raw)


Module = namedtuple("Module", "rhat rstd rc ctx core")


def ref_module(q, k, v, g, L, eps=GN_EPS, **kw):
    """+ per-head LayerNorm and gate; g (N, H, T, 64).  rc = rstd / (sqrt(i + 1) all_scale) (N, H, T)."""
    core = ref_core(q, k, v, L, **kw)
    out = core.out
    mu = out.mean(-1, keepdim=True)
    var = ((out - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    rhat = (out - mu) * rstd
    i = torch.arange(out.shape[2]) % L
    rc = rstd.squeeze(-1) / (torch.sqrt(i.to(F64) + 1.0) * core.all_scale)
    return Module(rhat, rstd.squeeze(-1), rc, swish(g.to(F64)) * rhat, core)


def gate_gn_bwd(dctx, g, rhat, rc, *, drop_rhat_term=False, dg_swish=False):
    """closed form of the gate + per-head LayerNorm backward from the operands the kernel reads: dctx, g, rhat (N, H, T, 64),
    rc (N, H, T) -> (o~ = c_t d out_t, d_g).  Mutation hooks: drop the rhat term; swish instead of swish' in d_g."""
    dctx, g, rhat, rc = dctx.to(F64), g.to(F64), rhat.to(F64), rc.to(F64)
    drh = dctx * swish(g)
    dr = drh - drh.mean(-1, keepdim=True)
    if not drop_rhat_term:
        dr = dr - rhat * (drh * rhat).mean(-1, keepdim=True)
    dg = dctx * rhat * (swish(g) if dg_swish else dswish(g))
    return rc[..., None] * dr, dg


def causal(T, strict=False):
    return torch.tril(torch.ones(T, T, dtype=torch.bool), -1 if strict else 0)


def chunk_shifted(T, L, shift):
    """the (query t, key s) visibility when a cross-chunk state is off by one chunk: shift +1 = the prefix state of chunk c (dq) or
    the suffix state R_c (dk, dv) also includes chunk c itself; shift -1 = it misses the neighbouring chunk"""
    c = torch.arange(T) // L
    if shift > 0:
        return causal(T) | (c[:, None] == c[None, :])
    return causal(T) & ~(c[:, None] == c[None, :] + 1)


def bwd_core(q, k, v, ot, *, mask_q=None, mask_kv=None, bound=False):
    """dq_t = sum_{s <= t} (o~_t . v_s) k_s,  dk_s = sum_{t >= s} (o~_t . v_s) q_t,  dv_s = sum_{t >= s} (q_t . k_s) o~_t in float64
    (q, k, v, ot (N, H, T, 64)).  mask_q / mask_kv (T, T) bool [t, s]: the visibility of the dq / of the dk and dv sums (mutations).
    bound: also the sums of |terms| (dq, dk, dv), the scale of the impulse bar."""
    q, k, v, ot = (x.to(F64) for x in (q, k, v, ot))
    T = q.shape[2]
    mq = (causal(T) if mask_q is None else mask_q).to(F64)
    mk = (causal(T) if mask_kv is None else mask_kv).to(F64)
    A = ot @ v.transpose(-1, -2)
    S = q @ k.transpose(-1, -2)
    res = ((A * mq) @ k, (A * mk).transpose(-1, -2) @ q, (S * mk).transpose(-1, -2) @ ot)
    if not bound:
        return res
    Aa, Sa = A.abs(), S.abs()
    return res, ((Aa * mq) @ k.abs(), (Aa * mk).transpose(-1, -2) @ q.abs(), (Sa * mk).transpose(-1, -2) @ ot.abs())


def ref_bwd(q, k, v, g, dctx, L, Tv):
    """float64 autograd of sum(ctx * dctx) over the first Tv frames, through the gate and the LayerNorm, scales detached.
    q, k, v, g, dctx (N, H, T, 64).  Returns dict(dq, dk, dv, dg, ot): ot the closed-form o~ (gate_gn_bwd of the float64 rhat / rc),
    so a failure can be pinned on stage 1 (gate / LayerNorm) or stage 2 (retention products)."""
    q, k, v, g = (x[:, :, :Tv].detach().to(F64).requires_grad_(True) for x in (q, k, v, g))
    m = ref_module(q, k, v, g, L)
    (m.ctx * dctx[:, :, :Tv].to(F64)).sum().backward()
    ot, _ = gate_gn_bwd(dctx[:, :, :Tv], g.detach(), m.rhat.detach(), m.rc.detach())
    return dict(dq=q.grad, dk=k.grad, dv=v.grad, dg=g.grad, ot=ot)


# ---- metrics
def row_err(got, want):
    """max |got - want| over a row's 64 features / RMS of that row of want; (..., T, 64) -> (..., T)"""
    got, want = got.double(), want.double()
    rms = want.pow(2).mean(-1).sqrt().clamp_min(1e-6)
    return (got - want).abs().amax(-1) / rms


def impulse_err(got, want):
    """max |got - want| / max(1, |want|): compare with IMPULSE_BAR"""
    got, want = got.double(), want.double()
    return ((got - want).abs() / want.abs().clamp_min(1.0)).max().item()


def bound_err(got, want, bound):
    """max |got - want| / sum |terms|: compare with IMPULSE_BWD"""
    return ((got.double() - want.double()).abs() / bound.double().clamp_min(1e-30)).max().item()


def fwd_excess(got, want):
    """the project's forward bar as one number: (share of elements over atol + rtol |want|, worst error / tolerance); passes when
    share <= FWD_STRAY and worst <= FWD_CAP"""
    err = (got.double() - want.double()).abs()
    tol = FWD_ATOL + FWD_RTOL * want.double().abs()
    return (err > tol).double().mean().item(), (err / tol).max().item()


def fwd_ok(got, want):
    share, worst = fwd_excess(got, want)
    return share <= FWD_STRAY and worst <= FWD_CAP


def rel_l2(got, want):
    return ((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-300)).item()


def rel_worst(got, want):
    return ((got.double() - want.double()).abs().max() / want.double().abs().max().clamp_min(1e-300)).item()


def rel_rows(got, want):
    """max |got - want| / |want| (rc: one positive number per row and head)"""
    return ((got.double() - want.double()).abs() / want.double().abs()).max().item()


def exact16(x):
    """x survives a round trip through f16 and through bf16"""
    return bool(torch.equal(x.to(torch.float16).double(), x.double()) and torch.equal(x.to(torch.bfloat16).double(), x.double()))


# ---- impulse construction
def probe_frames(T, L):
    s = set()
    for f0 in range(0, T, L):
        f1 = min(f0 + L, T)
        s.update((f0, f1 - 1))
        for e in range(f0, f1, 16):
            s.update((e - 1, e))
    for e in range(0, T, 16):
        s.update((e - 1, e))
    return sorted(t for t in s if 0 <= t < T)


def impulse_qkv(nseq, T, L, H=4):
    """float64 Q, K, V (nseq, H, T, 64), G and dctx (same shape, multiples of 1/4 and 1/8) and the probe frames"""
    pr = probe_frames(T, L)
    pt = torch.tensor(pr)
    K = torch.zeros(nseq, H, T, 64, dtype=F64)
    K[:, :, pt, torch.arange(len(pr)) % 64] = 1.0
    rank = torch.searchsorted(pt, torch.arange(T), right=True) - 1               # last probe at or before t (frame 0 is a probe)
    Q = torch.zeros_like(K)
    for d in (-2, -1, 0, 1, 2):
        r = rank + d
        ok = (r >= 0) & (r < len(pr))
        Q[:, :, torch.arange(T)[ok], r[ok] % 64] = 1.0
    t = torch.arange(T)
    prev0 = torch.searchsorted(pt, (t // L - 1) * L)                             # ... and of the first probe of the previous chunk
    ok = t >= L
    Q[:, :, t[ok], prev0[ok] % 64] = 1.0
    V = torch.stack([stair_values(T, 64, 7 * h) for h in range(H)])[None].expand(nseq, H, T, 64).clone()
    for n in range(nseq):                                                        # sequences differ (a wrong sequence offset shows)
        V[n] = torch.roll(V[n], 3 * n, -1)
    G = torch.stack([stair_values(T, 64, 5 * h + 1) for h in range(H)])[None].expand(nseq, H, T, 64).clone() / 4
    dctx = torch.stack([stair_values(T, 64, 3 * h + 2) for h in range(H)])[None].expand(nseq, H, T, 64).clone() / 8
    return Q, K, V, G, dctx, pr


# ---- scale regimes
REGIMES = ("clamped", "inner", "cross", "mixed")


def _grid(shape, gen, e):
    return torch.randint(-8, 9, shape, generator=gen).to(F64) / 8 * 2.0 ** e


def regime_qkv(regime, nseq, T, L, seed=0, H=4, floor=True):
    """float64 q, k, v, g, dctx (nseq, H, T, 64) of one scale regime (module docstring).  E |q . k| = 2.4 x 2^(eq + ek), so
    inner_raw = 2.4 x 2^(eq + ek) sqrt(i + 1); cross_raw = 22 x 2^(ek + ev) sqrt(chunks before c)."""
    gen = torch.Generator().manual_seed(1000 * seed + T + L)
    shape = (nseq, H, T, 64)
    c = (torch.arange(T) // L)[None, None, :, None]
    if regime == "clamped":          # inner_raw <= 2.4 x 2^-7 sqrt(512) = 0.43, cross_raw <= 22 x 2^-8 x 4 = 0.35 up to 16 chunks
        eq, ek, ev = -3, -4, -4
    elif regime == "inner":          # inner_raw = 2.4 sqrt(i + 1); cross_raw = 22 x 2^ev sqrt(c) stays under it.  var_head(out) falls like
        eq, ek = 0, 0                # 4^ev t / (i + 1)^2: short chunks (i + 1 <= L small, t large) need a smaller V to reach the eps floor
        ev = -6 if L >= 64 or not floor else -10     # floor=False: the backward cases, which take rhat and rc as operands
    elif regime == "cross":          # inner_raw < 1; cross_raw = 88 sqrt(c) from chunk 1 on
        eq, ek, ev = -6, -1, 3
    elif regime == "mixed":          # inner_raw passes 1 near i = L / 3; chunk 0 has small V so that cross_raw(1) < 1 < cross_raw(2)
        eqk = -round(math.log2(2.4 * math.sqrt(L / 3.0)))
        ek, ev = 2, -6
        eq = eqk - ek
    else:
        raise ValueError(regime)
    q, k, v = _grid(shape, gen, eq), _grid(shape, gen, ek), _grid(shape, gen, ev)
    if regime == "mixed":
        v = torch.where(c == 0, v / 16, v)
    g = _grid(shape, gen, 1)
    dctx = _grid(shape, gen, -7)
    return q, k, v, g, dctx


# the (L, chunks) shapes of the forward cases and the regimes that hold >= 10 % of the rows in their branch (mixed: in each of the
# three) and >= 10 % of the rows at or under the eps floor there (asserted by tests/test_ret_edges_ref.py)
FWD_SHAPES = [(4, 16), (6, 21), (64, 1), (64, 3), (64, 16), (100, 2), (100, 4), (500, 1), (500, 3), (512, 2), (544, 2)]
REGIME_CASES = [("clamped", 4, 16), ("inner", 4, 16), ("cross", 4, 16), ("clamped", 6, 21), ("inner", 6, 21), ("cross", 6, 21), ("clamped", 64, 1), ("inner", 64, 1),
                ("clamped", 64, 3), ("inner", 64, 3), ("cross", 64, 3), ("mixed", 64, 3), ("clamped", 64, 16), ("cross", 64, 16),
                ("clamped", 100, 2), ("inner", 100, 2), ("cross", 100, 2), ("clamped", 100, 4), ("inner", 100, 4), ("cross", 100, 4),
                ("mixed", 100, 4), ("clamped", 500, 1), ("inner", 500, 1), ("clamped", 500, 3), ("inner", 500, 3), ("cross", 500, 3),
                ("mixed", 500, 3), ("clamped", 512, 2), ("inner", 512, 2), ("cross", 512, 2), ("clamped", 544, 2), ("inner", 544, 2),
                ("cross", 544, 2), ("clamped", 300, 2), ("inner", 300, 2), ("cross", 300, 2)]


def branch_shares(core):
    """share of the rows in each branch of all_scale = max(inner_raw, cross_raw, 1): dict(clamped, inner, cross)"""
    a = core.inner_raw
    L = a.shape[2] // core.cross_raw.shape[2]
    cr = core.cross_raw.repeat_interleave(L, 2)
    one = (a <= 1) & (cr <= 1)
    inner = ~one & (a >= cr)
    cross = ~one & (a < cr)
    return dict(clamped=one.double().mean().item(), inner=inner.double().mean().item(), cross=cross.double().mean().item())


def floor_share(core, eps=GN_EPS):
    """share of the rows with var_head(out) <= 4 eps (the LayerNorm's eps changes their normalised values by more than 10 %), and
    the share within a factor 4 of eps"""
    var = core.out.var(-1, unbiased=False)
    return (var <= 4 * eps).double().mean().item(), ((var <= 4 * eps) & (var >= eps / 4)).double().mean().item()


def poison_tail(x, T_valid, sign_shift=0):
    """frames >= T_valid of (N, H, T, 64) overwritten with +-POISON"""
    x = x.clone()
    n = x.shape[2] - T_valid
    if n > 0:
        x[:, :, T_valid:] = torch.roll(poison_rows(n, 64), sign_shift, -1)
    return x


# ---- 0 / 1 projection for eend_retention_stream_f16: the 256 columns of x hold ONE head's q | k | v | g features of a frame; head h
# reads them rotated by 16 h features (q and k by the same rotation, so q . k is unchanged), which makes the four heads' rows differ
def stream_w():
    """(W [1024][256], b [1024]) float64, 0 / 1 weights: feature d of head h of part p (q, k, v, g) = x[64 p + (d + 16 h) % 64]"""
    W = torch.zeros(1024, 256, dtype=F64)
    for part in range(4):
        for h in range(4):
            for d in range(64):
                W[part * 256 + h * 64 + d, part * 64 + (d + 16 * h) % 64] = 1.0
    return W, torch.zeros(1024, dtype=F64)


def stream_x(q, k, v, g):
    """(N, T, 64) each (one head's rows) -> x (N * T, 256)"""
    return torch.cat([q, k, v, g], -1).reshape(-1, 256)


def split_hi_lo(q):
    """q = hi + lo, both exact in f16, for the Xlo rows of eend_retention_stream_f16 (added on the query path): with u the smallest
    non-zero |q|, lo carries the odd multiples' last unit (q / u mod 2) u and hi the rest.  For the 0 / 1 impulse queries lo is q itself:
    a kernel that drops, mis-strides or mis-scales the lo rows loses or changes every score."""
    u = q[q != 0].abs().min()
    lo = torch.round(q / u).remainder(2) * u
    return q - lo, lo


def stream_heads(x, W, b, nseq, T):
    """float64 projection of x (nseq * T, 256) -> q, k, v, g (nseq, 4, T, 64): exact for 0 / 1 weights"""
    y = x.double() @ W.double().t() + b.double()
    return tuple(y[:, i * 256:(i + 1) * 256].reshape(nseq, T, 4, 64).transpose(1, 2) for i in range(4))
