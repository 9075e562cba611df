"""Constructions and exact references for the non-GEMM part of the training step (csrc/train_rows.hip, csrc/ls_train.hip,
csrc/optim.hip behind csrc/api_train.hip; no GPU needed).

Every kernel here is a persistent or split row loop that writes per-block partials into a workspace, followed by a fixed-order
reduction.  With the operands below every partial sum of every summation order is an integer (or a small multiple of 2^-3) below 2^24
and therefore exact in f32: a correct kernel gives the bits of the int64 / float64 restatements of this module whatever its grid, and
one row dropped, doubled, taken from beyond Tv or paired with the wrong tap changes them.  `assert_exact` checks that condition on the
INPUTS of a case; it says nothing about the kernel.

The grid functions restate the launchers' formulas (blocks, rows per block and pass, which rows share a block); the tables at the
bottom are the shapes tests/test_rowgrad_edges.py runs on the GPU, and tests/test_rowgrad_edges_ref.py shows on the CPU that the
one-step mistakes change the reference at those shapes."""
import torch

F16, BF16, F32, F64, I64 = torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int64
D = 256
VALS = (-2, -1, 1, 2)
LIMIT = 1 << 24


def ints(shape, seed, vals=VALS):
    """int64 tensor drawn from `vals` (non-zero by default: a lost row must show)"""
    g = torch.Generator().manual_seed(seed)
    v = torch.tensor(vals, dtype=I64)
    return v[torch.randint(0, len(vals), tuple(shape), generator=g)]


def as_t(t, dtype):
    """int64 / float64 -> f16 / bf16 / f32, asserting that nothing is rounded"""
    r = t.to(dtype)
    assert torch.equal(r.double(), t.double()), f"not exact in {dtype}"
    return r


def assert_exact(*terms, unit=1.0):
    """the exactness guard: every column sum of |term| over the rows (dim 0), in units of `unit` (a power of two, all terms multiples
    of it), stays below 2^24 -- so every partial sum in every order is exact in f32.  Returns the largest bound."""
    worst = 0
    for t in terms:
        t = t.double()
        assert torch.equal(torch.round(t / unit) * unit, t), "term is not a multiple of the unit"
        b = float((t.abs() / unit).reshape(t.shape[0], -1).sum(0).max()) if t.dim() > 1 else float((t.abs() / unit).sum())
        assert b < LIMIT, b
        worst = max(worst, b)
    return worst


# ------------------------------------------------------------------------------------------------ grids (the launchers' formulas)
def rows_grid(M):
    """ln_bwd / ln_bwd2 / resgrad_cast: blocks of four waves, one row per wave and pass -> (blocks, rows per block and pass, passes)"""
    nb = min((M + 3) // 4, 1024)
    return nb, 4, (M + 4 * nb - 1) // (4 * nb)


def rows_block_of(r, M):
    nb = rows_grid(M)[0]
    return (r // 4) % nb, r // (4 * nb)                       # (block, pass)


def slot_grid(frames):
    """slot_sum_kernel: at most 256 blocks of four frames per pass"""
    nb = min((frames + 3) // 4, 256)
    return nb, 4, (frames + 4 * nb - 1) // (4 * nb)


def bn_splits(BT):
    """bn_colstats / bn_bwd: (splits, rows per split); a split walks its rows sixteen at a time"""
    ns = min((BT + 255) // 256, 512)
    return ns, (BT + ns - 1) // ns


def bn16_blocks(nrows):
    """bn_colstats16 / bn_swish_bwd_stats: (blocks, rows per block); a block walks its rows four at a time"""
    nb = min((nrows + 31) // 32, 4096)
    return nb, (nrows + nb - 1) // nb


def conv_strips(nseq, Tp):
    return nseq * ((Tp + 63) // 64)


def sumsq_grid(n):
    """sumsq_partial_kernel: (blocks, float4 passes, scalar tail length); the tail n % 4 is block 0's"""
    n4 = n // 4
    nb = min(max((n4 + 255) // 256, 1), 1024)
    return nb, (n4 + 256 * nb - 1) // (256 * nb), n - 4 * n4


def frames_pad(t):
    return (t + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------ dropout (oracle/dropout_ref.py masks)
def keep(rows, ncols, seed, thresh24):
    """bool [len(rows)][ncols]: the mask of element (row, column); thresh24 == 0: everything kept"""
    from oracle import dropout_ref as DR
    if thresh24 == 0:
        return torch.ones(len(rows), ncols, dtype=torch.bool)
    return DR.keep_mask(rows.to(I64)[:, None], torch.arange(ncols)[None, :], seed, thresh24)


HALF = 1 << 23          # thresh24 of p = 0.5: scale 2


# ------------------------------------------------------------------------------------------------ LayerNorm backward family
def ln_operands(M, seed):
    """(g, xhat, rstd, gamma) float64 with  sum_j d_j = 256 a,  sum_j d_j x_j = 640 b  (d = g * gamma; a, b small integers per row), so that
    c1 = a, c2 = 2.5 b and ds = rstd * (e - 1.5 b x) hold exactly in f32: x in {-2,-1,1,2} (64 columns each, shuffled per row), e = +-1
    summing to zero inside each group of equal x, rstd in {0.5, 1, 2}, gamma = +-1.  ds is never zero (|e| = 1, 1.5 b x is a multiple of 1.5)."""
    gen = torch.Generator().manual_seed(seed)
    base = torch.tensor([-2, -1, 1, 2], dtype=I64).repeat_interleave(64)
    order = torch.rand(M, D, generator=gen).argsort(1)
    x = base[order]
    e_sorted = torch.tensor([1, -1], dtype=I64).repeat(128)[None, :].expand(M, D)          # +1 / -1 alternate inside every 64-group
    flip = (torch.randint(0, 2, (M, 4), generator=gen) * 2 - 1).repeat_interleave(64, 1)
    e = (e_sorted * flip).gather(1, order)
    a = torch.randint(-1, 3, (M, 1), generator=gen)
    b = torch.randint(-1, 3, (M, 1), generator=gen)
    gamma = torch.randint(0, 2, (D,), generator=gen) * 2 - 1
    d = a + b * x + e
    g = d * gamma                                              # gamma = +-1: g * gamma == d
    rstd = torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 3, (M,), generator=gen)]
    return g.double(), x.double(), rstd, gamma.double()


def ref_ln_ds(g, x, rstd, gamma):
    """float64 restatement of the LayerNorm input gradient (exact for ln_operands)"""
    d = g * gamma
    c1, c2 = d.mean(1, keepdim=True), (d * x).mean(1, keepdim=True)
    return rstd[:, None] * (d - c1 - x * c2)


def ref_ln(g, x, rstd, gamma, alpha16=1.0, seed=0, thresh24=0, w=None):
    """-> dict ds, ds16 (= alpha16 * dropout(ds)), dgamma, dbeta, dbias.   w: per-row multiplicity in the three column sums (mutations)"""
    M = g.shape[0]
    w = torch.ones(M, dtype=F64) if w is None else w.double()
    ds = ref_ln_ds(g, x, rstd, gamma)
    k = keep(torch.arange(M), D, seed, thresh24).double() * (2.0 if thresh24 else 1.0)
    ds16 = alpha16 * ds * k
    return dict(ds=ds, ds16=ds16, dgamma=(w[:, None] * g * x).sum(0), dbeta=(w[:, None] * g).sum(0), dbias=(w[:, None] * ds16).sum(0))


def ref_resgrad(g, alpha, seed=0, thresh24=0, w=None):
    M = g.shape[0]
    w = torch.ones(M, dtype=F64) if w is None else w.double()
    ds16 = alpha * g * keep(torch.arange(M), D, seed, thresh24).double() * (2.0 if thresh24 else 1.0)
    return dict(ds16=ds16, dbias=(w[:, None] * ds16).sum(0))


def row_weights(name, M, nb_rows):
    """per-row multiplicity of a row mutation of a persistent grid of nb_rows rows per pass (4 * blocks), or None where the shape gives
    the mistake nothing to act on"""
    w = torch.ones(M, dtype=I64)
    second = nb_rows if M > nb_rows else None                  # first row of the second grid pass
    if name == "drop_last_row":
        w[M - 1] = 0
    elif name == "double_last_row":
        w[M - 1] = 2
    elif name == "drop_first_row_of_second_pass":
        if second is None:
            return None
        w[second] = 0
    elif name == "double_first_row_of_second_pass":
        if second is None:
            return None
        w[second] = 2
    elif name == "no_second_pass":
        if second is None:
            return None
        w[second:] = 0
    else:
        raise KeyError(name)
    return w


ROW_MUTATIONS = ("drop_last_row", "double_last_row", "drop_first_row_of_second_pass", "double_first_row_of_second_pass", "no_second_pass")
ROW_M = (1, 3, 4, 5, 4095, 4096, 4097, 12290)


# ------------------------------------------------------------------------------------------------ convert fan-out backward
def ref_slot_sum(g0, B, C, Tp, w=None):
    """g0 int64 [(b*C + c)*Tp + t][256] -> gsum [B*Tp][256], dpc [C][256].  w: per-frame multiplicity (b*Tp + t) in dpc"""
    g4 = g0.view(B, C, Tp, D)
    w = torch.ones(B * Tp, dtype=I64) if w is None else w
    return g4.sum(1).reshape(B * Tp, D), (g4 * w.view(B, 1, Tp, 1)).sum((0, 2))


SLOT_CASES = [(1, 64, C) for C in range(1, 13)] + [(B, 64, C) for B in (16, 17, 33) for C in (1, 6, 12)]       # (B, Tp, C)


# ------------------------------------------------------------------------------------------------ FS BatchNorm (padded input through a pointer table)
def bn_rows(lens, T, bufs, which, pad_value, F):
    """the padded [B*T][F] int64 input: utterance b is bufs[which[b]][:lens[b]] followed by pad_value"""
    out = torch.full((len(lens), T, F), int(pad_value), dtype=I64)
    for b, (l, k) in enumerate(zip(lens, which)):
        out[b, :l] = bufs[k][:l]
    return out.view(-1, F)


def bn_balance(bufs, lens, T, which, pad_value, F):
    """adjust the buffers by +-1 in a few rows so that every column of the padded input sums to a multiple of n = B*T: the mean is then
    an integer, both statistics passes are exact, and var = float32(s2) / float32(n) in one rounding.  Returns the padded rows."""
    n = len(lens) * T
    for _ in range(8):
        rows = bn_rows(lens, T, bufs, which, pad_value, F)
        s = rows.sum(0)
        delta = s - n * torch.round(s.double() / n).to(I64)
        if not delta.any():
            return rows
        # one buffer row shared by `mult` utterances moves the sum by mult: use the rows of buffers used once where possible
        for k, buf in enumerate(bufs):
            mult = sum(1 for b, kk in enumerate(which) if kk == k and lens[b] > 0)
            if mult != 1:
                continue
            lmax = max(lens[b] for b, kk in enumerate(which) if kk == k)
            step = delta.clamp(-lmax, lmax)
            idx = torch.arange(lmax)[:, None]
            buf[:lmax] -= (idx < step.abs()[None, :]).to(I64) * step.sign()[None, :]
            delta = delta - step
    raise AssertionError("could not balance the column sums")


CHUNK = 16384                             # (the references walk large inputs in chunks of rows: memory)


def ref_bn_stats(rows, w=None):
    """-> (sum, mean, var biased, var unbiased) float64 per column.  w: per-row multiplicity"""
    w = torch.ones(rows.shape[0], dtype=I64) if w is None else w
    n = float(rows.shape[0])
    s = sum((w[i:i + CHUNK, None] * rows[i:i + CHUNK]).sum(0) for i in range(0, rows.shape[0], CHUNK)).double()
    mean = s / n
    m2 = sum((w[i:i + CHUNK, None].double() * (rows[i:i + CHUNK].double() - mean) ** 2).sum(0) for i in range(0, rows.shape[0], CHUNK))
    return s, mean, m2 / n, m2 / (n - 1)


def ref_bn_bwd(rows, dy, mean, rstd, w=None):
    """dgamma = sum dy (x - mean) rstd, dbeta = sum dy over the B*T rows (int64 in, exact)"""
    w = torch.ones(rows.shape[0], dtype=I64) if w is None else w
    dg, db = 0, 0
    for i in range(0, rows.shape[0], CHUNK):
        wd = w[i:i + CHUNK, None] * dy[i:i + CHUNK]
        dg = dg + (wd * (rows[i:i + CHUNK] - mean[None, :]) * rstd).sum(0)
        db = db + wd.sum(0)
    return dg, db


def split_weights(name, n, nsplit, rps):
    """row multiplicities of a split-boundary mistake: the first row of every split but the first dropped / counted by both neighbours"""
    if nsplit < 2:
        return None
    w = torch.ones(n, dtype=I64)
    starts = [s * rps for s in range(1, nsplit) if s * rps < n]
    if not starts:
        return None
    w[starts] = 0 if name == "split_boundary_dropped" else 2
    return w


SPLIT_MUTATIONS = ("split_boundary_dropped", "split_boundary_doubled")
# (F, lens, T, which buffer each utterance reads, ld - F): B*T in {2, 255, 256, 257}, T in {1, 7}, ends inside a 16-row group, a length of 1
BN_CASES = [
    dict(F=345, lens=(1, 1), T=1, which=(0, 1), gap=0),
    dict(F=320, lens=(2,), T=2, which=(0,), gap=8),
    dict(F=345, lens=(255,), T=255, which=(0,), gap=7),
    dict(F=256, lens=(128, 1), T=128, which=(0, 1), gap=0),
    dict(F=320, lens=(257,), T=257, which=(0,), gap=64),
    dict(F=345, lens=tuple([7, 1, 3, 7, 5] * 8 + [7] * 4), T=7, which=tuple(range(44)), gap=39),                # 308 rows: 2 splits of 154
    dict(F=256, lens=tuple([1] * 300), T=1, which=tuple(range(300)), gap=0),                                     # 300 rows, T = 1
    dict(F=320, lens=(100, 64, 7, 1), T=100, which=(0, 1, 2, 3), gap=0),                                         # 400 rows: 2 splits of 200
]
# just above 512 * 256 rows: 65 utterances of T = 2017 frames alias 5 buffers (the first three are read once: they carry the balancing,
# and 31 pairs read buffer 3 and its negative, so that the aliased rows cancel in the column sums)
BN_BIG = dict(F=345, T=2017, lens=tuple([2017, 1999, 1] + [2017 - 3 * ((i // 2) % 5) for i in range(62)]),
              which=tuple([0, 1, 2] + [3 + (i % 2) for i in range(62)]), gap=7, neg=(4, 3))


def bn_id(c):
    return f"F{c['F']}-B{len(c['lens'])}-T{c['T']}"


def bn_buffers(c, seed):
    nbuf = max(c["which"]) + 1
    bufs = [ints((c["T"], c["F"]), seed + k) for k in range(nbuf)]
    if "neg" in c:
        bufs[c["neg"][0]] = -bufs[c["neg"][1]]
    return bufs


# ------------------------------------------------------------------------------------------------ LS BatchNorm over the valid frames of slabs
def valid_rows(nseq, Tp, Tv, extra=0):
    """slab rows (seq*Tp + t) of the frames t < Tv + extra, in the kernels' walking order"""
    return (torch.arange(nseq)[:, None] * Tp + torch.arange(Tv + extra)[None, :]).reshape(-1)


def ref_bn16_stats(c, nseq, Tp, Tv, w=None, extra=0):
    """c int64 [nseq*Tp][256] -> (sum int64, n, mean float64, M2 float64) over the frames t < Tv (+ extra: the Tv mutation)"""
    rows = valid_rows(nseq, Tp, Tv, extra)
    v = c[rows]
    w = torch.ones(len(rows), dtype=I64) if w is None else w
    s = (w[:, None] * v).sum(0)
    n = nseq * Tv
    mean = s.double() / n
    return s, n, mean, (w[:, None].double() * (v.double() - mean) ** 2).sum(0)


def ref_bn_swish_stats(ds, c, mean, rstd, nseq, Tp, Tv, w=None, extra=0):
    """with swish' == 1 (beta = 30): S1 = sum ds, S2 = sum ds * c_hat, c_hat = (c - mean) * rstd, all int64"""
    rows = valid_rows(nseq, Tp, Tv, extra)
    w = torch.ones(len(rows), dtype=I64) if w is None else w
    dv, ch = ds[rows], (c[rows] - mean[None, :]) * rstd
    return (w[:, None] * dv).sum(0), (w[:, None] * dv * ch).sum(0)


def ref_bn_swish_apply(ds, c, mean, rstd, gamma, m1, m2, nseq, Tp, Tv):
    """d_c = gamma * rstd * (ds - m1 - c_hat * m2) for t < Tv, zero elsewhere (int64; swish' == 1)"""
    out = torch.zeros_like(ds)
    rows = valid_rows(nseq, Tp, Tv)
    ch = (c[rows] - mean[None, :]) * rstd
    out[rows] = gamma[None, :] * rstd * (ds[rows] - m1[None, :] - ch * m2[None, :])
    return out


# (nseq, Tp, Tv): nseq*Tv in {1, 31, 32, 33}, Tv = 1, Tv far below Tp, and one shape just above 4096 * 32 rows
BN16_CASES = [(1, 64, 1), (31, 64, 1), (1, 64, 31), (1, 64, 32), (32, 64, 1), (1, 64, 33), (33, 64, 1), (3, 64, 11), (2, 128, 65),
              (7, 128, 65), (3, 256, 130)]
BN16_BIG = (1009, 192, 130)               # 131170 rows > 131072: 4096 blocks of 33 rows, the last blocks empty


# ------------------------------------------------------------------------------------------------ conv module
GATE = 30.0                               # sigmoid(30) == 1 in f32: u = value, d_gate == 0
BETA = 40.0                               # BatchNorm + swish backward: gamma * c_hat + BETA >= 28, sigmoid == 1 and swish' == 1 in f32
CONV_K = (7, 15, 16, 31)


def conv_tv(k):
    return tuple(sorted({1, k - 2, k - 1, k, 63, 64, 65, 127, 128, 129}))


def conv_operands(nseq, Tp, Tv, k, seed):
    """(value [nseq][Tp][256], w [256][k], dc [nseq][Tp][256]) int64; the last sequence carries an impulse at t = 0 (its c reads the taps
    back one by one).  Frames t >= Tv hold +-1000 (value) and must not matter."""
    val = ints((nseq, Tp, D), seed)
    val[-1] = 0
    val[-1, 0] = 1
    val[:, Tv:] = 1000 * ints((nseq, Tp - Tv, D), seed + 1, vals=(-1, 1))
    w = ints((D, k), seed + 2)
    dc = ints((nseq, Tp, D), seed + 3)
    return val, w, dc


def ref_conv_fwd(val, w, Tv, shift=0, tv_extra=0):
    """c[t] = sum_j w[ch][j] u[t - (k-1) + j + shift] for t < Tv, u = value for 0 <= t < Tv + tv_extra, zero elsewhere; rows t >= Tv zero"""
    nseq, Tp, _ = val.shape
    k = w.shape[1]
    u = torch.zeros(nseq, Tp + 2 * k, D, dtype=I64)
    hi = min(Tv + tv_extra, Tp)
    u[:, k:k + hi] = val[:, :hi]
    c = torch.zeros(nseq, Tp, D, dtype=I64)
    for j in range(k):
        lo = k - (k - 1) + j + shift
        c[:, :Tv] += w[:, j].view(1, 1, D) * u[:, lo:lo + Tv]
    return c


def ref_conv_bwd(val, w, dc, Tv, shift=0, tv_extra=0):
    """du[t] = sum_m w[k-1-m] dc[t+m+shift] (t + m < Tv + tv_extra), dw[ch][k-1-m] = sum_{seq, t < Tv} u[t] dc[t+m+shift] -> (du, dw) int64"""
    nseq, Tp, _ = val.shape
    k = w.shape[1]
    g = torch.zeros(nseq, Tp + 2 * k + 2, D, dtype=I64)                       # frame t at index t + 1
    hi = min(Tv + tv_extra, Tp)
    g[:, 1:1 + hi] = dc[:, :hi]
    du = torch.zeros(nseq, Tp, D, dtype=I64)
    dw = torch.zeros(D, k, dtype=I64)
    for m in range(k):
        seg = g[:, 1 + m + shift:1 + m + shift + Tv]
        du[:, :Tv] += w[:, k - 1 - m].view(1, 1, D) * seg
        dw[:, k - 1 - m] = (val[:, :Tv] * seg).sum((0, 1))
    return du, dw


# ------------------------------------------------------------------------------------------------ optimiser
SUMSQ_N = (1, 2, 3, 4, 5, 1023, 1024, 1025, (1 << 20) - 1, (1 << 20) + 1, (1 << 20) + 2, (1 << 20) + 3, (1 << 21) + 7)
ADAM_N = (1, 255, 256, 257)


def ref_sumsq(g, w=None):
    g = g.to(I64)
    w = torch.ones_like(g) if w is None else w
    return int((w * g * g).sum())


def sumsq_weights(name, n):
    nb, passes, tail = sumsq_grid(n)
    w = torch.ones(n, dtype=I64)
    if name == "drop_tail":
        if not tail:
            return None
        w[n - tail:] = 0
    elif name == "tail_in_every_block":
        if not tail or nb < 2:
            return None
        w[n - tail:] = nb
    elif name == "drop_last_float4":
        if n < 4:
            return None
        w[(n // 4 - 1) * 4:(n // 4) * 4] = 0
    elif name == "no_second_pass":
        if passes < 2:
            return None
        w[4 * 256 * nb:4 * (n // 4)] = 0
    else:
        raise KeyError(name)
    return w


SUMSQ_MUTATIONS = ("drop_tail", "tail_in_every_block", "drop_last_float4", "no_second_pass")


def ref_adam(p, g, m, v, lr, step, max_norm, sumsq, b1=0.9, b2=0.98, eps=1e-9):
    """float64 Adam step with clip_grad_norm_ folded in (max_norm <= 0: no clipping) -> (p, m, v)"""
    coef = 1.0
    if max_norm > 0:
        coef = min(max_norm / (sumsq ** 0.5 + 1e-6), 1.0)
    gi = g * coef
    m = b1 * m + (1 - b1) * gi
    v = b2 * v + (1 - b2) * gi * gi
    denom = v.sqrt() / (1 - b2 ** step) ** 0.5 + eps
    return p - (lr / (1 - b1 ** step)) * (m / denom), m, v
