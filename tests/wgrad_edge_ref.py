"""Constructions and the exact reference for the weight-gradient family (csrc/wgrad.hip; no GPU needed).

The contraction dW[n][k] = sum_m dY[m][n] X[m][k] runs over f32 accumulators.  With small-integer operands every partial sum of every
summation order is an integer below 2^24 and therefore exact in f32: a correct kernel gives the bits of the int64 reference below
whatever its split, stage and tile order, and one token row dropped, doubled or paired with the wrong row changes them.  The guard
`assert_exact` checks the condition on the INPUTS (max_{n,k} sum_m |dY[m,n]| |X[m,k]| < 2^24); it says nothing about the kernel.

The tables at the bottom are the shapes tests/test_wgrad_edges.py runs on the GPU together with the plan class (tile, nsplit,
m_per_split) each case was written for; tests/test_wgrad_edges_ref.py shows on the CPU that every one-step mistake of MUTATIONS changes
the reference for those shapes."""
import torch

F16, BF16, F32, I64 = torch.float16, torch.bfloat16, torch.float32, torch.int64
VALS = (-2, -1, 1, 2)
LIMIT = 1 << 24
DY_SCALE_EXPONENTS = (-20, -40)      # dY = integer * 2^e: exact in bf16; below f16's normal range / below f16 altogether
GENEROUS = 600                       # workspace cap (in splits) that never binds: the planner wants at most 2 * CUs = 512


# ------------------------------------------------------------------------------------------------ operands
def ints(shape, seed, vals=VALS):
    """int64 tensor drawn from `vals` (non-zero by default: a lost boundary row must show)"""
    g = torch.Generator().manual_seed(seed)
    v = torch.tensor(vals, dtype=I64)
    return v[torch.randint(0, len(vals), tuple(shape), generator=g)]


def as16(t, dtype):
    """int64 / float64 -> f16 / bf16, asserting that nothing is rounded"""
    r = t.to(dtype)
    assert torch.equal(r.double(), t.double()), f"not exact in {dtype}"
    return r


def assert_exact(dy, x, extra=0):
    """the exactness guard: every f32 partial sum of sum_m dY[m][n] X[m][k] (+ extra) is an exact integer below 2^24"""
    ady, ax = dy.abs().to(I64), x.abs().to(I64)
    bound = int(ady.max()) * int(ax.max()) * dy.shape[0]              # cheap upper bound first
    if bound + extra >= LIMIT:
        bound = int((ady.double().t() @ ax.double()).max())           # (exact: integers far below 2^53)
    assert bound + extra < LIMIT, (bound, extra)
    return bound


def tie_x(M, K, seed):
    """f16 integers in [0, 2047] rich in bf16 rounding ties (bf16 keeps 8 significant bits: ulp 2 from 256, 4 from 512, 8 from 1024)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 2048, (M, K), generator=g)
    ties = torch.tensor([257, 259, 261, 263, 509, 511, 514, 518, 522, 1022, 1026, 1028, 1036, 1044, 2044, 2047, 255, 256, 0, 1])
    pick = torch.randint(0, len(ties), (M, K), generator=g)
    use = torch.rand(M, K, generator=g) < 0.5
    return torch.where(use, ties[pick], x)


def trunc_bf16(x16):
    """f16 -> bf16 by dropping the low 16 bits of the f32 (the mistake the tie construction pins)"""
    bits = x16.float().view(torch.int32) & ~0xFFFF
    return bits.view(F32).to(BF16)


# ------------------------------------------------------------------------------------------------ blocked layout
def to_blocked(t, pad=0.0):
    """row-major [M][F] -> the blocked layout of the stream entries, [ceil(M/16)*16][F] storage (padding rows = pad)."""
    M, F = t.shape
    Mp = (M + 15) // 16 * 16
    tp = torch.full((Mp, F), pad, dtype=t.dtype, device=t.device)
    tp[:M] = t
    return tp.view(Mp // 16, 16, F // 32, 32).permute(0, 2, 1, 3).contiguous().view(Mp, F)


def from_blocked(tb, M):
    Mp, F = tb.shape
    return tb.view(Mp // 16, F // 32, 16, 32).permute(0, 2, 1, 3).contiguous().view(Mp, F)[:M]


def pad_rows(t, pad_rows_):
    """[M][F] followed by the rows of pad_rows_ up to the next multiple of 16 (what to_blocked stores, row-major)"""
    M = t.shape[0]
    Mp = (M + 15) // 16 * 16
    return torch.cat([t, pad_rows_[:Mp - M].to(t.dtype)], 0)


# ------------------------------------------------------------------------------------------------ the reference
def ref_dw(dy, x, w=None):
    """int64 dW[n][k] = sum_m w[m] dY[m][n] X[m][k]   (w: per-row multiplicity, the handle of the row mutations; None = 1)"""
    a = dy.to(I64)
    if w is not None:
        a = a * w.to(I64)[:, None]
    return a.t() @ x.to(I64)


def ref_db(dy, w=None):
    a = dy.to(I64)
    if w is not None:
        a = a * w.to(I64)[:, None]
    return a.sum(0)


def conv_pairs(nseq, Tp, ilens, ktaps, pad, mut=None, mps=None):
    """(valid [M][ktaps] bool, src [M][ktaps] global X row) of the Conv1d weight gradient, as the definition: output frame t of a
    sequence meets, for tap j, input frame t + j - pad of the SAME sequence if that lies in [0, ilen).  mut: a conv mutation name."""
    M = nseq * Tp
    gr = torch.arange(M)[:, None]
    seq, t = gr // Tp, gr % Tp
    j = torch.arange(ktaps)[None, :]
    ts = t + j - pad + (1 if mut == "conv_tap_off_by_one" else 0)
    il = torch.as_tensor(ilens, dtype=I64)[seq]
    hi = Tp if mut == "conv_ignore_ilen" else il
    valid = (ts >= 0) & (ts < hi)
    if mut == "conv_neighbour_sequence":             # frames before the sequence start taken from the previous sequence's tail
        valid = (ts < hi) & (seq * Tp + ts >= 0)
    if mut == "conv_clip_at_split_start":            # the split's first row taken for the sequence's first frame
        valid = valid & (seq * Tp + ts >= (gr // mps) * mps)
    src = (seq * Tp + ts).clamp(0, M - 1)
    return valid, src


def ref_conv_dw(dy, x, nseq, Tp, ilens, ktaps, pad, mut=None, mps=None, via_f64=False):
    """int64 [cout][cin][ktaps]: dY [nseq*Tp][cout], X [nseq*Tp][cin] (frames >= ilen hold poison that must not contribute).
    via_f64: the products through the float64 BLAS (exact for these integers, far below 2^53; for the one large case)"""
    valid, src = conv_pairs(nseq, Tp, ilens, ktaps, pad, mut, mps)
    a, b = dy.to(I64), x.to(I64)
    out = torch.empty(a.shape[1], b.shape[1], ktaps, dtype=I64)
    at = a.double().t().contiguous() if via_f64 else a.t()
    for j in range(ktaps):
        bj = b[src[:, j]] * valid[:, j, None]
        out[:, :, j] = (at @ bj.double()).to(I64) if via_f64 else at @ bj
    return out


# ------------------------------------------------------------------------------------------------ one-step mistakes
def split_bounds(M, nsplit, mps):
    return [(s * mps, min((s + 1) * mps, M)) for s in range(nsplit)]


def row_weights(name, M, nsplit, mps):
    """per-row multiplicity of a row mutation, or None where the shape gives the mistake nothing to act on"""
    w = torch.ones(M, dtype=I64)
    sb = split_bounds(M, nsplit, mps)
    if name == "drop_last_row_of_split":
        for _, e in sb:
            w[e - 1] = 0
    elif name == "drop_first_row_of_split":
        for b, _ in sb:
            w[b] = 0
    elif name == "boundary_row_in_both_splits":
        if nsplit < 2:
            return None
        for b, _ in sb[1:]:
            w[b] = 2
    elif name == "drop_last_stage_of_split":          # the last (possibly partial) 32-row stage of the last split
        b, e = sb[-1]
        w[b + (e - b - 1) // 32 * 32:e] = 0
    elif name == "drop_rows_beyond_last_64":
        if M % 64 == 0:
            return None
        w[M // 64 * 64:] = 0
    elif name == "drop_one_split":
        b, e = sb[nsplit // 2]
        w[b:e] = 0
    else:
        raise KeyError(name)
    return w


ROW_MUTATIONS = ("drop_last_row_of_split", "drop_first_row_of_split", "boundary_row_in_both_splits", "drop_last_stage_of_split",
                 "drop_rows_beyond_last_64", "drop_one_split")
CONV_MUTATIONS = ("conv_tap_off_by_one", "conv_ignore_ilen", "conv_clip_at_split_start", "conv_neighbour_sequence")


def bias_from_ktile1_too(db, K, tile):
    return db * 2 if K // tile >= 2 else None


def bias_first_ntile_only(db, N, tile):
    if N // tile < 2:
        return None
    r = db.clone()
    r[tile:] = 0
    return r


def transposed_output(dw):
    N, K = dw.shape
    return dw.t().contiguous().view(N, K)


def tiles_k_major(dw, tile):
    """the output tiles written in k-major instead of n-major order: slot i = tn * ntk + tk receives tile (i % ntn, i // ntn)"""
    N, K = dw.shape
    ntn, ntk = N // tile, K // tile
    if ntn < 2 or ntk < 2:
        return None
    r = torch.empty_like(dw)
    for tn in range(ntn):
        for tk in range(ntk):
            i = tn * ntk + tk
            sn, sk = i % ntn, i // ntn
            r[tn * tile:(tn + 1) * tile, tk * tile:(tk + 1) * tile] = dw[sn * tile:(sn + 1) * tile, sk * tile:(sk + 1) * tile]
    return r


# ------------------------------------------------------------------------------------------------ the GPU tables
def _case(group, M, N, K, cap, tile, nsplit, mps, **kw):
    d = dict(group=group, M=M, N=N, K=K, cap=cap, tile=tile, nsplit=nsplit, mps=mps)
    d.update(kw)
    return d


def _up64(M):
    return (M + 63) // 64 * 64


A_M = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 161, 257, 1000)
B_S = (2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 63, 64, 65, 72, 512)
B_TAIL = (1, 33, 64)
# (M, cap) -> (nsplit, m_per_split): splits several stages long, a shorter last split
B_CAPPED = {(1000, 3): (3, 384), (1000, 5): (4, 256), (2049, 9): (7, 320)}
C_NK = ((256, 128), (128, 384), (384, 256))
C_M = (65, 200)
D_M = (16384, 16385, 16384 + 33, 16384 + 63)


def gemm_cases():
    """every (M, N, K, workspace cap) of groups a - d with its plan class (a 256-CU device)"""
    out = []
    for M in A_M:                                                            # a: one split, 1 .. 32 stages
        out.append(_case("a", M, 128, 128, 1, 128, 1, _up64(M)))
    for s in B_S:                                                            # b: nsplit == s, 64 rows per split
        for tail in B_TAIL:
            out.append(_case("b", 64 * (s - 1) + tail, 128, 128, GENEROUS, 128, s, 64))
    for (M, cap), (ns, mps) in B_CAPPED.items():
        out.append(_case("b", M, 128, 128, cap, 128, ns, mps))
    for N, K in C_NK:                                                        # c: several tiles, N != K
        for M in C_M:
            out.append(_case("c", M, N, K, GENEROUS, 128, (M + 63) // 64, 64))
    for M in D_M:                                                            # d: the 256 tile, one long split and 16 splits
        out.append(_case("d", M, 256, 512, 1, 256, 1, _up64(M)))
        sps = ((M + 63) // 64 + 15) // 16
        out.append(_case("d", M, 256, 512, 16, 256, ((M + 63) // 64 + sps - 1) // sps, sps * 64))
    out.append(_case("d", 16384, 256, 256, GENEROUS, 128, 128, 128))         # a single 256 x 256 output keeps the small tile
    out.append(_case("d", 16383, 256, 512, GENEROUS, 128, 64, 256))          # under 16384 rows too
    return out


def case_id(c):
    return f"{c['group']}-M{c['M']}-N{c['N']}-K{c['K']}-cap{c['cap']}"


def ws_floats(c, bias):
    return c["cap"] * (c["N"] * c["K"] + (c["N"] if bias else 0))


def _conv(nseq, Tp, ilens, cap, tile, nsplit, mps, ktaps=19, pad=9):
    return dict(nseq=nseq, Tp=Tp, ilens=tuple(ilens), cap=cap, tile=tile, nsplit=nsplit, mps=mps, ktaps=ktaps, pad=pad)


def conv_cases():
    out = []
    Tp = 192                                                                  # nseq 2: splits begin at t = 64 and t = 128
    for il in ((Tp, Tp), (1, Tp), (0, 5), (9, 10), (Tp - 1, 64), (65, 127)):
        out.append(_conv(2, Tp, il, 8, 128, 6, 64))
    out.append(_conv(7, 64, (64, 1, 0, 5, 9, 10, 63), 8, 128, 7, 64))         # a split per sequence
    out.append(_conv(7, 64, (63, 64, 10, 9, 1, 64, 0), 4, 128, 4, 128))       # a split spans two sequences
    for il in ((Tp, Tp, Tp), (Tp - 1, 64, 1), (65, 127, 129), (0, 5, 9)):     # 128-row splits: t = 128 of seq 0, t = 64 of seq 1, ...
        out.append(_conv(3, Tp, il, 5, 128, 5, 128))
    out.append(_conv(2, Tp, (65, 127), 8, 128, 6, 64, ktaps=7, pad=3))
    out.append(_conv(2, Tp, (Tp, 3), 8, 128, 6, 64, ktaps=7, pad=3))
    big = [512, 1, 0, 9, 10, 511, 65, 127, 64, 63, 256, 257] + [512 - 13 * (i % 7) for i in range(20)]
    out.append(_conv(32, 512, big, 8, 256, 8, 2048))                          # >= 16384 rows, conv_cin == 256: the 256 tile
    return out


def conv_id(c):
    il = "-".join(str(i) for i in c["ilens"][:4])
    return f"n{c['nseq']}-Tp{c['Tp']}-k{c['ktaps']}-cap{c['cap']}-il{il}"


# eend_colsum_f32: (M, N, ns): the workspace holds exactly ns rows of N floats; ns = min(ws / N, 1024, ceil(M / 64))
COLSUM_CASES = [(M, N, 1) for N in (8, 264, 2048) for M in (1, 7, 8, 9, 63, 64, 65, 1000)] + \
               [(1000, 264, 15), (1000, 2048, 16), (1000, 8, 16), (1025, 264, 17), (4161, 2048, 65), (4097, 8, 65)]
