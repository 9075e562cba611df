"""Constructions, exact references, case tables and mutations for the training GEMM, fused-FFN and head-projection entries of
csrc/api_train.hip (no GPU needed): csrc/gemm.hip with bf16 operands (EPI_PLAIN_BF16, EPI_MASK_BF16, EPI_RES_SCALE, EPI_RES_LNBWD,
EPI_F32_ROWMASK) and its training epilogues on f16 operands (EPI_RES_LN_TRAIN, EPI_RES_SCALE_LN16_TRAIN, EPI_L2NORM_TRAIN,
EPI_PLAIN_RELU_F16 with dropout), csrc/ffn.hip MODE 3 / 4 and csrc/proj.hip's PROJ_HEADS_BOTH stores.

The method is that of tests/linear_edge_ref.py, whose helpers are imported: operands are small integers, so every f32 partial sum of
every summation order is an exact integer below 2^24 and the linear part of every epilogue has ONE right answer in bits.  Dropout is
p = 0.5 (thresh24 = 2^23, scale 2: dropped elements are 0, kept ones exactly doubled), alphas and drop scales are powers of two.  Two
guards are asserted on the inputs and references of every case, never on a kernel's output:
  (a) every sum bound (sum_k |A||W| + the additive terms, for each product of a case) is below 2^24        (sum_bound)
  (b) every reference value that lands in a 2-byte output is exactly representable there                    (reference() -> E.as16)

reference(c, mut) returns the expected contents of every OUTPUT BUFFER of a case, guard rows and guard columns included, as float64 with
NaN where nothing may be written; `mut` names a one-step mistake (MUTATIONS) and gives the buffers such a kernel would leave.

Outputs behind rsqrt / exp are compared against float64 computed from the exact rows (compare()).  Their bounds (TOL):
  - where the project already bounds the same output of the same entry, that bound, unchanged: linear_edge_ref.TOL (ln32 / ln16 / l2_32 /
    l2_16) and the ds bounds of tests/test_train_kernels.py::test_gemm_acc_layernorm_bwd_fused;
  - elsewhere (rstd, xhat_f16, inv_norm, a_f16, the un-normalised stream behind an unsaturated Swish) 8 x gap32, a 2-byte output
    additionally half an ulp of its type at the reference value.  gap32 is the largest error of a plain torch CPU fp32 evaluation of the
    same formula from the same exact rows against float64: over the case's rows for the row-major outputs, and for the per-row scalars
    (rstd, inv_norm) relative to the reference value over the rows of all the entry's cases (pooled_gap() says why).  Only the summation
    order differs between that evaluation and a kernel's, and the factor 8 is the precedent of tests/test_lstm_gpu.py.  No bound comes
    from a kernel's output.
Every toleranced row has non-zero variance / norm (asserted in reference())."""
import functools
import zlib

import torch

from tests import rowgrad_edge_ref as RG
from tests.linear_edge_ref import (BF16, F16, F32, F64, GUARD_ROWS, LIMIT, NAN, PAD_FILL, V1, V3, as16, assert_exact, conv_columns, ints,
                                   layer_norm, same)
from tests.linear_edge_ref import TOL as LINEAR_TOL

HALF = RG.HALF                        # thresh24 of p = 0.5
EPS = 1e-5
SWISH_SAT = 1024                      # |b1| of the saturated Swish cases: sigmoid(z) is exactly 0 or 1 in f32, z stays an f16 integer
NCU_MI355X = 256                      # multi_processor_count of the MI355X: what the CPU module resolves the persistent cases with
SUBNORMAL16 = 2.0 ** -24              # the smallest f16 subnormal: a non-zero activation

FAMILY = {"gemm_bf16": "g128", "gemm_relu_bwd_bf16": "g128", "linear_relu_train_f16": "g128",
          "gemm_acc_bf16": "acc", "gemm_acc_lnbwd_bf16": "lnbwd", "conv1d_dgrad_bf16": "dgrad",
          "linear_res_ln_train_f16": "resln", "linear_res_scale_ln_train_f16": "resln", "conv1d_l2norm_train_f16": "l2train",
          "inproj_heads_train_bf16": "heads", "ffn_train_f16": "ffn", "ffn_swish_train_f16": "ffn", "ffn_bwd_data_bf16": "ffnbwd"}
ROW_TILE = {"g128": 128, "acc": 64, "lnbwd": 64, "dgrad": 64, "resln": 64, "l2train": 64, "heads": 128, "ffn": 128, "ffnbwd": 128}

# name -> (kind, atol, rtol, source).  "elem": atol + rtol |want| per element; "gap": 8 gap32 (+ half an ulp of a 2-byte output type);
# "scale": rtol * the case's scale (lnbwd: max |g gamma| * max rstd for ds32, max |ds16| for ds16)
TOL = {
    "ln32": LINEAR_TOL["ln32"] + ("tests/linear_edge_ref.py TOL['ln32'] (test_hip_kernels.py::test_linear_res_ln)",),
    "ln16": LINEAR_TOL["ln16"] + ("tests/linear_edge_ref.py TOL['ln16']",),
    "l2_32": LINEAR_TOL["l2_32"] + ("tests/linear_edge_ref.py TOL['l2_32'] (test_hip_kernels.py::test_conv1d_l2norm)",),
    "l2_16": LINEAR_TOL["l2_16"] + ("tests/linear_edge_ref.py TOL['l2_16']",),
    "ds32": ("scale", 0.0, 1e-4, "test_train_kernels.py::test_gemm_acc_layernorm_bwd_fused: |ds_f32 - float64| < 1e-4 * max|g gamma| * max rstd"),
    "ds16": ("scale", 0.0, 1e-2, "test_train_kernels.py::test_gemm_acc_layernorm_bwd_fused: |ds_bf16 - want| < 1e-2 * max|want|"),
    "gap32": ("gap", 0.0, 8.0, "8 x gap32 (no project bound for this output; factor: tests/test_lstm_gpu.py)"),
    "gap16": ("gap", 0.5, 8.0, "8 x gap32 + half an f16 ulp at the reference value"),
}


# ------------------------------------------------------------------------------------------------ cases
def case_id(c):
    keys = ("M", "N", "K", "F", "lda", "ldw", "ldo", "ldact", "ldx", "bias", "drop", "drop2", "scale", "res", "alpha", "out32", "out16", "alias",
            "dbias", "nseq", "Tp", "cin", "ktaps", "pad", "lens", "mlens", "xt", "unnorm", "sat", "persist")
    parts = [c["entry"]]
    for k in keys:
        if c.get(k) is not None:
            v = c[k]
            parts.append(f"{k}{'x'.join(map(str, v)) if isinstance(v, (list, tuple)) else v}")
    return "-".join(parts)


def resolve(c, ncu=NCU_MI355X):
    """the persistent FFN cases take M = 128 * ncu + 129 (ncu read from the device at run time): some workgroup takes a second tile and a
    ragged last one"""
    if c.get("persist") and c.get("M") is None:
        return dict(c, M=128 * ncu + 129, ncu=ncu)
    return c


def rows_of(c):
    return c["M"] if c.get("M") else c["nseq"] * c["Tp"]


def _seed(c):
    return zlib.crc32(case_id(c).encode()) & 0x3FFFFFFF


def sum_bound(A, W, *adds):
    """guard (a) for a product whose operands may hold zeros (a ReLU'd or dropped hidden row, a masked gradient)"""
    extra = sum(float(x.abs().max()) for x in adds if x is not None)
    bound = float(A.abs().max()) * float(W.abs().max()) * A.shape[1]
    assert bound + extra < LIMIT, (bound, extra)
    return bound + extra


def keep2(rows, ncols, seed, on, mut=None, tile=128):
    """the factor dropout at p = 0.5 puts on element (row, column): 0 or 2 (1 everywhere without dropout)"""
    if not on:
        return torch.ones(len(rows), ncols, dtype=F64)
    if mut == "drop_row_tile_local":
        rows = rows % tile
    k = RG.keep(rows, ncols, seed, HALF).double()
    return k if mut == "drop_scale_missing" else 2.0 * k


def mask_pattern(M, N, seed):
    """a saved activation [M][N] as float64 with every kind of zero and non-zero the ReLU-backward mask must tell apart: +0, -0.0 (0x8000:
    zero), the smallest f16 subnormal (non-zero), small integers; the first two rows alternate zero / non-zero inside every 32-bit pair"""
    g = torch.Generator().manual_seed(seed)
    kinds = torch.tensor([0.0, -0.0, SUBNORMAL16, 1.0, -2.0, 0.0, 3.0, -0.0], dtype=F64)
    a = kinds[torch.randint(0, len(kinds), (M, N), generator=g)]
    a[0, 0::2], a[0, 1::2] = 0.0, 1.0
    a[0, 2:N:8] = -0.0
    a[0, 3:N:8] = SUBNORMAL16
    if M > 1:
        a[1, 0::2], a[1, 1::2] = SUBNORMAL16, -0.0
    return a


def is_zero16(a, mut=None):
    """zero <=> no magnitude bits; the mutation counts the sign bit too"""
    if mut == "mask_sign_bit_counts":
        return (a == 0) & ~torch.signbit(a)
    return a == 0


@functools.lru_cache(maxsize=None)
def _operands(cid, M):
    c = dict(_BY_ID[cid])
    if c.get("persist"):
        c["M"] = M
    s, fam, e = _seed(_BY_ID[cid]), FAMILY[c["entry"]], c["entry"]
    o = {"seed": s, "drop_seed": (s * 2654435761) & 0xFFFFFFFF, "drop2_seed": (s * 40503 + 17) & 0xFFFFFFFF}
    gen = torch.Generator().manual_seed(s + 4)
    if fam == "g128":
        o["A"], o["W"] = ints((M, c["K"]), s, V1), ints((c["N"], c["K"]), s + 1, V1)
        o["bias"] = ints((c["N"],), s + 2, V3) * 2 if c.get("bias") else None          # even: A W^T + b stays even, exact in bf16
        if e == "gemm_relu_bwd_bf16":
            o["act"] = mask_pattern(M, c["N"], s + 3)
    elif fam == "acc":
        o["A"], o["W"] = ints((M, c["K"]), s, V1), ints((256, c["K"]), s + 1, V1)
        o["res"] = ints((M, 256), s + 3, V3) * 2 if c["res"] else None
    elif fam == "lnbwd":
        o["A"], o["W"] = ints((M, c["K"]), s, V1), ints((256, c["K"]), s + 1, V1)
        o["g"], o["xhat"], o["rstd"], o["gamma"] = RG.ln_operands(M, s + 2)          # g = A W^T + g0 is this construction
        o["g0"] = o["g"] - o["A"] @ o["W"].t()
    elif fam == "dgrad":
        o["A"] = ints((M, 256), s, V1)                                                 # dY: non-zero beyond src_lens too
        o["W"] = ints((256, c["ktaps"] * 256), s + 1, V1)
    elif fam == "resln":
        o["A"], o["W"] = ints((M, c["K"]), s, V1), ints((256, c["K"]), s + 1, V1)
        o["bias"] = ints((256,), s + 2, V3) if c["bias"] else None
        o["res"] = ints((M, 256), s + 3, V3) * 4 if c["res"] else None
    elif fam == "l2train":
        o["A"] = ints((M, c["cin"]), s, V1)
        o["W"] = ints((256, c["ktaps"] * c["cin"]), s + 1, V1)
        o["bias"] = ints((256,), s + 2, V3)
    elif fam == "heads":
        o["A"], o["W"] = ints((M, 256), s, V1), ints((768, 256), s + 1, V1)
        o["bias"] = ints((768,), s + 2, V3) * 2
    elif fam == "ffn":
        F = c["F"]
        o["A"], o["W"] = ints((M, 256), s, V1), ints((F, 256), s + 1, V1)
        o["bias"] = ints((F,), s + 2, V3) * 2
        if c.get("sat"):
            o["bias"] = ints((F,), s + 2, V1) * SWISH_SAT
        o["W2"], o["b2"] = ints((256, F), s + 5, V1), ints((256,), s + 6, V3)
        o["res"] = ints((M, 256), s + 3, V3) * 4
    elif fam == "ffnbwd":
        F = c["F"]
        o["A"], o["W"] = ints((M, 256), s, V1), ints((F, 256), s + 1, V1)              # dY, W2^T
        o["act"] = mask_pattern(M, F, s + 3)
        o["W2"] = ints((256, F), s + 5, V1)                                            # W1^T
        o["res"] = ints((M, 256), s + 6, V3) * 4                                       # the gradient stream the product joins
    if fam in ("resln", "ffn"):
        o["gamma"] = 1.0 + torch.randint(-4, 5, (256,), generator=gen).double() / 16
        o["beta"] = torch.randint(-8, 9, (256,), generator=gen).double() / 16
    return o


def operands(c):
    """the case's operands as float64 CPU tensors (computed once per case and row count, never modified)"""
    assert c.get("M") or c.get("nseq"), "resolve() the case first"
    return _operands(case_id(dict(c, M=None, ncu=None) if c.get("persist") else c), rows_of(c))


# ------------------------------------------------------------------------------------------------ mutations
MUTATIONS = ("ktile_dropped", "ktile_doubled", "rows_shifted", "last_tile_row_lost", "mask_at_ldo", "mask_sign_bit_counts",
             "drop_row_tile_local", "drop_scale_missing", "pad_row_in_colsum", "tap_crosses_sequence", "rowmask_off_by_one",
             "head_layout_transposed", "qk_swapped", "second_tile_reuses_first")


def applies(mut, c):
    fam, e, M = FAMILY[c["entry"]], c["entry"], rows_of(c)
    dropped = bool(c.get("drop") or c.get("drop2"))
    if fam == "dgrad" and not any(l > 0 for l in c["mlens"]):            # every row masked: the output is all zero whatever the product
        return mut in ("rowmask_off_by_one", "last_tile_row_lost")
    if mut in ("ktile_dropped", "ktile_doubled", "last_tile_row_lost"):
        return True
    if mut == "rows_shifted":
        return M >= 2
    if mut == "mask_at_ldo":
        return e == "gemm_relu_bwd_bf16" and c["ldact"] != c["ldo"] and M >= 2
    if mut == "mask_sign_bit_counts":
        return e in ("gemm_relu_bwd_bf16", "ffn_bwd_data_bf16")
    if mut == "drop_row_tile_local":
        return dropped and M > ROW_TILE[fam]
    if mut == "drop_scale_missing":
        return dropped or (c.get("scale") or 1) != 1
    if mut == "pad_row_in_colsum":
        return fam == "lnbwd" and M % 64 != 0
    if mut == "tap_crosses_sequence":
        return fam in ("dgrad", "l2train") and c["pad"] > 0 and c["nseq"] >= 2 and (fam != "dgrad" or any(l > 0 for l in c["mlens"][1:]))
    if mut == "rowmask_off_by_one":
        return fam == "dgrad" and any(0 <= l < c["Tp"] for l in c["mlens"])
    if mut in ("head_layout_transposed", "qk_swapped"):
        return fam == "heads"
    if mut == "second_tile_reuses_first":
        return bool(c.get("persist"))
    raise KeyError(mut)


# ------------------------------------------------------------------------------------------------ the references
def _product(A, W, mut, bias=None):
    """exact y = A W^T (+ bias) as float64 integers; the k-tile and row mutations applied"""
    K = W.shape[1]
    if mut == "ktile_dropped":
        W = W.clone(); W[:, K - 64:] = 0
    elif mut == "ktile_doubled":
        W = W.clone(); W[:, K - 64:] *= 2
    y = A @ W.t()
    if bias is not None:
        y = y + bias
    if mut == "rows_shifted":
        y = torch.roll(y, 1, 0)
    return y


def _buf(y, ld, mut):
    """[M][N] rows (or an [M] vector) -> the output buffer with GUARD_ROWS NaN rows behind row M and NaN guard columns up to ld"""
    M = y.shape[0]
    if y.dim() == 1:
        buf = torch.full((M + GUARD_ROWS,), NAN, dtype=F64)
        buf[:M] = y
    else:
        buf = torch.full((M + GUARD_ROWS, ld), NAN, dtype=F64)
        buf[:M, :y.shape[1]] = y
    if mut == "last_tile_row_lost":
        buf[M - 1] = NAN
    return buf


def _norm_parts(y, gamma, beta, dt):
    """LayerNorm of the rows y evaluated in dtype dt with plain torch ops: ln, xhat, rstd"""
    y = y.to(dt)
    mu = y.mean(1, keepdim=True)
    var = ((y - mu) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xhat = (y - mu) * rstd
    return dict(ln=xhat * gamma.to(dt) + beta.to(dt), xhat=xhat, rstd=rstd[:, 0])


def _l2_parts(y, dt):
    y = y.to(dt)
    inv = 1.0 / torch.linalg.vector_norm(y, dim=1, keepdim=True)
    return dict(unit=y * inv, inv=inv[:, 0])


def swish(z, dt=F64):
    z = z.to(dt)
    return z * torch.sigmoid(z)


def _gap(parts64, parts32, rel=False):
    return {k: float(((parts32[k].double() - parts64[k]).abs() / (parts64[k].abs() if rel else 1.0)).max()) for k in parts64}


def _head_rows(y, nseq, Tp, mut):
    """[M][256] -> [nseq][4][Tp][64]"""
    if mut == "head_layout_transposed":
        return y.reshape(nseq, Tp, 4, 64).permute(0, 2, 3, 1).reshape(nseq, 4, Tp, 64)
    return y.reshape(nseq, Tp, 4, 64).permute(0, 2, 1, 3).contiguous()


def _head_rows_t(y, nseq, Tp, mut):
    """[M][256] -> [nseq][4][64][Tp]"""
    if mut == "head_layout_transposed":
        return y.reshape(nseq, Tp, 4, 64).permute(0, 2, 1, 3).reshape(nseq, 4, 64, Tp)
    return y.reshape(nseq, Tp, 4, 64).permute(0, 2, 3, 1).contiguous()


def _conv_case(c, lens):
    return dict(nseq=c["nseq"], Tp=c["Tp"], cin=c.get("cin", 256), ktaps=c["ktaps"], pad=c["pad"], ilens=list(lens))


def _second_tile(rows, c, mut):
    """second_tile_reuses_first: the workgroup that takes a second 128-row tile (rows 128 ncu ..) writes its first tile's rows again"""
    if mut == "second_tile_reuses_first":
        rows = rows.clone()
        n0 = 128 * c["ncu"]
        n = min(128, rows.shape[0] - n0)
        rows[n0:n0 + n] = rows[:n]
    return rows


def reference(c, mut=None, a16=None, with_aux=False):
    """name -> expected output buffer (float64, NaN = untouched) of the resolved case c; mut: the buffers a kernel with that mistake would
    leave.  a16 (unsaturated Swish cases on the GPU): the saved activation the kernel itself wrote, as float64 -- it is the f16 operand of
    the second product, and whether it rounds a value up or down is not decided by the exact rows; the CPU module passes nothing and the
    reference rounds float64 Swish to f16 itself.  with_aux: also return the figures the toleranced comparisons need (gap32 per output of
    an fp32 evaluation, the ds scales).  The plain references are computed once and shared (copies are handed out)."""
    if mut is not None or a16 is not None:
        return _reference(c, mut, a16, with_aux)
    key = (case_id(c), rows_of(c))
    if key in _REF_CACHE:
        out, aux = _REF_CACHE[key]
    else:
        out, aux = _reference(c, None, None, True)
        _AUX_CACHE[key] = aux
        if rows_of(c) <= 4096:                           # (the persistent cases' buffers are not kept)
            _REF_CACHE[key] = (out, aux)
    out = {k: v.clone() for k, v in out.items()}
    return (out, aux) if with_aux else out


_REF_CACHE, _AUX_CACHE = {}, {}


def aux_of(c):
    key = (case_id(c), rows_of(c))
    if key not in _AUX_CACHE:
        reference(c)
    return _AUX_CACHE[key]


def _reference(c, mut, a16, with_aux):
    o, fam, e, M = operands(c), FAMILY[c["entry"]], c["entry"], rows_of(c)
    out, aux = {}, {"gap": {}}
    rows = torch.arange(M)
    kmut = mut if mut in ("ktile_dropped", "ktile_doubled", "rows_shifted") else None
    if fam == "g128":
        assert_exact(o["A"], o["W"], o["bias"])
        y = _product(o["A"], o["W"], kmut, o["bias"])
        if e == "gemm_relu_bwd_bf16":
            act = o["act"]
            zero = is_zero16(act, mut)
            if mut == "mask_at_ldo":                     # the mask read with the output's row stride
                flat = torch.full((M, c["ldact"]), float(PAD_FILL), dtype=F64)
                flat[:, :c["N"]] = act
                idx = (rows[:, None] * c["ldo"] + torch.arange(c["N"])[None, :]).clamp_max(flat.numel() - 1)
                zero = is_zero16(flat.reshape(-1)[idx])
            scale = 1.0 if mut == "drop_scale_missing" else c["scale"]
            y = torch.where(zero, torch.zeros_like(y), y * scale)
        elif e == "linear_relu_train_f16":
            y = y.relu() * keep2(rows, c["N"], o["drop_seed"], c.get("drop"), mut, 128)
        out["out"] = _buf(y, c["ldo"], mut)
    elif fam == "acc":
        assert_exact(o["A"], o["W"], o["res"])
        y = _product(o["A"], o["W"], kmut) * c["alpha"]
        if o["res"] is not None:
            y = y + o["res"]
        if c["out32"]:
            out["out32"] = _buf(y, 256, mut)
        if c["out16"]:
            out["out16"] = _buf(y, 256, mut)
    elif fam == "lnbwd":
        sum_bound(o["A"], o["W"], o["g0"])                  # (g0 = g - A W^T may hold zeros)
        g = _product(o["A"], o["W"], kmut) + (torch.roll(o["g0"], 1, 0) if mut == "rows_shifted" else o["g0"])
        x, rstd, gamma = o["xhat"], o["rstd"], o["gamma"]
        ds = RG.ref_ln_ds(g, x, rstd, gamma)
        ds16 = ds * keep2(rows, 256, o["drop_seed"], c.get("drop"), mut, 64)
        if mut is None:
            assert torch.equal(g, o["g"]) and RG.assert_exact(g, g * x, ds16, unit=2.0 ** -4) < LIMIT
        w = torch.ones(M, dtype=F64)
        if mut == "pad_row_in_colsum":                   # the clamped row behind row M counted into the column sums
            w[M - 1] = 2
        elif mut == "last_tile_row_lost":
            w[M - 1] = 0
        out["ds32"], out["ds16"] = _buf(ds, 256, mut), _buf(ds16, 256, mut)
        out["dgamma"], out["dbeta"] = (w[:, None] * g * x).sum(0), (w[:, None] * g).sum(0)
        if c["dbias"]:
            out["dbias"] = (w[:, None] * ds16).sum(0)
        aux["scale"] = {"ds32": float((o["g"] * gamma).abs().max() * rstd.max()),
                        "ds16": float(RG.ref_ln_ds(o["g"], x, rstd, gamma).abs().max()) * (2.0 if c.get("drop") else 1.0)}
    elif fam == "dgrad":
        cmut = "conv_tap_across_sequences" if mut == "tap_crosses_sequence" else None
        cols = conv_columns(_conv_case(c, c["lens"]), o["A"], cmut)
        sum_bound(cols, o["W"])
        y = _product(cols, o["W"], kmut)
        ml = torch.tensor(c["mlens"])[rows // c["Tp"]] + (1 if mut == "rowmask_off_by_one" else 0)
        y = torch.where(((rows % c["Tp"]) < ml)[:, None], y, torch.zeros_like(y))
        out["out32"] = _buf(y, 256, mut)
    elif fam == "resln":
        assert_exact(o["A"], o["W"], o["bias"], o["res"])
        y = _product(o["A"], o["W"], kmut, o["bias"]) * keep2(rows, 256, o["drop_seed"], c.get("drop"), mut, 64) * c["alpha"]
        if o["res"] is not None:
            y = y + o["res"]
        assert float(y.abs().max()) * 2 < LIMIT
        out.update(_normed(c, o, y, mut, aux, unnorm=(e == "linear_res_scale_ln_train_f16")))
    elif fam == "l2train":
        cmut = "conv_tap_across_sequences" if mut == "tap_crosses_sequence" else None
        cols = conv_columns(_conv_case(c, c["lens"]), o["A"], cmut)
        sum_bound(cols, o["W"], o["bias"])
        y = _product(cols, o["W"], kmut, o["bias"])
        p64 = _l2_parts(y, F64)
        assert (torch.linalg.vector_norm(y, dim=1) > 0).all(), "a reference row with zero norm must not decide a case"
        out["out32"], out["out16"], out["inv_norm"] = _buf(p64["unit"], 256, mut), _buf(p64["unit"], 256, mut), _buf(p64["inv"], 0, mut)
        if with_aux and mut is None:
            aux["gap"]["inv_norm"] = _gap(p64, _l2_parts(y, F32), rel=True)["inv"]
    elif fam == "heads":
        assert_exact(o["A"], o["W"], o["bias"])
        W, b = o["W"], o["bias"]
        if mut == "qk_swapped":
            W, b = torch.cat([W[256:512], W[:256], W[512:]]), torch.cat([b[256:512], b[:256], b[512:]])
        y = _product(o["A"], W, kmut, b)
        if mut == "last_tile_row_lost":
            y = y.clone(); y[M - 1] = NAN
        for i, n in enumerate("QKV"):
            out[n] = _head_rows(y[:, 256 * i:256 * (i + 1)], c["nseq"], c["Tp"], mut)
            if n == "V" or c["xt"] == "all":
                out[n + "t"] = _head_rows_t(y[:, 256 * i:256 * (i + 1)], c["nseq"], c["Tp"], mut)
    elif fam == "ffn":
        assert_exact(o["A"], o["W"], o["bias"])
        z = _product(o["A"], o["W"], kmut, o["bias"])
        k1 = keep2(rows, c["F"], o["drop_seed"], c.get("drop"), mut, 128)
        if e == "ffn_train_f16":
            hid = z.relu() * k1
        else:
            act = swish(z)
            if c.get("sat") and mut is None:             # sigmoid is exactly 0 or 1 in f32: a is z or 0, in bits
                assert (z.abs() >= 512).all() and torch.equal(act, z.relu()) and torch.equal(swish(z, F32).double(), act)
            hid = act * k1
            out["z"] = _buf(_second_tile(z, c, mut), c["F"], mut)
            if not c.get("sat") and with_aux and mut is None:
                aux["gap"]["hid"] = float(((swish(z, F32).double() - act) * k1).abs().max())
        hid_out = hid
        if e == "ffn_swish_train_f16" and not c.get("sat"):
            hid = hid.to(F16).double() if a16 is None else a16[:M].double()
        sum_bound(hid, o["W2"], o["b2"])
        k2 = keep2(rows, 256, o["drop2_seed"], c.get("drop2"), mut, 128)
        y = (hid @ o["W2"].t() + o["b2"]) * k2 * c["alpha"] + o["res"]
        assert float(y.abs().max()) * 2 < LIMIT
        if e == "ffn_swish_train_f16" and not c.get("sat") and with_aux and mut is None:
            y32 = (hid.float() @ o["W2"].float().t() + o["b2"].float()) * k2.float() * c["alpha"] + o["res"].float()
            aux["y_gap"] = float((y32.double() - y).abs().max())
        out["hid"] = _buf(_second_tile(hid_out, c, mut), c["F"], mut)
        out.update(_normed(c, o, _second_tile(y, c, mut), mut, aux, unnorm=bool(c.get("unnorm")), with_gap=with_aux,
                           stream_exact=(e == "ffn_train_f16" or bool(c.get("sat")))))
    elif fam == "ffnbwd":
        sum_bound(o["A"], o["W"])
        d = _product(o["A"], o["W"], kmut)
        scale = 1.0 if mut == "drop_scale_missing" else c["scale"]
        dH = torch.where(is_zero16(o["act"], mut), torch.zeros_like(d), d * scale)
        sum_bound(dH, o["W2"], o["res"])
        g = dH @ o["W2"].t() + o["res"]
        out["dH"], out["g"] = _buf(_second_tile(dH, c, mut), c["F"], mut), _buf(_second_tile(g, c, mut), 256, mut)
    if mut is None:
        for name, kind in exact_outputs(c).items():
            if kind in (F16, BF16) and name in out:
                as16(out[name], kind)                    # guard (b)
    return (out, aux) if with_aux else out


def _normed(c, o, y, mut, aux, unnorm, with_gap=True, stream_exact=True):
    """the LayerNorm outputs of the rows y: out32 (the stream itself in the un-normalised form), out16, xhat, rstd"""
    p64 = _norm_parts(y, o["gamma"], o["beta"], F64)
    if mut is None:
        layer_norm(y, o["gamma"], o["beta"], EPS)        # asserts non-zero variance in every row
    if mut is None and with_gap:
        p32 = _norm_parts(y, o["gamma"], o["beta"], F32)
        aux["gap"].update(xhat=_gap(p64, p32)["xhat"], rstd=_gap(p64, p32, rel=True)["rstd"])
        if unnorm and not stream_exact:                  # behind an unsaturated Swish the stream is not exact: y itself, evaluated in fp32
            aux["gap"]["out32"] = aux["y_gap"]
    return {"out32": _buf(y if unnorm else p64["ln"], 256, mut), "out16": _buf(p64["ln"], 256, mut),
            "xhat": _buf(p64["xhat"], 256, mut), "rstd": _buf(p64["rstd"], 0, mut)}


def exact_outputs(c):
    """name -> dtype of the outputs compared bit for bit; the others go through tolerance()"""
    fam, e = FAMILY[c["entry"]], c["entry"]
    if fam == "g128":
        return {"out": F16 if e == "linear_relu_train_f16" else BF16}
    if fam == "acc":
        return {"out32": F32, "out16": BF16}
    if fam == "lnbwd":
        return {"dgamma": F32, "dbeta": F32, "dbias": F32}
    if fam == "dgrad":
        return {"out32": F32}
    if fam == "resln":
        return {"out32": F32} if e == "linear_res_scale_ln_train_f16" else {}
    if fam == "heads":
        return {k: BF16 for k in ("Q", "K", "V", "Qt", "Kt", "Vt")}
    if fam == "ffn":
        if e == "ffn_train_f16":
            return {"hid": F16}
        ex = {"z": F16}
        if c.get("sat"):
            ex["hid"] = F16
            if c.get("unnorm"):
                ex["out32"] = F32
        return ex
    if fam == "ffnbwd":
        return {"dH": BF16, "g": F32}
    return {}


def tolerance(c, name):
    """TOL key of an output that is not bitwise"""
    fam = FAMILY[c["entry"]]
    if fam == "lnbwd":
        return name                                      # ds32 / ds16
    if fam == "l2train":
        return {"out32": "l2_32", "out16": "l2_16", "inv_norm": "gap32"}[name]
    if name == "out32" and c.get("unnorm"):              # the un-normalised stream behind an unsaturated Swish
        return "gap32"
    return {"out32": "ln32", "out16": "ln16", "xhat": "gap16", "rstd": "gap32", "hid": "gap16"}[name]


def ulp16(v):
    """the spacing of f16 at |v| (float64 tensor)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - 10)


ROW_SCALARS = ("rstd", "inv_norm")     # one f32 per row: gap32 relative to the reference value, pooled over the entry's table


@functools.lru_cache(maxsize=None)
def pooled_gap(entry, name, ncu=NCU_MI355X):
    """gap32 of a per-row f32 scalar (1/sigma, 1/||x||): the largest RELATIVE error of the CPU fp32 evaluation over the rows of every
    tabled case of the entry.  A case's own rows are too few to measure it: an f32 result has two neighbours around the float64 value,
    the fp32 evaluation of ONE row (the M = 1 cases) lands on the near one (0.04 ulp) or the far one (0.96 ulp) depending on the host
    CPU's summation order -- the same row gave 1.6e-13 on one host and 3.8e-12 on another -- and the rows of one case differ in
    magnitude by orders (1/sigma of a saturated Swish row against a residual-only row).  Over the table's rows it is about one ulp."""
    return max(aux_of(resolve(c, ncu))["gap"][name] for c in cases_of(entry))


def compare(c, name, got, want, aux):
    """(ok, max error, bound at the worst element) of one output buffer under the comparison of the GPU test: bitwise (up to the sign of
    zero) where the output is exact, TOL elsewhere; NaN must sit exactly where the reference has it"""
    got, want = got.double().reshape(want.shape), want.double()
    if name in exact_outputs(c):
        return same(got, want), (0.0 if same(got, want) else float((got - want).abs().nan_to_num(1.0).max())), 0.0
    if not torch.equal(got.isnan(), want.isnan()):
        return False, NAN, NAN
    kind, atol, rtol = TOL[tolerance(c, name)][:3]
    live = ~want.isnan()
    err, w = (got[live] - want[live]).abs(), want[live]
    if kind == "elem":
        bound = atol + rtol * w.abs()
    elif kind == "scale":
        bound = torch.full_like(w, rtol * aux["scale"][name])
    elif name in ROW_SCALARS:
        bound = rtol * pooled_gap(c["entry"], name, c.get("ncu", NCU_MI355X)) * w.abs()
    else:
        bound = rtol * aux["gap"][name] + atol * ulp16(w)
    return bool((err <= bound).all()), float(err.max()), float(bound[err.argmax()] if bound.numel() else 0.0)


# ------------------------------------------------------------------------------------------------ the case tables
M128, M64 = (1, 127, 128, 129, 257), (1, 63, 64, 65, 129)


def g128_cases():
    shapes = [(M, 128, 64, {}) for M in M128] + [(M, 384, 256, {}) for M in M128]
    shapes += [(129, 128, 320, {}), (257, 384, 320, {}), (129, 128, 768, {}), (128, 384, 768, {}), (127, 2048, 256, {}), (1, 2048, 320, {}),
               (257, 2048, 64, {}),
               (129, 128, 64, dict(lda=72, ldw=80, ldo=136, ldact=144)), (257, 384, 256, dict(lda=264, ldw=272, ldo=392, ldact=384)),
               (127, 128, 320, dict(lda=328, ldw=320, ldo=128, ldact=136)), (130, 384, 768, dict(lda=776, ldw=784, ldo=400, ldact=392))]
    cs = []
    for i, (M, N, K, ld) in enumerate(shapes):
        base = dict(M=M, N=N, K=K, lda=ld.get("lda", K), ldw=ld.get("ldw", K), ldo=ld.get("ldo", N))
        cs.append(dict(base, entry="gemm_bf16", bias=i % 2))
        cs.append(dict(base, entry="gemm_relu_bwd_bf16", ldact=ld.get("ldact", N), scale=(2.0, 1.0, 4.0)[i % 3]))
        cs.append(dict(base, entry="linear_relu_train_f16", bias=1, drop=(i + 1) % 2))
    cs.append(dict(entry="linear_relu_train_f16", M=257, N=384, K=256, lda=256, ldw=256, ldo=384, bias=0, drop=1))
    cs.append(dict(entry="linear_relu_train_f16", M=257, N=128, K=320, lda=320, ldw=320, ldo=128, bias=1, drop=1))
    return cs


def acc_cases():
    modes = [dict(out32=1, out16=0, alias=0), dict(out32=0, out16=1, alias=0), dict(out32=1, out16=1, alias=0), dict(out32=1, out16=0, alias=1),
             dict(out32=1, out16=1, alias=1)]
    cs, i = [], 0
    for K in (64, 256, 2048):
        for M in M64:
            cs.append(dict(entry="gemm_acc_bf16", M=M, K=K, lda=K, ldw=K, res=1, alpha=(1.0, 0.5, 2.0)[i % 3], **modes[i % 5]))
            i += 1
    cs += [dict(entry="gemm_acc_bf16", M=65, K=64, lda=72, ldw=80, res=1, alpha=1.0, out32=1, out16=1, alias=0),
           dict(entry="gemm_acc_bf16", M=129, K=256, lda=264, ldw=256, res=0, alpha=2.0, out32=1, out16=1, alias=0),
           dict(entry="gemm_acc_bf16", M=63, K=320, lda=320, ldw=328, res=0, alpha=1.0, out32=0, out16=1, alias=0)]
    return cs


def lnbwd_cases():
    cs, i = [], 0
    for K in (64, 256, 2048):
        for M in M64:
            cs.append(dict(entry="gemm_acc_lnbwd_bf16", M=M, K=K, lda=K, ldw=K, drop=i % 2, dbias=int(i % 3 != 2), alias=int(i % 4 == 1)))
            i += 1
    cs += [dict(entry="gemm_acc_lnbwd_bf16", M=65, K=64, lda=72, ldw=80, drop=1, dbias=1, alias=0),
           dict(entry="gemm_acc_lnbwd_bf16", M=129, K=320, lda=328, ldw=320, drop=1, dbias=1, alias=1),
           dict(entry="gemm_acc_lnbwd_bf16", M=191, K=256, lda=256, ldw=264, drop=0, dbias=1, alias=0)]
    return cs


def resln_cases():
    cs, i = [], 0
    for e in ("linear_res_ln_train_f16", "linear_res_scale_ln_train_f16"):
        for K in (64, 256, 2048):
            for M in M64:
                cs.append(dict(entry=e, M=M, K=K, lda=K, ldw=K, bias=int(i % 4 != 3), res=int(i % 5 != 4), alpha=(1.0, 0.5, 2.0)[i % 3],
                               drop=i % 2, alias=int(i % 3 == 0 and i % 5 != 4)))
                i += 1
        cs += [dict(entry=e, M=65, K=64, lda=72, ldw=80, bias=1, res=1, alpha=1.0, drop=1, alias=0),
               dict(entry=e, M=129, K=320, lda=328, ldw=336, bias=1, res=1, alpha=0.5, drop=1, alias=1)]
    return cs


CONV_SHAPES = ((1, 64), (3, 64), (2, 128))
CONV_TAPS = ((1, 0), (3, 0), (3, 2), (19, 9))


def _lens(nseq, Tp, i):
    pool = (Tp, Tp - 1, 1)
    return [pool[(i + s) % 3] for s in range(nseq)]


def dgrad_cases():
    cs, i = [], 0
    for nseq, Tp in CONV_SHAPES:
        for ktaps, pad in CONV_TAPS:
            lens = _lens(nseq, Tp, i)
            mlens = [(0, l, max(l - 3, 0))[(i + s + 1) % 3] for s, l in enumerate(lens)]
            cs.append(dict(entry="conv1d_dgrad_bf16", nseq=nseq, Tp=Tp, ktaps=ktaps, pad=pad, lens=lens, mlens=mlens))
            i += 1
    cs.append(dict(entry="conv1d_dgrad_bf16", nseq=3, Tp=64, ktaps=19, pad=9, lens=[64, 64, 64], mlens=[64, 61, 0]))
    cs.append(dict(entry="conv1d_dgrad_bf16", nseq=2, Tp=128, ktaps=3, pad=2, lens=[127, 128], mlens=[124, 128]))
    return cs


def l2train_cases():
    cs, i = [], 0
    for cin in (64, 256):
        for nseq, Tp in CONV_SHAPES:
            for ktaps, pad in CONV_TAPS:
                cs.append(dict(entry="conv1d_l2norm_train_f16", nseq=nseq, Tp=Tp, cin=cin, ktaps=ktaps, pad=pad, lens=_lens(nseq, Tp, i)))
                i += 1
    return cs


def heads_cases():
    cs = []
    for nseq, Tp in ((1, 64), (3, 64), (2, 192)):
        for xt in ("all", "v"):
            cs.append(dict(entry="inproj_heads_train_bf16", nseq=nseq, Tp=Tp, lda=256, xt=xt))
    cs += [dict(entry="inproj_heads_train_bf16", nseq=3, Tp=64, lda=320, xt="all"), dict(entry="inproj_heads_train_bf16", nseq=2, Tp=192, lda=264, xt="v")]
    return cs


def ffn_cases():
    cs, i = [], 0
    for F in (64, 128, 2048):
        for M in M128:
            v = dict(M=M, F=F, ldx=256, alpha=(1.0, 0.5, 2.0)[i % 3], alias=int(i % 3 == 1))
            cs.append(dict(v, entry="ffn_train_f16", drop=i % 2, drop2=(i // 2) % 2))
            cs.append(dict(v, entry="ffn_swish_train_f16", drop=(i + 1) % 2, drop2=i % 2, unnorm=i % 2, sat=1))
            cs.append(dict(entry="ffn_bwd_data_bf16", M=M, F=F, ldx=256, scale=(2.0, 1.0)[i % 2]))
            i += 1
    cs += [dict(entry="ffn_train_f16", M=129, F=128, ldx=320, alpha=1.0, alias=0, drop=1, drop2=1),
           dict(entry="ffn_swish_train_f16", M=129, F=64, ldx=264, alpha=1.0, alias=0, drop=1, drop2=1, unnorm=1, sat=1),
           dict(entry="ffn_bwd_data_bf16", M=129, F=128, ldx=264, scale=2.0),
           # an unsaturated Swish (z = X W1^T + b1 as it falls): a_f16 through its tolerance, the second product from the kernel's own a_f16
           dict(entry="ffn_swish_train_f16", M=129, F=64, ldx=256, alpha=1.0, alias=0, drop=0, drop2=0, unnorm=0, sat=0),
           dict(entry="ffn_swish_train_f16", M=257, F=128, ldx=256, alpha=1.0, alias=0, drop=1, drop2=0, unnorm=1, sat=0),
           # persistent grid: M = 128 ncu + 129, one workgroup takes a second tile and the last tile is ragged
           dict(entry="ffn_train_f16", M=None, F=64, ldx=256, alpha=1.0, alias=1, drop=1, drop2=1, persist=1),
           dict(entry="ffn_swish_train_f16", M=None, F=64, ldx=256, alpha=1.0, alias=0, drop=1, drop2=1, unnorm=1, sat=1, persist=1),
           dict(entry="ffn_bwd_data_bf16", M=None, F=64, ldx=256, scale=2.0, persist=1)]
    return cs


# each returns EEND_EINVAL and leaves its NaN-filled outputs untouched: (entry, argument overrides on a small legal call, why)
REFUSALS = [
    ("gemm_bf16", dict(K=72, lda=72, ldw=72), "K % 64"), ("gemm_bf16", dict(N=192, ldo=192), "N % 128"), ("gemm_bf16", dict(ldo=132), "ldo & 7"),
    ("gemm_bf16", dict(lda=68), "lda & 7"),
    ("gemm_relu_bwd_bf16", dict(K=96, lda=96, ldw=96), "K % 64"), ("gemm_relu_bwd_bf16", dict(N=64, ldo=64, ldact=64), "N % 128"),
    ("gemm_relu_bwd_bf16", dict(ldo=132), "ldo & 7"), ("gemm_relu_bwd_bf16", dict(ldact=132), "ldact & 7"), ("gemm_relu_bwd_bf16", dict(lda=68), "lda & 7"),
    ("linear_relu_train_f16", dict(K=72, lda=72, ldw=72), "K % 64"), ("linear_relu_train_f16", dict(N=192, ldo=192), "N % 128"),
    ("linear_relu_train_f16", dict(ldo=132), "ldo & 7"), ("linear_relu_train_f16", dict(lda=68), "lda & 7"),
    ("gemm_acc_bf16", dict(K=72, lda=72, ldw=72), "K % 64"), ("gemm_acc_bf16", dict(lda=68), "lda & 7"), ("gemm_acc_bf16", dict(out32=0, out16=0), "both outputs NULL"),
    ("gemm_acc_lnbwd_bf16", dict(K=72, lda=72, ldw=72), "K % 64"), ("gemm_acc_lnbwd_bf16", dict(lda=68), "lda & 7"),
    ("gemm_acc_lnbwd_bf16", dict(ws_short=1), "one workspace float short of ceil(M/64) * 768"),
    ("linear_res_ln_train_f16", dict(K=72, lda=72, ldw=72), "K % 64"), ("linear_res_ln_train_f16", dict(lda=68), "lda & 7"),
    ("linear_res_scale_ln_train_f16", dict(K=72, lda=72, ldw=72), "K % 64"), ("linear_res_scale_ln_train_f16", dict(lda=68), "lda & 7"),
    ("conv1d_dgrad_bf16", dict(ktaps=3, pad=3), "pad >= ktaps"), ("conv1d_dgrad_bf16", dict(Tp=96), "Tp % 64"),
    ("conv1d_l2norm_train_f16", dict(ktaps=3, pad=3), "pad >= ktaps"), ("conv1d_l2norm_train_f16", dict(Tp=96), "Tp % 64"),
    ("inproj_heads_train_bf16", dict(H=2), "H != 4"), ("inproj_heads_train_bf16", dict(H=8), "H != 4"), ("inproj_heads_train_bf16", dict(lda=260), "lda & 7"),
    ("ffn_train_f16", dict(F=96), "F % 64"), ("ffn_swish_train_f16", dict(F=96), "F % 64"),
    ("ffn_bwd_data_bf16", dict(g_off=4), "g_f32 not 16-byte aligned"), ("ffn_bwd_data_bf16", dict(F=96), "F % 64"),
]


def all_cases():
    return g128_cases() + acc_cases() + lnbwd_cases() + resln_cases() + dgrad_cases() + l2train_cases() + heads_cases() + ffn_cases()


def cases_of(*entries):
    return [c for c in all_cases() if c["entry"] in entries]


_BY_ID = {}
for _c in all_cases():
    assert case_id(_c) not in _BY_ID, case_id(_c)
    _BY_ID[case_id(_c)] = _c
