"""Constructions, exact references and case tables for the linear entry points of csrc/api.hip (no GPU needed).

Every entry computes y = A W^T (+ bias) on f32 accumulators and finishes with an epilogue.  With small-integer operands, integer bias /
residual / slot constants and power-of-two alphas, every f32 partial sum of every summation order is an exact integer below 2^24, so
the linear part of every epilogue has ONE right answer in bits whatever kernel, tile, k-split or wave order produced it: a k-tile
dropped or doubled, rows shifted by one, Q and K swapped, a transposed head layout ... changes those bits (MUTATIONS;
tests/test_linear_edges_ref.py shows it on the CPU for every tabled case).  Two guards are asserted on the inputs and references of every
case, never on a kernel's output:
  (a) max_{m,n} sum_k |A||W| + |bias| + |res| (+ |pc|) < 2^24                          (assert_exact)
  (b) every reference value that lands in a 2-byte output is exactly representable there    (reference() -> as16)
Values that pass through exp / rsqrt / sigmoid (Swish, unsaturated GLU, LayerNorm, L2 norm) are compared with the tolerances the
project already uses for those entries (TOL), against float64 computed from the exact rows; every such row must have non-zero
variance / norm (asserted here).

reference(c) returns the expected contents of every OUTPUT BUFFER of a case, guard rows and guard columns included, as float64 with
NaN where nothing may be written (the GPU test pre-fills with NaN).  The tables at the bottom tag every case with the route
(eend_linear_route) it was written for."""
import functools
import zlib

import torch

F16, BF16, F32, I64, F64 = torch.float16, torch.bfloat16, torch.float32, torch.int64, torch.float64
LIMIT = 1 << 24
NAN = float("nan")
V1, V2, V3 = (-1, 1), (-2, -1, 1, 2), (-3, -2, -1, 1, 2, 3)
GUARD_ROWS = 3                       # NaN rows behind row M of every row-major output
PAD_FILL = 3                         # operand columns between K and lda / ldw: non-zero, so that reading them shows
GLU_SATURATED = 1024                 # |gate bias| of the saturated GLU cases: sigmoid is exactly 0 or 1 in f32

# route names = fs_eend_amd.lib.ROUTES (EEND_ROUTE_* of include/eend_hip.h); entries = lib.LINEAR_ENTRIES
ROUTES_OF_ENTRY = {
    "linear_f16": {"skinny", "skinny_splitk", "proj", "gemm128_straight", "gemm128_looped", "refused"},
    "linear_glu_f16": {"skinny", "skinny_splitk", "gemm128_straight", "gemm128_looped", "refused"},
    "inproj_heads_bf16": {"proj", "gemm128_straight", "gemm128_looped", "refused"},
    "retention_proj_f16": {"proj", "gemm128_straight", "gemm128_looped", "refused"},
    "linear_res_ln_f16": {"skinny", "skinny_splitk", "gemm64x256", "refused"},
    "linear_res16_ln_f16": {"gemm64x256", "refused"},
    "linear_res_scale_f16": {"skinny", "skinny_splitk", "gemm64x256", "refused"},
    "linear_res_scale_ln16_f16": {"skinny", "skinny_splitk", "gemm64x256", "refused"},
    "convert_fanout_f16": {"convert_rows", "gemm64x256", "refused"},
    "linear_step_f32": {"skinny", "skinny_splitk", "skinny_rowgroups", "skinny_rowgroups_splitk", "f32_mfma", "f32_mfma_splitk", "refused"},
    "linear_res_ln_step_f32": {"skinny", "skinny_splitk", "skinny_rowgroups", "skinny_rowgroups_splitk", "f32_mfma", "f32_mfma_splitk",
                               "refused"},
    "linear_res_scale_ln_step_f32": {"skinny", "skinny_splitk", "skinny_rowgroups", "skinny_rowgroups_splitk", "f32_mfma",
                                     "f32_mfma_splitk", "refused"},
}
FAMILY = {"linear_f16": "plain", "linear_step_f32": "plain", "linear_glu_f16": "glu", "inproj_heads_bf16": "heads",
          "retention_proj_f16": "heads", "linear_res_ln_f16": "res", "linear_res16_ln_f16": "res", "linear_res_scale_f16": "res",
          "linear_res_scale_ln16_f16": "res", "linear_res_ln_step_f32": "res", "linear_res_scale_ln_step_f32": "res",
          "convert_fanout_f16": "fanout", "conv1d_l2norm_f16": "conv"}

# (atol, rtol) against the float64 reference, for values behind exp / rsqrt / sigmoid -- the bounds of the existing tests of the same
# entries: tests/test_hip_kernels.py (f16 entries: test_linear_swish, test_linear_glu, test_linear_res_ln, test_conv1d_l2norm),
# tests/test_skinny.py (skinny forms: max-norm bounds), tests/test_ls_streaming.py::test_f32_frame_step_entries_vs_torch (f32 steps:
# relative to max |want|).  "max" bounds are atol + rtol * max |want|, the others atol + rtol * |want| per element.
TOL = {
    "act16": ("elem", 2e-3, 2e-3), "act16_skinny": ("max", 2e-3, 1e-3),
    "ln32": ("elem", 2e-4, 2e-4), "ln16": ("elem", 3e-3, 2e-3),
    "ln32_skinny": ("max", 3e-3, 0.0), "ln16_skinny": ("max", 6e-3, 0.0),
    "l2_32": ("elem", 2e-4, 1e-3), "l2_16": ("elem", 1e-3, 2e-3),
    "ln32_step": ("max", 0.0, 5e-6), "ln16_step": ("max", 0.0, 2e-3), "act32_step": ("max", 2e-6, 2e-6),
}


# ------------------------------------------------------------------------------------------------ operands
def ints(shape, seed, vals=V2):
    """float64 tensor of integers drawn from `vals` (non-zero: a lost row or k-tile must show)"""
    g = torch.Generator().manual_seed(seed)
    v = torch.tensor(vals, dtype=F64)
    return v[torch.randint(0, len(vals), tuple(shape), generator=g)]


def as16(t, dtype):
    """float64 -> f16 / bf16 (NaN kept), asserting that nothing is rounded: guard (b)"""
    r = t.to(dtype)
    assert torch.equal(r.double().nan_to_num(0.0), t.nan_to_num(0.0)), f"not exact in {dtype}"
    return r


def assert_exact(A, W, *adds):
    """guard (a): every f32 partial sum of sum_k A[m][k] W[n][k] plus the additive terms is an exact integer below 2^24"""
    extra = sum(float(x.abs().max()) for x in adds if x is not None)
    bound = float(A.abs().max()) * float(W.abs().max()) * A.shape[1]
    if bound + extra >= LIMIT:
        bound = float((A.abs() @ W.abs().t()).max())
    assert bound + extra < LIMIT, (bound, extra)
    for x in (A, W) + tuple(a for a in adds if a is not None):
        assert (x != 0).all(), "operands are non-zero"
    return bound + extra


def _seed(c):
    return zlib.crc32(case_id(c).encode()) & 0x7FFFFFFF


def case_id(c):
    keys = ("M", "N", "K", "lda", "ldw", "ldo", "act", "bias", "nseq", "Tp", "H", "C", "B", "cin", "ktaps", "pad", "ilens", "res", "alpha",
            "gamma", "out32", "out16", "alias", "sat", "bias_off", "why")
    parts = [c["entry"], c["route"]]
    for k in keys:
        if k in c and c[k] is not None:
            v = c[k]
            parts.append(f"{k}{'x'.join(map(str, v)) if isinstance(v, (list, tuple)) else v}")
    return "-".join(parts)


@functools.lru_cache(maxsize=None)
def _operands(cid):
    c = _BY_ID[cid]
    s, fam, vals = _seed(c), FAMILY[c["entry"]], c.get("vals", V2)
    o = {}
    if fam == "plain":
        o["A"], o["W"] = ints((c["M"], c["K"]), s, vals), ints((c["N"], c["K"]), s + 1, vals)
        o["bias"] = ints((c["N"],), s + 2, V3) if c["bias"] else None
    elif fam == "glu":
        o["A"], o["W"] = ints((c["M"], c["K"]), s, vals), ints((c["N"], c["K"]), s + 1, vals)
        o["bias"] = ints((c["N"],), s + 2, V3)
        if c["sat"]:                                    # gate rows (odd): far beyond where sigmoid differs from 0 / 1 in f32
            o["bias"][1::2] = ints((c["N"] // 2,), s + 3, V1) * GLU_SATURATED
    elif fam == "heads":
        D = c["H"] * 64
        nout = 3 * D if c["entry"] == "inproj_heads_bf16" else 4 * D
        o["A"], o["W"] = ints((c["nseq"] * c["Tp"], c["K"]), s, vals), ints((nout, c["K"]), s + 1, vals)
        o["bias"] = ints((nout,), s + 2, V3)
    elif fam == "res":
        o["A"], o["W"] = ints((c["M"], c["K"]), s, vals), ints((256, c["K"]), s + 1, vals)
        o["bias"] = ints((256,), s + 2, V3) if c["bias"] else None
        o["res"] = ints((c["M"], 256), s + 3, V3) * 4 if c["res"] else None
        g = torch.Generator().manual_seed(s + 4)
        o["gamma"] = 1.0 + torch.randint(-4, 5, (256,), generator=g).double() / 16 if c["gamma"] else None
        o["beta"] = torch.randint(-8, 9, (256,), generator=g).double() / 16 if c["gamma"] else None
    elif fam == "fanout":
        o["A"], o["W"] = ints((c["B"] * c["Tp"], 256), s, vals), ints((256, 256), s + 1, vals)
        o["pc"] = ints((c["C"], 256), s + 2, V3) * 8
    elif fam == "conv":
        o["A"] = ints((c["nseq"] * c["Tp"], c["cin"]), s, V1)              # raw X: non-zero beyond ilens too, the kernel must mask
        o["W"] = ints((256, c["ktaps"] * c["cin"]), s + 1, V1)
        o["bias"] = ints((256,), s + 2, V3)
    return o


def operands(c):
    """the case's operands as float64 CPU tensors (computed once per case, never modified): A, W, bias | None, ..."""
    return _operands(case_id(c))


# ------------------------------------------------------------------------------------------------ mutations
# one-step mistakes a linear kernel can make; reference(c, mut) gives the buffers such a kernel would leave
MUTATIONS = ("ktile_dropped", "ktile_doubled", "rows_shifted", "qk_swapped", "head_layout_transposed", "seq_from_tile_row",
             "slot_of_neighbour", "conv_tap_across_sequences", "conv_ignores_ilen", "tail_row_from_clamp", "glu_halves_not_pairs")


def applies(mut, c):
    fam = FAMILY[c["entry"]]
    M = c.get("M") or c.get("nseq", c.get("B", 0)) * c["Tp"]
    if mut in ("ktile_dropped", "ktile_doubled"):
        return True
    if mut == "rows_shifted":
        return M >= 2
    if mut == "qk_swapped":
        return fam == "heads"
    if mut == "head_layout_transposed":
        return fam == "heads"
    if mut == "seq_from_tile_row":                       # a 128-row tile straddles two sequences
        return fam == "heads" and c["Tp"] == 64 and c["nseq"] >= 2
    if mut == "slot_of_neighbour":
        return fam == "fanout" and c["C"] >= 2
    if mut == "conv_tap_across_sequences":
        return fam == "conv" and c["pad"] > 0 and c["nseq"] >= 2
    if mut == "conv_ignores_ilen":
        return fam == "conv" and any(l < c["Tp"] for l in c["ilens"])
    if mut == "tail_row_from_clamp":
        return fam != "heads"
    if mut == "glu_halves_not_pairs":
        return fam == "glu"
    raise KeyError(mut)


# ------------------------------------------------------------------------------------------------ the references
def _ktile(c):
    K = c["ktaps"] * c["cin"] if FAMILY[c["entry"]] == "conv" else c.get("K", 256)
    return K, (64 if K >= 64 else 8)


def _product(c, o, mut, A=None):
    """exact y = A W^T (+ bias) as float64 integers; k-tile and row mutations applied"""
    A, W = o["A"] if A is None else A, o["W"]
    K, kt = _ktile(c)
    if mut == "ktile_dropped":
        W = W.clone(); W[:, K - kt:] = 0
    elif mut == "ktile_doubled":
        W = W.clone(); W[:, K - kt:] *= 2
    y = A @ W.t()
    if o.get("bias") is not None:
        y = y + o["bias"]
    if mut == "rows_shifted":
        y = torch.roll(y, 1, 0)
    return y


def _rows_buffer(y, ldo, mut, guard=GUARD_ROWS):
    """[M][N] rows -> the [M + guard][ldo] output buffer, NaN in the guard rows and guard columns"""
    M, N = y.shape
    buf = torch.full((M + guard, ldo), NAN, dtype=F64)
    buf[:M, :N] = y
    if mut == "tail_row_from_clamp":
        buf[M, :N] = y[M - 1]
    return buf


def layer_norm(y, gamma, beta, eps):
    mu = y.mean(1, keepdim=True)
    var = ((y - mu) ** 2).mean(1, keepdim=True)
    assert (var > 0).all(), "a reference row with zero variance must not decide a case"
    x = (y - mu) / torch.sqrt(var + eps)
    return x * gamma + beta if gamma is not None else x


def _head_rows(y, nseq, Tp, H, mut):
    """[M][H*64] -> [nseq][H][Tp][64]"""
    if mut == "head_layout_transposed":
        return y.reshape(nseq, Tp, H, 64).permute(0, 2, 3, 1).reshape(nseq, H, Tp, 64)
    if mut == "seq_from_tile_row":
        out = torch.full((nseq, H, Tp, 64), NAN, dtype=F64)
        rows = torch.arange(nseq * Tp)
        seq, t = (rows // 128 * 128) // Tp, rows % Tp
        for r in range(nseq * Tp):
            out[seq[r], :, t[r]] = y[r].view(H, 64)
        return out
    return y.reshape(nseq, Tp, H, 64).permute(0, 2, 1, 3).contiguous()


def _head_rows_t(y, nseq, Tp, H, mut):
    """[M][H*64] -> [nseq][H][64][Tp]"""
    if mut == "head_layout_transposed":
        return y.reshape(nseq, Tp, H, 64).permute(0, 2, 1, 3).reshape(nseq, H, 64, Tp)
    return _head_rows(y, nseq, Tp, H, mut).transpose(2, 3).contiguous()


def conv_columns(c, X, mut=None):
    """im2col of the look-ahead Conv1d as its definition: output frame t meets, for tap j, frame t + j - pad of the SAME sequence, zero
    outside [0, ilen) (the reference model truncates to ilen and zero-pads)."""
    nseq, Tp, cin, ktaps, pad = c["nseq"], c["Tp"], c["cin"], c["ktaps"], c["pad"]
    M = nseq * Tp
    rows = torch.arange(M)
    seq, t = rows // Tp, rows % Tp
    il = torch.tensor(c["ilens"])[seq]
    cols = torch.zeros(M, ktaps, cin, dtype=F64)
    for j in range(ktaps):
        ts = t + j - pad
        hi = torch.full_like(il, Tp) if mut == "conv_ignores_ilen" else il
        ok = (ts >= 0) & (ts < hi)
        src = seq * Tp + ts
        if mut == "conv_tap_across_sequences":           # lower bound forgotten: frames before the slab come from the neighbour's tail
            ok = (src >= 0) & (ts < hi)
        cols[ok, j] = X[src[ok]]
    return cols.view(M, ktaps * cin)


def reference(c, mut=None):
    """name -> expected output buffer (float64, NaN = untouched) of case c; mut: the buffers a kernel with that mistake would leave"""
    o, fam, e = operands(c), FAMILY[c["entry"]], c["entry"]
    out = {}
    if fam == "plain":
        assert_exact(o["A"], o["W"], o["bias"])
        y = _product(c, o, mut)
        if c["act"] == 1:
            y = y.relu()
        elif c["act"] == 2:
            y = y * torch.sigmoid(y)
        out["out"] = _rows_buffer(y, c["ldo"], mut)
    elif fam == "glu":
        assert_exact(o["A"], o["W"], o["bias"])
        y = _product(c, o, mut)
        v, g = (y[:, :c["N"] // 2], y[:, c["N"] // 2:]) if mut == "glu_halves_not_pairs" else (y[:, 0::2], y[:, 1::2])
        r = v * torch.sigmoid(g)
        if c["sat"] and mut is None:                     # sigmoid is exactly 0 or 1: the pairing of value and gate rows is bitwise
            assert (g.abs() > 100).all() and torch.equal(r, torch.where(g > 0, v, torch.zeros_like(v)))
        out["out"] = _rows_buffer(r, c["ldo"], mut)
    elif fam == "heads":
        assert_exact(o["A"], o["W"], o["bias"])
        nseq, Tp, H = c["nseq"], c["Tp"], c["H"]
        D = H * 64
        oo = o
        if mut == "qk_swapped":
            oo = dict(o, W=torch.cat([o["W"][D:2 * D], o["W"][:D], o["W"][2 * D:]]), bias=torch.cat([o["bias"][D:2 * D], o["bias"][:D], o["bias"][2 * D:]]))
        y = _product(c, oo, mut)
        out["Q"], out["K"] = _head_rows(y[:, :D], nseq, Tp, H, mut), _head_rows(y[:, D:2 * D], nseq, Tp, H, mut)
        out["Vt"] = _head_rows_t(y[:, 2 * D:3 * D], nseq, Tp, H, mut)
        if e == "retention_proj_f16":
            out["Kt"] = _head_rows_t(y[:, D:2 * D], nseq, Tp, H, mut)
            out["G"] = y[:, 3 * D:].clone()
    elif fam == "res":
        assert_exact(o["A"], o["W"], o["bias"], o["res"])
        y = _product(c, o, mut) * c["alpha"]
        if o["res"] is not None:
            y = y + o["res"]
        assert float(y.abs().max()) < LIMIT
        scale_only = e == "linear_res_scale_f16"
        ln = None if scale_only else layer_norm(y, o["gamma"], o["beta"], c["eps"])
        if e in ("linear_res_ln_f16", "linear_res16_ln_f16", "linear_res_ln_step_f32"):
            rows32, rows16 = ln, ln
        elif scale_only:
            rows32, rows16 = y, y
        else:                                            # res_scale_ln16 / res_scale_ln_step: un-normalised stream + LayerNorm of it
            rows32, rows16 = y, ln
        if c["out32"]:
            out["out32"] = _rows_buffer(rows32, 256, mut)
        if c["out16"]:
            out["out16"] = _rows_buffer(rows16, 256, mut)
        if e == "linear_res_scale_ln_step_f32":
            out["ln32"] = _rows_buffer(ln, 256, mut)
    elif fam == "fanout":
        assert_exact(o["A"], o["W"], o["pc"])
        B, Tp, C = c["B"], c["Tp"], c["C"]
        y = _product(c, o, mut).view(B, 1, Tp, 256)
        pc = torch.roll(o["pc"], -1, 0) if mut == "slot_of_neighbour" else o["pc"]
        rows = (y + pc.view(1, C, 1, 256)).reshape(B * C * Tp, 256)
        out["out16"] = _rows_buffer(rows, 256, mut)
        if c["out32"]:
            out["out32"] = _rows_buffer(rows, 256, mut)
    elif fam == "conv":
        cols = conv_columns(c, o["A"], mut)
        assert_exact(torch.ones_like(cols), o["W"], o["bias"])           # |cols| <= 1 (zeros where masked)
        y = _product(c, o, mut, A=cols)
        nrm = torch.linalg.vector_norm(y, dim=1, keepdim=True)
        assert (nrm > 0).all(), "a reference row with zero norm must not decide a case"
        out["out32"] = _rows_buffer(y / nrm, 256, mut)
        out["out16"] = _rows_buffer(y / nrm, 256, mut)
    for name, kind in exact_outputs(c).items():
        if kind in (F16, BF16) and name in out and mut is None:
            as16(out[name], kind)                        # guard (b)
    return out


def exact_outputs(c):
    """name -> dtype of the outputs that are compared bit for bit (everything that is linear); the others go through TOL"""
    fam, e = FAMILY[c["entry"]], c["entry"]
    if fam == "plain":
        return {} if c["act"] == 2 else {"out": F32 if e == "linear_step_f32" else F16}
    if fam == "glu":
        return {"out": F16} if c["sat"] else {}
    if fam == "heads":
        t = BF16 if e == "inproj_heads_bf16" else F16
        return {k: t for k in ("Q", "K", "Vt", "Kt", "G")}
    if fam == "res":
        if e == "linear_res_scale_f16":
            return {"out32": F32, "out16": F16}
        if e in ("linear_res_scale_ln16_f16", "linear_res_scale_ln_step_f32"):
            return {"out32": F32}
        return {}
    if fam == "fanout":
        return {"out32": F32, "out16": F16}
    return {}


def tolerance(c, name):
    """TOL key of an output that is not bitwise"""
    fam, e, skinny = FAMILY[c["entry"]], c["entry"], c["route"].startswith("skinny")
    if e == "linear_step_f32":
        return "act32_step"
    if fam in ("plain", "glu"):
        return "act16_skinny" if skinny else "act16"
    if fam == "conv":
        return "l2_32" if name == "out32" else "l2_16"
    if e.endswith("_step_f32"):
        return "ln16_step" if name == "out16" else "ln32_step"
    return ("ln32" if name == "out32" else "ln16") + ("_skinny" if skinny else "")


def within(got, want, tol):
    """(ok, max error, bound at the worst element): NaN must sit exactly where the reference has it"""
    kind, atol, rtol = TOL[tol]
    got, want = got.double(), want.double()
    if got.shape != want.shape or not torch.equal(got.isnan(), want.isnan()):
        return False, NAN, NAN
    live = ~want.isnan()
    err = (got[live] - want[live]).abs()
    bound = atol + rtol * (want[live].abs().max() if kind == "max" else want[live].abs())
    return bool((err <= bound).all()), float(err.max()), float(torch.as_tensor(bound).max())


def same(got, want):
    """bit for bit up to the sign of zero; NaN (the pre-fill) exactly where it is expected"""
    got, want = got.double(), want.double()
    return got.shape == want.shape and torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(0.0), want.nan_to_num(0.0))


# ------------------------------------------------------------------------------------------------ the route query's arguments
def route_fields(c, **over):
    """keyword arguments of fs_eend_amd.lib.linear_route for case c (aligned, present pointers unless the case says otherwise)"""
    fam, e = FAMILY[c["entry"]], c["entry"]
    f = {}
    if fam in ("plain", "glu"):
        f = dict(M=c["M"], N=c["N"], K=c["K"], lda=c["lda"], ldw=c["ldw"], ldo=c["ldo"], act=c.get("act", 0))
        f["bias"] = -1 if not c["bias"] else (c.get("bias_off") or 0)
    elif fam == "heads":
        f = dict(nseq=c["nseq"], Tp=c["Tp"], H=c["H"], dh=c.get("dh", 64), K=c["K"], lda=c["lda"], ldw=c["ldw"])
    elif fam == "res":
        f = dict(M=c["M"], K=c["K"], lda=c["lda"], ldw=c["ldw"], bias=0 if c["bias"] else -1, res=0 if c["res"] else -1,
                 gamma=0 if c["gamma"] else -1, beta=0 if c["gamma"] else -1, out_f32=0 if c["out32"] else -1,
                 out_f16=0 if c["out16"] else -1)
    elif fam == "fanout":
        f = dict(nseq=c["B"], Tp=c["Tp"], C=c["C"], out_f32=0 if c["out32"] else -1)
    f.update(c.get("route_over", {}))
    f.update(over)
    return f


# ------------------------------------------------------------------------------------------------ the case tables
def _plain(entry, route, M, N, K, *, lda=None, ldw=None, ldo=None, bias=True, act=0, vals=None, bias_off=0, why=None):
    vals = vals or (V1 if K > 512 else V2)
    ldo = ldo or (N + 3) // 4 * 4
    return dict(entry=entry, route=route, M=M, N=N, K=K, lda=lda or K, ldw=ldw or K, ldo=ldo, bias=bias, act=act, vals=vals,
                bias_off=bias_off or None, why=why)


def linear_f16_cases():
    L = lambda *a, **k: _plain("linear_f16", *a, **k)
    cs = []
    # skinny: every row bucket edge and one above, dead waves in the last workgroup (N = 130) and none (N = 128)
    for M in (1, 2, 3, 4, 5, 8, 9, 12, 13, 16):
        cs.append(L("skinny", M, 130 if M & 1 else 128, 64))
        cs.append(L("skinny_splitk", M, 128 if M & 1 else 130, 520))
    for K in (8, 64, 504, 512):                          # idle lanes, one full chunk, a partial last chunk
        cs.append(L("skinny", 5, 128, K, act=1))
    for K in (520, 2048, 2056):                          # one wave busy, one full round, a remainder round
        cs.append(L("skinny_splitk", 16, 130, K, why="k"))
    cs += [L("skinny", 9, 128, 64, lda=72, ldw=80, ldo=136), L("skinny_splitk", 3, 128, 1032, lda=1040, ldw=1048, ldo=132),
           L("skinny", 4, 130, 64, bias=False), L("skinny", 7, 128, 64, act=2), L("skinny_splitk", 7, 128, 520, act=2),
           L("skinny", 16, 256, 256, why="pair"), L("skinny_splitk", 6, 128, 520, bias=False, act=1)]
    # proj: every group count, rows around the 128-row tile, strided input and output rows
    for M in (17, 127, 128, 129, 300):
        cs.append(L("proj", M, 256, 256))
    for N in (512, 768, 1024):
        cs.append(L("proj", 129, N, 256))
    cs += [L("proj", 129, 512, 256, lda=320), L("proj", 127, 256, 256, ldo=264), L("proj", 300, 1024, 256, lda=320, ldo=1040)]
    # GEMM, K = 256 straight-line: reached through each condition that leaves proj
    for M in (17, 127, 128, 129, 257):
        cs.append(L("gemm128_straight", M, 256, 256, bias=False))
    cs += [L("gemm128_straight", 129, 1280, 256), L("gemm128_straight", 128, 256, 256, ldw=264), L("gemm128_straight", 257, 256, 256, act=1),
           L("gemm128_straight", 129, 256, 256, act=2), L("gemm128_straight", 130, 256, 256, ldo=264, lda=264, act=1),
           L("gemm128_straight", 17, 256, 256, why="pair", ldw=264), L("gemm128_straight", 300, 1024, 256, ldw=264, why="pair")]
    # GEMM, looped: one k-tile (empty steady state), even and odd tile counts, a long K
    for K in (64, 128, 192, 320, 2048):
        cs.append(L("gemm128_looped", 129, 256, K))
    cs += [L("gemm128_looped", 200, 128, 320, lda=328, ldw=336, ldo=136, act=1), L("gemm128_looped", 17, 128, 64, bias=False)]
    # every workgroup count 1 .. 17 through xcd_remap on both forms, and composite counts over two tile columns
    for t in range(1, 18):
        cs.append(L("gemm128_straight", 128 * t - 5, 128, 256, why=f"wg{t}"))
        cs.append(L("gemm128_looped", 128 * t - 5, 128, 128, why=f"wg{t}"))
    for t in (2, 3, 4, 5):
        cs.append(L("gemm128_straight", 128 * t - 5, 384, 256, why=f"wg{3 * t}"))
        cs.append(L("gemm128_looped", 128 * t - 5, 384, 64, why=f"wg{3 * t}"))
    return cs


def glu_cases():
    def G(route, M, N2, K, *, sat, ldo=None, lda=None, ldw=None):
        return dict(entry="linear_glu_f16", route=route, M=M, N=N2, K=K, lda=lda or K, ldw=ldw or K, ldo=ldo or N2 // 2, bias=True,
                    sat=int(sat), vals=V1 if K > 512 else V2)
    return [G("skinny", 1, 256, 256, sat=True), G("skinny", 13, 256, 64, sat=False), G("skinny", 16, 260, 504, sat=True, ldo=134),
            G("skinny_splitk", 5, 256, 520, sat=True, ldo=136), G("skinny_splitk", 12, 1024, 2056, sat=False),
            G("gemm128_straight", 17, 256, 256, sat=True), G("gemm128_straight", 129, 1024, 256, sat=True, ldo=520),
            G("gemm128_straight", 257, 256, 256, sat=False, lda=264, ldw=264),
            G("gemm128_looped", 129, 256, 320, sat=True, ldo=130), G("gemm128_looped", 300, 1024, 320, sat=False),
            G("gemm128_looped", 127, 256, 64, sat=True)]


def heads_cases():
    cs = []
    for entry in ("inproj_heads_bf16", "retention_proj_f16"):
        vals = V1 if entry == "inproj_heads_bf16" else V2
        def Hc(route, nseq, Tp, *, H=4, K=256, lda=None, ldw=None, why=None):
            return dict(entry=entry, route=route, nseq=nseq, Tp=Tp, H=H, K=K, lda=lda or K, ldw=ldw or K, vals=vals, why=why)
        for nseq, Tp in ((1, 64), (3, 64), (2, 128), (1, 192)):
            cs.append(Hc("proj", nseq, Tp))
            cs.append(Hc("gemm128_straight", nseq, Tp, ldw=264))
            cs.append(Hc("gemm128_looped", nseq, Tp, K=320))
        cs += [Hc("gemm128_straight", 3, 64, H=2), Hc("gemm128_straight", 3, 64, H=8), Hc("gemm128_looped", 3, 64, H=2, K=64),
               Hc("proj", 3, 64, lda=320, why="lda"), Hc("gemm128_straight", 1, 192, H=8, lda=264, why="lda")]
    return cs


def res_cases():
    def R(entry, route, M, K, *, res=True, bias=True, gamma=True, alpha=1.0, out32=True, out16=True, alias=False, lda=None, ldw=None):
        return dict(entry=entry, route=route, M=M, K=K, lda=lda or K, ldw=ldw or K, res=int(res), bias=int(bias), gamma=int(gamma),
                    alpha=alpha, eps=1e-5, out32=int(out32), out16=int(out16), alias=int(alias) or None, vals=V1 if K > 512 else V2)
    cs = []
    three = ("linear_res_ln_f16", "linear_res_scale_f16", "linear_res_scale_ln16_f16")
    for e in three:
        g = e != "linear_res_scale_f16"
        cs += [R(e, "skinny", 1, 256, gamma=g), R(e, "skinny", 16, 64, gamma=g, alpha=0.5, alias=True),
               R(e, "skinny", 9, 320, gamma=g, res=False), R(e, "skinny_splitk", 13, 2048, gamma=g, alpha=2.0),
               R(e, "skinny_splitk", 4, 520, gamma=g, bias=False)]
        for M in (17, 63, 64, 65, 130):
            cs.append(R(e, "gemm64x256", M, 256, gamma=g, alias=(M == 65)))
        cs += [R(e, "gemm64x256", 65, 64, gamma=g, alpha=0.5), R(e, "gemm64x256", 130, 320, gamma=g, res=False, lda=328, ldw=336),
               R(e, "gemm64x256", 63, 2048, gamma=g, alpha=2.0, bias=False)]
    e = "linear_res_ln_f16"
    cs += [R(e, "gemm64x256", 1, 256, out32=False), R(e, "gemm64x256", 16, 320, out32=False, alpha=0.5),
           R(e, "gemm64x256", 65, 256, gamma=False), R(e, "skinny", 5, 256, gamma=False), R(e, "gemm64x256", 130, 64, out16=False)]
    cs += [R("linear_res_scale_f16", "gemm64x256", 65, 320, out32=False), R("linear_res_scale_f16", "skinny", 8, 256, out16=False)]
    e = "linear_res16_ln_f16"
    for M in (1, 16, 17, 63, 64, 65, 130):
        cs.append(R(e, "gemm64x256", M, 256, out32=(M != 63)))
    cs += [R(e, "gemm64x256", 65, 64, alpha=0.5), R(e, "gemm64x256", 130, 320), R(e, "gemm64x256", 17, 2048, alpha=2.0, bias=False)]
    return cs


def fanout_cases():
    cs = []
    for C, route in ((1, "convert_rows"), (12, "convert_rows"), (32, "convert_rows"), (33, "gemm64x256"), (40, "gemm64x256")):
        for (B, Tp), out32 in (((1, 64), True), ((2, 64), False), ((1, 128), True)):
            cs.append(dict(entry="convert_fanout_f16", route=route, B=B, Tp=Tp, C=C, out32=int(out32), K=256))
    return cs


def conv_cases():
    """eend_conv1d_l2norm_f16 has one kernel (the 64x256 tile with the implicit-GEMM loads): no route, edges only"""
    cs = []
    Tp = 64
    for (ktaps, pad), cin in (((19, 9), 256), ((19, 9), 64), ((1, 0), 64), ((3, 0), 256), ((3, 2), 64), ((3, 2), 256)):
        for ilens in ((0, 1, Tp), (pad, Tp - pad, Tp), (Tp, Tp, Tp - 1)):
            cs.append(dict(entry="conv1d_l2norm_f16", route="gemm64x256", nseq=3, Tp=Tp, cin=cin, ktaps=ktaps, pad=pad, ilens=list(ilens)))
    return cs


def step_f32_cases():
    cs = []
    P = lambda *a, **k: _plain("linear_step_f32", *a, **k)
    for M in (1, 5, 16):
        cs += [P("skinny", M, 130, 264, act=M % 3), P("skinny_splitk", M, 24, 520)]
    for M in (17, 63, 64, 65, 130):
        cs += [P("f32_mfma", M, 80, 256), P("f32_mfma_splitk", M, 80, 784)]
    cs += [P("f32_mfma", 65, 16, 16), P("f32_mfma", 130, 768, 768, act=1), P("f32_mfma", 17, 16, 256, bias=False, act=2),
           P("f32_mfma", 33, 80, 768, lda=772, ldw=776, ldo=84), P("f32_mfma_splitk", 65, 16, 2048), P("f32_mfma_splitk", 130, 80, 4864),
           P("f32_mfma_splitk", 33, 768, 784, act=1)]
    for M in (17, 33, 130):                              # row groups through each condition that leaves the MFMA kernel
        cs += [P("skinny_rowgroups", M, 80, 264), P("skinny_rowgroups_splitk", M, 80, 520), P("skinny_rowgroups", M, 24, 256),
               P("skinny_rowgroups", M, 80, 256, bias_off=4), P("skinny_rowgroups_splitk", M, 24, 784, act=1)]

    def R(entry, route, M, K, *, res=True, bias=True, alpha=1.0, alias=False, out16=True, route_over=None):
        return dict(entry=entry, route=route, M=M, K=K, lda=K, ldw=K, res=int(res), bias=int(bias), gamma=1, alpha=alpha, eps=1e-5, out32=1,
                    out16=int(out16), alias=int(alias) or None, vals=V1 if K > 512 else V2, route_over=route_over or {},
                    bias_off=4 if route_over else None)
    for e in ("linear_res_ln_step_f32", "linear_res_scale_ln_step_f32"):
        cs += [R(e, "skinny", 1, 256), R(e, "skinny", 16, 264, alpha=0.5, alias=True), R(e, "skinny_splitk", 12, 2048, res=False),
               R(e, "skinny_splitk", 3, 520, bias=False, out16=False)]
        for M in (17, 63, 64, 65, 130):
            cs += [R(e, "f32_mfma", M, 256, alias=(M == 64)), R(e, "f32_mfma_splitk", M, 784, alpha=0.5)]
        cs += [R(e, "f32_mfma", 65, 16), R(e, "f32_mfma", 130, 768, res=False), R(e, "f32_mfma_splitk", 65, 2048, bias=False),
               R(e, "skinny_rowgroups", 17, 264), R(e, "skinny_rowgroups", 130, 264, alpha=2.0, alias=True),
               R(e, "skinny_rowgroups_splitk", 33, 520), R(e, "skinny_rowgroups", 33, 256, route_over={"bias": 4})]
    return cs


# refusals each entry's routing code states: (entry, route-query fields, why).  The GPU test makes the same call on real buffers and
# asserts EEND_EINVAL with every output untouched; the shapes are chosen so that the buffers of the nearest legal case cover them.
REFUSALS = [
    ("linear_f16", dict(M=17, N=192, K=64, lda=64, ldw=64, ldo=192), "N % 128 on the GEMM route"),
    ("linear_f16", dict(M=17, N=128, K=72, lda=72, ldw=72, ldo=128), "K % 64 at M = 17"),
    ("linear_f16", dict(M=4, N=128, K=64, lda=64, ldw=64, ldo=130), "ldo % 4"),
    ("linear_f16", dict(M=4, N=128, K=64, lda=64, ldw=64, ldo=128, act=3), "unknown activation"),
    ("linear_f16", dict(M=17, N=128, K=64, lda=64, ldw=64, ldo=132), "ldo % 8 == 4 at M > 16: 16-byte stores to 8-byte rows"),
    ("linear_f16", dict(M=17, N=128, K=64, lda=68, ldw=64, ldo=128), "lda % 8 on the GEMM route"),
    ("linear_f16", dict(M=4, N=128, K=64, lda=64, ldw=64, ldo=128, out_f16=-1), "NULL output"),
    ("linear_glu_f16", dict(M=4, N=130, K=64, lda=64, ldw=64, ldo=65), "odd ldo"),
    ("linear_glu_f16", dict(M=4, N=129, K=64, lda=64, ldw=64, ldo=66), "odd N2"),
    ("linear_glu_f16", dict(M=17, N=192, K=64, lda=64, ldw=64, ldo=96), "N2 % 128 on the GEMM route"),
    ("linear_glu_f16", dict(M=4, N=128, K=64, lda=64, ldw=64, ldo=64, bias=-1), "NULL bias"),
    ("inproj_heads_bf16", dict(nseq=1, Tp=96, H=4, dh=64, K=256, lda=256, ldw=256), "Tp % 64"),
    ("inproj_heads_bf16", dict(nseq=1, Tp=64, H=3, dh=64, K=256, lda=256, ldw=256), "odd head count: a tile would straddle Q | K"),
    ("inproj_heads_bf16", dict(nseq=1, Tp=64, H=4, dh=32, K=256, lda=256, ldw=256), "dh != 64"),
    ("inproj_heads_bf16", dict(nseq=1, Tp=64, H=4, dh=64, K=288, lda=288, ldw=288), "K % 64 on the GEMM route"),
    ("inproj_heads_bf16", dict(nseq=0, Tp=64, H=4, dh=64, K=256, lda=256, ldw=256), "no sequence"),
    ("retention_proj_f16", dict(nseq=1, Tp=96, H=4, dh=64, K=256, lda=256, ldw=256), "Tp % 64"),
    ("retention_proj_f16", dict(nseq=1, Tp=64, H=4, dh=64, K=256, lda=260, ldw=264), "lda % 8 on the GEMM route"),
    ("retention_proj_f16", dict(nseq=1, Tp=64, H=4, dh=64, K=256, lda=256, ldw=256, bias=-1), "NULL bias"),
    ("linear_res_ln_f16", dict(M=17, K=72, lda=72, ldw=72), "K % 64 at M = 17"),
    ("linear_res_ln_f16", dict(M=4, K=64, lda=64, ldw=64, beta=-1), "gamma without beta"),
    ("linear_res_ln_f16", dict(M=4, K=64, lda=64, ldw=64, out_f32=-1, out_f16=-1), "no output"),
    ("linear_res_ln_f16", dict(M=0, K=64, lda=64, ldw=64), "no rows"),
    ("linear_res16_ln_f16", dict(M=17, K=64, lda=64, ldw=64, res=-1), "NULL f16 residual"),
    ("linear_res16_ln_f16", dict(M=17, K=64, lda=64, ldw=64, gamma=-1, beta=-1), "NULL gamma"),
    ("linear_res16_ln_f16", dict(M=4, K=72, lda=72, ldw=72), "K % 64 (no skinny form)"),
    ("linear_res_scale_f16", dict(M=17, K=64, lda=64, ldw=68), "ldw % 8"),
    ("linear_res_scale_f16", dict(M=4, K=64, lda=64, ldw=64, out_f32=-1, out_f16=-1), "no output"),
    ("linear_res_scale_ln16_f16", dict(M=4, K=64, lda=64, ldw=64, out_f32=-1), "NULL stream output"),
    ("linear_res_scale_ln16_f16", dict(M=17, K=96, lda=96, ldw=96), "K % 64 at M = 17"),
    ("convert_fanout_f16", dict(nseq=1, Tp=64, C=0), "C <= 0"),
    ("convert_fanout_f16", dict(nseq=0, Tp=64, C=4), "B <= 0"),
    ("convert_fanout_f16", dict(nseq=1, Tp=64, C=4, res=-1), "NULL pc"),
    ("linear_step_f32", dict(M=4, N=16, K=12, lda=12, ldw=12, ldo=16), "K % 8"),
    ("linear_step_f32", dict(M=4, N=16, K=16, lda=18, ldw=16, ldo=16), "lda % 4"),
    ("linear_step_f32", dict(M=0, N=16, K=16, lda=16, ldw=16, ldo=16), "no rows"),
    ("linear_step_f32", dict(M=4, N=16, K=16, lda=16, ldw=16, ldo=16, a=4), "A not 16-byte aligned"),
    ("linear_res_ln_step_f32", dict(M=4, K=16, lda=16, ldw=16, gamma=-1, beta=-1), "NULL gamma"),
    ("linear_res_ln_step_f32", dict(M=17, K=20, lda=20, ldw=20), "K % 8"),
    ("linear_res_scale_ln_step_f32", dict(M=4, K=16, lda=16, ldw=16, out_f32=-1), "NULL stream output"),
    ("linear_res_scale_ln_step_f32", dict(M=17, K=16, lda=16, ldw=18), "ldw % 4"),
]


def all_cases():
    return linear_f16_cases() + glu_cases() + heads_cases() + res_cases() + fanout_cases() + conv_cases() + step_f32_cases()


_BY_ID = {}
for _c in all_cases():
    assert case_id(_c) not in _BY_ID, case_id(_c)
    _BY_ID[case_id(_c)] = _c
