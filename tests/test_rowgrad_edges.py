"""GPU: the non-GEMM entries of the training step (csrc/train_rows.hip, csrc/ls_train.hip, csrc/optim.hip behind csrc/api_train.hip)
at their grid, split, strip and tail edges, against the exact references of tests/rowgrad_edge_ref.py.

Wherever the operands make every partial sum exact in f32 (the guard E.assert_exact checks that condition on the inputs; the
constructions are explained in tests/rowgrad_edge_ref.py) the comparison is bit for bit and has no tolerance: a row dropped, doubled,
taken from beyond Tv or paired with the wrong tap fails it (tests/test_rowgrad_edges_ref.py shows that on the CPU).  Outputs that
cannot be exact (softmax, BCE, L2 norm, variances about a rounded mean, Adam) are compared with float64 under the bars of BARS below.

Every case pre-fills its outputs with NaN, keeps poison (NaN, or +-1000 where a value is loaded and then discarded) in every frame at
or beyond Tv / T and in the rows behind M, puts canary rows or columns beside the outputs, and allocates its own NaN-filled workspace of
exactly the documented minimum (include/eend_hip.h) followed by a canary region that must stay NaN.  Every case prints the grid it
exercised: blocks, rows per block, passes."""
import ctypes
import functools

import pytest
import torch

from tests import rowgrad_edge_ref as E

pytestmark = pytest.mark.gpu
F16, BF16, F32, F64, I32, I64 = torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.int64
NAN = float("nan")
EINVAL = -1
D = 256
TAIL = 256                      # canary floats behind every workspace

# Bars of the float64 comparisons: twice the worst error measured on the MI355X (the measured figure stands beside each bar), which
# leaves headroom for f32 reorderings without hiding an O(1) indexing error, and never above the bar the existing test of the entry uses
# (tests/test_train_kernels.py, tests/test_ls_train_kernels.py).  rel: relative to the largest reference magnitude.
BARS = {
    "spk_attn_bwd relnorm": 3.4e-3,        # measured 1.67e-3 (every C in 1..12; existing bar 6e-3)
    "head loss abs": 1.6e-7,               # measured 7.9e-8  (existing bar 1e-5)
    "head logits abs": 5.4e-8,             # measured 2.7e-8  (existing bar 1e-5)
    "head da rel": 5.3e-7,                 # measured 2.63e-7 (existing bar 1e-4)
    "head de rel": 3.1e-7,                 # measured 1.53e-7 (existing bar 1e-4)
    "l2norm_bwd rel": 4.5e-3,              # measured 2.24e-3 (one bf16 store; existing bar 6e-3)
    "bn var rel": 9.3e-8,                  # measured 4.6e-8  (exact sums, one division; existing bar 1e-5)
    "bn run_mean abs": 3.4e-7,             # measured 1.67e-7 (existing bar 1e-5)
    "bn run_var rel": 1.7e-7,              # measured 8.5e-8  (existing bar 1e-5)
    "bn16 M2 rel": 7.2e-7,                 # measured 3.56e-7 (deviations about the rounded f32 mean; existing bar 1e-3)
    "adam p abs": 5.5e-7,                  # measured 2.71e-7 (three steps; existing bar 2e-6)
    "adam m rel": 5.7e-7,                  # measured 2.81e-7 (no existing assertion on the moments)
    "adam v rel": 2.3e-6,                  # measured 1.12e-6 (likewise)
    "ret_gate ot rel": 4.3e-3,             # measured 2.11e-3 (one bf16 store; existing bar 8e-3)
    "ret_gate dg rel": 4.3e-3,             # measured 2.12e-3 (likewise)
}
WORST = {}


def _bar(key, err):
    """print the measured error, remember the worst, assert the bar"""
    err = float(err)
    WORST[key] = max(WORST.get(key, 0.0), err)
    print(f"  {key}: error {err:.3e} (bar {BARS[key]:.1e}, worst so far {WORST[key]:.3e})")
    assert err <= BARS[key], (key, err)


def _rc(L, name, *args):
    """one C-ABI call on the current stream -> its return code"""
    a = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in args]
    return getattr(L, name)(*a, torch.cuda.current_stream().cuda_stream)


def _same(got, want):
    """bit-for-bit up to the sign of zero; NaN (the pre-fill) must sit exactly where it is expected"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return got.shape == want.shape and torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(0.0), want.nan_to_num(0.0))


def _nan(shape, dtype, dev):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), NAN, dtype=dtype, device=dev)


def _ws(dev, n):
    """a NaN-filled workspace of exactly n floats followed by the canary region"""
    return torch.full((n + TAIL,), NAN, dtype=F32, device=dev)


def _ws_tail_untouched(ws, n):
    return bool(ws[n:].isnan().all())


def _padrows(t, extra, fill):
    """t [M][...] followed by `extra` rows of `fill`"""
    t = t if t.is_floating_point() else t.double()
    pad = torch.full((extra,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    return torch.cat([t, pad], 0)


def _spec(seed, thresh24):
    from fs_eend_amd import lib as Lb
    return Lb.Dropout(seed, thresh24, 2.0 if thresh24 else 1.0)


SEED = 0x5EED


# ==================================================================================================== persistent row kernels
LN_WS, RES_WS = 1024 * 768, 1024 * 256


@functools.lru_cache(maxsize=2)
def _ln_case(M):
    g, x, rstd, gamma = E.ln_operands(M, 100 + M)
    refs = {(a, t): E.ref_ln(g, x, rstd, gamma, a, SEED, t) for a in (1.0, 0.5) for t in (0, E.HALF)}
    for r in refs.values():
        E.assert_exact(g * x, g, r["ds16"], r["ds"] + 2, unit=0.125)
    return g, x, rstd, gamma, refs


def _grid_line(what, M):
    nb, rpb, passes = E.rows_grid(M)
    print(f"{what}: M {M} -> blocks {nb}, rows per block and pass {rpb}, passes {passes}")


def _ln_inputs(dev, M, g_dtype=F32):
    """device operands with NaN rows behind M (a read beyond M poisons the sums)"""
    g, x, rstd, gamma, refs = _ln_case(M)
    gd = _padrows(E.as_t(g, g_dtype), 4, NAN).to(dev)
    xd = _padrows(E.as_t(x, F16), 4, NAN).to(dev)
    rd = _padrows(E.as_t(rstd, F32), 4, NAN).to(dev)
    return gd, xd, rd, E.as_t(gamma, F32).to(dev), refs


def _check_ln_outputs(r, M, dg, db, dbias, ds32, ds16, ds32_want=None):
    want3 = lambda v: _padrows(v[None, :], 1, NAN)                                     # [2][256]: the sums and a canary row
    assert _same(dg, want3(r["dgamma"])), "dgamma"
    assert _same(db, want3(r["dbeta"])), "dbeta"
    if dbias is not None:
        assert _same(dbias, want3(r["dbias"])), "dbias"
    if ds32 is not None:
        assert _same(ds32, _padrows(r["ds"] if ds32_want is None else ds32_want, 4, NAN)), "ds32"
    if ds16 is not None:
        assert _same(ds16, _padrows(r["ds16"], 4, NAN)), "ds16 (zeros exactly where the oracle mask drops)"


@pytest.mark.parametrize("M", E.ROW_M)
def test_layernorm_bwd(hip_lib, dev, M):
    """eend_layernorm_bwd_f32: dgamma, dbeta, dbias, ds32, ds16 bit for bit; with and without p = 0.5 dropout; ds32 in place over g; null
    ds16 with null dbias"""
    L = hip_lib
    _grid_line("eend_layernorm_bwd_f32", M)
    gd, xd, rd, gam, refs = _ln_inputs(dev, M)
    for thresh in (0, E.HALF):
        spec = _spec(SEED, thresh)
        dref = ctypes.byref(spec) if thresh else None
        r = refs[(1.0, thresh)]
        for form in ("separate", "in_place", "no_ds16"):
            ws = _ws(dev, LN_WS)
            dg, db, dbias = (_nan((2, D), F32, dev) for _ in range(3))
            gin = gd.clone()
            ds32 = gin if form == "in_place" else _nan((M + 4, D), F32, dev)
            ds16 = None if form == "no_ds16" else _nan((M + 4, D), BF16, dev)
            rc = _rc(L, "eend_layernorm_bwd_f32", gin, xd, rd, gam, ds32, ds16, ws, LN_WS, dg, db, None if form == "no_ds16" else dbias, M, dref)
            assert rc == 0, (form, thresh)
            _check_ln_outputs(r, M, dg, db, None if form == "no_ds16" else dbias, ds32, ds16)
            if form == "no_ds16":
                assert dbias.isnan().all()
            else:
                assert torch.equal(gin[:M], gd[:M]) or form == "in_place"
            assert _ws_tail_untouched(ws, LN_WS)


@pytest.mark.parametrize("M", E.ROW_M)
def test_layernorm_bwd2(hip_lib, dev, M):
    """eend_layernorm_bwd2_f32: bf16 / f32 input x accumulate / overwrite, alpha16 = 0.5, with and without p = 0.5 dropout"""
    L = hip_lib
    _grid_line("eend_layernorm_bwd2_f32", M)
    prior = E.ints((M, D), 9 + M).double()
    for g16 in (0, 1):
        gd, xd, rd, gam, refs = _ln_inputs(dev, M, BF16 if g16 else F32)
        for acc in (0, 1):
            for thresh in (0, E.HALF):
                spec = _spec(SEED, thresh)
                r = refs[(0.5, thresh)]
                ws = _ws(dev, LN_WS)
                dg, db, dbias = (_nan((2, D), F32, dev) for _ in range(3))
                ds32 = _padrows(E.as_t(prior, F32), 4, NAN).to(dev) if acc else _nan((M + 4, D), F32, dev)
                ds16 = _nan((M + 4, D), BF16, dev)
                rc = _rc(L, "eend_layernorm_bwd2_f32", gd, g16, xd, rd, gam, ds32, acc, ds16, 0.5, ws, LN_WS, dg, db, dbias, M,
                         ctypes.byref(spec) if thresh else None)
                assert rc == 0, (g16, acc, thresh)
                _check_ln_outputs(r, M, dg, db, dbias, ds32, ds16, ds32_want=prior + r["ds"] if acc else None)
                assert _ws_tail_untouched(ws, LN_WS)
    # null ds_f32 and null ds_bf16 / dbias: the parameter gradients alone
    ws = _ws(dev, LN_WS)
    dg, db, dbias = (_nan((2, D), F32, dev) for _ in range(3))
    assert _rc(L, "eend_layernorm_bwd2_f32", gd, 1, xd, rd, gam, None, 0, None, 0.5, ws, LN_WS, dg, db, None, M, None) == 0
    _check_ln_outputs(refs[(0.5, 0)], M, dg, db, None, None, None)
    assert dbias.isnan().all()
    assert _rc(L, "eend_layernorm_bwd2_f32", gd, 1, xd, rd, gam, None, 1, None, 0.5, ws, LN_WS, dg, db, None, M, None) == EINVAL      # accumulate into nothing


@pytest.mark.parametrize("M", E.ROW_M)
def test_layernorm_bwd_is_bwd2_with_unit_alpha(hip_lib, dev, M):
    """eend_layernorm_bwd_f32 and eend_layernorm_bwd2_f32(g_is_bf16 = 0, accumulate = 0, alpha16 = 1.0) run one kernel: the same operands
    give byte-identical ds32, ds16, dgamma, dbeta and dbias, with and without p = 0.5 dropout, with ds_f32 aliasing g and separate"""
    L = hip_lib
    _grid_line("eend_layernorm_bwd_f32 / eend_layernorm_bwd2_f32", M)
    gd, xd, rd, gam, refs = _ln_inputs(dev, M)
    raw = lambda t: t.contiguous().view(torch.uint8)
    for thresh in (0, E.HALF):
        spec = _spec(SEED, thresh)
        dref = ctypes.byref(spec) if thresh else None
        for in_place in (False, True):
            outs = []
            for entry in ("eend_layernorm_bwd_f32", "eend_layernorm_bwd2_f32"):
                ws = _ws(dev, LN_WS)
                dg, db, dbias = (_nan((2, D), F32, dev) for _ in range(3))
                gin = gd.clone()
                ds32 = gin if in_place else _nan((M + 4, D), F32, dev)
                ds16 = _nan((M + 4, D), BF16, dev)
                if entry == "eend_layernorm_bwd_f32":
                    rc = _rc(L, entry, gin, xd, rd, gam, ds32, ds16, ws, LN_WS, dg, db, dbias, M, dref)
                else:
                    rc = _rc(L, entry, gin, 0, xd, rd, gam, ds32, 0, ds16, 1.0, ws, LN_WS, dg, db, dbias, M, dref)
                assert rc == 0, (entry, thresh, in_place)
                assert _ws_tail_untouched(ws, LN_WS)
                assert in_place or torch.equal(raw(gin), raw(gd)), "g is an input"
                _check_ln_outputs(refs[(1.0, thresh)], M, dg, db, dbias, ds32, ds16)
                outs.append((ds32, ds16, dg, db, dbias))
            for name, a, b in zip(("ds32", "ds16", "dgamma", "dbeta", "dbias"), *outs):
                assert torch.equal(raw(a), raw(b)), (name, thresh, in_place)


@pytest.mark.parametrize("M", E.ROW_M)
def test_resgrad_cast(hip_lib, dev, M):
    L = hip_lib
    _grid_line("eend_resgrad_cast_bf16", M)
    g = _ln_case(M)[0]
    gd = _padrows(E.as_t(g, F32), 4, NAN).to(dev)
    for alpha in (1.0, 0.5):
        for thresh in (0, E.HALF):
            spec = _spec(SEED + 1, thresh)
            r = E.ref_resgrad(g, alpha, SEED + 1, thresh)
            E.assert_exact(r["ds16"], unit=0.5)
            ws = _ws(dev, RES_WS)
            ds16, dbias = _nan((M + 4, D), BF16, dev), _nan((2, D), F32, dev)
            assert _rc(L, "eend_resgrad_cast_bf16", gd, ds16, alpha, ws, RES_WS, dbias, M, ctypes.byref(spec) if thresh else None) == 0
            assert _same(ds16, _padrows(r["ds16"], 4, NAN)), "ds16"
            assert _same(dbias, _padrows(r["dbias"][None, :], 1, NAN)), "dbias"
            assert _ws_tail_untouched(ws, RES_WS)


# ==================================================================================================== convert fan-out backward
@pytest.mark.parametrize("B,Tp,C", E.SLOT_CASES)
def test_convert_fanout_bwd(hip_lib, dev, B, Tp, C):
    L = hip_lib
    nb, rpb, passes = E.slot_grid(B * Tp)
    print(f"eend_convert_fanout_bwd_f32: B {B} Tp {Tp} C {C}: frames {B * Tp} -> blocks {nb}, frames per block and pass {rpb}, passes {passes}")
    g0 = E.ints((B * C * Tp, D), 7 + B + C)
    E.assert_exact(g0.view(B, C, Tp, D).permute(0, 2, 1, 3).reshape(B * Tp, C * D))
    gsum_w, dpc_w = E.ref_slot_sum(g0, B, C, Tp)
    wsf = 256 * C * 256
    ws = _ws(dev, wsf)
    gsum, dpc = _nan((B * Tp + 4, D), BF16, dev), _nan((C + 1, D), F32, dev)
    assert _rc(L, "eend_convert_fanout_bwd_f32", _padrows(E.as_t(g0, F32), 4, NAN).to(dev), gsum, ws, wsf, dpc, B, Tp, C) == 0
    assert _same(dpc, _padrows(dpc_w, 1, NAN)), "dpc"
    assert _same(gsum, _padrows(gsum_w, 4, NAN)), "gsum"
    assert _ws_tail_untouched(ws, wsf)


def test_convert_fanout_bwd_refuses_slot_counts_it_does_not_serve(hip_lib, dev):
    g0 = torch.ones(13 * 64, D, device=dev)
    gsum, dpc, ws = _nan((64, D), BF16, dev), _nan((13, D), F32, dev), _ws(dev, 256 * 13 * 256)
    for C in (0, 13):
        assert _rc(hip_lib, "eend_convert_fanout_bwd_f32", g0, gsum, ws, 256 * 13 * 256, dpc, 1, 64, C) == EINVAL
    torch.cuda.synchronize()
    assert gsum.isnan().all() and dpc.isnan().all() and ws.isnan().all()


# ==================================================================================================== speaker-axis attention backward
def _spk_ref(qkv, dO, B, C, Tp):
    x = qkv.double().view(B, C, Tp, 3, 4, 64).requires_grad_(True)
    q, k, v = (x[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(3))                   # (B, Tp, H, C, 64)
    p = torch.softmax((q @ k.transpose(-1, -2)) * 0.125, -1)
    o = (p @ v).permute(0, 3, 1, 2, 4).reshape(B * C * Tp, D)
    (o * dO.double()).sum().backward()
    return x.grad.reshape(B * C * Tp, 3 * D)


@pytest.mark.parametrize("C", range(1, 13))
def test_spk_attn_bwd(hip_lib, dev, C):
    """every template instance against float64 autograd; B * Tp = 66 frames: 17 blocks, the last one half empty"""
    B, Tp = 2, 33
    rows = B * C * Tp
    print(f"eend_spk_attn_bwd_bf16: C {C}: frames {B * Tp} -> blocks {(B * Tp + 3) // 4}, frames per block 4, passes 1")
    gen = torch.Generator().manual_seed(40 + C)
    qkv = torch.randn(rows, 3 * D, generator=gen).to(F16)
    dO = (torch.randn(rows, D, generator=gen) * 1e-4).to(BF16)
    want = _spk_ref(qkv, dO, B, C, Tp)
    out = _nan((rows + 1, 3 * D), BF16, dev)
    assert _rc(hip_lib, "eend_spk_attn_bwd_bf16", qkv.to(dev), dO.to(dev), out, B, C, Tp, 4, 0.125, None) == 0
    got = out.cpu().double()
    assert got[rows].isnan().all() and not got[:rows].isnan().any()
    _bar("spk_attn_bwd relnorm", (got[:rows] - want).norm() / want.norm())


# ==================================================================================================== FS BatchNorm
@functools.lru_cache(maxsize=1)
def _bn_case(key):
    c = E.BN_BIG if key == "big" else E.BN_CASES[key]
    bufs = E.bn_buffers(c, 3)
    rows = E.bn_balance(bufs, c["lens"], c["T"], c["which"], -1, c["F"])
    return c, bufs, rows, E.ref_bn_stats(rows)


def _bn_device(dev, c, bufs):
    """the utterance buffers (NaN behind the longest length that reads each), the pointer table and the lengths"""
    dbufs = []
    for k, b in enumerate(bufs):
        lmax = max(l for l, kk in zip(c["lens"], c["which"]) if kk == k)
        t = E.as_t(b, F32)
        t[lmax:] = NAN
        dbufs.append(t.to(dev))
    ptrs = torch.tensor([dbufs[k].data_ptr() for k in c["which"]], dtype=I64, device=dev)
    return dbufs, ptrs, torch.tensor(c["lens"], dtype=I32, device=dev)


BN_KEYS = list(range(len(E.BN_CASES))) + ["big"]


@pytest.mark.parametrize("key", BN_KEYS, ids=[E.bn_id(c) for c in E.BN_CASES] + ["big"])
def test_bn_train_stats(hip_lib, dev, key):
    c, bufs, rows, (s, mean, var, varu) = _bn_case(key)
    F, T, B = c["F"], c["T"], len(c["lens"])
    n = B * T
    ns, rps = E.bn_splits(n)
    print(f"eend_bn_train_stats_f32: F {F} B {B} T {T}: rows {n} -> splits {ns}, rows per split {rps} ({(rps + 15) // 16} groups of 16), "
          f"column blocks {(F + 255) // 256}, passes 2")
    E.assert_exact(rows, (rows - mean.to(I64)) ** 2)
    dbufs, ptrs, lens = _bn_device(dev, c, bufs)
    wsf = (ns + 1) * 2 * F
    ws = _ws(dev, wsf)
    mo, vo = _nan(F + 8, F32, dev), _nan(F + 8, F32, dev)
    gen = torch.Generator().manual_seed(5)
    rm0, rv0 = torch.randn(F, generator=gen), torch.rand(F, generator=gen) + 0.5
    rm, rv = _padrows(rm0, 8, NAN).to(dev), _padrows(rv0, 8, NAN).to(dev)
    assert _rc(hip_lib, "eend_bn_train_stats_f32", ptrs, lens, -1.0, ws, wsf, mo, vo, rm, rv, 0.1, B, T, F) == 0
    assert _same(mo, _padrows(mean, 8, NAN)), "mean = pass-0 sums / n (an integer per column)"
    assert mo[F:].isnan().all() and vo[F:].isnan().all() and rm[F:].isnan().all() and rv[F:].isnan().all() and _ws_tail_untouched(ws, wsf)
    _bar("bn var rel", (vo[:F].cpu().double() - var).abs().max() / var.max())
    _bar("bn run_mean abs", (rm[:F].cpu().double() - (0.9 * rm0.double() + 0.1 * mean)).abs().max())
    want_rv = 0.9 * rv0.double() + 0.1 * varu
    _bar("bn run_var rel", (rv[:F].cpu().double() - want_rv).abs().max() / want_rv.max())
    # without running statistics
    mo2, vo2 = _nan(F + 8, F32, dev), _nan(F + 8, F32, dev)
    assert _rc(hip_lib, "eend_bn_train_stats_f32", ptrs, lens, -1.0, ws, wsf, mo2, vo2, None, None, 0.1, B, T, F) == 0
    assert torch.equal(mo2[:F], mo[:F]) and torch.equal(vo2[:F], vo[:F])


@pytest.mark.parametrize("key", BN_KEYS, ids=[E.bn_id(c) for c in E.BN_CASES] + ["big"])
def test_bn_bwd(hip_lib, dev, key):
    c, bufs, rows, _ = _bn_case(key)
    F, T, B, ld = c["F"], c["T"], len(c["lens"]), c["F"] + c["gap"]
    n, Tp = B * T, T + (0 if key == "big" else 3)
    ns, rps = E.bn_splits(n)
    print(f"eend_bn_bwd_f32: F {F} ld {ld} B {B} T {T} Tp {Tp}: rows {n} -> splits {ns}, rows per split {rps}, reduction "
          f"{'one launch (F % 32 == 0)' if F % 32 == 0 else 'two launches'}")
    dy = E.ints((n, F), 11)
    mu = E.ints((F,), 12, vals=(-1, 0, 1))
    E.assert_exact(dy * (rows - mu) * 2, dy)
    dg_w, db_w = E.ref_bn_bwd(rows, dy, mu, 2)
    dbufs, ptrs, lens = _bn_device(dev, c, bufs)
    dyd = _nan((B, Tp, ld), BF16, dev)                                      # NaN in the frames >= T and in the columns >= F
    dyd[:, :T, :F] = E.as_t(dy, BF16).view(B, T, F).to(dev)
    wsf = ns * 2 * F
    ws = _ws(dev, wsf)
    dg, db = _nan(F + 8, F32, dev), _nan(F + 8, F32, dev)
    var = torch.full((F,), 0.25, device=dev)
    assert _rc(hip_lib, "eend_bn_bwd_f32", ptrs, lens, -1.0, E.as_t(mu, F32).to(dev), var, 0.0, dyd, ld, ws, wsf, dg, db, B, T, Tp, F) == 0
    assert _same(dg, _padrows(dg_w, 8, NAN)), "dgamma"
    assert _same(db, _padrows(db_w, 8, NAN)), "dbeta"
    assert _ws_tail_untouched(ws, wsf)


def test_bn_train_stats_refuses_a_single_frame(hip_lib, dev):
    x = torch.ones(1, 345, device=dev)
    ptrs, lens = torch.tensor([x.data_ptr()], dtype=I64, device=dev), torch.tensor([1], dtype=I32, device=dev)
    ws, mo, vo = _ws(dev, 4 * 345), _nan(345, F32, dev), _nan(345, F32, dev)
    assert _rc(hip_lib, "eend_bn_train_stats_f32", ptrs, lens, -1.0, ws, 4 * 345, mo, vo, None, None, 0.1, 1, 1, 345) == EINVAL
    torch.cuda.synchronize()
    assert mo.isnan().all() and vo.isnan().all() and ws.isnan().all()


# ==================================================================================================== LS BatchNorm over the valid frames
def _slab(t, nseq, Tp, Tv, dtype, dev):
    """int64 [nseq*Tp][256] -> device slab with NaN in every frame t >= Tv and a NaN canary row behind it"""
    d = E.as_t(t, dtype).view(nseq, Tp, D).clone()
    d[:, Tv:] = NAN
    return _padrows(d.view(nseq * Tp, D), 1, NAN).to(dev)


@pytest.mark.parametrize("nseq,Tp,Tv", E.BN16_CASES + [E.BN16_BIG])
def test_bn_batch_stats_and_swish_bwd_stats(hip_lib, dev, nseq, Tp, Tv):
    L = hip_lib
    n = nseq * Tv
    nb, rpb = E.bn16_blocks(n)
    print(f"eend_bn_batch_stats_f16 / eend_bn_swish_bwd_stats_bf16: nseq {nseq} Tp {Tp} Tv {Tv}: rows {n} -> blocks {nb}, rows per block {rpb} "
          f"({(rpb + 3) // 4} groups of 4), empty blocks {sum(1 for b in range(nb) if b * rpb >= n)}, passes 2 / 1")
    c = E.ints((nseq * Tp, D), nseq + Tv)
    ds = E.ints((nseq * Tp, D), nseq + Tv + 1)
    mu = E.ints((D,), 5, vals=(-1, 0, 1))
    gam = E.ints((D,), 6, vals=(-1, 1, 2))
    rows = E.valid_rows(nseq, Tp, Tv)
    E.assert_exact(c[rows], ds[rows], ds[rows] * (c[rows] - mu) * 2)
    s, nn, mean, m2 = E.ref_bn16_stats(c, nseq, Tp, Tv)
    c16, ds16 = _slab(c, nseq, Tp, Tv, F16, dev), _slab(ds, nseq, Tp, Tv, BF16, dev)
    wsf = (nb + 1) * 256
    ws = _ws(dev, wsf)
    stats = _nan(513 + 8, F32, dev)
    assert _rc(L, "eend_bn_batch_stats_f16", c16, ws, wsf, stats, nseq, Tp, Tv) == 0
    st = stats.cpu()
    assert st[513:].isnan().all() and _ws_tail_untouched(ws, wsf)
    assert st[512].item() == n, "n"
    assert torch.equal(st[:256], s.float() / torch.tensor(float(n))), "mean = exact column sum / n, one rounding"
    _bar("bn16 M2 rel", (st[256:512].double() - m2).abs().max() / m2.max().clamp_min(1.0))
    # backward statistics: gamma * c_hat + beta >= 28, so swish' == 1 and d_y == d_s exactly; var = 0.25, eps = 0: rstd == 2
    s1, s2 = E.ref_bn_swish_stats(ds, c, mu, 2, nseq, Tp, Tv)
    wsf = nb * 512
    ws = _ws(dev, wsf)
    sums, dgam, dbet = _nan(512 + 8, F32, dev), _nan(256 + 8, F32, dev), _nan(256 + 8, F32, dev)
    var, beta = torch.full((D,), 0.25, device=dev), torch.full((D,), E.BETA, device=dev)
    mud, gamd = E.as_t(mu, F32).to(dev), E.as_t(gam, F32).to(dev)
    assert _rc(L, "eend_bn_swish_bwd_stats_bf16", ds16, c16, mud, var, 0.0, gamd, beta, ws, wsf, sums, dgam, dbet, nseq, Tp, Tv) == 0
    assert _same(sums, _padrows(torch.cat([s1, s2]), 8, NAN)), "sums"
    assert _same(dbet, _padrows(s1, 8, NAN)) and _same(dgam, _padrows(s2, 8, NAN)), "dbeta / dgamma"
    assert _ws_tail_untouched(ws, wsf)
    if n > 4096:
        return
    # the apply pass with given (all-reduced) sums: m1 = sums / n integers
    a1, a2 = E.ints((D,), 7), E.ints((D,), 8)
    want = E.ref_bn_swish_apply(ds, c, mu, 2, gam, a1, a2, nseq, Tp, Tv)
    sums_in = E.as_t(torch.cat([a1, a2]) * 4, F32).to(dev)
    n_dev = torch.tensor([4.0], device=dev)
    assert _rc(L, "eend_bn_swish_bwd_apply_bf16", ds16, c16, mud, var, 0.0, gamd, beta, sums_in, n_dev, nseq, Tp, Tv) == 0
    assert _same(ds16, _padrows(want, 1, NAN)), "d_c (zero at and beyond Tv)"


# ==================================================================================================== conv module
@pytest.mark.parametrize("k", E.CONV_K)
def test_conv_module(hip_lib, dev, k):
    """eend_glu_dwconv_f16, eend_bn_swish_bwd_apply_bf16, eend_dwconv_glu_bwd_bf16 with Tv at the strip edges and below the filter length"""
    L, nseq = hip_lib, 2
    for Tv in E.conv_tv(k):
        for Tp in (E.frames_pad(Tv), E.frames_pad(Tv) + 64):
            strips = E.conv_strips(nseq, Tp)
            print(f"conv module k {k} Tv {Tv} Tp {Tp}: blocks {strips} ({Tp // 64} strips of 64 frames x {nseq} sequences), "
                  f"apply blocks {nseq * ((Tp + 15) // 16)} of 16 frames, passes 1")
            val, w, dc = E.conv_operands(nseq, Tp, Tv, k, 10 * k + Tv)
            c_w = E.ref_conv_fwd(val, w, Tv)
            du_w, dw_w = E.ref_conv_bwd(val, w, dc, Tv)
            E.assert_exact(dw_w.reshape(1, -1), (val[:, :Tv].abs().sum((0, 1))[None, :] * 2).reshape(1, -1))
            P = torch.cat([E.as_t(val, F16), torch.full((nseq, Tp, D), E.GATE, dtype=F16)], -1).view(nseq * Tp, 2 * D)
            Pd = _padrows(P, 1, NAN).to(dev)
            wd = E.as_t(w, F32).to(dev)
            c16 = _nan((nseq * Tp + 1, D), F16, dev)
            assert _rc(L, "eend_glu_dwconv_f16", Pd, wd, c16, nseq, Tp, Tv, k) == 0
            assert _same(c16, _padrows(c_w.view(-1, D), 1, NAN)), ("c", Tv, Tp)
            # BatchNorm + swish backward, apply pass, on the convolution output: rstd = 2^-5 keeps gamma * c_hat + beta >= 28 (swish' == 1)
            # for a 31-tap sum; every f32 step is exact, the result is rounded to bf16 once (to nearest even, here as there)
            mu, gam = E.ints((D,), 5, vals=(-1, 0, 1)), E.ints((D,), 6, vals=(-1, 1, 2))
            var = torch.full((D,), 1024.0, device=dev)                               # rstd = 1 / 32: c_hat = (c - mu) / 32, multiples of 2^-5
            ch = (c_w.double() - mu.double()) / 32
            assert float(ch.abs().max()) * 2 <= E.BETA - 28
            a1, a2 = E.ints((D,), 7), E.ints((D,), 8, vals=(-32, 32))
            dsd = _slab(dc.view(-1, D), nseq, Tp, Tv, BF16, dev)
            want = torch.zeros(nseq, Tp, D, dtype=F64)
            want[:, :Tv] = (gam.double() / 32 * (dc.double() - a1.double() - ch * a2.double()))[:, :Tv]
            sums_in = E.as_t(torch.cat([a1, a2]) * 4, F32).to(dev)
            assert _rc(L, "eend_bn_swish_bwd_apply_bf16", dsd, c16, E.as_t(mu, F32).to(dev), var, 0.0, E.as_t(gam, F32).to(dev),
                       torch.full((D,), E.BETA, device=dev), sums_in, torch.tensor([4.0], device=dev), nseq, Tp, Tv) == 0
            assert _same(dsd, _padrows(want.to(BF16).view(-1, D), 1, NAN)), ("apply", Tv, Tp)
            # depthwise conv + GLU backward
            dcd = _slab(dc.view(-1, D), nseq, Tp, Tv, BF16, dev)
            wsf = strips * 256 * k
            ws = _ws(dev, wsf)
            dP, dw = _nan((nseq * Tp + 1, 2 * D), BF16, dev), _nan((D + 1, k), F32, dev)
            assert _rc(L, "eend_dwconv_glu_bwd_bf16", dcd, Pd, wd, dP, ws, wsf, dw, nseq, Tp, Tv, k) == 0
            dP_w = torch.cat([du_w, torch.zeros_like(du_w)], -1).view(-1, 2 * D)
            assert _same(dP, _padrows(dP_w, 1, NAN)), ("dP", Tv, Tp)
            assert _same(dw, _padrows(dw_w, 1, NAN)), ("dw", Tv, Tp)
            assert _ws_tail_untouched(ws, wsf)


def test_conv_module_refuses_taps_it_does_not_serve(hip_lib, dev):
    P, w = torch.zeros(64, 512, dtype=F16, device=dev), torch.zeros(D, 32, device=dev)
    c16, dP, dw, ws = _nan((64, D), F16, dev), _nan((64, 512), BF16, dev), _nan((D, 32), F32, dev), _ws(dev, 256 * 32)
    dc = torch.zeros(64, D, dtype=BF16, device=dev)
    for k in (1, 8, 17, 32):
        assert _rc(hip_lib, "eend_glu_dwconv_f16", P, w, c16, 1, 64, 64, k) == EINVAL
        assert _rc(hip_lib, "eend_dwconv_glu_bwd_bf16", dc, P, w, dP, ws, 256 * 32, dw, 1, 64, 64, k) == EINVAL
    assert _rc(hip_lib, "eend_glu_dwconv_f16", P, w, c16, 1, 64, 65, 16) == EINVAL          # Tv > Tp
    torch.cuda.synchronize()
    assert c16.isnan().all() and dP.isnan().all() and dw.isnan().all() and ws.isnan().all()


# ==================================================================================================== head + BCE
def _head_ref(emb, attr, lab, ilens, ncols, B, T, Tp, C):
    """float64: loss, logits (B, T, C), d loss / d attr, d loss / d emb as the entry defines them"""
    er, ar = emb.double().clone().requires_grad_(True), attr.double().clone().requires_grad_(True)
    a4 = ar.view(B, C, Tp, D)
    an = a4 / a4.norm(dim=-1, keepdim=True)
    logit = (er.view(B, 1, Tp, D) * an).sum(-1).permute(0, 2, 1)[:, :T]                   # (B, T, C)
    n_frames = sum(ilens)
    loss = 0
    for b in range(B):
        y, t = logit[b, :ilens[b], :ncols[b]], lab[b, :ilens[b], :ncols[b]].double()
        loss = loss + torch.nn.functional.binary_cross_entropy_with_logits(y, t, reduction="sum") / ncols[b]
    loss = loss / n_frames
    da, de = torch.autograd.grad(loss, [ar, er], retain_graph=True)
    dl, = torch.autograd.grad(loss, [logit], retain_graph=True)
    return loss.detach(), logit.detach(), da, de, dl


@pytest.mark.parametrize("C", [1, 12])
def test_head_bce(hip_lib, dev, C):
    """both modes; T < Tp, an utterance of one frame, ncols < C; frames t >= T hold NaN"""
    L, B, T, Tp = hip_lib, 3, 50, 64
    ilens, ncols = [50, 1, 37], [C, max(1, C - 5), max(1, C // 2)]
    nb = (B * Tp + 3) // 4
    print(f"eend_head_bce_f32: B {B} T {T} Tp {Tp} C {C}: frames {B * Tp} -> blocks {nb}, frames per block 4, passes 1")
    gen = torch.Generator().manual_seed(60 + C)
    emb = torch.nn.functional.normalize(torch.randn(B * Tp, D, generator=gen), dim=-1)
    attr = torch.randn(B * C * Tp, D, generator=gen) * 3
    lab = (torch.rand(B, T, C, generator=gen) < 0.3).float()
    loss_w, logit_w, da_w, de_w, dl_w = _head_ref(emb, attr, lab, ilens, ncols, B, T, Tp, C)
    embd, attrd = emb.clone().view(B, Tp, D), attr.clone().view(B * C, Tp, D)
    embd[:, T:] = NAN
    attrd[:, T:] = NAN
    embd, attrd = embd.view(-1, D).to(dev), attrd.view(-1, D).to(dev)
    il, nc = torch.tensor(ilens, dtype=I32, device=dev), torch.tensor(ncols, dtype=I32, device=dev)
    for mode in ("bce", "dlogits"):
        ws = _ws(dev, nb)
        logits, da, de, lo = _nan((B * T * C + 8,), F32, dev), _nan((B * C * Tp + 1, D), F32, dev), _nan((B * Tp + 1, D), F32, dev), _nan((2,), F32, dev)
        if mode == "bce":
            rc = _rc(L, "eend_head_bce_f32", embd, attrd, lab.to(dev), il, nc, 1.0 / sum(ilens), None, logits, da, de, ws, nb, lo, B, T, Tp, C)
        else:
            rc = _rc(L, "eend_head_bce_f32", embd, attrd, None, None, None, 0.0, dl_w.float().contiguous().to(dev), logits, da, de, ws, nb, lo, B, T, Tp, C)
        assert rc == 0
        assert _ws_tail_untouched(ws, nb) and lo[1].isnan() and logits[B * T * C:].isnan().all() and da[-1].isnan().all() and de[-1].isnan().all()
        da_g, de_g = da[:-1].cpu().double(), de[:-1].cpu().double()
        assert not da_g.isnan().any() and not de_g.isnan().any()
        assert (da_g.view(B * C, Tp, D)[:, T:] == 0).all() and (de_g.view(B, Tp, D)[:, T:] == 0).all()
        if mode == "bce":
            _bar("head loss abs", (lo[0].cpu().double() - loss_w).abs())
        _bar("head logits abs", (logits[:B * T * C].cpu().double().view(B, T, C) - logit_w).abs().max())
        da_ref, de_ref = da_w.clone().view(B * C, Tp, D), de_w.clone().view(B, Tp, D)
        da_ref[:, T:] = 0
        de_ref[:, T:] = 0
        _bar("head da rel", (da_g - da_ref.view(-1, D)).abs().max() / da_ref.abs().max())
        _bar("head de rel", (de_g - de_ref.view(-1, D)).abs().max() / de_ref.abs().max())


def test_l2norm_bwd(hip_lib, dev):
    B, T, Tp = 3, 33, 64
    print(f"eend_l2norm_bwd_bf16: B {B} T {T} Tp {Tp}: rows {B * Tp} -> blocks {(B * Tp + 3) // 4}, rows per block 4, passes 1")
    gen = torch.Generator().manual_seed(7)
    x = (torch.randn(B, Tp, D, generator=gen) * 2).double().requires_grad_(True)
    dy = (torch.randn(B, Tp, D, generator=gen) * 1e-4).double()
    e = x / x.norm(dim=-1, keepdim=True)
    want, = torch.autograd.grad(e, [x], dy)
    yd, dyd, inv = e.detach().float().clone(), dy.float().clone(), (1 / x.detach().norm(dim=-1)).float().clone()
    yd[:, T:] = NAN
    dyd[:, T:] = NAN
    inv[:, T:] = NAN
    out = _nan((B * Tp + 1, D), BF16, dev)
    assert _rc(hip_lib, "eend_l2norm_bwd_bf16", yd.view(-1, D).to(dev), dyd.view(-1, D).to(dev), inv.view(-1).to(dev), out, B, T, Tp) == 0
    got = out.cpu().double()
    assert got[-1].isnan().all() and (got[:-1].view(B, Tp, D)[:, T:] == 0).all() and not got[:-1].isnan().any()
    _bar("l2norm_bwd rel", (got[:-1].view(B, Tp, D)[:, :T] - want[:, :T]).abs().max() / want[:, :T].abs().max())


def test_attn_rowdot(hip_lib, dev):
    """attn_rowdot_kernel through its only caller, eend_attn_causal_bwd_bf16 (zero Q / K / V: the rest of the backward runs on zeros):
    D[seq][head][t] = sum_d dO O over every row of the slab, exact on integers"""
    nseq, Tp = 3, 128
    M = nseq * Tp
    print(f"eend_attn_causal_bwd_bf16 (row dot): nseq {nseq} Tp {Tp}: rows {M} -> blocks {(M + 3) // 4}, rows per block 4, passes 1")
    dO, O = E.ints((M, D), 71), E.ints((M, D), 72)
    want = (dO * O).view(nseq, Tp, 4, 64).sum(-1).permute(0, 2, 1).reshape(-1)                  # [nseq][4][Tp]
    z = torch.zeros(nseq * 4 * Tp * 64, dtype=BF16, device=dev)
    lse = torch.zeros(nseq * 4 * Tp, device=dev)
    dot_ws, dh = torch.empty(M * D, dtype=BF16, device=dev), _nan((nseq * 4 * Tp + 8,), F32, dev)
    dqkv = _nan((M, 3 * D), BF16, dev)
    rc = _rc(hip_lib, "eend_attn_causal_bwd_bf16", z, z, z, z, z, E.as_t(dO, BF16).to(dev), 256, E.as_t(O, F16).to(dev), 256, lse, dot_ws, dh, dqkv, 768,
             nseq, 4, Tp, 0, Tp, Tp, 1.0, 0.125, 0.6931471805599453, None)
    assert rc == 0
    assert _same(dh, _padrows(want, 8, NAN))
    assert torch.isfinite(dqkv.float()).all()


def _swish(x):
    return x * torch.sigmoid(x)


def test_ret_gate_gn_bwd(hip_lib, dev):
    """ret_gate_gn_bwd_kernel through its C-ABI entry eend_retention_bwd_bf16 (zero Q / K / V), ldg = 264 and ldq = 1032: o~ and d_g
    against float64, zero at and beyond T_valid, canary columns untouched"""
    nseq, Tp, L, Tv, ldg, ldq = 2, 128, 4, 36, 264, 1032
    M, nc = nseq * Tp, Tv // L
    print(f"eend_retention_bwd_bf16 (gate + per-head LayerNorm backward): nseq {nseq} Tp {Tp} T_valid {Tv} ldg {ldg} ldq {ldq}: rows {M} -> "
          f"blocks {(M + 3) // 4}, rows per block 4, passes 1")
    gen = torch.Generator().manual_seed(73)
    dctx = (torch.randn(M, D, generator=gen) * 1e-3).float()
    g16 = torch.randn(M, D, generator=gen).to(F16)
    rh16 = torch.randn(M, D, generator=gen).to(F16)
    rcv = (torch.rand(M, 4, generator=gen) + 0.5).float()
    d, g, rh, rcd = (t.double().view(M, 4, -1) for t in (dctx, g16, rh16, rcv))
    sg = torch.sigmoid(g)
    drh = d * _swish(g)
    dr = drh - drh.mean(-1, keepdim=True) - rh * (drh * rh).mean(-1, keepdim=True)
    ot_w = (rcd * dr).view(nseq, Tp, D)
    dg_w = (d * rh * sg * (1 + g * (1 - sg))).view(nseq, Tp, D)
    ot_w[:, Tv:] = 0
    dg_w[:, Tv:] = 0

    def poisoned(t, width=None):
        t = t.clone().view(nseq, Tp, -1)
        t[:, Tv:] = NAN
        if width:
            t = torch.cat([t, torch.full((nseq, Tp, width - t.shape[-1]), NAN, dtype=t.dtype)], -1)
        return t.view(M, -1).contiguous().to(dev)
    z = torch.zeros(nseq * 4 * Tp * 64, dtype=BF16, device=dev)
    ot, out = _nan((M + 1, D), BF16, dev), _nan((M, ldq), BF16, dev)
    kv_ws, g_ws = (torch.empty(nseq * 4 * nc * 4096, device=dev) for _ in range(2))
    st = torch.empty(nseq * 4 * nc * 6 * 4096, dtype=BF16, device=dev)
    rc = _rc(hip_lib, "eend_retention_bwd_bf16", z, None, z, None, z, None, poisoned(dctx), poisoned(g16, ldg), ldg, poisoned(rh16), poisoned(rcv),
             ot, None, kv_ws, g_ws, st, out, ldq, nseq, 4, Tp, L, Tv, 0.125)
    assert rc == 0
    ot_g, out_g = ot.cpu().double(), out.cpu().double()
    assert ot_g[M].isnan().all() and out_g[:, 1024:].isnan().all() and not ot_g[:M].isnan().any() and not out_g[:, :1024].isnan().any()
    ot_g, dg_g = ot_g[:M].view(nseq, Tp, D), out_g[:, 768:1024].view(nseq, Tp, D)
    assert (ot_g[:, Tv:] == 0).all() and (out_g.view(nseq, Tp, ldq)[:, Tv:, :1024] == 0).all()
    _bar("ret_gate ot rel", (ot_g - ot_w).abs().max() / ot_w.abs().max())
    _bar("ret_gate dg rel", (dg_g - dg_w).abs().max() / dg_w.abs().max())


# ==================================================================================================== optimiser
@pytest.mark.parametrize("n", E.SUMSQ_N)
def test_grad_sumsq(hip_lib, dev, n):
    nb, passes, tail = E.sumsq_grid(n)
    print(f"eend_grad_sumsq_f32: n {n} -> blocks {nb}, float4 per block and pass 256, passes {passes}, scalar tail {tail} (block 0)")
    g = E.ints((n,), n % 1000)
    want = E.ref_sumsq(g)
    assert want < E.LIMIT
    gd = _padrows(E.as_t(g, F32), 8, NAN).to(dev)                          # a read beyond n poisons the sum
    ws, out = _ws(dev, 1024), _nan((2,), F32, dev)
    assert _rc(hip_lib, "eend_grad_sumsq_f32", gd, n, ws, 1024, out) == 0
    assert out[0].item() == float(want) and out[1].isnan() and _ws_tail_untouched(ws, 1024)


@pytest.mark.parametrize("n", E.ADAM_N)
def test_grad_accumulate(hip_lib, dev, n):
    print(f"eend_grad_accumulate_f32: n {n} -> blocks {(n + 255) // 256}, elements per block 256, passes 1")
    g1, g2 = E.ints((n,), n), E.ints((n,), n + 1)
    acc = _nan((n + 8,), F32, dev)
    assert _rc(hip_lib, "eend_grad_accumulate_f32", acc, _padrows(E.as_t(g1, F32), 8, NAN).to(dev), 0.5, 1, n) == 0        # first: NaN overwritten
    assert _same(acc, _padrows(g1.double() * 0.5, 8, NAN))
    assert _rc(hip_lib, "eend_grad_accumulate_f32", acc, _padrows(E.as_t(g2, F32), 8, NAN).to(dev), 0.25, 0, n) == 0
    assert _same(acc, _padrows(g1.double() * 0.5 + g2.double() * 0.25, 8, NAN))


@pytest.mark.parametrize("max_norm,gscale", [(5.0, 2.0), (5.0, 1e-3), (0.0, 2.0), (-1.0, 2.0)], ids=["clip_active", "clip_inactive", "max_norm_0", "max_norm_neg"])
@pytest.mark.parametrize("n", E.ADAM_N)
def test_adam_step(hip_lib, dev, n, max_norm, gscale):
    """three steps against float64; the clip coefficient is applied iff max_norm > 0 and the norm exceeds it"""
    L = hip_lib
    print(f"eend_adam_step_f32: n {n} -> blocks {(n + 255) // 256}, elements per block 256, passes 1")
    gen = torch.Generator().manual_seed(n)
    p64 = torch.randn(n, generator=gen).double()
    m64, v64 = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    p, m, v = (_padrows(t.float(), 8, NAN).to(dev) for t in (p64, m64, v64))
    p64 = p64.float().double()
    hp, ss = torch.zeros(4, device=dev), _nan((2,), F32, dev)
    ws = _ws(dev, 1024)
    for step in (1, 2, 3):
        g = torch.randn(n, generator=gen) * gscale * (10.0 if n == 1 else 1.0)
        gd = _padrows(g, 8, NAN).to(dev)
        assert _rc(L, "eend_grad_sumsq_f32", gd, n, ws, 1024, ss) == 0
        sumsq = float((g.double() ** 2).sum())
        clipped = max_norm > 0 and sumsq ** 0.5 > max_norm
        assert clipped == (max_norm > 0 and gscale > 1) or n < 255
        lr = 1e-3 * step
        hp.copy_(torch.tensor([lr, 1 - 0.9 ** step, 1 - 0.98 ** step, max_norm]))
        assert _rc(L, "eend_adam_step_f32", p, gd, m, v, n, hp, ss, 0.9, 0.98, 1e-9) == 0
        p64, m64, v64 = E.ref_adam(p64, g.double(), m64, v64, lr, step, max_norm, sumsq)
        assert p[n:].isnan().all() and m[n:].isnan().all() and v[n:].isnan().all(), "canary behind n"
        _bar("adam p abs", (p[:n].cpu().double() - p64).abs().max())
        _bar("adam m rel", (m[:n].cpu().double() - m64).abs().max() / m64.abs().max())
        _bar("adam v rel", (v[:n].cpu().double() - v64).abs().max() / v64.abs().max())


# ==================================================================================================== workspace contract
def test_one_float_less_than_the_documented_workspace_is_refused(hip_lib, dev):
    """every entry with a ws_floats argument: the minimum of include/eend_hip.h minus one float -> EEND_EINVAL, nothing written (the
    minimum itself, with a canary region behind it, is what every case above passes)"""
    L = hip_lib
    M, B, T, Tp, C, F, nseq, Tv, k = 8, 2, 5, 64, 3, 345, 2, 40, 7
    ws = _ws(dev, 1 << 20)
    out = [_nan((1 << 17,), F32, dev) for _ in range(5)]
    o16 = [_nan((1 << 17,), BF16, dev) for _ in range(2)]
    z32, z16, zb16 = torch.zeros(1 << 16, device=dev), torch.zeros(1 << 16, dtype=F16, device=dev), torch.zeros(1 << 16, dtype=BF16, device=dev)
    one = torch.ones(1 << 12, device=dev)
    x = torch.zeros(T, F, device=dev)
    ptrs, lens = torch.tensor([x.data_ptr()] * B, dtype=I64, device=dev), torch.tensor([T] * B, dtype=I32, device=dev)
    il = torch.tensor([T] * B, dtype=I32, device=dev)
    nb_bce, ns, nb16 = (B * Tp + 3) // 4, E.bn_splits(B * T)[0], E.bn16_blocks(nseq * Tv)[0]
    calls = {
        "eend_layernorm_bwd_f32": (1024 * 768, lambda w: _rc(L, "eend_layernorm_bwd_f32", z32, z16, one, one, out[0], o16[0], ws, w, out[1], out[2], out[3], M, None)),
        "eend_layernorm_bwd2_f32": (1024 * 768, lambda w: _rc(L, "eend_layernorm_bwd2_f32", z32, 0, z16, one, one, out[0], 0, o16[0], 1.0, ws, w, out[1], out[2], out[3], M, None)),
        "eend_resgrad_cast_bf16": (1024 * 256, lambda w: _rc(L, "eend_resgrad_cast_bf16", z32, o16[0], 1.0, ws, w, out[0], M, None)),
        "eend_head_bce_f32": (nb_bce, lambda w: _rc(L, "eend_head_bce_f32", one.new_ones(B * Tp * D), one.new_ones(B * C * Tp * D), z32, il, il.clamp(max=C), 0.1, None,
                                                    out[0], out[1], out[2], ws, w, out[3], B, T, Tp, C)),
        "eend_convert_fanout_bwd_f32": (256 * C * 256, lambda w: _rc(L, "eend_convert_fanout_bwd_f32", one.new_ones(B * C * Tp * D), o16[0], ws, w, out[0], B, Tp, C)),
        "eend_bn_train_stats_f32": ((ns + 1) * 2 * F, lambda w: _rc(L, "eend_bn_train_stats_f32", ptrs, lens, -1.0, ws, w, out[0], out[1], None, None, 0.1, B, T, F)),
        "eend_bn_bwd_f32": (ns * 2 * F, lambda w: _rc(L, "eend_bn_bwd_f32", ptrs, lens, -1.0, one, one, 0.0, zb16, 352, ws, w, out[0], out[1], B, T, Tp, F)),
        "eend_grad_sumsq_f32": (1024, lambda w: _rc(L, "eend_grad_sumsq_f32", z32, 1000, ws, w, out[0])),
        "eend_bn_batch_stats_f16": ((nb16 + 1) * 256, lambda w: _rc(L, "eend_bn_batch_stats_f16", z16, ws, w, out[0], nseq, Tp, Tv)),
        "eend_bn_swish_bwd_stats_bf16": (nb16 * 512, lambda w: _rc(L, "eend_bn_swish_bwd_stats_bf16", zb16, z16, one, one, 0.0, one, one, ws, w, out[0], out[1], out[2], nseq, Tp, Tv)),
        "eend_dwconv_glu_bwd_bf16": (nseq * 1 * 256 * k, lambda w: _rc(L, "eend_dwconv_glu_bwd_bf16", zb16, z16, one, o16[0], ws, w, out[0], nseq, Tp, Tv, k)),
    }
    for name, (minimum, call) in calls.items():
        assert call(minimum - 1) == EINVAL, name
    torch.cuda.synchronize()
    assert ws.isnan().all() and all(o.isnan().all() for o in out) and all(o.isnan().all() for o in o16)
    # ... and the same arguments with the minimum are served
    for name, (minimum, call) in calls.items():
        assert call(minimum) == 0, name
    torch.cuda.synchronize()
