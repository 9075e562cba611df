"""GPU: every weight-gradient entry (eend_wgrad_bf16, eend_wgrad_bias_bf16, eend_wgrad_bias_grouped_bf16, eend_conv1d_wgrad_bf16,
eend_colsum_f32; csrc/wgrad.hip) against the int64 reference of tests/wgrad_edge_ref.py, bit for bit, at the split, stage-ring, tile,
destination and tail edges.  The operands are small integers, so every f32 summation order gives the same bits (the guard
E.assert_exact checks that condition on the inputs of every case): there is no tolerance in this file, every comparison is
torch.equal, and a token row dropped, doubled or mispaired fails it (tests/test_wgrad_edges_ref.py shows that on the CPU).

Every case allocates its own NaN-filled workspace, sized to steer the planner (cap = ws_floats / (N K [+ N]) splits), prints the plan
eend_wgrad_plan reports and asserts the plan class the case was written for.  Outputs are pre-filled with NaN, or with known integers
where the call accumulates."""
import ctypes
import functools

import pytest
import torch

from tests import wgrad_edge_ref as E

pytestmark = pytest.mark.gpu
F16, BF16, F32, I32 = torch.float16, torch.bfloat16, torch.float32, torch.int32
NAN = float("nan")
EINVAL = -1
GEMM = E.gemm_cases()


def _rc(L, name, *args):
    """one C-ABI call on the current stream -> its return code"""
    a = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in args]
    return getattr(L, name)(*a, torch.cuda.current_stream().cuda_stream)


def _plan(L, M, N, K, cin, ws_floats, bias):
    t, n, m = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    assert L.eend_wgrad_plan(M, N, K, cin, ws_floats, int(bias), ctypes.byref(t), ctypes.byref(n), ctypes.byref(m)) == 0
    return t.value, n.value, m.value


def _assert_plan(L, what, M, N, K, cin, ws_floats, bias, want):
    got = _plan(L, M, N, K, cin, ws_floats, bias)
    print(f"{what}: M {M} N {N} K {K} ws {ws_floats} bias {int(bias)} -> tile {got[0]} nsplit {got[1]} m_per_split {got[2]} (case: {want})")
    assert got == tuple(want), what


def _same(got, want):
    """bit-for-bit up to the sign of zero; NaN (the pre-fill) must sit exactly where it is expected"""
    got, want = got.cpu(), want.cpu()
    return got.shape == want.shape and torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(0.0), want.nan_to_num(0.0))


def _ws(dev, n):
    return torch.full((n,), NAN, dtype=F32, device=dev)


def _prefill(shape, acc):
    """NaN, or small known integers for an accumulating call"""
    if not acc:
        return torch.full(shape, NAN, dtype=F32)
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n) * 7) % 5 - 2).float().view(shape)


@functools.lru_cache(maxsize=8)
def _operands(M, N, K):
    """(dY, X, dW, db) as int64 on the CPU: computed once per shape, never modified"""
    dy, x = E.ints((M, N), 1000 + M), E.ints((M, K), 2000 + M)
    assert (dy != 0).all() and (x != 0).all()
    return dy, x, E.ref_dw(dy, x), E.ref_db(dy)


def _run(L, dev, c, *, bias, f16, K_out=None, ld_out=None, scale=1.0, acc=0, tag=""):
    """one eend_wgrad[_bias]_bf16 call of a table case: plan class, weight (and bias) gradient, untouched surroundings"""
    M, N, K = c["M"], c["N"], c["K"]
    K_out = K if K_out is None else K_out
    ld_out = K_out if ld_out is None else ld_out
    dy, x, dw, db = _operands(M, N, K)
    E.assert_exact(dy, x, extra=2)
    assert 2 * E.assert_exact(dy, x) + 2 < E.LIMIT                        # |scale| <= 2, pre-fill <= 2
    wsf = E.ws_floats(c, bias)
    _assert_plan(L, E.case_id(c) + tag, M, N, K, 0, wsf, bias, (c["tile"], c["nsplit"], c["mps"]))
    dy16, x16 = E.as16(dy, BF16).to(dev), E.as16(x, F16 if f16 else BF16).to(dev)
    ws = _ws(dev, wsf)
    out0, b0 = _prefill((N, ld_out), acc), _prefill((N,), acc)
    out, bo = out0.to(dev), b0.to(dev)
    if bias:
        rc = _rc(L, "eend_wgrad_bias_bf16", dy16, N, x16, K, int(f16), M, N, K, ws, wsf, out, ld_out, K_out, bo, scale, acc)
    else:
        rc = _rc(L, "eend_wgrad_bf16", dy16, N, x16, K, int(f16), M, N, K, ws, wsf, out, ld_out, K_out, scale, acc)
    assert rc == 0
    want = out0.clone()
    want[:, :K_out] = (out0[:, :K_out] if acc else 0) + scale * dw[:, :K_out].float()
    assert _same(out, want), "weight gradient"
    if bias:
        assert _same(bo, (b0 if acc else 0) + scale * db.float()), "bias gradient"
    else:
        assert _same(bo, b0)


# ---- a. one split: 1 .. 32 stages (under the three-stage prologue, exactly the ring, several ring wraps)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("c", [c for c in GEMM if c["group"] == "a"], ids=E.case_id)
def test_single_split_stage_ring(hip_lib, dev, c, f16, bias):
    assert c["nsplit"] == 1
    _run(hip_lib, dev, c, bias=bias, f16=f16)


# ---- b. split-count classes: both block -> split mappings, every remainder of the reductions, capped plans with long splits
@pytest.mark.parametrize("c", [c for c in GEMM if c["group"] == "b"], ids=E.case_id)
def test_split_count_classes(hip_lib, dev, c):
    f16 = bool((c["M"] + c["nsplit"]) & 1)
    _run(hip_lib, dev, c, bias=True, f16=f16, tag=" bias")
    _run(hip_lib, dev, c, bias=False, f16=not f16)


# ---- c. several tiles, N != K: tile order, the bias of every n-tile, nothing from k-tiles >= 1
@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("c", [c for c in GEMM if c["group"] == "c"], ids=E.case_id)
def test_tile_order_and_asymmetry(hip_lib, dev, c, f16):
    _run(hip_lib, dev, c, bias=True, f16=f16)


# ---- d. the 256 tile: one workgroup per tile over ~514 stages, 16 splits; 256-aligned shapes that keep the 128 tile
@pytest.mark.parametrize("c", [c for c in GEMM if c["group"] == "d"], ids=E.case_id)
def test_big_tile(hip_lib, dev, c):
    assert c["tile"] == (256 if c["M"] >= 16384 and c["K"] == 512 else 128)
    _run(hip_lib, dev, c, bias=True, f16=bool(c["M"] & 1))
    if c["cap"] == 1:
        _run(hip_lib, dev, c, bias=False, f16=not (c["M"] & 1))


# ---- e. destination forms on both tiles
_E128 = E._case("e", 200, 128, 384, E.GENEROUS, 128, 4, 64)
_E256 = E._case("e", 16384 + 33, 256, 512, 16, 256, 16, 1088)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("form", ["narrow", "narrow_gap_acc", "full_acc"])
@pytest.mark.parametrize("c", [_E128, _E256], ids=E.case_id)
def test_destination_forms(hip_lib, dev, c, form, bias):
    K = c["K"]
    K_out = 345 if K == 384 else 473
    if form == "narrow":                                   # K_out < K, ld_out == K_out: columns >= K_out do not exist
        _run(hip_lib, dev, c, bias=bias, f16=True, K_out=K_out, ld_out=K_out, scale=0.5)
    elif form == "narrow_gap_acc":                         # ld_out > K: the row gaps keep their integers
        _run(hip_lib, dev, c, bias=bias, f16=False, K_out=K_out, ld_out=K + 8, scale=2.0, acc=1)
    else:
        _run(hip_lib, dev, c, bias=bias, f16=True, scale=-1.0, acc=1)


# ---- f. operand forms
@pytest.mark.parametrize("f16", [True, False])
def test_column_blocks_of_wider_tensors(hip_lib, dev, f16):
    L, M, N, K = hip_lib, 200, 128, 256
    wsf = E.GENEROUS * (N * K + N)
    _assert_plan(L, "column blocks", M, N, K, 0, wsf, True, (128, 4, 64))
    wdy, wx = E.ints((M, 3 * N), 31), E.ints((M, 2 * K), 32)                # non-zero neighbours on both sides
    dy, x = wdy[:, N:2 * N], wx[:, K:]
    E.assert_exact(dy, x)
    dyd, xd = E.as16(wdy, BF16).to(dev), E.as16(wx, F16 if f16 else BF16).to(dev)
    out, bo = _prefill((N, K), 0).to(dev), _prefill((N,), 0).to(dev)
    assert _rc(L, "eend_wgrad_bias_bf16", dyd[:, N:], 3 * N, xd[:, K:], 2 * K, int(f16), M, N, K, _ws(dev, wsf), wsf, out, K, K, bo, 1.0, 0) == 0
    assert torch.equal(out.cpu(), E.ref_dw(dy, x).float()) and torch.equal(bo.cpu(), E.ref_db(dy).float())


@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("M", [208, 193, 207])
@pytest.mark.parametrize("which", ["x", "x_wide", "dy", "dy_zero_pad_bias"])
def test_blocked_operands(hip_lib, dev, which, M, f16):
    """a blocked operand with non-zero padding rows (M % 16 in {0, 1, 15}); the row-major operand holds non-zero rows behind M, which
    must read as zero.  The bias of a blocked dY is asserted with zero padding rows only: that is the entry's contract."""
    L, N, K = hip_lib, 128, 128
    Mp = (M + 15) // 16 * 16
    bias = which == "dy_zero_pad_bias"
    wsf = E.GENEROUS * (N * K + (N if bias else 0))
    _assert_plan(L, f"blocked {which}", M, N, K, 0, wsf, bias, (128, 4, 64))
    dy, x = E.ints((Mp + 64, N), 41 + M), E.ints((Mp + 64, 2 * K if which == "x_wide" else K), 42 + M)
    E.assert_exact(dy[:M], x[:M])
    xt = F16 if f16 else BF16
    out, bo = _prefill((N, K), 0).to(dev), _prefill((N,), 0).to(dev)
    if which in ("x", "x_wide"):                            # x_wide: the first K features of a blocked tensor of 2 K
        xb = E.to_blocked(E.as16(x[:M], xt), pad=3.0).to(dev)
        assert xb.shape[0] == Mp
        rc = _rc(L, "eend_wgrad_bf16", E.as16(dy, BF16).to(dev), N, xb, x.shape[1], int(f16) | 2, M, N, K, _ws(dev, wsf), wsf, out, K, K, 1.0, 0)
    else:
        dyb = E.to_blocked(E.as16(dy[:M], BF16), pad=0.0 if bias else 3.0).to(dev)
        xd = E.as16(x, xt).to(dev)
        if bias:
            rc = _rc(L, "eend_wgrad_bias_bf16", dyb, N, xd, K, int(f16) | 4, M, N, K, _ws(dev, wsf), wsf, out, K, K, bo, 1.0, 0)
        else:
            rc = _rc(L, "eend_wgrad_bf16", dyb, N, xd, K, int(f16) | 4, M, N, K, _ws(dev, wsf), wsf, out, K, K, 1.0, 0)
    assert rc == 0
    assert torch.equal(out.cpu(), E.ref_dw(dy[:M], x[:M, :K]).float())
    if bias:
        assert torch.equal(bo.cpu(), E.ref_db(dy[:M]).float())


# ---- g. grouped entry
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("group_rows", [128, 256])
def test_grouped(hip_lib, dev, group_rows, scale):
    L, M, N, K = hip_lib, 200, 512, 128
    ng = N // group_rows
    stride = group_rows * K + group_rows + 64                # weight, bias, and a gap that must keep its pre-fill
    wsf = E.GENEROUS * (N * K + N)
    plan = (128, 4, 64)
    _assert_plan(L, f"grouped {group_rows}", M, N, K, 0, wsf, True, plan)
    dy, x, dw, db = _operands(M, N, K)
    E.assert_exact(dy, x)
    dy16, x16 = E.as16(dy, BF16).to(dev), E.as16(x, F16).to(dev)
    buf = torch.full((ng * stride,), NAN, dtype=F32, device=dev)
    assert _rc(L, "eend_wgrad_bias_grouped_bf16", dy16, N, x16, K, 1, M, N, K, _ws(dev, wsf), wsf, buf, buf[group_rows * K:], group_rows, stride, scale) == 0
    want = torch.full((ng, stride), NAN, dtype=F32)
    for g in range(ng):
        want[g, :group_rows * K] = scale * dw[g * group_rows:(g + 1) * group_rows].float().reshape(-1)
        want[g, group_rows * K:group_rows * K + group_rows] = scale * db[g * group_rows:(g + 1) * group_rows].float()
    assert _same(buf, want.view(-1))
    # the ungrouped calls on the column blocks of dY, same plan: the same bits
    w1f = E.GENEROUS * (group_rows * K + group_rows)
    _assert_plan(L, "ungrouped", M, group_rows, K, 0, w1f, True, plan)
    for g in range(ng):
        w1, b1 = _prefill((group_rows, K), 0).to(dev), _prefill((group_rows,), 0).to(dev)
        assert _rc(L, "eend_wgrad_bias_bf16", dy16[:, g * group_rows:], N, x16, K, 1, M, group_rows, K, _ws(dev, w1f), w1f, w1, K, K, b1, scale, 0) == 0
        assert torch.equal(w1.view(-1), buf[g * stride:g * stride + group_rows * K])
        assert torch.equal(b1, buf[g * stride + group_rows * K:g * stride + group_rows * K + group_rows])


# ---- h. Conv1d form
@pytest.mark.parametrize("c", E.conv_cases(), ids=E.conv_id)
def test_conv1d_wgrad(hip_lib, dev, c):
    """X holds non-zero integers in every frame: those at or beyond ilen are poison.  dY is non-zero in every frame, including frames
    >= ilen, which legitimately contribute through the in-range X frames their taps reach."""
    L, nseq, Tp, kt, pad = hip_lib, c["nseq"], c["Tp"], c["ktaps"], c["pad"]
    M, K = nseq * Tp, kt * 256
    wsf = c["cap"] * 256 * K
    _assert_plan(L, E.conv_id(c), M, 256, K, 256, wsf, False, (c["tile"], c["nsplit"], c["mps"]))
    dy, x = E.ints((M, 256), 7 + M), E.ints((M, 256), 8 + M)
    assert (dy != 0).all() and (x != 0).all() and all(0 <= i <= Tp for i in c["ilens"])
    E.assert_exact(dy, x)
    want = E.ref_conv_dw(dy, x, nseq, Tp, c["ilens"], kt, pad, via_f64=M >= 16384)
    il = torch.tensor(c["ilens"], dtype=I32, device=dev)
    tmp, out = _ws(dev, 256 * K), torch.full((256, 256, kt), NAN, dtype=F32, device=dev)
    rc = _rc(L, "eend_conv1d_wgrad_bf16", E.as16(dy, BF16).to(dev), E.as16(x, F16).to(dev), il, nseq, Tp, 256, kt, pad, _ws(dev, wsf), wsf, tmp, out)
    assert rc == 0
    assert torch.equal(out.cpu(), want.float())


# ---- i. eend_colsum_f32
@pytest.mark.parametrize("M,N,ns", E.COLSUM_CASES)
def test_colsum(hip_lib, dev, M, N, ns):
    L, ld = hip_lib, N + 8
    assert min(ns, 1024, (M + 63) // 64) == ns               # what the entry makes of a workspace of ns * N floats
    y = E.ints((M, ld), 50 + M + N)                          # non-zero neighbours in the columns >= N
    want = E.ref_db(y[:, :N]).float()
    assert 2 * int(y.abs().sum(0).max()) + 2 < E.LIMIT
    for bf, scale, acc in ((1, 1.0, 0), (0, -0.5, 1), (1, 2.0, 1), (0, 1.0, 0)):
        o0 = _prefill((N + 8,), acc)
        out = o0.to(dev)
        assert _rc(L, "eend_colsum_f32", E.as16(y, BF16 if bf else F16).to(dev), ld, M, N, bf, _ws(dev, ns * N), ns * N, out, scale, acc) == 0
        w = o0.clone()
        w[:N] = (o0[:N] if acc else 0) + scale * want
        assert _same(out, w), (bf, scale, acc)


# ---- j. conversion pins
@pytest.mark.parametrize("M,plan", [(64, (128, 1, 64)), (4096, (128, 64, 64))])
def test_f16_to_bf16_rounds_to_nearest_even(hip_lib, dev, M, plan):
    L, N, K = hip_lib, 128, 128
    wsf = E.GENEROUS * N * K
    _assert_plan(L, "ties", M, N, K, 0, wsf, False, plan)
    x = E.as16(E.tie_x(M, K, M), F16)
    dy = E.ints((M, N), M + 1, vals=(-1, 0, 1))
    xr = x.to(BF16).to(E.I64)                                # torch rounds to nearest even
    E.assert_exact(dy, xr)
    out = _prefill((N, K), 0).to(dev)
    assert _rc(L, "eend_wgrad_bf16", E.as16(dy, BF16).to(dev), N, x.to(dev), K, 1, M, N, K, _ws(dev, wsf), wsf, out, K, K, 1.0, 0) == 0
    assert torch.equal(out.cpu(), E.ref_dw(dy, xr).float())


@pytest.mark.parametrize("e", E.DY_SCALE_EXPONENTS)
def test_scaled_dy_never_passes_through_f16(hip_lib, dev, e):
    L, M, N, K = hip_lib, 1000, 128, 128
    wsf = E.GENEROUS * (N * K + N)
    _assert_plan(L, "scaled dY", M, N, K, 0, wsf, True, (128, 16, 64))
    dy, x, dw, db = _operands(M, N, K)
    E.assert_exact(dy, x)
    dys = E.as16(dy.double() * 2.0 ** e, BF16)
    out, bo = _prefill((N, K), 0).to(dev), _prefill((N,), 0).to(dev)
    assert _rc(L, "eend_wgrad_bias_bf16", dys.to(dev), N, E.as16(x, F16).to(dev), K, 1, M, N, K, _ws(dev, wsf), wsf, out, K, K, bo, 1.0, 0) == 0
    assert torch.equal(out.cpu().double(), dw.double() * 2.0 ** e) and torch.equal(bo.cpu().double(), db.double() * 2.0 ** e)


# ---- k. rejections: argument checks made before any launch, on buffers that would keep every access in bounds anyway
def test_rejections(hip_lib, dev):
    L, M, N, K = hip_lib, 100, 128, 128
    dy = E.as16(E.ints((256, 512), 61), BF16).to(dev)
    x = E.as16(E.ints((256, 512), 62), F16).to(dev)
    wsf = 1 << 20
    ws = _ws(dev, wsf)
    out = torch.full((512 * 512,), 7.0, dtype=F32, device=dev)
    bo = torch.full((512,), 7.0, dtype=F32, device=dev)

    def plain(dY=dy, lda=512, X=x, ldb=512, fl=1, N=N, K=K, wsf=wsf, ld_out=K, K_out=K):
        return _rc(L, "eend_wgrad_bf16", dY, lda, X, ldb, fl, M, N, K, ws, wsf, out, ld_out, K_out, 1.0, 0)

    def biased(dY=dy, lda=512, X=x, ldb=512, fl=1, N=N, K=K, wsf=wsf, ld_out=K, K_out=K):
        return _rc(L, "eend_wgrad_bias_bf16", dY, lda, X, ldb, fl, M, N, K, ws, wsf, out, ld_out, K_out, bo, 1.0, 0)

    def grouped(group_rows=128, stride=256 * 128 + 512, N=256):
        return _rc(L, "eend_wgrad_bias_grouped_bf16", dy, 512, x, 512, 1, M, N, K, ws, wsf, out, out[128 * 128:], group_rows, stride, 1.0)

    for f in (plain, biased):
        bad = {
            "N % 128": dict(N=64), "K % 128": dict(K=192),
            "workspace under one tile": dict(wsf=N * K - 1 if f is plain else N * K + N - 1),
            "lda % 8": dict(lda=516), "ldb % 8": dict(ldb=516),
            "dY not 16-byte aligned": dict(dY=dy.view(-1)[4:]), "X not 16-byte aligned": dict(X=x.view(-1)[4:]),
            "blocked X, ld % 32": dict(fl=3, ldb=488), "blocked dY, ld % 32": dict(fl=5, lda=488),
            "blocked dY, N > lda": dict(fl=5, lda=96), "blocked X, K > ldb": dict(fl=3, ldb=96),
            "K_out > K": dict(K_out=K + 1, ld_out=K + 1), "ld_out < K_out": dict(ld_out=K - 1),
        }
        for what, kw in bad.items():
            assert f(**kw) == EINVAL, (f.__name__, what)
    for what, kw in {"group_rows does not divide N": dict(group_rows=96), "group_stride < group_rows * K": dict(stride=128 * 128 - 1, N=256)}.items():
        assert grouped(**kw) == EINVAL, what
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (bo == 7.0).all() and ws.isnan().all()
    # ... and the arguments the rejected calls were derived from are served
    assert plain() == 0 and biased() == 0 and biased(fl=3) == 0 and grouped() == 0
    torch.cuda.synchronize()
    assert not out[:N * K].isnan().any() and (out[:N * K] != 7.0).any()
