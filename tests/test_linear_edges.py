"""GPU: every kernel a linear entry point of csrc/api.hip can dispatch to -- skinny.hip (plain, split-K, f32 row groups), proj.hip,
the 128x128 GEMM tile (straight-line at K = 256 and looped), the 64x256 whole-row tile, convert_rows.hip and the f32 MFMA kernel
(plain and split-K) -- against the exact reference of tests/linear_edge_ref.py, at its row-bucket, tile, k-tile, stride, workgroup-count
and tail edges.

The operands are small integers (E.assert_exact guards that on the inputs of every case), so everything linear is compared with
torch.equal: plain / ReLU / residual-scale outputs, Q / K / V^T / K^T head rows, the slot fan-out, saturated GLU, the un-normalised
stream of the pre-norm joins.  Values behind exp / rsqrt / sigmoid use the tolerances of the existing tests of the same entries
(E.TOL) against float64; each figure is printed before it is asserted.  Every case prints and asserts the route eend_linear_route
reports for the very pointers it passes, pre-fills its outputs with NaN and checks the guard rows behind row M and the guard columns
beyond N: NaN must sit exactly where nothing may be written."""
import pytest
import torch

from tests import linear_edge_ref as E

pytestmark = pytest.mark.gpu
F16, BF16, F32, I32 = torch.float16, torch.bfloat16, torch.float32, torch.int32
NAN = float("nan")
EINVAL = -1


def _cases(entries, routes=None):
    return [c for c in E.all_cases() if c["entry"] in entries and (routes is None or c["route"] in routes)]


def _rc(L, name, *args):
    """one C-ABI call on the current stream -> its return code"""
    a = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in args]
    return getattr(L, name)(*a, torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype, dev, ld=None):
    """float64 [R][C] (or a vector) -> device tensor of `dtype`, rows `ld` apart with non-zero fill between C and ld; nothing rounds"""
    if t is None:
        return None
    if t.dim() == 2 and ld is not None and ld != t.shape[1]:
        buf = torch.full((t.shape[0], ld), float(E.PAD_FILL), dtype=torch.float64)
        buf[:, :t.shape[1]] = t
        t = buf
    r = t.to(dtype)
    assert torch.equal(r.double(), t), "operand not exact"
    return r.to(dev)


def _offset_vec(t, dev, off_bytes):
    """f32 vector whose address is off_bytes past a 16-byte boundary"""
    n = off_bytes // 4
    buf = torch.zeros(t.numel() + n, dtype=F32, device=dev)
    buf[n:] = t.float().to(dev)
    v = buf[n:]
    assert v.data_ptr() % 16 == off_bytes
    return v


def _nan(shape, dtype, dev):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=dev)


def _bits(t):
    return E_NULL if t is None else t.data_ptr() & 15


E_NULL = -1


def _assert_route(c, **ptrs):
    """print and assert the route of the call about to be made: the table's fields with the address bits of the real pointers"""
    from fs_eend_amd import lib as L
    fields = E.route_fields(c, **{k: _bits(v) for k, v in ptrs.items()})
    got = L.linear_route(c["entry"], **fields)
    print(f"{E.case_id(c)}: route {got} (case: {c['route']})")
    assert got == c["route"], E.case_id(c)


def _check(c, got, want):
    """every output buffer of the case against the reference: bitwise where linear, E.TOL elsewhere (figures printed first)"""
    exact = E.exact_outputs(c)
    assert set(got) == set(want)
    torch.cuda.synchronize()
    for name, g in got.items():
        g = g.cpu().double().view(want[name].shape)
        if name in exact:
            assert E.same(g, want[name]), f"{E.case_id(c)}: {name} differs from the exact reference"
        else:
            tol = E.tolerance(c, name)
            ok, err, bound = E.within(g, want[name], tol)
            print(f"{E.case_id(c)}: {name} max |err| {err:.3e} (bound {bound:.3e}, {tol})")
            assert ok, f"{E.case_id(c)}: {name} max |err| {err:.3e} > {bound:.3e} or NaN misplaced"


# ------------------------------------------------------------------------------------------------ the runners, one per family
def _run_plain(L, dev, c):
    o, want = E.operands(c), E.reference(c)
    dt = F32 if c["entry"] == "linear_step_f32" else F16
    A, W = _dev(o["A"], dt, dev, c["lda"]), _dev(o["W"], dt, dev, c["ldw"])
    bias = None if o["bias"] is None else _offset_vec(o["bias"], dev, c.get("bias_off") or 0)
    out = _nan(want["out"].shape, dt, dev)
    if dt == F32:
        _assert_route(c, a=A, w=W, bias=bias, out_f32=out)
    else:
        _assert_route(c, a=A, w=W, bias=bias, out_f16=out)
    assert _rc(L, "eend_" + c["entry"], A, c["lda"], W, c["ldw"], bias, out, c["ldo"], c["M"], c["N"], c["K"], c["act"]) == 0
    _check(c, {"out": out}, want)
    return out


def _run_glu(L, dev, c):
    o, want = E.operands(c), E.reference(c)
    A, W, bias = _dev(o["A"], F16, dev, c["lda"]), _dev(o["W"], F16, dev, c["ldw"]), _dev(o["bias"], F32, dev)
    out = _nan(want["out"].shape, F16, dev)
    _assert_route(c, a=A, w=W, bias=bias, out_f16=out)
    assert _rc(L, "eend_linear_glu_f16", A, c["lda"], W, c["ldw"], bias, out, c["ldo"], c["M"], c["N"], c["K"]) == 0
    _check(c, {"out": out}, want)


def _run_heads(L, dev, c):
    o, want = E.operands(c), E.reference(c)
    A, W, bias = _dev(o["A"], F16, dev, c["lda"]), _dev(o["W"], F16, dev, c["ldw"]), _dev(o["bias"], F32, dev)
    dt = BF16 if c["entry"] == "inproj_heads_bf16" else F16
    tail = 512                                           # NaN elements behind every head buffer
    bufs = {k: _nan((v.numel() + tail,), dt, dev) for k, v in want.items()}
    _assert_route(c, a=A, w=W, bias=bias, out_f16=bufs["Q"])
    shape = (c["nseq"], c["Tp"], c["H"], 64, c["K"])
    if c["entry"] == "inproj_heads_bf16":
        rc = _rc(L, "eend_inproj_heads_bf16", A, c["lda"], W, c["ldw"], bias, bufs["Q"], bufs["K"], bufs["Vt"], *shape)
    else:
        rc = _rc(L, "eend_retention_proj_f16", A, c["lda"], W, c["ldw"], bias, bufs["Q"], bufs["K"], bufs["Kt"], bufs["Vt"], bufs["G"], *shape)
    assert rc == 0
    for k, b in bufs.items():
        assert b[-tail:].isnan().all(), f"{E.case_id(c)}: wrote behind {k}"
    got = {k: b[:-tail] for k, b in bufs.items()}
    _check(c, got, want)
    return got


def _run_res(L, dev, c):
    o, want = E.operands(c), E.reference(c)
    e = c["entry"]
    step = e.endswith("_step_f32")
    dt = F32 if step else F16
    A, W = _dev(o["A"], dt, dev, c["lda"]), _dev(o["W"], dt, dev, c["ldw"])
    bias = None if o["bias"] is None else _offset_vec(o["bias"], dev, c.get("bias_off") or 0)
    gamma, beta = _dev(o["gamma"], F32, dev), _dev(o["beta"], F32, dev)
    rows = c["M"] + E.GUARD_ROWS
    out32 = _nan((rows, 256), F32, dev) if c["out32"] else None
    out16 = _nan((rows, 256), F16, dev) if c["out16"] else None
    res = _dev(o["res"], F16 if e == "linear_res16_ln_f16" else F32, dev)
    if c.get("alias"):                                   # the residual stream updated in place: out_f32 IS res
        out32[:c["M"]] = res
        res = out32
    _assert_route(c, a=A, w=W, bias=bias, res=res, gamma=gamma, beta=beta, out_f32=out32, out_f16=out16)
    head = (A, c["lda"], W, c["ldw"], bias, res, c["alpha"])
    got = {}
    if e == "linear_res_scale_f16":
        rc = _rc(L, "eend_" + e, *head, out32, out16, c["M"], c["K"])
    elif e == "linear_res_scale_ln_step_f32":
        got["ln32"] = _nan((rows, 256), F32, dev)
        rc = _rc(L, "eend_" + e, *head, gamma, beta, c["eps"], out32, got["ln32"], out16, c["M"], c["K"])
    else:
        rc = _rc(L, "eend_" + e, *head, gamma, beta, c["eps"], out32, out16, c["M"], c["K"])
    assert rc == 0
    if out32 is not None:
        got["out32"] = out32
    if out16 is not None:
        got["out16"] = out16
    _check(c, got, want)


def _run_fanout(L, dev, c):
    o, want = E.operands(c), E.reference(c)
    A, W, pc = _dev(o["A"], F16, dev), _dev(o["W"], F16, dev), _dev(o["pc"], F32, dev)
    got = {"out16": _nan(want["out16"].shape, F16, dev)}
    if c["out32"]:
        got["out32"] = _nan(want["out32"].shape, F32, dev)
    _assert_route(c, a=A, w=W, res=pc, out_f32=got.get("out32"), out_f16=got["out16"])
    assert _rc(L, "eend_convert_fanout_f16", A, W, pc, got.get("out32"), got["out16"], c["B"], c["Tp"], c["C"]) == 0
    _check(c, got, want)
    return got


def _run_conv(L, dev, c):
    o, want = E.operands(c), E.reference(c)
    X, W, bias = _dev(o["A"], F16, dev), _dev(o["W"], F16, dev), _dev(o["bias"], F32, dev)
    il = torch.tensor(c["ilens"], dtype=I32, device=dev)
    got = {"out32": _nan(want["out32"].shape, F32, dev), "out16": _nan(want["out16"].shape, F16, dev)}
    print(f"{E.case_id(c)}: one kernel (64x256 tile, implicit-GEMM loads), no route")
    assert _rc(L, "eend_conv1d_l2norm_f16", X, W, bias, il, got["out32"], got["out16"], c["nseq"], c["Tp"], c["cin"], c["ktaps"], c["pad"]) == 0
    _check(c, got, want)


# ------------------------------------------------------------------------------------------------ eend_linear_f16
@pytest.mark.parametrize("c", _cases({"linear_f16"}, {"skinny", "skinny_splitk"}), ids=E.case_id)
def test_linear_skinny(hip_lib, dev, c):
    _run_plain(hip_lib, dev, c)


@pytest.mark.parametrize("c", _cases({"linear_f16"}, {"proj"}), ids=E.case_id)
def test_linear_proj(hip_lib, dev, c):
    _run_plain(hip_lib, dev, c)


@pytest.mark.parametrize("c", [c for c in _cases({"linear_f16"}, {"gemm128_straight", "gemm128_looped"}) if not (c.get("why") or "").startswith("wg")],
                         ids=E.case_id)
def test_linear_gemm_tile(hip_lib, dev, c):
    _run_plain(hip_lib, dev, c)


@pytest.mark.parametrize("c", [c for c in _cases({"linear_f16"}) if (c.get("why") or "").startswith("wg")], ids=E.case_id)
def test_linear_gemm_workgroup_counts(hip_lib, dev, c):
    """every workgroup count 1 .. 17 (and 6, 9, 12, 15 over three tile columns) through xcd_remap, a tail of 123 rows in the last tile"""
    nwg = (c["M"] + 127) // 128 * (c["N"] // 128)
    assert f"wg{nwg}" == c["why"]
    _run_plain(hip_lib, dev, c)


def test_linear_boundary_pairs_agree(hip_lib, dev):
    """the same rows on either side of a routing boundary: bit for bit the same result (both equal the exact reference)"""
    L = hip_lib
    from fs_eend_amd import lib as lib_
    A64, W64, b64 = E.ints((17, 256), 11), E.ints((1280, 256), 12), E.ints((1280,), 13, E.V3)
    E.assert_exact(A64, W64, b64)
    A, bias = _dev(A64, F16, dev), _dev(b64, F32, dev)
    want = A64 @ W64.t() + b64

    def call(M, N, ldw):
        W = _dev(W64[:N], F16, dev, ldw)
        out = _nan((M + E.GUARD_ROWS, N), F16, dev)
        route = lib_.linear_route("linear_f16", M=M, N=N, K=256, lda=256, ldw=ldw, ldo=N, a=_bits(A), w=_bits(W), bias=_bits(bias), out_f16=_bits(out))
        assert _rc(L, "eend_linear_f16", A, 256, W, ldw, bias, out, N, M, N, 256, 0) == 0
        torch.cuda.synchronize()
        assert out[M:].isnan().all() and E.same(out[:M].cpu(), want[:M, :N])
        return route, out[:M]

    (r16, o16), (r17, o17) = call(16, 256, 256), call(17, 256, 256)
    (r1024, o1024), (r1280, o1280) = call(17, 1024, 256), call(17, 1280, 256)
    r264, o264 = call(17, 256, 264)
    print(f"M 16 | 17: {r16} | {r17};  N 1024 | 1280: {r1024} | {r1280};  ldw 256 | 264: {r17} | {r264}")
    assert (r16, r17, r1024, r1280, r264) == ("skinny", "proj", "proj", "gemm128_straight", "gemm128_straight")
    assert torch.equal(o16, o17[:16]) and torch.equal(o1024, o1280[:, :1024]) and torch.equal(o17, o264)


# ------------------------------------------------------------------------------------------------ eend_linear_glu_f16
@pytest.mark.parametrize("c", _cases({"linear_glu_f16"}), ids=E.case_id)
def test_linear_glu(hip_lib, dev, c):
    _run_glu(hip_lib, dev, c)


# ------------------------------------------------------------------------------------------------ the head-row entries
@pytest.mark.parametrize("c", _cases({"inproj_heads_bf16", "retention_proj_f16"}), ids=E.case_id)
def test_head_rows(hip_lib, dev, c):
    _run_heads(hip_lib, dev, c)


@pytest.mark.parametrize("entry", ["inproj_heads_bf16", "retention_proj_f16"])
@pytest.mark.parametrize("nseq,Tp", [(3, 64), (2, 128)])
def test_head_rows_both_routes_agree(hip_lib, dev, entry, nseq, Tp):
    """K = 256, H = 4 through proj.hip (ldw = 256) and through the GEMM tile (the same weight rows 264 apart): the same bits"""
    L = hip_lib
    from fs_eend_amd import lib as lib_
    nout = 768 if entry == "inproj_heads_bf16" else 1024
    vals = E.V1 if entry == "inproj_heads_bf16" else E.V2
    A64, W64, b64 = E.ints((nseq * Tp, 256), 21, vals), E.ints((nout, 256), 22, vals), E.ints((nout,), 23, E.V3)
    E.assert_exact(A64, W64, b64)
    A, bias = _dev(A64, F16, dev), _dev(b64, F32, dev)
    dt = BF16 if entry == "inproj_heads_bf16" else F16
    res = []
    for ldw in (256, 264):
        W = _dev(W64, F16, dev, ldw)
        bufs = [_nan((nseq * Tp * 256,), dt, dev) for _ in range(3 if nout == 768 else 5)]
        route = lib_.linear_route(entry, nseq=nseq, Tp=Tp, H=4, dh=64, K=256, lda=256, ldw=ldw, a=_bits(A), w=_bits(W))
        assert _rc(L, "eend_" + entry, A, 256, W, ldw, bias, *bufs, nseq, Tp, 4, 64, 256) == 0
        torch.cuda.synchronize()
        res.append((route, bufs))
    print(f"{entry} ({nseq}, {Tp}): ldw 256 -> {res[0][0]}, ldw 264 -> {res[1][0]}")
    assert (res[0][0], res[1][0]) == ("proj", "gemm128_straight")
    for a, b in zip(res[0][1], res[1][1]):
        assert not a.isnan().any() and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the four residual entries
@pytest.mark.parametrize("c", _cases({"linear_res_ln_f16", "linear_res16_ln_f16", "linear_res_scale_f16", "linear_res_scale_ln16_f16"}), ids=E.case_id)
def test_residual_entries(hip_lib, dev, c):
    _run_res(hip_lib, dev, c)


# ------------------------------------------------------------------------------------------------ eend_conv1d_l2norm_f16
@pytest.mark.parametrize("c", _cases({"conv1d_l2norm_f16"}), ids=E.case_id)
def test_conv1d_l2norm(hip_lib, dev, c):
    _run_conv(hip_lib, dev, c)


# ------------------------------------------------------------------------------------------------ eend_convert_fanout_f16
@pytest.mark.parametrize("c", _cases({"convert_fanout_f16"}), ids=E.case_id)
def test_convert_fanout(hip_lib, dev, c):
    _run_fanout(hip_lib, dev, c)


def test_convert_fanout_first_slots_do_not_depend_on_the_kernel(hip_lib, dev):
    """C = 33 (EPI_CONVERT) and C = 32 (rows kernel) on the same embeddings and slot constants: the first 32 slots agree bit for bit"""
    L = hip_lib
    B, Tp = 2, 64
    E64, W64, pc64 = E.ints((B * Tp, 256), 31), E.ints((256, 256), 32), E.ints((33, 256), 33, E.V3) * 8
    E.assert_exact(E64, W64, pc64)
    Ed, W, pc = _dev(E64, F16, dev), _dev(W64, F16, dev), _dev(pc64, F32, dev)
    outs = {}
    for C in (32, 33):
        o32, o16 = _nan((B * C * Tp, 256), F32, dev), _nan((B * C * Tp, 256), F16, dev)
        assert _rc(L, "eend_convert_fanout_f16", Ed, W, pc, o32, o16, B, Tp, C) == 0
        torch.cuda.synchronize()
        outs[C] = (o32.view(B, C, Tp, 256), o16.view(B, C, Tp, 256))
    want = ((E64 @ W64.t()).view(B, 1, Tp, 256) + pc64.view(1, 33, 1, 256))
    for k in (0, 1):
        assert torch.equal(outs[33][k][:, :32], outs[32][k]) and E.same(outs[33][k].cpu(), want)


# ------------------------------------------------------------------------------------------------ the three f32 step entries
@pytest.mark.parametrize("c", _cases({"linear_step_f32"}), ids=E.case_id)
def test_linear_step_f32(hip_lib, dev, c):
    _run_plain(hip_lib, dev, c)


@pytest.mark.parametrize("c", _cases({"linear_res_ln_step_f32", "linear_res_scale_ln_step_f32"}), ids=E.case_id)
def test_residual_step_f32(hip_lib, dev, c):
    _run_res(hip_lib, dev, c)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("entry", sorted(E.ROUTES_OF_ENTRY))
def test_refusals(hip_lib, dev, entry):
    """every refusal the entry's routing code states: the query says refused, the entry returns EEND_EINVAL, no output is touched.
    The buffers are far larger than any of the refused shapes; a pointer the case wants NULL is NULL, one it wants misaligned is
    misaligned."""
    L = hip_lib
    from fs_eend_amd import lib as lib_
    mine = [(f, why) for e, f, why in E.REFUSALS if e == entry]
    assert mine
    step = entry.endswith("_step_f32")
    big = 1 << 16
    for f, why in mine:
        assert lib_.linear_route(entry, **f) == "refused", why
        src = torch.ones(big + 4, dtype=F32 if step else F16, device=dev)
        vec = torch.ones(big + 4, dtype=F32, device=dev)
        o32, o16 = _nan((big + 4,), F32, dev), _nan((big + 4,), F16, dev)

        def ptr(t, field):                               # NULL / misaligned / aligned as the case asks
            bits = f.get(field, 0)
            return None if bits < 0 else t.data_ptr() + bits
        g = lambda k, d=0: f.get(k, d)
        A, W, bias, res = ptr(src, "a"), ptr(src, "w"), ptr(vec, "bias"), ptr(src if entry == "linear_res16_ln_f16" else vec, "res")
        gamma, beta, p32, p16 = ptr(vec, "gamma"), ptr(vec, "beta"), ptr(o32, "out_f32"), ptr(o16, "out_f16")
        if entry == "linear_f16":
            args = (A, g("lda"), W, g("ldw"), bias, p16, g("ldo"), g("M"), g("N"), g("K"), g("act"))
        elif entry == "linear_glu_f16":
            args = (A, g("lda"), W, g("ldw"), bias, p16, g("ldo"), g("M"), g("N"), g("K"))
        elif entry == "inproj_heads_bf16":
            args = (A, g("lda"), W, g("ldw"), bias, p16, p16, p16, g("nseq"), g("Tp"), g("H"), g("dh"), g("K"))
        elif entry == "retention_proj_f16":
            args = (A, g("lda"), W, g("ldw"), bias, p16, p16, p16, p16, p16, g("nseq"), g("Tp"), g("H"), g("dh"), g("K"))
        elif entry == "linear_res_scale_f16":
            args = (A, g("lda"), W, g("ldw"), bias, res, 1.0, p32, p16, g("M"), g("K"))
        elif entry == "convert_fanout_f16":
            args = (A, W, res, p32, p16, g("nseq"), g("Tp"), g("C"))
        elif entry == "linear_step_f32":
            args = (A, g("lda"), W, g("ldw"), bias, p32, g("ldo"), g("M"), g("N"), g("K"), g("act"))
        elif entry == "linear_res_scale_ln_step_f32":
            args = (A, g("lda"), W, g("ldw"), bias, res, 1.0, gamma, beta, 1e-5, p32, None, p16, g("M"), g("K"))
        else:
            args = (A, g("lda"), W, g("ldw"), bias, res, 1.0, gamma, beta, 1e-5, p32, p16, g("M"), g("K"))
        rc = getattr(L, "eend_" + entry)(*args, torch.cuda.current_stream().cuda_stream)
        print(f"{entry}: {why}: {f} -> {rc}")
        assert rc == EINVAL, why
        torch.cuda.synchronize()
        assert o32.isnan().all() and o16.isnan().all(), why
