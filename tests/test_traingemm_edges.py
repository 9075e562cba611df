"""GPU: the data-gradient and training-forward GEMMs of the training step -- csrc/gemm.hip with bf16 operands (the 128 x 128 tile straight-line
and looped, the 64 x 256 whole-row tile with the residual, LayerNorm-backward and Conv1d row-mask epilogues), its training epilogues on f16
operands, csrc/ffn.hip MODE 3 / 4 (persistent, 128-row tiles) and csrc/proj.hip's head stores in both layouts -- against the exact reference
of tests/traingemm_edge_ref.py, at their row-tile, k-tile, stride, mask, dropout-index, sequence and workgroup-tile edges.

The operands are small integers (guards (a) and (b) of the reference module, asserted on the inputs), so everything linear is compared
with torch.equal up to the sign of zero; the ReLU-backward masks additionally leave the bit pattern +0.  Values behind rsqrt / exp use
E.TOL against float64; every figure is printed before it is asserted.  Every output is pre-filled with NaN and carries E.GUARD_ROWS extra
rows (and guard columns where ldo > N): NaN must sit exactly where the reference has it.  Launches go through fs_eend_amd.train._call;
the refusals read the raw return code."""
import ctypes

import pytest
import torch

from tests import traingemm_edge_ref as E

pytestmark = pytest.mark.gpu
F16, BF16, F32, I32 = torch.float16, torch.bfloat16, torch.float32, torch.int32
NAN = float("nan")
EINVAL = -1
G = E.GUARD_ROWS


@pytest.fixture(scope="module")
def T(hip_lib, dev):
    from fs_eend_amd import train
    return train


def _dev(t, dtype, dev, ld=None, guard=0):
    """float64 [R][C] (or a vector) -> device tensor of `dtype`, rows `ld` apart with non-zero fill between C and ld and `guard` NaN rows
    behind the last one; nothing rounds"""
    if t is None:
        return None
    if t.dim() == 2 and ld is not None and ld != t.shape[1]:
        buf = torch.full((t.shape[0], ld), float(E.PAD_FILL), dtype=torch.float64)
        buf[:, :t.shape[1]] = t
        t = buf
    r = t.to(dtype)
    assert torch.equal(r.double(), t) and torch.equal(torch.signbit(r), torch.signbit(t)), "operand not exact"
    if guard:
        r = torch.cat([r, torch.full((guard,) + tuple(r.shape[1:]), NAN, dtype=dtype)])
    return r.to(dev)


def _nan(shape, dtype, dev):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=dev)


def _drop(o, on, which="drop_seed"):
    """(eend_dropout at p = 0.5 kept alive by the caller, the pointer to pass) or (None, None)"""
    if not on:
        return None, None
    from fs_eend_amd import lib as L
    spec = L.Dropout(o[which], E.HALF, 2.0)
    return spec, ctypes.byref(spec)


def _check(c, got, want, aux):
    """every output buffer of the case against the reference: bitwise where exact, E.TOL elsewhere (figures printed first)"""
    assert set(got) == set(want), (set(got), set(want))
    torch.cuda.synchronize()
    exact = E.exact_outputs(c)
    for name, g in got.items():
        ok, err, bound = E.compare(c, name, g.cpu(), want[name], aux)
        if name in exact:
            print(f"{E.case_id(c)}: {name} exact: {ok}")
            assert ok, f"{E.case_id(c)}: {name} differs from the exact reference (max |diff| {err})"
        else:
            tol = E.tolerance(c, name)
            print(f"{E.case_id(c)}: {name} max |err| {err:.3e} (bound {bound:.3e}, {tol}, ratio {err / bound if bound else NAN:.3f}"
                  + (f", gap32 {E.pooled_gap(c['entry'], name, c.get('ncu', E.NCU_MI355X)):.3e} of the value, over the entry's table"
                     if name in E.ROW_SCALARS else f", gap32 {aux['gap'][name]:.3e}" if E.TOL[tol][0] == "gap" else "") + ")")
            assert ok, f"{E.case_id(c)}: {name} max |err| {err:.3e} > {bound:.3e} ({E.TOL[tol][3]}) or NaN misplaced"


def _stream_in_place(c, o, M, dev):
    """(res, out32): the f32 stream output NaN-filled with guard rows; aliased cases update the residual stream in place (out_f32 IS res)"""
    out32 = _nan((M + G, 256), F32, dev)
    res = _dev(o.get("res"), F32, dev)
    if c.get("alias"):
        out32[:M] = res
        res = out32
    return res, out32


# ------------------------------------------------------------------------------------------------ the runners, one per family
def _run_g128(T, dev, c):
    o, (want, aux) = E.operands(c), E.reference(c, with_aux=True)
    e, M, N, K = c["entry"], c["M"], c["N"], c["K"]
    dt = F16 if e == "linear_relu_train_f16" else BF16
    A, W = _dev(o["A"], dt, dev, c["lda"]), _dev(o["W"], dt, dev, c["ldw"])
    bias = _dev(o["bias"], F32, dev)
    out = _nan(want["out"].shape, dt, dev)
    if e == "gemm_bf16":
        T._call("eend_gemm_bf16", A, c["lda"], W, c["ldw"], bias, out, c["ldo"], M, N, K)
    elif e == "gemm_relu_bwd_bf16":
        act = _dev(o["act"], F16, dev, c["ldact"])
        T._call("eend_gemm_relu_bwd_bf16", A, c["lda"], W, c["ldw"], act, c["ldact"], out, c["ldo"], M, N, K, c["scale"])
        torch.cuda.synchronize()
        masked = (o["act"] == 0)
        bits = out[:M, :N].cpu().view(torch.int16)[masked]
        print(f"{E.case_id(c)}: {int(masked.sum())} masked elements, bit patterns {sorted(set(bits.tolist()))[:4]}")
        assert (bits == 0).all(), "a masked element is not +0"
    else:
        spec, dr = _drop(o, c["drop"])
        T._call("eend_linear_relu_train_f16", A, c["lda"], W, c["ldw"], bias, out, c["ldo"], M, N, K, dr)
    _check(c, {"out": out}, want, aux)


def _run_acc(T, dev, c):
    o, (want, aux) = E.operands(c), E.reference(c, with_aux=True)
    M, K = c["M"], c["K"]
    A, W = _dev(o["A"], BF16, dev, c["lda"]), _dev(o["W"], BF16, dev, c["ldw"])
    res, out32 = _stream_in_place(c, o, M, dev)
    out32 = out32 if c["out32"] else None
    out16 = _nan((M + G, 256), BF16, dev) if c["out16"] else None
    T._call("eend_gemm_acc_bf16", A, c["lda"], W, c["ldw"], res, c["alpha"], out32, out16, M, K)
    got = {}
    if out32 is not None:
        got["out32"] = out32
    if out16 is not None:
        got["out16"] = out16
    _check(c, got, want, aux)


def _run_lnbwd(T, dev, c):
    o, (want, aux) = E.operands(c), E.reference(c, with_aux=True)
    M, K = c["M"], c["K"]
    A, W = _dev(o["A"], BF16, dev, c["lda"]), _dev(o["W"], BF16, dev, c["ldw"])
    xhat, rstd, gamma = _dev(o["xhat"], F16, dev, guard=G), _dev(o["rstd"], F32, dev, guard=G), _dev(o["gamma"], F32, dev)
    nws = (M + 63) // 64 * 768                           # exactly what the entry asks for; NaN behind it must survive
    spec, dr = _drop(o, c["drop"])

    def call(with_dbias):
        g = _dev(o["g0"], F32, dev, guard=G)             # NaN behind row M of g, x_hat and rstd: a padded row in a column sum shows
        ds32 = g if c["alias"] else _nan((M + G, 256), F32, dev)
        ds16 = _nan((M + G, 256), BF16, dev)
        ws = _nan((nws + 64,), F32, dev)
        dg, db = _nan((256,), F32, dev), _nan((256,), F32, dev)
        dbias = _nan((256,), F32, dev) if with_dbias else None
        T._call("eend_gemm_acc_lnbwd_bf16", A, c["lda"], W, c["ldw"], g, xhat, rstd, gamma, ds32, ds16, ws, nws, dg, db, dbias, M, K, dr)
        torch.cuda.synchronize()
        assert ws[nws:].isnan().all(), "wrote behind ceil(M/64) * 768 workspace floats"
        got = {"ds32": ds32, "ds16": ds16, "dgamma": dg, "dbeta": db}
        if with_dbias:
            got["dbias"] = dbias
        return got
    got = call(bool(c["dbias"]))
    _check(c, got, want, aux)
    again = call(not c["dbias"])                        # the optional bias gradient changes nothing else, bit for bit
    for k in ("ds32", "ds16", "dgamma", "dbeta"):
        assert torch.equal(again[k].float().nan_to_num(7.0), got[k].float().nan_to_num(7.0)), f"{E.case_id(c)}: {k} depends on dbias"


def _run_dgrad(T, dev, c):
    o, (want, aux) = E.operands(c), E.reference(c, with_aux=True)
    dY, Wd = _dev(o["A"], BF16, dev), _dev(o["W"], BF16, dev)
    sl, ml = torch.tensor(c["lens"], dtype=I32, device=dev), torch.tensor(c["mlens"], dtype=I32, device=dev)
    out = _nan(want["out32"].shape, F32, dev)
    T._call("eend_conv1d_dgrad_bf16", dY, Wd, sl, ml, out, c["nseq"], c["Tp"], 256, c["ktaps"], c["pad"])
    _check(c, {"out32": out}, want, aux)


def _run_resln(T, dev, c):
    o, (want, aux) = E.operands(c), E.reference(c, with_aux=True)
    M, K = c["M"], c["K"]
    A, W = _dev(o["A"], F16, dev, c["lda"]), _dev(o["W"], F16, dev, c["ldw"])
    bias, gamma, beta = _dev(o["bias"], F32, dev), _dev(o["gamma"], F32, dev), _dev(o["beta"], F32, dev)
    res, out32 = _stream_in_place(c, o, M, dev)
    got = {"out32": out32, "out16": _nan((M + G, 256), F16, dev), "xhat": _nan((M + G, 256), F16, dev), "rstd": _nan((M + G,), F32, dev)}
    spec, dr = _drop(o, c["drop"])
    T._call("eend_" + c["entry"], A, c["lda"], W, c["ldw"], bias, res, c["alpha"], gamma, beta, E.EPS, out32, got["out16"], got["xhat"],
            got["rstd"], M, K, dr)
    _check(c, got, want, aux)


def _run_l2train(T, dev, c):
    o, (want, aux) = E.operands(c), E.reference(c, with_aux=True)
    M = c["nseq"] * c["Tp"]
    X, W, bias = _dev(o["A"], F16, dev), _dev(o["W"], F16, dev), _dev(o["bias"], F32, dev)
    il = torch.tensor(c["lens"], dtype=I32, device=dev)
    got = {"out32": _nan((M + G, 256), F32, dev), "out16": _nan((M + G, 256), F16, dev), "inv_norm": _nan((M + G,), F32, dev)}
    T._call("eend_conv1d_l2norm_train_f16", X, W, bias, il, got["out32"], got["out16"], got["inv_norm"], c["nseq"], c["Tp"], c["cin"],
            c["ktaps"], c["pad"])
    _check(c, got, want, aux)


def _run_heads(T, dev, c):
    o, (want, aux) = E.operands(c), E.reference(c, with_aux=True)
    A, W, bias = _dev(o["A"], F16, dev, c["lda"]), _dev(o["W"], F16, dev), _dev(o["bias"], F32, dev)
    tail = 512                                           # NaN elements behind every head buffer
    bufs = {k: _nan((v.numel() + tail,), BF16, dev) for k, v in want.items()}
    T._call("eend_inproj_heads_train_bf16", A, c["lda"], W, bias, bufs["Q"], bufs.get("Qt"), bufs["K"], bufs.get("Kt"), bufs["V"], bufs["Vt"],
            c["nseq"], c["Tp"], 4)
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b[-tail:].isnan().all(), f"{E.case_id(c)}: wrote behind {k}"
    _check(c, {k: b[:-tail] for k, b in bufs.items()}, want, aux)


def _run_ffn(T, dev, c):
    o = E.operands(c)
    e, M, F = c["entry"], c["M"], c["F"]
    X = _dev(o["A"], F16, dev, c["ldx"])
    W1, b1, W2, b2 = _dev(o["W"], F16, dev), _dev(o["bias"], F32, dev), _dev(o["W2"], F16, dev), _dev(o["b2"], F32, dev)
    gamma, beta = _dev(o["gamma"], F32, dev), _dev(o["beta"], F32, dev)
    res, out32 = _stream_in_place(c, o, M, dev)
    got = {"out32": out32, "out16": _nan((M + G, 256), F16, dev), "hid": _nan((M + G, F), F16, dev), "xhat": _nan((M + G, 256), F16, dev),
           "rstd": _nan((M + G,), F32, dev)}
    s1, d1 = _drop(o, c["drop"])
    s2, d2 = _drop(o, c["drop2"], "drop2_seed")
    head = (X, c["ldx"], W1, b1, W2, b2, res, c["alpha"], gamma, beta, E.EPS, out32, got["out16"])
    a16 = None
    if e == "ffn_train_f16":
        T._call("eend_ffn_train_f16", *head, got["hid"], got["xhat"], got["rstd"], M, F, d1, d2)
    else:
        got["z"] = _nan((M + G, F), F16, dev)
        T._call("eend_ffn_swish_train_f16", *head, got["z"], got["hid"], got["xhat"], got["rstd"], M, F, c["unnorm"], d1, d2)
        if not c["sat"]:                                 # the second product is checked on the f16 activation the kernel itself saved
            torch.cuda.synchronize()
            a16 = got["hid"].cpu().double()
            assert not a16[:M].isnan().any()
    want, aux = E.reference(c, a16=a16, with_aux=True)
    _check(c, got, want, aux)


def _run_ffnbwd(T, dev, c):
    o, (want, aux) = E.operands(c), E.reference(c, with_aux=True)
    M, F = c["M"], c["F"]
    dY, W2T, W1T = _dev(o["A"], BF16, dev, c["ldx"]), _dev(o["W"], BF16, dev), _dev(o["W2"], BF16, dev)
    hid = _dev(o["act"], F16, dev)
    g = _dev(o["res"], F32, dev, guard=G)                # in place on the gradient stream
    dH = _nan((M + G, F), BF16, dev)
    T._call("eend_ffn_bwd_data_bf16", dY, c["ldx"], W2T, hid, W1T, c["scale"], dH, g, M, F)
    torch.cuda.synchronize()
    masked = (o["act"] == 0)
    bits = dH[:M].cpu().view(torch.int16)[masked]
    print(f"{E.case_id(c)}: {int(masked.sum())} masked elements, all +0: {bool((bits == 0).all())}")
    assert (bits == 0).all(), "a masked element is not +0"
    _check(c, {"dH": dH, "g": g}, want, aux)


def _ncu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ------------------------------------------------------------------------------------------------ one test per entry family
@pytest.mark.parametrize("c", E.cases_of("gemm_bf16"), ids=E.case_id)
def test_gemm_bf16(T, dev, c):
    _run_g128(T, dev, c)


@pytest.mark.parametrize("c", E.cases_of("gemm_relu_bwd_bf16"), ids=E.case_id)
def test_gemm_relu_bwd_bf16(T, dev, c):
    _run_g128(T, dev, c)


@pytest.mark.parametrize("c", E.cases_of("linear_relu_train_f16"), ids=E.case_id)
def test_linear_relu_train_f16(T, dev, c):
    _run_g128(T, dev, c)


@pytest.mark.parametrize("c", E.cases_of("gemm_acc_bf16"), ids=E.case_id)
def test_gemm_acc_bf16(T, dev, c):
    _run_acc(T, dev, c)


@pytest.mark.parametrize("c", E.cases_of("gemm_acc_lnbwd_bf16"), ids=E.case_id)
def test_gemm_acc_lnbwd_bf16(T, dev, c):
    _run_lnbwd(T, dev, c)


@pytest.mark.parametrize("c", E.cases_of("conv1d_dgrad_bf16"), ids=E.case_id)
def test_conv1d_dgrad_bf16(T, dev, c):
    _run_dgrad(T, dev, c)


@pytest.mark.parametrize("c", E.cases_of("linear_res_ln_train_f16", "linear_res_scale_ln_train_f16"), ids=E.case_id)
def test_linear_res_ln_train_entries(T, dev, c):
    _run_resln(T, dev, c)


@pytest.mark.parametrize("c", E.cases_of("conv1d_l2norm_train_f16"), ids=E.case_id)
def test_conv1d_l2norm_train_f16(T, dev, c):
    _run_l2train(T, dev, c)


@pytest.mark.parametrize("c", E.cases_of("inproj_heads_train_bf16"), ids=E.case_id)
def test_inproj_heads_train_bf16(T, dev, c):
    _run_heads(T, dev, c)


@pytest.mark.parametrize("c", E.cases_of("ffn_train_f16", "ffn_swish_train_f16"), ids=E.case_id)
def test_ffn_train_entries(T, dev, c):
    c = E.resolve(c, _ncu(dev))
    if c.get("persist"):
        print(f"{E.case_id(c)}: {c['ncu']} compute units -> M = {c['M']}: {(c['M'] + 127) // 128} tiles, the last of {c['M'] % 128} rows")
    _run_ffn(T, dev, c)


@pytest.mark.parametrize("c", E.cases_of("ffn_bwd_data_bf16"), ids=E.case_id)
def test_ffn_bwd_data_bf16(T, dev, c):
    c = E.resolve(c, _ncu(dev))
    if c.get("persist"):
        print(f"{E.case_id(c)}: {c['ncu']} compute units -> M = {c['M']}: {(c['M'] + 127) // 128} tiles, the last of {c['M'] % 128} rows")
    _run_ffnbwd(T, dev, c)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("entry", sorted(E.FAMILY))
def test_refusals(hip_lib, dev, entry):
    """every shape or pointer the entry must refuse: EEND_EINVAL, and no output is touched.  The buffers cover every refused shape, so a
    call that were accepted by mistake would still stay inside them."""
    L = hip_lib
    mine = [(f, why) for e, f, why in E.REFUSALS if e == entry]
    assert mine
    big = 1 << 20
    src, vec = torch.ones(big, dtype=F16, device=dev), torch.ones(big, dtype=F32, device=dev)
    il = torch.full((8,), 64, dtype=I32, device=dev)
    for f, why in mine:
        a = dict(dict(M=65 if entry == "gemm_acc_lnbwd_bf16" else 17, N=128, K=64, lda=64, ldw=64, ldo=128, ldact=128, nseq=1, Tp=64, ktaps=3, pad=1,
                      cin=64, F=64, H=4, out32=1, out16=1, ws_short=0, g_off=0), **f)
        if entry == "inproj_heads_train_bf16":
            a["lda"] = f.get("lda", 256)
        outs = {k: _nan((big,), dt, dev) for k, dt in (("o32", F32), ("o16", F16), ("o16b", F16), ("o16c", F16), ("r32", F32), ("dg", F32), ("db", F32), ("dbias", F32))}
        o32, o16, o16b, o16c, r32 = (outs[k] for k in ("o32", "o16", "o16b", "o16c", "r32"))
        M, N, K = a["M"], a["N"], a["K"]
        if entry == "gemm_bf16":
            args = (src, a["lda"], src, a["ldw"], vec, o16, a["ldo"], M, N, K)
        elif entry == "gemm_relu_bwd_bf16":
            args = (src, a["lda"], src, a["ldw"], src, a["ldact"], o16, a["ldo"], M, N, K, 2.0)
        elif entry == "linear_relu_train_f16":
            args = (src, a["lda"], src, a["ldw"], vec, o16, a["ldo"], M, N, K, None)
        elif entry == "gemm_acc_bf16":
            args = (src, a["lda"], src, a["ldw"], vec, 1.0, o32 if a["out32"] else None, o16 if a["out16"] else None, M, K)
        elif entry == "gemm_acc_lnbwd_bf16":
            args = (src, a["lda"], src, a["ldw"], vec, src, vec, vec, o32, o16, r32, (M + 63) // 64 * 768 - a["ws_short"], outs["dg"], outs["db"],
                    outs["dbias"], M, K, None)
        elif entry in ("linear_res_ln_train_f16", "linear_res_scale_ln_train_f16"):
            args = (src, a["lda"], src, a["ldw"], vec, vec, 1.0, vec, vec, 1e-5, o32, o16, o16b, r32, M, K, None)
        elif entry == "conv1d_dgrad_bf16":
            args = (src, src, il, il, o32, a["nseq"], a["Tp"], 256, a["ktaps"], a["pad"])
        elif entry == "conv1d_l2norm_train_f16":
            args = (src, src, vec, il, o32, o16, r32, a["nseq"], a["Tp"], a["cin"], a["ktaps"], a["pad"])
        elif entry == "inproj_heads_train_bf16":
            args = (src, a["lda"], src, vec, o16, None, o16b, None, o16c, None, a["nseq"], a["Tp"], a["H"])
        elif entry == "ffn_train_f16":
            args = (src, 256, src, vec, src, vec, vec, 1.0, vec, vec, 1e-5, o32, o16, o16b, o16c, r32, M, a["F"], None, None)
        elif entry == "ffn_swish_train_f16":
            z16 = outs.setdefault("z16", _nan((big,), F16, dev))
            args = (src, 256, src, vec, src, vec, vec, 1.0, vec, vec, 1e-5, o32, o16, z16, o16b, o16c, r32, M, a["F"], 0, None, None)
        else:
            assert entry == "ffn_bwd_data_bf16"
            args = (src, 256, src, src, src, 2.0, o16, o32.data_ptr() + a["g_off"], M, a["F"])
        raw = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in args]
        rc = getattr(L, "eend_" + entry)(*raw, torch.cuda.current_stream().cuda_stream)
        print(f"{entry}: {why}: {f} -> {rc}")
        assert rc == EINVAL, why
        torch.cuda.synchronize()
        for k, t in outs.items():
            assert t.isnan().all(), (why, k)
