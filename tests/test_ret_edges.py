"""GPU: every retention entry of the chunk-recurrent form against the float64 reference of tests/ret_edge_ref.py on the SAME rounded
operands the kernel consumes, at the chunk, scale-clamp and padding edges: impulse keys (one probe admitted or lost is an O(0.1 .. 1)
error), the three scale regimes at the LayerNorm's eps floor (where the detached scales show in the output and in rc), poison in every
frame at or beyond T_valid and NaN-prefilled outputs.  tests/test_ret_edges_ref.py shows on the CPU that each one-step mutation of the
operator moves what is asserted here past the bar by the stated gap.  Every figure is printed before it is asserted.

eend_retention_bwd_bf16 serves the envelope of the training forward (L <= 512, L % 4 == 0) and nseq * nc <= 65535 with one launch per
chunk and refuses everything else: test_retention_bwd_rejects_what_the_forward_rejects."""
import pytest
import torch

from tests import ret_edge_ref as E

pytestmark = pytest.mark.gpu
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
NAN = float("nan")
EINVAL = -1


def _pad(x, Tp, T_valid, shift=0):
    """(N, H, T, 64) float64 -> (N, H, Tp, 64) with +-1000 in the frames at or beyond T_valid"""
    x = torch.nn.functional.pad(x, (0, 0, 0, Tp - x.shape[2]))
    return E.poison_tail(x, T_valid, shift)


def _rows(x):
    """(N, H, T, 64) -> (N * T, 256)"""
    return E.heads_to_rows(x).reshape(-1, 256).contiguous()


def _inputs(kind, nseq, L, nc, seed=0, floor=True):
    T = L * nc
    if kind == "impulse":
        return E.impulse_qkv(nseq, T, L)[:5]
    return E.regime_qkv(kind, nseq, T, L, seed, floor=floor)


def _fwd_ws(dev, nseq, Tp, L):
    nc = (Tp + L - 1) // L
    return (torch.empty(nseq * 4 * nc * 2 * 4096, dtype=F16, device=dev), torch.zeros(nseq * 4 * nc, dtype=F32, device=dev),
            torch.empty(nseq * 4 * nc, dtype=F32, device=dev))


def _check_rows(kind, got, want, what):
    """impulse: IMPULSE_BAR elementwise; regimes: the project's forward bar"""
    assert torch.isfinite(got).all(), what
    if kind == "impulse":
        e = E.impulse_err(got, want)
        print(f"{what}: impulse err {e:.3e} (bar {E.IMPULSE_BAR:.3e})")
        assert e <= E.IMPULSE_BAR, what
    else:
        share, worst = E.fwd_excess(got, want)
        print(f"{what}: share over tol {share:.2e} (<= {E.FWD_STRAY}), worst err / tol {worst:.2f} (<= {E.FWD_CAP})")
        assert share <= E.FWD_STRAY and worst <= E.FWD_CAP, what


def _fwd_cases():
    out = []
    for L, nc in E.FWD_SHAPES:
        out.append(("impulse", L, nc))
        out += [(r, l, n) for r, l, n in E.REGIME_CASES if (l, n) == (L, nc)]
    return out


@pytest.mark.parametrize("kind,L,nc", _fwd_cases())
def test_retention_chunk_edges(hip_lib, dev, kind, L, nc):
    """eend_retention_chunk_f16: normalised rows and the cross_scale workspace; T < Tp with poison behind T.  The chunk-resident kernel
    (L <= 512, L % 4 == 0) must leave the rows of the skipped chunks untouched (include/eend_hip.h)."""
    from fs_eend_amd import ops
    nseq, T = 2, L * nc
    Tp = ops.frames_pad(T + 1) + 64
    q, k, v, g, _ = _inputs(kind, nseq, L, nc)
    m = E.ref_module(q, k, v, g, L)
    qp, kp, vp, gp = (_pad(x, Tp, T, i) for i, x in enumerate((q, k, v, g)))
    q16, k16, v16 = (x.to(F16).to(dev).contiguous() for x in (qp, kp, vp))
    assert torch.equal(q16.double().cpu(), qp) and torch.equal(k16.double().cpu(), kp) and torch.equal(v16.double().cpu(), vp)
    kt, vt = k16.transpose(-1, -2).contiguous(), v16.transpose(-1, -2).contiguous()
    g16 = _rows(gp).to(F16).to(dev)
    st, cs, se = _fwd_ws(dev, nseq, Tp, L)
    o = torch.full((nseq * Tp, 256), NAN, dtype=F16, device=dev)
    ops.retention_chunk(q16.view(-1), k16.view(-1), kt.view(-1), vt.view(-1), g16, o, st, cs, se, nseq, 4, Tp, L, 1e-6, t_valid=T)
    torch.cuda.synchronize()
    got = o.view(nseq, Tp, 256).cpu()
    _check_rows(kind, got[:, :T], E.heads_to_rows(m.ctx), f"retention_chunk {kind} L={L} nc={nc}")
    full = L <= 512 and L % 4 == 0
    ncw = nc if full else (Tp + L - 1) // L                         # chunks the entry walks: the workspace's chunk stride
    cgot = cs[:nseq * 4 * ncw].view(nseq, 4, ncw)[:, :, :nc].double().cpu()
    cerr = ((cgot - m.core.cross_scale).abs() / m.core.cross_scale).max().item()
    print(f"   cross_scale rel err {cerr:.2e}")
    assert cerr <= 1e-3                                              # the bar of test_hip_kernels.py::test_retention_chunk
    if full:
        assert torch.isnan(got[:, T:]).all(), "rows of skipped chunks were written"


STREAM_SHAPES = ((64, 3), (300, 2), (500, 3), (512, 2))
STREAM_CASES = [(kind, L, nc, lo) for L, nc in STREAM_SHAPES for kind, lo in
                [("impulse", False), ("impulse", True)] + [(r, True) for r, l, n in E.REGIME_CASES if (l, n) == (L, nc)]]


@pytest.mark.parametrize("kind,L,nc,lo", STREAM_CASES)
def test_retention_stream_edges(hip_lib, dev, kind, L, nc, lo):
    """eend_retention_stream_f16 through 0 / 1 projection weights that reproduce the head rows exactly; without the lo rows, and with
    the query columns split x = hi + lo (ret_edge_ref.split_hi_lo: for the impulse queries lo carries q itself, so ignored, mis-strided
    or mis-scaled lo rows are an O(1) error); the last chunk again from a carried state_in"""
    from fs_eend_amd import ops
    assert ops.retention_stream_ok(L, 64 * 16)
    nseq, T = 2, L * nc
    Tp = ops.frames_pad(T + 1) + 64
    q, k, v, g, _ = (x[:, 0] for x in _inputs(kind, nseq, L, nc))              # one head's rows; the weights rotate them per head
    W, b = E.stream_w()
    qhi, qlo = E.split_hi_lo(q) if lo else (q, torch.zeros_like(q))
    assert not lo or float(qlo.abs().max()) > 0

    def slab(parts, poison):
        y = torch.nn.functional.pad(E.stream_x(*parts).view(nseq, T, 256), (0, 0, 0, Tp - T))
        if poison:
            y[:, T:] = E.poison_rows(Tp - T, 256)
        return y.reshape(-1, 256)
    x, xl = slab((qhi, k, v, g), True), slab((qlo, 0 * k, 0 * v, 0 * g), False)
    assert E.exact16(x) and E.exact16(xl)
    qh, kh, vh, gh = E.stream_heads(x, W, b, nseq, Tp)
    qh = qh + E.stream_heads(xl, W, b, nseq, Tp)[0]                            # the lo rows enter the query projection only
    m = E.ref_module(qh[:, :, :T], kh[:, :, :T], vh[:, :, :T], gh[:, :, :T], L)
    x16 = x.to(F16).to(dev)
    xlo = xl.to(F16).to(dev) if lo else None
    ws = ops.retention_stream_pack(W.to(F32).to(dev).contiguous())
    b32 = b.to(F32).to(dev)
    st, cs, se = _fwd_ws(dev, nseq, Tp, L)
    o = torch.full((nseq * Tp, 256), NAN, dtype=F16, device=dev)
    ops.retention_stream(x16, xlo, ws, b32, o, st, cs, se, nseq, Tp, L, 1e-6, t_valid=T)
    torch.cuda.synchronize()
    got = o.view(nseq, Tp, 256).cpu()
    want = E.heads_to_rows(m.ctx)
    _check_rows(kind, got[:, :T], want, f"retention_stream {kind} L={L} nc={nc} lo={lo}")
    cerr = ((cs[:nseq * 4 * nc].view(nseq, 4, nc).double().cpu() - m.core.cross_scale).abs() / m.core.cross_scale).max().item()
    print(f"   cross_scale rel err {cerr:.2e}")
    assert cerr <= 1e-3
    # carried state: the last chunk alone, from the float64 state of the chunks before it
    T0 = L * (nc - 1)
    Tp1 = ops.frames_pad(L)

    def tail(y, poison):
        y1 = torch.nn.functional.pad(y.view(nseq, Tp, 256)[:, T0:T], (0, 0, 0, Tp1 - L))
        if poison:
            y1[:, L:] = E.poison_rows(Tp1 - L, 256)
        return y1.reshape(-1, 256).to(F16).to(dev)
    state = (kh[:, :, :T0].transpose(-1, -2) @ vh[:, :, :T0]).to(F32).to(dev).contiguous()
    st1, cs1, se1 = _fwd_ws(dev, nseq, Tp1, L)
    o1 = torch.full((nseq * Tp1, 256), NAN, dtype=F16, device=dev)
    ops.retention_stream(tail(x, True), tail(xl, False) if lo else None, ws, b32, o1, st1, cs1, se1, nseq, Tp1, L, 1e-6, t_valid=L, state_in=state)
    torch.cuda.synchronize()
    _check_rows(kind, o1.view(nseq, Tp1, 256)[:, :L].cpu(), want[:, T0:], f"   carried state_in {kind} L={L}")


def test_retention_stream_envelope(hip_lib, dev):
    """eend_retention_stream_ok admits L <= 512 on 64-frame slabs with 8-element strides and rejects the rest"""
    from fs_eend_amd import ops
    for L in (1, 64, 300, 500, 512):
        assert ops.retention_stream_ok(L, 1024)
    for L, Tp, ldx, ldo in ((544, 1088, 256, 256), (1000, 1024, 256, 256), (0, 1024, 256, 256), (500, 1000, 256, 256), (500, 1024, 260, 256),
                            (500, 1024, 256, 260)):
        assert not ops.retention_stream_ok(L, Tp, ldx, ldo), (L, Tp, ldx, ldo)


def _train_fwd(dev, q, k, v, g, L, T, Tp):
    """runs eend_retention_chunk_train_f16 and the inference entry on the padded + poisoned operands"""
    from fs_eend_amd import ops
    from fs_eend_amd.train import _call
    nseq = q.shape[0]
    qp, kp, vp, gp = (_pad(x, Tp, T, i) for i, x in enumerate((q, k, v, g)))
    q16, k16, v16 = (x.to(F16).to(dev).contiguous() for x in (qp, kp, vp))
    kt, vt = k16.transpose(-1, -2).contiguous(), v16.transpose(-1, -2).contiguous()
    g16 = _rows(gp).to(F16).to(dev)
    st, cs, se = _fwd_ws(dev, nseq, Tp, L)
    kv = torch.empty(nseq * 4 * ((Tp + L - 1) // L) * 4096, dtype=F32, device=dev)
    M = nseq * Tp
    ctx = torch.full((M, 256), NAN, dtype=F16, device=dev)
    rhat = torch.full((M, 256), NAN, dtype=F16, device=dev)
    rc = torch.full((M, 4), NAN, dtype=F32, device=dev)
    _call("eend_retention_chunk_train_f16", q16, k16, kt, vt, g16, ctx, rhat, rc, st, kv, cs, se, nseq, 4, Tp, L, 256, 256, 1e-6, T)
    o = torch.full((M, 256), NAN, dtype=F16, device=dev)
    ops.retention_chunk(q16.view(-1), k16.view(-1), kt.view(-1), vt.view(-1), g16, o, st, cs, se, nseq, 4, Tp, L, 1e-6, t_valid=T)
    torch.cuda.synchronize()
    return ctx, rhat, rc, o


TRAIN_CASES = [(kind, L, nc) for kind, L, nc in _fwd_cases() if L in (4, 64, 100, 500, 512)]


@pytest.mark.parametrize("kind,L,nc", TRAIN_CASES)
def test_retention_train_forward_edges(hip_lib, dev, kind, L, nc):
    """eend_retention_chunk_train_f16 with T_valid = nc L and Tp >> T_valid: ctx bit-equal to the inference entry, rhat, and
    rc = rstd / (sqrt(i + 1) all_scale) per regime; the pad rows of ctx / rhat / rc untouched or zero."""
    nseq, T = 2, L * nc
    Tp = (T + 63) // 64 * 64 + 192
    q, k, v, g, _ = _inputs(kind, nseq, L, nc)
    m = E.ref_module(q, k, v, g, L)
    ctx, rhat, rc, o = _train_fwd(dev, q, k, v, g, L, T, Tp)
    c3, r3, o3 = (x.view(nseq, Tp, 256) for x in (ctx, rhat, o))
    assert torch.equal(c3[:, :T], o3[:, :T]), "ctx differs from the inference entry"
    what = f"retention_train {kind} L={L} nc={nc}"
    _check_rows(kind, c3[:, :T].cpu(), E.heads_to_rows(m.ctx), what + " ctx")
    _check_rows(kind, r3[:, :T].cpu(), E.heads_to_rows(m.rhat), what + " rhat")
    got_rc = rc.view(nseq, Tp, 4)[:, :T].double().cpu()
    want_rc = m.rc.transpose(1, 2)                                   # (nseq, T, H)
    assert torch.isfinite(got_rc).all()
    e = E.rel_rows(got_rc, want_rc)
    bar = E.IMPULSE_RC if kind == "impulse" else E.RC_BAR
    print(f"{what}: rc rel err {e:.3e} (bar {bar:.1e})")
    assert e <= bar, what
    for name, t in (("ctx", c3[:, T:]), ("rhat", r3[:, T:]), ("rc", rc.view(nseq, Tp, 4)[:, T:])):
        assert (torch.isnan(t) | (t == 0)).all(), f"{what}: pad rows of {name} written with non-zero values"


def _bwd_run(lib, dev, q, k, v, g, dctx, rhat, rc, L, T, Tp, transposed=True, ldq=1024):
    """eend_retention_bwd_bf16 on padded + poisoned operands; q, k, v, g, dctx, rhat (N, H, T, 64) float64, rc (N, H, T).
    Returns (return code, dqkvg (M, ldq) bf16, ot (M, 256) bf16, the rounded operands in float64 head layout)."""
    nseq = q.shape[0]
    M = nseq * Tp
    qp, kp, vp, gp, dp, rp = (_pad(x, Tp, T, i) for i, x in enumerate((q, k, v, g, dctx, rhat)))
    qb, kb, vb = (x.to(BF16).to(dev).contiguous() for x in (qp, kp, vp))
    tr = lambda x: x.transpose(-1, -2).contiguous() if transposed else None
    g16, rh16 = _rows(gp).to(F16).to(dev), _rows(rp).to(F16).to(dev)
    d32 = _rows(dp).to(F32).to(dev)
    rcp = torch.nn.functional.pad(rc.transpose(1, 2), (0, 0, 0, Tp - T), value=E.POISON).reshape(M, 4).to(F32).to(dev).contiguous()
    nc = T // L
    ot = torch.full((M * 256,), NAN, dtype=BF16, device=dev)
    ott = torch.full((M * 256,), NAN, dtype=BF16, device=dev) if transposed else None
    kv_ws = torch.empty(nseq * 4 * nc * 4096, dtype=F32, device=dev)
    g_ws = torch.empty(nseq * 4 * nc * 4096, dtype=F32, device=dev)
    st = torch.empty(nseq * 4 * nc * 6 * 4096, dtype=BF16, device=dev)
    out = torch.full((M, ldq), NAN, dtype=BF16, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    code = lib.eend_retention_bwd_bf16(p(qb), p(tr(qb)), p(kb), p(tr(kb)), p(vb), p(tr(vb)), p(d32), p(g16), 256, p(rh16), p(rcp),
                        p(ot), p(ott), p(kv_ws), p(g_ws), p(st), p(out), ldq, nseq, 4, Tp, L, T, 0.125, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ops64 = dict(q=qb.double().cpu()[:, :, :T], k=kb.double().cpu()[:, :, :T], v=vb.double().cpu()[:, :, :T],
                 g=E.rows_to_heads(g16.double().cpu().view(nseq, Tp, 256))[:, :, :T],
                 dctx=E.rows_to_heads(d32.double().cpu().view(nseq, Tp, 256))[:, :, :T],
                 rhat=E.rows_to_heads(rh16.double().cpu().view(nseq, Tp, 256))[:, :, :T],
                 rc=rcp.double().cpu().view(nseq, Tp, 4)[:, :T].transpose(1, 2))
    return code, out, ot.view(M, 256), ops64


def _bwd_check(kind, out, ot, o64, nseq, L, T, Tp, what):
    """stage 1 (o~, d_g with non-zero rhat), stage 2 (dq, sk dk, dv from the kernel's own o~), pad rows zero.  Returns the figures."""
    ot3 = ot.view(nseq, Tp, 256).double().cpu()
    o4 = out.view(nseq, Tp, -1)[:, :, :1024].double().cpu()
    assert torch.isfinite(ot3).all() and torch.isfinite(o4).all(), what
    if Tp > T:
        assert float(ot3[:, T:].abs().max()) == 0.0 and float(o4[:, T:].abs().max()) == 0.0, what + ": pad rows not zero"
    ot_want, dg_want = E.gate_gn_bwd(o64["dctx"], o64["g"], o64["rhat"], o64["rc"])
    ot_got = E.rows_to_heads(ot3[:, :T])
    parts = [E.rows_to_heads(o4[:, :T, i * 256:(i + 1) * 256]) for i in range(4)]
    e_ot, e_dg = E.rel_worst(ot_got, ot_want), E.rel_worst(parts[3], dg_want)
    print(f"{what}: o~ err / max {e_ot:.3e} (bar {E.OT_BAR:.1e}), d_g err / max {e_dg:.3e} (bar {E.DG_BAR:.1e})")
    assert e_ot <= E.OT_BAR and e_dg <= E.DG_BAR, what
    (dq, dk, dv), bounds = E.bwd_core(o64["q"], o64["k"], o64["v"], ot_got, bound=True)
    fig = {}
    for name, want, got, bd, sc in (("dq", dq, parts[0], bounds[0], 1.0), ("dk", dk, parts[1], bounds[1], 0.125), ("dv", dv, parts[2], bounds[2], 1.0)):
        if kind == "impulse":
            e = E.bound_err(got, sc * want, sc * bd)
            print(f"   {name}: err / sum|terms| {e:.3e} (bar {E.IMPULSE_BWD:.3e})")
            assert e <= E.IMPULSE_BWD, (what, name)
            fig[name] = e
        else:
            l2, worst = E.rel_l2(got, sc * want), E.rel_worst(got, sc * want)
            print(f"   {name}: rel L2 {l2:.2e} (bar {E.BWD_L2}), worst entry {worst:.2e} (bar {E.BWD_WORST})")
            assert l2 < E.BWD_L2 and worst < E.BWD_WORST, (what, name)
            fig[name] = (l2, worst)
    return fig


def _bwd_case(lib, dev, kind, L, nc, nseq=2, transposed=True, extra_pad=64):
    T = L * nc
    Tp = (T + 63) // 64 * 64 + extra_pad
    q, k, v, g, dctx = _inputs(kind, nseq, L, nc, floor=False)       # V of 2^-6 at every L: rhat of O(1) on most rows
    m = E.ref_module(q, k, v, g, L)                                  # non-zero rhat and the reference's own rc
    code, out, ot, o64 = _bwd_run(lib, dev, q, k, v, g, dctx, m.rhat, m.rc, L, T, Tp, transposed)
    assert code == 0
    return out, ot, o64, T, Tp


@pytest.mark.parametrize("kind", ["impulse", "inner"])
@pytest.mark.parametrize("L,nc", [(4, 16), (64, 3), (64, 16), (100, 4), (500, 1), (500, 3), (512, 2)])
def test_retention_bwd_fused_edges(hip_lib, dev, kind, L, nc):
    """eend_retention_bwd_bf16 (one launch per chunk, L <= 512, L % 4 == 0): both stages, every row class, on the impulse inputs
    and on the random inputs of the `inner` regime (q, k of O(1)); Qt / Kt / Vt / ott_ws = NULL gives the same bits"""
    out, ot, o64, T, Tp = _bwd_case(hip_lib, dev, kind, L, nc)
    _bwd_check(kind, out, ot, o64, 2, L, T, Tp, f"retention_bwd fused {kind} L={L} nc={nc}")
    out2, ot2, _, _, _ = _bwd_case(hip_lib, dev, kind, L, nc, transposed=False)
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16)) and torch.equal(ot2.view(torch.int16), ot.view(torch.int16))


@pytest.mark.parametrize("L,nc,nseq", [(6, 21, 2), (10, 13, 2), (516, 2, 2), (544, 2, 2), (1000, 2, 2), (4, 16, 4096)])
def test_retention_bwd_rejects_what_the_forward_rejects(hip_lib, dev, L, nc, nseq):
    """L > 512, L % 4 != 0 (refused by eend_retention_chunk_train_f16 as well) and nseq * nc > 65535: EEND_EINVAL before any launch, with
    or without the [d][t] copies -- the outputs keep their NaN prefill"""
    T = L * nc
    Tp = (T + 63) // 64 * 64
    s = torch.cuda.current_stream().cuda_stream
    small = torch.zeros(4096, dtype=F32, device=dev)                 # never read: the entry returns before its first launch
    out = torch.full((4096,), NAN, dtype=F32, device=dev)
    p = small.data_ptr()
    for tp in (p, None):
        code = hip_lib.eend_retention_bwd_bf16(p, tp, p, tp, p, tp, p, p, 256, p, p, out.data_ptr(), tp, p, p, p, out.data_ptr(), 1024, nseq, 4, Tp, L,
                                               T, 0.125, s)
        assert code == EINVAL, (L, nc, nseq, code)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and float(small.abs().max()) == 0.0


def test_retention_envelope(hip_lib, dev):
    """EEND_EINVAL for what the entries do not serve"""
    L, nc, nseq = 64, 2, 1
    T, Tp = 128, 192
    q, k, v, g, dctx = _inputs("inner", nseq, L, nc)
    m = E.ref_module(q, k, v, g, L)
    code, _, _, _ = _bwd_run(hip_lib, dev, q, k, v, g, dctx, m.rhat, m.rc, L, T, Tp)
    assert code == 0
    # backward: T_valid % L, ldq < 1024, ldq % 8, L % 4
    assert _bwd_run(hip_lib, dev, q, k, v, g, dctx, m.rhat, m.rc, 48, T, Tp)[0] == EINVAL                     # 128 % 48 != 0
    assert _bwd_run(hip_lib, dev, q, k, v, g, dctx, m.rhat, m.rc, L, T, Tp, ldq=768)[0] == EINVAL
    assert _bwd_run(hip_lib, dev, q, k, v, g, dctx, m.rhat, m.rc, L, T, Tp, ldq=1028)[0] == EINVAL
    q2, k2, v2, g2, d2 = _inputs("inner", nseq, 10, 12)
    m2 = E.ref_module(q2, k2, v2, g2, 10)
    assert _bwd_run(hip_lib, dev, q2, k2, v2, g2, d2, m2.rhat, m2.rc, 10, 120, 128, transposed=False)[0] == EINVAL
    assert _bwd_run(hip_lib, dev, q2, k2, v2, g2, d2, m2.rhat, m2.rc, 10, 120, 128, transposed=True)[0] == EINVAL
    # H != 4 on the backward, and the train forward's envelope (T_valid % L, L > 512, L % 4)
    lib = hip_lib
    s = torch.cuda.current_stream().cuda_stream
    Z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    p = lambda t: t.data_ptr()
    hb, g16, rh16, d32, rc32 = Z(Tp * 256, BF16), Z(Tp * 256, F16), Z(Tp * 256, F16), Z(Tp * 256, F32), Z(Tp * 4, F32)
    otw, ottw, kvw, gw, stw, dq = Z(Tp * 256, BF16), Z(Tp * 256, BF16), Z(8 * 4096, F32), Z(8 * 4096, F32), Z(8 * 6 * 4096, BF16), Z(Tp * 1024, BF16)
    bwd = lambda H, Lc, Tv, ldq: lib.eend_retention_bwd_bf16(p(hb), p(hb), p(hb), p(hb), p(hb), p(hb), p(d32), p(g16), 256, p(rh16), p(rc32), p(otw),
                                                             p(ottw), p(kvw), p(gw), p(stw), p(dq), ldq, 1, H, Tp, Lc, Tv, 0.125, s)
    assert bwd(4, 64, 128, 1024) == 0
    assert bwd(2, 64, 128, 1024) == EINVAL and bwd(8, 64, 128, 1024) == EINVAL
    assert bwd(4, 64, 100, 1024) == EINVAL and bwd(4, 64, 256, 1024) == EINVAL and bwd(4, 0, 128, 1024) == EINVAL
    h16, o16, r16, rcw, st16, csw, sew = Z(Tp * 256, F16), Z(Tp * 256, F16), Z(Tp * 256, F16), Z(Tp * 4, F32), Z(8 * 2 * 4096, F16), Z(8, F32), Z(8, F32)
    fwd = lambda Lc, Tv, Tpp: lib.eend_retention_chunk_train_f16(p(h16), p(h16), p(h16), p(h16), p(g16), p(o16), p(r16), p(rcw), p(st16), p(kvw), p(csw),
                                                                 p(sew), 1, 4, Tpp, Lc, 256, 256, 1e-6, Tv, s)
    assert fwd(64, 128, Tp) == 0
    assert fwd(64, 100, Tp) == EINVAL              # T_valid % L
    assert fwd(6, 126, Tp) == EINVAL and fwd(10, 120, Tp) == EINVAL                                   # L % 4
    assert fwd(544, 1088, 1088) == EINVAL and fwd(1000, 1000, 1024) == EINVAL                         # L > 512
    assert fwd(64, 256, Tp) == EINVAL and fwd(64, 0, Tp) == EINVAL                                    # T_valid > Tp, T_valid = 0
    torch.cuda.synchronize()
