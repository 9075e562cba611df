"""CPU: the constructions of tests/rowgrad_edge_ref.py really pin the row and channel kernels of the training step -- the exact
references agree with torch autograd / float64 restatements, every case of the GPU tables passes the exactness guard (so that a correct
kernel is bit-exact whatever its summation order), and the one-step mistakes (a row dropped or counted twice -- the first row of a second
grid pass and the last row --, a frame at or beyond Tv admitted, taps shifted by one, a split boundary off by one) change the asserted
outputs at the shapes of tests/test_rowgrad_edges.py.  A kernel making one of these mistakes could therefore not pass there.

Where a shape gives a mistake nothing to act on (no second pass below 4097 rows, one split, no scalar tail) the mutation returns None;
the tests assert that this happens only where the shape explains it, and that every mutation acts on at least one shape."""
import pytest
import torch
import torch.nn.functional as Fn

from tests import rowgrad_edge_ref as E

D = E.D


# ---------------------------------------------------------------------------------------------------- grids
def test_grid_formulas():
    assert E.rows_grid(1) == (1, 4, 1) and E.rows_grid(5) == (2, 4, 1) and E.rows_grid(4096) == (1024, 4, 1)
    assert E.rows_grid(4097) == (1024, 4, 2) and E.rows_grid(12290) == (1024, 4, 4)
    assert E.rows_block_of(4096, 4097) == (0, 1) and E.rows_block_of(12289, 12290) == (0, 3) and E.rows_block_of(4095, 4096) == (1023, 0)
    assert E.slot_grid(64) == (16, 4, 1) and E.slot_grid(1024) == (256, 4, 1) and E.slot_grid(1088) == (256, 4, 2) and E.slot_grid(2112) == (256, 4, 3)
    assert E.bn_splits(2) == (1, 2) and E.bn_splits(256) == (1, 256) and E.bn_splits(257) == (2, 129) and E.bn_splits(131105) == (512, 257)
    assert E.bn16_blocks(1) == (1, 1) and E.bn16_blocks(32) == (1, 32) and E.bn16_blocks(33) == (2, 17) and E.bn16_blocks(131170) == (4096, 33)
    assert E.sumsq_grid(3) == (1, 0, 3) and E.sumsq_grid(1025) == (1, 1, 1) and E.sumsq_grid((1 << 20) + 3) == (1024, 1, 3)
    assert E.sumsq_grid((1 << 21) + 7) == (1024, 3, 3)
    from fs_eend_amd import ops
    assert all(ops.frames_pad(t) == E.frames_pad(t) for t in (1, 63, 64, 65, 129))


# ---------------------------------------------------------------------------------------------------- LayerNorm backward family
def test_ln_reference_equals_autograd():
    M = 37
    g, x, rstd, gamma = E.ln_operands(M, 1)
    # a LayerNorm whose x_hat and 1/sigma are the given ones: s = x / rstd has mean 0 and variance 2.5 / rstd^2, so rescale x_hat
    xh = x / 2.5 ** 0.5
    s = (xh / rstd[:, None]).clone().requires_grad_(True)
    gm = gamma.clone().requires_grad_(True)
    be = torch.zeros(D, dtype=torch.float64, requires_grad=True)
    y = Fn.layer_norm(s, (D,), gm, be, 0.0)
    gs, gg, gb = torch.autograd.grad(y, [s, gm, be], g)
    r = E.ref_ln(g, xh, rstd, gamma)
    assert (r["ds"] - gs).abs().max() < 1e-9 and (r["dgamma"] - gg).abs().max() < 1e-9 and torch.equal(r["dbeta"], gb)


@pytest.mark.parametrize("M", E.ROW_M)
def test_ln_operands_are_exact_and_mutations_show(M):
    g, x, rstd, gamma = E.ln_operands(M, 100 + M)
    d = g * gamma
    assert (d.sum(1) % 256 == 0).all() and ((d * x).sum(1) % 640 == 0).all()
    for t, dt in ((g, E.F32), (g, E.BF16), (x, E.F16), (rstd, E.F32), (gamma, E.F32)):
        E.as_t(t, dt)
    nb, rpb, passes = E.rows_grid(M)
    for alpha, thresh in ((1.0, 0), (0.5, 0), (0.5, E.HALF)):
        r = E.ref_ln(g, x, rstd, gamma, alpha, 5, thresh)
        assert (r["ds"] != 0).all()                                          # a zero of ds16 is a dropped element, nothing else
        E.as_t(r["ds"], E.F32), E.as_t(r["ds16"], E.BF16)
        E.assert_exact(g * x, g, r["ds16"], r["ds"] + 2, unit=0.125)
        if thresh:
            assert M < 64 or abs(float((r["ds16"] == 0).double().mean()) - 0.5) < 0.02
        for name in E.ROW_MUTATIONS:
            w = E.row_weights(name, M, nb * rpb)
            if w is None:
                assert passes == 1 and "second_pass" in name
                continue
            m = E.ref_ln(g, x, rstd, gamma, alpha, 5, thresh, w)
            for k in ("dgamma", "dbeta", "dbias"):
                assert not torch.equal(m[k], r[k]), (name, k)
        rr, mm = E.ref_resgrad(g, alpha, 5, thresh), None
        E.as_t(rr["ds16"], E.BF16)
        for name in E.ROW_MUTATIONS:
            w = E.row_weights(name, M, nb * rpb)
            if w is not None:
                assert not torch.equal(E.ref_resgrad(g, alpha, 5, thresh, w)["dbias"], rr["dbias"]), name


def test_row_mutations_act_somewhere():
    for name in E.ROW_MUTATIONS:
        assert sum(E.row_weights(name, M, 4 * E.rows_grid(M)[0]) is not None for M in E.ROW_M) >= 2, name
    assert {E.rows_grid(M)[2] for M in E.ROW_M} == {1, 2, 4}


# ---------------------------------------------------------------------------------------------------- convert fan-out backward
@pytest.mark.parametrize("B,Tp,C", E.SLOT_CASES)
def test_slot_sum_mutations_show(B, Tp, C):
    g0 = E.ints((B * C * Tp, D), 7 + B + C)
    E.assert_exact(g0.view(B, C, Tp, D).permute(0, 2, 1, 3).reshape(B * Tp, C * D))
    gsum, dpc = E.ref_slot_sum(g0, B, C, Tp)
    E.as_t(gsum, E.BF16)
    assert torch.equal(dpc.double(), g0.double().view(B, C, Tp, D).sum((0, 2)))
    nb, rpb, passes = E.slot_grid(B * Tp)
    assert passes == (1 if B * Tp <= 1024 else 2 if B * Tp <= 2048 else 3)
    for name in E.ROW_MUTATIONS:
        w = E.row_weights(name, B * Tp, nb * rpb)
        if w is None:
            assert passes == 1
            continue
        assert not torch.equal(E.ref_slot_sum(g0, B, C, Tp, w)[1], dpc), name
    if C > 1:                                                                # slots of one frame exchanged: gsum keeps, dpc shows
        perm = g0.view(B, C, Tp, D).clone()
        perm[0, 0, 0], perm[0, 1, 0] = g0.view(B, C, Tp, D)[0, 1, 0], g0.view(B, C, Tp, D)[0, 0, 0]
        assert not torch.equal(E.ref_slot_sum(perm.view(-1, D), B, C, Tp)[1], dpc)


# ---------------------------------------------------------------------------------------------------- FS BatchNorm
@pytest.mark.parametrize("c", E.BN_CASES + [E.BN_BIG], ids=E.bn_id)
def test_bn_cases_are_exact_and_mutations_show(c):
    F, T, lens = c["F"], c["T"], c["lens"]
    bufs = E.bn_buffers(c, 3)
    rows = E.bn_balance(bufs, lens, T, c["which"], -1, F)
    n = rows.shape[0]
    assert n == len(lens) * T and n >= 2 and all(1 <= l <= T for l in lens)
    s, mean, var, varu = E.ref_bn_stats(rows)
    assert (rows.sum(0) % n == 0).all() and torch.equal(mean, torch.round(mean))          # integer mean: both passes are exact
    E.assert_exact(rows, (rows - mean.to(E.I64)) ** 2)
    if n <= 4096:
        assert (var - rows.double().var(0, unbiased=False)).abs().max() < 1e-9 and (varu - rows.double().var(0, unbiased=True)).abs().max() < 1e-9
    dy = E.ints((n, F), 11)
    mu = E.ints((F,), 12, vals=(-1, 0, 1))
    dg, db = E.ref_bn_bwd(rows, dy, mu, 2)
    E.assert_exact(dy * (rows - mu) * 2, dy)
    ns, rps = E.bn_splits(n)
    for name in E.SPLIT_MUTATIONS:
        w = E.split_weights(name, n, ns, rps)
        if w is None:
            assert ns == 1
            continue
        ms = E.ref_bn_stats(rows, w)
        assert not torch.equal(ms[0], s) and not torch.equal(ms[2], var), name
        mg, mb = E.ref_bn_bwd(rows, dy, mu, 2, w)
        assert not torch.equal(mg, dg) and not torch.equal(mb, db), name
    for name in ("drop_last_row", "double_last_row"):
        w = E.row_weights(name, n, n)
        assert not torch.equal(E.ref_bn_stats(rows, w)[0], s) and not torch.equal(E.ref_bn_bwd(rows, dy, mu, 2, w)[1], db), name
    # a frame beyond an utterance's length taken from its buffer instead of the pad value
    if any(l < T for l in lens):
        full = E.bn_rows([T if l < T else l for l in lens], T, bufs, c["which"], -1, F)
        assert not torch.equal(E.ref_bn_stats(full)[0], s)


def test_bn_table_covers_what_it_claims():
    ns = {E.bn_splits(len(c["lens"]) * c["T"])[0] for c in E.BN_CASES + [E.BN_BIG]}
    assert ns == {1, 2, 512}
    assert {len(c["lens"]) * c["T"] for c in E.BN_CASES} >= {2, 255, 256, 257}
    assert {c["F"] for c in E.BN_CASES} == {345, 320, 256} and any(c["gap"] for c in E.BN_CASES)
    assert any(c["T"] == 1 for c in E.BN_CASES) and any(c["T"] == 7 for c in E.BN_CASES) and any(1 in c["lens"] and c["T"] > 1 for c in E.BN_CASES)
    n = len(E.BN_BIG["lens"]) * E.BN_BIG["T"]
    assert 512 * 256 < n < 512 * 257 and E.bn_splits(n)[1] % 16 != 0                     # the cap binds; boundaries inside a 16-row group


# ---------------------------------------------------------------------------------------------------- LS BatchNorm over valid frames
@pytest.mark.parametrize("nseq,Tp,Tv", E.BN16_CASES + [E.BN16_BIG])
def test_bn16_cases_are_exact_and_mutations_show(nseq, Tp, Tv):
    c = E.ints((nseq * Tp, D), nseq + Tv)
    ds = E.ints((nseq * Tp, D), nseq + Tv + 1)
    mu = E.ints((D,), 5, vals=(-1, 0, 1))
    n = nseq * Tv
    s, nn, mean, m2 = E.ref_bn16_stats(c, nseq, Tp, Tv)
    s1, s2 = E.ref_bn_swish_stats(ds, c, mu, 2, nseq, Tp, Tv)
    rows = E.valid_rows(nseq, Tp, Tv)
    E.assert_exact(c[rows], ds[rows], ds[rows] * (c[rows] - mu) * 2)
    assert nn == n and torch.equal(s.double(), c.double().view(nseq, Tp, D)[:, :Tv].sum((0, 1)))
    nb, rpb = E.bn16_blocks(n)
    for name in E.SPLIT_MUTATIONS + ("drop_last_row", "double_last_row"):
        w = E.split_weights(name, n, nb, rpb) if name in E.SPLIT_MUTATIONS else E.row_weights(name, n, n)
        if w is None:
            assert nb == 1
            continue
        assert not torch.equal(E.ref_bn16_stats(c, nseq, Tp, Tv, w)[0], s), name
        m1, m2_ = E.ref_bn_swish_stats(ds, c, mu, 2, nseq, Tp, Tv, w)
        assert not torch.equal(m1, s1) and not torch.equal(m2_, s2), name
    if Tv < Tp:                                                              # frame Tv admitted
        assert not torch.equal(E.ref_bn16_stats(c, nseq, Tp, Tv, extra=1)[0], s)
        assert not torch.equal(E.ref_bn_swish_stats(ds, c, mu, 2, nseq, Tp, Tv, extra=1)[0], s1)
    if n <= 4096:                                                            # the apply pass: zero at and beyond Tv, bf16-exact inside
        gam, a1, a2 = E.ints((D,), 6, vals=(-1, 1, 2)), E.ints((D,), 7), E.ints((D,), 8)
        out = E.ref_bn_swish_apply(ds, c, mu, 2, gam, a1, a2, nseq, Tp, Tv)
        E.as_t(out, E.BF16)
        assert (out.view(nseq, Tp, D)[:, Tv:] == 0).all() and (E.BETA - (c[rows] - mu).abs().max() * 2 * 2 >= 28)       # swish' == 1 in f32


def test_bn16_table_covers_what_it_claims():
    rows = {n * tv for n, _, tv in E.BN16_CASES}
    assert rows >= {1, 31, 32, 33} and (2, 128, 65) in E.BN16_CASES and any(tv == 1 and n > 1 for n, _, tv in E.BN16_CASES)
    n, Tp, Tv = E.BN16_BIG
    assert n * Tv > 4096 * 32 and E.bn16_blocks(n * Tv) == (4096, 33) and 4095 * 33 > n * Tv       # the cap binds and the last blocks are empty


# ---------------------------------------------------------------------------------------------------- conv module
@pytest.mark.parametrize("k", E.CONV_K)
def test_conv_reference_and_mutations(k):
    for Tv in E.conv_tv(k):
        for Tp in (E.frames_pad(Tv), E.frames_pad(Tv) + 64):
            nseq = 2
            val, w, dc = E.conv_operands(nseq, Tp, Tv, k, 10 * k + Tv)
            c = E.ref_conv_fwd(val, w, Tv)
            du, dw = E.ref_conv_bwd(val, w, dc, Tv)
            E.as_t(c, E.F16), E.as_t(du, E.BF16)
            E.assert_exact(dw.reshape(1, -1), (val[:, :Tv].abs().sum((0, 1))[None, :] * 2).reshape(1, -1))
            assert (c[:, Tv:] == 0).all() and (du[:, Tv:] == 0).all()
            # the impulse reads the taps back one by one
            for t in range(min(Tv, k)):
                assert torch.equal(c[-1, t], w[:, k - 1 - t])
            if Tp != E.frames_pad(Tv) or Tv not in (k, 65):
                continue
            # float64 autograd over the same operands (gate = +30: sigmoid == 1 to 1e-13)
            P = torch.cat([val[:, :Tv].double(), torch.full((nseq, Tv, D), E.GATE, dtype=torch.float64)], -1).requires_grad_(True)
            wd = w.double().requires_grad_(True)
            u = P[..., :D] * torch.sigmoid(P[..., D:])
            cc = Fn.conv1d(Fn.pad(u.transpose(1, 2), (k - 1, 0)), wd[:, None, :], groups=D).transpose(1, 2)
            assert (cc.detach() - c[:, :Tv].double()).abs().max() < 1e-9
            gP, gw = torch.autograd.grad(cc, [P, wd], dc[:, :Tv].double())
            assert (gP[..., :D] - du[:, :Tv].double()).abs().max() < 1e-9 and gP[..., D:].abs().max() < 1e-9 and (gw - dw.double()).abs().max() < 1e-9
            # one-step mistakes
            for shift in (-1, 1):
                assert not torch.equal(E.ref_conv_fwd(val, w, Tv, shift=shift), c)
                mdu, mdw = E.ref_conv_bwd(val, w, dc, Tv, shift=shift)
                assert not torch.equal(mdu, du) and not torch.equal(mdw, dw)
            if Tv < Tp:
                mdu, mdw = E.ref_conv_bwd(val, w, dc, Tv, tv_extra=1)
                assert not torch.equal(mdu, du) and not torch.equal(mdw, dw)


# ---------------------------------------------------------------------------------------------------- optimiser
@pytest.mark.parametrize("n", E.SUMSQ_N)
def test_sumsq_mutations_show(n):
    g = E.ints((n,), n % 1000)
    want = E.ref_sumsq(g)
    assert want < E.LIMIT and want == int((g.double() ** 2).sum())
    nb, passes, tail = E.sumsq_grid(n)
    for name in E.SUMSQ_MUTATIONS:
        w = E.sumsq_weights(name, n)
        if w is None:
            assert (name in ("drop_tail", "tail_in_every_block") and (tail == 0 or nb < 2)) or (name == "drop_last_float4" and n < 4) or \
                (name == "no_second_pass" and passes < 2), (name, n)
            continue
        assert E.ref_sumsq(g, w) != want, name


def test_sumsq_mutations_act_somewhere():
    for name in E.SUMSQ_MUTATIONS:
        assert any(E.sumsq_weights(name, n) is not None for n in E.SUMSQ_N), name


def test_adam_reference_equals_torch():
    n = 257
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1.0, betas=(0.9, 0.98), eps=1e-9)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in (1, 2, 3):
        gr = torch.randn(n, generator=g, dtype=torch.float64) * (2.0 if step == 1 else 0.01)
        ref.grad = gr.clone()
        torch.nn.utils.clip_grad_norm_([ref], 5.0)
        for q in opt.param_groups:
            q["lr"] = 1e-3 * step
        opt.step()
        p, m, v = E.ref_adam(p, gr, m, v, 1e-3 * step, step, 5.0, float((gr ** 2).sum()))
        assert (p - ref.detach()).abs().max() < 1e-12
