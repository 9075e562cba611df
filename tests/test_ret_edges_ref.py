"""CPU: the constructions of tests/ret_edge_ref.py really pin the retention kernels -- the float64 reference agrees with
oracle/ls_eend_ref.retention_chunk, the inputs are exact in both 16-bit formats and sit in the scale branch they claim, and every
one-step mutation of the reference moves the quantity tests/test_ret_edges.py asserts on past that test's bar by at least GAP = 4 x.
A kernel making one of these mistakes could therefore not pass there.

What cannot be detected is not claimed: all_scale = max(inner_raw, cross_raw, 1), and dropping ONE clamp alone leaves that maximum
unchanged, so the table mutates all_scale itself (each of its three effective arguments taken alone)."""
import pytest
import torch

from oracle import ls_eend_ref as O
from tests import ret_edge_ref as E

IMPULSE_SHAPES = [(4, 16), (6, 21), (64, 3), (64, 16), (100, 4), (500, 3), (512, 2), (544, 2)]


def test_reference_agrees_with_the_oracle():
    g = torch.Generator().manual_seed(5)
    for N, T, L, s in ((2, 192, 64, 1.0), (1, 60, 10, 0.05), (2, 300, 100, 4.0), (1, 1000, 500, 0.3)):
        q, k, v = (torch.randn(N, 4, T, 64, generator=g, dtype=torch.float64) * s for _ in range(3))
        want = O.retention_chunk(q, k, E.heads_to_rows(v), L).transpose(1, 2)               # (N, H, T, 64)
        c = E.ref_core(q, k, v, L)
        assert ((c.out - want).abs().max() / want.abs().max()).item() < 1e-12
        # the module: per-head LayerNorm and gate as oracle.msr applies them
        gate = torch.randn(N, 4, T, 64, generator=g, dtype=torch.float64)
        m = E.ref_module(q, k, v, gate, L)
        ln = O.layer_norm(want.transpose(1, 2), None, None, O.GN_EPS).transpose(1, 2)
        assert (m.rhat - ln).abs().max().item() < 1e-9
        assert (m.ctx - O.swish(gate) * ln).abs().max().item() < 1e-9


def test_carried_state_equals_one_call():
    q, k, v, g, _ = E.regime_qkv("mixed", 1, 256, 64)
    whole = E.ref_core(q, k, v, 64).out
    st = k[:, :, :128].transpose(-1, -2) @ v[:, :, :128]
    part = E.ref_core(q[:, :, 128:], k[:, :, 128:], v[:, :, 128:], 64, state_in=st).out
    assert (part - whole[:, :, 128:]).abs().max().item() < 1e-15


def test_closed_form_backward_equals_autograd():
    """o~ / d_g of gate_gn_bwd and dq / dk / dv of bwd_core == float64 autograd through the gate and the LayerNorm, scales detached"""
    for kind, L, nc in (("impulse", 64, 3), ("mixed", 64, 3), ("cross", 100, 2)):
        q, k, v, g, dctx = E.impulse_qkv(1, L * nc, L)[:5] if kind == "impulse" else E.regime_qkv(kind, 1, L * nc, L)
        r = E.ref_bwd(q, k, v, g, dctx, L, L * nc)
        m = E.ref_module(q, k, v, g, L)
        ot, dg = E.gate_gn_bwd(dctx, g, m.rhat, m.rc)
        dq, dk, dv = E.bwd_core(q, k, v, ot)
        for name, a, b in (("dg", dg, r["dg"]), ("dq", dq, r["dq"]), ("dk", dk, r["dk"]), ("dv", dv, r["dv"])):
            assert E.rel_worst(a, b) < 1e-9, (kind, name)


@pytest.mark.parametrize("L,nc", IMPULSE_SHAPES + [(300, 2), (10, 13), (1000, 2), (500, 1), (64, 1), (100, 2)])
def test_impulse_inputs_are_exact(L, nc):
    q, k, v, g, dctx, pr = E.impulse_qkv(2, L * nc, L)
    assert all(E.exact16(x) for x in (q, k, v, g, dctx))
    T = L * nc
    for f0 in range(0, T, L):
        assert f0 in pr and f0 + L - 1 in pr
    for e in range(16, T, 16):
        assert e in pr and e - 1 in pr
    assert (k.sum(-1)[0, 0, pr] == 1).all() and k.sum().item() == 2 * 4 * len(pr)
    # every sum the kernels form is a multiple of 0.5 under 2^11: exact in f16 products, f32 accumulators and hi / lo state pairs
    raw = (torch.tril(torch.ones(T, T, dtype=torch.float64)) * (q @ k.transpose(-1, -2))) @ v
    assert raw.abs().max().item() < 2048 and torch.equal(raw * 2, (raw * 2).round())
    st = torch.cumsum((k.transpose(-1, -2)[..., None] * v[:, :, None]).sum(0).sum(0), 1) if T <= 256 else None
    assert st is None or st.abs().max().item() < 2048
    # no row sits near the eps floor (eps moves a normalised value by < 1 %): these cases pin the masks and chunk edges, not the scales
    assert E.ref_core(q, k, v, L).out.var(-1, unbiased=False).min().item() > 1e-4


@pytest.mark.parametrize("regime,L,nc", E.REGIME_CASES)
def test_regime_inputs_sit_in_their_branch(regime, L, nc):
    q, k, v, g, dctx = E.regime_qkv(regime, 2, L * nc, L)
    assert all(E.exact16(x) for x in (q, k, v, g))
    c = E.ref_core(q, k, v, L)
    sh = E.branch_shares(c)
    fl, near = E.floor_share(c)
    print(regime, L, nc, sh, "at or under the floor", fl, "within 4 x of eps", near)
    if regime == "mixed":
        assert min(sh.values()) >= 0.1, sh
        inner = c.inner_raw.view(2, 4, nc, L)                       # rows pass 1 inside a chunk; the cross sum passes 1 between chunks
        assert (inner.amin(-1) < 1).all() and (inner.amax(-1) > 1).all()
        assert (c.cross_raw[:, :, 1] < 1).all() and (c.cross_raw[:, :, 2] > 1).all()
    else:
        assert sh[regime] >= 0.1, sh
    assert fl >= 0.1


def _imp_rows(L, nc, **kw):
    q, k, v, g, _, _ = E.impulse_qkv(1, L * nc, L)
    return E.ref_module(q, k, v, g, L, **kw)


def _imp_moved(good, bad):
    """how far the mutation moves what the impulse case asserts (ctx and rhat), in units of IMPULSE_BAR"""
    return max(E.impulse_err(bad.ctx, good.ctx), E.impulse_err(bad.rhat, good.rhat)) / E.IMPULSE_BAR


FWD_MUTATIONS = {
    "strict diagonal": lambda L: dict(mask=torch.tril(torch.ones(L, L, dtype=torch.bool), -1)),
    "chunk start + 1 (scores)": lambda L: dict(mask=torch.tril(torch.ones(L, L, dtype=torch.bool)) & (torch.arange(L)[None, :] >= 1)),
    "chunk start + 1 (state)": lambda L: dict(kv_range=(1, L)),
    "chunk end - 1 (state)": lambda L: dict(kv_range=(0, L - 1)),
    "prefix state includes its own chunk": lambda L: dict(prefix_shift=1),
    "prefix state lags one chunk": lambda L: dict(prefix_shift=-1),
}


@pytest.mark.parametrize("L,nc", IMPULSE_SHAPES)
@pytest.mark.parametrize("name", list(FWD_MUTATIONS))
def test_forward_mutations_fail_the_impulse_case(name, L, nc):
    good = _imp_rows(L, nc)
    moved = _imp_moved(good, _imp_rows(L, nc, **FWD_MUTATIONS[name](L)))
    bad_rc = _imp_rows(L, nc, **FWD_MUTATIONS[name](L)).rc
    rc = E.rel_rows(bad_rc, good.rc) / E.IMPULSE_RC
    print(f"{name} L={L} nc={nc}: moved {moved:.0f} x the bar; rc {rc:.0f} x its bar")
    assert rc >= E.GAP
    assert moved >= 10 * E.GAP                                       # stated gap of the impulse cases: 40 x the bar (0.08 absolute)


@pytest.mark.parametrize("L,nc", [(64, 3), (100, 4), (500, 3), (512, 2), (544, 2)])
def test_dropped_tile_fails_the_impulse_case(L, nc):
    """one interior 32-key tile lost for the rows behind it"""
    m = torch.tril(torch.ones(L, L, dtype=torch.bool))
    m[48:, 16:48] = False
    moved = _imp_moved(_imp_rows(L, nc), _imp_rows(L, nc, mask=m))
    assert moved >= 10 * E.GAP
    # ... and the random case under the project's bar
    q, k, v, g, _ = E.regime_qkv("inner", 1, L * nc, L)
    good, bad = E.ref_module(q, k, v, g, L), E.ref_module(q, k, v, g, L, mask=m)
    assert E.fwd_excess(bad.ctx, good.ctx)[1] >= E.GAP * E.FWD_CAP


TINY = 1e-12                                                         # keeps a mutated scale of a row without scores finite
_true = lambda a, c: torch.maximum(torch.maximum(a, c), torch.ones_like(a))
# name -> (all_scale_fn(inner_raw, cross_raw), regimes in which it is not the identity).  The raw state sum is zero before chunk 0
# (nothing to divide by), so that mutation keeps chunk 0 right and must be caught from chunk 1 on.
SCALE_MUTATIONS = {
    "all_scale = raw inner sum": (lambda a, c: a.clamp_min(TINY), ("clamped", "cross", "mixed")),
    "all_scale = raw state sum (from chunk 1 on)": (lambda a, c: torch.where(c > 0, c, _true(a, c)), ("clamped", "inner", "mixed")),
    "all_scale = 1": (lambda a, c: torch.ones_like(a), ("inner", "cross", "mixed")),
    "all_scale = max(state, 1): inner sum dropped": (lambda a, c: c.clamp_min(1), ("inner", "mixed")),
    "all_scale = max(inner, 1): state sum dropped": (lambda a, c: a.clamp_min(1), ("cross", "mixed")),
    "all_scale = max(inner, state): clamp at 1 dropped": (lambda a, c: torch.maximum(a, c).clamp_min(TINY), ("clamped", "mixed")),
}
TRAIN_L = (4, 64, 100, 500, 512)                                      # chunk lengths at which the GPU test asserts rc


def _scale_moved(good, bad):
    """the forward bar is passed when at most FWD_STRAY of the elements are over tolerance and none by more than FWD_CAP x: a mutation
    is caught when the share over tolerance is GAP x FWD_STRAY or the worst element GAP x FWD_CAP tolerances out; rc: GAP x RC_BAR"""
    assert all(bool(torch.isfinite(x).all()) for x in (bad.ctx, bad.rhat, bad.rc))
    share, worst = E.fwd_excess(bad.ctx, good.ctx)
    share_r, worst_r = E.fwd_excess(bad.rhat, good.rhat)
    return max(worst, worst_r) / E.FWD_CAP, max(share, share_r) / E.FWD_STRAY, E.rel_rows(bad.rc, good.rc) / E.RC_BAR


# every regime case the GPU tests assert (chunk entry: all; stream: L = 300 too); a regime whose all_scale IS the mutated expression is
# left out of that mutation's list: one chunk has no state to take a sum of, and the only clamped rows of `cross` (chunk 0, large V) are far
# above the eps floor, where no scale can be seen -- the dropped clamp is shown on `clamped` and `mixed`
@pytest.mark.parametrize("name,regime,L,nc", [(n, *c) for n in SCALE_MUTATIONS for c in E.REGIME_CASES if c[0] in SCALE_MUTATIONS[n][1] and not (n.startswith("all_scale = raw state sum") and c[2] == 1)])
def test_scale_mutations_fail_the_regime_cases(name, regime, L, nc):
    fn = SCALE_MUTATIONS[name][0]
    q, k, v, g, _ = E.regime_qkv(regime, 2, L * nc, L)
    good, bad = E.ref_module(q, k, v, g, L), E.ref_module(q, k, v, g, L, all_scale_fn=fn)
    worst, share, rc = _scale_moved(good, bad)
    print(f"{name} on {regime} L={L} nc={nc}: rows {worst:.1f} x cap, {share:.0f} x stray share; rc {rc:.0f} x bar")
    assert worst >= E.GAP or share >= E.GAP
    if L in TRAIN_L:
        assert rc >= E.GAP


@pytest.mark.parametrize("regime,L,nc", [c for c in E.REGIME_CASES if c[0] in ("cross", "mixed") and c[2] >= 3])
@pytest.mark.parametrize("shift", [1, -1])
def test_neighbour_chunk_scale_fails_the_regime_cases(shift, regime, L, nc):
    """the cross scale of chunk c taken from chunk c +- 1; the cross_scale workspace itself is compared at 1e-3"""
    q, k, v, g, _ = E.regime_qkv(regime, 2, L * nc, L)
    good, bad = E.ref_module(q, k, v, g, L), E.ref_module(q, k, v, g, L, cscale_shift=shift)
    worst, share, rc = _scale_moved(good, bad)
    cs = ((bad.core.cross_scale - good.core.cross_scale).abs() / good.core.cross_scale).max().item() / 1e-3
    print(f"cscale shift {shift} on {regime} L={L} nc={nc}: rows {worst:.1f} x cap, {share:.0f} x stray share; rc {rc:.0f} x bar; cscale {cs:.0f} x bar")
    assert (worst >= E.GAP or share >= E.GAP) and cs >= E.GAP and (rc >= E.GAP or L not in TRAIN_L)


@pytest.mark.parametrize("kind,L,nc", [("impulse", 64, 3), ("inner", 64, 3), ("inner", 500, 3), ("impulse", 100, 4), ("inner", 4, 16)])
def test_gate_layernorm_backward_mutations_fail(kind, L, nc):
    """the rhat term of the LayerNorm backward dropped; d_g with swish instead of swish' -- with the non-zero rhat of the module"""
    q, k, v, g, dctx = E.impulse_qkv(1, L * nc, L)[:5] if kind == "impulse" else E.regime_qkv("inner", 1, L * nc, L, floor=False)
    m = E.ref_module(q, k, v, g, L)
    rh = m.rhat.to(torch.float16).double()
    ot, dg = E.gate_gn_bwd(dctx, g, rh, m.rc)
    ot_bad, _ = E.gate_gn_bwd(dctx, g, rh, m.rc, drop_rhat_term=True)
    _, dg_bad = E.gate_gn_bwd(dctx, g, rh, m.rc, dg_swish=True)
    a, b = E.rel_worst(ot_bad, ot) / E.OT_BAR, E.rel_worst(dg_bad, dg) / E.DG_BAR
    print(f"{kind} L={L}: rhat term dropped moves o~ {a:.0f} x the bar; swish for swish' moves d_g {b:.0f} x the bar")
    assert a >= E.GAP and b >= E.GAP
    # ... and with rhat = 0 (the older test) both mutations are invisible
    z = torch.zeros_like(rh)
    assert torch.equal(E.gate_gn_bwd(dctx, g, z, m.rc, drop_rhat_term=True)[0], E.gate_gn_bwd(dctx, g, z, m.rc)[0])
    assert E.gate_gn_bwd(dctx, g, z, m.rc, dg_swish=True)[1].abs().max().item() == 0


BWD_MUTATIONS = {
    "strict diagonal": lambda T, L: dict(mask_q=E.causal(T, True), mask_kv=E.causal(T, True)),
    "suffix state R_c includes chunk c": lambda T, L: dict(mask_kv=E.chunk_shifted(T, L, 1)),
    "suffix state R_c misses chunk c + 1": lambda T, L: dict(mask_kv=E.chunk_shifted(T, L, -1)),
    "prefix state includes its own chunk": lambda T, L: dict(mask_q=E.chunk_shifted(T, L, 1)),
    "prefix state lags one chunk": lambda T, L: dict(mask_q=E.chunk_shifted(T, L, -1)),
}


@pytest.mark.parametrize("L,nc", [(4, 16), (6, 21), (10, 13), (64, 3), (100, 4), (500, 3), (512, 2), (544, 2)])
@pytest.mark.parametrize("name", list(BWD_MUTATIONS))
def test_backward_mutations_fail(name, L, nc):
    T = L * nc
    worst_imp = worst_rnd = 0.0
    for kind in ("impulse", "random"):
        q, k, v, g, dctx = E.impulse_qkv(1, T, L)[:5] if kind == "impulse" else E.regime_qkv("inner", 1, T, L, floor=False)
        m = E.ref_module(q, k, v, g, L)
        ot = E.gate_gn_bwd(dctx, g, m.rhat, m.rc)[0].to(torch.bfloat16).double()
        good, bounds = E.bwd_core(q, k, v, ot, bound=True)
        bad = E.bwd_core(q, k, v, ot, **BWD_MUTATIONS[name](T, L))
        for a, b, bd in zip(good, bad, bounds):
            if kind == "impulse":
                worst_imp = max(worst_imp, E.bound_err(b, a, bd) / E.IMPULSE_BWD)
            else:
                worst_rnd = max(worst_rnd, E.rel_l2(b, a) / E.BWD_L2, E.rel_worst(b, a) / E.BWD_WORST)
    print(f"{name} L={L} nc={nc}: impulse {worst_imp:.0f} x bar, random {worst_rnd:.0f} x bar")
    assert worst_imp >= E.GAP and worst_rnd >= E.GAP
