"""CPU: the constructions of tests/attn_edge_ref.py really pin the attention mask -- the float64 reference reproduces the staircase
answers, and every one-key mutation of the reference's own mask (delay +- 1, kv_len +- 1, q_len + 1 in the backward, one interior
32-key tile dropped) moves some row past the bar by at least 0.25.  tests/test_attn_edges.py runs the same constructions through
the HIP kernels; these checks show that a kernel making one of these mistakes could not pass there."""
import pytest
import torch

from tests import attn_edge_ref as R

GAP = 0.25


def _stair_out(nseq, H, Tp, delay, kv_len, reverse=False, mask=None):
    Q, K, V = R.stair_qkv(nseq, H, Tp, kv_len, reverse=reverse)
    o, _ = R.ref_attn(Q, K, V, delay, kv_len, R.LN2, mask=mask)
    return o, V


@pytest.mark.parametrize("Tp,delay,kv_len", [(64, 0, 64), (128, 1, 100), (128, 31, 33), (256, 64, 129), (512, 511, 512), (576, 0, 1),
                                             (1024, 513, 1000), (4096, 0, 4096), (4096, 1 << 25, 4095)])
def test_staircase_reference_is_exact(Tp, delay, kv_len):
    """row i of the staircase is V[min(i + delay, kv_len - 1)], of the reverse staircase V[0], up to the 2^-32 weight of the runner-up
    key -- also over poison rows of 1e3"""
    o, V = _stair_out(1, 2, Tp, delay, kv_len)
    want = V[:, :, R.last_visible(Tp, delay, kv_len)]
    assert (o - want).abs().max().item() < 1e-6
    o, V = _stair_out(1, 2, Tp, delay, kv_len, reverse=True)
    assert (o - V[:, :, :1]).abs().max().item() < 1e-6
    # adjacent value rows are >= 0.5 apart and exact in both 16-bit formats
    v = V[0, :, :kv_len]
    assert v.abs().max() <= 8
    assert torch.equal(v.to(torch.float16).double(), v) and torch.equal(v.to(torch.bfloat16).double(), v)
    if kv_len > 1:
        assert (v[:, 1:] - v[:, :-1]).abs().amax(-1).min() >= 0.5
    if kv_len > 32:
        assert (v[:, 32:] - v[:, :-32]).abs().amax(-1).min() >= 0.5


def test_stair_inproj_matches_head_rows():
    """the fused in-projection construction (x, 0 / 1 weights) projects to exactly the head-row staircase, in f16"""
    for reverse in (False, True):
        x = R.stair_x(2, 1024, 700, reverse=reverse)
        W, b = R.stair_inproj(reverse=reverse)
        assert torch.equal(x.to(torch.float16).double(), x)
        q, k, v = R.inproj_heads(x.to(torch.float16), W.to(torch.float16), b, 2, 1024)
        Q, K, _ = R.stair_qkv(2, 4, 1024, 700, reverse=reverse)
        assert torch.equal(q, Q) and torch.equal(k[..., :700, :], K[..., :700, :])
        assert (k[..., 700:, :2] * (-1 if reverse else 1) == R.POISON).all()
        assert (v[..., :700, :].abs() <= 8).all() and (v[..., 700:, :].abs() == R.POISON).all()
        o, _ = R.ref_attn(q, k, v, 3, 700, R.LN2)
        want = v[:, :, :1] if reverse else v[:, :, R.last_visible(1024, 3, 700)]
        assert (o - want).abs().max().item() < 1e-6


@pytest.mark.parametrize("Tp,delay,kv_len", [(128, 0, 100), (512, 31, 480), (640, 64, 577), (1024, 511, 1024)])
def test_mask_mutations_fail_the_staircase(Tp, delay, kv_len):
    """delay +- 1 and kv_len +- 1 in the reference's mask: some row moves by >= 0.25 (kv_len + 1 reaches a poison row)"""
    good, _ = _stair_out(1, 2, Tp, delay, kv_len)
    for d, kv in ((delay + 1, kv_len), (delay - 1, kv_len), (delay, kv_len - 1), (delay, kv_len + 1)):
        if d < 0 or kv > Tp or kv < 1:
            continue
        bad, _ = _stair_out(1, 2, Tp, delay, kv_len, mask=R.visible(Tp, Tp, d, kv))
        assert (bad - good).abs().max().item() >= GAP, (d, kv)


@pytest.mark.parametrize("Tp,delay,kv_len,tile", [(128, 0, 128, 1), (512, 0, 500, 7), (512, 600, 300, 3), (1024, 5, 1000, 20)])
def test_dropped_tile_fails_the_row_metric(Tp, delay, kv_len, tile):
    """random inputs: a mask that loses one interior 32-key tile moves some row's per-row error past 0.25"""
    g = torch.Generator().manual_seed(Tp + tile)
    q, k, v = (torch.randn(1, 2, Tp, 64, generator=g, dtype=torch.float64) for _ in range(3))
    good, _ = R.ref_attn(q, k, v, delay, kv_len, 0.125)
    m = R.visible(Tp, Tp, delay, kv_len)
    m[:, tile * 32:(tile + 1) * 32] = False
    m[:, 0] |= R.visible(Tp, Tp, delay, kv_len)[:, 0]          # every row keeps a key
    bad, _ = R.ref_attn(q, k, v, delay, kv_len, 0.125, mask=m)
    assert R.row_err(bad, good).max().item() >= GAP


def test_backward_mutations_fail():
    """q_len + 1 lets a poison dO row in; delay + 1 moves a staircase row's dV to its neighbour key"""
    nseq, H, Tp, delay, kv_len, q_len = 1, 2, 128, 1, 120, 100
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(nseq, H, Tp, 64, generator=g, dtype=torch.float64) for _ in range(3))
    dO = torch.randn(nseq, H, Tp, 64, generator=g, dtype=torch.float64)
    dO[..., q_len:, :] = R.POISON
    good = R.ref_attn_bwd(q, k, v, dO, delay, kv_len, q_len, 0.125)
    bad = R.ref_attn_bwd(q, k, v, dO, delay, kv_len, q_len + 1, 0.125)
    assert all((a - b).abs().max().item() >= GAP for a, b in zip(good, bad))
    # padding rows: dQ beyond q_len and dK / dV beyond kv_len are exactly zero
    assert (good[0][..., q_len:, :] == 0).all() and (good[1][..., kv_len:, :] == 0).all() and (good[2][..., kv_len:, :] == 0).all()
    Q, K, V = R.stair_qkv(nseq, H, Tp, kv_len)
    dq, dk, dv = R.ref_attn_bwd(Q, K, V, dO, delay, kv_len, q_len, R.LN2)
    want = _stair_dv(dO, delay, kv_len, q_len)
    assert (dv - want).abs().max().item() < 1e-6
    assert (_stair_dv(dO, delay + 1, kv_len, q_len) - want).abs().max().item() >= GAP


def _stair_dv(dO, delay, kv_len, q_len, keep_scale=None):
    """closed form of the staircase's dV: dV_j = sum of dO_i (times its keep * scale) over the rows i < q_len whose last visible key is j"""
    Tp = dO.shape[-2]
    last = R.last_visible(Tp, delay, kv_len)
    dv = torch.zeros_like(dO, dtype=torch.float64)
    w = dO.double() if keep_scale is None else dO.double() * keep_scale
    dv.index_add_(-2, last[:q_len], w[..., :q_len, :])
    return dv


def test_dropout_keep_mask_matches_the_oracle_generator():
    """drop_keep is oracle/dropout_ref.HashDropout.attn's mask (the generator test_train_kernels.py checks the kernels against)"""
    from oracle import dropout_ref as DR
    nseq, H, Tp = 2, 4, 128
    seed, th, sc = R.drop_spec(0.2, Tp)
    d = DR.HashDropout(0.2, 42, 7, Tp)
    p = torch.ones(nseq, H, Tp, Tp, dtype=torch.float64)
    keep = R.drop_keep(seed, th, nseq, H, Tp)
    assert torch.equal(d.attn(p, 3), keep.double() * sc)
    assert 0.75 < keep.double().mean().item() < 0.85
    # the staircase under dropout: row i is scale * V[last] if (i, last) is kept, else ~0; flipping one row's bit is an O(1) error
    Q, K, V = R.stair_qkv(nseq, H, Tp, 100)
    o, _ = R.ref_attn(Q, K, V, 0, 100, R.LN2, keep, sc)
    last = R.last_visible(Tp, 0, 100)
    kb = keep[:, :, torch.arange(Tp), last]
    want = V[:, :, last] * (kb.double() * sc)[..., None]
    assert (o - want).abs().max().item() < 1e-6
