"""attnout_spk_ffn_stream (dec_stream.hip): the whole FS decoder layer behind the time-axis attention in one launch, against the two
launches it replaces (attnout_spk_stream + attnout_ffn_stream) and against a torch fp32 restatement with the same f16 rounding points."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

ops = importlib.import_module("fs-eend_amd.ops")
_lib = importlib.import_module("fs-eend_amd.lib")
F16, F32 = torch.float16, torch.float32


def _weights(Fh, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to("cuda")
    W = dict(wo1=r(256, 256, sc=1 / 16).half(), win=r(768, 256, sc=1 / 8).half(), wo2=r(256, 256, sc=0.06).half(),
             w1=r(Fh, 256, sc=0.08).half(), w2=r(256, Fh, sc=0.04).half(),
             bo1=r(256, sc=0.1), g11=1 + r(256, sc=0.1), be11=r(256, sc=0.1), bin=r(768, sc=0.3),
             bo2=r(256, sc=0.2), g21=1 + r(256, sc=0.2), be21=r(256, sc=0.1), b1=r(Fh, sc=0.3), b2=r(256, sc=0.3),
             g22=1 + r(256, sc=0.2), be22=r(256, sc=0.1))
    W["wsd"] = ops.dec_stream_pack(W["wo1"], W["win"], W["wo2"], W["w1"], W["w2"])
    return W


def _rows(M, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(M, 256, generator=g)).to("cuda").half(), (torch.randn(M, 256, generator=g)).to("cuda").half()


def _fused(a, res, W, B, C, Tp):
    out = torch.full_like(res, float("nan"))
    ops.attnout_spk_ffn_stream(a, W["wsd"], W["bo1"], res, W["g11"], W["be11"], 1e-5, W["bin"], W["bo2"], W["g21"], W["be21"], 1e-5,
                               W["b1"], W["b2"], W["g22"], W["be22"], 1e-5, out, B, C, Tp)
    return out


def _pair(a, res, W, B, C, Tp):
    ws1 = ops.spk_stream_pack(W["wo1"], W["win"])
    ws = ops.ffn_stream_pack(W["wo2"], W["w1"], W["w2"])
    x1 = torch.empty_like(res); o = torch.empty_like(a); out = torch.full_like(res, float("nan"))
    ops.attnout_spk_stream(a, ws1, W["bo1"], res, W["g11"], W["be11"], 1e-5, x1, W["bin"], o, B, C, Tp)
    ops.attnout_ffn_stream(o, ws, W["bo2"], None, x1, W["g21"], W["be21"], 1e-5, W["b1"], W["b2"], W["g22"], W["be22"], 1e-5, None, out)
    return out


def _torch_ref(a, res, W, B, C, Tp):
    ln = torch.nn.functional.layer_norm
    x1 = ln(a.float() @ W["wo1"].float().T + W["bo1"] + res.float(), (256,), W["g11"], W["be11"], 1e-5).half().float()
    q, k, v = (x1 @ W["win"].float().T + W["bin"]).split(256, dim=1)
    sh = lambda t: t.view(B, C, Tp, 4, 64).permute(0, 2, 3, 1, 4)      # B, Tp, H, C, dh
    p = torch.softmax(sh(q) @ sh(k).transpose(-1, -2) * 0.125, dim=-1)
    o = (p @ sh(v)).permute(0, 3, 1, 2, 4).reshape(B * C * Tp, 256).half().float()
    x = ln(o @ W["wo2"].float().T + W["bo2"] + x1, (256,), W["g21"], W["be21"], 1e-5)
    h = (x.half().float() @ W["w1"].float().T + W["b1"]).relu().half().float()
    return ln(h @ W["w2"].float().T + W["b2"] + x, (256,), W["g22"], W["be22"], 1e-5)


@pytest.mark.parametrize("C,Tp,B,Fh", [(C, Tp, 2, 2048) if Tp * C <= 2048 else (C, Tp, 1, 512) for C in (3, 6) for Tp in (64, 128, 320, 512)]
                         + [(6, 512, 8, 2048)])           # the headline layer shape (F = 2048) at 8 utterances
def test_dec_stream_vs_pair_and_torch(C, Tp, B, Fh):
    assert ops.dec_stream_ok(C, Tp)
    W = _weights(Fh, 100 + C)
    a, res = _rows(B * C * Tp, 200 + Tp)
    got = _fused(a, res, W, B, C, Tp)
    pair = _pair(a, res, W, B, C, Tp)
    want = _torch_ref(a, res, W, B, C, Tp)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    d_pair = (got.float() - pair.float()).abs().max().item()
    d_ref = (got.float() - want).abs().max().item()
    d_pair_ref = (pair.float() - want).abs().max().item()
    assert d_pair < 8e-3, f"fused vs two launches: {d_pair:.3e}"
    assert d_ref < 6e-3, f"fused vs torch: {d_ref:.3e} (two launches vs torch: {d_pair_ref:.3e})"


@pytest.mark.parametrize("B,C,Tp", [(70, 6, 96), (90, 6, 128), (23, 3, 192), (300, 3, 64), (41, 6, 160)])
def test_dec_stream_part_filled_last_round(B, C, Tp):
    """row counts whose tiles leave the last round part-filled (and, 70 x 6 x 96, fewer tiles than CUs); in place as the model calls it"""
    W = _weights(2048, 7)
    a, res = _rows(B * C * Tp, 8)
    pair = _pair(a, res, W, B, C, Tp)
    want = _torch_ref(a, res, W, B, C, Tp)
    r2 = res.clone()
    ops.attnout_spk_ffn_stream(a, W["wsd"], W["bo1"], r2, W["g11"], W["be11"], 1e-5, W["bin"], W["bo2"], W["g21"], W["be21"], 1e-5,
                               W["b1"], W["b2"], W["g22"], W["be22"], 1e-5, r2, B, C, Tp)
    got = _fused(a, res, W, B, C, Tp)
    torch.cuda.synchronize()
    assert torch.equal(r2, got)
    assert (got.float() - pair.float()).abs().max().item() < 8e-3
    assert (got.float() - want).abs().max().item() < 6e-3


def test_dec_stream_rows_independent_of_tile_mates():
    """the same utterance at another batch position, among other utterances, gives bit-identical rows"""
    C, Tp = 6, 512
    W = _weights(2048, 9)
    n = C * Tp
    ua, ur = _rows(n, 10)
    outs = []
    for B, pos, seed in ((1, 0, 0), (3, 2, 11), (7, 4, 12)):
        a, res = _rows(B * n, seed) if B > 1 else (ua.clone(), ur.clone())
        a[pos * n:(pos + 1) * n] = ua; res[pos * n:(pos + 1) * n] = ur
        outs.append(_fused(a, res, W, B, C, Tp)[pos * n:(pos + 1) * n])
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("Fh", [64, 2048])
def test_dec_stream_pack_is_exact(Fh):
    """items 0..31 are spk_stream's stream, 32..39 Wo2 in O's register order, the rest ffn_stream's W1 / W2 items"""
    W = _weights(Fh, 13)
    ws = W["wsd"].view(-1, 16, 64, 8)                       # item, fragment, lane, element
    assert torch.equal(ws[:32].reshape(-1), ops.spk_stream_pack(W["wo1"], W["win"]))
    assert torch.equal(ws[40:].reshape(-1), ops.ffn_stream_pack(W["wo2"], W["w1"], W["w2"]).view(-1, 16, 64, 8)[8:].reshape(-1))
    i = torch.arange(16).view(16, 1, 1); l = torch.arange(64).view(1, 64, 1); e = torch.arange(8).view(1, 1, 8)
    f, g = l & 15, l >> 4
    n = (f >> 2) * 64 + i * 4 + (f & 3)
    wo2 = W["wo2"].cpu()
    for h in range(4):
        for u in range(2):
            want = wo2[n.expand(16, 64, 8), (h * 64 + g * 16 + u * 8 + e).expand(16, 64, 8)]
            assert torch.equal(ws[32 + h * 2 + u].cpu(), want)


def test_dec_stream_rejects_out_of_envelope_shapes():
    assert not ops.dec_stream_ok(13, 512) and not ops.dec_stream_ok(0, 512) and not ops.dec_stream_ok(6, 500)
    assert not ops.dec_stream_ok(3, 96) and ops.dec_stream_ok(6, 96) and ops.dec_stream_ok(3, 64)
    # slot counts whose instantiations would spill stay on the two launches
    assert not any(ops.dec_stream_ok(C, 512) for C in (1, 2, 4, 5, 7, 8, 9, 10, 11, 12))
    L = _lib.load()
    assert L.eend_dec_stream_elems(2112) == 0 and L.eend_dec_stream_elems(96) == 0 and L.eend_dec_stream_elems(32) == 0
    W = _weights(256, 14)
    with pytest.raises(_lib.EendHipError):
        ops.dec_stream_pack(W["wo1"], W["win"], W["wo2"], torch.zeros(96, 256, dtype=F16, device="cuda"),
                            torch.zeros(256, 96, dtype=F16, device="cuda"))
    for B, C, Tp in ((1, 6, 80), (1, 13, 64), (1, 2, 96), (1, 4, 64), (1, 12, 64)):
        a, res = _rows(B * C * Tp, 15)
        r2 = res.clone()
        with pytest.raises(_lib.EendHipError):               # in place, as the model calls it
            ops.attnout_spk_ffn_stream(a, W["wsd"], W["bo1"], r2, W["g11"], W["be11"], 1e-5, W["bin"], W["bo2"], W["g21"], W["be21"],
                                       1e-5, W["b1"], W["b2"], W["g22"], W["be22"], 1e-5, r2, B, C, Tp)
        torch.cuda.synchronize()
        assert torch.equal(r2, res)                          # nothing launched: the residual rows are untouched
