"""CPU: the float64 restatement of the differentiable attractor path (tests/eda_train_ref.py) against torch's float64 autograd and
against the golden vectors the reference itself produced (tools/gen_golden_eda_train.py), and the host rules of
fs_eend_amd.eda_model's two `forward` methods.

Bars.  Against torch float64 autograd (nn.LSTM(...).double(), Linear, bmm on CPU): 1e-10 relative to the largest magnitude of the
compared tensor -- both sides are float64, only the order of the sums differs.  Against a golden: FACTOR = 4 times the reference's own
fp32-vs-float64 gap stored with it, as in test_eda_ref.py (the golden is the reference's fp32 result, the restatement is float64).
"""
import numpy as np
import pytest
import torch

from oracle import fixtures as FX
from tests import eda_train_ref as TR

FACTOR = 4.0
H = 256
CASES = FX.list_cases("edatrain_")


def _modules(seed):
    torch.manual_seed(seed)
    enc = torch.nn.LSTM(H, H, 1, batch_first=True).double()
    dec = torch.nn.LSTM(H, H, 1, batch_first=True).double()
    cnt = torch.nn.Linear(H, 1).double()
    with torch.no_grad():
        for p in list(enc.parameters()) + list(dec.parameters()):
            p.mul_(1.5)
        cnt.weight.mul_(16.0)
    return enc, dec, cnt


def _named(enc, dec, cnt, grad=False):
    pick = (lambda p: p.grad) if grad else (lambda p: p)
    out = {f"encoder.{k}": pick(p) for k, p in enc.named_parameters()}
    out.update({f"decoder.{k}": pick(p) for k, p in dec.named_parameters()})
    out.update({f"counter.{k}": pick(p) for k, p in cnt.named_parameters()})
    return out


def _close(got, want, what, tol=1e-10):
    want = np.asarray(want.detach().numpy() if isinstance(want, torch.Tensor) else want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max()) / scale
    assert err <= tol, f"{what}: {err:.2e}"


@pytest.mark.parametrize("B,T,n_speakers", [(1, 1, [0]), (1, 2, [0]), (3, 7, [2, 0, 3])])
@pytest.mark.parametrize("permuted", [False, True])
def test_restatement_vs_float64_autograd(B, T, n_speakers, permuted):
    enc, dec, cnt = _modules(7 + T)
    g = torch.Generator().manual_seed(50 + B + T)
    xs = torch.randn(B, T, H, generator=g, dtype=torch.float64).requires_grad_(True)
    C = max(n_speakers) + 1
    Ra = 0.01 * torch.randn(B, C, H, generator=g, dtype=torch.float64)
    order = np.random.RandomState(T).permutation(T) if permuted else None
    xo = xs if order is None else xs[:, torch.as_tensor(order)]
    # the reference's forward, line by line (model :118-123)
    _, (hn, cn) = enc(xo)
    attractors, _ = dec(torch.zeros(B, C, H, dtype=torch.float64), (hn, cn))
    labels = torch.cat([torch.tensor([[1.0] * n + [0.0]], dtype=torch.float64) for n in n_speakers], dim=1)
    logit = torch.cat([cnt(att[:n + 1, :]).reshape(-1, n + 1) for att, n in zip(attractors, n_speakers)], dim=1)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, labels)
    dloss = 0.7
    (dloss * loss + (attractors * Ra).sum()).backward()
    r = TR.attractor_path(_named(enc, dec, cnt), xs, n_speakers, order, dloss=dloss, dattractors=Ra)
    _close(r["loss"], loss, "loss")
    _close(r["attractors"], attractors, "attractors")
    _close(r["dxs"], xs.grad, "dxs")
    grads = _named(enc, dec, cnt, grad=True)
    assert set(grads) == set(TR.EDA_PARAMS) == set(r["grads"])
    for k in TR.EDA_PARAMS:
        _close(r["grads"][k], grads[k], k)
    assert not grads["decoder.weight_ih_l0"].any()                 # torch returns zeros for the zero input, and so do we


@pytest.mark.parametrize("B,T,C", [(1, 1, 1), (3, 7, 4)])
def test_head_backward_vs_float64_autograd(B, T, C):
    g = torch.Generator().manual_seed(B + T)
    emb = torch.randn(B, T, H, generator=g, dtype=torch.float64).requires_grad_(True)
    att = torch.randn(B, C, H, generator=g, dtype=torch.float64).requires_grad_(True)
    R = torch.randn(B, T, C, generator=g, dtype=torch.float64)
    (torch.bmm(emb, att.transpose(1, 2)) * R).sum().backward()
    da, de = TR.head_backward(R, emb, att)
    _close(da, att.grad, "d attractors")
    _close(de, emb.grad, "d emb")


def test_lstm_backward_with_initial_state_and_final_state_gradients():
    """The encoder form of the recurrence alone: h0 / c0 given, upstream dhT / dcT and dh_all together."""
    enc, _, _ = _modules(3)
    B, T = 2, 5
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, T, H, generator=g, dtype=torch.float64)
    h0 = torch.randn(B, H, generator=g, dtype=torch.float64).requires_grad_(True)
    c0 = torch.randn(B, H, generator=g, dtype=torch.float64).requires_grad_(True)
    R1, R2, R3 = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((B, T, H), (B, H), (B, H)))
    y, (hn, cn) = enc(x, (h0[None], c0[None]))
    ((y * R1).sum() + (hn[0] * R2).sum() + (cn[0] * R3).sum()).backward()
    p = {k: v.detach().numpy() for k, v in enc.named_parameters()}
    G = x.numpy() @ p["weight_ih_l0"].T + p["bias_ih_l0"] + p["bias_hh_l0"]
    fwd = TR.lstm_forward(p["weight_hh_l0"], G, None, h0, c0)
    _close(fwd["h_all"], y, "h_all")
    dG, dh0, dc0 = TR.lstm_backward(p["weight_hh_l0"], fwd, None, dh_all=R1, dhT=R2, dcT=R3)
    _close(dh0, h0.grad, "dh0")
    _close(dc0, c0.grad, "dc0")
    _close(np.einsum("btn,btk->nk", dG, fwd["h_prev"]), enc.weight_hh_l0.grad, "dW_hh")
    _close(dG.sum((0, 1)), enc.bias_hh_l0.grad, "db")


def test_the_two_goldens_exist():
    assert CASES == ["edatrain_B3", "edatrain_T37"]
    assert FX.list_cases("eda_") == ["eda_T37", "eda_T700", "eda_ragged"]      # the inference goldens keep their prefix to themselves


@pytest.mark.parametrize("name", CASES)
def test_restatement_vs_golden(name):
    meta, arr = FX.load_case(name)
    assert meta["kind"] == "eda_train"
    eda = TR.build_mirror(meta)
    xs, Ra, order = TR.golden_inputs(meta)
    if order is not None:
        assert np.array_equal(order, arr["order"])
    r = TR.attractor_path(dict(eda.named_parameters()), xs, meta["n_speakers"], order, dattractors=Ra)
    assert r["attractors"].shape == arr["attractors"].shape == (meta["B"], max(meta["n_speakers"]) + 1, H)
    for key, got in (("loss", np.asarray([r["loss"]])), ("attractors", r["attractors"]), ("dxs", r["dxs"])):
        want = arr[key].astype(np.float64)
        err, bar = float(np.abs(got - want).max() / np.sqrt((want ** 2).mean())), FACTOR * meta["gaps"][key]["rel"]
        print(f"{name} {key}: err {err:.2e} bar {bar:.2e}")
        assert err <= bar, f"{name} {key}: {err:.2e} > {bar:.2e}"
    for k in TR.EDA_PARAMS:
        want = meta["grad_norms"][k]
        got = float(np.sqrt((r["grads"][k] ** 2).sum()))
        if want == 0.0:
            assert got == 0.0, k
            continue
        err, bar = abs(got - want) / want, FACTOR * meta["grad_norm_gaps"][k]
        print(f"{name} |d {k}|: err {err:.2e} bar {bar:.2e}")
        assert err <= bar, f"{name} |d {k}|: {err:.2e} > {bar:.2e}"


def _model():
    from fs_eend_amd.eda_model import TransformerEDADiarization
    torch.manual_seed(0)
    return TransformerEDADiarization(n_speakers=None, in_size=345, n_units=256, n_heads=4, n_layers=1, dropout=0.1)


def test_forward_rule_default_model_still_raises_not_implemented():
    """Any enc.* parameter that requires grad: NotImplementedError before every other check (tgt = None, CPU tensors)."""
    m = _model()
    with pytest.raises(NotImplementedError, match="encoder backward"):
        m([torch.zeros(5, 345)], None, [5])
    m.enc.requires_grad_(False)
    m.enc.encoder.bias.requires_grad_(True)                        # one is enough
    with pytest.raises(NotImplementedError, match="frozen|freeze"):
        m([torch.zeros(5, 345)], None, [5])


def test_forward_rule_frozen_encoder_on_cpu_raises_eend_hip_error():
    from fs_eend_amd.lib import EendHipError
    m = _model()
    m.enc.requires_grad_(False)
    src, tgt = [torch.zeros(5, 345), torch.zeros(3, 345)], [torch.zeros(5, 2), torch.zeros(3, 1)]
    with pytest.raises(EendHipError):
        m(src, tgt, [5, 3])
    with pytest.raises(ValueError):
        m(src, tgt[:1], [5, 3])
    with pytest.raises(ValueError):
        m(src, [torch.zeros(5, 16), torch.zeros(3, 1)], [5, 3])     # more speakers than the 15 the counter is built for


def test_eda_forward_host_rules():
    from fs_eend_amd.lib import EendHipError
    eda = _model().eda
    xs = torch.zeros(2, 4, 256)
    for bad in ([0, 1, 2], [0, 0, 1, 2], [0, 1, 2, 4], [0.0, 1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            eda(xs, [1, 2], order=bad)
    for bad in ([1], [1, 2, 3], [1, -1], [1, 16], [1.5, 2]):
        with pytest.raises(ValueError):
            eda(xs, bad)
    with pytest.raises(EendHipError):
        eda(xs, [1, 2])                                           # CPU tensor: no fallback
    with pytest.raises(EendHipError):
        eda(xs, [1, 2], order=[3, 2, 1, 0])
    with pytest.raises(EendHipError):
        eda(torch.zeros(4, 256), [1])
