"""GPU: eend_lstm_f32 (csrc/lstm.hip) against the float64 LSTM of tests/eda_ref.py.

Bar: K x gap32 per compared tensor, where gap32 is torch's own CPU fp32 nn.LSTM against the float64 restatement on the same inputs,
computed here.  K = 8: the kernel keeps W_hh, h, c and every sum in f32 (the weights are re-read from L2 every step, nothing on the
path is 16-bit), so the order of the sums is the only difference from torch's fp32 LSTM.  The input pre-activations are computed on
the device by eend_linear_step_f32, as the model computes them.
"""
import numpy as np
import pytest
import torch

from tests import eda_ref as ER
from tests import lstm_cases as LC
from tests.lstm_cases import H

pytestmark = pytest.mark.gpu

K = 8.0
SHAPES = [(1, 1), (1, 2), (3, 65), (2, 130), (17, 5)]


@pytest.fixture(scope="module")
def net():
    """The seeded nn.LSTM (CPU fp32: the gap32 side) and its parameters in float64."""
    lstm = LC.seeded_lstm()
    return lstm, {k: v.detach().double().numpy() for k, v in lstm.named_parameters()}


def _dev_params(net, dev):
    return LC.dev_params(net[0], dev)


def _run(dev, P, x=None, order=None, h0=None, c0=None, T=None, with_all=True, G=None):
    """The kernel: G from x on the device (or given, or None = zero input) -> hT, cT, h_all (CPU float64 numpy)."""
    from fs_eend_amd import ops
    f32 = dict(dtype=torch.float32, device=dev)
    if x is not None:
        G, _ = LC.device_G(P, x, dev)
    B = G.shape[0] if G is not None else h0.shape[0]
    T = G.shape[1] if G is not None else T
    hT, cT = torch.empty(B, H, **f32), torch.empty(B, H, **f32)
    h_all = torch.full((B, T, H), float("nan"), **f32) if with_all else None
    ops.lstm(G, LC.dev_order(order, dev), None if G is not None else P["b"], P["w_hh"], None if h0 is None else h0.to(dev),
             None if c0 is None else c0.to(dev), hT, cT, h_all, B, T)
    torch.cuda.synchronize()
    return hT.cpu(), cT.cpu(), None if h_all is None else h_all.cpu()


def _check(name, got, ref, t32):
    """got / ref / t32: (hT, cT, h_all) of the kernel, the float64 restatement, torch's fp32 LSTM."""
    for what, g, r, t in zip(("hT", "cT", "h_all"), got, ref, t32):
        err, bar, _ = LC.err_and_bar(name, what, g, r, t.double().numpy(), K)       # bar = K x gap32
        assert err <= bar, f"{name} {what}: {err:.2e} > {bar:.2e}"


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("state", [False, True])
def test_recurrence_vs_float64(hip_lib, dev, net, B, T, permuted, state):
    lstm, p64 = net
    g = torch.Generator().manual_seed(100 * B + T)
    x = torch.randn(B, T, H, generator=g)
    order = np.random.RandomState(T).permutation(T) if permuted else None
    h0 = 0.5 * torch.randn(B, H, generator=g) if state else None
    c0 = torch.randn(B, H, generator=g) if state else None
    xo = x if order is None else x[:, torch.as_tensor(order)]
    with torch.no_grad():
        y, (hn, cn) = lstm(xo, None if h0 is None else (h0[None], c0[None]))
    G64 = x.double().numpy() @ p64["weight_ih_l0"].T + p64["bias_ih_l0"] + p64["bias_hh_l0"]
    ref = ER.lstm(p64["weight_hh_l0"], G64, order, h0, c0)
    got = _run(dev, _dev_params(net, dev), x, order, h0, c0)
    _check(f"B{B} T{T} perm{int(permuted)} state{int(state)}", got, ref, (hn[0], cn[0], y))
    assert torch.equal(got[0], got[2][:, -1])                                  # hT is the last step's h
    # hT / cT without the per-step output: the same bits
    lean = _run(dev, _dev_params(net, dev), x, order, h0, c0, with_all=False)
    assert torch.equal(lean[0], got[0]) and torch.equal(lean[1], got[1])


@pytest.mark.parametrize("B", [1, 3])
def test_zero_input_decoder_form(hip_lib, dev, net, B):
    """G = NULL: 15 steps from a given state, the pre-activation is the bias sum alone (no GEMM)."""
    lstm, p64 = net
    g = torch.Generator().manual_seed(7 + B)
    h0, c0 = 0.5 * torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)
    with torch.no_grad():
        y, (hn, cn) = lstm(torch.zeros(B, 15, H), (h0[None], c0[None]))
    ref = ER.lstm(p64["weight_hh_l0"], None, None, h0, c0, p64["bias_ih_l0"] + p64["bias_hh_l0"], 15)
    got = _run(dev, _dev_params(net, dev), None, None, h0, c0, T=15)
    _check(f"zero-input B{B}", got, ref, (hn[0], cn[0], y))


def test_saturating_preactivations_stay_finite(hip_lib, dev, net):
    g = torch.Generator().manual_seed(99)
    G = (torch.randint(0, 2, (2, 9, 4 * H), generator=g).float() * 160.0 - 80.0).to(dev)
    c0 = 50.0 * torch.randn(2, H, generator=g)
    hT, cT, h_all = _run(dev, _dev_params(net, dev), G=G, h0=torch.zeros(2, H), c0=c0)
    for t in (hT, cT, h_all):
        assert torch.isfinite(t).all()
    assert h_all.abs().max() <= 1.0
    # +-80 are hard gates: an open forget gate with a closed input gate keeps c, a closed forget gate with an open input gate sets it
    i, f, gg = (G[:, 0, k * H:(k + 1) * H].cpu() > 0 for k in range(3))
    c1 = torch.where(f, c0, torch.zeros_like(c0)) + torch.where(i, torch.where(gg, 1.0, -1.0), torch.zeros_like(c0))
    G1 = G[:, :1].contiguous()
    _, cT1, _ = _run(dev, _dev_params(net, dev), G=G1, h0=torch.zeros(2, H), c0=c0)
    assert (cT1 - c1).abs().max() < 1e-4      # W_hh h = 0 at the first step; sigmoid(+-80), tanh(+-80) are 0 / 1 / -1 to f32


def test_bits_do_not_depend_on_the_run_or_the_batch(hip_lib, dev, net):
    g = torch.Generator().manual_seed(5)
    B, T = 5, 33
    x = torch.randn(B, T, H, generator=g)
    order = np.random.RandomState(3).permutation(T)
    P = _dev_params(net, dev)
    a = _run(dev, P, x, order)
    b = _run(dev, P, x, order)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for i in (0, 3, 4):
        alone = _run(dev, P, x[i:i + 1], order)
        for u, v in zip(alone, a):
            assert torch.equal(u[0], v[i])


def test_rejected_shapes(hip_lib, dev, net):
    from fs_eend_amd import ops
    from fs_eend_amd.lib import EendHipError
    f32 = dict(dtype=torch.float32, device=dev)
    P = _dev_params(net, dev)
    hT, cT = torch.empty(1, H, **f32), torch.empty(1, H, **f32)
    assert not ops.lstm_ok(1, 1, 128) and not ops.lstm_ok(1, 0, H) and not ops.lstm_ok(0, 1, H) and ops.lstm_ok(1, 1, H)
    with pytest.raises(EendHipError):                                          # hidden size 128
        ops.lstm(torch.zeros(1, 2, 512, **f32), None, None, torch.zeros(512, 128, **f32), None, None, torch.empty(1, 128, **f32),
                 torch.empty(1, 128, **f32), None, 1, 2)
    with pytest.raises(EendHipError):                                          # T = 0
        ops.lstm(torch.zeros(1, 1, 4 * H, **f32), None, None, P["w_hh"], None, None, hT, cT, None, 1, 0)
    with pytest.raises(EendHipError):                                          # fewer rows of G than steps
        ops.lstm(torch.zeros(1, 2, 4 * H, **f32), None, None, P["w_hh"], None, None, hT, cT, None, 1, 3)
    L = hip_lib
    s = torch.cuda.current_stream().cuda_stream
    assert L.eend_lstm_f32(None, 0, None, P["b"].data_ptr(), P["w_hh"].data_ptr(), None, None, hT.data_ptr(), cT.data_ptr(), None, 0, 15,
                           H, s) == -1                                         # B = 0
