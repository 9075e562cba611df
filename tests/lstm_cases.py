"""What tests/test_lstm_gpu.py and tests/test_lstm_bwd_gpu.py share: the seeded nn.LSTM, its parameters on the device, the input
pre-activations computed on the device as the model computes them, and the K x gap32 comparison."""
import numpy as np
import torch

H = 256


def seeded_lstm():
    """The one nn.LSTM of both suites (CPU fp32: the gap32 side)."""
    torch.manual_seed(1234)
    lstm = torch.nn.LSTM(H, H, 1, batch_first=True)
    with torch.no_grad():
        for p in lstm.parameters():
            p.mul_(1.5)                   # a livelier recurrence than the default 1/16 range
    return lstm


def dev_params(lstm, dev):
    w_ih = lstm.weight_ih_l0.detach().to(dev).contiguous()
    return dict(w_ih=w_ih, w_ih_t=w_ih.t().contiguous(), w_hh=lstm.weight_hh_l0.detach().to(dev).contiguous(),
                b=(lstm.bias_ih_l0 + lstm.bias_hh_l0).detach().to(dev).contiguous())


def dev_order(order, dev):
    return None if order is None else torch.as_tensor(np.asarray(order), dtype=torch.int32, device=dev)


def device_G(P, x, dev):
    """x (B, T, H) -> G f32 (B, T, 4H) = x W_ih^T + b by eend_linear_step_f32, and x's rows (B T, H) on the device."""
    from fs_eend_amd import ops
    B, T, _ = x.shape
    G = torch.empty(B, T, 4 * H, dtype=torch.float32, device=dev)
    xd = x.to(dev).reshape(B * T, H).contiguous()
    ops.linear_step_f32(xd, P["w_ih"], P["b"], G.view(B * T, 4 * H))
    return G, xd


def err_and_bar(name, what, got, ref, t32, K, rel_floor=0.0):
    """got: a CPU tensor; ref / t32: float64 arrays of the float64 reference and of torch's fp32 one.  Prints and returns
    (err, bar, err / bar) with bar = K x max(gap32, rel_floor max|ref|); got must be finite."""
    g = got.double().numpy()
    gap32 = float(np.abs(t32 - ref).max())
    bar = K * max(gap32, rel_floor * float(np.abs(ref).max()))
    err = float(np.abs(g - ref).max())
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{name} {what}: err {err:.2e} gap32 {gap32:.2e} err/bar {ratio:.3f}")
    assert np.isfinite(g).all(), f"{name} {what}"
    return err, bar, ratio
