"""GPU: eend_lstm_train_f32, eend_lstm_bwd_f32 (csrc/lstm.hip) and eend_wgrad_f32 (csrc/wgrad_f32.hip) against torch's CPU float64
autograd of a seeded nn.LSTM (weights x 1.5, as in test_lstm_gpu.py).

The scalar is S = sum(h_all R1) + sum(hT R2) + sum(cT R3) with seeded R.  To read d S / d G (the pre-activation gradient, which nn.LSTM
does not expose) the reference LSTM takes 1024 extra input columns e against an identity block appended to W_ih, so that its
pre-activation is x W_ih^T + e + b and d S / d e at e = 0 is dG in step order.

Bar per tensor: K x max(gap32, 2^-24 max|ref|) with K = 8, where gap32 is torch's own CPU fp32 autograd against the float64 one on
the same inputs: nothing on the path is 16-bit, only the order of the sums differs (the bar of test_lstm_gpu.py, for the same reason).
The worst err / bar per tensor class goes to profiles/eda_train_margins.json.

eend_wgrad_f32 alone: every element within M 2^-24 sum_m |dY X| of the float64 sum, the worst case of an M-long fmaf chain.  Its rows
are cut into 16 slices of 4 ceil(M / 64) rows, so M = 64 is the size at which every slice holds one MFMA step ("one round" below).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import lstm_cases as LC
from tests.lstm_cases import H

pytestmark = pytest.mark.gpu

K = 8.0
SHAPES = [(1, 1), (1, 2), (3, 65), (2, 130), (17, 5)]
MARGINS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eda_train_margins.json")
_worst = {}


def _record(cls, ratio):
    _worst[cls] = max(_worst.get(cls, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _write_margins():
    yield
    if not _worst:
        return
    data = {}
    if os.path.exists(MARGINS):
        with open(MARGINS) as f:
            data = json.load(f)
    data["test_lstm_bwd_gpu"] = dict(K=K, worst_err_over_bar={k: _worst[k] for k in sorted(_worst)})
    with open(MARGINS, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def net():
    """The seeded nn.LSTM of test_lstm_gpu.py and its widened twins (1024 identity input columns) in fp32 and float64."""
    lstm = LC.seeded_lstm()
    wide = {}
    for dt in (torch.float32, torch.float64):
        w = torch.nn.LSTM(H + 4 * H, H, 1, batch_first=True).to(dt)
        with torch.no_grad():
            w.weight_ih_l0.copy_(torch.cat([lstm.weight_ih_l0, torch.eye(4 * H)], dim=1).to(dt))
            w.weight_hh_l0.copy_(lstm.weight_hh_l0.to(dt))
            w.bias_ih_l0.copy_(lstm.bias_ih_l0.to(dt))
            w.bias_hh_l0.copy_(lstm.bias_hh_l0.to(dt))
        wide[dt] = w
    return lstm, wide


def _dev_params(net, dev):
    return LC.dev_params(net[0], dev)


def _orders(order, B, T):
    """None / (T,) / (B, T) -> a (B, T) int64 array of the row each sequence reads at each step."""
    if order is None:
        return np.tile(np.arange(T), (B, 1))
    o = np.asarray(order)
    return np.tile(o, (B, 1)) if o.ndim == 1 else o


def _reference(wide, dt, x, order, h0, c0, R, zero_input=False):
    """torch autograd of the widened LSTM in dtype dt -> dict of gradients (float64 numpy), dG in the row layout."""
    w = wide[dt]
    w.zero_grad()
    B, T = R[0].shape[:2]
    ob = torch.as_tensor(_orders(order, B, T))
    xs = (torch.zeros(B, T, H, dtype=dt) if zero_input else x.to(dt).clone()).requires_grad_(not zero_input)
    e = torch.zeros(B, T, 4 * H, dtype=dt, requires_grad=True)
    xo = torch.gather(xs, 1, ob[:, :, None].expand(B, T, H))
    h = (torch.zeros(B, H) if h0 is None else h0).to(dt).clone().requires_grad_(True)
    c = (torch.zeros(B, H) if c0 is None else c0).to(dt).clone().requires_grad_(True)
    y, (hn, cn) = w(torch.cat([xo, e], dim=2), (h[None], c[None]))
    S = (y * R[0].to(dt)).sum()
    if R[1] is not None:
        S = S + (hn[0] * R[1].to(dt)).sum() + (cn[0] * R[2].to(dt)).sum()
    S.backward()
    dG = torch.zeros(B, T, 4 * H, dtype=dt)
    dG.scatter_(1, ob[:, :, None].expand(B, T, 4 * H), e.grad)
    out = dict(dG=dG, dh0=h.grad, dc0=c.grad, dW_hh=w.weight_hh_l0.grad, db=w.bias_ih_l0.grad)
    if not zero_input:
        out.update(dW_ih=w.weight_ih_l0.grad[:, :H], dx=xs.grad)
    return {k: v.detach().double().numpy().copy() for k, v in out.items()}


def _kernel(dev, P, x, order, h0, c0, R):
    """The device path: G by eend_linear_step_f32 (or zero input), the training forward, the backward, the weight gradients."""
    from fs_eend_amd import ops
    f32 = dict(dtype=torch.float32, device=dev)
    zero_input = x is None
    B, T = (R[0].shape[0], R[0].shape[1])
    G, xd = (None, None) if zero_input else LC.device_G(P, x, dev)
    o = LC.dev_order(order, dev)
    h0d, c0d = (None if t is None else t.to(dev) for t in (h0, c0))
    hT, cT = torch.empty(B, H, **f32), torch.empty(B, H, **f32)
    h_all, c_all, h_prev = (torch.full((B, T, H), float("nan"), **f32) for _ in range(3))
    gates = torch.full((B, T, 4 * H), float("nan"), **f32)
    ops.lstm_train(G, o, None if G is not None else P["b"], P["w_hh"], h0d, c0d, hT, cT, h_all, gates, c_all, h_prev, B, T)
    dG = torch.full((B, T, 4 * H), float("nan"), **f32)
    dh0, dc0 = torch.empty(B, H, **f32), torch.empty(B, H, **f32)
    Rd = [None if r is None else r.to(dev).contiguous() for r in R]
    ops.lstm_bwd(gates, c_all, c0d, P["w_hh"], Rd[0], Rd[1], Rd[2], o, dG, dh0, dc0, B, T)
    ws = torch.empty(ops.wgrad_f32_workspace_bytes(4 * H, H, True) // 4, **f32)
    dW_hh, db = torch.empty(4 * H, H, **f32), torch.empty(4 * H, **f32)
    ops.wgrad_f32(dG.view(B * T, 4 * H), h_prev.view(B * T, H), ws, dW_hh, db)
    out = dict(dG=dG, dh0=dh0, dc0=dc0, dW_hh=dW_hh, db=db)
    if not zero_input:
        dW_ih, dx = torch.empty(4 * H, H, **f32), torch.empty(B, T, H, **f32)
        ops.wgrad_f32(dG.view(B * T, 4 * H), xd, ws, dW_ih, None)
        ops.linear_step_f32(dG.view(B * T, 4 * H), P["w_ih_t"], None, dx.view(B * T, H))
        out.update(dW_ih=dW_ih, dx=dx)
    torch.cuda.synchronize()
    fwd = dict(hT=hT.cpu(), cT=cT.cpu(), h_all=h_all.cpu(), h_prev=h_prev.cpu(), G=G)
    return {k: v.cpu() for k, v in out.items()}, fwd


def _check(name, got, ref, t32):
    failed = []
    for what in ref:
        err, bar, ratio = LC.err_and_bar(name, what, got[what], ref[what], t32[what], K, 2.0 ** -24)
        _record(what, ratio)
        if err > bar:
            failed.append(f"{what}: {err:.2e} > {bar:.2e}")
    assert not failed, f"{name}: " + "; ".join(failed)


def _forward(dev, P, G, o, h0, c0, B, T, keep):
    """hT, cT, h_all of ops.lstm (keep None), or of ops.lstm_train without (False) / with (True) the backward's three buffers."""
    from fs_eend_amd import ops
    f32 = dict(dtype=torch.float32, device=dev)
    hT, cT, h_all = torch.empty(B, H, **f32), torch.empty(B, H, **f32), torch.full((B, T, H), float("nan"), **f32)
    args = (G, o, None if G is not None else P["b"], P["w_hh"], None if h0 is None else h0.to(dev), None if c0 is None else c0.to(dev))
    if keep is None:
        ops.lstm(*args, hT, cT, h_all, B, T)
    else:
        kept = (torch.empty(B, T, 4 * H, **f32), torch.empty(B, T, H, **f32), torch.empty(B, T, H, **f32)) if keep else (None,) * 3
        ops.lstm_train(*args, hT, cT, h_all, *kept, B, T)
    torch.cuda.synchronize()
    return hT.cpu(), cT.cpu(), h_all.cpu()


def _inputs(B, T, state, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, H, generator=g)
    h0 = 0.5 * torch.randn(B, H, generator=g) if state else None
    c0 = torch.randn(B, H, generator=g) if state else None
    R = [torch.randn(B, T, H, generator=g), torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)]
    return x, h0, c0, R


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("order_kind", ["identity", "permuted", "per_sequence"])
@pytest.mark.parametrize("state", [False, True])
def test_backward_vs_float64_autograd(hip_lib, dev, net, B, T, order_kind, state):
    _, wide = net
    x, h0, c0, R = _inputs(B, T, state, 100 * B + T)
    order = None
    if order_kind == "permuted":
        order = np.random.RandomState(T).permutation(T)
    elif order_kind == "per_sequence":
        order = np.stack([np.random.RandomState(1000 + 7 * b + T).permutation(T) for b in range(B)])
    ref = _reference(wide, torch.float64, x, order, h0, c0, R)
    t32 = _reference(wide, torch.float32, x, order, h0, c0, R)
    P = _dev_params(net, dev)
    got, fwd = _kernel(dev, P, x, order, h0, c0, R)
    _check(f"B{B} T{T} {order_kind} state{int(state)}", got, ref, t32)
    # the training forward has the inference entry's bits
    hT, cT, h_all = _forward(dev, P, fwd["G"], LC.dev_order(order, dev), h0, c0, B, T, None)
    assert torch.equal(hT, fwd["hT"]) and torch.equal(cT, fwd["cT"]) and torch.equal(h_all, fwd["h_all"])
    # h_prev: row order[t] holds the hidden state that entered step t
    ob = _orders(order, B, T)
    first = torch.zeros(B, H) if h0 is None else h0
    for b in range(B):
        for t in range(T):
            want = first[b] if t == 0 else fwd["h_all"][b, t - 1]
            assert torch.equal(fwd["h_prev"][b, ob[b, t]], want), (b, t)


@pytest.mark.parametrize("T", [1, 2, 15, 16])
def test_decoder_form(hip_lib, dev, net, T):
    """G = NULL (the pre-activation is the bias), upstream dh_all only: every step's h is an attractor."""
    _, wide = net
    B = 3
    g = torch.Generator().manual_seed(40 + T)
    h0, c0 = 0.5 * torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)
    R = [torch.randn(B, T, H, generator=g), None, None]
    ref = _reference(wide, torch.float64, None, None, h0, c0, R, zero_input=True)
    t32 = _reference(wide, torch.float32, None, None, h0, c0, R, zero_input=True)
    got, fwd = _kernel(dev, _dev_params(net, dev), None, None, h0, c0, R)
    _check(f"decoder T{T}", got, ref, t32)
    assert torch.equal(fwd["h_prev"][:, 0], h0) and (T == 1 or torch.equal(fwd["h_prev"][:, 1:], fwd["h_all"][:, :-1]))


def test_a_taller_slab_of_G_leaves_the_backward_operands_T_rows_tall(hip_lib, dev, net):
    """G with more rows than steps (a padded slab, as the model's encoder hands it over) while h_prev and dG have T rows: the bits of a
    dense G, and no row beyond T is read or written."""
    from fs_eend_amd import ops
    B, T, rows = 2, 37, 64
    x, _, _, R = _inputs(B, T, False, 77)
    order = np.random.RandomState(9).permutation(T)
    P = _dev_params(net, dev)
    want, fwd = _kernel(dev, P, x, order, None, None, R)
    f32 = dict(dtype=torch.float32, device=dev)
    G = torch.full((B, rows, 4 * H), float("nan"), **f32)
    G[:, :T] = fwd["G"]
    o = torch.as_tensor(order, dtype=torch.int32, device=dev)
    hT, cT, dh0, dc0 = (torch.empty(B, H, **f32) for _ in range(4))
    gates, c_all, h_prev = torch.empty(B, T, 4 * H, **f32), torch.empty(B, T, H, **f32), torch.empty(B, T, H, **f32)
    ops.lstm_train(G, o, None, P["w_hh"], None, None, hT, cT, None, gates, c_all, h_prev, B, T)
    dG = torch.empty(B, T, 4 * H, **f32)
    ops.lstm_bwd(gates, c_all, None, P["w_hh"], R[0].to(dev), R[1].to(dev), R[2].to(dev), o, dG, dh0, dc0, B, T)
    torch.cuda.synchronize()
    assert torch.equal(h_prev.cpu(), fwd["h_prev"]) and torch.equal(hT.cpu(), fwd["hT"])
    assert torch.equal(dG.cpu(), want["dG"]) and torch.equal(dh0.cpu(), want["dh0"]) and torch.equal(dc0.cpu(), want["dc0"])


def test_bits_do_not_depend_on_the_run_or_the_batch(hip_lib, dev, net):
    B, T = 5, 33
    x, h0, c0, R = _inputs(B, T, True, 5)
    order = np.random.RandomState(3).permutation(T)
    P = _dev_params(net, dev)
    a, _ = _kernel(dev, P, x, order, h0, c0, R)
    b, _ = _kernel(dev, P, x, order, h0, c0, R)
    for k in a:
        assert torch.equal(a[k], b[k]), k                       # weight gradients included
    for i in (0, 3, 4):
        alone, _ = _kernel(dev, P, x[i:i + 1], order, h0[i:i + 1], c0[i:i + 1], [r[i:i + 1] for r in R])
        for k in ("dG", "dh0", "dc0", "dx"):
            assert torch.equal(alone[k][0], a[k][i]), (k, i)


def test_saturating_preactivations_give_finite_gradients(hip_lib, dev, net):
    from fs_eend_amd import ops
    g = torch.Generator().manual_seed(99)
    B, T = 2, 9
    f32 = dict(dtype=torch.float32, device=dev)
    G = (torch.randint(0, 2, (B, T, 4 * H), generator=g).float() * 160.0 - 80.0).to(dev)
    c0 = (50.0 * torch.randn(B, H, generator=g)).to(dev)
    h0 = torch.zeros(B, H, **f32)
    R = [torch.randn(B, T, H, generator=g).to(dev), torch.randn(B, H, generator=g).to(dev), torch.randn(B, H, generator=g).to(dev)]
    P = _dev_params(net, dev)
    hT, cT = torch.empty(B, H, **f32), torch.empty(B, H, **f32)
    h_all, c_all, h_prev = (torch.empty(B, T, H, **f32) for _ in range(3))
    gates = torch.empty(B, T, 4 * H, **f32)
    ops.lstm_train(G, None, None, P["w_hh"], h0, c0, hT, cT, h_all, gates, c_all, h_prev, B, T)
    dG, dh0, dc0 = torch.empty(B, T, 4 * H, **f32), torch.empty(B, H, **f32), torch.empty(B, H, **f32)
    ops.lstm_bwd(gates, c_all, c0, P["w_hh"], R[0], R[1], R[2], None, dG, dh0, dc0, B, T)
    ws = torch.empty(ops.wgrad_f32_workspace_bytes(4 * H, H, True) // 4, **f32)
    dW, db = torch.empty(4 * H, H, **f32), torch.empty(4 * H, **f32)
    ops.wgrad_f32(dG.view(B * T, 4 * H), h_prev.view(B * T, H), ws, dW, db)
    torch.cuda.synchronize()
    for t in (gates, c_all, h_prev, dG, dh0, dc0, dW, db):
        assert torch.isfinite(t).all()


@pytest.mark.parametrize("B,T", [(1, 1), (3, 65), (2, 130)])
def test_one_launcher_gives_one_set_of_bits(hip_lib, dev, net, B, T):
    """eend_lstm_orders_f32, eend_lstm_train_f32 with nothing to keep (the inference instance) and with all three buffers (the
    training instance): the same hT, cT and h_all, with an order per sequence and a given initial state."""
    x, h0, c0, _ = _inputs(B, T, True, 300 * B + T)
    P = _dev_params(net, dev)
    G, _ = LC.device_G(P, x, dev)
    o = LC.dev_order(np.stack([np.random.RandomState(2000 + 7 * b + T).permutation(T) for b in range(B)]), dev)
    runs = [_forward(dev, P, G, o, h0, c0, B, T, keep) for keep in (None, False, True)]
    assert all(torch.isfinite(t).all() for t in runs[0])
    for other in runs[1:]:
        assert all(torch.equal(u, v) for u, v in zip(runs[0], other))


def test_zero_input_with_a_shared_order(hip_lib, dev, net):
    """The one argument rule on which the entries differ: over a zero input lstm() ignores a shared order, lstm_train() refuses it."""
    from fs_eend_amd.lib import EendHipError
    B, T = 2, 3
    _, h0, c0, _ = _inputs(B, T, True, 11)
    P = _dev_params(net, dev)
    order = LC.dev_order(np.array([2, 0, 1]), dev)
    plain, ordered = (_forward(dev, P, None, o, h0, c0, B, T, None) for o in (None, order))
    assert all(torch.isfinite(t).all() for t in plain) and all(torch.equal(u, v) for u, v in zip(plain, ordered))
    with pytest.raises(EendHipError):
        _forward(dev, P, None, order, h0, c0, B, T, False)


ROUND = 64          # 16 slices x the MFMA's 4 rows


# 130: 11 slices of 12 rows, the last with 10 (not a multiple of the MFMA's 4); 257: 13 slices of 20 rows, the last with 17, so its
# second 16-row pass holds one live row
@pytest.mark.parametrize("M", [1, 15, 16, 17, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 2, 3 * ROUND + 7, 4 * ROUND + 1, 1031])
def test_wgrad_f32_alone(hip_lib, dev, M):
    from fs_eend_amd import ops
    N, Kk = 4 * H, H
    g = torch.Generator().manual_seed(M)
    dy, x = torch.randn(M, N, generator=g), torch.randn(M, Kk, generator=g)
    ref = dy.double().T @ x.double()
    bound = M * 2.0 ** -24 * (dy.double().abs().T @ x.double().abs())
    f32 = dict(dtype=torch.float32, device=dev)
    ws = torch.full((ops.wgrad_f32_workspace_bytes(N, Kk, True) // 4,), float("nan"), **f32)
    runs = []
    for _ in range(2):
        dw, db = torch.full((N, Kk), float("nan"), **f32), torch.full((N,), float("nan"), **f32)
        ops.wgrad_f32(dy.to(dev), x.to(dev), ws, dw, db)
        torch.cuda.synchronize()
        runs.append((dw.cpu(), db.cpu()))
    dw, db = runs[0]
    assert torch.equal(dw, runs[1][0]) and torch.equal(db, runs[1][1])
    err = (dw.double() - ref).abs()
    print(f"M{M}: worst err / bound {float((err / bound).max()):.3f}")
    _record("wgrad_f32_alone", float((err / bound).max()))
    assert bool((err <= bound).all())
    berr = (db.double() - dy.double().sum(0)).abs()
    assert bool((berr <= M * 2.0 ** -24 * dy.double().abs().sum(0)).all())
    # without the bias, and with row strides wider than the rows: the same weight gradient
    wide_dy, wide_x = torch.zeros(M, N + 64, **f32), torch.zeros(M, Kk + 4, **f32)
    wide_dy[:, :N], wide_x[:, :Kk] = dy.to(dev), x.to(dev)
    dw2 = torch.empty(N, Kk, **f32)
    L = hip_lib
    s = torch.cuda.current_stream().cuda_stream
    assert L.eend_wgrad_f32(wide_dy.data_ptr(), N + 64, wide_x.data_ptr(), Kk + 4, M, N, Kk, ws.data_ptr(), ws.numel() * 4, dw2.data_ptr(),
                            None, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(dw2.cpu(), dw)


def test_rejected_shapes(hip_lib, dev):
    """EEND_EINVAL before any launch: the pointers below are never dereferenced."""
    L = hip_lib
    p = 0x1000
    assert L.eend_wgrad_f32_workspace_bytes(1024, 256, 0) == 16 * 1024 * 256 * 4
    assert L.eend_wgrad_f32_workspace_bytes(1024, 256, 1) == 16 * (1024 * 256 + 1024) * 4
    assert L.eend_wgrad_f32_workspace_bytes(1000, 256, 0) == 0 and L.eend_wgrad_f32_workspace_bytes(1024, 100, 0) == 0
    big = 1 << 30
    wg = lambda dY=p, ldy=1024, X=p, ldx=256, M=8, N=1024, Kk=256, ws=p, wsb=big, dW=p, db=None: \
        L.eend_wgrad_f32(dY, ldy, X, ldx, M, N, Kk, ws, wsb, dW, db, None)
    for kw in (dict(N=1000), dict(Kk=100), dict(N=0), dict(M=0), dict(ldy=1023), dict(ldx=255), dict(dY=None), dict(X=None), dict(ws=None),
               dict(dW=None), dict(wsb=16 * 1024 * 256 * 4 - 1), dict(db=p, wsb=16 * 1024 * 256 * 4)):
        assert wg(**kw) == -1, kw
    tr = lambda G=p, rows=4, order=None, stride=0, bias=p, W=p, h0=None, c0=None, hT=p, cT=p, hp=4, B=1, T=4, Hh=256: \
        L.eend_lstm_train_f32(G, rows, order, stride, bias, W, h0, c0, hT, cT, None, p, p, p, hp, B, T, Hh, None)
    for kw in (dict(Hh=128), dict(T=0), dict(B=0), dict(rows=3), dict(W=None), dict(hT=None), dict(cT=None), dict(G=None, bias=None),
               dict(G=None, order=p), dict(stride=4), dict(order=p, stride=3), dict(h0=p), dict(c0=p), dict(hp=3), dict(hp=0)):
        assert tr(**kw) == -1, kw
    assert L.eend_eda_count_loss_workspace_bytes(3) == 3 * 258 * 4 and L.eend_eda_count_loss_workspace_bytes(0) == 0
    cl = lambda attr=p, n=p, loss=p, da=p, dw=p, db=p, ws=p, wsb=3 * 258 * 4, B=3, C=4: \
        L.eend_eda_count_loss_f32(attr, p, p, n, loss, da, dw, db, ws, wsb, B, C, None)
    for kw in (dict(B=0), dict(C=0), dict(C=17), dict(attr=None), dict(n=None), dict(loss=None), dict(ws=None), dict(wsb=3 * 258 * 4 - 1),
               dict(da=None), dict(dw=None, db=None), dict(da=None, dw=None)):
        assert cl(**kw) == -1, kw
    bw = lambda gates=p, c_all=p, W=p, dh_all=p, dhT=None, dcT=None, order=None, stride=0, dG=p, rows=4, dh0=p, dc0=p, B=1, T=4, Hh=256: \
        L.eend_lstm_bwd_f32(gates, c_all, None, W, dh_all, dhT, dcT, order, stride, dG, rows, dh0, dc0, B, T, Hh, None)
    for kw in (dict(Hh=128), dict(T=0), dict(B=0), dict(rows=3), dict(gates=None), dict(c_all=None), dict(W=None), dict(dG=None),
               dict(dh0=None), dict(dc0=None), dict(dh_all=None), dict(stride=4), dict(order=p, stride=3)):
        assert bw(**kw) == -1, kw
