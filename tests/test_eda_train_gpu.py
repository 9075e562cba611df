"""GPU: the differentiable attractor path of fs_eend_amd.eda_model -- `EncoderDecoderAttractor.forward` under autograd against the
golden vectors the reference produced (tools/gen_golden_eda_train.py), and `TransformerEDADiarization.forward` with a frozen encoder
against the float64 restatement (tests/eda_train_ref.py) fed the kernels' own embeddings.

Bars.  Goldens: max |got - golden| / rms(golden) within 2^13 times the golden's stored fp32-vs-float64 gap, the bar test_eda_gpu.py
uses for outputs that pass through f16 encoder operands.  Nothing here is 16-bit, so that bar is only the ceiling: err / bar is
printed and recorded in profiles/eda_train_margins.json.  Frozen-encoder gradients: K x max(gap32, 2^-24 max|ref|), K = 8, with gap32
torch's CPU fp32 autograd of the same modules on the same embeddings against the float64 restatement (the bar of test_lstm_bwd_gpu.py).
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

from oracle import fixtures as FX
from tests import eda_train_ref as TR

pytestmark = pytest.mark.gpu

RATIO = 2.0 ** 13
K = 8.0
CASES = FX.list_cases("edatrain_")
MARGINS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eda_train_margins.json")


def _record(key, rows):
    data = {}
    if os.path.exists(MARGINS):
        with open(MARGINS) as f:
            data = json.load(f)
    data[key] = rows
    with open(MARGINS, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def _rel_err(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(got.detach().cpu().double().numpy().reshape(want.shape) - want).max() / np.sqrt((want ** 2).mean()))


def test_the_two_goldens_exist():
    assert CASES == ["edatrain_B3", "edatrain_T37"]


@pytest.mark.parametrize("name", CASES)
def test_eda_forward_and_backward_vs_golden(hip_lib, dev, name):
    meta, arr = FX.load_case(name)
    eda = TR.build_mirror(meta).to(dev)
    xs, Ra, order = TR.golden_inputs(meta)
    xs = xs.to(dev).requires_grad_(True)
    loss, attractors = eda(xs, meta["n_speakers"], order=order)
    assert loss.shape == () and attractors.shape == (meta["B"], max(meta["n_speakers"]) + 1, 256)
    (loss + (attractors * Ra.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    report, failed = {}, []
    for key, got in (("loss", loss), ("attractors", attractors), ("dxs", xs.grad)):
        assert torch.isfinite(got).all(), key
        err, bar = _rel_err(got, arr[key]), RATIO * meta["gaps"][key]["rel"]
        report[key] = dict(err=err, bar=bar, ratio=err / bar)
        print(f"{name} {key}: err {err:.3e} bar {bar:.3e} err/bar {err / bar:.5f}")
        if err > bar:
            failed.append(f"{key}: {err:.3e} > {bar:.3e}")
    grads = dict(eda.named_parameters())
    assert set(grads) == set(TR.EDA_PARAMS)
    for k in TR.EDA_PARAMS:
        g = grads[k].grad
        assert g is not None and g.shape == grads[k].shape and torch.isfinite(g).all(), k
        want = meta["grad_norms"][k]
        if want == 0.0:
            continue
        err, bar = abs(float(g.double().norm()) - want) / want, RATIO * meta["grad_norm_gaps"][k]
        report["norm " + k] = dict(err=err, bar=bar, ratio=err / bar)
        print(f"{name} |d {k}|: err {err:.3e} bar {bar:.3e} err/bar {err / bar:.5f}")
        if err > bar:
            failed.append(f"|d {k}|: {err:.3e} > {bar:.3e}")
    _record(name, report)
    assert not failed, f"{name}: " + "; ".join(failed)
    assert not eda.decoder.weight_ih_l0.grad.any()                 # zero input: exactly zero, as torch returns
    assert torch.equal(eda.encoder.bias_ih_l0.grad, eda.encoder.bias_hh_l0.grad)
    assert torch.equal(eda.decoder.bias_ih_l0.grad, eda.decoder.bias_hh_l0.grad)


def test_without_grad_mode_nothing_is_kept(hip_lib, dev, monkeypatch):
    """torch.no_grad() with parameters that require grad (a validation loop): the same bits, the recurrence is handed no buffer for
    gates, cell states or h_prev, the loss kernel none for its gradients, and the call's peak memory is below the training call's by
    at least those buffers."""
    from fs_eend_amd import ops
    meta, _ = FX.load_case("edatrain_B3")
    eda = TR.build_mirror(meta).to(dev)
    assert all(p.requires_grad for p in eda.parameters())
    xs, _, order = TR.golden_inputs(meta)
    xs = xs.to(dev)
    B, T, C = meta["B"], meta["T"], max(meta["n_speakers"]) + 1
    seen = []
    real_train, real_loss = ops.lstm_train, ops.eda_count_loss

    def spy_train(G, order, bias, w_hh, h0, c0, hT, cT, h_all, gates, c_all, h_prev, B, T):
        seen.append(("lstm", gates is None and c_all is None and h_prev is None))
        return real_train(G, order, bias, w_hh, h0, c0, hT, cT, h_all, gates, c_all, h_prev, B, T)

    def spy_loss(attractors, w, bias, n_spk, loss, dattractors, dw, dbias):
        seen.append(("loss", dattractors is None and dw is None and dbias is None))
        return real_loss(attractors, w, bias, n_spk, loss, dattractors, dw, dbias)

    monkeypatch.setattr(ops, "lstm_train", spy_train)
    monkeypatch.setattr(ops, "eda_count_loss", spy_loss)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base

    eda(xs, meta["n_speakers"], order=order)                       # warm-up: operand copies are made once
    seen.clear()
    (loss, attractors), peak_train = peak(lambda: eda(xs, meta["n_speakers"], order=order))
    assert seen == [("lstm", False), ("lstm", False), ("loss", False)] and loss.grad_fn is not None
    seen.clear()
    with torch.no_grad():
        (loss2, attractors2), peak_eval = peak(lambda: eda(xs, meta["n_speakers"], order=order))
    assert seen == [("lstm", True), ("lstm", True), ("loss", True)]
    assert torch.equal(loss2, loss.detach()) and torch.equal(attractors2, attractors.detach())
    assert not loss2.requires_grad and loss2.grad_fn is None
    kept = 4 * (B * T * (4 * 256 + 256 + 256) + B * C * (4 * 256 + 256 + 256 + 256))      # gates, c_all, h_prev twice; d attractors
    print(f"peak bytes: training call {peak_train}, no-grad call {peak_eval}, buffers kept for the backward {kept}")
    assert peak_eval <= peak_train - kept


def test_an_in_place_write_before_backward_raises(hip_lib, dev):
    """The saved tensors go through save_for_backward: torch's version check holds for xs and for the parameters."""
    meta, _ = FX.load_case("edatrain_T37")
    eda = TR.build_mirror(meta).to(dev)
    xs = TR.golden_inputs(meta)[0].to(dev).requires_grad_(True)
    loss, _ = eda(xs, meta["n_speakers"])
    with torch.no_grad():
        xs.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    loss, _ = eda(xs, meta["n_speakers"])
    with torch.no_grad():
        eda.encoder.weight_hh_l0.mul_(0.5)                         # an optimiser step between forward and backward
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    loss, _ = eda(xs, meta["n_speakers"])
    loss.backward()
    with pytest.raises(RuntimeError):                              # once differentiable, and the buffers are gone
        loss.backward()


LENGTHS, N_SPK = [37, 20], [2, 3]


@pytest.fixture(scope="module")
def frozen(dev):
    from fs_eend_amd.eda_model import TransformerEDADiarization
    torch.manual_seed(41)
    m = TransformerEDADiarization(n_speakers=None, in_size=345, n_units=256, n_heads=4, n_layers=2, dropout=0.1, attractor_loss_ratio=0.5)
    FX.perturb_(m, 61)
    with torch.no_grad():
        m.eda.counter.weight.mul_(16.0)
    m = m.to(dev)
    m.enc.requires_grad_(False)
    src = [s.to(dev) for s in FX.make_src(LENGTHS, 345, 831)]
    tgt = [t.to(dev) for t in FX.make_labels(LENGTHS, N_SPK, 841)]
    return m, src, tgt


def _total(output, aloss, tgt):
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    return aloss + sum(bce(y, t) for y, t in zip(output, tgt)) / len(output)


def test_frozen_encoder_forward(hip_lib, dev, frozen):
    m, src, tgt = frozen
    m.zero_grad()
    output, aloss, emb, attractors = m(src, tgt, LENGTHS)
    T, C = max(LENGTHS), max(N_SPK) + 1
    assert [tuple(y.shape) for y in output] == [(l, n) for l, n in zip(LENGTHS, N_SPK)]
    assert aloss.shape == () and emb.shape == (2, T, 256) and attractors.shape == (2, C - 1, 256)
    assert not emb.requires_grad and aloss.requires_grad and output[0].requires_grad
    total = _total(output, aloss, tgt)
    total.backward()
    torch.cuda.synchronize()
    # the logits are test()'s, bit for bit
    m.test(src, LENGTHS, n_spk=max(N_SPK), order=np.arange(T))
    for b, (y, l, n) in enumerate(zip(output, LENGTHS, N_SPK)):
        assert torch.equal(y.detach(), m.last_logits[b, :l, :n]), b
    assert all(p.grad is None for p in m.enc.parameters())
    # float64: the restatement on the kernels' own embeddings, the head and the BCE through torch float64 on the restated logits
    e64 = emb.detach().cpu().double()
    p64 = {k: v.detach().cpu().double() for k, v in m.eda.named_parameters()}
    att = torch.as_tensor(TR.attractor_path(p64, e64, N_SPK)["attractors"]).requires_grad_(True)
    logits = torch.bmm(e64, att.transpose(1, 2))
    out64 = [logits[b, :l, :n] for b, (l, n) in enumerate(zip(LENGTHS, N_SPK))]
    _total(out64, torch.zeros((), dtype=torch.float64), [t.cpu().double() for t in tgt]).backward()
    ref = TR.attractor_path(p64, e64, N_SPK, dloss=m.attractor_loss_ratio, dattractors=att.grad)
    # gap32: torch's fp32 autograd of the same modules on the same embeddings (the reference's forward, model :40-52)
    eda32 = copy.deepcopy(m.eda).cpu()
    eda32.zero_grad()
    e32 = emb.detach().cpu()
    _, (hn, cn) = eda32.encoder(e32)
    a32, _ = eda32.decoder(torch.zeros(2, C, 256), (hn, cn))
    labels = torch.cat([torch.tensor([[1.0] * n + [0.0]]) for n in N_SPK], dim=1)
    logit = torch.cat([eda32.counter(a[:n + 1, :]).reshape(-1, n + 1) for a, n in zip(a32, N_SPK)], dim=1)
    l32 = torch.nn.functional.binary_cross_entropy_with_logits(logit, labels)
    y32 = torch.bmm(e32, a32.transpose(1, 2))
    _total([y32[b, :l, :n] for b, (l, n) in enumerate(zip(LENGTHS, N_SPK))], m.attractor_loss_ratio * l32, [t.cpu() for t in tgt]).backward()
    g32 = {k: v.grad for k, v in eda32.named_parameters()}
    report, failed = {}, []
    for k, p in m.eda.named_parameters():
        want = ref["grads"][k]
        gap32 = float(np.abs(g32[k].double().numpy() - want).max())
        bar = K * max(gap32, 2.0 ** -24 * float(np.abs(want).max()))
        err = float(np.abs(p.grad.cpu().double().numpy() - want).max())
        if bar == 0.0:
            assert err == 0.0, k
            continue
        report[k] = dict(err=err, gap32=gap32, ratio=err / bar)
        print(f"frozen {k}: err {err:.2e} gap32 {gap32:.2e} err/bar {err / bar:.3f}")
        if err > bar:
            failed.append(f"{k}: {err:.2e} > {bar:.2e}")
    _record("frozen_encoder", report)
    assert not failed, "; ".join(failed)


def test_twenty_adam_steps_lower_the_loss(hip_lib, dev, frozen):
    """A check of sign and scaling, not a measurement."""
    m, src, tgt = frozen
    m = copy.deepcopy(m)
    opt = torch.optim.Adam(m.eda.parameters(), lr=1e-3)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        output, aloss, _, _ = m(src, tgt, LENGTHS)
        total = _total(output, aloss, tgt)
        total.backward()
        opt.step()
        losses.append(float(total.detach()))
    print("total loss:", " ".join(f"{v:.4f}" for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
