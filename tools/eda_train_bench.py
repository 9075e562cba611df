"""Times of the differentiable EEND-EDA attractor path (fs_eend_amd.eda_model.EncoderDecoderAttractor.forward + backward) and of its
kernels alone (eend_lstm_train_f32, eend_lstm_bwd_f32, eend_wgrad_f32), next to torch's CPU nn.LSTM forward + backward for the same
shapes on the same box.  Not bench.py: nothing here is a pass/fail figure.

    python tools/eda_train_bench.py [--out profiles/eda_train_bench.json]

Shapes: B = 1, T = 5000 and B = 64, T = 500, as tools/eda_bench.py.  The parent process never opens the GPU: every GPU step is a child
process of its own under `timeout`, run one after the other, and the first one that fails ends the run.  Device times are medians of
7 repeats between two events on the stream, after warm-up calls.
"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from tools.eda_bench import _median_ms, cpu_lstm, main  # noqa: E402

SHAPES = {"b1": (1, 5000), "b64": (64, 500)}
STEPS = [("train_b1", 240), ("train_b64", 240)]
H, N_SPK, REPS = 256, 4, 7


def gpu_step(name):
    import numpy as np
    import torch
    from fs_eend_amd import ops
    from fs_eend_amd.eda_model import EncoderDecoderAttractor
    B, T = SHAPES[name.split("_")[1]]
    dev = torch.device("cuda:0")
    f32 = dict(dtype=torch.float32, device=dev)
    torch.manual_seed(0)
    eda = EncoderDecoderAttractor(H).to(dev)
    xs = torch.randn(B, T, H, **f32).requires_grad_(True)
    Ra = 1e-3 * torch.randn(B, N_SPK + 1, H, **f32)
    order = np.random.RandomState(0).permutation(T)
    res = dict(step=name, B=B, T=T, n_speakers=N_SPK, device=torch.cuda.get_device_name(0))

    def fwd_bwd():
        xs.grad = None
        eda.zero_grad()
        loss, att = eda(xs, [N_SPK] * B, order=order)
        (loss + (att * Ra).sum()).backward()

    def fwd_only():
        with torch.no_grad():
            eda(xs, [N_SPK] * B, order=order)

    med, lo, hi = _median_ms(fwd_bwd, 2, REPS)
    res.update(fwd_bwd_ms=med, fwd_bwd_ms_min=lo, fwd_bwd_ms_max=hi)
    res.update(fwd_ms=_median_ms(fwd_only, 2, REPS)[0])
    # the kernels alone, on the encoder LSTM's shapes
    P = eda._prepare()
    G = torch.randn(B, T, 4 * H, **f32)
    o = torch.as_tensor(order.astype(np.int32), device=dev)
    hT, cT, dh0, dc0 = (torch.empty(B, H, **f32) for _ in range(4))
    gates, c_all, h_prev = torch.empty(B, T, 4 * H, **f32), torch.empty(B, T, H, **f32), torch.empty(B, T, H, **f32)
    med, _, _ = _median_ms(lambda: ops.lstm_train(G, o, None, P["enc_whh"], None, None, hT, cT, None, gates, c_all, h_prev, B, T), 2, REPS)
    res.update(lstm_train_ms=med, lstm_train_us_per_step=1e3 * med / T)
    med, _, _ = _median_ms(lambda: ops.lstm(G, o, None, P["enc_whh"], None, None, hT, cT, None, B, T), 2, REPS)
    res.update(lstm_infer_ms=med, lstm_infer_us_per_step=1e3 * med / T)
    dG, dhT, dcT = torch.empty(B, T, 4 * H, **f32), torch.randn(B, H, **f32), torch.randn(B, H, **f32)
    med, lo, hi = _median_ms(lambda: ops.lstm_bwd(gates, c_all, None, P["enc_whh"], None, dhT, dcT, o, dG, dh0, dc0, B, T), 2, REPS)
    res.update(lstm_bwd_ms=med, lstm_bwd_ms_min=lo, lstm_bwd_ms_max=hi, lstm_bwd_us_per_step=1e3 * med / T)
    ws = torch.empty(ops.wgrad_f32_workspace_bytes(4 * H, H, True) // 4, **f32)
    dW, db = torch.empty(4 * H, H, **f32), torch.empty(4 * H, **f32)
    med, _, _ = _median_ms(lambda: ops.wgrad_f32(dG.view(B * T, 4 * H), h_prev.view(B * T, H), ws, dW, db), 2, REPS)
    res.update(wgrad_f32_ms=med, wgrad_f32_tflops=2.0 * B * T * 4 * H * H / (med * 1e-3) / 1e12)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main(__file__, STEPS, gpu_step, lambda B, T: cpu_lstm(B, T, backward=True), "eda_train_bench.json")
