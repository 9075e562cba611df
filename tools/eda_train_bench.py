"""Times of the differentiable EEND-EDA attractor path (fs_eend_amd.eda_model.EncoderDecoderAttractor.forward + backward) and of its
kernels alone (eend_lstm_train_f32, eend_lstm_bwd_f32, eend_wgrad_f32), next to torch's CPU nn.LSTM forward + backward for the same
shapes on the same box.  Not bench.py: nothing here is a pass/fail figure.

    python tools/eda_train_bench.py [--out profiles/eda_train_bench.json]

Shapes: B = 1, T = 5000 and B = 64, T = 500, as tools/eda_bench.py.  The parent process never opens the GPU: every GPU step is a child
process of its own under `timeout`, run one after the other, and the first one that fails ends the run.  Device times are medians of
7 repeats between two events on the stream, after warm-up calls.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = {"b1": (1, 5000), "b64": (64, 500)}
STEPS = [("train_b1", 240), ("train_b64", 240)]
H, N_SPK, REPS = 256, 4, 7


def _median_ms(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


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


def cpu_lstm(B, T, reps=3):
    import torch
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(H, H, 1, batch_first=True)
    x = torch.randn(B, T, H, requires_grad=True)
    R = torch.randn(B, T, H)
    out = []
    for i in range(reps + 1):
        lstm.zero_grad()
        x.grad = None
        t0 = time.perf_counter()
        y, _ = lstm(x)
        (y * R).sum().backward()
        if i:                                      # the first call warms up
            out.append(1e3 * (time.perf_counter() - t0))
    med = statistics.median(out)
    return dict(step=f"cpu_nn_lstm_fwd_bwd_B{B}_T{T}", B=B, T=T, fwd_bwd_ms=med, us_per_step=1e3 * med / T, threads=torch.get_num_threads())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eda_train_bench.json"))
    a = ap.parse_args()
    if a.step:
        gpu_step(a.step)
        return
    results = []
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(f"{name}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            results.append(dict(step=name, failed=r.returncode))
            break                                  # nothing more is started on the GPU after a failed step
        results.append(json.loads(lines[-1][7:]))
        print(lines[-1], flush=True)
    for B, T in SHAPES.values():
        results.append(cpu_lstm(B, T))
        print("RESULT " + json.dumps(results[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    if any("failed" in r for r in results):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
