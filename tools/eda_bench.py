"""Times of offline EEND-EDA inference (fs_eend_amd.eda_model) and of the LSTM recurrence alone (eend_lstm_f32), next to torch's
CPU nn.LSTM for the same shapes on the same box.  Not bench.py: nothing here is a pass/fail figure.

    python tools/eda_bench.py [--out profiles/eda_bench.json]

Shapes: B = 1, T = 5000 (the shipped inference config: one whole recording) and B = 64, T = 500.  The parent process never opens the
GPU: every GPU step is a child process of its own under `timeout`, run one after the other, and the first one that fails ends the
run.  Device times are medians over repeats between two events on the stream, after warm-up calls.
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
STEPS = [("lstm_b1", 120), ("lstm_b64", 120), ("test_b1", 240), ("test_b64", 240)]
N_LAYERS, IN_SIZE, H = 4, 345, 256


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
    from fs_eend_amd.eda_model import TransformerEDADiarization
    kind, shape = name.split("_")
    B, T = SHAPES[shape]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = TransformerEDADiarization(n_speakers=None, in_size=IN_SIZE, n_units=H, n_heads=4, n_layers=N_LAYERS, dropout=0.1).eval().to(dev)
    res = dict(step=name, B=B, T=T, device=torch.cuda.get_device_name(0))
    if kind == "lstm":
        P = m.eda._prepare()
        G = torch.randn(B, T, 4 * H, device=dev)
        order = torch.as_tensor(np.random.RandomState(0).permutation(T).astype(np.int32), device=dev)
        hT, cT = torch.empty(B, H, device=dev), torch.empty(B, H, device=dev)
        med, lo, hi = _median_ms(lambda: ops.lstm(G, order, None, P["enc_whh"], None, None, hT, cT, None, B, T), 2, 7)
        res.update(ms=med, ms_min=lo, ms_max=hi, us_per_step=1e3 * med / T)
        att = torch.empty(B, 15, H, device=dev)
        med, lo, hi = _median_ms(lambda: ops.lstm(None, None, P["dec_b"], P["dec_whh"], hT, cT, hT.clone(), cT.clone(), att, B, 15), 2, 7)
        res.update(decoder_ms=med, decoder_us_per_step=1e3 * med / 15)
    else:
        src = [torch.randn(T, IN_SIZE, device=dev) * 2 - 3 for _ in range(B)]
        order = np.random.RandomState(0).permutation(T)
        med, lo, hi = _median_ms(lambda: m.test(src, [T] * B, n_spk=4, order=order), 2, 5)
        res.update(ms=med, ms_min=lo, ms_max=hi, ms_per_frame=med / (B * T), n_layers=N_LAYERS)
    print("RESULT " + json.dumps(res), flush=True)


def cpu_lstm(B, T, reps=3, backward=False):
    """torch's CPU nn.LSTM on the same shape: the forward without grad mode, or (tools/eda_train_bench.py) forward + backward."""
    import torch
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(H, H, 1, batch_first=True)
    x = torch.randn(B, T, H, requires_grad=backward)
    R = torch.randn(B, T, H) if backward else None
    out = []
    for i in range(reps + 1):
        lstm.zero_grad()
        x.grad = None
        t0 = time.perf_counter()
        if backward:
            (lstm(x)[0] * R).sum().backward()
        else:
            with torch.no_grad():
                lstm(x)
        if i:                                      # the first call warms up
            out.append(1e3 * (time.perf_counter() - t0))
    med = statistics.median(out)
    res = dict(step=f"cpu_nn_lstm_fwd_bwd_B{B}_T{T}", fwd_bwd_ms=med) if backward else dict(step=f"cpu_nn_lstm_B{B}_T{T}", ms=med)
    return dict(res, B=B, T=T, us_per_step=1e3 * med / T, threads=torch.get_num_threads())


def main(script=__file__, steps=STEPS, gpu_step=gpu_step, cpu=cpu_lstm, out="eda_bench.json"):
    """--step NAME: that GPU step in this process; otherwise every step of `script` as a child process, then the CPU lines."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out))
    a = ap.parse_args()
    if a.step:
        gpu_step(a.step)
        return
    results = []
    for name, limit in steps:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(script), "--step", name],
                           capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(f"{name}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            results.append(dict(step=name, failed=r.returncode))
            break                                  # nothing more is started on the GPU after a failed step
        results.append(json.loads(lines[-1][7:]))
        print(lines[-1], flush=True)
    for B, T in SHAPES.values():
        results.append(cpu(B, T))
        print("RESULT " + json.dumps(results[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    if any("failed" in r for r in results):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
