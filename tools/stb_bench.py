"""Steady-state throughput of block-online EEND-EDA with a speaker-tracing buffer (fs_eend_amd.stb.StbSession) at 1 / 16 / 64
streams, blk 100 / buf 1000 (conf/spk_STB.yaml: four encoder layers), with the share of every stage of a step, next to what a user
can write without the session on the same box: a per-stream loop over `model.test` with the tracking in torch and scipy (the
reference's loop: a host read of the count and a linear_sum_assignment on the CPU per block).  Not bench.py: nothing here is a
pass/fail figure.

    python tools/stb_bench.py [--out profiles/stb_bench.json]

Steady state: every stream's buffer is full (11 warm-up blocks), so a step is one group of T = 1100 rows per stream.  The parent
process never opens the GPU: every configuration is a child process of its own under `timeout`, run one after the other, and the
first one that fails ends the run.  Step times are medians over repeats between two events on the stream; the stage split comes
from events around the stage calls of a step, in a run of its own (the events themselves cost a little).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

STREAMS = [1, 16, 64]
STEPS = [(f"session_{b}", 300) for b in STREAMS] + [(f"loop_{b}", 420) for b in STREAMS]
N_LAYERS, IN_SIZE, H, BLK, BUF, TH = 4, 345, 256, 100, 1000, 0.5
WARM_BLOCKS, REPS = BUF // BLK + 1, 7


def _model(dev):
    import torch
    from fs_eend_amd.eda_model import TransformerEDADiarization
    torch.manual_seed(0)
    m = TransformerEDADiarization(n_speakers=None, in_size=IN_SIZE, n_units=H, n_heads=4, n_layers=N_LAYERS, dropout=0.1).eval()
    with torch.no_grad():
        m.eda.counter.weight.mul_(16.0)          # spreads the 15 existence probabilities, so that counts other than 0 and 15 occur
    return m.to(dev)


def _blocks(B, n, dev, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, IN_SIZE, generator=g) * 2 - 3).to(dev) for _ in range(B)]


def session_step(B):
    import torch
    from fs_eend_amd import ops
    from fs_eend_amd.stb import StbSession
    dev = torch.device("cuda:0")
    m = _model(dev)
    sess = StbSession(m, B, buf_size=BUF, blk_size=BLK, th=TH, policy="kld", seed=0)
    slots = [sess.open() for _ in range(B)]
    feed = [_blocks(B, BLK, dev, 100 + i) for i in range(4)]
    for i in range(WARM_BLOCKS + 2):
        sess.step(dict(zip(slots, feed[i % 4])))
    torch.cuda.synchronize()
    assert all(l == BUF for l in sess.L)
    times = []
    for i in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sess.step(dict(zip(slots, feed[i % 4])))
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    med = statistics.median(times)
    res = dict(step=f"session_{B}", streams=B, T=BUF + BLK, device=torch.cuda.get_device_name(0), ms=med, ms_min=min(times),
               ms_max=max(times), stream_blocks_per_s=1e3 * B / med, n_layers=N_LAYERS)
    # the split: events around the stage calls of one step
    marks = []

    def timed(mod, name, label):
        fn = getattr(mod, name)

        def wrapper(*args, **kw):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn(*args, **kw)
            b.record()
            marks.append((label, a, b))
            return out
        setattr(mod, name, wrapper)
        return fn

    saved = [(ops, n, timed(ops, n, l)) for n, l in (("stb_center", "center"), ("lstm_train", "lstm"), ("stb_track", "track"),
                                                     ("eda_head", "head"), ("eda_count", "count"), ("linear_step_f32", "lstm_input_gemm"))]
    saved.append((m, "_encode", timed(m, "_encode", "encoder")))
    split = {}
    for i in range(3):
        marks.clear()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sess.step(dict(zip(slots, feed[i % 4])))
        b.record()
        b.synchronize()
        total = a.elapsed_time(b)
        once = {}
        for label, x, y in marks:                  # a stage called twice in a step (the two recurrences) counts as their sum
            once[label] = once.get(label, 0.0) + x.elapsed_time(y)
        for label, v in once.items():
            split.setdefault(label, []).append(v)
        split.setdefault("step", []).append(total)
    for mod, n, fn in saved:
        setattr(mod, n, fn)
    per = {k: statistics.median(v) for k, v in split.items()}
    res["split_ms"] = per
    res["stb_kernels_share"] = (per["center"] + per["track"]) / per["step"]
    print("RESULT " + json.dumps(res), flush=True)


def loop_step(B):
    """What a user can write at the offline model alone: per stream and block, centre in torch, model.test (which reads the count
    back), sigmoid, correlations in torch, linear_sum_assignment on the host, torch.multinomial for the buffer draw."""
    import numpy as np
    import torch
    from scipy.optimize import linear_sum_assignment
    dev = torch.device("cuda:0")
    m = _model(dev)
    feed = [_blocks(B, BLK, dev, 100 + i) for i in range(4)]
    state = [None] * B

    def block(s, x_i):
        if state[s] is None:
            xc = x_i - x_i.mean(dim=0, keepdim=True)
            y = torch.sigmoid(m.test([xc], [xc.shape[0]], th=TH)[0][0])
            state[s] = (xc, y)
            return y
        x_buf, y_buf = state[s]
        x_cat = torch.cat([x_buf, x_i], dim=0)
        xc = x_cat - x_cat.mean(dim=0, keepdim=True)
        L = x_buf.shape[0]
        p = torch.sigmoid(m.test([xc], [xc.shape[0]], th=TH)[0][0])
        Sn = max(y_buf.shape[1], p.shape[1])
        z_buf = torch.nn.functional.pad(y_buf, (0, Sn - y_buf.shape[1]))
        p = torch.nn.functional.pad(p, (0, Sn - p.shape[1]))
        if Sn:
            a = z_buf - z_buf.mean(dim=0, keepdim=True)
            e = p[:L] - p[:L].mean(dim=0, keepdim=True)
            corr = (a.T @ e) / (a.norm(dim=0)[:, None] * e.norm(dim=0)[None, :] + 1e-6)
            perm = linear_sum_assignment(corr.cpu().numpy(), True)[1]
            y_i = p[L:, torch.as_tensor(perm, device=dev)]
        else:
            y_i = p[L:]
        y_cat = torch.cat([z_buf, y_i], dim=0)
        if x_cat.shape[0] > BUF:
            if Sn:
                tot = y_cat.sum(dim=1, keepdim=True)
                # rows buffered while no speaker was tracked are all zero: 0 / 0 there (the reference's NaN) would reach
                # torch.multinomial, whose device-side check of its weights traps the queue
                q = torch.where(tot > 0, y_cat / tot.clamp_min(1e-30), torch.zeros_like(y_cat))
                q = q.masked_fill(q == 0, 1e-6)
                w = (q * torch.log(q * Sn)).sum(dim=1).clamp_min(0)
                w = w.masked_fill(w == 0, 1e-6)
            else:
                w = torch.ones(x_cat.shape[0], device=dev)
            if not bool(torch.isfinite(w).all() and (w > 0).all()):      # a host check first: never hand multinomial bad weights
                raise RuntimeError("baseline loop: selection weights are not finite and positive")
            sel = torch.multinomial(w, BUF, replacement=False).sort().values
            x_cat, y_cat = x_cat[sel], y_cat[sel]
        state[s] = (x_cat, y_cat)
        return y_i

    np.random.seed(0)
    for i in range(WARM_BLOCKS + 1):
        for s in range(B):
            block(s, feed[i % 4][s])
    torch.cuda.synchronize()
    times = []
    for i in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for s in range(B):
            block(s, feed[i % 4][s])
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    med = statistics.median(times)
    print("RESULT " + json.dumps(dict(step=f"loop_{B}", streams=B, T=BUF + BLK, device=torch.cuda.get_device_name(0), ms=med,
                                      ms_min=min(times), ms_max=max(times), stream_blocks_per_s=1e3 * B / med, n_layers=N_LAYERS)),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stb_bench.json"))
    a = ap.parse_args()
    if a.step:
        kind, b = a.step.split("_")
        (session_step if kind == "session" else loop_step)(int(b))
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
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    if any("failed" in r for r in results):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
