"""Time the collar DER scorer on one GPU.

    python tools/der_bench.py [--recordings 64] [--frames 360000] [--speakers 8] [--subsampling 10] [--iters 20]

Recordings of --frames label frames (one hour at 10 ms) with sparse activity of --speakers speakers.  Prints one JSON line with,
each as the median of --iters device-synchronised calls after warm-up:
    score_batch_ms      CollarDER.score_batch on tensors already on the GPU: packing, the launches, the copy of the results back
    packed_ms           collar_der_packed on a batch packed once: three launches
for the whole batch and for one recording, the bytes the pass reads, and cpu_grid_ms, the vectorised numpy restatement
(tests/der_ref.py grid) on one recording.  The first recording's counters are compared with the restatement before timing.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np
import torch

from tests import der_ref as R


def recording(seed, T, C, sub):
    rng = np.random.default_rng(seed)
    ref = np.stack([R.run_track(rng, T, 600, 9000) for _ in range(C)], axis=1)
    hyp = np.stack([R.run_track(rng, T // sub, 60, 900) for _ in range(C)], axis=1)
    hyp[:, :C - 2] |= np.roll(ref[::sub][:T // sub], 2, axis=1)[:, :C - 2]
    return ref, hyp


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--frames", type=int, default=360000)
    ap.add_argument("--speakers", type=int, default=8)
    ap.add_argument("--subsampling", type=int, default=10)
    ap.add_argument("--collar", type=int, default=50)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "der_bench needs a GPU"
    import __graft_entry__ as G
    G.build()
    from fs_eend_amd import metrics as M
    dev = torch.device("cuda:0")
    ref0, hyp0 = recording(1, a.frames, a.speakers, a.subsampling)
    t = time.perf_counter()
    want = R.grid(ref0, hyp0, a.subsampling, a.collar)
    cpu_ms = (time.perf_counter() - t) * 1e3
    r0, h0 = torch.from_numpy(ref0).to(dev), torch.from_numpy(hyp0).to(dev)
    refs = [r0] + [r0.roll(977 * b, 0).roll(b, 1) for b in range(1, a.recordings)]
    hyps = [h0] + [h0.roll(89 * b, 0) for b in range(1, a.recordings)]
    got = M.collar_der_counters(refs, hyps, a.collar, a.subsampling)[0].cpu().tolist()
    assert got[0] == want["counters"], (got[0], want["counters"])
    res = dict(recordings=a.recordings, frames=a.frames, speakers=a.speakers, subsampling=a.subsampling, collar=a.collar,
               cpu_grid_ms=round(cpu_ms, 3), device=torch.cuda.get_device_name(0))
    for name, rs, hs in (("batch", refs, hyps), ("one", refs[:1], hyps[:1])):
        metric = M.CollarDER(a.collar, a.subsampling)
        batch = M.pack(rs, hs, a.subsampling)
        out = M.collar_der_packed(batch, a.collar, a.subsampling)
        res[f"score_batch_ms_{name}"] = round(timed(lambda: metric.score_batch(rs, hs), a.iters), 4)
        res[f"packed_ms_{name}"] = round(timed(lambda: M.collar_der_packed(batch, a.collar, a.subsampling, out=out), a.iters), 4)
        res[f"bytes_read_{name}"] = int(batch[0].numel() + batch[2].numel())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
