"""Time the collar DER sweep against the host loop it replaces, on one GPU.

    python tools/sweep_bench.py [--recordings 64] [--frames 360000] [--speakers 8] [--subsampling 10] [--iters 20]

Recordings of --frames label frames (one hour at 10 ms) with sparse activity of --speakers speakers, posteriors at the model rate
made of the hypothesis tracks plus a per-frame offset plus noise (tests/sweep_ref.py).  For the grid of 5 thresholds x 2 medians
and for the 32-point limit (16 x 2), each as the median of --iters device-synchronised calls after warm-up, the two taken in
turn in one process:
    sweep_ms            collar_der_sweep_packed on batches packed once, grids on the device, outputs given: three launches
    loop_ms             the loop it replaces, from functions that were there before the sweep: per point, postproc.activity per
                        recording, metrics.pack, metrics.collar_der_packed
with the smallest and largest sample of each (the run-to-run spread the gap has to exceed), and
    sweep_g1_ms / packed_ms   the sweep at one point next to collar_der_packed alone on that point's uint8 batch: what the float
                              staging costs
    bytes_read, sweep_gbps    the bytes one pass reads (reference rows + posterior rows) and that over sweep_ms
Before timing, every point's counters and co-occurrence counts from the sweep are compared with the loop's, exactly.
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
from tests import sweep_ref as W


def recording(seed, T, C, sub):
    rng = np.random.default_rng(seed)
    ref = np.stack([R.run_track(rng, T, 600, 9000) for _ in range(C)], axis=1)
    hyp = np.stack([R.run_track(rng, T // sub, 60, 900) for _ in range(C)], axis=1)
    hyp[:, :C - 2] |= np.roll(ref[::sub][:T // sub], 2, axis=1)[:, :C - 2]
    return ref, W.posteriors(rng, hyp)


def timed_in_turn(fns, iters):
    """-> per function (median, min, max) ms of `iters` device-synchronised calls, the functions taken in turn."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(iters):
        for samples, fn in zip(out, fns):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            samples.append((time.perf_counter() - t) * 1e3)
    return [(round(statistics.median(s), 4), round(min(s), 4), round(max(s), 4)) for s in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--frames", type=int, default=360000)
    ap.add_argument("--speakers", type=int, default=8)
    ap.add_argument("--subsampling", type=int, default=10)
    ap.add_argument("--collar", type=int, default=50)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sweep_bench needs a GPU"
    import __graft_entry__ as G
    G.build()
    from fs_eend_amd import metrics as M
    from fs_eend_amd import postproc
    dev = torch.device("cuda:0")
    ref0, pred0 = recording(1, a.frames, a.speakers, a.subsampling)
    r0, p0 = torch.from_numpy(ref0).to(dev), torch.from_numpy(pred0).to(dev)
    refs = [r0] + [r0.roll(977 * b, 0).roll(b, 1) for b in range(1, a.recordings)]
    preds = [p0] + [p0.roll(89 * b, 0) for b in range(1, a.recordings)]
    ref_batch, pred_batch = M.pack_references(refs), M.pack_predictions(preds)
    bytes_read = int(ref_batch[0].numel() + 4 * pred_batch[0].numel())
    res = dict(recordings=a.recordings, frames=a.frames, speakers=a.speakers, subsampling=a.subsampling, collar=a.collar, iters=a.iters,
               bytes_read=bytes_read, device=torch.cuda.get_device_name(0))

    def loop(ths, meds):
        out = []
        for th in ths:
            for k in meds:
                hyps = [postproc.activity(p, th, k) for p in preds]
                out.append(M.collar_der_packed(M.pack(refs, hyps, a.subsampling), a.collar, a.subsampling))
        return out

    grids = {"g10": ([0.3, 0.4, 0.5, 0.6, 0.7], [1, 11]), "g32": ([round(0.2 + 0.04 * i, 2) for i in range(16)], [1, 11])}
    for name, (ths, meds) in grids.items():
        th_dev, med_dev = torch.tensor(ths, dtype=torch.float32, device=dev), torch.tensor(meds, dtype=torch.int32, device=dev)
        out = M.collar_der_sweep_packed(ref_batch, pred_batch, th_dev, med_dev, a.collar, a.subsampling)
        want = loop(ths, meds)
        for g, w in enumerate(want):
            assert torch.equal(out[0][g], w[0]) and torch.equal(out[1][g], w[1]), f"{name}: point {g} differs from the loop"
        if name == "g10":
            c = R.grid(ref0, W.activity(pred0, 0.5, 11), a.subsampling, a.collar)["counters"]
            assert out[0][5, 0].cpu().tolist() == c, (out[0][5, 0].cpu().tolist(), c)
            res["rates_g10"] = [round(M.rate(int(s[0]), int(s[1] + s[2] + s[3])), 5) for s in out[0].sum(dim=1).cpu()]
        sweep, looped = timed_in_turn([lambda: M.collar_der_sweep_packed(ref_batch, pred_batch, th_dev, med_dev, a.collar, a.subsampling, out=out),
                                       lambda: loop(ths, meds)], a.iters)
        res[f"sweep_ms_{name}"], res[f"sweep_min_max_{name}"] = sweep[0], sweep[1:]
        res[f"loop_ms_{name}"], res[f"loop_min_max_{name}"] = looped[0], looped[1:]
        res[f"sweep_gbps_{name}"] = round(bytes_read / sweep[0] / 1e6, 1)
    th_dev, med_dev = torch.tensor([0.5], dtype=torch.float32, device=dev), torch.tensor([11], dtype=torch.int32, device=dev)
    out1 = M.collar_der_sweep_packed(ref_batch, pred_batch, th_dev, med_dev, a.collar, a.subsampling)
    batch = M.pack(refs, [postproc.activity(p, 0.5, 11) for p in preds], a.subsampling)
    outp = M.collar_der_packed(batch, a.collar, a.subsampling)
    assert torch.equal(out1[0][0], outp[0]) and torch.equal(out1[1][0], outp[1])
    one, packed = timed_in_turn([lambda: M.collar_der_sweep_packed(ref_batch, pred_batch, th_dev, med_dev, a.collar, a.subsampling, out=out1),
                                 lambda: M.collar_der_packed(batch, a.collar, a.subsampling, out=outp)], a.iters)
    res["sweep_g1_ms"], res["sweep_g1_min_max"], res["packed_ms"], res["packed_min_max"] = one[0], one[1:], packed[0], packed[1:]
    res["packed_bytes_read"] = int(batch[0].numel() + batch[2].numel())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
