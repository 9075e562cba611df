"""Time the collar DER scorer on one GPU.

    python tools/der_bench.py [--recordings 64] [--frames 360000] [--speakers 8] [--subsampling 10] [--iters 20]

Recordings of --frames label frames (one hour at 10 ms) with sparse activity of --speakers speakers.  Prints one JSON line with,
each as the median of --iters device-synchronised calls after warm-up:
    score_batch_ms      CollarDER.score_batch on tensors already on the GPU: packing, the launches, the copy of the results back
    packed_ms           collar_der_packed on a batch packed once: three launches
for the whole batch and for one recording, the bytes the pass reads, and cpu_grid_ms, the vectorised numpy restatement
(tests/der_ref.py grid) on one recording.  The first recording's counters are compared with the restatement before timing.

With --regions, on the batch: regions_none_ms (collar_der_regions_packed without a table: the marginal times alone),
regions_uem_ms (with --intervals scoring regions per recording, about half of each recording inside them), jer_assign_ms (the
Jaccard assignment on the batch's matrices) and raster_ms (the references rasterised from their segment tables); packed_ms_batch,
regions_none_ms and regions_uem_ms are taken in turn, one call of each per round, so that they see the same machine.
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


def timed_in_turn(fns, iters):
    """Medians of `iters` rounds in which every function runs once: a drift of the machine hits all alike."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t) * 1e3)
    return [statistics.median(o) for o in out], [max(o) - min(o) for o in out]


def regions(M, a, refs, hyps, ref0, res):
    dev = refs[0].device
    step = a.frames // a.intervals
    uems = [[(k * step + 7 * b, k * step + 7 * b + step // 2) for k in range(a.intervals)] for b in range(len(refs))]
    batch = M.pack(refs, hyps, a.subsampling)
    table = M.pack_uem(uems, dev)
    out3 = M.collar_der_packed(batch, a.collar, a.subsampling)
    out5 = M.collar_der_regions_packed(batch, None, a.collar, a.subsampling)
    assert all(torch.equal(x, y) for x, y in zip(out3, out5[:3])), "the entry with regions, without a table, is not the old one"
    from tests import der_region_ref as Q
    got = M.collar_der_regions_packed(batch, table, a.collar, a.subsampling)
    small = slice(0, 3 * step)                                     # the restatement loops in Python: the first three regions
    want = Q.region(ref0[small], hyps[0].cpu().numpy()[:3 * step // a.subsampling], uems[0][:3], a.subsampling, a.collar)
    part = M.collar_der_regions_packed(M.pack([refs[0][small]], [hyps[0][:3 * step // a.subsampling]], a.subsampling),
                                       M.pack_uem([uems[0][:3]], dev), a.collar, a.subsampling)
    assert part[0][0].cpu().tolist() == want["counters"] and part[3][0].cpu().tolist() == want["ref_time"]
    (old, none, uem), spread = timed_in_turn([lambda: M.collar_der_packed(batch, a.collar, a.subsampling, out=out3),
                                              lambda: M.collar_der_regions_packed(batch, None, a.collar, a.subsampling, out=out5),
                                              lambda: M.collar_der_regions_packed(batch, table, a.collar, a.subsampling, out=got)],
                                             a.iters)
    res.update(intervals=a.intervals, packed_in_turn_ms=round(old, 4), regions_none_ms=round(none, 4), regions_uem_ms=round(uem, 4),
               in_turn_spread_ms=[round(s, 4) for s in spread], frames_kept_share=round(got[0][:, 5].sum().item() / (len(refs) * a.frames), 4))
    jer = M.jer_assign(got[1], got[3], got[4], a.speakers, a.speakers)
    res["jer_assign_ms"] = round(timed(lambda: M.jer_assign(got[1], got[3], got[4], a.speakers, a.speakers, out=jer), a.iters), 4)
    segs = []
    for r in (ref0, np.roll(ref0, 977, axis=0)):
        edges = np.diff(np.concatenate([np.zeros((1, r.shape[1]), np.int8), r.astype(np.int8), np.zeros((1, r.shape[1]), np.int8)]), axis=0)
        segs.append([(c, int(s), int(e)) for c in range(r.shape[1])
                     for s, e in zip(np.flatnonzero(edges[:, c] == 1), np.flatnonzero(edges[:, c] == -1))])
    tables = [segs[b % 2] for b in range(len(refs))]
    rows, _ = M.segments_raster(tables[:1], [a.frames], a.speakers)
    assert torch.equal(rows, refs[0]), "the rasteriser does not give back the reference"
    res["raster_ms"] = round(timed(lambda: M.segments_raster(tables, [a.frames] * len(refs), a.speakers), a.iters), 4)
    res["raster_segments"] = sum(len(t) for t in tables)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--frames", type=int, default=360000)
    ap.add_argument("--speakers", type=int, default=8)
    ap.add_argument("--subsampling", type=int, default=10)
    ap.add_argument("--collar", type=int, default=50)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--regions", action="store_true", help="also time the entry with scoring regions, the JER kernel and the rasteriser")
    ap.add_argument("--intervals", type=int, default=100, help="scoring regions per recording with --regions")
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
    if a.regions:
        regions(M, a, refs, hyps, ref0, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
