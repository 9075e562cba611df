"""Time one call of the device room impulse response generator (fs_eend_amd/rooms.py) against the float64 numpy restatement of
its contract (tests/room_ref.py) on the same box.

    python tools/room_bench.py [--rooms 256] [--sources 4] [--taps 4000] [--seed 1] [--rounds 5] [--iters 5] [--warmup 2]
                               [--host-rows 4] [--stats kernel_stats.csv] [--out profiles/room_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o room --output-format csv -- python tools/room_bench.py --worker 5

The case: rooms x sources responses (1024) of `taps` taps each, the rooms from rooms.draw_rooms at its defaults, one
room_responses call: one descriptor copy and one launch.  Each round is the median of --iters calls that end in a device
synchronise, after --warmup calls; the result is the median of the rounds.  `image_taps` counts the (image, tap) pairs the
contract sums (every image whose window meets [0, K), times its taps inside [0, K)), computed on the host from the
restatement's image list; `candidate_tile_visits` the (image, tile) pairs the kernel walks, 64 lane-taps each.  The host form
is the restatement on --host-rows evenly spaced rows, scaled by their share of image_taps.  --worker N runs warm-up and N
calls only, for a kernel trace in a run of its own; --stats merges the kernel's row of that run's kernel_stats.csv.  Writes one
JSON object to --out and prints it on one line."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=256)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--taps", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-rows", type=int, default=4, help="rows the float64 restatement runs (its time is scaled to all of them)")
    ap.add_argument("--worker", type=int, default=0, help="warm up, run this many calls and exit (for a kernel trace)")
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a --worker run: merge the kernel's row")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "room_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import room_ref as R
    assert torch.cuda.is_available(), "room_bench needs a GPU"
    from fs_eend_amd import rooms as RM
    dev = torch.device("cuda:0")
    rows, _ = RM.draw_rooms(a.seed, a.rooms, a.sources)
    K, T = a.taps, RM.limits()["tile"]

    def device():
        return RM.room_responses(rows, K, device=dev, normalize="direct")

    for _ in range(a.warmup):
        device()
    torch.cuda.synchronize()
    if a.worker:
        for _ in range(a.worker):
            device()
            torch.cuda.synchronize()
        return
    rounds = []
    for _ in range(a.rounds):
        ms = []
        for _ in range(a.iters):
            t = time.perf_counter()
            device()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) * 1e3)
        rounds.append(round(statistics.median(ms), 4))
    med = statistics.median(rounds)
    t = time.perf_counter()
    p = RM.plan_rooms(rows, K, normalize="direct")
    plan_ms = (time.perf_counter() - t) * 1e3

    # the work of the call, from the restatement's image lists
    pairs, visits, images = np.zeros(len(rows)), 0, 0
    for i, r in enumerate(rows):
        kc, f, _ = R.row_images(r["size"], r["source"], r["receiver"], r["beta"], r["c"], 1.0, K)
        lo, hi = np.maximum(kc + np.where(f < 0, -32, -31), 0), np.minimum(kc + np.where(f > 0, 32, 31), K - 1)
        pairs[i] = float((hi - lo + 1).sum())
        visits += int((hi // T - lo // T + 1).sum())
        images += len(kc)
    picked = sorted(set(np.linspace(0, len(rows) - 1, max(a.host_rows, 1)).astype(int).tolist()))
    got = device().samples.cpu().numpy().reshape(len(rows), K)
    t = time.perf_counter()
    worst = 0.0
    for i in picked:
        r = rows[i]
        p0 = np.subtract(r["source"], r["receiver"])
        g = float(np.sqrt(p0[0] * p0[0] + (p0[1] * p0[1] + p0[2] * p0[2])))
        ref, n, S = R.response(r["size"], r["source"], r["receiver"], r["beta"], r["c"], g, K)
        bound = (n + 16) * 2.0 ** -24 * S
        nz = bound > 0
        worst = max(worst, float((np.abs(got[i] - ref)[nz] / bound[nz]).max()))
    host_ms = (time.perf_counter() - t) * 1e3 * float(pairs.sum()) / float(pairs[picked].sum())
    out = {"tool": "room_bench", "responses": len(rows), "taps": K, "seed": a.seed, "tiles": int(len(p["tiles"])), "images": images,
           "image_taps": float(pairs.sum()), "candidate_tile_visits": visits, "round_medians_ms": rounds, "device_ms": round(med, 4),
           "plan_rooms_host_ms": round(plan_ms, 2), "responses_per_s": round(len(rows) / (med * 1e-3), 1),
           "image_taps_per_s": float(f"{pairs.sum() / (med * 1e-3):.4g}"), "lane_taps_per_s": float(f"{visits * 64 / (med * 1e-3):.4g}"),
           "host_rows_timed": len(picked), "host_float64_ms_scaled": round(host_ms, 1), "host_over_device": round(host_ms / med, 1),
           "worst_fraction_of_bound_on_host_rows": float(f"{worst:.4g}"),
           "timing": "host clock around one room_responses() call that ends in a device synchronise; per round the median of iters calls"}
    if a.stats:
        for r in csv.DictReader(open(a.stats)):
            if "room_rir" in r["Name"]:
                out["kernel_trace"] = {"name": r["Name"], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 1),
                                       "min_us": round(float(r["MinNs"]) / 1e3, 1), "max_us": round(float(r["MaxNs"]) / 1e3, 1),
                                       "source": "rocprofv3 --kernel-trace --stats, a run of its own (--worker)"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
