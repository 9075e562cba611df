"""Many LS-EEND streams per frame step: one LsMultiStreamSession (S slots, one graph replay per frame) against S
LsStreamSession(batch=1) objects pushed one after another and against one lockstep LsStreamSession(batch=S) (the cost floor:
same rows, one shared stream position), in the same run, alternating.  LS yaml shapes (bench.py LS_CFG: 4 + 2 layers, FFN
2048), max_nspks C = 10; every form is first pushed past the look-ahead, so every timed frame steps encoder and decoder.  LS
state is O(1) per stream: the cost of a frame does not depend on the stream position.  Prints one JSON line.

    python tools/ls_multistream_bench.py [--slots 1,8,32,64] [--steps 20] [--warmup 3] [--rounds 3] [--no-baseline]

Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run (e.g. --slots 64 --no-baseline);
`--stats <kernel_stats.csv>` with the same --slots / --steps / --warmup / --rounds then turns the ragged retention kernel's
total time into achieved state bytes per second: each advanced row reads and writes H * 64 * 64 * 4 B per layer."""
import argparse
import csv
import json
import sys
import os
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LS_CFG = dict(n_units=256, n_heads=4, enc_n_layers=4, dec_n_layers=2, dropout=0.1, max_seqlen=1000,
              recurrent_chunk_size=500, feed_forward_expansion_factor=4, dec_dim_feedforward=2048,
              conv_expansion_factor=2, conv_kernel_size=16, half_step_residual=True, conv_delay=9)   # = bench.py LS_CFG
C = 10
HBM_BPS = 6.3e12                                                                 # MI355X, measured copy rate
ROW_BYTES = LS_CFG["n_heads"] * 64 * 64 * 4                                      # one row's retention state, one layer


def state_bytes(S, enc_frames, dec_frames):
    """Retention state bytes read + written by the ragged step over frames that advance the encoder / decoder of S slots."""
    return 2 * ROW_BYTES * S * (LS_CFG["enc_n_layers"] * enc_frames + C * LS_CFG["dec_n_layers"] * dec_frames)


def frames_of_run(args):
    """(encoder frames, decoder frames) of the multi-session's run: look-ahead fill + warm-up + timed rounds."""
    fill = LS_CFG["conv_delay"]
    n = fill + args.warmup + args.steps * args.rounds
    return n, n - fill


def stats(args):
    rows = [r for r in csv.DictReader(open(args.stats))]
    ret = [r for r in rows if "ret_step_ragged_kernel" in r["Name"]]
    S = int(args.slots.split(",")[0])
    ns = sum(float(r["TotalDurationNs"]) for r in ret)
    calls = sum(int(r["Calls"]) for r in ret)
    fe, fd = frames_of_run(args)
    byts = state_bytes(S, fe, fd)
    out = dict(tool="ls_multistream_bench --stats", slots=S, ret_calls=calls, enc_frames=fe, dec_frames=fd, state_bytes=byts,
               state_bytes_per_frame=state_bytes(S, 1, 1), ret_kernel_ms=ns / 1e6,
               ret_kernel_us_per_frame=ns / 1e3 / fe, state_bytes_per_s=byts / (ns * 1e-9),
               share_of_6p3_TBps=byts / (ns * 1e-9) / HBM_BPS,
               note="kernel time of every ragged retention call of the run; the capture warm-up's calls (all masks off, no "
                    "state traffic) are included")
    top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:12]
    out["top_kernels"] = [dict(name=r["Name"][:80], calls=int(r["Calls"]), total_ms=float(r["TotalDurationNs"]) / 1e6) for r in top]
    out["all_kernels_ms"] = sum(float(r["TotalDurationNs"]) for r in rows) / 1e6
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,8,32,64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true", help="time the multi-stream session only")
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a --no-baseline run: print achieved state bytes/s")
    args = ap.parse_args()
    if args.stats:
        return stats(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ls_multistream_bench needs a GPU")
    from fs_eend_amd.ls_model import OnlineConformerRetentionDADiarization
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    from fs_eend_amd.ls_stream import LsStreamSession
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = OnlineConformerRetentionDADiarization(n_speakers=None, in_size=345, **LS_CFG).eval().to(dev)
    slots = [int(s) for s in args.slots.split(",")]
    K, W = args.steps, args.warmup
    fill = LS_CFG["conv_delay"]
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(max(slots), K + W + fill, 345, generator=g) * 2 - 3).to(dev)
    results = []
    for S in slots:
        ses = LsMultiStreamSession(m, S, C)
        for _ in range(S):
            ses.open()
        # LsStreamSession's graphs point into frame-step scratch cached on the model, which a session with more rows than any
        # before it re-allocates: the lockstep session (the most rows) first, then the single-stream ones, all new per S
        lock = None if args.no_baseline else LsStreamSession(m, C, batch=S)
        base = [] if args.no_baseline else [LsStreamSession(m, C, batch=1) for _ in range(S)]
        T = K + W + fill

        def run_multi(n):
            for i in range(n):
                ses.step(push={s: x[s, i % T] for s in range(S)})

        def run_seq(n):
            for i in range(n):
                for s in range(S):
                    base[s].push(x[s, i % T])

        def run_lock(n):
            for i in range(n):
                lock.push(x[:S, i % T])

        forms = [("multi", run_multi)] + ([] if args.no_baseline else [("sequential", run_seq), ("lockstep", run_lock)])
        for _, fn in forms:
            fn(fill + W)                                                     # past the look-ahead, then warm
        torch.cuda.synchronize()
        times = {name: [] for name, _ in forms}
        for _ in range(args.rounds):                                         # alternating, same run
            for name, fn in forms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(K)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / K)
        r = dict(slots=S)
        for name, ts in times.items():
            best = min(ts)
            r[f"{name}_ms_per_step"] = best * 1e3
            r[f"{name}_ms_per_step_all"] = [round(v * 1e3, 4) for v in ts]
            r[f"{name}_stream_frames_per_s"] = S / best
        if not args.no_baseline:
            r["speedup_vs_sequential"] = r["multi_stream_frames_per_s"] / r["sequential_stream_frames_per_s"]
            r["ms_ratio_to_lockstep"] = r["multi_ms_per_step"] / r["lockstep_ms_per_step"]
        r["state_bytes_per_step"] = state_bytes(S, 1, 1)
        r["state_bound_ms_at_6p3_TBps"] = r["state_bytes_per_step"] / HBM_BPS * 1e3
        results.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        del ses, lock, base
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    print(json.dumps(dict(tool="ls_multistream_bench", device=torch.cuda.get_device_name(0), config="bench LS_CFG, C=10",
                          steps=K, warmup=W, rounds=args.rounds, timing="host clock around K steps ending in a device synchronise; "
                          "best of the rounds", results=results)))


if __name__ == "__main__":
    main()
