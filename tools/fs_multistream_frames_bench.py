"""Many frames per slot and step: FsMultiStreamSession.step_frames (max_frames = m, n frames pushed per slot and step) against the
per-frame session (step, one replay per frame), in the same run, alternating.  Bench FS config (bench.py FS_CFG: 4 + 2 layers,
FFN 2048), max_nspks C = 6, every slot at stream position t (seek: the history counters move, the K/V caches keep what they
hold).  Rates are stream-frames per second (slots x frames per step / step time).  Prints one JSON line.

    python tools/fs_multistream_frames_bench.py [--slots 1,8,64] [--pos 500,5000] [--frames 1,4,8,16] [--fewer 16:4,16:8]

--frames n runs max_frames = n with n frames pushed (n = 1: the per-frame session alone); --fewer m:n runs max_frames = m with
n frames pushed.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of one configuration (e.g.
--slots 64 --pos 5000 --frames 8 --fewer "" --no-baseline); `--stats <kernel_stats.csv>` with the same arguments then turns the
chunk attention kernel's total time into achieved K/V bytes per second: each stream reads
(L_enc + C * L_dec) * 2 * t * 256 * 2 B of K/V per step, once for all its frames of the step."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.fs_multistream_bench import C, FS_CFG, HBM_BPS, cap_for  # noqa: E402


def kv_bytes(S, t, n, steps):
    """K/V bytes the chunk attention reads over `steps` steps of n frames from position t."""
    per_pos = lambda tt: (FS_CFG["enc_n_layers"] * tt + C * FS_CFG["dec_n_layers"] * max(0, tt - 9)) * 2 * 256 * 2
    return S * sum(per_pos(t + i * n) for i in range(steps))


def configs(args):
    out = [(n, n) for n in (int(v) for v in args.frames.split(",") if v)]
    out += [tuple(int(v) for v in p.split(":")) for p in args.fewer.split(",") if p]
    return out


def stats(args):
    rows = [r for r in csv.DictReader(open(args.stats))]
    main = [r for r in rows if "attn_chunk_ragged_kernel" in r["Name"]]
    merge = [r for r in rows if "attn_chunk_ragged_merge_kernel" in r["Name"]]
    S, t = int(args.slots.split(",")[0]), int(args.pos.split(",")[0])
    m, n = configs(args)[0]
    ns_main = sum(float(r["TotalDurationNs"]) for r in main)
    ns_merge = sum(float(r["TotalDurationNs"]) for r in merge)
    calls = sum(int(r["Calls"]) for r in main)
    steps = args.warmup + args.steps * args.rounds          # the steps that read K/V (the capture's warm-up runs with every count 0)
    byts = kv_bytes(S, t, n, steps)
    out = dict(tool="fs_multistream_frames_bench --stats", slots=S, pos=t, max_frames=m, frames=n, chunk_calls=calls, steps=steps,
               kv_bytes=byts, chunk_kernel_ms=ns_main / 1e6, merge_kernel_ms=ns_merge / 1e6,
               kv_bytes_per_s=byts / (ns_main * 1e-9), kv_bytes_per_s_with_merge=byts / ((ns_main + ns_merge) * 1e-9),
               share_of_6p3_TBps=byts / (ns_main * 1e-9) / HBM_BPS,
               note="kernel time of every chunk attention call of the run, the capture warm-up's (no K/V read) included")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,8,64")
    ap.add_argument("--pos", default="500,5000")
    ap.add_argument("--frames", default="1,4,8,16")
    ap.add_argument("--fewer", default="16:4,16:8")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a --no-baseline run: print achieved K/V bytes/s")
    args = ap.parse_args()
    if args.stats:
        return stats(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fs_multistream_frames_bench needs a GPU")
    from fs_eend_amd.fs_model import OnlineTransformerDADiarization
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    from fs_eend_amd.fs_stream import StreamingTransformerEDADiarization, copy_params_from_masked_to_streaming
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    fm = OnlineTransformerDADiarization(n_speakers=None, in_size=345, **FS_CFG).eval().to(dev)
    sm = StreamingTransformerEDADiarization(in_size=345, **FS_CFG).eval().to(dev)
    copy_params_from_masked_to_streaming(fm, sm)
    slots = [int(s) for s in args.slots.split(",")]
    positions = [int(p) for p in args.pos.split(",")]
    K, W, Rn = args.steps, args.warmup, args.rounds
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(max(slots), 16, 345, generator=g) * 2 - 3).to(dev)
    results = []
    for t in positions:
        for S in slots:
            for m, n in configs(args):
                cap = cap_for(t + n * (K + W) * (Rn + 1) + 16)
                forms, per, ses = [], None, None
                if not args.no_baseline:
                    per = FsMultiStreamSession(sm, S, C, cap=cap)
                    for _ in range(S):
                        per.seek(per.open(), t)

                    def run_per(k, per=per):
                        for i in range(k * n):
                            per.step(push={s: x[s, i % 16] for s in range(S)})
                    forms.append(("per_frame", run_per))
                if m > 1:
                    ses = FsMultiStreamSession(sm, S, C, cap=cap, max_frames=m)
                    for _ in range(S):
                        ses.seek(ses.open(), t)

                    def run_frames(k, ses=ses):
                        for _ in range(k):
                            ses.step_frames(push={s: x[s, :n] for s in range(S)})
                    forms.append(("frames", run_frames))
                if not forms:
                    continue
                for _, fn in forms:
                    fn(W)
                torch.cuda.synchronize()
                times = {name: [] for name, _ in forms}
                for _ in range(Rn):                                          # alternating, same run
                    for name, fn in forms:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn(K)
                        torch.cuda.synchronize()
                        times[name].append((time.perf_counter() - t0) / K)  # seconds per n stream-frames of every slot
                r = dict(slots=S, pos=t, max_frames=m, frames=n, cap=cap)
                for name, ts in times.items():
                    best = sorted(ts)[len(ts) // 2]
                    r[f"{name}_ms_per_step"] = round(best * 1e3, 4)
                    r[f"{name}_stream_frames_per_s"] = round(S * n / best, 1)
                if "per_frame" in times and "frames" in times:
                    r["speedup"] = round(r["frames_stream_frames_per_s"] / r["per_frame_stream_frames_per_s"], 3)
                results.append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
                forms = per = ses = run_per = run_frames = None               # release both sessions' caches
                torch.cuda.empty_cache()
    print(json.dumps(dict(tool="fs_multistream_frames_bench", C=C, steps=K, rounds=Rn, results=results)))


if __name__ == "__main__":
    main()
