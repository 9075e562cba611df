"""Many frames per slot and step: LsMultiStreamSession.step_frames (max_frames = m, n frames pushed per slot and step) against
the per-frame session (step, one replay per frame; max_frames = 1, the default path), in the same run, alternating.  Bench LS
config (tools/ls_multistream_bench.py LS_CFG: 4 + 2 layers, FFN 2048), max_nspks C = 10; every session is first pushed past
the look-ahead, so every timed frame steps encoder and decoder.  LS state is O(1) per stream, so the stream position does
not matter.  Rates are stream-frames per second (slots x frames per step / step time), median of the rounds.  Prints one
JSON line.

    python tools/ls_multistream_frames_bench.py [--slots 1,8,64] [--frames 4,8,16] [--fewer 16:4]

--frames n runs max_frames = n with n frames pushed; --fewer m:n runs max_frames = m with n frames pushed.  Kernel times come
from a separate `rocprofv3 --kernel-trace --stats` run of one configuration (e.g. --slots 64 --frames 8 --fewer ""
--no-baseline); `--stats <kernel_stats.csv>` with the same arguments then turns the chunk retention kernel's total time into
achieved state bytes per second (each step reads and writes every advanced sequence's state once) and lists the f32 linears'
share of the kernel time."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.ls_multistream_bench import C, HBM_BPS, LS_CFG, state_bytes  # noqa: E402

F32_LINEARS = ("ret_proj_step_kernel", "linear_f32_mfma_kernel", "skinny_")          # kernel names of the f32 linears


def configs(args):
    out = [(n, n) for n in (int(v) for v in args.frames.split(",") if v)]
    out += [tuple(int(v) for v in p.split(":")) for p in args.fewer.split(",") if p]
    return out


def stats(args):
    rows = [r for r in csv.DictReader(open(args.stats))]
    ret = [r for r in rows if "ret_chunk_ragged_kernel" in r["Name"]]
    S = int(args.slots.split(",")[0])
    m, n = configs(args)[0]
    ns = sum(float(r["TotalDurationNs"]) for r in ret)
    steps = -(-LS_CFG["conv_delay"] // n) + args.warmup + args.steps * args.rounds      # steps that move state
    byts = state_bytes(S, steps, steps)                                              # once per step, whatever n
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    lin = sum(float(r["TotalDurationNs"]) for r in rows if any(k in r["Name"] for k in F32_LINEARS))
    top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:12]
    print(json.dumps(dict(tool="ls_multistream_frames_bench --stats", slots=S, max_frames=m, frames=n, steps=steps,
                          state_bytes=byts, state_bytes_per_step=state_bytes(S, 1, 1), ret_chunk_kernel_ms=ns / 1e6,
                          ret_chunk_us_per_step=ns / 1e3 / steps, state_bytes_per_s=byts / (ns * 1e-9) if ns else None,
                          share_of_6p3_TBps=byts / (ns * 1e-9) / HBM_BPS if ns else None, all_kernels_ms=total / 1e6,
                          f32_linears_share=lin / total if total else None,
                          top_kernels=[dict(name=r["Name"][:80], calls=int(r["Calls"]), total_ms=float(r["TotalDurationNs"]) / 1e6)
                                       for r in top],
                          note="kernel time of every chunk retention call of the run, the capture warm-up's (no state "
                               "traffic) included; the first steps (look-ahead fill) move the encoder state only")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,8,64")
    ap.add_argument("--frames", default="4,8,16")
    ap.add_argument("--fewer", default="16:4")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a --no-baseline run: achieved state bytes/s")
    args = ap.parse_args()
    if args.stats:
        return stats(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ls_multistream_frames_bench needs a GPU")
    from fs_eend_amd.ls_model import OnlineConformerRetentionDADiarization
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = OnlineConformerRetentionDADiarization(n_speakers=None, in_size=345, **LS_CFG).eval().to(dev)
    slots = [int(s) for s in args.slots.split(",")]
    K, W, Rn = args.steps, args.warmup, args.rounds
    fill = LS_CFG["conv_delay"]
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(max(slots), 64, 345, generator=g) * 2 - 3).to(dev)
    results = []
    for S in slots:
        for m, n in configs(args):
            forms, per, ses = [], None, None
            if not args.no_baseline:
                per = LsMultiStreamSession(model, S, C)
                for _ in range(S):
                    per.open()

                def run_per(k, per=per):
                    for i in range(k * n):
                        per.step(push={s: x[s, i % 64] for s in range(S)})
                forms.append(("per_frame", run_per, -(-fill // n)))
            ses = LsMultiStreamSession(model, S, C, max_frames=m)
            for _ in range(S):
                ses.open()

            def run_frames(k, ses=ses):
                for _ in range(k):
                    ses.step_frames(push={s: x[s, :n] for s in range(S)})
            forms.append(("frames", run_frames, -(-fill // n)))
            for _, fn, f in forms:
                fn(f + W)                                                    # past the look-ahead, then warm
            torch.cuda.synchronize()
            times = {name: [] for name, _, _ in forms}
            for _ in range(Rn):                                              # alternating, same run
                for name, fn, _ in forms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(K)
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / K)      # seconds per n stream-frames of every slot
            r = dict(slots=S, max_frames=m, frames=n)
            for name, ts in times.items():
                med = sorted(ts)[len(ts) // 2]
                r[f"{name}_ms_per_step"] = round(med * 1e3, 4)
                r[f"{name}_ms_per_step_all"] = [round(v * 1e3, 4) for v in ts]
                r[f"{name}_stream_frames_per_s"] = round(S * n / med, 1)
            if "per_frame" in times:
                r["speedup"] = round(r["frames_stream_frames_per_s"] / r["per_frame_stream_frames_per_s"], 3)
            results.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
            forms = per = ses = run_per = run_frames = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    print(json.dumps(dict(tool="ls_multistream_frames_bench", device=torch.cuda.get_device_name(0), config="bench LS_CFG, C=10",
                          steps=K, warmup=W, rounds=Rn, timing="host clock around K steps ending in a device synchronise; "
                          "median of the rounds", results=results)))


if __name__ == "__main__":
    main()
