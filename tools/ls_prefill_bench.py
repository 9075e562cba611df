"""Prefill of an LS-EEND stream slot from a backlog: LsMultiStreamSession.prefill against the same frames through step_frames
at max_frames = 64, in the same run, alternating.  Bench LS config (tools/ls_multistream_bench.py LS_CFG: 4 + 2 layers, FFN
2048), max_nspks C = 10; one slot of a session of S slots is brought forward by T frames (LS state is O(1): the stream goes on
from wherever the last round left it, the position does not change the cost).  Prints one JSON line.

    python tools/ls_prefill_bench.py [--slots 1,64] [--frames 5000] [--rounds 3] [--kernel 1:1024,10:1024]

--kernel Nseq:T,... times the retention prefill alone (device time, three launches) against ops.retention_chunk_ragged chained
at nmax = 64 over the same frames, alternating in the same run.  --no-backlog skips the session part."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.ls_multistream_bench import C, LS_CFG  # noqa: E402

H, D = 4, 256


def median(ts):
    return sorted(ts)[len(ts) // 2]


def kernel_bench(torch, dev, spec, reps, t0=1000):
    from fs_eend_amd import ops
    Nseq, T = (int(v) for v in spec.split(":"))
    g = torch.Generator().manual_seed(2)
    qkvg = torch.randn(Nseq * T, 4 * D, generator=g)
    qkvg[:, D:2 * D] *= 0.125
    qkvg = qkvg.to(dev)
    kv = (torch.randn(Nseq, H, 64, 64, generator=g) * 0.3).to(dev)
    out = torch.empty(Nseq * T, D, device=dev)
    ws = torch.empty(ops.retention_prefill_ws(Nseq, H, T), device=dev)
    nch = (T + 63) // 64
    chunks = torch.zeros(nch, Nseq, 64, 4 * D, device=dev)                       # the serial path's layout, staged outside the timing
    q3 = qkvg.view(Nseq, T, 4 * D)
    for c in range(nch):
        n = min(64, T - 64 * c)
        chunks[c, :, :n] = q3[:, 64 * c:64 * c + n]
    lens = [torch.full((Nseq,), t0 + 64 * c, dtype=torch.int32, device=dev) for c in range(nch)]
    cnts = [torch.full((Nseq,), min(64, T - 64 * c), dtype=torch.int32, device=dev) for c in range(nch)]
    o64 = torch.empty(Nseq * 64, D, device=dev)

    def prefill():
        ops.retention_prefill(qkvg, kv, ws, 0, Nseq, H, t0, T, 1e-6, out32=out)

    def serial():
        for c in range(nch):
            ops.retention_chunk_ragged(chunks[c].view(-1, 4 * D), kv, lens[c], cnts[c], 1, Nseq, H, 64, 1e-6, out32=o64)

    forms = [("prefill", prefill), ("serial_chunks", serial)]
    for _, fn in forms:
        fn()
    times = {name: [] for name, _ in forms}
    for _ in range(reps):
        for name, fn in forms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    r = dict(Nseq=Nseq, T=T, t0=t0, work_items_per_pass=Nseq * H * nch)
    for name, ts in times.items():
        r[f"{name}_ms"] = round(median(ts), 4)
        r[f"{name}_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
    r["speedup"] = round(r["serial_chunks_ms"] / r["prefill_ms"], 2)
    r["note"] = "device time between events; serial = ops.retention_chunk_ragged x ceil(T / 64), launches included in both"
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,64")
    ap.add_argument("--frames", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-frames", type=int, default=64)
    ap.add_argument("--prefill-rows", type=int, default=1024)
    ap.add_argument("--kernel", default="1:1024,10:1024")
    ap.add_argument("--kernel-reps", type=int, default=9)
    ap.add_argument("--no-backlog", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ls_prefill_bench needs a GPU")
    from fs_eend_amd.ls_model import OnlineConformerRetentionDADiarization
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    out = dict(tool="ls_prefill_bench", device=torch.cuda.get_device_name(0), C=C, frames=args.frames, rounds=args.rounds,
               max_frames=args.max_frames, prefill_rows=args.prefill_rows, results=[])
    if not args.no_backlog:
        model = OnlineConformerRetentionDADiarization(n_speakers=None, in_size=345, **LS_CFG).eval().to(dev)
        T, m = args.frames, args.max_frames
        g = torch.Generator().manual_seed(1)
        x = (torch.randn(T, 345, generator=g) * 2 - 3).to(dev)
        for S in (int(s) for s in args.slots.split(",") if s):
            ses = LsMultiStreamSession(model, S, C, max_frames=m, prefill_rows=args.prefill_rows)
            s = ses.open()

            def run_prefill():
                ses.prefill(s, x)

            def run_frames():
                for a in range(0, T, m):
                    ses.step_frames(push={s: x[a:a + m]})

            forms = [("prefill", run_prefill), ("step_frames", run_frames)]
            for _, fn in forms:                                                  # warm-up: scratch, graph capture, operand caches
                fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _ in forms}
            for _ in range(args.rounds):                                         # alternating, same run
                for name, fn in forms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[name].append(time.perf_counter() - t0)
            r = dict(slots=S, frames=T, steps=(T + m - 1) // m)
            for name, ts in times.items():
                r[f"{name}_ms"] = round(median(ts) * 1e3, 3)
                r[f"{name}_ms_min_max"] = [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]
                r[f"{name}_frames_per_s"] = round(T / median(ts), 1)
            r["speedup"] = round(r["step_frames_ms"] / r["prefill_ms"], 2)
            r["faster_beyond_spread"] = max(times["prefill"]) < min(times["step_frames"])
            out["results"].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
            ses = run_prefill = run_frames = forms = None                        # release the session's buffers
            torch.cuda.empty_cache()
    if args.kernel:
        out["kernel"] = [kernel_bench(torch, dev, spec, args.kernel_reps) for spec in args.kernel.split(",") if spec]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
