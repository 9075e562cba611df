"""Time the audio ingest in front of the incremental front-end on one GPU.

    python tools/ingest_bench.py [--baseline DIR] [--rounds 3] [--slots 64] [--chunk-ms 160] [--iters 30] [--hour]

One `AudioFrontEnd.feed` of --slots slots x --chunk-ms of audio from the host, each call device-synchronised, the median of
--iters calls after warm-up:
    feed_8k_f32      8 kHz float, the default path (no ingest: three launches)
    feed_48k_s16     the same audio as 48 kHz 16-bit PCM (two more launches)
    feed_8k_mulaw    the same audio as 8 kHz G.711 mu-law (two more launches)
Every measurement runs in a process of its own.  With --baseline DIR, a built checkout of another commit (the parent), the
8 kHz float feed is measured on both trees in turn, --rounds times each, so that the difference between the two can be read
against the spread between rounds of the same tree.  --hour adds one hour of 48 kHz 16-bit PCM through
feature.extract_fbank_wave (logmel23), the ingest's share of it, and the 8 kHz float hour next to it.  Prints one JSON line.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of  --worker feed_48k_s16."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"feed_8k_f32": (8000, "f32"), "feed_48k_s16": (48000, "s16"), "feed_8k_mulaw": (8000, "mulaw")}


def audio(torch, n, rate, encoding, seed):
    """n samples of seeded noise in the encoding's dtype (the timing does not depend on the values)."""
    g = torch.Generator().manual_seed(seed)
    if encoding == "f32":
        return torch.randn(n, generator=g) * 0.1
    if encoding == "s16":
        return (torch.randn(n, generator=g) * 3000).clamp(-32768, 32767).to(torch.int16)
    return torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8)


def timed(torch, fn, warmup, iters):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for i in range(iters):
        t = time.perf_counter()
        fn(warmup + i)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def worker(a):
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    assert torch.cuda.is_available(), "ingest_bench needs a GPU"
    import __graft_entry__ as G
    G.build()
    from fs_eend_amd import feature
    from fs_eend_amd.audio_stream import AudioFrontEnd
    dev = torch.device("cuda:0")
    if a.worker == "hour":
        res = {}
        for name, rate, enc in (("hour_8k_f32", 8000, "f32"), ("hour_48k_s16", 48000, "s16")):
            y = audio(torch, rate * 3600, rate, enc, 2).to(dev)
            kw = {} if (rate, enc) == (8000, "f32") else dict(sample_rate=rate, encoding=enc)
            ms = timed(torch, lambda i: feature.extract_fbank_wave(y, input_transform="logmel23", **kw), 1, 5)
            res[name + "_ms"] = round(statistics.median(ms), 3)
            if kw:
                from fs_eend_amd import audio_ingest
                ms = timed(torch, lambda i: audio_ingest.convert(y, rate, enc), 1, 5)
                res["hour_48k_s16_ingest_ms"] = round(statistics.median(ms), 3)
            del y
        print(json.dumps(res))
        return
    rate, enc = CASES[a.worker]
    kw = {} if (rate, enc) == (8000, "f32") else dict(sample_rate=rate, encoding=enc)
    S, n = a.slots, rate * a.chunk_ms // 1000
    calls = a.warmup + a.iters
    y = audio(torch, S * (calls * n + 100), rate, enc, 1).view(S, -1)
    fe = AudioFrontEnd(S, "logmel23", device=dev, **kw)
    for s in range(S):
        fe.reset(s)
    fe.feed({s: y[s, :100] for s in range(S)})                           # start mid-frame, as live audio
    ms = timed(torch, lambda i: fe.feed({s: y[s, 100 + i * n:100 + (i + 1) * n] for s in range(S)}), a.warmup, a.iters)
    print(json.dumps({"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                      "launches": 3 + (2 if kw else 0)}))


def run(a, root, case):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", case, "--root", root, "--slots", str(a.slots), "--chunk-ms",
           str(a.chunk_ms), "--iters", str(a.iters), "--warmup", str(a.warmup)]
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", default=None, help="a built checkout of the commit to compare the default path with")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--chunk-ms", type=int, default=160)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--hour", action="store_true")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    res = dict(tool="ingest_bench", slots=a.slots, chunk_ms=a.chunk_ms, iters=a.iters, rounds=a.rounds)
    trees = [("this", ROOT)] + ([("baseline", a.baseline)] if a.baseline else [])
    rounds = {name: [] for name, _ in trees}
    for _ in range(a.rounds):                                            # alternated: baseline, this, baseline, this, ...
        for name, root in reversed(trees):
            rounds[name].append(run(a, root, "feed_8k_f32"))
    for name in rounds:
        res[f"feed_8k_f32_{name}"] = rounds[name]
    for case in ("feed_48k_s16", "feed_8k_mulaw"):
        res[case] = [run(a, ROOT, case) for _ in range(a.rounds)]
    if a.hour:
        res["hour"] = run(a, ROOT, "hour")
    res["timing"] = "host clock around one feed that ends in a device synchronise; median, min and max of iters calls per process"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
