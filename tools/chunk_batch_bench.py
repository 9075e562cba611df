"""Time the device data path (fs_eend_amd/device_data.py) against the only other way this project has to build the same tensors.

    python tools/chunk_batch_bench.py [--batches 64,1] [--rounds 5] [--iters 20] [--warmup 5] [--storage f32]

The FS-EEND training shape: B chunks x 5000 STFT frames, context 7, subsampling 10, logmel23_mn, 4 speakers, about 100 segments
per recording; the audio is resident on the device for both forms.
    batched   one DeviceCorpus.batch call: three launches and one descriptor copy
    loop      B calls of feature.extract_fbank_wave on slices of the resident waveforms (three launches and three allocations each), the labels
              rasterised on the host by the reference's rule (slice assignment per segment) and copied over
Each batch size runs in a process of its own under its own time limit (the run stops at the first that fails).  Inside it the
two forms alternate, --rounds times, each round the median of --iters calls that end in a device synchronise, after --warmup
calls of both; the outputs of the two forms are compared bit for bit before anything is timed.  Prints one JSON line.  Kernel
times come from a separate  rocprofv3 --kernel-trace --stats -- python tools/chunk_batch_bench.py --worker 64  run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK, CTX, SUB, TRANSFORM, SPEAKERS = 5000, 7, 10, "logmel23_mn", 4


def host_labels(np, segrows, start, end, n, n_speakers):
    """feature.py:295-317 on pre-rounded segment frames: (n, n_speakers) float32."""
    T = np.zeros((n, n_speakers), dtype=np.float32)
    for sf, ef, spk in segrows:
        a = sf - start if start <= sf < end else None
        b = ef - start if start < ef <= end else None
        if a is not None or b is not None:
            T[a:b, spk] = 1
    return T


def worker(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "chunk_batch_bench needs a GPU"
    from fs_eend_amd import lib as _lib
    _lib.load()
    from fs_eend_amd import device_data as DD, feature
    dev = torch.device("cuda:0")
    B, n_rec, n_frames = a.worker, a.recordings, a.minutes * 6000
    rng = np.random.default_rng(1)
    g = torch.Generator().manual_seed(1)
    corpus = DD.DeviceCorpus(dev, storage=a.storage)
    waves, segrows = {}, {}
    for r in range(n_rec):
        rec = f"rec{r}"
        w = torch.randn(n_frames * 80, generator=g) * 0.1
        if a.storage == "s16":
            w = (w * 32768).clamp(-32768, 32767).to(torch.int16)
        st = rng.uniform(0.0, n_frames / 100 - 8.0, 100)
        seg = [(f"{rec}_u{i}", float(st[i]), float(st[i] + rng.uniform(0.5, 8.0))) for i in range(100)]
        utt2spk = {f"{rec}_u{i}": f"spk{i % SPEAKERS}" for i in range(100)}
        corpus.add(rec, w, seg, utt2spk)
        waves[rec] = (w.float() / 32768 if a.storage == "s16" else w).to(dev)
        segrows[rec] = corpus._segrows[corpus._seg[rec][0]:corpus._seg[rec][1]]
    corpus.finalize()
    rows = [(f"rec{int(rng.integers(n_rec))}", int(s), int(s) + CHUNK) for s in rng.integers(0, n_frames - CHUNK, B)]

    def batched():
        return corpus.batch(rows, CTX, SUB, TRANSFORM, SPEAKERS)

    def loop():
        feats = [feature.extract_fbank_wave(waves[rec][st * 80:ed * 80], CTX, 200, 80, TRANSFORM, SUB) for rec, st, ed in rows]
        labels = [torch.from_numpy(np.ascontiguousarray(host_labels(np, segrows[rec], st, ed, ed - st, SPEAKERS)[::SUB])).to(dev, non_blocking=True)
                  for rec, st, ed in rows]
        return feats, labels, [r[0] for r in rows]

    fb, lb, _ = batched()
    fl, ll, _ = loop()
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(fb, fl)) and all(torch.equal(x, y) for x, y in zip(lb, ll))
    active = float(sum(float(l.sum()) for l in lb)) / sum(l.numel() for l in lb)
    forms = {"loop": loop, "batched": batched}
    for _ in range(a.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in forms}
    for _ in range(a.rounds):                                # alternated: loop, batched, loop, batched, ...
        for name, fn in forms.items():
            ms = []
            for _ in range(a.iters):
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t) * 1e3)
            rounds[name].append(round(statistics.median(ms), 4))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    print(json.dumps({"B": B, "frames_per_chunk": CHUNK, "storage": a.storage, "outputs_bit_identical": same,
                      "label_density": round(active, 4), "round_medians_ms": rounds,
                      "median_ms": {k: round(v, 4) for k, v in med.items()}, "loop_over_batched": round(med["loop"] / med["batched"], 2)}))
    if not same:
        sys.exit("the two forms disagree")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--recordings", type=int, default=8)
    ap.add_argument("--minutes", type=int, default=10)
    ap.add_argument("--storage", default="f32", choices=["f32", "s16"])
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each batch size may take")
    ap.add_argument("--worker", type=int, default=None, help="run one batch size in this process (what the profiler wraps)")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    res = {"tool": "chunk_batch_bench", "rounds": a.rounds, "iters": a.iters, "warmup": a.warmup, "results": [],
           "timing": "host clock around one call that ends in a device synchronise; per round the median of iters calls, forms alternated"}
    for B in [int(b) for b in a.batches.split(",")]:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", str(B), "--rounds",
               str(a.rounds), "--iters", str(a.iters), "--warmup", str(a.warmup), "--recordings", str(a.recordings), "--minutes",
               str(a.minutes), "--storage", a.storage]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                 # a failed or hung step ends the run: nothing more is started on the GPU
            res["failed"] = {"B": B, "returncode": p.returncode, "stdout": p.stdout[-2000:]}
            print(json.dumps(res))
            sys.exit(1)
        res["results"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
