"""Time one call of the device mixture simulator (fs_eend_amd/simulate.py) against a single-process host path on the same box.

    python tools/simulate_bench.py [--mixtures 64] [--samples 400000] [--speakers 3] [--taps 4000] [--rounds 5] [--iters 5]
                                   [--warmup 2] [--host-mixtures 64] [--storage f32]

The training shape: M mixtures x N samples (50 s at 8 kHz), 3 speakers each with utterances of 2 .. 8 s between exponential
silences, one 4000-tap impulse response and gain per speaker, one noise per mixture at 10 / 15 / 20 dB.  All sources are
resident on the device for the device form and in host memory for the host form.
    device    one simulate() call: one descriptor copy and four launches, the FIR as a Toeplitz product on the exact-f32 MFMA
    host      per track scipy.signal.fftconvolve in float32 over the dry track, summed, the noise scaled by float64 powers and
              added: what a CPU mixing script does, one process
`executed_tflops` counts the MFMA flops the kernel issues (2 x 2048 outputs x steps of every (tile, track, slice) whose span
meets a placement; skipped silences are not counted) against the 157.3 TFLOP/s f32 matrix peak; `useful_gflop` counts 2 K per
placed source sample.  Each round is the median of --iters calls that end in a device synchronise, after
--warmup calls.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TFLOPS = 157.3


def executed_flop(np, p, tile, slice_):
    """MFMA flops of one eend_sim_mix_f32 call with plan p: csrc/simulate.hip's slice loop and its skip test, on the host."""
    flop = 0
    for N, _, track0, ntracks, *_ in p["mix"].tolist():
        t0 = np.arange(0, N, tile, dtype=np.int64)
        for tr in p["tracks"][track0:track0 + ntracks].tolist():
            K, place0, npl = tr[1], tr[3], tr[4]
            pl = p["places"][place0:place0 + npl]
            Mr = (K + 15 + 3) // 4 * 4
            for ms in range(0, Mr, slice_):
                Ls = min(slice_, Mr - ms)
                lo = np.maximum(t0 + 16 - ms - Ls, 0)
                hi = np.minimum(t0 + 16 - ms - Ls + tile + Ls - 16, N)
                met = np.zeros(len(t0), dtype=bool)
                for a, _, n in pl.tolist():
                    met |= np.maximum(lo, a) < np.minimum(hi, a + n)
                flop += int(met.sum()) * 2 * tile * Ls
    return flop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mixtures", type=int, default=64)
    ap.add_argument("--samples", type=int, default=400000)
    ap.add_argument("--speakers", type=int, default=3)
    ap.add_argument("--taps", type=int, default=4000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-mixtures", type=int, default=64, help="mixtures the host form runs (its time is scaled to all of them)")
    ap.add_argument("--storage", default="f32", choices=["f32", "s16"])
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from scipy.signal import fftconvolve
    assert torch.cuda.is_available(), "simulate_bench needs a GPU"
    from fs_eend_amd import simulate as S
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    M, N, K = a.mixtures, a.samples, a.taps
    utts, rirs, noises = S.SourcePool(dev, "f32"), S.SourcePool(dev), S.SourcePool(dev, "f32")
    host_u, host_h, host_n = {}, {}, {}
    for i in range(48):
        host_u[f"u{i}"] = (rng.standard_normal(int(rng.integers(2 * 8000, 8 * 8000))) * 0.05).astype(np.float32)
    for i in range(16):
        host_h[f"h{i}"] = (rng.standard_normal(K) * np.exp(-np.arange(K) / (K / 6))).astype(np.float32) * np.float32(0.05)
    for i in range(4):
        host_n[f"n{i}"] = (rng.standard_normal(30 * 8000) * 0.02).astype(np.float32)
    for pool, waves in ((utts, host_u), (rirs, host_h), (noises, host_n)):
        for name, w in waves.items():
            pool.add(name, w)
        pool.finalize()
    recipes = []
    for m in range(M):                                      # draw_recipes' layout, cut at N samples
        tracks = []
        for s in range(a.speakers):
            pos, pl = 0, []
            while True:
                utt = f"u{int(rng.integers(48))}"
                pos += int(np.rint(rng.exponential(2.0) * 8000))
                if pos >= N:
                    break
                pl.append((utt, pos))
                pos += len(host_u[utt])
            tracks.append({"speaker": f"s{s}", "rir": f"h{int(rng.integers(16))}", "gain": float(10 ** (rng.uniform(-3, 3) / 20)), "placements": pl})
        noise = f"n{int(rng.integers(4))}"
        recipes.append({"name": f"mix{m}", "length": N, "tracks": tracks, "noise": noise, "noise_offset": int(rng.integers(len(host_n[noise]))),
                        "snr_db": float(rng.choice([10.0, 15.0, 20.0]))})
    p = S.plan(recipes, utts, rirs, noises)
    flop = executed_flop(np, p, S.TILE, S.SLICE)
    covered = sum(2 * t[1] * int(p["places"][t[3]:t[3] + t[4], 2].sum()) for t in p["tracks"].tolist())

    def device():
        return S.simulate(utts, rirs, noises, recipes, storage=a.storage)

    def host(n_mix):
        outs = []
        for r in recipes[:n_mix]:
            y = np.zeros(N, dtype=np.float32)
            for t in r["tracks"]:
                d = np.zeros(N, dtype=np.float32)
                for utt, start in t["placements"]:
                    w = host_u[utt][:N - start]
                    d[start:start + len(w)] = w
                y += fftconvolve(d, np.float32(t["gain"]) * host_h[t["rir"]])[:N]
            nz = host_n[r["noise"]]
            n = nz[(r["noise_offset"] + np.arange(N)) % len(nz)]
            Ps, Pn = float(np.sum(y.astype(np.float64) ** 2)), float(np.sum(n.astype(np.float64) ** 2))
            scale = np.float32(np.sqrt(10.0 ** (-r["snr_db"] / 10.0) * Ps / Pn)) if Ps > 0 and Pn > 0 else np.float32(0)
            out = y + scale * n
            outs.append(np.clip(np.rint(out * 32768.0), -32768, 32767).astype(np.int16) if a.storage == "s16" else out)
        return outs

    for _ in range(a.warmup):
        device()
    torch.cuda.synchronize()
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
    corpus, stats = device()
    got = corpus.samples[:N * min(a.host_mixtures, M)].cpu().numpy().reshape(-1, N)
    t = time.perf_counter()
    want = host(min(a.host_mixtures, M))
    host_ms = (time.perf_counter() - t) * 1e3 * M / max(min(a.host_mixtures, M), 1)
    diff = max(float(np.abs(g.astype(np.float64) - w.astype(np.float64)).max()) for g, w in zip(got, want)) if want else 0.0
    print(json.dumps({"tool": "simulate_bench", "mixtures": M, "samples": N, "speakers": a.speakers, "taps": K, "storage": a.storage,
                      "tiles": int(len(p["tiles"])), "placements": int(len(p["places"])), "round_medians_ms": rounds, "device_ms": round(med, 4),
                      "executed_gflop": round(flop / 1e9, 2), "useful_gflop": round(covered / 1e9, 2),
                      "executed_tflops": round(flop / (med * 1e-3) / 1e12, 2), "fraction_of_f32_mfma_peak": round(flop / (med * 1e-3) / 1e12 / PEAK_TFLOPS, 4),
                      "host_mixtures_timed": min(a.host_mixtures, M), "host_ms": round(host_ms, 1), "host_over_device": round(host_ms / med, 1),
                      "max_abs_device_minus_host": diff, "clipped": int(stats["clipped"].sum().item()),
                      "timing": "host clock around one simulate() call that ends in a device synchronise; per round the median of iters calls"}))


if __name__ == "__main__":
    main()
