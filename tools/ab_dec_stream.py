"""Same-box timing of attnout_spk_ffn_stream (dec_stream.hip) against the two launches it replaces (attnout_spk_stream +
attnout_ffn_stream) at the FS model.test decoder shape (B=64, C=6, Tp=512, F=2048).  Interleaved rounds whose order alternates
(odd rounds run the fused launch first), HIP events, medians.
Usage: python tools/ab_dec_stream.py [rounds] [launches per round] [C]"""
import importlib, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

ops = importlib.import_module("fs-eend_amd.ops")


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    C = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    B, Tp, Fh = 64 * 6 // C, 512, 2048                     # ~196 608 rows at every C
    M = B * C * Tp
    g = torch.Generator(device="cpu").manual_seed(0)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to("cuda")
    a = r(M, 256).half(); res = r(M, 256).half()
    wo1, win, wo2 = r(256, 256, sc=1 / 16).half(), r(768, 256, sc=1 / 8).half(), r(256, 256, sc=0.06).half()
    w1, w2 = r(Fh, 256, sc=0.08).half(), r(256, Fh, sc=0.04).half()
    v = lambda n, base=0.0, sc=0.1: base + r(n, sc=sc)
    bo1, g11, be11, bin_ = v(256), v(256, 1.0), v(256), v(768, sc=0.3)
    bo2, g21, be21, b1, b2, g22, be22 = v(256), v(256, 1.0), v(256), v(Fh, sc=0.3), v(256, sc=0.3), v(256, 1.0), v(256)
    ws1, ws, wsd = ops.spk_stream_pack(wo1, win), ops.ffn_stream_pack(wo2, w1, w2), ops.dec_stream_pack(wo1, win, wo2, w1, w2)
    x1, o, out_p, out_f = torch.empty_like(res), torch.empty_like(a), torch.empty_like(res), torch.empty_like(res)

    def pair():
        ops.attnout_spk_stream(a, ws1, bo1, res, g11, be11, 1e-5, x1, bin_, o, B, C, Tp)
        ops.attnout_ffn_stream(o, ws, bo2, None, x1, g21, be21, 1e-5, b1, b2, g22, be22, 1e-5, None, out_p)

    def fused():
        ops.attnout_spk_ffn_stream(a, wsd, bo1, res, g11, be11, 1e-5, bin_, bo2, g21, be21, 1e-5, b1, b2, g22, be22, 1e-5, out_f, B, C, Tp)

    variants = {"two launches (spk_stream + ffn_stream)": pair, "fused (dec_stream)": fused}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for rnd in range(rounds):
        for k, fn in (list(variants.items())[::-1] if rnd & 1 else variants.items()):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
            ev[0].record()
            for i in range(reps):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
            times[k].append(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(reps)) * 1e3)
    d = (out_f.float() - out_p.float())
    print(f"B={B} C={C} Tp={Tp} F={Fh}")
    print(f"fused vs two launches: max |d| {d.abs().max().item():.3e}, rows differing {(d != 0).any(1).sum().item()} of {M}, "
          f"elements differing {(d != 0).sum().item()} of {d.numel()}")
    base = statistics.median(times["two launches (spk_stream + ffn_stream)"])
    for k, t in times.items():
        med = statistics.median(t)
        print(f"{k:40s} median {med:8.1f} us  per-round medians {['%.1f' % x for x in t]}  ({(1 - med / base) * 100:+.1f} % vs two launches)")


if __name__ == "__main__":
    main()
