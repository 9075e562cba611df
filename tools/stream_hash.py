"""SHA-256 of every output tensor of the weight-stream entries at small fixed-seed shapes that reach each tiling, the phantom-slot
forms, a ragged last tile, both tile sizes and a second grid round.  Two builds of the library compute the same bits exactly when
their listings are identical:   python tools/stream_hash.py > a.txt;  EEND_HIP_LIB=<other .so> python tools/stream_hash.py > b.txt"""
import ctypes, hashlib, importlib, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

ops = importlib.import_module("fs-eend_amd.ops")
train = importlib.import_module("fs-eend_amd.train")
lib = importlib.import_module("fs-eend_amd.lib")

g = torch.Generator(device="cpu").manual_seed(0)
r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to("cuda")
v = lambda n, base=0.0, sc=0.1: base + r(n, sc=sc)


def show(case, **outs):
    torch.cuda.synchronize()
    for k, t in outs.items():
        print(f"{case:58s} {k:8s} {hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()}")


wo1, win, wo2 = r(256, 256, sc=1 / 16).half(), r(768, 256, sc=1 / 8).half(), r(256, 256, sc=0.06).half()
bo1, g11, be11, bin_ = v(256), v(256, 1.0), v(256), v(768, sc=0.3)
bo2, g21, be21, b2, g22, be22 = v(256), v(256, 1.0), v(256), v(256, sc=0.3), v(256, 1.0), v(256)
ws_spk = ops.spk_stream_pack(wo1, win)

for B, C, Tp in ((2, 3, 64), (2, 6, 64), (2, 12, 64), (2, 1, 64), (3, 4, 64), (2, 7, 64), (90, 6, 128)):
    M = B * C * Tp
    a, res = r(M, 256).half(), r(M, 256).half()
    x16, o = torch.zeros_like(res), torch.zeros_like(a)
    ops.attnout_spk_stream(a, ws_spk, bo1, res, g11, be11, 1e-5, x16, bin_, o, B, C, Tp)
    show(f"attnout_spk_stream B={B} C={C} Tp={Tp}", x16=x16, out16=o)
    x32, o = torch.zeros(M, 256, device="cuda"), torch.zeros_like(a)
    ops.attnout_spk_stream_res32(a, ws_spk, bo1, res.float(), g11, be11, 1e-5, x32, bin_, o, B, C, Tp)
    show(f"attnout_spk_stream_res32 B={B} C={C} Tp={Tp}", x32=x32, out16=o)

for Fh in (64, 2048):
    w1, w2, b1 = r(Fh, 256, sc=0.08).half(), r(256, Fh, sc=0.04).half(), v(Fh, sc=0.3)
    ws_dec = ops.dec_stream_pack(wo1, win, wo2, w1, w2)
    for B, C, Tp in ((2, 3, 64), (2, 6, 64), (90, 6, 128)):
        M = B * C * Tp
        a, res = r(M, 256).half(), r(M, 256).half()
        out = torch.zeros_like(res)
        ops.attnout_spk_ffn_stream(a, ws_dec, bo1, res, g11, be11, 1e-5, bin_, bo2, g21, be21, 1e-5, b1, b2, g22, be22, 1e-5, out, B, C, Tp)
        show(f"attnout_spk_ffn_stream B={B} C={C} Tp={Tp} F={Fh}", out16=out)

Fh = 256
w1, w2, b1 = r(Fh, 256, sc=0.08).half(), r(256, Fh, sc=0.04).half(), v(Fh, sc=0.3)
wo_lo = (wo2.float() * 2 ** -11).half()
ws_ffn, ws_lo, ws_plain = ops.ffn_stream_pack(wo2, w1, w2), ops.ffn_stream_pack_lo(wo2, wo_lo, w1, w2), ops.ffn_stream_pack(None, w1, w2)
for M in (192, 77, 300, 70000):
    a, res = r(M, 256).half(), r(M, 256)
    for rname, r32, r16 in (("res32", res, None), ("res16", None, res.half())):
        for with32 in (False, True):
            out16, out32 = torch.zeros(M, 256, dtype=torch.float16, device="cuda"), torch.zeros(M, 256, device="cuda") if with32 else None
            ops.attnout_ffn_stream(a, ws_ffn, bo2, r32, r16, g21, be21, 1e-5, b1, b2, g22, be22, 1e-5, out32, out16)
            show(f"attnout_ffn_stream M={M} {rname} out32={int(with32)}", out16=out16, **({"out32": out32} if with32 else {}))
    out16, out32, lo = torch.zeros(M, 256, dtype=torch.float16, device="cuda"), torch.zeros(M, 256, device="cuda"), torch.zeros(M, 256, dtype=torch.float16, device="cuda")
    ops.attnout_ffn_stream_lo(a, ws_lo, bo2, res, g21, be21, 1e-5, b1, b2, g22, be22, 1e-5, out32, out16, lo)
    show(f"attnout_ffn_stream_lo M={M}", out16=out16, out32=out32, out16lo=lo)
M = 300
x, res = r(M, 256).half(), r(M, 256)
for act, name in ((ops.ACT_RELU, "relu"), (ops.ACT_SWISH, "swish")):
    for unnorm in (False, True):
        out16, out32 = torch.zeros(M, 256, dtype=torch.float16, device="cuda"), torch.zeros(M, 256, device="cuda")
        ops.ffn_stream(x, ws_plain, b1, b2, res, g22, be22, out32, out16, act=act, alpha=0.5, residual_unnormalised=unnorm)
        show(f"ffn_stream M={M} {name} unnormalised={int(unnorm)}", out16=out16, out32=out32)

# the training GEMM g += A Wt^T on a packed stream: below and above one tile, both tile sizes
L = lib.load()
for M, K in ((100, 256), (300, 768), (70000, 256)):
    a = r(M, K, sc=0.5).bfloat16()
    wt = r(256, K, sc=1 / 16).bfloat16()
    gq = r(M, 256)
    ws = torch.empty(L.eend_gemm_acc_stream_elems(K), dtype=torch.bfloat16, device="cuda")
    train._call("eend_gemm_acc_stream_pack_bf16", wt, K, ws, K)
    train._call("eend_gemm_acc_stream_bf16", a, K, ws, gq, M, K)
    show(f"gemm_acc_stream M={M} K={K}", g=gq)

# the training FFN on packed streams: forward without and with dropout, then the data gradient on the dropout forward's hidden rows;
# one shape below a tile and one above (rows in whole 16-row blocks)
Fh = 256
for M in (96, 400):
    x, res = r(M, 256).half(), r(M, 256)
    w1, w2 = r(Fh, 256, sc=1 / 16).half(), r(256, Fh, sc=1 / math.sqrt(Fh)).half()
    b1, b2t = v(Fh), v(256)
    ws = torch.empty(L.eend_ffn_train_stream_elems(Fh), dtype=torch.float16, device="cuda")
    train._call("eend_ffn_train_stream_pack", w1, w2, ws, Fh)
    for pdrop in (0.0, 0.1):
        o32, o16 = torch.zeros(M, 256, device="cuda"), torch.zeros(M, 256, dtype=torch.float16, device="cuda")
        hid, xh, rs = torch.zeros(M, Fh, dtype=torch.float16, device="cuda"), torch.zeros(M, 256, dtype=torch.float16, device="cuda"), torch.zeros(M, device="cuda")
        if pdrop > 0:
            s1 = lib.Dropout(12345, int(round(pdrop * (1 << 24))), 1.0 / (1.0 - pdrop))
            s2 = lib.Dropout(54321, int(round(pdrop * (1 << 24))), 1.0 / (1.0 - pdrop))
            r1, r2 = ctypes.byref(s1), ctypes.byref(s2)
        else:
            r1 = r2 = None
        train._call("eend_ffn_train_stream_f16", x, 256, ws, b1, b2t, res, 1.0, g22, be22, 1e-5, o32, o16, hid, xh, rs, M, Fh, r1, r2)
        show(f"ffn_train_stream fwd M={M} p={pdrop}", out32=o32, out16=o16, hid=hid, xhat16=xh, rstat=rs)
    dy, g32 = r(M, 256, sc=1e-2).bfloat16(), r(M, 256, sc=1e-2)
    w2t, w1t = w2.t().contiguous().bfloat16(), w1.t().contiguous().bfloat16()
    dh, wsb = torch.zeros(M, Fh, dtype=torch.bfloat16, device="cuda"), torch.empty(L.eend_ffn_train_stream_elems(Fh), dtype=torch.bfloat16, device="cuda")
    train._call("eend_ffn_train_stream_pack", w2t, w1t, wsb, Fh)
    train._call("eend_ffn_bwd_data_stream_bf16", dy, 256, wsb, hid, 1.0 / 0.9, dh, g32, M, Fh)
    show(f"ffn_bwd_data_stream M={M}", dH=dh, g=g32)

# the Conv1d + L2 norm on a packed stream: one sequence of one tile, and ragged sequences over several tiles
for nseq, Tp, lens in ((1, 64, [64]), (3, 128, [128, 77, 1])):
    ktaps, pad = 19, 9
    x = r(nseq * Tp, 256).half()
    wr = r(256, ktaps * 256, sc=1 / 40).half()
    bias, il = v(256), torch.tensor(lens, dtype=torch.int32, device="cuda")
    o32, o16 = torch.zeros(nseq * Tp, 256, device="cuda"), torch.zeros(nseq * Tp, 256, dtype=torch.float16, device="cuda")
    ops.conv1d_l2norm_stream(x, ops.conv_stream_pack(wr, ktaps), bias, il, o32, o16, nseq, Tp, ktaps, pad)
    show(f"conv1d_l2norm_stream nseq={nseq} Tp={Tp}", out32=o32, out16=o16)
