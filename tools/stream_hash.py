"""SHA-256 of every output tensor of the weight-stream entries at small fixed-seed shapes that reach each tiling, the phantom-slot
forms, a ragged last tile, both tile sizes and a second grid round, and of the forward entries that reach the flash and retention tile
loops (flash_tile.h): resident / tiled / packed / long / training attention, chunk-resident / tiled / fused retention; and of every
streaming state entry (decode_tile.h, ls_rows.h) with the state it leaves: K/V caches, partials, retention state, conv cache, windows;
and of every epilogue family of the tiled GEMM (gemm.hip) through its public entries and every launch of the fused FFN family (ffn.hip),
row statistics, x_hat and column partials included (row_epilogue.h).
Two builds of the library compute the same bits exactly when their listings are identical:   python tools/stream_hash.py > a.txt;  EEND_HIP_LIB=<other .so> python tools/stream_hash.py > b.txt"""
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

# ---- the flash and retention tile loops (flash_tile.h): every forward entry that reaches attn*.hip, retention*.hip and ret_stream.hip
nseq, H = 2, 4
z16 = lambda *s: torch.zeros(*s, dtype=torch.float16, device="cuda")
drops = lambda: ((0.0, None), (0.2, ctypes.byref(lib.Dropout(777, int(round(0.2 * (1 << 24))), 1.0 / 0.8))))
w_in = r(768, 256, sc=1 / 8).half()
w_in[:256] = (w_in[:256].float() * ops.QSCALE_LOG2).half()
wp, b_in = ops.inproj_attn_pack(w_in), v(768, sc=0.3)
for Tp in (64, 192, 512, 576):                     # <= 512: the resident kernel (192: odd tile count), 576: the tiled one
    q, k, vt = (r(nseq * H * Tp * 64).bfloat16() for _ in range(3))
    for delay in (0, 65):
        for sname, scale in (("lazy", ops.LN2), ("scaled", 0.125)):
            o = z16(nseq * Tp, 256)
            ops.attn_causal(q, k, vt, o, nseq, H, Tp, delay, Tp - 3, scale)
            show(f"attn_causal Tp={Tp} delay={delay} {sname}", out16=o)
    if Tp in (64, 512):
        for pdrop, dr in drops():
            o, lse = z16(nseq * Tp, 256), torch.zeros(nseq * H * Tp, device="cuda")
            train._call("eend_attn_causal_lse_bf16", q, k, vt, o, lse, nseq, H, Tp, 256, 0, Tp - 3, ops.LN2, dr)
            show(f"attn_causal_lse Tp={Tp} p={pdrop}", out16=o, lse=lse)
for Tp in (64, 192, 512, 576, 1024):               # <= 512: packed, beyond: the long form (576: a short last group)
    x = r(nseq * Tp, 256).half()
    for delay in (0, 65):
        o = z16(nseq * Tp, 256)
        if Tp <= 512:
            ops.inproj_attn_causal_packed(x, wp, b_in, o, nseq, H, Tp, delay, Tp - 3)
        else:
            need = ops.inproj_attn_long_scratch(nseq, Tp, delay, Tp - 3)
            ops.inproj_attn_causal_long(x, wp, b_in, o, z16(need[0]), torch.zeros(need[1], device="cuda"), nseq, H, Tp, delay, Tp - 3)
        show(f"inproj_attn_causal Tp={Tp} delay={delay}", out16=o)
    if Tp in (64, 512):
        for pdrop, dr in drops():
            o, lse = z16(nseq * Tp, 256), torch.zeros(nseq * H * Tp, device="cuda")
            qh, kh, vh = (torch.zeros(nseq * H * Tp * 64, dtype=torch.bfloat16, device="cuda") for _ in range(3))
            train._call("eend_inproj_attn_train_bf16", x, 256, wp, b_in, o, 256, qh, kh, vh, lse, nseq, H, Tp, 0, Tp - 3, dr)
            show(f"inproj_attn_train Tp={Tp} p={pdrop}", out16=o, lse=lse, q=qh, k=kh, v=vh)

wq = r(1024, 256, sc=1 / 16)
wret, bret = ops.retention_stream_pack(wq), v(1024, sc=0.3)
for Tp, Lc in ((128, 64), (192, 100), (320, 300), (640, 576)):      # ragged last chunk; L > 256: two query halves; L > 512: the tiled kernel
    nc = (Tp + Lc - 1) // Lc
    q, k, vv = (r(nseq, H, Tp, 64, sc=0.5).half() for _ in range(3))
    kt, vt, gate, x = k.transpose(-1, -2).contiguous(), vv.transpose(-1, -2).contiguous(), r(nseq * Tp, 256).half(), r(nseq * Tp, 256).half()
    st, cs, se = z16(nseq * H * nc * 2 * 4096), torch.zeros(nseq * H * nc, device="cuda"), torch.zeros(nseq * H * nc, device="cuda")
    for carried in (False, True):
        s_in = r(nseq, H, 64, 64) if carried else None
        s_out = torch.zeros(nseq, H, 64, 64, device="cuda") if carried else None
        o = z16(nseq * Tp, 256)
        ops.retention_chunk(q, k, kt, vt, gate, o, st, cs, se, nseq, H, Tp, Lc, state_in=s_in, state_out=s_out)
        show(f"retention_chunk Tp={Tp} L={Lc} state={int(carried)}", out16=o, **({"state": s_out} if carried else {}))
        if Lc <= 512:
            o = z16(nseq * Tp, 256)
            s_out = torch.zeros(nseq, H, 64, 64, device="cuda") if carried else None
            ops.retention_stream(x, None, wret, bret, o, st, cs, se, nseq, Tp, Lc, state_in=s_in, state_out=s_out)
            show(f"retention_stream Tp={Tp} L={Lc} state={int(carried)}", out16=o, **({"state": s_out} if carried else {}))
    if (Tp, Lc) == (128, 64):
        ctx, rhat, rc = z16(nseq * Tp, 256), z16(nseq * Tp, 256), torch.zeros(nseq * Tp, H, device="cuda")
        kv = torch.zeros(nseq * H * nc * 4096, device="cuda")
        train._call("eend_retention_chunk_train_f16", q, k, kt, vt, gate, ctx, rhat, rc, st, kv, cs, se, nseq, H, Tp, Lc, 256, 256, 1e-6, Tp)
        show(f"retention_chunk_train Tp={Tp} L={Lc}", ctx=ctx, rhat=rhat, rc=rc)

# ---- the streaming state kernels (decode_tile.h, ls_rows.h): outputs and the whole state after each call, stale rows included
i32 = lambda *vals: torch.tensor(vals, dtype=torch.int32, device="cuda")
H, D = 4, 256
for t in (0, 1, 63, 64, 65, 130):                  # one wave per (n, h): 64-key chunks, the last one ragged
    N, cap = 2, 256
    qkv, K0, V0 = r(N, 3 * D).half(), r(N, H, cap, 64).half(), r(N, H, cap, 64).half()
    K, V, o = K0.clone(), V0.clone(), z16(N, D)
    ops.attn_decode(qkv, K, V, o, N, H, cap, t)
    show(f"attn_decode t={t}", out16=o, K=K, V=V)
    K, V, o = K0.clone(), V0.clone(), z16(N, D)
    ops.attn_decode_dev(qkv, K, V, o, N, H, cap, i32(t))
    show(f"attn_decode_dev t={t}", out16=o, K=K, V=V)
for t in (0, 1, 255, 256, 257, 511, 512, 513, 1300):     # 512-key blocks of four waves x 64 keys
    N, cap = 2, 2048
    qkv, K, V, o = r(N, 3 * D).half(), r(N, H, cap, 64).half(), r(N, H, cap, 64).half(), z16(N, D)
    ws = r(ops.attn_decode_split_ws(N, H, cap))
    ops.attn_decode_split(qkv, K, V, o, ws, N, H, cap, i32(t))
    show(f"attn_decode_split t={t}", out16=o, K=K, V=V, ws=ws)
for rps in (1, 3):
    for lens, mask in (((0, 65, 513, 1300), (1, 1, 1, 1)), ((0, 65, 513, 1300), (1, 0, 1, 1)), ((0, 65, 2048, 1300), (1, 1, 1, 1))):
        N, cap = 4 * rps, 2048
        qkv, K, V, o = r(N, 3 * D).half(), r(N, H, cap, 64).half(), r(N, H, cap, 64).half(), r(N, D).half()
        ws = r(ops.attn_decode_ragged_ws(N, H, cap))
        ops.attn_decode_ragged(qkv, K, V, o, ws, N, H, cap, rps, i32(*lens), i32(*mask))
        show(f"attn_decode_ragged rps={rps} lens={lens} mask={mask}", out16=o, K=K, V=V, ws=ws)
for nmax in (1, 16, 17, 64):
    for rps in (1, 3):
        lens, cnt = (0, 31, 33, 129, 512, 600), tuple(min(c, nmax) for c in (64, 1, 0, 16, 17, 64))
        Nseq, cap = 6 * rps, 1024
        qkv, K, V, o = r(Nseq * nmax, 3 * D).half(), r(Nseq, H, cap, 64).half(), r(Nseq, H, cap, 64).half(), r(Nseq * nmax, D).half()
        ws = r(ops.attn_chunk_ragged_ws(Nseq, H, cap, nmax))
        ops.attn_chunk_ragged(qkv, K, V, o, ws, Nseq, H, cap, nmax, rps, i32(*lens), i32(*cnt))
        show(f"attn_chunk_ragged nmax={nmax} rps={rps}", out16=o, K=K, V=V, ws=ws)
for t0, Tq in ((0, 1), (0, 128), (0, 129), (37, 33), (500, 200)):
    for ldq in (768, 800):
        Nseq, cap = 2, 1024
        qkv = r(Nseq * Tq, ldq).half()[:, :3 * D]
        K, V, o = r(3, H, cap, 64).half(), r(3, H, cap, 64).half(), r(Nseq * Tq, D).half()
        ops.attn_prefill(qkv, K, V, o, 1, Nseq, H, t0, Tq)
        show(f"attn_prefill t0={t0} Tq={Tq} ldq={ldq}", out16=o, K=K, V=V)

for s0 in (0.0, 1.0, 7.0):                         # two steps in a row: the second runs on the first's state and scale
    N = 3
    kv16, kv32 = r(N, H, 64, 64), r(N, H, 64, 64)
    sc16, sc32 = torch.full((H,), s0, device="cuda"), torch.full((H,), s0, device="cuda")
    for step in (1, 2):
        o, nsc = z16(N, D), torch.zeros(H, device="cuda")
        ops.retention_step(r(N, 4 * D, sc=0.5).half(), kv16, sc16, nsc, o, N, H)
        show(f"retention_step scale_in={s0} step={step}", out16=o, kv=kv16, scale=nsc)
        sc16 = nsc
        o, o32, nsc = z16(N, D), torch.zeros(N, D, device="cuda"), torch.zeros(H, device="cuda")
        ops.retention_step_f32(r(N, 4 * D, sc=0.5), kv32, sc32, nsc, o, N, H, out32=o32)
        show(f"retention_step_f32 scale_in={s0} step={step}", out16=o, out32=o32, kv=kv32, scale=nsc)
        sc32 = nsc
lens, mask = (0, 1, 7, 100), (1, 1, 0, 1)
kv, o, o32 = r(4, H, 64, 64), r(4, D).half(), r(4, D)
ops.retention_step_ragged(r(4, 4 * D, sc=0.5), kv, i32(*lens), i32(*mask), 1, 4, H, out16=o, out32=o32)
show("retention_step_ragged", out16=o, out32=o32, kv=kv)
for nmax in (1, 5):
    cnt = (nmax, 0, 1, min(3, nmax))
    kv, o, o32 = r(4, H, 64, 64), r(4 * nmax, D).half(), r(4 * nmax, D)
    ops.retention_chunk_ragged(r(4 * nmax, 4 * D, sc=0.5), kv, i32(*lens), i32(*cnt), 1, 4, H, nmax, out16=o, out32=o32)
    show(f"retention_chunk_ragged nmax={nmax}", out16=o, out32=o32, kv=kv)

ktap = 16                                          # conv_kernel_size of the LS-EEND Conformer
wdw, bn = r(D, ktap, sc=0.3), (v(D, 1.0), v(D), v(D), v(D, 1.0).abs() + 0.1)
cache = r(3, D, ktap - 1)
for step in (1, 2):
    o = z16(3, D)
    ops.dwconv_step(r(3, D).half(), cache, wdw, bn, o)
    show(f"dwconv_step step={step}", out16=o, cache=cache)
cache, o = r(4, D, ktap - 1), r(4, D).half()
ops.dwconv_step_ragged(r(4, D).half(), cache, i32(*lens), i32(*mask), wdw, bn, o)
show("dwconv_step_ragged", out16=o, cache=cache)
for nmax in (1, 5):
    cnt = (nmax, 0, 1, min(3, nmax))
    cache, o = r(4, D, ktap - 1), r(4 * nmax, D).half()
    ops.dwconv_chunk_ragged(r(4 * nmax, D).half(), cache, i32(*lens), i32(*cnt), wdw, bn, o, nmax)
    show(f"dwconv_chunk_ragged nmax={nmax}", out16=o, cache=cache)

for C in (1, 3, 12, 16):
    o = r(2 * C, D)
    ops.spk_attn_step_f32(r(2 * C, 3 * D), o, 2, C)
    show(f"spk_attn_step_f32 C={C}", out32=o)
o = r(2 * 3 * 3, D)
ops.spk_attn_rows_f32(r(2 * 3 * 3, 3 * D), o, 2, 3, 3)
show("spk_attn_rows_f32 C=3 Tp=3", out32=o)

ktap, S = 19, 5                                    # the look-ahead window: keep / push / dummy, alone and over a chunk
mode = i32(0, 1, 2, 1, 3)
w16, w32, x = r(S, ktap * D).half(), r(S, ktap * D), r(S, D)
ops.window_push(w16, x, mode)
ops.window_push_f32(w32, x, mode)
show("window_push", win16=w16, win32=w32)
nmax, npush, ndummy, ndec = 5, i32(3, 0, 0, 5, 2), i32(0, 2, 0, 0, 1), i32(2, 2, 0, 5, 3)
w16, w32, x = r(S, ktap * D).half(), r(S, ktap * D), r(S * nmax, D)
c16, c32 = r(S * nmax, ktap * D).half(), r(S * nmax, ktap * D)
ops.window_chunk(w16, x, c16, npush, ndummy, ndec, nmax)
ops.window_chunk_f32(w32, x, c32, npush, ndummy, ndec, nmax)
show("window_chunk", win16=w16, cols16=c16, win32=w32, cols32=c32)

# ---- the tiled GEMM's epilogue families (gemm.hip, row_epilogue.h) through the public entries.  Rows: just above the skinny routes (17),
# one tile minus a tail (77), a ragged second tile (130 on the 128-row tile, 70 on the 64-row one); K on both sides of the launcher's
# straight-line / looped choice.  Weight rows are padded (ldw = K + 8) and N = 384 where packed rows or whole 256-feature groups would send
# the call to proj.hip; every routed entry asserts the route it is on.  The head-row and Conv1d entries take whole 64-frame slabs.
call = train._call
z32 = lambda *s: torch.zeros(*s, device="cuda")
zb16 = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
drop2 = lambda: ((0.0, None), (0.1, ctypes.byref(lib.Dropout(4242, int(round(0.1 * (1 << 24))), 1.0 / 0.9))))


def on_tile(entry, want, **f):
    got = lib.linear_route(entry, **f)
    assert got in want, (entry, f, got)
    return got


for K in (256, 2048):
    ldw = K + 8
    w384, w256 = r(384, ldw, sc=1 / math.sqrt(K)).half(), r(256, ldw, sc=1 / math.sqrt(K)).half()
    wb384, wb256 = w384.bfloat16(), w256.bfloat16()
    bias384, bias256, gam, bet = v(384, sc=0.3), v(256, sc=0.3), v(256, 1.0), v(256)
    tile128 = ("gemm128_straight",) if K == 256 else ("gemm128_looped",)
    for M in (17, 77, 130):
        a = r(M, K).half()
        for act, name in ((ops.ACT_NONE, "none"), (ops.ACT_RELU, "relu"), (ops.ACT_SWISH, "swish")):
            on_tile("linear_f16", tile128, M=M, N=384, K=K, lda=K, ldw=ldw, ldo=384, act=act)
            o = z16(M, 384)
            call("eend_linear_f16", a, K, w384, ldw, bias384, o, 384, M, 384, K, act)
            show(f"linear_f16 M={M} K={K} {name}", out16=o)
        on_tile("linear_glu_f16", tile128, M=M, N=384, K=K, lda=K, ldw=ldw, ldo=192)
        o = z16(M, 192)
        call("eend_linear_glu_f16", a, K, w384, ldw, bias384, o, 192, M, 384, K)
        show(f"linear_glu_f16 M={M} K={K}", out16=o)
        for pdrop, dr in drop2():
            o = z16(M, 384)
            call("eend_linear_relu_train_f16", a, K, w384, ldw, bias384, o, 384, M, 384, K, dr)
            show(f"linear_relu_train M={M} K={K} p={pdrop}", out16=o)
        ab, act16 = a.bfloat16(), (r(M, 384) * (r(M, 384) > 0)).half()
        o = zb16(M, 384)
        call("eend_gemm_bf16", ab, K, wb384, ldw, bias384, o, 384, M, 384, K)
        show(f"gemm_bf16 M={M} K={K}", out=o)
        o = zb16(M, 384)
        call("eend_gemm_relu_bwd_bf16", ab, K, wb384, ldw, act16, 384, o, 384, M, 384, K, 1.0 / 0.9)
        show(f"gemm_relu_bwd_bf16 M={M} K={K}", out=o)
    for M in (17, 77, 70):
        a, res = r(M, K).half(), r(M, 256)
        f = dict(M=M, N=256, K=K, lda=K, ldw=ldw, ldo=256)
        for entry, rr in (("linear_res_ln_f16", res), ("linear_res16_ln_f16", res.half())):
            on_tile(entry, ("gemm64x256",), **f)
            o32, o16 = z32(M, 256), z16(M, 256)
            call("eend_" + entry, a, K, w256, ldw, bias256, rr, 0.5, gam, bet, 1e-5, o32, o16, M, K)
            show(f"{entry} M={M} K={K}", out32=o32, out16=o16)
        on_tile("linear_res_scale_f16", ("gemm64x256",), **f)
        o32, o16 = z32(M, 256), z16(M, 256)
        call("eend_linear_res_scale_f16", a, K, w256, ldw, bias256, res, 0.5, o32, o16, M, K)
        show(f"linear_res_scale_f16 M={M} K={K}", out32=o32, out16=o16)
        on_tile("linear_res_scale_ln16_f16", ("gemm64x256",), **f)
        o32, o16 = z32(M, 256), z16(M, 256)
        call("eend_linear_res_scale_ln16_f16", a, K, w256, ldw, bias256, res, 0.5, gam, bet, 1e-5, o32, o16, M, K)
        show(f"linear_res_scale_ln16_f16 M={M} K={K}", out32=o32, out16=o16)
        for entry in ("eend_linear_res_ln_train_f16", "eend_linear_res_scale_ln_train_f16"):
            for pdrop, dr in drop2():
                o32, o16, xh, rs = z32(M, 256), z16(M, 256), z16(M, 256), z32(M)
                call(entry, a, K, w256, ldw, bias256, res, 0.5, gam, bet, 1e-5, o32, o16, xh, rs, M, K, dr)
                show(f"{entry[5:]} M={M} K={K} p={pdrop}", out32=o32, out16=o16, xhat16=xh, rstd=rs)
        ab, gq = a.bfloat16(), r(M, 256, sc=1e-2)
        o32, o16 = z32(M, 256), zb16(M, 256)
        call("eend_gemm_acc_bf16", ab, K, wb256, ldw, gq, 1.0, o32, o16, M, K)
        show(f"gemm_acc_bf16 M={M} K={K}", out32=o32, out=o16)
        xh, rs = r(M, 256).half(), v(M, 1.0).abs()
        for pdrop, dr in drop2():
            nb = (M + 63) // 64
            ds32, ds16, ws = z32(M, 256), zb16(M, 256), z32(nb * 768)
            dg, db, dbias = z32(256), z32(256), z32(256)
            call("eend_gemm_acc_lnbwd_bf16", ab, K, wb256, ldw, gq, xh, rs, gam, ds32, ds16, ws, nb * 768, dg, db, dbias, M, K, dr)
            show(f"gemm_acc_lnbwd_bf16 M={M} K={K} p={pdrop}", ds32=ds32, ds=ds16, colpart=ws, dgamma=dg, dbeta=db, dbias=dbias)
    for nseq in (1, 2, 3):                         # head rows: 64, 128 (one tile), 192 rows (a half-filled second tile)
        Tp, M = 64, nseq * 64
        a, w768, w1024 = r(M, K).half(), r(768, ldw, sc=1 / math.sqrt(K)).half(), r(1024, ldw, sc=1 / math.sqrt(K)).half()
        on_tile("inproj_heads_bf16", tile128, nseq=nseq, Tp=Tp, H=4, dh=64, K=K, lda=K, ldw=ldw)
        q, k, vt = (zb16(M * 256) for _ in range(3))
        call("eend_inproj_heads_bf16", a, K, w768, ldw, v(768, sc=0.3), q, k, vt, nseq, Tp, 4, 64, K)
        show(f"inproj_heads_bf16 nseq={nseq} K={K}", q=q, k=k, vt=vt)
        on_tile("retention_proj_f16", tile128, nseq=nseq, Tp=Tp, H=4, dh=64, K=K, lda=K, ldw=ldw)
        q, k, kt, vt, gg = (z16(M * 256) for _ in range(5))
        call("eend_retention_proj_f16", a, K, w1024, ldw, v(1024, sc=0.3), q, k, kt, vt, gg, nseq, Tp, 4, 64, K)
        show(f"retention_proj_f16 nseq={nseq} K={K}", q=q, k=k, kt=kt, vt=vt, g=gg)
for nseq, lens in ((1, (64,)), (3, (64, 17, 1))):  # the implicit-GEMM loads: Conv1d + L2 norm, its training form, the Conv1d data gradient
    Tp, ktaps, pad = 64, 3, 1
    x, wr, bias, il = r(nseq * Tp, 256).half(), r(256, ktaps * 256, sc=1 / 28).half(), v(256), i32(*lens)
    o32, o16 = z32(nseq * Tp, 256), z16(nseq * Tp, 256)
    call("eend_conv1d_l2norm_f16", x, wr, bias, il, o32, o16, nseq, Tp, 256, ktaps, pad)
    show(f"conv1d_l2norm_f16 nseq={nseq}", out32=o32, out16=o16)
    o32, o16, inv = z32(nseq * Tp, 256), z16(nseq * Tp, 256), z32(nseq * Tp)
    call("eend_conv1d_l2norm_train_f16", x, wr, bias, il, o32, o16, inv, nseq, Tp, 256, ktaps, pad)
    show(f"conv1d_l2norm_train_f16 nseq={nseq}", out32=o32, out16=o16, inv_norm=inv)
    o32 = z32(nseq * Tp, 256)
    call("eend_conv1d_dgrad_bf16", x.bfloat16(), wr.bfloat16(), il, il, o32, nseq, Tp, 256, ktaps, pad)
    show(f"conv1d_dgrad_bf16 nseq={nseq}", out32=o32)
for Bc, Tp, C in ((1, 17, 33), (2, 35, 33)):       # more than 32 slots: the fan-out stays on the GEMM tile (17 rows, 70 rows)
    on_tile("convert_fanout_f16", ("gemm64x256",), nseq=Bc, Tp=Tp, C=C)
    e, w1c, pc = r(Bc * Tp, 256).half(), r(256, 256, sc=1 / 16).half(), r(C, 256, sc=0.3)
    for with32 in (True, False):
        o32, o16 = z32(Bc * C * Tp, 256) if with32 else None, z16(Bc * C * Tp, 256)
        call("eend_convert_fanout_f16", e, w1c, pc, o32, o16, Bc, Tp, C)
        show(f"convert_fanout_f16 B={Bc} Tp={Tp} C={C} out32={int(with32)}", out16=o16, **({"out32": o32} if with32 else {}))

# ---- every launch of the fused FFN family (ffn.hip): a tile with a tail, a few tiles, and (F = 64) one row tile past a full grid round
ncu = torch.cuda.get_device_properties(0).multi_processor_count
for Fh in (64, 1024):
    w1, w2, b1 = r(Fh, 256, sc=0.08).half(), r(256, Fh, sc=1 / math.sqrt(Fh)).half(), v(Fh, sc=0.3)
    w2t, w1t = w2.t().contiguous().bfloat16(), w1.t().contiguous().bfloat16()
    for M in (77, 300) + ((ncu * 128 + 77,) if Fh == 64 else ()):
        x, a, res = r(M, 256).half(), r(M, 256).half(), r(M, 256)
        for act, name in ((ops.ACT_RELU, "relu"), (ops.ACT_SWISH, "swish")):
            for unnorm in (False, True):
                o32, o16 = z32(M, 256), z16(M, 256)
                ops.ffn_fused(x, w1, b1, w2, b2, res, g22, be22, o32, o16, act=act, alpha=0.5, residual_unnormalised=unnorm)
                show(f"ffn_fused M={M} F={Fh} {name} unnormalised={int(unnorm)}", out32=o32, out16=o16)
        for wl in (None, wo_lo):
            for with_lo in (False, True):
                o32, o16, lo = z32(M, 256), z16(M, 256), z16(M, 256) if with_lo else None
                ops.attnout_ffn_fused(a, wo2, bo2, res, g21, be21, 1e-5, w1, b1, w2, b2, g22, be22, 1e-5, o32, o16, out16lo=lo, wo_lo=wl)
                show(f"attnout_ffn_fused M={M} F={Fh} wo_lo={int(wl is not None)} lo={int(with_lo)}", out32=o32, out16=o16, **({"out16lo": lo} if with_lo else {}))
        o16 = z16(M, 256)
        ops.attnout_ffn_fused(a, wo2, bo2, res, g21, be21, 1e-5, w1, b1, w2, b2, g22, be22, 1e-5, None, o16)
        show(f"attnout_ffn_fused M={M} F={Fh} out32=NULL", out16=o16)
        o32, o16 = z32(M, 256), z16(M, 256)
        ops.attnout_ffn_fused_res16(a, wo2, bo2, res.half(), g21, be21, 1e-5, w1, b1, w2, b2, g22, be22, 1e-5, o32, o16)
        show(f"attnout_ffn_fused_res16 M={M} F={Fh}", out32=o32, out16=o16)
        for pdrop in (0.0, 0.1):
            if pdrop > 0:
                s1, s2 = lib.Dropout(12345, int(round(pdrop * (1 << 24))), 1.0 / (1.0 - pdrop)), lib.Dropout(54321, int(round(pdrop * (1 << 24))), 1.0 / (1.0 - pdrop))
                r1, r2 = ctypes.byref(s1), ctypes.byref(s2)
            else:
                r1 = r2 = None
            o32, o16, hid, xh, rs = z32(M, 256), z16(M, 256), z16(M, Fh), z16(M, 256), z32(M)
            call("eend_ffn_train_f16", x, 256, w1, b1, w2, b2, res, 1.0, g22, be22, 1e-5, o32, o16, hid, xh, rs, M, Fh, r1, r2)
            show(f"ffn_train M={M} F={Fh} p={pdrop}", out32=o32, out16=o16, hid=hid, xhat16=xh, rstd=rs)
            for unnorm in (0, 1):
                o32, o16, zz, aa, xh, rs = z32(M, 256), z16(M, 256), z16(M, Fh), z16(M, Fh), z16(M, 256), z32(M)
                call("eend_ffn_swish_train_f16", x, 256, w1, b1, w2, b2, res, 0.5, g22, be22, 1e-5, o32, o16, zz, aa, xh, rs, M, Fh, unnorm, r1, r2)
                show(f"ffn_swish_train M={M} F={Fh} p={pdrop} unnormalised={unnorm}", out32=o32, out16=o16, z=zz, a=aa, xhat16=xh, rstd=rs)
        dy, g32, dh = r(M, 256, sc=1e-2).bfloat16(), r(M, 256, sc=1e-2), zb16(M, Fh)
        call("eend_ffn_bwd_data_bf16", dy, 256, w2t, hid, w1t, 1.0 / 0.9, dh, g32, M, Fh)      # the mask: the dropout forward's hidden rows
        show(f"ffn_bwd_data M={M} F={Fh}", dH=dh, g=g32)
