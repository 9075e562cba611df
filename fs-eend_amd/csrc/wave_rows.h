// What the weight-stream kernels do inside the tile loop, once: the item skeleton around a kernel's MFMAs, the LayerNorm statistics of a
// wave's token rows, the C x C slot attention in registers and the staged row store (ffn_stream, spk_stream, dec_stream; ffn_train_stream,
// gemm_acc_stream and conv_stream use the parts that are the same formula).  Everything here is always-inline and takes the register
// arrays by reference; LDS is addressed from `smem` by the caller's local pointers (wstream.h: no pointer members).
// A body that names a kernel array only inside an asm operand under `if constexpr` first binds it to a local reference (`auto& hv = h;`):
// clang does not capture what only such an operand names.
#pragma once
#include "wstream.h"

// ---- small helpers
DEV u32x4 bload(const __amdgpu_buffer_rsrc_t& r, int off) { return __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0); }
DEV _Float16 relu_sat_f16(float v) { return (_Float16)__builtin_amdgcn_fmed3f(v, 0.f, 65504.f); }      // ReLU + saturation in one instruction
// the accumulators sit in the accumulator half of the register file whenever matrix work is about to run on them
template <int NJ>
DEV void pin_acc(f32x4 (&acc)[16][NJ]) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) asm volatile("" : "+a"(acc[i][j]));
}

// ---- one stream item: 16 fragments rotating through wf[NB], fetched PD fragments ahead.  A wave has waited for its own pieces of the NEXT
// item before the barrier, so the last PD fragments' places are refilled from the next slot (PFN: not in front of a VALU phase); COLD: the
// previous item did not request this item's first PD fragments.  The four DMA pieces of the item NSLOT-1 ahead go out on fragments 0 .. 3
// into the slot every wave finished before the barrier.  body(IC<pi>, w) holds fragment pi's MFMAs; ride(IC<pi>) is a side job that
// travels behind the fragment's LDS and DMA requests (the activation of the previous half-chunk, on some fragments).
template <int PD, bool COLD, bool PFN, class Ring, class W8, int NB, class Body, class Ride>
DEV void stream_item_waited(Ring& ring, W8 (&wf)[NB], const char* wl, Body&& body, Ride&& ride) {
    __builtin_amdgcn_s_barrier();
    const char* wc = wl + ring.slot * STREAM_ITEM;
    const char* wn = wl + ring.next_slot() * STREAM_ITEM;
    const int sd = ring.refill_slot();
    if constexpr (COLD) {
        sfor<PD>([&](auto Q) __attribute__((always_inline)) { wf[decltype(Q)::value % NB] = *(const W8*)(wc + decltype(Q)::value * 1024); });
    }
    sfor<8>([&](auto P2) __attribute__((always_inline)) {
        sfor<2>([&](auto PH) __attribute__((always_inline)) {
            constexpr int pi = decltype(P2)::value * 2 + decltype(PH)::value;
            const W8 w = wf[pi % NB];
            body(IC<pi>{}, w);
            if constexpr (pi + PD < 16) wf[(pi + PD) % NB] = *(const W8*)(wc + (pi + PD) * 1024);
            else if constexpr (PFN) wf[(pi + PD) % NB] = *(const W8*)(wn + (pi + PD - 16) * 1024);
            if constexpr (pi < 4) ring.template piece<pi>(sd);
            ride(IC<pi>{});
        });
        __builtin_amdgcn_sched_barrier(0);
    });
    ring.advance();
    ring.rotate();
}
template <int PD, bool COLD, bool PFN, class Ring, class W8, int NB, class Body>
DEV void stream_item_waited(Ring& ring, W8 (&wf)[NB], const char* wl, Body&& body) {
    stream_item_waited<PD, COLD, PFN>(ring, wf, wl, body, [](auto) __attribute__((always_inline)) {});
}
// ... behind vmcnt(VW): VW = this wave's VMEM operations certainly younger than its pieces of the next item (undercounting only waits for
// more).  A run-time choice between wait counts stays with the caller, in front of stream_item_waited.
template <int VW, int PD, bool COLD, bool PFN, class Ring, class W8, int NB, class Body, class Ride>
DEV void stream_item(Ring& ring, W8 (&wf)[NB], const char* wl, Body&& body, Ride&& ride) {
    wait_vm<VW>();
    stream_item_waited<PD, COLD, PFN>(ring, wf, wl, body, ride);
}
template <int VW, int PD, bool COLD, bool PFN, class Ring, class W8, int NB, class Body>
DEV void stream_item(Ring& ring, W8 (&wf)[NB], const char* wl, Body&& body) {
    stream_item<VW, PD, COLD, PFN>(ring, wf, wl, body, [](auto) __attribute__((always_inline)) {});
}

// ---- LayerNorm statistics of a token row of 256 features spread over the four 16-lane rows: val(i, q) = feature quad i (of 16), element
// q of this lane.  One pass: sum and sum of squares (f32; |x| = O(10)), the variance clamped at zero.
struct LnStats { float mean, rstd; };
template <class V>
DEV LnStats ln_stats_1pass(V&& val, float eps) {
    f32x2 sm = f32x2{0.f, 0.f}, sq2 = f32x2{0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const f32x2 x0 = f32x2{val(i, 0), val(i, 1)}, x1 = f32x2{val(i, 2), val(i, 3)};
        sm += x0 + x1;
        sq2 = x1 * x1 + (x0 * x0 + sq2);
    }
    const float sum = wave_g_allreduce_add(sm[0] + sm[1]);
    const float sqs = wave_g_allreduce_add(sq2[0] + sq2[1]);
    const float mean = sum * (1.0f / 256);
    return {mean, 1.0f / __builtin_sqrtf(__builtin_fmaxf(sqs * (1.0f / 256) - mean * mean, 0.f) + eps)};
}

// ---- the slot-grouped tile (spk_stream.hip): a wave's 16 NJ tokens are the NJ R slot positions of G consecutive frames, R = 16/G positions
// per token fragment, of which the first CC hold the model's slots: slot position of column fr of token fragment j
template <int G>
DEV int slot_of(int j, int fr) { return j * (16 / G) + fr / G; }

template <int N>
DEV float row_rot(float x) {          // value of the lane N places away inside the 16-lane row
    if constexpr (N == 0) return x;
    else return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + N, 0xF, 0xF, false));
}
// score bias of the key each (fragment, rotation) delivers to this lane: 0 for a real slot, -1e30 for a phantom position (rotated with
// the keys, so it always describes the lane it came from)
template <int G, int CC, int NJ, int NK>
DEV void slot_kbias(float (&kbias)[NK], int frow) {
    constexpr int R = 16 / G;
    if constexpr (CC != NJ * R) {
        sfor<NJ>([&](auto J2) __attribute__((always_inline)) {
            constexpr int j2 = decltype(J2)::value;
            const float own = slot_of<G>(j2, frow) < CC ? 0.f : -1e30f;
            sfor<R>([&](auto D) __attribute__((always_inline)) { kbias[j2 * R + decltype(D)::value] = row_rot<decltype(D)::value * G>(own); });
        });
    }
}
// The C x C attention of the wave's frames over one head's q, k, v accumulators (qkv[t*4 + ff][j]: features g*16 + ff*4 + r of the head):
// the keys and values of the other slots of a lane's frame are in the same lane (other token fragment) or a fixed rotation away inside
// the 16-lane row.  Packed f32 arithmetic (v_pk_fma_f32) on register pairs of the accumulator quads; bq / bv: this lane's 16 query /
// value bias entries in LDS, requested one fragment ahead of their use.  o16[u][j]: the head's output features g*16 + u*8 + e of token
// fragment j, saturated to f16 (an MFMA B operand as is).
template <int G, int CC, int NJ, int NK>
DEV void slot_attention(const f32x4 (&qkv)[12][NJ], const float* bq, const float* bv, float scale, const float (&kbias)[NK], f16x8 (&o16)[2][NJ]) {
    constexpr int R = 16 / G, C = NJ * R;
    constexpr bool FULL = CC == C;
    f32x4 bnext = *(const f32x4*)bq;
    f32x2 s2[NJ][C];
#pragma unroll
    for (int a = 0; a < NJ; ++a)
#pragma unroll
        for (int c = 0; c < C; ++c) s2[a][c] = f32x2{0.f, 0.f};
    sfor<4>([&](auto FF) __attribute__((always_inline)) {
        constexpr int ff = decltype(FF)::value;
        const f32x4 b4 = bnext;
        bnext = ff < 3 ? *(const f32x4*)(bq + (ff + 1) * 4) : *(const f32x4*)bv;
        f32x2 q[NJ][2];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const f32x4 t = (qkv[ff][j] + b4) * scale;
            q[j][0] = f32x2{t[0], t[1]}; q[j][1] = f32x2{t[2], t[3]};
        }
        sfor<NJ>([&](auto J2) __attribute__((always_inline)) {
            constexpr int j2 = decltype(J2)::value;
            const f32x4 k = qkv[4 + ff][j2];
            sfor<R>([&](auto D) __attribute__((always_inline)) {
                constexpr int d = decltype(D)::value;
                const f32x2 k0 = f32x2{row_rot<d * G>(k[0]), row_rot<d * G>(k[1])};
                const f32x2 k1 = f32x2{row_rot<d * G>(k[2]), row_rot<d * G>(k[3])};
#pragma unroll
                for (int j1 = 0; j1 < NJ; ++j1) s2[j1][j2 * R + d] = q[j1][1] * k1 + (q[j1][0] * k0 + s2[j1][j2 * R + d]);
            });
        });
    });
    float s[NJ][C];
#pragma unroll
    for (int a = 0; a < NJ; ++a) {
        float mx = -INFINITY, den = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            s[a][c] = s2[a][c][0] + s2[a][c][1];
            if constexpr (!FULL) s[a][c] += kbias[c];
            s[a][c] = wave_g_allreduce_add(s[a][c]);
            mx = __builtin_fmaxf(mx, s[a][c]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) { s[a][c] = __expf(s[a][c] - mx); den += s[a][c]; }
        const float inv = __builtin_amdgcn_rcpf(den);
#pragma unroll
        for (int c = 0; c < C; ++c) s[a][c] *= inv;
    }
    sfor<4>([&](auto FF) __attribute__((always_inline)) {
        constexpr int ff = decltype(FF)::value;
        const f32x4 b4 = bnext;
        if constexpr (ff < 3) bnext = *(const f32x4*)(bv + (ff + 1) * 4);
        f32x2 o[NJ][2];
#pragma unroll
        for (int j = 0; j < NJ; ++j) { o[j][0] = f32x2{b4[0], b4[1]}; o[j][1] = f32x2{b4[2], b4[3]}; }
        sfor<NJ>([&](auto J2) __attribute__((always_inline)) {
            constexpr int j2 = decltype(J2)::value;
            const f32x4 vv = qkv[8 + ff][j2];
            sfor<R>([&](auto D) __attribute__((always_inline)) {
                constexpr int d = decltype(D)::value;
                const f32x2 v0 = f32x2{row_rot<d * G>(vv[0]), row_rot<d * G>(vv[1])};
                const f32x2 v1 = f32x2{row_rot<d * G>(vv[2]), row_rot<d * G>(vv[3])};
#pragma unroll
                for (int j1 = 0; j1 < NJ; ++j1) {
                    const f32x2 pw = f32x2{s[j1][j2 * R + d], s[j1][j2 * R + d]};
                    o[j1][0] = pw * v0 + o[j1][0];
                    o[j1][1] = pw * v1 + o[j1][1];
                }
            });
        });
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            o16[ff >> 1][j][(ff & 1) * 4 + 0] = to_f16_sat(o[j][0][0]); o16[ff >> 1][j][(ff & 1) * 4 + 1] = to_f16_sat(o[j][0][1]);
            o16[ff >> 1][j][(ff & 1) * 4 + 2] = to_f16_sat(o[j][1][0]); o16[ff >> 1][j][(ff & 1) * 4 + 3] = to_f16_sat(o[j][1][1]);
        }
    });
}
// ---- staged row store: 8 token rows of 512 bytes leave through the wave's private staging tile `st` as whole lines.  A lane whose token
// row frow is one of the 8 puts its eight 16-byte slices (line slice g*8 + e, xor-swizzled by the row); after a wave_lds_sync every lane
// gets slice cc = lane & 31 of row rr = 2 q4 + (lane >> 5), q4 = 0 .. 3, and stores it; a second wave_lds_sync frees the tile.
// (Only the addresses are shared: with the loops and the stores behind callables the kernels' register counts moved.)
template <class T>
DEV void stage_put(char* st, int frow, int g, int e, T v) { *(T*)(st + (frow & 7) * 512 + (((g * 8 + e) ^ (frow & 7)) << 4)) = v; }
template <class T>
DEV T stage_get(const char* st, int rr, int cc) { return *(const T*)(st + rr * 512 + ((cc ^ rr) << 4)); }      // (same type as the puts: no type-based reordering)
