// One whole speaker-fusion decoder layer behind the time-axis attention, in one launch on one packed weight stream:
//     x1  = LayerNorm11(A Wo1^T + bo1 + res)                    (spk_stream.hip's head)
//     O   = MHA_over_slots(x1 Win2^T + bin2)
//     x   = LayerNorm21(O Wo2^T + bo2 + x1)                     (ffn_stream.hip's MODE 1 tail, f16 residual)
//     out = LayerNorm22(ReLU(x W1^T + b1) W2^T + b2 + x)
// Replaces eend_attnout_spk_stream_f16 + eend_attnout_ffn_stream_f16 for the FS decoder (f16 rows).  The two-launch pair wrote x1 and O
// (2 x 512 B per row) and read both back; here neither leaves the registers of the wave that computed it:
//   * a wave's 48 rows are spk_stream's slot-grouped tile (the C slots of 48/C consecutive frames), so the speaker attention is the
//     same register arithmetic; the tail is row-local and does not care which rows a wave holds.
//   * x1 stays in the f16 B-operand fragments of the in-projection (xf): exactly the f16 values the pair stored, in the layout
//     ffn_stream's f16 residual loads produce, so it is LayerNorm21's residual as is.
//   * O of all four heads stays in registers (ob, 96 VGPRs) in the layout the attention produces it (lane = token, 16 consecutive
//     head features per 16-lane group); Wo2's contraction index is permuted to that layout at packing time: item h*2 + u takes
//     head features g*16 + u*8 + e from lane group g.  The pair summed the out-projection in natural k order, so the f32 sums of
//     LayerNorm21's input differ from the pair's in rounding only.
//   * one weight stream per parameter version: the 32 items of spk_stream, the 8 Wo2 items, the 2F/32 W1 / W2 items of ffn_stream
//     (W1 in LayerNorm21's register order), flowing through the same 8-slot LDS-DMA ring continuously across tiles.
// Rows move through raw buffer resources (32-bit offsets; accesses beyond the last row are dropped / read as zeros), so every
// tile issues the same VMEM operations and the counted vmcnt waits hold on the last tile too (its prefetch of the next tile's rows
// reads zeros); phantom slot positions (C below the tiling's 3R) read the last slot's rows and their stores are dropped.
// Shipped for C = 3 and 6 only (eend_dec_stream_supported).
#include "common.h"
#include "kernels.h"
#include "wave_rows.h"

namespace {

constexpr int NJ = 3;                    // token fragments per wave (48 rows)
constexpr int SLOT = STREAM_ITEM;        // one stream item: 16 fragments of 1 KB
constexpr int NSLOT = 8;
constexpr int STAGE = NSLOT * SLOT;      // 4 x 2 KB wave-private output staging (4 rows x 512 B)
constexpr int VECS = STAGE + 4 * 2048;   // 11 per-feature f32 vectors (see V_*)
constexpr int B1L = VECS + 11 * 1024;    // b1, up to 2048 hidden units
constexpr int MAXF = 2048;
constexpr int SMEM = B1L + MAXF * 4;     // 158720
constexpr int NB = 8;                    // weight-fragment registers in rotation
constexpr int PD = 6;                    // fragment prefetch distance
constexpr int INFL = 4 * (NSLOT - 3);    // this wave's DMA pieces younger than the ones a barrier needs
constexpr int NSPK = 32;                 // spk_stream's items: Wo1 (8), in-projection (24)
constexpr int NHEAD = NSPK + 8;          // + Wo2 (8)
enum { V_BO1, V_G11, V_BE11, V_BQ, V_BV, V_BO2, V_G21, V_BE21, V_B2, V_G22, V_BE22 };

// ---------------------------------------------------------------------------------------------------------------
// weight stream packing, one thread per 16 bytes.  lane = (f = l & 15, g = l >> 4), n(i, f) = (f>>2)*64 + i*4 + (f&3):
//   items 0 .. 31     spk_stream's (Wo1, then the in-projection with its rows permuted inside each head)
//   items 32 .. 39    Wo2, item h*2 + u, fragment i : Wo2[n(i,f)][h*64 + g*16 + u*8 + e]     (O's register layout)
//   items 40 ..       ffn_stream's W1h(0), {W1h(k), W2h(k-1)}, W2h(U-1) with W1's columns in LayerNorm21's register order
__global__ void dec_stream_pack_kernel(const _Float16* __restrict__ Wo1, const _Float16* __restrict__ Win, const _Float16* __restrict__ Wo2,
                                       const _Float16* __restrict__ W1, const _Float16* __restrict__ W2, _Float16* __restrict__ out, int F) {
    const int U = F / 32;
    const long total = (long)(NHEAD + 2 * U) * (SLOT / 16);
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const int item = (int)(t >> 10), w = (int)(t & 1023);
        const int pfrag = w >> 6, l = w & 63, f = l & 15, g = l >> 4;
        _Float16 v[8];
        if (item < NHEAD) {
            const _Float16* src;
            if (item < 8) src = Wo1 + pack_wo_off(item >> 1, item & 1, pfrag, f, g);
            else if (item < NSPK) src = Win + pack_win_off(item - 8, pfrag, f, g);
            else src = Wo2 + (size_t)((f >> 2) * 64 + pfrag * 4 + (f & 3)) * 256 + ((item - NSPK) >> 1) * 64 + g * 16 + ((item - NSPK) & 1) * 8;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = src[e];
        } else {
            pack_ffn_frag(W1, W2, F, item - NHEAD, pfrag, f, g, true, v);
        }
        _Float16* dst = out + t * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) dst[e] = v[e];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// G frames per wave, R = 16/G slot positions per token fragment, C = 3R positions of which the first CC hold the model's slots (the
// phantom positions read the last slot's rows, are masked as keys and never stored: spk_stream.hip).
template <int G, int CC>
__global__ __launch_bounds__(256, 1)
void dec_stream_kernel(const DecStreamParams p) {
    constexpr int R = 16 / G, C = 3 * R;
    constexpr bool FULL = CC == C;
    static_assert(CC >= 1 && CC <= C, "slot count beyond the positions of this tiling");
    const int TPB = p.Tp / (4 * G);                       // tiles per utterance
    const int ntiles = p.B * TPB;
    const int M = p.B * CC * p.Tp;
    const int U = p.F >> 5;                               // half-chunks of 32 hidden units
    const int S = NHEAD + 2 * U;                          // stream items per tile

    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int frow = lane & 15, g = lane >> 4;
    int fo = g * 64;

    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, (M - 1) * p.lda * 2 + 512, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc((void*)p.res16, 0, M * 512, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(p.out16, 0, M * 512, 0x00020000);
    WeightRing<NSLOT> ring(p.wstream, S, wave, lane);
    ring.prime();

    float* vecs = (float*)(smem + VECS);
    float* b1l = (float*)(smem + B1L);
    {
        vecs[V_BO1 * 256 + tid] = p.bo1[tid];
        vecs[V_G11 * 256 + tid] = p.g11[tid];
        vecs[V_BE11 * 256 + tid] = p.be11[tid];
        vecs[V_BQ * 256 + tid] = p.bin[tid];
        vecs[V_BV * 256 + tid] = p.bin[512 + tid];       // (the key bias cancels in the softmax)
        vecs[V_BO2 * 256 + tid] = p.bo2[tid];
        vecs[V_G21 * 256 + tid] = p.g21[tid];
        vecs[V_BE21 * 256 + tid] = p.be21[tid];
        vecs[V_B2 * 256 + tid] = p.b2[tid];
        vecs[V_G22 * 256 + tid] = p.g22[tid];
        vecs[V_BE22 * 256 + tid] = p.be22[tid];
        for (int i = tid; i < p.F; i += 256) b1l[i] = p.b1[i];
    }
    auto vec4 = [&](int which, int i) __attribute__((always_inline)) { return *(const f32x4*)(vecs + which * 256 + fo + i * 4); };

    const char* wl = smem + lane * 16;
    f16x8 wf[NB];
    f32x4 acc[16][NJ];                                    // Wo1 / Wo2 + W2 accumulators, features fo + i*4 + r
    f32x4 qkv[12][NJ];                                    // one head: [t*4 + ff], features g*16 + ff*4 + r of the head
    f16x8 xf[8][NJ];                                      // input fragments, then x1 (LN11), then x (LN21)
    f16x8 ob[4][2][NJ];                                   // O of head h, features h*64 + g*16 + u*8 + e: ob[h][u]
    f32x4 h[2][NJ];
    f16x8 hbA[NJ], hbB[NJ];                               // hidden activations (W2 B operand), ping-pong
    f32x4 bcv[2];                                         // b1 of the half-chunk held in h
    f16x8 r8[NJ][8];                                      // residual rows of LayerNorm11

    auto row_tok = [&](int tile, int j, int fr) __attribute__((always_inline)) {
        const int b = tile / TPB, tt = tile - b * TPB;
        int c = slot_of<G>(j, fr);
        if constexpr (!FULL) c = c < CC ? c : CC - 1;
        return (b * CC + c) * p.Tp + tt * (4 * G) + wave * G + (fr % G);
    };
    auto load_in_frags = [&](int tile, auto J) __attribute__((always_inline)) {      // xf[s][j] = A[row][s*32 + g*8 ..]
        constexpr int j = decltype(J)::value;
        const int off = row_tok(tile, j, frow) * (p.lda * 2) + g * 16;
#pragma unroll
        for (int s = 0; s < 8; ++s) xf[s][j] = __builtin_bit_cast(f16x8, bload(rsA, off + s * 64));
    };
    auto load_res16 = [&](int tile, auto J) __attribute__((always_inline)) {
        constexpr int j = decltype(J)::value;
        const int off = row_tok(tile, j, frow) * 512 + fo * 2;
#pragma unroll
        for (int e = 0; e < 8; ++e) r8[j][e] = __builtin_bit_cast(f16x8, bload(rsR, off + e * 16));
    };

    wait_vm_lgkm0<4 * (NSLOT - 2)>();                       // item 0 has landed; lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    sfor<NJ>([&](auto J) __attribute__((always_inline)) { load_in_frags(blockIdx.x, J); });

    auto conv_part = [&](auto PART, f16x8 (&hbo)[NJ]) __attribute__((always_inline)) {          // part = hf * NJ + j  (2 NJ parts)
        constexpr int hf = decltype(PART)::value / NJ, j = decltype(PART)::value % NJ;
#pragma unroll
        for (int r = 0; r < 4; ++r) hbo[j][hf * 4 + r] = relu_sat_f16(h[hf][j][r]);
    };

    // One stream item = 16 fragments, 3 MFMAs each:
    //   KIND 0: acc += Wo1 x xf[src]            1: qkv[src*2 + hf] = Win2 x xf (src = t*2 + u)      2: acc += Wo2 x ob[src]
    //   KIND 3: h = W1h(k) x xf                 4: acc += W2h x hb, and (CONV) the activation of h into hbo rides on the fragments
    // vmcnt(INFL + VWX): VWX = this wave's row loads / stores certainly younger than its pieces of the NEXT item (undercounting only
    // waits for more).  COLD: the previous item did not request this item's first fragments; PFN: request the next item's.
    auto step = [&](auto KIND, auto SRCc, auto CONVc, auto COLDc, auto PFNc, auto VWXc, int k, f16x8 (&hb)[NJ],
                    f16x8 (&hbo)[NJ]) __attribute__((always_inline)) {
        constexpr int kind = decltype(KIND)::value, src = decltype(SRCc)::value, vw = INFL + decltype(VWXc)::value;
        constexpr bool conv = decltype(CONVc)::value, cold = decltype(COLDc)::value, pfn = decltype(PFNc)::value;
        stream_item<vw, PD, cold, pfn>(ring, wf, wl, [&](auto PI, const f16x8 w) __attribute__((always_inline)) {
            constexpr int pi = decltype(PI)::value, s_ = pi >> 1, hf = pi & 1;
            auto& hv = h; auto& xv = xf; auto& bv = bcv;      // (wave_rows.h)
            if constexpr (kind == 3 && pi == 0) {
                bcv[0] = *(const f32x4*)(b1l + k * 32 + g * 4);
                bcv[1] = *(const f32x4*)(b1l + k * 32 + 16 + g * 4);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if constexpr (kind == 0) acc[pi][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, xf[src][j], acc[pi][j], 0, 0, 0);
                else if constexpr (kind == 1)
                    qkv[src * 2 + hf][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, xf[s_][j], s_ == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : qkv[src * 2 + hf][j], 0, 0, 0);
                else if constexpr (kind == 2) acc[pi][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, ob[src >> 1][src & 1][j], acc[pi][j], 0, 0, 0);
                else if constexpr (kind == 3) {
                    // VGPR-destination MFMA by hand, the first k-step starts from the bias (ffn_stream.hip)
                    if constexpr (s_ == 0)
                        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %3" : "=&v"(hv[hf][j]) : "v"(w), "v"(xv[s_][j]), "v"(bv[hf]));
                    else
                        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(hv[hf][j]) : "v"(w), "v"(xv[s_][j]));
                } else acc[pi][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, hb[j], acc[pi][j], 0, 0, 0);
            }
        }, [&](auto PI) __attribute__((always_inline)) {
            constexpr int pi = decltype(PI)::value;
            if constexpr (kind == 4 && conv && pi >= 2 && pi < 2 + 4 * NJ && !(pi & 1)) conv_part(IC<(pi - 2) / 2>{}, hbo);
        });
    };
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // (the lane index is recomputed from the exec mask at every phase boundary: nothing lane-dependent stays live -- or is
        // spilled -- across a phase, the thread index included)
        auto relaunder = [&]() __attribute__((always_inline)) {
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
            frow = lane & 15; g = lane >> 4; fo = g * 64;
            ring.set_lane(lane);
            wl = smem + lane * 16;
        };
        relaunder();
        const int ntile = tile + (int)gridDim.x;
        using T = std::true_type;
        using Fa = std::false_type;

        // ---- x1 = LN11(A Wo1^T + bo1 + res)    (spk_stream.hip; x1 is kept in xf, not stored)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const f32x4 b4 = vec4(V_BO1, i);
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = b4;
        }
        pin_acc(acc);
        // items 0..5: the tile's 24 input-row loads (first tile) or the previous tile's 24 output stores are younger than the pieces
        // they wait for
        step(IC<0>{}, IC<0>{}, Fa{}, T{}, T{}, IC<24>{}, 0, hbA, hbB);
        step(IC<0>{}, IC<1>{}, Fa{}, Fa{}, T{}, IC<24>{}, 0, hbA, hbB);
        step(IC<0>{}, IC<2>{}, Fa{}, Fa{}, T{}, IC<24>{}, 0, hbA, hbB);
        step(IC<0>{}, IC<3>{}, Fa{}, Fa{}, T{}, IC<24>{}, 0, hbA, hbB);
        step(IC<0>{}, IC<4>{}, Fa{}, Fa{}, T{}, IC<24>{}, 0, hbA, hbB);
        step(IC<0>{}, IC<5>{}, Fa{}, Fa{}, T{}, IC<24>{}, 0, hbA, hbB);
        step(IC<0>{}, IC<6>{}, Fa{}, Fa{}, T{}, IC<0>{}, 0, hbA, hbB);
        load_res16(tile, IC<0>{});
        step(IC<0>{}, IC<7>{}, Fa{}, Fa{}, Fa{}, IC<8>{}, 0, hbA, hbB);
        pin_acc(acc);
        relaunder();
        sfor<NJ>([&](auto J) __attribute__((always_inline)) {
            constexpr int j = decltype(J)::value;
            auto resv = [&](int i, int q) __attribute__((always_inline)) { return (float)r8[j][i >> 1][(i & 1) * 4 + q]; };
            const LnStats ln = ln_stats_1pass([&](int i, int q) __attribute__((always_inline)) { return acc[i][j][q] + resv(i, q); }, p.eps11);
            const float mean = ln.mean, rstd = ln.rstd;
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (j + 1 < NJ) load_res16(tile, IC<j + 1>{});
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const f32x4 gg = vec4(V_G11, i) * rstd, bb = vec4(V_BE11, i) - vec4(V_G11, i) * (rstd * mean);
                const f32x4 a4 = acc[i][j];
#pragma unroll
                for (int q = 0; q < 4; ++q) xf[i >> 1][j][(i & 1) * 4 + q] = (_Float16)__builtin_fmaf(a4[q] + resv(i, q), gg[q], bb[q]);
                if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
            // laundered: LayerNorm21 reads x1 back from these fragments (without this hipcc kept the converted scalars live across
            // the heads as a second copy of x1 -- and spilled it)
#pragma unroll
            for (int s = 0; s < 8; ++s) asm volatile("" : "+v"(xf[s][j]));
            __builtin_amdgcn_sched_barrier(0);
        });

        // ---- per head: q, k, v of the wave's 48 tokens (6 items), then the C x C attention of its frames in registers -> ob
        float kbias[FULL ? 1 : C];
        slot_kbias<G, CC, NJ>(kbias, frow);
        sfor<4>([&](auto HEAD) __attribute__((always_inline)) {
            constexpr int head = decltype(HEAD)::value;
            // head 0: the residual loads of fragments 1, 2 (16) are younger than the pieces its waits need
            constexpr int yng = head == 0 ? 16 : 0;
            step(IC<1>{}, IC<0>{}, Fa{}, T{}, T{}, IC<yng>{}, 0, hbA, hbB);
            step(IC<1>{}, IC<1>{}, Fa{}, Fa{}, T{}, IC<yng>{}, 0, hbA, hbB);
            step(IC<1>{}, IC<2>{}, Fa{}, Fa{}, T{}, IC<yng>{}, 0, hbA, hbB);
            step(IC<1>{}, IC<3>{}, Fa{}, Fa{}, T{}, IC<yng>{}, 0, hbA, hbB);
            step(IC<1>{}, IC<4>{}, Fa{}, Fa{}, T{}, IC<yng>{}, 0, hbA, hbB);
            step(IC<1>{}, IC<5>{}, Fa{}, Fa{}, Fa{}, IC<yng>{}, 0, hbA, hbB);

            slot_attention<G, CC>(qkv, vecs + V_BQ * 256 + head * 64 + g * 16, vecs + V_BV * 256 + head * 64 + g * 16, p.scale, kbias, ob[head]);
            __builtin_amdgcn_sched_barrier(0);
        });

        // ---- x = LN21(O Wo2^T + bo2 + x1)    (ffn_stream.hip MODE 1, f16 residual = x1 in xf; alpha = 1)
        relaunder();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const f32x4 b4 = vec4(V_BO2, i);
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = b4;
        }
        pin_acc(acc);
        step(IC<2>{}, IC<0>{}, Fa{}, T{}, T{}, IC<0>{}, 0, hbA, hbB);
        step(IC<2>{}, IC<1>{}, Fa{}, Fa{}, T{}, IC<0>{}, 0, hbA, hbB);
        step(IC<2>{}, IC<2>{}, Fa{}, Fa{}, T{}, IC<0>{}, 0, hbA, hbB);
        step(IC<2>{}, IC<3>{}, Fa{}, Fa{}, T{}, IC<0>{}, 0, hbA, hbB);
        step(IC<2>{}, IC<4>{}, Fa{}, Fa{}, T{}, IC<0>{}, 0, hbA, hbB);
        step(IC<2>{}, IC<5>{}, Fa{}, Fa{}, T{}, IC<0>{}, 0, hbA, hbB);
        step(IC<2>{}, IC<6>{}, Fa{}, Fa{}, T{}, IC<0>{}, 0, hbA, hbB);
        step(IC<2>{}, IC<7>{}, Fa{}, Fa{}, Fa{}, IC<0>{}, 0, hbA, hbB);
        pin_acc(acc);
        relaunder();
        sfor<NJ>([&](auto J) __attribute__((always_inline)) {
            constexpr int j = decltype(J)::value;
            auto xval = [&](int i, int q) __attribute__((always_inline)) { return acc[i][j][q] + (float)xf[i >> 1][j][(i & 1) * 4 + q]; };
            const LnStats ln = ln_stats_1pass(xval, p.eps21);
            const float mean = ln.mean, rstd = ln.rstd;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const f32x4 g4 = vec4(V_G21, i), gg = g4 * rstd, bb = vec4(V_BE21, i) - g4 * (rstd * mean), b2 = vec4(V_B2, i);
                f32x4 xo;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float x = __builtin_fmaf(xval(i, q), gg[q], bb[q]);
                    xf[i >> 1][j][(i & 1) * 4 + q] = (_Float16)x;
                    xo[q] = x + b2[q];
                }
                acc[i][j] = xo;
                if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        });

        // ---- FFN: item k = { h = W1h(k) x | acc += W2h(k-1) hb(k-1), hb(k) = ReLU(h + b1) }, k = 0 .. U   (ffn_stream.hip)
        relaunder();
        pin_acc(acc);
        step(IC<3>{}, IC<0>{}, Fa{}, T{}, Fa{}, IC<0>{}, 0, hbA, hbB);
        asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");      // the hand-written MFMAs' results are read by VALU instructions next
        sfor<2 * NJ>([&](auto Q) __attribute__((always_inline)) { conv_part(Q, hbA); });
        step(IC<3>{}, IC<0>{}, Fa{}, T{}, T{}, IC<0>{}, 1, hbA, hbB);
        for (int k = 2; k < U; k += 2) {                    // U is even
            relaunder();
            step(IC<4>{}, IC<0>{}, T{}, Fa{}, T{}, IC<0>{}, 0, hbA, hbB);          // W2h(k-2) x hbA, h(k-1) -> hbB
            step(IC<3>{}, IC<0>{}, Fa{}, Fa{}, T{}, IC<0>{}, k, hbA, hbB);         // W1h(k)
            step(IC<4>{}, IC<0>{}, T{}, Fa{}, T{}, IC<0>{}, 0, hbB, hbA);          // W2h(k-1) x hbB, h(k) -> hbA
            step(IC<3>{}, IC<0>{}, Fa{}, Fa{}, T{}, IC<0>{}, k + 1, hbA, hbB);     // W1h(k+1)
        }
        // x is dead: the next tile's input rows are requested here and travel under the last two items and the epilogue
        // (unconditionally -- rows beyond the last read as zeros -- so that the wait counts hold on the last tile too)
        sfor<NJ>([&](auto J) __attribute__((always_inline)) { load_in_frags(ntile, J); });
        step(IC<4>{}, IC<0>{}, T{}, Fa{}, T{}, IC<8 * NJ>{}, 0, hbA, hbB);          // W2h(U-2) x hbA, h(U-1) -> hbB
        step(IC<4>{}, IC<0>{}, Fa{}, Fa{}, Fa{}, IC<8 * NJ>{}, 0, hbB, hbA);        // W2h(U-1) x hbB
        pin_acc(acc);

        // ---- epilogue, one token fragment at a time: LayerNorm22; rows leave through the wave's 2-KB staging tile as whole
        // 512-byte rows, four at a time; phantom slot rows get an offset beyond the buffer and are dropped
        relaunder();
        char* st = smem + STAGE + wave * 2048;
        sfor<NJ>([&](auto J) __attribute__((always_inline)) {
            constexpr int j = decltype(J)::value;
            const LnStats ln = ln_stats_1pass([&](int i, int q) __attribute__((always_inline)) { return acc[i][j][q]; }, p.eps22);
            const float mean = ln.mean, rstd = ln.rstd;
            __builtin_amdgcn_sched_barrier(0);
            f16x8 o[8];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const f32x4 g4 = vec4(V_G22, i), gg = g4 * rstd, bb = vec4(V_BE22, i) - g4 * (rstd * mean);
                const f32x4 a4 = acc[i][j];
#pragma unroll
                for (int q = 0; q < 4; ++q) o[i >> 1][(i & 1) * 4 + q] = (_Float16)__builtin_fmaf(a4[q], gg[q], bb[q]);
                if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int qr = 0; qr < 4; ++qr) {              // token rows 4 qr .. 4 qr + 3 of the fragment
                if ((frow >> 2) == qr) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) *(f16x8*)(st + (frow & 3) * 512 + (((g * 8 + e) ^ (frow & 3)) << 4)) = o[e];
                }
                wave_lds_sync();
#pragma unroll
                for (int q2 = 0; q2 < 2; ++q2) {
                    const int rr = 2 * q2 + (lane >> 5), cc = lane & 31, fr = qr * 4 + rr;
                    const f16x8 v = *(const f16x8*)(st + rr * 512 + ((cc ^ rr) << 4));
                    const int off = (FULL || slot_of<G>(j, fr) < CC) ? row_tok(tile, j, fr) * 512 + cc * 16 : 0x7FFFFFF0;
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsO, off, 0, 0);
                }
                wave_lds_sync();
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // no LDS-DMA may outlive the workgroup
}

template <int G, int CC>
int launch(const DecStreamParams& p, hipStream_t stream) {
    return stream_launch<dec_stream_kernel<G, CC>>(p, SMEM, p.B * (p.Tp / (4 * G)), eend_cu_count(), stream);
}

constexpr int frames_per_wave(int C) { return C <= 3 ? 16 : C <= 6 ? 8 : 4; }

}  // namespace

long eend_dec_stream_nelems(int F) { return (long)(NHEAD + 2 * (F / 32)) * (SLOT / 2); }

// Shipped for the slot counts that fill a tiling and whose instantiation has been measured against the two-launch pair: C = 3
// (G = 16, no scratch) and C = 6 (G = 8, the headline; 4 VGPRs spilled, 20 B of scratch, one reload per tile).  The other slot
// counts compile to 8 (C = 2, 5), 20 (4) and 51 .. 72 (7 .. 12) spilled VGPRs: they stay on the two launches.
int eend_dec_stream_supported(int C, int Tp) {
    if (C != 3 && C != 6) return 0;
    return Tp > 0 && Tp % (4 * frames_per_wave(C)) == 0;
}

int eend_launch_dec_stream_pack(const void* Wo1, const void* Win, const void* Wo2, const void* W1, const void* W2, void* out, int F,
                                hipStream_t stream) {
    if (!Wo1 || !Win || !Wo2 || !W1 || !W2 || !out || F < 64 || F > MAXF || (F % 64) != 0) return EEND_EINVAL;
    return stream_pack_launch(dec_stream_pack_kernel, eend_dec_stream_nelems(F) / 8, stream, (const _Float16*)Wo1, (const _Float16*)Win,
                              (const _Float16*)Wo2, (const _Float16*)W1, (const _Float16*)W2, (_Float16*)out, F);
}

int eend_launch_dec_stream(const DecStreamParams& p, hipStream_t stream) {
    if (!p.A || !p.wstream || !p.bo1 || !p.g11 || !p.be11 || !p.res16 || !p.bin || !p.bo2 || !p.g21 || !p.be21 || !p.b1 || !p.b2 ||
        !p.g22 || !p.be22 || !p.out16 || p.B <= 0 || p.lda < 256 || (p.lda & 7) || !eend_dec_stream_supported(p.C, p.Tp) || p.F < 64 ||
        p.F > MAXF || (p.F % 64) != 0)
        return EEND_EINVAL;
    // 32-bit buffer offsets: every row of A / res / out, plus the next grid of tiles the input prefetch runs ahead into
    const long rows = (long)p.B * p.C * p.Tp + 65536;
    if (rows * p.lda * 2 >= (1L << 31) || rows * 512 >= (1L << 31)) return EEND_EINVAL;
    switch (p.C) {
#define DEC_CASE(n) case n: return launch<frames_per_wave(n), n>(p, stream);
        DEC_CASE(3) DEC_CASE(6)
#undef DEC_CASE
        default: return EEND_EINVAL;
    }
}
