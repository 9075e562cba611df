// Shared machinery of the persistent weight-stream kernels (ffn_stream, spk_stream, dec_stream, conv_stream, proj_stream,
// gemm_acc_stream, ffn_train_stream): one 256-thread workgroup per CU, one wave per SIMD, packed weights flowing as 16-KB items
// through an LDS ring filled by LDS-DMA, one barrier per item.  Also the compile-time loop, the checked s_waitcnt helpers and the
// pack layouts that more than one stream packs.
#pragma once
#include "common.h"
#include <type_traits>
#include <utility>

template <class F, int... I>
__device__ __forceinline__ void sfor_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void sfor(F&& f) { sfor_impl(f, std::make_integer_sequence<int, N>{}); }
template <int V> using IC = std::integral_constant<int, V>;

typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---- s_waitcnt immediates: vmcnt is a 6-bit field split over bits 3:0 and 15:14, expcnt bits 6:4, lgkmcnt bits 11:8
template <int N>
DEV void wait_vm() {                     // vmcnt(N); expcnt and lgkmcnt untouched
    static_assert(0 <= N && N <= 63, "vmcnt is a 6-bit field");
    __builtin_amdgcn_s_waitcnt(0x0F70 | (N & 15) | ((N >> 4) << 14));
}
template <int N>
DEV void wait_vm_lgkm0() {               // vmcnt(N) lgkmcnt(0)
    static_assert(0 <= N && N <= 63, "vmcnt is a 6-bit field");
    __builtin_amdgcn_s_waitcnt(0x0070 | (N & 15) | ((N >> 4) << 14));
}
DEV void wait_lgkm0() { __builtin_amdgcn_s_waitcnt(0xC07F); }      // lgkmcnt(0); vmcnt and expcnt untouched

// Bytes of one stream item (16 MFMA fragments of 1 KB): the ring's slot and every stream kernel's SLOT.
constexpr int STREAM_ITEM = 16384;

// The dynamic LDS of the stream kernels: one symbol, addressed directly by the ring and the kernel bodies (through a pointer member the
// compiler loses the in-bounds facts of the ring's addresses, and register allocation and waits shift).
extern __shared__ __attribute__((aligned(16))) char smem[];

// ---- the weight ring: NSLOT slots of one 16-KB item at LDS byte offset BASE.  Wave w moves bytes w*4 KB .. w*4 KB + 4095 of every
// item as four 1-KB pieces (one 16-byte buffer load per lane each), so a wave that has waited for its own pieces of an item (counted
// vmcnt) and passed the barrier behind it sees the whole item.  The stream repeats every `nitems` items, continuously across tiles.
// A kernel consumes slot `slot`; the pieces it requests meanwhile fill refill_slot() (the slot every wave finished before the barrier).
template <int NSLOT, int BASE = 0>
struct WeightRing {
    static constexpr int SLOT = STREAM_ITEM;
    __amdgpu_buffer_rsrc_t rs;
    int nitems;
    int wave;
    int dvo;                             // this lane's byte offset in its wave's 4 KB of an item (set_lane() with the laundered lane)
    int nxt = 0;                         // next stream item to request (0 .. nitems - 1)
    int slot = 0;                        // ring slot of the item being consumed

    DEV WeightRing(const void* stream, int nitems_, int wave_, int lane)
        : rs(__builtin_amdgcn_make_buffer_rsrc((void*)stream, 0, nitems_ * SLOT, 0x00020000)), nitems(nitems_), wave(wave_),
          dvo(lane * 16 + wave_ * 4096) {}
    DEV void set_lane(int lane) { dvo = lane * 16 + wave * 4096; }
    // piece I of stream item nxt -> ring slot sd
    template <int I>
    DEV void piece(int sd) const {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_char*)(smem + BASE + sd * SLOT + wave * 4096 + I * 1024), 16, dvo, nxt * SLOT + I * 1024, 0, 0);
    }
    DEV void advance() { nxt = nxt + 1 == nitems ? 0 : nxt + 1; }
    // items 0 .. NSLOT-2 into slots 0 .. NSLOT-2
    DEV void prime() {
        sfor<NSLOT - 1>([&](auto IT) __attribute__((always_inline)) {
            sfor<4>([&](auto I) __attribute__((always_inline)) { piece<decltype(I)::value>(decltype(IT)::value); });
            advance();
        });
    }
    DEV int next_slot() const {
        if constexpr ((NSLOT & (NSLOT - 1)) == 0) return (slot + 1) & (NSLOT - 1);
        else return slot + 1 == NSLOT ? 0 : slot + 1;
    }
    DEV int refill_slot() const {
        if constexpr ((NSLOT & (NSLOT - 1)) == 0) return (slot + NSLOT - 1) & (NSLOT - 1);
        else return slot == 0 ? NSLOT - 1 : slot - 1;
    }
    DEV void rotate() { slot = next_slot(); }
};

// ---- persistent launch: min(ntiles, ncu) workgroups of 256 threads with `lds_bytes` of dynamic LDS (set once per device)
template <auto KERN, class P>
int stream_launch(const P& p, int lds_bytes, long ntiles, int ncu, hipStream_t stream) {
    static EendOncePerDevice attr_once;
    if (!eend_set_dynamic_lds(attr_once, (const void*)KERN, lds_bytes)) return EEND_ELAUNCH;
    hipLaunchKernelGGL(KERN, dim3(ntiles < ncu ? ntiles : ncu), dim3(256), lds_bytes, stream, p);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

// Token fragments per wave (tiles of 64 NJ rows): 192-row tiles reuse every weight fragment for three MFMAs; when they leave CUs idle in
// the only (or last of few) rounds, 128-row tiles finish earlier: compare rounds x rows-per-tile (the time of a tile is close to linear
// in its rows; per-tile cost model: rows + fixed part).
inline int stream_pick_nj(int M, int ncu) {
    const long t3 = (M + 191) / 192, t2 = (M + 127) / 128;
    const long c3 = ((t3 + ncu - 1) / ncu) * (3 * 10 + 9), c2 = ((t2 + ncu - 1) / ncu) * (2 * 10 + 9);
    return c2 < c3 ? 2 : 3;
}

// ---- pack kernels: one thread per 16 bytes of the stream, grid-stride over `total` threads
template <class K, class... A>
int stream_pack_launch(K kern, long total, hipStream_t stream, A... args) {
    const int blocks = (int)((total + 255) / 256);
    hipLaunchKernelGGL(kern, dim3(blocks < 4096 ? blocks : 4096), dim3(256), 0, stream, args...);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

// Pack layouts shared by several streams; lane = (f = l & 15, g = l >> 4) of fragment `pfrag`, 8 elements e per lane.
// Out-projection item (kc, sl), fragment i : Wo[(f>>2)*64 + i*4 + (f&3)][kc*64 + sl*32 + g*8 + e]      (ffn_stream, spk_stream, dec_stream)
DEV size_t pack_wo_off(int kc, int sl, int pfrag, int f, int g) { return (size_t)((f >> 2) * 64 + pfrag * 4 + (f & 3)) * 256 + kc * 64 + sl * 32 + g * 8; }
// Speaker in-projection item q = h*6 + t*2 + u (t = 0 q, 1 k, 2 v), fragment p = s*2 + hf, rows permuted inside each head:
// Win[t*256 + h*64 + (f>>2)*16 + (u*2+hf)*4 + (f&3)][g*64 + 8s + e]                                    (spk_stream, dec_stream)
DEV size_t pack_win_off(int q, int pfrag, int f, int g) {
    const int h = q / 6, tt = (q % 6) >> 1, u = q & 1;
    const int s_ = pfrag >> 1, hf = pfrag & 1;
    return (size_t)(tt * 256 + h * 64 + (f >> 2) * 16 + (u * 2 + hf) * 4 + (f & 3)) * 256 + g * 64 + 8 * s_;
}
// FFN item order over U = F/32 half-chunks: q = 0: W1h(0); 2k-1: W1h(k); 2k: W2h(k-1); 2U-1: W2h(U-1)     (ffn_stream, dec_stream, ffn_train_stream)
DEV void ffn_item_of(int q, int U, bool& is_w1, int& k) {
    if (q == 0) { is_w1 = true; k = 0; }
    else if (q == 2 * U - 1) { is_w1 = false; k = U - 1; }
    else if (q & 1) { is_w1 = true; k = (q + 1) >> 1; }
    else { is_w1 = false; k = (q >> 1) - 1; }
}
// The inference FFN's item q, fragment pfrag (ffn_stream, dec_stream):
//   W1h(k) fragment p = s*2 + hf : W1[k*32 + hf*16 + f][kcol(s,g) + e], kcol = g*64 + 8s (k_permuted: LayerNorm1's register layout)
//                                  or s*32 + g*8 (X read from memory)
//   W2h(k) fragment i            : W2[(f>>2)*64 + i*4 + (f&3)][k*32 + (e>>2)*16 + g*4 + (e&3)]
DEV void pack_ffn_frag(const _Float16* __restrict__ W1, const _Float16* __restrict__ W2, int F, int q, int pfrag, int f, int g, bool k_permuted,
                       _Float16 (&v)[8]) {
    bool is_w1;
    int k;
    ffn_item_of(q, F / 32, is_w1, k);
    if (is_w1) {
        const int s_ = pfrag >> 1, hf = pfrag & 1;
        const int k0 = k_permuted ? g * 64 + 8 * s_ : s_ * 32 + g * 8;
        const _Float16* src = W1 + (size_t)(k * 32 + hf * 16 + f) * 256 + k0;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = src[e];
    } else {
        const int n = (f >> 2) * 64 + pfrag * 4 + (f & 3);
        const _Float16* src = W2 + (size_t)n * F + k * 32 + g * 4;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = src[(e >> 2) * 16 + (e & 3)];
    }
}
