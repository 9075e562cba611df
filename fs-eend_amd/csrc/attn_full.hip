// Causal MHA for chunks that fit on chip (Tp <= 512, i.e. the T = 500 chunks FS-EEND is
// trained and benchmarked on): ONE workgroup per (sequence, head) keeps the head's whole K
// ([Tp][64]) and V^T ([64][Tp]) in LDS (2 x 64 KB), loaded from HBM exactly once, and its 8 waves
// then run the flash loop with NO further barriers.
//
// Why (PMC + timing of the tiled kernel, attn.hip): at T = 500 there are at most 8 key tiles per
// query tile, so that kernel is a chain of load -> LDS -> barrier round trips (51 % of wave cycles
// parked, MFMA pipe 12 % busy), and the 4 query-tile workgroups of a head each re-read its K/V.
// Here the per-tile synchronisation disappears and K/V traffic drops 2.5x.
//
// Causal load balance: the Tp/32 query blocks are dealt to the 8 waves in pairs (w, nq-1-w): a
// late block needs many key tiles, its early partner few -- every wave does ~the same work.
//
// Same arithmetic as attn.hip: the 64-key step is flash_tile.h's (transposed formulation, S^T = K Q^T and
// O^T = V^T P^T on v_mfma_f32_32x32x16_bf16, key rows fed with index bits 2<->3 swapped, online softmax in
// the log2 domain -- lazy reference or running maximum --, index-predicate mask j - i <= mask_delay &&
// j < kv_len); results are bit-identical to it.  O leaves through flash_tile.h's row hand-off: a per-wave
// 4 KB LDS tile, so that global stores are full 128-byte rows (16 B per lane).  This file keeps the LDS-DMA
// load pipeline, the dealing of query blocks to waves and the trace / ablation switches.
#include "flash_tile.h"
#include "kernels.h"

namespace {

constexpr int TMAX = 512;
constexpr int KB = 64;
constexpr int TILE = KB * 128;                       // one [64][64] bf16 tile
constexpr int NW = 8;                                // waves per workgroup
constexpr int OSTG = 32 * 128;                       // per-wave O staging: 32 rows x 128 B (chunk-swizzled)

// LAZY (scale_log2 == 1: the caller folded 1/sqrt(dh) * log2(e) into the q projection): flash_tile.h's softmax_lazy.  The
// softmax is VALU-bound at dh = 64 (PMC: 19 VALU instructions per MFMA, VALU busy 44 % vs MFMA 18 %), so -m_ref is the C operand of
// the first QK^T MFMA and the scores leave the matrix pipe already re-referenced.
// Perf-study build (-DEEND_ATT_TRACE, tools/attn_trace.py): p.Lse is a u64 buffer [blocks][8 waves][16 stamps] of
// s_memtime values at the phase boundaries below; never defined in the shipped library.
#ifdef EEND_ATT_TRACE
#define ATT_STAMP(k)                                                                                             \
    do {                                                                                                         \
        if (lane == 0)                                                                                           \
            ((unsigned long long*)p.Lse)[(((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + wave) * 16 + (k)] = \
                __builtin_amdgcn_s_memtime();                                                                    \
    } while (0)
#else
#define ATT_STAMP(k) do {} while (0)
#endif

template <bool LAZY, bool DROP>
__global__ __launch_bounds__(512)
void attn_causal_full_kernel(const AttnParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ntiles = p.Tp / KB;                    // <= 8
    const int ng = (ntiles + 1) >> 1;                // key groups of 2 tiles (128 keys): the unit of the load pipeline
    char* Ks = smem;                                 // [ntiles][64 keys][128 B]
    char* Vs = smem + ntiles * TILE;                 // [ntiles][64 d][128 B] (64 keys of that tile)
    char* Os = smem + 2 * ntiles * TILE;             // [8 waves][32][128 B]; Tp = 512 -> 160 KB in total

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.x, seq = blockIdx.y;
    const int lq = lane & 31, hi = lane >> 5;
    const size_t sh = (size_t)seq * p.H + h;
    const __bf16* __restrict__ Qg = (const __bf16*)p.Q + sh * p.Tp * 64;
    const __bf16* __restrict__ Kg = (const __bf16*)p.K + sh * p.Tp * 64;
    const __bf16* __restrict__ Vg = (const __bf16*)p.Vt + sh * 64 * p.Tp;

    const int nq = p.Tp / 32;                        // query blocks of 32 rows
    const int krow = swap23(lq);
    char* Ow = Os + wave * OSTG;

    // Causal load balance: the query blocks are dealt to the 8 waves in pairs (nq-1-w, w).  The LATE block of the
    // pair runs first and walks the key groups in order, so it can start on keys 0..127 as soon as those have
    // landed while the other three quarters of K / V^T are still in flight; the early block follows with
    // everything resident.
    const int qb_big = nq - 1 - wave, qb_small = wave;
    const bool has_big = qb_big >= qb_small;         // (false: fewer blocks than waves, this wave's pair is done by another)
    const bool has_small = qb_small < qb_big;        // (false: the pair coincides)

    // ---- the head's whole K and V^T, once, by LDS-DMA (no staging registers, no ds_write pass): 32 pieces of 1 KB
    // per key group (16 of K, 16 of V^T), 4 per wave; the swz128 image is produced by permuting the per-lane
    // SOURCE address (every global row is still read as full 128-byte lines).  Group 0 and the late block's Q
    // fragments are requested first and waited for together; the other groups are requested behind them and
    // land while the first tiles are being computed: `group_ready(g)` is the per-group completion wait (VMEM
    // returns in order) + workgroup barrier.
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void*)Kg, 0, p.Tp * 128, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)Vg, 0, p.Tp * 128, 0x00020000);
    // a piece is 8 tile rows; LDS slot s of tile row r holds source chunk s ^ ((r >> 1) & 7) (common.h swz128)
    const int r8 = lane >> 3;
    const int vok = r8 * 128;                            // K: row r8 of the piece
    const int vov = r8 * p.Tp * 2;                       // V^T: d-row r8 of the piece
    auto dma_group = [&](int g) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = wave * 4 + i;                // 0..15: K pieces, 16..31: V^T pieces of this group
            int t = 2 * g + ((idx >> 3) & 1);
            t = t < ntiles ? t : ntiles - 1;             // odd tile count: the last group re-fetches its only tile
            const int sp = idx & 7;
            const int chunk = (lane & 7) ^ (((sp * 8 + r8) >> 1) & 7);
            if (idx < 16)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (lds_char*)(Ks + t * TILE + sp * 1024), 16, vok + chunk * 16,
                                                         (t * 64 + sp * 8) * 128, 0, 0);
            else
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (lds_char*)(Vs + t * TILE + sp * 1024), 16, vov + chunk * 16,
                                                         sp * 8 * p.Tp * 2 + t * 128, 0, 0);
        }
    };
    bf16x8 qf[4];
    ATT_STAMP(0);
#ifndef EEND_ATT_NOLOAD          // (perf-study ablation: phase costs)
    dma_group(0);
#endif
    {
        const int qrow = (has_big ? qb_big : 0) * 32 + lq;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const bf16x8*)(Qg + (size_t)qrow * 64 + ks * 16 + hi * 8);
    }
    // the fragments are pinned here, so that their wait (which, VMEM being in order, is also group 0's) is not
    // re-inserted by the compiler in front of every use behind the later groups' requests
    asm volatile("" : "+v"(qf[0]), "+v"(qf[1]), "+v"(qf[2]), "+v"(qf[3]));
    ATT_STAMP(1);
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    ATT_STAMP(2);
#ifndef EEND_ATT_NOLOAD
    for (int g = 1; g < ng; ++g) dma_group(g);
#endif
    ATT_STAMP(3);
    auto group_ready = [&](int g) __attribute__((always_inline)) {       // g >= 1
#ifndef EEND_ATT_NOLOAD
        switch (ng - 1 - g) {                            // DMA instructions of later groups that may stay in flight
            case 2: asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory"); break;
            case 1: asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory"); break;
            default: asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory"); break;
        }
#endif
    };

    // per-pass state
    f32x16 oT[2];
    f32x16 mneg;                                     // LAZY: -m_ref of this lane's query in every entry
    float m_run, l_run, m_ref_final;
    int qw0, q;

    auto begin_pass = [&](int qb) __attribute__((always_inline)) {
        qw0 = qb * 32;
        q = qw0 + lq;
#pragma unroll
        for (int i = 0; i < 16; ++i) { oT[0][i] = 0.f; oT[1][i] = 0.f; mneg[i] = 0.f; }
        m_run = -INFINITY; l_run = 0.f; m_ref_final = 0.f;
    };
    auto tiles_of = [&]() __attribute__((always_inline)) -> int {
        int last_key = qw0 + 31 + p.mask_delay;
        last_key = last_key < p.kv_len - 1 ? last_key : p.kv_len - 1;
#ifdef EEND_ATT_NOCOMP
        return 0;
#else
        return last_key < 0 ? 0 : last_key / KB + 1;
#endif
    };

    // one 64-key tile of the flash loop
    auto tile = [&](int j) __attribute__((always_inline)) {
        const int key0 = j * KB;
        const char* kb_ = Ks + j * TILE;
        const char* vb_ = Vs + j * TILE;
        f32x16 s[2];
        tile_scores<bf16x8>(s, LAZY ? mneg : zero16(), kb_, krow, hi, qf);
        const int wlim = qw0 + p.mask_delay < p.kv_len - 1 ? qw0 + p.mask_delay : p.kv_len - 1;
        if (key0 + KB - 1 > wlim) tile_mask(s, key0, hi, -INFINITY, q + p.mask_delay < p.kv_len - 1 ? q + p.mask_delay : p.kv_len - 1);
        const float tmax = tile_rowmax(s);
        if constexpr (LAZY) softmax_lazy(s, oT, mneg, l_run, tmax, j == 0);
        else softmax_running(s, oT, m_run, l_run, tmax, p.scale_log2);
        if constexpr (DROP) tile_dropout(s, p.drop, (unsigned)(sh * p.Tp + q), key0, hi);      // training
        att_pv(oT, s, vb_, lq, hi);
    };

    // O[q][d] = O^T / l: stage the wave's 32 x 64 f16 tile, then 128-byte rows to HBM
    auto end_pass = [&]() __attribute__((always_inline)) {
        if constexpr (LAZY) m_ref_final = -mneg[0]; else m_ref_final = m_run;
        const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
        const float inv = 1.0f / l_tot;
#ifndef EEND_ATT_TRACE
        if (p.Lse && hi == 0)                          // training: log2-domain log-sum-exp of the row, for the backward
            p.Lse[sh * p.Tp + q] = m_ref_final + __builtin_amdgcn_logf(l_tot);
#endif
        stage_rows(Ow, lq, hi, [&](int db, int i) __attribute__((always_inline)) { return to_f16_sat(oT[db][i] * inv); });
        store_staged_rows(Ow, lane, (_Float16*)p.O + ((size_t)seq * p.Tp + qw0) * p.ldo + h * 64, p.ldo);
    };

    // ---- late block of the pair: group by group behind the load stream (every wave takes part in every
    // group_ready, whatever its own tile count)
    bf16x8 qs[4];
    {
        begin_pass(has_big ? qb_big : 0);
        const int jend = has_big ? tiles_of() : 0;
        for (int g = 0; g < ng; ++g) {
            if (g > 0) { ATT_STAMP(2 + 2 * g); group_ready(g); ATT_STAMP(3 + 2 * g); }
            if (g == ng - 1 && has_small) {              // everything has landed: the early block's Q rides under the last tiles
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) qs[ks] = *(const bf16x8*)(Qg + (size_t)(qb_small * 32 + lq) * 64 + ks * 16 + hi * 8);
            }
            if (2 * g < jend) tile(2 * g);
            if (2 * g + 1 < jend) tile(2 * g + 1);
        }
        ATT_STAMP(10);
        if (has_big) end_pass();
        ATT_STAMP(11);
    }
    // ---- early block: everything is resident
    if (has_small) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = qs[ks];
        begin_pass(qb_small);
        const int jend = tiles_of();
        for (int j = 0; j < jend; ++j) tile(j);
        ATT_STAMP(12);
        end_pass();
    }
    ATT_STAMP(13);
}

}  // namespace

int eend_launch_attn_causal_full(const AttnParams& p, hipStream_t stream) {
    if (p.Tp <= 0 || p.Tp > TMAX || (p.Tp % 64) != 0 || (p.ldo & 7)) return EEND_EINVAL;
    const int smem = 2 * (p.Tp / KB) * TILE + NW * OSTG;
    static EendOncePerDevice attr_once[4];
    {
        const int cap = 2 * (TMAX / KB) * TILE + NW * OSTG;
        if (!eend_set_dynamic_lds(attr_once[0], (const void*)attn_causal_full_kernel<false, false>, cap) ||
            !eend_set_dynamic_lds(attr_once[1], (const void*)attn_causal_full_kernel<true, false>, cap) ||
            !eend_set_dynamic_lds(attr_once[2], (const void*)attn_causal_full_kernel<false, true>, cap) ||
            !eend_set_dynamic_lds(attr_once[3], (const void*)attn_causal_full_kernel<true, true>, cap))
            return EEND_ELAUNCH;
    }
    const float dev1 = p.scale_log2 - 1.0f;
    const bool lazy = dev1 < 1e-6f && dev1 > -1e-6f;   // scores arrive in the log2 domain (scale folded into the q projection)
    const bool drop = p.drop.thresh24 != 0;            // training-time dropout of the probabilities: its own instantiation
    const dim3 grid(p.H, p.nseq), block(512);
    if (lazy && !drop) hipLaunchKernelGGL((attn_causal_full_kernel<true, false>), grid, block, smem, stream, p);
    else if (lazy) hipLaunchKernelGGL((attn_causal_full_kernel<true, true>), grid, block, smem, stream, p);
    else if (!drop) hipLaunchKernelGGL((attn_causal_full_kernel<false, false>), grid, block, smem, stream, p);
    else hipLaunchKernelGGL((attn_causal_full_kernel<false, true>), grid, block, smem, stream, p);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
