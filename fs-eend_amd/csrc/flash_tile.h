// One 64-key step of the transposed flash loop, once: what attn.hip, attn_full.hip and attn_stream.hip (bf16, softmax) and retention.hip,
// retention_full.hip and ret_stream.hip (f16, no softmax) do between their load phases and their stores.  A wave owns 32 query rows, lane
// (lq = lane & 31, hi = lane >> 5) one of them:
//   S^T = K Q^T   : v_mfma_f32_32x32x16(A = K tile, B = Q^T)   -> s[kb][i] of lane (lq, hi) <-> key tile_key(key0, kb, i, hi)
//   O^T = V^T P^T : v_mfma_f32_32x32x16(A = V^T tile, B = P^T) -> oT[db][i] <-> d = db*32 + 8*(i>>2) + 4*hi + (i&3)
// K rows are fed with bits 2<->3 of the row index swapped (swap23), which makes the 8 keys a lane holds per k-step contiguous, so the
// matching V^T fragment is one ds_read_b128 and P goes back as the B operand straight from registers.  K and V^T are [64][128 B] LDS
// tiles in the swz128 image (common.h).  Everything here is always-inline and takes its state by reference; which tiles a wave walks,
// how they got into LDS and where the rows go stay with the kernels.
// How a piece takes its scalars is part of its contract with the register allocator: a by-value parameter is `noundef`, and with that
// LLVM drops freezes and keeps nsw flags far upstream of the call -- enough to move the spill counts of the kernels that sit at the
// 256-register limit.  The step functions take them by value, the row hand-off by const reference: the forms with which
// every kernel keeps its parent's register, spill and scratch counts.  Where no form did, a kernel keeps its own text for the piece and
// says so (attn_stream.hip: scores and mask; retention.hip: mask, |s| sum and P V; retention_full.hip: cross-chunk term).
// Not here: the retention epilogue (row scale, per-head LayerNorm statistics).  Its results depend on which of a row's 32 `o - mean`
// subtractions the compiler contracts with the mean's multiply into an FMA (20 of 32 today, the others subtract a rounded mean), and
// behind a shared function that choice moved: one-ulp differences on rows that nearly cancel.  The three kernels keep that text.
#pragma once
#include "common.h"

DEV int swap23(int r) { return (r & 0x13) | ((r & 4) << 1) | ((r & 8) >> 1); }
// the key that score register i of s[kb] holds in a lane of half hi
DEV int tile_key(int key0, int kb, int i, int hi) { return key0 + kb * 32 + (i & 7) + 8 * hi + 16 * (i >> 3); }

// d = c + a b on v_mfma_f32_32x32x16 of the operand type
template <class F8>
DEV void mfma32(f32x16& d, F8 a, F8 b, const f32x16& c) {
    if constexpr (__is_same(F8, bf16x8)) d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    else d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
DEV f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}

// ---- scores of the tile at kt: s = seed + K Q^T, with Q = q (+ ql: ret_stream.hip's q hi and q lo).  The seed is the C operand of the
// first MFMA: zero16(), or the lazy softmax's -m_ref.
template <class F8, class... QL>
DEV void tile_scores(f32x16 (&s)[2], const f32x16& seed, const char* kt, int krow, int hi, const F8 (&q)[4], const QL (&... ql)[4]) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const F8 kf = *(const F8*)(kt + swz128(kb * 32 + krow, ks * 2 + hi));
            mfma32(s[kb], kf, q[ks], ks == 0 ? seed : (const f32x16&)s[kb]);
            (mfma32(s[kb], kf, ql[ks], s[kb]), ...);
        }
}
// ---- index mask: `fill` (-inf before a softmax, 0 without one) for the keys above `last`
DEV void tile_mask(f32x16 (&s)[2], int key0, int hi, float fill, int last) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (tile_key(key0, kb, i, hi) > last) s[kb][i] = fill;
}
// ---- maximum of the query's 64 scores (both lane halves)
DEV float tile_rowmax(const f32x16 (&s)[2]) {
    float tmax = s[0][0];
#pragma unroll
    for (int i = 1; i < 16; ++i) tmax = __builtin_fmaxf(tmax, s[0][i]);
#pragma unroll
    for (int i = 0; i < 16; ++i) tmax = __builtin_fmaxf(tmax, s[1][i]);
    return wave_xor_max(tmax, 32);
}
// ---- softmax, lazy reference (scores in the log2 domain, seeded with mneg = -m_ref): the softmax is VALU-bound at dh = 64, so the
// reference of a query row only moves when a tile's scores exceed it by more than 2^8 or, on the first tile, sit far below it (exact
// either way: numerator and denominator share m_ref) -- no per-score scale, subtract or rescale of O on the common path.
DEV void softmax_lazy(f32x16 (&s)[2], f32x16 (&oT)[2], f32x16& mneg, float& l_run, float tmax, bool first) {
    const bool move = tmax > 8.0f || (first && tmax < -8.0f);
    if (__builtin_amdgcn_ballot_w64(move) != 0) {
        float d = first ? tmax : __builtin_fmaxf(tmax, 0.f);
        d = d == -INFINITY ? 0.f : d;
        const float alpha = __builtin_amdgcn_exp2f(-d);
        l_run *= alpha;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            oT[0][i] *= alpha; oT[1][i] *= alpha;
            s[0][i] -= d; s[1][i] -= d;
            mneg[i] -= d;
        }
    }
    float lsum0 = 0.f, lsum1 = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        s[0][i] = __builtin_amdgcn_exp2f(s[0][i]);
        s[1][i] = __builtin_amdgcn_exp2f(s[1][i]);
        lsum0 += s[0][i];
        lsum1 += s[1][i];
    }
    l_run += lsum0 + lsum1;
}
// ---- softmax, running maximum (raw scores, scale_log2 = scale * log2(e))
DEV void softmax_running(f32x16 (&s)[2], f32x16 (&oT)[2], float& m_run, float& l_run, float tmax, float scale_log2) {
    const float m_new = __builtin_fmaxf(m_run, tmax * scale_log2);
    const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
    float lsum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][i], scale_log2, -m_use));
            s[kb][i] = pv;
            lsum += pv;
        }
    l_run = l_run * alpha + lsum;
    m_run = m_new;
#pragma unroll
    for (int i = 0; i < 16; ++i) { oT[0][i] *= alpha; oT[1][i] *= alpha; }
}
// ---- training: dropout of the probabilities of row-like index da (the row sum stays un-dropped)
DEV void tile_dropout(f32x16 (&s)[2], const DropSpec& drop, unsigned da, int key0, int hi) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) s[kb][i] = drop_apply(drop, s[kb][i], da, (unsigned)tile_key(key0, kb, i, hi));
}
// ---- O^T += V^T P^T; P^T fragment of k-step (kb, kk): element j = cvt(s[kb][kk*8 + j])
template <class F8, class Cvt>
DEV void tile_pv(f32x16 (&oT)[2], const f32x16 (&s)[2], const char* vt, int lq, int hi, Cvt&& cvt) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            F8 pf;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) pf[jj] = cvt(s[kb][kk * 8 + jj]);
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                const F8 vf = *(const F8*)(vt + swz128(db * 32 + lq, kb * 4 + kk * 2 + hi));
                mfma32(oT[db], vf, pf, oT[db]);
            }
        }
}
DEV void att_pv(f32x16 (&oT)[2], const f32x16 (&s)[2], const char* vt, int lq, int hi) {
    tile_pv<bf16x8>(oT, s, vt, lq, hi, [](float x) __attribute__((always_inline)) { return (__bf16)x; });
}

// ---- retention: sum of |s| of the tile
DEV void tile_abs_sum(const f32x16 (&s)[2], float& absum) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) absum += __builtin_fabsf(s[kb][i]);
}
// ---- retention, cross-chunk term: O^T += up * S_c^T Q^T against the chunk state at Sg ([hd][kd] f16, hi part then lo part, prescaled by
// 1 / up).  Two products, S_hi q + S_lo q, or with q's lo fragments a third, S_hi q_lo.  A lane whose row is not `mine` (it belongs to
// another chunk: retention.hip's waves span chunk boundaries) multiplies by zero.
template <class... QL>
DEV void cross_chunk_add(f32x16 (&oT)[2], const _Float16* Sg, float up, int lq, int hi, bool mine, const f16x8 (&q)[4], const QL (&... ql)[4]) {
    f32x16 x[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) { x[0][i] = 0.f; x[1][i] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        f16x8 qm = q[ks];
        if (!mine) {
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) qm[jj] = (_Float16)0.f;
        }
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            const _Float16* frag = Sg + (db * 32 + lq) * 64 + ks * 16 + hi * 8;
            const f16x8 sa = *(const f16x8*)frag;
            const f16x8 sb = *(const f16x8*)(frag + 4096);
            mfma32(x[db], sa, qm, x[db]);
            mfma32(x[db], sb, qm, x[db]);
            (mfma32(x[db], sa, ql[ks], x[db]), ...);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) { oT[0][i] = __builtin_fmaf(x[0][i], up, oT[0][i]); oT[1][i] = __builtin_fmaf(x[1][i], up, oT[1][i]); }
}
// ---- row hand-off through a wave's 4-KB staging tile st: 32 rows x 128 B, the 16-byte chunk index XORed with row & 7.
// Out: lane (lq, hi) puts its 16 f16x4 -- val(db, i) = feature db*32 + 8*(i>>2) + 4*hi + (i&3) of row lq -- and the tile leaves as
// 128-byte rows (16 B per lane, 8 rows per instruction), LIMIT: only rows below nrows.  A wave's LDS operations run in order; the
// wave_lds_sync after each half keeps the compiler from moving or reusing accesses across it.
DEV char* stage_o_at(char* st, const int& lq, const int& hi, const int& db, const int& g) { return st + lq * 128 + (((db * 4 + g) ^ (lq & 7)) << 4) + hi * 8; }
template <class V>
DEV void stage_rows(char* st, const int& lq, const int& hi, V&& val) {
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f16x4 o;
            o[0] = val(db, g * 4 + 0);
            o[1] = val(db, g * 4 + 1);
            o[2] = val(db, g * 4 + 2);
            o[3] = val(db, g * 4 + 3);
            *(f16x4*)stage_o_at(st, lq, hi, db, g) = o;
        }
    wave_lds_sync();
}
template <bool LIMIT = false>
DEV void store_staged_rows(char* st, const int& lane, _Float16* __restrict__ const& Og, const int& ldo, const int& nrows = 32) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + (lane >> 3), ch = lane & 7;
        if (LIMIT && row >= nrows) continue;
        const u32x4 v = *(const u32x4*)(st + row * 128 + ((ch ^ (row & 7)) << 4));
        *(u32x4*)(Og + (size_t)row * ldo + ch * 8) = v;
    }
    wave_lds_sync();
}
// In: a projection's packed rows pk[ff][jt0 + jl] (4 features ff*16 + fkg*4 .. +3 of token jl*16 + frow, lane = (frow, fkg)) into the
// tile as [token][64 features] rows; then the flash loop's B operand fragments of the 32 tokens
template <int NJ>
DEV void stage_packed(char* st, const int& frow, const int& fkg, const u32x2 (&pk)[4][NJ], const int& jt0) {
#pragma unroll
    for (int jl = 0; jl < 2; ++jl)
#pragma unroll
        for (int ff = 0; ff < 4; ++ff) {
            const int row = jl * 16 + frow;
            *(u32x2*)(st + row * 128 + (((ff * 2 + (fkg >> 1)) ^ (row & 7)) << 4) + (fkg & 1) * 8) = pk[ff][jt0 + jl];
        }
    wave_lds_sync();
}
template <class F8>
DEV void staged_operand(const char* st, const int& lq, const int& hi, F8 (&qf)[4]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = __builtin_bit_cast(F8, *(const u32x4*)(st + lq * 128 + (((ks * 2 + hi) ^ (lq & 7)) << 4)));
    wave_lds_sync();
}
