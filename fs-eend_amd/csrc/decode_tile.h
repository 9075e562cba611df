// The steps of the FS-EEND decode attention over a K/V cache (FS-EEND/nnet/modules/streaming_tfm.py:15-37), shared by its four
// forms: one stream (stream.hip), ragged one-frame (stream_multi.hip), ragged chunk (stream_chunk.hip) and prefill
// (attn_prefill.hip).  The products are written out (__builtin_fmaf) where a copy had them written out or where two copies had
// compiled differently (decode_combine4); every other expression is local to its function, so every caller compiles it alike.
// Each kernel keeps its own P.V loop: the serial, the 8-rows-in-flight and the 8-row-group forms sum in different orders, and
// those orders define the bits.
#pragma once
#include "common.h"

constexpr int DT_R = 512;                                // keys per split block, anchored at key 0
constexpr int DT_PART = 66;                              // a partial: o[64], max, sum

// Partials of a split launch: one per (row, head, key block) and query (nq = 1 for the one-frame forms).
inline int decode_nsplit(int cap) { return (cap + DT_R - 1) / DT_R; }
inline long decode_ws_floats(int N, int H, int cap, int nq) { return (long)N * H * decode_nsplit(cap) * nq * DT_PART; }

// Append the new token's k / v (row = the head's q columns of a [q | k | v] row of width 3 D) at cache row t.
DEV void decode_append(_Float16* __restrict__ Kh, _Float16* __restrict__ Vh, int t, const _Float16* __restrict__ row, int D, int lane) {
    Kh[(size_t)t * 64 + lane] = row[D + lane];
    Vh[(size_t)t * 64 + lane] = row[2 * D + lane];
}

// The head's q row times the softmax scale, whole in every lane.
DEV void decode_q_scaled(float (&qf)[64], const _Float16* __restrict__ row, float scale) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const f16x8 q8 = *(const f16x8*)(row + i * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[i * 8 + e] = (float)q8[e] * scale;
    }
}

// Lane = key: the score of this lane's K row kr (one 128-B row per lane, all of it requested before the first product).
DEV float decode_score(const float (&qf)[64], const _Float16* __restrict__ kr) {
    f16x8 k8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k8[i] = *(const f16x8*)(kr + i * 8);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = __builtin_fmaf(qf[i * 8 + e], (float)k8[i][e], acc);
    return acc;
}

// The new token's own score q . k_new (its cache rows are not read back).
DEV float decode_self_score(const _Float16* __restrict__ row, int D, int lane, float scale) {
    float sn = (float)row[lane] * scale * (float)row[D + lane];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) sn = wave_xor_add(sn, m);
    return sn;
}

// Online softmax over one 64-key chunk, lane = key, s = -inf for a lane without a key: moves (m_run, l_run), -> this lane's
// weight p; the caller scales its accumulator by alpha (exp(-inf) = 0 on a first chunk) before it adds P.V.
DEV float decode_softmax_chunk(float s, float& m_run, float& l_run, float& alpha) {
    float cm = s;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) cm = wave_xor_max(cm, m);
    const float m_new = __builtin_fmaxf(m_run, cm);
    alpha = __expf(m_run - m_new);
    const float p = __expf(s - m_new);
    float ps = p;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) ps = wave_xor_add(ps, m);
    l_run = l_run * alpha + ps;
    m_run = m_new;
    return p;
}

// The four waves' (o[64], max, sum) of one query, wave w's at red + w * wstride, into the block's partial pp; the calling
// thread owns dimension d.  A wave without keys holds (0, -inf, 0) and weighs nothing; four of them leave (0, -inf, 0).
// FUSED_O: o's products are fused into the sum (attn_decode_split_kernel has always compiled so, the ragged forms never: the
// partials differ in their last bits, and each keeps its own).
template <bool FUSED_O>
DEV void decode_combine4(const float* red, int wstride, int d, float* __restrict__ pp) {
#pragma clang fp contract(off)
    const float m0 = red[64], m1 = red[wstride + 64], m2 = red[2 * wstride + 64], m3 = red[3 * wstride + 64];
    const float M = __builtin_fmaxf(__builtin_fmaxf(m0, m1), __builtin_fmaxf(m2, m3));
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float mw = red[w * wstride + 64];
        const float f = mw > -INFINITY ? __expf(mw - M) : 0.f;
        L = __builtin_fmaf(red[w * wstride + 65], f, L);
        O = FUSED_O ? __builtin_fmaf(red[w * wstride + d], f, O) : O + red[w * wstride + d] * f;
    }
    pp[d] = O;
    if (d == 0) { pp[64] = M; pp[65] = L; }
}

// Fold (os, ms, ls) into the running (O, M, L) of a merge.  FROM_EMPTY: the running state may still be (0, -inf, 0).
template <bool FROM_EMPTY>
DEV void decode_fold(float& M, float& L, float& O, float ms, float ls, float os) {
    const float Mn = __builtin_fmaxf(M, ms);
    const float a = !FROM_EMPTY || M > -INFINITY ? __expf(M - Mn) : 0.f, b = __expf(ms - Mn);
    L = L * a + ls * b;
    O = O * a + os * b;
    M = Mn;
}

// Walk a row's ns partials in key order, `stride` floats apart; lane = dimension.  SKIP_EMPTY: a partial without keys
// (sum not > 0, as a block at or beyond t leaves it) is passed over.
template <bool SKIP_EMPTY, bool FROM_EMPTY>
DEV void decode_walk(float& M, float& L, float& O, const float* __restrict__ pp, size_t stride, int ns, int lane) {
    for (int s = 0; s < ns; ++s, pp += stride) {
        const float ms = pp[64], ls = pp[65];
        if (SKIP_EMPTY && !(ls > 0.f)) continue;
        decode_fold<FROM_EMPTY>(M, L, O, ms, ls, pp[lane]);
    }
}

// One 32-key chunk against one 16-query tile on mfma_f32_16x16x32_f16: S^T = K Q^T, mask, row maximum, rescale, P^T rounded
// to f16 and summed, O^T += V^T P^T.  kf: K rows of the two 16-key tiles (A operand: row = key, k = d); qf: Q^T[d = 32 ks +
// 8 hq + e][query]; vf: V^T[d = 16 dt + col][key of k slot 8 hq + e], whose k index 8 h + e stands for key 4 h + e (e < 4) or
// 16 + 4 h + e - 4 of the chunk, so that P^T feeds the second product straight from the score registers.  visible(key) says
// whether this lane's query (column lane & 15) sees cache key `key`; the chunk's first key must be visible to every query.
template <class Vis>
DEV void decode_mfma_step(const f16x8 (&kf)[2][2], const f16x8 (&vf)[4], const f16x8 (&qf)[2], f32x4 (&o)[4], float& m_run,
                          float& l_run, int c0, int hq, float scale, Vis visible) {
    f32x4 s[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kt][0], qf[0], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kt][1], qf[1], s[kt], 0, 0, 0);
    }
    float cm = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[kt][r] = visible(c0 + kt * 16 + hq * 4 + r) ? s[kt][r] * scale : -INFINITY;
            cm = __builtin_fmaxf(cm, s[kt][r]);
        }
    cm = wave_xor_max(cm, 16);
    cm = wave_xor_max(cm, 32);                              // finite: the chunk's first key is in every query's column
    const float m_new = __builtin_fmaxf(m_run, cm);
    const float alpha = __expf(m_run - m_new);              // exp(-inf) = 0 on the first chunk
    f16x8 pf;
    float ps = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        pf[e] = (_Float16)__expf(s[e >> 2][e & 3] - m_new);
        ps += (float)pf[e];                                 // the sum of the rounded weights the product uses
    }
    l_run = l_run * alpha + ps;
    m_run = m_new;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        o[dt] *= alpha;
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[dt], pf, o[dt], 0, 0, 0);
    }
}
