// One LS-EEND stream slot taken forward by a backlog of any length (LsMultiStreamSession.prefill, ls_multistream.py): the two
// state touches of the LS frame step that have no long-T form in ls_chunk.hip.
//
// Retention.  ret_chunk_ragged_kernel walks a sequence's frames serially, one wave per (sequence, head).  The recurrence of
// ls_rows.h has decay 1,
//     kv_t = kv_{t-1} sqrt(t / (t+1)) + v_t k_t^T / sqrt(t+1),    o_t[a] = sum_b q_t[b] kv_t[a][b],
// so kv_t = (sqrt(t0) kv_{t0-1} + sum_{i = t0..t} v_i k_i^T) / sqrt(t+1), and in chunks of 64 frames three passes do the work
// of T dependent frame updates, each with one work item per (sequence, head, chunk):
//     sums    P_c = sum_{i in c} v_i k_i^T                                               64 x 64 per item, into the workspace
//     scan    S_c = sqrt(t0) kv_in + sum_{c' < c} P_c' (in chunk order, in place over P_c);  kv_out = (S_last + P_last) / sqrt(t0 + T)
//     outputs o_i = ((Q K^T . [j <= i]) V + Q S_c^T)_i / sqrt(t0 + 64 c + i + 1), then ret_norm_gate's LayerNorm and gate
// Every operand and accumulator is f32 on v_mfma_f32_16x16x4_f32, as in gemm_f32.hip: the k index inside a 16-wide block is
// permuted the same way for both operands (lane (f, kk) holds k = kb + 4 kk + s at step s).  Rows of a tail chunk beyond T
// are loaded as zeros, never read.
//
// Depthwise-conv cache.  dwconv_frame's fma chain per (frame, channel), the taps read from (old cache ++ x) instead of a
// shifted cache; a second launch writes the new cache, so no thread reads a cache row another one has rewritten.
#include <limits.h>

#include "common.h"
#include "kernels.h"
#include "ls_rows.h"

namespace {

constexpr int LD = 68;                 // LDS row stride in floats: 64 + 4, so the float4 fragment reads of 16 rows spread over the banks
constexpr int TILE = 64 * LD;          // one 64 x 64 f32 tile

// 64 rows x 64 floats from src (row stride ld floats) into an LDS tile; rows from nrows on are zeros and are not read.
DEV void load_tile(float* __restrict__ dst, const float* __restrict__ src, size_t ld, int nrows) {
    for (int e = threadIdx.x; e < 1024; e += 256) {
        const int r = e >> 4, c4 = (e & 15) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < nrows) v = *(const float4*)(src + (size_t)r * ld + c4);
        *(float4*)(dst + r * LD + c4) = v;
    }
}

DEV float comp(const float4& v, int s) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; }

// item = (i*H + h)*nchunk + c: chunk c of head h of call sequence i
struct Item {
    int c, h, i, nrows;
    size_t row0;                       // first row of the chunk in qkvg / out
};
DEV Item decode_item(int item, int H, int T, int nchunk) {
    Item it;
    it.c = item % nchunk;
    const int sh = item / nchunk;
    it.h = sh % H;
    it.i = sh / H;
    it.nrows = T - 64 * it.c < 64 ? T - 64 * it.c : 64;
    it.row0 = (size_t)it.i * T + (size_t)64 * it.c;
    return it;
}

// P_c[a][b] = sum_i v_i[a] k_i[b] over the frames of the chunk -> ws[item][a][b].  Wave w owns a = 16 w .. 16 w + 15.
__global__ __launch_bounds__(256)
void ret_prefill_sums_kernel(const float* __restrict__ qkvg, float* __restrict__ ws, int H, int T, int nchunk) {
    extern __shared__ float lds[];
    float* Ks = lds;
    float* Vs = lds + TILE;
    const Item it = decode_item(blockIdx.x, H, T, nchunk);
    const int D = H * 64;
    const float* row = qkvg + it.row0 * 4 * D + it.h * 64;
    load_tile(Ks, row + D, (size_t)4 * D, it.nrows);
    load_tile(Vs, row + 2 * D, (size_t)4 * D, it.nrows);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f = lane & 15, kk = lane >> 4;
    f32x4 acc[4];
#pragma unroll
    for (int bt = 0; bt < 4; ++bt) acc[bt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < 64; kb += 16)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = kb + 4 * kk + s;                     // the frame this lane feeds at this step
            const float vb = Vs[j * LD + 16 * wave + f];
#pragma unroll
            for (int bt = 0; bt < 4; ++bt)                     // D[b = 16 bt + 4 kk + r][a = 16 wave + f] += k_j[b] v_j[a]
                acc[bt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ks[j * LD + 16 * bt + f], vb, acc[bt], 0, 0, 0);
        }
    float* P = ws + (size_t)blockIdx.x * 4096 + (16 * wave + f) * 64 + 4 * kk;
#pragma unroll
    for (int bt = 0; bt < 4; ++bt) *(float4*)(P + 16 * bt) = make_float4(acc[bt][0], acc[bt][1], acc[bt][2], acc[bt][3]);
}

// The exclusive prefix over a (sequence, head)'s chunk sums, in chunk order, and the new state.  One thread per four state
// elements; t0 == 0: the old state is not read.
__global__ __launch_bounds__(256)
void ret_prefill_scan_kernel(float* __restrict__ ws, float* __restrict__ kv, int seq0, int H, int nchunk, int t0, int T) {
    const size_t e4 = (size_t)blockIdx.x * 256 + threadIdx.x;  // (i*H + h)*1024 + float4 index: the grid is exact
    const size_t sh = e4 >> 10;
    const int e = (int)(e4 & 1023) * 4;
    float* st = kv + ((size_t)seq0 * H + sh) * 4096 + e;
    float4 run = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t0 > 0) {
        const float s = (float)__builtin_sqrt((double)t0);
        const float4 o = *(const float4*)st;
        run = make_float4(o.x * s, o.y * s, o.z * s, o.w * s);
    }
    float* p = ws + sh * nchunk * 4096 + e;
    for (int c = 0; c < nchunk; ++c, p += 4096) {
        const float4 pc = *(const float4*)p;
        *(float4*)p = run;
        run.x += pc.x; run.y += pc.y; run.z += pc.z; run.w += pc.w;
    }
    const float d = (float)__builtin_sqrt((double)t0 + (double)T);
    *(float4*)st = make_float4(run.x / d, run.y / d, run.z / d, run.w / d);
}

// The outputs of one chunk.  Wave w owns frames i = 16 w .. 16 w + 15 of the chunk and all 64 values a of the head, so the
// per-head LayerNorm stays inside the wave.  The scores come out of their MFMA as D[j = 16 jt + 4 kk + r][i = 16 w + f], which
// is the B operand the (scores V) MFMA wants at step r of key block jt: they go from registers to registers.
__global__ __launch_bounds__(256)
void ret_prefill_out_kernel(const float* __restrict__ qkvg, const float* __restrict__ ws, _Float16* __restrict__ out16,
                            float* __restrict__ out32, int H, int T, int nchunk, int t0, float eps) {
    extern __shared__ float lds[];
    float* Qs = lds;
    float* Ks = lds + TILE;
    float* Vs = lds + 2 * TILE;
    float* Ss = lds + 3 * TILE;
    const Item it = decode_item(blockIdx.x, H, T, nchunk);
    const int D = H * 64;
    const float* row = qkvg + it.row0 * 4 * D + it.h * 64;
    load_tile(Qs, row, (size_t)4 * D, it.nrows);
    load_tile(Ks, row + D, (size_t)4 * D, it.nrows);
    load_tile(Vs, row + 2 * D, (size_t)4 * D, it.nrows);
    load_tile(Ss, ws + (size_t)blockIdx.x * 4096, 64, 64);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f = lane & 15, kk = lane >> 4;
    const int i = 16 * wave + f;                               // this lane's frame of the chunk (B operand / D column)
    float4 q4[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) q4[kb] = *(const float4*)(Qs + i * LD + 16 * kb + 4 * kk);
    // acc[at]: D[a = 16 at + 4 kk + r][i] = sum_b S_c[a][b] q_i[b]
    f32x4 acc[4];
#pragma unroll
    for (int at = 0; at < 4; ++at) {
        acc[at] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const float4 s4 = *(const float4*)(Ss + (16 * at + f) * LD + 16 * kb + 4 * kk);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[at] = __builtin_amdgcn_mfma_f32_16x16x4f32(comp(s4, s), comp(q4[kb], s), acc[at], 0, 0, 0);
        }
    }
    // key blocks jt <= wave (the later ones are wholly masked): sc = D[j = 16 jt + 4 kk + r][i] = k_j . q_i, kept where j <= i
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
        if (jt > wave) break;
        f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const float4 k4 = *(const float4*)(Ks + (16 * jt + f) * LD + 16 * kb + 4 * kk);
#pragma unroll
            for (int s = 0; s < 4; ++s) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(comp(k4, s), comp(q4[kb], s), sc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = 16 * jt + 4 * kk + r;
            const float p = j <= i ? sc[r] : 0.f;
#pragma unroll
            for (int at = 0; at < 4; ++at)                     // D[a][i] += v_j[a] p[i][j]
                acc[at] = __builtin_amdgcn_mfma_f32_16x16x4f32(Vs[j * LD + 16 * at + f], p, acc[at], 0, 0, 0);
        }
    }
    // 1 / sqrt(t + 1) of the frame, the per-head LayerNorm over a (16 values here, the rest in lanes f + 16 / 32 / 48), the gate
    float keep, add;
    ret_scale_factors((float)(t0 + 64 * it.c + i), keep, add);
    float sum = 0.f;
#pragma unroll
    for (int at = 0; at < 4; ++at)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            acc[at][r] *= add;
            sum += acc[at][r];
        }
    sum = wave_xor_add(wave_xor_add(sum, 16), 32);
    const float mean = sum * (1.0f / 64.0f);
    float var = 0.f;
#pragma unroll
    for (int at = 0; at < 4; ++at)
#pragma unroll
        for (int r = 0; r < 4; ++r) var += (acc[at][r] - mean) * (acc[at][r] - mean);
    var = wave_xor_add(wave_xor_add(var, 16), 32);
    const float rstd = 1.0f / __builtin_sqrtf(var * (1.0f / 64.0f) + eps);
    if (i >= it.nrows) return;
    const size_t orow = it.row0 + i;
    const float* grow = qkvg + orow * 4 * D + 3 * D + it.h * 64 + 4 * kk;
#pragma unroll
    for (int at = 0; at < 4; ++at) {
        const float4 g = *(const float4*)(grow + 16 * at);
        float y[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float gg = comp(g, r);
            y[r] = gg / (1.0f + __expf(-gg)) * ((acc[at][r] - mean) * rstd);
        }
        const size_t o = orow * D + it.h * 64 + 16 * at + 4 * kk;
        if (out32) *(float4*)(out32 + o) = make_float4(y[0], y[1], y[2], y[3]);
        if (out16) *(f16x4*)(out16 + o) = f16x4{to_f16_sat(y[0]), to_f16_sat(y[1]), to_f16_sat(y[2]), to_f16_sat(y[3])};
    }
}

// Frame i, channel ch of slot b: tap j of the frame is entry i + j of (old cache ++ x), the chain dwconv_frame's.
__global__ __launch_bounds__(256)
void dwconv_prefill_kernel(const _Float16* __restrict__ x, const float* __restrict__ cache, int fresh, const float* __restrict__ w,
                           const float* __restrict__ bw, const float* __restrict__ bb, const float* __restrict__ bm,
                           const float* __restrict__ bv, float eps, _Float16* __restrict__ out, int T, int D, int k) {
#pragma clang fp contract(off)
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)T * D) return;
    const int i = (int)(idx / D), ch = (int)(idx - (size_t)i * D);
    const float sc = bw[ch] / __builtin_sqrtf(bv[ch] + eps);
    const float m = bm[ch], be = bb[ch];
    const float* cc = cache + (size_t)ch * (k - 1);
    const float* wc = w + (size_t)ch * k;
    float y = wc[k - 1] * (float)x[idx];
    for (int j = k - 2; j >= 0; --j) {
        const int e = i + j;                                   // entry of (old cache ++ x)
        const float cur = e >= k - 1 ? (float)x[(size_t)(e - (k - 1)) * D + ch] : fresh ? 0.f : cc[e];
        y = __builtin_fmaf(wc[j], cur, y);
    }
    y = __builtin_fmaf(y - m, sc, be);
    out[idx] = to_f16_sat(y / (1.0f + __expf(-y)));
}

// The new cache of slot b: the last k - 1 entries of (old cache ++ x).  One thread per channel walks its row upwards: entry j
// comes from entry T + j > j of the old row (or from x), which this thread has not written yet.
__global__ __launch_bounds__(256)
void dwconv_prefill_cache_kernel(const _Float16* __restrict__ x, float* __restrict__ cache, int fresh, int T, int D, int k) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= D) return;
    float* cc = cache + (size_t)ch * (k - 1);
    for (int j = 0; j < k - 1; ++j) {
        const long e = (long)T + j;
        cc[j] = e >= k - 1 ? (float)x[(size_t)(e - (k - 1)) * D + ch] : fresh ? 0.f : cc[e];
    }
}

EendOncePerDevice g_out_lds;

}  // namespace

long eend_ret_prefill_ws_floats(int Nseq, int H, int T) { return (long)Nseq * H * ((T + 63) / 64) * 4096; }

int eend_launch_ret_prefill(const float* qkvg, float* kv, void* out16, float* out32, float* ws, long ws_floats, int Ncache, int seq0,
                            int Nseq, int H, int t0, int T, float eps, hipStream_t stream) {
    if (!qkvg || !kv || !ws || (!out16 && !out32) || (((size_t)qkvg | (size_t)kv | (size_t)ws | (size_t)out16 | (size_t)out32) & 15) ||
        T < 1 || t0 < 0 || t0 > INT_MAX - 64 - T || H < 1 || Nseq < 1 || seq0 < 0 || Ncache < 1 || seq0 > Ncache - Nseq)
        return EEND_EINVAL;
    const int nchunk = (T + 63) / 64;
    const long items = (long)Nseq * H * nchunk;
    if (items > 0x7fffffffL / 4 || ws_floats < eend_ret_prefill_ws_floats(Nseq, H, T)) return EEND_EINVAL;
    const int out_lds = 4 * TILE * (int)sizeof(float);
    if (!eend_set_dynamic_lds(g_out_lds, (const void*)ret_prefill_out_kernel, out_lds)) return EEND_ELAUNCH;
    hipLaunchKernelGGL(ret_prefill_sums_kernel, dim3((unsigned)items), dim3(256), 2 * TILE * sizeof(float), stream, qkvg, ws, H, T, nchunk);
    hipLaunchKernelGGL(ret_prefill_scan_kernel, dim3((unsigned)((long)Nseq * H * 4)), dim3(256), 0, stream, ws, kv, seq0, H, nchunk, t0, T);
    hipLaunchKernelGGL(ret_prefill_out_kernel, dim3((unsigned)items), dim3(256), out_lds, stream, qkvg, (const float*)ws,
                       (_Float16*)out16, out32, H, T, nchunk, t0, eps);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_dwconv_prefill(const void* x16, float* cache, int b, int t0, const float* w, const float* bn_w, const float* bn_b,
                               const float* bn_mean, const float* bn_var, float eps, void* out16, int T, int B, int D, int k,
                               hipStream_t stream) {
    if (!x16 || !cache || !w || !bn_w || !bn_b || !bn_mean || !bn_var || !out16 || T < 1 || t0 < 0 || B < 1 || b < 0 || b >= B || D < 1 ||
        k < 2 || (long)T * D > 0x7fffffffL - 255)
        return EEND_EINVAL;
    float* row = cache + (size_t)b * D * (k - 1);
    const int fresh = t0 == 0;
    hipLaunchKernelGGL(dwconv_prefill_kernel, dim3((unsigned)(((long)T * D + 255) / 256)), dim3(256), 0, stream, (const _Float16*)x16,
                       (const float*)row, fresh, w, bn_w, bn_b, bn_mean, bn_var, eps, (_Float16*)out16, T, D, k);
    hipLaunchKernelGGL(dwconv_prefill_cache_kernel, dim3((D + 255) / 256), dim3(256), 0, stream, (const _Float16*)x16, row, fresh, T, D, k);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
