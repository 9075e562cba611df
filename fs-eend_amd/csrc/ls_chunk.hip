// Many frames per slot in one LS-EEND multi-stream step (LsMultiStreamSession with max_frames = n, ls_multistream.py): the
// state touches of ls_multi.hip over a chunk.  Slot s takes cnt[s] (0..nmax) frames in one launch; its rows are the first
// cnt[s] of its nmax rows, the others come out as zeros and touch no state.  Each kernel walks the frames of a chunk in order
// with the per-frame arithmetic of ls_rows.h, so a chunk of c frames is bit for bit c one-frame calls.
#include "common.h"
#include "kernels.h"
#include "ls_rows.h"

namespace {

// ret_step_ragged_kernel over a chunk.  Sequence q (slot s = q / seq_per_slot: 1 sequence per slot in the encoder, C in the
// decoder) owns rows q*nmax .. q*nmax + nmax - 1 of qkvg / out; with t = len[s] and c = cnt[s] its first c rows are frames
// t .. t + c - 1.  One wave per (q, h), lane a owns state row kv[a][:] and keeps it in registers (64 VGPRs) across the chunk:
// the state is read once (not at all when t == 0: an empty state, whatever the memory holds) and written once; c == 0 (or a
// negative length, or a count outside 0..nmax) neither reads nor writes it.  k and q of a frame are the same for every lane
// of the wave (uniform addresses).
__global__ __launch_bounds__(256)
void ret_chunk_ragged_kernel(const float* __restrict__ qkvg, float* __restrict__ kv, const int* __restrict__ len,
                             const int* __restrict__ cnt, int seq_per_slot, int nmax, _Float16* __restrict__ out,
                             float* __restrict__ out32, int Nseq, int H, float eps) {
    const int lane = threadIdx.x & 63;
    const int idx = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);       // q*H + h
    if (idx >= Nseq * H) return;
    const int q = idx / H, h = idx - q * H;
    const int D = H * 64;
    const int slot = q / seq_per_slot;
    const int t = __builtin_amdgcn_readfirstlane(len[slot]);
    int c = __builtin_amdgcn_readfirstlane(cnt[slot]);
    if (t < 0 || c < 0 || c > nmax) c = 0;
    const size_t r0 = (size_t)q * nmax;
    if (c > 0) {
        float* st = kv + ((size_t)idx * 64 + lane) * 64;
        float4 s[16];
        if (t == 0) {
#pragma unroll
            for (int b = 0; b < 16; ++b) s[b] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
#pragma unroll
            for (int b = 0; b < 16; ++b) s[b] = *(const float4*)(st + b * 4);
        }
        for (int j = 0; j < c; ++j) {
            const float* row = qkvg + (r0 + j) * 4 * D;
            float keep, add;
            ret_scale_factors((float)(t + j), keep, add);
            const float va = row[2 * D + h * 64 + lane] * add;
            const float o = ret_row_update_reg(s, row + D + h * 64, row + h * 64, keep, va);
            const float r = ret_norm_gate(o, row[3 * D + h * 64 + lane], eps);
            if (out) out[(r0 + j) * D + h * 64 + lane] = to_f16_sat(r);
            if (out32) out32[(r0 + j) * D + h * 64 + lane] = r;
        }
#pragma unroll
        for (int b = 0; b < 16; ++b) *(float4*)(st + b * 4) = s[b];
    }
    for (int j = c; j < nmax; ++j) {
        if (out) out[(r0 + j) * D + h * 64 + lane] = (_Float16)0.f;
        if (out32) out32[(r0 + j) * D + h * 64 + lane] = 0.f;
    }
}

// dwconv_step_ragged_kernel over a chunk: slot b takes the first cnt[b] of its rows x[b*nmax + j] through its cache in order.
// A thread owns one channel of one slot; the cache row (k - 1 floats) stays in this thread's cache lines between frames.
__global__ __launch_bounds__(256)
void dwconv_chunk_ragged_kernel(const _Float16* __restrict__ x, float* __restrict__ cache, const int* __restrict__ len,
                                const int* __restrict__ cnt, int nmax, const float* __restrict__ w, const float* __restrict__ bw,
                                const float* __restrict__ bb, const float* __restrict__ bm, const float* __restrict__ bv, float eps,
                                _Float16* __restrict__ out, int B, int D, int k) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;       // b*D + ch
    if (i >= B * D) return;
    const int b = i / D, ch = i - b * D;
    const int t = len[b];
    int c = cnt[b];
    if (t < 0 || c < 0 || c > nmax) c = 0;
    const size_t r0 = (size_t)b * nmax * D + ch;
    if (c > 0) {
        const float sc = bw[ch] / __builtin_sqrtf(bv[ch] + eps);
        const float m = bm[ch], be = bb[ch];
        float* cc = cache + (size_t)i * (k - 1);
        const float* wc = w + (size_t)ch * k;
        for (int j = 0; j < c; ++j) {
            const float y = dwconv_frame(cc, wc, (float)x[r0 + (size_t)j * D], t == 0 && j == 0, k, m, sc, be);
            out[r0 + (size_t)j * D] = to_f16_sat(y);
        }
    }
    for (int j = c; j < nmax; ++j) out[r0 + (size_t)j * D] = (_Float16)0.f;
}

// Speaker-axis attention in f32 (self_attn2 of the LS decoder layer, merge_retnet_layer.py:300-307, inside the all-f32 decoder
// frame step; eend_launch_spk_attn_step_f32 of stream.hip is this kernel at Tp = 1) on decoder slabs: qkv f32
// [(b*C + c)*Tp + t][768] = [q | k | v] (head h at column h*64), out f32 [(b*C + c)*Tp + t][256]; the C rows of frame (b, t)
// attend to each other.  One wave per (row, head); lane = head dimension; C <= 16 scores per wave.
__global__ __launch_bounds__(64)
void spk_attn_rows_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int C, int Tp, float scale) {
    const int lane = threadIdx.x, row = blockIdx.x, h = blockIdx.y;
    const int b = row / (C * Tp), t = row % Tp;
    const size_t b0 = (size_t)b * C * Tp + t;                   // row of speaker 0 of this frame; speaker c is Tp*c rows on
    const float q = qkv[(size_t)row * 768 + h * 64 + lane] * scale;
    float sc[16];
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        float d = 0.f;
        if (c < C) {
            d = q * qkv[(b0 + (size_t)c * Tp) * 768 + 256 + h * 64 + lane];
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) d = wave_xor_add(d, m);
            mx = __builtin_fmaxf(mx, d);
        }
        sc[c] = d;
    }
    float den = 0.f, o = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c)
        if (c < C) {
            const float pr = __expf(sc[c] - mx);
            den += pr;
            o = __builtin_fmaf(pr, qkv[(b0 + (size_t)c * Tp) * 768 + 512 + h * 64 + lane], o);
        }
    out[(size_t)row * 256 + h * 64 + lane] = o / den;
}

}  // namespace

int eend_launch_ret_chunk_ragged(const float* qkvg, float* kv, const int* len, const int* cnt, int seq_per_slot, int nmax, void* out16,
                                 float* out32, int Nseq, int H, float eps, hipStream_t stream) {
    if (!qkvg || !kv || !len || !cnt || (!out16 && !out32) || Nseq <= 0 || H <= 0 || seq_per_slot <= 0 || Nseq % seq_per_slot ||
        nmax < 1 || nmax > 64 || (long)Nseq * H > 0x7fffffffL - 3 || (long)Nseq * nmax * 4 * H * 64 > 0x7fffffffL)
        return EEND_EINVAL;
    hipLaunchKernelGGL(ret_chunk_ragged_kernel, dim3((Nseq * H + 3) / 4), dim3(256), 0, stream, qkvg, kv, len, cnt, seq_per_slot, nmax,
                       (_Float16*)out16, out32, Nseq, H, eps);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_dwconv_chunk_ragged(const void* x16, float* cache, const int* len, const int* cnt, int nmax, const float* w,
                                    const float* bn_w, const float* bn_b, const float* bn_mean, const float* bn_var, float eps, void* out16,
                                    int B, int D, int k, hipStream_t stream) {
    if (!x16 || !cache || !len || !cnt || !w || !bn_w || !bn_b || !bn_mean || !bn_var || !out16 || B <= 0 || D <= 0 || k < 2 ||
        nmax < 1 || nmax > 64 || (long)B * D > 0x7fffffffL - 255 || (long)B * nmax * D > 0x7fffffffL)
        return EEND_EINVAL;
    hipLaunchKernelGGL(dwconv_chunk_ragged_kernel, dim3((B * D + 255) / 256), dim3(256), 0, stream, (const _Float16*)x16, cache, len, cnt,
                       nmax, w, bn_w, bn_b, bn_mean, bn_var, eps, (_Float16*)out16, B, D, k);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_spk_attn_rows_f32(const float* qkv, float* out, int B, int C, int Tp, float scale, hipStream_t stream) {
    if (!qkv || !out || B <= 0 || C <= 0 || C > 16 || Tp < 1 || (long)B * C * Tp > 0x7fffffffL / 768) return EEND_EINVAL;
    hipLaunchKernelGGL(spk_attn_rows_f32_kernel, dim3(B * C * Tp, 4), dim3(64), 0, stream, qkv, out, C, Tp, scale);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
