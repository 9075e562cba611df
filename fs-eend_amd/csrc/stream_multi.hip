// Many FS-EEND streams in one frame step (FsMultiStreamSession, fs_multistream.py): S slots, each with its own K/V
// history length and its own lifetime, advanced together by one graph replay per frame.  The kernels here are the pieces
// whose state is per slot: the decode attention over ragged histories, the masked history counters and the look-ahead
// window push.  Every row computes every frame (fixed shapes for the captured graph); a per-slot mask in device memory
// decides which state changes.
#include "common.h"
#include "kernels.h"
#include "decode_tile.h"

namespace {

// ---- decode attention over ragged histories (FS-EEND/nnet/modules/streaming_tfm.py:15-37, one new token per row).
// Key-split form ("flash decoding") as attn_decode_split_kernel of stream.hip, on the same steps (decode_tile.h), with
// per-sequence lengths and append masks:
// row n belongs to sequence s = n / rows_per_seq (1 for encoder layers, C for decoder layers); t = len[s].
//   mask[s] != 0 and t < cap: append the new k / v at row t, attend over t + 1 tokens;
//   otherwise: caches untouched, output row = 0.
// The 512-key blocks are anchored at key 0 and the merge walks ceil(t / 512) partials, so a row's result depends on its
// own history only -- not on cap, not on the other rows, not on the row's position (the slot-invariance of the session).
// Grid = (N*H, cap / DT_R), fixed per cache capacity; blocks whose key range starts at or beyond t exit at once.
// Per 64-key chunk of a wave: scores with lane = key (one 128-B K row per lane); P.V with lane = (row group r = lane / 8,
// dims 8 * (lane % 8) ..+7): one 16-B V load per lane covers 8 rows per instruction, and the 8 row groups are summed once
// at the end of the wave's range instead of per chunk.
__global__ __launch_bounds__(256)
void attn_decode_ragged_kernel(const _Float16* __restrict__ qkv, _Float16* __restrict__ Kc, _Float16* __restrict__ Vc,
                               float* __restrict__ part, int H, int cap, int nsplit, int rows_per_seq,
                               const int* __restrict__ len, const int* __restrict__ mask, float scale) {
    __shared__ float red[4][DT_PART];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int idx = blockIdx.x, sp = blockIdx.y;
    const int n = idx / H, h = idx - n * H;
    const int seq = n / rows_per_seq;
    const int t = __builtin_amdgcn_readfirstlane(len[seq]);
    const int on = __builtin_amdgcn_readfirstlane(mask[seq]);
    const int k0 = sp * DT_R;
    const int D = H * 64;
    const _Float16* row = qkv + (size_t)n * 3 * D + h * 64;
    _Float16* Kh = Kc + (size_t)idx * cap * 64;
    _Float16* Vh = Vc + (size_t)idx * cap * 64;
    if (!on || t >= cap || t < 0 || k0 >= t) {
        if (on && t >= 0 && t < cap && sp == 0 && wave == 0) decode_append(Kh, Vh, t, row, D, lane);      // t == 0: only the append
        return;                                                     // the merge reads no partial of this block
    }
    if (sp == 0 && wave == 0) decode_append(Kh, Vh, t, row, D, lane);      // row t is never read back in this launch
    const int k1 = k0 + DT_R < t ? k0 + DT_R : t;
    float qf[64];
    decode_q_scaled(qf, row, scale);
    const int rg = lane >> 3, dq = (lane & 7) * 8;
    float m_run = -INFINITY, l_run = 0.f;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
    for (int c0 = k0 + wave * 64; c0 < k1; c0 += 256) {
        const int key = c0 + lane;
        const float s = key < k1 ? decode_score(qf, Kh + (size_t)key * 64) : -INFINITY;
        f16x8 v8[8];                                                // issued before the softmax reductions: in flight meanwhile
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int kv = c0 + rg + 8 * i;
            if (kv < k1) v8[i] = *(const f16x8*)(Vh + (size_t)kv * 64 + dq);
            else v8[i] = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};             // stale rows beyond t may hold anything: never read
        }
        float alpha;
        const float p = decode_softmax_chunk(s, m_run, l_run, alpha);      // 0 for key >= k1
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] *= alpha;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float pj = __shfl(p, rg + 8 * i, 64);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = __builtin_fmaf(pj, (float)v8[i][e], o[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {                                   // sum the 8 row groups: lanes l, l^8, l^16, ... hold dims dq..dq+7
        o[e] = wave_xor_add(o[e], 8);
        o[e] = wave_xor_add(o[e], 16);
        o[e] = wave_xor_add(o[e], 32);
    }
    if (lane < 8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[wave][dq + e] = o[e];
    }
    if (lane == 0) { red[wave][64] = m_run; red[wave][65] = l_run; }
    __syncthreads();
    if (wave == 0) decode_combine4<false>(&red[0][0], DT_PART, lane, part + ((size_t)idx * nsplit + sp) * DT_PART);
}

__global__ __launch_bounds__(64)
void attn_decode_ragged_merge_kernel(const _Float16* __restrict__ qkv, const float* __restrict__ part, _Float16* __restrict__ out,
                                     int H, int cap, int nsplit, int rows_per_seq, const int* __restrict__ len,
                                     const int* __restrict__ mask, float scale) {
    const int lane = threadIdx.x, idx = blockIdx.x;
    const int n = idx / H, h = idx - n * H;
    const int seq = n / rows_per_seq;
    const int t = __builtin_amdgcn_readfirstlane(len[seq]);
    const int on = __builtin_amdgcn_readfirstlane(mask[seq]);
    const int D = H * 64;
    if (!on || t < 0 || t >= cap) {
        out[(size_t)n * D + h * 64 + lane] = (_Float16)0.f;
        return;
    }
    const _Float16* row = qkv + (size_t)n * 3 * D + h * 64;
    float M = decode_self_score(row, D, lane, scale), L = 1.0f, O = (float)row[2 * D + lane];
    decode_walk<false, false>(M, L, O, part + (size_t)idx * nsplit * DT_PART, DT_PART, (t + DT_R - 1) / DT_R, lane);
    out[(size_t)n * D + h * 64 + lane] = to_f16_sat(O / L);
}

// len[s] += mask[s] for all s (the graph's own per-slot "t += 1").
__global__ __launch_bounds__(256)
void counter_add_masked_kernel(int* __restrict__ len, const int* __restrict__ mask, int S) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S && mask[s]) len[s] += 1;
}

// The look-ahead window of each slot ([S][k*D] of T, [tap*D + c], oldest tap first; T = f16 for FS-EEND, f32 for the all-f32
// LS frame step): mode 1 shifts it by one frame and appends x[s] (f32 -> T, round to nearest even as a tensor cast), mode 2
// shifts and appends zeros (the reference driver's dummy_conv_input / flushing frames), any other mode leaves the slot alone.
// A thread owns one channel of one slot.
template <typename T>
__global__ __launch_bounds__(256)
void window_push_kernel(T* __restrict__ win, const float* __restrict__ x, const int* __restrict__ mode, int S, int k, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * D) return;
    const int s = i / D, c = i - s * D;
    const int m = mode[s];
    if (m != 1 && m != 2) return;
    T* w = win + (size_t)s * k * D + c;
    for (int j = 0; j + 1 < k; ++j) w[(size_t)j * D] = w[(size_t)(j + 1) * D];
    w[(size_t)(k - 1) * D] = m == 1 ? (T)x[i] : (T)0.f;
}

}  // namespace

int eend_launch_attn_decode_ragged(const void* qkv, void* Kc, void* Vc, void* out16, float* part, long part_floats, int N, int H, int cap,
                                   int rows_per_seq, const int* len, const int* mask, float scale, hipStream_t stream) {
    if (!qkv || !Kc || !Vc || !out16 || !part || !len || !mask || N <= 0 || H <= 0 || cap <= 0 || rows_per_seq <= 0 || N % rows_per_seq)
        return EEND_EINVAL;
    const int nsplit = decode_nsplit(cap);
    if (nsplit > 65535 || (long)N * H > 0x7fffffffL || part_floats < decode_ws_floats(N, H, cap, 1)) return EEND_EINVAL;
    hipLaunchKernelGGL(attn_decode_ragged_kernel, dim3(N * H, nsplit), dim3(256), 0, stream, (const _Float16*)qkv, (_Float16*)Kc,
                       (_Float16*)Vc, part, H, cap, nsplit, rows_per_seq, len, mask, scale);
    if (hipGetLastError() != hipSuccess) return EEND_ELAUNCH;
    hipLaunchKernelGGL(attn_decode_ragged_merge_kernel, dim3(N * H), dim3(64), 0, stream, (const _Float16*)qkv, (const float*)part,
                       (_Float16*)out16, H, cap, nsplit, rows_per_seq, len, mask, scale);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_counter_add_masked(int* len, const int* mask, int S, hipStream_t stream) {
    if (!len || !mask || S <= 0) return EEND_EINVAL;
    hipLaunchKernelGGL(counter_add_masked_kernel, dim3((S + 255) / 256), dim3(256), 0, stream, len, mask, S);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_window_push(void* win16, const float* x, const int* mode, int S, int k, int D, hipStream_t stream) {
    if (!win16 || !x || !mode || S <= 0 || k < 1 || D <= 0 || (long)S * D > 0x7fffffffL) return EEND_EINVAL;
    hipLaunchKernelGGL(window_push_kernel<_Float16>, dim3((S * D + 255) / 256), dim3(256), 0, stream, (_Float16*)win16, x, mode, S, k, D);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_window_push_f32(float* win, const float* x, const int* mode, int S, int k, int D, hipStream_t stream) {
    if (!win || !x || !mode || S <= 0 || k < 1 || D <= 0 || (long)S * D > 0x7fffffffL - 255) return EEND_EINVAL;
    hipLaunchKernelGGL(window_push_kernel<float>, dim3((S * D + 255) / 256), dim3(256), 0, stream, win, x, mode, S, k, D);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
