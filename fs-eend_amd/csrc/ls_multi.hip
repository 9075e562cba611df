// Many LS-EEND streams in one frame step (LsMultiStreamSession, ls_multistream.py): S slots, each at its own stream position
// and with its own lifetime, advanced together by one graph replay per frame.  The kernels here are the state touches of the
// LS frame step made per slot: the recurrent retention step (whose scale is the slot's own position) and the Conformer's
// depthwise-conv cache (the f32 look-ahead window is window_push_kernel<float> of stream_multi.hip).  Every row computes
// every frame (fixed shapes for the captured graph); per-slot int32 lengths and masks in device memory decide what each row
// reads and which state changes.
#include "common.h"
#include "kernels.h"
#include "ls_rows.h"

namespace {

// MultiScaleRetention.recurrent_forward (LS-EEND/nnet/modules/retention.py:126-144, decay 1) + per-head LayerNorm + swish
// gate on f32 projections, as ret_step_kernel<float> of stream.hip, with the scale taken from the row's own sequence:
// row n belongs to sequence s = n / rows_per_seq, t = len[s] frames already in its state, so scale_{t} = t and
// scale_{t+1} = t + 1 (decay 1: the reference's running scale is the frame count, exactly representable up to 2^24).
//   mask[s] != 0, t >= 0: state updated in place, output row written.  t == 0 is an empty state: the old state is not read
//                         (a reused slot's leftovers, NaN included, cannot leak; keep = 0 times NaN would still be NaN).
//   otherwise:            state neither read nor written, output row = 0.
// The keep / add factors and the row update are the functions ret_step_kernel<float> calls (ls_rows.h), so a slot at position
// t is bit-identical to eend_retention_step_f32 with scale_in = t.  One wave per (n, h): lane a owns row kv[a][:].
__global__ __launch_bounds__(256)
void ret_step_ragged_kernel(const float* __restrict__ qkvg, float* __restrict__ kv, const int* __restrict__ len,
                            const int* __restrict__ mask, int rows_per_seq, _Float16* __restrict__ out, float* __restrict__ out32,
                            int N, int H, float eps) {
    const int lane = threadIdx.x & 63;
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);       // n*H + h
    if (idx >= N * H) return;
    const int n = idx / H, h = idx - n * H;
    const int D = H * 64;
    const int seq = n / rows_per_seq;
    const int t = __builtin_amdgcn_readfirstlane(len[seq]);
    const int on = __builtin_amdgcn_readfirstlane(mask[seq]);
    if (!on || t < 0) {                                        // paused / free slot: no state traffic
        if (out) out[(size_t)n * D + h * 64 + lane] = (_Float16)0.f;
        if (out32) out32[(size_t)n * D + h * 64 + lane] = 0.f;
        return;
    }
    const float* row = qkvg + (size_t)n * 4 * D;
    float keep, add;
    ret_scale_factors((float)t, keep, add);
    const float va = row[2 * D + h * 64 + lane] * add;
    float* st = kv + ((size_t)idx * 64 + lane) * 64;
    const float o = t == 0 ? ret_row_update<true>(st, row + D + h * 64, row + h * 64, keep, va)
                           : ret_row_update<false>(st, row + D + h * 64, row + h * 64, keep, va);
    const float r = ret_norm_gate(o, row[3 * D + h * 64 + lane], eps);
    if (out) out[(size_t)n * D + h * 64 + lane] = to_f16_sat(r);
    if (out32) out32[(size_t)n * D + h * 64 + lane] = r;
}

// ConformerConvModule.forward_one_step, depthwise part (conformer/convolution.py:157-163), per slot: as dwconv_step_kernel of
// stream.hip for the slots with mask[b] != 0 (cache [b][c][k-1] shifted in place); len[b] == 0 reads the cache as zeros (the
// driver's zero-initialised conv_caches, LS-EEND/streaming_infer_dia.py:40-45) and overwrites it.  mask[b] == 0: the cache is
// left as it is and the output row is zero.  A thread owns one channel of one slot.
__global__ __launch_bounds__(256)
void dwconv_step_ragged_kernel(const _Float16* __restrict__ x, float* __restrict__ cache, const int* __restrict__ len,
                               const int* __restrict__ mask, const float* __restrict__ w, const float* __restrict__ bw,
                               const float* __restrict__ bb, const float* __restrict__ bm, const float* __restrict__ bv, float eps,
                               _Float16* __restrict__ out, int B, int D, int k) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;       // b*D + c
    if (i >= B * D) return;
    const int b = i / D, c = i - b * D;
    const int t = len[b];
    if (!mask[b] || t < 0) {
        out[i] = (_Float16)0.f;
        return;
    }
    const float sc = bw[c] / __builtin_sqrtf(bv[c] + eps);
    const float y = dwconv_frame(cache + (size_t)i * (k - 1), w + (size_t)c * k, (float)x[i], t == 0, k, bm[c], sc, bb[c]);
    out[i] = to_f16_sat(y);
}

}  // namespace

int eend_launch_ret_step_ragged(const float* qkvg, float* kv, const int* len, const int* mask, int rows_per_seq, void* out16, float* out32,
                                int N, int H, float eps, hipStream_t stream) {
    if (!qkvg || !kv || !len || !mask || (!out16 && !out32) || N <= 0 || H <= 0 || rows_per_seq <= 0 || N % rows_per_seq ||
        (long)N * H > 0x7fffffffL - 3)
        return EEND_EINVAL;
    hipLaunchKernelGGL(ret_step_ragged_kernel, dim3((N * H + 3) / 4), dim3(256), 0, stream, qkvg, kv, len, mask, rows_per_seq,
                       (_Float16*)out16, out32, N, H, eps);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_dwconv_step_ragged(const void* x16, float* cache, const int* len, const int* mask, const float* w, const float* bn_w,
                                   const float* bn_b, const float* bn_mean, const float* bn_var, float eps, void* out16, int B, int D,
                                   int k, hipStream_t stream) {
    if (!x16 || !cache || !len || !mask || !w || !bn_w || !bn_b || !bn_mean || !bn_var || !out16 || B <= 0 || D <= 0 || k < 2 ||
        (long)B * D > 0x7fffffffL - 255)
        return EEND_EINVAL;
    hipLaunchKernelGGL(dwconv_step_ragged_kernel, dim3((B * D + 255) / 256), dim3(256), 0, stream, (const _Float16*)x16, cache, len, mask,
                       w, bn_w, bn_b, bn_mean, bn_var, eps, (_Float16*)out16, B, D, k);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
