// The attractor path of the offline EEND-EDA baseline (FS-EEND/nnet/model/offl_tfm_enc_lstm_enc_dec.py:79-107): a single-layer
// LSTM recurrence (eend_lstm_f32, eend_lstm_orders_f32), the attractor-existence counter with the speaker count taken from it (eend_eda_count_f32) and the
// embedding . attractor head (eend_eda_head_f32).  The contracts are in include/eend_hip.h; DESIGN 12 has the reasoning and the times.
//
// eend_lstm_f32.  One workgroup of 16 waves owns one sequence from its first step to its last; workgroups never talk to each other
// (no flags, no spins, no cooperative launch) and every loop is bounded by T.  W_hh stays f32 in global memory and is re-read from L2
// every step (1 MiB; an XCD's L2 is 4 MiB): the f32 copy is the only one that holds the recurrence to a summation-order distance of
// torch's fp32 LSTM, and an f16 copy fits on chip only split between registers and LDS with about 32 working registers per lane.
//
// A step: wave w owns hidden units 16 w .. 16 w + 15, that is 64 gate rows (4 gates x 16 units).  A row of W_hh is 1 KiB = one
// coalesced float4 load per lane; lane l multiplies it with h[4 l .. 4 l + 3] (four registers, read from LDS once per step) into one
// partial per row.  The 64 partials of a lane are then reduced ACROSS lanes and scattered in one butterfly of 63 exchanges (halves
// 32, 16, .. 1: a lane keeps the half of its values whose row has its own lane bit and sends the other half), after which lane l holds
// the full dot product of row l of the wave: gate l / 16 of unit 16 w + l % 16.  Three more exchanges bring a unit's four gates to
// lanes 0 .. 15, which keep c in a register, apply the gate functions and write h to the other half of a double-buffered LDS row:
// one workgroup barrier per step.  The order of every sum is fixed by (row, lane) alone, so a sequence's bits do not depend on its
// batch mates or on the run.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int LH = LSTM_HIDDEN;         // 256
constexpr int LG = 4 * LSTM_HIDDEN;     // gate rows, PyTorch order i, f, g, o
constexpr int LNT = 1024;               // 16 waves x 64 rows = the 1024 gate rows
constexpr int LOADS_IN_FLIGHT = 8;      // row pairs per load batch: 16 float4 loads = 64 of a lane's 128 registers

typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

// finite for every finite x: exp overflows to +inf only where 1 / (1 + inf) = 0 is the limit
DEV float lstm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(LNT) void lstm_seq_kernel(const float* __restrict__ G, int g_rows, const int* __restrict__ order,
                                                       const float* __restrict__ bias, const float* __restrict__ Whh,
                                                       const float* __restrict__ h0, const float* __restrict__ c0,
                                                       float* __restrict__ hT, float* __restrict__ cT, float* __restrict__ h_all, int T,
                                                       int order_stride) {
    __shared__ __attribute__((aligned(16))) float hbuf[2][LH];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (order) order += (size_t)b * order_stride;                 // 0: one order for the batch, T: one per sequence
    const int unit = wave * 16 + (lane & 15);
    const int my_row = (lane >> 4) * LH + unit;                  // the gate row this lane holds after the butterfly
    if (threadIdx.x < LH) hbuf[0][threadIdx.x] = h0 ? h0[(size_t)b * LH + threadIdx.x] : 0.f;
    float c = 0.f, h = 0.f;
    if (lane < 16) {
        c = c0 ? c0[(size_t)b * LH + unit] : 0.f;
        h = h0 ? h0[(size_t)b * LH + unit] : 0.f;
    }
    const float bias_r = G ? 0.f : bias[my_row];                  // zero input: the pre-activation is the bias sum alone
    const float* Gb = G ? G + (size_t)b * g_rows * LG + my_row : nullptr;
    // a wave-uniform row base in scalar registers plus one 32-bit lane offset: 64 per-lane row addresses would take every register
    // (typed as global memory: a pointer that went through the asm below would otherwise be loaded from with flat instructions)
    const gfloat* wwave = (const gfloat*)Whh + (size_t)__builtin_amdgcn_readfirstlane(wave) * 16 * LH;
    const unsigned loff = lane * 4;
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const int cur = t & 1;
        float pre = bias_r;
        if (Gb) {                                                 // issued first: lands behind the weight stream
            int o = order ? order[t] : t;
            o = o < 0 ? 0 : (o >= T ? T - 1 : o);                 // the host validates the permutation; never read outside G
            pre = Gb[(size_t)o * LG];
        }
        const f32x4 hv = *(const f32x4*)&hbuf[cur][lane * 4];
        // rows r and r + 32 together, so that the butterfly's first exchange retires them at once: 32 partials stay live, not 64.
        // LOADS_IN_FLIGHT row pairs are loaded per batch (the scheduling barrier keeps the compiler from hoisting all 64 loads,
        // 256 registers, above the first use)
        float p[32];
        const bool up32 = (lane & 32) != 0;
        const gfloat* wt = wwave;
        asm volatile("" : "+s"(wt));      // opaque per step: the row addresses are scalar adds here, not 64 hoisted register pairs
#pragma unroll
        for (int r0 = 0; r0 < 32; r0 += LOADS_IN_FLIGHT) {
            f32x4 wa[LOADS_IN_FLIGHT], wb[LOADS_IN_FLIGHT];
#pragma unroll
            for (int j = 0; j < LOADS_IN_FLIGHT; ++j) {
                const int r = r0 + j;
                wa[j] = *(const gf32x4*)(wt + ((r >> 4) * LH + (r & 15)) * LH + loff);
                wb[j] = *(const gf32x4*)(wt + (((r >> 4) + 2) * LH + (r & 15)) * LH + loff);
            }
#pragma unroll
            for (int j = 0; j < LOADS_IN_FLIGHT; ++j) {
                const float a = fmaf(wa[j].w, hv.w, fmaf(wa[j].z, hv.z, fmaf(wa[j].y, hv.y, wa[j].x * hv.x)));
                const float bb = fmaf(wb[j].w, hv.w, fmaf(wb[j].z, hv.z, fmaf(wb[j].y, hv.y, wb[j].x * hv.x)));
                p[r0 + j] = (up32 ? bb : a) + __shfl_xor(up32 ? a : bb, 32, 64);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int half = 16; half >= 1; half >>= 1) {
            const bool up = (lane & half) != 0;
#pragma unroll
            for (int i = 0; i < half; ++i) {
                float lo = p[i], hi = p[i + half];
                asm("" : "+v"(lo), "+v"(hi));     // two register selects; left alone the compiler turns them into a select of the
                const float keep = up ? hi : lo;  // array INDEX, which on registers is a 32-way compare chain per element
                const float send = up ? lo : hi;
                p[i] = keep + __shfl_xor(send, half, 64);
            }
        }
        pre += p[0];
        const float gf = __shfl(pre, (lane & 15) + 16, 64);
        const float gg = __shfl(pre, (lane & 15) + 32, 64);
        const float go = __shfl(pre, (lane & 15) + 48, 64);
        if (lane < 16) {
            c = lstm_sigmoid(gf) * c + lstm_sigmoid(pre) * tanhf(gg);
            h = lstm_sigmoid(go) * tanhf(c);
            hbuf[cur ^ 1][unit] = h;
            if (h_all) h_all[((size_t)b * T + t) * LH + unit] = h;
        }
        __syncthreads();
    }
    if (lane < 16) {
        hT[(size_t)b * LH + unit] = h;
        cT[(size_t)b * LH + unit] = c;
    }
}

DEV float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// one workgroup per sequence: a wave per attractor, then one lane scans the C probabilities
__global__ __launch_bounds__(256) void eda_count_kernel(const float* __restrict__ attr, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float th, float* __restrict__ probs,
                                                        int* __restrict__ count, int C) {
    __shared__ float ps[EDA_MAX_ATTRACTORS];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const f32x4 wv = *(const f32x4*)(w + lane * 4);
    for (int cidx = wave; cidx < C; cidx += 4) {
        const f32x4 a = *(const f32x4*)(attr + ((size_t)b * C + cidx) * LH + lane * 4);
        const float s = wave_sum(fmaf(a.w, wv.w, fmaf(a.z, wv.z, fmaf(a.y, wv.y, a.x * wv.x)))) + bias[0];
        if (lane == 0) {
            const float pr = lstm_sigmoid(s);
            ps[cidx] = pr;
            probs[(size_t)b * C + cidx] = pr;
        }
    }
    __syncthreads();
    if (count && threadIdx.x == 0) {
        int n = C;
        for (int cidx = C - 1; cidx >= 0; --cidx)
            if (ps[cidx] < th) n = cidx;
        count[b] = n;
    }
}

// 16 frames of one sequence per workgroup; its attractors staged in LDS once
__global__ __launch_bounds__(256) void eda_head_kernel(const float* __restrict__ emb, int emb_rows, const float* __restrict__ attr,
                                                       float* __restrict__ logits, int T, int C) {
    __shared__ __attribute__((aligned(16))) float as[EDA_MAX_ATTRACTORS * LH];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < C * (LH / 4); i += 256)
        *(f32x4*)&as[i * 4] = *(const f32x4*)(attr + (size_t)b * C * LH + i * 4);
    __syncthreads();
    for (int r = 0; r < 4; ++r) {
        const int t = blockIdx.x * 16 + wave * 4 + r;
        if (t >= T) break;                                        // wave-uniform
        const f32x4 e = *(const f32x4*)(emb + ((size_t)b * emb_rows + t) * LH + lane * 4);
        for (int cidx = 0; cidx < C; ++cidx) {
            const f32x4 a = *(const f32x4*)&as[cidx * LH + lane * 4];
            const float s = wave_sum(fmaf(a.w, e.w, fmaf(a.z, e.z, fmaf(a.y, e.y, a.x * e.x))));
            if (lane == 0) logits[((size_t)b * T + t) * C + cidx] = s;
        }
    }
}

}  // namespace

int eend_lstm_shape_ok(int B, int T, int hidden) { return hidden == LSTM_HIDDEN && T >= 1 && B >= 1; }

int eend_launch_lstm(const float* G, int g_rows, const int* order, const float* bias, const float* Whh, const float* h0, const float* c0,
                     float* hT, float* cT, float* h_all, int B, int T, int hidden, int order_stride, hipStream_t stream) {
    if (!eend_lstm_shape_ok(B, T, hidden) || !Whh || !hT || !cT) return EEND_EINVAL;
    if (order_stride != 0 && (order_stride < T || !order || !G)) return EEND_EINVAL;
    if (G ? g_rows < T : !bias) return EEND_EINVAL;               // rows of G per sequence; zero input needs the bias sum
    if ((h0 == nullptr) != (c0 == nullptr)) return EEND_EINVAL;
    hipLaunchKernelGGL(lstm_seq_kernel, dim3(B), dim3(LNT), 0, stream, G, g_rows, order, bias, Whh, h0, c0, hT, cT, h_all, T,
                       order_stride);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_eda_count(const float* attr, const float* w, const float* bias, float th, float* probs, int* count, int B, int C,
                          hipStream_t stream) {
    if (B < 1 || C < 1 || C > EDA_MAX_ATTRACTORS || !attr || !w || !bias || !probs) return EEND_EINVAL;
    hipLaunchKernelGGL(eda_count_kernel, dim3(B), dim3(256), 0, stream, attr, w, bias, th, probs, count, C);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_eda_head(const float* emb, int emb_rows, const float* attr, float* logits, int B, int T, int C, hipStream_t stream) {
    if (B < 1 || B > 65535 || T < 1 || emb_rows < T || C < 1 || C > EDA_MAX_ATTRACTORS || !emb || !attr || !logits) return EEND_EINVAL;
    hipLaunchKernelGGL(eda_head_kernel, dim3((T + 15) / 16, B), dim3(256), 0, stream, emb, emb_rows, attr, logits, T, C);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
