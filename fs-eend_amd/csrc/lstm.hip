// The attractor path of the offline EEND-EDA baseline (FS-EEND/nnet/model/offl_tfm_enc_lstm_enc_dec.py:79-107): a single-layer
// LSTM recurrence (eend_lstm_f32, eend_lstm_orders_f32), the attractor-existence counter with the speaker count taken from it (eend_eda_count_f32) and the
// embedding . attractor head (eend_eda_head_f32); and what makes that path differentiable (model :109-127): the recurrence that keeps
// its gates and states (eend_lstm_train_f32), its backward (eend_lstm_bwd_f32), the attractor-existence loss with its gradients
// (eend_eda_count_loss_f32) and the head's backward (eend_eda_head_bwd_f32); the weight gradients are wgrad_f32.hip.  The three
// recurrence entries reach lstm_seq_kernel<TRAIN> through one launcher, eend_launch_lstm, with one block of argument rules: TRAIN only
// where something is kept.  The counter, its loss and the head share one 256-wide dot (dot256).  The contracts are in
// include/eend_hip.h; DESIGN 12 has the reasoning and the times.
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

// TRAIN: the same steps, and what the backward needs of every step (eend_lstm_train_f32): the four gates after their functions and the
// cell state in step order, the hidden state that ENTERS step t at the row of G the step read (hp_rows rows per sequence), which is
// the row the step's pre-activation gradient goes to, so that dW_hh = dG^T h_prev needs no gather.
template <bool TRAIN>
__global__ __launch_bounds__(LNT) void lstm_seq_kernel(const float* __restrict__ G, int g_rows, const int* __restrict__ order,
                                                       const float* __restrict__ bias, const float* __restrict__ Whh,
                                                       const float* __restrict__ h0, const float* __restrict__ c0,
                                                       float* __restrict__ hT, float* __restrict__ cT, float* __restrict__ h_all, int T,
                                                       int order_stride, float* __restrict__ gates, float* __restrict__ c_all,
                                                       float* __restrict__ h_prev, int hp_rows) {
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
        int row = t;
        if (Gb) {                                                 // issued first: lands behind the weight stream
            int o = order ? order[t] : t;
            o = o < 0 ? 0 : (o >= T ? T - 1 : o);                 // the host validates the permutation; never read outside G
            pre = Gb[(size_t)o * LG];
            row = o;
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
            if constexpr (TRAIN) {
                const float si = lstm_sigmoid(pre), sf = lstm_sigmoid(gf), tg = tanhf(gg), so = lstm_sigmoid(go);
                if (h_prev) h_prev[((size_t)b * hp_rows + row) * LH + unit] = h;
                c = sf * c + si * tg;
                h = so * tanhf(c);
                if (gates) {
                    float* gt = gates + ((size_t)b * T + t) * LG + unit;
                    gt[0] = si; gt[LH] = sf; gt[2 * LH] = tg; gt[3 * LH] = so;
                }
                if (c_all) c_all[((size_t)b * T + t) * LH + unit] = c;
            } else {
                c = lstm_sigmoid(gf) * c + lstm_sigmoid(pre) * tanhf(gg);
                h = lstm_sigmoid(go) * tanhf(c);
            }
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

// eend_lstm_bwd_f32: backpropagation through time of the recurrence above, again one workgroup of 16 waves per sequence, from step
// T - 1 down to 0, everything f32.  A step has two halves and two barriers:
//   units  threads 0 .. 255 own one hidden unit each and keep its dc in a register: dh = dh_all[t] + the recurrent part (the 16 wave
//          partials of the step before, summed in wave order), the four pre-activation gradients into LDS and into dG at the row of G
//          the forward step read;
//   W^T    wave w owns gate rows 64 w .. 64 w + 63: lane l loads its float4 of each row (the forward's coalesced 1-KiB row requests,
//          1 MiB of W_hh from L2 per step) and accumulates four column partials of W_hh^T dpre against the broadcast dpre[r], r
//          ascending; the 16 x 256 partials go to LDS.
// No cross-lane reduction is needed (the forward's butterfly sums over the columns a lane holds; here a lane's columns are the outputs).
// The order of every sum is fixed by (row, wave), so a sequence's bits do not depend on its batch mates or on the run.  The units'
// operands of step t - 1 are requested before the weight stream of step t, so their latency hides behind it.
constexpr int BWD_LOADS_IN_FLIGHT = 16;  // rows per load batch: 16 float4 loads = 64 registers

__global__ __launch_bounds__(LNT) void lstm_bwd_kernel(const float* __restrict__ gates, const float* __restrict__ c_all,
                                                       const float* __restrict__ c0, const float* __restrict__ Whh,
                                                       const float* __restrict__ dh_all, const float* __restrict__ dhT,
                                                       const float* __restrict__ dcT, const int* __restrict__ order, int order_stride,
                                                       float* __restrict__ dG, int g_rows, float* __restrict__ dh0,
                                                       float* __restrict__ dc0, int T) {
    __shared__ __attribute__((aligned(16))) float dpre[LG];
    __shared__ __attribute__((aligned(16))) float part[16][LH];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (order) order += (size_t)b * order_stride;
    const bool owner = tid < LH;                                  // waves 0 .. 3: wave-uniform
    const int u = tid & (LH - 1);
    for (int i = tid; i < 16 * LH; i += LNT) part[i / LH][i % LH] = (i < LH && dhT) ? dhT[(size_t)b * LH + i] : 0.f;
    float dc = (owner && dcT) ? dcT[(size_t)b * LH + u] : 0.f;
    const gfloat* wwave = (const gfloat*)Whh + (size_t)__builtin_amdgcn_readfirstlane(wave) * 64 * LH;
    const unsigned loff = lane * 4;
    // the operands of the unit half, one step ahead
    float gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f, ct = 0.f, cp = 0.f, du = 0.f;
    auto fetch = [&](int t) {
        const float* gt = gates + ((size_t)b * T + t) * LG + u;
        gi = gt[0]; gf = gt[LH]; gg = gt[2 * LH]; go = gt[3 * LH];
        ct = c_all[((size_t)b * T + t) * LH + u];
        cp = t > 0 ? c_all[((size_t)b * T + t - 1) * LH + u] : (c0 ? c0[(size_t)b * LH + u] : 0.f);
        du = dh_all ? dh_all[((size_t)b * T + t) * LH + u] : 0.f;
    };
    if (owner) fetch(T - 1);
    __syncthreads();

    for (int t = T - 1; t >= 0; --t) {
        if (owner) {
            float rec = part[0][u];
#pragma unroll
            for (int w = 1; w < 16; ++w) rec += part[w][u];
            const float dh = du + rec;
            const float tc = tanhf(ct);
            dc += dh * go * (1.0f - tc * tc);
            const float d_i = dc * gg * (gi * (1.0f - gi));
            const float d_f = dc * cp * (gf * (1.0f - gf));
            const float d_g = dc * gi * (1.0f - gg * gg);
            const float d_o = dh * tc * (go * (1.0f - go));
            dc *= gf;
            dpre[u] = d_i; dpre[LH + u] = d_f; dpre[2 * LH + u] = d_g; dpre[3 * LH + u] = d_o;
            int o = order ? order[t] : t;
            o = o < 0 ? 0 : (o >= T ? T - 1 : o);                 // as the forward: never outside the T rows
            float* dg = dG + ((size_t)b * g_rows + o) * LG + u;
            dg[0] = d_i; dg[LH] = d_f; dg[2 * LH] = d_g; dg[3 * LH] = d_o;
            if (t > 0) fetch(t - 1);                              // lands behind the weight stream below
        }
        __syncthreads();
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const gfloat* wt = wwave;
        asm volatile("" : "+s"(wt));      // opaque per step: the row addresses are scalar adds here, not hoisted register pairs
        const float* dw = &dpre[wave * 64];
#pragma unroll
        for (int r0 = 0; r0 < 64; r0 += BWD_LOADS_IN_FLIGHT) {
            f32x4 wv[BWD_LOADS_IN_FLIGHT];
#pragma unroll
            for (int j = 0; j < BWD_LOADS_IN_FLIGHT; ++j) wv[j] = *(const gf32x4*)(wt + (r0 + j) * LH + loff);
#pragma unroll
            for (int j = 0; j < BWD_LOADS_IN_FLIGHT; j += 4) {
                const f32x4 d = *(const f32x4*)&dw[r0 + j];       // one address for the wave: a broadcast read
                const float ds[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc.x = fmaf(ds[q], wv[j + q].x, acc.x);
                    acc.y = fmaf(ds[q], wv[j + q].y, acc.y);
                    acc.z = fmaf(ds[q], wv[j + q].z, acc.z);
                    acc.w = fmaf(ds[q], wv[j + q].w, acc.w);
                }
            }
            // the next batch's loads stay below this batch's sums: all 64 rows at once are 256 registers, which spill
            asm volatile("" : "+v"(acc.x), "+v"(acc.y), "+v"(acc.z), "+v"(acc.w) : : "memory");
            __builtin_amdgcn_sched_barrier(0);
        }
        *(f32x4*)&part[wave][lane * 4] = acc;
        __syncthreads();
    }
    if (owner) {
        float rec = part[0][u];
#pragma unroll
        for (int w = 1; w < 16; ++w) rec += part[w][u];
        dh0[(size_t)b * LH + u] = rec;
        dc0[(size_t)b * LH + u] = dc;
    }
}

// NOT train_common.h's wave_sum: that one adds the halves 1 -> 32, this one 32 -> 1.  The two orders give different bits, so neither
// may stand in for the other (the counter's probabilities and the logits are pinned bit for bit).
DEV float wave_sum_32to1(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the 256-wide dot of the counter and the head: lane l's four columns as one fmaf chain from x up, then the sum above
DEV float dot256(f32x4 a, f32x4 b) { return wave_sum_32to1(fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)))); }

// one workgroup per sequence: a wave per attractor, then one lane scans the C probabilities
__global__ __launch_bounds__(256) void eda_count_kernel(const float* __restrict__ attr, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float th, float* __restrict__ probs,
                                                        int* __restrict__ count, int C) {
    __shared__ float ps[EDA_MAX_ATTRACTORS];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const f32x4 wv = *(const f32x4*)(w + lane * 4);
    for (int cidx = wave; cidx < C; cidx += 4) {
        const f32x4 a = *(const f32x4*)(attr + ((size_t)b * C + cidx) * LH + lane * 4);
        const float s = dot256(a, wv) + bias[0];
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
            const float s = dot256(a, e);
            if (lane == 0) logits[((size_t)b * T + t) * C + cidx] = s;
        }
    }
}

// eend_eda_count_loss_f32, first pass: one workgroup per sequence.  A wave per attractor forms the counter's logit, its BCE term and
// d loss / d logit (already divided by the element count of the whole batch); then thread j writes column j of d attractors and
// of the sequence's part of dw (c ascending).  ws [B][EDA_COUNT_LOSS_WS]: dw part (256), loss part, dbias part.
DEV int eda_clamp_n(int n, int C) { return n < 0 ? 0 : (n > C - 1 ? C - 1 : n); }

__global__ __launch_bounds__(256) void eda_count_loss_kernel(const float* __restrict__ attr, const float* __restrict__ w,
                                                             const float* __restrict__ bias, const int* __restrict__ n_spk,
                                                             float* __restrict__ dattr, float* __restrict__ ws, int B, int C) {
    __shared__ float dz[EDA_MAX_ATTRACTORS], le[EDA_MAX_ATTRACTORS];
    __shared__ int ntot;
    const int b = blockIdx.x, j = threadIdx.x, lane = j & 63, wave = j >> 6;
    if (j == 0) {
        int n = 0;
        for (int i = 0; i < B; ++i) n += eda_clamp_n(n_spk[i], C) + 1;
        ntot = n;
    }
    const int nb = eda_clamp_n(n_spk[b], C);
    const f32x4 wv = *(const f32x4*)(w + lane * 4);
    __syncthreads();
    const float inv = 1.0f / (float)ntot;
    for (int cidx = wave; cidx < C; cidx += 4) {
        float l = 0.f, g = 0.f;
        if (cidx <= nb) {                                         // wave-uniform: labels [1] * n_b + [0], nothing beyond
            const f32x4 a = *(const f32x4*)(attr + ((size_t)b * C + cidx) * LH + lane * 4);
            const float z = dot256(a, wv) + bias[0];
            const float y = cidx < nb ? 1.f : 0.f;
            l = fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z)));   // BCE with logits, finite for every finite z
            g = (lstm_sigmoid(z) - y) * inv;
        }
        if (lane == 0) { dz[cidx] = g; le[cidx] = l; }
    }
    __syncthreads();
    if (dattr) {                                                  // NULL: the loss alone
        const float wj = w[j];
        float dwp = 0.f;
        for (int cidx = 0; cidx < C; ++cidx) {
            const float g = dz[cidx];
            const size_t at = ((size_t)b * C + cidx) * LH + j;
            dattr[at] = g * wj;
            dwp = fmaf(g, attr[at], dwp);
        }
        ws[(size_t)b * EDA_COUNT_LOSS_WS + j] = dwp;
    }
    if (j == 0) {
        float ls = 0.f, db = 0.f;
        for (int cidx = 0; cidx < C; ++cidx) { ls += le[cidx]; db += dz[cidx]; }
        ws[(size_t)b * EDA_COUNT_LOSS_WS + LH] = ls;
        ws[(size_t)b * EDA_COUNT_LOSS_WS + LH + 1] = db;
    }
}

// second pass, one workgroup: the sequences' parts summed in batch order
__global__ __launch_bounds__(256) void eda_count_loss_reduce_kernel(const float* __restrict__ ws, const int* __restrict__ n_spk,
                                                                    float* __restrict__ loss, float* __restrict__ dw,
                                                                    float* __restrict__ dbias, int B, int C) {
    const int j = threadIdx.x;
    if (dw) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += ws[(size_t)b * EDA_COUNT_LOSS_WS + j];
        dw[j] = s;
    }
    if (j == 0) {
        int n = 0;
        float ls = 0.f, db = 0.f;
        for (int b = 0; b < B; ++b) {
            n += eda_clamp_n(n_spk[b], C) + 1;
            ls += ws[(size_t)b * EDA_COUNT_LOSS_WS + LH];
            db += ws[(size_t)b * EDA_COUNT_LOSS_WS + LH + 1];
        }
        loss[0] = ls / (float)n;
        if (dbias) dbias[0] = db;
    }
}

// eend_eda_head_bwd_f32: EDA_HEAD_BWD_TILE frames of one sequence per workgroup, thread j owns column j of emb and of the attractors.
// d emb of a frame is complete here; d attractors is the tile's part (frames ascending), summed over the tiles in order afterwards.
__global__ __launch_bounds__(256) void eda_head_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ emb, int emb_rows,
                                                           const float* __restrict__ attr, float* __restrict__ part,
                                                           float* __restrict__ demb, int T, int C) {
    __shared__ float dl[EDA_HEAD_BWD_TILE][EDA_MAX_ATTRACTORS];
    const int b = blockIdx.y, t0 = blockIdx.x * EDA_HEAD_BWD_TILE, j = threadIdx.x;
    const int nt = T - t0 < EDA_HEAD_BWD_TILE ? T - t0 : EDA_HEAD_BWD_TILE;
    for (int i = j; i < EDA_HEAD_BWD_TILE * EDA_MAX_ATTRACTORS; i += 256) {
        const int r = i / EDA_MAX_ATTRACTORS, cidx = i % EDA_MAX_ATTRACTORS;
        dl[r][cidx] = (r < nt && cidx < C) ? dlogits[((size_t)b * T + t0 + r) * C + cidx] : 0.f;   // zeros leave a sum as it is
    }
    float a[EDA_MAX_ATTRACTORS], acc[EDA_MAX_ATTRACTORS];
#pragma unroll
    for (int cidx = 0; cidx < EDA_MAX_ATTRACTORS; ++cidx) {
        a[cidx] = cidx < C ? attr[((size_t)b * C + cidx) * LH + j] : 0.f;
        acc[cidx] = 0.f;
    }
    __syncthreads();
    for (int r = 0; r < nt; ++r) {
        const float e = emb[((size_t)b * emb_rows + t0 + r) * LH + j];
        float de = 0.f;
#pragma unroll
        for (int cidx = 0; cidx < EDA_MAX_ATTRACTORS; ++cidx) {
            const float d = dl[r][cidx];                          // one address for the workgroup: a broadcast read
            acc[cidx] = fmaf(d, e, acc[cidx]);
            de = fmaf(d, a[cidx], de);
        }
        if (demb) demb[((size_t)b * T + t0 + r) * LH + j] = de;
    }
    if (part) {
#pragma unroll
        for (int cidx = 0; cidx < EDA_MAX_ATTRACTORS; ++cidx)
            if (cidx < C) part[(((size_t)b * gridDim.x + blockIdx.x) * C + cidx) * LH + j] = acc[cidx];
    }
}

__global__ __launch_bounds__(256) void eda_head_bwd_reduce_kernel(const float* __restrict__ part, float* __restrict__ dattr, int ntiles,
                                                                  int C) {
    const int b = blockIdx.x / C, cidx = blockIdx.x % C, j = threadIdx.x;
    float s = 0.f;
    for (int i = 0; i < ntiles; ++i) s += part[(((size_t)b * ntiles + i) * C + cidx) * LH + j];
    dattr[(size_t)blockIdx.x * LH + j] = s;
}

}  // namespace

int eend_lstm_shape_ok(int B, int T, int hidden) { return hidden == LSTM_HIDDEN && T >= 1 && B >= 1; }

// One launcher for eend_lstm_f32, eend_lstm_orders_f32 and eend_lstm_train_f32.  With nothing to keep it runs the inference instance,
// whose hT, cT and h_all have the training instance's bits.  h_prev has hp_rows >= T rows per sequence, its own count: the
// backward's operands need not be as tall as a padded slab of G.
int eend_launch_lstm(const float* G, int g_rows, const int* order, const float* bias, const float* Whh, const float* h0, const float* c0,
                     float* hT, float* cT, float* h_all, float* gates, float* c_all, float* h_prev, int hp_rows, int B, int T, int hidden,
                     int order_stride, hipStream_t stream) {
    if (!eend_lstm_shape_ok(B, T, hidden) || !Whh || !hT || !cT) return EEND_EINVAL;
    if (order_stride != 0 && (order_stride < T || !order)) return EEND_EINVAL;
    if (G ? g_rows < T : (!bias || order)) return EEND_EINVAL;    // rows of G per sequence; zero input needs the bias sum, takes no order
    if ((h0 == nullptr) != (c0 == nullptr) || (h_prev && hp_rows < T)) return EEND_EINVAL;
    const auto kernel = !gates && !c_all && !h_prev ? lstm_seq_kernel<false> : lstm_seq_kernel<true>;
    hipLaunchKernelGGL(kernel, dim3(B), dim3(LNT), 0, stream, G, g_rows, order, bias, Whh, h0, c0, hT, cT, h_all, T, order_stride, gates,
                       c_all, h_prev, hp_rows);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_lstm_bwd(const float* gates, const float* c_all, const float* c0, const float* Whh, const float* dh_all, const float* dhT,
                         const float* dcT, const int* order, int order_stride, float* dG, int g_rows, float* dh0, float* dc0, int B, int T,
                         int hidden, hipStream_t stream) {
    if (!eend_lstm_shape_ok(B, T, hidden) || !gates || !c_all || !Whh || !dG || !dh0 || !dc0 || g_rows < T) return EEND_EINVAL;
    if (!dh_all && !dhT && !dcT) return EEND_EINVAL;              // no upstream gradient at all
    if (order_stride != 0 && (order_stride < T || !order)) return EEND_EINVAL;
    hipLaunchKernelGGL(lstm_bwd_kernel, dim3(B), dim3(LNT), 0, stream, gates, c_all, c0, Whh, dh_all, dhT, dcT, order, order_stride, dG,
                       g_rows, dh0, dc0, T);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_eda_count_loss(const float* attr, const float* w, const float* bias, const int* n_spk, float* loss, float* dattr,
                               float* dw, float* dbias, float* ws, long ws_bytes, int B, int C, hipStream_t stream) {
    if (B < 1 || C < 1 || C > EDA_MAX_ATTRACTORS || !attr || !w || !bias || !n_spk || !loss || !ws) return EEND_EINVAL;
    if ((!dattr || !dw || !dbias) && (dattr || dw || dbias)) return EEND_EINVAL;      // the three gradients together, or none
    if (ws_bytes < eend_eda_count_loss_ws_floats(B) * (long)sizeof(float)) return EEND_EINVAL;
    hipLaunchKernelGGL(eda_count_loss_kernel, dim3(B), dim3(256), 0, stream, attr, w, bias, n_spk, dattr, ws, B, C);
    hipLaunchKernelGGL(eda_count_loss_reduce_kernel, dim3(1), dim3(256), 0, stream, ws, n_spk, loss, dw, dbias, B, C);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

long eend_eda_count_loss_ws_floats(int B) { return B < 1 ? 0 : (long)B * EDA_COUNT_LOSS_WS; }

long eend_eda_head_bwd_ws_floats(int B, int T, int C) {
    if (B < 1 || T < 1 || C < 1 || C > EDA_MAX_ATTRACTORS) return 0;
    return (long)B * ((T + EDA_HEAD_BWD_TILE - 1) / EDA_HEAD_BWD_TILE) * C * LSTM_HIDDEN;
}

int eend_launch_eda_head_bwd(const float* dlogits, const float* emb, int emb_rows, const float* attr, float* dattr, float* demb, float* ws,
                             long ws_bytes, int B, int T, int C, hipStream_t stream) {
    if (B < 1 || B > 65535 || T < 1 || emb_rows < T || C < 1 || C > EDA_MAX_ATTRACTORS || !dlogits || !emb || !attr) return EEND_EINVAL;
    if (!dattr && !demb) return EEND_EINVAL;
    if (dattr && (!ws || ws_bytes < eend_eda_head_bwd_ws_floats(B, T, C) * (long)sizeof(float))) return EEND_EINVAL;
    const int ntiles = (T + EDA_HEAD_BWD_TILE - 1) / EDA_HEAD_BWD_TILE;
    hipLaunchKernelGGL(eda_head_bwd_kernel, dim3(ntiles, B), dim3(256), 0, stream, dlogits, emb, emb_rows, attr, dattr ? ws : nullptr, demb,
                       T, C);
    if (dattr) hipLaunchKernelGGL(eda_head_bwd_reduce_kernel, dim3(B * C), dim3(256), 0, stream, ws, dattr, ntiles, C);
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
