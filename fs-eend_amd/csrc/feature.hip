// Feature front-end: 8 kHz waveform -> STFT (Hann 200 zero-padded to n_fft 256,
// hop 80, centred) -> |.|^2 -> 23 Slaney mel bands -> log10(max(., 1e-10)) -> optional (cumulative) mean
// normalisation -> +-c frame splice -> subsample, i.e. {LS,FS}-EEND/datasets/feature.py: stft :166-191,
// transform :43-131 (logmel23 / logmel23_mn / logmel23_cummn), splice :141-163, subsample :133-138,
// extract_fbank :324-336.  One hour of audio is 115 MB in and 50 MB out: the stage is bandwidth-trivial next
// to the model, so the kernels are written for exactness (fp32 end to end, exact-fp32 MFMA) and simplicity.
//
// stft_logmel_kernel: a block owns 64 frames.  The 129-bin DFT of the 200 non-zero window taps is a
// [64 x 200] x [200 x 288] product on v_mfma_f32_16x16x4_f32 (exact fp32 multiply, fp32 accumulate): the
// table already carries the window, columns 0..128 are the cosine (real) and 144..272 the -sine (imaginary)
// parts, so real and imaginary parts of a bin sit in the same lane/register of accumulator tiles t and t+9 and
// the power needs no data movement.  The table streams through LDS in 20-tap slices; the block's samples are
// staged once (frames overlap: 5240 samples for 64 frames).  Power tiles go through LDS to become the A operand
// of the [16 x 132] x [132 x 32] mel product; log10 in the epilogue.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int WIN = 200, HOP = 80, NCOL = 288, IMOFF = 144, NBIN = 129, KMEL = 132, NMEL = 23, MELP = 32;
constexpr int FB = 64;                               // frames per block
constexpr int XSPAN = (FB - 1) * HOP + WIN;          // 5240 samples
constexpr int KC = 20;                               // window taps per staged table slice
constexpr int PSTR = KMEL + 1;                       // padded power row
constexpr int SM_X = 0;
constexpr int SM_B = SM_X + XSPAN * 4;               // 20960
constexpr int SM_P = SM_B + KC * NCOL * 4;           // + 23040
constexpr int SM_M = SM_P + 4 * 16 * PSTR * 4;       // + 34048
constexpr int SM_BYTES = SM_M + KMEL * MELP * 4;     // + 16896 = 94944

// The per-tile body of both STFT kernels: FB consecutive frames whose samples gather(i), i = 0..XSPAN-1, returns (tap 0 of
// the tile's first frame is i = 0), written as log-mel rows out[r][23] for r < rows.  Batch and incremental front-ends run
// exactly this instruction sequence, so their log-mel frames are bit-identical.
template <class Gather>
__device__ __forceinline__ void stft_logmel_tile(char* smem, Gather gather, const float* __restrict__ dft,
                                                 const float* __restrict__ melT, float* __restrict__ out, int rows) {
    float* xs = (float*)(smem + SM_X);
    float* Bs = (float*)(smem + SM_B);
    float* Pw = (float*)(smem + SM_P);
    float* Ms = (float*)(smem + SM_M);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fk = lane >> 4;

    for (int i = tid; i < XSPAN; i += 256) xs[i] = gather(i);
    for (int i = tid; i < KMEL * MELP; i += 256) Ms[i] = melT[i];

    f32x4 acc[18];
#pragma unroll
    for (int t = 0; t < 18; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < WIN; k0 += KC) {
        __syncthreads();
        for (int i = tid; i < KC * NCOL; i += 256) Bs[i] = dft[(long)k0 * NCOL + i];
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < KC; ks += 4) {
            const float a = xs[(wave * 16 + frow) * HOP + k0 + ks + fk];
#pragma unroll
            for (int t = 0; t < 18; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[(ks + fk) * NCOL + t * 16 + frow], acc[t], 0, 0, 0);
        }
    }
    // power spectrum of the wave's 16 frames -> LDS [frame][bin]  (D layout: column = lane & 15, row = (lane >> 4) * 4 + reg)
    float* P = Pw + wave * 16 * PSTR;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int bin = t * 16 + frow;
        if (bin < KMEL) {
#pragma unroll
            for (int r = 0; r < 4; ++r) P[(fk * 4 + r) * PSTR + bin] = acc[t][r] * acc[t][r] + acc[t + 9][r] * acc[t + 9][r];
        }
    }
    __syncthreads();
    f32x4 am[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll 3
    for (int k0 = 0; k0 < KMEL; k0 += 4) {
        const float a = P[frow * PSTR + k0 + fk];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
            am[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Ms[(k0 + fk) * MELP + mt * 16 + frow], am[mt], 0, 0, 0);
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int m = mt * 16 + frow;
        if (m < NMEL) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = wave * 16 + fk * 4 + r;
                if (f < rows) out[(long)f * NMEL + m] = log10f(__builtin_fmaxf(am[mt][r], 1e-10f));
            }
        }
    }
}

__global__ __launch_bounds__(256)
void stft_logmel_kernel(const float* __restrict__ y, long len, long first, int n_frames, const float* __restrict__ dft,
                        const float* __restrict__ melT, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int f0 = blockIdx.x * FB;
    const long base = first + (long)f0 * HOP;            // sample index of tap 0 of the block's first frame
    auto gather = [=](int i) {
        const long idx = base + i;
        return (idx >= 0 && idx < len) ? y[idx] : 0.f;
    };
    stft_logmel_tile(smem, gather, dft, melT, out + (long)f0 * NMEL, n_frames - f0);
}

// Mean normalisations of a (T, F) map, one block per column, the running column sum carried in fp64:
//   mode 1 (logmel23_mn)    out = Y - mean over all frames
//   mode 2 (logmel23_cummn) out[t] = Y[t] - (Y[0] + .. + Y[t]) / (t + 1)
// colnorm_column is the whole body, one block of NT2 threads per column of one map (wsum: NT2 / 64 doubles and carry: one
// double of LDS): the single-waveform and the batched kernel both call it, so their sums are added in the same order.
constexpr int NT2 = 1024, PER = 4;
__device__ __forceinline__ void colnorm_column(const float* __restrict__ Y, float* __restrict__ out, int T, int F, int col, int mode,
                                               double* wsum, double* carry) {
    double& carry_s = *carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0.0;
    __syncthreads();
    if (mode == 1) {
        double s = 0.0;
        for (int t = tid; t < T; t += NT2) s += (double)Y[(long)t * F + col];
        for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
        if (lane == 0) wsum[wave] = s;
        __syncthreads();
        if (tid == 0) {
            double tot = 0.0;
            for (int w = 0; w < NT2 / 64; ++w) tot += wsum[w];
            carry_s = tot / (double)T;
        }
        __syncthreads();
        const float mean = (float)carry_s;
        for (int t = tid; t < T; t += NT2) out[(long)t * F + col] = Y[(long)t * F + col] - mean;
        return;
    }
    for (int t0 = 0; t0 < T; t0 += NT2 * PER) {
        float v[PER];
        double loc[PER], s = 0.0;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int t = t0 + tid * PER + i;
            v[i] = t < T ? Y[(long)t * F + col] : 0.f;
            s += (double)v[i];
            loc[i] = s;
        }
        double incl = s;                                         // inclusive scan of the per-thread sums inside the wave
        for (int d = 1; d < 64; d <<= 1) {
            const double o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        double pre = carry_s;
        for (int w = 0; w < wave; ++w) pre += wsum[w];
        pre += incl - s;                                         // exclusive prefix of this thread
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int t = t0 + tid * PER + i;
            if (t < T) out[(long)t * F + col] = v[i] - (float)((pre + loc[i]) / (double)(t + 1));
        }
        __syncthreads();
        if (tid == NT2 - 1) carry_s = pre + s;
        __syncthreads();
    }
}

__global__ __launch_bounds__(NT2)
void colnorm_kernel(const float* __restrict__ Y, float* __restrict__ out, int T, int F, int mode) {
    __shared__ double wsum[NT2 / 64];
    __shared__ double carry_s;
    colnorm_column(Y, out, T, F, blockIdx.x, mode, wsum, &carry_s);
}

// Element e = c * F + m of model frame j, the splice of frames j sub - ctx .. j sub + ctx side by side: Y[f - row0][m] for
// f = j sub + c - ctx in [lo, hi) (Y's first row is frame row0), zero outside.  The one rule of all three splice kernels.
__device__ __forceinline__ float splice_at(const float* Y, long lo, long hi, long row0, long j, int e, int F, int ctx, int sub) {
    const int c = e / F, m = e - c * F;
    const long f = j * sub + c - ctx;
    return (f >= lo && f < hi) ? Y[(f - row0) * F + m] : 0.f;
}

// out[j][c * F + m] = Y[j * sub + c - ctx][m] (zero outside [0, T)): splice of 2 ctx + 1 frames, every sub-th row
__global__ __launch_bounds__(256)
void splice_subsample_kernel(const float* __restrict__ Y, int T, int F, int ctx, int sub, int To, float* __restrict__ out) {
    const int W = F * (2 * ctx + 1);
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)To * W) return;
    const int j = (int)(idx / W), e = (int)(idx - (long)j * W);
    out[idx] = splice_at(Y, 0, T, 0, j, e, F, ctx, sub);
}


// ---- incremental front-end: many streams ("slots"), each fed its audio in chunks of any size (eend_audio_feed_f32) ----
// Per slot the device keeps the sample tail (TAIL floats: samples 80 f - 100 .. of its next log-mel frame f, fewer than 200
// received), the fp64 column sums of cumulative mean normalisation and a ring of the last normalised log-mel frames that the
// splice of its next model frame needs.  The host keeps the counters and builds one descriptor per slot named in the call
// (FEED_* fields) and the two tile tables.  Y is the call's scratch of normalised log-mel rows: a slot's region starts at
// row ybase with its ring frames rb .. f_before - 1 followed by its new frames f_before .. f_after - 1.
constexpr int TAIL = 200, RING = 32;
enum { FEED_CHUNK, FEED_RECV0, FEED_RECV1, FEED_F0, FEED_F1, FEED_RB0, FEED_RB1, FEED_YBASE, FEED_SLOT, FEED_N };

// Sample idx of a slot's stream during a call: zero before 0 and from recv1 on, from the new chunk from recv0 on, below that
// from the slot's tail tl (received before this call), whose element 0 is the first sample of log-mel frame f0.
__device__ __forceinline__ float feed_sample(long idx, const long* __restrict__ d, const float* __restrict__ tl) {
    if (idx < 0 || idx >= d[FEED_RECV1]) return 0.f;
    if (idx >= d[FEED_RECV0]) return ((const float*)d[FEED_CHUNK])[idx - d[FEED_RECV0]];
    const long q = idx - (d[FEED_F0] * HOP - 100);
    return q < TAIL ? tl[q] : 0.f;
}

// One block per tile of up to FB new log-mel frames of one slot (tile = {descriptor, first frame, rows}).
__global__ __launch_bounds__(256)
void feed_stft_kernel(const long* __restrict__ desc, const long* __restrict__ tiles, const float* __restrict__ tail,
                      const float* __restrict__ dft, const float* __restrict__ melT, float* __restrict__ Y) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const long* t = tiles + 3 * (long)blockIdx.x;
    const long* d = desc + FEED_N * t[0];
    const long f_a = t[1];
    const float* tl = tail + (long)d[FEED_SLOT] * TAIL;
    const long base = f_a * HOP - 100;
    auto gather = [=](int i) { return feed_sample(base + i, d, tl); };
    float* out = Y + (d[FEED_YBASE] + f_a - d[FEED_RB0]) * NMEL;
    stft_logmel_tile(smem, gather, dft, melT, out, (int)t[2]);
}

// One block per slot: history rows from the ring, normalisation of the new rows in place (mode 2: out[t] = Y[t] - (Y[0] + .. +
// Y[t]) / (t + 1), the fp64 sum added strictly in frame order, so the result does not depend on the chunking), then the new
// ring and tail.  Everything the block overwrites is read before the barrier.
__global__ __launch_bounds__(256)
void feed_state_kernel(const long* __restrict__ desc, float* __restrict__ tail, float* __restrict__ ring, double* __restrict__ sums,
                       float* __restrict__ Y, int mode) {
    __shared__ float nr[RING * NMEL];
    const int tid = threadIdx.x;
    const long* d = desc + FEED_N * (long)blockIdx.x;
    const long f0 = d[FEED_F0], f1 = d[FEED_F1];
    const long rb0 = d[FEED_RB0], rb1 = d[FEED_RB1], slot = d[FEED_SLOT];
    float* Ys = Y + d[FEED_YBASE] * NMEL;
    float* rg = ring + slot * RING * NMEL;
    float* tl = tail + slot * TAIL;
    const int hist = (int)(f0 - rb0), n_new = (int)(f1 - f0);

    for (int i = tid; i < hist * NMEL; i += 256) {
        const float v = rg[i];
        Ys[i] = v;
        const long q = rb0 + i / NMEL - rb1;
        if (q >= 0) nr[q * NMEL + i % NMEL] = v;
    }
    const float tv = tid < TAIL ? feed_sample(f1 * HOP - 100 + tid, d, tl) : 0.f;
    float* Yn = Ys + (long)hist * NMEL;
    if (mode == 2) {
        if (tid < NMEL) {
            double s = f0 ? sums[slot * NMEL + tid] : 0.0;
            constexpr int U = 8;
            for (int i0 = 0; i0 < n_new; i0 += U) {
                float v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = i0 + u < n_new ? Yn[(long)(i0 + u) * NMEL + tid] : 0.f;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int i = i0 + u;
                    if (i < n_new) {
                        s += (double)v[u];
                        const float o = v[u] - (float)(s / (double)(f0 + i + 1));
                        Yn[(long)i * NMEL + tid] = o;
                        const long q = f0 + i - rb1;
                        if (q >= 0) nr[q * NMEL + tid] = o;
                    }
                }
            }
            sums[slot * NMEL + tid] = s;
        }
    } else {
        const long skip = rb1 > f0 ? (rb1 - f0) * NMEL : 0;        // only the frames that stay in the ring
        for (long i = skip + tid; i < (long)n_new * NMEL; i += 256) nr[(f0 - rb1) * NMEL + i] = Yn[i];
    }
    __syncthreads();
    for (int i = tid; i < (int)(f1 - rb1) * NMEL; i += 256) rg[i] = nr[i];
    if (tid < TAIL) tl[tid] = tv;
}

// One block per tile of up to SPL_ROWS model frames of one slot (tile = {descriptor, first model frame j, rows, output row}):
// model frame j = frames j sub - ctx .. j sub + ctx side by side, zero outside [0, f_after).
constexpr int SPL_ROWS = 16;
__global__ __launch_bounds__(256)
void feed_splice_kernel(const long* __restrict__ desc, const long* __restrict__ tiles, const float* __restrict__ Y,
                        float* __restrict__ out, int ctx, int sub) {
    const long* t = tiles + 4 * (long)blockIdx.x;
    const long* d = desc + FEED_N * t[0];
    const long j0 = t[1], f1 = d[FEED_F1], rb = d[FEED_RB0];
    const int rows = (int)t[2], W = NMEL * (2 * ctx + 1);
    const float* Ys = Y + d[FEED_YBASE] * NMEL;
    float* o = out + t[3] * W;
    for (int i = threadIdx.x; i < rows * W; i += 256) {
        const int r = i / W;
        o[i] = splice_at(Ys, rb, f1, rb, j0 + r, i - r * W, NMEL, ctx, sub);
    }
}

// ---- labelled training batches from resident audio (eend_chunk_batch_f32): many chunks of a device-resident corpus, each ----
// treated as a file of its own (LS-EEND/datasets/diarization_dataset_on_the_fly.py:87-131, datasets/feature.py:255-322).  The
// host builds one descriptor per chunk (CHUNK_* fields) and the two tile tables; Y / Yn hold the chunks' log-mel rows back to back.
enum { CHUNK_OFF, CHUNK_LEN, CHUNK_FRAMES, CHUNK_YBASE, CHUNK_START, CHUNK_END, CHUNK_SEG0, CHUNK_SEG1, CHUNK_N };

__device__ __forceinline__ float sample_f32(float v) { return v; }
__device__ __forceinline__ float sample_f32(short v) { return (float)v * (1.f / 32768.f); }       // exact: a power of two

// One block per tile of up to FB log-mel frames of one chunk (tile = {descriptor, first frame, rows}): the third gather of
// stft_logmel_tile, corpus[off + i] for 0 <= i < len and zero outside, i.e. stft_logmel_kernel's with first = -100 per chunk.
template <class S>
__global__ __launch_bounds__(256)
void chunk_stft_kernel(const S* __restrict__ corpus, const long* __restrict__ desc, const long* __restrict__ tiles,
                       const float* __restrict__ dft, const float* __restrict__ melT, float* __restrict__ Y) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const long* t = tiles + 3 * (long)blockIdx.x;
    const long* d = desc + CHUNK_N * t[0];
    const S* x = corpus + d[CHUNK_OFF];
    const long len = d[CHUNK_LEN], f_a = t[1];
    const long base = f_a * HOP - 100;
    auto gather = [=](int i) {
        const long idx = base + i;
        return (idx >= 0 && idx < len) ? sample_f32(x[idx]) : 0.f;
    };
    stft_logmel_tile(smem, gather, dft, melT, Y + (d[CHUNK_YBASE] + f_a) * NMEL, (int)t[2]);
}

// grid (NMEL, chunks): colnorm_kernel on every chunk's own rows
__global__ __launch_bounds__(NT2)
void chunk_colnorm_kernel(const long* __restrict__ desc, const float* __restrict__ Y, float* __restrict__ out, int mode) {
    __shared__ double wsum[NT2 / 64];
    __shared__ double carry_s;
    const long* d = desc + CHUNK_N * (long)blockIdx.y;
    const int T = (int)d[CHUNK_FRAMES];
    if (T <= 0) return;
    const long at = d[CHUNK_YBASE] * NMEL;
    colnorm_column(Y + at, out + at, T, NMEL, blockIdx.x, mode, wsum, &carry_s);
}

// One block per tile of up to SPL_ROWS model frames of one chunk (tile = {descriptor, first model frame j, rows, output row}):
// the feature rows as feed_splice_kernel (frames j sub - ctx .. j sub + ctx, zero outside [0, n)), and the label rows of frames
// j sub, rasterised from the recording's segments {start_frame, end_frame, speaker} by the reference's rule (feature.py:301-317).
__global__ __launch_bounds__(256)
void chunk_splice_label_kernel(const long* __restrict__ desc, const long* __restrict__ tiles, const int* __restrict__ segs,
                               const float* __restrict__ Y, float* __restrict__ feats, float* __restrict__ labels, int S_max,
                               int ctx, int sub) {
    const long* t = tiles + 4 * (long)blockIdx.x;
    const long* d = desc + CHUNK_N * t[0];
    const long j0 = t[1], n = d[CHUNK_FRAMES];
    const int rows = (int)t[2], W = NMEL * (2 * ctx + 1);
    const float* Ys = Y + d[CHUNK_YBASE] * NMEL;
    float* o = feats + t[3] * W;
    for (int i = threadIdx.x; i < rows * W; i += 256) {
        const int r = i / W;
        o[i] = splice_at(Ys, 0, n, 0, j0 + r, i - r * W, NMEL, ctx, sub);
    }
    const long start = d[CHUNK_START], end = d[CHUNK_END], seg0 = d[CHUNK_SEG0], seg1 = d[CHUNK_SEG1];
    float* lab = labels + t[3] * S_max;
    for (int i = threadIdx.x; i < rows * S_max; i += 256) {
        const int r = i / S_max, s = i - r * S_max;
        const long f = (j0 + r) * sub;                              // < n: the tile's rows are model frames of the chunk
        float v = 0.f;
        for (long g = seg0; g < seg1; ++g) {
            const int* sg = segs + 3 * g;
            if (sg[2] != s) continue;
            const long sf = sg[0], ef = sg[1];
            const bool has_a = start <= sf && sf < end, has_b = start < ef && ef <= end;
            if (!has_a && !has_b) continue;                         // also a segment that covers the whole chunk
            const long lo = has_a ? sf - start : 0, hi = has_b ? ef - start : n;
            if (f >= lo && f < hi) v = 1.f;
        }
        lab[i] = v;
    }
}

}  // namespace

int eend_launch_stft_logmel(const float* y, long len, long first, int n_frames, const float* dft, const float* melT, float* out,
                            hipStream_t stream) {
    if (!y || !dft || !melT || !out || len <= 0 || n_frames <= 0) return EEND_EINVAL;
    static EendOncePerDevice attr_once;
    if (!eend_set_dynamic_lds(attr_once, (const void*)stft_logmel_kernel, SM_BYTES)) return EEND_ELAUNCH;
    hipLaunchKernelGGL(stft_logmel_kernel, dim3((n_frames + FB - 1) / FB), dim3(256), SM_BYTES, stream, y, len, first, n_frames, dft, melT, out);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_colnorm(const float* Y, float* out, int T, int F, int mode, hipStream_t stream) {
    if (!Y || !out || T <= 0 || F <= 0 || mode < 1 || mode > 2) return EEND_EINVAL;
    hipLaunchKernelGGL(colnorm_kernel, dim3(F), dim3(NT2), 0, stream, Y, out, T, F, mode);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_splice_subsample(const float* Y, int T, int F, int ctx, int sub, float* out, hipStream_t stream) {
    if (!Y || !out || T <= 0 || F <= 0 || ctx < 0 || sub < 1) return EEND_EINVAL;
    const int To = (T + sub - 1) / sub;
    const long n = (long)To * F * (2 * ctx + 1);
    hipLaunchKernelGGL(splice_subsample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, Y, T, F, ctx, sub, To, out);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_audio_feed(const long* desc, int n_desc, const long* stft_tiles, int n_stft, const long* splice_tiles, int n_splice,
                           float* tail, float* ring, double* sums, float* Y, float* out, int mode, int ctx, int sub,
                           const float* dft, const float* melT, hipStream_t stream) {
    if (n_desc < 0 || n_stft < 0 || n_splice < 0 || (mode != 0 && mode != 2) || ctx < 0 || ctx > 15 || sub < 1 || sub > 16)
        return EEND_EINVAL;
    if (n_desc == 0) return (n_stft || n_splice) ? EEND_EINVAL : EEND_OK;
    if (!desc || !tail || !ring || !sums || (n_stft && (!stft_tiles || !Y || !dft || !melT)) || (n_splice && (!splice_tiles || !out)))
        return EEND_EINVAL;
    if (n_stft) {
        static EendOncePerDevice attr_once;
        if (!eend_set_dynamic_lds(attr_once, (const void*)feed_stft_kernel, SM_BYTES)) return EEND_ELAUNCH;
        hipLaunchKernelGGL(feed_stft_kernel, dim3(n_stft), dim3(256), SM_BYTES, stream, desc, stft_tiles, tail, dft, melT, Y);
    }
    hipLaunchKernelGGL(feed_state_kernel, dim3(n_desc), dim3(256), 0, stream, desc, tail, ring, sums, Y, mode);
    if (n_splice)
        hipLaunchKernelGGL(feed_splice_kernel, dim3(n_splice), dim3(256), 0, stream, desc, splice_tiles, Y, out, ctx, sub);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

namespace {
template <class S>
bool launch_chunk_stft(const void* corpus, const long* desc, const long* tiles, int n_tiles, const float* dft, const float* melT,
                       float* Y, hipStream_t stream) {
    static EendOncePerDevice attr_once;                          // one per instantiation
    if (!eend_set_dynamic_lds(attr_once, (const void*)chunk_stft_kernel<S>, SM_BYTES)) return false;
    hipLaunchKernelGGL(chunk_stft_kernel<S>, dim3(n_tiles), dim3(256), SM_BYTES, stream, (const S*)corpus, desc, tiles, dft, melT, Y);
    return true;
}
}  // namespace

int eend_launch_chunk_batch(const void* corpus, int storage, const int* segments, const long* desc, int n_chunks,
                            const long* stft_tiles, int n_stft, const long* splice_tiles, int n_splice, float* Y, float* Yn,
                            float* feats, float* labels, int S_max, int mode, int ctx, int sub, const float* dft, const float* melT,
                            hipStream_t stream) {
    if (n_chunks < 0 || n_chunks > 65535 || n_stft < 0 || n_splice < 0 || storage < 0 || storage > 1 || mode < 0 || mode > 2 ||
        ctx < 0 || ctx > 64 || sub < 1 || sub > 4096 || S_max < 1 || S_max > 64)
        return EEND_EINVAL;
    if (n_chunks == 0) return (n_stft || n_splice) ? EEND_EINVAL : EEND_OK;
    if (!desc || !segments || (n_stft && (!corpus || !stft_tiles || !Y || !dft || !melT || (mode && !Yn))) ||
        (n_splice && (!n_stft || !splice_tiles || !feats || !labels)))
        return EEND_EINVAL;
    if (n_stft) {
        const bool ok = storage == 0 ? launch_chunk_stft<float>(corpus, desc, stft_tiles, n_stft, dft, melT, Y, stream)
                                     : launch_chunk_stft<short>(corpus, desc, stft_tiles, n_stft, dft, melT, Y, stream);
        if (!ok) return EEND_ELAUNCH;
        if (mode) hipLaunchKernelGGL(chunk_colnorm_kernel, dim3(NMEL, n_chunks), dim3(NT2), 0, stream, desc, Y, Yn, mode);
    }
    if (n_splice)
        hipLaunchKernelGGL(chunk_splice_label_kernel, dim3(n_splice), dim3(256), 0, stream, desc, splice_tiles, segments,
                           mode ? Yn : Y, feats, labels, S_max, ctx, sub);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
