// Reverberant, noisy training mixtures from resident dry sources (eend_sim_mix_f32; the contract is in include/eend_hip.h and
// DESIGN 10d).  A mixture is up to 64 tracks; a track is utterances placed on a silent time line, convolved with a room impulse
// response scaled by a gain; the tracks are summed, a noise is added at a requested SNR:
//
//     y[t]   = sum_s sum_k a_s[k] d_s[t - k]                     f32, tracks ascending, taps ascending, one accumulator per output
//     out[t] = fmaf(scale, n[(o + t) mod L_n], y[t])             scale = f32(sqrt(c Ps / Pn)), Ps, Pn float64 sums
//
// The FIR is the whole cost (thousands of taps over minutes of audio) and runs on the exact-f32 matrix pipe as a Toeplitz
// product.  For a block of 256 consecutive outputs starting at u and one track,
//
//     Y[i][j] = y[u + 16 j + i] = sum_m A[i][m] B[m][j],   A[i][m] = a[m + i - 15],   B[m][j] = d[u + 16 j + 15 - m]
//
// over m = 0 .. K + 14 with a = 0 outside [0, K): the terms of output (i, j) in ascending m are its taps in ascending k,
// preceded and followed by zero products, which leave an f32 accumulator as it is.  v_mfma_f32_16x16x4_f32 is an m-ordered fmaf
// chain, so every output is exactly `acc = fmaf(a[k], d[t - k], acc)` for k = 0 .. K - 1, track after track: its bits depend on
// its own taps and samples only, not on the tile, the slice or the call it fell in.  Both operands are single LDS reads at
// lane-dependent addresses: lane l takes A[l & 15][m0 + (l >> 4)] = ta[m0 + (l >> 4) + (l & 15)] from the staged taps and
// B[m0 + (l >> 4)][l & 15] from the staged dry span.  Nothing is transposed.
//
// Item = (mixture, tile of SIM_TILE outputs), one workgroup of four waves, each wave two 256-output blocks (two independent
// accumulators cover the MFMA's dependent latency).  m runs in slices of at most SIM_SLICE steps; per (track, slice) the
// workgroup stages the slice's taps (SIM_SLICE + 15 floats) and the dry span its outputs read (SIM_TILE + slice - 16 samples),
// gathered from the utterance pool through the placement table: there is no dry-track copy in HBM.  A slice whose span meets no
// placement is skipped without staging (silences are a large share of a simulated mixture); this is the only data-dependent
// branch, and a skipped slice would have added zero products only.  The only flops beyond the taps are the 15 (18 at most,
// rounding K + 15 up to 4) zero columns per track.
//
// LDS banks: the B read strides 16 floats across the 16 columns, which would put them on two banks.  The span is stored with one
// pad float after every 16 (sample x at x + (x >> 4)), so the columns of one m sit 17 apart, on 16 different banks; the two m of
// a 32-lane group are neighbours and collide on at most one bank.  The A read touches 19 consecutive floats.
//
// The row passes: per tile the float64 sums of y^2 and noise^2 (256 partial sums of stride 256 in sample order, then a binary
// tree), per mixture the sums of its tiles in the same shape and the scale, then the noise add and the store (f32, or 16-bit PCM
// rounded half to even and clamped, the clamped samples counted per mixture with one integer atomic per workgroup).  Four
// launches whatever the call holds.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int NT = 256;
constexpr int TILE = SIM_TILE, SLICE = SIM_SLICE;
constexpr int SPAN = TILE + SLICE - 16;              // dry samples a full slice reads
constexpr int SPAN_P = SPAN + SPAN / 16 + 1;         // with a pad float after every 16
enum { MIX_N, MIX_OUT, MIX_TRACK0, MIX_NTRACKS, MIX_NOISE, MIX_NLEN, MIX_NOFF, MIX_C, MIX_TILE0, MIX_NTILES, MIX_WORDS };
enum { TRK_RIR, TRK_K, TRK_GAIN, TRK_PLACE0, TRK_NPLACE, TRK_WORDS };
enum { PLC_START, PLC_SRC, PLC_LEN, PLC_WORDS };
static_assert(MIX_WORDS == SIM_MIX_WORDS && TRK_WORDS == SIM_TRACK_WORDS && PLC_WORDS == SIM_PLACE_WORDS, "descriptor layout");
static_assert(TILE == 2048 && SLICE % 4 == 0 && SLICE >= 16, "four waves of two 256-output blocks; whole MFMA steps");

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }
__device__ __forceinline__ long lmax(long a, long b) { return a > b ? a : b; }

__device__ __forceinline__ float sample(const void* pool, int storage, long i) {
    return storage ? (float)((const short*)pool)[i] * (1.f / 32768.f) : ((const float*)pool)[i];
}

__global__ __launch_bounds__(NT)
void sim_fir_kernel(const void* __restrict__ utts, int storage, const float* __restrict__ rirs, const long* __restrict__ mix,
                    const long* __restrict__ tracks, const long* __restrict__ places, const long* __restrict__ tiles,
                    float* __restrict__ Y) {
    __shared__ float ta[SLICE + 16];
    __shared__ float dw[SPAN_P];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long* tl = tiles + 2 * (long)blockIdx.x;
    const long* md = mix + MIX_WORDS * tl[0];
    const long t0 = tl[1], N = md[MIX_N];
    const int li = lane & 15, lk = lane >> 4;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const int ntracks = (int)md[MIX_NTRACKS];
    for (int s = 0; s < ntracks; ++s) {
        const long* td = tracks + TRK_WORDS * (md[MIX_TRACK0] + s);
        const int K = (int)td[TRK_K];
        const float g = __int_as_float((int)td[TRK_GAIN]);
        const long rir = td[TRK_RIR];
        const long* pl = places + PLC_WORDS * td[TRK_PLACE0];
        const int npl = (int)td[TRK_NPLACE];
        const int Mr = (K + 15 + 3) & ~3;                                   // m steps of this track, whole MFMAs
        for (int ms = 0; ms < Mr; ms += SLICE) {
            const int Ls = Mr - ms < SLICE ? Mr - ms : SLICE;
            const int span = TILE + Ls - 16;
            const long tlo = t0 + 16 - ms - Ls;                             // dw[x] holds d[tlo + x]
            const long wlo = lmax(tlo, 0L), whi = lmin(tlo + span, N);
            int p0 = 0, p1 = npl;                                           // the first placement that ends after wlo: they are sorted
            while (p0 < p1) {                                               // and disjoint (uniform: every thread reads the same table)
                const int mid = (p0 + p1) >> 1;
                if (pl[PLC_WORDS * mid + PLC_START] + pl[PLC_WORDS * mid + PLC_LEN] <= wlo) p0 = mid + 1;
                else p1 = mid;
            }
            if (p0 == npl || pl[PLC_WORDS * p0 + PLC_START] >= whi) continue;
            __syncthreads();                                                // the previous slice has been read
            for (int x = tid; x < span + (span >> 4) + 1; x += NT) dw[x] = 0.f;
            for (int x = tid; x < Ls + 15; x += NT) {
                const int k = ms - 15 + x;
                ta[x] = (k >= 0 && k < K) ? (rir >= 0 ? __fmul_rn(g, rirs[rir + k]) : g) : 0.f;
            }
            __syncthreads();
            for (int p = p0; p < npl; ++p) {
                const long a = pl[PLC_WORDS * p + PLC_START], src = pl[PLC_WORDS * p + PLC_SRC];
                if (a >= whi) break;
                const long lo = lmax(a, wlo), hi = lmin(a + pl[PLC_WORDS * p + PLC_LEN], whi);
                for (long t = lo + tid; t < hi; t += NT) {
                    const int x = (int)(t - tlo);
                    dw[x + (x >> 4)] = sample(utts, storage, src + (t - a));
                }
            }
            __syncthreads();
            // B[m][j] of block q: d[t0 + 256 (2 wave + q) + 16 j + 15 - m] = dw at x = 256 (2 wave + q) + 16 j + Ls - 1 - (m - ms)
            // a turn of four steps moves x down by 16, its padded place by 17: the four places of a turn are kept, not recomputed
            const int xb = 512 * wave + 16 * li + Ls - 1 - lk;
            const float* tap = ta + lk + li;
            int pb[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) pb[q] = (xb - 4 * q) + ((xb - 4 * q) >> 4);
            int m = 0;
            for (; m + 16 <= Ls; m += 16) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float av = tap[4 * q];
                    const float b0 = dw[pb[q]], b1 = dw[pb[q] + 272];       // 256 samples on: 256 + 16 pads
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc1, 0, 0, 0);
                    pb[q] -= 17;
                }
                tap += 16;
            }
            for (; m < Ls; m += 4) {                                        // K + 15 is no multiple of 16: up to three more steps
                const int x0 = xb - m;
                const float av = ta[lk + li + m];
                const float b0 = dw[x0 + (x0 >> 4)], b1 = dw[x0 + (x0 >> 4) + 272];
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc1, 0, 0, 0);
            }
        }
    }
    // D[i][j]: lane holds rows i = 4 (lane >> 4) + r of column j = lane & 15, i.e. outputs u + 16 j + i
    float* y = Y + md[MIX_OUT];
    const long u = t0 + 512 * wave + 16 * li + 4 * lk;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (u + r < N) y[u + r] = acc0[r];
        if (u + 256 + r < N) y[u + 256 + r] = acc1[r];
    }
}

// Sum of the 256 threads' values in a fixed binary tree; the result is valid in thread 0.
__device__ __forceinline__ double tree_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    return red[0];
}

// One workgroup per tile: part[tile] = {sum y^2, sum noise^2} over the tile's samples below N.
__global__ __launch_bounds__(NT)
void sim_power_kernel(const float* __restrict__ Y, const void* __restrict__ noises, int nstorage, const long* __restrict__ mix,
                      const long* __restrict__ tiles, double* __restrict__ part) {
    __shared__ double red[NT];
    const int tid = threadIdx.x;
    const long* tl = tiles + 2 * (long)blockIdx.x;
    const long* md = mix + MIX_WORDS * tl[0];
    const long t0 = tl[1], t1 = lmin(t0 + TILE, md[MIX_N]);
    const long nl = md[MIX_NLEN], no = md[MIX_NOISE];
    const float* y = Y + md[MIX_OUT];
    double ps = 0.0, pn = 0.0;
    for (long t = t0 + tid; t < t1; t += NT) {
        const double v = (double)y[t];
        ps += v * v;
        if (nl > 0) {
            const double w = (double)sample(noises, nstorage, no + (md[MIX_NOFF] + t) % nl);
            pn += w * w;
        }
    }
    ps = tree_sum(ps, red);
    __syncthreads();
    pn = tree_sum(pn, red);
    if (tid == 0) {
        part[2 * (long)blockIdx.x] = ps;
        part[2 * (long)blockIdx.x + 1] = pn;
    }
}

// One workgroup per mixture: Ps, Pn from its tiles' partial sums, the scale, and the clamp counter back to zero.
__global__ __launch_bounds__(NT)
void sim_scale_kernel(const long* __restrict__ mix, const double* __restrict__ part, double* __restrict__ Ps, double* __restrict__ Pn,
                      float* __restrict__ scale, int* __restrict__ clipped) {
    __shared__ double red[NT];
    const int tid = threadIdx.x;
    const long* md = mix + MIX_WORDS * (long)blockIdx.x;
    const long tile0 = md[MIX_TILE0], ntiles = md[MIX_NTILES];
    double ps = 0.0, pn = 0.0;
    for (long i = tid; i < ntiles; i += NT) {
        ps += part[2 * (tile0 + i)];
        pn += part[2 * (tile0 + i) + 1];
    }
    ps = tree_sum(ps, red);
    __syncthreads();
    pn = tree_sum(pn, red);
    if (tid == 0) {
        const double c = __longlong_as_double(md[MIX_C]);
        const bool on = md[MIX_NLEN] > 0 && pn > 0.0 && ps > 0.0;
        Ps[blockIdx.x] = ps;
        Pn[blockIdx.x] = pn;
        scale[blockIdx.x] = on ? (float)sqrt(c * ps / pn) : 0.f;
        clipped[blockIdx.x] = 0;
    }
}

// One workgroup per tile: out = fmaf(scale, noise, y), stored as f32 or as 16-bit PCM.
__global__ __launch_bounds__(NT)
void sim_store_kernel(const float* __restrict__ Y, const void* __restrict__ noises, int nstorage, const long* __restrict__ mix,
                      const long* __restrict__ tiles, const float* __restrict__ scale, void* __restrict__ out, int ostorage,
                      int* __restrict__ clipped) {
    __shared__ int nclip;
    const int tid = threadIdx.x;
    const long* tl = tiles + 2 * (long)blockIdx.x;
    const long* md = mix + MIX_WORDS * tl[0];
    const long t0 = tl[1], t1 = lmin(t0 + TILE, md[MIX_N]);
    const long nl = md[MIX_NLEN], no = md[MIX_NOISE], base = md[MIX_OUT];
    const float sc = scale[tl[0]];
    if (tid == 0) nclip = 0;
    __syncthreads();
    int mine = 0;
    for (long t = t0 + tid; t < t1; t += NT) {
        float v = Y[base + t];
        if (nl > 0 && sc != 0.f) v = fmaf(sc, sample(noises, nstorage, no + (md[MIX_NOFF] + t) % nl), v);
        if (ostorage) {
            float r = rintf(v * 32768.f);                       // round to nearest, ties to even
            if (r > 32767.f) { r = 32767.f; ++mine; }
            if (r < -32768.f) { r = -32768.f; ++mine; }
            ((short*)out)[base + t] = (short)(int)r;
        } else {
            ((float*)out)[base + t] = v;
        }
    }
    if (ostorage) {
        if (mine) atomicAdd(&nclip, mine);
        __syncthreads();
        if (tid == 0 && nclip) atomicAdd(clipped + tl[0], nclip);
    }
}

}  // namespace

int eend_launch_sim_mix(const void* utts, int utt_storage, const float* rirs, const void* noises, int noise_storage, const long* mix,
                        int n_mix, const long* tracks, const long* places, const long* tiles, int n_tiles, float* Y, double* part,
                        void* out, int out_storage, double* Ps, double* Pn, float* scale, int* clipped, hipStream_t stream) {
    if (n_mix < 0 || n_mix > 65535 || n_tiles < 0 || utt_storage < 0 || utt_storage > 1 || noise_storage < 0 || noise_storage > 1 ||
        out_storage < 0 || out_storage > 1)
        return EEND_EINVAL;
    if (n_mix == 0) return n_tiles ? EEND_EINVAL : EEND_OK;
    if (n_tiles < n_mix || !utts || !rirs || !noises || !mix || !tracks || !places || !tiles || !Y || !part || !out || !Ps || !Pn ||
        !scale || !clipped)
        return EEND_EINVAL;
    hipLaunchKernelGGL(sim_fir_kernel, dim3(n_tiles), dim3(NT), 0, stream, utts, utt_storage, rirs, mix, tracks, places, tiles, Y);
    hipLaunchKernelGGL(sim_power_kernel, dim3(n_tiles), dim3(NT), 0, stream, Y, noises, noise_storage, mix, tiles, part);
    hipLaunchKernelGGL(sim_scale_kernel, dim3(n_mix), dim3(NT), 0, stream, mix, part, Ps, Pn, scale, clipped);
    hipLaunchKernelGGL(sim_store_kernel, dim3(n_tiles), dim3(NT), 0, stream, Y, noises, noise_storage, mix, tiles, scale, out,
                       out_storage, clipped);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
