// Audio ingest in front of the incremental front-end (eend_audio_ingest): live audio at its own sample rate and encoding ->
// f32 samples at 8 kHz, for many streams ("slots") per call.  Decoding: f32 as is, 16-bit PCM / 32768, G.711 mu-law and A-law
// through a 256-entry table each.  Rate conversion rate -> 8000 Hz with L = 8000 / gcd, M = rate / gcd and a windowed-sinc
// prototype h[-H..H] on the rate * L grid, stored phase-major: table f32 [L][P], row (n M) mod L holds the taps of output n in
// the order of its input samples k = ceil((n M - H) / L) .. floor((n M + H) / L), zero-padded to P = 2 H / L + 1:
//
//     y[n] = sum_k h[n M - k L] x[k],   x zero outside [0, n_in)
//
// accumulated in f32 with fmaf from zero in ascending k.  That order is the contract: an output's bits depend on its own taps
// and samples only, not on where chunks, tiles or the history end.  The whole job is VALU on LDS (an hour of 48 kHz audio is
// about 6 GFLOP); the matrix pipe would reorder the sum.
//
// Per slot the device keeps hist f32 [256]: the decoded samples ceil((n M - H) / L) .. recv - 1 that its next output n still
// needs (at most P - 1 of them).  The host owns all counters and builds one descriptor per slot named in the call (ING_*
// fields) and the tile table.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int NT = 256;                              // threads per workgroup = outputs per tile = history row
constexpr int XS = INGEST_SPAN;                      // LDS floats: the input span of one tile
enum { ING_CHUNK, ING_RECV0, ING_RECV1, ING_OUT0, ING_OUT1, ING_ROW, ING_ENDED, ING_SLOT, ING_N };
enum { ENC_F32, ENC_S16, ENC_MULAW, ENC_ALAW };

__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }
__device__ __forceinline__ long lmax(long a, long b) { return a > b ? a : b; }

__device__ __forceinline__ long ceil_div(long a, long b) {           // b > 0, any a
    const long q = a / b;
    return q + (a % b > 0);
}

__device__ __forceinline__ long floor_div(long a, long b) {          // b > 0, any a
    const long q = a / b;
    return q - (a % b < 0);
}

// First input sample output n reads (not clamped at 0)
__device__ __forceinline__ long first_tap(long n, int L, int M, int H) { return ceil_div(n * M - H, L); }

__device__ __forceinline__ float decode_at(const void* chunk, long i, int enc, const float* __restrict__ decode) {
    switch (enc) {
    case ENC_F32: return ((const float*)chunk)[i];
    case ENC_S16: return (float)((const short*)chunk)[i] * (1.f / 32768.f);
    case ENC_MULAW: return decode[((const unsigned char*)chunk)[i]];
    default: return decode[256 + ((const unsigned char*)chunk)[i]];
    }
}

// Decoded sample idx of a slot's stream during a call: zero before 0 and from recv1 on, from the new chunk from recv0 on, from
// the history (which starts at sample hb0) below.
__device__ __forceinline__ float sample_at(long idx, const long* __restrict__ d, long hb0, const float* __restrict__ hrow, int enc,
                                           const float* __restrict__ decode) {
    if (idx < 0 || idx >= d[ING_RECV1]) return 0.f;
    if (idx >= d[ING_RECV0]) return decode_at((const void*)d[ING_CHUNK], idx - d[ING_RECV0], enc, decode);
    const long q = idx - hb0;
    return (q >= 0 && q < NT) ? hrow[q] : 0.f;
}

// One workgroup per tile {descriptor, first output, outputs <= 256}, one output per thread.  The tile's input span, at most
// 255 M / L + P samples, is staged in LDS already decoded; each thread then runs the taps of its phase row over it.
__global__ __launch_bounds__(NT)
void ingest_resample_kernel(const long* __restrict__ desc, const long* __restrict__ tiles, const float* __restrict__ hist,
                            const float* __restrict__ table, const float* __restrict__ decode, int L, int M, int H, int P, int enc,
                            float* __restrict__ out) {
    __shared__ float xs[XS];
    const int tid = threadIdx.x;
    const long* t = tiles + 3 * (long)blockIdx.x;
    const long* d = desc + ING_N * t[0];
    const long n0 = t[1];
    const int cnt = (int)lmin(t[2], (long)NT);
    const long lo = first_tap(n0, L, M, H), hi = floor_div((n0 + cnt - 1) * M + H, L);
    const long hb0 = lmax(0L, first_tap(d[ING_OUT0], L, M, H));
    const float* hrow = hist + d[ING_SLOT] * NT;
    const int span = (int)lmin(hi - lo + 1, (long)XS);
    for (int i = tid; i < span; i += NT) xs[i] = sample_at(lo + i, d, hb0, hrow, enc, decode);
    __syncthreads();
    if (tid >= cnt) return;
    const long n = n0 + tid, nm = n * M;
    const long k0 = ceil_div(nm - H, L);
    const int taps = (int)(floor_div(nm + H, L) - k0) + 1;             // P or P - 1
    const int phase = (int)(nm - floor_div(nm, L) * L);                 // uniform (0) when L == 1
    const float* c = table + (long)phase * P;
    const float* x = xs + (k0 - lo);
    float acc = 0.f;
    for (int j = 0; j < taps; ++j) acc = fmaf(c[j], x[j], acc);
    out[d[ING_ROW] + (n - d[ING_OUT0])] = acc;
}

// One workgroup per descriptor: the slot's new history, samples max(0, first tap of output out1) .. recv1 - 1, read from the old
// history and the chunk before the barrier and written in place after it.  A launch of its own after the resample launch: the
// tiles of a slot read the old history, and stream order is the only fence between workgroups.
__global__ __launch_bounds__(NT)
void ingest_history_kernel(const long* __restrict__ desc, float* __restrict__ hist, const float* __restrict__ decode, int L, int M, int H,
                           int enc) {
    const int tid = threadIdx.x;
    const long* d = desc + ING_N * (long)blockIdx.x;
    if (d[ING_ENDED]) return;                                           // no output follows: the row is dead until the slot is reset
    float* hrow = hist + d[ING_SLOT] * NT;
    const long hb0 = lmax(0L, first_tap(d[ING_OUT0], L, M, H));
    const long hb1 = lmax(0L, first_tap(d[ING_OUT1], L, M, H));
    const float v = sample_at(hb1 + tid, d, hb0, hrow, enc, decode);
    __syncthreads();
    hrow[tid] = v;
}

}  // namespace

int eend_launch_audio_ingest(const long* desc, int n_desc, const long* tiles, int n_tiles, float* hist, const float* table,
                             const float* decode, int L, int M, int H, int P, int encoding, float* out, hipStream_t stream) {
    if (n_desc < 0 || n_tiles < 0 || L < 1 || M < L || H < 0 || P < 1 || P > 255 || P != 2 * H / L + 1 || encoding < ENC_F32 ||
        encoding > ENC_ALAW || (255L * M) / L + P + 2 > XS)
        return EEND_EINVAL;
    if (n_desc == 0) return n_tiles ? EEND_EINVAL : EEND_OK;
    if (!desc || !hist || !table || !decode || (n_tiles && (!tiles || !out))) return EEND_EINVAL;
    if (n_tiles)
        hipLaunchKernelGGL(ingest_resample_kernel, dim3(n_tiles), dim3(NT), 0, stream, desc, tiles, hist, table, decode, L, M, H, P,
                           encoding, out);
    hipLaunchKernelGGL(ingest_history_kernel, dim3(n_desc), dim3(NT), 0, stream, desc, hist, decode, L, M, H, encoding);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
