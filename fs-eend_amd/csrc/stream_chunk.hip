// Many frames per slot in one FS-EEND multi-stream step (FsMultiStreamSession.step_frames, fs_multistream.py): each slot
// advances by its own number of frames, up to nmax, in one replay.  Rows are laid out as the batch forward's (B, C, Tp)
// slabs with B = S slots and Tp = nmax: row q * nmax + j is frame j of sequence q.  The kernels here are the per-slot
// pieces of that step: the chunk attention over ragged histories (a "chunked prefill" over the K/V caches), the look-ahead
// window over a chunk of frames and the history counters advanced by a count.
#include "common.h"
#include "kernels.h"
#include "decode_tile.h"

namespace {

// ---- chunk attention over ragged histories (FS-EEND/nnet/modules/streaming_tfm.py:15-37 applied to cnt frames in order).
// Sequence q (rows q*nmax .. +nmax-1 of qkv) belongs to slot s = q / rows_per_seq; t = len[s], c = cnt[s].  Query j < c sits
// at position t + j and attends over cache keys [0, t) and over the chunk's own keys 0..j; its k / v are appended at cache
// row t + j.  c == 0 or t + c > cap: caches untouched, every output row of the sequence zero.
// Split launch: grid (Nseq*H, ceil(cap / 512)); block sp reads cache keys [512 sp, min(512 sp + 512, t)) ONCE for all c
// queries and leaves one (o[64], max, sum) partial per query.  A wave takes 32-key chunks in turn; per chunk and per
// 16-query tile S^T = K Q^T and O^T += V^T P^T on mfma_f32_16x16x32_f16 (C/D: column = lane & 15 = query, rows
// 4 (lane >> 4) + r).  The P^T tile feeds the second product straight from the score registers: its k index 8h + e stands
// for key 4h + e (e < 4, first 16-key tile) or 16 + 4h + e - 4 (second tile), and V^T takes the same keys from a row-major
// LDS copy of the chunk (decode_mfma_step of decode_tile.h, the step the prefill runs).  The merge launch walks a query's
// partials in key order, then folds in the causal part inside the chunk, read from qkv (never from the cache: the appends of
// the same launch cannot race with it).
constexpr int CK_SV = 72;                                // LDS row stride of the V chunk (halves)

DEV bool chunk_live(int t, int c, int cap, int nmax) { return c > 0 && c <= nmax && t >= 0 && t + c <= cap; }

__global__ __launch_bounds__(256)
void attn_chunk_ragged_kernel(const _Float16* __restrict__ qkv, const _Float16* __restrict__ Kc, const _Float16* __restrict__ Vc,
                              float* __restrict__ part, int H, int cap, int nsplit, int nmax, int rows_per_seq,
                              const int* __restrict__ len, const int* __restrict__ cnt, float scale) {
    __shared__ _Float16 vs[4][32 * CK_SV];
    __shared__ float red[4][16][DT_PART];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int idx = blockIdx.x, sp = blockIdx.y;
    const int q = idx / H, h = idx - q * H;
    const int slot = q / rows_per_seq;
    const int t = __builtin_amdgcn_readfirstlane(len[slot]);
    const int c = __builtin_amdgcn_readfirstlane(cnt[slot]);
    const int k0 = sp * DT_R;
    if (!chunk_live(t, c, cap, nmax) || k0 >= t) return;            // the merge reads no partial of this block
    const int k1 = k0 + DT_R < t ? k0 + DT_R : t;
    const int D = H * 64;
    const int col = lane & 15, hq = lane >> 4;
    const int nt = (c + 15) >> 4;                                   // 16-query tiles in use (<= 4)
    const _Float16* Kh = Kc + (size_t)idx * cap * 64;
    const _Float16* Vh = Vc + (size_t)idx * cap * 64;

    f16x8 qf[4][2];                                                 // B operand of S^T: Q^T[d = 32 ks + 8 hq + e][query col]
    f32x4 o[4][4];                                                  // O^T tiles: rows d = 16 dt + 4 hq + r, column = query
    float m_run[4], l_run[4];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
        const int j = qt * 16 + col;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qf[qt][ks] = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
            if (qt < nt && j < c) qf[qt][ks] = *(const f16x8*)(qkv + ((size_t)q * nmax + j) * 3 * D + h * 64 + ks * 32 + hq * 8);
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[qt][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        m_run[qt] = -INFINITY;
        l_run[qt] = 0.f;
    }
    _Float16* myv = vs[wave];
    for (int c0 = k0 + wave * 32; c0 < k1; c0 += 128) {
        // K rows of the two 16-key tiles (A operand: row = key, k = d), zero beyond k1 (stale rows may hold anything)
        f16x8 kf[2][2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            const int key = c0 + kt * 16 + col;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                kf[kt][ks] = key < k1 ? *(const f16x8*)(Kh + (size_t)key * 64 + ks * 32 + hq * 8) : (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
        }
        // V chunk, row-major into this wave's LDS slice (rows beyond k1 as zeros: 0 * NaN would poison the product)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int g = i * 64 + lane, r = g >> 3, d0 = (g & 7) * 8;
            const f16x8 v8 = c0 + r < k1 ? *(const f16x8*)(Vh + (size_t)(c0 + r) * 64 + d0) : (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
            *(f16x8*)(myv + r * CK_SV + d0) = v8;
        }
        __builtin_amdgcn_wave_barrier();
        f16x8 vf[4];                                                // A operand of O^T: V^T[d = 16 dt + col][key of k slot 8 hq + e]
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int key = e < 4 ? 4 * hq + e : 16 + 4 * hq + e - 4;
                vf[dt][e] = myv[key * CK_SV + dt * 16 + col];
            }
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            if (qt >= nt) break;
            decode_mfma_step(kf, vf, qf[qt], o[qt], m_run[qt], l_run[qt], c0, hq, scale, [&](int key) { return key < k1; });
        }
        __builtin_amdgcn_wave_barrier();
    }
    // combine the four waves' (o, m, l) per query, one 16-query tile at a time, and leave the block's partial
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
        if (qt >= nt) break;
        float l = l_run[qt];
        l = wave_xor_add(l, 16);
        l = wave_xor_add(l, 32);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][col][dt * 16 + hq * 4 + r] = o[qt][dt][r];
        if (hq == 0) { red[wave][col][64] = m_run[qt]; red[wave][col][65] = l; }
        __syncthreads();
        for (int e = threadIdx.x; e < 16 * 64; e += 256) {
            const int jj = e >> 6, d = e & 63, j = qt * 16 + jj;
            if (j < c) decode_combine4<false>(&red[0][jj][0], 16 * DT_PART, d, part + (((size_t)idx * nsplit + sp) * nmax + j) * DT_PART);
        }
        __syncthreads();
    }
}

// One block per (sequence, head): the chunk's q / k / v of this head into LDS, the appends, then per query (a wave each,
// in turn) the partials in key order and the causal part inside the chunk (lane = key for the scores, lane = d for P.V).
__global__ __launch_bounds__(256)
void attn_chunk_ragged_merge_kernel(const _Float16* __restrict__ qkv, const float* __restrict__ part, _Float16* __restrict__ Kc,
                                    _Float16* __restrict__ Vc, _Float16* __restrict__ out, int H, int cap, int nsplit, int nmax,
                                    int rows_per_seq, const int* __restrict__ len, const int* __restrict__ cnt, float scale) {
    __shared__ float qs[64][65], ks[64][65], vsh[64][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int idx = blockIdx.x;
    const int q = idx / H, h = idx - q * H;
    const int slot = q / rows_per_seq;
    const int t = __builtin_amdgcn_readfirstlane(len[slot]);
    const int c = __builtin_amdgcn_readfirstlane(cnt[slot]);
    const int D = H * 64;
    const bool live = chunk_live(t, c, cap, nmax);
    const int cc = live ? c : 0;
    for (int j = wave; j < nmax; j += 4) {                          // rows j >= cnt (and every row of a dead sequence): zero
        if (j >= cc) out[((size_t)q * nmax + j) * D + h * 64 + lane] = (_Float16)0.f;
    }
    if (!live) return;
    for (int j = wave; j < c; j += 4) {
        const _Float16* row = qkv + ((size_t)q * nmax + j) * 3 * D + h * 64;
        const _Float16 kx = row[D + lane], vx = row[2 * D + lane];
        qs[j][lane] = (float)row[lane] * scale;
        ks[j][lane] = (float)kx;
        vsh[j][lane] = (float)vx;
        Kc[((size_t)idx * cap + t + j) * 64 + lane] = kx;          // append (rows >= t are never read in this launch)
        Vc[((size_t)idx * cap + t + j) * 64 + lane] = vx;
    }
    __syncthreads();
    const int ns = (t + DT_R - 1) / DT_R;
    for (int j = wave; j < c; j += 4) {
        float M = -INFINITY, L = 0.f, O = 0.f;
        decode_walk<false, true>(M, L, O, part + ((size_t)idx * nsplit * nmax + j) * DT_PART, (size_t)nmax * DT_PART, ns, lane);
        // in-chunk keys 0..j: lane = key
        float sc = -INFINITY;
        if (lane <= j) {
            float acc = 0.f;
#pragma unroll 16
            for (int d = 0; d < 64; ++d) acc = __builtin_fmaf(qs[j][d], ks[lane][d], acc);
            sc = acc;
        }
        float mc = sc;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) mc = wave_xor_max(mc, m);
        const float p = lane <= j ? __expf(sc - mc) : 0.f;
        float lc = p;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) lc = wave_xor_add(lc, m);
        float oc = 0.f;
        for (int kk = 0; kk <= j; ++kk) oc = __builtin_fmaf(__shfl(p, kk, 64), vsh[kk][lane], oc);
        decode_fold<true>(M, L, O, mc, lc, oc);
        out[((size_t)q * nmax + j) * D + h * 64 + lane] = to_f16_sat(O / L);
    }
}

// len[s] += cnt[s] for all s.
__global__ __launch_bounds__(256)
void counter_add_count_kernel(int* __restrict__ len, const int* __restrict__ cnt, int S) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S) len[s] += cnt[s];
}

// The look-ahead window over a chunk: slot s takes npush[s] frames x[s*nmax + j] (f32 -> the window's element type T: f16 for
// FS-EEND, f32 for the all-f32 LS frame step) and then ndummy[s] zero frames.
// With z = (the k stored taps, then the npush + ndummy new frames), the window after push m is z[m .. m + k - 1].  Conv
// input row s*nmax + i (i < ndec[s]) gets the window after push npush + ndummy - ndec + i + 1, rows i >= ndec zeros, and
// the stored window ends as z[P .. P + k - 1] -- what P calls of window_push_kernel leave.  A thread owns one channel of
// one slot.  Counts out of range (P > nmax or ndec > P) leave the slot alone with zero rows.
template <typename T>
__global__ __launch_bounds__(256)
void window_chunk_kernel(T* __restrict__ win, const float* __restrict__ x, T* __restrict__ cols,
                         const int* __restrict__ npush, const int* __restrict__ ndummy, const int* __restrict__ ndec,
                         int S, int nmax, int k, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * D) return;
    const int s = i / D, ch = i - s * D;
    int np = npush[s], nd = ndummy[s], ne = ndec[s];
    const int P = np + nd;
    if (np < 0 || nd < 0 || ne < 0 || P > nmax || ne > P) np = nd = ne = 0;
    T* w = win + (size_t)s * k * D + ch;
    const float* xs = x + (size_t)s * nmax * D + ch;
    auto z = [&](int u) -> T {
        if (u < k) return w[(size_t)u * D];
        u -= k;
        return u < np ? (T)xs[(size_t)u * D] : (T)0.f;
    };
    for (int r = 0; r < nmax; ++r) {
        T* dst = cols + ((size_t)s * nmax + r) * k * D + ch;
        const int m = P - ne + r + 1;
        for (int tap = 0; tap < k; ++tap) dst[(size_t)tap * D] = r < ne ? z(m + tap) : (T)0.f;
    }
    if (P > 0)
        for (int tap = 0; tap < k; ++tap) w[(size_t)tap * D] = z(P + tap);      // ascending: reads index P + tap >= tap
}

}  // namespace

int eend_launch_attn_chunk_ragged(const void* qkv, void* Kc, void* Vc, void* out16, float* part, long part_floats, int Nseq, int H,
                                  int cap, int nmax, int rows_per_seq, const int* len, const int* cnt, float scale, hipStream_t stream) {
    if (!qkv || !Kc || !Vc || !out16 || !part || !len || !cnt || Nseq <= 0 || H <= 0 || cap <= 0 || nmax < 1 || nmax > 64 ||
        rows_per_seq <= 0 || Nseq % rows_per_seq)
        return EEND_EINVAL;
    const int nsplit = decode_nsplit(cap);
    if (nsplit > 65535 || (long)Nseq * H > 0x7fffffffL || (long)Nseq * nmax * 3 * H * 64 > 0x7fffffffL ||
        part_floats < decode_ws_floats(Nseq, H, cap, nmax))
        return EEND_EINVAL;
    hipLaunchKernelGGL(attn_chunk_ragged_kernel, dim3(Nseq * H, nsplit), dim3(256), 0, stream, (const _Float16*)qkv, (const _Float16*)Kc,
                       (const _Float16*)Vc, part, H, cap, nsplit, nmax, rows_per_seq, len, cnt, scale);
    if (hipGetLastError() != hipSuccess) return EEND_ELAUNCH;
    hipLaunchKernelGGL(attn_chunk_ragged_merge_kernel, dim3(Nseq * H), dim3(256), 0, stream, (const _Float16*)qkv, (const float*)part,
                       (_Float16*)Kc, (_Float16*)Vc, (_Float16*)out16, H, cap, nsplit, nmax, rows_per_seq, len, cnt, scale);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_counter_add_count(int* len, const int* cnt, int S, hipStream_t stream) {
    if (!len || !cnt || S <= 0) return EEND_EINVAL;
    hipLaunchKernelGGL(counter_add_count_kernel, dim3((S + 255) / 256), dim3(256), 0, stream, len, cnt, S);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_window_chunk(void* win16, const float* x, void* cols16, const int* npush, const int* ndummy, const int* ndec, int S,
                             int nmax, int k, int D, hipStream_t stream) {
    if (!win16 || !x || !cols16 || !npush || !ndummy || !ndec || S <= 0 || nmax < 1 || k < 1 || D <= 0 ||
        (long)S * nmax * k * D > 0x7fffffffL)
        return EEND_EINVAL;
    hipLaunchKernelGGL(window_chunk_kernel<_Float16>, dim3((S * D + 255) / 256), dim3(256), 0, stream, (_Float16*)win16, x, (_Float16*)cols16,
                       npush, ndummy, ndec, S, nmax, k, D);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_window_chunk_f32(float* win, const float* x, float* cols, const int* npush, const int* ndummy, const int* ndec, int S,
                                 int nmax, int k, int D, hipStream_t stream) {
    if (!win || !x || !cols || !npush || !ndummy || !ndec || S <= 0 || nmax < 1 || nmax > 64 || k < 1 || D <= 0 ||
        (long)S * nmax * k * D > 0x7fffffffL)
        return EEND_EINVAL;
    hipLaunchKernelGGL(window_chunk_kernel<float>, dim3((S * D + 255) / 256), dim3(256), 0, stream, win, x, cols, npush, ndummy, ndec, S,
                       nmax, k, D);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
