// Causal prefill attention over the FS-EEND multi-stream K/V caches (FsMultiStreamSession.prefill, fs_multistream.py): Nseq
// sequences with the same history length t0 take Tq new frames each in one call -- FS-EEND/nnet/modules/streaming_tfm.py:15-37
// applied to the Tq frames in order.  Row i*Tq + j of qkv is frame j of call sequence i = cache sequence seq0 + i: its k / v
// land in cache row t0 + j (bit-exact copies of the qkv columns) and its output row is the softmax attention of query j over
// cache keys [0, t0 + j].
// Two launches.  The append launch copies the k / v columns into the caches.  The flash launch takes one work item per
// (sequence, head, 128-query tile): a workgroup of four waves, 32 queries (two 16-query MFMA tiles) per wave, walks cache keys
// [0, t0 + end of its tile) once in 64-key tiles anchored at key 0.  A tile's K rows and V^T (keys in the k order of the second
// product) lie in LDS for all four waves; the next tile's global loads are in flight while the current one is computed.  Per
// 32-key chunk and 16-query tile S^T = K Q^T and O^T += V^T P^T run on mfma_f32_16x16x32_f16 with an online softmax, and P^T feeds
// the second product straight from the score registers (decode_mfma_step of decode_tile.h, the step attn_chunk_ragged_kernel
// of stream_chunk.hip runs): k index 8h + e of the second product stands for key 4h + e (e < 4) or 16 + 4h + e - 4 of the
// chunk.  Causal tiles differ in length, so block ids count the query tiles down: the long items start first.  A row's result
// depends on its own sequence, t0 and Tq alone: not on cap, seq0, the other sequences or cache rows at or beyond t0 + Tq,
// which are never read.
// Few queries over a long history give few work items: that case stays with the chunk attention of step_frames.
#include "common.h"
#include "kernels.h"
#include "decode_tile.h"

namespace {

constexpr int PF_QB = 128;                               // queries per workgroup (32 per wave)
constexpr int PF_KT = 64;                                // keys per LDS tile

// key kk (0..31) of a chunk -> its k index in the second product
DEV int pf_slot(int kk) { return kk < 16 ? 8 * (kk >> 2) + (kk & 3) : 8 * ((kk - 16) >> 2) + 4 + (kk & 3); }

// One thread per 16-byte piece: (row, head, 8 halves of the head's 64).
__global__ __launch_bounds__(256)
void attn_prefill_append_kernel(const _Float16* __restrict__ qkv, long ldq, _Float16* __restrict__ Kc, _Float16* __restrict__ Vc,
                                int seq0, int H, int cap, int t0, int Tq, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int piece = (int)(idx & 7);
    const long rh = idx >> 3;
    const int h = (int)(rh % H);
    const long row = rh / H;
    const int i = (int)(row / Tq), j = (int)(row - (long)i * Tq);
    const int D = H * 64;
    const _Float16* src = qkv + row * ldq + h * 64 + piece * 8;
    const size_t dst = ((((size_t)(seq0 + i) * H + h) * cap) + t0 + j) * 64 + piece * 8;
    *(f16x8*)(Kc + dst) = *(const f16x8*)(src + D);
    *(f16x8*)(Vc + dst) = *(const f16x8*)(src + 2 * D);
}

__global__ __launch_bounds__(256)
void attn_prefill_kernel(const _Float16* __restrict__ qkv, long ldq, const _Float16* __restrict__ Kc, const _Float16* __restrict__ Vc,
                         _Float16* __restrict__ out, int seq0, int NH, int H, int cap, int t0, int Tq, int nqt, float scale) {
    __shared__ __attribute__((aligned(16))) unsigned char ksm[PF_KT * 128];     // K tile: [key][64 d], swz128
    __shared__ __attribute__((aligned(16))) unsigned char vsm[64 * 128];        // V^T tile: [d][64 k slots], swz128
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, hq = lane >> 4;
    const int item = blockIdx.x;
    const int qtile = nqt - 1 - item / NH;                          // the long items first
    const int sh = item % NH;
    const int i = sh / H, h = sh - i * H;
    const int D = H * 64;
    const int q0 = qtile * PF_QB;
    const int qn = Tq - q0 < PF_QB ? Tq - q0 : PF_QB;               // queries of this tile (>= 1)
    const int kend = t0 + q0 + qn;                                  // keys [0, kend): never beyond t0 + Tq
    const _Float16* Kh = Kc + ((size_t)(seq0 + i) * H + h) * cap * 64;
    const _Float16* Vh = Vc + ((size_t)(seq0 + i) * H + h) * cap * 64;
    const int qw = q0 + wave * 32;                                  // this wave's first query
    const bool wave_live = qw < Tq;

    f16x8 qf[2][2];                                                 // B operand of S^T: Q^T[d = 32 ks + 8 hq + e][query col]
    f32x4 o[2][4];                                                  // O^T tiles: rows d = 16 dt + 4 hq + r, column = query
    float m_run[2], l_run[2];
    int lim[2], last[2];                                            // this lane's last visible key; the tile's last visible key
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int j = qw + qt * 16 + col;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qf[qt][ks] = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
            if (j < Tq) qf[qt][ks] = *(const f16x8*)(qkv + ((size_t)i * Tq + j) * ldq + h * 64 + ks * 32 + hq * 8);
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[qt][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        m_run[qt] = -INFINITY;
        l_run[qt] = 0.f;
        lim[qt] = t0 + (j < Tq ? j : Tq - 1);
        const int jl = qw + qt * 16 + 15;
        last[qt] = qw + qt * 16 < Tq ? t0 + (jl < Tq ? jl : Tq - 1) : -1;      // -1: a tile of padding only, never computed
    }

    // global -> registers for one 64-key tile: K rows as they are (thread: row p >> 3, piece p & 7), V by (key, 8-d group) so that
    // the transposing LDS stores of a half wave go to one row of V^T; rows at or beyond kend are zeros (stale rows may hold anything)
    f16x8 kreg[2], vreg[2];
    const int vkk = tid & 31, vdg = tid >> 5;
    auto fetch = [&](int tile0) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int p = tid + 256 * it;
            const int kr = tile0 + (p >> 3), vr = tile0 + it * 32 + vkk;
            kreg[it] = kr < kend ? *(const f16x8*)(Kh + (size_t)kr * 64 + (p & 7) * 8) : (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
            vreg[it] = vr < kend ? *(const f16x8*)(Vh + (size_t)vr * 64 + vdg * 8) : (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
        }
    };
    fetch(0);
    for (int tile0 = 0; tile0 < kend; tile0 += PF_KT) {
        __syncthreads();                                            // the previous tile has been read
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int p = tid + 256 * it;
            *(f16x8*)(ksm + swz128(p >> 3, p & 7)) = kreg[it];
            const int slot = it * 32 + pf_slot(vkk);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                *(_Float16*)(vsm + swz128(vdg * 8 + e, slot >> 3) + (slot & 7) * 2) = vreg[it][e];
        }
        __syncthreads();
        if (tile0 + PF_KT < kend) fetch(tile0 + PF_KT);
        if (!wave_live) continue;
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            const int c0 = tile0 + ch * 32;
            if (c0 > last[0] && c0 > last[1]) break;                // beyond every query of this wave (wave-uniform)
            f16x8 kf[2][2], vf[4];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) kf[kt][ks] = *(const f16x8*)(ksm + swz128(ch * 32 + kt * 16 + col, ks * 4 + hq));
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) vf[dt] = *(const f16x8*)(vsm + swz128(dt * 16 + col, ch * 4 + hq));
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                if (c0 > last[qt]) continue;                        // wave-uniform; key c0 is visible to the tile's last query
                // finite row maximum: key 0, in the first chunk, is visible to every query
                decode_mfma_step(kf, vf, qf[qt], o[qt], m_run[qt], l_run[qt], c0, hq, scale, [&](int key) { return key <= lim[qt]; });
            }
        }
    }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int j = qw + qt * 16 + col;
        float l = l_run[qt];
        l = wave_xor_add(l, 16);
        l = wave_xor_add(l, 32);
        if (j < Tq) {
            const float inv = 1.f / l;
            _Float16* dst = out + ((size_t)i * Tq + j) * D + h * 64 + hq * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                f16x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = to_f16_sat(o[qt][dt][r] * inv);
                *(f16x4*)(dst + dt * 16) = v;
            }
        }
    }
}

}  // namespace

int eend_launch_attn_prefill(const void* qkv, long ldq, void* Kc, void* Vc, void* out16, int Ncache, int seq0, int Nseq, int H, int cap,
                             int t0, int Tq, float scale, hipStream_t stream) {
    if (!qkv || !Kc || !Vc || !out16 || Ncache <= 0 || seq0 < 0 || Nseq <= 0 || (long)seq0 + Nseq > Ncache || H <= 0 || cap <= 0 ||
        t0 < 0 || Tq < 1 || (long)t0 + Tq > cap || ldq < 3L * H * 64 || (ldq & 7) ||
        (((size_t)qkv | (size_t)Kc | (size_t)Vc | (size_t)out16) & 15))
        return EEND_EINVAL;
    const int nqt = (Tq + PF_QB - 1) / PF_QB;
    const long items = (long)Nseq * H * nqt, pieces = (long)Nseq * Tq * H * 8;
    if (items > 0x7fffffffL || (pieces + 255) / 256 > 0x7fffffffL) return EEND_EINVAL;
    hipLaunchKernelGGL(attn_prefill_append_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, stream, (const _Float16*)qkv, ldq,
                       (_Float16*)Kc, (_Float16*)Vc, seq0, H, cap, t0, Tq, pieces);
    if (hipGetLastError() != hipSuccess) return EEND_ELAUNCH;
    hipLaunchKernelGGL(attn_prefill_kernel, dim3((unsigned)items), dim3(256), 0, stream, (const _Float16*)qkv, ldq, (const _Float16*)Kc,
                       (const _Float16*)Vc, (_Float16*)out16, seq0, Nseq * H, H, cap, t0, Tq, nqt, scale);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
