// The "block owns whole 256-feature rows" epilogue of the tiled GEMM (gemm.hip, 64-row tiles, 4 waves) and the fused FFN family
// (ffn.hip, 128-row tiles, 8 waves): the row sum across the block's n-waves, the two-pass row statistics on it, and the two LDS
// staging images through which every global store instruction writes whole rows.  Device-only.
// ffn.hip runs on all of it; gemm.hip on static_for, the staging addresses, block_rowsum and row_stats (its write and store passes
// are its own text on these addresses: the shared ones cost its L2-norm and residual kernels registers).
//
// Accumulator layout of both kernels (weights are the MFMA "A" operand): acc[i][j][r] is feature n0 + i*16 + r of tile row
// row0 + j*16, where n0 already holds the lane's fkg*4 and row0 its frow (fkg = lane >> 4, frow = lane & 15).
#pragma once
#include "common.h"
#include <type_traits>
#include <utility>

// Compile-time loop: f(std::integral_constant<int, I>{}) for I in [0, N).  Register arrays
// indexed through it have constant indices at IR-generation time (a `#pragma unroll` loop
// variable is only constant after unrolling, too late for SROA -> the array lands in scratch).
template <class F, int... I>
DEV void static_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
DEV void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// tile row -> global row (or -1): plain contiguous row tiles
struct RowsContiguous {
    int m0, M;
    DEV int operator()(int r) const { return m0 + r < M ? m0 + r : -1; }
};

// ---- staging images ---------------------------------------------------------------------------
// f32 image, [rows][1 KB]: 16-B chunk c of row r at chunk c ^ (r & 7).  2-byte image, [rows][512 B]: 16-B chunk c of row r at
// chunk c ^ ((r >> 1) & 7).  _frag: where a lane's 4 consecutive features n .. n+3 of a row go; _row: what lane c of a whole-row
// read (64 lanes x 16 B = one f32 row, 32 lanes x 16 B = one 2-byte row) fetches.  Both directions are bank-conflict free.
DEV int stage32_frag(int row, int n) { return row * 1024 + (((n >> 2) ^ (row & 7)) << 4); }
DEV int stage32_row(int row, int c) { return row * 1024 + ((c ^ (row & 7)) << 4); }
DEV int stage16_frag(int row, int n) { return row * 512 + (((n >> 3) ^ ((row >> 1) & 7)) << 4) + ((n >> 2) & 1) * 8; }
DEV int stage16_row(int row, int c) { return row * 512 + ((c ^ ((row >> 1) & 7)) << 4); }

// Fragment-side write passes: val(i, j) is the lane's 4 values (f32x4 / a 4 x 2-byte vector) of accumulator fragment [i][j].
template <int FR, int FL, class Val>
DEV void stage_frags32(char* stg, int row0, int n0, Val&& val) {
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int j = 0; j < FL; ++j) *(f32x4*)(stg + stage32_frag(row0 + j * 16, n0 + i * 16)) = val(i, j);
}
template <int FR, int FL, class Val>
DEV void stage_frags16(char* stg, int row0, int n0, Val&& val) {
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int j = 0; j < FL; ++j) {
            const auto v = val(i, j);
            *(std::remove_const_t<decltype(v)>*)(stg + stage16_frag(row0 + j * 16, n0 + i * 16)) = v;
        }
}

// Store passes, staged tile -> dst[rowmap(row)][col0 ..]: one 1 KB row (f32) / two 512 B rows (2-byte) per wave instruction;
// NW waves share the ROWS rows of the tile, rows whose rowmap is negative are dropped.  (A barrier between the write pass and this.)
template <int NW, int ROWS, class RowMap>
DEV void store_rows32(const char* stg, float* __restrict__ dst, int ld, int col0, int wave, int lane, const RowMap rowmap) {
#pragma unroll
    for (int k = 0; k < ROWS / NW; ++k) {
        const int row = k * NW + wave;
        const f32x4 v = *(const f32x4*)(stg + stage32_row(row, lane));
        const auto gr = rowmap(row);
        if (gr >= 0) *(f32x4*)(dst + (size_t)gr * ld + col0 + lane * 4) = v;
    }
}
template <int NW, int ROWS, class T16, class RowMap>
DEV void store_rows16(const char* stg, T16* __restrict__ dst, int ld, int col0, int wave, int lane, const RowMap rowmap) {
#pragma unroll
    for (int k = 0; k < ROWS / (2 * NW); ++k) {
        const int row = (k * NW + wave) * 2 + (lane >> 5), c = lane & 31;
        const u32x4 v = *(const u32x4*)(stg + stage16_row(row, c));
        const auto gr = rowmap(row);
        if (gr >= 0) *(u32x4*)(dst + (size_t)gr * ld + col0 + c * 8) = v;
    }
}

// ---- row statistics ---------------------------------------------------------------------------
// part[j] (this lane's partial of tile row row0 + j*16) -> the row's sum over the whole block: the four fkg lane groups by two
// shuffles, the NWN n-waves through red[NWN][stride] (LDS; every thread of the block calls this: two barriers).  FROM_ZERO is the
// summation order over the n-waves, part of each kernel's bits: 0.f + w0 + w1 + ... (gemm.hip) or w0 + w1 + ... (ffn.hip).
template <int NWN, bool FROM_ZERO, int FL>
DEV void block_rowsum(float (&part)[FL], float* red, int stride, int wn, int row0, int fkg) {
#pragma unroll
    for (int j = 0; j < FL; ++j) {
        part[j] = wave_xor_add(part[j], 16);
        part[j] = wave_xor_add(part[j], 32);
    }
    __syncthreads();
    if (fkg == 0) {
#pragma unroll
        for (int j = 0; j < FL; ++j) red[wn * stride + row0 + j * 16] = part[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FL; ++j) {
        float s = FROM_ZERO ? 0.f + red[row0 + j * 16] : red[row0 + j * 16];
#pragma unroll
        for (int w = 1; w < NWN; ++w) s += red[w * stride + row0 + j * 16];
        part[j] = s;
    }
}

// Two-pass statistics of the rows in acc (nfeat = 1 / feature count).  LN: mean, then the centred squares, scale = 1/sqrt(var + eps);
// !LN, the L2 norm: mean = 0, scale = 1/||x||, eps unused.  after_mean() runs behind the first row sum (every wave is past
// whatever it read from LDS before the call).
template <bool LN, int NWN, bool FROM_ZERO, int FR, int FL, class Hook>
DEV void row_stats(const f32x4 (&acc)[FR][FL], float nfeat, float eps, float (&mean)[FL], float (&scale)[FL],
                   float* red, int stride, int wn, int row0, int fkg, Hook&& after_mean) {
    float part[FL];
    if constexpr (LN) {
#pragma unroll
        for (int j = 0; j < FL; ++j) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < FR; ++i) s += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
            part[j] = s;
        }
        block_rowsum<NWN, FROM_ZERO>(part, red, stride, wn, row0, fkg);
        after_mean();
#pragma unroll
        for (int j = 0; j < FL; ++j) mean[j] = part[j] * nfeat;
    } else {
#pragma unroll
        for (int j = 0; j < FL; ++j) mean[j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < FL; ++j) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < FR; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float d = acc[i][j][r] - mean[j]; s += d * d; }
        part[j] = s;
    }
    block_rowsum<NWN, FROM_ZERO>(part, red, stride, wn, row0, fkg);
#pragma unroll
    for (int j = 0; j < FL; ++j)
        scale[j] = LN ? 1.0f / __builtin_sqrtf(part[j] * nfeat + eps) : 1.0f / __builtin_sqrtf(part[j]);
}
template <bool LN, int NWN, bool FROM_ZERO, int FR, int FL>
DEV void row_stats(const f32x4 (&acc)[FR][FL], float nfeat, float eps, float (&mean)[FL], float (&scale)[FL],
                   float* red, int stride, int wn, int row0, int fkg) {
    row_stats<LN, NWN, FROM_ZERO>(acc, nfeat, eps, mean, scale, red, stride, wn, row0, fkg, [] {});
}
