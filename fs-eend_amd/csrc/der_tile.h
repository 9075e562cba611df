// The tile layout and the reference-side staging that der_collar.hip and der_sweep.hip share: both walk tiles of DER_TILE label
// frames with 256 threads, thread (i, j) = (tid / 16, tid % 16) owning one co-occurrence count.
#pragma once
#include "common.h"
#include "kernels.h"

namespace der {

constexpr int CMAX = DER_CMAX;                    // speakers per side
constexpr int TILE = DER_TILE;                    // reference frames per tile
constexpr int HMAX = DER_HMAX;                    // largest half collar
constexpr int NT = 256;                           // threads: thread (i, j) = (tid / 16, tid % 16) owns cooc[i][j]
constexpr int EXT = TILE + 2 * HMAX;              // reference frames a tile reads
constexpr int NWORDS = (EXT + 63) / 64;           // boundary-bit words
constexpr int NGRP = TILE / 64;                   // 64-frame groups of a tile
constexpr int STAGE_WORDS = NT * CMAX / 4 + 1;    // NT rows of CMAX bytes, entered at any byte of the first word
static_assert(TILE % NT == 0 && NT == CMAX * CMAX && NWORDS <= NT, "der_collar tile layout");

// mask[e] = speaker bits of frame f0 + e of a recording of `len` frames (row `row0 + f` of `rows`, C bytes each; non-zero:
// active), 0 outside [0, len), for e in [0, n).  NT frames per round; `stage` is free for other use on return.
DEV void load_masks(const unsigned char* __restrict__ rows, long row0, int len, int C, int f0, int n, unsigned short* mask,
                    unsigned* stage) {
    const int tid = threadIdx.x;
    for (int c0 = 0; c0 < n; c0 += NT) {
        int fa = f0 + c0, fb = f0 + (c0 + NT < n ? c0 + NT : n);
        fa = fa < 0 ? 0 : fa;
        fb = fb > len ? len : fb;
        unsigned lead = 0;
        if (fa < fb) {
            const uintptr_t p = (uintptr_t)rows + (size_t)(row0 + fa) * C, pe = p + (size_t)(fb - fa) * C;
            const uintptr_t a = p & ~(uintptr_t)3;
            lead = (unsigned)(p - a);
            const int nw = (int)((pe - a + 3) >> 2);
            for (int k = tid; k < nw; k += NT) {
                const uintptr_t q = a + 4 * (uintptr_t)k;
                unsigned v = 0;
                if (q >= p && q + 4 <= pe) v = *(const unsigned*)q;
                else
                    for (int b = 0; b < 4; ++b)
                        if (q + b >= p && q + b < pe) v |= (unsigned)*(const unsigned char*)(q + b) << (8 * b);
                stage[k] = v;
            }
        }
        __syncthreads();
        const int e = c0 + tid, f = f0 + e;
        if (e < n) {
            unsigned m = 0;
            if (f >= fa && f < fb) {
                const unsigned char* s = (const unsigned char*)stage + lead + (size_t)(f - fa) * C;
                for (int c = 0; c < C; ++c) m |= (s[c] != 0 ? 1u : 0u) << c;
            }
            mask[e] = (unsigned short)m;
        }
        __syncthreads();
    }
}

// a median the sweep scores: odd, 1 .. DER_SWEEP_KMAX
DEV bool median_ok(int k) { return k >= 1 && k <= DER_SWEEP_KMAX && (k & 1); }

}  // namespace der
