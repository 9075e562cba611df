// The tile that der_collar.hip and der_sweep.hip score: both walk tiles of DER_TILE label frames with 256 threads, thread
// (i, j) = (tid / 16, tid % 16) owning one co-occurrence count.  Here, once, for both: the tile's constants, load_masks, and
// what the two launchers share (der_args_ok, der_clear, der_tile_groups); decision.h holds the scalar rules (winner_update,
// median_ok, median_of).  Also here, what der_collar.hip's two kernels are made of: the recording header (Rec), the tile's
// extents (Tile), the reference side of a tile (boundary_words, boundaries_below, ref_side) and the hypothesis side of one
// operating point (score_point, add_counter); der_sweep_pass_kernel holds the same in its own text (der_sweep.hip says why).
// The scoring regions of eend_collar_der_regions_u64 (Regions, region_clear, region_fill, region_bit) are one more term of keep:
// both kernels take it from here, as template instances of their own (REG), and the marginal times with it (MARG); the
// instances <false, false> are the kernels of the entries without regions, instruction for instruction.
#pragma once
#include "common.h"
#include "kernels.h"
#include "decision.h"

namespace der {

constexpr int CMAX = DER_CMAX;                    // speakers per side
constexpr int TILE = DER_TILE;                    // reference frames per tile
constexpr int HMAX = DER_HMAX;                    // largest half collar
constexpr int NT = 256;                           // threads: thread (i, j) = (tid / 16, tid % 16) owns cooc[i][j]
constexpr int EXT = TILE + 2 * HMAX;              // reference frames a tile reads
constexpr int NWORDS = (EXT + 63) / 64;           // boundary-bit words
constexpr int NGRP = TILE / 64;                   // 64-frame groups of a tile
constexpr int ROUNDS = TILE / NT;                 // reference frames per thread and tile
constexpr int STAGE_WORDS = NT * CMAX / 4 + 1;    // NT rows of CMAX bytes, entered at any byte of the first word
static_assert(TILE % NT == 0 && NT == CMAX * CMAX && NWORDS <= NT && ROUNDS == 4, "der_collar tile layout");

// Recording `rec` of a packed batch: its first rows, its lengths and T = max(Tr, Th * sub).  !ok: out of scope; the pass kernels
// leave its sums at 0 and der_collar_assign_kernel marks it.
struct Rec {
    long r0, h0, Tl;
    int Tr, Th, T, ntiles;
    bool ok;
};
DEV Rec rec_header(const int* __restrict__ roff, const int* __restrict__ hoff, int rec, int sub) {
    Rec R;
    R.r0 = roff[rec];
    R.h0 = hoff[rec];
    const long Trl = (long)roff[rec + 1] - R.r0, Thl = (long)hoff[rec + 1] - R.h0;
    R.Tl = Trl > Thl * sub ? Trl : Thl * sub;
    R.ok = Trl >= 0 && Thl >= 0 && R.Tl <= DER_MAX_FRAMES;
    R.Tr = (int)Trl;
    R.Th = (int)Thl;
    R.T = (int)R.Tl;
    R.ntiles = (int)((R.Tl + TILE - 1) / TILE);
    return R;
}

// Tile `tile` of a recording of T frames: reference frames t0 .. t0 + tl - 1, read with the halo as t0 - h .. t0 - h + n - 1;
// the hypothesis frames under them k0 .. k0 + nk - 1; ng 64-frame groups in the rounds that hold a frame.
struct Tile {
    int t0, tl, n, k0, nk, ng;
};
DEV Tile tile_extents(int tile, int T, int sub, int h) {
    Tile t;
    t.t0 = tile * TILE;                                           // < T <= DER_MAX_FRAMES, so t0 + TILE + 2 h stays an int
    t.tl = T - t.t0 < TILE ? T - t.t0 : TILE;
    t.n = t.tl + 2 * h;
    t.k0 = t.t0 / sub;
    t.nk = (t.t0 + t.tl - 1) / sub - t.k0 + 1;
    t.ng = ((t.tl + NT - 1) / NT) * (NT / 64);
    return t;
}

// mask[e] = speaker bits of frame f0 + e of a recording of `len` frames (row `row0 + f` of `rows`, C bytes each; non-zero:
// active), 0 outside [0, len), for e in [0, n).  NT frames per round; `stage` is free for other use on return.  n >= 1 (a tile
// holds a frame), so at least one round runs: callers count on its two barriers (der_collar_pass_kernel for wsum = 0).
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

// ---- the scoring regions of a recording (a UEM): sorted, disjoint, half-open intervals [s, e) of reference frames

// Recording `rec` of the table uem i32 [.][2] under the offsets uoff i32 [B + 1]: its n intervals from iv.
struct Regions {
    const int2* iv;
    int n;
};
DEV Regions rec_regions(const int* __restrict__ uem, const int* __restrict__ uoff, int rec) {
    Regions g;
    const int a = uoff[rec], n = uoff[rec + 1] - a;
    g.iv = (const int2*)uem + a;
    g.n = n > 0 ? n : 0;
    return g;
}

// What the kernels with regions take beyond the arguments of those without, as one argument: the table and the marginal times.
struct RegionArgs {
    const int *uem, *uoff;
    unsigned long long *ref_time, *hyp_time;
};
DEV const RegionArgs& region_args(const RegionArgs& x) { return x; }

// regw [NGRP]: bit j of the words = frame t0 + j of the tile lies in some interval.  region_clear, a barrier, region_fill, a
// barrier, then region_bit.  The fill: a binary search on the starts finds the first interval that reaches the tile; from there
// thread k takes every NT-th interval up to the first that starts beyond the tile, so a tile of hundreds of one-frame regions
// is a few rounds of the loop, not a fixed stage.  An interval ORs its bits into each word it meets (LDS atomics: two intervals
// may share a word).  The frames of a tile lie in [0, T), which clips the intervals; an unsorted table ends the loop early or
// late but writes nowhere else.
DEV void region_clear(unsigned long long* regw) {
    if (threadIdx.x < NGRP) regw[threadIdx.x] = 0;
}
DEV void region_fill(const Regions& g, int t0, int tl, unsigned long long* regw) {
    const int tend = t0 + tl;
    int lo = 0, hi = g.n;                                         // -> the intervals that start at or before t0
#pragma unroll 1
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (g.iv[mid].x <= t0) lo = mid + 1;
        else hi = mid;
    }
    const int first = lo > 0 && g.iv[lo - 1].y > t0 ? lo - 1 : lo;
#pragma unroll 1
    for (long k = (long)first + threadIdx.x; k < g.n; k += NT) {
        const int2 se = g.iv[k];
        if (se.x >= tend) break;
        const int a = (se.x > t0 ? se.x : t0) - t0, b = (se.y < tend ? se.y : tend) - t0;   // bits [a, b) of the tile
        if (a >= b) continue;
#pragma unroll 1
        for (int w = a >> 6; w <= (b - 1) >> 6; ++w) {
            const int x = a > w * 64 ? a - w * 64 : 0, y = b < w * 64 + 64 ? b - w * 64 : 64;
            const unsigned long long upto = y == 64 ? ~0ull : (1ull << y) - 1;
            atomicOr(regw + w, upto & ~((1ull << x) - 1));
        }
    }
}
// frame r NT + tid of the tile: word r NT / 64 + wave, bit lane
DEV bool region_bit(const unsigned long long* regw, int r) {
    return regw[r * (NT / 64) + (threadIdx.x >> 6)] >> (threadIdx.x & 63) & 1ull;
}

// ---- the reference side of a tile

// What the reference side leaves in LDS: the boundary bits, the boundaries in the words before each, the planes R_i & keep.
struct RefLds {
    unsigned long long bits[NWORDS], planes[NGRP][CMAX];
    unsigned before[NWORDS];
};
// ... and in a thread's registers, for its frames r NT + tid: byte r of nrk = nr if the frame is kept, else 0x80; the frame's
// hypothesis frame, from k0; the wave's ballot of keep.
struct RefRegs {
    unsigned nrk;
    int hidx[ROUNDS];
    unsigned long long kp[ROUNDS];
};

// bit e of `bits`: a boundary (mask[b - 1] != mask[b]) at b = t0 - h + 1 + e, e in [0, n - 1); the words up to that of position
// n - 1 are written, and before[w] = the boundaries in the words below w.  Ends after a barrier.
DEV void boundary_words(const unsigned short* rmask, int n, RefLds& L) {
    const int tid = threadIdx.x;
    for (int e0 = 0; e0 <= n - 1; e0 += NT) {
        const int e = e0 + tid;
        const unsigned long long w = __ballot(e < n - 1 && rmask[e] != rmask[e + 1]);
        if ((tid & 63) == 0 && e <= n - 1) L.bits[e >> 6] = w;
    }
    __syncthreads();
    if (tid < ((n - 1) >> 6) + 1) {
        unsigned c = 0;
        for (int k = 0; k < tid; ++k) c += __popcll(L.bits[k]);
        L.before[tid] = c;
    }
    __syncthreads();
}

// The boundaries below bit e = 64 w + k, with below = (1 << k) - 1.  Frame t = t0 + j is clear of the collar iff no boundary b
// lies in [t - h + 1, t + h]: bits [j, j + 2 h), so iff as many lie below j + 2 h as below j.
DEV unsigned boundaries_below(const RefLds& L, int w, unsigned long long below) {
    return L.before[w] + __popcll(L.bits[w] & below);
}

// From rmask (the tile's masks with the halo): keep and nr of every frame, total and frames kept added up per thread, the planes
// R_i & keep.  The caller's barrier comes before the planes are read or rmask is written.  REG: a kept frame also has its bit in
// regw (region_fill, a barrier since).  MARG: lane i < Cr of a wave adds the kept frames of speaker i in its groups to rtime.
template <bool REG = false, bool MARG = false>
DEV void ref_side(const Tile& t, const unsigned short* rmask, int Cr, int sub, int h, int skip, RefLds& L, RefRegs& f,
                  unsigned long long& total, unsigned long long& kept, const unsigned long long* regw = nullptr,
                  unsigned long long* rtime = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    boundary_words(rmask, t.n, L);
    // frame j = r NT + tid asks about bits j and j + 2 h: the same bit of a word in every round, NT / 64 words on per round
    const int lo = tid, hi = tid + 2 * h;
    const unsigned long long mlo = (1ull << (lo & 63)) - 1, mhi = (1ull << (hi & 63)) - 1;
    f.nrk = 0;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int j = r * NT + tid;
        const bool valid = j < t.tl;
        unsigned rr = 0;
        bool keep = valid;
        f.hidx[r] = 0;
        if (valid) {
            rr = rmask[h + j];
            f.hidx[r] = (t.t0 + j) / sub - t.k0;
            if (h > 0) {
                const int up = r * (NT / 64);
                keep = boundaries_below(L, (hi >> 6) + up, mhi) == boundaries_below(L, (lo >> 6) + up, mlo);
            }
        }
        const unsigned nr = __popc(rr);
        if (skip && nr >= 2) keep = false;
        if constexpr (REG) keep = keep && region_bit(regw, r);
        if (keep) {
            total += nr;
            kept += 1;
        }
        f.nrk |= (keep ? nr : 0x80u) << (8 * r);
        f.kp[r] = __ballot(keep);
        unsigned long long mine = 0;
        for (int s = 0; s < Cr; ++s) {
            const unsigned long long pr = __ballot(keep && (rr >> s & 1u));
            if (lane == s) mine = pr;
        }
        if (lane < CMAX) L.planes[r * (NT / 64) + wave][lane] = mine;
        if constexpr (MARG) *rtime += __popcll(mine);
    }
}

// ---- the hypothesis side of one operating point

// hm[k]: the speaker mask of hypothesis frame k0 + k at this point, complete before the call (a barrier lies between).  The
// planes H_j go to PH [NGRP][CMAX].  wsum [NT / 64][2], the point's sums per wave, in LDS and 0 at first: this wave's sum of nh
// over its kept frames (popcount(H_j & keep)) and of min(nr, nh) (ballots over the 7 bits of a thread's sum, <= 4 * 16) are
// added by lane 0, before the barrier that would otherwise expose the round trip.  Returns thread (i, j)'s
// popcount(R_i & keep & H_j) over the tile.  The next write to PH or L.planes must follow a barrier.  MARG: lane j < Ch of a wave
// adds the kept frames under hypothesis speaker j in its groups to htime.
template <bool MARG = false>
DEV unsigned score_point(const Tile& t, const RefLds& L, const RefRegs& f, const unsigned short* hm, int Cr, int Ch,
                         unsigned long long* PH, unsigned long long (*wsum)[2], unsigned long long* htime = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ci = tid >> 4, cj = tid & 15;
    unsigned bt = 0, nhw = 0, bw = 0;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r)
        if (r * NT < t.tl) {
            const unsigned m = r * NT + tid < t.tl ? hm[f.hidx[r]] : 0u;
            const unsigned nr = f.nrk >> (8 * r) & 0xffu, nh = __popc(m);
            if (nr < 0x80u) bt += nr < nh ? nr : nh;
            unsigned long long mine = 0;
            for (int s = 0; s < Ch; ++s) {
                const unsigned long long ph = __ballot(m >> s & 1u);
                if (lane == s) mine = ph;
                nhw += __popcll(ph & f.kp[r]);
            }
            if (lane < CMAX) PH[(r * (NT / 64) + wave) * CMAX + lane] = mine;
            if constexpr (MARG) *htime += __popcll(mine & f.kp[r]);
        }
#pragma unroll
    for (int b = 0; b < 7; ++b) bw += (unsigned)__popcll(__ballot(bt >> b & 1u)) << b;
    if (lane == 0) {
        wsum[wave][0] += nhw;
        wsum[wave][1] += bw;
    }
    __syncthreads();
    unsigned v = 0;
    if (ci < Cr && cj < Ch)
        for (int q = 0; q < t.ng; ++q) v += __popcll(L.planes[q][ci] & PH[q * CMAX + cj]);
    return v;
}

// A point's sums -> its counters, one by each of the threads k = 0 .. 4: total, missed detection = total - sum of min, false
// alarm = sum of nh - sum of min, frames kept and the sum of min(nr, nh); 64-bit integer atomics, since other workgroups add to
// the same recording.  Five threads in one instruction and not one thread five times: with one recording every workgroup of
// the grid adds to the same cache line, and added by one thread the call on one hour of one recording measured 0.109 ms for
// 0.096 ms (profiles/score_refactor/bench_pairs.txt).  der_sweep_pass_kernel keeps its own form, one thread per point: its G
// points lie in G cache lines.
DEV void add_counter(unsigned long long* out, int k, unsigned long long total, unsigned long long kept,
                     const unsigned long long (*wsum)[2]) {
    unsigned long long nhs = 0, both = 0;
    for (int w = 0; w < NT / 64; ++w) {
        nhs += wsum[w][0];
        both += wsum[w][1];
    }
    const unsigned long long v = k == 0 ? total : k == 1 ? total - both : k == 2 ? nhs - both : k == 3 ? kept : both;
    if (v) atomicAdd(out + (k < 3 ? k : k == 3 ? 5 : 7), v);
}

// ---- what the two launchers share

inline bool der_args_ok(int Cr, int Ch, int B, int sub, int h) {
    return Cr >= 1 && Cr <= CMAX && Ch >= 1 && Ch <= CMAX && B >= 1 && B <= 65535 && sub >= 1 && h >= 0 && h <= HMAX;
}

// the lengths live on the device, so the tile groups are sized by the batch alone: about 4096 workgroups, at most
// DER_MAX_GROUPS per recording; a group beyond a recording's last tile ends at once
inline int der_tile_groups(int B) {
    const int groups = 4096 / B;
    return groups < 1 ? 1 : (groups > DER_MAX_GROUPS ? DER_MAX_GROUPS : groups);
}

// counters and co-occurrence counts of n matrices start at 0.  A kernel, not hipMemsetAsync: memset nodes of a captured graph
// came back with other values than 0 on replay (seen once with eend_collar_der_u64 in torch.cuda.graph; a launch replays as it
// was recorded).
static __global__ __launch_bounds__(NT)
void der_clear_kernel(unsigned long long* __restrict__ counters, unsigned long long* __restrict__ cooc, long n) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i < (size_t)n * 8) counters[i] = 0;
    if (i < (size_t)n * CMAX * CMAX) cooc[i] = 0;
}
inline bool der_clear(unsigned long long* counters, unsigned long long* cooc, long n, hipStream_t stream) {
    hipLaunchKernelGGL(der_clear_kernel, dim3((unsigned)n), dim3(NT), 0, stream, counters, cooc, n);   // n x NT = n x 16 x 16 counts
    return hipGetLastError() == hipSuccess;
}
// ... and with them the marginal times of the entries with regions, 2 x 16 per matrix
static __global__ __launch_bounds__(NT)
void der_clear_times_kernel(unsigned long long* __restrict__ counters, unsigned long long* __restrict__ cooc,
                            unsigned long long* __restrict__ ref_time, unsigned long long* __restrict__ hyp_time, long n) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i < (size_t)n * 8) counters[i] = 0;
    if (i < (size_t)n * CMAX * CMAX) cooc[i] = 0;
    if (i < (size_t)n * CMAX) {
        ref_time[i] = 0;
        hyp_time[i] = 0;
    }
}
inline bool der_clear_times(unsigned long long* counters, unsigned long long* cooc, unsigned long long* ref_time,
                            unsigned long long* hyp_time, long n, hipStream_t stream) {
    hipLaunchKernelGGL(der_clear_times_kernel, dim3((unsigned)n), dim3(NT), 0, stream, counters, cooc, ref_time, hyp_time, n);
    return hipGetLastError() == hipSuccess;
}

// The marginal times of a workgroup: the lanes i < 16 of its waves hold their sums for speaker i; added up in LDS (tsum [CMAX],
// 0 and a barrier before), then, after a barrier, one integer atomic per speaker by flush_times.
DEV void gather_times(unsigned long long* tsum, unsigned long long mine) {
    if ((threadIdx.x & 63) < CMAX && mine) atomicAdd(tsum + (threadIdx.x & 63), mine);
}
DEV void flush_times(unsigned long long* out, const unsigned long long* tsum) {
    if (threadIdx.x < CMAX && tsum[threadIdx.x]) atomicAdd(out + threadIdx.x, tsum[threadIdx.x]);
}

// the table of the entries with regions: both pointers or neither, pairs loaded as int2
inline bool der_regions_ok(const int* uem, const int* uoff) {
    return (uem == nullptr) == (uoff == nullptr) && ((uintptr_t)uem & 7) == 0;
}

}  // namespace der
