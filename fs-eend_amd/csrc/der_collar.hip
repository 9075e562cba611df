// Collar DER with the optimal speaker mapping (LS-EEND/metrics.py:41-108: pyannote's DiarizationErrorRate(collar=50) over the
// label runs and the thresholded, median-filtered predictions).  The contract is stated in include/eend_hip.h at
// eend_collar_der_u64; all of it is integer work on 0 / 1 activity that is already on the device.
//
// der_collar_pass_kernel, grid (tile groups, recordings), 256 threads: a workgroup walks tiles of DER_TILE reference frames of
// one recording (tile g, g + groups, ...).  Per tile
//   1. the uint8 rows of the reference, with h frames of halo on each side, and of the hypothesis frames under the tile go
//      through an LDS staging buffer in aligned 4-byte words (bytes only at the two ragged ends) and become one 16-bit speaker
//      mask per frame;
//   2. boundary bits (mask[f - 1] != mask[f], zeros outside the recording) are packed by wave ballots into 64-bit words, and a
//      prefix population count over the words answers "any boundary within (t - h, t + h]" for every h in two lookups;
//   3. kept frames add to total / miss / false alarm / sum of min(nr, nh) in registers;
//   4. a ballot per speaker turns 64 frames into bit planes R_i & keep and H_j, and thread (i, j) adds popcount(R_i & H_j) to
//      its co-occurrence count: 256 population counts per 64 frames.
// All partial sums stay in registers over the workgroup's tiles; one 64-bit integer atomic per counter follows at the end, so
// the results are the same on every run (der_collar_clear_kernel zeroes the sums first).  der_collar_assign_kernel, one wave
// per recording: the shortest-augmenting-path assignment of pit.hip in 64-bit integers, on the negated counts padded to a
// square and staged in LDS, then confusion, correct, the frames removed and the mapping.  Summed over frames, correct is the
// value of the optimal assignment, so no second pass over the frames is needed.
#include "common.h"
#include "kernels.h"
#include "der_tile.h"

namespace {

using namespace der;                              // the tile layout and load_masks, shared with der_sweep.hip

// counters and co-occurrence counts start at 0.  A kernel, not hipMemsetAsync: memset nodes of a captured graph came back with
// other values than 0 on replay (seen once with this entry in torch.cuda.graph; a launch replays as it was recorded).
__global__ __launch_bounds__(NT)
void der_collar_clear_kernel(unsigned long long* __restrict__ counters, unsigned long long* __restrict__ cooc, int B) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i < (size_t)B * 8) counters[i] = 0;
    if (i < (size_t)B * CMAX * CMAX) cooc[i] = 0;
}

__global__ __launch_bounds__(NT)
void der_collar_pass_kernel(const unsigned char* __restrict__ ref, const int* __restrict__ roff, int Cr,
                            const unsigned char* __restrict__ hyp, const int* __restrict__ hoff, int Ch, int sub, int h, int skip,
                            unsigned long long* __restrict__ counters, unsigned long long* __restrict__ cooc) {
    __shared__ unsigned short rmask[EXT], hmask[TILE];
    __shared__ unsigned stage[STAGE_WORDS];
    __shared__ unsigned long long bits[NWORDS], planes[NGRP][2 * CMAX], sums[5];
    __shared__ unsigned before[NWORDS];
    const int rec = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long r0 = roff[rec], h0 = hoff[rec];
    const long Trl = (long)roff[rec + 1] - r0, Thl = (long)hoff[rec + 1] - h0;
    const long Tl = Trl > Thl * sub ? Trl : Thl * sub;
    if (Trl < 0 || Thl < 0 || Tl > DER_MAX_FRAMES) return;         // refused: the assignment kernel marks the recording
    const int Tr = (int)Trl, Th = (int)Thl, T = (int)Tl;
    const int ntiles = (int)(((long)T + TILE - 1) / TILE);
    const int ci = tid >> 4, cj = tid & 15;
    unsigned long long total = 0, miss = 0, fa = 0, both = 0, kept = 0, pair = 0;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int t0 = tile * TILE;                               // < T <= DER_MAX_FRAMES, so t0 + TILE + 2 h stays an int
        const int tl = T - t0 < TILE ? T - t0 : TILE;
        const int n = tl + 2 * h;                                 // reference frames t0 - h .. t0 + tl + h - 1
        const int k0 = t0 / sub, nk = (t0 + tl - 1) / sub - k0 + 1;
        load_masks(ref, r0, Tr, Cr, t0 - h, n, rmask, stage);
        load_masks(hyp, h0, Th, Ch, k0, nk, hmask, stage);
        // bit e of `bits`: a boundary at b = t0 - h + 1 + e, e in [0, n - 1); the words up to that of position n - 1 are written
        for (int e0 = 0; e0 <= n - 1; e0 += NT) {
            const int e = e0 + tid;
            const unsigned long long w = __ballot(e < n - 1 && rmask[e] != rmask[e + 1]);
            if (lane == 0 && e <= n - 1) bits[e >> 6] = w;
        }
        __syncthreads();
        const int nw = ((n - 1) >> 6) + 1;
        if (tid < nw) {
            unsigned c = 0;
            for (int k = 0; k < tid; ++k) c += __popcll(bits[k]);
            before[tid] = c;
        }
        __syncthreads();
        for (int j0 = 0; j0 < tl; j0 += NT) {
            const int j = j0 + tid, t = t0 + j;
            const bool valid = j < tl;
            unsigned r = 0, m = 0;
            bool keep = valid;
            if (valid) {
                r = rmask[h + j];
                m = hmask[t / sub - k0];
                if (h > 0) {                                      // boundaries b in [t - h + 1, t + h]: bits [j, j + 2 h)
                    const int lo = j, hi = j + 2 * h;
                    const unsigned clo = before[lo >> 6] + __popcll(bits[lo >> 6] & ((1ull << (lo & 63)) - 1));
                    const unsigned chi = before[hi >> 6] + __popcll(bits[hi >> 6] & ((1ull << (hi & 63)) - 1));
                    keep = chi == clo;
                }
                const int nr = __popc(r), nh = __popc(m);
                if (skip && nr >= 2) keep = false;
                if (keep) {
                    total += nr;
                    miss += nr > nh ? nr - nh : 0;
                    fa += nh > nr ? nh - nr : 0;
                    both += nr < nh ? nr : nh;
                    kept += 1;
                }
            }
            const int g = (j0 >> 6) + wave;
            for (int s = 0; s < CMAX; ++s) {
                const unsigned long long pr = __ballot(keep && (r >> s & 1u)), ph = __ballot(valid && (m >> s & 1u));
                if (lane == s) {
                    planes[g][s] = pr;
                    planes[g][CMAX + s] = ph;
                }
            }
        }
        __syncthreads();
        const int ng = ((tl + NT - 1) / NT) * (NT / 64);
        if (ci < Cr && cj < Ch)
            for (int g = 0; g < ng; ++g) pair += __popcll(planes[g][ci] & planes[g][CMAX + cj]);
        // the next tile's first write to `planes`, `bits` or `before` comes after the barriers of load_masks
    }

    if (tid < 5) sums[tid] = 0;
    __syncthreads();
    if (total) atomicAdd(&sums[0], total);
    if (miss) atomicAdd(&sums[1], miss);
    if (fa) atomicAdd(&sums[2], fa);
    if (kept) atomicAdd(&sums[3], kept);
    if (both) atomicAdd(&sums[4], both);
    __syncthreads();
    unsigned long long* out = counters + (size_t)rec * 8;
    const int slot = tid < 3 ? tid : (tid == 3 ? 5 : 7);          // total, miss, false alarm, frames kept, sum of min(nr, nh)
    if (tid < 5 && sums[tid]) atomicAdd(out + slot, sums[tid]);
    if (pair) atomicAdd(cooc + ((size_t)rec * CMAX + ci) * CMAX + cj, pair);
}

// One wave per matrix m = g * B + b (the sweep of der_sweep.hip scores G points per recording b; here G = 1): the lengths are
// those of recording b, the sums and the mapping those of m.  `medians` (the sweep's, nmed of them, point g uses g % nmed; may be
// null): a point whose median is out of the sweep's range is marked like an out-of-scope recording.  `totals` (may be null):
// u64 [G][8] running sums that every scored matrix's eight counters are added to.
// rows = reference speakers, columns = hypothesis speakers, a[i][j] = -cooc[i][j]; the rows and columns
// beyond Cr and Ch are 0 (cleared, never added to), which pads the matrix to a square of n = max(Cr, Ch).  The minimum-cost
// perfect matching of the square, restricted to pairs with cooc > 0, is the mapping.  The wave stages the matrix in LDS with
// coalesced loads, then lane 0 runs the solver on LDS arrays: the serial chain of its steps then waits for LDS, not for HBM
// (read from global memory step by step it took 130-270 us, most of a call).
__global__ __launch_bounds__(64)
void der_collar_assign_kernel(const int* __restrict__ roff, const int* __restrict__ hoff, int Cr, int Ch, int sub, int B,
                              const int* __restrict__ medians, int nmed, unsigned long long* __restrict__ counters,
                              const unsigned long long* __restrict__ cooc, int* __restrict__ mapping,
                              unsigned long long* __restrict__ totals) {
    __shared__ long long a[CMAX * CMAX], u[CMAX + 1], v[CMAX + 1], minv[CMAX + 1];
    __shared__ int p[CMAX + 1], way[CMAX + 1];
    __shared__ bool used[CMAX + 1];
    const int m = blockIdx.x, b = m % B, g = m / B, lane = threadIdx.x;
    unsigned long long* cnt = counters + (size_t)m * 8;
    int* map = mapping + (size_t)m * CMAX;
    const unsigned long long* c = cooc + (size_t)m * CMAX * CMAX;
    const long Trl = (long)roff[b + 1] - roff[b], Thl = (long)hoff[b + 1] - hoff[b];
    const long Tl = Trl > Thl * sub ? Trl : Thl * sub;
    if (lane < CMAX) map[lane] = -1;
    const bool point_ok = !medians || median_ok(medians[g % nmed]);
    if (Trl < 0 || Thl < 0 || Tl > DER_MAX_FRAMES || !point_ok) {  // out of scope: every counter reads ~0
        if (lane < 8) cnt[lane] = ~0ull;
        return;
    }
    for (int k = lane; k < CMAX * CMAX; k += 64) a[k] = -(long long)c[k];
    __syncthreads();
    if (lane != 0) return;
    const int n = Cr > Ch ? Cr : Ch;
    const long long INF = 0x3fffffffffffffffLL;
    for (int k = 0; k <= n; ++k) { u[k] = 0; v[k] = 0; p[k] = 0; way[k] = 0; }
    for (int i = 1; i <= n; ++i) {
        p[0] = i;
        int j0 = 0;
        for (int k = 0; k <= n; ++k) { minv[k] = INF; used[k] = false; }
        do {
            used[j0] = true;
            const int i0 = p[j0];
            const long long ui = u[i0];
            long long delta = INF;
            int j1 = 0;
            for (int j = 1; j <= n; ++j)
                if (!used[j]) {
                    const long long cur = a[(i0 - 1) * CMAX + (j - 1)] - ui - v[j];
                    if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
                    if (minv[j] < delta) { delta = minv[j]; j1 = j; }
                }
            for (int j = 0; j <= n; ++j)
                if (used[j]) { u[p[j]] += delta; v[j] -= delta; }
                else minv[j] -= delta;
            j0 = j1;
        } while (p[j0] != 0);
        do {
            const int j1 = way[j0];
            p[j0] = p[j1];
            j0 = j1;
        } while (j0);
    }
    unsigned long long best = 0;
    for (int j = 1; j <= Ch; ++j) {
        const int i = p[j];
        if (i >= 1 && i <= Cr && a[(i - 1) * CMAX + (j - 1)] < 0) {
            map[j - 1] = i - 1;
            best += (unsigned long long)-a[(i - 1) * CMAX + (j - 1)];
        }
    }
    cnt[3] = cnt[7] - best;                                        // confusion = sum of min(nr, nh) - correct
    cnt[4] = best;
    cnt[6] = (unsigned long long)Tl - cnt[5];
    if (totals)
        for (int k = 0; k < 8; ++k)
            if (cnt[k]) atomicAdd(totals + (size_t)g * 8 + k, cnt[k]);
}

}  // namespace

int eend_launch_collar_der(const unsigned char* ref, const int* roff, int Cr, const unsigned char* hyp, const int* hoff, int Ch, int B,
                           int sub, int h, int skip, unsigned long long* counters, unsigned long long* cooc, int* mapping,
                           hipStream_t stream) {
    if (!ref || !roff || !hyp || !hoff || !counters || !cooc || !mapping) return EEND_EINVAL;
    if (Cr < 1 || Cr > CMAX || Ch < 1 || Ch > CMAX || B < 1 || B > 65535 || sub < 1 || h < 0 || h > HMAX) return EEND_EINVAL;
    hipLaunchKernelGGL(der_collar_clear_kernel, dim3(B), dim3(NT), 0, stream, counters, cooc, B);   // B x NT = B x 16 x 16 counts
    if (hipGetLastError() != hipSuccess) return EEND_ELAUNCH;
    // the lengths live on the device, so the tile groups are sized by the batch alone: about 4096 workgroups, at most
    // DER_MAX_GROUPS per recording; a group beyond a recording's last tile ends at once
    int groups = 4096 / B;
    groups = groups < 1 ? 1 : (groups > DER_MAX_GROUPS ? DER_MAX_GROUPS : groups);
    hipLaunchKernelGGL(der_collar_pass_kernel, dim3(groups, B), dim3(NT), 0, stream, ref, roff, Cr, hyp, hoff, Ch, sub, h,
                       skip ? 1 : 0, counters, cooc);
    if (hipGetLastError() != hipSuccess) return EEND_ELAUNCH;
    return eend_launch_collar_der_assign(roff, hoff, Cr, Ch, B, 1, sub, nullptr, 0, counters, cooc, mapping, nullptr, stream);
}

int eend_launch_collar_der_assign(const int* roff, const int* hoff, int Cr, int Ch, int B, int G, int sub, const int* medians, int nmed,
                                  unsigned long long* counters, const unsigned long long* cooc, int* mapping,
                                  unsigned long long* totals, hipStream_t stream) {
    hipLaunchKernelGGL(der_collar_assign_kernel, dim3((unsigned)G * B), dim3(64), 0, stream, roff, hoff, Cr, Ch, sub, B, medians, nmed,
                       counters, cooc, mapping, totals);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
