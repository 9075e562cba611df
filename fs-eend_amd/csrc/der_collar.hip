// Collar DER with the optimal speaker mapping (LS-EEND/metrics.py:41-108: pyannote's DiarizationErrorRate(collar=50) over the
// label runs and the thresholded, median-filtered predictions).  The contract is stated in include/eend_hip.h at
// eend_collar_der_u64; all of it is integer work on 0 / 1 activity that is already on the device.
//
// der_collar_pass_kernel, grid (tile groups, recordings), 256 threads: a workgroup walks tiles of DER_TILE reference frames of
// one recording (tile g, g + groups, ...).  It is the one-point case of der_sweep_pass_kernel, made of the parts of der_tile.h.
// Per tile
//   1. load_masks: the uint8 rows of the reference, with h frames of halo on each side, and of the hypothesis frames under the
//      tile go through an LDS staging buffer in aligned 4-byte words (bytes only at the two ragged ends) and become one 16-bit
//      speaker mask per frame;
//   2. ref_side: boundary bits (mask[f - 1] != mask[f], zeros outside the recording) are packed by wave ballots into 64-bit
//      words, and a prefix population count over the words answers "any boundary within (t - h, t + h]" for every h in two
//      lookups; kept frames add to total and frames kept; a ballot per speaker makes the bit planes R_i & keep of 64 frames;
//   3. score_point: the planes H_j, the sums of nh and of min(nr, nh) over the kept frames by ballots, and thread (i, j) adds
//      popcount(R_i & keep & H_j) to its co-occurrence count: 256 population counts per 64 frames.
// All partial sums stay in registers or LDS over the workgroup's tiles; one 64-bit integer atomic per counter follows at the end
// (add_counter: miss = total - sum of min, false alarm = sum of nh - sum of min), so the results are the same on every run
// (der_clear_kernel zeroes the sums first).  der_collar_assign_kernel, one wave per recording: the shortest-augmenting-path
// assignment of assign.h, which pit.hip runs in fp64, in 64-bit integers on the negated counts padded to a square and staged in
// LDS, then confusion, correct, the frames removed and the mapping.  Summed over frames, correct is the value of the optimal
// assignment, so no second pass over the frames is needed.
// With scoring regions (eend_collar_der_regions_u64) the pass is another instance of the same template: the region term of
// der_tile.h joins keep, and the marginal times of both sides are counted next to the co-occurrence counts.  From those,
// jer_assign_kernel (eend_jer_assign_f64) pairs the speakers for the Jaccard error rate, in float64.
#include "common.h"
#include "kernels.h"
#include "assign.h"
#include "der_tile.h"

namespace {

using namespace der;

// <REG, MARG>: <false, false> is the kernel of eend_collar_der_u64, with that entry's argument list (the pack is empty) and,
// compared instruction by instruction, the code it had before there were regions.  eend_collar_der_regions_u64 runs
// <false, true> without a table and <true, true> with one; both take one RegionArgs more (der_tile.h).
template <bool REG, bool MARG, typename... Extra>
__global__ __launch_bounds__(NT)
void der_collar_pass_kernel(const unsigned char* __restrict__ ref, const int* __restrict__ roff, int Cr,
                            const unsigned char* __restrict__ hyp, const int* __restrict__ hoff, int Ch, int sub, int h, int skip,
                            unsigned long long* __restrict__ counters, unsigned long long* __restrict__ cooc, Extra... extra) {
    const int *uem = nullptr, *uoff = nullptr;
    unsigned long long *ref_time = nullptr, *hyp_time = nullptr;
    if constexpr (MARG) {
        const RegionArgs& x = region_args(extra...);
        uem = x.uem, uoff = x.uoff, ref_time = x.ref_time, hyp_time = x.hyp_time;
    }
    __shared__ unsigned short rmask[EXT], hmask[TILE];
    __shared__ unsigned stage[STAGE_WORDS];
    __shared__ RefLds L;
    __shared__ unsigned long long PH[NGRP * CMAX], wsum[NT / 64][2], sums[2];
    __shared__ unsigned long long regw[REG ? NGRP : 1], tsum[MARG ? 2 : 1][CMAX];
    const int rec = blockIdx.y, tid = threadIdx.x;
    const Rec R = rec_header(roff, hoff, rec, sub);
    if (!R.ok) return;                                            // refused: the assignment kernel marks the recording
    if (tid < 2 * (NT / 64)) (&wsum[0][0])[tid] = 0;              // read after the barriers of load_masks or of the end
    unsigned long long total = 0, kept = 0, pair = 0, rtime = 0, htime = 0;
    Regions rg;
    if constexpr (REG) rg = rec_regions(uem, uoff, rec);

    for (int tile = blockIdx.x; tile < R.ntiles; tile += gridDim.x) {
        const Tile t = tile_extents(tile, R.T, sub, h);
        if constexpr (REG) region_clear(regw);                   // the last tile's reads: before score_point's barrier
        load_masks(ref, R.r0, R.Tr, Cr, t.t0 - h, t.n, rmask, stage);
        if constexpr (REG) region_fill(rg, t.t0, t.tl, regw);    // between the barriers of the two load_masks
        load_masks(hyp, R.h0, R.Th, Ch, t.k0, t.nk, hmask, stage);   // its barriers: the last tile's reads of L.planes and PH
        RefRegs rf;
        ref_side<REG, MARG>(t, rmask, Cr, sub, h, skip, L, rf, total, kept, regw, &rtime);
        pair += score_point<MARG>(t, L, rf, hmask, Cr, Ch, PH, wsum, &htime);
    }

    if (tid < 2) sums[tid] = 0;
    if constexpr (MARG)
        if (tid < 2 * CMAX) (&tsum[0][0])[tid] = 0;
    __syncthreads();
    if (total) atomicAdd(&sums[0], total);
    if (kept) atomicAdd(&sums[1], kept);
    if constexpr (MARG) {
        gather_times(tsum[0], rtime);
        gather_times(tsum[1], htime);
    }
    __syncthreads();
    if (tid < 5) add_counter(counters + (size_t)rec * 8, tid, sums[0], sums[1], wsum);
    if (pair) atomicAdd(cooc + ((size_t)rec * CMAX + (tid >> 4)) * CMAX + (tid & 15), pair);
    if constexpr (MARG) {
        flush_times(ref_time + (size_t)rec * CMAX, tsum[0]);
        flush_times(hyp_time + (size_t)rec * CMAX, tsum[1]);
    }
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
    const Rec R = rec_header(roff, hoff, b, sub);
    if (lane < CMAX) map[lane] = -1;
    const bool point_ok = !medians || median_ok(medians[g % nmed]);
    if (!R.ok || !point_ok) {                                      // out of scope: every counter reads ~0
        if (lane < 8) cnt[lane] = ~0ull;
        return;
    }
    for (int k = lane; k < CMAX * CMAX; k += 64) a[k] = -(long long)c[k];
    __syncthreads();
    if (lane != 0) return;
    assign_rows<long long>(a, CMAX, Cr > Ch ? Cr : Ch, 0x3fffffffffffffffLL, u, v, minv, p, way, used);
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
    cnt[6] = (unsigned long long)R.Tl - cnt[5];
    if (totals)
        for (int k = 0; k < 8; ++k)
            if (cnt[k]) atomicAdd(totals + (size_t)g * 8 + k, cnt[k]);
}

// Jaccard error rate: one wave per matrix m of `n`.  Reference speaker i exists iff ref_time[i] > 0, hypothesis speaker j iff
// hyp_time[j] > 0; cost[i][j] = 1 - inter / union in float64 for a pair of both (inter = cooc[i][j], union = ref_time[i] +
// hyp_time[j] - inter), 1 for an existing reference speaker against anything else (left alone its error is 1, and no pair costs
// more, so the padded square has the optimum of the rectangle) and 0 in the rows of speakers that do not exist.  As
// der_collar_assign_kernel: staged in LDS, solved by lane 0 with assign_rows, here in float64, the form pit.hip runs.  Out:
// pairing i32 [n][16], reference -> hypothesis, -1 where the speaker is not paired, does not exist, or its pair has inter = 0
// (the cost of such a pair is the unpaired 1); speakers u64 [n][16][3] = ref_time, the paired hyp_time or 0, inter.
__global__ __launch_bounds__(64)
void jer_assign_kernel(const unsigned long long* __restrict__ cooc, const unsigned long long* __restrict__ ref_time,
                       const unsigned long long* __restrict__ hyp_time, int Cr, int Ch, int* __restrict__ pairing,
                       unsigned long long* __restrict__ speakers) {
    __shared__ double a[CMAX * CMAX], u[CMAX + 1], v[CMAX + 1], minv[CMAX + 1];
    __shared__ unsigned long long rt[CMAX], ht[CMAX];
    __shared__ int p[CMAX + 1], way[CMAX + 1];
    __shared__ bool used[CMAX + 1];
    const int m = blockIdx.x, lane = threadIdx.x;
    const unsigned long long* c = cooc + (size_t)m * CMAX * CMAX;
    int* pr = pairing + (size_t)m * CMAX;
    unsigned long long* sp = speakers + (size_t)m * CMAX * 3;
    if (lane < CMAX) {
        rt[lane] = lane < Cr ? ref_time[(size_t)m * CMAX + lane] : 0;
        ht[lane] = lane < Ch ? hyp_time[(size_t)m * CMAX + lane] : 0;
        pr[lane] = -1;
    }
    __syncthreads();
    for (int k = lane; k < CMAX * CMAX; k += 64) {
        const int i = k >> 4, j = k & 15;
        double cost = rt[i] ? 1.0 : 0.0;
        if (rt[i] && ht[j]) {
            const unsigned long long inter = c[k];
            cost = 1.0 - (double)inter / (double)(rt[i] + ht[j] - inter);
        }
        a[k] = cost;
    }
    __syncthreads();
    if (lane != 0) return;
    const int n = Cr > Ch ? Cr : Ch;
    assign_rows<double>(a, CMAX, n, 1e300, u, v, minv, p, way, used);
    for (int i = 0; i < CMAX; ++i) sp[i * 3] = rt[i], sp[i * 3 + 1] = 0, sp[i * 3 + 2] = 0;
    for (int j = 1; j <= n; ++j) {
        const int i = p[j] - 1;
        if (i < 0 || i >= Cr || j > Ch || !rt[i] || !ht[j - 1] || !c[i * CMAX + (j - 1)]) continue;
        pr[i] = j - 1;
        sp[i * 3 + 1] = ht[j - 1];
        sp[i * 3 + 2] = c[i * CMAX + (j - 1)];
    }
}

}  // namespace

int eend_launch_collar_der(const unsigned char* ref, const int* roff, int Cr, const unsigned char* hyp, const int* hoff, int Ch, int B,
                           int sub, int h, int skip, unsigned long long* counters, unsigned long long* cooc, int* mapping,
                           hipStream_t stream) {
    if (!ref || !roff || !hyp || !hoff || !counters || !cooc || !mapping) return EEND_EINVAL;
    if (!der_args_ok(Cr, Ch, B, sub, h)) return EEND_EINVAL;
    if (!der_clear(counters, cooc, B, stream)) return EEND_ELAUNCH;
    hipLaunchKernelGGL((der_collar_pass_kernel<false, false>), dim3(der_tile_groups(B), B), dim3(NT), 0, stream, ref, roff, Cr, hyp,
                       hoff, Ch, sub, h, skip ? 1 : 0, counters, cooc);
    if (hipGetLastError() != hipSuccess) return EEND_ELAUNCH;
    return eend_launch_collar_der_assign(roff, hoff, Cr, Ch, B, 1, sub, nullptr, 0, counters, cooc, mapping, nullptr, stream);
}

int eend_launch_collar_der_regions(const unsigned char* ref, const int* roff, int Cr, const unsigned char* hyp, const int* hoff, int Ch,
                                   int B, int sub, int h, int skip, const int* uem, const int* uoff, unsigned long long* counters,
                                   unsigned long long* cooc, int* mapping, unsigned long long* ref_time, unsigned long long* hyp_time,
                                   hipStream_t stream) {
    if (!ref || !roff || !hyp || !hoff || !counters || !cooc || !mapping || !ref_time || !hyp_time) return EEND_EINVAL;
    if (!der_args_ok(Cr, Ch, B, sub, h) || !der_regions_ok(uem, uoff)) return EEND_EINVAL;
    if (!der_clear_times(counters, cooc, ref_time, hyp_time, B, stream)) return EEND_ELAUNCH;
    const dim3 grid(der_tile_groups(B), B);
    const RegionArgs x{uem, uoff, ref_time, hyp_time};
    if (uem)
        hipLaunchKernelGGL((der_collar_pass_kernel<true, true, RegionArgs>), grid, dim3(NT), 0, stream, ref, roff, Cr, hyp, hoff, Ch,
                           sub, h, skip ? 1 : 0, counters, cooc, x);
    else
        hipLaunchKernelGGL((der_collar_pass_kernel<false, true, RegionArgs>), grid, dim3(NT), 0, stream, ref, roff, Cr, hyp, hoff, Ch,
                           sub, h, skip ? 1 : 0, counters, cooc, x);
    if (hipGetLastError() != hipSuccess) return EEND_ELAUNCH;
    return eend_launch_collar_der_assign(roff, hoff, Cr, Ch, B, 1, sub, nullptr, 0, counters, cooc, mapping, nullptr, stream);
}

int eend_launch_jer_assign(const unsigned long long* cooc, const unsigned long long* ref_time, const unsigned long long* hyp_time, int Cr,
                           int Ch, long n, int* pairing, unsigned long long* speakers, hipStream_t stream) {
    if (!cooc || !ref_time || !hyp_time || !pairing || !speakers) return EEND_EINVAL;
    if (Cr < 1 || Cr > CMAX || Ch < 1 || Ch > CMAX || n < 1 || n > 0x7fffffffL) return EEND_EINVAL;
    hipLaunchKernelGGL(jer_assign_kernel, dim3((unsigned)n), dim3(64), 0, stream, cooc, ref_time, hyp_time, Cr, Ch, pairing, speakers);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_collar_der_assign(const int* roff, const int* hoff, int Cr, int Ch, int B, int G, int sub, const int* medians, int nmed,
                                  unsigned long long* counters, const unsigned long long* cooc, int* mapping,
                                  unsigned long long* totals, hipStream_t stream) {
    hipLaunchKernelGGL(der_collar_assign_kernel, dim3((unsigned)G * B), dim3(64), 0, stream, roff, hoff, Cr, Ch, sub, B, medians, nmed,
                       counters, cooc, mapping, totals);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
