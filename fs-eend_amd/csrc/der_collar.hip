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
#include "common.h"
#include "kernels.h"
#include "assign.h"
#include "der_tile.h"

namespace {

using namespace der;

__global__ __launch_bounds__(NT)
void der_collar_pass_kernel(const unsigned char* __restrict__ ref, const int* __restrict__ roff, int Cr,
                            const unsigned char* __restrict__ hyp, const int* __restrict__ hoff, int Ch, int sub, int h, int skip,
                            unsigned long long* __restrict__ counters, unsigned long long* __restrict__ cooc) {
    __shared__ unsigned short rmask[EXT], hmask[TILE];
    __shared__ unsigned stage[STAGE_WORDS];
    __shared__ RefLds L;
    __shared__ unsigned long long PH[NGRP * CMAX], wsum[NT / 64][2], sums[2];
    const int rec = blockIdx.y, tid = threadIdx.x;
    const Rec R = rec_header(roff, hoff, rec, sub);
    if (!R.ok) return;                                            // refused: the assignment kernel marks the recording
    if (tid < 2 * (NT / 64)) (&wsum[0][0])[tid] = 0;              // read after the barriers of load_masks or of the end
    unsigned long long total = 0, kept = 0, pair = 0;

    for (int tile = blockIdx.x; tile < R.ntiles; tile += gridDim.x) {
        const Tile t = tile_extents(tile, R.T, sub, h);
        load_masks(ref, R.r0, R.Tr, Cr, t.t0 - h, t.n, rmask, stage);
        load_masks(hyp, R.h0, R.Th, Ch, t.k0, t.nk, hmask, stage);   // its barriers: the last tile's reads of L.planes and PH
        RefRegs rf;
        ref_side(t, rmask, Cr, sub, h, skip, L, rf, total, kept);
        pair += score_point(t, L, rf, hmask, Cr, Ch, PH, wsum);
    }

    if (tid < 2) sums[tid] = 0;
    __syncthreads();
    if (total) atomicAdd(&sums[0], total);
    if (kept) atomicAdd(&sums[1], kept);
    __syncthreads();
    if (tid < 5) add_counter(counters + (size_t)rec * 8, tid, sums[0], sums[1], wsum);
    if (pair) atomicAdd(cooc + ((size_t)rec * CMAX + (tid >> 4)) * CMAX + (tid & 15), pair);
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

}  // namespace

int eend_launch_collar_der(const unsigned char* ref, const int* roff, int Cr, const unsigned char* hyp, const int* hoff, int Ch, int B,
                           int sub, int h, int skip, unsigned long long* counters, unsigned long long* cooc, int* mapping,
                           hipStream_t stream) {
    if (!ref || !roff || !hyp || !hoff || !counters || !cooc || !mapping) return EEND_EINVAL;
    if (!der_args_ok(Cr, Ch, B, sub, h)) return EEND_EINVAL;
    if (!der_clear(counters, cooc, B, stream)) return EEND_ELAUNCH;
    hipLaunchKernelGGL(der_collar_pass_kernel, dim3(der_tile_groups(B), B), dim3(NT), 0, stream, ref, roff, Cr, hyp, hoff, Ch,
                       sub, h, skip ? 1 : 0, counters, cooc);
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
