// Collar DER over a grid of G = n_thresholds x n_medians operating points in one pass over the rows: what the reference's
// scoring scripts tune on a development set (LS-EEND/metrics.py and sad_post_process.py take --thredshold and --median).  The
// contract is stated in include/eend_hip.h at eend_collar_der_sweep_u64; point g = i_theta * n_medians + i_median gives exactly
// eend_collar_der_u64 over eend_sad_fuse_f32 (with flags) + eend_activity_median_u8 of the posteriors at that point.
//
// der_sweep_pass_kernel, grid (tile groups, recordings), 256 threads, is der_collar_pass_kernel at G points: a workgroup walks
// tiles of DER_TILE reference frames of one recording.  From der_tile.h it takes load_masks, the launcher's parts and the scalar
// rules of decision.h.  Its recording header, tile extents and steps 1 and 4 below are rec_header, tile_extents, ref_side and
// score_point of der_tile.h in this kernel's own text, so a change to one of them is made in both places: written with the
// functions the kernel compiled to other code (147 or 165 VGPRs for 164; with the header and extents alone the same
// instructions but one) that measured 0.1 to 1.8 % slower on the 5 x 2 and 16 x 2 grids.  Per tile
//   1. once, the reference side: speaker masks with the collar halo, boundary bits and their prefix
//      population count, keep; total and frames kept; the bit planes R_i & keep; per thread, keep and nr of its 4 frames and the
//      hypothesis frame under each (one byte and one index per frame, in registers);
//   2. once, the float32 posterior rows of the hypothesis frames under the tile plus max(median) / 2 frames on each side (zeros
//      beyond the recording's own first and last frame, so a neighbour's rows are never seen), 256 rows per round through LDS:
//      16-byte loads where a vector lies inside the round's bytes, 4-byte loads at the two ragged ends (a row start is only
//      4-byte aligned).  One thread per row compares every value with every threshold (unrolled over the 16 thresholds, so the
//      decisions stay in registers), finds the row's winner once, applies the flag, and leaves one 16-bit decision mask per
//      threshold and frame in LDS: from here on the floats are not needed;
//   3. per threshold, a ballot per speaker turns the masks into bit planes over the staged frames, and a prefix population count
//      over their 64-bit words follows;
//   4. per median k of that threshold, the filtered mask of a hypothesis frame is 16 window counts, each the difference of two
//      prefix counts (k = 1 copies the decision); then per reference frame nh, min(nr, nh) and a ballot per speaker
//      into the planes H_j, and thread (i, j) adds popcount(R_i & keep & H_j) over the tile's 64-frame groups.
// The sums of nh over kept frames fall out of the ballots (popcount(H_j & keep)), the sums of min(nr, nh) are taken by ballots
// over its 7 bits, both per wave in scalar registers; miss = total - sum of min, false alarm = sum of nh - sum of min.  The 32
// co-occurrence accumulators of a thread are named registers: the point loop is not unrolled, the add selects the register by
// an unrolled compare, so nothing is indexed dynamically and nothing spills.  All sums are 64-bit; one integer atomic per sum
// and workgroup at the end, after der_clear_kernel, so every run gives the same bits.  The assignment is
// der_collar_assign_kernel on G * B matrices, which also marks the points with a median out of range and adds to the totals.
//
// LDS per workgroup: 21 488 bytes static (16 416 of them one block that holds, in turn, the reference masks, the float rows
// and the planes of steps 3 and 4) + 2 * n_thresholds * staged frames for the decision masks, staged frames = min(1024,
// 1023 / subsampling + 2) + 126: 2.3 KB for 5 thresholds at subsampling 10, 36.8 KB at the limits (16 thresholds, subsampling
// 1), so at most 58.3 KB and never beyond the 64 KB a launch gets without asking.  164 VGPRs (64 of them the accumulators), no
// scratch, 113 SGPRs kept in VGPR lanes: 3 waves per SIMD, which is 3 workgroups per CU; LDS alone would admit 6 at the
// 5 x 2 grid.  Like der_collar_pass_kernel the pass is far from the HBM rate: its time grows with the points at a fixed number
// of bytes read (DESIGN.md section 8 has the measurement).
#include "common.h"
#include "kernels.h"
#include "der_tile.h"

namespace {

using namespace der;

constexpr int NTH = DER_SWEEP_NTHETA, NMED = DER_SWEEP_NMED, GMAX = DER_SWEEP_GMAX;
constexpr int HKMAX = DER_SWEEP_KMAX / 2;                       // largest median halo, hypothesis frames
constexpr int FSTAGE = NT * CMAX + 8;                           // floats: NT rows of CMAX, entered at any float of the first 16 bytes
constexpr int PW = (TILE + 2 * HKMAX + NT - 1) / NT * (NT / 64) + 1;   // plane words per speaker, and one prefix count beyond
constexpr int P_BYTES = CMAX * PW * 8, PH_BYTES = NGRP * CMAX * 8, CUM_BYTES = CMAX * PW * 2, HM_BYTES = TILE * 2;
constexpr int REF_BYTES = EXT * 2 + STAGE_WORDS * 4, POINT_BYTES = P_BYTES + PH_BYTES + CUM_BYTES + HM_BYTES;
constexpr int SCRATCH = FSTAGE * 4;
static_assert(SCRATCH >= REF_BYTES && SCRATCH >= POINT_BYTES && SCRATCH % 16 == 0 && (EXT * 2) % 4 == 0, "der_sweep scratch block");
static_assert(GMAX == NTH * 2 && NT / 64 == 4, "der_sweep layout");

// <REG, MARG>, as for der_collar_pass_kernel: <false, false> is the kernel of eend_collar_der_sweep_u64, with that entry's
// argument list and its code of before; eend_collar_der_sweep_regions_u64 runs <false, true> without a table and <true, true>
// with one, both with one RegionArgs more.  The region term comes from
// der_tile.h (region_clear, region_fill, region_bit), the same calls at the same place of step 1 as in ref_side.  The marginal
// times: the reference's in a register per thread (one for all points), the hypothesis's, one per point, in LDS (hsum, 2 KB:
// lane j of every wave adds popcount(H_j & keep) with an LDS atomic; a workgroup's sum is below 2^31 frames, so 32 bits do),
// which keeps the LDS at the limits below 64 KB and adds no accumulator registers to the 64 of the co-occurrence counts.
template <bool REG, bool MARG, typename... Extra>
__global__ __launch_bounds__(NT)
void der_sweep_pass_kernel(const unsigned char* __restrict__ ref, const int* __restrict__ roff, int Cr,
                           const float* __restrict__ pred, const int* __restrict__ poff, int Ch,
                           const unsigned char* __restrict__ sad, const float* __restrict__ thresholds, int nth,
                           const int* __restrict__ medians, int nmed, int sub, int h, int skip, int hcap, int B,
                           unsigned long long* __restrict__ counters, unsigned long long* __restrict__ cooc, Extra... extra) {
    const int *uem = nullptr, *uoff = nullptr;
    unsigned long long *ref_time = nullptr, *hyp_time = nullptr;
    if constexpr (MARG) {
        const RegionArgs& x = region_args(extra...);
        uem = x.uem, uoff = x.uoff, ref_time = x.ref_time, hyp_time = x.hyp_time;
    }
    extern __shared__ unsigned short dmask[];                     // [nth][hcap]: decisions per threshold and staged frame
    __shared__ uint4 scratch4[SCRATCH / 16];
    __shared__ unsigned long long bits[NWORDS], planes_r[NGRP][CMAX], wsum[GMAX][NT / 64][2], sums[2];
    __shared__ unsigned before[NWORDS];
    __shared__ unsigned long long regw[REG ? NGRP : 1], tsum[MARG ? CMAX : 1];
    __shared__ unsigned hsum[MARG ? GMAX : 1][CMAX];
    unsigned char* const scratch = (unsigned char*)scratch4;
    unsigned short* const rmask = (unsigned short*)scratch;       // step 1
    unsigned* const stage = (unsigned*)(scratch + EXT * 2);
    float* const fstage = (float*)scratch;                        // step 2
    unsigned long long* const P = (unsigned long long*)scratch;   // steps 3 and 4: [CMAX][PW]
    unsigned long long* const PH = P + CMAX * PW;                 // [NGRP][CMAX]
    unsigned short* const cum = (unsigned short*)(PH + NGRP * CMAX);   // [CMAX][PW]
    unsigned short* const hm = cum + CMAX * PW;                   // [TILE]

    const int rec = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long r0 = roff[rec], h0 = poff[rec];
    const long Trl = (long)roff[rec + 1] - r0, Thl = (long)poff[rec + 1] - h0;
    const long Tl = Trl > Thl * sub ? Trl : Thl * sub;
    if (Trl < 0 || Thl < 0 || Tl > DER_MAX_FRAMES) return;         // refused: the assignment kernel marks the recording
    const int Tr = (int)Trl, Th = (int)Thl, T = (int)Tl;
    const int ntiles = (int)(((long)T + TILE - 1) / TILE);
    const int ci = tid >> 4, cj = tid & 15;
    const int G = nth * nmed;

    float th[NTH];
#pragma unroll
    for (int i = 0; i < NTH; ++i) th[i] = i < nth ? thresholds[i] : __builtin_inff();
    int HK = 0;                                                   // the halo: half the largest median that is scored
#pragma unroll
    for (int i = 0; i < NMED; ++i)
        if (i < nmed) {
            const int k = medians[i];
            if (median_ok(k) && (k >> 1) > HK) HK = k >> 1;
        }
    int rot = tid % Ch;                                           // a thread starts its row at another column: LDS banks

    for (int k = tid; k < GMAX * (NT / 64) * 2; k += NT) (&wsum[0][0][0])[k] = 0;
    if constexpr (MARG)
        for (int k = tid; k < GMAX * CMAX; k += NT) (&hsum[0][0])[k] = 0;
    Regions rg;
    if constexpr (REG) rg = rec_regions(uem, uoff, rec);
    unsigned long long total = 0, kept = 0, rtime = 0, pair[GMAX];
#pragma unroll
    for (int q = 0; q < GMAX; ++q) pair[q] = 0;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();                                          // the last tile's reads of the scratch block (and wsum = 0)
        const int t0 = tile * TILE;                               // < T <= DER_MAX_FRAMES, so t0 + TILE + 2 h stays an int
        const int tl = T - t0 < TILE ? T - t0 : TILE;
        const int n = tl + 2 * h;                                 // reference frames t0 - h .. t0 + tl + h - 1
        const int k0 = t0 / sub, nk = (t0 + tl - 1) / sub - k0 + 1;
        const int ng = ((tl + NT - 1) / NT) * (NT / 64);

        // ---- 1. the reference side, as ref_side of der_tile.h
        if constexpr (REG) region_clear(regw);                   // the last tile's reads lie before the barrier above
        load_masks(ref, r0, Tr, Cr, t0 - h, n, rmask, stage);
        if constexpr (REG) region_fill(rg, t0, tl, regw);        // after the barriers of load_masks, before those of the bits
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
        unsigned nrk = 0;                                         // byte r: nr of frame r NT + tid if it is kept, else 0x80
        int hidx[ROUNDS];                                         // its hypothesis frame, from k0
        unsigned long long kp[ROUNDS];                            // ballot of keep
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int j = r * NT + tid, t = t0 + j;
            const bool valid = j < tl;
            unsigned rr = 0;
            bool keep = valid;
            hidx[r] = 0;
            if (valid) {
                rr = rmask[h + j];
                hidx[r] = t / sub - k0;
                if (h > 0) {                                      // boundaries b in [t - h + 1, t + h]: bits [j, j + 2 h)
                    const int lo = j, hi = j + 2 * h;
                    const unsigned clo = before[lo >> 6] + __popcll(bits[lo >> 6] & ((1ull << (lo & 63)) - 1));
                    const unsigned chi = before[hi >> 6] + __popcll(bits[hi >> 6] & ((1ull << (hi & 63)) - 1));
                    keep = chi == clo;
                }
            }
            const unsigned nr = __popc(rr);
            if (skip && nr >= 2) keep = false;
            if constexpr (REG) keep = keep && region_bit(regw, r);
            if (keep) {
                total += nr;
                kept += 1;
            }
            nrk |= (keep ? nr : 0x80u) << (8 * r);
            kp[r] = __ballot(keep);
            unsigned long long mine = 0;
            for (int s = 0; s < Cr; ++s) {
                const unsigned long long pr = __ballot(keep && (rr >> s & 1u));
                if (lane == s) mine = pr;
            }
            if (lane < CMAX) planes_r[r * (NT / 64) + wave][lane] = mine;
            if constexpr (MARG) rtime += __popcll(mine);
        }
        __syncthreads();                                          // rmask is done with: the block takes the float rows

        // ---- 2. posteriors of the frames ks .. ks + nhx - 1 -> decision masks per threshold
        const int ks = k0 - HK, nhx = nk + 2 * HK;                // nhx <= hcap by the launcher's arithmetic
        for (int c0 = 0; c0 < nhx; c0 += NT) {
            int fa = ks + c0, fb = ks + (c0 + NT < nhx ? c0 + NT : nhx);
            fa = fa < 0 ? 0 : fa;
            fb = fb > Th ? Th : fb;
            unsigned lead = 0;
            if (fa < fb) {
                const uintptr_t p = (uintptr_t)pred + (size_t)(h0 + fa) * Ch * 4, pe = p + (size_t)(fb - fa) * Ch * 4;
                const uintptr_t a = p & ~(uintptr_t)15;
                lead = (unsigned)(p - a) >> 2;
                const int nv = (int)((pe - a + 15) >> 4);
                for (int k = tid; k < nv; k += NT) {
                    const uintptr_t q = a + 16 * (uintptr_t)k;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (q >= p && q + 16 <= pe) v = *(const float4*)q;
                    else {
                        if (q >= p && q + 4 <= pe) v.x = *(const float*)q;
                        if (q + 4 >= p && q + 8 <= pe) v.y = *(const float*)(q + 4);
                        if (q + 8 >= p && q + 12 <= pe) v.z = *(const float*)(q + 8);
                        if (q + 12 >= p && q + 16 <= pe) v.w = *(const float*)(q + 12);
                    }
                    ((float4*)fstage)[k] = v;
                }
            }
            __syncthreads();
            const int e = c0 + tid, f = ks + e;
            if (e < nhx) {
                unsigned d[NTH];
#pragma unroll
                for (int i = 0; i < NTH; ++i) d[i] = 0;
                if (f >= fa && f < fb) {
                    const float* row = fstage + lead + (size_t)(f - fa) * Ch;
                    int best = -1;
                    float top = 0.f;
                    int cc = rot;
                    for (int c = 0; c < Ch; ++c) {
                        const float v = row[cc];
#pragma unroll
                        for (int i = 0; i < NTH; ++i) d[i] |= (v > th[i] ? 1u : 0u) << cc;
                        winner_update(best, top, v, cc);
                        cc = cc + 1 == Ch ? 0 : cc + 1;
                    }
                    if (sad) {
                        const bool speech = sad[h0 + f] != 0;
                        const unsigned win = best >= 0 ? 1u << best : 0u;
#pragma unroll
                        for (int i = 0; i < NTH; ++i) d[i] = speech ? (d[i] ? d[i] : win) : 0u;
                    }
                }
#pragma unroll
                for (int i = 0; i < NTH; ++i)
                    if (i < nth) dmask[i * hcap + e] = (unsigned short)d[i];
            }
            __syncthreads();
        }

        // ---- 3. and 4. the points, threshold-major
        const int nwd = ((nhx + NT - 1) / NT) * (NT / 64);        // plane words written per speaker
        for (int it = 0; it < nth; ++it) {
            const unsigned short* dm = dmask + it * hcap;
            for (int e0 = 0; e0 < nhx; e0 += NT) {
                const int e = e0 + tid;
                const unsigned d = e < nhx ? dm[e] : 0u;
                unsigned long long mine = 0;
                for (int s = 0; s < Ch; ++s) {
                    const unsigned long long pl = __ballot(d >> s & 1u);
                    if (lane == s) mine = pl;
                }
                if (lane < CMAX) P[lane * PW + (e0 >> 6) + wave] = mine;
            }
            __syncthreads();
            for (int idx = tid; idx < Ch * (nwd + 1); idx += NT) {  // cum[s][w]: decisions of speaker s in the words before w
                const int s = idx / (nwd + 1), w = idx - s * (nwd + 1);
                unsigned c = 0;
                for (int k = 0; k < w; ++k) c += __popcll(P[s * PW + k]);
                cum[s * PW + w] = (unsigned short)c;
            }
            __syncthreads();
            for (int ik = 0; ik < nmed; ++ik) {
                const int g = it * nmed + ik, k = medians[ik];
                if (!median_ok(k)) continue;                      // the same for every thread; the assignment kernel marks the point
                const int hk = k >> 1;
                for (int e = tid; e < nk; e += NT) {              // hypothesis frame k0 + e: bit e + HK of the planes
                    unsigned m = 0;
                    if (hk == 0) m = dm[e + HK];
                    else {
                        // decisions in [x - hk, x + hk] = prefix(x + hk + 1) - prefix(x - hk); position nwd * 64 reads one
                        // word beyond those written, under an empty bit mask
                        const int lo = e + HK - hk, hi = e + HK + hk + 1;
                        const unsigned long long mlo = (1ull << (lo & 63)) - 1, mhi = (1ull << (hi & 63)) - 1;
                        for (int s = 0; s < Ch; ++s) {
                            const int o = s * PW;
                            const unsigned clo = cum[o + (lo >> 6)] + __popcll(P[o + (lo >> 6)] & mlo);
                            const unsigned chi = cum[o + (hi >> 6)] + __popcll(P[o + (hi >> 6)] & mhi);
                            m |= (median_of(chi - clo, k) ? 1u : 0u) << s;
                        }
                    }
                    hm[e] = (unsigned short)m;
                }
                __syncthreads();
                // as score_point of der_tile.h: this thread's sum of min(nr, nh); this wave's sum of nh over kept frames
                unsigned bt = 0, nhw = 0, ht = 0;
#pragma unroll
                for (int r = 0; r < ROUNDS; ++r)
                    if (r * NT < tl) {
                        const unsigned m = r * NT + tid < tl ? hm[hidx[r]] : 0u;
                        const unsigned nr = nrk >> (8 * r) & 0xffu, nh = __popc(m);
                        if (nr < 0x80u) bt += nr < nh ? nr : nh;
                        unsigned long long mine = 0;
                        for (int s = 0; s < Ch; ++s) {
                            const unsigned long long ph = __ballot(m >> s & 1u);
                            if (lane == s) mine = ph;
                            nhw += __popcll(ph & kp[r]);
                        }
                        if (lane < CMAX) PH[(r * (NT / 64) + wave) * CMAX + lane] = mine;
                        if constexpr (MARG) ht += __popcll(mine & kp[r]);
                    }
                if constexpr (MARG)
                    if (lane < CMAX && ht) atomicAdd(&hsum[g][lane], ht);
                unsigned bw = 0;                                  // bt <= 4 * 16: 7 bits
#pragma unroll
                for (int b = 0; b < 7; ++b) bw += (unsigned)__popcll(__ballot(bt >> b & 1u)) << b;
                if (lane == 0) {
                    wsum[g][wave][0] += nhw;
                    wsum[g][wave][1] += bw;
                }
                __syncthreads();
                unsigned v = 0;
                if (ci < Cr && cj < Ch)
                    for (int q = 0; q < ng; ++q) v += __popcll(planes_r[q][ci] & PH[q * CMAX + cj]);
#pragma unroll
                for (int q = 0; q < GMAX; ++q) pair[q] += q == g ? v : 0u;
                // the next writes to hm come before a barrier that follows these reads of PH, those to PH and P after it
            }
        }
    }

    __syncthreads();
    if (tid < 2) sums[tid] = 0;
    if constexpr (MARG)
        if (tid < CMAX) tsum[tid] = 0;
    __syncthreads();
    if (total) atomicAdd(&sums[0], total);
    if (kept) atomicAdd(&sums[1], kept);
    if constexpr (MARG) gather_times(tsum, rtime);
    __syncthreads();
    if constexpr (MARG)                                           // thread (q, c): speaker c at the points q, q + 16
        for (int q = ci; q < G; q += NT / CMAX) {
            const size_t o = ((size_t)q * B + rec) * CMAX + cj;
            if (tsum[cj]) atomicAdd(ref_time + o, tsum[cj]);
            if (hsum[q][cj]) atomicAdd(hyp_time + o, (unsigned long long)hsum[q][cj]);
        }
    if (tid < G) {                                                // total, miss, false alarm, frames kept, sum of min(nr, nh)
        unsigned long long nhs = 0, both = 0;
        for (int w = 0; w < NT / 64; ++w) {
            nhs += wsum[tid][w][0];
            both += wsum[tid][w][1];
        }
        unsigned long long* out = counters + ((size_t)tid * B + rec) * 8;
        if (sums[0]) atomicAdd(out + 0, sums[0]);
        if (sums[0] - both) atomicAdd(out + 1, sums[0] - both);
        if (nhs - both) atomicAdd(out + 2, nhs - both);
        if (sums[1]) atomicAdd(out + 5, sums[1]);
        if (both) atomicAdd(out + 7, both);
    }
#pragma unroll
    for (int q = 0; q < GMAX; ++q)
        if (q < G && pair[q]) atomicAdd(cooc + (((size_t)q * B + rec) * CMAX + ci) * CMAX + cj, pair[q]);
}

}  // namespace

// hypothesis frames a tile stages at most: those under DER_TILE reference frames and the largest halo on each side
static int sweep_staged_frames(int sub) {
    const int core = (DER_TILE - 1) / sub + 2;
    return (core < DER_TILE ? core : DER_TILE) + 2 * HKMAX;
}

int eend_launch_collar_der_sweep(const unsigned char* ref, const int* roff, int Cr, const float* pred, const int* poff, int Ch,
                                 const unsigned char* sad, int B, const float* thresholds, int nth, const int* medians, int nmed, int sub,
                                 int h, int skip, unsigned long long* counters, unsigned long long* cooc, int* mapping,
                                 unsigned long long* totals, hipStream_t stream) {
    if (!ref || !roff || !pred || !poff || !thresholds || !medians || !counters || !cooc || !mapping) return EEND_EINVAL;
    if (!der_args_ok(Cr, Ch, B, sub, h)) return EEND_EINVAL;
    if (nth < 1 || nth > NTH || nmed < 1 || nmed > NMED || nth * nmed > GMAX) return EEND_EINVAL;
    if (((uintptr_t)pred & 3) != 0) return EEND_EINVAL;
    const int G = nth * nmed;
    if (!der_clear(counters, cooc, (long)G * B, stream)) return EEND_ELAUNCH;
    const int hcap = sweep_staged_frames(sub);
    hipLaunchKernelGGL((der_sweep_pass_kernel<false, false>), dim3(der_tile_groups(B), B), dim3(NT), (size_t)nth * hcap * 2, stream, ref,
                       roff, Cr, pred, poff, Ch, sad, thresholds, nth, medians, nmed, sub, h, skip ? 1 : 0, hcap, B, counters, cooc);
    if (hipGetLastError() != hipSuccess) return EEND_ELAUNCH;
    return eend_launch_collar_der_assign(roff, poff, Cr, Ch, B, G, sub, medians, nmed, counters, cooc, mapping, totals, stream);
}

int eend_launch_collar_der_sweep_regions(const unsigned char* ref, const int* roff, int Cr, const float* pred, const int* poff, int Ch,
                                         const unsigned char* sad, int B, const float* thresholds, int nth, const int* medians, int nmed,
                                         int sub, int h, int skip, const int* uem, const int* uoff, unsigned long long* counters,
                                         unsigned long long* cooc, int* mapping, unsigned long long* totals, unsigned long long* ref_time,
                                         unsigned long long* hyp_time, hipStream_t stream) {
    if (!ref || !roff || !pred || !poff || !thresholds || !medians || !counters || !cooc || !mapping || !ref_time || !hyp_time)
        return EEND_EINVAL;
    if (!der_args_ok(Cr, Ch, B, sub, h) || !der_regions_ok(uem, uoff)) return EEND_EINVAL;
    if (nth < 1 || nth > NTH || nmed < 1 || nmed > NMED || nth * nmed > GMAX) return EEND_EINVAL;
    if (((uintptr_t)pred & 3) != 0) return EEND_EINVAL;
    const int G = nth * nmed;
    if (!der_clear_times(counters, cooc, ref_time, hyp_time, (long)G * B, stream)) return EEND_ELAUNCH;
    const int hcap = sweep_staged_frames(sub);
    const dim3 grid(der_tile_groups(B), B);
    const size_t lds = (size_t)nth * hcap * 2;
    const RegionArgs x{uem, uoff, ref_time, hyp_time};
    if (uem)
        hipLaunchKernelGGL((der_sweep_pass_kernel<true, true, RegionArgs>), grid, dim3(NT), lds, stream, ref, roff, Cr, pred, poff, Ch, sad,
                           thresholds, nth, medians, nmed, sub, h, skip ? 1 : 0, hcap, B, counters, cooc, x);
    else
        hipLaunchKernelGGL((der_sweep_pass_kernel<false, true, RegionArgs>), grid, dim3(NT), lds, stream, ref, roff, Cr, pred, poff, Ch, sad,
                           thresholds, nth, medians, nmed, sub, h, skip ? 1 : 0, hcap, B, counters, cooc, x);
    if (hipGetLastError() != hipSuccess) return EEND_ELAUNCH;
    return eend_launch_collar_der_assign(roff, poff, Cr, Ch, B, G, sub, medians, nmed, counters, cooc, mapping, totals, stream);
}
