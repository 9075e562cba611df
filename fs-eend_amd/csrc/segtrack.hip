// Live RTTM segments (SegmentTracker, live_rttm.py): the per-slot incremental form of activity_median_kernel + segments_kernel
// of postproc.hip.  make_rttm's filter is causal up to a look-ahead of h = k / 2 frames: the zero-padded median of frame u reads
// raw decisions u - h .. u + h, so it is final once frame u + h has arrived (or the stream has ended, zeros past the end), and
// so is a change point at u.  Per (slot, track) the device keeps the last k - 1 raw decisions as a bit word and the start of
// the open segment (-1: none, which is also the last finalised filtered decision); per slot a header {frames, count, overflow}
// and a ring of closed segments {track, start, end}.  Every feed of a stream with its end flag set therefore yields exactly
// the segments of make_rttm over the concatenated rows, however the rows were cut.
// The SAD instantiation gates the raw decisions with an external speech-activity mask (one uint8 flag per row), as
// sad_fuse_kernel of postproc.hip does for a whole file: a non-speech row is cleared, a speech row in which no track passed the
// threshold gets the track with the largest value.  Everything behind the raw decision bit is shared.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kBatch = 16;       // rows whose loads / decisions are issued together before the serial filter steps

// frames == 0 means "empty stream": the slot's words are not read (a reopened slot computes what a fresh one does).
// One wave per descriptor entry, lane = track.  desc i64 [n][2] = {address of the entry's first row, slot}.
// SAD: sad_desc i64 [n] = address of the entry's counts[e] flags, read only for the rows the entry brings.
template <bool SAD>
__global__ __launch_bounds__(64)
void segtrack_kernel(const long* __restrict__ desc, const int* __restrict__ counts, const int* __restrict__ ends,
                     const long* __restrict__ sad_desc, int ld, int col0, int ntracks, float thr, int k, int is_prob,
                     unsigned long long* __restrict__ hist_all, int* __restrict__ open_all, int* __restrict__ box, int S, int cap) {
    const int lane = threadIdx.x;
    const int e = blockIdx.x;
    const int slot = (int)desc[2 * e + 1];
    if (slot < 0 || slot >= S) return;
    const float* __restrict__ x = (const float*)desc[2 * e];
    const int cnt = max(counts[e], 0);
    const bool fin = ends && ends[e] != 0;
    int* hdr = box + (size_t)slot * (SEGTRACK_HDR + 3 * (size_t)cap);
    int* ring = hdr + SEGTRACK_HDR;
    const int n0 = __builtin_amdgcn_readfirstlane(hdr[0]);
    int base = __builtin_amdgcn_readfirstlane(hdr[1]);
    int ovf = __builtin_amdgcn_readfirstlane(hdr[2]);
    const bool on = lane < ntracks;
    const int h = k >> 1;
    const unsigned long long keep = (1ull << (k - 1)) - 1ull;         // k <= 63: the last k - 1 raw decisions
    unsigned long long hist = n0 > 0 ? hist_all[(size_t)slot * 64 + lane] : 0ull;
    int st = n0 > 0 ? open_all[(size_t)slot * 64 + lane] : -1;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const unsigned char* __restrict__ flags = nullptr;
    if constexpr (SAD) {
        if (cnt > 0) flags = (const unsigned char*)sad_desc[e];
    }

    // filtered decision f of frame u (final): a segment opens at u or the open one closes at u (exclusive end); closes are
    // appended in track order (ballot + prefix popcount), so the ring is ordered by end frame, then track.
    auto settle = [&](bool f, int u) {
        if (f && st < 0) st = u;
        const bool close = !f && st >= 0;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(close);
        if (m) {
            const int pos = base + __builtin_popcountll(m & lt);
            if (close) {
                if (pos < cap) {
                    ring[3 * pos] = lane;
                    ring[3 * pos + 1] = st;
                    ring[3 * pos + 2] = u;
                }
                st = -1;
            }
            base += __builtin_popcountll(m);
        }
    };

    for (int j0 = 0; j0 < cnt; j0 += kBatch) {
        unsigned dec = 0;                                             // bit i = raw decision of row j0 + i
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
            const int j = j0 + i;
            if constexpr (!SAD) {
                if (on && j < cnt) {
                    const float v = x[(size_t)j * ld + col0 + lane];
                    const bool d = is_prob ? v > thr : 1.0f / (1.0f + expf(-v)) > thr; // NaN: inactive
                    dec |= (unsigned)d << i;
                }
            } else {
                float v = 0.f;
                bool d = false;
                if (on && j < cnt) {
                    v = x[(size_t)j * ld + col0 + lane];
                    d = is_prob ? v > thr : 1.0f / (1.0f + expf(-v)) > thr;
                }
                if (j < cnt) {                                                         // wave-uniform, as is the row's flag
                    if (__builtin_amdgcn_readfirstlane((int)flags[j]) == 0) {
                        d = false;
                    } else if (__builtin_amdgcn_ballot_w64(d) == 0ull) {               // speech, nobody active: the largest value
                        const bool cand = on && j < cnt && v == v;                     // (raw logits order as their sigmoids do)
                        float top = cand ? v : -INFINITY;
#pragma unroll
                        for (int m = 1; m < 64; m <<= 1) top = fmaxf(top, __shfl_xor(top, m, 64));
                        const unsigned long long w = __builtin_amdgcn_ballot_w64(cand && v == top);
                        d = w != 0ull && lane == __builtin_ctzll(w);                   // ties: the lowest track (decision.h
                                                                                       // winner_update is the scalar statement)
                    }
                }
                dec |= (unsigned)d << i;
            }
        }
        const int nb = min(kBatch, cnt - j0);
        for (int i = 0; i < nb; ++i) {
            const int t = n0 + j0 + i;                                // raw frame index
            const unsigned long long w = hist | ((unsigned long long)((dec >> i) & 1u) << (k - 1));   // raw t - k + 1 .. t
            if (t >= h) settle(__builtin_popcountll(w) >= h + 1, t - h);
            hist = (w >> 1) & keep;
        }
    }
    const int n = n0 + cnt;
    if (fin) {
        for (int t = n; t < n + h; ++t) {                             // zero frames past the end finalise u = n - h .. n - 1
            if (t >= h) settle(__builtin_popcountll(hist) >= h + 1, t - h);
            hist >>= 1;
        }
        settle(false, n);                                             // segments still open end with the stream
    }
    hist_all[(size_t)slot * 64 + lane] = hist;
    open_all[(size_t)slot * 64 + lane] = st;
    if (base > cap) {
        ovf = 1;
        base = cap;
    }
    if (lane == 0) {
        hdr[0] = n;
        hdr[1] = base;
        hdr[2] = ovf;
    }
}

}  // namespace

template <bool SAD>
static int launch_segtrack(const long* desc, const int* counts, const int* ends, const long* sad_desc, int n, int ld, int col0,
                           int ntracks, float thr, int k, int is_prob, unsigned long long* hist, int* open, int* box, int S, int cap,
                           hipStream_t stream) {
    if (!desc || !counts || !hist || !open || !box || n < 0 || n > S || S <= 0 || cap <= 0 || ntracks < 1 || ntracks > 64 ||
        col0 < 0 || ld < col0 + ntracks || k < 1 || k > 63 || (k & 1) == 0 || (long)S * (SEGTRACK_HDR + 3L * cap) > 0x7fffffffL)
        return EEND_EINVAL;
    if (n == 0) return EEND_OK;
    hipLaunchKernelGGL(segtrack_kernel<SAD>, dim3(n), dim3(64), 0, stream, desc, counts, ends, sad_desc, ld, col0, ntracks, thr, k,
                       is_prob, hist, open, box, S, cap);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_segtrack(const long* desc, const int* counts, const int* ends, int n, int ld, int col0, int ntracks, float thr, int k,
                         int is_prob, unsigned long long* hist, int* open, int* box, int S, int cap, hipStream_t stream) {
    return launch_segtrack<false>(desc, counts, ends, nullptr, n, ld, col0, ntracks, thr, k, is_prob, hist, open, box, S, cap, stream);
}

int eend_launch_segtrack_sad(const long* desc, const int* counts, const int* ends, const long* sad_desc, int n, int ld, int col0,
                             int ntracks, float thr, int k, int is_prob, unsigned long long* hist, int* open, int* box, int S, int cap,
                             hipStream_t stream) {
    if (!sad_desc) return EEND_EINVAL;
    return launch_segtrack<true>(desc, counts, ends, sad_desc, n, ld, col0, ntracks, thr, k, is_prob, hist, open, box, S, cap, stream);
}
