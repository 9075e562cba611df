// The scalar rules of a frame's decisions, stated once for postproc.hip (sad_fuse_kernel, activity_median_kernel) and the DER
// sweep (der_sweep.hip steps 2 and 4); segtrack.hip holds wave-parallel forms of the same contracts.
#pragma once
#include "common.h"
#include "kernels.h"

namespace der {

// The winner of a speech row in which nobody passed the threshold: the largest posterior, never NaN, the lowest index on ties
// (as torch.argmax).  (best, top) start at (-1, any); value v at column c, the columns in any order.
DEV void winner_update(int& best, float& top, float v, int c) {
    if (v == v && (best < 0 || v > top || (v == top && c < best))) {
        best = c;
        top = v;
    }
}
// a median the sweep scores: odd, 1 .. DER_SWEEP_KMAX
DEV bool median_ok(int k) { return k >= 1 && k <= DER_SWEEP_KMAX && (k & 1); }
// the median of k (odd) binary values of which `ones` are 1: at least k / 2 + 1 of k
DEV bool median_of(unsigned ones, int k) { return ones >= (unsigned)(k >> 1) + 1; }

}  // namespace der
