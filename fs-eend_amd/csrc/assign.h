// The shortest-augmenting-path (Jonker-Volgenant / Hungarian) solver of an n x n assignment, O(n^3), run by one thread: n <= 16
// here, so this is latency, not throughput, work.  pit.hip runs it in fp64 on per-thread arrays, der_collar.hip in 64-bit
// integers on LDS arrays (inlined, so the arrays keep the address space the caller gave them).
#pragma once
#include "common.h"

// Minimum-cost perfect matching of a[i * lda + j], i, j in [0, n).  On return p[j], j in 1 .. n, is the row (from 1) matched to
// column j.  INF: above every sum of costs.  u, v, minv, p, way, used: n + 1 entries each, any contents.
template <typename T>
DEV void assign_rows(const T* a, int lda, int n, T INF, T* u, T* v, T* minv, int* p, int* way, bool* used) {
    for (int k = 0; k <= n; ++k) { u[k] = 0; v[k] = 0; p[k] = 0; way[k] = 0; }
    for (int i = 1; i <= n; ++i) {
        p[0] = i;
        int j0 = 0;
        for (int k = 0; k <= n; ++k) { minv[k] = INF; used[k] = false; }
        do {
            used[j0] = true;
            const int i0 = p[j0];
            const T ui = u[i0];
            T delta = INF;
            int j1 = 0;
            for (int j = 1; j <= n; ++j)
                if (!used[j]) {
                    const T cur = a[(i0 - 1) * lda + (j - 1)] - ui - v[j];
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
}
