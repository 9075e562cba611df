// Room impulse responses of shoebox rooms by the image method (eend_room_rir_f32; the contract is in include/eend_hip.h and
// DESIGN 10e).  A response is a sum over image sources (n, l, m, u, v, w) of  A w(k - tau):  a windowed sinc of 64 taps placed
// at the image's delay tau = q d, scaled by the walls' reflection coefficients over the distance.
//
// Gather, not scatter.  Item = (row, tile of ROOM_TILE = 64 consecutive taps), one workgroup of four waves; lane i of every
// wave owns tap k0 + i, so no two lanes ever add to one tap and nothing is atomic.  The images whose window meets the tile lie
// in the shell  (k0 - 32) / q < d < (klast + 32) / q.  They are found from the axes, never by walking the lattice:
//
//   segments    a segment is (y entry, z entry, u): the y and z image coordinates give r2 = py^2 + pz^2, and the admissible x
//               images of parity u are the n with  lo^2 - r2 < px^2 < hi^2 - r2,  px = +-sx + 2 n Lx - rx:  two short runs of
//               n from a pair of square roots (one run where the inner radius is not reached).  One lane per segment, 64
//               segments per wave step, the waves of the workgroup taking the steps round robin.  The runs are widened by a
//               hair (1e-9 relative): a candidate outside the shell is dropped below by an exact test, one missed would be lost;
//   candidates  an inclusive scan of the runs' lengths over the wave numbers the step's candidates; lane i takes candidate
//               base + i, finds its segment by a binary search of the scan (ds_bpermute, no LDS array) and computes in float64
//               what the contract wants in float64: p, d, tau = kc + f, A; and from them the four f32 words the taps need;
//   taps        the wave walks the live candidates (a ballot; the words by v_readlane, so the walk reads no memory): with
//               j = k - kc every lane adds  B (-1)^j / (j - f) sin^2(pi y / 64),  y = 32 - |j - f| taken as (32 - |j|) +- f so
//               that it is exact at the window's edge, B = -A sin(pi f) / pi (one sine per image, in float64), and
//               A sinc(f) sin^2(..) at j = 0.  About 40 instructions per candidate, half of the lanes live.
//
// The per-axis coefficient products x0^|n - u| x1^|n| are tabled in LDS per item (float64, by squaring; 0^0 = 1), only as deep
// as the tile's outer radius reaches.  The four waves' partial tiles meet in LDS and are summed as (w0 + w1) + (w2 + w3).  The
// order of every sum is a function of the row and the tile alone: the bits of a response do not depend on the call it is in.
//
// The whole file is compiled without floating-point contraction: the geometry is IEEE float64 operation by operation, as the
// float64 restatement computes it, so tau, kc and f are the same bits there and here.  Fused operations are written as fmaf.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256, NW = 4;
constexpr int T = ROOM_TILE, HW = ROOM_WINDOW / 2;
constexpr int MAXE = ROOM_MAX_AXIS;              // table entries per axis: 2 (2 N + 1)
constexpr int MAXN = (MAXE / 2 - 1) / 2;
enum { RM_L = 0, RM_S = 3, RM_R = 6, RM_BETA = 9, RM_Q = 15, RM_G = 16, RM_K = 17, RM_OUT = 18, RM_NTILES = 19, RM_WORDS = 20 };
static_assert(RM_WORDS == ROOM_WORDS && T == 64 && ROOM_WINDOW == 64, "one lane per tap; the window polynomial is for W = 64");
static_assert(2 * (2 * MAXN + 1) <= MAXE, "axis table");

constexpr double PI = 3.14159265358979323846;
constexpr double PW = PI / ROOM_WINDOW;          // the Hann factor is cos^2(pi x / W) = sin^2(pi (W / 2 - |x|) / W)

// sin(PW y) / y as a polynomial in y^2, 0 <= y <= 32 (the argument up to pi / 2): the terms to y^13, truncation 7e-10
constexpr double pw_pow(int n) { return n == 0 ? 1.0 : PW * pw_pow(n - 1); }
constexpr float HC0 = (float)(pw_pow(1)), HC1 = (float)(-pw_pow(3) / 6.0), HC2 = (float)(pw_pow(5) / 120.0),
                HC3 = (float)(-pw_pow(7) / 5040.0), HC4 = (float)(pw_pow(9) / 362880.0), HC5 = (float)(-pw_pow(11) / 39916800.0),
                HC6 = (float)(pw_pow(13) / 6227020800.0);

DEV double ipow(double b, int e) {               // b^e by squaring, e >= 0; 0^0 = 1
    double r = 1.0;
    while (e) {
        if (e & 1) r *= b;
        b *= b;
        e >>= 1;
    }
    return r;
}

// image coordinate minus receiver coordinate: ((+-s) + (2 n) L) - r, each operation rounded once
DEV double axis_off(double s, double L, double r, int n, int u) { return ((u ? -s : s) + (double)(2 * n) * L) - r; }

// sin(z) / z, |z| <= pi / 2, float64 to 3e-14: sinc(f) = sinc_poly((pi f)^2)
DEV double sinc_poly(double z2) {
    double p = 1.0 / 355687428096000.0;                             // 1 / 17!
    p = p * z2 - 1.0 / 1307674368000.0;
    p = p * z2 + 1.0 / 6227020800.0;
    p = p * z2 - 1.0 / 39916800.0;
    p = p * z2 + 1.0 / 362880.0;
    p = p * z2 - 1.0 / 5040.0;
    p = p * z2 + 1.0 / 120.0;
    p = p * z2 - 1.0 / 6.0;
    return p * z2 + 1.0;
}

__global__ __launch_bounds__(NT)
void room_rir_kernel(const long* __restrict__ rooms, const long* __restrict__ tiles, float* __restrict__ out) {
    __shared__ double coef[3][MAXE];
    __shared__ float part[NW][T];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long* tl = tiles + 2 * (long)blockIdx.x;
    const long* rw = rooms + RM_WORDS * tl[0];
    const int k0 = (int)tl[1], K = (int)rw[RM_K];
    const int klast = (k0 + T - 1 < K - 1) ? k0 + T - 1 : K - 1;
    const double Lx = __longlong_as_double(rw[RM_L]), Ly = __longlong_as_double(rw[RM_L + 1]), Lz = __longlong_as_double(rw[RM_L + 2]);
    const double sx = __longlong_as_double(rw[RM_S]), sy = __longlong_as_double(rw[RM_S + 1]), sz = __longlong_as_double(rw[RM_S + 2]);
    const double rx = __longlong_as_double(rw[RM_R]), ry = __longlong_as_double(rw[RM_R + 1]), rz = __longlong_as_double(rw[RM_R + 2]);
    const double q = __longlong_as_double(rw[RM_Q]), g = __longlong_as_double(rw[RM_G]);
    const double dhi = (double)(klast + HW) / q, dlo = (double)(k0 - HW) / q;       // the shell; dlo < 0 in a row's first tile
    const double eps2 = 1e-9 * (1.0 + dhi * dhi);                                   // a hair, on squared lengths

    // |n| <= dhi / (2 L) + 1 on every axis: |p| > 2 (|n| - 1) L for a source and a receiver inside the room
    const int Nx = (int)fmin(floor(dhi / (2.0 * Lx)) + 1.0, (double)MAXN);
    const int Ny = (int)fmin(floor(dhi / (2.0 * Ly)) + 1.0, (double)MAXN);
    const int Nz = (int)fmin(floor(dhi / (2.0 * Lz)) + 1.0, (double)MAXN);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const int N = ax == 0 ? Nx : ax == 1 ? Ny : Nz;
        const double b0 = __longlong_as_double(rw[RM_BETA + 2 * ax]), b1 = __longlong_as_double(rw[RM_BETA + 2 * ax + 1]);
        for (int e = tid; e < 2 * (2 * N + 1); e += NT) {
            const int n = (e >> 1) - N, u = e & 1;
            coef[ax][e] = ipow(b0, n - u < 0 ? u - n : n - u) * ipow(b1, n < 0 ? -n : n);
        }
    }
    __syncthreads();

    const int nY = 2 * (2 * Ny + 1), nZ = 2 * (2 * Nz + 1);
    const int nseg = 2 * nY * nZ, nsteps = (nseg + 63) >> 6;
    const int k = k0 + lane;
    const double i2L = 0.5 / Lx, fN = (double)Nx;
    float acc = 0.f;
    for (int c = wave; c < nsteps; c += NW) {
        // ---- one segment per lane: (y entry, z entry, u) -> the runs of n
        const int sidx = c * 64 + lane;
        const bool sv = sidx < nseg;
        const int pr = sv ? sidx >> 1 : 0;
        const int ez = pr / nY, ey = pr - ez * nY;
        const double py = axis_off(sy, Ly, ry, (ey >> 1) - Ny, ey & 1), pz = axis_off(sz, Lz, rz, (ez >> 1) - Nz, ez & 1);
        const double r2 = py * py + pz * pz, cyz = coef[1][ey] * coef[2][ez];
        const double hi2 = (dhi * dhi - r2) + eps2;
        int nneg = 0, cneg = 0, npos = 0, cpos = 0;
        if (sv && cyz != 0.0 && hi2 > 0.0) {
            const double base = ((lane & 1) ? -sx : sx) - rx;
            const double b = sqrt(hi2) * (1.0 + 1e-12);
            const double lo2 = dlo > 0.0 ? (dlo * dlo - r2) - eps2 : -1.0;
            const double lo_all = fmax(ceil((-b - base) * i2L - 1e-9), -fN), hi_all = fmin(floor((b - base) * i2L + 1e-9), fN);
            nneg = (int)lo_all;
            if (lo2 <= 0.0) {
                cneg = (int)hi_all - nneg + 1;
            } else {
                const double a = sqrt(lo2) * (1.0 - 1e-12);
                const int ihn = (int)fmin(floor((-a - base) * i2L + 1e-9), fN);
                int ilp = (int)fmax(ceil((a - base) * i2L - 1e-9), -fN);
                if (ilp <= ihn) ilp = ihn + 1;                              // never one n twice
                cneg = ihn - nneg + 1;
                npos = ilp;
                cpos = (int)hi_all - ilp + 1;
            }
            cneg = cneg < 0 ? 0 : cneg;
            cpos = cpos < 0 ? 0 : cpos;
        }
        const int cnt = cneg + cpos;
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        const int total = __builtin_amdgcn_readfirstlane(__shfl(incl, 63, 64));
        // ---- one candidate per lane, then the wave walks the live ones
        for (int base = 0; base < total; base += 64) {
            const bool cv = base + lane < total;
            const int id = cv ? base + lane : total - 1;
            int s = 0;                                                      // the first segment whose scan exceeds id
#pragma unroll
            for (int step = 32; step > 0; step >>= 1)
                if (__shfl(incl, s + step - 1, 64) <= id) s += step;
            const int off = id - (__shfl(incl, s, 64) - __shfl(cnt, s, 64));
            const int s_cneg = __shfl(cneg, s, 64), s_nneg = __shfl(nneg, s, 64), s_npos = __shfl(npos, s, 64);
            const double s_r2 = __shfl(r2, s, 64), s_cyz = __shfl(cyz, s, 64);
            const int u = s & 1;
            int n = off < s_cneg ? s_nneg + off : s_npos + (off - s_cneg);
            n = n < -Nx ? -Nx : n > Nx ? Nx : n;
            const double px = axis_off(sx, Lx, rx, n, u);
            const double d = sqrt(px * px + s_r2);
            const double tau = q * d, kcd = rint(tau), f = tau - kcd;
            const int kc = (int)fmin(kcd, 1e9);
            const double A = d > 0.0 ? ((g * coef[0][(n + Nx) * 2 + u]) * s_cyz) / d : 0.0;
            // live taps are j = k - kc in [-31, 31], and 32 with f > 0, -32 with f < 0: |j - f| < 32 exactly
            const bool live = cv && A != 0.0 && k0 - kc <= (f > 0.0 ? 32 : 31) && klast - kc >= (f < 0.0 ? -32 : -31);
            const double P = sinc_poly((PI * f) * (PI * f));
            const float ff = (float)f, Bv = (float)(-(A * f) * P), A0 = (float)(A * P);
            unsigned long long mask = __ballot(live);
            while (mask) {
                const int i = __builtin_ctzll(mask);
                mask &= mask - 1;
                const int kci = __builtin_amdgcn_readlane(kc, i);
                const float ffi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ff), i));
                const int Bi = __builtin_amdgcn_readlane(__float_as_int(Bv), i);
                const float A0i = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(A0), i));
                const int j = k - kci;
                const float jf = (float)j;
                const float sg = j > 0 ? 1.f : j < 0 ? -1.f : (ffi >= 0.f ? -1.f : 1.f);
                const float y = __builtin_fmaf(sg, ffi, 32.f - __builtin_fabsf(jf));          // 32 - |j - f|
                const float x = jf - ffi;
                float r = __builtin_amdgcn_rcpf(x);
                r = __builtin_fmaf(r, __builtin_fmaf(-x, r, 1.f), r);                          // one Newton step
                const float t = j == 0 ? A0i : __int_as_float(Bi ^ (int)((unsigned)j << 31)) * r;       // B (-1)^j / (j - f)
                const float y2 = y * y;
                float p = HC6;
                p = __builtin_fmaf(p, y2, HC5);
                p = __builtin_fmaf(p, y2, HC4);
                p = __builtin_fmaf(p, y2, HC3);
                p = __builtin_fmaf(p, y2, HC2);
                p = __builtin_fmaf(p, y2, HC1);
                p = __builtin_fmaf(p, y2, HC0) * y;                                            // sin(pi y / 64)
                acc += y > 0.f ? (t * p) * p : 0.f;
            }
        }
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (tid < T && k0 + tid < K)
        out[rw[RM_OUT] + k0 + tid] = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
}

}  // namespace

int eend_launch_room_rir(const long* rooms, int n_rows, const long* tiles, int n_tiles, float* out, hipStream_t stream) {
    if (n_rows < 0 || n_rows > ROOM_MAX_ROWS || n_tiles < 0) return EEND_EINVAL;
    if (n_rows == 0) return n_tiles ? EEND_EINVAL : EEND_OK;
    if (n_tiles < n_rows || !rooms || !tiles || !out) return EEND_EINVAL;
    hipLaunchKernelGGL(room_rir_kernel, dim3(n_tiles), dim3(NT), 0, stream, rooms, tiles, out);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
