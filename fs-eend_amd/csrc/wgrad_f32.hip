// Exact-f32 weight gradient of the EEND-EDA attractor path (eend_wgrad_f32):
//
//   dW[n][k] = sum_m dY[m][n] X[m][k]          db[n] = sum_m dY[m][n]            dY f32 [M][ldy], X f32 [M][ldx], all f32
//
// for the two LSTMs' W_hh (dG^T h_prev), the encoder LSTM's W_ih (dG^T xs) and their biases.  wgrad.hip's kernels take bf16 operands;
// these gradients are held to a summation-order distance of an fp32 autograd, so the products run on v_mfma_f32_16x16x4_f32, which is
// an m-ordered fmaf chain with one rounding per product.
//
// The M rows are cut into WGRAD_F32_SLICES slices of equal length (a multiple of the MFMA's 4 rows); the count is a constant, not a
// function of the device, so the bits are the same on every device and in every run.  A workgroup owns a 64 x 64 block of dW for one
// slice: wave w the 16 rows n0 + 16 w .. of it, as four 16 x 16 accumulators.  Per 4 rows of M a lane loads one element of dY and
// four of X (lanes 0 .. 15 of a quarter wave read 64 contiguous bytes) and issues four MFMAs; the workgroups of the first column block
// issue a fifth against a constant 1, which is the column sum of dY.  Rows past the end of a slice read as zero, which leaves an
// accumulator as it is.  The slices' partials go to the caller's workspace and are summed in slice order.
#include "common.h"
#include "kernels.h"

namespace {

__global__ __launch_bounds__(256) void wgrad_f32_kernel(const float* __restrict__ dY, int ldy, const float* __restrict__ X, int ldx, long M,
                                                        int N, int K, long rows_per_slice, float* __restrict__ part,
                                                        float* __restrict__ part_b) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = lane & 15, kk = lane >> 4;
    const int kt = blockIdx.x % (K / 64), nt = blockIdx.x / (K / 64);
    const int n0 = nt * 64 + wave * 16, k0 = kt * 64;
    const long ms = (long)blockIdx.y * rows_per_slice;
    const long me = ms + rows_per_slice < M ? ms + rows_per_slice : M;        // ms < M: the host launches no empty slice
    const bool with_b = part_b != nullptr && kt == 0;                          // workgroup-uniform
    f32x4 acc[4], accb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* yp = dY + n0 + f;
    const float* xp = X + k0 + f;
    for (long m0 = ms; m0 < me; m0 += 16) {                                    // 16 rows = 4 MFMA steps: 20 loads in flight
        float a[4], x[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long m = m0 + 4 * q + kk;
            const bool ok = m < me;
            const long mc = ok ? m : me - 1;                                   // a row of the slice: never outside the operands
            a[q] = yp[mc * ldy];
#pragma unroll
            for (int j = 0; j < 4; ++j) x[q][j] = xp[mc * ldx + 16 * j];
            if (!ok) {
                a[q] = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) x[q][j] = 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // D[n][k] += dY[m][n] X[m][k]: the lane holds rows n0 + 4 kk + r of column k0 + 16 j + f
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], x[q][j], acc[j], 0, 0, 0);
            }
            if (with_b) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], 1.0f, accb, 0, 0, 0);
        }
    }
    float* out = part + (size_t)blockIdx.y * N * K;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(size_t)(n0 + 4 * kk + r) * K + k0 + 16 * j + f] = acc[j][r];
    if (with_b && f == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) part_b[(size_t)blockIdx.y * N + n0 + 4 * kk + r] = accb[r];
    }
}

// out[i] = sum over the slices of part[s][i], s ascending
__global__ __launch_bounds__(256) void wgrad_f32_reduce_kernel(const float* __restrict__ part, long n, int nslices, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int k = 1; k < nslices; ++k) s += part[(size_t)k * n + i];
    out[i] = s;
}

}  // namespace

long eend_wgrad_f32_ws_floats(int N, int K, int with_bias) {
    if (N < 64 || K < 64 || N % 64 || K % 64) return 0;
    return (long)WGRAD_F32_SLICES * ((long)N * K + (with_bias ? N : 0));
}

int eend_launch_wgrad_f32(const float* dY, int ldy, const float* X, int ldx, long M, int N, int K, float* ws, long ws_bytes, float* dW,
                          float* db, hipStream_t stream) {
    const long need = eend_wgrad_f32_ws_floats(N, K, db != nullptr);
    if (!dY || !X || !ws || !dW || M < 1 || need == 0 || ldy < N || ldx < K || ws_bytes < need * (long)sizeof(float)) return EEND_EINVAL;
    // WGRAD_F32_SLICES slices of one length, a multiple of 4 rows; the last ones may be short or missing
    const long rps = 4 * ((M + 4L * WGRAD_F32_SLICES - 1) / (4L * WGRAD_F32_SLICES));
    const int nslices = (int)((M + rps - 1) / rps);
    float* part_b = db ? ws + (size_t)WGRAD_F32_SLICES * N * K : nullptr;
    hipLaunchKernelGGL(wgrad_f32_kernel, dim3((N / 64) * (K / 64), nslices), dim3(256), 0, stream, dY, ldy, X, ldx, M, N, K, rps, ws, part_b);
    const long nk = (long)N * K;
    hipLaunchKernelGGL(wgrad_f32_reduce_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, stream, ws, nk, nslices, dW);
    if (db) hipLaunchKernelGGL(wgrad_f32_reduce_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, part_b, (long)N, nslices, db);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
