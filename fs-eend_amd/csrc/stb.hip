// Block-online EEND-EDA with a speaker-tracing buffer (reference FS-EEND/train/tfm_STB.py:147-204 with find_best_perm, cal_cor,
// upd_buf and upd_buf_FIFO of train/utils/utils.py): everything between two model calls of a stream, so that many streams advance in
// one batched model pass without the host reading a count or solving an assignment.  The contracts are in include/eend_hip.h.
//
// eend_stb_center_f32   [x_buf; x_i] - column mean -> the model's input rows.  A workgroup owns 64 columns of one sequence: thread
//                       (column, lane r of 16) sums rows r, r + 16, .. in float64, the 16 partials are added in the order r = 0 .. 15.
// eend_stb_track_f32    one workgroup per sequence does all that follows the head: sigmoid, the tracked width, the correlations
//                       (two passes over 64-row tiles staged in LDS, every sum float64 in ascending row order), the assignment
//                       (csrc/assign.h on one thread), the emitted block, the selection weights and race keys (float64, in LDS), the
//                       rank count, a prefix scan and the compaction of the kept rows into the other half of the stream's buffer.
// Every order of summation is fixed by (row, column) alone: a sequence's bits depend on its own rows only.
#include "common.h"
#include "kernels.h"
#include "assign.h"

namespace {

constexpr int SC = STB_MAX_SPEAKERS;    // 15 columns, rows of 15 floats
constexpr int SP = 16;                  // padded column count of the LDS tiles and of the cost matrix
constexpr int TNT = 512;                // threads of the track kernel
constexpr int TILE = 64;                // rows per staged tile

// murmur3's finaliser; the counter-based draw of row t of block k of a stream is mix(mix(mix(seed ^ 0x9E3779B9) + k) + t)
DEV unsigned stb_mix(unsigned x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

// correctly rounded to within one f32 ulp of the float64 sigmoid
DEV float stb_sigmoid(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }

struct Seq {
    const float* xbuf_src; const float* ybuf_src; const float* xblk;
    float* xbuf_dst; float* ybuf_dst; int* width; float* y_out;
    int L, n; unsigned k, seed;
};

// L and n of a descriptor, forced into what the buffers hold: 0 <= L <= buf_size, 1 <= n = T - L <= blk_size
DEV void stb_rows(const long* d, int T, int buf_size, int blk_size, int& L, int& n) {
    int lo = T - blk_size; lo = lo < 0 ? 0 : lo;
    int hi = T - 1 < buf_size ? T - 1 : buf_size;
    long l = d[1];
    L = l < lo ? lo : (l > hi ? hi : (int)l);
    n = T - L;
}

__global__ __launch_bounds__(1024) void stb_center_kernel(const long* __restrict__ desc, float* __restrict__ out, int T, int F,
                                                          int buf_size, int blk_size) {
    __shared__ double part[16][64];
    const int b = blockIdx.y, col = blockIdx.x * 64 + (threadIdx.x & 63), r = threadIdx.x >> 6;
    const long* d = desc + (size_t)b * STB_DESC_WORDS;
    int L, n;
    stb_rows(d, T, buf_size, blk_size, L, n);
    const float* xbuf = (const float*)d[0];
    const float* xblk = (const float*)d[2];
    const bool live = col < F;
    double s = 0.0;
    if (live)
        for (int t = r; t < T; t += 16) s += (double)(t < L ? xbuf[(size_t)t * F + col] : xblk[(size_t)(t - L) * F + col]);
    part[r][threadIdx.x & 63] = s;
    __syncthreads();
    double tot = 0.0;
    for (int i = 0; i < 16; ++i) tot += part[i][threadIdx.x & 63];
    const double mean = tot / (double)T;
    if (live) {
        float* o = out + (size_t)b * T * F;
        for (int t = r; t < T; t += 16) {
            const float x = t < L ? xbuf[(size_t)t * F + col] : xblk[(size_t)(t - L) * F + col];
            o[(size_t)t * F + col] = (float)((double)x - mean);
        }
    }
}

__global__ __launch_bounds__(TNT) void stb_track_kernel(const float* __restrict__ logits, const int* __restrict__ count,
                                                        const float* __restrict__ xc, const long* __restrict__ desc,
                                                        int* __restrict__ perm_out, int* __restrict__ sel_out, int T, int F,
                                                        int buf_size, int blk_size, int policy) {
    __shared__ double keys[STB_MAX_ROWS];
    __shared__ int pos[STB_MAX_ROWS];
    __shared__ float zb[TILE][SP], zp[TILE][SP];
    __shared__ double mean_b[SP], mean_p[SP], cost[SP * SP];
    __shared__ double au[SP + 1], av[SP + 1], aminv[SP + 1];
    __shared__ int ap[SP + 1], away[SP + 1], perm[SP], chunk[TNT];
    __shared__ bool aused[SP + 1];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long* d = desc + (size_t)b * STB_DESC_WORDS;
    int L, n;
    stb_rows(d, T, buf_size, blk_size, L, n);
    const float* xbuf_src = (const float*)d[0];
    const float* xblk = (const float*)d[2];
    const float* ybuf_src = (const float*)d[4];
    float* xbuf_dst = (float*)d[5];
    float* ybuf_dst = (float*)d[6];
    int* width = (int*)d[7];
    float* y_out = (float*)d[8];
    const unsigned k = (unsigned)d[9], seed = (unsigned)d[10];
    const float* lg = logits + (size_t)b * T * SC;
    int c = count[b];
    c = c < 0 ? 0 : (c > SC ? SC : c);
    int S = L == 0 ? 0 : *width;                                   // read before any thread writes it (barriers below)
    S = S < 0 ? 0 : (S > SC ? SC : S);
    const int Sn = S > c ? S : c;

    if (tid < SP) perm[tid] = tid;
    if (L > 0 && Sn > 0) {
        // pass 1: column means over the L buffer rows; thread j < 15 the tracked column j, thread 16 + j the predicted one
        double acc = 0.0;
        for (int t0 = 0; t0 < L; t0 += TILE) {
            const int rows = L - t0 < TILE ? L - t0 : TILE;
            __syncthreads();
            for (int i = tid; i < rows * SP; i += TNT) {
                const int r = i / SP, j = i % SP;
                zb[r][j] = j < S ? ybuf_src[(size_t)(t0 + r) * SC + j] : 0.f;
                zp[r][j] = j < c ? stb_sigmoid(lg[(size_t)(t0 + r) * SC + j]) : 0.f;
            }
            __syncthreads();
            if (tid < 2 * SP) {
                const float(*z)[SP] = tid < SP ? zb : zp;
                for (int r = 0; r < rows; ++r) acc += (double)z[r][tid & (SP - 1)];
            }
        }
        if (tid < SP) mean_b[tid] = acc / (double)L;
        else if (tid < 2 * SP) mean_p[tid - SP] = acc / (double)L;
        // pass 2: thread (r, q) the covariance and the two sums of squares of tracked column r and predicted column q
        const int r_ = tid / SP, q_ = tid % SP;
        double cov = 0.0, vr = 0.0, vq = 0.0, mr = 0.0, mq = 0.0;
        for (int t0 = 0; t0 < L; t0 += TILE) {
            const int rows = L - t0 < TILE ? L - t0 : TILE;
            __syncthreads();
            if (t0 == 0 && tid < SP * SP) { mr = mean_b[r_]; mq = mean_p[q_]; }
            for (int i = tid; i < rows * SP; i += TNT) {
                const int r = i / SP, j = i % SP;
                zb[r][j] = j < S ? ybuf_src[(size_t)(t0 + r) * SC + j] : 0.f;
                zp[r][j] = j < c ? stb_sigmoid(lg[(size_t)(t0 + r) * SC + j]) : 0.f;
            }
            __syncthreads();
            if (tid < SP * SP)
                for (int r = 0; r < rows; ++r) {
                    const double a = (double)zb[r][r_] - mr, e = (double)zp[r][q_] - mq;
                    cov += a * e; vr += a * a; vq += e * e;
                }
        }
        if (tid < SP * SP) cost[tid] = (r_ < Sn && q_ < Sn) ? -(cov / (sqrt(vr) * sqrt(vq) + 1e-6)) : 0.0;
        __syncthreads();
        if (tid == 0) {
            // rows r >= S and columns q >= c are padding with correlation 0: only the pairs of a tracked row and a predicted
            // column are taken from the solver, every other row takes the columns left over in ascending order
            assign_rows<double>(cost, SP, Sn, 1e30, au, av, aminv, ap, away, aused);
            bool taken[SP];
            for (int j = 0; j < SP; ++j) { taken[j] = false; perm[j] = -1; }
            for (int j = 1; j <= Sn; ++j) {
                const int r = ap[j] - 1, q = j - 1;
                if (r >= 0 && r < S && q < c) { perm[r] = q; taken[q] = true; }
            }
            int q = 0;
            for (int r = 0; r < Sn; ++r)
                if (perm[r] < 0) {
                    while (taken[q]) ++q;
                    perm[r] = q; taken[q] = true;
                }
            for (int r = Sn; r < SP; ++r) perm[r] = r;
        }
    }
    __syncthreads();
    if (perm_out && tid < SC) perm_out[(size_t)b * SC + tid] = perm[tid];

    // the emitted block: y_i[:, r] = z_i[:, perm[r]], zero columns beyond the new width
    for (int i = tid; i < n * SC; i += TNT) {
        const int t = i / SC, r = i % SC;
        const int q = perm[r];
        y_out[i] = (r < Sn && q < c) ? stb_sigmoid(lg[(size_t)(L + t) * SC + q]) : 0.f;
    }
    __syncthreads();                                               // y_out is read back below by other threads
    __threadfence_block();

    // which rows stay
    const bool select = T > buf_size;
    if (select && policy == STB_POLICY_KLD) {
        for (int t = tid; t < T; t += TNT) {
            const float* y = t < L ? ybuf_src + (size_t)t * SC : y_out + (size_t)(t - L) * SC;
            const int cols = t < L ? S : Sn;                       // a buffer row is zero beyond the old width
            double w = 1.0;
            if (Sn > 0) {
                double s = 0.0;
                for (int j = 0; j < cols; ++j) s += (double)y[j];
                w = 0.0;
                for (int j = 0; j < Sn; ++j) {
                    double p = (j < cols && s != 0.0) ? (double)y[j] / s : 0.0;
                    if (p == 0.0) p = 1e-6;
                    w += p * log(p * (double)Sn);
                }
                if (w < 0.0) w = 0.0;
                if (w == 0.0) w = 1e-6;
            }
            const unsigned h = stb_mix(stb_mix(stb_mix(seed ^ 0x9E3779B9u) + k) + (unsigned)t);
            const double u = ((double)h + 0.5) * (1.0 / 4294967296.0);
            keys[t] = w / -log(u);
        }
        __syncthreads();
        for (int t = tid; t < T; t += TNT) {
            const double kt = keys[t];
            int rank = 0;
            for (int s = 0; s < T; ++s) {
                const double ks = keys[s];
                rank += (ks > kt || (ks == kt && s < t)) ? 1 : 0;
            }
            pos[t] = rank < buf_size ? 1 : 0;
        }
    } else {
        for (int t = tid; t < T; t += TNT) pos[t] = (!select || t >= T - buf_size) ? 1 : 0;
    }
    __syncthreads();
    // exclusive prefix scan of the keep flags: a thread's run of rows, the runs' totals by one thread, the rows again
    const int per = (T + TNT - 1) / TNT;
    const int t_lo = tid * per, t_hi = t_lo + per < T ? t_lo + per : T;
    int mine = 0;
    for (int t = t_lo; t < t_hi; ++t) mine += pos[t];
    chunk[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < TNT; ++i) { const int v = chunk[i]; chunk[i] = run; run += v; }
    }
    __syncthreads();
    int run = chunk[tid];
    for (int t = t_lo; t < t_hi; ++t) {
        const int keep = pos[t];
        pos[t] = keep ? run : -1;
        run += keep;
    }
    __syncthreads();
    // compaction into the other half: block 0 stores its centred rows, later blocks the raw ones
    const float* xcb = xc + (size_t)b * T * F;
    const int cap = T < buf_size ? T : buf_size;
    for (int t = wave; t < T; t += TNT / 64) {
        const int p = pos[t];
        if (p < 0 || p >= cap) continue;                           // wave-uniform
        const float* xs = L == 0 ? xcb + (size_t)t * F : (t < L ? xbuf_src + (size_t)t * F : xblk + (size_t)(t - L) * F);
        for (int f = lane; f < F; f += 64) xbuf_dst[(size_t)p * F + f] = xs[f];
        if (lane < SC) {
            const float* y = t < L ? ybuf_src + (size_t)t * SC : y_out + (size_t)(t - L) * SC;
            ybuf_dst[(size_t)p * SC + lane] = (t < L && lane >= S) ? 0.f : y[lane];
        }
        if (sel_out && lane == 0) sel_out[(size_t)b * buf_size + p] = t;
    }
    if (tid == 0) *width = Sn;
}

}  // namespace

int eend_launch_stb_center(const long* desc, float* out, int B, int T, int F, int buf_size, int blk_size, hipStream_t stream) {
    if (!desc || !out || B < 1 || B > 65535 || T < 1 || F < 1 || F > STB_MAX_FEATURES || blk_size < 1 || buf_size < blk_size ||
        buf_size + blk_size > STB_MAX_ROWS || T > buf_size + blk_size)
        return EEND_EINVAL;
    hipLaunchKernelGGL(stb_center_kernel, dim3((F + 63) / 64, B), dim3(1024), 0, stream, desc, out, T, F, buf_size, blk_size);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}

int eend_launch_stb_track(const float* logits, const int* count, const float* xc, const long* desc, int* perm_out, int* sel_out, int B,
                          int T, int F, int buf_size, int blk_size, int policy, hipStream_t stream) {
    if (!logits || !count || !xc || !desc || B < 1 || T < 1 || F < 1 || F > STB_MAX_FEATURES || blk_size < 1 || buf_size < blk_size ||
        buf_size + blk_size > STB_MAX_ROWS || T > buf_size + blk_size || (policy != STB_POLICY_KLD && policy != STB_POLICY_FIFO))
        return EEND_EINVAL;
    hipLaunchKernelGGL(stb_track_kernel, dim3(B), dim3(TNT), 0, stream, logits, count, xc, desc, perm_out, sel_out, T, F, buf_size,
                       blk_size, policy);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
