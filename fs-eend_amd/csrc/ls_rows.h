// The per-row arithmetic of the LS-EEND state touches, shared by the single-stream kernels (stream.hip), the one-frame
// many-stream kernels (ls_multi.hip) and the chunk kernels (ls_chunk.hip), so that c frames of a chunk are bit for bit c
// one-frame calls in any of them.  Every contraction is written out (__builtin_fmaf) and the compiler's own contraction is
// off inside these functions (ret_norm_gate excepted, see there): every caller reaches the same instructions whatever
// surrounds the call.
#pragma once
#include "common.h"

// Four state elements of row kv[a][b..b+3]: s = s * keep + (v[a] * add) * k[b..], -> their part of q . kv_t[a][:].
DEV float ret_upd4(float4& s, const float4 kk, const float4 qq, float keep, float va) {
#pragma clang fp contract(off)
    s.x = __builtin_fmaf(s.x, keep, va * kk.x);
    s.y = __builtin_fmaf(s.y, keep, va * kk.y);
    s.z = __builtin_fmaf(s.z, keep, va * kk.z);
    s.w = __builtin_fmaf(s.w, keep, va * kk.w);
    return __builtin_fmaf(qq.w, s.w, __builtin_fmaf(qq.z, s.z, __builtin_fmaf(qq.x, s.x, qq.y * s.y)));
}

// kv_t[a][:] = kv_{t-1}[a][:] * keep + v[a] k[:] * add in place (FRESH: the old row is taken as zero, not read); -> q . kv_t[a][:]
template <bool FRESH>
DEV float ret_row_update(float* __restrict__ st, const float* __restrict__ kr, const float* __restrict__ qr, float keep, float va) {
#pragma clang fp contract(off)
    float o = 0.f;
#pragma unroll
    for (int b = 0; b < 64; b += 4) {
        float4 s = FRESH ? make_float4(0.f, 0.f, 0.f, 0.f) : *(const float4*)(st + b);
        o = o + ret_upd4(s, *(const float4*)(kr + b), *(const float4*)(qr + b), keep, va);
        *(float4*)(st + b) = s;
    }
    return o;
}

// The same update on a row held in registers (16 float4 = the lane's 64 state elements).
DEV float ret_row_update_reg(float4 (&s)[16], const float* __restrict__ kr, const float* __restrict__ qr, float keep, float va) {
#pragma clang fp contract(off)
    float o = 0.f;
#pragma unroll
    for (int b = 0; b < 16; ++b) o = o + ret_upd4(s[b], *(const float4*)(kr + b * 4), *(const float4*)(qr + b * 4), keep, va);
    return o;
}

// keep = sqrt(ps / (ps + 1)), add = 1 / sqrt(ps + 1) of the frame behind a running scale ps (decay 1: the scale is the frame
// count t).  The decay of the old state is applied 36 000 times over an hour of audio: formed in double and rounded once, the
// running product of the factors follows sqrt(s / t) to f32 rounding noise instead of accumulating the bias of the device's
// fast f32 sqrt / divide sequences.
DEV void ret_scale_factors(float ps, float& keep, float& add) {
    const float ns = ps + 1.0f;
    keep = (float)__builtin_sqrt((double)ps / (double)ns);
    add = (float)(1.0 / __builtin_sqrt((double)ns));
}

// Per-head LayerNorm (no affine) over the wave's 64 values o, then the swish gate g.  Left to the compiler's contraction on
// purpose: it folds the first step of the variance reduction into an fma on the shuffled operand (var = d*d + d'*d' with d' the
// neighbour lane's d), and that cannot be written in the source.  The expression is local, so every caller compiles it alike
// (the chunk tests hold them bit-equal on the device).
DEV float ret_norm_gate(float o, float g, float eps) {
    float sum = o;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) sum = wave_xor_add(sum, m);
    const float mean = sum * (1.0f / 64.0f);
    float var = (o - mean) * (o - mean);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) var = wave_xor_add(var, m);
    const float y = (o - mean) / __builtin_sqrtf(var * (1.0f / 64.0f) + eps);
    return g / (1.0f + __expf(-g)) * y;
}

// One frame through one channel's depthwise-conv cache cc[k-1] (shifted in place; fresh: read as zeros): the taps' sum.
DEV float dwconv_taps(float* __restrict__ cc, const float* __restrict__ wc, float xn, bool fresh, int k) {
#pragma clang fp contract(off)
    float y = wc[k - 1] * xn;
    float prev = xn;
    for (int j = k - 2; j >= 0; --j) {           // walk backwards so the shift can be done in place
        const float cur = fresh ? 0.f : cc[j];
        y = __builtin_fmaf(wc[j], cur, y);
        cc[j] = prev;                            // new_cache[j] = window[j+1]
        prev = cur;
    }
    return y;
}

// BatchNorm (eval; sc = weight / sqrt(var + eps)) and swish behind the taps' sum.
DEV float bn_swish(float y, float bm, float sc, float bb) {
#pragma clang fp contract(off)
    y = __builtin_fmaf(y - bm, sc, bb);
    return y / (1.0f + __expf(-y));
}

// One frame through one channel: taps, BatchNorm, swish.
DEV float dwconv_frame(float* __restrict__ cc, const float* __restrict__ wc, float xn, bool fresh, int k, float bm, float sc, float bb) {
    return bn_swish(dwconv_taps(cc, wc, xn, fresh, k), bm, sc, bb);
}
