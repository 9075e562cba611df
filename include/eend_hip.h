/*
 * eend_hip.h -- C-ABI of libeend_hip.so: the MI355X (gfx950) kernels behind the
 * FS-EEND / LS-EEND frame-wise diarization forward.
 *
 * The reference (Audio-WestlakeU/FS-EEND) is pure Python on torch.nn and has no FFI of
 * its own; each entry point below replaces the stock ATen kernels that one group of
 * reference lines dispatches, and cites those lines (paths relative to the reference
 * root).  The Python host (fs-eend_amd/) binds them with ctypes; INTEGRATION.md shows
 * the stub.
 *
 * Conventions (every entry point):
 *   - returns 0 on success, EEND_EINVAL (-1) for a rejected argument, EEND_ELAUNCH (-2)
 *     when the HIP launch failed; never throws, never allocates, never synchronises;
 *   - all pointers are DEVICE pointers owned by the caller and must stay alive until the
 *     stream has executed the call; `stream` is a hipStream_t passed as void*;
 *   - kernels are stateless and stream ordered (safe under hipGraph capture);
 *   - "slab" layout: activations of `nseq` sequences are stored [nseq][Tp][D] with
 *     Tp % 64 == 0 >= T (frames t >= T are padding the caller never reads);
 *   - f16 = IEEE binary16, bf16 = bfloat16, f32 = IEEE binary32; accumulation is f32.
 */
#ifndef EEND_HIP_H
#define EEND_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define EEND_OK 0
#define EEND_EINVAL (-1)
#define EEND_ELAUNCH (-2)

/* ABI version of this header (bumped on any signature change).
 *   4 (round 6): eend_attnout_ffn_fused_f16 gained out_lo_f16 / Wo_lo and eend_convert_fanout_f32 gained out_lo_f16 (round 5, shipped
 *      under 3 by mistake); a caller built against the version-3 header must refuse this library. */
/*   5 (round 6): the dropout mask function of eend_dropout changed (two 24-bit-multiply rounds instead of the murmur3 finaliser): a caller
 *      that regenerates masks itself (as oracle/dropout_ref.py does) must follow; eend_inproj_heads_train_bf16 accepts NULL Qt / Kt;
 *      x_is_f16 of eend_wgrad[_bias]_bf16 became a flag word (bits 1, 2: blocked operands); new eend_ffn_train_stream_* entries. */
#define EEND_ABI_VERSION 5
int eend_abi_version(void);

/* Eval-mode BatchNorm1d over features + cast + zero pad to the frame slab.
 * Replaces FS-EEND/nnet/model/onl_tfm_enc_1dcnn_enc_linear_non_autoreg_pos_enc_l2norm.py:165-166
 * (pad_sequence(-1) is done by the host; BN uses running stats) and, with apply_bn = 0,
 * the plain cast in front of LS-EEND's input projection (LS-EEND/nnet/conformer/encoder.py:195).
 * x f32 [B][T][Fin] -> out f16 [B][Tp][Fpad] (Fpad % 64 == 0, zero filled beyond Fin / T). */
int eend_bn_cast_pad_f16(const float* x, const float* bn_weight, const float* bn_bias,
                         const float* bn_mean, const float* bn_var, float eps, void* out_f16,
                         int B, int T, int Tp, int Fin, int Fpad, int apply_bn, void* stream);

/* The same, reading the B utterances through a device table of pointers (x_ptrs[b] -> f32
 * [lens[b]][Fin]) and using `pad_value` for frames lens[b] <= t < T: pad_sequence (FS model :165 pads
 * with -1, LS model :280 with 0) + BatchNorm + cast + slab padding in ONE launch. */
int eend_gather_bn_cast_pad_f16(const void* const* x_ptrs, const int* lens, float pad_value,
                                const float* bn_weight, const float* bn_bias, const float* bn_mean,
                                const float* bn_var, float eps, void* out_f16, int B, int T, int Tp, int Fin,
                                int Fpad, int apply_bn, void* stream);

/* Encoder input in ONE launch (encin.hip): pad_sequence(pad_value) + BatchNorm(eval) + cast, the input projection
 * (in_size -> 256) and its LayerNorm, i.e. eend_gather_bn_cast_pad_f16 followed by eend_linear_res_ln_f16 without a residual
 * (FS model :162-170: pad_sequence(-1), self.bn, enc.encoder, enc.encoder_norm) -- the f32 features are read once, the f16 copy
 * never exists.  x_ptrs: device table of B pointers to (len_b, Fin) f32 rows (16-byte aligned), lens[b] frames valid (frames
 * len_b <= t < T take pad_value through the BatchNorm, frames T <= t < Tp are zero before the projection, exactly as the pair);
 * W f16 [256][ldw] with columns >= Fin zero; out_f16 [B*Tp][256], out_f32 optional.  Supported where
 * eend_encoder_input_ok(Fin, Tp, ldw) != 0 (320 < Fin <= 384, Tp a multiple of 32); EEND_EINVAL otherwise. */
int eend_encoder_input_ok(int Fin, int Tp, int ldw);
int eend_encoder_input_f16(const float* const* x_ptrs, const int* lens, float pad_value, const float* bn_w, const float* bn_b,
                           const float* bn_mean, const float* bn_var, float bn_eps, const void* W_f16, int ldw, const float* bias,
                           const float* gamma, const float* beta, float eps, float* out_f32, void* out_f16, int B, int T, int Tp,
                           int Fin, void* stream);

/* out = act(A W^T + bias), f16 in / f16 out, f32 accumulate; act: 0 none, 1 ReLU, 2 Swish.
 * torch.nn.Linear call sites: FFN linear1+ReLU of nn.TransformerEncoderLayer (FS model :147) and of
 * the fusion layer (FS-EEND/nnet/modules/merge_tfm_encoder.py:397-399), packed in-proj of the speaker
 * MHA (merge_tfm_encoder.py:388-394), Linear+Swish of LS-EEND's FeedForwardModule
 * (LS-EEND/nnet/conformer/feed_forward.py:49-50).  A [M][lda], W [N][ldw], N % 128 == 0, K % 64 == 0; up to 16 rows with
 * 16-byte aligned A / W rows take any N and K % 8 == 0.  ldo % 4 == 0, and ldo % 8 == 0 where the GEMM tile serves the call
 * (it writes 16-byte pieces of the output rows); eend_linear_route names the kernel a call takes. */
int eend_linear_f16(const void* A, int lda, const void* W, int ldw, const float* bias, void* out_f16,
                    int ldo, int M, int N, int K, int act, void* stream);

/* Pointwise Conv1d(D -> 2D) + GLU over channels (LS-EEND/nnet/conformer/convolution.py:141-142,
 * activation.py:39-41).  Wi / bias_i have the value and gate rows interleaved
 * (row 2n = W[n], row 2n+1 = W[n + N2/2]); out[m][n] = v_n * sigmoid(g_n), f16 [M][ldo]. */
int eend_linear_glu_f16(const void* A, int lda, const void* Wi, int ldw, const float* bias_i, void* out_f16,
                        int ldo, int M, int N2, int K, void* stream);

/* Packed MHA in-projection (3D x D) whose epilogue scatters Q, K (bf16 [nseq][H][Tp][dh]) and
 * V transposed (bf16 [nseq][H][dh][Tp]) for eend_attn_causal_bf16.  Replaces the in-proj half of
 * nn.MultiheadAttention in nn.TransformerEncoderLayer (FS model :147) and _sa_block1
 * (merge_tfm_encoder.py:379-385).  A f16 [nseq*Tp][lda], W f16 [3*H*dh][ldw], bias f32 [3*H*dh]. */
int eend_inproj_heads_bf16(const void* A, int lda, const void* W, int ldw, const float* bias, void* Q_bf16,
                           void* K_bf16, void* Vt_bf16, int nseq, int Tp, int H, int dh, int K, void* stream);

/* out = LayerNorm((A W^T + bias) * alpha + res) * gamma + beta, N = 256; writes f32 (residual
 * stream) and f16 (next MFMA operand) copies; res / out32 / out16 / gamma may be null.  Replaces
 * Linear -> LayerNorm (FS model :173-174), out-proj + residual + norm1 / norm11 / norm21 and
 * linear2 + residual + norm2 / norm22 (torch TransformerEncoderLayer; merge_tfm_encoder.py:364,373-374),
 * and with alpha = 0.5 the half-step FFN + block-final LayerNorm of the Conformer block
 * (LS-EEND/nnet/conformer/encoder.py:104-110). */
int eend_linear_res_ln_f16(const void* A, int lda, const void* W, int ldw, const float* bias,
                           const float* res, float alpha, const float* gamma, const float* beta, float eps,
                           float* out_f32, void* out_f16, int M, int K, void* stream);

/* y = (A W^T + bias) * alpha + res -> out_f32 (residual stream, not normalised) and
 * LayerNorm(y) * gamma + beta -> out_f16: the pre-norm input of the NEXT Conformer sub-module
 * (feed_forward.py:48, attention.py:100, convolution.py:139) fused into its producer.  N = 256. */
int eend_linear_res_scale_ln16_f16(const void* A, int lda, const void* W, int ldw, const float* bias,
                                   const float* res, float alpha, const float* gamma, const float* beta,
                                   float eps, float* out_f32, void* out_f16, int M, int K, void* stream);

/* out = (A W^T + bias) * alpha + res, N = 256, f32 + f16 copies (no normalisation).  Replaces the
 * LS-EEND residual wrappers: ResidualConnectionModule with module_factor 0.5 / 1
 * (LS-EEND/nnet/conformer/modules.py:32-33) around the second Linear of FeedForwardModule
 * (feed_forward.py:47-57), the retention out_proj (LS-EEND/nnet/modules/retention.py:226) and the
 * last pointwise conv of ConformerConvModule (convolution.py:138-149). */
int eend_linear_res_scale_f16(const void* A, int lda, const void* W, int ldw, const float* bias,
                              const float* res, float alpha, float* out_f32, void* out_f16, int M, int K,
                              void* stream);

/* Look-ahead Conv1d(cin -> 256, ktaps, padding = pad) as an implicit GEMM, + bias, then
 * x / ||x||_2 (no eps).  Frames >= ilens[seq] read as zero (the reference truncates to ilen and
 * zero re-pads before the conv).  Replaces FS model :38-41 / LS model :80-87.
 * X f16 [nseq][Tp][cin]; Wr f16 [256][ktaps*cin] with Wr[o][tap*cin + i] = conv.weight[o][i][tap]. */
int eend_conv1d_l2norm_f16(const void* X, const void* Wr, const float* bias, const int* ilens,
                           float* out_f32, void* out_f16, int nseq, int Tp, int cin, int ktaps, int pad,
                           void* stream);

/* The same operator on a packed weight stream (conv_stream.hip; cin = 256, ktaps <= 24): the tile's input rows are staged once in
 * LDS and every tap reads them shifted, the weights -- re-ordered once per parameter version by eend_conv_stream_pack_f16 from the
 * same Wr [256][ktaps*256] into eend_conv_stream_elems(ktaps) f16 elements -- flow through an LDS-DMA ring.  EEND_EINVAL where
 * eend_conv_stream_ok(cin, ktaps, pad) == 0 (the caller keeps eend_conv1d_l2norm_f16). */
int eend_conv_stream_elems(int ktaps);
int eend_conv_stream_ok(int cin, int ktaps, int pad);
int eend_conv_stream_pack_f16(const void* Wr, void* stream_out, int ktaps, void* stream);
int eend_conv1d_l2norm_stream_f16(const void* X, const void* wstream, const float* bias, const int* ilens, float* out_f32,
                                  void* out_f16, int nseq, int Tp, int ktaps, int pad, void* stream);

/* attr0[(b,c)][t][:] = W1 emb[b][t][:] + pc[c][:], the factored form of
 * convert(cat(emb, pe[c])) (FS model :113-114, LS model :216-217): W1 = convert.weight[:, :D],
 * pc[c] = convert.weight[:, D:] pe[c] + convert.bias.  E f16 [B][Tp][256] ->
 * out f32/f16 [B*C][Tp][256] (decoder slab, sequence index = b*C + c). */
int eend_convert_fanout_f16(const void* E, const void* W1, const float* pc, float* out_f32, void* out_f16,
                            int B, int Tp, int C, void* stream);
/* The same stage with f32 operands on the exact-f32 MFMA: E_f32 [B][Tp][256], W_f32 = convert.weight ([256][ldw], the first 256
 * columns are W1).  The LS-EEND batch forward takes it (the decoder retention's per-head LayerNorm, eps 1e-6, amplifies the f16
 * operand rounding of this linear; with 12 speaker slots the f16 form left the 1e-3 bar).  out_f32 may be NULL.  out_lo_f16 (optional,
 * same layout as out_f16): f16(v - f16(v)), the remainder the retention's query path reads next to out_f16 (eend_retention_stream_f16). */
int eend_convert_fanout_f32(const float* E_f32, const float* W_f32, int ldw, const float* pc, float* out_f32, void* out_f16,
                            void* out_lo_f16, int B, int Tp, int C, void* stream);

/* Fused causal MHA core: softmax(mask(Q K^T / sqrt(dh))) V with
 * allowed(i,j) <=> j - i <= mask_delay && j < kv_len evaluated on indices (the (T,T) {0,-inf} tensor
 * of FS model :107-110,:152-155 is never built; has_mask=False is mask_delay >= Tp, kv_len = T).
 * dh = 64.  Q,K bf16 [nseq][H][Tp][64], Vt bf16 [nseq][H][64][Tp] -> O f16 [nseq*Tp][ldo]. */
int eend_attn_causal_bf16(const void* Q, const void* K, const void* Vt, void* O_f16, int nseq, int H,
                          int Tp, int ldo, int mask_delay, int kv_len, float scale, void* stream);

/* Whole position-wise feed-forward block in one launch, hidden activations never leave the CU:
 *   y = (act(X W1^T + b1) W2^T + b2) * alpha + res ;  out_f16 = LayerNorm(y) * gamma + beta ;
 *   out_f32 = LayerNorm(y)... (residual_stream_unnormalised = 0) or y (= 1).
 * act: 1 ReLU (nn.TransformerEncoderLayer linear1/linear2 + norm2, FS model :147; _ff_block + norm22,
 * FS merge_tfm_encoder.py:374,397-399, LS merge_retnet_layer.py:252,309-311), 2 Swish (Conformer
 * FeedForwardModule + half-step residual, LS conformer/feed_forward.py:47-57, encoder.py:76-110).
 * X f16 [M][ldx] (256 features), W1 f16 [F][256], W2 f16 [256][F], F % 64 == 0. */
int eend_ffn_fused_f16(const void* X, int ldx, const void* W1, const float* b1, const void* W2, const float* b2,
                       const float* res, float alpha, const float* gamma, const float* beta, float eps,
                       float* out_f32, void* out_f16, int M, int F, int act, int residual_stream_unnormalised,
                       void* stream);

/* Attention out-projection + residual + norm1 AND the position-wise feed-forward block + residual +
 * norm2 of one post-LN layer in ONE launch (ReLU FFN):
 *   x = LayerNorm1(A Wo^T + bo + res) * g1 + be1 ;  out = LayerNorm2(relu(x W1^T + b1) W2^T + b2 + x) * g2 + be2
 * i.e. nn.TransformerEncoderLayer's out_proj/dropout1/norm1 + linear1/linear2/norm2 (FS model :147) and
 * the second half of the fusion layers (out_proj of self_attn2 + norm21, _ff_block + norm22: FS
 * merge_tfm_encoder.py:371-376,397-399; LS merge_retnet_layer.py:248-253,309-311).  x never leaves the CU.
 * A f16 [M][lda] (attention output), Wo f16 [256][256], res f32 [M][256] (stream before the attention
 * sub-layer; may alias out_f32), out_f32 f32 [M][256], out_f16 f16 [M][256] (may alias A); out_lo_f16 (optional, f16 [M][256]):
 * f16(out - f16(out)), the remainder next to out_f16 (the next layer's retention reads both: eend_retention_stream_f16).  Wo_lo (optional,
 * f16 [256][256]): f16(Wo_f32 - f16(Wo_f32)) -- the out-projection then runs as two products on the same A fragments (the weight's f16
 * rounding was the largest single term of the worst LS-EEND logit at 12 speaker slots; +3 % of the launch). */
int eend_attnout_ffn_fused_f16(const void* A, int lda, const void* Wo, const float* bo, const float* res,
                               const float* g1, const float* be1, float eps1, const void* W1, const float* b1,
                               const void* W2, const float* b2, const float* g2, const float* be2, float eps2,
                               float* out_f32, void* out_f16, void* out_lo_f16, const void* Wo_lo, int M, int F, void* stream);
/* The two post-norm joins above with the residual taken from the f16 stream: in a post-norm stack (nn.TransformerEncoderLayer,
 * merge_tfm_encoder.py:356-376) the residual IS the previous LayerNorm's output, whose f16 copy the next MFMA reads anyway, so
 * the f32 stream's write + read (1 KB per row per sub-layer, the dominant traffic of the HBM-bound out-projection GEMM) can be
 * dropped; out_f32 may be NULL (only the last layer's output is needed in f32, by the head).  Emulated on the oracle: max
 * |d logit| 2.4e-4 -> 2.6e-4. */
int eend_linear_res16_ln_f16(const void* A, int lda, const void* W, int ldw, const float* bias, const void* res_f16,
                             float alpha, const float* gamma, const float* beta, float eps, float* out_f32,
                             void* out_f16, int M, int K, void* stream);
int eend_attnout_ffn_fused_res16_f16(const void* A, int lda, const void* Wo, const float* bo, const void* res_f16,
                                     const float* g1, const float* be1, float eps1, const void* W1, const float* b1,
                                     const void* W2, const float* b2, const float* g2, const float* be2, float eps2,
                                     float* out_f32, void* out_f16, int M, int F, void* stream);

/* Rows one launch of the packed-stream layer-tail kernels addresses (32-bit buffer offsets, one grid of tiles of prefetch ahead);
 * eend_ffn_stream_f16 / eend_attnout_ffn_stream_f16 serve larger M in several launches over row ranges of that size. */
int eend_ffn_stream_max_rows(int lda);
/* TEST HOOK (process-wide, not for production callers): force the row-tile size of the packed-stream layer-tail kernels
 * (tile_fragments = 2 / 3 for 128- / 192-row tiles, 0 = the launcher's cost model) and cap the rows of one launch
 * (max_rows_per_launch > 0; 0 = the 32-bit addressing limit), so that the tile-size agreement and the multi-launch path can be
 * exercised at small sizes (tests/test_hip_ffn_stream.py).  Replaces the EEND_FS_NJ / EEND_FFN_STREAM_MAX_ROWS environment
 * switches of rounds 4 - 5. */
int eend_debug_ffn_stream_set(int tile_fragments, long max_rows_per_launch);

/* Round 4: the same two operators (eend_ffn_fused_f16 / eend_attnout_ffn_fused[_res16]_f16; reference sites as above:
 * nn.TransformerEncoderLayer of FS model :147, merge_tfm_encoder.py:356-399, LS merge_retnet_layer.py:240-253,
 * conformer/feed_forward.py:47-57) on a PACKED WEIGHT STREAM.  eend_ffn_stream_pack_f16 re-orders Wo (optional, [256][256]),
 * W1 ([F][256]) and W2 ([256][F]) once per parameter version into the sequence of 1-KB MFMA fragments the kernel consumes
 * (eend_ffn_stream_elems(F, with_wo) f16 elements; F a multiple of 64, at most 2048).  With Wo the stream serves eend_attnout_ffn_stream_f16
 * (the contraction index of W1 follows the register layout LayerNorm1 leaves), without it eend_ffn_stream_f16 (natural order).
 * The kernel gives one wave 48 token rows end to end: the hidden activations and x stay in its registers, weights flow
 * through a 4-slot LDS-DMA ring.  Results equal the un-packed entries up to fp32 summation order. */
int eend_ffn_stream_elems(int F, int with_wo);
int eend_ffn_stream_pack_f16(const void* Wo, const void* W1, const void* W2, void* stream_out, int F, void* stream);
int eend_ffn_stream_f16(const void* X, int ldx, const void* wstream, const float* b1, const float* b2,
                        const float* res, float alpha, const float* gamma, const float* beta, float eps,
                        float* out_f32, void* out_f16, int M, int F, int act, int residual_stream_unnormalised,
                        void* stream);
/* The LO form (round 6; LS-EEND decoder layer tail, merge_retnet_layer.py:240-253 on the f32 attractor rows): the out-projection weight
 * as an f16 hi / lo pair (Wo_lo = f16(Wo - f16(Wo)): a second product on the same input fragments; eend_ffn_stream_elems(F, 2) elements)
 * and the rows leaving as f32 AND as an f16 hi / lo pair (out_lo_f16 = f16(y - f16(y)); may be NULL), as eend_attnout_ffn_fused_f16
 * with Wo_lo / out_lo_f16 does on un-packed weights. */
int eend_ffn_stream_pack_lo_f16(const void* Wo, const void* Wo_lo, const void* W1, const void* W2, void* stream_out, int F, void* stream);
int eend_attnout_ffn_stream_lo_f16(const void* A, int lda, const void* wstream, const float* bo, const float* res, const float* g1,
                                   const float* be1, float eps1, const float* b1, const float* b2, const float* g2, const float* be2,
                                   float eps2, float* out_f32, void* out_f16, void* out_lo_f16, int M, int F, void* stream);
/* res (f32) or res_f16 (f16), exactly one non-null; out_f32 may be NULL */
int eend_attnout_ffn_stream_f16(const void* A, int lda, const void* wstream, const float* bo, const float* res,
                                const void* res_f16, const float* g1, const float* be1, float eps1, const float* b1,
                                const float* b2, const float* g2, const float* be2, float eps2,
                                float* out_f32, void* out_f16, int M, int F, void* stream);

/* First half of a speaker-fusion decoder layer in one launch on a packed weight stream (spk_stream.hip):
 *   x1 = LayerNorm11(A Wo1^T + bo1 + res)    (out-projection of the time-axis attention, residual, norm11)
 *   O  = MHA over the C slots of every frame of (x1 W_in^T + b_in)      (self_attn2 of the fusion layers)
 * i.e. eend_linear_res16_ln_f16 followed by eend_spk_qkv_attn_f16 (FS merge_tfm_encoder.py:356-394; LS
 * merge_retnet_layer.py:301-306), with q, k, v kept in f32 registers.  Rows are (b*C + c)*Tp + t.  Supported where
 * eend_spk_stream_ok(C, Tp) != 0 (1 <= C <= 12, Tp a multiple of 64 / 32 / 16 for C <= 3 / 6 / 12); other shapes return EEND_EINVAL and
 * the caller uses the two-launch path.  eend_spk_stream_pack_f16 re-orders Wo1 [256][256] and W_in [768][256] (both f16) into the stream
 * (eend_spk_stream_elems() f16 elements).  x_f16 may be res_f16 and O_f16 may be A (lda == 256): rows are read before written. */
int eend_spk_stream_elems(void);
int eend_spk_stream_ok(int C, int Tp);
int eend_spk_stream_pack_f16(const void* Wo, const void* W_in, void* stream_out, void* stream);
int eend_attnout_spk_stream_f16(const void* A, int lda, const void* wstream, const float* bo, const void* res_f16,
                                const float* g1, const float* be1, float eps1, void* x_f16, const float* b_in, void* O_f16,
                                int B, int C, int Tp, float scale, void* stream);
/* ... with an f32 residual stream (round 5; LS-EEND's decoder, merge_retnet_layer.py:301-306 behind the retention's out-projection: replaces
 * eend_linear_res_ln_f16 + eend_spk_qkv_attn_f16 there): res_f32 rows in, x1 rows out as f32 (x_f32 may be res_f32), no f16 copy of x1.
 * 16-byte aligned f32 buffers; same shapes and weight stream as above. */
int eend_attnout_spk_stream_res32_f16(const void* A, int lda, const void* wstream, const float* bo, const float* res_f32,
                                      const float* g1, const float* be1, float eps1, float* x_f32, const float* b_in, void* O_f16,
                                      int B, int C, int Tp, float scale, void* stream);
/* The whole FS decoder layer behind the time-axis attention in one launch on one packed weight stream (dec_stream.hip):
 *   x1  = LayerNorm11(A Wo1^T + bo1 + res),   O = MHA over the C slots of (x1 W_in^T + b_in),
 *   x   = LayerNorm21(O Wo2^T + bo2 + x1),    out = LayerNorm22(ReLU(x W1^T + b1) W2^T + b2 + x)
 * i.e. eend_attnout_spk_stream_f16 followed by eend_attnout_ffn_stream_f16 with x1 and O kept on chip (x1 rounded to f16 as there; the
 * Wo2 sum runs in another order, so rows may differ from the pair's in the last f16 bit).  f16 rows (b*C + c)*Tp + t of 256 features,
 * out_f16 may be res_f16.  Supported where eend_dec_stream_ok(C, Tp) != 0 and F is a multiple of 64
 * in [64, 2048]; other shapes return EEND_EINVAL before any launch.  eend_dec_stream_ok admits C = 3 and C = 6 only (the tilings whose
 * instantiations keep inside the register file; other slot counts use the two launches).  eend_dec_stream_pack_f16 re-orders Wo1, W_in [768][256], Wo2,
 * W1 [F][256] and W2 [256][F] (f16) into the stream (eend_dec_stream_elems(F) f16 elements; 0 for an unsupported F). */
int eend_dec_stream_elems(int F);
int eend_dec_stream_ok(int C, int Tp);
int eend_dec_stream_pack_f16(const void* Wo1, const void* W_in, const void* Wo2, const void* W1, const void* W2, void* stream_out, int F,
                             void* stream);
int eend_attnout_spk_ffn_stream_f16(const void* A, int lda, const void* wstream, const float* bo1, const void* res_f16, const float* g11,
                                    const float* be11, float eps11, const float* b_in, const float* bo2, const float* g21, const float* be21,
                                    float eps21, const float* b1, const float* b2, const float* g22, const float* be22, float eps22,
                                    void* out_f16, int B, int C, int Tp, int F, float scale, void* stream);


/* Embedding-consistency loss (FS model :46-57; LS model :92-113): mean over (b,i,j) of
 * (cos(emb_i, emb_j) - cos(label_i, label_j))^2 with the reference's "+1e-6" denominators, without
 * materialising the (B,T,T) maps.  emb f32 [B][Tp][D] (rows >= T ignored), labels f32 [B][T][C] zero-padded
 * (C <= 16), partial_ws f32 [B * ceil(T/64)^2] scratch, out f32 [1].  lens (device int [B]) may be null; when
 * given, embeddings of frames >= lens[b] count as zero (the LS model's length mask, :100).  inv_count > 0
 * replaces the default 1/(B*T*T) normalisation (LS: 1/sum(len^2)).  Exact-fp32 MFMA; deterministic. */
int eend_emb_consistency_f32(const float* emb, const float* labels, const int* lens, float inv_count,
                             float* partial_ws, float* out, int B, int T, int Tp, int D, int C, void* stream);

/* ---- output-side post-processing (FS-EEND/train/utils/make_rttm.py:10-28, train/utils/loss.py:198-236;
 * the LS-EEND copies are identical).  Bit exact against the reference.  ---- */

/* pred f32 [T][ld] (S <= ld columns used; probabilities) -> act u8 [T][S]: (pred > threshold), then the
 * zero-padded median of `median` (odd) frames along time, i.e. scipy.signal.medfilt(x, (median, 1)). */
int eend_activity_median_u8(const float* pred, int ld, int T, int S, float threshold, int median,
                            unsigned char* act, void* stream);

/* act u8 [T][S] -> per speaker the increasing frame indices (0..T) at which the zero-padded track changes:
 * changes i32 [S][cap] (even entries = segment starts, odd = ends; entries beyond cap are dropped),
 * counts i32 [S] (number found, may exceed cap). */
int eend_activity_segments_i32(const unsigned char* act, int T, int S, int* changes, int* counts, int cap,
                               void* stream);

/* Live segments for many streams ("slots"; fs-eend_amd/live_rttm.py, additive to ABI version 5): the incremental form of
 * eend_activity_median_u8 + eend_activity_segments_i32.  One wave per entry e < n advances slot desc[2e + 1] by counts[e] rows
 * (device int32; <= 0: none) of a row-major f32 matrix starting at address desc[2e] (desc i64 [n][2], row stride ld floats),
 * columns col0 .. col0 + ntracks - 1 (1 <= ntracks <= 64, ld >= col0 + ntracks).  Decision: x > threshold with is_prob, else
 * 1 / (1 + expf(-x)) > threshold (NaN inactive); then the zero-padded median of `median` (odd, 1..63) frames, whose decision of
 * frame u is final once frame u + median / 2 has arrived.  ends (device int32 [n], may be NULL): != 0 ends the stream after its
 * rows -- the last median / 2 decisions are finalised with zeros past the end and open segments close at the frame count.
 * State: hist u64 [slots][64] (last median - 1 raw decisions per track), open i32 [slots][64] (start of the open segment, -1:
 * none), box i32 [slots][4 + 3 cap] = {frames, count, overflow, 0} then a ring of cap closed segments {track, start, end (exclusive)},
 * appended by end frame, then track; a full ring sets overflow and drops the segment.  frames == 0 marks an empty stream whose
 * hist / open words are not read; the host zeroes {frames, count, overflow} to start a stream and {count, overflow} after reading
 * the ring.  A slot may appear in at most one entry per call. */
int eend_segtrack_feed_f32(const long* desc, const int* counts, const int* ends, int n, int ld, int col0, int ntracks, float threshold,
                           int median, int is_prob, unsigned long long* hist, int* open, int* box, int slots, int cap, void* stream);

/* External speech-activity mask, whole file (LS-EEND/sad_post_process.py:23-33; additive to ABI version 5).  pred f32 [T][ld]
 * (S <= ld columns used), sad u8 [T] (non-zero: speech) -> out f32 [T][S] of 0 / 1: out[t][s] = pred[t][s] > threshold where
 * sad[t] is set and 0 elsewhere; a speech row with no column above the threshold gets a 1 at its largest value (the lowest
 * column on ties, as torch.argmax; -inf and 0 are ordinary values).  NaN is never above the threshold and never the largest; a
 * speech row of NaN only stays 0.  eend_activity_median_u8(out, S, T, S, 0.5f, median, ...) then filters it as usual. */
int eend_sad_fuse_f32(const float* pred, int ld, int T, int S, float threshold, const unsigned char* sad, float* out, void* stream);

/* eend_segtrack_feed_f32 behind an external speech-activity mask (additive to ABI version 5): the same arguments and state, plus
 * sad_desc i64 [n]: entry e's address of counts[e] u8 flags, one per row it brings (never read when counts[e] <= 0).  The raw
 * decision of a row is gated as eend_sad_fuse_f32 gates it, over the tracked columns col0 .. col0 + ntracks - 1 only; without
 * is_prob the largest value is taken over the raw logits.  The median, the segments and the end of a stream are unchanged, so a
 * stream's segments are those of eend_sad_fuse_f32 + eend_activity_median_u8 + eend_activity_segments_i32 over its rows. */
int eend_segtrack_feed_sad_f32(const long* desc, const int* counts, const int* ends, const long* sad_desc, int n, int ld, int col0,
                               int ntracks, float threshold, int median, int is_prob, unsigned long long* hist, int* open, int* box,
                               int slots, int cap, void* stream);

/* Frame-level DER counters of pre-activations pred f32 [T][ldp] against 0/1 labels f32 [T][ldl], C columns,
 * label_delay as in the reference: counters u64 [8] = speech_scored, speech_miss, speech_falarm,
 * speaker_scored, speaker_miss, speaker_falarm, speaker_error, #(label == decision).  Zeroed by the call. */
int eend_der_counters_u64(const float* pred, int ldp, const float* label, int ldl, int T, int C, int label_delay,
                          unsigned long long* counters, void* stream);

/* Collar DER with the optimal speaker mapping, as the papers report it (LS-EEND/metrics.py:41-108: pyannote's
 * DiarizationErrorRate(collar=50) over the label runs and the thresholded, median-filtered predictions; additive to ABI
 * version 5).  A ragged batch of B recordings (1 <= B <= 65535), rows concatenated: recording b has the reference rows
 * ref_off[b] .. ref_off[b + 1] - 1 of ref u8 [.][Cr] (label rate) and the hypothesis rows hyp_off[b] .. hyp_off[b + 1] - 1 of
 * hyp u8 [.][Ch] (model rate); the i32 [B + 1] offsets live on the device and do not decrease; non-zero is active; Cr and Ch are
 * independent, each in 1 .. 16.  Hypothesis frame k covers the reference frames [k * subsampling, (k + 1) * subsampling).  With
 * Tr and Th the two row counts, T = max(Tr, Th * subsampling); a side is zero beyond its own end, an empty side is legal, and
 * everything is counted in reference frames.
 *   1. Collar: half_collar = collar / 2 for pyannote's collar (the total width centred on a boundary).  Reference speaker s
 *      has a boundary at b in 0 .. Tr where ref[b - 1][s] != ref[b][s] (zeros outside [0, Tr), so a speaker active in frame 0 or
 *      Tr - 1 has one at 0 or Tr).  Frame t is removed iff some speaker has a boundary b with t - h < b <= t + h; the collar of
 *      the boundary at Tr reaches into a hypothesis-only tail.  Collars come from the reference only.  On the frame grid this is
 *      pyannote's interval arithmetic (collars [b - collar / 2, b + collar / 2) taken out of the union extent).
 *   2. skip_overlap != 0: frames with two or more active reference speakers are removed as well.
 *   3. cooc[i][j] = kept frames in which reference speaker i and hypothesis speaker j are both active.
 *   4. Mapping hypothesis j -> reference i, one-to-one and partial, maximising the sum of cooc; pairs with cooc = 0 are not
 *      mapped.  Where several mappings are optimal any one of them is returned; the counters do not depend on the choice.
 *   5. Per kept frame with nr reference and nh hypothesis speakers: total += nr, miss += max(0, nr - nh), false alarm +=
 *      max(0, nh - nr), correct += mapped pairs active on both sides, confusion += min(nr, nh) - those.  Summed over the
 *      frames, correct is the value of the optimal mapping, so one pass over the frames and one assignment do it.
 *      DER = (miss + false alarm + confusion) / total.
 * counters u64 [B][8] = total, miss, false alarm, confusion, correct, frames kept, frames removed within [0, T) (by a collar or
 * as overlap), sum of min(nr, nh); cooc u64 [B][16][16] (rows and columns beyond Cr and Ch are 0); mapping i32 [B][16],
 * hypothesis -> reference, -1 = unmapped.  All three are written by the call: a clearing launch, one pass over the rows (workgroups
 * walk tiles of reference frames, at most 512 tile groups per recording, 64-bit integer atomics only, so every run gives the
 * same bits) and one assignment launch; nothing is allocated and the host is not waited for.  EEND_EINVAL: a NULL pointer, Cr
 * or Ch outside 1 .. 16, B outside 1 .. 65535, subsampling < 1, half_collar < 0 or above the cap eend_collar_der_limits reports.
 * A recording with T > 2^31 - 2^16, or with decreasing offsets, is out of scope: it is not read, its counters are all ~0 and its
 * mapping is -1.  One quirk of the reference's script is not reproduced: there a second speaker with the very same run (s, e)
 * overwrites the first (`reference[Segment(s, e)] = str(spkid)`); here both count. */
int eend_collar_der_u64(const unsigned char* ref, const int* ref_off, int Cr, const unsigned char* hyp, const int* hyp_off, int Ch, int B,
                        int subsampling, int half_collar, int skip_overlap, unsigned long long* counters, unsigned long long* cooc,
                        int* mapping, void* stream);

/* The reference frames per tile of eend_collar_der_u64's pass and the largest half_collar it takes (host arithmetic only). */
int eend_collar_der_limits(int* tile, int* max_half_collar);

/* Collar DER over a grid of operating points in one pass over the rows: what a development set is tuned with (the reference's
 * scoring scripts take --thredshold and --median, LS-EEND/metrics.py and sad_post_process.py; additive to ABI version 5).  The
 * grid is n_thresholds x n_medians, G = n_thresholds * n_medians points, point g = i_threshold * n_medians + i_median
 * (threshold-major).  For every point g and recording b the results are exactly those of eend_collar_der_u64 over the activity
 * that eend_sad_fuse_f32 (with sad) and eend_activity_median_u8 make of the posteriors at thresholds[i_threshold] and
 * medians[i_median].
 *   Inputs, all in device memory.  The reference as for eend_collar_der_u64: ref u8 [.][Cr], ref_off i32 [B + 1].  The hypothesis
 * side as posteriors, packed the same way: pred f32 [.][Ch] (4-byte aligned; rows are dense, so a row start has no other
 * alignment when Ch is odd), pred_off i32 [B + 1]; Cr and Ch independent, each in 1 .. 16; 1 <= B <= 65535.  sad u8 [.], one flag per
 * posterior row under the same offsets (non-zero: speech), or NULL for no mask.  thresholds f32 [n_thresholds] and medians i32
 * [n_medians] are read by the kernels, not by the host, so the call copies nothing and can be captured in a graph; thresholds
 * may come in any order and may repeat (equal thresholds give equal results).
 *   Per point.  1. The decision of a value p is p > threshold, strict: NaN is never active, +-inf are ordinary values (a NaN
 * threshold makes nobody active).  2. With sad, a decision stands only in a speech row, and a speech row with no decision at
 * this threshold gets its largest non-NaN value (the lowest column on ties; the winner does not depend on the threshold), as
 * eend_sad_fuse_f32 states it; a speech row of NaN only stays 0.  3. The median of k (odd) along time is 1 iff at least k / 2 +
 * 1 of the k decisions are 1; the window is centred and sees zeros beyond the recording's own first and last row (scipy's
 * medfilt), never a neighbour's rows in the packed buffer.  It comes after the mask, so it may bridge a short non-speech gap;
 * k = 1 is no filter.  4. The result is scored against the reference as eend_collar_der_u64 states it: T = max(Tr, Th *
 * subsampling), a side is zero beyond its own end, half_collar, skip_overlap, the co-occurrence counts over the kept frames, the
 * mapping and the counters.  total, frames kept and frames removed come from the reference alone and are equal for all g.
 *   Outputs: counters u64 [G][B][8], cooc u64 [G][B][16][16], mapping i32 [G][B][16], slots and meaning as for eend_collar_der_u64;
 * all three are written by the call.  totals u64 [G][8] (may be NULL) belongs to the caller and is not cleared: the eight
 * counters of every scored (g, b) are added to row g with 64-bit integer atomics, so a development set larger than one batch
 * accumulates on the device in any order.  Three launches (clear, one pass in which the reference work of a tile is done once and
 * only the co-occurrence counts differ per point, the assignment of eend_collar_der_u64 on G * B matrices); integer atomics
 * only, so every run gives the same bits; nothing is allocated and the host is not waited for.
 *   EEND_EINVAL: a NULL pointer other than sad and totals, pred not 4-byte aligned, n_thresholds outside 1 .. 16, n_medians
 * outside 1 .. 4, G > 32 (eend_der_sweep_limits reports these), and the domain of eend_collar_der_u64 for Cr, Ch, B, subsampling and
 * half_collar.  A median must be odd and in 1 .. 127; the host cannot see the values, so a point whose median is not is not
 * scored: its counters are all ~0 and its mapping is -1 for every recording, and it adds nothing to totals; the other points
 * are unaffected.  A recording out of the scope of eend_collar_der_u64 is marked in the same way at every point. */
int eend_collar_der_sweep_u64(const unsigned char* ref, const int* ref_off, int Cr, const float* pred, const int* pred_off, int Ch,
                              const unsigned char* sad, int B, const float* thresholds, int n_thresholds, const int* medians,
                              int n_medians, int subsampling, int half_collar, int skip_overlap, unsigned long long* counters,
                              unsigned long long* cooc, int* mapping, unsigned long long* totals, void* stream);

/* The grid limits of eend_collar_der_sweep_u64: thresholds, medians and points per call, and the largest median (host arithmetic
 * only); the speaker, frame and collar limits are those of eend_collar_der_u64. */
int eend_der_sweep_limits(int* max_thresholds, int* max_medians, int* max_points, int* max_median);

/* eend_collar_der_u64 with scoring regions (the UEM files of AMI and DIHARD: pyannote's metric(reference, hypothesis, uem=uem))
 * and with the marginal times the Jaccard error rate needs; additive to ABI version 5.  Everything eend_collar_der_u64 states
 * holds; what is new, in reference frames:
 *   Regions.  uem i32 [.][2] (8-byte aligned) holds half-open intervals [s, e), 0 <= s < e, recording after recording; recording
 * b has the intervals uem_off[b] .. uem_off[b + 1] - 1 (uem_off i32 [B + 1], on the device, not decreasing), sorted and disjoint.
 * A frame t of [0, T) is kept iff (a) it lies in some interval of its recording, (b) no reference boundary b has
 * t - h < b <= t + h (rule 1 of eend_collar_der_u64), and (c) with skip_overlap it has fewer than two reference speakers.  The
 * boundaries are those of the uncropped reference: a boundary outside every interval still removes the frames of an interval
 * that its collar reaches, and an interval's edge is not a boundary.  This is the order of pyannote's uemify (the collars are
 * cut out of the UEM, then both sides are cropped to what is left), and it is why zeroing the activity outside the regions is
 * no substitute: that turns every edge into a boundary and still counts the frames outside as kept.  Intervals are clipped to
 * [0, T); a recording with no interval scores nothing (total = 0, frames kept = 0); one interval [0, e) with e >= T gives
 * the counters of eend_collar_der_u64.  frames kept + frames removed = T as before: the frames outside the regions are removed.
 * uem = uem_off = NULL: no regions anywhere, every frame of [0, T) passes (a); one of the two NULL is EEND_EINVAL.  The host
 * does not read the table: an interval with e <= s adds nothing, an unsorted table may lose intervals but is read within its
 * offsets only.
 *   Marginal times.  ref_time u64 [B][16]: the kept frames in which reference speaker i is active; hyp_time u64 [B][16]: the
 * kept reference frames under an active frame of hypothesis speaker j (a hypothesis frame counts once per kept reference
 * frame under it, as in cooc).  Entries beyond Cr and Ch are 0.
 *   counters, cooc and mapping are those of eend_collar_der_u64 over the kept frames.  Three launches (clear, one pass, the
 * assignment); per tile of reference frames the region term is built from the intervals that meet the tile (a binary search on
 * the starts, then a loop over as many intervals as there are) and is one more term of the bit that says a frame is kept;
 * integer atomics only, the same bits on every run, nothing allocated, the host not waited for. */
int eend_collar_der_regions_u64(const unsigned char* ref, const int* ref_off, int Cr, const unsigned char* hyp, const int* hyp_off, int Ch,
                                int B, int subsampling, int half_collar, int skip_overlap, const int* uem, const int* uem_off,
                                unsigned long long* counters, unsigned long long* cooc, int* mapping, unsigned long long* ref_time,
                                unsigned long long* hyp_time, void* stream);

/* eend_collar_der_sweep_u64 with the regions and marginal times of eend_collar_der_regions_u64: the kept frames are the same at
 * every point.  ref_time, hyp_time u64 [G][B][16]; ref_time is equal for all g.  Everything else as the two entries state. */
int eend_collar_der_sweep_regions_u64(const unsigned char* ref, const int* ref_off, int Cr, const float* pred, const int* pred_off, int Ch,
                                      const unsigned char* sad, int B, const float* thresholds, int n_thresholds, const int* medians,
                                      int n_medians, int subsampling, int half_collar, int skip_overlap, const int* uem,
                                      const int* uem_off, unsigned long long* counters, unsigned long long* cooc, int* mapping,
                                      unsigned long long* totals, unsigned long long* ref_time, unsigned long long* hyp_time,
                                      void* stream);

/* Jaccard error rate (DIHARD's second metric) from the outputs of the two entries above, n matrices (B, or G * B of the sweep):
 * cooc u64 [n][16][16], ref_time and hyp_time u64 [n][16]; Cr, Ch in 1 .. 16 as there.  All counts are over the kept frames, so
 * the usual figure is scored with half_collar = 0.  Reference speaker i is a speaker of the recording iff ref_time[i] > 0,
 * hypothesis speaker j iff hyp_time[j] > 0.  For a pair of both, inter = cooc[i][j], union = ref_time[i] + hyp_time[j] - inter,
 * cost = 1 - inter / union in float64.  The pairing is the one-to-one assignment of minimal total cost (not the mapping of the
 * DER, which maximises the overlap); a reference speaker left alone costs 1, and a pair with inter = 0, which costs the same,
 * is reported as unpaired.  Where several pairings are optimal any one is returned.
 *   Outputs: pairing i32 [n][16], reference -> hypothesis, -1 = unpaired or no such speaker; speakers u64 [n][16][3] = ref_time,
 * the paired speaker's hyp_time or 0, inter.  The caller forms the ratios: a speaker's error is (union - inter) / union (1 when
 * unpaired), a recording's the mean over its reference speakers.  One launch, one wave per matrix, the float64
 * shortest-augmenting-path solver on a cost matrix in LDS; the host is not waited for.  EEND_EINVAL: a NULL pointer, Cr or Ch
 * outside 1 .. 16, n < 1. */
int eend_jer_assign_f64(const unsigned long long* cooc, const unsigned long long* ref_time, const unsigned long long* hyp_time, int Cr,
                        int Ch, long n, int* pairing, unsigned long long* speakers, void* stream);

/* Reference segments -> the packed label rows eend_collar_der_u64 reads.  segments i32 [n_segments][4] (16-byte aligned) =
 * recording, speaker, start frame, end frame (half-open); ref_off i32 [B + 1] on the device, the rows of recording b being
 * ref_off[b] .. ref_off[b + 1] - 1 of rows u8 [n_rows][C] (16-byte aligned; n_rows >= ref_off[B], C in 1 .. 16).  All n_rows rows
 * are zeroed, then every frame of every segment gets a 1 in its speaker's column; frames outside the recording's rows, and
 * segments whose recording or speaker is outside the table, write nothing, and a segment with end <= start is empty.  Two
 * launches (clear, one workgroup per segment); overlapping segments store the same value, so the bytes do not depend on order. */
int eend_segments_raster_u8(const int* segments, long n_segments, const int* ref_off, int B, int C, unsigned char* rows, long n_rows,
                            void* stream);

/* ---- feature front-end ({LS,FS}-EEND/datasets/feature.py: stft :166-191, transform :43-131, splice :141-163,
 * subsample :133-138, extract_fbank :324-336); fp32 throughout.  ---- */

/* STFT (Hann window of 200 samples zero-padded to n_fft = 256, hop 80) -> power -> 23 mel bands -> log10(max(.,1e-10)).
 * Frame t uses samples y[first + 80 t + k], k = 0..199 (the non-zero window taps), zero outside [0, len):
 * first = -100 reproduces librosa.stft(center=True, pad_mode="constant"); a host that pre-pads the signal
 * itself (e.g. reflect) passes the padded buffer and first = 28.  dft f32 [200][288]: windowed DFT table,
 * row k = w[k] * cos(2 pi (k+28) n / 256) in column n (n <= 128) and -w[k] * sin(..) in column 144 + n, zeros
 * elsewhere; melT f32 [132][32]: mel filterbank transposed (rows = bins, 129 used), zero padded.
 * out f32 [n_frames][23]. */
int eend_stft_logmel23_f32(const float* y, long len, long first, int n_frames, const float* dft, const float* melT,
                           float* out, void* stream);

/* Column-mean normalisation of Y f32 [T][F] into out: mode 1 = subtract the mean over all frames
 * (logmel23_mn), mode 2 = subtract the running mean of frames 0..t (logmel23_cummn).  fp64 running sums. */
int eend_feature_meannorm_f32(const float* Y, float* out, int T, int F, int mode, void* stream);

/* out f32 [ceil(T/sub)][F (2 ctx + 1)]: row j = frames j sub - ctx .. j sub + ctx of Y f32 [T][F] side by side,
 * zero outside [0, T) (splice + subsample). */
int eend_splice_subsample_f32(const float* Y, int T, int F, int ctx, int sub, float* out, void* stream);

/* Incremental front-end: many streams ("slots") fed audio in chunks of any size; the log-mel frames are those of
 * eend_stft_logmel23_f32 (first = -100) bit for bit, normalised (mode 0 = logmel23, 2 = logmel23_cummn with the fp64
 * running sum added in frame order), spliced (ctx 0..15) and subsampled (sub 1..16) as eend_splice_subsample_f32.
 * Per-slot device state: tail f32 [slots][200] (samples 80 f - 100 .. of the slot's next log-mel frame f), ring f32
 * [slots][32][23] (its last normalised frames that later splices read), sums f64 [slots][23].  desc i64 [n_desc][9], one
 * row per slot in the call: {device address of its new samples, samples received before / after, log-mel frames before /
 * after, first frame held in the ring before / after, row of that frame in Y, slot}.  stft_tiles i64 [n_stft][3]:
 * {desc row, first new log-mel frame, frames <= 64}; splice_tiles i64 [n_splice][4]: {desc row, first model frame,
 * frames <= 16, output row}.  Y f32 scratch [rows][23]: per slot its ring frames then its new frames; out f32
 * [rows][23 (2 ctx + 1)].  At most three launches; the host owns all counters (see fs-eend_amd/audio_stream.py). */
int eend_audio_feed_f32(const long* desc, int n_desc, const long* stft_tiles, int n_stft, const long* splice_tiles, int n_splice,
                        float* tail, float* ring, double* sums, float* Y, float* out, int mode, int ctx, int sub,
                        const float* dft, const float* melT, void* stream);

/* Labelled training batches from resident audio: what LS-EEND/datasets/diarization_dataset_on_the_fly.py:87-131 (__getitem__:
 * get_labeledSTFT -> transform -> splice -> subsample) and datasets/feature.py:255-322 (get_labeledSTFT) do per item on one CPU
 * core, for a whole batch of chunks in three launches.  corpus: the samples of every recording back to back, storage 0 = f32,
 * 1 = 16-bit PCM decoded as v / 32768 (what soundfile returns for such a file with dtype='float32').  A chunk is treated as a
 * file of its own: its log-mel frames are those of eend_stft_logmel23_f32 on corpus[off .. off + len) with first = -100, its
 * normalisation (mode 0 = logmel23, 1 = logmel23_mn, 2 = logmel23_cummn) that of eend_feature_meannorm_f32 with the fp64 sums
 * added in the same order, its rows those of eend_splice_subsample_f32: all three bit for bit.
 * desc i64 [n_chunks][8], one row per chunk: {off = index in corpus of its first sample, len = its samples (already clipped at
 * the end of the recording), n = its log-mel frames (1 + len / 80, minus one when len % 80 == 0), row of its first frame in Y,
 * start, end = the chunk in STFT frames of its recording as the dataset row names it (end not clipped), seg0, seg1 = its
 * recording's range of rows in segments}.  stft_tiles i64 [n_stft][3]: {desc row, first frame, frames <= 64}; splice_tiles i64
 * [n_splice][4]: {desc row, first model frame j, frames <= 16, output row}.  segments i32 [rows][3]: {start_frame, end_frame,
 * speaker index}, CSR by recording, frames rounded on the host (feature.py:305-308).  Label rule (feature.py:301-317) for a
 * chunk [start, end) of n frames: a = start_frame - start if start <= start_frame < end, b = end_frame - start if start <
 * end_frame <= end; a segment with neither is skipped (also one that covers the whole chunk); else frames [a or 0, min(b or n,
 * n)) of its speaker are 1.  Y, Yn f32 scratch [sum n][23] (Yn unused with mode 0); feats f32 [sum ceil(n / sub)][23 (2 ctx +
 * 1)], labels f32 [sum ceil(n / sub)][S_max] (0.0 / 1.0; columns of speakers without a segment stay 0), both fully written.
 * Stateless, stream-ordered, nothing allocated, the host not waited for; the descriptors are trusted (the host checks off + len
 * against the corpus, see fs-eend_amd/device_data.py).  EEND_EINVAL: a NULL pointer that is needed, storage outside 0 .. 1,
 * mode outside 0 .. 2, ctx outside 0 .. 64, sub outside 1 .. 4096, S_max outside 1 .. 64, n_chunks above 65535.  Limits: frame
 * size 200 and shift 80 at 8 kHz only; at most 2^31 - 1 frames and output rows per call; speaker-id targets (use_speaker_id),
 * frame shuffling and reflect padding are not covered. */
int eend_chunk_batch_f32(const void* corpus, int storage, const int* segments, const long* desc, int n_chunks,
                         const long* stft_tiles, int n_stft, const long* splice_tiles, int n_splice, float* Y, float* Yn,
                         float* feats, float* labels, int S_max, int mode, int ctx, int sub, const float* dft, const float* melT,
                         void* stream);

/* Audio ingest in front of eend_audio_feed_f32: many streams ("slots"), each fed raw audio at one sample rate and encoding in
 * chunks of any size, decoded and converted to f32 samples at 8 kHz.  encoding 0 = f32 (the value itself), 1 = 16-bit PCM
 * (v / 32768), 2 = G.711 mu-law, 3 = G.711 A-law (decode f32 [2][256]: the value of every mu-law, then every A-law byte).
 * With g = gcd(rate, 8000), L = 8000 / g, M = rate / g and a low-pass prototype h[-H..H] on the rate * L grid, output n of a
 * stream is  y[n] = sum_k h[n M - k L] x[k]  over k = ceil((n M - H) / L) .. floor((n M + H) / L), x zero outside the stream,
 * accumulated in f32 with fmaf from zero in ascending k: its bits do not depend on how the audio was cut.  table f32 [L][P],
 * P = 2 H / L + 1 <= 255: row (n M) mod L holds the taps of output n in that order, zero-padded (L = M = 1, H = 0, table {1}
 * decodes only).  Per-slot device state: hist f32 [slots][256], the decoded samples max(0, ceil((n M - H) / L)) .. received
 * - 1 that the slot's next output n still reads (fewer than P).  desc i64 [n_desc][8], one row per slot in the call: {device
 * address of its raw chunk, input samples received before / after, outputs made before / after, index in out of its first
 * new output, 1 if the stream ends with this call, slot}.  tiles i64 [n_tiles][3]: {desc row, first output, outputs <= 256}.
 * out f32: the new outputs of every slot, packed.  Two launches: the tiles (one workgroup each, the input span staged in LDS),
 * then the new history rows (one workgroup per desc row; a later launch because the tiles read the rows it overwrites).
 * The host owns all counters (see fs-eend_amd/audio_ingest.py).  EEND_EINVAL: a NULL pointer that is needed, M < L (a rate
 * below 8 kHz), P outside 1 .. 255 or unlike 2 H / L + 1, an unknown encoding, or a tile span 255 M / L + P + 2 above 2048. */
int eend_audio_ingest(const long* desc, int n_desc, const long* tiles, int n_tiles, float* hist, const float* table,
                      const float* decode, int L, int M, int H, int P, int encoding, float* out, void* stream);

/* Simulated training mixtures from resident dry sources: single-speaker utterances laid out with silences, convolved with a room
 * impulse response per speaker, summed, with noise added at a chosen SNR (the `data_simu_*` sets both shipped configs train on;
 * the reference takes them as files made elsewhere).  All audio is 8 kHz; all inputs are assumed finite.  Pools: utts and noises
 * hold their waves back to back, storage 0 = f32, 1 = 16-bit PCM decoded as v / 32768; rirs f32.
 *
 * Arithmetic contract.  Mixture m has N samples and S <= 64 tracks.  Track s has a gain g (f32), an impulse response h[0 .. K),
 * K <= 8192, or none, and placements (start >= 0, source, len), sorted by start and disjoint, len already clipped to N - start.
 *   dry track   d_s[t] = the source sample where a placement covers t, 0 elsewhere and for t < 0;
 *   taps        a_s[k] = f32(g h[k]), one f32 multiply; without a response a_s = {g}, K = 1;
 *   wet mix     y[t] = sum_s sum_k a_s[k] d_s[t - k] for 0 <= t < N (the tail past N is dropped), in f32 with one accumulator per
 *               output: acc = fmaf(a_s[k], d_s[t - k], acc) from +0, tracks ascending, taps ascending.  Zero products are added
 *               or left out freely (before and after the taps, and whole spans that meet no placement): they leave acc as it
 *               is, so an output's value depends on its own taps and samples only, not on its tile, on the other mixtures of
 *               the call or on the silences skipped (only the sign of a zero that arose from a product underflowing to -0 can
 *               differ);
 *   noise       Ps = sum_t y[t]^2 and Pn = sum_t n[(o + t) mod L]^2 over t < N in float64, both in one fixed order (per tile of
 *               2048 samples 256 running sums of stride 256, then a binary tree; per mixture the same over its tiles);
 *               scale = f32(sqrt(c Ps / Pn)) in float64 with c = 10^(-snr_db / 10) from the host, 0 when there is no noise
 *               (L = 0) or Pn = 0 or Ps = 0;  out[t] = fmaf(scale, n[(o + t) mod L], y[t]), and y[t] itself when scale = 0;
 *   storage     out_storage 0 stores out as f32; 1 stores rint(out 32768), half to even, clamped to [-32768, 32767], and
 *               clipped[m] counts the clamped samples.
 * Tables, i64, trusted (fs-eend_amd/simulate.py `plan` builds and checks them): mix [n_mix][10] = {N, index of its first sample in
 * Y and out, first track row, tracks, index in noises of its noise, L (0 = none), o >= 0, the bits of the double c, first tile
 * row, tiles}; tracks [.][5] = {index in rirs of h or -1, K, the bits of the f32 g, first placement row, placements}; places
 * [.][3] = {start, index in utts of the utterance's first sample, len}; tiles [n_tiles][2] = {mixture, first output}, the tiles
 * of a mixture consecutive and 2048 outputs apart.  Y f32 scratch [sum N]: the wet mix; part f64 scratch [n_tiles][2]; out f32
 * or s16 [sum N]; Ps, Pn f64 [n_mix], scale f32 [n_mix], clipped i32 [n_mix].  Four launches whatever the call holds: the FIR
 * on v_mfma_f32_16x16x4_f32 (a Toeplitz product, csrc/simulate.hip), the tile sums, the scales, the store.  Stateless,
 * stream-ordered, nothing allocated, the host not waited for.  EEND_EINVAL: a NULL pointer (pass any valid address for an empty
 * pool), a storage outside 0 .. 1, n_mix above 65535, fewer tiles than mixtures. */
int eend_sim_mix_f32(const void* utts, int utt_storage, const float* rirs, const void* noises, int noise_storage, const long* mix,
                     int n_mix, const long* tracks, const long* places, const long* tiles, int n_tiles, float* Y, double* part,
                     void* out, int out_storage, double* Ps, double* Pn, float* scale, int* clipped, void* stream);

/* The layout constants of eend_sim_mix_f32: outputs per tile, FIR steps per tap slice, the most taps of a track (host arithmetic
 * only). */
int eend_sim_limits(int* tile, int* slice, int* max_taps);

/* Room impulse responses of shoebox rooms by the image method: the `rirs` pool of eend_sim_mix_f32 made on the device.  8 kHz
 * throughout; all inputs are finite doubles from the host.  One row is one response of K taps, 1 <= K <= 8192.
 *
 * Arithmetic contract.  A row has a room L = (Lx, Ly, Lz), a source s and a receiver r strictly inside it, six wall reflection
 * coefficients in [0, 1] (x0 the wall at x = 0, x1 the wall at x = Lx, then y0, y1, z0, z1), q = 8000 / c samples per metre, a
 * scale g.  Image (n, l, m, u, v, w), n, l, m integer, u, v, w in {0, 1}:
 *   offset      p = (((1 - 2u) sx + 2n Lx) - rx, ((1 - 2v) sy + 2l Ly) - ry, ((1 - 2w) sz + 2m Lz) - rz)
 *   distance    d = sqrt(px px + (py py + pz pz)),  delay  tau = q d  samples,  tau = kc + f with kc = rint(tau), |f| <= 1/2
 *   amplitude   A = g x0^|n-u| x1^|n| y0^|l-v| y1^|l| z0^|m-w| z1^|m| / d,  0^0 = 1
 *               all of this in IEEE float64, the offset, distance and delay operation by operation as written, without fused
 *               multiply-adds: kc and f are then the same bits on any machine;
 *   interpolator  w(x) = sinc(x) (1 + cos(2 pi x / W)) / 2 for |x| < W / 2, else 0; W = 64 samples; sinc(0) = 1.  At tap k the
 *               image stands at x = j - f, j = k - kc, and is evaluated in the split form, which keeps f where x would lose it:
 *                 sin(pi x) = -(-1)^j sin(pi f),    (1 + cos(2 pi x / W)) / 2 = sin^2(pi y / W),  y = W / 2 - |x| = (W / 2 - |j|) +- f,
 *               live exactly when y > 0: |j| < 32, or j = 32 with f > 0, or j = -32 with f < 0;
 *   response    h[k] = sum A_i w(k - tau_i), k = 0 .. K - 1, over every image whose window meets [0, K): the image set is defined
 *               by time, not by a reflection order; what falls at k < 0 or k >= K is dropped; images with A = 0 are skipped.
 *               Output f32.  Against the float64 sum every tap satisfies |h[k] - ref[k]| <= (n_k + 16) 2^-24 S_k, n_k the number
 *               of images with a non-zero term at k and S_k the sum of the terms' magnitudes: an f32 sum of n_k terms in any
 *               order plus 16 units for one term (tests/room_ref.py is the float64 restatement).
 *   bits        a response's bits depend on its own row only: not on the other rows, their order or the run.  No atomics.
 * rooms i64 [n_rows][20], trusted (fs-eend_amd/rooms.py `plan_rooms` builds and checks them): words 0 .. 16 the bits of the doubles
 * Lx, Ly, Lz, sx, sy, sz, rx, ry, rz, x0, x1, y0, y1, z0, z1, q, g; 17 = K; 18 = index in out of the row's first tap; 19 = the
 * row's tiles.  tiles i64 [n_tiles][2] = {row, first tap}, a multiple of 64, in any order (the host puts the tiles with the most
 * images first).  out f32: every tap k < K of every tile is written once.  One launch, one workgroup per tile (csrc/room.hip);
 * stateless, stream-ordered, nothing allocated, the host not waited for.  A row must keep 2 (2 N + 1) <= 1022 on every axis,
 * N = floor((K + 31) / (2 q L)) + 1 (eend_room_limits); the kernel clamps N there and would lose images beyond it.
 * EEND_EINVAL: a NULL pointer, n_rows above 65535, fewer tiles than rows. */
int eend_room_rir_f32(const long* rooms, int n_rows, const long* tiles, int n_tiles, float* out, void* stream);

/* The layout constants of eend_room_rir_f32: taps per tile, W, the most rows of a call, the most table entries of an axis (host
 * arithmetic only). */
int eend_room_limits(int* tile, int* window, int* max_rows, int* max_axis);

/* ---- offline EEND-EDA attractor path (FS-EEND/nnet/model/offl_tfm_enc_lstm_enc_dec.py): inference ---- */

/* Whether eend_lstm_f32 takes the shape: hidden == 256, T >= 1, B >= 1 (host arithmetic only). */
int eend_lstm_ok(int B, int T, int hidden);

/* Single-layer, unidirectional LSTM recurrence of B independent sequences over T steps, PyTorch gate order (i, f, g, o), hidden
 * size 256: the nn.LSTM calls of EncoderDecoderAttractor.eda_forward (offl_tfm_enc_lstm_enc_dec.py:82-83, :88, :91) without their
 * input GEMM.
 *   G      f32 [B][g_rows][1024], g_rows >= T: the input pre-activations x W_ih^T + b_ih + b_hh, computed beforehand (any f32 linear
 *          entry, e.g. eend_linear_step_f32).  Step t reads row order[t] of its sequence: the shuffle of model :62-65 is an index,
 *          nothing is gathered or copied.  NULL = zero input (the decoder's zeros of :104): the pre-activation is `bias` alone.
 *   order  i32 [T], a permutation of 0 .. T-1 shared by the batch; NULL = identity.  Validated by the host; the kernel clamps an
 *          entry into [0, T) so that it never reads outside G.
 *   bias   f32 [1024] = b_ih + b_hh, read only when G is NULL.
 *   W_hh   f32 [1024][256] as nn.LSTM stores weight_hh_l0.
 *   h0, c0 f32 [B][256], both or neither; NULL = zeros.
 *   hT, cT f32 [B][256]: the state after step T-1.  h_all (optional) f32 [B][T][256]: h after every step, in step order.
 *   step   z = G[order[t]] + W_hh h;  c = sigmoid(z_f) c + sigmoid(z_i) tanh(z_g);  h = sigmoid(z_o) tanh(c).
 * h, c and every sum are f32; the gate functions are finite for every finite pre-activation.  A sequence's bits depend on its own
 * inputs only (not on its batch mates or the run).  One workgroup per sequence from the first step to the last, no workgroup waits
 * on another; W_hh is re-read from L2 every step (csrc/lstm.hip).  Stateless, stream-ordered, nothing allocated, the host not waited
 * for.  EEND_EINVAL: hidden != 256, T < 1, B < 1, g_rows < T, a NULL W_hh / hT / cT, G and bias both NULL, one of h0 / c0 alone. */
int eend_lstm_f32(const float* G, int g_rows, const int* order, const float* bias, const float* W_hh, const float* h0, const float* c0,
                  float* hT, float* cT, float* h_all, int B, int T, int hidden, void* stream);

/* eend_lstm_f32 with one frame order per sequence: order i32 [B][T], row b a permutation of 0 .. T-1 read by sequence b alone, so
 * that sequences of different streams share a launch and none depends on its batch mates.  The same kernel as eend_lstm_f32 (which
 * passes an order stride of 0); with B equal rows the two entries give the same bits.  G must be given (an order over a zero input
 * means nothing).  EEND_EINVAL: as eend_lstm_f32, and a NULL G or order. */
int eend_lstm_orders_f32(const float* G, int g_rows, const int* order, const float* W_hh, const float* h0, const float* c0, float* hT,
                         float* cT, float* h_all, int B, int T, int hidden, void* stream);

/* probs[b][c] = sigmoid(attractors[b][c] . w + bias[0]) (model :106, `counter` is Linear(256, 1)) and, where count is given,
 * count[b] = the first c with probs[b][c] < th, C if there is none: the speaker count of model :72-73 per sequence.
 * attractors f32 [B][C][256], w f32 [256], bias f32 [1], probs f32 [B][C], count i32 [B] or NULL; 1 <= C <= 16. */
int eend_eda_count_f32(const float* attractors, const float* w, const float* bias, float th, float* probs, int* count, int B, int C,
                       void* stream);

/* logits[b][t][c] = emb[b][t] . attractors[b][c] (the torch.bmm of model :66) over all C columns.  emb f32 [B][emb_rows][256] with
 * emb_rows >= T (a slab: rows t >= T are never read), attractors f32 [B][C][256], logits f32 [B][T][C]; 1 <= C <= 16, B <= 65535. */
int eend_eda_head_f32(const float* emb, int emb_rows, const float* attractors, float* logits, int B, int T, int C, void* stream);

/* ---- the differentiable attractor path: EncoderDecoderAttractor.forward (model :109-127) and its backward.  The encoder backward
 * and the Lightning module are not built. ---- */

/* eend_lstm_f32 / eend_lstm_orders_f32 (the same kernel body; hT, cT and h_all have the same bits) which also keeps what the backward
 * reads.  order_stride: 0 = order i32 [T] for the batch, T = order i32 [B][T], one per sequence.  Each of the three may be NULL:
 *   gates   f32 [B][T][1024]  sigmoid(z_i), sigmoid(z_f), tanh(z_g), sigmoid(z_o) of every step, in step order
 *   c_all   f32 [B][T][256]   the cell state after every step, in step order
 *   h_prev  f32 [B][hp_rows][256], hp_rows >= T: the hidden state that enters step t, written at row order[t] (row t without an
 *           order): the row of dG the step's gradient goes to.  hp_rows is its own count, so that the backward's operands can be
 *           T rows tall where G is a taller slab.  Rows no step reads are not written.
 * EEND_EINVAL: as eend_lstm_f32; an order with a NULL G; 0 < order_stride < T; h_prev with hp_rows < T. */
int eend_lstm_train_f32(const float* G, int g_rows, const int* order, int order_stride, const float* bias, const float* W_hh,
                        const float* h0, const float* c0, float* hT, float* cT, float* h_all, float* gates, float* c_all, float* h_prev,
                        int hp_rows, int B, int T, int hidden, void* stream);

/* Backpropagation through time of eend_lstm_train_f32, step T-1 down to 0, all f32, one workgroup per sequence.
 *   gates, c_all, order, order_stride as the forward wrote / read them; c0 f32 [B][256] the forward's c0 (NULL = zeros); W_hh.
 *   dh_all  f32 [B][T][256] or NULL: d loss / d h of every step (the decoder: every h is an attractor)
 *   dhT, dcT f32 [B][256] or NULL: d loss / d of the final state (the encoder, fed by the decoder's dh0 / dc0).  One of the three at least.
 *   dG      f32 [B][g_rows][1024]: step t's pre-activation gradients at row order[t] (row t without an order); other rows are not written
 *   dh0, dc0 f32 [B][256]: d loss / d of the initial state.
 *   step    dh = dh_all[t] + W_hh^T dz(t+1);  dc += dh o (1 - tanh^2 c_t);  dz_o = dh tanh(c_t) o (1 - o);  dz_i = dc g i (1 - i);
 *           dz_g = dc i (1 - g^2);  dz_f = dc c_{t-1} f (1 - f);  dc <- dc f.
 * The order of every sum is fixed by (gate row, wave): a sequence's bits depend neither on its batch mates nor on the run.
 * EEND_EINVAL: hidden != 256, T < 1, B < 1, g_rows < T, a NULL gates / c_all / W_hh / dG / dh0 / dc0, no upstream gradient,
 * order_stride != 0 with a NULL order or below T. */
int eend_lstm_bwd_f32(const float* gates, const float* c_all, const float* c0, const float* W_hh, const float* dh_all, const float* dhT,
                      const float* dcT, const int* order, int order_stride, float* dG, int g_rows, float* dh0, float* dc0, int B, int T,
                      int hidden, void* stream);

/* Bytes of workspace eend_wgrad_f32 needs for these sizes (with_bias: db is asked for); 0 where it refuses them. */
long eend_wgrad_f32_workspace_bytes(int N, int K, int with_bias);
/* dW[n][k] = sum_m dY[m][n] X[m][k] and, where db is given, db[n] = sum_m dY[m][n]; dY f32 [M][ldy], X f32 [M][ldx], dW f32 [N][K],
 * everything f32 on the exact-f32 MFMA (an m-ordered fmaf chain).  The rows are cut into a fixed number of slices (16, whatever the
 * device), whose partials go to ws and are summed in slice order: the bits are the same in every run.  Overwrites dW and db.
 * EEND_EINVAL: N or K not a multiple of 64, M < 1, ldy < N, ldx < K, a NULL dY / X / ws / dW, ws_bytes below the query. */
int eend_wgrad_f32(const float* dY, int ldy, const float* X, int ldx, long M, int N, int K, float* ws, long ws_bytes, float* dW, float* db,
                   void* stream);

/* The attractor-existence loss of model :121-123 and its gradients for d loss = 1.  With n_b = n_spk[b] (i32 [B], 0 <= n_b < C; the
 * kernel clamps into that range): z[b][c] = attractors[b][c] . w + bias for c <= n_b, labels [1] * n_b + [0],
 * loss[0] = mean over the sum_b (n_b + 1) elements of BCE-with-logits.  dattractors f32 [B][C][256] (zero rows for c > n_b), dw f32
 * [256], dbias f32 [1]: all three, or all three NULL for the loss alone.  ws: eend_eda_count_loss_workspace_bytes(B) bytes.  Sums
 * run in the order (c, then b).  1 <= C <= 16.  EEND_EINVAL: sizes, a NULL input / loss / ws, a short ws, some gradients only. */
long eend_eda_count_loss_workspace_bytes(int B);
int eend_eda_count_loss_f32(const float* attractors, const float* w, const float* bias, const int* n_spk, float* loss, float* dattractors,
                            float* dw, float* dbias, float* ws, long ws_bytes, int B, int C, void* stream);

/* Bytes of workspace eend_eda_head_bwd_f32 needs when dattractors is asked for; 0 for sizes it refuses. */
long eend_eda_head_bwd_workspace_bytes(int B, int T, int C);
/* Backward of eend_eda_head_f32: dattractors[b][c] = sum_t dlogits[b][t][c] emb[b][t] (partials of 64 frames, frames ascending,
 * summed in tile order) and demb[b][t] = sum_c dlogits[b][t][c] attractors[b][c].  dlogits f32 [B][T][C], emb f32 [B][emb_rows][256],
 * dattractors f32 [B][C][256] or NULL, demb f32 [B][T][256] or NULL (one of the two at least).  Sizes as eend_eda_head_f32. */
int eend_eda_head_bwd_f32(const float* dlogits, const float* emb, int emb_rows, const float* attractors, float* dattractors, float* demb,
                          float* ws, long ws_bytes, int B, int T, int C, void* stream);

/* ---- block-online EEND-EDA with a speaker-tracing buffer, STB (FS-EEND/train/tfm_STB.py:147-204; find_best_perm, cal_cor, upd_buf,
 * upd_buf_FIFO of train/utils/utils.py) ----
 *
 * Both entries read one descriptor of 12 64-bit words per sequence, desc i64 [B][12] in device memory:
 *   0 x_buf   f32 [L][F]   the stream's buffered feature rows (the current half of its ping-pong buffer); unread when L = 0
 *   1 L       buffered rows, 0 for a stream's first block
 *   2 x_i     f32 [n][F]   the new block's raw rows
 *   3 n       rows of the block; L + n = T, the T of the call
 *   4 y_buf   f32 [L][15]  the tracked posteriors of the buffered rows, zero beyond the tracked width
 *   5 x_buf'  f32 [min(T, buf_size)][F]   the OTHER half of the buffer, written; never the half of word 0
 *   6 y_buf'  f32 [min(T, buf_size)][15]  likewise
 *   7 width   i32 [1]      the tracked width S: read (ignored when L = 0), then overwritten with the new width
 *   8 y_i     f32 [n][15]  the emitted block, written
 *   9 k       the block index and 10 seed, the stream's 32-bit seed: the counters of the draw;  11 unused
 * A kernel forces L into [max(0, T - blk_size), min(buf_size, T - 1)] and takes n = T - L, so that a wrong descriptor cannot make
 * it leave buffers of the stated sizes.  Stateless, stream-ordered, nothing allocated, the host not waited for.
 * EEND_EINVAL (before any launch): a NULL pointer, B < 1, T < 1, F < 1 or F > 512, blk_size < 1, blk_size > buf_size,
 * buf_size + blk_size > 4096, T > buf_size + blk_size, an unknown policy. */

/* out f32 [B][T][F]: rows [x_buf; x_i] of sequence b minus their column mean (tfm_STB.py:168, :177-178).  The column sums are
 * float64: thread r of 16 adds rows r, r + 16, .. in ascending order and the 16 partial sums are added in the order r = 0 .. 15;
 * out = (float)((double)x - sum / T).  A sequence's bits depend on its own rows only. */
int eend_stb_center_f32(const long* desc, float* out, int B, int T, int F, int buf_size, int blk_size, void* stream);

/* Everything of a block after the head, one workgroup per sequence.  logits f32 [B][T][15] (eend_eda_head_f32 on the centred rows),
 * count i32 [B] (eend_eda_count_f32, forced into 0 .. 15), xc f32 [B][T][F] the centred rows (eend_stb_center_f32; read for L = 0 only).
 *   p       = (float) sigmoid in float64 of logits[:, :c];  S' = max(S, c);  columns beyond c or S are zero
 *   L = 0   y_i = p, the buffer takes the centred rows and p, the width becomes c (tfm_STB.py:165-172)
 *   L > 0   corr[r][q] = cov / (sqrt(var_r) sqrt(var_q) + 1e-6) of tracked column r and predicted column q over the L buffer rows, two
 *           passes, float64 sums in ascending row order (cal_cor);  perm = the assignment of largest total correlation
 *           (csrc/assign.h): only its pairs of a tracked row r < S with a predicted column q < c are kept, the other rows take the
 *           columns left over in ascending order (padding rows and columns have correlation 0 with everything, so this is an
 *           optimum and the choice among equal ones is fixed);  y_i[:, r] = p[L:, perm[r]]
 *   buffer  T <= buf_size: all T rows of [x_buf; x_i] (raw) and [y_buf; y_i].  Otherwise buf_size of them in ascending time order:
 *           policy 1 (fifo) the last ones (upd_buf_FIFO); policy 0 (kld, upd_buf) p_t = y_t / sum_c y_t (0 where the sum is 0), zeros
 *           set to 1e-6, w_t = sum_c p log(p S') over the S' columns, negative set to 0, then 0 set to 1e-6 (w = 1 when S' = 0); the
 *           rows of the buf_size largest keys  key_t = w_t / -ln(u_t),  u_t = (h + 0.5) 2^-32,  h = mix(mix(mix(seed ^ 0x9E3779B9) + k) + t)
 *           in 32-bit arithmetic,  mix(x): x ^= x >> 16, x *= 0x85EBCA6B, x ^= x >> 13, x *= 0xC2B2AE35, x ^= x >> 16  (the
 *           exponential race: a draw of buf_size rows without replacement with probability proportional to w); on equal keys the
 *           lower t wins.  w and the keys are float64 from the f32 posteriors.
 * perm_out i32 [B][15] or NULL: perm (identity where nothing was assigned).  sel_out i32 [B][buf_size] or NULL: the kept rows' indices
 * into [x_buf; x_i], the first min(T, buf_size) entries of a row written. */
int eend_stb_track_f32(const float* logits, const int* count, const float* xc, const long* desc, int* perm_out, int* sel_out, int B,
                       int T, int F, int buf_size, int blk_size, int policy, void* stream);

/* ---- permutation-invariant label assignment (FS-EEND/train/utils/loss.py:257-327 batch_pit_n_speaker_loss;
 * LS-EEND/train/utils/loss.py:350-379 pit_loss_multispk) ---- */

/* cost f64 [B][C][C]: cost[b][i][j] = sum_t BCEwithLogits(y[b][t][i], labels[b][t][j]) over all T frames of
 * the padded batch (the reference pads both logits and labels with -1, pad_sequence); y, labels f32 [B][T][C],
 * C <= 16.  batch_pit's losses[b][i][s] is cost[b][i][(i+s) % C]; pit_loss_multispk's cost_mxs is cost itself. */
int eend_pit_cost_f64(const float* y, const float* labels, int B, int T, int C, double* cost, void* stream);

/* Optimal assignment on the leading nspk[b] x nspk[b] block of every cost matrix (shortest augmenting paths,
 * fp64; the remaining slots keep their place): perm i32 [B][C] = label column assigned to prediction i,
 * loss f64 [B] = mean over the C slots of the assigned costs (batch_pit's per-utterance minimum). */
int eend_pit_assign_i32(const double* cost, const int* nspk, int B, int C, int* perm, double* loss, void* stream);

/* q/k/v/g projections of MultiScaleRetention (LS-EEND/nnet/modules/retention.py:200-207) in the
 * layouts eend_retention_chunk_f16 consumes.  Wqkvg f16 [4*H*dh][ldw] = rows of q_proj, k_proj * dk^-0.5,
 * v_proj, g_proj (bias likewise); Q,K f16 [nseq][H][Tp][dh]; Kt,Vt f16 [nseq][H][dh][Tp]; G f16 [M][H*dh]. */
int eend_retention_proj_f16(const void* A, int lda, const void* Wqkvg, int ldw, const float* bias, void* Q,
                            void* K, void* Kt, void* Vt, void* G, int nseq, int Tp, int H, int dh, int Kdim,
                            void* stream);

/* Chunk-recurrent retention with decay 1 (retention.py:146-194 + RetNetRelPos :30-47), the per-head
 * LayerNorm (eps gn_eps, no affine, :222) and the swish gate (:224) in one pass:
 * O = swish(G) * LN_head(retention(Q,K,V)).  L = recurrent_chunk_size; workspaces: St_ws f16
 * [nseq][H][nc][2][64][64], kv_ws f32 [nseq][H][nc][64][64], cscale_ws / sexp_ws f32 [nseq][H][nc],
 * nc = ceil(Tp / L).  Three launches: chunk-parallel K_c^T V_c, per-(seq,head) prefix scan, core.
 * T_valid (0 = Tp): frames at or beyond it are slab padding (Tp rounds the chunk-padded length up to 64);
 * chunks that start there are skipped and their rows of O are left untouched.
 * state_in / state_out (optional, f32 [nseq][H][64][64], the reference's `prev_key_value` before its scaling,
 * retention.py:176-180): the chunk state before the first / after the last chunk of this call, so a long recording
 * can be processed a few chunks at a time with the state carried across calls (BASELINE config 5). */
int eend_retention_chunk_f16(const void* Q, const void* K, const void* Kt, const void* Vt, const void* G,
                             void* O_f16, void* St_ws, float* kv_ws, float* cscale_ws, float* sexp_ws, int nseq,
                             int H, int Tp, int L, int ldo, int ldg, float gn_eps, int T_valid,
                             const float* state_in, float* state_out, void* stream);

/* The same operator with its four projections fused on chip (ret_stream.hip, round 5): replaces eend_retention_proj_f16 +
 * eend_retention_chunk_f16 (`MultiScaleRetention.forward`, LS-EEND/nnet/modules/retention.py:196-228, called from
 * conformer/attention.py and merge_retnet_layer.py:233-253): q / k / k^T / v^T / g never exist in HBM.  X f16 [nseq*Tp][ldx]: the
 * retention's input rows; Xlo (optional, same layout): f16(x - f16(x)) of the f32 stream the rows were rounded from -- with it the
 * QUERY projection carries ~22 significand bits (three f16 MFMA products); the query is a hi/lo f16 pair in the score and cross-chunk
 * products either way.  W_packed: eend_retention_stream_pack_f16 of the f32 [q; k * dk^-0.5; v; g] rows ([1024][256]) into
 * eend_retention_stream_elems() f16 elements (hi and lo parts of the q rows), once per parameter version; bias f32 [1024] likewise.
 * H = 4, dh = 64, L <= 512 (eend_retention_stream_ok; the caller keeps the two-call form otherwise).  Workspaces, T_valid,
 * state_in / state_out: as eend_retention_chunk_f16.  Three launches: chunk K^T V products (projecting K, V on the fly), prefix scan,
 * rows. */
int eend_retention_stream_elems(void);
int eend_retention_stream_ok(int L, int Tp, int ldx, int ldo);
int eend_retention_stream_pack_f16(const float* Wqkvg_f32, void* packed_out, void* stream);
int eend_retention_stream_f16(const void* X_f16, int ldx, const void* Xlo_f16, const void* W_packed, const float* bias, void* O_f16, int ldo,
                              void* St_ws, float* kv_ws, float* cscale_ws, float* sexp_ws, int nseq, int Tp, int L, float gn_eps,
                              int T_valid, const float* state_in, float* state_out, void* stream);

/* Stand-alone LayerNorm f32 [M][D] -> f16 (D <= 1024): second of two back-to-back LayerNorms
 * (conformer/encoder.py:110 then feed_forward.py:48; encoder.py:196 then feed_forward.py:48). */
int eend_layernorm_f16(const float* x, const float* gamma, const float* beta, float eps, void* out_f16, int M,
                       int D, void* stream);

/* Causal depthwise Conv1d (k taps, left context k-1, no bias) -> BatchNorm1d(eval) -> Swish
 * (conformer/convolution.py:65-68,143-147).  x,out f16 [nseq][Tp][D]; w f32 [D][k].  halo_f16 (optional,
 * [nseq][k-1][D]): the k-1 input frames preceding the slab (carried from the previous call); null = zeros. */
int eend_dwconv_bn_swish_f16(const void* x_f16, const float* w, const float* bn_weight, const float* bn_bias,
                             const float* bn_mean, const float* bn_var, float eps, void* out_f16, int nseq,
                             int Tp, int D, int k, const void* halo_f16, void* stream);

/* Incremental self-attention of FS-EEND streaming (FS-EEND/nnet/modules/streaming_tfm.py:15-37,
 * used by StreamingTransformerEncoderLayer :61-66 and StreamingAttractorDecoderLayer :197-201): the
 * packed in-proj of ONE new token per sequence (qkv f16 [N][3*H*64]) is appended to the projected
 * K/V caches (f16 [N][H][cap][64], `t` tokens already present, t < cap) and attends over all t+1
 * tokens.  out f16 [N][H*64]. */
int eend_attn_decode_f16(const void* qkv, void* K_cache, void* V_cache, void* out_f16, int N, int H, int cap,
                         int t, float scale, void* stream);
/* eend_attn_decode_dev_f16 for long histories (BASELINE config 5: t up to 36 000): the key axis is split over
 * cap/512 workgroups per (n, h) whose (max, sum, o) partials a second kernel merges with the new token -- the per-frame
 * cost follows HBM bandwidth instead of one wave's latency chain.  ws: f32 scratch of N*H*ceil(cap/512)*66 floats.
 * Same results as the single-wave kernel up to fp32 summation order. */
int eend_attn_decode_split_f16(const void* qkv, void* K_cache, void* V_cache, void* out_f16, float* ws, long ws_floats, int N,
                               int H, int cap, const int* t_dev, float scale, void* stream);

/* The same with the token count read from device memory (*t_dev), so that a captured hipGraph of the frame step
 * (FS-EEND/streaming_infer_dia.py's per-frame loop) stays valid while the history grows; *t_dev >= cap makes the
 * launch a no-op.  eend_counter_add_i32: *counter += inc on the stream (the graph's own "t += 1"). */
int eend_attn_decode_dev_f16(const void* qkv, void* K_cache, void* V_cache, void* out_f16, int N, int H, int cap,
                             const int* t_dev, float scale, void* stream);
int eend_counter_add_i32(int* counter, int inc, void* stream);

/* Many streams in one frame step (FsMultiStreamSession): S slots, each with its own history length and lifetime; every row
 * computes every frame and per-slot int32 masks in device memory decide which state changes (additive to ABI version 5).
 *
 * eend_attn_decode_ragged_f16: the incremental self-attention of FS-EEND streaming (FS-EEND/nnet/modules/streaming_tfm.py:15-37)
 * over ragged histories, key-split as eend_attn_decode_split_f16.  Row n of qkv f16 [N][3*H*64] belongs to sequence
 * s = n / rows_per_seq (1 for encoder layers, C for decoder layers; N % rows_per_seq == 0) whose history length is len_dev[s].
 * mask_dev[s] != 0 and len < cap: the new k / v are appended at row len of K_cache / V_cache (f16 [N][H][cap][64]) and the row
 * attends over len + 1 tokens; otherwise the caches are untouched and the output row (out f16 [N][H*64]) is zero.  The length
 * is not advanced here (eend_counter_add_masked_i32).  A row's result depends on its own history alone, not on cap or on the
 * other rows: 512-key blocks anchored at key 0, merged in key order.  ws: f32 scratch of N*H*ceil(cap/512)*66 floats; the grid
 * is fixed per cap, so a captured hipGraph stays valid while the lengths grow. */
int eend_attn_decode_ragged_f16(const void* qkv, void* K_cache, void* V_cache, void* out_f16, float* ws, long ws_floats, int N, int H,
                                int cap, int rows_per_seq, const int* len_dev, const int* mask_dev, float scale, void* stream);
/* len_dev[s] += (mask_dev[s] != 0) for s < S, in one launch. */
int eend_counter_add_masked_i32(int* len_dev, const int* mask_dev, int S, void* stream);
/* The look-ahead window of the streaming Conv1d (FS-EEND/nnet/modules/streaming_tfm.py:141-167 keeps the last k frames) for S
 * slots: win f16 [S][k*D] ([tap*D + c], oldest tap first).  mode_dev[s] == 1: shift by one frame and append x f32 [S][D] row s
 * (cast to f16); == 2: shift and append zeros (the dummy_conv_input frames of FS-EEND/streaming_infer_dia.py:77-95);
 * anything else: the slot's window is left as it is. */
int eend_window_push_f16(void* win_f16, const float* x, const int* mode_dev, int S, int k, int D, void* stream);

/* Many frames per slot in one multi-stream step (FsMultiStreamSession.step_frames; additive to ABI version 5).  Rows follow the
 * batch forward's (B, C, Tp) slabs with Tp = nmax (1 <= nmax <= 64): row q*nmax + j is frame j of sequence q.
 *
 * eend_attn_chunk_ragged_f16: the chunked form of eend_attn_decode_ragged_f16 ("chunked prefill" over ragged K/V histories).
 * qkv f16 [Nseq*nmax][3*H*64]; sequence q belongs to slot s = q / rows_per_seq (Nseq % rows_per_seq == 0) with history length
 * len_dev[s] and cnt_dev[s] (0..nmax) new frames.  Query j < cnt sits at position len + j and attends, scale `scale`, over cache
 * keys [0, len) and the chunk's own keys 0..j; its k / v are appended at row len + j of K_cache / V_cache (f16 [Nseq][H][cap][64])
 * and no other cache row changes.  Output rows (out f16 [Nseq*nmax][H*64]) with j >= cnt are zero; cnt == 0 or len + cnt > cap
 * leaves the sequence's caches untouched with all its rows zero.  Cache rows at or beyond len are never read.  As in the decode,
 * 512-key blocks anchored at key 0 merged in key order make a row depend on its own history and chunk alone.  The lengths are not
 * advanced (eend_counter_add_count_i32).  ws: f32 scratch of Nseq*H*ceil(cap/512)*nmax*66 floats; the grid is fixed per cap
 * and nmax, so a captured hipGraph stays valid while the lengths and counts change. */
int eend_attn_chunk_ragged_f16(const void* qkv, void* K_cache, void* V_cache, void* out_f16, float* ws, long ws_floats, int Nseq, int H,
                               int cap, int nmax, int rows_per_seq, const int* len_dev, const int* cnt_dev, float scale, void* stream);
/* len_dev[s] += cnt_dev[s] for s < S, in one launch. */
int eend_counter_add_count_i32(int* len_dev, const int* cnt_dev, int S, void* stream);
/* The look-ahead window (as eend_window_push_f16: win f16 [S][k*D]) over a chunk: slot s takes npush_dev[s] frames of x f32
 * [S*nmax][D] (rows s*nmax + j) and then ndummy_dev[s] zero frames, npush + ndummy <= nmax.  The windows that emit are written as
 * the Conv1d's f16 im2col rows cols_f16 [S*nmax][k*D]: row s*nmax + i (i < ndec_dev[s] <= npush + ndummy) holds the window after
 * push npush + ndummy - ndec + i + 1, rows i >= ndec are zero.  The stored window ends exactly as npush + ndummy calls of
 * eend_window_push_f16 leave it.  Counts out of range leave the slot's window alone with zero rows. */
int eend_window_chunk_f16(void* win_f16, const float* x, void* cols_f16, const int* npush_dev, const int* ndummy_dev, const int* ndec_dev,
                          int S, int nmax, int k, int D, void* stream);

/* Prefill of a stream from a backlog (FsMultiStreamSession.prefill; additive to ABI version 5).
 *
 * eend_attn_prefill_f16: causal attention of Tq >= 1 new frames per sequence over the K/V caches, for Nseq sequences that share
 * the history length t0: FS-EEND/nnet/modules/streaming_tfm.py:15-37 applied to the Tq frames in order.  qkv f16 [Nseq*Tq] rows of
 * 3*H*64 halves at a row stride of ldq halves (ldq % 8 == 0); row i*Tq + j is frame j of call sequence i, which is sequence
 * seq0 + i of K_cache / V_cache (f16 [Ncache][H][cap][64]).  Frame j's k / v are copied bit for bit to cache row t0 + j, and
 * output row i*Tq + j (out f16 [Nseq*Tq][H*64]) is the softmax attention, scale `scale`, of query j over cache keys [0, t0 + j].
 * Cache rows at or beyond t0 + Tq are neither read nor written and no other sequence is touched; key tiles are anchored at
 * key 0, so a row's result depends on its own sequence, t0 and Tq alone (not on cap, seq0 or Ncache).  t0 + Tq > cap, a NULL
 * or unaligned (16 B) pointer or a sequence range outside [0, Ncache) returns EEND_EINVAL with nothing touched.  Work items are
 * (sequence, head, 128-query tile): a call with few queries over a long history has few of them and belongs to
 * eend_attn_chunk_ragged_f16. */
int eend_attn_prefill_f16(const void* qkv, long ldq, void* K_cache, void* V_cache, void* out_f16, int Ncache, int seq0, int Nseq, int H,
                          int cap, int t0, int Tq, float scale, void* stream);

/* Suspend / resume of a stream slot (MultiStreamSession.snapshot / resume; additive to ABI version 5).
 *
 * eend_copy_blocks: a batched strided block copy, device memory to device memory.  Entry i moves nblocks blocks of block_bytes
 * bytes: block b from src + b * src_stride to dst + b * dst_stride.  That is every piece of a slot's state: the rows [0, len) of
 * nseq * H K (or V) sequences of an f16 [N][H][cap][64] cache are nseq * H blocks of len * 128 bytes at a stride of cap * 128 on
 * the cache side and len * 128 in a packed blob; a retention state, a conv cache or a window row is one block.  `entries` is a
 * HOST array of n <= EEND_COPY_BLOCKS_MAX entries: they are passed by value in the kernel arguments (one launch for all of
 * them, no device table, nothing the caller must keep alive), and every check happens on the host.  Every address, size and
 * stride is a multiple of 16 bytes; offsets are 64-bit.  EEND_EINVAL, before any launch, for: entries == NULL with n > 0; n < 0
 * or n > EEND_COPY_BLOCKS_MAX; a negative or misaligned field; a NULL src or dst in an entry that moves bytes; a stride below
 * block_bytes where nblocks > 1; a source range [src, src + (nblocks - 1) * src_stride + block_bytes) that overlaps the entry's
 * destination range.  An entry with nblocks == 0 or block_bytes == 0 is skipped (its pointers may be NULL), and a call that moves
 * nothing returns EEND_OK without a launch.  Bytes outside the destination blocks are not written and no source byte is.  Two
 * entries of one call must not write the same bytes (not checked).  Work is cut into tiles of eend_copy_blocks_tile_bytes()
 * bytes, one workgroup each, that never span two blocks; the grid is sized to the device and strides over the tiles. */
#define EEND_COPY_BLOCKS_MAX 64
typedef struct eend_block_copy {
    const void* src;
    void* dst;
    long nblocks, block_bytes, src_stride, dst_stride;
} eend_block_copy;
int eend_copy_blocks(const eend_block_copy* entries, int n, void* stream);
long eend_copy_blocks_tile_bytes(void);

/* Many LS-EEND streams in one frame step (LsMultiStreamSession): the state touches of the LS frame step per slot (additive to
 * ABI version 5).  Row n belongs to sequence s = n / rows_per_seq (1 for encoder rows, C for decoder rows); len_dev / mask_dev
 * are int32 [S] in device memory, so a captured hipGraph stays valid from frame to frame.
 *
 * eend_retention_step_ragged_f32: eend_retention_step_f32 (MultiScaleRetention.recurrent_forward, LS-EEND/nnet/modules/
 * retention.py:126-144, decay 1, + per-head LayerNorm and swish gate) with each sequence's own scale: the reference keeps one
 * incremental_state["scale"] per batch (retention.py:141-142), here scale_in = len_dev[s] and scale_out = len_dev[s] + 1, so a
 * slot at position t is bit-identical to eend_retention_step_f32 with scale_in = t.  len_dev[s] == 0 is an empty state: the
 * old kv_state rows are not read (whatever a reused slot holds, NaN included, cannot leak).  mask_dev[s] == 0 (or a negative
 * length): kv_state untouched and not read, output rows zero.  qkvg_f32 [N][4*H*64], kv_state f32 [N][H][64][64], out_f16
 * and / or out_f32 [N][H*64].  The lengths are not advanced (eend_counter_add_masked_i32). */
int eend_retention_step_ragged_f32(const float* qkvg_f32, float* kv_state, const int* len_dev, const int* mask_dev, int rows_per_seq,
                                   void* out_f16, float* out_f32, int N, int H, float gn_eps, void* stream);
/* eend_dwconv_step_f16 (ConformerConvModule.forward_one_step, conformer/convolution.py:157-163) per slot b < B: mask_dev[b] != 0
 * shifts the slot's cache f32 [B][D][k-1] in place, with len_dev[b] == 0 reading it as zeros (the zero-initialised conv_caches
 * of LS-EEND/streaming_infer_dia.py:40-45); mask_dev[b] == 0 leaves the cache as it is and writes a zero output row. */
int eend_dwconv_step_ragged_f16(const void* x_f16, float* cache, const int* len_dev, const int* mask_dev, const float* w,
                                const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var, float eps,
                                void* out_f16, int B, int D, int k, void* stream);
/* eend_window_push_f16 on an f32 window win_f32 [S][k*D] (the all-f32 look-ahead window of the LS frame step, LS model
 * :151-186): mode_dev[s] == 1 shifts and appends x f32 [S][D] row s, == 2 shifts and appends zeros, anything else keeps it. */
int eend_window_push_f32(float* win_f32, const float* x, const int* mode_dev, int S, int k, int D, void* stream);

/* Many frames per slot in one LS-EEND multi-stream step (LsMultiStreamSession with max_frames = nmax; additive to ABI version 5).
 * cnt_dev int32 [S]: the frames slot s takes in this launch (0..nmax; anything else counts as 0); its rows are the first
 * cnt_dev[s] of its nmax rows, the others are written as zeros.  The lengths are not advanced (eend_counter_add_count_i32).
 *
 * eend_retention_chunk_ragged_f32: sequence q < Nseq (slot s = q / seq_per_slot: 1 for the encoder, C for the decoder) owns rows
 * q*nmax .. q*nmax + nmax - 1 of qkvg_f32 [Nseq*nmax][4*H*64] and of out_f16 and / or out_f32 [Nseq*nmax][H*64]; its first
 * cnt_dev[s] rows are frames len_dev[s] .. len_dev[s] + cnt - 1.  The state kv_state f32 [Nseq][H][64][64] is read once (not at
 * all when len_dev[s] == 0) and written once; cnt == 0 leaves it unread and unwritten.  Outputs and final state are bit for bit
 * those of cnt successive eend_retention_step_ragged_f32 calls (lengths advanced in between).  nmax in 1..64. */
int eend_retention_chunk_ragged_f32(const float* qkvg_f32, float* kv_state, const int* len_dev, const int* cnt_dev, int seq_per_slot,
                                    int nmax, void* out_f16, float* out_f32, int Nseq, int H, float gn_eps, void* stream);
/* eend_dwconv_step_ragged_f16 over a chunk: x_f16 / out_f16 [B*nmax][D], slot b's frames are rows b*nmax + j, j < cnt_dev[b]; the
 * cache f32 [B][D][k-1] ends as after cnt one-frame calls (bit-identical, outputs too).  nmax in 1..64. */
int eend_dwconv_chunk_ragged_f16(const void* x_f16, float* cache, const int* len_dev, const int* cnt_dev, int nmax, const float* w,
                                 const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var, float eps,
                                 void* out_f16, int B, int D, int k, void* stream);
/* eend_window_chunk_f16 on the f32 window of eend_window_push_f32: win_f32 [S][k*D], x f32 [S*nmax][D], im2col rows cols_f32
 * [S*nmax][k*D]; the stored window ends bit for bit as the same pushes and dummies through eend_window_push_f32.  nmax in 1..64. */
int eend_window_chunk_f32(float* win_f32, const float* x, float* cols_f32, const int* npush_dev, const int* ndummy_dev, const int* ndec_dev,
                          int S, int nmax, int k, int D, void* stream);
/* eend_spk_attn_step_f32 on decoder slabs: qkv f32 [(b*C + c)*Tp + t][768], out_f32 [(b*C + c)*Tp + t][256]; the C rows of frame
 * (b, t) attend to each other.  C <= 16; Tp = 1 is the layout of eend_spk_attn_step_f32. */
int eend_spk_attn_rows_f32(const float* qkv, float* out_f32, int B, int C, int Tp, float scale, void* stream);

/* Prefill of an LS-EEND stream from a backlog (LsMultiStreamSession.prefill; additive to ABI version 5).
 *
 * eend_retention_prefill_f32: T >= 1 new frames per sequence through the recurrence of eend_retention_step_ragged_f32, for Nseq
 * sequences that share the position t0 >= 0 (a host int, as in eend_attn_prefill_f16), in chunk-parallel form: call sequence i is
 * sequence seq0 + i of kv_state f32 [Ncache][H][64][64] (Nseq = 1 on an encoder state, C at s*C on a decoder state); row i*T + j of
 * qkvg_f32 [Nseq*T][4*H*64] (q | k | v | g) is its frame t0 + j, and out_f16 and / or out_f32 [Nseq*T][H*64] get the same rows.
 * With kv_t = (sqrt(t0) kv_{t0-1} + sum_{i = t0..t} v_i k_i^T) / sqrt(t + 1) the frames go in chunks of 64 through three passes,
 * each with one work item per (sequence, head, chunk): the chunk sums P_c = sum v_i k_i^T; their exclusive prefix S_c = sqrt(t0)
 * kv_in + sum_{c' < c} P_c' in chunk order, with kv_out = (S_last + P_last) / sqrt(t0 + T); and the outputs o_i = ((Q K^T .
 * [j <= i]) V + Q S_c^T)_i / sqrt(t0 + 64 c + i + 1) followed by the per-head LayerNorm and swish gate.  All operands and
 * accumulators are f32 (v_mfma_f32_16x16x4_f32); out_f16 is the saturating f16 rounding of the value written to out_f32.  The
 * state ends as after T per-frame updates (up to the summation order); with t0 == 0 it is not read, whatever the memory holds.
 * No other state sequence and no other row is read or written; rows of a tail chunk beyond T are taken as zeros, not read.  ws:
 * at least Nseq * H * ceil(T / 64) * 4096 floats.  A NULL or unaligned (16 B) pointer, T < 1, t0 < 0, both outputs NULL, a
 * sequence range outside [0, Ncache) or a workspace that is too small returns EEND_EINVAL before any launch. */
int eend_retention_prefill_f32(const float* qkvg_f32, float* kv_state, void* out_f16, float* out_f32, float* ws, long ws_floats,
                               int Ncache, int seq0, int Nseq, int H, int t0, int T, float gn_eps, void* stream);
/* eend_dwconv_step_ragged_f16 for slot b alone over T >= 1 frames x_f16 / out_f16 [T][D], one thread per (frame, channel): the taps
 * of frame i are the last k - 1 entries of (old cache ++ x[0..i-1]), a slot at t0 == 0 reads its cache row as zeros, and the fma
 * chain is the one-frame kernel's, so outputs and the final cache row (the last k - 1 entries of (old cache ++ x), written by a
 * second launch) are bit for bit those of T one-frame calls.  Only row b of cache f32 [B][D][k-1] is touched. */
int eend_dwconv_prefill_f16(const void* x_f16, float* cache, int b, int t0, const float* w, const float* bn_weight, const float* bn_bias,
                            const float* bn_mean, const float* bn_var, float eps, void* out_f16, int T, int B, int D, int k,
                            void* stream);

/* One frame of MultiScaleRetention.recurrent_forward (retention.py:126-144, decay 1) + per-head
 * LayerNorm + swish gate, state updated in place.  qkvg f16 [N][4*H*64] = [q | k*dk^-0.5 | v | g];
 * kv_state f32 [N][H][64][64] in the reference's incremental_state["prev_key_value"] layout;
 * scale_in / scale_out f32 [H] (incremental_state["scale"]; zero state + scale 0 before frame 0). */
int eend_retention_step_f16(const void* qkvg, float* kv_state, const float* scale_in, float* scale_out,
                            void* out_f16, int N, int H, float gn_eps, void* stream);
/* Frame-by-frame sessions: the retention projections of one frame in full f32 -- qkvg_f32 [N][1024] =
 * LayerNorm(x)[N][256] . Wqkvg^T + bias with the packed f32 weight [q; k*dk^-0.5; v; g] (ln_gamma == NULL: no
 * LayerNorm, the decoder's post-norm stream) -- and the recurrent step on those f32 projections.  The
 * recurrence amplifies operand rounding with the stream position (retention.py:126-144 normalises a state that grows like
 * sqrt(t)); f16 projections cost > 1e-3 on the logits late in a one-hour stream, f32 ones keep the reference's fp32
 * streaming within the 1e-3 bar (tests/test_long_horizon.py). */
int eend_retention_proj_step_f32(const float* x, const float* ln_gamma, const float* ln_beta, float ln_eps, const float* Wqkvg,
                                 const float* bias, float* qkvg_f32, int N, void* stream);
int eend_retention_step_f32(const float* qkvg, float* kv_state, const float* scale_in, float* scale_out, void* out_f16, float* out_f32,
                            int N, int H, float gn_eps, void* stream);      /* out_f16 and / or out_f32 [N][256] */
/* The remaining pieces of an all-f32 LS decoder frame step (merge_retnet_layer.py:255-276 with <= 16 rows = one frame x
 * max_nspks slots): y = act(A W^T + bias) with f32 activations AND f32 weights in torch's nn.Linear layout (act 0 none /
 * 1 relu / 2 swish; K % 8 == 0, any M >= 1: up to 16 rows take the wave-per-feature kernel, more rows the f32 MFMA kernel where
 * N % 16 == 0, K % 16 == 0 and bias / out are 16-byte aligned, else the wave-per-feature kernel in groups of 16 rows); the post-norm join out = LayerNorm((A W^T + bias) * alpha + res) (N = 256; out_f16
 * optional copy); the speaker-axis attention of the frame on f32 [B*C][768] = [q | k | v] rows (C <= 16).  Why f32: DESIGN
 * 9a -- the decoder retention's per-head LayerNorm amplifies f16 operand rounding ~30x on isolated frames. */
int eend_linear_step_f32(const float* A, int lda, const float* W, int ldw, const float* bias, float* out_f32, int ldo, int M, int N,
                         int K, int act, void* stream);
int eend_linear_res_ln_step_f32(const float* A, int lda, const float* W, int ldw, const float* bias, const float* res, float alpha,
                                const float* gamma, const float* beta, float eps, float* out_f32, void* out_f16, int M, int K,
                                void* stream);
int eend_spk_attn_step_f32(const float* qkv, float* out_f32, int B, int C, float scale, void* stream);
/* ... and of the Conformer encoder's f32 half-step FFNs (feed_forward.py:47-57 inside the pre-norm blocks of
 * conformer/encoder.py:76-113): the pre-norm join out_f32 = (A W^T + bias) * alpha + res (the un-normalised stream) with the NEXT
 * sub-layer's LayerNorm of it as ln_out_f32 and / or ln_out_f16; and a plain row LayerNorm f32 -> f32 (256 features). */
int eend_linear_res_scale_ln_step_f32(const float* A, int lda, const float* W, int ldw, const float* bias, const float* res, float alpha,
                                      const float* gamma, const float* beta, float eps, float* out_f32, float* ln_out_f32,
                                      void* ln_out_f16, int M, int K, void* stream);
int eend_layernorm_rows_f32(const float* x, const float* gamma, const float* beta, float eps, float* out_f32, int M, void* stream);
/* y[r] = x[r] / ||x[r]||_2, f32 rows of 256 features: the embedding normalisation (LS model :87, no eps) behind the f32
 * look-ahead conv of a frame step (the conv itself is eend_linear_step_f32 over the flattened 19-frame window). */
int eend_l2norm_rows_f32(const float* x, float* y, int rows, void* stream);
/* Frame-by-frame decoder input in f32: out[b*C + c] = W[:, :256] emb[b] + pc[c] (`convert(cat(emb, pe))`, LS model
 * :229-233; pc from eend_convert_const_f32).  W_f32 is the convert.weight parameter itself ([256][ldw], ldw = 512).
 * f32 for the same reason as the projections above: the decoder retention amplifies the f16 rounding of this linear ~30x
 * at some frames of a long stream.  out_f32 / out_f16 [B*C][256]; C <= 64. */
int eend_convert_fanout_step_f32(const float* emb_f32, const float* W_f32, int ldw, const float* pc, float* out_f32, void* out_f16,
                                 int B, int C, void* stream);

/* One frame of the causal depthwise conv + BatchNorm(eval) + Swish of ConformerConvModule.
 * forward_one_step (conformer/convolution.py:157-163); cache f32 [B][D][k-1] (the driver's
 * conv_caches layout, streaming_infer_dia.py:42-45) shifted in place.  x,out f16 [B][D]. */
int eend_dwconv_step_f16(const void* x_f16, float* cache, const float* w, const float* bn_weight,
                         const float* bn_bias, const float* bn_mean, const float* bn_var, float eps,
                         void* out_f16, int B, int D, int k, void* stream);

/* Unmasked MHA core over the C (<= 12) attractor slots of each frame (_sa_block2,
 * merge_tfm_encoder.py:388-394; LS-EEND/nnet/modules/merge_retnet_layer.py:301-306).
 * qkv f16 [B*C*Tp][768] (row = (b*C + c)*Tp + t) -> O f16 [B*C*Tp][256].  H = 4, dh = 64. */
int eend_spk_attn_f16(const void* qkv, void* O_f16, int B, int C, int Tp, int H, float scale,
                      void* stream);


/* Packed in-projection + causal multi-head attention in one launch (nn.MultiheadAttention(x, x, x) on the time axis:
 * nn.TransformerEncoderLayer.self_attn, FS model :147; self_attn1 of the fusion layers, merge_tfm_encoder.py:379-385),
 * Tp = 64 m <= 512 (round 6; rounds 4 - 5: 512 only), H = 4, d_model = 256 (attn_stream.hip): the in-projection weights pre-packed in MFMA fragment order, a wave keeps
 * the X rows of the 64 tokens whose queries it runs in registers, the head's 96 KB of weights arrive by LDS-DMA, Q, K and V never
 * reach HBM.  eend_inproj_attn_pack_f16 re-orders W_in f16 [768][256] (= in_proj_weight with the q rows pre-multiplied by
 * 1/sqrt(64) * log2(e)) into eend_inproj_attn_packed_elems() f16 elements, once per parameter version.  mask: key j visible to
 * query i iff j - i <= mask_delay and j < kv_len (1 <= kv_len <= Tp, EEND_EINVAL otherwise).  Equivalent to eend_inproj_heads_bf16 followed by
 * eend_attn_causal_bf16(scale = ln 2), which is what the caller uses for other chunk lengths (EEND_EINVAL here).  The key bias
 * is not applied (it cancels in the softmax); b_in is the [768] in_proj_bias, q part pre-scaled. */
int eend_inproj_attn_packed_elems(void);
int eend_inproj_attn_pack_f16(const void* W_in, void* packed_out, void* stream);
int eend_inproj_attn_causal_packed_f16(const void* X_f16, int ldx, const void* W_packed, const float* b_in, void* O_f16,
                                       int nseq, int H, int Tp, int ldo, int mask_delay, int kv_len, void* stream);

/* The same operator on the C speaker slots of n_utt = nseq / C utterances whose input rows differ by a constant per slot (the first
 * fusion layer behind eend_convert_fanout_f16: row (b, c, t) = row (b, 0, t) + pd[c]), Tp = 512 only (EEND_EINVAL otherwise; the caller
 * keeps the entry above there), 1 <= C <= 12, C | nseq.  Only the rows of slot 0 (sequences b C) are read: K and V^T are projected once
 * per (utterance, head) and serve every slot -- a constant added to all keys cancels in the softmax, one added to all values passes
 * through it -- and per slot Q_c = bf16(q_acc + dq_c) and O_c = f16(O / l + dv_c), both adds in f32 before the only rounding.
 * slot_delta f32 [C][512]: row c = (W_q (pd[c] - pd[0]) with W_q pre-scaled like the packed q rows | W_v (pd[c] - pd[0])), row 0 zero
 * (not read; NULL allowed for C = 1).  An item of the kernel covers slots_per_item consecutive slots (a divisor of C, EEND_EINVAL
 * otherwise; 0: eend_inproj_attn_slots_choice for the device's workgroup count); the result does not depend on it, bit for bit, and
 * slot 0 equals the entry above on the slot-0 sequences.  Rows of O go to sequence b C + c. */
int eend_inproj_attn_slots_choice(int n_utt, int C, int workgroups);
int eend_inproj_attn_causal_slots_f16(const void* X_f16, int ldx, const void* W_packed, const float* b_in, void* O_f16,
                                      int nseq, int H, int Tp, int ldo, int mask_delay, int kv_len, int C, const float* slot_delta,
                                      int slots_per_item, void* stream);

/* The same operator for windows of more than 512 frames (round 6; Tp = 64 m, 1 <= kv_len <= Tp, mask_delay >= 0; whole recordings at
 * test time, FS model :147 on an un-chunked sequence): the frames are cut into groups of 512 and the launch runs one item of the kernel
 * above per (sequence, head, query group, key group the mask reaches).  The item of a group with itself writes its rows of O; an item
 * of two different groups projects Q from the query group's rows and K / V from the key group's, and leaves normalised partial rows in
 * part_f16; every item leaves the log2 of its softmax denominators in lse_f32, and a second launch weighs the partial rows of a query
 * group with them (O = sum_i 2^(lse_i - lse) O_i).  Scratch sizes from eend_inproj_attn_long_scratch_elems (EEND_EINVAL for a shape
 * this form does not cover: Tp <= 512 -- use the entry above --, more than 64 items or 9 key groups per query group; the caller
 * keeps eend_inproj_heads_bf16 + eend_attn_causal_bf16 there).  Same weights, bias and mask convention as the entry above. */
int eend_inproj_attn_long_scratch_elems(int nseq, int Tp, int mask_delay, int kv_len, long long* part_f16_elems, long long* lse_f32_elems);
int eend_inproj_attn_causal_long_f16(const void* X_f16, int ldx, const void* W_packed, const float* b_in, void* O_f16, void* part_f16,
                                     float* lse_f32, int nseq, int H, int Tp, int ldo, int mask_delay, int kv_len, void* stream);


/* attractors / ||attractors||_2 and logits[b,t,c] = <emb[b,t], attractors[b,t,c]>
 * (FS model :43,:60 / :76,:79; LS model :89,:117).  emb f32 [B][Tp][D], attr f32 [B*C][Tp][D]
 * -> attr_out f32 [B][T][C][D], logits f32 [B][T][C]. */
int eend_head_l2dot_f32(const float* emb, const float* attr, float* attr_out, float* logits, int B, int T,
                        int Tp, int C, int D, void* stream);
/* The same reading the un-normalised attractors from the f16 stream (FS-EEND f16 residual mode: the last decoder LayerNorm's
 * output is then never written in f32). */
int eend_head_l2dot_a16_f32(const float* emb, const void* attr_f16, float* attr_out, float* logits, int B, int T,
                            int Tp, int C, int D, void* stream);


/* ======================================================================================================
 * TRAINING STEP (BASELINE config 4).  The reference trains through torch autograd + torch.optim.Adam under
 * PyTorch-Lightning (FS-EEND/train/oln_tfm_enc_dec.py:51-91 training_step, train/utils/loss.py:119-125
 * standard_loss, FS-EEND/train_dia.py:77-100 optimiser, :145-156 Trainer); the entry points below are the
 * hand-written backward of every forward op above, the loss, and the optimiser.  Gradient tensors that feed
 * an MFMA are bf16 (exponent range), saved forward activations f16, accumulation and the residual-gradient
 * stream f32.  `ws` arguments are caller-owned f32 scratch (`ws_floats` = its capacity in floats); parameter
 * gradients are written in fixed summation order (no atomics), so a step is bit-reproducible.
 * ====================================================================================================== */

/* Dropout (torch.nn.Dropout in train mode: FS model :147 / merge_tfm_encoder.py:209-219,385,394,398-399,609-614 and
 * nn.MultiheadAttention(dropout=p)).  The reference draws its masks from torch's Philox stream, which no other
 * implementation can reproduce; here a mask is a pure function of (seed, element index), so the backward recomputes it
 * instead of storing it and a step stays bit-reproducible:
 *   h = mix((a * 0x9E3779B1 + b) ^ seed),   keep <=> (h >> 8) >= thresh24,
 *   mix(x): x ^= x >> 16; x = (x & 0xFFFFFF) * 0x6B2F4D; x ^= x >> 13; x = (x & 0xFFFFFF) * 0x9E3779   (32-bit wrap-around; ABI 5 --
 *   versions up to 4 used the murmur3 finaliser, whose 32-bit multiplies are quarter rate on CDNA4)
 * with (a, b) = (row, column) of the element (attention: a = (seq*H + head)*Tp + query, b = key; speaker attention:
 * a = ((b*Tp + t)*4 + head)*16 + query slot, b = key slot).  thresh24 = round(p * 2^24), scale = 1/(1-p).
 * A null pointer or thresh24 == 0 means no dropout.  Host struct, read at call time. */
typedef struct eend_dropout {
    unsigned seed;
    unsigned thresh24;
    float scale;
} eend_dropout;

/* Training forward of nn.MultiheadAttention(x, x, x) on the time axis in one launch (attn_stream.hip, round 6; windows Tp = 64 m <= 512,
 * H = 4): eend_inproj_heads_train_bf16 + eend_attn_causal_lse_bf16 with Q / K / V^T staying on chip between projection and attention.
 * W_packed = eend_inproj_attn_pack_f16 of the f16 in-projection operand copy (q rows pre-scaled as for the two entries it replaces), b_in
 * [768] (the key bias IS applied here: the saved K is the reference's).  Out: O_f16 [nseq*Tp][ldo] (the heads' context rows), Q / K / V
 * bf16 head rows [nseq][H][Tp][64] and lse [nseq][H][Tp] (log2 domain) for eend_attn_causal_bwd_bf16; `drop` acts on the attention
 * probabilities, element ((seq*H + head)*Tp + query, key), as in eend_attn_causal_lse_bf16.  EEND_EINVAL for longer windows: the caller
 * keeps the two entries (and the [d][t] copies their backward reads). */
int eend_inproj_attn_train_bf16(const void* X_f16, int ldx, const void* W_packed, const float* b_in, void* O_f16, int ldo, void* Q_bf16,
                                void* K_bf16, void* V_bf16, float* lse, int nseq, int H, int Tp, int mask_delay, int kv_len,
                                const eend_dropout* drop, void* stream);

/* g_f32[M][256] += A[M][K] Wt^T in place on a packed weight stream (gemm_acc_stream.hip, round 6): eend_gemm_acc_bf16(res = out = g,
 * alpha = 1) for the data gradients whose K is large -- autograd of nn.MultiheadAttention's in_proj (K = 768; FS model :147,
 * merge_tfm_encoder.py:379-385) and of MultiScaleRetention's projections (K = 1024; LS retention.py:146-160).  A bf16 [M][lda],
 * Wt bf16 [256][ldw] (the transposed weight, as eend_gemm_acc_bf16 takes it), K a multiple of 128 in 256 .. 2048, re-ordered once per
 * parameter version by eend_gemm_acc_stream_pack_bf16 into eend_gemm_acc_stream_elems(K) 16-bit elements.  eend_gemm_acc_stream_ok is
 * the shape predicate; EEND_EINVAL otherwise (the caller keeps eend_gemm_acc_bf16 / eend_gemm_acc_lnbwd_bf16). */
int eend_gemm_acc_stream_elems(int K);
int eend_gemm_acc_stream_ok(int M, int K, int lda);
int eend_gemm_acc_stream_pack_bf16(const void* Wt, int ldw, void* stream_out, int K, void* stream);
int eend_gemm_acc_stream_bf16(const void* A, int lda, const void* wstream, float* g_f32, int M, int K, void* stream);

/* K = 256 input projections on a packed weight stream (proj_stream.hip, round 6): nn.MultiheadAttention's in_proj (FS model :147,
 * merge_tfm_encoder.py:379-385) and MultiScaleRetention's q / k / v / g projections (LS retention.py:146-160) in the training forward,
 * where the f16 operands of the forward kernel and the bf16 Q / K / V the hand-written backward keeps used to be two projections of the
 * same rows.  Y = X W^T + bias, X f16 [M][ldx] (256 features), W f16 [N][256], N = 256 n <= 1024, re-ordered once per parameter version
 * by eend_proj_stream_pack_f16 into eend_proj_stream_elems(N) f16 elements.  Each 256-feature output group g names up to three
 * destinations, all written from one pass over the rows:
 *   rows            rows_kind 1: [M][rows_ld] row-major (pointer at the group's first column); 2: head rows [seq][H][Tp][64];
 *                   f16, or bf16 with rows_bf16
 *   rows2_bf16_heads  a second copy as bf16 head rows
 *   heads_t         transposed head rows [seq][H][64][Tp] (f16, or bf16 with heads_t_bf16)
 * Head destinations need H = 4, Tp a multiple of 64 and M a multiple of Tp.  eend_proj_stream_ok is the shape predicate (pointers of
 * `groups` only tested for null / alignment); EEND_EINVAL on anything else -- the caller keeps eend_inproj_heads_train_bf16 /
 * eend_retention_proj_f16 / eend_gemm_f16 there. */
typedef struct eend_proj_group {
    void* rows;
    int rows_kind, rows_bf16, rows_ld;
    void* rows2_bf16_heads;
    void* heads_t;
    int heads_t_bf16;
} eend_proj_group;
int eend_proj_stream_elems(int N);
int eend_proj_stream_pack_f16(const void* W, void* stream_out, int N, void* stream);
int eend_proj_stream_ok(int ldx, int M, int N, int Tp, int H, const eend_proj_group* groups);
int eend_proj_stream_f16(const void* X, int ldx, const void* wstream, const float* bias, int M, int N, int Tp, int H,
                         const eend_proj_group* groups, void* stream);

/* eend_linear_res_ln_f16 that also saves what LayerNorm backward needs: xhat_f16 [M][256] = the normalised
 * row before the affine, rstd [M] = 1/sigma.  (torch.nn.LayerNorm inside nn.TransformerEncoderLayer, FS model
 * :147,:174; merge_tfm_encoder.py:364,373-374.)  `drop` acts on (A W^T + bias) before the residual (dropout1 /
 * dropout2 / dropout11 / dropout21), element (row m, column n). */
int eend_linear_res_ln_train_f16(const void* A, int lda, const void* W, int ldw, const float* bias, const float* res,
                                 float alpha, const float* gamma, const float* beta, float eps, float* out_f32,
                                 void* out_f16, void* xhat_f16, float* rstd, int M, int K, const eend_dropout* drop,
                                 void* stream);
/* relu(A W^T + bias) with dropout after the activation (the FFN's inner `self.dropout`, merge_tfm_encoder.py:398,613);
 * the stored activation is the dropped one, so its zeros are the ReLU-and-dropout mask of the backward.
 * N % 128 == 0, K % 64 == 0, lda / ldw / ldo % 8 == 0 (the tile writes 16-byte pieces of the output rows); EEND_EINVAL otherwise. */
int eend_linear_relu_train_f16(const void* A, int lda, const void* W, int ldw, const float* bias, void* out_f16, int ldo,
                               int M, int N, int K, const eend_dropout* drop, void* stream);
/* The two entries above as ONE launch for a post-norm ReLU block (round 5; FS nn.TransformerEncoderLayer._ff_block + norm2,
 * merge_tfm_encoder.py:397-399 / :612-614; LS merge_retnet_layer.py:250-253):
 *   hid = drop_hidden(relu(X W1^T + b1))            f16 [M][F], written once and never re-read by this launch
 *   y   = drop_out(hid W2^T + b2) * alpha + res     out_f32 / out_f16 = LayerNorm(y); xhat_f16, rstd as eend_linear_res_ln_train_f16
 * Same dropout indexing (row, column) per site as the two-launch form, so a given eend_dropout produces the same masks.
 * K = N = 256, F a multiple of 64, M * F * 2 < 2^32 bytes, 16-byte aligned hid / xhat; out_f32 may be res (in place).
 * EEND_EINVAL outside that: the caller keeps the two launches. */
int eend_ffn_train_f16(const void* X, int ldx, const void* W1, const float* b1, const void* W2, const float* b2, const float* res,
                       float alpha, const float* gamma, const float* beta, float eps, float* out_f32, void* out_f16, void* hid_f16,
                       void* xhat_f16, float* rstd, int M, int F, const eend_dropout* drop_hidden, const eend_dropout* drop_out,
                       void* stream);
/* The Macaron half-step FFN of a Conformer block (LS-EEND conformer/feed_forward.py:47-57 inside modules.py:32-33's residual) as one
 * launch: z = X W1^T + b1 (saved, f16), a = drop_hidden(swish(z)) (saved, f16), y = drop_out(a W2^T + b2) * alpha + res; then either
 * (residual_stream_unnormalised = 1, the pre-norm join: eend_linear_res_scale_ln_train_f16) out_f32 = y and out_f16 / xhat / rstd = the NEXT
 * sub-layer's LayerNorm of y, or (0: the block-final LayerNorm, eend_linear_res_ln_train_f16) out_f32 = out_f16 = LayerNorm(y).
 * Replaces eend_linear_f16 + eend_swish_dropout_f16 + that GEMM entry.  Shapes as eend_ffn_train_f16. */
int eend_ffn_swish_train_f16(const void* X, int ldx, const void* W1, const float* b1, const void* W2, const float* b2, const float* res,
                             float alpha, const float* gamma, const float* beta, float eps, float* out_f32, void* out_f16, void* z_f16,
                             void* a_f16, void* xhat_f16, float* rstd, int M, int F, int residual_stream_unnormalised,
                             const eend_dropout* drop_hidden, const eend_dropout* drop_out, void* stream);
/* Data-gradient backward of the same block in one launch (round 5; replaces eend_gemm_relu_bwd_bf16 + eend_gemm_acc_bf16 of its FFN):
 *   dH = drop_scale * (dY W2) where hid_f16 != 0, else 0     bf16 [M][F], written once (the weight gradient of linear1 reads it)
 *   g  += dH W1                                              the f32 residual-gradient stream [M][256], in place
 * dY bf16 [M][ldy], W2T = W2 transposed, bf16 [F][256]; W1T = W1 transposed, bf16 [256][F] (the copies the two-launch form uses).
 * F a multiple of 64, M * F * 2 < 2^32 bytes, 16-byte aligned buffers; EEND_EINVAL outside that. */
int eend_ffn_bwd_data_bf16(const void* dY, int ldy, const void* W2T, const void* hid_f16, const void* W1T, float drop_scale,
                           void* dH_bf16, float* g_f32, int M, int F, void* stream);
/* Round 6: eend_ffn_train_f16 / eend_ffn_bwd_data_bf16 on a PACKED WEIGHT STREAM (ffn_train_stream.hip; same reference sites): one
 * wave owns 32 / 48 token rows end to end, the hidden units stay in its registers and leave (hid, dH) / arrive (the mask) as 16-byte
 * accesses per lane.  eend_ffn_train_stream_pack re-orders two 16-bit matrices A [F][256], B [256][F] into the fragment sequence the
 * kernel consumes (eend_ffn_train_stream_elems(F) elements; F a multiple of 64, at most 2048): (W1, W2) in f16 for the forward,
 * (W2^T, W1^T) in bf16 for the data gradient.  Pack once per parameter version.  Results, saved tensors and dropout masks as the
 * un-packed entries (up to fp32 summation order), EXCEPT the layout of hid_f16 and dH_bf16: BLOCKED [ceil(M/16)][F/32][16 rows][32 units]
 * (element (m, u) at ((m>>4) * (F/32) + (u>>5)) * 512 + (m&15) * 32 + (u&31); allocate ceil(M/16) * 16 rows) -- a wave then writes its 16
 * rows as one sequential stream of whole cache lines, where row-major rows made the launch write-pattern-bound (594 -> 488 us forward,
 * 812 -> 493 us data gradient at [196608, 2048]).  The only consumers are eend_ffn_bwd_data_stream_bf16 (the mask) and the weight
 * gradients (eend_wgrad[_bias]_bf16 with x_is_f16 & 2 / & 4).  eend_ffn_train_stream_ok: the row count one launch can address (32-bit
 * offsets); outside it -> EEND_EINVAL, the caller keeps the un-packed, row-major entries. */
int eend_ffn_train_stream_elems(int F);
int eend_ffn_train_stream_ok(int M, int F, int ldx);
int eend_ffn_train_stream_pack(const void* A, const void* B, void* stream_out, int F, void* stream);
int eend_ffn_train_stream_f16(const void* X, int ldx, const void* wstream, const float* b1, const float* b2, const float* res, float alpha,
                              const float* gamma, const float* beta, float eps, float* out_f32, void* out_f16, void* hid_f16, void* xhat_f16,
                              float* rstd, int M, int F, const eend_dropout* drop_hidden, const eend_dropout* drop_out, void* stream);
int eend_ffn_bwd_data_stream_bf16(const void* dY, int ldy, const void* wstream, const void* hid_f16, float drop_scale, void* dH_bf16,
                                  float* g_f32, int M, int F, void* stream);
/* eend_spk_attn_f16 with dropout of the attention probabilities. */
int eend_spk_attn_train_f16(const void* qkv, void* O_f16, int B, int C, int Tp, int H, float scale,
                            const eend_dropout* drop, void* stream);

/* eend_conv1d_l2norm_f16 that also saves inv_norm [nseq*Tp] = 1/||conv output|| (FS model :40-41). */
int eend_conv1d_l2norm_train_f16(const void* X, const void* Wr, const float* bias, const int* ilens, float* out_f32,
                                 void* out_f16, float* inv_norm, int nseq, int Tp, int cin, int ktaps, int pad,
                                 void* stream);

/* Packed MHA in-projection for training: Q, K, V in BOTH head layouts (bf16 [nseq][H][Tp][64] and
 * [nseq][H][64][Tp]) -- the forward attention reads Q, K, Vt, its backward Q, K, V and, for windows beyond 512 frames
 * (the two kernels of the attention backward), Qt, Kt.  Qt / Kt may be NULL (not written) when Tp <= 512; Vt may be NULL when no consumer
 * reads it (the retention backward never does).  K = 256. */
int eend_inproj_heads_train_bf16(const void* A, int lda, const void* W, const float* bias, void* Q, void* Qt,
                                 void* K, void* Kt, void* V, void* Vt, int nseq, int Tp, int H, void* stream);

/* eend_attn_causal_bf16 that also writes lse [nseq][H][Tp]: the log2-domain log-sum-exp of every query row.
 * `drop`: dropout of the softmax probabilities (the normaliser stays un-dropped, as in torch). */
int eend_attn_causal_lse_bf16(const void* Q, const void* K, const void* Vt, void* O_f16, float* lse, int nseq, int H,
                              int Tp, int ldo, int mask_delay, int kv_len, float scale, const eend_dropout* drop,
                              void* stream);

/* Backward of the causal time-axis attention (torch autograd through nn.MultiheadAttention's core: FS model :147,
 * merge_tfm_encoder.py:379-385).  dO bf16 [nseq*Tp][ldo] (gradient w.r.t. the concatenated head outputs), O f16
 * the forward output; dQKV bf16 [nseq*Tp][ldg] receives dQ | dK | dV at columns 0 / 256 / 512 (+ h*64).
 * dOt_ws (bf16, nseq*Tp*256) and dh_ws (f32, nseq*H*Tp) are scratch.  scale_log2 as given to the forward
 * (its `scale` * log2 e); sq / sk: factors applied to dQ / dK (for the pre-scaled-q convention of
 * eend_attn_causal_bf16: scale_log2 = 1, sq = 1/sqrt(dh), sk = ln 2).  1 <= kv_len, q_len <= Tp (EEND_EINVAL otherwise, before any
 * launch).  `drop`: the forward's spec; O_f16 is the
 * forward output (computed from the dropped probabilities), which keeps D_i = <dO_i, O_i> valid. */
int eend_attn_causal_bwd_bf16(const void* Q, const void* Qt, const void* K, const void* Kt, const void* V,
                              const void* dO, int ldo, const void* O_f16, int ldout, const float* lse, void* dOt_ws,
                              float* dh_ws, void* dQKV, int ldg, int nseq, int H, int Tp, int mask_delay, int kv_len,
                              int q_len, float scale_log2, float sq, float sk, const eend_dropout* drop, void* stream);

/* Gradient GEMMs, bf16 operands, f32 accumulate (autograd of every torch.nn.Linear on the path):
 *   out = A W^T (+ bias)            -> bf16 [M][ldo]                 N % 128 == 0, K % 64 == 0 */
int eend_gemm_bf16(const void* A, int lda, const void* W, int ldw, const float* bias, void* out_bf16, int ldo,
                   int M, int N, int K, void* stream);
/*   out = drop_scale * (A W^T) where act != 0    (ReLU [+ dropout] backward; act = the saved forward activation, any
 *   2-byte float; drop_scale = 1/(1-p) of eend_linear_relu_train_f16, or 1) */
int eend_gemm_relu_bwd_bf16(const void* A, int lda, const void* W, int ldw, const void* act, int ldact,
                            void* out_bf16, int ldo, int M, int N, int K, float drop_scale, void* stream);
/*   out_f32 = (A W^T) * alpha + res_f32 (N = 256; the residual-gradient stream), optional bf16 copy */
int eend_gemm_acc_bf16(const void* A, int lda, const void* W, int ldw, const float* res_f32, float alpha,
                       float* out_f32, void* out_bf16, int M, int K, void* stream);

/* eend_gemm_acc_bf16 FOLLOWED by eend_layernorm_bwd_f32 of the post-norm site in front of the branch, in one launch (round 6): the
 * f32 gradient stream is read once and written once instead of twice each.
 *   g   = A W^T + g_f32                  (the data gradient of a K -> 256 linear joining the gradient w.r.t. a LayerNorm OUTPUT)
 *   dz  = rstd * (g gamma - mean(g gamma) - x_hat mean(g gamma x_hat))  -> ds_f32 (may alias g_f32), ds_bf16 = bf16 of dz under `drop`
 *   dgamma = sum_rows g x_hat, dbeta = sum_rows g, dbias (optional) = sum_rows of the masked dz      (overwritten, fixed summation order)
 * A bf16 [M][lda], W bf16 [256][ldw] (the transposed copy), x_hat f16 [M][256], ws >= ceil(M/64) * 768 floats. */
int eend_gemm_acc_lnbwd_bf16(const void* A, int lda, const void* W, int ldw, const float* g_f32, const void* xhat_f16, const float* rstd,
                             const float* gamma, float* ds_f32, void* ds_bf16, float* ws, long ws_floats, float* dgamma, float* dbeta,
                             float* dbias, int M, int K, const eend_dropout* drop, void* stream);

/* Conv1d(256,256,k) data gradient as an implicit GEMM over (tap, c_out) (autograd of FS model :40): dY bf16 slab,
 * Wd bf16 [c_in][k*c_out] with Wd[ci][tap'*c_out + co] = W[co][ci][k-1-tap']; frames >= src_lens[seq] of dY count as
 * zero; out_f32 rows t >= mask_lens[seq] are written as zero (the input was truncated to ilen, FS model :38-39). */
int eend_conv1d_dgrad_bf16(const void* dY, const void* Wd, const int* src_lens, const int* mask_lens, float* out_f32,
                           int nseq, int Tp, int cout, int ktaps, int pad, void* stream);

/* Weight gradient out[n][k] (row stride ld_out, k < K_out) (+)= scale * sum_m dY[m][n] X[m][k]; dY bf16 [M][lda],
 * X f16 (x_is_f16 & 1) or bf16 [M][ldb]; N, K % 128 == 0.  x_is_f16 & 2: X is stored in the blocked layout of
 * eend_ffn_train_stream_f16's hid (ldb = its full width F); x_is_f16 & 4: dY is (eend_ffn_bwd_data_stream_bf16's dH, lda = F). */
int eend_wgrad_bf16(const void* dY, int lda, const void* X, int ldb, int x_is_f16, long M, int N, int K, float* ws,
                    long ws_floats, float* out, int ld_out, int K_out, float scale, int accumulate, void* stream);
/* Host-only query: the output tile (128 / 256), the number of token splits and the rows per split (a multiple of 64) that
 * eend_wgrad_bf16 (with_bias = 0), eend_wgrad_bias[_grouped]_bf16 (with_bias = 1) and eend_conv1d_wgrad_bf16 (conv_cin = cin, N = 256,
 * K = ktaps * cin, M = nseq * Tp; 0 otherwise) take for these arguments on the current device -- the entries call the same planner.
 * Launches nothing and touches no device memory.  EEND_EINVAL where the entries refuse (N, K % 128, workspace under one split). */
int eend_wgrad_plan(long M, int N, int K, int conv_cin, long ws_floats, int with_bias, int* tile, int* nsplit, long* m_per_split);
/* eend_wgrad_bias_bf16 for N / group_rows linear layers that share the input X and whose (weight, bias) gradients sit equally spaced in
 * one buffer (the q / k / v / g projections of a retention module in the flat gradient buffer): rows g * group_rows .. of dY's N columns go
 * to out + g * group_stride (row stride K), their bias gradient to bias_out + g * group_stride.  One pass over X instead of N / group_rows,
 * one reduction launch each for weights and biases.  Overwrites (no accumulate). */
int eend_wgrad_bias_grouped_bf16(const void* dY, int lda, const void* X, int ldb, int x_is_f16, long M, int N, int K, float* ws,
                                 long ws_floats, float* out, float* bias_out, int group_rows, long group_stride, float scale, void* stream);
/* The same with the bias gradient on the side: bias_out[n] = scale * sum_m dY[m][n] (+ bias_out if accumulate), accumulated
 * from the dY tiles the kernel stages anyway instead of by a separate pass over dY (eend_colsum_f32).  ws needs
 * nsplit * (N*K + N) floats.  A blocked dY (x_is_f16 & 4) is summed by whole 16-row blocks: bias_out is the column sum of the M rows
 * only if the padding rows of the last block are zero (or M % 16 == 0, which is what the trainer requires); the weight gradient does
 * not depend on them (they meet rows of X beyond M, which read as zero). */
int eend_wgrad_bias_bf16(const void* dY, int lda, const void* X, int ldb, int x_is_f16, long M, int N, int K, float* ws,
                         long ws_floats, float* out, int ld_out, int K_out, float* bias_out, float scale, int accumulate, void* stream);
/* Conv1d weight gradient into the parameter's own (c_out, c_in, k) layout; tmp: f32 [c_out][k*c_in] scratch.  X frames at or beyond
 * ilens[seq] count as zero, every dY frame counts; Tp % 64 == 0.  ilens are trusted, not validated on the device: 0 <= ilens[seq] <= Tp. */
int eend_conv1d_wgrad_bf16(const void* dY, const void* X_f16, const int* ilens, int nseq, int Tp, int cin, int ktaps,
                           int pad, float* ws, long ws_floats, float* tmp, float* out, void* stream);
/* out[n] (+)= scale * sum_m Y[m][n]   (bias gradients); Y bf16 or f16 [M][ld]. */
int eend_colsum_f32(const void* Y, int ld, long M, int N, int is_bf16, float* ws, long ws_floats, float* out,
                    float scale, int accumulate, void* stream);

/* LayerNorm backward (autograd of torch.nn.LayerNorm): g = gradient w.r.t. the output (f32 [M][256]); writes the
 * gradient w.r.t. the input as f32 (ds_f32, may alias g) and bf16, and dgamma / dbeta [256].  `drop`: the spec of the
 * producing eend_linear_res_ln_train_f16 -- applied to the bf16 copy only (the branch gradient), not to ds_f32 (the
 * residual stream).  dbias (optional, [256]): column sums of that branch gradient = the bias gradient of the linear layer in
 * front of the LayerNorm (saves a separate pass over ds_bf16).
 * ws_floats >= 1024 * 768 (the row pass writes [blocks <= 1024][3][256] partials), whatever M. */
int eend_layernorm_bwd_f32(const float* g, const void* xhat_f16, const float* rstd, const float* gamma, float* ds_f32,
                           void* ds_bf16, float* ws, long ws_floats, float* dgamma, float* dbeta, float* dbias, long M,
                           const eend_dropout* drop, void* stream);

/* Head forward + standard_loss + their gradient in one pass (FS model :43,:60; train/utils/loss.py:119-125 with
 * label_delay = 0): labels f32 [B][T][C] (prepared: silence / speakers / none columns, zero padded), ilens / ncols
 * [B]; loss_out[0] = BCE loss; da f32 slab [(b*C+c)*Tp+t][256] = gradient w.r.t. the un-normalised attractors,
 * de f32 [B*Tp][256] = gradient w.r.t. the unit embeddings (overwritten); logits (optional) f32 [B][T][C].
 * With dlogits_in (f32 [B][T][C]: the caller's own d loss / d logits, e.g. torch autograd over the reference's
 * standard_loss) the loss part is skipped and that gradient is propagated (labels / ilens / ncols may be null).
 * ws_floats >= ceil(B * Tp / 4) (one loss partial per block of four frames). */
int eend_head_bce_f32(const float* emb, const float* attr, const float* labels, const int* ilens, const int* ncols,
                      float inv_frames, const float* dlogits_in, float* logits, float* da, float* de, float* ws,
                      long ws_floats, float* loss_out, int B, int T, int Tp, int C, void* stream);

/* x / ||x|| backward (FS model :41): y unit rows f32, dy f32, inv_norm from the forward -> dx bf16, rows t >= T zero. */
int eend_l2norm_bwd_bf16(const float* y, const float* dy, const float* inv_norm, void* dx_bf16, int B, int T, int Tp,
                         void* stream);

/* `convert` fan-out backward (FS model :113-114): gsum bf16 [B*Tp][256] = sum over speaker slots of g0,
 * dpc f32 [C][256] = sum over (b, t) of g0 per slot.  ws_floats >= 256 * C * 256 ([blocks <= 256][C][256] partials), whatever B * Tp; 1 <= C <= 12. */
int eend_convert_fanout_bwd_f32(const float* g0, void* gsum_bf16, float* ws, long ws_floats, float* dpc, int B, int Tp,
                                int C, void* stream);
/* mode 0: pc[c] = W[:, 256:] pe[c] + bias (the forward's per-slot constant); mode 1: dW[:, 256:] and dbias from dpc.
 * W / dW: the (256, 512) convert weight. */
int eend_convert_const_f32(int mode, const float* W, const float* bias, const float* pe, float* pc, const float* dpc,
                           float* dW, float* dbias, int C, void* stream);

/* Speaker-axis attention backward (merge_tfm_encoder.py:388-394): qkv f16 [rows][768] from the forward in-projection,
 * dO bf16 [rows][256] -> dqkv bf16 [rows][768]. */
int eend_spk_attn_bwd_bf16(const void* qkv_f16, const void* dO_bf16, void* dqkv_bf16, int B, int C, int Tp, int H,
                           float scale, const eend_dropout* drop, void* stream);

/* Train-mode BatchNorm1d statistics over the padded input (FS model :165-166): mean / biased var [F] of all B*T
 * frames (pad_value for frames beyond each length) and the running-statistics update (momentum, unbiased var).
 * ws_floats >= (ns + 1) * 2 * F with ns = min(ceil(B * T / 256), 512) row splits; B * T >= 2 (the unbiased variance). */
int eend_bn_train_stats_f32(const void* const* x_ptrs, const int* lens, float pad_value, float* ws, long ws_floats,
                            float* mean, float* var, float* run_mean, float* run_var, float momentum, int B, int T,
                            int F, void* stream);
/* BatchNorm weight / bias gradients from dy bf16 [B*Tp][ld] (gradient w.r.t. the BN output).  ws_floats >= ns * 2 * F, ns as above. */
int eend_bn_bwd_f32(const void* const* x_ptrs, const int* lens, float pad_value, const float* mean, const float* var,
                    float eps, const void* dy_bf16, int ld, float* ws, long ws_floats, float* dgamma, float* dbeta,
                    int B, int T, int Tp, int F, void* stream);

/* Embedding-consistency loss gradient (FS model :46-57): de f32 [B*Tp][256] += d loss / d emb. */
int eend_emb_consistency_bwd_f16(const void* emb_f16, const float* labels, const int* lens, float inv_count, float* de,
                                 int B, int T, int Tp, int D, int C, void* stream);

/* Optimiser on flat f32 buffers (FS-EEND/train_dia.py:83-100,153): sum of squares of the gradient; Adam step with
 * clip_grad_norm_ folded in (hp = {lr, 1-beta1^t, 1-beta2^t, max_norm} on the device).  eend_grad_sumsq_f32: ws_floats >= 1024 (one partial per block), whatever n. */
int eend_grad_sumsq_f32(const float* g, long n, float* ws, long ws_floats, float* out, void* stream);
int eend_adam_step_f32(float* p, const float* g, float* m, float* v, long n, const float* hp, const float* gsumsq,
                       float beta1, float beta2, float eps, void* stream);

/* Gradient accumulation over micro-batches (Lightning accumulate_grad_batches, FS-EEND/train_dia.py:151):
 * acc = (first ? 0 : acc) + scale * g on the flat buffers. */
int eend_grad_accumulate_f32(float* acc, const float* g, float scale, int first, long n, void* stream);

/* One entry of the weight re-layout table of eend_prep_weights: dst[a][b][c] (dims A x B x Cpad, zero for
 * c >= C) = convert(src[off + a*sa + b*sb + c*sc] * (a < nscale ? scale : 1)); dtype 0 f16, 1 bf16, 2 f32. */
typedef struct eend_prep_entry {
    const float* src;
    long off;
    void* dst;
    int A, B, C, Cpad;
    long sa, sb, sc;
    int dtype, nscale;
    float scale;
    int reserved;
} eend_prep_entry;
/* MFMA-operand copies of all parameters (f16 forward layouts, bf16 transposed backward layouts) in one launch;
 * `table` is a device array of n entries. */
int eend_prep_weights(const eend_prep_entry* table, int n, void* stream);

/* ======================================================================================================
 * LS-EEND TRAINING STEP (the LS half of BASELINE config 4: LS-EEND/train/oln_tfm_enc_dec_on_the_fly.py:52-92
 * training_step under train_dia_simu.py:97-117,159-173).  Same conventions as the FS-EEND training entries above.
 * Sequence slabs have Tp rows of which the first Tv (the reference's chunk-padded length, LS model :281-283) exist
 * in the reference; rows t >= Tv never enter a statistic and receive zero gradients.
 * ====================================================================================================== */

/* a = dropout(swish(z)) (conformer/feed_forward.py:51-52: Swish, nn.Dropout); z f16 [M][F] is the saved
 * pre-activation.  Backward, in place on the bf16 gradient: dz = da * keep * scale * swish'(z). */
int eend_swish_dropout_f16(const void* z_f16, void* a_f16, long M, int F, const eend_dropout* drop, void* stream);
int eend_swish_bwd_bf16(void* dz_bf16, const void* z_f16, long M, int F, const eend_dropout* drop, void* stream);

/* torch.nn.LayerNorm(256) forward keeping x_hat / 1/sigma for its backward (the pre-norm of the first sub-layer of a
 * Conformer block, feed_forward.py:48, applied to the previous block's output). */
int eend_layernorm_train_f16(const float* x, const float* gamma, const float* beta, float eps, void* y_f16,
                             void* xhat_f16, float* rstd, long M, void* stream);

/* LayerNorm backward, general form.  g: gradient w.r.t. the LayerNorm output, f32 or (g_is_bf16) bf16 [M][256].
 * ds_f32 (optional): the input gradient, overwritten or (accumulate) added to -- the latter is the pre-norm residual
 * block of conformer/modules.py:32-33, where the LayerNorm sits on the branch.  ds_bf16 (optional) = alpha16 *
 * dropout(input gradient), dbias (optional, needs ds_bf16) its column sums.  dgamma / dbeta [256] are overwritten.  ws_floats >= 1024 * 768, whatever M. */
int eend_layernorm_bwd2_f32(const void* g, int g_is_bf16, const void* xhat_f16, const float* rstd, const float* gamma,
                            float* ds_f32, int accumulate, void* ds_bf16, float alpha16, float* ws, long ws_floats,
                            float* dgamma, float* dbeta, float* dbias, long M, const eend_dropout* drop, void* stream);

/* Residual-stream gradient g f32 [M][256] -> gradient of a pre-norm branch output: ds_bf16 = alpha * dropout(g)
 * (ResidualConnectionModule module_factor, the branch's trailing nn.Dropout) and dbias [256] = its column sums.  ws_floats >= 1024 * 256, whatever M. */
int eend_resgrad_cast_bf16(const float* g, void* ds_bf16, float alpha, float* ws, long ws_floats, float* dbias, long M,
                           const eend_dropout* drop, void* stream);

/* eend_linear_res_scale_ln16_f16 for training: out_f32 = dropout(A W^T + bias) * alpha + res (un-normalised
 * residual stream), out_f16 = LayerNorm(out_f32) with x_hat / 1/sigma saved (the next sub-layer's pre-norm). */
int eend_linear_res_scale_ln_train_f16(const void* A, int lda, const void* W, int ldw, const float* bias,
                                       const float* res, float alpha, const float* gamma, const float* beta, float eps,
                                       float* out_f32, void* out_f16, void* xhat_f16, float* rstd, int M, int K,
                                       const eend_dropout* drop, void* stream);

/* ConformerConvModule, train mode (conformer/convolution.py:138-149).  P f16 [nseq*Tp][512] = pointwise-conv-1
 * output (value | gate); c = causal depthwise conv (k taps, zero left context) of value * sigmoid(gate), f16
 * [nseq*Tp][256], zero for t >= Tv. */
int eend_glu_dwconv_f16(const void* P_f16, const float* w, void* c_f16, int nseq, int Tp, int Tv, int k, void* stream);
/* BatchNorm1d batch statistics of c over the nseq*Tv valid frames, two-pass: stats f32 [513] = mean[256], M2[256]
 * (sum of squared deviations), n.  The triples of several ranks merge exactly (SyncBatchNorm, train_dia_simu.py:167).
 * ws_floats >= (nb + 1) * 256 with nb = min(ceil(nseq * Tv / 32), 4096) row blocks. */
int eend_bn_batch_stats_f16(const void* c_f16, float* ws, long ws_floats, float* stats, int nseq, int Tp, int Tv,
                            void* stream);
/* stats [R][513] of R ranks -> mean, biased var [256], n_out[1] = total frame count; running statistics updated
 * like torch BatchNorm1d / SyncBatchNorm in train mode (momentum, unbiased variance) when run_mean is given. */
int eend_bn_merge_f32(const float* stats, int R, float* mean, float* var, float* n_out, float* run_mean, float* run_var,
                      float momentum, void* stream);
/* s = swish(BatchNorm(c)) with the given batch statistics, f16 [M][256]. */
int eend_bn_swish_f16(const void* c_f16, const float* mean, const float* var, float eps, const float* gamma,
                      const float* beta, void* s_f16, long M, void* stream);
/* Backward of the two, pass 1: sums f32 [512] = per-channel sum of d_y and of d_y * c_hat over this rank's valid
 * frames (d_y = ds * swish'(BN(c))); also written as dbeta / dgamma.  Pass 2 (sums / n may be the all-reduced global
 * ones): ds <- d_c = gamma * rstd * (d_y - S1/n - c_hat * S2/n), zero for t >= Tv, in place (bf16).
 * eend_bn_swish_bwd_stats_bf16: ws_floats >= nb * 512, nb = min(ceil(nseq * Tv / 32), 4096). */
int eend_bn_swish_bwd_stats_bf16(const void* ds_bf16, const void* c_f16, const float* mean, const float* var, float eps,
                                 const float* gamma, const float* beta, float* ws, long ws_floats, float* sums,
                                 float* dgamma, float* dbeta, int nseq, int Tp, int Tv, void* stream);
int eend_bn_swish_bwd_apply_bf16(void* ds_bf16, const void* c_f16, const float* mean, const float* var, float eps,
                                 const float* gamma, const float* beta, const float* sums, const float* n_dev, int nseq,
                                 int Tp, int Tv, void* stream);
/* Depthwise conv + GLU backward: dP bf16 [nseq*Tp][512] (gradient of the pointwise-conv-1 output), dw f32 [256][k].
 * ws_floats >= nseq * ceil(Tp / 64) * 256 * k (one [256][k] partial per 64-frame strip); k in {7, 15, 16, 31}. */
int eend_dwconv_glu_bwd_bf16(const void* dc_bf16, const void* P_f16, const float* w, void* dP_bf16, float* ws,
                             long ws_floats, float* dw, int nseq, int Tp, int Tv, int k, void* stream);

/* eend_retention_chunk_f16 (chunk-resident kernel, L <= 512) that also saves rhat_f16 [nseq*Tp][ldo] = the per-head
 * normalised retention rows and rc f32 [nseq*Tp][H] = 1/sigma times the detached row scale (retention.py:163,180,185:
 * inner_scale / kv_scale carry no gradient). */
int eend_retention_chunk_train_f16(const void* Q, const void* K, const void* Kt, const void* Vt, const void* G,
                                   void* O_f16, void* rhat_f16, float* rc, void* St_ws, float* kv_ws, float* cscale_ws,
                                   float* sexp_ws, int nseq, int H, int Tp, int L, int ldo, int ldg, float gn_eps,
                                   int T_valid, void* stream);
/* MultiScaleRetention backward from the gradient of its out_proj input (f32 [nseq*Tp][256]; retention.py:196-228, chunk-recurrent form
 * :146-194): swish gate and per-head LayerNorm backward, then the linear-attention backward with the detached scales,
 *   dq_t = sum_{s<=t} (o~_t.v_s) k_s,  dk_s = sum_{t>=s} (o~_t.v_s) q_t,  dv_s = sum_{t>=s} (q_t.k_s) o~_t,
 * intra-chunk on bf16 MFMA tiles, across chunks through 64x64 prefix / suffix states.  Q..Vt: bf16 head layouts of
 * eend_inproj_heads_train_bf16 (k rows pre-scaled by dk^-1/2); dqkvg bf16 [nseq*Tp][ldq]: dq | sk*dk | dv | dg at
 * columns 0 / 256 / 512 / 768.  ot_ws: bf16 scratch [nseq*Tp*256]; kv_ws, g_ws: f32 [nseq*H*nc*4096];
 * St_ws: bf16 [nseq*H*nc*6*4096].  Envelope: that of eend_retention_chunk_train_f16 (L <= 512, L % 4 == 0) and nseq * nc <= 65535; anything
 * else is EEND_EINVAL, before anything is launched.  Only the row-major head layouts (Q, K, V) are read (the transposed fragments come out
 * of the LDS reads); there is no other form: Qt, Kt, Vt and ott_ws are ignored and may be NULL, and eend_inproj_heads_train_bf16 need not
 * write them. */
int eend_retention_bwd_bf16(const void* Q, const void* Qt, const void* K, const void* Kt, const void* V, const void* Vt,
                            const float* dctx_f32, const void* g_f16, int ldg, const void* rhat_f16, const float* rc,
                            void* ot_ws, void* ott_ws, float* kv_ws, float* g_ws, void* St_ws, void* dqkvg_bf16, int ldq,
                            int nseq, int H, int Tp, int L, int T_valid, float sk, void* stream);

/* Host-only query: the kernel one of the linear entry points takes for these arguments.  The entries and the query run the same
 * routing code -- the query passes stand-in addresses with the given NULL-ness and low address bits, and every launcher returns the
 * route in place of launching -- so a condition that moves in an entry moves here too (tests/test_linear_edges.py asserts the route
 * each of its cases was written for).  Launches nothing and touches no device memory.  Returns an EEND_ROUTE_* value;
 * EEND_ROUTE_REFUSED where the entry returns EEND_EINVAL; EEND_EINVAL for an unknown entry or args == NULL.
 * Fields an entry does not take are ignored: N of the N = 256 entries; lda / ldw / ldo of eend_convert_fanout_f16 (B = nseq,
 * slots = C) and ldo of the residual entries; M of the two head entries (nseq * Tp rows).  An address field is the pointer's low
 * four bits, or EEND_ROUTE_NULL for a NULL pointer: a, w, bias, res (f32 or f16 residual; pc of the fan-out), gamma, beta, out_f32,
 * out_f16 (every 2-byte destination of a head entry). */
#define EEND_ROUTE_REFUSED 0
#define EEND_ROUTE_SKINNY 1              /* skinny.hip, one wave per output feature (K <= 512) */
#define EEND_ROUTE_SKINNY_SPLITK 2       /* skinny.hip, one workgroup per output feature */
#define EEND_ROUTE_SKINNY_ROWGROUPS 3    /* skinny.hip f32, M > 16 in groups of 16 rows (K <= 512) */
#define EEND_ROUTE_SKINNY_ROWGROUPS_SPLITK 4
#define EEND_ROUTE_PROJ 5                /* proj.hip, X-resident */
#define EEND_ROUTE_GEMM128_STRAIGHT 6    /* gemm.hip 128x128 tile, K = 256 straight-line */
#define EEND_ROUTE_GEMM128_LOOPED 7      /* gemm.hip 128x128 tile, k-tile loop */
#define EEND_ROUTE_GEMM64X256 8          /* gemm.hip 64x256 whole-row tile */
#define EEND_ROUTE_CONVERT_ROWS 9        /* convert_rows.hip */
#define EEND_ROUTE_F32_MFMA 10           /* gemm_f32.hip (K <= 768) */
#define EEND_ROUTE_F32_MFMA_SPLITK 11    /* gemm_f32.hip, K split over the workgroup's waves */
#define EEND_ROUTE_NULL (-1)
enum eend_linear_entry {
    EEND_ENTRY_LINEAR_F16 = 0, EEND_ENTRY_LINEAR_GLU_F16, EEND_ENTRY_INPROJ_HEADS_BF16, EEND_ENTRY_RETENTION_PROJ_F16,
    EEND_ENTRY_LINEAR_RES_LN_F16, EEND_ENTRY_LINEAR_RES16_LN_F16, EEND_ENTRY_LINEAR_RES_SCALE_F16,
    EEND_ENTRY_LINEAR_RES_SCALE_LN16_F16, EEND_ENTRY_CONVERT_FANOUT_F16, EEND_ENTRY_LINEAR_STEP_F32,
    EEND_ENTRY_LINEAR_RES_LN_STEP_F32, EEND_ENTRY_LINEAR_RES_SCALE_LN_STEP_F32, EEND_ENTRY_COUNT
};
typedef struct eend_linear_route_args {
    int M, N, K, lda, ldw, ldo, act;
    int nseq, Tp, H, dh, C;
    int a, w, bias, res, gamma, beta, out_f32, out_f16;
} eend_linear_route_args;
int eend_linear_route(int entry, const eend_linear_route_args* args);

#ifdef __cplusplus
}
#endif
#endif /* EEND_HIP_H */
