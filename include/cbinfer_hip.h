/*
 * cbinfer_hip.h -- C ABI of libcbinfer_hip.so: hand-written HIP (gfx950 / MI355X) kernels for
 * CBinfer's change-based convolution hot path.
 *
 * This is the drop-in boundary.  Every entry point replaces one native launcher (or one torch op) of
 * the reference; the reference interface it replaces is cited as file:line relative to
 * /root/reference/pycbinfer.  Conventions (the reference has none of these):
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless stated otherwise;
 *   - the library allocates nothing and keeps no global state: every buffer is caller-owned;
 *   - every launcher takes the HIP stream to enqueue on (cbStream_t = hipStream_t, NULL = default
 *     stream) and never synchronises; it is safe to call while the stream is being graph-captured;
 *   - return value: 0 on success, a positive hipError_t if the launch failed, a negative CB_ERR_* for
 *     rejected arguments.  cbinfer_status_string() turns either into text;
 *   - launch geometry is chosen inside the library (the reference computes it in Python and passes
 *     six ints, conv2d_cg.py:106-111);
 *   - dtype: CB_F32 (cbconv2d_cg_backend.cu) or CB_F16 (cbconv2d_cg_half_backend.cu);
 *   - tensors are NCHW, batch 1, contiguous.  Index lists are int32 flat pixel indices y*W+x in
 *     ascending order.  "count" pointers are device int32 scalars holding the list length N, so that
 *     a whole frame can be enqueued without a host round trip; where a launcher takes both a host
 *     `numChanges` and a device `countDev`, countDev (if non-NULL) wins and numChanges is only the
 *     capacity the grid is sized for.
 *
 * The same library also exports the reference's own symbol names and signatures
 * (cbconv2d_{cg,cg_half,fg}_backend compat shims, cbinfer_amd/csrc/cb_compat.cpp) so the reference's cffi
 * cdef/dlopen (conv2d_cg.py:6-50, conv2d_fg.py:13-32) binds without change.
 */
#ifndef CBINFER_HIP_H
#define CBINFER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* cbStream_t; /* hipStream_t */

#define CB_F32 0
#define CB_F16 1
/* f32 tensors whose contraction runs as bf16x3 split products on the bf16 MFMA (f32 accumulation): every
 * operand x = hi + mid + lo (three bf16 terms, 24 significant bits), the six cross products above 2^-24 of
 * the product are summed -- f32-level accuracy at 16/6 of the f32 MFMA's rate.  Accepted wherever a `dtype`
 * selects the arithmetic of a gather-mode contraction (cbinfer_prep_weights, cbinfer_prepared_weights_bytes,
 * cbinfer_conv_changed[_from_mask], cbinfer_conv_accumulate_from_mask, cbinfer_cbconv2d_forward[_pooled,
 * _fg]); the tensors stay f32 and CB_F32 keeps the exact f32 fma chain. */
#define CB_F32S 2

#define CB_OK 0
#define CB_ERR_BADARG (-1)      /* null pointer, non-positive size, unsupported dtype */
#define CB_ERR_UNSUPPORTED (-2) /* shape outside what the kernels implement (e.g. kWHalf > 63) */

/* 1: round 1.  2: CB_F32S, row-segment / patch-staged contractions, fine-grained frame, fused 1x1 tail,
 * cbinfer_weights_ckkpad(Ckk, dtype).  3: fine-grained frame on the mask-driven contractions
 * (cbinfer_cbconv2d_forward_fg_masked and its parts).  4: split-state frame (cbinfer_split_*, several sequences
 * per launch), cbinfer_tail1x1_supported.  5: cbinfer_split_forward_tail (the 1x1 tail in the contraction's second
 * launch), cbinfer_split_tail_supported.  6: row-pair frame (cbinfer_*rowpairs*), cbinfer_dilate_change_indexes,
 * updateInputState = 2.  7: chained layers (cbinfer_*_after: the producer's change count ends an idle frame).
 * 8: the f32-EQUIVALENT (bf16-triple) form of the split-state frame: cbinfer_split3_*, CBINFER_SPLIT_X3,
 * weightScale == 0, cbNextDetect.arith.  9: cbinfer_hsplit_forward_group (cbHalfLayer / cbHalfNext: two layers of one
 * geometry per launch, the consumers' change detection in the producing launch); cbinfer_hsplit_* take contractions
 * of a single k-stage and up (1x1 layers on >= 64 channels).  10: cbinfer_split_*_next (a split-state layer's contraction
 * in window order carrying the pooled change detection of the layer behind the 2x2 pool).
 * 11 (unchanged): the general-geometry entry points (cbGeom, cbinfer_geom_*, cbinfer_*_geom) were ADDED under this
 * number -- new symbols break no caller, every earlier symbol keeps its signature and behaviour.  Likewise the
 * general pooling entry points (cbPool, cbinfer_pool_*, cbinfer_cbpool2d_forward), the sum (cbinfer_add_changed,
 * cbinfer_cbadd_forward) and the decoder operators (cbUpsample, cbinfer_upsample_supported,
 * cbinfer_cbupsample_forward, cbinfer_cbconcat_forward) and the transposed convolution (cbTGeom, cbinfer_tconv_*,
 * cbinfer_*_tconv, cbinfer_cbconvtranspose2d_forward), the depthwise convolution (cbinfer_dwconv_*,
 * cbinfer_cbdwconv2d_forward*), the element-wise functions (CB_PW_*, cbinfer_pointwise_supported,
 * cbinfer_pointwise_changed, cbinfer_cbpointwise_forward) and the grouped convolution (cbinfer_groupconv_*,
 * cbinfer_conv_changed_grouped, cbinfer_cbgroupconv2d_forward) and the rearrangements (cbRearrange, CB_REARRANGE_*,
 * cbinfer_rearrange_supported, cbinfer_rearrange_out_shape, cbinfer_cbrearrange_forward) and the per-pixel channel
 * reductions (CB_CH_*, cbinfer_chanreduce_supported, cbinfer_chanreduce_changed, cbinfer_cbchanreduce_forward) and the
 * resize to any size (cbResize, CB_RESIZE_*, cbinfer_resize_supported, cbinfer_cbresize_forward) and the padding (cbPad,
 * CB_PAD_*, cbinfer_pad_supported, cbinfer_pad_out_size, cbinfer_cbpad_forward) and the element-wise operators of two
 * maps (CB_BIN_*, cbinfer_binary_supported, cbinfer_binary_changed, cbinfer_cbbinary_forward) and the adaptive pools
 * (CB_ADAPT_*, cbinfer_adaptive_pool_*, cbinfer_cbadaptivepool2d_forward) and the collapse of the channel axis
 * (CB_CC_*, cbinfer_chancollapse_supported, cbinfer_chancollapse_changed, cbinfer_cbchancollapse_forward) and the
 * channel attention scale (CB_CS_*, cbinfer_chanscale_supported, cbinfer_chanscale_gate, cbinfer_chanscale_changed,
 * cbinfer_cbchanscale_forward) and the group norm (cbinfer_groupnorm_supported, cbinfer_groupnorm_partials,
 * cbinfer_groupnorm_stats, cbinfer_groupnorm_changed, cbinfer_cbgroupnorm_forward) and the peak suppression (cbPeaks,
 * cbinfer_peaks_supported, cbinfer_peaks_changed, cbinfer_cbpeaks_forward, cbinfer_peaks_list). */
#define CBINFER_ABI_VERSION 11

int cbinfer_abi_version(void);
const char* cbinfer_status_string(int status);

/* ---- geometry helpers (host, pure) --------------------------------------------------------- */
/* Row-padded bit mask layout used by the sync-free path: one uint64 word per 64 pixels of a row,
 * rows padded to whole words.  Returns words per row / total words for an H x W map. */
int cbinfer_mask_words_per_row(int W);
long cbinfer_mask_words(int H, int W);
/* Padded sizes of the prepared weight matrix (see cbinfer_prep_weights); the k-depth padding depends on
 * the dtype (fp32: whole 32-deep stages, fp16: stage pairs of 2 x 64).  Size buffers with
 * cbinfer_prepared_weights_bytes. */
int cbinfer_weights_kpad(int K);
int cbinfer_weights_ckkpad(int Ckk, int dtype);

/* ---- a1: change detection + dilation (+ feedback state update) ------------------------------
 * replaces changeDetection, conv2d_cg.py:100-122 -> cbconv2d_cg_backend.cu:83-100 (kernels :6-81),
 * half: cbconv2d_cg_half_backend.cu:10-88.
 * change(p) = OR_c |state[c,p] - in[c,p]| > th (strict; half: compared in half precision after one
 * rounding of the difference).  A changed pixel marks its (2kHHalf+1)x(2kWHalf+1) neighbourhood in
 * changeMap [H,W] int8 and, if updateInputState == 1, gets in[:,p] copied into state[:,p] (the feedback refresh).
 * updateInputState == 2 (round 4): EVERY pixel's in[:,p] is copied into state[:,p] in the same pass -- the
 * reference's prevInput.copy_(input) of a layer that is not in feedback mode (conv2d.py:234-236) without the
 * full-tensor copy launch behind the detection.
 * The map is zeroed by the library (the reference's caller does it, conv2d_cg.py:105). */
int cbinfer_change_detection(const void* input, void* state, int8_t* changeMap, int W, int H, int C,
                             int kHHalf, int kWHalf, float threshold, int updateInputState,
                             int dtype, cbStream_t stream);

/* Same computation, emitting the dilated mask as a row-padded BIT mask (wave ballot -> one word per
 * 64 pixels; bitsOut must be zero on entry, cbinfer_compact_bits re-zeroes a buffer for the next
 * frame).  This is the form the sync-free frame pipeline uses. */
int cbinfer_change_detection_bits(const void* input, void* state, uint64_t* bitsOut, int W, int H,
                                  int C, int kHHalf, int kWHalf, float threshold,
                                  int updateInputState, int dtype, cbStream_t stream);

/* ---- a2: stand-alone mask dilation ------------------------------------------------------------
 * replaces changePropagation, conv2d_cg.py:159-177 -> cbconv2d_cg_backend.cu:126-136 (kernel :101). */
int cbinfer_change_propagation(const int8_t* mapIn, int8_t* mapOut, int W, int H, int kHHalf,
                               int kWHalf, cbStream_t stream);

/* ---- a3: changed-index extraction (stream compaction) ----------------------------------------
 * replaces changeIndexesExtr[_python], conv2d_cg.py:200-213 (torch.nonzero(map.view(-1)).int()).
 * idxOut (capacity numel) receives the ascending flat indices of the non-zero bytes, countDev the
 * number of them.  scratchWords: caller-owned uint64 scratch of ceil(numel/64) words. */
int cbinfer_change_indexes_extr(const int8_t* changeMap, long numel, uint64_t* scratchWords,
                                int32_t* idxOut, int32_t* countDev, cbStream_t stream);

/* Compaction of a row-padded bit mask (from cbinfer_change_detection_bits) into flat indices y*W+x.
 * If clearBits is non-NULL that (other) mask buffer of the same geometry is zeroed for the next
 * frame.  If mapOut is non-NULL the mask is also expanded to an int8 [H,W] map (saveChangeMap). */
int cbinfer_compact_bits(const uint64_t* bits, int W, int H, int32_t* idxOut, int32_t* countDev,
                         uint64_t* clearBits, int8_t* mapOut, cbStream_t stream);

/* ---- a5: gather -> im2col rows of the changed pixels ------------------------------------------
 * replaces genXMatrix, conv2d_cg.py:239-261 -> cbconv2d_cg_backend.cu:163-173 (kernel :138-161).
 * columns [N, C*kH*kW] row-major, column (c*kH+ky)*kW+kx; zero outside the image. */
int cbinfer_gen_x_matrix(void* columns, const void* input, const int32_t* changeList, int kW, int kH,
                         int C, int W, int H, int numChanges, const int32_t* countDev, int dtype,
                         cbStream_t stream);

/* ---- a6/a7: the dense contraction ------------------------------------------------------------
 * replaces matrixMult_python, conv2d_cg.py:342-349 (torch matmul -> cuBLAS) and, with
 * transposeOut=1, also the transpose+contiguous of conv2d.py:247 / conv2d_cg.py:305.
 * Y = X[N,Ckk] . W[K,Ckk]^T + bias; Y is [N,K] (transposeOut=0) or [K,N] (transposeOut=1).
 * fp32: exact-f32 MFMA (v_mfma_f32_32x32x2_f32); fp16: f16 MFMA with f32 accumulation.
 * weightsPrepared is the buffer produced by cbinfer_prep_weights from the [K,C,kH,kW] filter bank:
 * the matrix padded to the MFMA tile grid, W[Kpad][CkkPad] with k contiguous, followed by a k->(c,ky,kx)
 * tap table (byte offset, dy, dx per k, which depends on the H x W of the feature map the layer runs
 * on); cbinfer_prepared_weights_bytes gives its size.  For a plain [K,Ckk] matrix pass C=Ckk,
 * kH=kW=H=W=1. */
long cbinfer_prepared_weights_bytes(int K, int C, int kH, int kW, int dtype);
int cbinfer_prep_weights(const void* weight, void* weightsPrepared, int K, int C, int kH, int kW,
                         int H, int W, int dtype, cbStream_t stream);
int cbinfer_matrix_mult(const void* X, const void* weightsPrepared, const void* bias, void* Y,
                        int N, const int32_t* countDev, int Ckk, int K, int transposeOut, int dtype,
                        cbStream_t stream);

/* ---- a8: scatter-back -------------------------------------------------------------------------
 * replaces updateOutput, conv2d_cg.py:292-313 -> cbconv2d_cg_backend.cu:191-197 (kernel :175-189).
 * output[k*HW + changeList[n]] = relu ? (v <= 0 ? 0 : v) : v with v = Yt[k*N + n]. */
int cbinfer_update_output(const void* Yt, void* output, const int32_t* changeList,
                          int numOutputPixel, int numChanges, const int32_t* countDev,
                          int nOutputPlane, int relu, int dtype, cbStream_t stream);

/* ---- a5+a6+a7+a8 fused: gather -> MFMA -> bias/ReLU -> scatter, no X / Y in HBM --------------
 * One launch replaces conv2d.py:240-251 (genXMatrix, matrixMult_python, transpose, updateOutput).
 * input is the layer state the gather reads from (conv2d.py:242 reads self.prevInput).
 * accumulate=1 adds to output instead of overwriting (no bias/ReLU): used by the deterministic
 * fine-grained variant (a12) where `input` holds the masked deltas.
 * clearBits (optional, clearWords words): a change bit mask this launch zeroes on the way, so the
 * next frame's cbinfer_change_detection_bits finds it clean (keeps the frame free of memset nodes).
 * workspace (optional, cbinfer_conv_workspace_bytes() bytes, ZERO on first use and left zero): lets the
 * persistent kernel split a short change list along k across workgroups (deterministic slab
 * reduction).  One workspace must not be used by two launches that can run concurrently. */
long cbinfer_conv_workspace_bytes(void);
int cbinfer_conv_changed(const void* input, const int32_t* changeList, int numChanges,
                         const int32_t* countDev, const void* weightsPrepared, const void* bias,
                         void* output, int C, int H, int W, int K, int kH, int kW, int relu,
                         int accumulate, uint64_t* clearBits, long clearWords, void* workspace,
                         int dtype, cbStream_t stream);

/* ---- a14 in one call: CBConv2d.forward_normal (conv2d.py:178-259) enqueued without a host sync --
 * detection(+dilation,+feedback) -> compaction -> [state copy] -> fused gather/MFMA/scatter.
 *   bits      : row-padded change mask (cbinfer_mask_words(H,W) words), zero on first use; left zero
 *               (may be NULL when haveIndexes=1)
 *   idx/count : capacity H*W int32 / one int32; on return (stream order) the frame's change list
 *   mapOut    : optional int8 [H,W] copy of the dilated mask (saveChangeMap)
 *   haveIndexes=1: idx/count were produced upstream (propChangeIndexes protocol): skip detection
 *   feedbackLoop=1: prevInput refreshed at changed pixels only; else, if copyInput, prevInput <- input
 *                   (copyInput=0: the gather reads `input` and the caller re-points its state at it,
 *                   conv2d.py:237-238)
 *   capN      : capacity of idx the fused kernel may assume (H*W, or the exact N if the caller
 *               synchronised);  workspace: see cbinfer_conv_changed */
int cbinfer_cbconv2d_forward(const void* input, void* prevInput, void* prevOutput, uint64_t* bits,
                             int32_t* idx, int32_t* countDev, int8_t* mapOut,
                             const void* weightsPrepared, const void* bias, int C, int H, int W,
                             int K, int kH, int kW, float threshold, int feedbackLoop,
                             int copyInput, int relu, int haveIndexes, int capN, void* workspace,
                             int selfCompact, int dtype, cbStream_t stream);

/* selfCompact=1 (fp32 or fp16, no mapOut, no upstream indexes, cbinfer_mask_words(H,W) <=
 * cbinfer_frame_mask_max_words()): `bits` is a zero-initialised buffer of cbinfer_frame_mask_bytes(H,W)
 * bytes holding two alternating masks and a device-side parity; the compaction launch disappears, the
 * fused kernel derives the change list from the mask by itself and still writes idx/countDev.
 * The two launches are also available on their own: */
long cbinfer_frame_mask_bytes(int H, int W);
/* byte offset, inside a frame mask buffer, of the COPY of the current frame's change mask (cbinfer_mask_words(H,W) words)
 * that a self-compacting contraction (selfCompact = 1) leaves behind: the producerMask a chained consumer's detection takes
 * (cbinfer_hsplit_forward[_group]); round 6 */
long cbinfer_frame_mask_copy_offset(int H, int W);
int cbinfer_frame_mask_max_words(void);
int cbinfer_change_detection_frame(const void* input, void* state, uint64_t* frameMasks, int W, int H,
                                   int C, int kHHalf, int kWHalf, float threshold,
                                   int updateInputState, int dtype, cbStream_t stream);
/* A feedback-mode layer behind a 2x2/stride-2 max pool (CBPoolMax2d, conv2d.py:24-84) with the pool
 * folded into its change detection: prePool [C,pH,pW] is the pool's INPUT; H x W is the pooled size
 * (pH/2 or ceil).  The pooled value is computed on the fly, compared with the state and written to the
 * state at the changed pixels; the pooled map itself is never materialised (the layer gathers from its
 * state).  Identical results to cbinfer_max_pool2d + cbinfer_cbconv2d_forward(feedbackLoop=1), one
 * launch less per frame. */
int cbinfer_change_detection_frame_pooled(const void* prePool, int pH, int pW, void* state,
                                          uint64_t* frameMasks, int W, int H, int C, int kHHalf,
                                          int kWHalf, float threshold, int dtype, cbStream_t stream);
int cbinfer_cbconv2d_forward_pooled(const void* prePool, int pH, int pW, void* prevInput,
                                    void* prevOutput, uint64_t* bits, int32_t* idx, int32_t* countDev,
                                    const void* weightsPrepared, const void* bias, int C, int H, int W,
                                    int K, int kH, int kW, float threshold, int relu, void* workspace,
                                    int dtype, cbStream_t stream);
int cbinfer_conv_changed_from_mask(const void* input, uint64_t* frameMasks, int32_t* idxOut,
                                   int32_t* countOut, const void* weightsPrepared, const void* bias,
                                   void* output, int C, int H, int W, int K, int kH, int kW, int relu,
                                   void* workspace, int dtype, cbStream_t stream);
/* Chains of change-based layers (conv -> conv, the producer's output buffer handed on untouched; no counterpart in
 * the reference, whose every layer scans its whole input, conv2d.py:228-233): upstreamCount is the device word the
 * PRODUCING layer's contraction left its change count in this frame (its countDev).  Zero there: the producer
 * rewrote no output pixel, this layer's input is bit for bit what it compared with its state last frame, the
 * detection could find nothing -- both launches return after one scalar load, countDev receives 0 (so that the
 * next layer of the chain is skipped the same way), masks, parity, state and output stay as they are; the copy of
 * the frame's mask behind the masks is left EMPTY, as the count is (a module handed it reads this frame's).  Non-zero
 * (or upstreamCount = NULL): cbinfer_cbconv2d_forward(selfCompact=1) exactly.  The CALLER guarantees the premise:
 * same input buffer and threshold as in this layer's previous frame, which followed the producer's previous frame;
 * no other writer to that buffer.  (cbinfer_amd/conv2d.py: CBConv2d._upstream_count checks it per frame.) */
int cbinfer_change_detection_frame_after(const int32_t* upstreamCount, const void* input, void* state,
                                         uint64_t* frameMasks, int W, int H, int C, int kHHalf, int kWHalf,
                                         float threshold, int updateInputState, int dtype, cbStream_t stream);
int cbinfer_conv_changed_from_mask_after(const int32_t* upstreamCount, const void* input, uint64_t* frameMasks,
                                         int32_t* idxOut, int32_t* countOut, const void* weightsPrepared,
                                         const void* bias, void* output, int C, int H, int W, int K, int kH, int kW,
                                         int relu, void* workspace, int dtype, cbStream_t stream);
int cbinfer_cbconv2d_forward_after(const int32_t* upstreamCount, const void* input, void* prevInput,
                                   void* prevOutput, uint64_t* bits, int32_t* idx, int32_t* countDev,
                                   const void* weightsPrepared, const void* bias, int C, int H, int W, int K, int kH,
                                   int kW, float threshold, int feedbackLoop, int copyInput, int relu,
                                   void* workspace, int dtype, cbStream_t stream);

/* ---- a5..a8 fused, row-segment form (fp32, small filter banks) ----------------------------------
 * Same contract as cbinfer_conv_changed (gather -> MFMA -> bias/ReLU -> scatter, replaces conv2d.py:240-251)
 * for layers cbinfer_rowconv_supported() accepts -- the 3->16 and 16->64 7x7 layers of the scene-labeling
 * net -- driven directly by the change BIT MASK: one workgroup per 64-pixel row segment (mask word) stages
 * the kH x (64+kW-1) input rows of every channel once in LDS and derives all taps from there.
 *   bits     : single row-padded mask (cbinfer_mask_words(H,W) words) as cbinfer_change_detection_bits
 *              (or cbinfer_change_detection_bits_pooled) fills it; zero on first use, left zero;
 *   arrive   : cbinfer_mask_words(H,W) int32, zero on first use, left zero;
 *   maskCopy : receives the frame's mask (cbinfer_compact_bits makes the index list from it on demand);
 *   prepared : cbinfer_rowconv_prep_weights' re-layout of the [K,C,kH,kW] filter bank
 *              (cbinfer_rowconv_prepared_bytes bytes).
 * cbinfer_cbconv2d_forward_rows is CBConv2d.forward_normal (conv2d.py:178-259) on it: detection (pooled on
 * the fly when prePool != NULL, see cbinfer_cbconv2d_forward_pooled) -> [state copy] -> contraction. */
int cbinfer_rowconv_supported(int C, int K, int kH, int kW);
long cbinfer_rowconv_prepared_bytes(int C, int K, int kH, int kW);
int cbinfer_rowconv_prep_weights(const float* weight, void* prepared, int K, int C, int kH, int kW,
                                 cbStream_t stream);
int cbinfer_conv_changed_rows(const float* state, uint64_t* bits, int32_t* arrive, uint64_t* maskCopy,
                              const void* prepared, const float* bias, float* output, int C, int H, int W,
                              int K, int kH, int kW, int relu, cbStream_t stream);
/* producerMask (may be NULL): the change mask (cbinfer_mask_words(pH,pW) words, this frame) of the layer that
 * wrote prePool; pooled pixels none of whose window pixels it rewrote are not even read.  ASSUMPTION the
 * caller must uphold: those pixels were compared against the SAME state with the SAME threshold on the previous
 * call (then they compare exactly as they did, i.e. not above it).  After a change of the threshold, or against a
 * state that was (re)allocated or written from outside, pass NULL for one frame (CBConv2d._forward_pooled does). */
int cbinfer_change_detection_bits_pooled(const void* prePool, int pH, int pW, const uint64_t* producerMask,
                                         void* state, uint64_t* bitsOut, int W, int H, int C, int kHHalf,
                                         int kWHalf, float threshold, int dtype, cbStream_t stream);
int cbinfer_cbconv2d_forward_rows(const float* input, const float* prePool, int pH, int pW,
                                  const uint64_t* producerMask, float* prevInput,
                                  float* prevOutput, uint64_t* bits, int32_t* arrive, uint64_t* maskCopy,
                                  const void* rowWeights, const float* bias, int C, int H, int W, int K,
                                  int kH, int kW, float threshold, int feedbackLoop, int copyInput, int relu,
                                  cbStream_t stream);

/* ---- a5..a8 fused, patch-staged form (fp32 tensors, CB_F32S arithmetic, wide layers) -----------
 * Same contract, buffers and mask protocol as cbinfer_conv_changed_rows for the layers with many channels
 * (16->64, 64->256 7x7): one workgroup per unit of R rows x 64 columns and 64 output channels; the input rows
 * under the unit are staged once per 8-channel chunk in LDS, pre-split into three bf16 planes, every tap reads
 * its 16-byte B fragment from there, the pre-split weights stream from L2 in MFMA fragment order
 * (cbinfer_blockconv_prep_weights, cbinfer_blockconv_prepared_bytes bytes). */
int cbinfer_blockconv_supported(int C, int K, int kH, int kW);
long cbinfer_blockconv_prepared_bytes(int C, int K, int kH, int kW);
int cbinfer_blockconv_prep_weights(const float* weight, void* prepared, int K, int C, int kH, int kW,
                                   cbStream_t stream);
int cbinfer_conv_changed_blocks(const float* state, uint64_t* bits, int32_t* arrive, uint64_t* maskCopy,
                                const void* prepared, const float* bias, float* output, int C, int H, int W,
                                int K, int kH, int kW, int relu, cbStream_t stream);
int cbinfer_cbconv2d_forward_blocks(const float* input, const float* prePool, int pH, int pW,
                                    const uint64_t* producerMask, float* prevInput,
                                    float* prevOutput, uint64_t* bits, int32_t* arrive, uint64_t* maskCopy,
                                    const void* blockWeights, const float* bias, int C, int H, int W, int K,
                                    int kH, int kW, float threshold, int feedbackLoop, int copyInput, int relu,
                                    cbStream_t stream);

/* ---- a9: change-based 2x2/stride-2 max pooling -----------------------------------------------
 * replaces maxPool2d, conv2d_cg.py:58-82 -> cbconv2d_cg_backend.cu:229-240 (kernel :199-227).
 * changeIndexes are INPUT-resolution pixel indices.  Unlike the reference, windows with
 * yo >= oH or xo >= oW (odd size, floor mode) are skipped instead of written out of bounds. */
int cbinfer_max_pool2d(const void* input, void* output, const int32_t* changeIndexes, int numChanges,
                       const int32_t* countDev, int C, int iH, int iW, int oH, int oW, int dtype,
                       cbStream_t stream);

/* ---- 8f-4: change indexes through a pool ------------------------------------------------------
 * The reference's CBPoolMax2d passes the INPUT-resolution index list on when propChangeIndexes is set
 * (conv2d.py:80-83), which is not usable at the pooled resolution.  This marks, for every changed input
 * pixel y*iW+x, bit (y/2, x/2) of a row-padded bit mask of the oH x oW pooled map (layout of
 * cbinfer_mask_words; bitsOut must be zero on entry); cbinfer_compact_bits turns it into the ascending
 * duplicate-free list of changed OUTPUT pixels and its device-side count. */
int cbinfer_pool_change_indexes(const int32_t* changeIndexes, int numChanges, const int32_t* countDev,
                                int iW, int oH, int oW, uint64_t* bitsOut, cbStream_t stream);
/* A CBConv2d fed propagated change indexes skips its own change detection whatever its filter size
 * (conv2d.py:180-190, :220; __init__.py:68-77) and recomputes exactly the listed pixels -- right for 1x1, short of
 * the filter's reach for k > 1.  This marks the filter support of every listed pixel (rows y +- kHHalf, columns
 * x +- kWHalf, clipped) in a row-padded bit mask of the H x W map (bitsOut zero on entry; cbinfer_compact_bits makes
 * the list): the output pixels the listed INPUT pixels reach -- what changeDetection's dilation
 * (cbconv2d_cg_backend.cu:62-72) marks when every listed pixel changed.  CBConv2d.dilatePropagatedIndexes. */
int cbinfer_dilate_change_indexes(const int32_t* changeIndexes, int numChanges, const int32_t* countDev, int H, int W,
                                  int kHHalf, int kWHalf, uint64_t* bitsOut, cbStream_t stream);

/* ---- a10-a12: fine-grained path ---------------------------------------------------------------
 * replaces changeDetectionFG, conv2d_fg.py:34-46 -> cbconv2d_fg_backend.cu:25-35 (kernel :7-23):
 * d = in - prev; changeMap = |d| > th; diffs = d where changed.  zeroUnchanged=1 additionally writes
 * diffs = 0 elsewhere (the reference leaves it uninitialised). */
int cbinfer_change_detection_fg(const float* input, const float* prevInput, float* diffs,
                                int8_t* changeMap, long numVals, float threshold, int zeroUnchanged,
                                cbStream_t stream);
/* replaces updateOutputFG, conv2d_fg.py:48-72 -> cbconv2d_fg_backend.cu:68-79 (kernel :37-66):
 * atomicAdd of w[:,ci,ky,kx]*d into the K*kH*kW outputs each changed value touches.
 * changeCoords: int64 flat coordinates into [C,H,W] (torch.nonzero, conv2d_fg.py:82). */
int cbinfer_update_output_fg(const float* diffs, const float* weight, float* output,
                             const int64_t* changeCoords, int K, int C, int H, int W, int kH, int kW,
                             long numChanges, cbStream_t stream);
/* a11 + a12 without the host round trip: the same scatter driven by an int32 coordinate list with a
 * device-side length, as cbinfer_change_indexes_extr produces it from the per-value change map (replaces
 * torch.nonzero, conv2d_fg.py:82, and its int64 list).  capacity: number of entries the grid may assume. */
int cbinfer_update_output_fg_list(const float* diffs, const float* weight, float* output,
                                  const int32_t* changeCoords, long capacity, const int32_t* countDev,
                                  int K, int C, int H, int W, int kH, int kW, cbStream_t stream);

/* ---- a14 (fine-grained) in one call: CBConv2d.forward_fg (conv2d.py:160-176) for the frames after the
 * first, enqueued without a host sync, atomics or coordinate list.
 *   cbinfer_change_detection_fg_frame: delta[c,p] = |in - prev| > th ? in - prev : 0 for EVERY value
 *     (dense fp32 [C,H,W] workspace); pixels with a changed value, dilated by the filter support, are ORed
 *     into the frame mask (layout of cbinfer_change_detection_frame); refreshState=1 also stores
 *     prev <- in wherever they differ (the reference's `prevInput = input`, conv2d.py:175, in place);
 *   cbinfer_conv_accumulate_from_mask: output += conv(weights, delta) at the masked pixels (same fused
 *     gather/MFMA kernel as cbinfer_conv_changed_from_mask, accumulating epilogue, no bias), and
 *     reluOut = relu(output) there if reluOut is non-NULL (conv2d.py:172-174);
 *   cbinfer_cbconv2d_forward_fg: both.  Deterministic.  fp32 only, like the reference's FG path. */
int cbinfer_change_detection_fg_frame(const float* input, float* prevInput, float* delta,
                                      uint64_t* frameMasks, int W, int H, int C, int kHHalf, int kWHalf,
                                      float threshold, int refreshState, cbStream_t stream);
int cbinfer_conv_accumulate_from_mask(const float* delta, uint64_t* frameMasks, int32_t* idxOut,
                                      int32_t* countOut, const void* weightsPrepared, float* output,
                                      float* reluOut, int C, int H, int W, int K, int kH, int kW,
                                      void* workspace, int dtype, cbStream_t stream);
int cbinfer_cbconv2d_forward_fg(const float* input, float* prevInput, float* delta, float* prevOutput,
                                float* reluOut, uint64_t* frameMasks, int32_t* idx, int32_t* countDev,
                                const void* weightsPrepared, int C, int H, int W, int K, int kH, int kW,
                                float threshold, int refreshState, void* workspace, int dtype,
                                cbStream_t stream);

/* The same frame on the mask-driven contractions (single mask + arrival counters + mask copy, as
 * cbinfer_conv_changed_rows / _blocks; weights prepared by cbinfer_rowconv_prep_weights /
 * cbinfer_blockconv_prep_weights): cbinfer_change_detection_fg_bits writes the delta tensor and ORs the dilated
 * touched-pixel mask into `bits`; cbinfer_conv_accumulate_rows / _blocks add conv(weights, delta) to `output`
 * at the mask's pixels (reluOut as above); cbinfer_cbconv2d_forward_fg_masked (blocks = 0 / 1): both. */
int cbinfer_change_detection_fg_bits(const float* input, float* prevInput, float* delta, uint64_t* bits, int W,
                                     int H, int C, int kHHalf, int kWHalf, float threshold, int refreshState,
                                     cbStream_t stream);
int cbinfer_conv_accumulate_rows(const float* delta, uint64_t* bits, int32_t* arrive, uint64_t* maskCopy,
                                 const void* prepared, float* output, float* reluOut, int C, int H, int W,
                                 int K, int kH, int kW, cbStream_t stream);
int cbinfer_conv_accumulate_blocks(const float* delta, uint64_t* bits, int32_t* arrive, uint64_t* maskCopy,
                                   const void* prepared, float* output, float* reluOut, int C, int H, int W,
                                   int K, int kH, int kW, cbStream_t stream);
int cbinfer_cbconv2d_forward_fg_masked(int blocks, const float* input, float* prevInput, float* delta,
                                       float* prevOutput, float* reluOut, uint64_t* bits, int32_t* arrive,
                                       uint64_t* maskCopy, const void* weightsPrepared, int C, int H, int W,
                                       int K, int kH, int kW, float threshold, int refreshState,
                                       cbStream_t stream);

/* ---- change-based 1x1 tail: conv1x1 -> [ReLU] -> conv1x1 at the changed pixels of the producing layer,
 * one launch.  Replaces two CBConv2d fed by propagated change indexes (sceneLabeling/modelLoader.py:41-44,
 * experiment 1) or the dense baseline modules 8..10 the other experiments keep (:45-47): a 1x1 layer's
 * output changes only where its input did.  output [C2,H,W] keeps every other pixel.  fp32.
 *   w1Prepared: w1 [C1,C0] re-laid out by cbinfer_tail1x1_prep (cbinfer_tail1x1_prepared_bytes bytes);
 *   C1 <= cbinfer_tail1x1_max_hidden(); w2 is the plain [C2,C1] matrix. */
int cbinfer_tail1x1_max_hidden(void);
int cbinfer_tail1x1_supported(int C0, int C1, int C2);   /* hidden width and LDS budget of cbinfer_tail1x1 */
long cbinfer_tail1x1_prepared_bytes(int C1, int C0);
int cbinfer_tail1x1_prep(const float* w1, float* w1Prepared, int C1, int C0, cbStream_t stream);
int cbinfer_tail1x1(const float* input, const int32_t* changeList, int numChanges, const int32_t* countDev,
                    const float* w1Prepared, const float* b1, const float* w2, const float* b2,
                    float* output, int C0, int C1, int C2, int H, int W, int relu1, int relu2,
                    cbStream_t stream);

/* ---- a1 + a5..a8 fused, SPLIT-STATE form (round 3; fp32 tensors, feedback mode, 16 / 32 / 64 input channels).
 * Replaces, per frame and layer, the launcher sequence changeDetection (cbconv2d_cg_backend.cu:83-100, with
 * updateInputState) -> torch.nonzero (conv2d_cg.py:200-209) -> genXMatrix (:138-173) -> matmul (conv2d_cg.py:
 * 342-349) -> updateOutput (:175-197) of CBConv2d.forward_normal (conv2d.py:220-251) -- for up to
 * CBINFER_SPLIT_MAX_SEQUENCES independent sequences (own state each, shared weights) in ONE launch per step.
 * The layer state is kept twice: prevInput [C,H,W] f32 (the module's buffer, refreshed at the changed pixels
 * as .cu:74-80 does) and a pixel-major pre-split f16-pair copy with a zero border (cbinfer_split_state_bytes;
 * cbinfer_split_state_init once, then maintained by cbinfer_split_detect), from which the contraction gathers
 * by LDS-DMA.  Arithmetic: x * 2^-4 = hi + lo * 2^-11 with f16 hi, lo (weights likewise, scaled by the power of
 * two weightScale that brings max|w| into [2^13, 2^14)); products hi.hi + (hi.lo + lo.hi) 2^-11 on the f16 MFMA,
 * f32 accumulation: |error| <= 5 * 2^-24 |a||b| per product (two operand roundings of 2^-23 and the dropped lo.lo
 * term; measured beside the exact f32 chain in tests/test_gpu_split.py).  Range of the state values: |x| < 2^20; a
 * refreshed value beyond it sets *rangeFlag, and from that launch on the contraction computes the sequence's tiles from
 * `state` in plain f32 (slow, right) until the caller moves the layer to another arithmetic.
 *   frameMasks : cbinfer_frame_mask_bytes(H,W) bytes, zero on first use: ONE mask (cbinfer_mask_words words) the
 *                detection ORs into and the contraction zeroes again; the second slot holds the (sharded) arrival
 *                counters of the contraction's workgroups
 *   idxOut     : change list of the frame (H*W ints), countOut its length -- by-products, ascending order
 *   workspace  : cbinfer_split_workspace_bytes(nSeq, ...) bytes, zero on first use (0 bytes / NULL for layers of
 *                fewer than 48 k-stages).  A deep contraction is ALWAYS the left-to-right sum of four partial sums
 *                over fixed k-ranges, whether these are computed by four workgroups (few tiles: slabs + a reduce
 *                launch) or one after the other by the same one (many tiles): a sequence gets the same bits alone
 *                and inside a batch.
 * mode bit 0 (CBINFER_SPLIT_POOLED): `input` is the tensor in FRONT of a 2x2/stride-2 max pool [C,pH,pW] (CBPoolMax2d
 * folded into the detection, see cbinfer_cbconv2d_forward_pooled); producerMask as for
 * cbinfer_change_detection_bits_pooled.  mode bit 1 (CBINFER_SPLIT_COPY_ALL, round 4): the layer is NOT in feedback
 * mode and keeps a copy of its input (feedbackLoop=False, copyInput=True: what convert() makes, conv2d.py:234-236,
 * `prevInput.copy_(input)`): the detection writes EVERY value of the frame into prevInput and into the pre-split
 * copy, not only those of the changed pixels -- the gather then reads this frame's input everywhere, as the
 * reference's does.
 *
 * The f32-EQUIVALENT form (round 5, "x3"): the same frame with every f32 operand kept as THREE bf16 terms, exactly
 * (x = b0 + b1 + b2, 8 significant bits each; bf16 has f32's exponent range: no scale, no range flag), and a product
 * made of the six term products above 2^-24 of it on the bf16 MFMA -- b0 w0 in one f32 accumulator, the five small
 * ones in a second, summed at the end: operands of 24 bits as conv2d_cg.py:342-349's sgemm has them, with FEWER
 * accumulation roundings than its fma chain (one per 16 k).  Records are 96 bytes per 16 channels, weights 6 KB per
 * stage and 32-row tile.  Selected by: the cbinfer_split3_* functions for the buffers (state bytes / init / rebuild,
 * prepared bytes / prep_weights), mode bit 3 (CBINFER_SPLIT_X3) of cbinfer_split_detect, and weightScale == 0 wherever
 * a frame function takes a weightScale (the triple form has none; cbinfer_split_forward[_tail,_fg] derive the
 * detection's mode bit from it).  rangeFlag is not used.  Workspace as for the pair form. */
#define CBINFER_SPLIT_MAX_SEQUENCES 8
#define CBINFER_SPLIT_POOLED 1
#define CBINFER_SPLIT_COPY_ALL 2
#define CBINFER_SPLIT_FG 4        /* cbinfer_split_detect only: the fine-grained frame's detection (cbinfer_split_forward_fg) */
#define CBINFER_SPLIT_X3 8        /* the split state holds bf16 triples (cbinfer_split3_state_bytes) */
typedef struct {
    const float* input;           /* this frame's layer input (or the pool's input) */
    float* state;                 /* prevInput [C,H,W] */
    void* splitState;             /* cbinfer_split_state_bytes(C,H,W,kH,kW) */
    uint64_t* frameMasks;
    const uint64_t* producerMask; /* pooled only; may be NULL */
    float* output;                /* prevOutput [K,H,W] */
    int32_t* idxOut;
    int32_t* countOut;
    int32_t* rangeFlag;           /* may be NULL */
    uint64_t* maskCopy;           /* may be NULL: receives this frame's change mask (cbinfer_mask_words words) at a
                                     fixed address -- the producerMask of the next layer's pooled detection */
    float* delta;                 /* fine-grained frame only (cbinfer_split_forward_fg): [C,H,W] f32, the thresholded
                                     differences of this frame (every value written) */
    float* reluOut;               /* fine-grained frame only, may be NULL: [K,H,W] kept at relu(output) */
} cbSplitSeq;
int cbinfer_split_supported(int C, int K, int kH, int kW);
int cbinfer_split_max_sequences(void);
long cbinfer_split_max_mask_words(int K);   /* cbinfer_mask_words(H,W) x sequences a launch of a K-channel layer takes */
long cbinfer_split_state_bytes(int C, int H, int W, int kH, int kW);
long cbinfer_split_prepared_bytes(int C, int K, int kH, int kW);
long cbinfer_split_workspace_bytes(int nSeq, int C, int H, int W, int K, int kH, int kW);
int cbinfer_split_prep_weights(const float* weight, void* prepared, int K, int C, int kH, int kW, int H, int W,
                               float weightScale, cbStream_t stream);
int cbinfer_split_state_init(void* splitState, int C, int H, int W, int kH, int kW, cbStream_t stream);
int cbinfer_split_state_rebuild(const float* state, void* splitState, int C, int H, int W, int kH, int kW,
                                int32_t* rangeFlag, cbStream_t stream);
long cbinfer_split3_state_bytes(int C, int H, int W, int kH, int kW);
long cbinfer_split3_prepared_bytes(int C, int K, int kH, int kW);
int cbinfer_split3_prep_weights(const float* weight, void* prepared, int K, int C, int kH, int kW, int H, int W,
                                cbStream_t stream);
int cbinfer_split3_state_init(void* splitState, int C, int H, int W, int kH, int kW, cbStream_t stream);
int cbinfer_split3_state_rebuild(const float* state, void* splitState, int C, int H, int W, int kH, int kW,
                                 cbStream_t stream);
int cbinfer_split_detect(const cbSplitSeq* seqs, int nSeq, int mode, int pH, int pW, int C, int H, int W,
                         int kH, int kW, float threshold, cbStream_t stream);
int cbinfer_split_conv(const cbSplitSeq* seqs, int nSeq, const void* prepared, const float* bias, int C, int H,
                       int W, int K, int kH, int kW, float weightScale, int relu, void* workspace, int forceSplit,
                       cbStream_t stream);
/* the other launches of a frame for several sequences at once (own tensors per sequence, shared weights):
 * cbinfer_change_detection_bits, cbinfer_conv_changed_rows and cbinfer_tail1x1 with arrays of nSeq pointers */
int cbinfer_change_detection_bits_batched(const float* const* inputs, float* const* states, uint64_t* const* bitsOut,
                                          int nSeq, int W, int H, int C, int kHHalf, int kWHalf, float threshold,
                                          int updateInputState, cbStream_t stream);
int cbinfer_conv_changed_rows_batched(const float* const* states, uint64_t* const* bits, int32_t* const* arrive,
                                      uint64_t* const* maskCopies, float* const* outputs, int nSeq,
                                      const void* prepared, const float* bias, int C, int H, int W, int K, int kH,
                                      int kW, int relu, cbStream_t stream);
typedef struct {
    const float* input;
    const int32_t* changeList;
    const int32_t* countDev; /* may be NULL: numChanges entries */
    float* output;
} cbTailSeq;
int cbinfer_tail1x1_batched(const cbTailSeq* seqs, int nSeq, int numChanges, const float* w1Prepared,
                            const float* b1, const float* w2, const float* b2, int C0, int C1, int C2, int H, int W,
                            int relu1, int relu2, cbStream_t stream);
int cbinfer_split_forward(const cbSplitSeq* seqs, int nSeq, int mode, int pH, int pW, const void* prepared,
                          const float* bias, int C, int H, int W, int K, int kH, int kW, float threshold,
                          float weightScale, int relu, void* workspace, cbStream_t stream);
/* The FINE-GRAINED frame (CBConv2d.forward_fg, conv2d.py:160-176 -> conv2d_fg.py:75-85: changeDetectionFG,
 * torch.nonzero, updateOutputFG's K*kH*kW atomicAdds per changed value, cbconv2d_fg_backend.cu:7-66) on the
 * split-state kernels (round 4), same contract as cbinfer_cbconv2d_forward_fg with refreshState = 1: prevInput
 * (`state`) takes the frame, `delta` the thresholded differences, `output` += conv(weights, delta) at the pixels of
 * the dilated any-channel mask, `reluOut` (optional) = relu(output) there; idxOut / countOut / maskCopy as for
 * cbinfer_split_forward.  No bias; fixed summation order.  pooled != 0: `input` is the tensor in front of a
 * 2x2/stride-2 max pool [C,pH,pW] (CBPoolMax2d folded into the detection; H x W the pooled size). */
int cbinfer_split_forward_fg(const cbSplitSeq* seqs, int nSeq, int pooled, int pH, int pW, const void* prepared, int C,
                             int H, int W, int K, int kH, int kW, float threshold, float weightScale, void* workspace,
                             cbStream_t stream);
/* The layer + the fused 1x1 tail behind it (sceneLabeling/modelLoader.py:45-47: the dense conv1x1 -> ReLU -> conv1x1
 * the experiments keep; cbinfer_tail1x1 evaluates it at the changed pixels) with the tail folded into the second
 * launch of a deep contraction: the launch that finishes the layer's outputs -- summing the partial tiles of a split
 * contraction -- keeps each group of 16 finished pixel columns in LDS and runs the tail on them.  Same arithmetic
 * as cbinfer_split_forward followed by cbinfer_tail1x1 (bit-identical outputs), one launch and the tail's gather
 * pass over prevOutput less.  cbinfer_split_tail_supported: deep contraction (>= 48 k-stages), K a multiple of 16
 * and a tail cbinfer_tail1x1_supported(K, C1, C2) takes with C1 >= 4; `bias` and `b1` 16-byte aligned. */
typedef struct {
    const float* w1Prepared;      /* cbinfer_tail1x1_prep */
    const float* b1;
    const float* w2;              /* [C2, C1] */
    const float* b2;
    int C1, C2, relu1, relu2;
    float* output[CBINFER_SPLIT_MAX_SEQUENCES];   /* [C2,H,W] per sequence */
} cbSplitTail;
int cbinfer_split_tail_supported(int C, int K, int kH, int kW, int C1, int C2);
int cbinfer_split_conv_tail(const cbSplitSeq* seqs, int nSeq, const void* prepared, const float* bias, int C, int H,
                            int W, int K, int kH, int kW, float weightScale, int relu, void* workspace, int forceSplit,
                            const cbSplitTail* tail, cbStream_t stream);
int cbinfer_split_forward_tail(const cbSplitSeq* seqs, int nSeq, int mode, int pH, int pW, const void* prepared,
                               const float* bias, int C, int H, int W, int K, int kH, int kW, float threshold,
                               float weightScale, int relu, void* workspace, int forceSplit, const cbSplitTail* tail,
                               cbStream_t stream);
/* cbinfer_split_forward_fg with the fused 1x1 tail in the contraction's second launch (round 5): that launch adds the
 * partial tiles' sum to `output`, keeps `reluOut`, and evaluates the tail on relu(output) when reluOut is given (what
 * the network hands the next module, conv2d.py:169-173), else on output.  Same bits as cbinfer_split_forward_fg
 * followed by cbinfer_tail1x1. */
int cbinfer_split_forward_fg_tail(const cbSplitSeq* seqs, int nSeq, int pooled, int pH, int pW, const void* prepared,
                                  int C, int H, int W, int K, int kH, int kW, float threshold, float weightScale,
                                  void* workspace, const cbSplitTail* tail, cbStream_t stream);

/* ---- fp16 layers on the split-state machinery (round 4): the frame of a CBConv2d in half precision
 * (cbconv2d_cg_half_backend.cu:10-88 change detection, :146-197 genXMatrix / updateOutput around an fp16 matmul;
 * conv2d.py:178-259) of 64 and more input channels (round 5: a count that is not a multiple of 64 -- OpenPose's 185 --
 * is padded to the next one in the pixel-major copy and the prepared weights: zero records, zero weights; the tensors
 * keep their C).  Beside prevInput [C,H,W] f16 the layer keeps a
 * pixel-major copy [Hp][Wp][C] f16 with a zero border (cbinfer_hsplit_state_bytes; no split -- the values are f16
 * already), so that a pixel's 64 channels of one tap are 128 contiguous bytes and both operands of the contraction go
 * global -> LDS by LDS-DMA; v_mfma_f32_32x32x16_f16, f32 accumulation, outputs rounded to f16 once (the arithmetic
 * of cbinfer_conv_changed with CB_F16, another summation order).  feedbackLoop = 1: both states take the changed
 * pixels' values (.cu:74-80 of the half backend); 0: every value of the frame (the layer keeps a copy of its input,
 * conv2d.py:234-236).  frameMasks: cbinfer_frame_mask_bytes(H,W) bytes, zero once; workspace:
 * cbinfer_hsplit_workspace_bytes (0 for fewer than 48 k-stages), zero once; upstreamCount: optional, as for
 * cbinfer_cbconv2d_forward_after.  idxOut / countOut / maskCopy as for cbinfer_split_forward.  pooled != 0: `input`
 * is the tensor in front of a 2x2/stride-2 max pool [C,pH,pW] (CBPoolMax2d folded into the detection; H x W the
 * pooled size), producerMask as for cbinfer_change_detection_bits_pooled.  pooled == 0 with a producerMask (round
 * 5): `input` is the output buffer of another change-based layer of the SAME resolution and producerMask that layer's
 * change mask of this frame (cbinfer_mask_words(H,W) words): 64-pixel segments it did not rewrite are skipped.  Valid
 * under the conditions of upstreamCount (the buffer is what this layer compared last frame wherever the producer
 * rewrote nothing; state not fresh or restored, threshold unchanged since the last frame). */
int cbinfer_hsplit_supported(int C, int K, int kH, int kW);
long cbinfer_hsplit_max_mask_words(int K);
long cbinfer_hsplit_state_bytes(int C, int H, int W, int kH, int kW);
long cbinfer_hsplit_prepared_bytes(int C, int K, int kH, int kW);
long cbinfer_hsplit_workspace_bytes(int C, int H, int W, int K, int kH, int kW);
int cbinfer_hsplit_prep_weights(const void* weight, void* prepared, int K, int C, int kH, int kW, int H, int W,
                                cbStream_t stream);
int cbinfer_hsplit_state_init(void* pixelState, int C, int H, int W, int kH, int kW, cbStream_t stream);
int cbinfer_hsplit_state_rebuild(const void* state, void* pixelState, int C, int H, int W, int kH, int kW,
                                 cbStream_t stream);
int cbinfer_hsplit_forward(const int32_t* upstreamCount, const void* input, int pooled, int pH, int pW,
                           const uint64_t* producerMask, void* state, void* pixelState, uint64_t* frameMasks,
                           void* output, int32_t* idxOut, int32_t* countOut, uint64_t* maskCopy, const void* prepared,
                           const void* bias, int C, int H, int W, int K, int kH, int kW, float threshold,
                           int feedbackLoop, int relu, void* workspace, cbStream_t stream);

/* ---- a GROUP of fp16 layers in one set of launches, each doing the change detection of its CONSUMERS (round 6,
 * ABI 9).  Two things the reference's structure offers and one launch per op hides:
 *  (1) layers chain through their state tensors -- a CBConv2d's input IS the prevOutput of the CBConv2d in front
 *      (conv2d.py:259 returns the state tensor itself; ('changeIndexes', out, idx) at :180-186, :256-259 hands the
 *      producer's change list on) -- so the producing launch knows every value the consumer's changeDetection
 *      (cbconv2d_cg_half_backend.cu:45-88) could find changed: those of the pixels it just recomputed.  For a consumer
 *      that keeps a COPY of its input (feedbackLoop = False, copyInput = True: conv2d.py:234-236, what convert() makes)
 *      the detection decomposes per VALUE -- compare with the consumer's prevInput in half precision (strict >), write
 *      the value into prevInput and into the consumer's pixel-major copy where it differs bit for bit, OR the dilated
 *      pixel into the consumer's frame mask -- and rides in the epilogue of the producing contraction (in the reduce
 *      launch of a contraction that was split along k).  The consumer then runs with detect = 0: its contraction alone.
 *      Valid exactly where the chained detection's producer-mask shortcut is (cbinfer_hsplit_forward above): the
 *      consumer compared this very buffer last frame into this very state with this very threshold; the caller falls
 *      back to detect = 1 for one frame otherwise.  Results are those of the separate launches, bit for bit.
 *  (2) the two branches of an OpenPose stage (poseDetection/openPose/PoseModel.py:122-137) are independent layers of
 *      ONE geometry: nLayers = 2 issues both as one persistent grid (items of both layers in one launch; own weights,
 *      states, masks, lists each; K may differ while the padded tile height agrees -- 38 and 19 outputs both pad to 64).
 * cbHalfLayer: one layer's tensors (all f16 unless said otherwise); next[]: up to CBINFER_HNEXT_MAX consumers of its
 * output (same H x W; in_channels = K).  workspace: cbinfer_hsplit_group_workspace_bytes(nLayers, ...), zero once. */
#define CBINFER_HGROUP_MAX 2
#define CBINFER_HNEXT_MAX 2
typedef struct {
    void* state;              /* the consumer's prevInput [K,H,W] */
    void* pixelState;         /* its pixel-major copy: cbinfer_hsplit_state_bytes(K, H, W, kH, kW) */
    uint64_t* frameMasks;     /* its frame mask */
    int kH, kW;               /* its filter: dilation, and the border geometry of pixelState */
    float threshold;
    int reserved;
} cbHalfNext;
typedef struct {
    const int32_t* upstreamCount;   /* optional (nLayers == 1 only), as for cbinfer_hsplit_forward */
    const void* input;              /* this frame's input (pooled: the pool's input); unused with detect = 0 */
    const uint64_t* producerMask;   /* optional, as for cbinfer_hsplit_forward */
    void* state;                    /* prevInput [C,H,W] */
    void* pixelState;
    uint64_t* frameMasks;
    void* output;                   /* prevOutput [K,H,W] */
    int32_t* idxOut;
    int32_t* countOut;
    uint64_t* maskCopy;             /* may be NULL */
    const void* prepared;           /* cbinfer_hsplit_prep_weights */
    const void* bias;               /* [K] f16, may be NULL */
    int K;
    float threshold;
    int relu;
    int detect;                     /* 1: this call runs the layer's change detection; 0: a producer's launch did */
    int nNext;
    int reserved;
    cbHalfNext next[CBINFER_HNEXT_MAX];
} cbHalfLayer;
long cbinfer_hsplit_group_workspace_bytes(int nLayers, int C, int H, int W, int K, int kH, int kW);
int cbinfer_hsplit_forward_group(const cbHalfLayer* layers, int nLayers, int pooled, int pH, int pW, int C, int H, int W,
                                 int kH, int kW, int feedbackLoop, void* workspace, cbStream_t stream);

/* ---- a5..a8 fused for a layer of few channels, ROW-PAIR form, with the NEXT layer's pooled change detection folded
 * in (round 4).  Replaces, per frame, the launcher sequence genXMatrix -> matmul -> updateOutput
 * (cbconv2d_cg_backend.cu:138-197, conv2d_cg.py:342-349) of a feedback-mode CBConv2d with at most 4 input and 16
 * output channels AND -- when `next` names the split-state layer (cbinfer_split_*) behind a 2x2/stride-2 max pool --
 * that layer's CBPoolMax2d (conv2d.py:49-78) + changeDetection with updateInputState (cbconv2d_cg_backend.cu:40-81):
 * a workgroup owns a row PAIR of a 64-pixel mask word, i.e. whole pooling windows, so it compares the pooled values
 * of the windows it rewrote with the next layer's state, refreshes that state (and its pre-split copy) and ORs the
 * dilated changes into the next layer's frame mask itself.  The next layer then runs cbinfer_split_conv[_tail] WITHOUT
 * cbinfer_split_detect.  Results are those of the separate launches (same predicate, same refresh, same mask); a
 * window none of whose pixels changed is skipped exactly as the producer-mask shortcut of cbinfer_split_detect skips
 * it, so the caller must fall back to the separate detection for one frame whenever that shortcut is not valid (fresh
 * or restored next-layer state, changed next-layer threshold).
 *   bits / maskCopy : as for cbinfer_conv_changed_rows (every workgroup zeroes the mask words of its own units); ctl:
 *                     unused (kept for the signature: one int32)
 *   prepared        : cbinfer_rowconv_prep_weights
 *   next            : may be NULL (or next->state NULL): no folding */
typedef struct {
    float* state;             /* the next layer's prevInput [K, H, W] */
    void* splitState;         /* its cbinfer_split_state_bytes(K, H, W, kH, kW) buffer (arith 1: cbinfer_split3_state_bytes) */
    uint64_t* frameMasks;     /* its frame mask (cbSplitSeq.frameMasks) */
    int32_t* rangeFlag;       /* may be NULL */
    int H, W, kH, kW;         /* the next layer's map size (behind the pool) and filter */
    float threshold;
    int arith;                /* 0: its split state holds f16 pairs, 1: bf16 triples (cbinfer_split3_*) */
} cbNextDetect;
typedef struct {                /* ONE sequence's tensors for the batched form (own state each, shared weights) */
    const float* state;         /* prevInput [C,H,W] */
    float* output;              /* prevOutput [K,H,W] */
    uint64_t* bits;
    uint64_t* maskCopy;         /* may be NULL */
    float* nextState;           /* the next layer's tensors as in cbNextDetect; NULL: no folding */
    void* nextSplitState;
    uint64_t* nextFrameMasks;
    int32_t* nextRangeFlag;     /* may be NULL */
} cbPairSeq;
int cbinfer_rowpairs_supported(int C, int K, int kH, int kW, int H, int W);
int cbinfer_conv_changed_rowpairs_batched(const cbPairSeq* seqs, int nSeq, const void* prepared, const float* bias,
                                          int C, int H, int W, int K, int kH, int kW, int relu,
                                          const cbNextDetect* next, cbStream_t stream);
/* round 6 (ABI 11): the row-pair launch WITH the layer's own change detection (replaces changeDetection +
 * updateInputState, conv2d_cg.py:100-122 / cbconv2d_cg_backend.cu:40-81, as a launch of its own in front of the contraction).
 * Every workgroup compares the patch of its row pair in `input` and `prevInput`, dilates the changed pixels into its own two
 * mask words (maskCopy takes them: there is no other mask) and multiplies the refreshed values.  prevInput is NOT written --
 * every workgroup must see the old state -- : the caller refreshes it behind this launch (cbinfer_refresh_state).  One
 * sequence, 7x7 filters; `next` as for cbinfer_conv_changed_rowpairs. */
int cbinfer_conv_rowpairs_detect(const float* input, const float* prevInput, float* prevOutput, uint64_t* maskCopy,
                                 const void* prepared, const float* bias, int C, int H, int W, int K, int kH, int kW,
                                 float threshold, int relu, const cbNextDetect* next, cbStream_t stream);
int cbinfer_refresh_state(const float* frame, float* state, int C, int H, int W, float threshold, cbStream_t stream);
int cbinfer_conv_changed_rowpairs(const float* state, uint64_t* bits, int32_t* ctl, uint64_t* maskCopy,
                                  const void* prepared, const float* bias, float* output, int C, int H, int W, int K,
                                  int kH, int kW, int relu, const cbNextDetect* next, cbStream_t stream);
int cbinfer_cbconv2d_forward_rowpairs(const float* input, float* prevInput, float* prevOutput, uint64_t* bits,
                                      int32_t* ctl, uint64_t* maskCopy, const void* prepared, const float* bias, int C,
                                      int H, int W, int K, int kH, int kW, float threshold, int relu,
                                      const cbNextDetect* next, cbStream_t stream);

/* ---- round 6: the same folding for a split-state PRODUCER (the 16 -> 64 layer of the scene-labeling network in front of
 * its second pool; replaces the consumer's cbinfer_split_detect launch, i.e. CBPoolMax2d conv2d.py:49-78 + changeDetection
 * conv2d_cg.py:100-122 / cbconv2d_cg_backend.cu:40-81 of the NEXT layer).  The contraction's work list is ordered by 2x2
 * pooling WINDOW (a tile = 16 windows touched by the change mask; only their changed pixels are computed, the others'
 * stored outputs take part in the maximum), so the workgroup that recomputes a window also owns its pooled pixel: it
 * compares the maximum with the next layer's state (strict >, all channels), refreshes that state and its split copy at the
 * changed pooled pixels and ORs their dilation into the next layer's frame mask.  The change list the layer hands out
 * (cbSplitSeq.idxOut) keeps the reference's row-major order.  Taken: one sequence, bf16-triple arithmetic (weightScale 0),
 * K <= 64 output channels (a multiple of 16), fewer than 48 k-stages, a mask of at most 1280 words; next as for the
 * row-pair kernel.  The caller falls back to the separate detection under the same conditions as there.
 *   cbinfer_split_conv_next    : cbinfer_split_conv + next (this layer's own detection was its producer's business)
 *   cbinfer_split_forward_next : cbinfer_split_forward + next */
/* (ABI 11) `side`: the feedback refresh of ANOTHER layer's state carried by this launch's workgroups without a work item --
 * for the row-pair layer in front when it ran cbinfer_conv_rowpairs_detect (which leaves its state alone). */
typedef struct {
    const float* frame;       /* that layer's input of this frame [C, H, W] */
    float* state;             /* its prevInput */
    int C, H, W;
    float threshold;
} cbSideRefresh;
int cbinfer_split_conv_next_refresh(const cbSplitSeq* seqs, int nSeq, const void* prepared, const float* bias, int C, int H,
                                    int W, int K, int kH, int kW, float weightScale, int relu, void* workspace,
                                    const cbNextDetect* next, const cbSideRefresh* side, cbStream_t stream);
/* ... and the same side job on a PIXEL-order contraction (the consumer does not run in window order): one sequence, the
 * bf16-triple arithmetic, K <= 64, fewer than 48 k-stages, at most 1280 mask words. */
int cbinfer_split_refresh_supported(int C, int K, int kH, int kW, int H, int W);
int cbinfer_split_conv_refresh(const cbSplitSeq* seqs, int nSeq, const void* prepared, const float* bias, int C, int H, int W,
                               int K, int kH, int kW, float weightScale, int relu, void* workspace,
                               const cbSideRefresh* side, cbStream_t stream);
int cbinfer_split_next_supported(int C, int K, int kH, int kW, int H, int W, const cbNextDetect* next);
int cbinfer_split_conv_next(const cbSplitSeq* seqs, int nSeq, const void* prepared, const float* bias, int C, int H,
                            int W, int K, int kH, int kW, float weightScale, int relu, void* workspace,
                            const cbNextDetect* next, cbStream_t stream);
int cbinfer_split_forward_next(const cbSplitSeq* seqs, int nSeq, int mode, int pH, int pW, const void* prepared,
                               const float* bias, int C, int H, int W, int K, int kH, int kW, float threshold,
                               float weightScale, int relu, void* workspace, const cbNextDetect* next,
                               cbStream_t stream);

/* ---- channel concatenation of batch-1 [Ci,H,W] tensors into [sum Ci,H,W] as ONE launch on the caller's stream
 * (round 6).  The reference's pose network does torch.cat(dim=1) between its stages
 * (poseDetection/openPose/PoseModel.py:131); with this entry point a frame of that network consists of library calls only
 * and can be replayed from a recorded launch program (pycbinfer.FrameProgram).  sources / channels: n (<= 4) device
 * pointers and channel counts (host arrays); output: [sum channels, H, W] of the same dtype; HW = H * W. */
#define CBINFER_CONCAT_MAX 4
int cbinfer_concat_channels(const void* const* sources, const int32_t* channels, int n, void* output, long HW, int dtype,
                            cbStream_t stream);

/* ---- general geometry: strided, dilated, freely padded, even-sized and bias-free convolutions (cb_geomconv.hip) ----
 * The reference has no counterpart: its CBConv2d asserts stride 1, dilation 1, padding k/2 and a bias
 * (conv2d.py:92-104).  Input map Hi x Wi, filter kH x kW, stride (sH, sW), zero padding (pH, pW), dilation (dH, dW);
 * output map Ho = (Hi + 2 pH - dH (kH-1) - 1) / sH + 1, Wo likewise (torch's formula).  Limits per axis: k <= 7,
 * s <= 4, d <= 8, p <= 64 -- beyond them CB_ERR_UNSUPPORTED, a non-positive entry or a filter that does not fit the
 * padded map CB_ERR_BADARG; nothing is launched then.  The geometry travels as one HOST struct.
 * Output pixels no tap reaches: with p > d (k-1) on an axis (nn.Conv2d(3, 8, 3, padding=3)) the output pixels with
 * o s - p + (k-1) d < 0, and their mirror at the far edge, have no tap inside the input map.  The detection never
 * lists them, so NO entry point below ever writes them (cbinfer_conv_changed_geom does when a caller's own list names
 * one: bias, ReLU applied).  Their dense value is the bias (after the ReLU), 0 without one, in every frame: the caller
 * initialises prevOutput / output with it -- CBConv2d does when it allocates the state. */
typedef struct cbGeom {
    int kH, kW, sH, sW, pH, pW, dH, dW;
} cbGeom;
/* host, pure: the output size (status as above; Ho / Wo untouched on failure) */
int cbinfer_geom_out_size(int Hi, int Wi, const cbGeom* geom, int* Ho, int* Wo);
/* Prepared weights of a general-geometry layer: W[Kpad64][CkkPad32] in the tensors' element type (k contiguous, zero
 * padded; dtype CB_F32S shares CB_F32's layout -- operands are split into bf16 triples on their way into LDS) followed
 * by the k -> tap table for an Hi x Wi input map: byte offset (c Hi Wi + (ky dH - pH) Wi + (kx dW - pW)) elemSize
 * relative to the base pixel (oy sH, ox sW), and the signed dy, dx of the border test.  0 bytes for a rejected geometry. */
long cbinfer_geom_prepared_weights_bytes(int K, int C, const cbGeom* geom, int dtype);
int cbinfer_geom_prep_weights(const void* weight, void* prepared, int K, int C, int Hi, int Wi, const cbGeom* geom,
                              int dtype, cbStream_t stream);
/* split-k workspace of cbinfer_conv_changed_geom: partial-tile slabs (scratch) followed by the tiles' arrival
 * counters -- the last 2048 bytes, ZERO on first use and left zero by every launch.  One per layer: two launches that
 * can run concurrently must not share one (see cbinfer_conv_changed). */
long cbinfer_geom_workspace_bytes(void);
/* Detection, one launch.  change(p) on the INPUT map exactly as cbinfer_change_detection (a1); updateInputState as
 * there (1: feedback refresh at the changed pixels, 2: state <- input wherever they differ, 0: state untouched).  The
 * EXACT footprint of the changed pixels -- output (oy, ox) iff one of its taps (oy sH - pH + ky dH, ox sW - pW + kx dW)
 * lies inside the input map and changed; a lattice for d > 1, the reference's box for unit geometry -- is ORed into
 * the mask the parity selects of a frame mask buffer of the OUTPUT map (cbinfer_frame_mask_bytes(Ho, Wo) bytes, zero on
 * first use).  A changed pixel no tap reaches still refreshes the state. */
int cbinfer_change_detection_geom(const void* input, void* state, uint64_t* frameMasks, int C, int Hi, int Wi,
                                  const cbGeom* geom, float threshold, int updateInputState, int dtype,
                                  cbStream_t stream);
/* Contraction, one launch: gather -> MFMA -> bias / ReLU -> scatter at the listed OUTPUT pixels, nothing else of
 * output [K, Ho, Wo] is written.  bias may be NULL.  dtype selects the arithmetic as in cbinfer_conv_changed (CB_F16;
 * CB_F32S: bf16 triples, six products, f32 accumulation; CB_F32: the exact f32 MFMA).  Either
 *   frameMasks != NULL: the list is derived from the frame mask cbinfer_change_detection_geom filled (ascending
 *     oy Wo + ox), written to idxOut (capacity Ho Wo) / countOut, the frame's mask is copied to
 *     cbinfer_frame_mask_copy_offset(Ho, Wo), the other mask is zeroed and the parity flipped for the next frame; or
 *   changeList / numChanges / countDev as in cbinfer_conv_changed (entries outside the map are ignored).
 * A short list is split along k over idle workgroups and summed in slice order (deterministic) when a workspace is
 * given. */
int cbinfer_conv_changed_geom(const void* input, const int32_t* changeList, int numChanges, const int32_t* countDev,
                              uint64_t* frameMasks, int32_t* idxOut, int32_t* countOut, const void* prepared,
                              const void* bias, void* output, int C, int Hi, int Wi, int K, const cbGeom* geom, int relu,
                              void* workspace, int dtype, cbStream_t stream);
/* The whole frame of a general-geometry CBConv2d enqueued without a host sync: the counterpart of
 * cbinfer_cbconv2d_forward (same feedbackLoop / copyInput contract; prevInput [C,Hi,Wi], prevOutput [K,Ho,Wo]).
 * haveIndexes=1 (idx / countDev produced upstream, capN their capacity) is accepted only where the output map is the
 * input map and not in feedback mode; CB_ERR_UNSUPPORTED otherwise. */
int cbinfer_cbconv2d_forward_geom(const void* input, void* prevInput, void* prevOutput, uint64_t* frameMasks,
                                  int32_t* idx, int32_t* countDev, const void* prepared, const void* bias, int C, int Hi,
                                  int Wi, int K, const cbGeom* geom, float threshold, int feedbackLoop, int copyInput,
                                  int relu, int haveIndexes, int capN, void* workspace, int dtype, cbStream_t stream);

/* ---- change-based pooling for any window: max and average (cb_pool2d.hip) ----------------------------
 * The reference pools 2x2 / stride 2 only (a9, cbinfer_max_pool2d above).  Input map Hi x Wi, window kH x kW, stride
 * (sH, sW), zero padding (pH, pW), ceilMode 0 / 1, dilation 1.  Limits per axis: 1 <= k <= 8, 1 <= s <= 8,
 * 0 <= p <= k / 2 (torch's own rule); beyond them CB_ERR_UNSUPPORTED.  Bad arguments and out-of-limit windows return
 * a status and launch nothing.  The window travels as one HOST struct.
 *   output size per axis: o = floor_or_ceil((n + 2 p - k) / s) + 1, and in ceil mode o -= 1 if (o - 1) s >= n + p
 *     (torch's rule); a map with n + 2 p < k on an axis is refused (CB_ERR_BADARG).
 *   listed output pixels: (oy, ox) iff its window -- rows oy sH - pH ... + kH - 1, columns likewise --, clipped to the
 *     input map, holds a changed input pixel.  With s > k an input pixel between two windows lists nothing.
 *   values: listed pixels are recomputed for all channels from the input tensor, every other output pixel keeps its
 *     bits.  CB_POOL_MAX: the maximum over the window's in-map pixels (padding never wins; a NaN wins, as in torch).
 *     Average: the in-map values summed in f32 in row-major window order (ky outer, kx inner), divided by ONE IEEE f32
 *     division, rounded to f16 once for CB_F16; the divisor is
 *     (min(y0 + kH, Hi + pH) - y0) (min(x0 + kW, Wi + pW) - x0) with y0 = oy sH - pH, x0 = ox sW - pW for
 *     CB_POOL_AVG_PAD (torch's count_include_pad=True) and the number of in-map pixels for CB_POOL_AVG_NOPAD. */
#define CB_POOL_MAX 0
#define CB_POOL_AVG_PAD 1
#define CB_POOL_AVG_NOPAD 2
typedef struct cbPool {
    int kH, kW, sH, sW, pH, pW, ceilMode, op;
} cbPool;
/* host, pure: 1 if the window is within the limits above, else 0 */
int cbinfer_pool_supported(const cbPool* pool);
/* host, pure: the output size (CB_OK; CB_ERR_UNSUPPORTED beyond the limits, CB_ERR_BADARG for a map smaller than the
 * window; Ho / Wo untouched on failure) */
int cbinfer_pool_out_size(int Hi, int Wi, const cbPool* pool, int* Ho, int* Wo);
/* Launch 1: the listed output pixels ORed into `bits`, a row-padded mask of the OUTPUT map (cbinfer_mask_words(Ho, Wo)
 * words, zero on entry).  Exactly ONE of the producer's changes is given, else CB_ERR_BADARG:
 *   changeIndexes (int32 flat indexes y Wi + x; capN entries at most, countDev the device-side length or NULL: capN
 *     is the length): one thread per (entry, output row it reaches), at most two 64-bit atomicOr per row; an entry
 *     outside the map is dropped; capN == 0 launches nothing; or
 *   inputMask (the producer's row-padded change mask of the INPUT map, cbinfer_mask_words(Hi, Wi) words; countDev
 *     must be NULL): one wave per output mask word, one ballot, no atomics -- the producer's list is never made. */
int cbinfer_pool_footprint(const int32_t* changeIndexes, int capN, const int32_t* countDev, const uint64_t* inputMask,
                           int Hi, int Wi, const cbPool* pool, uint64_t* bits, cbStream_t stream);
/* Launch 2: pooling at the pixels of `bits` -- input [C, Hi, Wi], output [C, Ho, Wo], dtype CB_F32 or CB_F16.  Every
 * word of `bits` is copied to maskCopy (the frame's mask, cbinfer_compact_bits makes the list from it on demand) and
 * zeroed in `bits`, which is thus ready for the next frame's launch 1.  No atomics; bits != maskCopy. */
int cbinfer_pool_changed(const void* input, void* output, uint64_t* bits, uint64_t* maskCopy, int C, int Hi, int Wi,
                         const cbPool* pool, int dtype, cbStream_t stream);
/* The whole frame of a change-based pool enqueued without a host sync: cbinfer_pool_footprint, then
 * cbinfer_pool_changed (the latter also for an empty list: the mask copy is written every frame).  All arguments are
 * checked before the first launch. */
int cbinfer_cbpool2d_forward(const void* input, void* outputState, const int32_t* changeIndexes, int capN,
                             const int32_t* countDev, const uint64_t* inputMask, uint64_t* bits, uint64_t* maskCopy,
                             int C, int Hi, int Wi, const cbPool* pool, int dtype, cbStream_t stream);

/* ---- change-based element-wise sum: out = a + b [, ReLU] (cb_add.hip) ---------------------------------
 * No counterpart in the reference.  a, b and the state `out` are [C, H, W], contiguous, one dtype (CB_F32 or CB_F16).
 * Every producer of this library leaves the pixels outside its change list bit for bit as they were, so a + b can
 * differ from last frame's only at the union of the operands' changes; recomputing there is the dense sum, exactly.
 *   listed pixels: the union of the two operands' changes.  Per operand the changes come as its row-padded change
 *     MASK (cbinfer_mask_words(H, W) words), as an int32 LIST (flat indexes y W + x; entries outside the map are
 *     dropped), or not at all: every pixel is listed then.  Bits of the row padding are never set.
 *   values: at listed pixels, every channel, out = a + b -- CB_F32: one IEEE addition; CB_F16: the sum formed in f32
 *     and rounded to f16 once (the correctly rounded f16 sum).  relu != 0: v > 0 ? v : 0, and a NaN stays a NaN.  Every
 *     other pixel of `out` keeps its bits.
 *   hand-on: maskCopy receives the frame's union mask every frame (all zeros for an empty frame: cbinfer_compact_bits
 *     makes the ascending list from it on demand); `bits`, the working mask (cbinfer_mask_words(H, W) words, zero on
 *     first use), is zero again when the launch ends.
 * Bad arguments (a null tensor or mask, C / H / W < 1, an unknown dtype, a negative list capacity, bits == maskCopy,
 * H W or 64 C beyond an int32) return CB_ERR_BADARG and launch nothing.
 *
 * The mask-driven launch.  maskA / maskB: the operand's change mask, or NULL; allA / allB != 0: the operand lists every
 * pixel.  The kernel ORs `bits`, maskA and maskB word by word itself (or forms the full row word); an operand with
 * neither contributes what `bits` holds on entry.  No atomics. */
int cbinfer_add_changed(const void* a, const void* b, void* out, const uint64_t* maskA, int allA, const uint64_t* maskB,
                        int allB, uint64_t* bits, uint64_t* maskCopy, int C, int H, int W, int relu, int dtype,
                        cbStream_t stream);
/* The whole frame of a change-based sum enqueued without a host sync.  Per operand X: maskX != NULL: mask form;
 * listX != NULL: list form (capX entries at most, countX the device-side length or NULL: capX is the length; capX == 0
 * launches nothing); both NULL: no change information, every pixel is listed; both set: CB_ERR_BADARG.  With both
 * operands in mask or all form the frame is ONE launch (cbinfer_add_changed); an operand in list form costs one launch
 * in front, which ORs its bits into `bits` (cbinfer_pool_footprint with a 1x1 / stride-1 window: one 64-bit atomicOr
 * per entry) -- skipped when the other operand lists every pixel anyway.  All arguments are checked before the first
 * launch. */
int cbinfer_cbadd_forward(const void* a, const void* b, void* outputState, const uint64_t* maskA, const int32_t* listA,
                          int capA, const int32_t* countA, const uint64_t* maskB, const int32_t* listB, int capB,
                          const int32_t* countB, uint64_t* bits, uint64_t* maskCopy, int C, int H, int W, int relu,
                          int dtype, cbStream_t stream);

/* ---- change-based element-wise function: out = act(x scale[c] + shift[c]) (cb_pointwise.hip) ------------
 * No counterpart in the reference.  x and the state `out` are [C, H, W], contiguous, one dtype (CB_F32 or CB_F16), two
 * different tensors.  Every producer of this library leaves the pixels outside its change list bit for bit as they were,
 * so f(x) can differ from last frame's only at the operand's changed pixels; recomputing there is the dense result.
 *   listed pixels: the operand's changes, as its row-padded change MASK (cbinfer_mask_words(H, W) words), as an int32
 *     LIST (flat indexes y W + x; entries outside the map are dropped), or not at all: every pixel is listed then.  Bits
 *     of the row padding are never set.
 *   values: at listed pixels, every channel c, all in f32 and rounded to f16 once at the end for CB_F16:
 *     affine (scale != NULL; scale, shift f32 [C], also for CB_F16): v = fl(fl(x scale[c]) + shift[c]) -- two correctly
 *       rounded operations, never one FMA;
 *     then `kind` with the f32 parameters p0, p1, every operation correctly rounded in the order written, comparisons
 *     instead of fmin / fmax (a NaN stays a NaN), clamp(t, lo, hi) = t < lo ? lo : (t > hi ? hi : t):
 *       CB_PW_IDENTITY     v
 *       CB_PW_RELU         v < 0 ? 0 : v                      (-0 and a NaN stay)
 *       CB_PW_HARDTANH     clamp(v, p0, p1)                   (ReLU6: p0 = 0, p1 = 6)
 *       CB_PW_LEAKY        v > 0 ? v : v p0
 *       CB_PW_PRELU        v > 0 ? v : slope[c] v             (slope f32 [C])
 *       CB_PW_HARDSWISH    v clamp(v + 3, 0, 6) / 6           (left to right, an IEEE division)
 *       CB_PW_HARDSIGMOID  clamp(v + 3, 0, 6) / 6
 *       CB_PW_SIGMOID      1 / (1 + expf(-v))
 *       CB_PW_SILU         v / (1 + expf(-v))
 *       CB_PW_TANH         tanhf(v)
 *       CB_PW_GELU         0.5 v (1 + erff(v 0.70710678118654752440f))                    (nn.GELU, approximate='none')
 *       CB_PW_GELU_TANH    0.5 v (1 + tanhf(0.79788456080286535588f (v + 0.044715f (v v v))))       (approximate='tanh')
 *       CB_PW_ELU          v > 0 ? v : p0 expm1f(v p1)        (ELU: p0 = alpha, p1 = 1; CELU: p0 = alpha, p1 = 1 / alpha)
 *       CB_PW_SELU         v > 0 ? 1.0507009873554805f v : 1.7580993408473766f expm1f(v)
 *       CB_PW_SOFTPLUS     t = v p0; t > p1 ? v : log1pf(expf(t)) / p0                     (p0 = beta, p1 = threshold)
 *       CB_PW_MISH         v tanhf(log1pf(expf(v)))
 *     The first seven are torch's CPU operators bit for bit; the others call the device's expf / tanhf / erff / expm1f /
 *     log1pf and are bounded against the same formula in float64.  The kinds 10..15 are unassigned
 *     and refused: the second group starts at 16.  Every other pixel of `out` keeps its bits; a pixel's bits depend
 *     neither on the other listed pixels nor on the operand's form.
 *   hand-on: maskCopy receives the frame's mask every frame (all zeros for an empty frame: cbinfer_compact_bits makes
 *     the ascending list from it on demand); `bits`, the working mask (cbinfer_mask_words(H, W) words, zero on first
 *     use), is zero again when the launch ends.
 * All arguments are checked before the first launch.  A null tensor or mask buffer, x == out, bits == maskCopy, the
 * operand's mask == bits or maskCopy, both a mask and a list, a count without a list, capN < 0, an unknown kind or dtype,
 * CB_PW_HARDTANH with p0 > p1, CB_PW_ELU with a non-finite p0 or p1, CB_PW_SOFTPLUS with p0 zero or non-finite or p1 a
 * NaN, CB_PW_PRELU without slope, scale without shift or the reverse, C / H / W < 1, H W or 64 C beyond an int32 return
 * CB_ERR_BADARG and launch nothing. */
#define CB_PW_IDENTITY 0
#define CB_PW_RELU 1
#define CB_PW_HARDTANH 2
#define CB_PW_LEAKY 3
#define CB_PW_PRELU 4
#define CB_PW_HARDSWISH 5
#define CB_PW_HARDSIGMOID 6
#define CB_PW_SIGMOID 7
#define CB_PW_SILU 8
#define CB_PW_TANH 9
#define CB_PW_GELU 16
#define CB_PW_GELU_TANH 17
#define CB_PW_ELU 18
#define CB_PW_SELU 19
#define CB_PW_SOFTPLUS 20
#define CB_PW_MISH 21
/* host, pure: 1 if `kind` is one of CB_PW_* and its parameters are usable (CB_PW_HARDTANH: p0 <= p1; CB_PW_ELU: p0 and
 * p1 finite; CB_PW_SOFTPLUS: p0 finite and not zero, p1 no NaN), else 0 */
int cbinfer_pointwise_supported(int kind, float p0, float p1);
/* The mask-driven launch.  mask: the operand's change mask, or NULL; all != 0: every pixel is listed.  The kernel ORs
 * `bits` and mask word by word itself (or forms the full row word); without a mask the operand contributes what `bits`
 * holds on entry.  No atomics. */
int cbinfer_pointwise_changed(const void* x, void* out, const uint64_t* mask, int all, uint64_t* bits, uint64_t* maskCopy,
                              int C, int H, int W, int kind, float p0, float p1, const float* scale, const float* shift,
                              const float* slope, int dtype, cbStream_t stream);
/* The whole frame enqueued without a host sync.  mask != NULL: mask form, ONE launch (cbinfer_pointwise_changed);
 * list != NULL: list form (capN entries at most, countDev the device-side length or NULL: capN is the length; capN == 0
 * launches nothing in front), one launch in front, which ORs the list's bits into `bits` (cbinfer_pool_footprint with a
 * 1x1 / stride-1 window: one 64-bit atomicOr per entry); both NULL: no change information, every pixel is listed, one
 * launch. */
int cbinfer_cbpointwise_forward(const void* x, void* outputState, const uint64_t* mask, const int32_t* list, int capN,
                                const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy, int C, int H, int W, int kind,
                                float p0, float p1, const float* scale, const float* shift, const float* slope, int dtype,
                                cbStream_t stream);

/* ---- change-based reductions over the channels of one pixel (cb_chanreduce.hip) -------------------------
 * No counterpart in the reference.  Channels-first LayerNorm, L2 normalisation, softmax and log-softmax: the output at a
 * pixel depends on the C values at that pixel and on nothing else.  x and the state `out` are [C, H, W], contiguous, one
 * dtype (CB_F32 or CB_F16), two different tensors.  Every producer of this library leaves the pixels outside its change
 * list bit for bit as they were, so the output can differ from last frame's only at the operand's changed pixels;
 * recomputing there is the dense result.
 *   listed pixels: the operand's changes, as its row-padded change MASK (cbinfer_mask_words(H, W) words), as an int32
 *     LIST (flat indexes y W + x; entries outside the map are dropped), or not at all: every pixel is listed then.  Bits
 *     of the row padding are never set.
 *   values: at listed pixels, all in f32, every operation correctly rounded in the order written and never contracted
 *     to an FMA; the result is rounded to f16 once at the end for CB_F16.
 *       sum16(v) of v_0 .. v_{C-1}: 16 slices, slice s holds the channels c = s mod 16; a slice's partial starts at +0
 *         and adds its channels in ascending c; the 16 partials are combined in the fixed tree p[2i] + p[2i+1], four
 *         levels (an empty slice contributes +0).
 *       max16(v): the same slices and tree with op(a, b) = b > a ? b : a, a slice starting at -inf (a NaN is never taken).
 *       CB_CH_LAYERNORM    mean = sum16(x) / C;  d_c = x_c - mean;  var = sum16(d_c d_c) / C;  r = 1 / sqrtf(var + eps);
 *                          y_c = d_c r;  with gamma, beta (f32 [C], both or neither): y_c = y_c gamma_c, then
 *                          y_c = y_c + beta_c                      (F.layer_norm over the channel axis, biased variance)
 *       CB_CH_L2NORM       s = sum16(x_c x_c);  t = sqrtf(s);  y_c = x_c / (t < eps ? eps : t)
 *                                                                                       (F.normalize(x, p=2, dim=1, eps))
 *       CB_CH_SOFTMAX      m = max16(x);  a_c = x_c - m;  e_c = expf(a_c);  s = sum16(e);  y_c = e_c / s
 *       CB_CH_LOGSOFTMAX   the same m, a, s;  y_c = a_c - logf(s)
 *     Division and sqrtf are the IEEE correctly rounded ones; expf / logf are the device's.  Every other pixel of `out`
 *     keeps its bits; a pixel's bits depend neither on the other listed pixels nor on the operand's form -- how slices
 *     and pixels are dealt to lanes depends on a word's popcount, the arithmetic does not.
 *   hand-on: maskCopy receives the frame's mask every frame (all zeros for an empty frame: cbinfer_compact_bits makes
 *     the ascending list from it on demand); `bits`, the working mask (cbinfer_mask_words(H, W) words, zero on first
 *     use), is zero again when the launch ends.
 * All arguments are checked before the first launch.  A null tensor or mask buffer, x == out, bits == maskCopy, the
 * operand's mask == bits or maskCopy, both a mask and a list, a count without a list, capN < 0, an unknown kind or dtype,
 * eps < 0 or a NaN, gamma without beta or the reverse, gamma with a kind other than CB_CH_LAYERNORM, C / H / W < 1, H W or
 * 64 C beyond an int32 return CB_ERR_BADARG and launch nothing.  There is no other limit on C. */
#define CB_CH_LAYERNORM 0
#define CB_CH_L2NORM 1
#define CB_CH_SOFTMAX 2
#define CB_CH_LOGSOFTMAX 3
/* host, pure: 1 if `kind` is one of CB_CH_*, C >= 1 and eps >= 0 (not a NaN), else 0 */
int cbinfer_chanreduce_supported(int kind, int C, float eps);
/* The mask-driven launch.  mask: the operand's change mask, or NULL; all != 0: every pixel is listed.  The kernel ORs
 * `bits` and mask word by word itself (or forms the full row word); without a mask the operand contributes what `bits`
 * holds on entry.  gamma / beta: plain pointers, NULL = absent.  No atomics. */
int cbinfer_chanreduce_changed(const void* x, void* out, const uint64_t* mask, int all, uint64_t* bits, uint64_t* maskCopy,
                               int C, int H, int W, int kind, float eps, const float* gamma, const float* beta, int dtype,
                               cbStream_t stream);
/* The whole frame enqueued without a host sync.  mask != NULL: mask form, ONE launch (cbinfer_chanreduce_changed);
 * list != NULL: list form (capN entries at most, countDev the device-side length or NULL: capN is the length; capN == 0
 * launches nothing in front), one launch in front, which ORs the list's bits into `bits` (cbinfer_pool_footprint with a
 * 1x1 / stride-1 window: one 64-bit atomicOr per entry); both NULL: no change information, every pixel is listed, one
 * launch. */
int cbinfer_cbchanreduce_forward(const void* x, void* outputState, const uint64_t* mask, const int32_t* list, int capN,
                                 const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy, int C, int H, int W, int kind,
                                 float eps, const float* gamma, const float* beta, int dtype, cbStream_t stream);

/* ---- change-based collapse of the channel axis: sum, mean, norm, max, min, argmax, argmin (cb_chancollapse.hip,
 * DESIGN 5.27) -------------------------------------------------------------------------------------------------------
 * The reference ends a scene-labelling frame with torch.max(y.cpu(), 1); it has no change-based form.  The output at a
 * pixel depends on the C values at that pixel alone, so -- as for the reductions above -- recomputing at the operand's
 * changed pixels is the dense result.  x is [C, H, W], contiguous, CB_F32 or CB_F16.  A call carries nOps = 1 .. 4 VALUE
 * kinds (CB_CC_SUM .. CB_CC_MIN) or exactly ONE ARG kind (CB_CC_ARGMAX, CB_CC_ARGMIN), packed into the int `ops`: 4 bits
 * per op, op k in bits 4k .. 4k+3, every bit from 4 nOps on zero.  (Plain ints: a recorded call holds no host array.)
 *   value kinds: the state `out` is [nOps, H, W] in x's dtype, channel k is op k; every channel value is read ONCE.
 *   arg kinds:   the state `out` is [H, W] int64.
 *   listed pixels, masks, list form: exactly as for cbinfer_cbchanreduce_forward.
 *   values: at listed pixels, all in f32, every operation correctly rounded in the order written, never contracted; one
 *     rounding to f16 at the end for CB_F16 (a sum beyond the format's range is the infinity of its sign).
 *       CB_CC_SUM      sum16(x)                              (sum16 as defined above: slices c mod 16, the fixed tree)
 *       CB_CC_MEAN     sum16(x) / (float)C
 *       CB_CC_NORM     sqrtf(sum16(x_c x_c))                 (torch.linalg.vector_norm(x, dim=1))
 *       CB_CC_ARGMAX / CB_CC_ARGMIN   the smallest index c whose value is maximal / minimal under torch's CPU order: a
 *                      NaN beats every number and the first NaN wins; +0 == -0 is a tie, the first index wins.  Taking
 *                      the better of two (value, index) pairs under this order is associative, so the result does not
 *                      depend on the tree: it is torch.argmax / torch.argmin (x, 1) exactly.
 *       CB_CC_MAX / CB_CC_MIN   the value AT that index, x[argmax] / x[argmin]: torch.max(x, 1).values -- -0 where -0
 *                      comes first in a +-0 tie, a NaN where any channel is one.
 *     Every other pixel of `out` keeps its bits; a pixel's bits depend neither on the other listed pixels nor on the
 *     operand's form.
 *   hand-on: maskCopy receives the frame's mask every frame; `bits`, the working mask, is zero again when the launch
 *     ends; bits of the row padding are never set.
 *   labelMask (arg kinds only, may be NULL; cbinfer_mask_words(H, W) words): EVERY word is written.  A bit is set iff
 *     the pixel is listed this frame and either every pixel is listed without change information (all form) or the new
 *     label differs from the label `out` held before the launch.  A second mask beside maskCopy, not instead of it.
 * All arguments are checked before the first launch.  A null tensor or mask buffer, x == out, bits == maskCopy, the
 * operand's mask == bits or maskCopy, labelMask equal to any other argument buffer, labelMask with a value kind, both a
 * mask and a list, a count without a list, capN < 0, nOps outside 1 .. 4, a kind above CB_CC_ARGMIN, bits of `ops` beyond
 * its nOps kinds, an arg kind with nOps != 1, an unknown dtype, C / H / W < 1, H W or 64 C beyond an int32 return
 * CB_ERR_BADARG and launch nothing.  There is no other limit on C. */
#define CB_CC_SUM 0
#define CB_CC_MEAN 1
#define CB_CC_NORM 2
#define CB_CC_MAX 3
#define CB_CC_MIN 4
#define CB_CC_ARGMAX 5
#define CB_CC_ARGMIN 6
/* host, pure: 1 if `ops` packs nOps (1 .. 4) value kinds or one arg kind and C >= 1, else 0 */
int cbinfer_chancollapse_supported(int ops, int nOps, int C);
/* The mask-driven launch.  mask: the operand's change mask, or NULL; all != 0: every pixel is listed.  The kernel ORs
 * `bits` and mask word by word itself (or forms the full row word); without a mask the operand contributes what `bits`
 * holds on entry.  No atomics. */
int cbinfer_chancollapse_changed(const void* x, void* out, const uint64_t* mask, int all, uint64_t* bits,
                                 uint64_t* maskCopy, uint64_t* labelMask, int C, int H, int W, int ops, int nOps,
                                 int dtype, cbStream_t stream);
/* The whole frame enqueued without a host sync.  mask != NULL: mask form, ONE launch (cbinfer_chancollapse_changed);
 * list != NULL: list form, one launch in front, which ORs the list's bits into `bits` (capN == 0 launches nothing in
 * front); both NULL: every pixel is listed, one launch. */
int cbinfer_cbchancollapse_forward(const void* x, void* outputState, const uint64_t* mask, const int32_t* list, int capN,
                                   const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy, uint64_t* labelMask, int C,
                                   int H, int W, int ops, int nOps, int dtype, cbStream_t stream);

/* ---- change-based upsampling and channel concatenation for decoders (cb_decoder.hip) -------------------
 * No counterpart in the reference.  Both operators are exact for the reason the sum is: every producer leaves the pixels
 * outside its change list bit for bit as they were, so the output can differ from last frame's only at the footprint of
 * the operands' changes.  Tensors are contiguous, CB_F32 or CB_F16; masks are row-padded (cbinfer_mask_words); an
 * int32 list holds flat indexes y W + x, entries outside the map are dropped; bits of the row padding are never set.
 *
 * Upsample.  input [C, Hi, Wi], the state `out` [C, Ho, Wo] with Ho = Hi sH, Wo = Wi sW; 1 <= sH, sW <= 8.
 *   source coordinates per axis (n input, N = n s output pixels, o the output coordinate), ALL IN INTEGERS:
 *     CB_UPSAMPLE_NEAREST: i0 = o / s.  The value is copied bit for bit; (oy, ox) is listed iff its source pixel is.
 *     CB_UPSAMPLE_BILINEAR: alignCorners == 0: num = max(2 o + 1 - s, 0), den = 2 s;  alignCorners == 1:
 *       num = o (n - 1), den = N - 1 (N == 1: num = 0, den = 1).  i0 = num / den, rho = num - i0 den,
 *       i1 = min(i0 + 1, n - 1), lambda = (float)rho / (float)den -- one IEEE division of two integers (exactly
 *       representable for extents below 2^24).  With a, b, c, d the values at (y0,x0), (y0,x1), (y1,x0), (y1,x1):
 *         out = (1 - ly) ((1 - lx) a + lx b) + ly ((1 - lx) c + lx d)
 *       evaluated in f32 (the compiler may contract to FMAs) and rounded to the dtype once.  (oy, ox) is listed iff any of
 *       its four source pixels is -- a zero weight does not matter, the mask handed on is a function of the input's
 *       mask alone.  torch derives the source coordinate from a float scale; its lambda drifts by about o 2^-24, so
 *       bilinear is pinned against float64 math, not bit-compared with torch.
 *   the input's changes: inputMask (over the INPUT map; one launch, the footprint gathered inside it), list (capN
 *     entries at most, countDev the device-side length or NULL: capN is the length; one launch in front, which ORs the
 *     footprint into `bits`; capN == 0 launches nothing in front), or neither: every output pixel is listed.
 *   hand-on: maskCopy (cbinfer_mask_words(Ho, Wo) words) receives the frame's mask every frame; `bits`, the working
 *     mask of the OUTPUT map (zero on first use), is zero again when the frame ends.  Unlisted pixels keep their bits.
 * Bad arguments (a null tensor or mask, C / Hi / Wi < 1, an unknown dtype or mode, a scale outside 1..8, capN < 0, both
 * a mask and a list, a count without a list, inputMask == bits or maskCopy, bits == maskCopy, Ho Wo or 64 C beyond an
 * int32) return CB_ERR_BADARG and launch nothing. */
#define CB_UPSAMPLE_NEAREST 0
#define CB_UPSAMPLE_BILINEAR 1
typedef struct cbUpsample {
    int sH, sW, mode, alignCorners;
} cbUpsample;
/* host, pure: 1 if scales, mode and alignCorners (0 / 1) are within the limits above, else 0 */
int cbinfer_upsample_supported(const cbUpsample* up);
/* The whole frame of a change-based upsampling enqueued without a host sync. */
int cbinfer_cbupsample_forward(const void* input, void* outputState, const uint64_t* inputMask, const int32_t* list,
                               int capN, const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy, int C, int Hi,
                               int Wi, const cbUpsample* up, int dtype, cbStream_t stream);
/* Concat.  n = 2..4 operands sources[k] of [channels[k], H, W], the state `out` [sum channels, H, W].  The arrays are
 * HOST arrays of n entries; masks / lists / caps / counts may be NULL (no operand has one).  Per operand k: masks[k]:
 * mask form; lists[k]: list form (caps[k] entries at most, counts[k] the device-side length or NULL); neither: every
 * pixel is listed.  Operand k's channels are copied bit for bit at operand k's listed pixels ONLY -- an operand that
 * did not change is not touched --; every other value of `out` keeps its bits.  maskCopy receives the UNION of the
 * operands' masks every frame.  `bits` holds n working masks (n cbinfer_mask_words(H, W) words, operand k's at
 * bits + k words; zero on first use, zero again when the frame ends).  With every operand in mask or all form the
 * frame is ONE launch; an operand in list form costs one launch in front (cbinfer_pool_footprint with a 1x1 window).
 * Bad arguments (a null tensor or array, n outside 2..4, channels / H / W < 1, an unknown dtype, a capacity < 0, both a
 * mask and a list for one operand, a count without a list, an operand mask or maskCopy inside `bits`, an operand mask
 * == maskCopy, H W or 64 sum channels beyond an int32) return CB_ERR_BADARG and launch nothing. */
int cbinfer_cbconcat_forward(const void* const* sources, const int32_t* channels, int n, void* outputState,
                             const uint64_t* const* masks, const int32_t* const* lists, const int32_t* caps,
                             const int32_t* const* counts, uint64_t* bits, uint64_t* maskCopy, int H, int W, int dtype,
                             cbStream_t stream);

/* ---- change-based resize to any size (cb_resize.hip) -----------------------------------------------------
 * No counterpart in the reference.  F.interpolate to a size or by any scale, up or down: an output pixel reads 1, 2x2 or
 * 4x4 input pixels at coordinates that are a rational function of its own, so -- every producer leaves the pixels outside
 * its change list bit for bit as they were -- the output can differ from last frame's only at the footprint of the
 * input's changes.  Tensors, masks, lists and the frame (inputMask / list / neither, maskCopy, bits) are
 * cbinfer_cbupsample_forward's: input [C, Hi, Wi], the state `out` [C, Ho, Wo], CB_F32 or CB_F16; the mask form is one
 * launch, the list form one more in front, which ORs the footprint into `bits` (one thread per entry and candidate
 * output row, every candidate tested with the source rule, at most two 64-bit atomicOr per row).
 *
 * THIS SECTION IS THE SPECIFICATION; tests/resize_cases.py is its numpy twin and equals the kernel bit for bit.
 *   source coordinates per axis, ALL IN INTEGERS (exact; within the limits below an int32 holds every intermediate):
 *   n the input extent, N the output extent, o the output coordinate, a / b the step in input pixels per output pixel
 *   (aH / bH, aW / bW), handed in by the host:
 *     CB_RESIZE_NEAREST:        one tap i = min(o a / b, n - 1).
 *     CB_RESIZE_NEAREST_EXACT:  one tap i = min((2 o + 1) a / (2 b), n - 1).
 *     CB_RESIZE_BILINEAR, CB_RESIZE_BICUBIC:
 *       alignCorners == 0: num = (2 o + 1) a - b, den = 2 b;
 *       alignCorners == 1: num = o (n - 1), den = N - 1 (N == 1: num = 0, den = 1), whatever a / b is.
 *       BILINEAR: num = max(num, 0), i0 = num / den, rho = num - i0 den, the taps i0 and i0 + 1, both clamped to n - 1
 *         (within the limits below i0 <= n - 1 by itself).
 *       BICUBIC: num is not clamped, i0 = floor(num / den) (floor division for a negative num), rho = num - i0 den, the
 *         taps i0 - 1 .. i0 + 2, each clamped to [0, n - 1].
 *       t = (float)rho / (float)den, ONE correctly rounded division of two exactly represented integers.
 *   values: the nearest kinds copy bit for bit.  Otherwise everything is f32, every operation written below is rounded on
 *   its own (round to nearest even, never an FMA), in exactly this order, and the result is rounded to the dtype once:
 *     weights of an axis  BILINEAR: w0 = 1 - t, w1 = t.
 *                         BICUBIC, A = -0.75:  far(s) = ((A s - 5 A) s + 8 A) s - 4 A   evaluated as
 *                           m = A * s; m = m - (-3.75); m = m * s; m = m + (-6); m = m * s; m - (-3);
 *                         near(u) = ((A + 2) u - (A + 3)) u u + 1   evaluated as
 *                           m = 1.25 * u; m = m - 2.25; m = m * u; m = m * u; m + 1;
 *                         w0 = far(t + 1), w1 = near(t), w2 = near(1 - t), w3 = far(2 - t).
 *     a row  r_k = ((wx0 p(k,0) + wx1 p(k,1)) + wx2 p(k,2)) + wx3 p(k,3)  with p(k,j) the input at (tap row k, tap
 *            column j): the products in ascending j, summed left to right (BILINEAR: the first two terms);
 *     out    = ((wy0 r_0 + wy1 r_1) + wy2 r_2) + wy3 r_3, likewise.
 *   A pixel's bits therefore depend neither on the other listed pixels nor on the operand's form.  torch derives the
 *   source coordinate from a float scale, so bilinear and bicubic follow F.interpolate to about 1e-5 and are not
 *   bit-compared with it; the nearest kinds are bit-identical to torch.
 *   footprint: (oy, ox) is listed iff any of its 1 / 2x2 / 4x4 clamped taps is listed -- a zero weight does not
 *   matter, the mask handed on is a function of the input's mask alone.  An input pixel that no output reads
 *   (downscaling) lists nothing.
 * Limits (cbinfer_resize_supported): per axis 1 <= a, b <= 4096, 1/8 <= a / b <= 8, n / 8 <= N <= 8 n, n and N below
 * 2^15, and with alignCorners == 0 N a <= n b -- the output map does not reach beyond the input, as with torch's
 * a / b = n / N (size) or 1 / scale_factor with N = floor(n scale_factor); mode one of the four, alignCorners 0 or 1 and
 * 0 for the nearest kinds.
 * Bad arguments (a null tensor or mask, C / Hi / Wi < 1, an unknown dtype, a cbResize beyond the limits, capN < 0, both a
 * mask and a list, a count without a list, inputMask == bits or maskCopy, bits == maskCopy, Ho Wo or 64 C beyond an
 * int32) return CB_ERR_BADARG and launch nothing. */
#define CB_RESIZE_NEAREST 0
#define CB_RESIZE_NEAREST_EXACT 1
#define CB_RESIZE_BILINEAR 2
#define CB_RESIZE_BICUBIC 3
typedef struct cbResize {
    int Ho, Wo, aH, bH, aW, bW, mode, alignCorners;
} cbResize;
/* host, pure: 1 if the resize of an Hi x Wi map is within the limits above, else 0 */
int cbinfer_resize_supported(const cbResize* rs, int Hi, int Wi);
/* The whole frame of a change-based resize enqueued without a host sync. */
int cbinfer_cbresize_forward(const void* input, void* outputState, const uint64_t* inputMask, const int32_t* list,
                             int capN, const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy, int C, int Hi, int Wi,
                             const cbResize* rs, int dtype, cbStream_t stream);

/* ---- change-based pixel shuffle, pixel unshuffle and channel shuffle (cb_rearrange.hip) -----------------
 * No counterpart in the reference.  The three operators compute nothing: values are copied bit for bit, never converted,
 * and -- every producer leaves the pixels outside its change list bit for bit as they were -- the output can differ from
 * last frame's only at the footprint of the input's changes on the OUTPUT map.  Tensors are contiguous, CB_F32 or
 * CB_F16, batch 1; masks are row-padded (cbinfer_mask_words); an int32 list holds flat indexes y W + x of the INPUT map,
 * entries outside it are dropped; bits of the row padding are never set.  `factor` is r for the two pixel shuffles and
 * the group count g for the channel shuffle.
 *   CB_REARRANGE_SHUFFLE, 1 <= r <= 8:    input [Co r r, H, W] -> out [Co, H r, W r],
 *       out[c, y r + i, x r + j] = in[c r r + i r + j, y, x];  (oy, ox) is listed iff input pixel (oy / r, ox / r) is.
 *   CB_REARRANGE_UNSHUFFLE, 1 <= r <= 8:  input [C, Ho r, Wo r] -> out [C r r, Ho, Wo],
 *       out[c r r + i r + j, y, x] = in[c, y r + i, x r + j];  (y, x) is listed iff any of the r x r input pixels of its
 *       block is.
 *   CB_REARRANGE_CHANNELS, 1 <= g <= C, g divides C:  the same shape,
 *       out[k g + q] = in[q (C / g) + k] for q < g, k < C / g;  the same pixel is listed.
 *   the input's changes: inputMask (over the INPUT map; one launch, the footprint gathered inside it), list (capN
 *     entries at most, countDev the device-side length or NULL: capN is the length; one launch in front, which ORs the
 *     footprint into `bits` -- shuffle: the r x r block of every entry, at most two 64-bit atomicOr per row; unshuffle:
 *     cbinfer_pool_footprint with an r x r / stride-r window; channels: with a 1x1 window; capN == 0 launches nothing
 *     in front), or neither: every output pixel is listed.
 *   hand-on: maskCopy (cbinfer_mask_words(Ho, Wo) words) receives the frame's mask every frame; `bits`, the working
 *     mask of the OUTPUT map (zero on first use), is zero again when the frame ends.  Unlisted pixels keep their bits.
 * Bad arguments (a null tensor or mask buffer, input == outputState, C / H / W < 1, an unknown dtype or kind, a factor
 * outside the limits, a channel count that r r (shuffle) or g does not divide, a height or width that r (unshuffle) does
 * not divide, capN < 0, both a mask and a list, a count without a list, inputMask == bits or maskCopy, bits == maskCopy,
 * H W, Ho Wo or 64 Co beyond an int32) return CB_ERR_BADARG and launch nothing. */
enum { CB_REARRANGE_SHUFFLE, CB_REARRANGE_UNSHUFFLE, CB_REARRANGE_CHANNELS };
typedef struct cbRearrange {
    int kind;   /* CB_REARRANGE_* */
    int factor; /* r, or g for CB_REARRANGE_CHANNELS */
} cbRearrange;
/* host, pure: 1 if kind and factor are within the limits above (g <= C is the shape's matter), else 0 */
int cbinfer_rearrange_supported(const cbRearrange* r);
/* host, pure: the output shape of a [C, H, W] input (CB_OK; CB_ERR_UNSUPPORTED beyond the limits; CB_ERR_BADARG for a
 * null pointer, a size < 1 or a size the factor does not divide; Co / Ho / Wo untouched on failure) */
int cbinfer_rearrange_out_shape(const cbRearrange* r, int C, int H, int W, int* Co, int* Ho, int* Wo);
/* The whole frame of a change-based rearrangement enqueued without a host sync; C, H, W are the INPUT's. */
int cbinfer_cbrearrange_forward(const void* input, void* outputState, const uint64_t* inputMask, const int32_t* list,
                                int capN, const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy, int C, int H, int W,
                                const cbRearrange* r, int dtype, cbStream_t stream);

/* ---- change-based padding (cb_pad.hip) -----------------------------------------------------------------
 * No counterpart in the reference.  F.pad of a [C, H, W] map by (left, right, top, bottom) -- torch's order -- in the
 * modes constant (with a value), reflect, replicate and circular: nn.ReflectionPad2d, nn.ReplicationPad2d, nn.ZeroPad2d,
 * nn.ConstantPad2d, nn.CircularPad2d, and what torch runs in front of the contraction of an nn.Conv2d whose padding_mode
 * is not 'zeros'.  A pad computes nothing: values are copied bit for bit, never converted, and -- every producer leaves
 * the pixels outside its change list bit for bit as they were -- the output can differ from last frame's only at the
 * footprint of the input's changes on the OUTPUT map.  Tensors are contiguous, CB_F32 or CB_F16, batch 1; masks are
 * row-padded (cbinfer_mask_words); an int32 list holds flat indexes y W + x of the INPUT map, entries outside it are
 * dropped; bits of the row padding are never set.
 *
 * THIS SECTION IS THE SPECIFICATION; tests/pad_cases.py is its numpy twin and equals torch's F.pad bit for bit.
 *   output size: Ho = H + top + bottom, Wo = W + left + right.
 *   source coordinate per axis, with n the input extent, p the LEADING pad (top / left) and o the output coordinate:
 *   i = o - p, then
 *     CB_PAD_CONSTANT:   i if 0 <= i < n; otherwise the pixel takes `value` and reads no input;
 *     CB_PAD_REFLECT:    i <- |i|, then i <- 2 (n - 1) - i if i >= n;
 *     CB_PAD_REPLICATE:  clamp(i, 0, n - 1);
 *     CB_PAD_CIRCULAR:   i mod n (non-negative).
 *   out[c, oy, ox] = in[c, source(oy), source(ox)].  `value` is converted once to the tensor's dtype ((T)value, round
 *   to nearest even), which is what torch does.
 *   footprint: (oy, ox) is listed iff the input pixel it reads is listed.  A constant-mode border pixel reads nothing:
 *   it is written only by an every-pixel frame.  With a crop a listed input pixel may list nothing.
 *   the input's changes: inputMask (over the INPUT map; one launch, the footprint gathered inside it: lane j of a wave
 *     tests the input bit that output column 64 tile + j reads), list (capN entries at most, countDev the device-side
 *     length or NULL: capN is the length; one launch in front, which ORs the footprint into `bits`: per axis an input
 *     coordinate is read by at most three intervals of output coordinates -- its own image and up to two reflections /
 *     wraps; a replicated border run of up to 65 coordinates is contiguous with the image --, one 64-bit atomicOr per
 *     mask word an interval touches; capN == 0 launches nothing in front), or neither: every output pixel is listed.
 *   hand-on: maskCopy (cbinfer_mask_words(Ho, Wo) words) receives the frame's mask every frame; `bits`, the working
 *     mask of the OUTPUT map (zero on first use), is zero again when the frame ends.  Unlisted pixels keep their bits.
 * Limits (cbinfer_pad_supported): every |pad| <= 64 (cbGeom's padding bound); negative pads (cropping) in constant mode
 * only; Ho, Wo >= 1; reflect: every pad below the extent of its axis, circular: not above it (torch's own rules).
 * Bad arguments (a null tensor or mask buffer, input == outputState, C / H / W < 1, an unknown dtype or mode, a pad beyond
 * the limits, a negative pad outside constant mode, capN < 0, both a mask and a list, a count without a list,
 * inputMask == bits or maskCopy, bits == maskCopy, H W, Ho Wo or 64 C beyond an int32) return CB_ERR_BADARG and launch
 * nothing. */
enum { CB_PAD_CONSTANT, CB_PAD_REFLECT, CB_PAD_REPLICATE, CB_PAD_CIRCULAR };
typedef struct cbPad {
    int mode;                     /* CB_PAD_* */
    int left, right, top, bottom; /* torch's (l, r, t, b) order */
    float value;                  /* CB_PAD_CONSTANT only */
} cbPad;
/* host, pure: 1 if the padding of an H x W map is within the limits above, else 0 */
int cbinfer_pad_supported(const cbPad* p, int H, int W);
/* host, pure: the output size of an H x W map (CB_OK; CB_ERR_UNSUPPORTED beyond the limits; CB_ERR_BADARG for a null
 * pointer or a size < 1; Ho / Wo untouched on failure) */
int cbinfer_pad_out_size(const cbPad* p, int H, int W, int* Ho, int* Wo);
/* The whole frame of a change-based padding enqueued without a host sync; C, H, W are the INPUT's. */
int cbinfer_cbpad_forward(const void* input, void* outputState, const uint64_t* inputMask, const int32_t* list, int capN,
                          const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy, int C, int H, int W, const cbPad* p,
                          int dtype, cbStream_t stream);

/* ---- change-based element-wise operators of two maps (cb_binary.hip) -------------------------------------
 * No counterpart in the reference.  out = op(a, b) with op a sum, a difference, a product -- plain or gated,
 * a * sigmoid(b), a * hardsigmoid(b) --, a maximum or a minimum.  a and the state `out` are [C, H, W], contiguous, one
 * dtype (CB_F32 or CB_F16), two different tensors; b has the same dtype.  Every producer of this library leaves the
 * pixels outside its change list bit for bit as they were, so op(a, b) can differ from last frame's only at the union of
 * the operands' changes, and a constant operand never changes; recomputing there is the dense result, exactly.
 *
 * THIS SECTION IS THE SPECIFICATION; tests/binary_cases.py is its numpy twin.
 *   the second operand is addressed as b[c sc + p sp], p = y W + x, with the strides its form `bForm` gives:
 *     CB_BIN_MAP      [C, H, W]   sc = H W, sp = 1;
 *     CB_BIN_PIXEL    [1, H, W]   sc = 0,   sp = 1: one value per pixel, used for every channel;
 *     CB_BIN_CHANNEL  [C]         sc = 1,   sp = 0;
 *     CB_BIN_SCALAR   [1]         sc = 0,   sp = 0;
 *     CB_BIN_HALVES   `a` is really [2C, H, W] and b its upper half, a + C H W elements (nn.GLU over the channels): the
 *                     entry points derive that address from `a` themselves -- a caller that patches a new frame's address
 *                     into `a` also moves b --, and b must be NULL.
 *   values: at listed pixels, every channel c.  Both operands go to f32 (exact), then ONE correctly rounded f32 operation
 *   -- there is never a multiply-add, so no FMA can be formed --, rounded to f16 once for CB_F16 (the correctly rounded
 *   f16 result):
 *     CB_BIN_ADD      a + b
 *     CB_BIN_SUB      a - b;  reverse != 0: b - a (reverse is accepted with CB_BIN_SUB only)
 *     CB_BIN_MUL      a * g(b), g by `gate` (a gate is accepted with CB_BIN_MUL only):
 *                       CB_BIN_GATE_NONE         g(v) = v
 *                       CB_BIN_GATE_SIGMOID      1 / (1 + expf(-v))          (the device's expf: DESIGN 5.25 has the bound)
 *                       CB_BIN_GATE_HARDSIGMOID  clamp(v + 3, 0, 6) / 6,  clamp(t, lo, hi) = t < lo ? lo : (t > hi ? hi : t)
 *                     the pointwise formulas, evaluated in f32 and ROUNDED TO THE OPERAND DTYPE FIRST, as the separate
 *                     torch operator would round its result; then the product.
 *     CB_BIN_MAXIMUM  a != a ? a : (b != b ? b : (b > a ? b : a))
 *     CB_BIN_MINIMUM  a != a ? a : (b != b ? b : (b < a ? b : a))
 *                     comparisons, not fmaxf / fminf: a NaN if either operand is one; `a` on a tie, +0 against -0
 *                     included.
 *   Except for the sigmoid gate this is torch's CPU operator bit for bit in fp32 and fp16 (torch.add / sub / mul /
 *   maximum / minimum, a * F.hardsigmoid(b)); a NaN result is a NaN, its payload is not specified.  A pixel's bits depend
 *   neither on the other listed pixels nor on the forms the operands' changes arrive in.  Every other pixel of `out`
 *   keeps its bits.
 *   listed pixels: the union of the operands' changes.  `a` arrives as its row-padded change MASK
 *     (cbinfer_mask_words(H, W) words), as an int32 LIST (flat indexes y W + x; entries outside the map are dropped), or
 *     not at all: every pixel is listed then.  b in MAP or PIXEL form with bChanges == CB_BIN_B_OWN arrives the same way.
 *     With bChanges == CB_BIN_B_NONE -- a constant operand; always in HALVES form, whose changes are a's -- b contributes
 *     no pixel and takes neither mask nor list.  CHANNEL or SCALAR with CB_BIN_B_OWN lists every pixel: a per-frame
 *     channel vector changes the whole map.  Bits of the row padding are never set.
 *   hand-on: maskCopy receives the frame's union mask every frame (all zeros for an empty frame); `bits`, the working
 *     mask (cbinfer_mask_words(H, W) words, zero on first use), is zero again when the launch ends.
 * Bad arguments -- a null tensor or mask buffer, C / H / W < 1, an unknown dtype, bForm, op, gate or bChanges, a gate
 * without CB_BIN_MUL, reverse without CB_BIN_SUB, b != NULL in HALVES form or b == NULL in any other, `out` aliasing an
 * operand, a mask or list for b where b cannot have one (CHANNEL, SCALAR, HALVES; CB_BIN_B_NONE; CB_BIN_B_OWN in HALVES
 * form), both a mask and a list for one operand, a count without a list, a negative list capacity, bits == maskCopy, an
 * operand's mask == bits or maskCopy, H W or 64 C beyond an int32 -- return CB_ERR_BADARG and launch nothing. */
enum { CB_BIN_ADD, CB_BIN_SUB, CB_BIN_MUL, CB_BIN_MAXIMUM, CB_BIN_MINIMUM };
enum { CB_BIN_GATE_NONE, CB_BIN_GATE_SIGMOID, CB_BIN_GATE_HARDSIGMOID };
enum { CB_BIN_MAP, CB_BIN_PIXEL, CB_BIN_CHANNEL, CB_BIN_SCALAR, CB_BIN_HALVES };
enum { CB_BIN_B_NONE, CB_BIN_B_OWN };
/* host, pure: 1 if (op, gate, reverse) is a combination above, else 0 */
int cbinfer_binary_supported(int op, int gate, int reverse);
/* The mask-driven launch.  maskA / maskB: the operand's change mask, or NULL (maskB only in MAP or PIXEL form); allA /
 * allB != 0: the operand lists every pixel.  The kernel ORs `bits`, maskA and maskB word by word itself (or forms the
 * full row word); an operand with neither contributes what `bits` holds on entry.  In PIXEL form g(b[p]) is evaluated
 * once per listed pixel and shared over the channels through LDS.  No atomics. */
int cbinfer_binary_changed(const void* a, const void* b, void* out, const uint64_t* maskA, int allA, const uint64_t* maskB,
                           int allB, uint64_t* bits, uint64_t* maskCopy, int C, int H, int W, int bForm, int op, int gate,
                           int reverse, int dtype, cbStream_t stream);
/* The whole frame enqueued without a host sync.  Per operand X: maskX != NULL: mask form; listX != NULL: list form (capX
 * entries at most, countX the device-side length or NULL: capX is the length; capX == 0 launches nothing); both NULL: no
 * change information -- for `a`, and for b with CB_BIN_B_OWN, every pixel is listed; for b with CB_BIN_B_NONE, none.
 * With both operands in mask or all form the frame is ONE launch (cbinfer_binary_changed); an operand in list form costs
 * one launch in front, which ORs its bits into `bits` -- skipped when the other operand lists every pixel anyway.  All
 * arguments are checked before the first launch. */
int cbinfer_cbbinary_forward(const void* a, const void* b, void* outputState, const uint64_t* maskA, const int32_t* listA,
                             int capA, const int32_t* countA, const uint64_t* maskB, const int32_t* listB, int capB,
                             const int32_t* countB, int bForm, int bChanges, uint64_t* bits, uint64_t* maskCopy, int C,
                             int H, int W, int op, int gate, int reverse, int dtype, cbStream_t stream);

/* ---- change-based channel attention scale (cb_chanscale.hip) ---------------------------------------------
 * No counterpart in the reference.  out[c, p] = a[c, p] * held[c]: the excite of a squeeze-and-excitation block.  a and
 * the state `out` are [C, H, W], contiguous, one dtype (CB_F32 or CB_F16), two different tensors, 1 <= C <= 4096.  The
 * gate vector of a frame moves a little in every frame; a channel whose gate moved by no more than `threshold` keeps the
 * gate it last used, held[c], and only a channel that moved by more -- it TRIPPED -- has its whole plane recomputed.
 *
 * THIS SECTION IS THE SPECIFICATION; tests/chanscale_cases.py is its numpy twin.
 *   s [C], f32, from one of two sources:
 *     plain (R == 0; w1, b1, w2, b2 NULL; act CB_CS_ACT_NONE): s[c] = (float)v[c], v [C] in the dtype of `a`;
 *     excitation (1 <= R <= 1024; act CB_CS_ACT_RELU or CB_CS_ACT_SILU): v is the pooled vector z [C] in the dtype of
 *       `a`, w1 [R, C], w2 [C, R] f32, b1 [R] / b2 [C] f32 or NULL (then nothing is added):
 *         hidden[r] = act(sum16_c(w1[r, c] * z[c]) + b1[r]),   s[c] = sum16_r(w2[c, r] * hidden[r]) + b2[c],
 *       every product and sum a correctly rounded f32 operation of its own, never an FMA; sum16 is the order of
 *       tests/chanreduce_cases.py: 16 partial sums by index mod 16, each from +0 in ascending index, then the fixed tree
 *       p[2i] + p[2i+1];  ReLU: v < 0 ? 0 : v;  SiLU: v / (1 + expf(-v)).
 *   gate[c] = g(s[c]) in f32: CB_CS_GATE_NONE s;  CB_CS_GATE_SIGMOID 1 / (1 + expf(-s)) (the device's expf);
 *     CB_CS_GATE_HARDSIGMOID clamp(s + 3, 0, 6) / 6 with clamp(t, lo, hi) = t < lo ? lo : (t > hi ? hi : t).
 *   channel c trips iff all != 0 or !(fabsf(gate[c] - held[c]) <= threshold): strictly more than the threshold, and a
 *     NaN trips.  A tripped channel takes held[c] = gate[c]; any other keeps held[c] bit for bit, so slow drift adds up
 *     until it trips.  tripped: ceil(C / 64) words, bit c % 64 of word c / 64, every word written every frame, the bits
 *     beyond C zero; tripCount: their number.
 *   values: out[c, p] = (T)((float)a[c, p] * held[c]), one f32 product, one rounding to T, written
 *     at a listed pixel p for every channel c, and at every other pixel for the tripped channels.
 *   Every other element of `out` keeps its bits.
 *   listed pixels: `a` arrives as its row-padded change MASK, as an int32 LIST, or not at all (every pixel is listed), as
 *     for the operators above; with all != 0 every pixel is listed and the operand's change information is not read.
 *   hand-on: maskCopy receives the frame's mask every frame: the listed pixels, or every pixel of the map in a frame in
 *     which a channel tripped (a per-pixel mask cannot name a channel); `bits`, the working mask, is zero again when the
 *     launch ends.
 * Bad arguments -- a null tensor or buffer, C < 1 or > 4096, R < 0 or > 1024, an unknown dtype, gate or act, an act that
 * does not go with R, weights without R or R without weights, a negative or NaN threshold, `out` aliasing an operand,
 * gate == held, both a mask and a list, a count without a list, a negative capacity, bits == maskCopy, the operand's
 * mask == bits or maskCopy, H W beyond an int32 -- return CB_ERR_BADARG and launch nothing. */
enum { CB_CS_GATE_NONE, CB_CS_GATE_SIGMOID, CB_CS_GATE_HARDSIGMOID };
enum { CB_CS_ACT_NONE, CB_CS_ACT_RELU, CB_CS_ACT_SILU };
/* host, pure: 1 if (gate, act, C, R) is a combination above, else 0 */
int cbinfer_chanscale_supported(int gate, int act, int C, int R);
/* Launch 1, ONE workgroup: s, gate, the trip decisions, held, tripped and tripCount as above.  No atomics. */
int cbinfer_chanscale_gate(const void* v, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                           float* held, uint64_t* tripped, int32_t* tripCount, int C, int R, int gateFn, int act,
                           float threshold, int all, int dtype, cbStream_t stream);
/* Launch 2, the mask-driven one: reads held, tripped and tripCount as launch 1 left them on the same stream.  maskA: the
 * operand's change mask, or NULL: the operand contributes what `bits` holds on entry; all != 0: every pixel is listed. */
int cbinfer_chanscale_changed(const void* a, void* out, const float* held, const uint64_t* tripped,
                              const int32_t* tripCount, const uint64_t* maskA, int all, uint64_t* bits, uint64_t* maskCopy,
                              int C, int H, int W, int dtype, cbStream_t stream);
/* The whole frame enqueued without a host sync: launch 1 and launch 2, an operand in list form costs one launch in
 * front.  maskA != NULL: mask form; listA != NULL: list form (capA entries at most, countA the device-side length or
 * NULL); both NULL: every pixel is listed.  all != 0 (a fresh state): every channel trips and every pixel is written. */
int cbinfer_cbchanscale_forward(const void* a, const void* v, const float* w1, const float* b1, const float* w2,
                                const float* b2, void* outputState, float* gate, float* held, uint64_t* tripped,
                                int32_t* tripCount, const uint64_t* maskA, const int32_t* listA, int capA,
                                const int32_t* countA, uint64_t* bits, uint64_t* maskCopy, int C, int R, int H, int W,
                                int gateFn, int act, float threshold, int all, int dtype, cbStream_t stream);

/* ---- change-based group norm and instance norm (cb_groupnorm.hip) ---------------------------------------
 * No counterpart in the reference.  torch's nn.GroupNorm on a map -- nn.InstanceNorm2d without running statistics is
 * G == C, GroupNorm(1, C) is G == 1 --: out[c, p] = (a[c, p] - mean[g]) rstd[g] gamma[c] + beta[c] with g = c / (C / G)
 * and the statistics taken over the (C / G) H W values of the group.  A group's (mean, rstd) moves a little in every
 * frame of a video, so the library's threshold rule is applied to it: a group whose statistics moved by no more than
 * `threshold` keeps the pair it last used (`held`) and is recomputed only at the operand's changed pixels; a group whose
 * statistics moved by more -- it TRIPPED -- takes the new pair and its planes are recomputed completely.  At
 * threshold == 0 this is the dense operator.
 *
 * THIS SECTION IS THE SPECIFICATION; tests/groupnorm_cases.py is its numpy twin.
 *   operand and state: a and the state `out` are [C, H, W], contiguous, one dtype (CB_F32 or CB_F16), two different
 *     tensors; 1 <= C <= 4096, G >= 1 divides C, batch 1, H W within an int32.  gamma / beta: f32 [C] or NULL -- NULL: no
 *     multiplication / no addition.  eps: a HOST pointer to ONE double, read during the call (the scalar parameters of
 *     this ABI are int, long and float); relu 0 or 1; threshold >= 0.
 *   level 1, the segment partials, f64, caller-owned state of 2 C H wpr doubles, wpr = ceil(W / 64).  A segment is one
 *     word of the row-padded change mask: the 64 columns tile 64 ... tile 64 + 63 of one row.  P[k][c][y][tile], element
 *     ((k C + c) H + y) wpr + tile: the sum over the segment's columns < W of (double)x (k == 0) and of (double)x (double)x
 *     (k == 1; exact: the square of an f32 or f16 value is an f64 number) by the FIXED butterfly over 64 lanes, lane l
 *     holding column tile 64 + l or +0 beyond W: p_l = p_l + p_(l xor m) for m = 1, 2, 4, 8, 16, 32; the result is p_0.
 *     Every addition is one correctly rounded f64 addition.  The statistics are f64 since E[x^2] - mean^2 in f32 cancels
 *     on a map whose mean is large against its spread.  A frame recomputes exactly the partials of the DIRTY segments --
 *     those whose word of the listed pixels is not zero --, for every channel; every other partial keeps its bits, and
 *     the input pixels of a clean segment are never read.
 *   level 2, the statistics of group g: its N = (C / G) H wpr partials are contiguous from (k C + g C / G) H wpr.  1024
 *     lane sums s_l = +0; s_l += x_i for i = l, l + 1024, ... < N ascending; then s_l += s_(l + off) for l < off,
 *     off = 512, 256, ..., 1; S1 (k == 0) and S2 (k == 1) are s_0.  With n = (double)((C / G) H W):
 *       mean = S1 / n;  var = S2 / n - mean mean;  var = var < 0 ? 0 : var (a NaN stays);  rstd = 1 / sqrt(var + eps)
 *     every operation an f64 operation of its own; mean and rstd are then rounded ONCE to f32 and written to
 *     stats[g] / stats[G + g] every frame.
 *   the rule, in f32, every operation rounded on its own.  held is f32 [2][G]: held[g] the mean, held[G + g] the rstd the
 *     group last used.  Group g trips iff all != 0 (a fresh state), or !(fabsf(mean - heldMean) heldRstd <= threshold), or
 *     !(fabsf(rstd - heldRstd) <= threshold heldRstd): strictly more than the threshold, and a NaN trips.  A tripped
 *     group takes both new values; any other keeps both bit for bit, so slow drift adds up until it trips.  THE UNIT: the
 *     threshold is a shift of the mean in held standard deviations and a relative change of rstd; to first order the
 *     normalised value y of a held group is off by at most threshold (1 + |y|), before gamma.  tripped[g], one int32
 *     per group (1 or 0), is written every frame by the group's own workgroup: nothing needs zeroing.
 *   values: y = ((float)x - heldMean) heldRstd;  v = y gamma[c] (gamma != NULL);  v = v + beta[c] (beta != NULL);
 *     relu: v = v < 0 ? 0 : v (-0 and a NaN stay);  out = (T)v.  Every operation is a correctly rounded f32 operation of
 *     its own, never an FMA, and the conversion to f16 is a rounding of its own.
 *   what is written: a listed pixel for every channel; every other pixel for the channels of the tripped groups.  Every
 *     other element of `out` keeps its bits.
 *   listed pixels: `a` arrives as its row-padded change MASK, as an int32 LIST, or not at all (every pixel is listed), as
 *     for the operators above; with all != 0 every pixel is listed and the operand's change information is not read.
 *   hand-on: maskCopy receives the frame's mask every frame: the listed pixels, or EVERY pixel of the map in a frame in
 *     which a group tripped; `bits`, the working mask, is zero again when the frame ends.
 * Bad arguments -- a null tensor or buffer (gamma and beta may be NULL), C < 1 or > 4096, G < 1 or not dividing C,
 * H or W < 1, H W beyond an int32, an unknown dtype, a negative or NaN threshold, a negative or non-finite eps, relu
 * other than 0 or 1, `out` aliasing the operand or a buffer, stats == held, both a mask and a list, a count without a
 * list, a negative capacity, bits == maskCopy, the operand's mask == bits or maskCopy -- return CB_ERR_BADARG and launch
 * nothing. */
/* host, pure: 1 if 1 <= C <= 4096 and G >= 1 divides C, else 0 */
int cbinfer_groupnorm_supported(int C, int G);
/* Launch 1, level 1: a persistent grid over (mask word, block of 16 channels) units.  The listed word is
 * bits[w] | maskA[w] (either may be NULL; all != 0: the full row word); both are only read.  Clean words are skipped.
 * Lane = column, four channels in flight per wave.  A partial has ONE writer: segment = mask word.  No atomics. */
int cbinfer_groupnorm_partials(const void* a, double* partials, const uint64_t* maskA, const uint64_t* bits, int all,
                               int C, int H, int W, int dtype, cbStream_t stream);
/* Launch 2, level 2 and the rule: one workgroup of 1024 threads per group; stats, held and tripped as above.  Runs
 * every frame: an empty frame finds the same partials, hence the same statistics and no trip. */
int cbinfer_groupnorm_stats(const double* partials, float* stats, float* held, int32_t* tripped, int C, int G, int H,
                            int W, const double* eps, float threshold, int all, cbStream_t stream);
/* Launch 3, the mask-driven one: reads held and tripped as launch 2 left them on the same stream.  maskA: the operand's
 * change mask, or NULL: the operand contributes what `bits` holds on entry; all != 0: every pixel is listed. */
int cbinfer_groupnorm_changed(const void* a, void* out, const float* gamma, const float* beta, const float* held,
                              const int32_t* tripped, const uint64_t* maskA, int all, uint64_t* bits, uint64_t* maskCopy,
                              int C, int G, int H, int W, int relu, int dtype, cbStream_t stream);
/* The whole frame enqueued without a host sync: the three launches, an operand in list form costs one launch in front.
 * maskA != NULL: mask form; listA != NULL: list form (capA entries at most, countA the device-side length or NULL); both
 * NULL: every pixel is listed.  all != 0 (a fresh state): every group trips and every partial and pixel is written.  All
 * arguments are checked before the first launch.  Three launches and not fewer: the readers of `held` must not share a
 * launch with its writer, nor the readers of the partials with theirs. */
int cbinfer_cbgroupnorm_forward(const void* a, const float* gamma, const float* beta, void* outputState, double* partials,
                                float* stats, float* held, int32_t* tripped, const uint64_t* maskA, const int32_t* listA,
                                int capA, const int32_t* countA, uint64_t* bits, uint64_t* maskCopy, int C, int G, int H,
                                int W, const double* eps, int relu, float threshold, int all, int dtype,
                                cbStream_t stream);

/* ---- transposed convolution (cb_tconv.hip) ------------------------------------------------------------
 * The reference has no counterpart: its CBConv2d asserts transposed == False (conv2d.py:92-104).  Input map Hi x Wi,
 * weight [C, K, kH, kW] (torch's layout for nn.ConvTranspose2d), stride (sH, sW), padding (pH, pW), dilation (dH, dW),
 * output padding (opH, opW); output map Ho = (Hi - 1) sH - 2 pH + dH (kH - 1) + opH + 1, Wo likewise.
 *   out[co, oy, ox] = bias[co] + sum over c and the taps (ky, kx) for which ny = oy + pH - ky dH is divisible by sH,
 *     nx = ox + pW - kx dW by sW and (ny / sH, nx / sW) lies inside the input map, of in[c, ny/sH, nx/sW] w[c, co, ky, kx].
 *   The PHASE of an output pixel is ((oy + pH) mod sH, (ox + pW) mod sW); tap ky belongs to row phase ry iff
 *     (ry - ky dH) mod sH == 0, columns likewise.  A phase may own no tap (k < s; 1x1 stride 2; 3x3 s2 d2), and rows or
 *     columns added by the output padding may be out of reach: such pixels are never listed and NO entry point below
 *     writes them.  Their dense value is the bias (after the ReLU), 0 without one, in every frame: the caller
 *     initialises prevOutput / output with it -- CBConvTranspose2d does when it allocates the state.
 * Limits per axis: k <= 8, s <= 4, d <= 4, 0 <= p <= d (k-1), 0 <= op < max(s, d) (torch's own rule); groups 1, batch 1.
 * Beyond them CB_ERR_UNSUPPORTED.  A null geometry, tensor or mask, a non-positive k / s / d, a negative p / op, C, K,
 * Hi or Wi < 1, an input map so small that Ho or Wo < 1, an unknown dtype, Ho Wo, C Hi Wi or K Ho Wo beyond an int32, or a capacity < 0: CB_ERR_BADARG.  Nothing
 * is launched in either case.  The geometry travels as one HOST struct. */
typedef struct cbTGeom {
    int kH, kW, sH, sW, pH, pW, dH, dW, opH, opW;
} cbTGeom;
/* host, pure: the output size (status as above; Ho / Wo untouched on failure).  No counterpart in the reference. */
int cbinfer_tconv_out_size(int Hi, int Wi, const cbTGeom* geom, int* Ho, int* Wo);
/* Prepared weights (no counterpart in the reference): per phase ph = ry sW + rx with at least one tap, in phase order,
 * W_ph[Kpad64][CkkP_ph] in the tensors' element type (Ckk_ph = C taps(ph) padded to 32, k = c taps(ph) + tap, zero
 * padded; CB_F32S shares CB_F32's layout) followed by that phase's k -> tap table for an Hi x Wi input map: byte
 * offset relative to the pixel's base input pixel ((oy + pH) / sH, (ox + pW) / sW) and the signed dy, dx of the border
 * test.  cbinfer_tconv_prepared_weights_bytes: the total, 0 for a rejected geometry. */
long cbinfer_tconv_prepared_weights_bytes(int K, int C, const cbTGeom* geom, int dtype);
int cbinfer_tconv_prep_weights(const void* weight, void* prepared, int K, int C, int Hi, int Wi, const cbTGeom* geom,
                               int dtype, cbStream_t stream);
/* split-k workspace of cbinfer_conv_changed_tconv (no counterpart in the reference): partial-tile slabs followed by
 * the tiles' arrival counters -- the last 2048 bytes, ZERO on first use and left zero by every launch.  One per layer. */
long cbinfer_tconv_workspace_bytes(void);
/* Detection, one launch (no counterpart in the reference).  change(p) on the INPUT map exactly as
 * cbinfer_change_detection (a1); updateInputState as there (1: feedback refresh at the changed pixels, 2: state <-
 * input wherever they differ, 0: state untouched).  The EXACT footprint -- output (oy, ox) iff for some tap ny and nx
 * divide and (ny / sH, nx / sW) is inside the input map and changed -- is ORed into the mask the parity selects of a
 * frame mask buffer of the OUTPUT map (cbinfer_frame_mask_bytes(Ho, Wo) bytes, zero on first use).  A changed pixel
 * that reaches no output pixel still refreshes the state. */
int cbinfer_change_detection_tconv(const void* input, void* state, uint64_t* frameMasks, int C, int Hi, int Wi,
                                   const cbTGeom* geom, float threshold, int updateInputState, int dtype,
                                   cbStream_t stream);
/* Contraction, one launch (no counterpart in the reference): per phase, gather -> MFMA -> bias / ReLU -> scatter at
 * the listed OUTPUT pixels with at least one tap; nothing else of output [K, Ho, Wo] is written.  Tiles hold pixels of
 * one phase and spend CkkP_ph / 32 stages.  bias may be NULL; dtype selects the arithmetic as in
 * cbinfer_conv_changed_geom.  Either
 *   frameMasks != NULL: the listed pixels are those of the frame mask cbinfer_change_detection_tconv filled; the
 *     frame's mask is copied to cbinfer_frame_mask_copy_offset(Ho, Wo), the other mask is zeroed and the parity flipped
 *     for the next frame (no list is written: cbinfer_compact_bits makes one from the copy); or
 *   changeList (ascending flat output pixels) / numChanges (0 <= numChanges <= Ho Wo) / countDev (device-side length or
 *     NULL): entries outside the map and entries of a phase without a tap are dropped; the kernel buckets the rest by
 *     phase itself.
 * A short list is split along k over idle workgroups (per phase, capped by the phase's stage count) and summed in
 * slice order (deterministic) when a workspace is given. */
int cbinfer_conv_changed_tconv(const void* input, const int32_t* changeList, int numChanges, const int32_t* countDev,
                               uint64_t* frameMasks, const void* prepared, const void* bias, void* output, int C, int Hi,
                               int Wi, int K, const cbTGeom* geom, int relu, void* workspace, int dtype,
                               cbStream_t stream);
/* The whole frame of a CBConvTranspose2d enqueued without a host sync: detection + contraction (no counterpart in the
 * reference; feedbackLoop / copyInput contract of cbinfer_cbconv2d_forward; prevInput [C,Hi,Wi], prevOutput [K,Ho,Wo]).
 * The frame's change mask on the OUTPUT map is left at cbinfer_frame_mask_copy_offset(Ho, Wo) of frameMasks. */
int cbinfer_cbconvtranspose2d_forward(const void* input, void* prevInput, void* prevOutput, uint64_t* frameMasks,
                                      const void* prepared, const void* bias, int C, int Hi, int Wi, int K,
                                      const cbTGeom* geom, float threshold, int feedbackLoop, int copyInput, int relu,
                                      void* workspace, int dtype, cbStream_t stream);

/* ---- depthwise convolution (cb_dwconv.hip) ------------------------------------------------------------
 * The reference has no counterpart: its CBConv2d asserts groups == 1 (conv2d.py:92-104).  groups == in_channels with a
 * channel multiplier: input [C, Hi, Wi], weight [K, 1, kH, kW] (torch's layout, read as it is: no preparation, no
 * workspace), K = C mult, mult >= 1, a cbGeom within the general-geometry limits, output [K, Ho, Wo] by
 * cbinfer_geom_out_size.  At a listed output pixel, for every k:
 *   out[k, oy, ox] = act(bias[k] + sum over the taps (ky, kx) inside the input map of
 *                        w[k, 0, ky, kx] in[k / mult, oy sH - pH + ky dH, ox sW - pW + kx dW])
 *   evaluated in f32 in ONE fixed order: start from the bias (0 without one), taps row-major (ky outer, kx inner), one FMA
 *   per tap, out-of-map taps skipped, rounded to f16 once for CB_F16.  A pixel's bits depend neither on which other
 *   pixels are listed nor on the launch form.  act: CB_ACT_NONE; CB_ACT_RELU: v > 0 ? v : 0; CB_ACT_RELU6: additionally
 *   v < 6 ? v : 6; a NaN stays a NaN.  Every unlisted output value keeps its bits.  Output pixels no tap reaches (see the
 *   general geometry above) are NEVER written, listed or not: the caller initialises them to act(bias).
 * dtype CB_F32 or CB_F16 (no CB_F32S: f32 FMAs on exact operands need no bf16 triples).  All arguments are checked
 * before the first launch: a null geometry, tensor or mask, C, mult, Hi or Wi < 1, an unknown dtype or act, 64 C mult
 * beyond an int32: CB_ERR_BADARG; a geometry beyond the limits, K Ho Wo beyond an int32 or C Hi Wi 4 >= 2^30:
 * CB_ERR_UNSUPPORTED.  Nothing is launched in either case. */
#define CB_ACT_NONE 0
#define CB_ACT_RELU 1
#define CB_ACT_RELU6 2
/* host, pure: 1 if C, mult and the geometry are within the limits above, else 0.  No counterpart in the reference. */
int cbinfer_dwconv_supported(int C, int mult, const cbGeom* geom);
/* The stencil at the listed pixels (no counterpart in the reference).  Exactly ONE form is given, else CB_ERR_BADARG:
 *   frameMasks: the frame mask buffer of the OUTPUT map as cbinfer_change_detection_geom fills it; the protocol of
 *     cbinfer_conv_changed_tconv -- the frame's mask is copied to cbinfer_frame_mask_copy_offset(Ho, Wo), the other
 *     mask is zeroed, the last workgroup to arrive flips the parity; no list is written; one launch; or
 *   bits / maskCopy: the contract of cbinfer_pool_changed -- every word of `bits` is copied to maskCopy and zeroed;
 *     bits != maskCopy; a small launch in front moves the mask, the stencil launch reads maskCopy only. */
int cbinfer_dwconv_changed(const void* input, const void* weight, const void* bias, void* output, uint64_t* frameMasks,
                           uint64_t* bits, uint64_t* maskCopy, int C, int mult, int Hi, int Wi, const cbGeom* geom,
                           int act, int dtype, cbStream_t stream);
/* The whole frame with the layer's own detection, enqueued without a host sync (no counterpart in the reference):
 * cbinfer_change_detection_geom (unchanged, called as it is) + cbinfer_dwconv_changed.  feedbackLoop / copyInput contract
 * and the updateInputState mapping exactly as cbinfer_cbconv2d_forward_geom; prevInput [C,Hi,Wi], prevOutput [K,Ho,Wo].
 * The frame's change mask on the OUTPUT map is left at cbinfer_frame_mask_copy_offset(Ho, Wo) of frameMasks. */
int cbinfer_cbdwconv2d_forward(const void* input, void* prevInput, void* prevOutput, uint64_t* frameMasks,
                               const void* weight, const void* bias, int C, int mult, int Hi, int Wi, const cbGeom* geom,
                               float threshold, int feedbackLoop, int copyInput, int act, int dtype, cbStream_t stream);
/* The whole frame from propagated changes (no counterpart in the reference): cbinfer_pool_footprint (the producer's
 * list -- changeIndexes / capN / countDev -- or its mask of the INPUT map, inputMask; window = the filter) +
 * cbinfer_dwconv_changed in the bits / maskCopy form on the INPUT tensor itself: no detection runs and no state of the
 * input is kept.  Only where the pool footprint is the filter's: dilation 1 and p <= k / 2 per axis (and the pool
 * limits); CB_ERR_UNSUPPORTED otherwise.  allPixels != 0: every pixel is listed (the frame after the output state was
 * allocated) and the producer's changes are not read.  `bits`: the working mask of the OUTPUT map (zero on first use,
 * zero again when the frame ends); maskCopy receives the frame's mask every frame. */
int cbinfer_cbdwconv2d_forward_propagated(const void* input, void* outputState, const int32_t* changeIndexes, int capN,
                                          const int32_t* countDev, const uint64_t* inputMask, int allPixels,
                                          uint64_t* bits, uint64_t* maskCopy, const void* weight, const void* bias, int C,
                                          int mult, int Hi, int Wi, const cbGeom* geom, int act, int dtype,
                                          cbStream_t stream);

/* ---- grouped convolution (cb_groupconv.hip) -----------------------------------------------------------
 * The reference has no counterpart: its CBConv2d asserts groups == 1 (conv2d.py:92-104).  G = groups >= 2 with
 * C % G == 0 and K % G == 0: input [C, Hi, Wi], weight [K, Cg, kH, kW] (torch's layout), Cg = C / G, Kg = K / G, a cbGeom
 * within the general-geometry limits, output [K, Ho, Wo] by cbinfer_geom_out_size; output channel m reads the input
 * channels (m / Kg) Cg ... + Cg - 1 only.  groups == C (depthwise) is accepted and correct, but cbinfer_dwconv_* is the
 * fast path for it.  Status as in the general geometry: a null pointer, a non-positive C, K, groups, Hi or Wi or geometry
 * entry, an unknown dtype, a filter that does not fit the padded map, or Ho Wo >= 2^31: CB_ERR_BADARG; a geometry beyond
 * the limits, groups == 1, C or K no multiple of groups, Cg Hi Wi elemSize >= 2^31 (the tap table holds group-relative
 * byte offsets in an int) or Hi Wi >= 2^30: CB_ERR_UNSUPPORTED.  Nothing is launched in either case.  Output pixels no
 * tap reaches (see the general geometry) are never written by the frame entry point: the caller initialises them to
 * act(bias). */
/* host, pure: 1 if groups >= 2 divides C and K and the geometry is within the limits, else 0.  No counterpart in the
 * reference (groups == 1 asserted). */
int cbinfer_groupconv_supported(int C, int K, int groups, const cbGeom* geom);
/* Prepared weights (no counterpart in the reference): W[G][KgP][CkkgP] in the tensors' element type, k contiguous, zero
 * padded -- KgP = Kg rounded up to ROWS (16 if Kg <= 16, 32 if Kg <= 32, else 64), CkkgP = Cg kH kW rounded up to 32;
 * CB_F32S shares CB_F32's layout -- followed by the group-relative k -> tap table of 2 CkkgP ints for an Hi x Wi input
 * map (format of cbinfer_geom_prep_weights, c counted within the group; the same for every group).
 * G KgP CkkgP elemSize + 8 CkkgP bytes; 0 for a rejected shape. */
long cbinfer_groupconv_prepared_weights_bytes(int K, int C, int groups, const cbGeom* geom, int dtype);
int cbinfer_groupconv_prep_weights(const void* weight, void* prepared, int K, int C, int groups, int Hi, int Wi,
                                   const cbGeom* geom, int dtype, cbStream_t stream);
/* Contraction, one launch, no workspace (no counterpart in the reference): gather -> MFMA -> bias / ReLU -> scatter at
 * the listed OUTPUT pixels, nothing else of output [K, Ho, Wo] is written.  bias may be NULL.  dtype selects the
 * arithmetic as in cbinfer_conv_changed_geom (CB_F16; CB_F32S; CB_F32).  The list comes from frameMasks (idxOut /
 * countOut written, mask copied, other mask zeroed, parity flipped -- also for an empty mask) or from changeList /
 * numChanges / countDev, exactly as there; entries outside the map are ignored and never used for an address.  A listed
 * pixel's bits depend only on the input, the weights and the arithmetic: not on the other listed pixels, its place in
 * the list, or the list's source. */
int cbinfer_conv_changed_grouped(const void* input, const int32_t* changeList, int numChanges, const int32_t* countDev,
                                 uint64_t* frameMasks, int32_t* idxOut, int32_t* countOut, const void* prepared,
                                 const void* bias, void* output, int C, int Hi, int Wi, int K, int groups,
                                 const cbGeom* geom, int relu, int dtype, cbStream_t stream);
/* The whole frame enqueued without a host sync (no counterpart in the reference): cbinfer_change_detection_geom
 * (unchanged, called as it is: change over all C channels) + cbinfer_conv_changed_grouped from the frame mask.
 * feedbackLoop / copyInput contract and the updateInputState mapping exactly as cbinfer_cbconv2d_forward_geom, without
 * haveIndexes; prevInput [C,Hi,Wi], prevOutput [K,Ho,Wo]; idx (capacity Ho Wo) / countDev receive the frame's list.  All
 * arguments are checked before the first launch. */
int cbinfer_cbgroupconv2d_forward(const void* input, void* prevInput, void* prevOutput, uint64_t* frameMasks,
                                  int32_t* idx, int32_t* countDev, const void* prepared, const void* bias, int C, int Hi,
                                  int Wi, int K, int groups, const cbGeom* geom, float threshold, int feedbackLoop,
                                  int copyInput, int relu, int dtype, cbStream_t stream);

/* ---- change-based adaptive and global pooling: max and average (cb_adaptpool.hip) ----------------------
 * No counterpart in the reference.  torch's nn.AdaptiveMaxPool2d / nn.AdaptiveAvgPool2d on a map: input [C, H, W] (batch
 * 1, CB_F32 or CB_F16), output [C, oh, ow] with 1 <= oh <= H and 1 <= ow <= W.  Added under ABI 11.
 *   windows (torch's): output row i reads the input rows lo(i) ... hi(i) - 1 with lo(i) = floor(i H / oh) and
 *     hi(i) = ceil((i + 1) H / oh); output column j the input columns floor(j W / ow) ... ceil((j + 1) W / ow) - 1.
 *     Neighbouring windows share a row (a column) where the size does not divide, so an input row lies in one or two
 *     row windows: floor(y oh / H) ... ceil((y + 1) oh / H) - 1.
 *   two levels.  Level 1, the row-segment partials, f32, caller-owned state of cbinfer_adaptive_pool_partial_elems
 *     elements: P(c, y, j) is the sum (CB_ADAPT_AVG) or the maximum (CB_ADAPT_MAX) over the columns of window j in input
 *     row y of channel c.  LAYOUT [C][ow][H]: element (c ow + j) H + y -- the lanes of the second launch, which run along
 *     the rows of a window, read consecutive addresses.  Level 2: out(c, i, j) is the sum or maximum of P(c, y, j) over
 *     the rows y of window i; the average is that sum divided by float(rows cols) in ONE IEEE f32 division; CB_F16
 *     rounds the result to f16 once (f16 inputs are widened to f32 exactly).
 *   order of the additions, a function of (H, W, oh, ow) alone -- not of the changed pixels, the operand's form, the
 *     grid or the wave scheduling; every addition is one correctly rounded f32 addition, never an FMA.  Both levels
 *     are the same reduction of values x_0 ... x_(n-1) on L lanes: s_l = +0; s_l += x_k for k = l, l + L, l + 2 L, ...
 *     < n in ascending order (a lane without a value keeps +0); then for off = L / 2, L / 4, ..., 1: s_l += s_(l + off)
 *     for l < off; the result is s_0.  L = cbinfer_adaptive_pool_lanes(N, o) is the smallest power of two >= the
 *     longest window the axis can have (N / o if o divides N, else floor(N / o) + 2), at most 64.
 *     level 1: the segment's values from left to right, L = lanes(W, ow).
 *     level 2: the partials of the window's rows from top to bottom, L = lanes(H, oh).
 *   maximum: a NaN in the window wins (which NaN is not specified); among equal maxima the first in row-major window
 *     order wins, and +0 == -0 there, so the result is torch's bit for bit.  Both levels carry the position with the
 *     value through the same lanes and tree: a later value of a lane wins only if greater, and of two equal values in
 *     the tree the one that comes first -- further left in level 1, further up in level 2.
 *   the average is NOT torch's bits (torch sums the window in one run); it is this specification's, which
 *     tests/adaptpool_cases.py restates in numpy.
 *   a frame.  The operand's changes come as its row-padded change MASK of the INPUT map (cbinfer_mask_words(H, W)
 *     words), as an int32 LIST (flat indexes y W + x, entries outside the map are dropped), or not at all: every pixel
 *     counts as changed then (the form of a frame that writes a new state).  P(., y, j) is recomputed, for all channels,
 *     iff column window j of row y holds a changed pixel; output pixel (i, j) is listed and recomputed, for all
 *     channels, iff its window holds a changed pixel; every other partial and output value keeps its bits.  After any
 *     sequence of frames that began with an every-pixel frame, partials and output are what the last frame's input gives
 *     alone.  The work is O(C (lengths of the dirty segments + listed outputs x rows per window)): no launch reads an
 *     input pixel of a clean segment.
 *   hand-on: maskCopy (cbinfer_mask_words(oh, ow) words) receives the frame's mask on the OUTPUT map every frame, all
 *     zeros for an empty frame; outBits, the working mask of the output map (same size), and inBits, the working mask
 *     of the input map (cbinfer_mask_words(H, W) words, needed for a list only), are zero on first use and zero again
 *     when the frame ends.
 *   launches: the list, if any, ORed into inBits (one launch, as in cbinfer_cbadd_forward); then
 *     cbinfer_adaptive_pool_partials; then cbinfer_adaptive_pool_changed.  No host sync, no allocation, no waiting
 *     between workgroups; the only atomics are 64-bit ORs into outBits.
 * Status: a null tensor or mask buffer, C / H / W / oh / ow < 1, oh > H or ow > W, an unknown op or dtype, two of the
 * buffers the same, both a mask and a list, a count without a list, a list without inBits, capN < 0: CB_ERR_BADARG;
 * ow > 4096, H W, 64 C, (H + 1) oh, (W + 1) ow or the partials' element count beyond an int32: CB_ERR_UNSUPPORTED.  All arguments are checked
 * before the first launch; a refused call launches nothing. */
#define CB_ADAPT_MAX 0
#define CB_ADAPT_AVG 1
/* host, pure: 1 if the library pools an H x W map to oh x ow (the size rules above), else 0 */
int cbinfer_adaptive_pool_supported(int H, int W, int oh, int ow);
/* host, pure: the lanes L of the reduction along an N-long axis pooled to o (1 for a bad argument) */
int cbinfer_adaptive_pool_lanes(int N, int o);
/* host, pure: the elements (f32) of the partials, C H ow; 0 for a refused shape */
long cbinfer_adaptive_pool_partial_elems(int C, int H, int W, int oh, int ow);
/* Launch 1: partials and footprint.  The unit of work is (input row y, block of 32 channels) on a persistent grid; every
 * unit forms the row's dirty column windows from the row's words of inputMask | inBits (either may be NULL; all != 0:
 * every window) and recomputes its channels' partials of those windows, the lanes along x -- so each partial has ONE
 * writer, also where a column window spans two mask words.  The first channel block of a row ORs the dirty windows into
 * the one or two rows of outBits that hold y: one 64-bit atomicOr per dirty (row, output word).  inBits is only read. */
int cbinfer_adaptive_pool_partials(const void* input, float* partials, const uint64_t* inputMask, const uint64_t* inBits,
                                   int all, uint64_t* outBits, int C, int H, int W, int oh, int ow, int op, int dtype,
                                   cbStream_t stream);
/* Launch 2: the listed output pixels from the partials, one workgroup per word of outBits.  Every word of outBits is
 * copied to maskCopy and zeroed; inBits != NULL: its cbinfer_mask_words(H, W) words are zeroed too.  No atomics. */
int cbinfer_adaptive_pool_changed(const float* partials, void* output, uint64_t* inBits, uint64_t* outBits,
                                  uint64_t* maskCopy, int C, int H, int W, int oh, int ow, int op, int dtype,
                                  cbStream_t stream);
/* The whole frame enqueued without a host sync: two launches in mask or every-pixel form, three in list form (capN == 0
 * launches nothing for the list).  inputMask != NULL: mask form; changeIndexes != NULL: list form (capN entries at most,
 * countDev the device-side length or NULL: capN is the length); both NULL: every pixel. */
int cbinfer_cbadaptivepool2d_forward(const void* input, float* partials, void* outputState, const uint64_t* inputMask,
                                     const int32_t* changeIndexes, int capN, const int32_t* countDev, uint64_t* inBits,
                                     uint64_t* outBits, uint64_t* maskCopy, int C, int H, int W, int oh, int ow, int op,
                                     int dtype, cbStream_t stream);

/* ---- change-based peak suppression and peak lists (cb_peaks.hip) ----------------------------------------
 * No counterpart in the reference's library: its pose detector copies the full-resolution heat maps to the host and
 * searches the peaks there.  Torch has no module for the operator either; keypoint heads write it as
 * heat * (max_pool2d(heat, 3, 1, 1) == heat).  Added under ABI 11.
 *   the rule.  The operand is a map v [C, H, W] (batch 1, CB_F32 or CB_F16), the window kH x kW with each of kH, kW one of
 *     3, 5, 7 on its own axis, rH = kH / 2, rW = kW / 2.
 *     1. neighbourhood N(y, x).  cross == 0 ("window"): every in-map pixel (y + dy, x + dx) with |dy| <= rH and
 *        |dx| <= rW, the centre included.  cross == 1 (3 x 3 only): the centre and its in-map 4-neighbours.  Pixels
 *        outside the map do not take part: the -inf padding of a max pool.
 *     2. keep(c, y, x) holds iff v[c, y, x] >= v[c, n] by IEEE comparison for every n of N -- a NaN at the centre or at
 *        any neighbour gives false, +0 and -0 are equal -- and, with hasFloor, (float)v[c, y, x] >= floor (an f32).
 *     3. out[c, y, x] has the bits of v[c, y, x] where keep holds and is +0 elsewhere.
 *     4. peakBits holds one bit per pixel and channel: C cbinfer_mask_words(H, W) words, channel c's at
 *        c cbinfer_mask_words(H, W), each in the row-padded layout of every mask here.  The bit equals keep; the bits of
 *        the row padding are never set.
 *     5. the peak list names the pixels with keep ascending in (c, y, x) -- the order of peakMap[c].nonzero() taken
 *        channel after channel: int32 entries (c, y, x), three per peak, and scores v[c, y, x] in the map's dtype; count
 *        is the TRUE number of peaks and channelStart[0 .. C] the TRUE offsets of the channels (channelStart[C] ==
 *        count).  With a capacity capN < count the first capN entries in that order are written and nothing beyond them.
 *     For cross == 0 this is torch.where((F.max_pool2d(x, k, 1, k // 2) == x) & (x >= floor), x, 0) bit for bit (torch's
 *     pool lets a NaN win, so the equality fails exactly where rule 2 does); on NaN-free non-negative maps also the
 *     product above.  At interior pixels cross == 1 is the four-neighbour test with a threshold of the reference's pose
 *     detector, which crops a border ring where this rule uses the in-map neighbours.
 *   a frame.  The operand's changes come as its row-padded change MASK (cbinfer_mask_words(H, W) words), as an int32
 *     LIST (flat indexes y W + x; entries outside the map are dropped, duplicates and any order are fine), or not at
 *     all: every pixel counts as changed then (the form of a frame that writes a new state).  Listed and recomputed, for
 *     all channels, are the pixels of the FOOTPRINT: those whose kH x kW window (stride 1, padding k / 2) holds a changed
 *     pixel -- cross == 1 uses the 3 x 3 footprint too, a superset of what it needs, which is still the dense result.
 *     out and peakBits keep their bits at every other pixel.  A pixel's bits depend neither on the other listed pixels
 *     nor on the operand's form.
 *   hand-on: maskCopy (cbinfer_mask_words(H, W) words) receives the footprint every frame, all zeros for an empty frame;
 *     `bits`, the working mask (same size, zero on first use), is zero again when the frame ends.
 *   launches: mask or every-pixel form ONE (the footprint of a mask is gathered inside the walk); list form one more in
 *     front (cbinfer_pool_footprint with the window as a stride-1 CB_POOL_MAX pool: 64-bit atomicOr into `bits`).  The
 *     suppression launch has no atomics: the unit of work is (mask word, channel), one wave each, whose 64-bit ballot of
 *     keep becomes the word of peakBits, (old & ~word) | (ballot & word), stored by one lane.
 * Status: a null tensor or mask buffer, x == out, C / H / W < 1, an unknown dtype, two of the mask buffers the same,
 * both a mask and a list, a count without a list, capN < 0: CB_ERR_BADARG; a window that is even or outside 3 .. 7, cross
 * with another window than 3 x 3, a floor that is not finite, H W or 64 C beyond an int32: CB_ERR_UNSUPPORTED.  All
 * arguments are checked before the first launch; a refused call launches nothing. */
typedef struct cbPeaks {
    int kH, kW, cross, hasFloor;
    float floor;
} cbPeaks;
/* host, pure: 1 if the library takes the window, kind and floor (cross and hasFloor are 0 or 1), else 0 */
int cbinfer_peaks_supported(const cbPeaks* peaks);
/* The suppression launch.  mask (may be NULL): the OPERAND's change mask of this frame, whose footprint the launch
 * gathers; all != 0: every pixel is listed; otherwise, or in addition, the footprint stands in `bits` already. */
int cbinfer_peaks_changed(const void* x, void* out, uint64_t* peakBits, const uint64_t* mask, int all, uint64_t* bits,
                          uint64_t* maskCopy, int C, int H, int W, const cbPeaks* peaks, int dtype, cbStream_t stream);
/* The whole frame enqueued without a host sync.  mask != NULL: mask form; list != NULL: list form (capN entries at most,
 * countDev the device-side length or NULL: capN is the length); both NULL: every pixel. */
int cbinfer_cbpeaks_forward(const void* x, void* outputState, uint64_t* peakBits, const uint64_t* mask,
                            const int32_t* list, int capN, const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy,
                            int C, int H, int W, const cbPeaks* peaks, int dtype, cbStream_t stream);
/* The ordered peak list from peakBits, three launches: the peaks of every (channel, row) into work (int32, C H + 1
 * entries); their exclusive scan in place by ONE workgroup, which also stores count and channelStart (C + 1 entries);
 * the entries and scores, one thread per word of peakBits.  No workgroup waits for another one inside a launch and no
 * atomic decides an entry's position.  Every word of peakBits is read every frame: 1 / 32 of the map's bytes in CB_F32.
 * entries (3 capN int32) and scores (capN of the map's dtype) may be NULL when capN == 0.  Status: a null x, peakBits,
 * work, count or channelStart, entries or scores missing with capN > 0, C / H / W < 1, capN < 0, an unknown dtype:
 * CB_ERR_BADARG; C H W beyond an int32: CB_ERR_UNSUPPORTED. */
int cbinfer_peaks_list(const void* x, const uint64_t* peakBits, int32_t* work, int32_t* entries, void* scores, int capN,
                       int32_t* count, int32_t* channelStart, int C, int H, int W, int dtype, cbStream_t stream);

/* replaces conv2d_fg_cpu, cbconv2d_fg_backend.cu:81-112: HOST pointers, host code, race-free. */
void cbinfer_conv2d_fg_cpu(const float* input, const float* prevInput, float* output,
                           const float* weight, float threshold, int no, int ni, int h, int w,
                           int kh, int kw);

#ifdef __cplusplus
}
#endif
#endif /* CBINFER_HIP_H */
