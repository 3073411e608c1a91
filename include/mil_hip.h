/* mil_hip.h — C ABI of libmil_hip.so, the MI355X (gfx950) kernels under the ResNet-26 +
 * attention-MIL hot path.
 *
 * The reference (frankenz/Deep-convolutional-neural-network-ResNet-26-and-Attention-network) is
 * pure Python on stock PyTorch and has no FFI of its own; the "plugin interface" of this path is
 * the `nn.Module` surface of `Attention` (gbm/model.py:114-264).  This header is what a binding
 * for that path binds instead of the cuDNN/ATen library ops the reference dispatches to.  Each
 * entry point names the reference op(s) it replaces (file:line relative to the upstream repo).
 *
 * Conventions
 *   - plain C: raw device pointers, ints, floats; `stream` is a hipStream_t passed as void*.
 *   - every function returns MIL_OK (0) or an error code; nothing allocates, nothing synchronises,
 *     no global state: work is enqueued on `stream`, buffers are caller-owned.
 *   - the only environment read: six test knobs, on every call (MIL_PF_MIN_TILES, MIL_BUFFER_LIMIT_BYTES,
 *     MIL_RES_GRID_CAP, MIL_BLOCK_STRIP, MIL_STEM_WALK, MIL_ENTRY_BWD), with which tests drive small inputs through the
 *     large-launch paths and force either of two equivalent kernels.
 *   - activations are NHWC with channels padded to a multiple of 8 (20->24, 40, 60->64, 80; padded
 *     channels hold zeros); `dtype` selects the activation/weight-operand type:
 *         MIL_DT_F32  (0): exact-fp32 MFMA (v_mfma_f32_16x16x4_f32)  — the parity gate, bit-level
 *         MIL_DT_BF16 (1): bf16 operands, fp32 accumulate (v_mfma_f32_16x16x32_bf16) — the fast path
 *         MIL_DT_F32S (3): fp32 tensors exactly as MIL_DT_F32 (same layouts, same pointwise entry points), convolutions
 *                          and weight gradients as bf16x3 split products: each operand v = hi + lo (two bf16), product =
 *                          lo*hi + hi*lo + hi*hi with fp32 accumulation.  16 significant bits per operand: meets the 1e-3
 *                          gate on logits / attention weights (2.5e-4 measured) at 3/16 of the exact path's matrix time.
 *                          Accepted by mil_pack_conv_weights / mil_pack_job_fill (fragments [hi | lo], the byte count of
 *                          MIL_DT_F32), mil_conv_igemm, mil_conv_wgrad(_workspace), the wide-layer entry points
 *                          mil_wide_pack_weights, mil_wide_conv and mil_wide_wgrad(_workspace) (argument and shape rules,
 *                          packed byte count and workspace byte count of MIL_DT_F32), and — fused forms, where the shape has
 *                          one (MIL_ERR_UNSUPPORTED otherwise: the caller falls back to the un-fused calls) —
 *                          mil_conv_bwd_fused(_workspace) (20-channel layers), mil_conv_block_fwd (20-channel identity
 *                          blocks, maps of at least 8x16), mil_conv_chain (64 / 80 channels on 16x16 / 8x8 maps, and on the
 *                          19x19 / 10x10 maps of 300x300 tiles), mil_conv_s2_entry (all three stage entries: 20 -> 40,
 *                          40 -> 60 and 60 -> 80 channels, i.e. padded 24 -> 40, 40 -> 64, 64 -> 80), mil_conv_wgrad_pair
 *                          (20 -> 40 channels), mil_conv_dgrad_s2 (all three entries: 40 -> 20, 60 -> 40 and 80 -> 60
 *                          channels; the dense-output code MIL_DT_F32S_DGRAD only for the 40 -> 20 entry, cz_p == 40),
 *                          mil_stem_fwd_fused (xs must be null: no space-to-depth copy),
 *                          mil_stem_bwd_fused_nchw(_workspace) and their uint8-feed forms mil_stem_fwd_fused_u8 and
 *                          mil_stem_bwd_fused_u8(_workspace), and mil_stem_dgrad (MIL_PACK_STEM_DGRAD fragments [hi | lo]); every
 *                          pointwise entry point takes MIL_DT_F32 for the same tensors.
 *   - master weights, biases, all gradients of parameters, and the whole MIL head are fp32.
 */
#ifndef MIL_HIP_H
#define MIL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIL_OK 0
#define MIL_ERR_ARG 1
#define MIL_ERR_UNSUPPORTED 2
#define MIL_ERR_LAUNCH 3

#define MIL_DT_F32 0
#define MIL_DT_BF16 1
/* bf16 with the GRADIENT tensors of the 20-channel stage stored dense: dz / addend / dx of mil_conv_bwd_fused, the output of
 * mil_conv_dgrad_s2 (40 -> 20 channels) and g_pool of mil_stem_bwd_fused(_nchw) are [n,H,W,20] (40 bytes per pixel)
 * instead of [n,H,W,24]; every activation (x, act, widx) keeps its padded layout.  These tensors are produced and consumed
 * only by those entry points (autograd's intermediate gradients of gbm/model.py:24-29), so the layout is theirs to choose:
 * 17 % fewer bytes on three of the four tensor passes of the stage's fused backward.  Entry points (or shapes) without a
 * kernel for it return MIL_ERR_UNSUPPORTED; query with the *_workspace functions before choosing it. */
#define MIL_DT_BF16_DGRAD 2
#define MIL_DT_F32S 3
/* MIL_DT_F32S with the same GRADIENT tensors stored dense as fp32: [n,H,W,20] = 80 bytes = five 16-byte pieces per pixel instead
 * of 96 (no padding traffic on three of the four tensor passes of the stage's fused backward).  Accepted by mil_conv_bwd_fused
 * (16x16 tiles: maps of at least 16x16), mil_conv_dgrad_s2 (40 -> 20 channels) and mil_stem_bwd_fused_nchw; query with the
 * *_workspace functions before choosing it. */
#define MIL_DT_F32S_DGRAD 4

#define MIL_PACK_FWD 0   /* B[(tap,ci)][co] = W[co][ci][ky][kx]                     */
#define MIL_PACK_DGRAD 1 /* B[(tap,co)][ci] = W[co][ci][k-1-ky][k-1-kx]             */
#define MIL_PACK_STEM 2  /* 7x7/s2 filter as a 4x4/s1 filter over space-to-depth x  */
#define MIL_PACK_DGRAD_S2 3 /* parity-class order for mil_conv_dgrad_s2; `bias` = 1x1 projection weight */
#define MIL_PACK_STEM_DGRAD 4 /* the 7x7/s2 stem filter as the 4x4 transposed filter of mil_stem_dgrad: cout=20, cin=3, ks=7 only
                               * (any other shape: MIL_ERR_UNSUPPORTED from the three packing entry points); no bias_pad */

/* ABI version of this header (bumped on any signature change). */
int mil_abi_version(void);

/* Streaming device copy dst[0..bytes) = src[0..bytes) in 16-byte pieces (both 16-byte aligned, bytes a multiple of 16).  Not a
 * reference op: the calibration kernel bench.py times to state what a plain read+write stream reaches on the box, next to the
 * 8 TB/s specification its roofline fractions are priced against. */
int mil_stream_copy(void* dst, const void* src, size_t bytes, void* stream);
/* Diagnostic: the hi / lo bf16 split of MIL_DT_F32S as the split-precision kernels apply it to operands on their way into LDS
 * (hi = bf16(v), lo = bf16(v - hi); element pairs (2i, 2i+1) share one v_dot2c_f32_bf16 pair).  v [n] fp32 -> hi, lo [n] bf16 bit
 * patterns; n even.  Finite pairs: bit-identical to the plain subtraction.  A non-finite element makes its pair partner's lo a
 * NaN (Inf * 0 in the dot product). */
int mil_split_probe(const float* v, uint16_t* hi, uint16_t* lo, int n, void* stream);

/* ---- input packing ------------------------------------------------------------------------
 * fp32 NCHW tiles [n,3,H,W] (what `Attention.forward` receives, gbm/model.py:189-196) ->
 * NHWC space-to-depth [n, ceil(H/2), ceil(W/2), 16] of `dtype` (channel = c*4+dy*2+dx, 12 real).
 * Lets the 7x7 stride-2 stem conv (gbm/model.py:24) run as a 4x4 stride-1 implicit GEMM. */
int mil_stem_s2d(const float* x_nchw, void* out, int n, int H, int W, int dtype, void* stream);

/* ---- the uint8 tile feed ------------------------------------------------------------------
 * Every tile the reference's model sees is an 8-bit image behind ToTensor + Normalize(.5,.5) (RoiBuilder.py:193-210): each
 * element of the fp32 [n,3,H,W] tensor is one of 256 values, v = ((u / 255) - 0.5) / 0.5.  The *_u8 entry points take the bytes
 * themselves, x_u8 [n,3,H,W] planar (the fp32 tensor's own indexing, a quarter of its size), and decode them on their way into
 * LDS (reciprocal product + one Newton step = the correctly rounded u / 255 for all 256 codes, then one fma): results are bit
 * for bit those of the fp32 entry point on the decoded tensor, in every compute mode.  Conv zero padding stays 0.0 (code 0
 * decodes to -1: out-of-image loads are committed as zeros).
 * mil_u8_decode_table (HOST): out256[u] = the fp32 value code u decodes to — the kernels' own expression, compiled for the host. */
int mil_u8_decode_table(float* out256);
/* mil_stem_s2d from uint8 tiles: out is bit-identical to mil_stem_s2d of the decoded tensor (MIL_DT_F32 / MIL_DT_BF16).  The
 * feed of the exact-fp32 mode, and of the other two wherever the fused kernels below answer MIL_ERR_UNSUPPORTED. */
int mil_stem_s2d_u8(const uint8_t* x_u8, void* out, int n, int H, int W, int dtype, void* stream);

/* ---- weight packing -----------------------------------------------------------------------
 * fp32 master weights in the reference state-dict layout [Cout][Cin][k][k] ->
 * MFMA B-fragment order [kstep][ntile][64 lanes][8].  `bias_pad` (optional) receives the bias
 * zero-padded to ntile*16 floats.  Element count of the packed buffer: mil_packed_weight_elems. */
int mil_packed_weight_elems(size_t* elems, int cout, int cin, int ks, int mode);
int mil_pack_conv_weights(const float* w, const float* bias, void* wpack, float* bias_pad, int cout, int cin,
                          int ks, int mode, int dtype, void* stream);

/* ---- convolution forward / data-gradient ---------------------------------------------------
 * Replaces nn.Conv2d forward (+bias) fused with LeakyReLU(0.1) and the residual add of
 * BasicResBlock.forward (nnBlocks.py:175-189), the stem conv+LeakyReLU (gbm/model.py:51-52), the
 * 1x1 stride-2 projection (gbm/model.py:38-40), and — run over dz with MIL_PACK_DGRAD weights — the
 * autograd data-gradient of those convs fused with the LeakyReLU backward mask.
 *     y = mask( lrelu?( conv(x) + bias? + res? ) ),   mask(v) = v * (act > 0 ? 1 : slope) if act
 *   x   [n,H,W,cin_p]; y/res/act [n,Ho,Wo,cout_p]; ks in {1,3,4}; stride in {1,2}; pad = leading pad.
 *   zero_insert=1 reads x as if zeros sat between its pixels (transposed stride-2 conv: dgrad of a
 *   stride-2 conv); H,W are then the dims of the small tensor and Ho,Wo the full-resolution dims. */
int mil_conv_igemm(const void* x, const void* wpack, const float* bias_pad, const void* res, const void* act,
                   void* y, int n_img, int H, int W, int cin_p, int Ho, int Wo, int cout_p, int ks, int stride,
                   int pad, int zero_insert, int apply_lrelu, float slope, int dtype, void* stream);

/* The data gradients of a guided-backpropagation walk (`guided_backprop.py` of the reference's vendored saliency toolkit,
 * pytorch-cnn-visualizations-master/src, lines 41-50: every activation hands on (out > 0) * clamp(grad, min=0)).  The operands
 * are mil_conv_igemm's, run over dz with MIL_PACK_DGRAD weights, plus `rule`:
 *     rule == 0:  y = mask( lrelu?( conv(x) + bias? + res? ) ) — mil_conv_igemm's result on the generic implicit-GEMM kernel
 *     rule == 1:  v = lrelu?( conv(x) + bias? + res? );  y = (act > 0 && v > 0) ? v : +0        (act required; slope gates nothing)
 * v is the TOTAL gradient arriving at the activation `act` is the output of (the convolution's own sum plus `res`, the shortcut's
 * share), so the gate sees what the toolkit's hook sees; LeakyReLU(0.1) is read as a ReLU, its 0.1 branch carries nothing.
 * Always the generic kernel (256-pixel tiles where the halo and a filter chunk fit LDS, else 64-pixel tiles), never the
 * persistent, resident or streaming forms: rule 1 is bit for bit the gate applied to rule 0's output for the same operands with
 * act = NULL.  MIL_DT_BF16 / MIL_DT_F32 / MIL_DT_F32S; (cin_p, cout_p) the square widths 24, 40, 64, 80 and the stage-entry
 * gradients 40 -> 24, 64 -> 40, 80 -> 64, stride 1 or zero_insert; anything else: MIL_ERR_UNSUPPORTED.  Null x / wpack / y,
 * rule outside {0,1}, rule 1 without act, another dtype, a size below 1: MIL_ERR_ARG — all decided on the host. */
int mil_conv_dgrad_rule(const void* x, const void* wpack, const float* bias_pad, const void* res, const void* act,
                        void* y, int n_img, int H, int W, int cin_p, int Ho, int Wo, int cout_p, int ks, int stride,
                        int pad, int zero_insert, int apply_lrelu, float slope, int rule, int dtype, void* stream);

/* ---- convolution weight / bias gradient ----------------------------------------------------
 * Replaces the autograd weight- and bias-gradient of the same convs.  dw is written (not
 * accumulated) in the reference layout [cout][cin][k][k] fp32 (k = 7 when stem_mode), db [cout]
 * (may be null).  x [n,H,W,cpad(cin)] (or the 16-channel s2d tensor when stem_mode), dz
 * [n,Ho,Wo,cpad(cout)].  Split-K over workgroups with a fixed-order second pass: bitwise
 * reproducible.  `workspace` must hold mil_conv_wgrad_workspace() bytes.  accumulate=1 adds into dw/db
 * (gradient accumulation straight into the flat gradient bucket) instead of overwriting them. */
int mil_conv_wgrad_workspace(size_t* bytes, int n_img, int H, int W, int cin, int Ho, int Wo, int cout, int ks,
                             int stride, int pad, int stem_mode, int dtype);
int mil_conv_wgrad(const void* x, const void* dz, float* dw, float* db, void* workspace, size_t workspace_bytes,
                   int n_img, int H, int W, int cin, int Ho, int Wo, int cout, int ks, int stride, int pad,
                   int stem_mode, int accumulate, int dtype, void* stream);

/* ---- batched slab reductions -------------------------------------------------------------------------
 * Every weight-gradient producer below (mil_conv_wgrad, mil_conv_wgrad_pair, mil_conv_bwd_fused, mil_stem_bwd_fused) ends in
 * a fixed-order reduction of per-workgroup partial sums ("slabs" in its workspace) into dW/db: 28 launches of ~10 us in one
 * backward pass of the encoder (autograd of nnBlocks.py:169-171 / gbm/model.py:24).  Between mil_reduce_defer_begin and
 * mil_reduce_defer_end the producers called on THIS thread record that reduction as a job in the caller's host table
 * (max_jobs records of mil_reduce_job_bytes() bytes) instead of launching it; mil_wgrad_reduce_all then runs every recorded
 * job in ONE launch (same summation trees: bit-identical to the per-call reductions).  Contract: each producer's workspace
 * must stay untouched until mil_wgrad_reduce_all has run on the same stream; `jobs_dev` is a device copy of the table,
 * `jobs_host` the table itself; at most 64 jobs per table.  This is the library's only state: thread-local, and empty
 * outside a begin/end pair. */
int mil_reduce_job_bytes(void);
int mil_reduce_defer_begin(void* jobs_host, int max_jobs);
int mil_reduce_defer_end(int* njobs);
int mil_wgrad_reduce_all(const void* jobs_dev, const void* jobs_host, int njobs, void* stream);

/* ---- fused backward of a 3x3 stride-1 conv (bf16 path, narrow layers) --------------------------
 * One pass over dz and x yields BOTH autograd results of nn.Conv2d (nnBlocks.py:169-171):
 *     dx = (conv^T(dz, W) + addend?) * (apply_mask ? lrelu'(x) : 1)      and      dW, db
 * (replaces one mil_conv_igemm dgrad launch + one mil_conv_wgrad launch and their second read of x and
 * dz).  dz [n,H,W,cpad(cout)], x/addend/dx [n,H,W,cpad(cin)], wpack_dgrad = MIL_PACK_DGRAD weights.
 * Returns MIL_ERR_UNSUPPORTED for shapes without a fused kernel (caller then uses the two calls). */
int mil_conv_bwd_fused_workspace(size_t* bytes, int n_img, int H, int W, int cout, int cin, int ks, int pad, int dtype);
int mil_conv_bwd_fused(const void* dz, const void* wpack_dgrad, const void* x, const void* addend, void* dx, float* dw,
                       float* db, void* workspace, size_t workspace_bytes, int n_img, int H, int W, int cout, int cin,
                       int ks, int pad, int apply_mask, int accumulate, float slope, int dtype, void* stream);

/* ---- pooling -------------------------------------------------------------------------------
 * MaxPool2d(3, stride 2, pad 1) (gbm/model.py:26,53): y [n,Ho,Wo,cp], Ho=(H-1)/2+1; `widx` records per
 * output element (uint8, same shape as y) the winning tap (bits 0-3) and whether the winner is <= 0
 * (bit 4).  The backward gathers gy through widx into gx [n,H,W,cp]; with apply_lrelu_mask it also
 * applies the LeakyReLU backward of the stem activation (gbm/model.py:25,52) from bit 4, so the stem
 * output itself is never re-read. */
int mil_maxpool_fwd(const void* x, void* y, uint8_t* widx, int n, int H, int W, int cp, int dtype, void* stream);
int mil_maxpool_bwd(const void* gy, const uint8_t* widx, void* gx, int n, int H, int W, int cp,
                    int apply_lrelu_mask, float slope, int dtype, void* stream);
/* mil_maxpool_bwd under guided backpropagation (see mil_conv_dgrad_rule), for the stem's LeakyReLU: the same gather, then
 *     gx = (winner > 0 && s > 0) ? s : +0,    s = the SUM of the window contributions of the pixel (what
 * mil_maxpool_bwd(apply_lrelu_mask = 0) writes) — the gate applies to the total gradient arriving at the activation, not to
 * each window's share; the winner's sign is bit 4 of widx.  MIL_DT_BF16 / MIL_DT_F32 (the fp32 storage of both fp32 modes).
 * Null pointer, cp < 8 or cp % 8 != 0, n < 0, H or W < 1, another dtype: MIL_ERR_ARG; nothing to do: MIL_OK, no launch. */
int mil_maxpool_bwd_guided(const void* gy, const uint8_t* widx, void* gx, int n, int H, int W, int cp, int dtype, void* stream);

/* Tile pre-processing on the device (RoiBuilder.py:193-210: Pad(100) -> RandomCrop(roi) -> Resize(res) ->
 * RandomHorizontalFlip -> RandomVerticalFlip -> ToTensor -> Normalize(.5,.5); `img_finalize_flat` without pad/crop/flips):
 * uint8 ROIs [T,S,S,3] -> fp32 [T,3,R,R] in [-1,1], the tensor gbm/classify_combined.py:432 hands to the model.  The
 * resampling is Pillow's two-pass fixed-point bilinear filter, bit-exact.  mil_resize_plan/_coeffs run on the HOST and fill
 * host arrays (bounds [R*2], kk [R*ksize]) that the caller uploads once per (S,R); params [T,4] = (top, left, hflip,
 * vflip) drawn by the caller (top/left in [0, 2*pad]) or null for the flat chain. */
int mil_resize_plan(int in_size, int out_size, int* ksize);
int mil_resize_coeffs(int in_size, int out_size, int32_t* bounds, int32_t* kk);
/* The same tables for either of Pillow's filters: MIL_FILTER_BILINEAR (the triangle, support 1: exactly mil_resize_plan /
 * mil_resize_coeffs) or MIL_FILTER_LANCZOS (w(x) = sinc(x) sinc(x/3) on [-3, 3), sinc(0) = 1, support 3 max(scale, 1): what
 * Image.resize(..., Image.LANCZOS) — the toolkit's ANTIALIAS — builds).  Normalised in double, rounded to 22 bits as
 * (int)(+-0.5 + k 2^22) with the sign of k: Lanczos coefficients can be negative.  Same layout: bounds [out*2] = (first source
 * index, count), kk [out*ksize].  HOST functions.  Sizes below 1, another filter or a null pointer: MIL_ERR_ARG. */
#define MIL_FILTER_LANCZOS 1  /* the values of Pillow's Image.LANCZOS / Image.BILINEAR */
#define MIL_FILTER_BILINEAR 2
int mil_resample_plan(int in_size, int out_size, int filter, int* ksize);
int mil_resample_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk);
int mil_tile_preprocess(const uint8_t* rois, const int32_t* params, const int32_t* bounds_host, const int32_t* bounds_dev,
                        const int32_t* kk_dev, float* out, int T, int S, int pad, int R, void* stream);
/* Same chain, output as the bf16 space-to-depth NHWC tensor xs [T,R/2,R/2,16] (channel = c*4 + dy*2 + dx, 12 real, 4 zero)
 * that mil_stem_fwd_fused_xs / mil_stem_bwd_fused read: values = the bf16 roundings of mil_tile_preprocess's.  R even. */
int mil_tile_preprocess_s2d(const uint8_t* rois, const int32_t* params, const int32_t* bounds_host, const int32_t* bounds_dev,
                            const int32_t* kk_dev, void* xs, int T, int S, int pad, int R, void* stream);
/* Same chain, output left as bytes: out [T,3,R,R] uint8 planar = Pillow's resized (cropped, flipped) image before ToTensor +
 * Normalize (RoiBuilder.py:203-204 are the stem kernels' decode table).  Lossless: the uint8 feed decodes it to exactly
 * mil_tile_preprocess's values, so it serves all three compute modes.  Any R. */
int mil_tile_preprocess_u8(const uint8_t* rois, const int32_t* params, const int32_t* bounds_host, const int32_t* bounds_dev,
                           const int32_t* kk_dev, uint8_t* out, int T, int S, int pad, int R, void* stream);
/* The three entries above for ROIs that are WINDOWS of a larger image left in place (array_read_region followed by the
 * chains, RoiBuilder.py:117-124,193-210) instead of tiles of a contiguous stack: row y of window t starts at byte
 * base + win_off_dev[t] + y * row_pitch, at any byte alignment — mil_roi_stats' source convention (a slide [H,W,3]: row_pitch =
 * 3W, win_off = (row*W + col)*3; a stack: 3S and t*3*S*S).  win_off_dev is a DEVICE array [T]; base_bytes is the size of the
 * source: loads go through buffer descriptors that end with it, so no over-fetch leaves it.  Left and right of a window the
 * source's own pixels are masked: Pad() pads with zeros.  params, tables, outputs, T <= 65535 per call and status codes as
 * above, results bit for bit those of the stack entries for the same pixels; additionally null base / win_off_dev,
 * base_bytes < 0 or row_pitch < 3S: MIL_ERR_ARG, and a row_pitch so large that the source rows of eight output rows leave
 * 31-bit offsets: MIL_ERR_UNSUPPORTED — decided on the host before any GPU call. */
int mil_tile_preprocess_win(const uint8_t* base, int64_t base_bytes, const int64_t* win_off_dev, int64_t row_pitch,
                            const int32_t* params, const int32_t* bounds_host, const int32_t* bounds_dev,
                            const int32_t* kk_dev, float* out, int T, int S, int pad, int R, void* stream);
/* RoiBuilder.py:117-124,193-210 with mil_tile_preprocess_s2d's output (xs [T,R/2,R/2,16] bf16, R even). */
int mil_tile_preprocess_win_s2d(const uint8_t* base, int64_t base_bytes, const int64_t* win_off_dev, int64_t row_pitch,
                                const int32_t* params, const int32_t* bounds_host, const int32_t* bounds_dev,
                                const int32_t* kk_dev, void* xs, int T, int S, int pad, int R, void* stream);
/* RoiBuilder.py:117-124,193-210 with mil_tile_preprocess_u8's output (out [T,3,R,R] uint8 planar, any R). */
int mil_tile_preprocess_win_u8(const uint8_t* base, int64_t base_bytes, const int64_t* win_off_dev, int64_t row_pitch,
                               const int32_t* params, const int32_t* bounds_host, const int32_t* bounds_dev,
                               const int32_t* kk_dev, uint8_t* out, int T, int S, int pad, int R, void* stream);

/* Tissue selection (RoiBuilder.py:156-169, the loop body of RoiBuilder.build()): per roi_size window of a whole-slide image the
 * integers from which the reference's two tests are decided — ImageStat.Stat(roi).stddev[0] > 5 (from sum R, sum R^2 and the
 * pixel count) and more than 1000 pixels with h > 120, 50 < v < 210 in roi.convert('HSV').
 *     out[t] = (sum R, sum R^2, #{pixels with h > hue_min and v_min < v < v_max}, S*S)          int64 [n,4], device
 * Window t is the S x S interleaved-RGB uint8 image whose row y starts at byte base + win_off[t] + y * row_pitch, at any byte
 * alignment: a slide [H,W,3] has row_pitch = 3W and win_off = (row*W + col)*3, a contiguous ROI stack [n,S,S,3] has row_pitch =
 * 3S and win_off = t*3*S*S.  win_off is a DEVICE array [n].  base_bytes is the size of the source: loads go through buffer
 * descriptors that end with it, a window (or part of one) outside the source reads as zeros and touches nothing else.
 * The hue test is Pillow's rgb2hsv_row restated in integers (csrc/roi_select.hip), exact for hue_min = 120 on all 2^24 colours.
 * 1 <= S <= 4096 (above: MIL_ERR_UNSUPPORTED, as a row_pitch so large that one row of a window leaves 31-bit offsets); null
 * pointers, S < 1, row_pitch < 3S, n < 0, base_bytes < 0, hue_min outside [0,255]: MIL_ERR_ARG; n == 0: MIL_OK, no launch —
 * all decided on the host before any GPU call.  Any n (launches of 65535 windows).  out is zeroed by the call (same stream). */
int mil_roi_stats(const uint8_t* base, int64_t base_bytes, const int64_t* win_off, int64_t row_pitch, int n, int S,
                  int hue_min, int v_min, int v_max, int64_t* out, void* stream);

/* Attention heat maps (gbm/classify_combined.py:169-218, create_map(): the five tissue axes of `tissue_plots`, :185) rendered at
 * thumbnail scale from the source the windows lie in, instead of imshow() of every kept ROI ([T,1200,1200,3]) and one rectangle
 * patch per tile on the host.  Windows: mil_roi_stats' source convention (base, base_bytes, DEVICE win_off [T], row_pitch, S x S
 * interleaved RGB at any byte alignment, loads through buffer descriptors that end with the source).  D divides S; n = S / D.
 * Window t owns the n x n block of output pixels whose top-left one is (out_pos[t][0], out_pos[t][1]) (row, col; DEVICE int32
 * [T,2]) in each of the five panels of out, uint8 [5,Ht,Wt,3]; the part of a block outside [Ht,Wt] is not stored.  Blocks of
 * two windows must not overlap (the caller's to ensure; overlapping blocks are written in no defined order).  All integer:
 *     m[c]     = (sum over the window's pixels [aD,(a+1)D) x [bD,(b+1)D) of channel c + D*D/2) / (D*D)        for owned pixel (a,b)
 *     panel 0  = m if i0 < 0, else (m*(256 - alpha_tissue) + jet_lut[i0][c]*alpha_tissue + 128) >> 8       (ax[0,0], :189-193)
 *     panel 1  = viridis_lut[feat_idx[t][((a-g)*8/(n-2g))*10 + (b-g)*10/(n-2g)]][c] for g <= a,b < n-g, g = inset / D (0 when
 *                n - 2g < 1); the border of the block and, with feat_idx == NULL, the whole panel are not written   (ax[0,1], :203)
 *     panel 1+k = (255*(256 - alpha_map) + jet_lut[ik][c]*alpha_map + 128) >> 8 where ik >= 0, k = 1..3; else not written
 *                                                                                                        (ax[1,0..2], :194-202)
 * with ik = jet_idx[k*T + t] (DEVICE int16 [4,T]: row 0 the mean map, rows 1-3 the maps; negative = no rectangle, above 104
 * read as 104), jet_lut uint8 [105,3], viridis_lut uint8 [256,3] (may be NULL with feat_idx), feat_idx uint8 [T,80] or NULL, the
 * alphas in 1/256ths.  Pixels no window owns are not touched: the caller supplies the canvas.  The 32-bit channel sums hold
 * 255*D*D + D*D/2 up to D = 4096: D > 4096 or n > 4000 (one output row's sums must fit 48 KB of LDS), and a row_pitch so large
 * that the D source rows of one output row leave 31-bit offsets: MIL_ERR_UNSUPPORTED.  Null pointers (other than feat_idx and,
 * with it, viridis_lut), S < 1, D < 1, S % D != 0, T < 0, base_bytes < 0, row_pitch < 3S, inset < 0, Ht or Wt < 1, an alpha outside
 * [0,256]: MIL_ERR_ARG; T == 0: MIL_OK, no launch — all decided on the host before any GPU call.  Any T (launches of 65535
 * windows).  No atomics on global memory, no workspace: bit-repeatable. */
int mil_heatmap_render(const uint8_t* base, int64_t base_bytes, const int64_t* win_off, int64_t row_pitch, int T, int S, int D,
                       const int32_t* out_pos, const int16_t* jet_idx, const uint8_t* feat_idx, const uint8_t* jet_lut,
                       const uint8_t* viridis_lut, int inset, int alpha_tissue, int alpha_map, uint8_t* out, int Ht, int Wt,
                       void* stream);

/* Colour jitter (RoiBuilder.py:200, the line the reference keeps commented out: transforms.ColorJitter(brightness=0.2,
 * contrast=0.1, saturation=0.05, hue=0.02)) as torchvision's PIL backend computes it, IN PLACE on uint8 planar tiles [T,3,R,R]
 * — what mil_tile_preprocess*_u8 write: after Resize and the flips, before ToTensor —, bit for bit Pillow's bytes.  Per tile t
 * (all DEVICE arrays): order[t] (int32 [T,4]) the ops in the order they are applied, 0 brightness, 1 contrast, 2 saturation,
 * 3 hue, any other value (-1) = no op, each op at most once; factors[t] (float [T,3]) = (fb, fc, fs); hue_shift[t] (int32 [T],
 * its low 8 bits) what adjust_hue adds to h.
 *     blend(d, x, a) = d + a * (x - d) in float32 (a rounded multiply, then a rounded add; no FMA), truncated to uint8 when
 *                      0 <= a <= 1, otherwise 0 where <= 0, 255 where >= 255, truncated between        (libImaging/Blend.c)
 *     L              = (19595 R + 38470 G + 7471 B + 0x8000) >> 16                                          (convert("L"))
 *     brightness     blend(0, x, fb);      saturation  blend(L, x, fs)          (ImageEnhance.Brightness, ImageEnhance.Color)
 *     contrast       blend(m, x, fc), m = (2 sum L + R*R) / (2 R*R) over the tile as it is when the op is reached
 *                    = int(ImageStat.Stat(img.convert("L")).mean[0] + 0.5)                          (ImageEnhance.Contrast)
 *     hue            convert("HSV"), h = (h + hue_shift) mod 256, convert("RGB"): Pillow's rgb2hsv / hsv2rgb with their
 *                    float32 / double number formats; lossy also at shift 0                                   (adjust_hue)
 * lsum (uint32 [T], device) is a caller-owned workspace: the call zeroes it (same stream) and leaves sum L of every tile with a
 * contrast op in it; 255 R*R must fit 32 bits: R > 4096: MIL_ERR_UNSUPPORTED.  Null pointers, T < 0, R < 1: MIL_ERR_ARG;
 * T == 0: MIL_OK, no launch — all decided on the host before any GPU call.  Any R >= 1 (the planes of a tile may start at any
 * byte alignment; no access leaves a plane), any T (launches of 65535 tiles).  Integer sums only: bit-repeatable. */
int mil_color_jitter_u8(uint8_t* tiles, const int32_t* order, const float* factors, const int32_t* hue_shift, uint32_t* lsum,
                        int T, int R, void* stream);

/* H&E stain handling for the same resized tiles, uint8 [T,3,H,W] planar (H != W allowed; a plane may start at any byte
 * alignment): the affine map in optical-density (OD) space that stain normalisation (Macenko et al. 2009) and stain augmentation
 * (Tellez et al. 2018) both are, and the two reductions a Macenko fit needs.  tables (511 floats, DEVICE; mil_amd.ops.od_tables
 * builds them on the host in fp64 with log and rounds once):
 *     tables[v]       = L[v]  = -ln((v + 1) / 256),   v = 0..255   the OD of a byte, L[255] = 0
 *     tables[255 + k] = TH[k] = -ln((k + 0.5) / 256), k = 1..255   strictly decreasing: where the byte goes from k - 1 to k
 *     byte(o)         = #{k : o <= TH[k]}     255 for o <= TH[255], 0 for o > TH[1] (and for a NaN), a tie goes to the brighter byte
 * No exp decides a byte on the device: the kernel finds the count by comparisons against TH (from a guess), so
 * np.searchsorted on the same table gives the same bytes, and byte(L[v]) == v: the identity map returns its input.
 *
 * mil_stain_affine_u8: in place, per pixel and output channel i, with affine[t] (float [T,12], or [1,12] with shared = 1) holding
 * the rows A[i,0], A[i,1], A[i,2], b[i]:
 *     o_i = ((A[i,0] L[r] + A[i,1] L[g]) + A[i,2] L[b]) + b_i     every product and sum rounded once, in that order; no FMA
 * and byte(o_i) is stored; the three bytes of a pixel are read before any is written.  One pointwise launch (65535 tiles each):
 * four consecutive pixels of a plane per access, as one dword where the address lies on the 4-byte grid, byte by byte otherwise;
 * no access leaves a plane.
 *
 * mil_od_moments_u8: a pixel is TISSUE when L[r], L[g], L[b] are all >= beta.  out (double [groups,10]; a group is a tile, bag 0,
 * or the whole stack, bag 1) = the tissue count, sum od_c (3), sum od_c od_d for c <= d (rr, rg, rb, gg, gb, bb): the terms are
 * exact in fp64 and are added one rounded addition at a time in a fixed tree — slice s of MIL_OD_SLICES of a tile owns a run of
 * ceil(ceil(H W / 4) / MIL_OD_SLICES) four-pixel groups; a thread of 256 adds its groups (every 256th) in order, the 64 lanes of
 * a wave by a butterfly, the four waves in order; then a tile's slices in order (bag 0) or, in ONE workgroup, thread i the
 * slice sums i, i + 256, ... of the stack in order and the same wave / workgroup tree (bag 1).  No floating-point atomics: two
 * calls give the same bits.  workspace: T * MIL_OD_SLICES * 10 doubles.  T == 0 with bag 1 writes ten zeros.
 *
 * mil_od_project_u8: with P (float [2,3], DEVICE), p_k = (P[k,0] L[r] + P[k,1] L[g]) + P[k,2] L[b], rounded as above,
 *     mode 0  concentrations   maps [2,T,H,W]: maps[0] = p_0, maps[1] = p_1 at tissue pixels
 *     mode 1  ratio            maps [T,H,W] = p_1 / p_0 (IEEE division) at tissue pixels with p_0 > 0
 * every other pixel gets +inf (the division is not evaluated there); valid[t] (int32 [T]; the call zeroes it) counts tile t's
 * pixels that got a value (integer atomics).  +inf sorts above every value in mil_map_quantile.
 *
 * All three: null pointers, T < 0, H or W < 1, shared / bag / mode outside {0,1}, beta NaN, a workspace too small: MIL_ERR_ARG;
 * H W > 2^31 - 1 - 4096 (or T * MIL_OD_SLICES beyond 32 bits): MIL_ERR_UNSUPPORTED; T == 0: MIL_OK, no launch — all decided on
 * the host before any GPU call. */
#define MIL_OD_SLICES 16
int mil_stain_affine_u8(uint8_t* tiles, const float* affine, const float* tables, int T, int H, int W, int shared, void* stream);
int mil_od_moments_u8(const uint8_t* tiles, const float* tables, int T, int H, int W, float beta, int bag, double* workspace,
                      size_t workspace_bytes, double* out, void* stream);
int mil_od_project_u8(const uint8_t* tiles, const float* tables, const float* P, int T, int H, int W, int mode, float beta,
                      float* maps, int32_t* valid, void* stream);

/* Vahadane's stain fit (Vahadane et al. 2016) for the same stacks: the two stain vectors as a sparse non-negative
 * factorisation of the tissue pixels' ODs v = (L[r], L[g], L[b]) — minimise over W (3 x 2, unit non-negative columns) and
 * h_p >= 0   1/2 sum_p |v_p - W h_p|^2 + lam sum_p (h_p0 + h_p1)   by alternating an exact code step and a block-coordinate
 * dictionary step.  tests/stain_snmf_reference.py restates all of it in numpy.
 *
 * The coder.  coder (float [9], DEVICE) = W[0,0], W[0,1], W[1,0], W[1,1], W[2,0], W[2,1] (W row-major, rounded to fp32), c, d,
 * lam with, in fp64 from the fp64 W, every operation rounded once in the order written,
 *     c = (W[0,0] W[0,1] + W[1,0] W[1,1]) + W[2,0] W[2,1] ;  e = 1 - c c ;  d = 1 / e if e > 0, else 0
 * each rounded once to fp32.  Per pixel, in fp32, every operation rounded once (no FMA):
 *     q_k = ((W[0,k] L[r] + W[1,k] L[g]) + W[2,k] L[b]) - lam
 *     h0 = (q_0 - c q_1) d ;  h1 = (q_1 - c q_0) d
 *     h0 >= 0 and h1 >= 0: (h0, h1);  else h1 < 0: (q_0 if q_0 > 0 else 0, 0);  else: (0, q_1 if q_1 > 0 else 0)
 * — for unit columns with 0 <= c < 1 the exact minimiser of the two-variable non-negative lasso.  DEGENERATE W: collinear
 * columns (e <= 0, or e NaN) get d = 0, which makes h0 = h1 = +-0 for every pixel: every code is zero, every sum below is
 * zero, the update leaves both columns as they are.  d is finite whenever e > 0 (e >= 2^-53), so no NaN reaches a sum.
 *
 * mil_od_snmf_sums_u8: out (double [12]) over the TISSUE pixels of the stack (as mil_od_moments_u8 defines them) =
 *     count, sum h0 h0, sum h0 h1, sum h1 h1, sum v_r h0, sum v_r h1, sum v_g h0, sum v_g h1, sum v_b h0, sum v_b h1, sum h0, sum h1
 * the products of two fp32 values are exact in fp64, and they are added in mil_od_moments_u8's tree for bag 1 (slices, thread,
 * butterfly, waves, one finishing workgroup): no floating-point atomics, two calls give the same bits.  workspace:
 * T * MIL_OD_SLICES * 12 doubles.  T == 0 writes twelve zeros.
 *
 * mil_od_snmf_fit_u8: iters x (sums kernel + finishing kernel) enqueued by ONE call, no host synchronisation.  W (double [6],
 * DEVICE, row-major [3,2]) is read and left updated; moments (double [10], DEVICE) is what mil_od_moments_u8 (bag 1) wrote for
 * the same stack and beta; history (double [iters,2], DEVICE) gets one row per iteration.  One thread of the finishing
 * workgroup, in fp64, every operation rounded once, with A = [[s1, s2], [s2, s3]], B[c,j] = s[4 + 2c + j] of the twelve sums:
 *     f = ((sv2 / 2 - wb) + quad / 2) + lam (s10 + s11)        the objective of the W the codes were made with, where
 *         sv2 = (m4 + m7) + m9 ,  n_jk = (W[0,j] W[0,k] + W[1,j] W[1,k]) + W[2,j] W[2,k]
 *         wb = ((((W[0,0] B[0,0] + W[1,0] B[1,0]) + W[2,0] B[2,0]) + W[0,1] B[0,1]) + W[1,1] B[1,1]) + W[2,1] B[2,1]
 *         quad = (A[0,0] n_00 + (2 A[0,1]) n_01) + A[1,1] n_11
 *     for j = 0, 1 in turn, when A[j,j] > 0:   u_c = W[c,j] + (B[c,j] - (W[c,0] A[0,j] + W[c,1] A[1,j])) / A[j,j], u_c < 0 -> 0,
 *         nn = (u_0 u_0 + u_1 u_1) + u_2 u_2 ;  when nn > 0:  W[c,j] = u_c / sqrt(nn)       (otherwise column j stays)
 *     history row = (f, the largest |new W[c,j] - old W[c,j]|);  then c, d and the fp32 W of the next iteration's coder.
 * workspace: T * MIL_OD_SLICES * 12 + MIL_SNMF_EXTRA doubles.  T == 0: the finishing kernel alone, W unchanged, f = 0.
 *
 * mil_od_code_u8: the "sparse" form of mil_od_project_u8 — maps (float [2,T,H,W]) = (h0, h1) of the coder at tissue pixels,
 * +inf elsewhere; valid as there.
 *
 * All three: null pointers, T < 0, H or W < 1, beta NaN, lam NaN or negative, iters < 1, a workspace too small: MIL_ERR_ARG;
 * shapes as above: MIL_ERR_UNSUPPORTED; decided on the host before any GPU call. */
#define MIL_SNMF_TERMS 12
#define MIL_SNMF_EXTRA 20
int mil_od_snmf_sums_u8(const uint8_t* tiles, const float* tables, const float* coder, int T, int H, int W, float beta,
                        double* workspace, size_t workspace_bytes, double* out, void* stream);
int mil_od_snmf_fit_u8(const uint8_t* tiles, const float* tables, double* W, const double* moments, int T, int H, int Wd, float lam,
                       int iters, float beta, double* workspace, size_t workspace_bytes, double* history, void* stream);
int mil_od_code_u8(const uint8_t* tiles, const float* tables, const float* coder, int T, int H, int W, float beta, float* maps,
                   int32_t* valid, void* stream);

/* Rotation / affine augmentation of uint8 RGB images: torchvision's RandomAffine / RandomRotation as its PIL backend computes
 * them, Image.transform(size, Image.AFFINE, m, Image.BILINEAR, fillcolor=fill), bit for bit Pillow's bytes.  matrices (double
 * [n,6], DEVICE) holds a0..a5 per image: the map from OUTPUT pixel centres to INPUT coordinates.  For a source of W x H pixels
 * and output pixel (x, y), each channel separately, in IEEE double with every operation rounded once in the order written (no
 * FMA):
 *     xs = x + 0.5 ; ys = y + 0.5
 *     xin = (a0*xs + a1*ys) + a2          yin = (a3*xs + a4*ys) + a5
 *     not (0 <= xin < W and 0 <= yin < H):  out = fill   (all channels; a NaN coordinate counts as outside)
 *     xf = xin - 0.5 ; yf = yin - 0.5 ; X = floor(xf) ; Y = floor(yf) ; dx = xf - X ; dy = yf - Y
 *     x0 = clip(X, 0, W-1) ; x1 = clip(X+1, 0, W-1) ; y0 = clip(Y, 0, H-1)
 *     v1 = p[y0][x0] + (p[y0][x1] - p[y0][x0]) * dx
 *     v2 = p[Y+1][x0] + (p[Y+1][x1] - p[Y+1][x0]) * dx   if 0 <= Y+1 < H   else v1
 *     out = (uint8) trunc( v1 + (v2 - v1) * dy )
 * Bilinear only (Pillow's NEAREST is a separate 16.16 fixed-point path).  Integer matrix entries give dx = dy = 0: a bit copy,
 * so the quarter turns come out of the same kernel.
 *
 * Addressing, in bytes.  Channel c of source pixel (xx, yy) of image t is
 *     src[t * src_tile_stride + yy * src_row_stride + xx * src_pix_stride + c * src_chan_stride]       (64-bit products)
 * and channel c of output pixel number i = y * ow + x of image t is
 *     dst[t * 3 * ow * oh + i * dst_pix_stride + c * dst_chan_stride]
 * (the destination is a dense stack of n images of 3 * ow * oh bytes).  The layouts in use:
 *     planar       [n,3,H,W] -> [n,3,oh,ow]   src (3HW, W, 1, HW),    dst (1, ow*oh)
 *     interleaved  [n,H,W,3] -> [n,oh,ow,3]   src (3HW, 3W, 3, 1),    dst (3, 1)
 *     slide        [H,W,3]   -> [n,oh,ow,3]   src (0,   3W, 3, 1),    dst (3, 1): every window reads the SAME image, the caller
 *                  adds the window's origin (col, row) to (a2, a5); what lies outside the slide, and only that, becomes fill
 * Four consecutive output pixels per thread: one dword per plane (dst_pix_stride 1) or three consecutive dwords (dst strides
 * (3, 1)) at any byte alignment, byte stores for the last, partial group of an image and for any other strides.  No access
 * leaves the source image or the destination stack.  fill_rgb = r | g << 8 | b << 16.
 * Null pointers, n < 0, W / H / ow / oh < 1, a negative src_tile_stride, any other stride < 1: MIL_ERR_ARG; ow * oh >
 * 2^31 - 1 - 1024: MIL_ERR_UNSUPPORTED; n == 0: MIL_OK, no launch — all decided on the host before any GPU call.  Any n
 * (launches of 65535 images). */
int mil_affine_u8(const uint8_t* src, int64_t src_tile_stride, int64_t src_row_stride, int64_t src_pix_stride,
                  int64_t src_chan_stride, int W, int H, uint8_t* dst, int64_t dst_pix_stride, int64_t dst_chan_stride, int ow, int oh,
                  const double* matrices, uint32_t fill_rgb, int n, void* stream);

/* Elastic deformation fused into that resampling: mil_affine_u8 with one more term in the source coordinate, so a rotated AND
 * deformed image is interpolated once.  Everything mil_affine_u8 takes, plus (all DEVICE arrays)
 *     ctrl  double [n,2,ly,lx]   one control lattice per image: component 0 the x displacement, component 1 the y displacement,
 *                                in SOURCE pixels; ly = gy + 3, lx = gx + 3 where gy, gx >= 1 are the numbers of cells the
 *                                OUTPUT image is divided into
 *     iy    int32 [oh], wy double [oh,4]      the rows' table pair: first lattice row and the four weights of output row y
 *     ix    int32 [ow], wx double [ow,4]      the same for the columns
 * For output pixel (x, y), with c = ctrl[t][k], k = 0 for dx and k = 1 for dy:
 *     r_i = ((wy[y][0]*c[iy[y]+0][ix[x]+i] + wy[y][1]*c[iy[y]+1][ix[x]+i]) + wy[y][2]*c[iy[y]+2][ix[x]+i]) + wy[y][3]*c[iy[y]+3][ix[x]+i]
 *                                                                                                                  i = 0..3
 *     d   = ((wx[x][0]*r_0 + wx[x][1]*r_1) + wx[x][2]*r_2) + wx[x][3]*r_3
 *     xin = ((a0*xs + a1*ys) + a2) + dx          yin = ((a3*xs + a4*ys) + a5) + dy
 * and from xin, yin onward mil_affine_u8's contract word for word: inside test, fill, xf, taps, v1, v2, truncation.  IEEE double,
 * every product and sum rounded once in the order written, nothing fused.  In the slide-window form the caller has added the
 * window's origin to a2 and a5 first, as for mil_affine_u8.  The tables of the uniform cubic B-spline (mil_amd.ops.elastic_tables,
 * numpy doubles on the host), for x = 0..size-1 of an axis of `size` output pixels divided into `cells` cells:
 *     u = ((x + 0.5) * cells) / size ;  i = min(floor(u), cells-1) ;  t = u - i ;  s = 1 - t ;  t2 = t*t ;  t3 = t2*t
 *     w0 = ((s*s)*s)/6      w1 = ((3*t3 - 6*t2) + 4)/6      w2 = (((-3*t3 + 3*t2) + 3*t) + 1)/6      w3 = t3/6
 * A lattice of zeros (+0.0 or -0.0) changes neither the inside test nor a tap: the bytes are mil_affine_u8's, hence Pillow's.  The
 * weights are non-negative and sum to 1 within rounding, so |d| does not exceed the largest |ctrl| entry by more than rounding.
 * The kernel clamps iy to [0, ly-4] and ix to [0, lx-4] (valid tables lie there): no access leaves the lattice, the tables, the
 * source image or the destination stack.  Addressing, thread layout and store paths are mil_affine_u8's.
 * Null pointers, n < 0, W / H / ow / oh < 1, ly or lx < 4, a negative src_tile_stride, any other stride < 1: MIL_ERR_ARG; ow * oh >
 * 2^31 - 1 - 1024: MIL_ERR_UNSUPPORTED; n == 0: MIL_OK, no launch — all decided on the host before any GPU call.  Any n
 * (launches of 65535 images; the lattice pointer advances with the matrices). */
int mil_affine_elastic_u8(const uint8_t* src, int64_t src_tile_stride, int64_t src_row_stride, int64_t src_pix_stride,
                          int64_t src_chan_stride, int W, int H, uint8_t* dst, int64_t dst_pix_stride, int64_t dst_chan_stride,
                          int ow, int oh, const double* matrices, uint32_t fill_rgb, int n, const double* ctrl, int ly, int lx,
                          const int32_t* iy, const double* wy, const int32_t* ix, const double* wx, void* stream);

/* Forward of a whole identity-shortcut residual block in one pass (bf16 path; nnBlocks.py:175-189 with
 * downsample=None): o1 = lrelu(conv3x3(x)+b1) — written because the backward needs it — and
 * y = lrelu(conv3x3(o1)+b2+x).  x is read once (operand and residual), the mid activation feeds conv2 from LDS.
 * cp in {24, 40}, H and W >= 16; otherwise MIL_ERR_UNSUPPORTED (caller: two mil_conv_igemm calls). */
/* Two 3x3 stride-1 convs back to back on the small maps of the last two stages — 80 channels on 8x8 maps, 64 channels on
 * 16x16 maps (layers 4 and 3 at 256x256 tiles) —, one launch: a workgroup keeps whole images in LDS (no halo exchange
 * between workgroups on whole images) and streams both filters:
 *     outA = epiA( convA(x) ),   outB = epiB( convB(outA) ),   epi(v) = mask( lrelu?( v + bias? + res? ) )
 * i.e. mil_conv_igemm's epilogue contract for each.  That is BasicResBlock.forward with an identity shortcut
 * (nnBlocks.py:175-189: A = conv1+bias+lrelu -> o1, B = conv2+bias+x+lrelu -> out, resB = x) and the block's data-gradient
 * chain (A = conv2^T with MIL_PACK_DGRAD weights masked by o1 -> dmid, B = conv1^T + dz masked by x -> dx).  bf16,
 * (cp, H, W) in {(80, 8, 8), (64, 16, 16)}; otherwise MIL_ERR_UNSUPPORTED (the caller runs two mil_conv_igemm calls —
 * which take the same pixel-resident kernel one conv at a time on these shapes). */
int mil_conv_pair(const void* x, const void* wpackA, const float* biasA, const void* resA, const void* actA, int lreluA,
                  void* outA, const void* wpackB, const float* biasB, const void* resB, const void* actB, int lreluB,
                  void* outB, int n_img, int H, int W, int cp, float slope, int dtype, void* stream);

/* The general form: a chain of 1..6 such convs on the same resident images, one launch —
 *     out_0 = epi_0( conv_0(x) ),   out_k = epi_k( conv_k(out_{k-1}) )
 * where the res / act operand of a conv may be the output of an EARLIER conv of the chain (every lane re-reads exactly
 * the bytes it stored itself).  Five convs are everything of the last stage behind its stride-2 entry convs (conv2 of the
 * entry block + two identity blocks, gbm/model.py:29), or the stage's whole data-gradient chain.  `convs` is a HOST array.
 * Same shapes and error behaviour as mil_conv_pair. */
typedef struct MilChainConv {
    const void* wpack;      /* MIL_PACK_FWD / MIL_PACK_DGRAD fragments */
    const float* bias;      /* padded bias or NULL */
    const void* res;        /* [n,H,W,cp] or NULL */
    const void* act;        /* [n,H,W,cp] or NULL */
    void* out;              /* [n,H,W,cp] */
    int lrelu;
    int pad_;
} MilChainConv;
int mil_conv_chain(const void* x, const MilChainConv* convs, int nconv, int n_img, int H, int W, int cp, float slope,
                   int dtype, void* stream);

/* Forward of a whole identity-shortcut block in one pass (nnBlocks.py:175-189):
 *     o1 = lrelu(conv3x3(x) + bias1),   y = lrelu(conv3x3(o1) + bias2 + x)
 * x is read once (operand and residual), o1 and y are written (what the backward needs), the mid activation goes from the
 * accumulators to LDS.  bf16: cp in {24, 40}, H and W >= 16;  MIL_DT_F32S: cp = 24, H >= 8, W >= 16;  otherwise
 * MIL_ERR_UNSUPPORTED (caller: two mil_conv_igemm calls — same results bit for bit in bf16, to fp32 rounding in split precision).
 * Two kernels per precision, same arithmetic per output element (bit-identical, tested): tiles of one image (16x16 / 16x8
 * pixels, input halo staged per tile), or — maps 64 pixels wide (bf16: also 128) and enough images to fill the resident
 * workgroups evenly, about 512 — a row walk: one workgroup per image, input and mid activation in LDS rings, every input
 * pixel fetched once.  MIL_BLOCK_STRIP=0/1 (a test knob) forces either form. */
int mil_conv_block_fwd(const void* x, const void* wpack1, const float* bias1, const void* wpack2, const float* bias2,
                       void* o1, void* y, int n_img, int H, int W, int cp, float slope, int dtype, void* stream);

/* Forward of a stage-entry block's two stride-2 convs in one pass over the block input (bf16 path):
 *   y1 = lrelu(conv3x3_s2(x) + bias)   (nnBlocks.py:176-177)      y2 = conv1x1_s2(x)   (gbm/model.py:38-40)
 * wpack3 / wpack1: MIL_PACK_FWD fragments of the two filters.  (cin_p,cout_p) in {(24,40),(40,64),(64,80)}; otherwise
 * MIL_ERR_UNSUPPORTED (caller: two mil_conv_igemm calls). */
int mil_conv_s2_entry(const void* x, const void* wpack3, const float* bias_pad, const void* wpack1, void* y1, void* y2,
                      int n_img, int H, int W, int cin_p, int cout_p, float slope, int dtype, void* stream);

/* Weight gradients of a stage-entry block's two stride-2 convs from one pass over the block input (bf16 path; autograd
 * of the convs built at gbm/model.py:37-41): dw3 [cout,cin,3,3] and db3 [cout] from dz1 (gradient of the 3x3/s2 conv's
 * output), dw1 [cout,cin,1,1] from dz2 (gradient of the projection's output); x [n,H,W,cpad(cin)], dz1/dz2
 * [n,Ho,Wo,cpad(cout)].  The projection's A operand is the centre-tap rows the 3x3 weight gradient stages anyway.
 * (cin,cout) padded in {(24,40),(40,64),(64,80)}; otherwise MIL_ERR_UNSUPPORTED (caller: two mil_conv_wgrad calls). */
int mil_conv_wgrad_pair_workspace(size_t* bytes, int n_img, int H, int W, int cin, int Ho, int Wo, int cout, int dtype);
int mil_conv_wgrad_pair(const void* x, const void* dz1, const void* dz2, float* dw3, float* db3, float* dw1,
                        void* workspace, size_t workspace_bytes, int n_img, int H, int W, int cin, int Ho, int Wo,
                        int cout, int accumulate, int dtype, void* stream);

/* Data gradient of a stage-entry block's input in one pass (bf16 path; autograd of nnBlocks.py:175-189 for the
 * blocks built with stride 2 + projection at gbm/model.py:37-41):
 *   y = lrelu'(act) * ( conv3x3_s2^T(dz1) + conv1x1_s2^T(dz2) )
 * computed per output parity class over the compact dz maps (no zero-insert halo, no full-resolution temporary for
 * the projection term).  wpack: mil_pack_conv_weights(..., mode MIL_PACK_DGRAD_S2) of the 3x3 weight with the 1x1
 * projection weight passed in the `bias` argument (or null).  dz1/dz2 [n,h,w,cz_p], act/y [n,H,W,cx_p],
 * h = (H-1)/2+1; (cz_p,cx_p) in {(40,24),(64,40),(80,64)}; otherwise MIL_ERR_UNSUPPORTED (caller: two
 * mil_conv_igemm calls with zero_insert). */
int mil_conv_dgrad_s2(const void* dz1, const void* dz2, const void* wpack, const void* act, void* y, int n_img,
                      int h, int w, int cz_p, int H, int W, int cx_p, float slope, int dtype, void* stream);

/* Backward of a stage-entry block's two stride-2 convs in ONE launch (bf16 path): the data gradient of mil_conv_dgrad_s2 and
 * the weight gradients of mil_conv_wgrad_pair from one pass over dz1, dz2 and the block input,
 *   dx  = lrelu'(xin) * ( conv3x3_s2^T(dz1) + conv1x1_s2^T(dz2) )        (masked = 0: no lrelu' factor)
 *   dw3 [cout,cin,3,3], db3 [cout] from (xin, dz1);   dw1 [cout,cin,1,1] from (xin, dz2)
 * Every result is bit-identical to those two entry points': dx by the same parity-class arithmetic; the weight gradients because
 * the kernel sums the same dz tiles on the same workgroups in the same k-step order as mil_conv_wgrad_pair's kernel and ends in
 * the same two fixed-order slab reductions (deferrable: mil_reduce_defer_begin).  wpack: MIL_PACK_DGRAD_S2 fragments, as for
 * mil_conv_dgrad_s2; dz1/dz2 [n,h,w,cpad(cout)], xin and dx [n,H,W,cpad(cin)] (MIL_DT_BF16_DGRAD: dx [n,H,W,20]), h = (H-1)/2+1.
 * bf16; (cin,cout) = (40,60) on maps with a side above 8 pixels, (20,40) above 16; everything else MIL_ERR_UNSUPPORTED (caller:
 * mil_conv_wgrad_pair + mil_conv_dgrad_s2).  MIL_ENTRY_BWD=0 (a test knob) turns it off; MIL_RES_GRID_CAP caps its grid
 * (the sums then take another order). */
int mil_conv_entry_bwd_workspace(size_t* bytes, int n_img, int h, int w, int cout, int H, int W, int cin, int dtype);
int mil_conv_entry_bwd(const void* dz1, const void* dz2, const void* wpack, const void* xin, void* dx, float* dw3,
                       float* db3, float* dw1, void* workspace, size_t workspace_bytes, int n_img, int h, int w,
                       int cout, int H, int W, int cin, int masked, float slope, int accumulate, int dtype, void* stream);

/* Fused forward of the whole stem (bf16 path): space-to-depth + Conv2d(3,C,7,2,3) + bias + LeakyReLU +
 * MaxPool2d(3,2,1) in one pass over the fp32 NCHW tiles (gbm/model.py:24-26,51-53; alt_resnet.py:81-84,128-131
 * with slope 0).  Writes xs [n,H/2,W/2,16] (kept for the stem weight gradient; NULL = keep none, the backward is
 * then mil_stem_bwd_fused_nchw), pool [n,Hp,Wp,cout_p] and the
 * winner records widx (format of mil_maxpool_fwd); the intermediate tensors of mil_stem_s2d -> mil_conv_igemm(ks=4) ->
 * mil_maxpool_fwd are never materialised.  cout_p 64 (alt_resnet): bit-identical to that chain.  cout_p 24 (the 20-channel
 * stem, round 5): the maximum is taken over the fp32 accumulators in registers, as the reference pools fp32 activations
 * (gbm/model.py:51-53) — the chain pools the bf16-rounded stem tensor — so pool agrees with the chain's except where the
 * position code kept in the low four mantissa bits moves a bf16 rounding (< 1e-3 of the elements, one bf16 step), and
 * the recorded winner is the fp32 maximum (values that agree to 2^-19 compare by position; exact ties arise only between
 * identical input patches, whose weight-gradient contributions are identical whichever of them the gradient is routed to).
 * The packed filter (MIL_PACK_STEM) of a 20-channel stem carries six K-packed k-steps behind the eight standard ones
 * (mil_packed_weight_elems says so); bias_pad needs 32 floats.  H even, W % 4 == 0, x 16-byte aligned, otherwise
 * MIL_ERR_UNSUPPORTED (the caller then uses the three calls).
 * Two kernels for the 20-channel stem, bit-identical pool / widx: 8x16-pooled-pixel tiles, or — W == 256, xs == NULL and enough
 * images to fill the resident workgroups evenly, about 512 — a row walk (one workgroup per image, the space-to-depth rows in an
 * LDS ring, every input byte fetched once).  MIL_STEM_WALK=0/1 (a test knob) forces either form. */
int mil_stem_fwd_fused(const float* x_nchw, const void* wpack, const float* bias_pad, void* xs, void* pool,
                       uint8_t* widx, int n_img, int H, int W, int cout_p, float slope, int dtype, void* stream);
/* The same pass fed by the bf16 space-to-depth tensor xs [n,H2,W2,16] itself (mil_tile_preprocess_s2d's output): a
 * pre-processed tile then never exists as fp32 (RoiBuilder.py:193-210 -> gbm/model.py:24,51 without the fp32 stack in
 * between).  pool / widx are bit-identical to mil_stem_fwd_fused on the fp32 tiles xs is the bf16 rounding of; the
 * backward is mil_stem_bwd_fused(xs, ...).  bf16 only.  (The kernel keeps the next pixel's channels 8-11 in the padding
 * channels 12-15 of its LDS copy of a record; the tensor's own padding channels are not read and need not be zero.) */
int mil_stem_fwd_fused_xs(const void* xs, const void* wpack, const float* bias_pad, void* pool, uint8_t* widx, int n_img,
                          int H2, int W2, int cout_p, float slope, int dtype, void* stream);
/* The same pass fed by uint8 tiles x_u8 [n,3,H,W] (the uint8 feed above; RoiBuilder.py:203-204 -> gbm/model.py:24-26,51-53 without
 * the fp32 stack in between): mil_stem_fwd_fused with xs == NULL.  cout_p == 24 (the 20-channel stem): dtype MIL_DT_BF16 or
 * MIL_DT_F32S, the tiled and the row-walk kernel are chosen by the same rule (MIL_STEM_WALK included), the backward is
 * mil_stem_bwd_fused_u8.  cout_p == 64 (alt_resnet's stem): MIL_DT_BF16 only (MIL_DT_F32S is MIL_ERR_UNSUPPORTED: there is no
 * fused 64-channel split-precision stem for any feed), the tiled kernel; the stem weight gradient reads the space-to-depth
 * tensor, which the caller rebuilds with mil_stem_s2d_u8.  pool / widx are bit-identical to mil_stem_fwd_fused on the decoded
 * tiles.  H even, W % 4 == 0, x_u8 4-byte aligned, else MIL_ERR_UNSUPPORTED (the caller then runs mil_stem_s2d_u8 /
 * mil_conv_igemm / mil_maxpool_fwd). */
int mil_stem_fwd_fused_u8(const uint8_t* x_u8, const void* wpack, const float* bias_pad, void* pool, uint8_t* widx, int n_img,
                          int H, int W, int cout_p, float slope, int dtype, void* stream);

/* Fused backward of the whole stem (bf16 path): max-pool backward + LeakyReLU backward + the 7x7 conv's weight
 * and bias gradient in one pass over xs [n,H2,W2,16] (mil_stem_s2d output), g_pool [n,Hp,Wp,24] (gradient of
 * the pooled output) and widx (mil_maxpool_fwd's winner records).  Replaces mil_maxpool_bwd + mil_conv_wgrad
 * (stem_mode) and the 4x-larger d(stem output) tensor between them.  dw [20,3,7,7], db [20] fp32. */
int mil_stem_bwd_fused_workspace(size_t* bytes, int n, int H2, int W2, int dtype);
int mil_stem_bwd_fused(const void* xs, const void* g_pool, const uint8_t* widx, float* dw, float* db, void* workspace,
                       size_t workspace_bytes, int n, int H2, int W2, float slope, int accumulate, int dtype,
                       void* stream);
/* Same backward when no space-to-depth copy was kept (mil_stem_fwd_fused with xs = NULL): reads the fp32 tiles
 * x [n,3,H,W] themselves and rebuilds the bf16 s2d tile in LDS (H even, W % 4 == 0, x 16-byte aligned, else
 * MIL_ERR_UNSUPPORTED).  The stem then moves 1.07 GB less in the forward and 0.5 GB more in the (compute-bound)
 * backward per 2048 tiles of 256x256.
 * bf16, W == 256 and enough images to fill the resident workgroups evenly (about 512): a row walk (one workgroup per image,
 * s2d rows and pooling windows in LDS rings) instead of 16x16 tiles; dW / db agree between the two forms to fp32 summation
 * order (a workgroup's partial sums cover other pixels).  MIL_STEM_WALK=0/1 (a test knob) forces either form. */
int mil_stem_bwd_fused_nchw_workspace(size_t* bytes, int n, int H, int W, int dtype);
int mil_stem_bwd_fused_nchw(const float* x_nchw, const void* g_pool, const uint8_t* widx, float* dw, float* db,
                            void* workspace, size_t workspace_bytes, int n, int H, int W, float slope, int accumulate,
                            int dtype, void* stream);
/* mil_stem_bwd_fused_nchw reading uint8 tiles x_u8 [n,3,H,W] (the uint8 feed above), for the same four dtype codes (MIL_DT_BF16,
 * MIL_DT_BF16_DGRAD, MIL_DT_F32S, MIL_DT_F32S_DGRAD).  dW / db are bit-identical to the TILED form of mil_stem_bwd_fused_nchw on
 * the decoded tiles (same tiles, same slabs, same reduction).  The bf16 row-walk backward reads fp32 tiles only: this feed runs
 * the tiled kernel at every size, so against a row-walk run of the fp32 feed dW / db agree to fp32 summation order.  H even,
 * W % 4 == 0, x_u8 4-byte aligned, else MIL_ERR_UNSUPPORTED (the caller then runs mil_maxpool_bwd + mil_stem_s2d_u8 +
 * mil_conv_wgrad). */
int mil_stem_bwd_fused_u8_workspace(size_t* bytes, int n, int H, int W, int dtype);
int mil_stem_bwd_fused_u8(const uint8_t* x_u8, const void* g_pool, const uint8_t* widx, float* dw, float* db,
                          void* workspace, size_t workspace_bytes, int n, int H, int W, float slope, int accumulate,
                          int dtype, void* stream);

/* Data gradient of the stem convolution: what autograd of Conv2d(3,20,7,2,3) (gbm/model.py:24) returns for its INPUT when the
 * tiles require a gradient — the step `vanilla_backprop.py` / `grad_times_image.py` of the reference's vendored saliency toolkit
 * (pytorch-cnn-visualizations-master/src) take through the first layer.  dstem [n,H2,W2,24] (H2 = ceil(H/2), W2 = ceil(W/2);
 * bf16 under MIL_DT_BF16, fp32 under MIL_DT_F32 / MIL_DT_F32S) is the gradient of the UN-POOLED stem output with the LeakyReLU
 * mask applied, i.e. mil_maxpool_bwd's output; wpack = MIL_PACK_STEM_DGRAD fragments of conv1.weight.  The forward's 4x4 filter
 * over the 12 space-to-depth channels runs transposed, one implicit GEMM (K = 16 taps x 24 channels) per 16x16 tile of
 * space-to-depth pixels, and the result is stored depth-to-space:
 *     reduce == 0: dx_nchw [n,3,H,W] fp32 (sal is not touched)
 *     reduce == 1: sal [n,H,W] fp32 = max_c |dx| (Simonyan et al.'s saliency map) from the same accumulators; dx_nchw may be
 *                  NULL, the three-channel gradient is then never written
 * Odd H / W: the phantom last space-to-depth row / column is not stored.  No atomics, no workspace: bit-repeatable.
 * Null dstem / wpack, both outputs null, the output `reduce` selects null, reduce outside {0,1}, n < 0, H or W < 1, another
 * dtype: MIL_ERR_ARG; n == 0: MIL_OK, no launch; one image's dstem of 2 GiB or more: MIL_ERR_UNSUPPORTED — all decided on the
 * host before any GPU call. */
int mil_stem_dgrad(const void* dstem, const void* wpack, float* dx_nchw, float* sal, int n, int H, int W, int reduce, int dtype,
                   void* stream);

/* The accumulating form of mil_stem_dgrad(reduce = 0), the inner step of integrated gradients and SmoothGrad:
 *     acc_nchw [n,3,H,W] fp32 = acc_nchw + scale * dx
 * with dx what mil_stem_dgrad writes for the same dstem / wpack / dtype, from the same accumulators: each element is read, updated
 * as __fadd_rn(old, __fmul_rn(scale, dx)) — a product and a sum, never a fused multiply-add — and written back by the one lane that
 * owns it.  No temporary gradient tensor, no atomics, no workspace: bit-repeatable, and bit for bit `acc + scale * dx` in fp32.
 * There is no `reduce` form.  Null dstem / wpack / acc_nchw, n < 0, H or W < 1, another dtype: MIL_ERR_ARG; n == 0: MIL_OK, no
 * launch; one image's dstem of 2 GiB or more: MIL_ERR_UNSUPPORTED — all decided on the host before any GPU call. */
int mil_stem_dgrad_acc(const void* dstem, const void* wpack, float* acc_nchw, float scale, int n, int H, int W, int dtype,
                       void* stream);

/* The gated form of mil_stem_dgrad(reduce = 0), the last launch of guided Grad-CAM (`guided_gradcam.py` of the same toolkit: the
 * guided gradient times the class activation map):
 *     dx_nchw [n,3,H,W] fp32 = dx * (gate / 255)
 * with dx what mil_stem_dgrad writes for the same dstem / wpack / dtype, from the same accumulators, and gate [n,H,W] uint8 one
 * byte per pixel for its three channels (mil_grad_cam's map).  float(gate) / 255.f is one correctly rounded division and the
 * product one multiplication, never fused: bit for bit the fp32 `dx * (gate / 255)` of IEEE arithmetic.  No ungated tensor, no
 * atomics, no workspace: bit-repeatable.  There is no `reduce` form.  Null dstem / wpack / gate / dx_nchw, n < 0, H or W < 1,
 * another dtype: MIL_ERR_ARG; n == 0: MIL_OK, no launch; one image's dstem of 2 GiB or more: MIL_ERR_UNSUPPORTED — all decided
 * on the host before any GPU call. */
int mil_stem_dgrad_gated(const void* dstem, const void* wpack, const uint8_t* gate, float* dx_nchw, int n, int H, int W,
                         int dtype, void* stream);

/* A point of a straight path from a baseline colour to the tiles, optionally with Gaussian noise — the input of one step of
 * integrated gradients (`integrated_gradients.py`) or SmoothGrad (`smooth_grad.py`) of the same toolkit:
 *     out[t,c,y,x] = base[c] + alpha * (v - base[c]) + sigma * n(seed, sample, i)          out [n,3,H,W] fp32
 * tiles [n,3,H,W]: fp32 (is_u8 == 0; v the value) or uint8 (is_u8 == 1; v the decoded value of mil_u8_decode_table, so the result
 * is bit for bit that of the decoded fp32 tensor).  The differences, products and sums are single correctly rounded fp32 operations,
 * none fused.  sigma = noise_level * (range[1] - range[0]) with range a DEVICE float[2], or noise_level itself when range is NULL;
 * noise_level == 0: no generator runs and the third term is absent.  n(seed, sample, i), i the linear element index: Philox4x32-10
 * (multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85) with key (seed low, seed high) and counter
 * (i >> 2 low, i >> 2 high, sample, 0) gives r0..r3; u1 = ((r0 >> 8) + 1) 2^-24, u2 = (r1 >> 8) 2^-24, elements 4 (i >> 2) and + 1
 * get sqrt(-2 ln u1) cospi(2 u2) and sqrt(-2 ln u1) sinpi(2 u2), elements + 2 and + 3 the same of (r2, r3): a value depends on
 * (seed, sample, i) only.  Null tiles / out, is_u8 outside {0,1}, n < 0, H or W < 1, noise_level < 0 or NaN, alpha NaN: MIL_ERR_ARG;
 * n == 0: MIL_OK, no launch; H W of 2^31 or more: MIL_ERR_UNSUPPORTED — all decided on the host before any GPU call. */
int mil_path_point(const void* tiles, int is_u8, float* out, float base0, float base1, float base2, float alpha, float noise_level,
                   const float* range, unsigned long long seed, unsigned sample, int n, int H, int W, void* stream);

/* From an accumulated mean gradient acc [n,3,H,W] fp32 to what is shown; any subset of the three outputs (NULL: not made):
 *     attr [n,3,H,W]  = (v - base[c]) * acc                   one difference and one product per element, not fused
 *     map [n,H,W]       map_mode 0: |(a0 + a1) + a2|, a_c = attr of channel c        1: max_c |a_c|
 *                       map_mode 2: max_c |acc_c| — reads no tiles (tiles may be NULL when it is the only output)
 *     tile_sum [n]    = the sum of attr over the tile, in a fixed order: each of MIL_ATTR_SLICES workgroups per tile sums its pixels
 *                       ((a0 + a1) + a2 per pixel) into ws [n * MIL_ATTR_SLICES] fp32, a second small launch adds a tile's partial
 *                       sums in slice order.  No atomics: two calls give the same bits.  (This summation tree — a thread's items
 *                       in order, the butterfly over the wave's 64 lanes, the four waves in order, the slices in order — is the
 *                       one csrc/slice_sum.cuh implements for mil_attr_finish, mil_stage_seed, mil_stage_energy, mil_stage_match
 *                       and mil_pixel_reg; tests/slice_sum_reference.py restates it and the GPU tests hold it bit for bit.)
 * tiles as for mil_path_point.  Null acc, no output, tiles NULL where they are read, tile_sum without ws, is_u8 outside {0,1},
 * map_mode outside {0,1,2}, n < 0, H or W < 1: MIL_ERR_ARG; n == 0: MIL_OK, no launch; 3 H W of 2^31 or more:
 * MIL_ERR_UNSUPPORTED — all decided on the host before any GPU call. */
#define MIL_ATTR_SLICES 32
int mil_attr_finish(const float* acc, const void* tiles, int is_u8, float base0, float base1, float base2, float* attr, float* map,
                    int map_mode, float* tile_sum, float* ws, int n, int H, int W, void* stream);

/* Activation maximisation (`cnn_layer_visualization.py`, `deep_dream.py`, `generate_class_specific_samples.py` of the same toolkit):
 * the objective "one channel of a stage's output, averaged over the map" and the seed of its backward pass.
 *     act [n,h,w,cp]  a stage's output as the forward keeps it (behind the block's LeakyReLU), MIL_DT_BF16 or MIL_DT_F32, c real channels
 *     channels [n]    DEVICE int32, one channel per tile, 0 <= channels[t] < c (a value outside selects nothing: J = 0, dz = 0; no
 *                     address is formed from it)
 *     objective [n]   J_t = (sum over y,x of act[t,y,x,channels[t]]) / (h w), fp32
 *     dz [n,h,w,cp]   the gradient of the LOSS -J_t with respect to the PRE-activation map, the form the backward chain carries:
 *                     dz[t,y,x,k] = (-(1 / (h w))) * (act > 0 ? 1 : slope) for k == channels[t], 0 for every other k (padding included);
 *                     1 / (h w) is one fp32 division on the host, the product one fp32 multiplication, rounded to bf16 where dz is bf16
 * Every element of dz and objective is written; neither is read.  The sum has a fixed order: each of MIL_SEED_SLICES workgroups per
 * tile sums its pixels into ws [n * MIL_SEED_SLICES] fp32, a second small launch adds a tile's partial sums in slice order and divides
 * by h w (one correctly rounded division).  No atomics: two calls give the same bits.  Null pointers, n < 0, h or w < 1, cp not a
 * positive multiple of 8, c outside [1, cp], another dtype: MIL_ERR_ARG; n == 0: MIL_OK, no launch; h w of 2^24 or more or one map
 * of 2^31 elements or more: MIL_ERR_UNSUPPORTED — all decided on the host before any GPU call. */
#define MIL_SEED_SLICES 16
int mil_stage_seed(const void* act, const int* channels, float* objective, void* dz, float* ws, int n, int h, int w, int cp, int c,
                   float slope, int dtype, void* stream);

/* One optimiser step on an image stack, in place, in one pass: x, g, m, v fp32 with `total` elements each.  With g' = g + wd * x:
 *     rule 0 (torch.optim.SGD, no momentum):   x <- x - lr * g'                                  (m, v not read, may be NULL)
 *     rule 1 (torch.optim.Adam, coupled decay): m <- beta1 * m + one_minus_beta1 * g'
 *                                               v <- beta2 * v + (one_minus_beta2 * g') * g'
 *                                               x <- x - ((lr / bc1) * m) / (sqrt(v) / sqrt_bc2 + eps)
 * with bc1 = 1 - beta1^step, sqrt_bc2 = sqrt(1 - beta2^step), one_minus_beta = 1 - beta formed by the caller in double and passed as
 * fp32.  Then the projection of the new x:  project 0: none;  1: clamp to [-1, 1];  2: x <- table[encode(x)], the round trip through
 * bytes, table a DEVICE float[256] (the values of mil_u8_decode_table).  u8_out (NULL: not made) [total] = encode(x) of the value
 * stored, encode(x) = rint(clip(x / 2 + 0.5, 0, 1) * 255), half to even (np.round).  Every product, quotient, sum and difference
 * is a single correctly rounded fp32 operation in the order written, none fused: the same expressions in numpy fp32 give the same
 * bits.  16-byte accesses where every pointer is on its 16-byte (u8_out: 4-byte) grid, element by element otherwise and in a last
 * short group.  Null x / g, rule or project outside their range, rule 1 without m and v or with bc1 or sqrt_bc2 <= 0 or eps < 0,
 * project 2 without table, lr or wd NaN: MIL_ERR_ARG; total == 0: MIL_OK, no launch; more than 2^31 - 1 workgroups of 1024 elements:
 * MIL_ERR_UNSUPPORTED — all decided on the host before any GPU call. */
int mil_pixel_step(float* x, const float* g, float* m, float* v, unsigned char* u8_out, const float* table, size_t total, int rule,
                   int project, float lr, float weight_decay, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2,
                   float bc1, float sqrt_bc2, float eps, void* stream);

/* Feature inversion (`inverted_representation.py` of the same toolkit): the seed of "make this stage's output equal that one".
 *     act, target [n,h,w,cp]  two outputs of one stage as the forward keeps them, MIL_DT_BF16 or MIL_DT_F32, c real channels
 *     energy [n]      E_t = sum over y,x and the c real channels of target^2, fp32: mil_stage_energy writes it, mil_stage_match reads it
 *     loss [n]        weight * (D_t / E_t), D_t = sum over y,x and the real channels of (act - target)^2 — the toolkit's
 *                     1e-1 * euclidian_loss; one quotient, one product
 *     dz [n,h,w,cp]   the gradient of loss_t with respect to the PRE-activation map, the form the backward chain carries, for k < c:
 *                     dz[t,y,x,k] = (((2 * weight) / E_t) * (act - target)) * (act > 0 ? 1 : slope)
 *                     2 * weight is exact, the quotient is one fp32 division per tile, then one difference and two products in the order
 *                     written, rounded to bf16 where dz is bf16; dz is exactly 0 in the padding channels c .. cp - 1
 * Every square is one product of the fp32 value with itself.  Every element of energy / loss / dz is written.  The sums have a fixed
 * order: each of MIL_SEED_SLICES workgroups per tile sums its pixels (per thread in work-item order and, within an 8-channel group,
 * in channel order; a shuffle butterfly; the four waves in order) into ws [n * MIL_SEED_SLICES] fp32, a second small launch adds a
 * tile's partial sums in slice order.  No atomics: two calls give the same bits.  E_t == 0 is not looked for: scale and loss are what
 * IEEE division gives (inf or NaN), as in the toolkit, which divides by zero there too.  16-byte accesses where act, target and dz
 * are on the 16-byte grid, element by element otherwise.  Null pointers, n < 0, h or w < 1, cp not a positive multiple of 8,
 * c outside [1, cp], another dtype: MIL_ERR_ARG; n == 0: MIL_OK, no launch; h w of 2^24 or more or one map of 2^31 elements or
 * more: MIL_ERR_UNSUPPORTED — all decided on the host before any GPU call. */
int mil_stage_energy(const void* target, float* energy, float* ws, int n, int h, int w, int cp, int c, int dtype, void* stream);
int mil_stage_match(const void* act, const void* target, const float* energy, float* loss, void* dz, float* ws, int n, int h, int w, int cp,
                    int c, float weight, float slope, int dtype, void* stream);

/* The pixel regularisers of the same file and the way back through a jitter: x, g, out fp32 [n,3,H,W]; x is only read.
 *     out[t,c,i,j] = g[t,c,(i + dy) mod H,(j + dx) mod W] + ca * x^(alpha - 1) + ct * S[i,j]
 * with ca = alpha_weight * alpha (one fp32 product on the host), ct = 2 * tv_weight (exact) and, for v = x[t,c,i,j]:
 *     x^(alpha - 1)  p = v, then alpha - 2 times p = p * v — the gradient of the toolkit's alpha_norm sum x^alpha
 *     S[i,j]         half the gradient of total_variation_norm with beta = 2, sum over c, i < H - 1, j < W - 1 of
 *                    (x[i,j] - x[i+1,j])^2 + (x[i,j] - x[i,j+1])^2.  S = 0, then in this order, each where the trimmed slices hold it:
 *                      i < H - 1 and j < W - 1 (the cell's own term):   S = S + ((v - x[i+1,j]) + (v - x[i,j+1]))
 *                      i >= 1    and j < W - 1 (the term of the cell above):       S = S + (v - x[i-1,j])
 *                      j >= 1    and i < H - 1 (the term of the cell to the left): S = S + (v - x[i,j-1])
 *                    the last row and the last column own no term; H == 1 or W == 1: S = 0 everywhere
 *     out = g';  out = out + ca * p (only when alpha_weight != 0);  out = out + ct * S (only when tv_weight != 0)
 * A weight of exactly 0 skips its sum: with both 0, out is the shifted g bit for bit.  alpha: an even integer in 2..8.  Any integer
 * dy, dx: reduced mod H, W here.  out may BE g when the reduced shift is (0, 0); any other overlap of out with g or x is refused.
 * terms (NULL: not made) [2,n] fp32: terms[0,t] = sum of p * v (x^alpha), terms[1,t] = the total variation, per cell
 * (d1 * d1) + (d2 * d2) of the two differences above — whatever the weights are.  Their sums have a fixed order: each of
 * MIL_REG_SLICES workgroups per tile sums its share of the tile's 3 H W elements (groups of four consecutive elements; per thread in
 * group order, a shuffle butterfly, the four waves in order) into ws [2 * n * MIL_REG_SLICES] fp32, a second small launch adds the
 * partial sums in slice order.  No atomics.  The neighbours are read from global memory (no LDS tile).  A whole group is one
 * 16-byte access per tensor, on whatever 4-byte boundary it starts; where it lies in one row the rows above and below are one
 * 16-byte load each (for g: where its sources do not wrap), element by element otherwise and in a last short group.
 * Null x / g / out, terms without ws, alpha odd or outside 2..8, a NaN weight, the overlaps above, n < 0, H or W < 1: MIL_ERR_ARG;
 * n == 0: MIL_OK, no launch; a tile of 2^31 - 4 elements or more: MIL_ERR_UNSUPPORTED — all decided on the host before any GPU call. */
#define MIL_REG_SLICES 16
int mil_pixel_reg(const float* x, const float* g, float* out, float* terms, float* ws, int n, int H, int W, int alpha, float alpha_weight,
                  float tv_weight, int dy, int dx, void* stream);

/* The jittered copy out[t,c,i,j] = x[t,c,(i - dy) mod H,(j - dx) mod W]: a bit copy, the inverse of mil_pixel_reg's index map (the
 * gradient of a function of `out` with respect to x is that gradient read at (i + dy, j + dx)).  Any integer dy, dx.  Null pointers,
 * out overlapping x, n < 0, H or W < 1: MIL_ERR_ARG; n == 0: MIL_OK; sizes as for mil_pixel_reg. */
int mil_pixel_shift(const float* x, float* out, int n, int H, int W, int dy, int dx, void* stream);

/* A separable symmetric filter over a stack of planes, both passes in one launch — the Gaussian blur of the pixel optimisers (of the
 * image, of the gradient) and of attribution maps.  x, out: fp32 [planes,H,W], contiguous; planes any count >= 0 (a stack [T,3,H,W] is
 * 3 T planes, a map [T,H,W] is T).  taps: a DEVICE float[radius + 1] = w[0..radius], the centre tap and one half of the filter; the
 * arithmetic is defined for any taps, the Gaussian is the host's choice of them.  With v[d] the sample d places from the output's
 * own along the axis of a pass:
 *     acc = w[0] * v[0];   for k = 1 .. radius, in this order:   acc = acc + w[k] * (v[-k] + v[+k])
 * — the sum of the pair, then the product, then the accumulation, each a single correctly rounded fp32 operation, none fused.  The
 * horizontal pass (along W) runs first and its results are rounded to fp32; the vertical pass (along H) runs over those rounded
 * values.  The same expressions on numpy fp32 arrays give the same bits.  A sample outside the line of length n (W, then H) is the
 * sample at the source index the edge rule gives, per axis:
 *     edge 0  reflect    -i for i < 0, 2 (n - 1) - i for i > n - 1: the edge sample is not repeated (torch's `reflect` padding,
 *                        scipy's "mirror"); needs radius <= n - 1 on both axes
 *     edge 1  replicate  i clamped to [0, n - 1] (scipy's "nearest"); any radius
 *     edge 2  wrap       i mod n (scipy's "wrap", the cyclic jitter's rule); any radius, radius >= n too
 * One workgroup per 64 x 64 output tile of a plane: the tile and its halo staged in LDS through the index map, the horizontal pass
 * into a second LDS array, one barrier, the vertical pass to global memory; no atomics; 16-byte global accesses where four
 * consecutive elements of a row lie inside the plane on the 16-byte grid, element by element otherwise.
 * Null x / out / taps, out overlapping x (the filter is never in place), planes < 0, H or W < 1, radius outside
 * 1..MIL_BLUR_MAX_RADIUS, edge outside {0,1,2}, edge 0 with radius > min(H, W) - 1: MIL_ERR_ARG; planes == 0: MIL_OK, no launch; a plane
 * beyond what mil_pixel_shift takes as a third of a tile (3 H W >= 2^31 - 4), or more than 2^31 - 1 workgroups: MIL_ERR_UNSUPPORTED —
 * all decided on the host before any GPU call. */
#define MIL_BLUR_MAX_RADIUS 16
int mil_pixel_blur(const float* x, float* out, const float* taps, int planes, int H, int W, int radius, int edge, void* stream);

/* Pillow's `ImageFilter.GaussianBlur` on a stack of uint8 planes, bit for bit — the defocus augmentation of the train chain on planar
 * tile stacks [T,3,H,W] (planes = 3 T, planes_per_item = 3) and the smoothing of uint8 maps [T,H,W] (planes_per_item = 1).  Pillow's
 * Gaussian blur is three passes of an extended box blur along the rows, then three along the columns, in 32-bit integer fixed point,
 * rounded to a byte after every pass.  in, out: uint8 [planes,H,W], contiguous, any H, W >= 1; never in place.  params: a DEVICE
 * int32 [planes / planes_per_item, 6] = (r_x, ww_x, fw_x, r_y, ww_y, fw_y) per item; plane p takes row p / planes_per_item.  One pass
 * along a line of length n, with c(i) = min(max(i, 0), n - 1) and all arithmetic in uint32:
 *     out[x] = (ww * sum_{k=-r..r} in[c(x+k)] + fw * (in[c(x-r-1)] + in[c(x+r+1)]) + (1 << 23)) >> 24
 * Three such passes run along W with the x parameters, then three along H with the y parameters; each pass reads the bytes the pass
 * before wrote and clamps at the border of the PLANE.  The weights sum to at most 2^24, so nothing wraps; there is no floating point
 * on the device and any summation order gives the same bits.  (r, ww, fw) = (0, 2^24, 0) is the identity on that axis (what Pillow
 * does for a radius of 0: it skips the axis).  The host derives the integers from a sigma per axis in fp32, as Pillow's C does:
 *     radius = f32(sigma);  sigma2 = f32(radius * radius / f32(3))
 *     L = f32(sqrt(12.0 * double(sigma2) + 1.0));  l = f32(floor((double(L) - 1.0) / 2.0))
 *     a = f32((2 l + 1) * (l (l + 1) - 3 sigma2));  a = f32(a / f32(6 * (sigma2 - (l + 1) (l + 1))))
 *     fr = f32(l + a);  r = int(fr);  ww = int(f32(16777216) / f32(fr * 2 + 1))   (an fp32 division, truncated)
 *     fw = ((1 << 24) - (2 r + 1) * ww) / 2
 * r <= MIL_BLUR_U8_MAX_BOX on either axis, which admits every sigma <= 8.0; the halo of a 64 x 64 output block is then at most
 * 3 (r + 1) = 24 pixels per side.  One workgroup per block: the block and this item's halo staged in LDS as bytes, six passes between
 * two LDS byte arrays, the last written to global memory.
 * WHO CHECKS WHAT.  This entry decides on the host, before any GPU call: null in / out / params, in and out overlapping in any byte,
 * planes < 0, planes_per_item < 1, planes % planes_per_item != 0, H or W < 1: MIL_ERR_ARG; planes == 0: MIL_OK, no launch; a plane
 * of more than 2^31 - 4097 bytes or more than 2^31 - 1 workgroups: MIL_ERR_UNSUPPORTED.  It does NOT read `params`, which lies in
 * device memory: the caller (ops.gaussian_blur_u8 checks its host copy) guarantees 0 <= r <= MIL_BLUR_U8_MAX_BOX, ww >= 0, fw >= 0
 * and (2 r + 1) ww + 2 fw <= 2^24 per axis.  The kernel forces r into 0..MIL_BLUR_U8_MAX_BOX, so no parameter can make it leave its
 * arrays; weights outside the contract give bytes the contract does not define. */
#define MIL_BLUR_U8_MAX_BOX 7
int mil_gaussian_blur_u8(const uint8_t* in, uint8_t* out, const int32_t* params, int planes, int planes_per_item, int H, int W, void* stream);

/* torch.optim.SGD with momentum (no dampening, no Nesterov) on an image stack, in place, in one pass — mil_pixel_step's kernel with a
 * third rule, behind an entry of its own (mil_pixel_step keeps refusing rule 2):
 *     g' = g + wd * x;   buf <- momentum * buf + g';   x <- x - lr * buf
 * each operation rounded once in the order written.  With buf all +0 the step is torch's first one, which sets buf = g': buf ends
 * as g' and x as mil_pixel_step's rule 0 leaves it, bit for bit (momentum * 0 + g' is exact).  project, table,
 * u8_out, the accesses and the size limit: mil_pixel_step's.  Null x / g / buf, project outside {0,1,2}, project 2 without table,
 * lr, wd or momentum NaN: MIL_ERR_ARG; total == 0: MIL_OK, no launch. */
int mil_pixel_momentum_step(float* x, const float* g, float* buf, unsigned char* u8_out, const float* table, size_t total, int project,
                            float lr, float weight_decay, float momentum, void* stream);

/* Order statistics of attribution maps: what `convert_to_grayscale` of the same toolkit's misc_functions.py takes with np.min and
 * np.percentile(., 99).  x [n,channels,H,W] fp32: channels == 3 ranks gray = (|g0| + |g1|) + |g2| (fp32, numpy's axis-0 order),
 * channels == 1 ranks the map itself.  A group is one tile (bag == 0; n groups of H W values) or the whole bag (bag == 1; one group
 * of n H W values).  With N the values of a group, vi = (N - 1) * (q / 100) in fp64 (numpy's linear method), lo = floor(vi),
 * hi = min(lo + 1, N - 1), t = vi - lo and s the group's values in ascending order:
 *     stats[g] = (min, max, s[lo], s[hi])     fp32, bit for bit
 *     p[g]     = s[lo] + (s[hi] - s[lo]) * t when t < 0.5, s[hi] - (s[hi] - s[lo]) * (1 - t) otherwise; fp64, each operation rounded
 *                on its own — bit for bit np.percentile(values.astype(np.float64), q)
 * An exact radix select over the order-preserving 32-bit key of a value, in three digit passes (11, 11, 10 bits) of a histogram
 * launch and a select launch each; q == 100 needs the first histogram only.  Values order by IEEE value; -0.0 counts as (and is
 * returned as) +0.0; a NaN orders by its bits, above +inf or, with the sign bit set, below -inf.  Counts are integers merged with
 * integer atomics: two calls give the same bits.  workspace: mil_map_quantile_workspace(n, bag) bytes — MIL_QUANTILE_WS_WORDS
 * 32-bit words per tile, or for a bag MIL_QUANTILE_BAG_TABLES copies of them (tile t adds to copy t % 16, so that not every
 * workgroup adds to the same words; the select launch sums the copies); the call clears it itself.  Null x / workspace / stats / p, n < 1, H or W < 1,
 * channels outside {1,3}, bag outside {0,1}, q outside (0, 100] or NaN, a workspace too small: MIL_ERR_ARG; a tile of more
 * than 2^30 values or a group of 2^31 or more: MIL_ERR_UNSUPPORTED — all decided on the host before any GPU call. */
#define MIL_QUANTILE_WS_WORDS 4104
#define MIL_QUANTILE_BAG_TABLES 16
int mil_map_quantile_workspace(size_t* bytes, int n, int bag);
int mil_map_quantile(const float* x, int n, int channels, int H, int W, double q, int bag, void* workspace, size_t workspace_bytes,
                     float* stats, double* p, void* stream);

/* Attribution tensors to the toolkit's bytes, from x and the statistics of mil_map_quantile (group of tile t: bag ? 0 : t):
 *     mode 0  grayscale (convert_to_grayscale + format_np_output): x [n,channels,H,W], channels 3 (gray as above) or 1 (the map);
 *             out0 [n,H,W] = trunc(255 * clip((double(gray) - double(min)) / (p - double(min)), 0, 1)), fp64; p == min: zeros
 *     mode 1  colour (save_gradient_images): x [n,3,H,W]; out0 [n,H,W,3] = trunc(((g - min) / (max - min)) * 255) in fp32, each
 *             operation rounded; max == min: zeros.  The statistics are those of the gradient as a map (channels 1, 3 H rows)
 *     mode 2  positive / negative (get_positive_negative_saliency + save_gradient_images): out0 [n,H,W,3] =
 *             trunc((max(0, g) / max) * 255), out1 [n,H,W,3] = trunc((max(0, -g) / (-min)) * 255), fp32; max <= 0 / min >= 0: zeros
 * Pointwise, 16-byte loads and 4-byte stores where H W % 4 == 0 and the pointers allow, scalar accesses otherwise.  Null x / stats /
 * out0, mode 0 without p, mode 2 without out1, channels the mode does not take, mode outside {0,1,2}, bag outside {0,1}, n < 0,
 * H or W < 1: MIL_ERR_ARG; n == 0: MIL_OK, no launch; H W of 2^31 or more: MIL_ERR_UNSUPPORTED — decided on the host. */
int mil_attr_render(const float* x, int n, int channels, int H, int W, int mode, int bag, const float* stats, const double* p,
                    uint8_t* out0, uint8_t* out1, void* stream);

/* apply_colormap_on_image of the same file: heat [n,H,W,3] = lut[map] (lut [256,3] uint8, map [n,H,W] uint8) and on_image
 * [n,H,W,3] = Pillow's Image.alpha_composite of heat with alpha byte `alpha` over the opaque tile (tiles [n,3,H,W] uint8 planar):
 *     tmp = 64 * (src * alpha + dst * (255 - alpha)) + (0x80 << 6);   out = (((tmp >> 8) + tmp) >> 8) >> 6
 * per channel.  Either output may be NULL.  Null tiles / map / lut, both outputs null, alpha outside [0,255], n < 0, H or W < 1:
 * MIL_ERR_ARG; n == 0: MIL_OK, no launch; H W of 2^31 or more: MIL_ERR_UNSUPPORTED — decided on the host. */
int mil_cam_overlay(const uint8_t* tiles, const uint8_t* map, const uint8_t* lut, int alpha, int n, int H, int W, uint8_t* heat,
                    uint8_t* on_image, void* stream);

/* Slide mosaic of per-tile attribution maps: the uint8 maps or pictures of the T kept windows resampled into the blocks of
 * thumbnail pixels the windows own, coloured and composited over the tissue.  maps: channels == 1, uint8 [T,Hm,Wm] (what
 * mil_attr_render's mode 0 or mil_grad_cam write), coloured through lut, uint8 [256,3]; channels == 3, uint8 [T,Hm,Wm,3]
 * interleaved (modes 1 and 2, mil_cam_overlay's heat), used as the colour itself (lut may be NULL).  Window t owns the n x n block
 * of output pixels whose top-left one is (out_pos[t][0], out_pos[t][1]) (row, col; DEVICE int32 [T,2]) — mil_heatmap_render's
 * convention with n = S / D; the part of a block outside [Ht,Wt] is not stored, blocks of two windows must not overlap (the
 * caller's to ensure), pixels no window owns are not touched.  heat and on_tissue: uint8 [Ht,Wt,3], either may be NULL;
 * on_tissue is read and written in place (the caller has put the tissue thumbnail there), every output pixel by the one thread
 * that owns it.  All integer.  For owned pixel (a,b), 0 <= a,b < n, and channel c:
 *     wy[k] = max(0, min((a+1)*Hm, (k+1)*n) - max(a*Hm, k*n))      k = 0..Hm-1   (sums to Hm)
 *     wx[l] = max(0, min((b+1)*Wm, (l+1)*n) - max(b*Wm, l*n))      l = 0..Wm-1   (sums to Wm)
 *     v[c]  = (sum_k sum_l wy[k]*wx[l]*maps[t,k,l,c] + Hm*Wm/2) / (Hm*Wm)
 * the area (box) average of the map over the pixel's footprint, rounded half up: the k x k box mean with mil_heatmap_render's
 * rounding for Hm = k*n, the identity for Hm == n, pixel replication for n = k*Hm, fractional coverage otherwise.  Then
 *     src[c]    = lut[v][c] (channels == 1) or v[c] (channels == 3);      heat = src
 *     on_tissue = Pillow's alpha_composite as mil_cam_overlay states it, over the byte dst already there:
 *                 tmp = 64 * (src * a + dst * (255 - a)) + (0x80 << 6);   out = (((tmp >> 8) + tmp) >> 8) >> 6
 *                 a = alpha, or with alpha_by_value (channels == 1 only) a = (alpha * v + 127) / 255
 * The sums are 32-bit: 255*Hm*Wm + Hm*Wm/2 < 2^32 for Hm*Wm <= 2^24, above that MIL_ERR_UNSUPPORTED.  Two forms of one kernel
 * give the same bytes: a thread per owned pixel, or — where ceil(Hm/n) * ceil(Wm/n) >= 64 — a wave per owned pixel with a
 * shuffle reduction.  Null maps / out_pos, both outputs null, lut null with channels == 1, channels outside {1,3}, alpha outside
 * [0,255], alpha_by_value outside {0,1} or set with channels == 3, T < 0, Hm, Wm, n, Ht or Wt < 1: MIL_ERR_ARG; T == 0: MIL_OK,
 * no launch — all decided on the host before any GPU call.  Any T (launches of 65535 windows), any n.  No atomics on global
 * memory, no workspace: bit-repeatable. */
int mil_attr_mosaic(const uint8_t* maps, int channels, int T, int Hm, int Wm, int n, const int32_t* out_pos, const uint8_t* lut,
                    int alpha, int alpha_by_value, uint8_t* heat, uint8_t* on_tissue, int Ht, int Wt, void* stream);

/* Grad-CAM per tile: the post-processing of `gradcam.py:75-89` of the same toolkit (pytorch-cnn-visualizations-master/src), from
 * the output of a convolutional stage and the gradient of the class evidence with respect to it to the bytes the toolkit draws
 * over the tile.  act, grad [n,h,w,cs] (bf16 under MIL_DT_BF16, fp32 under MIL_DT_F32 / MIL_DT_F32S; c real channels of cs
 * stored, cs a multiple of 8; channels c..cs-1 are never used, whatever they hold).  Per tile t:
 *     w_k        = (sum over the pixels of grad[t,.,.,k]) / (h w)
 *     raw[t,i,j] = max(offset + sum_k w_k act[t,i,j,k], 0)        fp32 accumulation; offset = 1.0 is the toolkit's np.ones
 * raw (nullable) [n,h,w] fp32 receives it.  With out (nullable) [n,H,W] uint8 the call goes on:
 *     (mn, mx)   = the tile's own minimum and maximum of raw — or range[0], range[1] (range: a DEVICE float[2], nullable; raw is
 *                  clamped into it for the quantisation, the stored raw is not); range[0] <= range[1]
 *     q          = (uint8)(((raw - mn) / (mx - mn)) * 255.0f), IEEE fp32 with the correctly rounded division, truncated toward
 *                  zero as np.uint8 truncates; a constant tile (mx == mn), where the toolkit divides by zero, is all zeros
 *     out[t]     = q [h,w] resized to [H,W] by Pillow's two 8-bit passes (horizontal to uint8, then vertical to uint8; each from
 *                  1 << 21, int32 accumulation, arithmetic shift by 22, clamp to [0,255]; a pass whose sizes are equal is skipped)
 * with ybounds/ykk and xbounds/xkk the DEVICE copies of mil_resample_coeffs(h, H, MIL_FILTER_LANCZOS) and (w, W, ...), yksize /
 * xksize what mil_resample_plan returns for them.  out is bit for bit what numpy and Pillow make of the same fp32 raw.
 * One workgroup per tile, everything between the two tensors and the bytes in LDS; no atomics, no workspace: bit-repeatable.
 * Null act / grad, both outputs null, out without its four tables, n < 0, h, w, H or W < 1, c < 1, c > cs, cs % 8 != 0, a ksize
 * that is not mil_resample_plan's, another dtype: MIL_ERR_ARG; n == 0: MIL_OK, no launch; a tile whose maps, strip and tables
 * exceed the 160 KB of LDS (the largest supported: 128x128 -> 512x512), more than 256 16-byte pieces per pixel, one tile's tensor
 * of 2 GiB or more, act / grad off the 16-byte grid: MIL_ERR_UNSUPPORTED — all decided on the host before any GPU call. */
int mil_grad_cam(const void* act, const void* grad, int n, int h, int w, int c, int cs, int dtype, float offset,
                 const float* range, const int32_t* ybounds, const int32_t* ykk, int yksize, const int32_t* xbounds,
                 const int32_t* xkk, int xksize, float* raw, uint8_t* out, int H, int W, void* stream);

/* AdaptiveAvgPool2d((1,1)) + flatten + Linear(80,L,bias=False) (gbm/model.py:31-32,58-60).
 * x [n,hw,cp] -> pooled [n,c] fp32 (kept for backward), feats [n,nf] fp32 = pooled @ wfc^T (+ bias when given:
 * alt_resnet.py:93's Linear(512,num_classes) has one).  c, nf, cp <= 512.
 * Backward: dz [n,hw,cp] = lrelu'(act) * (dfeats @ wfc)/hw, dwfc [nf,c] = dfeats^T @ pooled, dbias [nf] (nullable). */
int mil_avgpool_fc_fwd(const void* x, const float* wfc, const float* bias, float* pooled, float* feats, int n, int hw,
                       int cp, int c, int nf, int dtype, void* stream);
int mil_avgpool_fc_bwd(const float* dfeats, const float* wfc, const float* pooled, const void* act, void* dz,
                       float* dwfc, float* dbias, int n, int hw, int cp, int c, int nf, int accumulate, float slope,
                       int dtype, void* stream);
/* The data half of mil_avgpool_fc_bwd (dwfc = NULL) under guided backpropagation (see mil_conv_dgrad_rule), for the last
 * block's LeakyReLU:  dz = (act > 0 && g > 0) ? g : +0,  g = (dfeats @ wfc)/hw — what the plain call writes with act = NULL.
 * No parameter gradient.  MIL_DT_BF16 / MIL_DT_F32.  Null pointer (act included), n < 0, hw < 1, c or nf outside [1, 512],
 * cp > 512, cp < c, cp % 8 != 0, another dtype: MIL_ERR_ARG; n == 0: MIL_OK, no launch. */
int mil_avgpool_fc_bwd_data_guided(const float* dfeats, const float* wfc, const void* act, void* dz, int n, int hw, int cp,
                                   int c, int nf, int dtype, void* stream);
/* The parameter gradients of the same layer on their own (two-stage, coalesced): dwfc [nf][c] (+)= dfeats^T pooled,
 * dbias [nf] (+)= column sums of dfeats (may be null).  mil_avgpool_fc_bwd skips them when its dwfc is null.
 * Workspace from mil_fc_wgrad_workspace. */
int mil_fc_wgrad_workspace(size_t* bytes, int n, int c, int nf);
int mil_fc_wgrad(const float* dfeats, const float* pooled, float* dwfc, float* dbias, void* workspace,
                 size_t workspace_bytes, int n, int c, int nf, int accumulate, void* stream);


/* ---- attention-MIL head --------------------------------------------------------------------
 * Replaces everything after the backbone in Attention.forward (gbm/model.py:198-246): ContextLayer
 * (batch-statistics BatchNorm1d + LeakyReLU + Dropout, :108-111), attention MLP + softplus/mask/L1
 * normalisation (:209-214), diagnostics (:201,216-219), buffer MLP (:223), pooling (:227-229),
 * softmax / argmax / label-smoothed weighted CE (:233-242, nnBlocks.py:71-85,121-134), l2 (:246).
 * Segmented over `nbags` bags: instances of bag b are rows [bag_offsets[b], bag_offsets[b+1]) of
 * H [ntot,80]; inst_bag[n] is the bag of row n.  keep_mask [ntot,80] uint8 (1 = kept) enables
 * Dropout(drop_p) as in training; null = eval.  class_weights [3] or null.
 * `weights` = 11 device pointers: context.bn.weight, context.bn.bias, attention.lin1.weight,
 * attention.lin1.bias, attention.lin2.weight, attention.lin2.bias, buffer.lin1.weight,
 * buffer.lin1.bias, buffer.classifier.weight, buffer.classifier.bias, weight_mask.
 * Outputs: a1 [ntot,3] (Aterm^T), wrois (bag b's [3,N_b] block at 3*bag_offsets[b]), bterm [ntot],
 * kld [nbags], rec [nbags, mil_head_rec_floats()] =
 *   {Mterm[3], y_pred[3], loss, error, Aterm_mu, Aterm_var, D[3], dloss/dM[3], y_hat, l2(bag 0)}.
 * Backward: dH [ntot,80] and `grads` (mil_head_grad_floats() floats: the 11 tensors' gradients back
 * to back, summed over bags), given grad_loss [nbags] and optional grad_l2 [1]. */
int mil_head_workspace_floats(size_t* floats, int ntot, int nbags);
int mil_head_grad_floats(void);
int mil_head_rec_floats(void);
int mil_head_fwd(const float* H, const int* bag_offsets, const int* inst_bag, const int64_t* labels,
                 const uint8_t* keep_mask, const float* class_weights, const float* const* weights,
                 float* workspace, float* a1, float* wrois, float* bterm, float* kld, float* rec, int ntot,
                 int nbags, float slope, float drop_p, float smoothing, float bn_eps, void* stream);
int mil_head_bwd(const float* H, const int* bag_offsets, const int* inst_bag, const uint8_t* keep_mask,
                 const float* const* weights, float* workspace, const float* bterm, const float* rec,
                 const float* grad_loss, const float* grad_l2, float* dH, float* grads, int ntot, int nbags,
                 float slope, float drop_p, void* stream);

/* ---- wide (64..512-channel) layers: the alt_resnet.py configuration -----------------------------
 * Channel-blocked implicit GEMM (64-wide output blocks x 32-wide input chunks staged through LDS) for channel
 * counts that do not fit the resident-filter kernels above.  Replaces conv3x3 / conv1x1 of alt_resnet.py:24-33
 * (bias-free, ReLU = slope 0) forward, data-gradient (MIL_PACK_DGRAD packing + zero_insert for stride 2) and
 * weight-gradient.  cin % 32 == 0, cout % 64 == 0; same tensor layout and epilogue semantics as mil_conv_igemm.
 * dtype: MIL_DT_BF16, MIL_DT_F32 or MIL_DT_F32S.  Packed filter: [co_block][ci_chunk][tap][4][64 lanes] fragments of eight
 * consecutive input channels; a fragment is 8 bf16 (MIL_DT_BF16), 8 floats (MIL_DT_F32) or, under MIL_DT_F32S,
 * [hi: 8 bf16][lo: 8 bf16] with hi = bf16(v), lo = bf16(v - hi) — the 32 bytes of the MIL_DT_F32 fragment, so
 * mil_wide_packed_elems counts elements of float for both.  Under MIL_DT_F32S every tensor is fp32 as under MIL_DT_F32 (res
 * and act enter the epilogue as exact fp32); x / dz are split into hi and lo bf16 planes on their way into LDS and each
 * 32-deep k-step is three bf16 MFMAs.  mil_wide_wgrad is bit-repeatable in every mode (one slab per workgroup, fixed-order
 * reduction); its workspace under MIL_DT_F32S is that of MIL_DT_F32. */
int mil_wide_packed_elems(size_t* elems, int cout, int cin, int ks, int mode);
int mil_wide_pack_weights(const float* w, void* wpack, int cout, int cin, int ks, int mode, int dtype, void* stream);
int mil_wide_conv(const void* x, const void* wpack, const float* bias, const void* res, const void* act, void* y, int n_img,
                  int H, int W, int cin, int Ho, int Wo, int cout, int ks, int stride, int pad, int zero_insert,
                  int apply_relu, float slope, int dtype, void* stream);
int mil_wide_wgrad_workspace(size_t* bytes, int n_img, int H, int W, int cin, int Ho, int Wo, int cout, int ks, int stride,
                             int pad, int dtype);
int mil_wide_wgrad(const void* x, const void* dz, float* dw, void* workspace, size_t workspace_bytes, int n_img, int H, int W,
                   int cin, int Ho, int Wo, int cout, int ks, int stride, int pad, int accumulate, int dtype, void* stream);

/* ---- wide layers, gather-GEMM form (bf16): one deep-pipelined GEMM per 256-pixel x 128-channel tile whose K-steps
 * (one filter tap x 64 input channels) are copied to LDS by LDS-DMA, the next two in flight across the single barrier per
 * K-step.  Same role as mil_wide_conv (conv3x3 / conv1x1 of alt_resnet.py:24-33 forward and data gradient; ReLU = slope 0)
 * for channel counts with cin_x % 64 == 0 and cout_x % 128 == 0 (as executed: a data gradient contracts over the conv's
 * Cout and produces its Cin).  transposed == 0: y = conv(x); transposed == 1: x is dz on the conv's output grid, y is the
 * gradient on its input grid — a stride-2 gradient runs as four output-parity classes with only the taps that reach each.
 * mil_gconv_pack_weights: fp32 [Cout][Cin][k][k] -> swizzled 128-row x 64-channel filter images, mode 0 forward /
 * 1 data gradient. */
int mil_gconv_supported(int cin_x, int cout_x, int ks, int stride);
int mil_gconv_packed_elems(size_t* elems, int cout, int cin, int ks, int mode);
int mil_gconv_pack_weights(const float* w, void* wpack, int cout, int cin, int ks, int mode, void* stream);
int mil_gconv(const void* x, const void* wpack, const void* res, const void* act, void* y, int n_img, int H, int W, int cin_x,
              int Ho, int Wo, int cout_x, int ks, int stride, int pad, int transposed, int apply_relu, float slope, void* stream);

/* ---- training-step closure ---------------------------------------------------
 * mil_adam_step: torch.optim.Adam (gbm/classify_combined.py:519, stepped at :450-454) over the flat fp32
 * parameter / gradient buckets in ONE launch; `step` is the 1-based step count (bias correction),
 * `grad_scale` multiplies the gradient first (1/accumulated-bags, or 1).
 * mil_pack_all: re-pack every conv filter into MFMA fragment order in ONE launch from a device-resident
 * table of mil_pack_job_bytes()-sized records filled on the host by mil_pack_job_fill (same index maps as
 * mil_pack_conv_weights). */
int mil_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);
int mil_pack_job_bytes(void);
int mil_pack_job_fill(void* job_host, const float* w, const float* bias, void* out, float* bias_pad, int cout, int cin,
                      int ks, int mode, int dtype);
int mil_pack_all(const void* jobs_device, int njobs, void* stream);

/* ---- per-tensor summaries (gbm/classify_combined.py:418 prime_activation_summary, :484-485 weight mean / max) -------
 * Statistics of a whole TABLE of tensors read where they lie, in TWO launches (per-chunk partial records, then one
 * finishing workgroup per tensor): no copy, no host synchronisation, no atomics, bit-repeatable.
 * A job is `n_pix` records of `c_pad` elements (MIL_DT_F32 or MIL_DT_BF16) of which the first `c_real` count: a
 * channel-padded NHWC activation, or with c_real = c_pad = 1 a flat run such as one parameter inside the flat bucket.
 * `x` needs the alignment of its element only.  out[job][8] (fp64): [0] finite elements, [1] their sum, [2] their sum
 * of squares, [3] min and [4] max over them (+inf / -inf when there is none), [5] finite elements < 0 (-0.0 is not),
 * [6] NaN / +-inf elements, [7] n_pix * c_real.  Pad channels are never read into a statistic.  Elements are widened
 * exactly and added in fp64 in an order that depends on the job's (n_pix, c_pad, dtype) alone.
 * The table is mil_stats_job_bytes()-sized records filled on the host by mil_stats_job_fill; the caller hands the host
 * table and a device copy of it.  mil_tensor_stats_workspace: bytes of `ws` for a table; the call writes every word of
 * `out` and reads no word of `ws` it has not written itself.  njobs == 0: MIL_OK, nothing launched.  Argument errors
 * (null pointer, c_real < 1, c_real > c_pad, n_pix < 0, njobs < 0, short ws: MIL_ERR_ARG; another dtype:
 * MIL_ERR_UNSUPPORTED) are decided on the host before any GPU call. */
int mil_stats_job_bytes(void);
int mil_stats_job_fill(void* job_host, const void* x, long long n_pix, int c_real, int c_pad, int dtype);
int mil_tensor_stats_workspace(size_t* bytes, const void* jobs_host, int njobs);
int mil_tensor_stats_all(const void* jobs_device, const void* jobs_host, int njobs, double* out, void* ws,
                         size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIL_HIP_H */
