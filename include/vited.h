/*
 * vited.h - C ABI of libvited_hip.so: the MI355X (gfx950) kernels behind the ViT encoder-decoder
 * hot path of glmanhtu/vit-ed.
 *
 * The reference has no FFI of its own (it is pure Python on PyTorch/timm); its boundary for this
 * path is the module contract of models/vision_transformer.py:13-420.  Each entry point below
 * replaces the ATen/cuDNN/SDPA call that the cited reference line dispatches implicitly, so a
 * maintainer binds them with ctypes from the Attention/Block/CrossBlock
 * forward methods.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes only; no C++ types, no exceptions, no torch types.
 *  - every pointer is a DEVICE pointer owned by the caller (inputs, outputs, saved tensors and
 *    workspace); kernels never allocate, free, or retain pointers past the call.
 *  - `stream` is a hipStream_t passed as void*; every launch goes to it; no entry synchronises,
 *    so all of them are hipGraph-capturable.
 *  - return value: 0 (VITED_OK) or a VITED_ERR_* code; vited_strerror() names it.
 *  - dtype arguments select the activation type (VITED_F32 or VITED_BF16); parameters, the
 *    residual stream, statistics, gradients of parameters and all accumulation are fp32.
 *  - strides (ld*, *_bs, *_ts) are in ELEMENTS of the tensor they describe.
 */
#ifndef VITED_H
#define VITED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VITED_ABI_VERSION 1

#define VITED_OK 0
#define VITED_ERR_BAD_ARG 1     /* null pointer, non-positive size, misaligned pointer/stride */
#define VITED_ERR_UNSUPPORTED 2 /* shape/dtype combination no kernel covers */
#define VITED_ERR_LAUNCH 3      /* hipGetLastError() after the launch */
#define VITED_ERR_WORKSPACE 4   /* workspace smaller than vited_*_workspace_bytes() */

#define VITED_F32 0
#define VITED_BF16 1
#define VITED_F16 2 /* the ranking entries (vited_retrieval_*, vited_group_retrieval_metrics) and vited_pair_scores_add only */
#define VITED_I32 3 /* integer index dtypes (vited_pair_scores_add) */
#define VITED_I64 4

/* GEMM epilogues (vited_gemm) */
#define VITED_EPI_STORE 0          /* out = T(acc + bias)                                          */
#define VITED_EPI_GELU 1           /* out = T(z), out2 = T(gelu_erf(z)), z = acc + bias            */
#define VITED_EPI_RESIDUAL 2       /* out_f32[orow] = residual[rrow] + acc + bias (row remap below) */
#define VITED_EPI_MUL_GELU_GRAD 3  /* out = T(acc * gelu_erf'(aux)), aux = saved pre-activation    */
#define VITED_EPI_STORE_F32 4      /* out_f32 = acc + bias (logits of the head stay fp32)           */
#define VITED_EPI_MUL 5            /* out = T((acc + bias) * aux), aux = a saved factor (gelu'(z))   */
#define VITED_EPI_GELU_GRAD 6      /* out = T(gelu_erf'(z)), out2 = T(gelu_erf(z)), z = acc + bias:
                                      what fc1 saves for backward (timm Mlp: the backward of GELU then is
                                      one multiply, VITED_EPI_MUL, instead of an erf/exp per element)  */

/* B-operand layouts (vited_gemm) */
#define VITED_B_NK 0 /* B is [N, K] row-major: out = A . B^T  (nn.Linear weight)                   */
#define VITED_B_KN 1 /* B is [K, N] row-major: out = A . B                                         */

int vited_abi_version(void);
const char* vited_strerror(int code);

/* Which implementation the last vited_gemm / vited_attention_* call on this thread dispatched to:
 * 0 = none yet, 1 = portable fp32-FMA kernel, 2 = bf16 MFMA kernel, 3 = persistent bf16 MFMA GEMM
 * (opt-in, VITED_NT=as).  Test/diagnostic use. */
int vited_last_gemm_path(void);
int vited_last_attention_path(void);

/* GEMM path 1 (the fp32 compute mode, and the bf16 shapes the bf16 MFMA kernels do not tile) has two kernels that produce the
 * same bits: the vector-ALU kernel and, for the shapes vited_gemm_f32_mfma_supported names, one on the f32-input matrix-core
 * instruction (v_mfma_f32_32x32x2_f32), whose result is the same k-ordered fmaf chain.
 *   vited_gemm_f32_mfma_supported  1 when vited_gemm of that shape (b_layout VITED_B_*, epilogue VITED_EPI_*) takes the matrix-core
 *                                  kernel under automatic selection, else 0.  Host-only: needs no GPU.
 *   vited_last_fp32_gemm_kernel    which one the last path-1 call of vited_gemm / vited_gemm_scaled / vited_linear_bwd_weight on
 *                                  this thread ran: 0 = none yet, 1 = vector-ALU kernel, 2 = matrix-core kernel.
 *   vited_fp32_gemm_select         mode 0 = automatic (the default), 1 = vector-ALU kernels only.  Process-wide; returns the
 *                                  previous mode, or VITED_ERR_BAD_ARG for any other mode (nothing changes).  Test/diagnostic use:
 *                                  it lets one process run both kernels on the same data. */
int vited_gemm_f32_mfma_supported(int64_t M, int64_t N, int64_t K, int b_layout, int epilogue);
int vited_last_fp32_gemm_kernel(void);
int vited_fp32_gemm_select(int mode);

/* Attention path 1 (the fp32 compute mode, and the bf16 operands the bf16 MFMA attention refuses) has two sets of kernels that
 * produce the same bits as well: the vector-ALU kernels and, for the calls vited_attention_f32_mfma_supported names, kernels on
 * v_mfma_f32_32x32x2_f32 that walk the same fmaf chains (forward, dQ + delta, dK / dV).
 *   vited_attention_f32_mfma_supported  1 when vited_attention_fwd* (backward = 0) or vited_attention_bwd* (backward = 1) of that
 *                                       dtype (VITED_F32 / VITED_BF16) and shape takes the matrix-core kernels under automatic
 *                                       selection once it is on path 1, else 0.  Host-only: needs no GPU.
 *   vited_last_fp32_attention_kernel    which set the last path-1 attention call on this thread ran: 0 = none yet, 1 = vector-ALU
 *                                       kernels, 2 = matrix-core kernels.
 *   vited_fp32_attention_select         mode 0 = automatic (the default), 1 = vector-ALU kernels only.  Process-wide and separate
 *                                       from vited_fp32_gemm_select; returns the previous mode, or VITED_ERR_BAD_ARG for any other
 *                                       mode (nothing changes).  Test/diagnostic use. */
int vited_attention_f32_mfma_supported(int dtype, int64_t batch, int heads, int64_t nq, int64_t nk, int head_dim, int backward);
int vited_last_fp32_attention_kernel(void);
int vited_fp32_attention_select(int mode);

/* ---- data movement -------------------------------------------------------------------------- */

/* dst[i] = (dst_dtype) src[i].  Used for the bf16 shadow of the fp32 master parameters. */
int vited_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);

/* dst[c, r] = (dst_dtype) src[r, c]; src is fp32 [rows, cols].  Transposed bf16 weight shadow used
 * by the input-gradient GEMMs. */
int vited_cast_transpose(const float* src, void* dst, int dst_dtype, int64_t rows, int64_t cols, void* stream);

/* Refresh every bf16 weight shadow of a model in ONE launch (after an optimizer step; replaces one
 * vited_cast + one vited_cast_transpose per weight).  desc is a DEVICE array of count x 6 int64:
 *   {src fp32 [rows, cols] address, dst bf16 [rows, cols] address or 0, dst_t bf16 [cols, rows] address or 0,
 *    rows, cols, first_tile}
 * where first_tile is the running sum of ceil(rows/64) * ceil(cols/64) over the preceding entries and
 * total_tiles the sum over all of them.  The reference has no counterpart: under autocast PyTorch
 * re-casts each weight inside every F.linear call (vision_transformer.py:49-80 via misc/engine.py:208). */
int vited_cast_weights(const int64_t* desc, int count, int64_t total_tiles, void* stream);

/* Patch extraction for timm PatchEmbed's Conv2d(k = s = p) (used at vision_transformer.py:383,391):
 * out[(b * G*G + py*G + px), (c*p + i)*p + j] = img[idx(b), c, py*p + i, px*p + j]
 * img is fp32 with batch stride img_bs (so x[:, 0] / x[:, 1] of the stacked pair tensor need no
 * copy, vision_transformer.py:408); batch_index (nullable int64[B]) gathers images by index
 * (hisfrag.py:153,226-227) without materialising the gathered copy. */
int vited_patchify(const float* img, int64_t img_bs, const int64_t* batch_index, void* out, int out_dtype,
                   int64_t batch, int chans, int img_size, int patch, void* stream);

/* The same from uint8 pixels, with the input pipeline's ToTensor + Normalize(mean, std) (data/transforms.py:14-18, applied per
 * sample on the host by the reference's loader, data/datasets/div2k_patch.py:108-162) folded in:
 * value = (pixel / 255 - mean[c]) / std[c].  mean / std are HOST arrays of `chans` (<= 4) floats.  A batch then crosses PCIe and
 * HBM at 1 byte per pixel (misc/engine.py:203-204 copies fp32). */
int vited_patchify_u8(const uint8_t* img, int64_t img_bs, const int64_t* batch_index, void* out, int out_dtype,
                      int64_t batch, int chans, int img_size, int patch, const float* mean, const float* std, void* stream);

/* Patch-pair assembly on the device (data/datasets/div2k_patch.py:108-121,155-162; transforms.py:14-18): per sample a uint8
 * region [chans, 2 S, 3 S] (the 3-column x 2-row grid of S x S cells the reference cuts with transforms.crop(patch, 3, 2)),
 * the two cells of its pair (cells int32 [batch, 2], 0..5 row-major) and the erosion size e = ceil(S (1 - erosion_ratio))
 * (erode int32 [batch], e <= S).  out uint8 [batch, 2, chans, S, S] = Resize(S)(CenterCrop(e)(cell)) with Pillow's 8-bit
 * bilinear resample, bit for bit; ToTensor + Normalize then happen inside vited_patchify_u8.  cells / erode are DEVICE arrays. */
int vited_crop_pairs_u8(const uint8_t* src, int64_t src_bs, const int* cells, const int* erode, uint8_t* out, int64_t batch,
                        int chans, int img_size, void* stream);

/* The stage in front of vited_crop_pairs_u8 (data/datasets/div2k_patch.py:84-111: RandomHorizontalFlip, RandomVerticalFlip,
 * A.ShiftScaleRotate, A.RGBShift, RandomCrop / CenterCrop) from images that stay on the device.  store holds n_images decoded
 * images back to back, uint8 HWC with 3 channels: image i starts at byte img_off[i] and is img_hw[2 i] rows of img_hw[2 i + 1]
 * pixels.  Sample b takes image[b] (clamped to [0, n_images)) and writes out[b] = uint8 [3, 2 S, 3 S] (S = img_size), the window
 * of the augmented image whose top-left corner is crop[b] = (top, left), clamped to [0, H - 2 S] x [0, W - 3 S]:
 *   flags[b]  bit 0 horizontal flip, bit 1 vertical flip, bit 2 warp, bit 3 colour shift
 *   minv[b]   6 doubles, the inverse (destination -> source) affine map, row-major; read when bit 2 is set
 *   rgb[b]    3 floats added per channel, then clamped to [0, 255] and floored (fp32); read when bit 3 is set
 * The warp is cv2.warpAffine's linear scheme: 1/32-pixel positions from fp64 terms rounded half-even at 10 fractional bits,
 * four taps with 15-bit integer weights, BORDER_REFLECT_101; the flips act on the tap fetch.  DESIGN.md section 16 defines
 * every step.  All arrays are DEVICE memory; an image smaller than 2 S x 3 S is the caller's error (the window is then reflected).
 * VITED_ERR_BAD_ARG: a null pointer, n_images <= 0, batch outside 1..65535, img_size outside 1..4096. */
int vited_div2k_regions_u8(const uint8_t* store, const int64_t* img_off, const int* img_hw, int n_images, const int* image,
                           const int* flags, const double* minv, const float* rgb, const int* crop, uint8_t* out, int64_t batch,
                           int img_size, void* stream);

/* Config H's input pipeline (hisfrag.py:63-81) from images that stay on the device, in three steps; DESIGN.md section 17 defines
 * every one.  All arrays are DEVICE memory; flags[b] carries one bit per augmentation for all three entry points:
 *   bit 0 RandomAffine, bit 1 A.ShiftScaleRotate, bit 2 ColorJitter, bit 3 GaussianBlur.
 * VITED_ERR_BAD_ARG everywhere: a null pointer, batch outside 1..65535, img_size outside 2..4096.
 *
 * vited_hisfrag_windows_u8: store / img_off / img_hw / image as for vited_div2k_regions_u8.  out[b] = uint8 [3, S, S], the window of
 * the augmented image whose top-left corner is origin[b] = (top, left) in unpadded image coordinates; they may be negative or
 * past the image (RandomCrop's pad_if_needed), everything outside the image is 0.
 *   afix[b]  6 int64, Pillow's 16.16 coefficients of the RandomAffine output -> input matrix (nearest); read when bit 0 is set
 *   minv[b]  6 doubles, the inverse ShiftScaleRotate map; read when bit 1 is set.  cv2's linear scheme as in
 *            vited_div2k_regions_u8, with BORDER_CONSTANT 0: a tap outside the image is 0.
 * Also VITED_ERR_BAD_ARG: n_images <= 0. */
int vited_hisfrag_windows_u8(const uint8_t* store, const int64_t* img_off, const int* img_hw, int n_images, const int* image,
                             const int* flags, const int64_t* afix, const double* minv, const int* origin, uint8_t* out, int64_t batch,
                             int img_size, void* stream);

/* ColorJitter on uint8 [batch, 3, S, S], Pillow's arithmetic bit for bit (ImageEnhance.Brightness / Contrast / Color, the HSV
 * round trip for hue).  Samples without bit 2 are copied.
 *   order[b]    4 ints, the operations in the order they run: 0 brightness, 1 contrast, 2 saturation, 3 hue (others do nothing)
 *   factors[b]  3 floats: brightness, contrast, saturation
 *   hue[b]      the uint8 added to H (mod 256)
 *   sums        workspace of `batch` int64, 8-byte aligned: zeroed here, then the sum of L over each crop as it stands when
 *               contrast's turn comes (two kernels: the sums, then the pixels)
 * out may be in itself. */
int vited_hisfrag_jitter_u8(const uint8_t* in, const int* flags, const int* order, const float* factors, const int* hue, int64_t* sums,
                            uint8_t* out, int64_t batch, int img_size, void* stream);

/* GaussianBlur((3, 3)) on uint8 [batch, 3, S, S]: weights[b] = (k_edge, k_mid) of the 3-tap kernel, the 2-D weight their fp32
 * product; nine fp32 products added in row-major order, rounded half to even; the border reflects without repeating the edge.
 * Samples without bit 3 are copied.  Also VITED_ERR_BAD_ARG: out == in. */
int vited_hisfrag_blur_u8(const uint8_t* in, const int* flags, const float* weights, uint8_t* out, int64_t batch, int img_size,
                          void* stream);

/* michigan.py's input pipeline (michigan.py:68-101) from images that stay on the device: vited_michigan_windows_u8, then
 * vited_hisfrag_jitter_u8 (unchanged: it reads bit 2 only), then vited_michigan_blur_gray_u8; DESIGN.md section 18 defines every
 * step.  All arrays are DEVICE memory; flags[b] carries one bit per augmentation:
 *   bit 0 CoarseDropout, bit 1 horizontal flip, bit 2 ColorJitter, bit 3 GaussianBlur, bit 4 vertical flip, bit 5 grayscale.
 * VITED_ERR_BAD_ARG everywhere: a null pointer, batch outside 1..65535, img_size outside 2..4096.
 *
 * vited_michigan_windows_u8: store / img_off / img_hw / image as for vited_div2k_regions_u8.  out[b] = uint8 [3, S, S].  The window
 * Wd(u, v), 0 <= u, v < S, is the image at (v + top, u + left), origin[b] = (top, left) in unpadded image coordinates (they may be
 * negative or past the image: RandomCrop's pad_if_needed), and 255 outside the image; a tap outside the window reads 255 too.
 * The window is resampled with Pillow's two-pass 8-bit bilinear scheme (horizontal, then vertical, a uint8 intermediate) from tap
 * tables: per output column x the first tap x0[b][x] (window coordinates) and three 22-bit fixed-point weights kx[b][x][0..2]
 * (unused taps 0), likewise y0 / ky per output row:
 *   T(x, r) = clip8((2^21 + sum_i kx[x][i] Wd(x0[x] + i, r)) >> 22),  R(x, y) = clip8((2^21 + sum_j ky[y][j] T(x, y0[y] + j)) >> 22).
 * With bit 0 set, a pixel of R inside any of the first n_holes[b] (clamped to 0..16) rectangles holes[b][h] = (x1, y1, x2, y2),
 * half-open, becomes 255.  out(x, y) is the holed image at (bit 1 ? S - 1 - x : x, bit 4 ? S - 1 - y : y).
 * Also VITED_ERR_BAD_ARG: n_images <= 0. */
int vited_michigan_windows_u8(const uint8_t* store, const int64_t* img_off, const int* img_hw, int n_images, const int* image,
                              const int* flags, const int* origin, const int* x0, const int* kx, const int* y0, const int* ky,
                              const int* holes, const int* n_holes, uint8_t* out, int64_t batch, int img_size, void* stream);

/* ImageFilter.GaussianBlur(radius <= 1) and RandomGrayscale on uint8 [batch, 3, S, S].  With bit 3 set: Pillow's box blur of box
 * radius 0, three passes along x, then three along y, each
 *   out[x] = (in[x] ww + (in[max(x - 1, 0)] + in[min(x + 1, S - 1)]) fw + 2^23) >> 24     (unsigned 32-bit)
 * with weights[b] = (ww, fw) and a uint8 intermediate after every pass.  With bit 5 set, afterwards, all three channels become
 * L = (R 19595 + G 38470 + B 7471 + 32768) >> 16.  With neither the sample is copied.  Also VITED_ERR_BAD_ARG: out == in. */
int vited_michigan_blur_gray_u8(const uint8_t* in, const int* flags, const int* weights, uint8_t* out, int64_t batch, int img_size,
                                void* stream);

/* Pillow's Image.resize((Rw, Rh), BILINEAR) for 8-bit RGB at any scale, antialiased where it shrinks, from images that stay on the
 * device (csrc/resample_u8.hip, the rule in csrc/resample_u8.h): what transforms.Resize does in
 * TwoImgSyncEval.normalize (pajigsaw.py, evaluation.py) and in michigan.py's evaluation transform.  All arrays are DEVICE memory.
 *   store / img_off / img_hw / image   as for vited_div2k_regions_u8 (indices are clamped)
 *   windows   int32 [batch, 4] = (top, left, h, w) in image coordinates, or null: the whole image.  A window may reach outside the
 *             image (top, left may be negative); pixels outside it are `fill` (0..255) in all three channels
 *   xtab      int32 [ncx, Rw, 2 + ksx]: per class of window width and per output column (first tap in window coordinates, tap count,
 *             ksx 22-bit fixed-point weights, unused ones 0) - Pillow's precompute_coeffs + normalize_coeffs_8bpc for w -> Rw, computed
 *             in fp64 by the caller; xcls int32 [batch] names each sample's class (clamped).  ytab / ycls / ncy / ksy likewise for
 *             h -> Rh.  max_h, max_w: the largest window the tables were made for; they size the LDS band and bound the ratio
 *   T(x, r) = clip8((2^21 + sum_j kx[x][j] Wd(first_x[x] + j, r)) >> 22),  R(x, y) = clip8((2^21 + sum_j ky[y][j] T(x, first_y[y] + j)) >> 22)
 *   out       uint8: sample b's planes [3, S, S] at out + b * out_bs bytes, R at (x + crop_left, y + crop_top); every byte of them is
 *             written on every call, nothing else is
 * No allocation, copy or synchronisation.  A first tap or count outside its range is clamped or skipped, never followed.
 * VITED_ERR_BAD_ARG: a null pointer other than windows, a misaligned table, batch outside 1..65535, a non-positive size, fill outside
 * 0..255, a crop that leaves the resized image, out_bs < 3 S^2 with batch > 1 (samples would overlap), ksx / ksy below
 * 2 ceil(max(max_len / out_len, 1)) + 1.  VITED_ERR_UNSUPPORTED: Rh or Rw above 1024, max_h > 8 Rh or max_w > 8 Rw, ksx or ksy above 17. */
int vited_resample_u8(const uint8_t* store, const int64_t* img_off, const int* img_hw, int n_images, const int* image, const int* windows,
                      int fill, const int* xtab, const int* xcls, int ncx, int ksx, const int* ytab, const int* ycls, int ncy, int ksy,
                      int max_h, int max_w, int Rh, int Rw, int crop_top, int crop_left, int img_size, uint8_t* out, int64_t out_bs,
                      int64_t batch, void* stream);

/* out[b, r] = (out_dtype) in[b, row_offset + r] for r < rows: drops the cls row of a token-gradient
 * tensor before the patch-embed weight gradient. in is fp32 [batch, in_rows, dim]. */
int vited_slice_rows_cast(const float* in, void* out, int out_dtype, int64_t batch, int64_t in_rows,
                          int64_t row_offset, int64_t rows, int64_t dim, void* stream);

/* x[b, 0, :] = cls[:] + pos[0, :] : the cls row of timm _pos_embed (vision_transformer.py:392). */
int vited_write_cls_row(float* x, const float* cls, const float* pos, int64_t batch, int64_t rows_per_batch,
                        int64_t dim, void* stream);

/* ---- patch dropout (timm PatchDropout(prob, num_prefix_tokens=1, ordered=False) as the reference's model constructs it and calls
 * it at vision_transformer.py:385,393; csrc/patch_keep.hip) ----------------------------------------------------
 * A keep table is a DEVICE int32 [batch, K]: per sample the K token indices timm's argsort(randn)[:, :K] kept, counted behind the
 * prefix slot, in keep order (not sorted), distinct within a row.  `lead` says where the prefix slot falls:
 *   lead = 0 (prepare_x2): the prefix is the cls token; the kept patch rows are patch(b, r) = keep[b, r], r < K.
 *   lead = 1 (forward_first_part): no cls token exists, the slot falls on patch 0, which is always kept and leads:
 *            patch(b, 0) = 0, patch(b, r) = 1 + keep[b, r - 1]; R = 1 + K rows.
 * R = K + lead below.  An index outside its range is clamped by the kernels, never followed out of bounds.
 * VITED_ERR_BAD_ARG everywhere: a null pointer, a non-positive size, lead other than 0 / 1, K + lead above the number of patches,
 * a pointer that is not aligned to its element (16 bytes for the fp32 token rows of vited_tokens_kept / _bwd, whose dim is a
 * multiple of 4).
 *
 * keep[b, 0..K) = the indices of the K smallest of keys[b, 0..L), in ascending key order, equal keys by ascending index (NaN after
 * every number): torch.argsort(keys, dim=-1, stable=True)[:, :K].  One workgroup per row, the keys in LDS; L > 4096 is
 * VITED_ERR_UNSUPPORTED, K > L VITED_ERR_BAD_ARG.  No host read: capturable. */
int vited_keep_from_keys(const float* keys, int32_t* keep, int64_t batch, int L, int K, void* stream);

/* vited_patchify / vited_patchify_u8 for the kept patches alone: out[(b * R + r), :] = the patch row of patch(b, r), bit-equal to
 * the row the full kernels write for that patch; a dropped patch is never read.  keep is indexed by the OUTPUT sample b (with
 * batch_index: by the pair, not by the gathered image).  R above 65535 is VITED_ERR_UNSUPPORTED. */
int vited_patchify_kept(const float* img, int64_t img_bs, const int64_t* batch_index, const int32_t* keep, int K, int lead, void* out,
                        int out_dtype, int64_t batch, int chans, int img_size, int patch, void* stream);
int vited_patchify_kept_u8(const uint8_t* img, int64_t img_bs, const int64_t* batch_index, const int32_t* keep, int K, int lead,
                           void* out, int out_dtype, int64_t batch, int chans, int img_size, int patch, const float* mean,
                           const float* std, void* stream);

/* timm _pos_embed for kept tokens: tok fp32 [batch * R, dim] is the patch-embedding product + bias of the kept rows, pos fp32
 * [1 + n_patches, dim].  Without cls (null): x fp32 [batch, R, dim], x[b, r] = tok[b, r] + pos[1 + patch(b, r)].  With cls fp32
 * [dim]: x [batch, 1 + R, dim], x[b, 0] = cls + pos[0] and x[b, 1 + r] as before.  One fp32 add per element. */
int vited_tokens_kept(const float* tok, const float* pos, const float* cls, const int32_t* keep, int K, int lead, float* x,
                      int64_t batch, int n_patches, int dim, void* stream);

/* inv int32 [batch, n_patches]: inv[b, p] = r where patch(b, r) == p, -1 where sample b dropped patch p. */
int vited_keep_inverse(const int32_t* keep, int K, int lead, int32_t* inv, int64_t batch, int n_patches, void* stream);

/* Backward of vited_tokens_kept with respect to pos and cls: dx fp32 [batch, rows, dim] with rows = R + with_cls.
 * dpos[1 + p] = sum over the samples b with inv[b, p] >= 0, in ascending b, of dx[b, with_cls + inv[b, p]] - exact zeros for a patch
 * nobody kept; dpos[0] (and dcls fp32 [dim], nullable, with_cls only) = sum_b dx[b, 0] with a cls row, exact zeros without.  Every
 * element of dpos [1 + n_patches, dim] is written once, without atomics: bitwise reproducible. */
int vited_tokens_kept_bwd(const float* dx, const int32_t* inv, float* dpos, float* dcls, int64_t batch, int rows, int with_cls,
                          int n_patches, int dim, void* stream);

/* ---- elementwise token dropout (timm's pos_drop = nn.Dropout(pos_drop_rate) at the end of _pos_embed, vision_transformer.py:378-380;
 * csrc/token_dropout.hip, the rule in csrc/token_dropout.h) ------------------------------------------------------
 * out[b, r, d] = keep ? x[b, r, d] * scale : 0 over a stream [batch, rows, dim] of `dtype` (VITED_F32 / VITED_BF16), x and out each with
 * a batch and a row stride (elements); out may be x itself with x's strides (in place), otherwise the two lie apart.  The mask comes
 * from a counter-based generator and is never stored: element e = (b * tokens + t) * dim + d (int64; t = the ORIGINAL token of row
 * r) reads word e & 3 of Philox4x32-10 with the counter (lo32(e >> 2), hi32(e >> 2), stream_id, 0) and the key (lo32, hi32) of
 * *seed, and is kept iff word >= thr.  The backward is the same call on the gradient with the same seed.
 *   tokens     the stream's full token count T; without a keep table rows == tokens and t = r
 *   keep       optional DEVICE int32 [batch, K] patch-dropout table with K + 1 == rows: row 0 is the prefix token 0 and row r the
 *              token of the patch vited_tokens_kept put there (lead = 1: 1 + keep[b, r - 1] of a stream without a cls token; lead = 0:
 *              the patch keep[b, r - 1] behind the cls token, token keep[b, r - 1] + 1); indices are clamped, never followed outside
 *   stream_id  0 (image-1 stream) or 1 (image-2 stream): two streams of one seed get unrelated masks
 *   seed       DEVICE pointer to one int64, read by the kernel: a captured graph sees the value written for each replay
 *   thr        min(2^32 - 1, int(p * 2^32)) in [0, 2^32 - 1];  scale = float(1 / (1 - p))
 * A kept element is one fp32 multiply rounded once to `dtype`; a dropped one is 0 by selection (also for inf / NaN inputs).  Every
 * output element is written; no allocation, copy or synchronisation.
 * VITED_ERR_BAD_ARG: a null x / out / seed, a non-positive size, dim % 4 != 0, a row stride below dim or a batch stride below a
 * sample's span (rows or samples would overlap), x and out overlapping without being the same layout, a stride that is no multiple
 * of 4 or a pointer not aligned to four elements (seed: 8 bytes, keep: 4), thr outside [0, 2^32 - 1], stream_id or lead outside
 * {0, 1}, K + 1 != rows or rows > tokens with a table, rows != tokens without.  VITED_ERR_UNSUPPORTED: another dtype, dim > 1024. */
int vited_token_dropout(const void* x, int64_t x_bs, int64_t x_rs, void* out, int64_t out_bs, int64_t out_rs, int dtype, int64_t batch,
                        int rows, int dim, int tokens, int stream_id, const int32_t* keep, int K, int lead, const int64_t* seed,
                        int64_t thr, float scale, void* stream);

/* out[r] = sum_b in[b, r] (fp32 out; in is `in_dtype` [batch, width]).  Deterministic two-pass;
 * workspace >= vited_sum_rows_workspace_bytes().  Serves bias gradients (column sums) and the
 * pos_embed / cls_token gradients (batch sums). */
int64_t vited_sum_rows_workspace_bytes(int64_t batch, int64_t width);
int vited_sum_rows(const void* in, int in_dtype, int64_t in_ld, float* out, int64_t batch, int64_t width,
                   float* workspace, int64_t workspace_bytes, void* stream);

/* ---- LayerNorm (nn.LayerNorm(eps=1e-6), vision_transformer.py:101,114,231,244,245,258,348,400) */

/* y[r, :] = (x[r, :] - mean) * rstd * gamma + beta ; saves mean/rstd (fp32 [rows]). */
int vited_layernorm_fwd(const float* x, int64_t x_ld, const float* gamma, const float* beta, void* y,
                        int y_dtype, int64_t y_ld, float* mean, float* rstd, int64_t rows, int64_t dim,
                        float eps, void* stream);

/* dx_out = (dx_in ? dx_in : 0) + LN'(dy); optional low-precision copy of dx_out (dx_lp, may be
 * null); dgamma/dbeta receive the column sums: overwritten, or added onto their current content when
 * `accumulate` != 0 (accumulation straight into a parameter's .grad).  workspace >= *_workspace_bytes. */
int64_t vited_layernorm_bwd_workspace_bytes(int64_t rows, int64_t dim);
int vited_layernorm_bwd(const void* dy, int dy_dtype, int64_t dy_ld, const float* x, int64_t x_ld,
                        const float* gamma, const float* mean, const float* rstd, const float* dx_in,
                        int64_t dx_in_ld, float* dx_out, int64_t dx_out_ld, void* dx_lp, int dx_lp_dtype,
                        int64_t dx_lp_ld, float* dgamma, float* dbeta, int accumulate, int64_t rows, int64_t dim,
                        float* workspace, int64_t workspace_bytes, void* stream);

/* vited_layernorm_bwd whose low-precision copy ALONE is scaled per row: dx_lp[r, :] = T(lp_scale[r] * dx_out[r, :]), dx_out
 * unscaled.  Under stochastic depth the copy is what the next branch's backward consumes (its d(input) GEMM, weight and bias
 * gradients), and that branch sees s[b] * dy while the residual path carries dy.  dx_lp is required and may be VITED_BF16 or
 * VITED_F32 (the exact path, where the copy otherwise is dx_out itself).  lp_scale == null is vited_layernorm_bwd. */
int vited_layernorm_bwd_scaled(const void* dy, int dy_dtype, int64_t dy_ld, const float* x, int64_t x_ld,
                               const float* gamma, const float* mean, const float* rstd, const float* dx_in,
                               int64_t dx_in_ld, float* dx_out, int64_t dx_out_ld, void* dx_lp, int dx_lp_dtype,
                               int64_t dx_lp_ld, const float* lp_scale, float* dgamma, float* dbeta, int accumulate,
                               int64_t rows, int64_t dim, float* workspace, int64_t workspace_bytes, void* stream);

/* dst[r, :] = (dst_dtype)(row_scale[r] * src[r, :]), src fp32 [rows, dim]: the scaled copy of the incoming stream gradient at the
 * head of a backward pass (the last branch of the encoder / decoder consumes it).  dim and the row strides multiples of 4. */
int vited_scale_rows_cast(const float* src, int64_t src_ld, const float* row_scale, void* dst, int dst_dtype, int64_t dst_ld,
                          int64_t rows, int64_t dim, void* stream);

/* ---- q/k-norm (qk_norm=True: q_norm / k_norm = LayerNorm(head_dim, eps=1e-6), vision_transformer.py:35-36,60,153-154,180) ---- */

/* For every token row and head: out[r, h, :] = (x[r, h, :] - mean) * rstd * gamma + beta over the head_dim elements, biased
 * variance of the centred values, statistics in fp32.  q and k are the two operands of ONE launch; either may be null (then its
 * other arguments are ignored), not both.  Each is `dtype` (VITED_F32 / VITED_BF16) [rows, heads * head_dim] with its own row
 * stride and a dense last dim - a column slice of the packed [M, 3D] / [M, 2D] projection or a dense [M, D] - and its own row
 * count; the output has the same shape and its own row stride (it may be the input itself: in place).  gamma / beta fp32
 * [head_dim], shared by all heads; mean / rstd fp32 [rows, heads] dense, saved for the backward.  head_dim 32 or 64 (else
 * VITED_ERR_UNSUPPORTED); a null pointer of a present operand, a row stride below heads * head_dim (rows would overlap) or a
 * pointer / stride that is no multiple of a lane's vector (head_dim / 8 elements, 16 bytes at most) is VITED_ERR_BAD_ARG. */
int vited_qk_norm_fwd(const void* q, int64_t q_ld, int64_t q_rows, const void* k, int64_t k_ld, int64_t k_rows,
                      const float* gamma_q, const float* beta_q, const float* gamma_k, const float* beta_k, void* q_out,
                      int64_t q_out_ld, void* k_out, int64_t k_out_ld, float* q_mean, float* q_rstd, float* k_mean,
                      float* k_rstd, int dtype, int64_t heads, int64_t head_dim, float eps, void* stream);

/* Backward of vited_qk_norm_fwd.  dq / dk hold d(out) on entry (where the attention backward wrote it, inside the d(qkv) / d(q) /
 * d(kv) buffers) and d(x) on return: dx = rstd * (g - mean_d(g) - xhat * mean_d(g * xhat)), g = dy * gamma, xhat recomputed from
 * the saved pre-norm q / k and mean / rstd.  dgamma += / = sum dy * xhat, dbeta += / = sum dy over all rows and heads (fp32
 * [head_dim]; `accumulate` != 0 adds onto their content), from per-workgroup partial rows in `workspace` summed in a fixed order:
 * no atomics, two runs give the same bits.  Either operand may be null.  workspace >= *_workspace_bytes. */
int64_t vited_qk_norm_bwd_workspace_bytes(int64_t q_rows, int64_t k_rows, int64_t heads, int64_t head_dim);
int vited_qk_norm_bwd(void* dq, int64_t dq_ld, const void* q, int64_t q_ld, const float* q_mean, const float* q_rstd,
                      const float* gamma_q, float* dgamma_q, float* dbeta_q, int64_t q_rows, void* dk, int64_t dk_ld,
                      const void* k, int64_t k_ld, const float* k_mean, const float* k_rstd, const float* gamma_k,
                      float* dgamma_k, float* dbeta_k, int64_t k_rows, int dtype, int accumulate, int64_t heads,
                      int64_t head_dim, float* workspace, int64_t workspace_bytes, void* stream);

/* ---- pooled head (timm global_pool='avg': forward_head's x[:, 1:].mean(dim=1); csrc/pool_head.hip) ---- */

/* x fp32 [items, tokens, dim] through an item stride and a token stride (in elements; dense last dim), `first` prefix tokens that
 * take no part (1: the cls row).  Without gamma: pooled[b, :] = (sum over t >= first of x[b, t, :]) / (tokens - first).  With gamma
 * and beta (fp32 [dim]): the same mean over LayerNorm(x[b, t, :]; gamma, beta, eps) - the normalised rows are never written - and,
 * when mean / rstd (fp32 [items * tokens], both or neither) are given, the statistics of row t >= first of item b at [b * tokens +
 * t] for the backward (the prefix rows' entries are left alone).  pooled fp32 [items, dim] with row stride pooled_ld.  fp32
 * accumulation in ONE order fixed by the shape: the tokens of an item are cut into chunks of 64 (a workgroup each), a chunk's rows
 * are added by 8 row owners whose sums are added in ascending order, the chunks' sums - through `workspace` - in ascending order;
 * no atomics, two runs give the same bits.  dim a multiple of 4 up to 1024 (else VITED_ERR_UNSUPPORTED); a null operand, tokens <=
 * first, a stride that lets rows or items overlap, a pointer that is not 16-byte aligned or a stride that is no multiple of 4 is
 * VITED_ERR_BAD_ARG.  workspace >= vited_token_pool_workspace_bytes() (one query serves both entries), 16-byte aligned; the forward
 * needs none while an item is one chunk. */
int64_t vited_token_pool_workspace_bytes(int64_t items, int64_t tokens, int64_t first, int64_t dim);
int vited_token_pool_fwd(const float* x, int64_t x_is, int64_t x_ts, const float* gamma, const float* beta, float eps,
                         float* pooled, int64_t pooled_ld, float* mean, float* rstd, int64_t items, int64_t tokens,
                         int64_t first, int64_t dim, float* workspace, int64_t workspace_bytes, void* stream);

/* Backward of vited_token_pool_fwd given g fp32 [items, dim] (row stride g_ld), the gradient at pooled.  Writes EVERY element of dx
 * fp32 [items, tokens, dim] (item / token strides) exactly once - the caller clears nothing: rows t < first get zero, the others
 * dy = g[b, :] / (tokens - first), or with gamma the LayerNorm backward of that row gradient, rstd * (dy gamma - mean_c(dy gamma) -
 * xhat * mean_c(dy gamma xhat)) with xhat recomputed from x and the saved mean / rstd.  Without gamma x, mean and rstd are not read
 * and may be null.  dx_lp (optional; VITED_BF16 or VITED_F32, strides of its own) receives the copy T(lp_scale[b] * dx[b, t, :]) in
 * the same pass; lp_scale (optional, fp32 [items], needs dx_lp) means what vited_layernorm_bwd_scaled means by it, one value per
 * item, and dx stays unscaled.  With gamma, dgamma += / = sum dy * xhat and dbeta += / = sum dy over the pooled rows of all items
 * (fp32 [dim]; `accumulate` != 0 adds onto their content) from per-workgroup partial rows in `workspace` added in a fixed order
 * (vited_layernorm_bwd's finishing pass).  Errors as in the forward; a bf16 dx_lp needs 8-byte alignment. */
int vited_token_pool_bwd(const float* g, int64_t g_ld, const float* x, int64_t x_is, int64_t x_ts, const float* gamma,
                         const float* mean, const float* rstd, float* dx, int64_t dx_is, int64_t dx_ts, void* dx_lp,
                         int dx_lp_dtype, int64_t dx_lp_is, int64_t dx_lp_ts, const float* lp_scale, float* dgamma,
                         float* dbeta, int accumulate, int64_t items, int64_t tokens, int64_t first, int64_t dim,
                         float* workspace, int64_t workspace_bytes, void* stream);

/* ---- Linear / GEMM (nn.Linear: qkv :34, proj :38, q :151, kv :152, timm Mlp fc1/fc2, head) ---- */

/* acc[m, n] = sum_k A[m, k] * B(n, k), fp32 accumulation; A is `dtype` [M, K] (row stride lda);
 * B is `dtype`, laid out per b_layout (row stride ldb); then the epilogue (VITED_EPI_*):
 *   bias      fp32 [N] or null
 *   aux       `dtype` [M, N] (row stride ldo)        - MUL_GELU_GRAD and MUL
 *   residual  fp32                                     - RESIDUAL only
 *   out/out2  `dtype` [M, N] (row stride ldo); for RESIDUAL and STORE_F32 `out` is fp32
 * RESIDUAL row remap (patch-embed writes tokens behind a cls row and adds a broadcast pos_embed):
 *   orow = (m / rows_per_batch) * out_rows_per_batch + m % rows_per_batch + row_offset
 *   rrow = residual_bcast ? (m % rows_per_batch + row_offset) : orow
 * with rows_per_batch == 0 meaning the identity map (orow = rrow = m). */
int vited_gemm(const void* A, int64_t lda, const void* B, int64_t ldb, int b_layout, int dtype, int64_t M,
               int64_t N, int64_t K, int epilogue, const float* bias, const void* aux,
               const float* residual, void* out, void* out2, int64_t ldo, int64_t rows_per_batch,
               int64_t out_rows_per_batch, int64_t row_offset, int residual_bcast, void* stream);

/* VITED_EPI_RESIDUAL under stochastic depth (timm DropPath, scale_by_keep; the residual adds of Block.forward / CrossBlock.forward,
 * vision_transformer.py:125-126, 269-271):  out[m, n] = residual[m, n] + row_scale[m] * (acc[m, n] + bias[n]),
 * row_scale fp32 [M] with the sample's 0 or 1 / keep repeated over its rows (read once per row, beside the residual row).
 * Identity row map; out and residual fp32 with row stride ldo.  row_scale == null is vited_gemm(VITED_EPI_RESIDUAL) itself: the
 * same kernel instance, so a model without stochastic depth runs the code it ran before. */
int vited_gemm_scaled(const void* A, int64_t lda, const void* B, int64_t ldb, int b_layout, int dtype, int64_t M, int64_t N,
                      int64_t K, const float* bias, const float* residual, const float* row_scale, float* out, int64_t ldo,
                      void* stream);

/* Several 384-column NT products of ONE bf16 A [M, 384] (row stride lda) in one launch, the weights held in registers
 * (csrc/gemm_nt_wreg.hip):  out_g = bf16(A . W[g * 384 : (g + 1) * 384, 0 : 384]^T + bias[g * 384 : (g + 1) * 384]),  g < groups,
 * W bf16 [groups * 384, 384] (row stride ldw), bias fp32 [groups * 384] or null.  Group g is written as an [M, 384] block with row
 * stride ldo at  out + (g / groups_inner) * group_stride + (g % groups_inner) * 384  (elements): groups = 1 is VITED_EPI_STORE of
 * vited_gemm at N = K = 384; groups = 2 L, groups_inner = 2, ldo = 768, group_stride = M * 768 writes the keys / values of L
 * decoder blocks as L dense [M, 768] tensors.  Every element is bit-identical to vited_gemm's on the same operands.
 * `workgroups`: 0 = one per CU; a small positive count makes long per-workgroup shares out of few rows (tests).  The launch has
 * max(1, workgroups / groups) * groups workgroups.  Errors: VITED_ERR_UNSUPPORTED where vited_gemm_nt_wreg_supported (host-only,
 * 1 / 0) refuses the strides, M or the group counts; VITED_ERR_BAD_ARG for null or misaligned (16 bytes) pointers.  Reports GEMM
 * path 2.
 *   vited_gemm_nt_wreg_select  mode 0 = automatic (the default): vited_gemm itself hands the shapes its dispatch names to this
 *                              kernel; 1 = vited_gemm never does.  Process-wide; returns the previous mode, or VITED_ERR_BAD_ARG
 *                              for any other mode.  Test/diagnostic use: one process can run both kernels on the same data. */
int vited_gemm_nt_wreg_supported(int64_t lda, int64_t ldw, int64_t ldo, int64_t M, int groups, int groups_inner, int64_t group_stride);
int vited_gemm_nt_wreg(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* out, int64_t ldo, int64_t M,
                       int groups, int groups_inner, int64_t group_stride, int workgroups, void* stream);
int vited_gemm_nt_wreg_select(int mode);

/* dW[n, k] = sum_m dY[m, n] * X[m, k] (fp32 [N, K]) and, if dbias != null, dbias[n] = sum_m dY[m, n];
 * overwritten, or added onto their current content when `accumulate` != 0.  dY / X are `dtype`.
 * workspace >= *_workspace_bytes. */
int64_t vited_linear_bwd_weight_workspace_bytes(int64_t M, int64_t N, int64_t K);
int vited_linear_bwd_weight(const void* dY, int64_t lddy, const void* X, int64_t ldx, int dtype, int64_t M,
                            int64_t N, int64_t K, float* dW, float* dbias, int accumulate, float* workspace,
                            int64_t workspace_bytes, void* stream);

/* Several weight gradients in ONE launch: the dW / dbias of every Linear of one transformer block (Block / CrossBlock backward,
 * vision_transformer.py:124-127, 268-272), queued by the caller and flushed together.  Arrays have `count` (<= 40) entries, all
 * host memory; entry i is the product of vited_linear_bwd_weight with the same meanings (dbias[i] may be null).  Sharing the
 * chip's workgroup slots between the products cuts the number of row splits - and the fp32 partial slabs - several-fold.
 * bf16 only, every K a multiple of 384 and every M >= 4096 (vited_linear_bwd_weight_batched_supported); otherwise the caller
 * issues vited_linear_bwd_weight per product. */
int vited_linear_bwd_weight_batched_supported(int count, const int64_t* M, const int64_t* N, const int64_t* K, int dtype);
int64_t vited_linear_bwd_weight_batched_workspace_bytes(int count, const int64_t* M, const int64_t* N, const int64_t* K);
int vited_linear_bwd_weight_batched(int count, const void* const* dY, const int64_t* lddy, const void* const* X,
                                    const int64_t* ldx, const int64_t* M, const int64_t* N, const int64_t* K, float* const* dW,
                                    float* const* dbias, int dtype, int accumulate, float* workspace, int64_t workspace_bytes,
                                    void* stream);

/* ---- Linear fused with the LayerNorm on the other side of it (row-complete tile, bf16 MFMA; gemm_row.hip, gemm_row768.hip) ----
 * The reference's blocks are chains  x = x + f(norm(x))  (Block.forward vision_transformer.py:124-127, CrossBlock.forward
 * :268-272, norm_layer :348): every residual Linear (attn.proj :38, cross_attn.proj :156, timm Mlp fc2) is followed by the next
 * sub-block's LayerNorm, and every Linear that consumes a LayerNorm's output (qkv :34, q :151, kv :152, fc1) is followed, in
 * backward, by that LayerNorm's backward.  These two entries do each pair in ONE kernel so the LayerNorm is not a separate
 * pass over the fp32 residual stream.  bf16 operands, K % 64 == 0, and the embed width one of
 *   N == 384 (configs/puzzle, configs/hisfrag, configs/test), K >= 64;
 *   N == 768 (ViT-Base: the reference's michigan base_patch16_384), K >= 768.
 * The entries take every such shape.  vited_linear_layernorm_supported() tells whether a caller SHOULD use them: at 384 for every
 * such shape; at 768 only where they measured faster than the two kernels - more than 24,576 rows and K neither N nor 4 N
 * (DESIGN.md section 35).  Otherwise the caller runs vited_gemm + vited_layernorm_fwd / vited_layernorm_bwd. */
int vited_linear_layernorm_supported(int64_t M, int64_t N, int64_t K);

/* y = residual + a . w^T + bias   (fp32 [M, N], row stride ldy; residual fp32 row stride ldr, may alias y row for row)
 * h = LayerNorm(y; gamma, beta, eps) bf16 [M, N] (row stride ldh), mean / rstd fp32 [M]   - or h == null: no LayerNorm
 *   a bf16 [M, K] (lda), w bf16 [N, K] (ldw), bias fp32 [N] or null */
int vited_linear_residual_layernorm_fwd(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias,
                                        const float* residual, int64_t ldr, float* y, int64_t ldy, const float* gamma,
                                        const float* beta, float eps, void* h, int64_t ldh, float* mean, float* rstd,
                                        int64_t M, int64_t N, int64_t K, void* stream);

/* The same with y = residual + row_scale[m] * (a . w^T + bias) (stochastic depth, see vited_gemm_scaled); the LayerNorm statistics
 * are those of the scaled y.  row_scale fp32 [M]; null = vited_linear_residual_layernorm_fwd (the unscaled kernel instance). */
int vited_linear_residual_layernorm_fwd_scaled(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias,
                                               const float* residual, int64_t ldr, const float* row_scale, float* y, int64_t ldy,
                                               const float* gamma, const float* beta, float eps, void* h, int64_t ldh, float* mean,
                                               float* rstd, int64_t M, int64_t N, int64_t K, void* stream);

/* dh = dy . wt^T  (wt = the transposed weight shadow, bf16 [N, K]: dX of y = LN(x) W^T), never written anywhere;
 * dx_out = (dx_in ? dx_in : 0) + LN'(dh; x, mean, rstd, gamma)  fp32 (dx_out may alias dx_in), optional bf16 copy dx_lp;
 * dgamma / dbeta: column sums of dh * xhat / dh, overwritten or (accumulate != 0) added.  workspace >= *_workspace_bytes.
 * With dgamma == dbeta == null the column partials stay in `workspace` as [vited_linear_layernorm_bwd_partial_rows_n(M, N)][2][N]
 * fp32 for vited_layernorm_bwd_finish_batched, which sums the partials of several LayerNorms in one launch. */
/* The same with the contraction dim cut into `segments` column blocks of seg_k, block j read from the tensor at
 * dy + j * seg_stride (elements): one [M, seg_k] tensor per decoder block (each contiguous for its own attention backward), all
 * contracted against wt [N, segments * seg_k] in one kernel. */
int vited_linear_layernorm_bwd_segmented(const void* dy, int64_t lddy, int64_t seg_k, int64_t seg_stride, int64_t segments,
                                         const void* wt, int64_t ldwt, const float* x, int64_t ldx, const float* gamma,
                                         const float* mean, const float* rstd, const float* dx_in, int64_t dx_in_ld,
                                         float* dx_out, int64_t dx_out_ld, void* dx_lp, int64_t dx_lp_ld, float* dgamma,
                                         float* dbeta, int accumulate, int64_t M, int64_t N, float* workspace,
                                         int64_t workspace_bytes, void* stream);
int64_t vited_linear_layernorm_bwd_partial_rows(int64_t M);               /* N == 384 */
int64_t vited_linear_layernorm_bwd_partial_rows_n(int64_t M, int64_t N);  /* either width; 0 for any other N */
int vited_layernorm_bwd_finish_batched(int count, const float* const* partial, const int* nparts, float* const* dgamma,
                                       float* const* dbeta, const int* accumulate, int64_t dim, void* stream);
int64_t vited_linear_layernorm_bwd_workspace_bytes(int64_t M, int64_t N);
int vited_linear_layernorm_bwd(const void* dy, int64_t lddy, const void* wt, int64_t ldwt, const float* x, int64_t ldx,
                               const float* gamma, const float* mean, const float* rstd, const float* dx_in,
                               int64_t dx_in_ld, float* dx_out, int64_t dx_out_ld, void* dx_lp, int64_t dx_lp_ld,
                               float* dgamma, float* dbeta, int accumulate, int64_t M, int64_t N, int64_t K,
                               float* workspace, int64_t workspace_bytes, void* stream);

/* vited_linear_layernorm_bwd with dx_lp[m, :] = bf16(lp_scale[m] * dx_out[m, :]) (see vited_layernorm_bwd_scaled); dx_lp is
 * required.  lp_scale == null is vited_linear_layernorm_bwd (the unscaled kernel instance). */
int vited_linear_layernorm_bwd_scaled(const void* dy, int64_t lddy, const void* wt, int64_t ldwt, const float* x, int64_t ldx,
                                      const float* gamma, const float* mean, const float* rstd, const float* dx_in,
                                      int64_t dx_in_ld, float* dx_out, int64_t dx_out_ld, void* dx_lp, int64_t dx_lp_ld,
                                      const float* lp_scale, float* dgamma, float* dbeta, int accumulate, int64_t M, int64_t N,
                                      int64_t K, float* workspace, int64_t workspace_bytes, void* stream);

/* ---- norm_context + kv projection of all decoder blocks as one GEMM (context_fold.hip) ----
 * Every CrossBlock normalises the SAME encoder features with its own norm_context (vision_transformer.py:245,269-270) before
 * its kv projection (:152,177-179).  With xhat = LayerNorm(features; 1, 0):  kv_l = xhat (W_l o gamma_l)^T + (W_l beta_l + b_l).
 * vited_fold_context_weights writes the folded bf16 weights of `count` (<= 16) blocks stacked [count * N, K], their transpose
 * [K, count * N] and the folded fp32 bias [count * N]; vited_unfold_context_grads turns the gradient of the folded weights /
 * bias (dwf [count * N, K], dbf [count * N], fp32) back into dW_l, db_l (may be null), dgamma_l, dbeta_l - overwritten, or added
 * when accumulate != 0.  Pointer arrays are host arrays of device pointers. */
int vited_fold_context_weights(int count, const float* const* w, const float* const* bias, const float* const* gamma,
                               const float* const* beta, int64_t N, int64_t K, void* w_out, void* wt_out, float* bias_out,
                               void* stream);
int vited_unfold_context_grads(int count, const float* dwf, const float* dbf, const float* const* w, const float* const* gamma,
                               const float* const* beta, float* const* dw, float* const* dbias, float* const* dgamma, float* const* dbeta, int64_t N,
                               int64_t K, int accumulate, void* stream);

/* ---- fused MLP branch of a block: y = x + fc2(gelu(fc1(LayerNorm(x)))) (vision_transformer.py:126,271; timm Mlp :115,:259) ---- */

/* One kernel for the second half of Block.forward / CrossBlock.forward (SURVEY.md section 8(b) "optional fused mlp"): LayerNorm
 * (eps as given), fc1 + bias, exact-erf GELU, fc2 + bias and the residual add, bf16 MFMA with fp32 accumulation; the LayerNorm
 * output and the hidden activation stay on chip.  Covers dim 384 / hidden 1536 (every shipped pjs config); other shapes return
 * VITED_ERR_UNSUPPORTED and the caller runs vited_layernorm_fwd + vited_gemm(GELU_GRAD) + vited_gemm(RESIDUAL) instead.
 *   x, y        fp32 [rows, dim] (row strides ldx, ldy); y may not alias x
 *   w1, w2      bf16 [hidden, dim], [dim, hidden] dense (the nn.Linear weights in the activation dtype); b1, b2, gamma, beta fp32
 *   h, gd, u, mean, rstd   what the backward kernels read - LN(x) bf16 [rows, dim], gelu'(z) and gelu(z) bf16 [rows, hidden]
 *               (dense), row statistics fp32 [rows] - all five given, or all five null for inference (nothing is saved) */
int vited_mlp_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, const void* w1, const float* b1,
                  const void* w2, const float* b2, float* y, int64_t ldy, void* h, void* gd, void* u, float* mean,
                  float* rstd, int64_t rows, int64_t dim, int64_t hidden, float eps, void* stream);

/* One encoder Block forward (Block.forward, vision_transformer.py:124-127) behind one call: the launch sequence
 * LayerNorm -> qkv GEMM -> attention -> proj + residual -> fused MLP branch on `stream` (5 launches; 7 when the MLP shape is
 * outside vited_mlp_fwd's cover).  bf16 activations, fp32 residual stream, inference form (nothing saved for backward).
 * The whole-block entries (this one and vited_cross_block_fwd) have no q/k-norm.
 *   x, y       fp32 [batch * tokens, dim] dense; y may not alias x
 *   wqkv [3 dim, dim], wproj [dim, dim], w1 [hidden, dim], w2 [dim, hidden]   bf16 dense; biases and LayerNorm parameters fp32
 *   workspace  >= vited_block_workspace_bytes(), 256-byte aligned */
int64_t vited_block_workspace_bytes(int64_t batch, int64_t tokens, int64_t dim, int64_t hidden, int heads);
int vited_block_fwd(const float* x, float* y, int64_t batch, int64_t tokens, int64_t dim, int heads, int64_t hidden,
                    const float* ln1_g, const float* ln1_b, const void* wqkv, const float* bqkv, const void* wproj,
                    const float* bproj, const float* ln2_g, const float* ln2_b, const void* w1, const float* b1,
                    const void* w2, const float* b2, float eps, void* workspace, int64_t workspace_bytes, void* stream);

/* One decoder CrossBlock forward (CrossBlock.forward, vision_transformer.py:268-272: self-attention branch, cross-attention of the
 * image-2 tokens over the image-1 features, MLP branch) behind one call - a launch sequence on `stream`, inference form.
 *   x          fp32 [batch * tokens, dim]       the image-2 token stream (cls + patches)
 *   context    fp32 [batch * ctx_tokens, dim]   the encoder features of image 1
 *   y          fp32 [batch * tokens, dim]; may not alias x
 *   ln1 / lnq / lnc / ln2   norm1, norm_cross, norm_context, norm2 (gamma, beta fp32)
 *   wqkv [3 dim, dim], wproj, wq, wcproj [dim, dim], wkv [2 dim, dim], w1 [hidden, dim], w2 [dim, hidden]   bf16 dense; biases fp32
 *   workspace  >= vited_cross_block_workspace_bytes(), 256-byte aligned */
int64_t vited_cross_block_workspace_bytes(int64_t batch, int64_t tokens, int64_t ctx_tokens, int64_t dim, int64_t hidden, int heads);
int vited_cross_block_fwd(const float* x, const float* context, float* y, int64_t batch, int64_t tokens, int64_t ctx_tokens,
                          int64_t dim, int heads, int64_t hidden, const float* ln1_g, const float* ln1_b, const void* wqkv,
                          const float* bqkv, const void* wproj, const float* bproj, const float* lnq_g, const float* lnq_b,
                          const float* lnc_g, const float* lnc_b, const void* wq, const float* bq, const void* wkv,
                          const float* bkv, const void* wcproj, const float* bcproj, const float* ln2_g, const float* ln2_b,
                          const void* w1, const float* b1, const void* w2, const float* b2, float eps, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* ---- optimizer step on the flat gradient buffer ----------------- */

/* Gradient clip + AdamW + bf16 weight-shadow refresh + gradient zeroing in three launches (sum of squares, a one-workgroup
 * decision, the update); replaces clip_grad_norm_ + optimizer.step() + zero_grad() of misc/utils.py:215-223 /
 * misc/engine.py:231 and the torch.optim.AdamW that misc/optimizer.py:25-27 builds (same update rule; parity in
 * tests/test_gpu_engine.py).
 *   desc        DEVICE array of count x 10 int64, one row per parameter:
 *               {p fp32 [rows, cols], g fp32 (its slice of grad_flat), exp_avg, exp_avg_sq, shadow bf16 [rows, cols] or 0,
 *                shadow_t bf16 [cols, rows] or 0, rows, cols, first_tile, group}
 *               first_tile = running sum of ceil(rows/64) * ceil(cols/64); total_tiles the sum over all rows.
 *   grad_flat   the contiguous fp32 gradient buffer every g points into (the L2 norm is taken over all of it)
 *   hyper       DEVICE fp32 array: [0] = number of updates applied so far (an applied update increments it: bias correction
 *               uses the incremented value), [1] = skip flag, [2] = number of updates skipped, [3..5] the EMA words of the *_ema entries below (never
 *               read or written here), [6..7] unused, then 8 floats
 *               per parameter group {lr, beta1, beta2, eps, weight_decay, 0, 0, 0} - device-resident so that a replayed
 *               hipGraph follows lr_scheduler.step_update (misc/engine.py:228)
 *   max_norm    clip_grad_norm_ threshold (<= 0: no clipping); norm_out (nullable) receives the pre-clip norm
 *   zero_grad   != 0: every g is zeroed after it was read
 *   workspace   >= vited_adamw_workspace_bytes()
 * Skipping (what GradScaler.step does for the reference, misc/utils.py:206-226): with hyper[1] != 0 and a pre-clip norm
 * that is inf or NaN, p, the moments and the shadows keep their bits, g is still zeroed when zero_grad is set, hyper[0]
 * stays, hyper[2] goes up by one and norm_out receives the non-finite norm.  With hyper[1] == 0 nothing is ever skipped (a
 * non-finite gradient then reaches its parameter).  The norm is that of grad_flat as passed in, i.e. of the ALL-REDUCED buffer in a
 * data-parallel run, so every rank takes the same decision.  On finite gradients the flag changes no bit of any output. */
int64_t vited_adamw_workspace_bytes(void);
int vited_adamw_step(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                     float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                     int64_t workspace_bytes, void* stream);

/* torch.optim.SGD (dampening 0; misc/optimizer.py:22-24 builds it with nesterov=True) in place of AdamW: same arguments, same
 * launches, same hyper header (skipping included), same workspace (vited_adamw_workspace_bytes).
 *   desc row    {p, g, momentum_buffer (may be 0 when the group's momentum is 0), 0, shadow, shadow_t, rows, cols, first_tile, group}
 *   group words {lr, momentum, nesterov (0 / 1), 0, weight_decay, 0, 0, 0}
 *   per element g' = g * clip + weight_decay * p;  buf = momentum * buf + g';  p -= lr * (nesterov ? g' + momentum * buf : buf)
 * A zero momentum buffer makes the first update torch's (buf = g'); with momentum == 0 buf is neither read nor written. */
int vited_sgd_step(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                   float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                   int64_t workspace_bytes, void* stream);

/* The same two updates with an exponential moving average of the parameters (timm's ModelEmaV2, --model-ema) kept in the update
 * launch; every other output is bit for bit what vited_adamw_step / vited_sgd_step give.  The rule is csrc/optim_update.h's
 * (ema_decay_at, ema_blend); with d = hyper[3], the warmup flag hyper[4] and n = hyper[5], the EMA updates done so far, an applied
 * update that produced the new parameter p' also does, per element,
 *     d_t = warmup ? min(d, (1 + n) / (10 + n)) : d          all fp32, n as fp32
 *     e'  = fl(fl(d_t * e) + fl((1.0f - d_t) * p'))           two rounded products and a rounded sum, never an fma
 * and hyper[5] goes up by one.  A skipped update leaves e and hyper[5] alone.  With a momentum of 0 the SGD entry still updates and
 * averages p.  vited_adamw_step / vited_sgd_step never read or write hyper[3..5].
 *   ema_flat    DEVICE fp32 [ema_numel], 16-byte aligned, laid out like grad_flat: the average of a row's p lies at the offset its g
 *               has in grad_flat (the 10-word descriptor row is the one above); it may not overlap any other buffer
 * VITED_ERR_BAD_ARG before any launch: ema_flat null or not 16-byte aligned, ema_numel < grad_numel, and whatever the entries above
 * refuse. */
int vited_adamw_step_ema(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                         float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                         int64_t workspace_bytes, float* ema_flat, int64_t ema_numel, void* stream);
int vited_sgd_step_ema(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                       float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                       int64_t workspace_bytes, float* ema_flat, int64_t ema_numel, void* stream);

/* Exchange every parameter of the table with its average, element for element, and rewrite the row's shadow and shadow_t (where not
 * 0) from the value now in p: one launch over the update's descriptor table and 64 x 64 tiling (words 2, 3 and 9 of a row are not
 * read).  Evaluation on the averaged weights happens between two calls; the second restores every bit of p, e and (shadows that were
 * current) both shadows.  ema_flat and grad_flat as above; the caller guarantees that ema_flat covers grad_flat's extent.
 * VITED_ERR_BAD_ARG before the launch: a null desc, ema_flat or grad_flat, ema_flat not 16-byte aligned, count or total_tiles < 1. */
int vited_ema_swap(const int64_t* desc, int count, int64_t total_tiles, float* ema_flat, const float* grad_flat, void* stream);

/* LAMB (You et al. 2020, Algorithm 2, with timm's Lamb conventions: bias correction, gradient averaging, weight decay inside the update,
 * the trust ratio only where it applies) in place of AdamW: same arguments, same descriptor row (exp_avg, exp_avg_sq), same hyper header
 * (skipping and the EMA words included).  The rule is csrc/optim_update.h's (lamb_u, lamb_ratio); with c the clip coefficient and t =
 * hyper[0] after the decision, per element and per tensor (= descriptor row)
 *     g' = g c;  m = m + (g' - m)(1 - beta1);  v = beta2 v + (1 - beta2) g' g'
 *     u  = (m / (1 - beta1^t)) / (sqrt(v) / sqrt(1 - beta2^t) + eps) + weight_decay p
 *     r  = (weight_decay == 0 and always_adapt == 0) ? 1 : ((|p| > 0 and |u| > 0) ? |p| / |u| : 1);  trust_clip != 0: r = min(r, 1)
 *     p  = p - lr r u
 * |.| is the 2-norm over the tensor, from fp32 sums of squares taken in a fixed order (no atomics: bits do not depend on scheduling).
 *   group words {lr, beta1, beta2, eps, weight_decay, always_adapt (0 / 1), trust_clip (0 / 1), 0}
 *   workspace   >= vited_lamb_workspace_bytes(total_tiles, count) (0 for arguments the step entries refuse): the words of
 *               vited_adamw_workspace_bytes(), then ratio[count] - r of every row as of the latest applied update, word 1028 + row -
 *               then {sum p^2, sum u^2} per tile
 * Five launches: sum of squares, decision, moments and per-tile sums, one wave per row for r, the apply pass (p, both shadows, the
 * average, g zeroed).  g is read by the third launch only and written by the last only, so zero_grad == 0 leaves its bits alone.  A
 * skipped update leaves p, m, v, the shadows, the average and ratio alone and still zeroes g when zero_grad is set.  The clip is the
 * step's own max_norm; there is no second max_grad_norm. */
int64_t vited_lamb_workspace_bytes(int64_t total_tiles, int count);
int vited_lamb_step(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                    float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                    int64_t workspace_bytes, void* stream);
int vited_lamb_step_ema(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                        float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                        int64_t workspace_bytes, float* ema_flat, int64_t ema_numel, void* stream);

/* Lion (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms", with timm's Lion conventions) in place of AdamW: same
 * arguments and argument checks, same three launches, same hyper header (skipping and the EMA words included), same workspace
 * (vited_adamw_workspace_bytes).  One moment, no step count in the rule (hyper[0] still counts the applied updates), no bias correction.
 *   desc row    {p, g, exp_avg, 0, shadow, shadow_t, rows, cols, first_tile, group}
 *   group words {lr, beta1, beta2, 0, weight_decay, 0, 0, 0}
 * The rule is csrc/optim_update.h's (lion_piece); with c the clip coefficient, per element
 *     g' = g c;  pe = p (1 - lr weight_decay);  s = sign(beta1 m + (1 - beta1) g')      +1, -1, 0 for 0, NaN for NaN
 *     p  = pe - lr s;  m = m + (g' - m)(1 - beta2)
 * Every product is rounded on its own, never contracted into an fma: the sign is decided by rounding where the two terms nearly
 * cancel, and so the kernel gives the bits of the same rule in separate fp32 operations.  12 B read and 12 B written per element, and
 * 4 B of shadows.  vited_lion_step_ema keeps the average as vited_adamw_step_ema does (same further arguments and checks). */
int vited_lion_step(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                    float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                    int64_t workspace_bytes, void* stream);
int vited_lion_step_ema(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                        float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                        int64_t workspace_bytes, float* ema_flat, int64_t ema_numel, void* stream);

/* Muon (Jordan et al. 2024, with torch.optim.Muon's conventions) for the 2-D tensors of the Muon groups and vited_adamw_step's rule, bit
 * for bit from the same tile body, for every tensor of another group (all 1-D parameters, cls_token, pos_embed, the patch projection,
 * the head): one optimizer, one flat buffer.  The rule is csrc/muon_update.h's; with c the clip coefficient, per Muon tensor [rows, cols]
 *     g'  = g c;  buf = buf + (g' - buf)(1 - momentum);  u = nesterov ? g' + (buf - g') momentum : buf
 *     X   = bf16(u / max(|u|_F, eps)), stored transposed when rows > cols, so that X is [m, n] with m <= n
 *     ns_steps times:  A = bf16(X X^T);  B = bf16(ns_b A + ns_c A A);  X = bf16(ns_a X + B X)
 *     p   = p (1 - lr weight_decay) - lr adj O,   O = X transposed back,
 *     adj = sqrt(max(1, rows / cols)) (adjust == 0) or 0.2 sqrt(max(rows, cols)) (adjust == 1, torch's 'match_rms_adamw')
 * bf16 operands and fp32 accumulation on the matrix cores; the only roundings to bf16 are at the three stores; the fp32 expressions of
 * the two epilogues are separate rounded operations, never an fma.  |u|_F comes from fp32 sums in a fixed order; there are no atomics,
 * so two runs give the same bits.
 *   desc row     the family's; word 2 is momentum_buffer on a Muon tensor and exp_avg on an aux tensor, word 3 exp_avg_sq on an aux
 *                tensor and unused on a Muon tensor
 *   group words  Muon group {lr, momentum, nesterov (0 / 1), eps, weight_decay, adjust (0 / 1), kind = 1, 0}; aux group AdamW's words
 *                with kind = 0 in word 6.  Word 0 is the rate in both.
 * The arguments of vited_lamb_step (vited_lamb_step_ema) come first, then
 *   tensor_tab   DEVICE int64 [count x 4]: {base of the tensor's region in the bf16 scratch in elements, or -1 for an aux tensor; mp; np;
 *                tall (rows > cols)} with m = min(rows, cols), n = max(rows, cols), mp and np these padded up to multiples of 64.  A
 *                region holds X0 [mp, np], X1, XT0 [np, mp], XT1, A [mp, mp], B [mp, mp]: 4 mp np + 2 mp mp elements, regions in table
 *                order without gaps.  This table decides which rule a tensor takes.
 *   tiles_sq     DEVICE int64 [n_sq x 8]: one row {tensor, tile row, tile column, base, mp, np, tall, 0} per 64 x 64 tile of every Muon
 *                tensor's A (and B): n_sq = sum of (mp / 64)^2
 *   tiles_x      DEVICE int64 [n_x x 8]: the same row per 64 x 64 tile of every Muon tensor's X: n_x = sum of (mp / 64)(np / 64)
 *   host_meta    HOST int64 [count x 5]: {rows, cols, ndim, is_muon, group} of every row of desc, from which the entries check the
 *                counts, the workspace and the refusals below before any launch
 *   host_kinds   HOST int64 [groups]: the kind word of every group as hyper holds it (1 Muon, 0 aux); a tensor whose is_muon disagrees
 *                with the kind of its group is refused, so no kernel reads one rule's group words as the other's
 *   ns_steps, ns_a, ns_b, ns_c   the Newton-Schulz steps (1..16) and coefficients, by value: a captured update bakes them in
 *   workspace    >= vited_muon_workspace_bytes(count, rows, cols, is_muon) (HOST int64 arrays; host-only; 0 for arguments the entries
 *                refuse): 1028 + count + total_tiles floats padded to a multiple of 64 floats, then the bf16 scratch
 * 6 + 3 ns_steps launches: sum of squares, decision, moments (aux tensors are finished here), one wave per tensor for |u|_F, pack, three
 * grouped GEMM launches per step over all Muon tensors at once, apply (p, both shadows, the average, g zeroed).  g is written by a
 * tensor's last pass only, so zero_grad == 0 leaves its bits alone.  A skipped update leaves p, buf, the moments, the shadows and the
 * average alone and still zeroes g when zero_grad is set.
 * VITED_ERR_BAD_ARG before any launch: a null or misaligned pointer, a Muon tensor whose ndim is not 2, ns_steps < 1 or > 16, table
 * counts that do not follow from host_meta, a tensor whose is_muon and whose group's kind disagree, and whatever vited_lamb_step refuses.  VITED_ERR_UNSUPPORTED: a Muon tensor whose short
 * side exceeds 1024. */
int64_t vited_muon_workspace_bytes(int count, const int64_t* rows, const int64_t* cols, const int64_t* is_muon);
int vited_muon_step(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                    float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                    int64_t workspace_bytes, void* stream, const int64_t* tiles_sq, int64_t n_sq, const int64_t* tiles_x,
                    int64_t n_x, const int64_t* tensor_tab, const int64_t* host_meta, const int64_t* host_kinds, int groups,
                    int ns_steps, float ns_a, float ns_b, float ns_c);
int vited_muon_step_ema(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                        float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                        int64_t workspace_bytes, float* ema_flat, int64_t ema_numel, void* stream, const int64_t* tiles_sq,
                        int64_t n_sq, const int64_t* tiles_x, int64_t n_x, const int64_t* tensor_tab,
                        const int64_t* host_meta, const int64_t* host_kinds, int groups, int ns_steps, float ns_a, float ns_b,
                        float ns_c);

/* One step of a per-iteration learning-rate schedule on the device (misc/lr_scheduler.py through misc/engine.py:228; the rules are
 * csrc/lr_schedule.h, in fp64): one launch of one workgroup, queued behind the update it follows.
 *   t = *counter;  for g < groups: dst[first + stride * g] = (float)(lr_schedule_value(table, base[g], t) * scale[g]);  *counter = t + 1
 *   table      DEVICE fp64 [44]: kind (0 cosine, 1 linear, 2 step, 3 multistep), warmup_t, warmup_lr_init, t_initial, lr_min,
 *              cycle_limit, warmup_prefix, lr_min_rate, decay_t, decay_rate, gamma, the milestone count, up to 32 ascending milestones
 *   base       DEVICE fp64 [groups]: every group's initial_lr;  scale  DEVICE fp64 [groups]: its lr_scale (1 where it has none)
 *   counter    DEVICE int64 [1]: the index of the update just done, advanced by the launch
 *   dst        DEVICE fp32 [dst_words]; the hyper array of vited_adamw_step / vited_sgd_step takes first = 8, stride = 8
 *   last_lr    DEVICE fp32 [groups] or null: receives the same values; may not overlap the words written in dst
 * Everything is read from device memory, so a captured hipGraph follows a schedule or a counter that was copied into these buffers.
 * No other word of dst is touched.  VITED_ERR_BAD_ARG: a null table, base, scale, counter or dst; groups outside [1, 4096];
 * first < 0, stride < 1 or a last word outside dst; fp64 / int64 pointers not 8-byte aligned, fp32 ones not 4-byte aligned. */
int vited_lr_schedule_step(const double* table, const double* base, const double* scale, int groups, int64_t* counter,
                           float* dst, int64_t dst_words, int64_t first, int64_t stride, float* last_lr, void* stream);

/* One record of the learning-rate range test (the reference's lr_finder.py; the rule is csrc/lr_finder.h, in fp64): one launch of one
 * workgroup, queued behind the training step whose loss it reads.  With i = state[0], while state[1] == 0 and 0 <= i < num_iter:
 *   s = (i == 0 or smooth_f == 0) ? loss : smooth_f * loss + (1 - smooth_f) * s_prev;   best = (i == 0 or s < best) ? s : best
 *   history[i] = {start[0] * (end[0] / start[0]) ** (i / num_iter), loss, s};   state[0] = i + 1
 *   state[1] = 3 where the loss is not finite, else 2 where s > diverge_th * best, else 1 where i + 1 == num_iter, else 0
 *   dst[first + stride * g] = state[1] == 0 ? (float)(start[g] * (end[g] / start[g]) ** ((i + 1) / num_iter)) : 0.0f
 * In every other state the launch writes 0.0f into the rate words and touches neither the history nor the state.
 *   loss       DEVICE fp32 [1]: the loss of the iteration that just ran
 *   state      DEVICE 4 words of 8 bytes: int64 rows written, int64 halt state (0 running, 1 num_iter reached, 2 diverged, 3 loss not
 *              finite), fp64 s of the last row, fp64 best; all zero before the first launch
 *   history    DEVICE fp64 [capacity, 3]
 *   start, end DEVICE fp64 [groups]: the ends of every group's sweep, positive and finite (the caller's check)
 *   dst        DEVICE fp32 [dst_words]; the hyper array of vited_adamw_step / vited_sgd_step takes first = 8, stride = 8
 * Everything is read from device memory, so an eager launch and a replayed one see the same thing.  No other word of dst is touched.
 * VITED_ERR_BAD_ARG: a null pointer; groups outside [1, 4096]; num_iter < 1 or > capacity; smooth_f outside [0, 1]; diverge_th not
 * above 1; first < 0, stride < 1 or a last word outside dst; 8-byte words not 8-byte aligned, fp32 ones not 4-byte aligned. */
int vited_lr_finder_step(const float* loss, int64_t* state, double* history, int64_t capacity, const double* start, const double* end,
                         int groups, int64_t num_iter, double smooth_f, double diverge_th, float* dst, int64_t dst_words,
                         int64_t first, int64_t stride, void* stream);

/* ---- attention core (F.scaled_dot_product_attention, vision_transformer.py:63-66,183-186) ----- */

/* o[b, i, h, :] = softmax_j(scale * q[b,i,h,:] . k[b,j,h,:]) v[b,j,h,:]   (no mask, no dropout)
 * q/k/v are addressed as ptr + b*bs + token*ts + h*head_dim (+d), so the packed qkv [B,N,3,h,hd]
 * (:58) and kv [B,Nc,2,h,hd] (:178) projections are consumed in place.  o is [B, Nq, H*hd] with
 * token stride o_ts; lse (fp32 [B, H, Nq]) = log sum exp of the scaled scores, saved for backward. */
int vited_attention_fwd(const void* q, int64_t q_bs, int64_t q_ts, const void* k, int64_t k_bs, int64_t k_ts,
                        const void* v, int64_t v_bs, int64_t v_ts, void* o, int64_t o_bs, int64_t o_ts,
                        float* lse, int dtype, int64_t batch, int heads, int64_t nq, int64_t nk, int head_dim,
                        float scale, void* stream);

/* The same with an indirection on the key/value side: batch item b attends over k / v of batch item kv_index[b]
 * (kv_index: DEVICE int64 [batch], values in [0, number of k/v batch items); null = identity).  Serves the pairwise
 * similarity-matrix inference (hisfrag.py:218-231): the cross-attention keys/values of an image-1 row block are projected
 * ONCE and every (i, j) pair of a pair batch reads row i's - no materialised features[i] gather (hisfrag.py:227), no
 * per-pair norm_context + kv projection (vision_transformer.py:174-179 re-runs them for every pair).  Its backward is
 * vited_attention_bwd_indexed. */
int vited_attention_fwd_indexed(const void* q, int64_t q_bs, int64_t q_ts, const void* k, int64_t k_bs, int64_t k_ts,
                                const void* v, int64_t v_bs, int64_t v_ts, const int64_t* kv_index, void* o, int64_t o_bs,
                                int64_t o_ts, float* lse, int dtype, int64_t batch, int heads, int64_t nq, int64_t nk,
                                int head_dim, float scale, void* stream);

/* dq/dk/dv in the same strided layouts; delta (fp32 [B, H, Nq]) is scratch for rowsum(dO * O). */
int vited_attention_bwd(const void* q, int64_t q_bs, int64_t q_ts, const void* k, int64_t k_bs, int64_t k_ts,
                        const void* v, int64_t v_bs, int64_t v_ts, const void* o, const void* d_o,
                        int64_t o_bs, int64_t o_ts, const float* lse, float* delta, void* dq, int64_t dq_bs,
                        int64_t dq_ts, void* dk, int64_t dk_bs, int64_t dk_ts, void* dv, int64_t dv_bs,
                        int64_t dv_ts, int dtype, int64_t batch, int heads, int64_t nq, int64_t nk,
                        int head_dim, float scale, void* stream);

/* vited_attention_bwd with the indirection of vited_attention_fwd_indexed: batch item b (a pair) reads k / v of item kv_index[b],
 * dq stays per pair, and dk / dv have kv_items batch items:  dk[g] = sum over the pairs b with kv_index[b] == g of pair b's dk
 * term, added in ascending b (the same for dv).  The training counterpart of the pair cache (hisfrag.py:117-159: the decoder
 * runs on mined pairs of a batch's images, and its cross-attention keys / values depend on image 1 only).
 *   kv_index     DEVICE int64 [batch], values in [0, kv_items)
 *   seg_order    DEVICE int64 [batch]: the stable argsort of kv_index (pair numbers grouped by item, ascending in a group)
 *   seg_offsets  DEVICE int64 [kv_items + 1]: group g is seg_order[seg_offsets[g] .. seg_offsets[g + 1])
 *   workspace    >= vited_attention_bwd_indexed_workspace_bytes(), 16-byte aligned
 * Two steps: the kernels of vited_attention_bwd (portable fp32, short-sequence MFMA or flash - vited_last_attention_path() tells
 * which) write every pair's dk / dv term into the workspace IN THE OPERAND DTYPE, then a segmented sum adds each item's terms in
 * fp32 and rounds once to the operand dtype.  No atomics: every element of every dk / dv item is written exactly once (an item
 * that no pair reads as zeros; the outputs need not be initialised) and two calls on the same operands give the same bits.
 * VITED_ERR_BAD_ARG: a null pointer, a non-positive size, a misaligned workspace.  VITED_ERR_UNSUPPORTED: dtype other than
 * VITED_F32 / VITED_BF16; batch, heads or kv_items above 65535.  VITED_ERR_WORKSPACE: workspace too small.  The index tables are
 * the caller's to validate (ops.pair_segments does): the kernels follow kv_index as given. */
int64_t vited_attention_bwd_indexed_workspace_bytes(int dtype, int64_t batch, int heads, int64_t nk, int head_dim);
int vited_attention_bwd_indexed(const void* q, int64_t q_bs, int64_t q_ts, const void* k, int64_t k_bs, int64_t k_ts,
                                const void* v, int64_t v_bs, int64_t v_ts, const int64_t* kv_index, const int64_t* seg_order,
                                const int64_t* seg_offsets, int64_t kv_items, const void* o, const void* d_o, int64_t o_bs,
                                int64_t o_ts, const float* lse, float* delta, void* dq, int64_t dq_bs, int64_t dq_ts, void* dk,
                                int64_t dk_bs, int64_t dk_ts, void* dv, int64_t dv_bs, int64_t dv_ts, int dtype, int64_t batch,
                                int heads, int64_t nq, int64_t nk, int head_dim, float scale, void* workspace,
                                int64_t workspace_bytes, void* stream);

/* Head-averaged relevancy map of one attention (scripts/visualise_attentions.py: avg_heads, generate_raw_attn,
 * generate_attn_gradcam), folded over the heads inside the kernel: no [B, H, Nq, Nk] tensor, no workspace, no atomics.
 *   P_h[i, j]  = exp(scale * q[b,i,h,:] . k[b,j,h,:] - lse[b,h,i])      lse: what vited_attention_fwd saved for these q / k
 *   dP_h[i, j] = d_o[b,i,h,:] . v[b,j,h,:]                              what the reference's attn.register_hook records
 *   mode VITED_CAM_GRAD: cam[b,i,j] = (1/H) sum_h max(P_h[i,j] * dP_h[i,j], 0)
 *   mode VITED_CAM_PROB: cam[b,i,j] = sum_h head_weight[b,h] * P_h[i,j]  (head_weight: DEVICE fp32 [B, H], null = 1/H each;
 *                        v and d_o are not read and may be null)
 * q / k / v as in vited_attention_fwd (packed projections in place); d_o is [B, Nq, H*hd] with batch stride do_bs and token stride
 * do_ts.  cam is fp32, element (b, i, j) at cam + b*cam_bs + i*cam_ld + j; every element with i < nq, j < nk is written exactly
 * once (the output need not be initialised), nothing else is touched, and two calls on the same operands give the same bits.
 * bf16 operands that meet the MFMA attention kernels' alignment (16-byte aligned pointers, strides multiples of 8 elements,
 * head_dim 32 or 64) take the MFMA kernel, everything else the portable fp32 kernel (any head_dim); vited_last_attention_path()
 * tells which.
 * VITED_ERR_BAD_ARG: unknown mode; q, k, lse or cam null; v or d_o null in VITED_CAM_GRAD; a non-positive size; cam_ld < nk;
 * cam_bs < 0.  VITED_ERR_UNSUPPORTED: dtype other than VITED_F32 / VITED_BF16; batch or heads above 65535; nq or nk above 2^20. */
enum { VITED_CAM_GRAD = 0, VITED_CAM_PROB = 1 };   /* mode of vited_attention_cam */
int vited_attention_cam(const void* q, int64_t q_bs, int64_t q_ts, const void* k, int64_t k_bs, int64_t k_ts,
                        const void* v, int64_t v_bs, int64_t v_ts, const void* d_o, int64_t do_bs, int64_t do_ts,
                        const float* lse, const float* head_weight, float* cam, int64_t cam_bs, int64_t cam_ld,
                        int mode, int dtype, int64_t batch, int heads, int64_t nq, int64_t nk, int head_dim,
                        float scale, void* stream);

/* ---- evaluation: retrieval metrics of a distance matrix (misc/wi19_evaluate.get_metrics) ------ */

/* Row records and their sums for the rows [r0, r1) of an n x n matrix D (dtype VITED_F32, VITED_BF16 or VITED_F16; row stride
 * ld elements).  Row i ranks its n columns ascending by (D[i, j], j): ties to the lower column, NaN after +inf - what
 * np.argsort(kind='stable') does.  With remove_self_column = 1 the first element of that order is dropped, whatever column it
 * is (sorted_indexes[:, 1:]).  A retrieval is correct when labels[j] == labels[i].  With from_similarity = 1, D holds
 * similarities and the row is ranked by dtype(1 - D) (fp32 subtract, one rounding): what `1 - similarity_matrix` is in the
 * reference (hisfrag.py:296), without the n x n temporary.
 *   labels   int32 [n], class ids in [0, num_classes)
 *   offsets  int32 [num_classes + 1], members int32 [n]: the columns of class c are members[offsets[c], offsets[c + 1])
 *   rows_out float64 [(r1 - r0) x 5]: sum over correct retrievals of m / rank_m (m-th correct retrieval at 1-based position
 *            rank_m), number of correct retrievals, top-1 hit (0/1), correct retrievals in the first 10, in the first 100
 *   sums     float64 [7]: sum of AP over rows with a correct retrieval, those rows, top-1 hits, sum of Pr@10, sum of Pr@100,
 *            rows without a correct retrieval, rows (r1 - r0).  Pr@k = hits_k / min(correct, k) is NaN on a row without a
 *            correct retrieval, as in the reference, and so is its sum.
 * The sums are formed in a fixed order: identical inputs give bit-identical outputs.  No workspace. */
int vited_retrieval_metrics(const void* D, int dtype, int64_t ld, int64_t n, int64_t r0, int64_t r1, const int* labels,
                            const int* offsets, const int* members, int num_classes, int remove_self_column, int from_similarity,
                            double* rows_out, double* sums, void* stream);

/* ---- evaluation: ranked retrieval lists and the wi19 ROC / F-score counts (wi19_evaluate.get_sorted_retrievals, compute_roc,
 *      compute_fscore; hisfrag_visualize_results.py's nlargest) ------ */

/* The first k retrievals of the rows [r0, r1) of an n x n matrix D (dtype, ld, from_similarity and the order as in
 * vited_retrieval_metrics: ascending by (value, column), ties to the lower column, NaN after +inf, -0 tied with +0).  With
 * remove_self_column = 1 (skip = 1) the first element of that order is dropped, whatever column it is; otherwise skip = 0.
 *   labels int32 [n], read only when hit is given; may be null otherwise
 *   idx    int32   [(r1 - r0) x k]: the columns at positions skip .. skip + k - 1 of the row's order
 *   val    float32 [(r1 - r0) x k]: the value each was ranked by, D[i, j] or dtype(1 - D[i, j]), widened
 *   hit    uint8   [(r1 - r0) x k], or null (not wanted): labels[idx] == labels[i]
 * Every output element is written exactly once; identical inputs give bit-identical outputs.  One launch, no workspace.
 * VITED_ERR_BAD_ARG: D, idx or val null; hit without labels; n < 1 or ld < n; rows not a non-empty range inside [0, n); a flag
 * other than 0 / 1; k < 1 or k + skip > n; a misaligned D.  VITED_ERR_UNSUPPORTED: an unknown dtype; k > 1024. */
int vited_retrieval_topk(const void* D, int dtype, int64_t ld, int64_t n, int64_t r0, int64_t r1, const int* labels, int k,
                         int remove_self_column, int from_similarity, int* idx, float* val, uint8_t* hit, void* stream);

/* The counts behind compute_roc and compute_fscore for the rows [r0, r1): the row kernel of vited_retrieval_metrics (same
 * arguments, same order, same checks), recording for every correct retrieval of row i its 0-based position pos after the drop.
 *   estimate int32 [n], or null: the per-row relevant_estimate of compute_fscore
 *   tp_at    uint64 [n - skip], ADDED onto (zero it before the first share): correct retrievals at each position, i.e.
 *            sorted_retrievals.sum(axis=0) over the rows of the call.  Integer adds: bit-identical whatever their order.
 *   rows_out int32 [(r1 - r0) x 2]: correct retrievals of the row, and those at positions pos < estimate[i] (0 without estimate)
 * One launch, no workspace.  VITED_ERR_BAD_ARG as vited_retrieval_metrics, and for a null or misaligned tp_at or a null rows_out. */
int vited_retrieval_curves(const void* D, int dtype, int64_t ld, int64_t n, int64_t r0, int64_t r1, const int* labels,
                           const int* offsets, const int* members, int num_classes, int remove_self_column, int from_similarity,
                           const int* estimate, uint64_t* tp_at, int* rows_out, void* stream);

/* ---- evaluation: group mAP / Pr@k of a distance matrix (misc/metric.calc_map_prak) ------------- */

/* Row records and their sums for the rows [r0, r1) of an n x n matrix D (dtype VITED_F32, VITED_BF16 or VITED_F16; row stride
 * ld elements).  Row i has the label a = labels[i]; column j is CORRECT when labels[j] is a positive label of a.  When a negative
 * relation is given, only the ELIGIBLE columns - labels[j] positive or negative for a - take part; otherwise every column does.
 * The eligible columns are ranked ascending by (D[i, j], j) (ties to the lower column, NaN after +inf: a stable argsort), the
 * first of that order is skipped whatever it is, and AP and hits_k are taken over the correct columns at the positions after it.
 *   labels      int32 [n], label ids in [0, num_labels)
 *   col_offsets int32 [num_labels + 1], col_members int32 [n]: the columns of label b are col_members[col_offsets[b], col_offsets[b + 1])
 *   pos_offsets int32 [num_labels + 1], pos_labels int32: the positive labels of a are pos_labels[pos_offsets[a], pos_offsets[a + 1]),
 *               ascending, without duplicates
 *   neg_offsets / neg_labels: the negative relation in the same form, or both null (no filter); may overlap the positives
 *   ks          HOST int32 [nk], 1 <= nk <= 8, every k >= 1: the Pr@k cut-offs
 *   rows_out    float64 [(r1 - r0) x (3 + nk)]: AP (0 when the row has no correct retrieval), valid (1 when it has one),
 *               correct retrievals, then hits_k = correct retrievals in the first k positions, for every k
 *   sums        float64 [2 + nk]: sum of AP over valid rows, valid rows, then for every k the sum over valid rows of
 *               hits_k / min(correct, k).  A row without a correct retrieval is left out of every sum, as in the reference.
 * The sums are formed in a fixed order: identical inputs give bit-identical outputs.  No workspace. */
int vited_group_retrieval_metrics(const void* D, int dtype, int64_t ld, int64_t n, int64_t r0, int64_t r1, const int* labels,
                                  int num_labels, const int* col_offsets, const int* col_members, const int* pos_offsets,
                                  const int* pos_labels, const int* neg_offsets, const int* neg_labels, const int* ks, int nk,
                                  double* rows_out, double* sums, void* stream);

/* ---- evaluation: pair-score aggregation (michigan.py:188-209, the distance maps of geshaem_test) ---- */

/* A record (i, j, score) adds d = 1 - score (fp32) to cell (i, j) and to cell (j, i) of an n x n grid of fragments (a diagonal
 * record adds it twice to (i, i)).  vited_pair_scores_add stores m records and counts them per cell; vited_pair_scores_finish
 * reduces every record stored so far.  The results are bit-identical whatever the batching and order of the records.
 *   pairs       [m, 2] fragment ids, VITED_I32 or VITED_I64, row stride pair_ld elements (column stride 1)
 *   scores      [m], VITED_F32, VITED_BF16 or VITED_F16, contiguous
 *   counts      int32 [n, n], zeroed by the caller before the first batch and accumulated by every add
 *   rec_cells   int32 [m, 2], rec_values float32 [m]: where add stores this batch's records (i, j, d); ids outside [0, n) are
 *               stored as (-1, -1), not counted, and set bit 0 of *bad (int32, device)
 * finish takes every stored record (rec_cells / rec_values [m] now span all batches, in any order) and writes, per cell,
 *   mean float32 [n, n] (fp64 sum / count, rounded once), min float32 [n, n], stdev float64 [n, n] (sample stdev, count > 1),
 *   with NaN where a cell has no value (stdev: fewer than two), and
 *   stats float64 [2]: the mean and the sample stdev of stdev over the cells with count > 1 (NaN with fewer than 1 / 2 of them).
 * n <= 46340.  workspace >= vited_pair_scores_workspace_bytes(n, m) bytes, 256-byte aligned (-1: bad n or m). */
int64_t vited_pair_scores_workspace_bytes(int64_t n, int64_t m);
int vited_pair_scores_add(const void* pairs, int pair_dtype, int64_t pair_ld, const void* scores, int score_dtype, int64_t m, int64_t n,
                          int* counts, int* rec_cells, float* rec_values, int* bad, void* stream);
int vited_pair_scores_finish(const int* rec_cells, const float* rec_values, int64_t m, int64_t n, const int* counts, float* mean,
                             float* minv, double* stdev, double* stats, int* bad, void* workspace, int64_t workspace_bytes,
                             void* stream);

/* ---- puzzle solving: the Paikin-Tal compatibility stage (paikin_tal_solver/inter_piece_distance.py), type-1 puzzles (type 2: below)
 * n pieces (2 <= n <= 46340), sides top 0, right 1, bottom 2, left 3, s^ = (s + 2) % 4.  All arrays are contiguous device memory:
 *   dq       int32 [4, n, n]: dq[s, i, j] = distance of side s of piece i to side s^ of piece j, >= 0 (the diagonal is not read)
 *   min_d, second_d int64 [n, 4]; candidate, best_buddy int32 [n, 4] (a piece id or -1); compat, mutual float32 [4, n, n]
 *   start_count int32 [n], start_total float32 [n], start_order int32 [n]; placed, changed int32 [n] (0 / 1)
 * Every result is exact and independent of the launch split (integer reductions, elementwise fp32 / fp64, a rank count).
 *
 * vited_puzzle_distances_from_logits: m ordered pairs (pi[r], pj[r]) (int64, i != j, both in [0, n)) and their logits [m, 4] fp32
 *   -> dq[s, i, j] = uint32(trunc(fp32(fp32(1 - sigmoid(logits[r, (s + 3) % 4])) * 1000))) for the 4 sides (evaluation.py:118-133).
 *   A pair outside [0, n) or with i == j is skipped and sets bit 0 of *bad (int32, device).
 * vited_puzzle_compat_init == InterPieceDistance.__init__: per (piece, side) min / second-best distance over j != i (second order
 *   statistic with multiplicity, seeded (maxsize - 1, maxsize)), the unique best-buddy candidate (-1 when the minimum is held by
 *   none or several j), compat (1 at d == 0, -maxsize at second == 0, else fp32(1 - d / second in fp64); diagonal inf), mutual
 *   ((C[s,i,j] + C[s^,j,i]) / 2 in fp32; diagonal inf), the mutual best buddies and the start-piece ordering (stable descending
 *   sort of (count, total)).
 * vited_puzzle_compat_recalc == recalculate_remaining_piece_compatibilities(placed): for unplaced i, min / second over unplaced
 *   j != i; changed[i] = 1 where one of its 8 values moved; compat of changed rows at unplaced j; mutual of every pair with a
 *   changed piece.  Best buddies and the start ordering are left alone, as the reference leaves them.
 * vited_puzzle_best_slot: the first maximum of mutual[(slot_side[k] + 2) % 4, p, slot_piece[k]] over unplaced p ascending (outer)
 *   x k < slots (inner) - the scan of solver.py:456-499 over the open slots the caller lists.  *best (int64, device) receives
 *   (key << 32) | (0xffffffff - (p * slots + k)), key the order-preserving uint32 image of the fp32 value; n * slots < 2^32. */
int vited_puzzle_distances_from_logits(const float* logits, const int64_t* pi, const int64_t* pj, int64_t m, int64_t n, int* dq,
                                       int* bad, void* stream);
int vited_puzzle_compat_init(const int* dq, int64_t n, int64_t* min_d, int64_t* second_d, int* candidate, int* best_buddy,
                             float* compat, float* mutual, int* start_count, float* start_total, int* start_order, void* stream);
int vited_puzzle_compat_recalc(const int* dq, int64_t n, const int* placed, int64_t* min_d, int64_t* second_d, float* compat,
                               float* mutual, int* changed, void* stream);
int vited_puzzle_best_slot(const float* mutual, int64_t n, const int* placed, const int* slot_piece, const int* slot_side,
                           int64_t slots, int64_t* best, void* stream);

/* ---- validation metrics of a multi-output binary classifier (main.py:49-132, DefaultTrainer.validate) -------------------------
 * vited_cls_metrics_update: one validation batch of logits [batch, classes] and targets [batch, classes] (fp32, row strides
 *   ld_logits / ld_targets >= classes, unit column stride; 1 <= classes <= 64, 1 <= batch <= INT32_MAX), one workgroup:
 *   loss   = BCEWithLogitsLoss (mean over batch x classes): an fp32 sum in a fixed order divided by batch * classes in fp32
 *   (an infinite or NaN element loss gives torch's inf / NaN);
 *   per column, pred = logit > 0 (NaN and -0 give 0): acc = (correct / batch) * 100 and sklearn 1.7's macro f1 / precision /
 *   recall (fp64) over the labels present in unique(target U pred), P = tp / npred, R = tp / ntrue (0 where the count is 0),
 *   F1 = 2 tp / (ntrue + npred); the batch values are the column sums in column order divided by classes.
 *   meters (fp64 [10], device): (sum, count) of loss, acc, f1, precision, recall, updated as AverageMeter.update(val, n=batch):
 *   sum += val * batch, count += batch (loss: the fp32 mean widened).  last (fp64 [5], device) receives the batch's 5 values.
 *   A target that is neither 0 nor 1 is not counted and sets bit 0 of *bad (int32, device).  No host sync, no allocation;
 *   bit-identical from run to run. */
int vited_cls_metrics_update(const float* logits, int64_t ld_logits, const float* targets, int64_t ld_targets, int64_t batch,
                             int64_t classes, double* meters, double* last, int* bad, void* stream);

/* ---- training: pair mining of the two-stage step on the device (hisfrag.py:117-145, michigan.py:120-150) ----------------------
 * One launch of one workgroup, no host read, a fixed-shape result.  targets int64 [n] (any values); keys fp32 [n * n] in [0, 1),
 * one per ordered cell c = i * n + j (i.i.d. uniform keys give the distribution of the reference's randperm subset).
 *   positives   the cells with i < j and targets[i] == targets[j], in ascending cell order
 *   candidates  the cells with different targets and i < j (ordered_negatives == 0, hisfrag.py:135) or i != j (!= 0,
 *               michigan.py:142-148)
 *   keep        min(#candidates, (int)(neg_per_pos * #positives)), the product formed in double and truncated; the kept negatives
 *               are the `keep` candidates with the smallest (key, cell) - the key compared as a float, equal keys to the lower
 *               cell - in that ascending order
 * Rows: positives, kept negatives, padding up to `capacity`.  groups int64 [capacity, 2] = (i, j); labels fp32 [capacity] 1 / 0;
 * weights fp32 [capacity] 1 for a pair, 0 for a padding row, which is pair (0, 0) with label 0.  When the pairs exceed capacity,
 * negatives are dropped from the end first, then positives.  seg_index [capacity] = groups[:, 1]; seg_order [capacity] its stable
 * grouping by item (ascending row number inside an item) and seg_offsets [n + 1] the group boundaries: the tables
 * vited_attention_bwd_indexed takes, padding rows at the end of item 0's group.
 * counts int32 [5]: positives found, candidates found, negatives emitted, pairs emitted, pairs dropped for lack of capacity.
 * Every output element is written on every call (the outputs need not be initialised), by plain stores: no atomics on global
 * memory, the same bits on every call.  All arrays are DEVICE memory.
 * VITED_ERR_BAD_ARG: a null pointer, n <= 0, capacity <= 0.  VITED_ERR_UNSUPPORTED: n > vited_mine_pairs_max_images() (128), or
 * capacity > 24576 (3 n (n - 1) / 2 + 1 at n = 128, rounded up to a multiple of 1024: the kernel keeps one byte of LDS per row). */
int vited_mine_pairs_max_images(void);
int vited_mine_pairs(const int64_t* targets, int n, const float* keys, double neg_per_pos, int ordered_negatives, int64_t capacity,
                     int64_t* groups, float* labels, float* weights, int64_t* seg_index, int64_t* seg_order, int64_t* seg_offsets,
                     int32_t* counts, void* stream);

/* ---- training: the loss of the two-stage step over a mined pair list, and its gradient, in one launch ---------------------------
 * BCE-with-logits over the rows of vited_mine_pairs' result: logits fp32 [rows, classes] (dense rows), labels / weights fp32 [rows],
 * counts int32 [5] as that entry leaves them; loss fp32 [1] and dlogits fp32 [rows, classes] are written in full on every call (they
 * need not be initialised).  All arrays are DEVICE memory; the pair count is read there, never on the host.  Per element (r, c), with
 * x = logits[r, c], y = labels[r], w = weights[r]:
 *   term    = (1 - y) x + m + log(exp(-m) + exp(-x - m)),  m = max(-x, 0)        (the stable form of vited_cls_metrics_update)
 *   denom   = (float)max(counts[3], 1) * (float)classes  when mean != 0,  1  otherwise (the sum)
 *   loss    = (scale * sum of (w != 0 ? w * term : +0)) / denom
 *   dlogits = w != 0 ? ((scale * w) * (sigmoid(x) - y)) / denom : +0,  sigmoid(x) - y formed without cancellation from
 *             q = e / (1 + e), e = exp(-|x|):  (1 - y) - q  for x >= 0,  q - y  for x < 0
 * The weight selects: a row with weight 0 (padding) contributes an exact +0 term and an exact +0 gradient whatever its logit holds,
 * NaN included; a NaN or inf logit in a weighted row makes the loss non-finite, as torch's does.  scale is the 1 / accumulation_steps
 * of the step.
 * One workgroup of 256 threads: thread t adds the flattened elements t, t + 256, ... in ascending order in fp32, a butterfly joins
 * each wave's 64 sums and one lane adds the four wave sums in order.  No atomics: the same bits on every call, and - padding rows
 * lying behind the pairs - the same loss bits whatever the capacity.
 * VITED_ERR_BAD_ARG: a null pointer, rows < 1, classes < 1, a scale that is not finite, a pointer not 4-byte aligned.
 * VITED_ERR_UNSUPPORTED: rows > 24576 (vited_mine_pairs' largest capacity) or classes > 64. */
int vited_mined_bce(const float* logits, const float* labels, const float* weights, const int32_t* counts, int64_t rows,
                    int64_t classes, int mean, float scale, float* loss, float* dlogits, void* stream);

/* ---- puzzle solving: the classical baseline's pixel work (solver_driver.py; paikin_tal_solver/puzzle_importer.py:182-232, :265-321,
 *      :448-473; puzzle_piece.py:535-609), type-1 puzzles (type 2: the section after this one) ------------------------------------------
 * Images, pieces and boards are uint8, HWC with 3 channels, contiguous DEVICE memory; csrc/puzzle_pixels.h states every rule.  n
 * pieces of eroded_width x eroded_width (We >= 2) cut from cells of piece_width x piece_width (P >= We).  Every output byte is written
 * exactly once by plain stores: the same bits on every call.  No host read, no synchronisation.
 *
 * vited_puzzle_cut == Puzzle.make_pieces: rows = height / P, cols = width / P, n = rows * cols; the grid is centred on the image
 *   (origin ((height - rows P) / 2, (width - cols P) / 2)); a piece is the centre crop of its cell at offset
 *   int(round((P - We) / 2.0)) (half to even).  pieces [n, We, We, 3]; piece k is cell order[k] (row-major; order int32 [n], a
 *   permutation the caller validated - an id outside [0, n) is clamped) or cell k without order.
 * vited_puzzle_resize_pieces: pieces [n, We, We, 3] -> out [n, 3, size, size], Pillow's 8-bit BILINEAR resize of each piece (22-bit
 *   fixed-point weights, horizontal pass into 8 bits, then vertical), size >= We (upscaling), size <= 1024: what
 *   vited_patchify_u8 takes.
 * vited_puzzle_pixel_distances == calculate_asymmetric_distance over all ordered pairs: dq int32 [4, n, n],
 *   dq[s, i, j] = sum over the 3 We border values of | 2 B_s(i) - B'_s(i) - B_(s+2)%4(j) |, B the border line of a side and B' the line
 *   next to it (top / bottom in column order, left / right in row order); the diagonal is 2^31 - 1.  n >= 2.  765 * 3 * We fits int32
 *   up to We = 935722.  workspace >= vited_puzzle_pixel_distances_workspace_bytes(n, We) bytes (-1: bad n or We), 8-byte aligned.
 * vited_puzzle_assemble == Puzzle.reconstruct_from_pieces: board [rows P, cols P, 3], rows * cols = n.  cells int32 [rows * cols]:
 *   -1 for an empty cell (black), else 2 * piece + framed (a piece id outside [0, n) is drawn as empty).  The piece lies at
 *   (r P + pad, c P + pad), pad = (P - We) / 2; with marker >= 0 (the colour, channel c in bits 8 c .. 8 c + 7) a framed piece gets
 *   a one-pixel ring of it; marker < 0: no frames.  Everything else is black.
 * VITED_ERR_BAD_ARG: a null pointer (order may be null), We < 2, P < We, n != rows * cols, size < We, n < 2 for the distances, a
 *   marker >= 0 with pad < 1 (the frame needs the pixel) or above 0xffffff, a misaligned workspace.  VITED_ERR_UNSUPPORTED: n > 46340,
 *   We > 935722, size > 1024.  VITED_ERR_WORKSPACE: a workspace too small. */
int vited_puzzle_cut(const uint8_t* image, int64_t height, int64_t width, int piece_width, int eroded_width, const int* order,
                     int64_t n, uint8_t* pieces, void* stream);
int vited_puzzle_resize_pieces(const uint8_t* pieces, int64_t n, int eroded_width, int size, uint8_t* out, void* stream);
int64_t vited_puzzle_pixel_distances_workspace_bytes(int64_t n, int eroded_width);
int vited_puzzle_pixel_distances(const uint8_t* pieces, int64_t n, int eroded_width, int* dq, void* workspace,
                                 int64_t workspace_bytes, void* stream);
int vited_puzzle_assemble(const uint8_t* pieces, int64_t n, int eroded_width, int piece_width, const int* cells, int64_t rows,
                          int64_t cols, int marker, uint8_t* board, void* stream);

/* ---- puzzle solving, type 2: pieces of unknown rotation (PuzzleType.type2 of paikin_tal_solver/) -----------------
 * Any side sj of piece j may meet side si of piece i.  dq2, compat and mutual are [4, n, n, 4], indexed [si, i, j, sj], contiguous
 * device memory, dq2 16-byte aligned; the slice [s, i, j, (s + 2) % 4] is the type-1 array.  Nothing here rotates a piece: the solver
 * assigns rotations, and only vited_puzzle_assemble2 turns pixels.  Every result is an integer reduction, an elementwise expression or
 * a max of packed integers, as in type 1: independent of the launch split, the same bits on every call.
 *
 * vited_puzzle_pixel_distances2 == calculate_asymmetric_distance over all ordered pairs and all 16 side pairings: dq2[si, i, j, sj] =
 *   sum over the 3 We border values of | 2 B_si(i) - B'_si(i) - B_sj(j) |, B_sj(j) read in reversed pixel order when si == sj or
 *   (si, sj) is (right, top), (top, right), (left, bottom) or (bottom, left); dq2[si, i, i, sj] = 2^31 - 1.  workspace >=
 *   vited_puzzle_pixel_distances2_workspace_bytes(n, We) bytes (-1: bad n or We), 8-byte aligned.
 * vited_puzzle_compat2_init == InterPieceDistance.__init__ for type 2: per (piece i, side si) the minimum and the second order statistic
 *   (with multiplicity, seeds (maxsize - 1, maxsize)) of dq2[si, i, j, sj] over j != i and the 4 sj, min_count int32 [n, 4] the
 *   number of candidates holding the minimum, candidate int32 [n, 4, 2] that (j, sj) when min_count is 1, else (-1, -1); compat as in
 *   type 1 on each candidate; mutual[si, i, j, sj] = (C[si, i, j, sj] + C[sj, j, i, si]) / 2 in fp32 (inf at j == i, as compat);
 *   best_buddy int32 [n, 4, 2]: the candidate (j, sj) whose own candidate is (i, si), else (-1, -1); the start keys and ordering of
 *   type 1 on those best buddies (start_total adds mutual[si, i, j, sj] in side order).
 * vited_puzzle_compat2_recalc == recalculate_remaining_piece_compatibilities(placed) for type 2, with the quirks of the type-1 entry:
 *   unplaced rows over unplaced j, compat of changed rows at unplaced j only, mutual of every pair with a changed piece.
 * vited_puzzle_best_slot2: the first maximum of mutual[side, p, slot_piece[k], slot_side[k]] over unplaced p ascending (outer) x
 *   k < slots x side 0..3 (inner) - _get_next_piece_from_pool for type 2, slot_side[k] the unrotated side of the placed piece that faces
 *   slot k.  *best = (key << 32) | (0xffffffff - ((p * slots + k) * 4 + side)); 4 * n * slots < 2^32.
 * vited_puzzle_assemble2 == Puzzle.reconstruct_from_pieces with rotations: as vited_puzzle_assemble, the piece of cell q entering as
 *   numpy.rot90(piece, rotations[q]) (int32 [rows * cols], quarter turns; only the low two bits are read).
 * Errors as in the type-1 entries; VITED_ERR_BAD_ARG also for a dq2 that is not 16-byte aligned. */
int64_t vited_puzzle_pixel_distances2_workspace_bytes(int64_t n, int eroded_width);
int vited_puzzle_pixel_distances2(const uint8_t* pieces, int64_t n, int eroded_width, int* dq2, void* workspace,
                                  int64_t workspace_bytes, void* stream);
int vited_puzzle_compat2_init(const int* dq2, int64_t n, int64_t* min_d, int64_t* second_d, int* min_count, int* candidate,
                              int* best_buddy, float* compat, float* mutual, int* start_count, float* start_total, int* start_order,
                              void* stream);
int vited_puzzle_compat2_recalc(const int* dq2, int64_t n, const int* placed, int64_t* min_d, int64_t* second_d, float* compat,
                                float* mutual, int* changed, void* stream);
int vited_puzzle_best_slot2(const float* mutual, int64_t n, const int* placed, const int* slot_piece, const int* slot_side,
                            int64_t slots, int64_t* best, void* stream);
int vited_puzzle_assemble2(const uint8_t* pieces, int64_t n, int eroded_width, int piece_width, const int* cells, const int* rotations,
                           int64_t rows, int64_t cols, int marker, uint8_t* board, void* stream);

/* ---- puzzle solving, type 2 from the pair model: turned pieces (csrc/puzzle_turn.h states every index rule) ---------
 * A turn k in 0..3 is k clockwise quarter turns: turn_k(x) = numpy.rot90(x, -k) over the pixel axes, the border that was side s becomes
 * side (s + k) % 4.  The model scores the pair (piece i, turn_k(piece j)); its bin b speaks of side si = (b + 1) % 4 of i against side
 * sj = (si + 2 - k) % 4 of the upright j, so four turns x four bins cover the 16 pairings of (i, j) once each and k = 0 is type 1.
 *
 * vited_patchify_turned / _u8: vited_patchify / vited_patchify_u8 of turn_k(image), gathered from the upright image: row (b, patch) of
 *   out equals, bit for bit, the row those entries write for the physically turned image.  turn int32 [batch] (device, one per OUTPUT
 *   image b, beside batch_index; only the low two bits are read) or NULL: every image is turned by turn_all in 0..3.
 * vited_puzzle_distances2_from_logits: m pairs (pi[r], pjt[r]) (int64; pjt = k n + j in [0, 4 n)) and their logits [m, 4] fp32 ->
 *   dq2[si, i, j, sj] = the quantisation of vited_puzzle_distances_from_logits of logits[r, b] for the 4 bins; dq2 int32 [4, n, n, 4].  A
 *   pair with i outside [0, n), pjt outside [0, 4 n) or j == i is skipped and sets bit 0 of *bad (int32, device). */
int vited_patchify_turned(const float* img, int64_t img_batch_stride, const int64_t* batch_index, const int32_t* turn, int turn_all,
                          void* out, int out_dtype, int64_t batch, int chans, int img_size, int patch, void* stream);
int vited_patchify_turned_u8(const uint8_t* img, int64_t img_batch_stride, const int64_t* batch_index, const int32_t* turn, int turn_all,
                             void* out, int out_dtype, int64_t batch, int chans, int img_size, int patch, const float* mean,
                             const float* std, void* stream);
int vited_puzzle_distances2_from_logits(const float* logits, const int64_t* pi, const int64_t* pjt, int64_t m, int64_t n, int* dq2,
                                        int* bad, void* stream);

/* ---- puzzle solving: point lookups of the mutual compatibility (mixed bags and unknown dimensions) ------------------
 * The placement loop of PaikinTalSolver reads a handful of M entries per placed piece (solver.py:490, :630, :688); these entries fetch
 * them from the device tensor, so that no host copy of M is needed.  lookups int32 [m, 3] = (side, p, q) reads mutual[side, p, q] of
 * the type-1 tensor [4, n, n]; vited_puzzle_mutual_gather2 takes lookups int32 [m, 4] = (side_p, p, q, side_q) and reads
 * mutual[side_p, p, q, side_q] of the type-2 tensor [4, n, n, 4].  out fp32 [m] receives the words of M bit for bit (-0, inf and the
 * images of -maxsize included).  A lookup with a side outside 0..3 or a piece outside [0, n) writes nothing to its slot and sets bit 0
 * of *bad (int32, device).  One thread per lookup, plain loads and stores, m >= 0; all arrays are contiguous DEVICE memory.
 * VITED_ERR_BAD_ARG: a null pointer, m < 0, n < 2 or n > 46340.  VITED_ERR_UNSUPPORTED: m > INT32_MAX. */
int vited_puzzle_mutual_gather(const float* mutual, int64_t n, const int* lookups, int64_t m, float* out, int* bad, void* stream);
int vited_puzzle_mutual_gather2(const float* mutual, int64_t n, const int* lookups, int64_t m, float* out, int* bad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VITED_H */
