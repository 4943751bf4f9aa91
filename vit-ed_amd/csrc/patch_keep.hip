// Patch dropout (timm PatchDropout): the embedding stage for the KEPT patches only.
//   vited_keep_from_keys     the K smallest keys of every row, in ascending (key, index) order: argsort(randn)[:, :K] without the sort
//   vited_patchify_kept(_u8) vited_patchify(_u8) writing the kept patch rows alone; a dropped patch is never read
//   vited_tokens_kept        x[b, t] = tok[b, t] + pos[1 + patch(b, t)], and the cls row, through the keep table
//   vited_keep_inverse       inv[b, p] = kept row of patch p, or -1
//   vited_tokens_kept_bwd    d pos / d cls: per patch the sum over the samples that kept it, in ascending sample order, no atomics
// All index arithmetic is patch_keep.h (shared with tools/patchkeep_host_check.cpp).  HBM-bound data movement: coalesced, 16 bytes
// per lane on the fp32 token rows.
#include "common.h"
#include "patch_keep.h"

// ------------------------------------------------------------------------------------------------
// keep indices: one workgroup per row, the row's keys in LDS, rank by counting (every lane reads the same LDS word per step: a
// broadcast, no bank conflict).  L <= PK_MAX_KEYS.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
keep_from_keys_kernel(const float* __restrict__ keys, int* __restrict__ keep, int L, int K) {
    __shared__ float row[PK_MAX_KEYS];
    const int64_t b = blockIdx.x;
    const float* src = keys + b * L;
    for (int i = threadIdx.x; i < L; i += blockDim.x) row[i] = src[i];
    __syncthreads();
    for (int i = threadIdx.x; i < L; i += blockDim.x) {
        const int rank = pk_rank(row, L, i);
        if (rank < K) keep[b * K + rank] = i;
    }
}

extern "C" int vited_keep_from_keys(const float* keys, int32_t* keep, int64_t batch, int L, int K, void* stream) {
    if (!keys || !keep || batch <= 0 || batch > 0x7fffffff || L <= 0 || K <= 0 || K > L) return VITED_ERR_BAD_ARG;
    if (((uintptr_t)keys | (uintptr_t)keep) % 4) return VITED_ERR_BAD_ARG;
    if (L > PK_MAX_KEYS) return VITED_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(keep_from_keys_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, keys, keep, L, K);
    return vited_check_launch();
}

// ------------------------------------------------------------------------------------------------
// kept patchify: one workgroup per (sample, kept row); the element order and the arithmetic are those of patchify_kernel /
// patchify_u8_kernel (elementwise.hip), so a kept row is bit-equal to the row the full kernel writes for that patch.
// ------------------------------------------------------------------------------------------------
struct PkNorm { float scale[4], shift[4]; };

template <typename S, typename D>
__global__ void __launch_bounds__(256)
patchify_kept_kernel(const S* __restrict__ img, int64_t img_bs, const int64_t* __restrict__ bidx, const int* __restrict__ keep, int K,
                     int lead, D* __restrict__ out, int chans, int img_size, int p, PkNorm nrm) {
    const int G = img_size / p, R = pk_rows(K, lead);
    const int64_t b = blockIdx.x;
    const int r = blockIdx.y;
    const int patch = pk_patch(keep + b * K, lead, r, G * G);
    const int py = patch / G, px = patch - py * G;
    const int64_t src_b = bidx ? bidx[b] : b;
    const S* base = img + src_b * img_bs + (int64_t)(py * p) * img_size + px * p;
    const int Kp = chans * p * p;
    D* o = out + (b * R + r) * (int64_t)Kp;
    for (int e = threadIdx.x; e < Kp; e += blockDim.x) {
        const int j = e % p, ci = e / p;        // ci = c * p + i
        const int i = ci % p, c = ci / p;
        const S raw = base[((int64_t)c * img_size + i) * img_size + j];
        float v;
        if constexpr (sizeof(S) == 1) v = fmaf((float)raw, nrm.scale[c], nrm.shift[c]);
        else v = raw;
        o[e] = from_f32<D>(v);
    }
}

static int patchify_kept_args(const void* img, const int32_t* keep, int K, int lead, const void* out, int64_t batch, int chans,
                              int img_size, int patch) {
    if (!img || !keep || !out || batch <= 0 || batch > 0x7fffffff || chans <= 0 || img_size <= 0 || patch <= 0 || img_size % patch)
        return VITED_ERR_BAD_ARG;
    const int64_t n = (int64_t)(img_size / patch) * (img_size / patch);
    if ((lead != 0 && lead != 1) || K <= 0 || (int64_t)K + lead > n || (uintptr_t)keep % 4) return VITED_ERR_BAD_ARG;
    if (pk_rows(K, lead) > 65535) return VITED_ERR_UNSUPPORTED;
    return VITED_OK;
}

extern "C" int vited_patchify_kept(const float* img, int64_t img_bs, const int64_t* batch_index, const int32_t* keep, int K, int lead,
                                   void* out, int out_dtype, int64_t batch, int chans, int img_size, int patch, void* stream) {
    if (int err = patchify_kept_args(img, keep, K, lead, out, batch, chans, img_size, patch)) return err;
    if ((uintptr_t)img % 4) return VITED_ERR_BAD_ARG;
    dim3 grid((unsigned)batch, (unsigned)pk_rows(K, lead));
    hipStream_t s = (hipStream_t)stream;
    const PkNorm none = {};
    if (out_dtype == VITED_BF16)
        hipLaunchKernelGGL((patchify_kept_kernel<float, bf16>), grid, dim3(256), 0, s, img, img_bs, batch_index, keep, K, lead, (bf16*)out,
                           chans, img_size, patch, none);
    else if (out_dtype == VITED_F32)
        hipLaunchKernelGGL((patchify_kept_kernel<float, float>), grid, dim3(256), 0, s, img, img_bs, batch_index, keep, K, lead, (float*)out,
                           chans, img_size, patch, none);
    else
        return VITED_ERR_UNSUPPORTED;
    return vited_check_launch();
}

extern "C" int vited_patchify_kept_u8(const uint8_t* img, int64_t img_bs, const int64_t* batch_index, const int32_t* keep, int K, int lead,
                                      void* out, int out_dtype, int64_t batch, int chans, int img_size, int patch, const float* mean,
                                      const float* std, void* stream) {
    if (int err = patchify_kept_args(img, keep, K, lead, out, batch, chans, img_size, patch)) return err;
    if (!mean || !std || chans > 4) return VITED_ERR_BAD_ARG;
    PkNorm nrm = {};
    for (int c = 0; c < chans; ++c) {       // the folding of vited_patchify_u8, to the bit
        if (!(std[c] > 0.f)) return VITED_ERR_BAD_ARG;
        nrm.scale[c] = 1.0f / (255.0f * std[c]);
        nrm.shift[c] = -mean[c] / std[c];
    }
    dim3 grid((unsigned)batch, (unsigned)pk_rows(K, lead));
    hipStream_t s = (hipStream_t)stream;
    if (out_dtype == VITED_BF16)
        hipLaunchKernelGGL((patchify_kept_kernel<uint8_t, bf16>), grid, dim3(256), 0, s, img, img_bs, batch_index, keep, K, lead, (bf16*)out,
                           chans, img_size, patch, nrm);
    else if (out_dtype == VITED_F32)
        hipLaunchKernelGGL((patchify_kept_kernel<uint8_t, float>), grid, dim3(256), 0, s, img, img_bs, batch_index, keep, K, lead,
                           (float*)out, chans, img_size, patch, nrm);
    else
        return VITED_ERR_UNSUPPORTED;
    return vited_check_launch();
}

// ------------------------------------------------------------------------------------------------
// position embedding (and the cls row) through the keep table: one thread per 16-byte piece of an output row, one fp32 add per
// element.  tok [B * R, dim] is what the patch-embedding GEMM wrote (product + bias); x [B, rows, dim], rows = R (+ 1 with cls).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
tokens_kept_kernel(const float* __restrict__ tok, const float* __restrict__ pos, const float* __restrict__ cls, const int* __restrict__ keep,
                   int K, int lead, float* __restrict__ x, int64_t total, int n_patches, int dim4) {
    const int R = pk_rows(K, lead), first = cls ? 1 : 0, rows = R + first;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t row = i / dim4;
        const int c = (int)(i - row * dim4) * 4;
        const int64_t b = row / rows;
        const int t = (int)(row - b * rows);
        f32x4 v;
        if (t < first) {
            v = *(const f32x4*)(cls + c) + *(const f32x4*)(pos + c);
        } else {
            const int r = t - first;
            const int patch = pk_patch(keep + b * K, lead, r, n_patches);
            v = *(const f32x4*)(tok + (b * R + r) * (int64_t)(dim4 * 4) + c) + *(const f32x4*)(pos + (int64_t)(1 + patch) * (dim4 * 4) + c);
        }
        *(f32x4*)(x + row * (int64_t)(dim4 * 4) + c) = v;
    }
}

extern "C" int vited_tokens_kept(const float* tok, const float* pos, const float* cls, const int32_t* keep, int K, int lead, float* x,
                                 int64_t batch, int n_patches, int dim, void* stream) {
    if (!tok || !pos || !keep || !x || batch <= 0 || n_patches <= 0 || dim <= 0 || dim % 4) return VITED_ERR_BAD_ARG;
    if ((lead != 0 && lead != 1) || K <= 0 || (int64_t)K + lead > n_patches || (uintptr_t)keep % 4) return VITED_ERR_BAD_ARG;
    if (((uintptr_t)tok | (uintptr_t)pos | (uintptr_t)cls | (uintptr_t)x) % 16) return VITED_ERR_BAD_ARG;
    const int64_t total = batch * (pk_rows(K, lead) + (cls ? 1 : 0)) * (dim / 4);
    int64_t blocks = ceil_div64(total, 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(tokens_kept_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tok, pos, cls, keep, K, lead, x, total,
                       n_patches, dim / 4);
    return vited_check_launch();
}

// ------------------------------------------------------------------------------------------------
// inverse table: one workgroup per sample clears its n_patches entries, then scatters the kept rows (distinct within a row: no
// conflict; were a table to repeat an index, one of its rows would win and nothing would be written out of bounds)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
keep_inverse_kernel(const int* __restrict__ keep, int K, int lead, int* __restrict__ inv, int n_patches) {
    const int64_t b = blockIdx.x;
    int* mine = inv + b * n_patches;
    pk_inverse_clear(mine, n_patches, threadIdx.x, blockDim.x);
    __syncthreads();        // the workgroup's own global writes are ordered by the barrier
    pk_inverse_fill(mine, keep + b * K, K, lead, n_patches, threadIdx.x, blockDim.x);
}

extern "C" int vited_keep_inverse(const int32_t* keep, int K, int lead, int32_t* inv, int64_t batch, int n_patches, void* stream) {
    if (!keep || !inv || batch <= 0 || batch > 0x7fffffff || n_patches <= 0) return VITED_ERR_BAD_ARG;
    if ((lead != 0 && lead != 1) || K <= 0 || (int64_t)K + lead > n_patches || ((uintptr_t)keep | (uintptr_t)inv) % 4) return VITED_ERR_BAD_ARG;
    hipLaunchKernelGGL(keep_inverse_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, keep, K, lead, inv, n_patches);
    return vited_check_launch();
}

// ------------------------------------------------------------------------------------------------
// backward of vited_tokens_kept w.r.t. pos (and cls): one thread per (row q of pos, 16-byte column piece) walks the samples in
// ascending order, accumulates in fp32 and writes its piece ONCE - no atomics, so two runs agree bit for bit (the pattern of
// attn_segsum_kernel).  q = 0 is the cls row (the batch sum of row 0; exact zeros without a cls row), q = 1 + p patch p; a patch
// nobody kept gets exact zeros.  dx [B, rows, dim], rows = R + first.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
tokens_kept_bwd_kernel(const float* __restrict__ dx, const int* __restrict__ inv, float* __restrict__ dpos, float* __restrict__ dcls,
                       int64_t batch, int rows, int first, int n_patches, int dim4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)(n_patches + 1) * dim4) return;
    const int q = (int)(i / dim4), c = (int)(i - (int64_t)q * dim4) * 4;
    const int dim = dim4 * 4, R = rows - first;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (q == 0) {
        if (first)
            for (int64_t b = 0; b < batch; ++b) acc += *(const f32x4*)(dx + b * rows * (int64_t)dim + c);
        if (dcls) *(f32x4*)(dcls + c) = acc;
    } else {
        const int* col = inv + (q - 1);
        int64_t b = 0;
        for (; b + 4 <= batch; b += 4) {         // four independent lookups in flight; the adds stay in ascending sample order
            int r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = col[(b + u) * n_patches];
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool kept = r[u] >= 0 && r[u] < R;
                v[u] = kept ? *(const f32x4*)(dx + ((b + u) * rows + first + (kept ? r[u] : 0)) * (int64_t)dim + c) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (r[u] >= 0 && r[u] < R) acc += v[u];
        }
        for (; b < batch; ++b) {
            const int r = col[b * n_patches];
            if (r >= 0 && r < R) acc += *(const f32x4*)(dx + (b * rows + first + r) * (int64_t)dim + c);
        }
    }
    *(f32x4*)(dpos + (int64_t)q * dim + c) = acc;
}

extern "C" int vited_tokens_kept_bwd(const float* dx, const int32_t* inv, float* dpos, float* dcls, int64_t batch, int rows, int with_cls,
                                     int n_patches, int dim, void* stream) {
    if (!dx || !inv || !dpos || batch <= 0 || n_patches <= 0 || dim <= 0 || dim % 4 || (with_cls != 0 && with_cls != 1)) return VITED_ERR_BAD_ARG;
    if (rows <= with_cls || rows - with_cls > n_patches || (!with_cls && dcls)) return VITED_ERR_BAD_ARG;
    if (((uintptr_t)dx | (uintptr_t)dpos | (uintptr_t)dcls) % 16 || (uintptr_t)inv % 4) return VITED_ERR_BAD_ARG;
    const int64_t total = (int64_t)(n_patches + 1) * (dim / 4);
    hipLaunchKernelGGL(tokens_kept_bwd_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, (hipStream_t)stream, dx, inv, dpos,
                       dcls, batch, rows, with_cls, n_patches, dim / 4);
    return vited_check_launch();
}
