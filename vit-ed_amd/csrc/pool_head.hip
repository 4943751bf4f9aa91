// Pooled head (timm global_pool='avg'): the mean over the tokens behind the prefix of every item of the last
// decoder block's output x fp32 [items, tokens, dim], plain or of LayerNorm(x[b, t]) (the `norm` of a model without fc_norm, whose
// normalised rows are then never written out), and its backward.  HBM-rate streaming kernels: x is read once forward; backward x is
// read once and dx and its low-precision copy are written once, every element of them by exactly one lane - the caller clears nothing.
//
// Mapping (pool_head.h states it and holds the arithmetic): a half-wave owns a token row, every lane moves 16-byte vectors, the row
// sums are the LayerNorm kernels' DPP half-wave sums; a workgroup owns one chunk of 64 pooled tokens of one item, so 1024 x 65 tokens
// is 1,024 workgroups and 72 x 1025 tokens is 72 x 16 = 1,152 (one workgroup per item would leave 184 of 256 CUs idle there).  The
// chunks' partial rows go to the workspace and a second small kernel adds them in ascending order; an item with one chunk is
// finished by its workgroup.  d gamma / d beta: per-lane register partials -> one LDS combine per workgroup -> [workgroups][2][dim]
// partial rows -> the LayerNorm kernels' fixed-order finishing pass.  No atomics anywhere: two runs give the same bits.
#include "common.h"
#include "pool_head.h"

int ln_bwd_finish(const float* partial, int nparts, int dim, float* dgamma, float* dbeta, int accumulate, hipStream_t s);   // layernorm.hip

#define POOL_THREADS (POOL_LANES * POOL_HALVES)

template <int VPL> __device__ __forceinline__ void pool_load(const float* __restrict__ p, int dim, int hl, float* v) {
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = pool_col(j, hl);
        const f32x4 t = c < dim ? *(const f32x4*)(p + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        v[4 * j] = t[0]; v[4 * j + 1] = t[1]; v[4 * j + 2] = t[2]; v[4 * j + 3] = t[3];
    }
}

template <int VPL, bool NORM>
__global__ void __launch_bounds__(POOL_THREADS)
token_pool_fwd_kernel(const float* __restrict__ x, int64_t x_is, int64_t x_ts, const float* __restrict__ gamma,
                      const float* __restrict__ beta, float eps, float* __restrict__ pooled, int64_t pooled_ld, float* __restrict__ mean,
                      float* __restrict__ rstd, float* __restrict__ partial, int64_t tokens, int64_t first, int dim, int nsplit) {
    extern __shared__ __attribute__((aligned(16))) float lds[];      // [8 half-waves][dim]
    const int hl = threadIdx.x & (POOL_LANES - 1), hid = threadIdx.x / POOL_LANES;
    const int64_t b = blockIdx.x / nsplit;
    const int64_t split = blockIdx.x - b * nsplit;
    int64_t t0, t1;
    pool_chunk(tokens, first, split, t0, t1);
    float acc[VPL * 4];
#pragma unroll
    for (int i = 0; i < VPL * 4; ++i) acc[i] = 0.f;
    const float inv_d = 1.f / dim;
    for (int64_t t = t0 + hid; t < t1; t += POOL_HALVES) {
        float v[VPL * 4];
        pool_load<VPL>(x + b * x_is + t * x_ts, dim, hl, v);
        if constexpr (NORM) {
            const float mu = half_wave_sum(pool_sum_part<VPL>(v)) * inv_d;
            const float rs = pool_rstd(half_wave_sum(pool_sq_part<VPL>(v, mu, dim, hl)), inv_d, eps);
            pool_acc_norm<VPL>(acc, v, mu, rs, dim, hl);
            if (mean && hl == 0) {
                mean[b * tokens + t] = mu;
                rstd[b * tokens + t] = rs;
            }
        } else {
            pool_acc_plain<VPL>(acc, v);
        }
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = pool_col(j, hl);
        if (c < dim) *(f32x4*)(lds + (size_t)hid * dim + c) = f32x4{acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]};
    }
    __syncthreads();
    const float count = (float)(tokens - first);
    for (int c = threadIdx.x; c < dim; c += POOL_THREADS) {
        const float s = pool_sum_ordered(lds + c, dim, POOL_HALVES);
        if (nsplit > 1) partial[(size_t)blockIdx.x * dim + c] = s;
        else if constexpr (NORM) pooled[b * pooled_ld + c] = pool_finish_norm(s, count, gamma[c], beta[c]);
        else pooled[b * pooled_ld + c] = pool_finish(s, count);
    }
}

// pooled[b, c] from the nsplit partial rows of item b, added in ascending chunk order
__global__ void __launch_bounds__(256)
token_pool_combine_kernel(const float* __restrict__ partial, const float* __restrict__ gamma, const float* __restrict__ beta,
                          float* __restrict__ pooled, int64_t pooled_ld, float count, int dim, int nsplit, int col_blocks) {
    const int64_t b = blockIdx.x / col_blocks;
    const int c = (int)(blockIdx.x - b * col_blocks) * 256 + threadIdx.x;
    if (c >= dim) return;
    const float s = pool_sum_ordered(partial + (size_t)b * nsplit * dim + c, dim, nsplit);
    pooled[b * pooled_ld + c] = gamma ? pool_finish_norm(s, count, gamma[c], beta[c]) : pool_finish(s, count);
}

template <int VPL> __device__ __forceinline__ void pool_store_row(float* __restrict__ dx, void* __restrict__ lp, int lp_f32, float lps,
                                                                  int dim, int hl, const float* v) {
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = pool_col(j, hl);
        if (c < dim) {
            f32x4 o{v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]};
            *(f32x4*)(dx + c) = o;
            if (lp) {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] *= lps;
                if (lp_f32) *(f32x4*)((float*)lp + c) = o;
                else *(bf16x4*)((bf16*)lp + c) = bf16x4{(bf16)o[0], (bf16)o[1], (bf16)o[2], (bf16)o[3]};
            }
        }
    }
}

template <int VPL, bool NORM>
__global__ void __launch_bounds__(POOL_THREADS)
token_pool_bwd_kernel(const float* __restrict__ g, int64_t g_ld, const float* __restrict__ x, int64_t x_is, int64_t x_ts,
                      const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ rstd,
                      float* __restrict__ dx, int64_t dx_is, int64_t dx_ts, void* __restrict__ dx_lp, int lp_f32, int64_t lp_is,
                      int64_t lp_ts, const float* __restrict__ lp_scale, float* __restrict__ partial, int64_t tokens, int64_t first,
                      int dim, int nsplit) {
    extern __shared__ __attribute__((aligned(16))) float lds[];      // with a LayerNorm: [8 half-waves][2][dim]
    const int hl = threadIdx.x & (POOL_LANES - 1), hid = threadIdx.x / POOL_LANES;
    const int64_t b = blockIdx.x / nsplit;
    const int64_t split = blockIdx.x - b * nsplit;
    int64_t t0, t1;
    pool_chunk(tokens, first, split, t0, t1);
    const float count = (float)(tokens - first);
    const float lps = lp_scale ? lp_scale[b] : 1.f;
    const int64_t lp_bytes = lp_f32 ? 4 : 2;
    char* lp_item = dx_lp ? (char*)dx_lp + b * lp_is * lp_bytes : nullptr;
    float dy[VPL * 4];
    pool_load<VPL>(g + b * g_ld, dim, hl, dy);
#pragma unroll
    for (int i = 0; i < VPL * 4; ++i) dy[i] = pool_grad(dy[i], count);
    if (split == 0) {                                   // the prefix rows take no part in the mean
        float zero[VPL * 4];
#pragma unroll
        for (int i = 0; i < VPL * 4; ++i) zero[i] = 0.f;
        for (int64_t t = hid; t < first; t += POOL_HALVES)
            pool_store_row<VPL>(dx + b * dx_is + t * dx_ts, lp_item ? lp_item + t * lp_ts * lp_bytes : nullptr, lp_f32, 1.f, dim, hl, zero);
    }
    if constexpr (!NORM) {
        for (int64_t t = t0 + hid; t < t1; t += POOL_HALVES)
            pool_store_row<VPL>(dx + b * dx_is + t * dx_ts, lp_item ? lp_item + t * lp_ts * lp_bytes : nullptr, lp_f32, lps, dim, hl, dy);
    } else {
        float gg[VPL * 4], dg[VPL * 4], db[VPL * 4];
        pool_load<VPL>(gamma, dim, hl, gg);
#pragma unroll
        for (int i = 0; i < VPL * 4; ++i) {
            gg[i] *= dy[i];
            dg[i] = 0.f;
            db[i] = 0.f;
        }
        const float inv_d = 1.f / dim;
        const float c1 = half_wave_sum(pool_sum_part<VPL>(gg)) * inv_d;
        for (int64_t t = t0 + hid; t < t1; t += POOL_HALVES) {
            float v[VPL * 4], xh[VPL * 4], o[VPL * 4];
            pool_load<VPL>(x + b * x_is + t * x_ts, dim, hl, v);
            const float mu = mean[b * tokens + t], rs = rstd[b * tokens + t];
            const float c2 = half_wave_sum(pool_bwd_parts<VPL>(dy, gg, v, mu, rs, xh, dg, db, dim, hl)) * inv_d;
            pool_bwd_out<VPL>(gg, xh, c1, c2, rs, o);
            pool_store_row<VPL>(dx + b * dx_is + t * dx_ts, lp_item ? lp_item + t * lp_ts * lp_bytes : nullptr, lp_f32, lps, dim, hl, o);
        }
        float* my = lds + (size_t)hid * 2 * dim;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = pool_col(j, hl);
            if (c < dim) {
                *(f32x4*)(my + c) = f32x4{dg[4 * j], dg[4 * j + 1], dg[4 * j + 2], dg[4 * j + 3]};
                *(f32x4*)(my + dim + c) = f32x4{db[4 * j], db[4 * j + 1], db[4 * j + 2], db[4 * j + 3]};
            }
        }
        __syncthreads();
        float* out = partial + (size_t)blockIdx.x * 2 * dim;
        for (int c = threadIdx.x; c < 2 * dim; c += POOL_THREADS) out[c] = pool_sum_ordered(lds + c, 2 * dim, POOL_HALVES);
    }
}

// what both entries check of the shape and of x
static int pool_check_shape(int64_t items, int64_t tokens, int64_t first, int64_t dim) {
    if (items <= 0 || tokens <= 0 || dim <= 0 || first < 0 || tokens <= first) return VITED_ERR_BAD_ARG;
    if (dim % 4 || dim > 128 * POOL_MAX_VPL) return VITED_ERR_UNSUPPORTED;
    if (items * pool_splits(tokens, first) > 0x7fffffffLL / 4) return VITED_ERR_UNSUPPORTED;      // grid sizes, partial-row counts
    return VITED_OK;
}
// [items, tokens, dim] through an item and a token stride: rows and items apart, 16-byte vectors (8-byte for a bf16 buffer)
static int pool_check_rows(const void* p, int64_t is, int64_t ts, int64_t tokens, int64_t dim, int align) {
    if (ts < dim || is < (tokens - 1) * ts + dim) return VITED_ERR_BAD_ARG;
    if (((uintptr_t)p & (align - 1)) || is % 4 || ts % 4) return VITED_ERR_BAD_ARG;
    return VITED_OK;
}

extern "C" int64_t vited_token_pool_workspace_bytes(int64_t items, int64_t tokens, int64_t first, int64_t dim) {
    if (pool_check_shape(items, tokens, first, dim) != VITED_OK) return 0;
    return items * pool_splits(tokens, first) * 2 * dim * (int64_t)sizeof(float);
}

extern "C" int vited_token_pool_fwd(const float* x, int64_t x_is, int64_t x_ts, const float* gamma, const float* beta, float eps,
                                    float* pooled, int64_t pooled_ld, float* mean, float* rstd, int64_t items, int64_t tokens,
                                    int64_t first, int64_t dim, float* workspace, int64_t workspace_bytes, void* stream) {
    if (!x || !pooled || (gamma && !beta) || (!gamma && (beta || mean || rstd)) || (!mean != !rstd)) return VITED_ERR_BAD_ARG;
    int rc = pool_check_shape(items, tokens, first, dim);
    if (rc != VITED_OK) return rc;
    if ((rc = pool_check_rows(x, x_is, x_ts, tokens, dim, 16)) != VITED_OK) return rc;
    if (pooled_ld < dim || pooled_ld % 4 || ((uintptr_t)pooled & 15) || (((uintptr_t)gamma | (uintptr_t)beta) & 15)) return VITED_ERR_BAD_ARG;
    if (((uintptr_t)mean | (uintptr_t)rstd) & 3) return VITED_ERR_BAD_ARG;
    const int64_t nsplit = pool_splits(tokens, first);
    if (nsplit > 1 && (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < vited_token_pool_workspace_bytes(items, tokens, first, dim)))
        return VITED_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(items * nsplit));
    const size_t lds = (size_t)POOL_HALVES * dim * sizeof(float);
    const int d = (int)dim, ns = (int)nsplit;
#define L1(V, N) hipLaunchKernelGGL((token_pool_fwd_kernel<V, N>), grid, dim3(POOL_THREADS), lds, s, x, x_is, x_ts, gamma, beta, eps, pooled, \
                                    pooled_ld, mean, rstd, workspace, tokens, first, d, ns)
#define L(V) do { if (gamma) L1(V, true); else L1(V, false); } while (0)
    switch ((int)ceil_div64(dim, 128)) {
        case 1: L(1); break;
        case 2: L(2); break;
        case 3: L(3); break;
        case 4: L(4); break;
        case 5: L(5); break;
        case 6: L(6); break;
        case 7: L(7); break;
        default: L(8); break;
    }
#undef L
#undef L1
    if (nsplit > 1) {
        const int col_blocks = (int)ceil_div64(dim, 256);
        hipLaunchKernelGGL(token_pool_combine_kernel, dim3((unsigned)(items * col_blocks)), dim3(256), 0, s, workspace, gamma, beta, pooled,
                           pooled_ld, (float)(tokens - first), d, ns, col_blocks);
    }
    return vited_check_launch();
}

extern "C" int vited_token_pool_bwd(const float* g, int64_t g_ld, const float* x, int64_t x_is, int64_t x_ts, const float* gamma,
                                    const float* mean, const float* rstd, float* dx, int64_t dx_is, int64_t dx_ts, void* dx_lp,
                                    int dx_lp_dtype, int64_t dx_lp_is, int64_t dx_lp_ts, const float* lp_scale, float* dgamma,
                                    float* dbeta, int accumulate, int64_t items, int64_t tokens, int64_t first, int64_t dim,
                                    float* workspace, int64_t workspace_bytes, void* stream) {
    if (!g || !dx || (lp_scale && !dx_lp)) return VITED_ERR_BAD_ARG;
    if (gamma && (!x || !mean || !rstd || !dgamma || !dbeta)) return VITED_ERR_BAD_ARG;
    int rc = pool_check_shape(items, tokens, first, dim);
    if (rc != VITED_OK) return rc;
    if (dx_lp && dx_lp_dtype != VITED_BF16 && dx_lp_dtype != VITED_F32) return VITED_ERR_UNSUPPORTED;
    const int lp_f32 = dx_lp && dx_lp_dtype == VITED_F32;
    if (g_ld < dim || g_ld % 4 || ((uintptr_t)g & 15) || ((uintptr_t)lp_scale & 3)) return VITED_ERR_BAD_ARG;
    if ((rc = pool_check_rows(dx, dx_is, dx_ts, tokens, dim, 16)) != VITED_OK) return rc;
    if (dx_lp && (rc = pool_check_rows(dx_lp, dx_lp_is, dx_lp_ts, tokens, dim, lp_f32 ? 16 : 8)) != VITED_OK) return rc;
    if (gamma) {
        if ((rc = pool_check_rows(x, x_is, x_ts, tokens, dim, 16)) != VITED_OK) return rc;
        if (((uintptr_t)gamma & 15) || (((uintptr_t)mean | (uintptr_t)rstd | (uintptr_t)dgamma | (uintptr_t)dbeta) & 3)) return VITED_ERR_BAD_ARG;
        if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < vited_token_pool_workspace_bytes(items, tokens, first, dim))
            return VITED_ERR_WORKSPACE;
    }
    const int64_t nsplit = pool_splits(tokens, first);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(items * nsplit));
    const size_t lds = gamma ? (size_t)POOL_HALVES * 2 * dim * sizeof(float) : 0;
    const int d = (int)dim, ns = (int)nsplit;
#define L1(V, N) hipLaunchKernelGGL((token_pool_bwd_kernel<V, N>), grid, dim3(POOL_THREADS), lds, s, g, g_ld, x, x_is, x_ts, gamma, mean, rstd, dx, \
                                    dx_is, dx_ts, dx_lp, lp_f32, dx_lp_is, dx_lp_ts, lp_scale, workspace, tokens, first, d, ns)
#define L(V) do { if (gamma) L1(V, true); else L1(V, false); } while (0)
    switch ((int)ceil_div64(dim, 128)) {
        case 1: L(1); break;
        case 2: L(2); break;
        case 3: L(3); break;
        case 4: L(4); break;
        case 5: L(5); break;
        case 6: L(6); break;
        case 7: L(7); break;
        default: L(8); break;
    }
#undef L
#undef L1
    rc = vited_check_launch();
    if (rc != VITED_OK || !gamma) return rc;
    return ln_bwd_finish(workspace, (int)(items * nsplit), d, dgamma, dbeta, accumulate, s);
}
