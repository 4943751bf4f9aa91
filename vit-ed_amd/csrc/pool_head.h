// The index and reduction arithmetic of the pooled-head kernels (pool_head.hip): the mean over the tokens behind a prefix of every
// item of x [items, tokens, dim], plain or of LayerNorm(x[b, t]), and its backward - written for ONE LANE's piece of a token row and
// for one workgroup's piece of an item, as plain C++, so that the same text runs in the kernels and in the host program under the
// sanitizers (tools/poolhead_host_check.cpp).
//
// Who owns what.  A token row is spread over POOL_LANES = 32 lanes (a half-wave), lane l holding the 16-byte vectors that start at
// column pool_col(j, l) = (j * 32 + l) * 4, j < VPL = ceil(dim / 128) <= 8: the LayerNorm kernels' mapping (layernorm.hip).  The
// pooled tokens of an item, t in [first, tokens), are cut into pool_splits() chunks of POOL_CHUNK = 64 consecutive tokens, one
// workgroup of POOL_HALVES = 8 half-waves each; half-wave h of a chunk that starts at t0 takes the tokens t0 + h, t0 + h + 8, ...
//
// The summation order, fixed by the shape alone (never by the grid or the device): a lane adds its tokens in ascending order; the 8
// half-waves' sums are added in ascending h (pool_sum_ordered); the chunks' sums in ascending chunk (pool_sum_ordered again, from
// the workspace).  An item with one chunk skips the last step, which adds nothing to a single term.
//
// With a LayerNorm the kernels pool xhat = (x - mean) * rstd and apply the affine part once per item: mean_t(xhat_t gamma + beta) =
// mean_t(xhat_t) gamma + beta.  The variance is that of the centred values (mean first, then sum (x - mean)^2), as in layernorm.hip.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define POOL_FN __host__ __device__ __forceinline__
#else
#define POOL_FN inline
#endif

#define POOL_LANES 32       // lanes per token row
#define POOL_HALVES 8       // token rows in flight per workgroup
#define POOL_CHUNK 64       // pooled tokens per workgroup
#define POOL_MAX_VPL 8      // 16-byte vectors per lane: dim <= 32 * 4 * 8 = 1024

POOL_FN int64_t pool_splits(int64_t tokens, int64_t first) { return (tokens - first + POOL_CHUNK - 1) / POOL_CHUNK; }

// the tokens [t0, t1) of chunk `split`
POOL_FN void pool_chunk(int64_t tokens, int64_t first, int64_t split, int64_t& t0, int64_t& t1) {
    t0 = first + split * POOL_CHUNK;
    t1 = t0 + POOL_CHUNK < tokens ? t0 + POOL_CHUNK : tokens;
}

POOL_FN int pool_col(int j, int lane) { return (j * POOL_LANES + lane) * 4; }

// p[0] + p[stride] + ... in ascending order
POOL_FN float pool_sum_ordered(const float* p, int64_t stride, int64_t n) {
    float s = p[0];
    for (int64_t i = 1; i < n; ++i) s += p[i * stride];
    return s;
}

// A lane's piece v[VPL * 4] of a row holds zeros at the columns past dim.
template <int VPL> POOL_FN float pool_sum_part(const float* v) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) s += (v[4 * j] + v[4 * j + 1]) + (v[4 * j + 2] + v[4 * j + 3]);
    return s;
}

template <int VPL> POOL_FN float pool_sq_part(const float* v, float mean, int dim, int lane) {
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        if (pool_col(j, lane) < dim) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[4 * j + e] - mean;
                q = fmaf(d, d, q);
            }
        }
    }
    return q;
}

POOL_FN float pool_rstd(float sq_sum, float inv_d, float eps) {
#if defined(__HIP_DEVICE_COMPILE__)
    return rsqrtf(sq_sum * inv_d + eps);
#else
    return 1.0f / sqrtf(sq_sum * inv_d + eps);
#endif
}

template <int VPL> POOL_FN void pool_acc_plain(float* acc, const float* v) {
#pragma unroll
    for (int i = 0; i < VPL * 4; ++i) acc[i] += v[i];
}

template <int VPL> POOL_FN void pool_acc_norm(float* acc, const float* v, float mean, float rstd, int dim, int lane) {
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        if (pool_col(j, lane) < dim) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[4 * j + e] += (v[4 * j + e] - mean) * rstd;
        }
    }
}

// one pooled element from the sum over its `count` tokens; gamma / beta: that column's, where a LayerNorm was pooled
POOL_FN float pool_finish(float sum, float count) { return sum / count; }
POOL_FN float pool_finish_norm(float sum, float count, float gamma, float beta) { return (sum / count) * gamma + beta; }

// backward of the mean: every pooled token's row gradient
POOL_FN float pool_grad(float g, float count) { return g / count; }

// backward through the LayerNorm of one row given dy (the same for every row of the item) and gg = dy * gamma: xhat, this lane's
// part of sum(gg * xhat), and the running column sums d gamma += dy * xhat, d beta += dy
template <int VPL>
POOL_FN float pool_bwd_parts(const float* dy, const float* gg, const float* x, float mean, float rstd, float* xhat, float* dgamma, float* dbeta,
                             int dim, int lane) {
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const bool in = pool_col(j, lane) < dim;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = 4 * j + e;
            xhat[i] = in ? (x[i] - mean) * rstd : 0.f;
            s2 = fmaf(gg[i], xhat[i], s2);
            dgamma[i] = fmaf(dy[i], xhat[i], dgamma[i]);
            dbeta[i] += dy[i];
        }
    }
    return s2;
}

// dx = rstd * (gg - mean_c(gg) - xhat * mean_c(gg * xhat)); c1, c2 are the two means over the whole row
template <int VPL> POOL_FN void pool_bwd_out(const float* gg, const float* xhat, float c1, float c2, float rstd, float* dx) {
#pragma unroll
    for (int i = 0; i < VPL * 4; ++i) dx[i] = rstd * (gg[i] - c1 - xhat[i] * c2);
}
