// The per-head-row arithmetic of the q/k-norm kernels (qk_norm.hip): LayerNorm over the head_dim elements of one head's query
// or key row, forward and backward, written for ONE LANE's piece of the row.  A head row is spread over QKN_LANES = 8 lanes,
// each holding E = head_dim / 8 consecutive elements (4 at head_dim 32, 8 at head_dim 64); the three row sums (the mean, the
// centred sum of squares, the backward's two means) are formed between the phases below by the caller - DPP adds inside the
// 8-lane group on the device, the same xor-1 / xor-2 / xor-4 butterfly over an array of lanes in the host program under the
// sanitizers (tools/qknorm_host_check.cpp).  Plain C++, so the same text runs in both places.
//
// The variance is that of the centred values, in the order csrc/layernorm.hip uses (mean first, then sum (x - mean)^2): never
// E[x^2] - E[x]^2.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define QKN_FN __host__ __device__ __forceinline__
#else
#define QKN_FN inline
#endif

#define QKN_LANES 8      // lanes per head row

// phase 1: this lane's part of sum(x)
template <int E> QKN_FN float qkn_sum_part(const float* x) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; e += 4) s += (x[e] + x[e + 1]) + (x[e + 2] + x[e + 3]);
    return s;
}

// phase 2: this lane's part of sum((x - mean)^2)
template <int E> QKN_FN float qkn_sq_part(const float* x, float mean) {
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const float d = x[e] - mean;
        q = fmaf(d, d, q);
    }
    return q;
}

QKN_FN float qkn_rstd(float sq_sum, float inv_d, float eps) {
#if defined(__HIP_DEVICE_COMPILE__)
    return rsqrtf(sq_sum * inv_d + eps);
#else
    return 1.0f / sqrtf(sq_sum * inv_d + eps);
#endif
}

// phase 3: y = (x - mean) * rstd * gamma + beta
template <int E> QKN_FN void qkn_fwd_out(const float* x, float mean, float rstd, const float* gamma, const float* beta, float* y) {
#pragma unroll
    for (int e = 0; e < E; ++e) y[e] = (x[e] - mean) * rstd * gamma[e] + beta[e];
}

// backward phase 1: xhat and g = dy * gamma of this lane's elements, its parts of sum(g) and sum(g * xhat), and the running
// column sums d gamma += dy * xhat, d beta += dy (a lane owns the same head_dim columns of every head row it sees)
template <int E>
QKN_FN void qkn_bwd_parts(const float* dy, const float* x, float mean, float rstd, const float* gamma, float* xhat, float* g, float& s1,
                          float& s2, float* dgamma, float* dbeta) {
    s1 = 0.f;
    s2 = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        xhat[e] = (x[e] - mean) * rstd;
        g[e] = dy[e] * gamma[e];
        s1 += g[e];
        s2 = fmaf(g[e], xhat[e], s2);
        dgamma[e] = fmaf(dy[e], xhat[e], dgamma[e]);
        dbeta[e] += dy[e];
    }
}

// backward phase 2: dx = rstd * (g - mean_d(g) - xhat * mean_d(g * xhat)); c1, c2 are the two means over the whole head row
template <int E> QKN_FN void qkn_bwd_out(const float* g, const float* xhat, float c1, float c2, float rstd, float* dx) {
#pragma unroll
    for (int e = 0; e < E; ++e) dx[e] = rstd * (g[e] - c1 - xhat[e] * c2);
}
