// The per-element update bodies of the fused optimizer kernels (optimizer.hip): torch.optim.AdamW's and torch.optim.SGD's rules
// on four consecutive elements of one parameter row, and the decision whether an update is applied at all.  Plain C++ (one call =
// one 4-element piece, the unit a thread of the update kernel handles), so that the same text runs inside the HIP kernels and in a
// host program under the sanitizers (tools/optim_host_check.cpp).
#pragma once
#include <stdint.h>
#include <string.h>
#include <math.h>

#if defined(__HIPCC__)
#define OPTIM_FN __host__ __device__ __forceinline__
#else
#define OPTIM_FN inline
#endif

// A product that is rounded on its own, never contracted into an fma with a following sum (torch.optim.SGD forms g * clip and
// momentum * buf in kernels of their own, so their roundings are part of its result).
#if defined(__HIP_DEVICE_COMPILE__)
#define OPTIM_MUL_RN(a, b) __fmul_rn((a), (b))
#else
#define OPTIM_MUL_RN(a, b) ((a) * (b))
#endif

struct alignas(16) OptimVec4 { float v[4]; };

// What one parameter group contributes to a piece, derived once per workgroup from the group's 8 hyper words.
struct AdamWCoef { float b1, b2, eps, step_size, inv_sqrt_bc2, decay; };
struct SgdCoef { float lr, momentum, wd; int nesterov; };

OPTIM_FN AdamWCoef adamw_coef(const float* hg, float step) {
    const float lr = hg[0], b1 = hg[1], b2 = hg[2], eps = hg[3], wd = hg[4];
    const float bc1 = 1.0f - powf(b1, step), bc2 = 1.0f - powf(b2, step);
    AdamWCoef k;
    k.b1 = b1; k.b2 = b2; k.eps = eps;
    k.step_size = lr / bc1; k.inv_sqrt_bc2 = 1.0f / sqrtf(bc2); k.decay = 1.0f - lr * wd;
    return k;
}

OPTIM_FN SgdCoef sgd_coef(const float* hg) {
    SgdCoef k;
    k.lr = hg[0]; k.momentum = hg[1]; k.nesterov = hg[2] != 0.f; k.wd = hg[4];
    return k;
}

// A norm that is inf or NaN (exponent bits all ones); written on the bits so that no floating-point option can fold it away.
OPTIM_FN bool optim_nonfinite(float norm) {
    uint32_t u;
    memcpy(&u, &norm, 4);
    return (u & 0x7f800000u) == 0x7f800000u;
}

OPTIM_FN float optim_clip_coef(float norm, float max_norm) {
    float clip = 1.0f;
    if (max_norm > 0.f) {
        clip = max_norm / (norm + 1e-6f);
        clip = clip < 1.0f ? clip : 1.0f;
    }
    return clip;
}

// The decision of one update, taken once (by one thread) after the norm is known: advances hyper[0] (updates applied) or hyper[2]
// (updates skipped) and leaves {norm, clip, applied, step count} in res for every workgroup of the update kernel.
OPTIM_FN void optim_decide(float norm, float max_norm, float* hyper, float* res) {
    const bool applied = !(hyper[1] != 0.f && optim_nonfinite(norm));
    if (applied) hyper[0] += 1.0f;
    else hyper[2] += 1.0f;
    res[0] = norm;
    res[1] = optim_clip_coef(norm, max_norm);
    res[2] = applied ? 1.0f : 0.f;
    res[3] = hyper[0];
}

// Elements [o, o + n) of one row, n = 1..4 (n < 4: the row's tail; `wide`: n == 4 and every pointer is 16-byte aligned there).
// pn receives the new parameter values (the caller casts them into the bf16 shadows); elements past n stay as the caller set them.
OPTIM_FN void adamw_piece(float* p, float* g, float* m, float* v, int64_t o, int n, bool wide, const AdamWCoef& k, float clip,
                          int zero_grad, float* pn) {
    float gv[4], pv[4], mv[4], vv[4];
    if (wide) {
        const OptimVec4 qg = *(const OptimVec4*)(g + o), qp = *(const OptimVec4*)(p + o), qm = *(const OptimVec4*)(m + o),
                        qv = *(const OptimVec4*)(v + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) { gv[e] = qg.v[e]; pv[e] = qp.v[e]; mv[e] = qm.v[e]; vv[e] = qv.v[e]; }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = e < n;
            gv[e] = in ? g[o + e] : 0.f; pv[e] = in ? p[o + e] : 0.f; mv[e] = in ? m[o + e] : 0.f; vv[e] = in ? v[o + e] : 0.f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ge = gv[e] * clip;
        const float pe = pv[e] * k.decay;
        mv[e] = mv[e] + (ge - mv[e]) * (1.0f - k.b1);
        vv[e] = vv[e] * k.b2 + (1.0f - k.b2) * ge * ge;
        const float denom = sqrtf(vv[e]) * k.inv_sqrt_bc2 + k.eps;
        pn[e] = pe - k.step_size * (mv[e] / denom);
    }
    if (wide) {
        *(OptimVec4*)(p + o) = OptimVec4{{pn[0], pn[1], pn[2], pn[3]}};
        *(OptimVec4*)(m + o) = OptimVec4{{mv[0], mv[1], mv[2], mv[3]}};
        *(OptimVec4*)(v + o) = OptimVec4{{vv[0], vv[1], vv[2], vv[3]}};
        if (zero_grad) *(OptimVec4*)(g + o) = OptimVec4{{0.f, 0.f, 0.f, 0.f}};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) { p[o + e] = pn[e]; m[o + e] = mv[e]; v[o + e] = vv[e]; if (zero_grad) g[o + e] = 0.f; }
    }
}

// torch.optim.SGD (dampening 0) after the clip:  g' = g clip + wd p;  buf = momentum buf + g';  d = nesterov ? g' + momentum buf : buf;
// p -= lr d.  A zero buffer makes the first update torch's (buf = g').  With momentum == 0 buf is neither read nor written (it may be
// null).
OPTIM_FN void sgd_piece(float* p, float* g, float* buf, int64_t o, int n, bool wide, const SgdCoef& k, float clip, int zero_grad,
                        float* pn) {
    const bool mom = k.momentum != 0.f;
    float gv[4], pv[4], bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (wide) {
        const OptimVec4 qg = *(const OptimVec4*)(g + o), qp = *(const OptimVec4*)(p + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) { gv[e] = qg.v[e]; pv[e] = qp.v[e]; }
        if (mom) {
            const OptimVec4 qb = *(const OptimVec4*)(buf + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[e] = qb.v[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = e < n;
            gv[e] = in ? g[o + e] : 0.f; pv[e] = in ? p[o + e] : 0.f;
            if (mom) bv[e] = in ? buf[o + e] : 0.f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float gc = OPTIM_MUL_RN(gv[e], clip);
        const float ge = gc + k.wd * pv[e];
        float d = ge;
        if (mom) {
            const float scaled = OPTIM_MUL_RN(k.momentum, bv[e]);
            bv[e] = scaled + ge;
            d = k.nesterov ? ge + k.momentum * bv[e] : bv[e];
        }
        pn[e] = pv[e] - k.lr * d;
    }
    if (wide) {
        *(OptimVec4*)(p + o) = OptimVec4{{pn[0], pn[1], pn[2], pn[3]}};
        if (mom) *(OptimVec4*)(buf + o) = OptimVec4{{bv[0], bv[1], bv[2], bv[3]}};
        if (zero_grad) *(OptimVec4*)(g + o) = OptimVec4{{0.f, 0.f, 0.f, 0.f}};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) { p[o + e] = pn[e]; if (mom) buf[o + e] = bv[e]; if (zero_grad) g[o + e] = 0.f; }
    }
}

// A skipped update: only the gradient is touched.
OPTIM_FN void skipped_piece(float* g, int64_t o, int n, bool wide, int zero_grad) {
    if (!zero_grad) return;
    if (wide) *(OptimVec4*)(g + o) = OptimVec4{{0.f, 0.f, 0.f, 0.f}};
    else
        for (int e = 0; e < n; ++e) g[o + e] = 0.f;
}
