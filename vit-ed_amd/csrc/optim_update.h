// The per-element update bodies of the fused optimizer kernels (optimizer.hip): torch.optim.AdamW's and torch.optim.SGD's rules and
// LAMB's and Lion's on four consecutive elements of one parameter row, and the decision whether an update is applied at all.  Plain C++
// (one call = one 4-element piece, the unit a thread of the update kernel handles), so that the same text runs inside the HIP kernels
// and in a host program under the sanitizers (tools/optim_host_check.cpp, tools/ema_host_check.cpp, tools/lamb_host_check.cpp,
// tools/lion_host_check.cpp).  The exponential moving average of the
// parameters (the *_ema entries, vited_ema_swap) is stated here as well: ema_decay_at / ema_blend are THE rule.
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

// ---- LAMB (You et al. 2020, Algorithm 2, with timm's Lamb conventions) ----------------------------------------------------------------
// Group words {lr, b1, b2, eps, wd, always_adapt, trust_clip, -}; c the clip coefficient, t the count of applied updates:
//     g' = g c;  m = m + (g' - m) (1 - b1);  v = b2 v + (1 - b2) g' g'                       (the moments as adamw_piece forms them)
//     u  = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd p                        (lamb_u: THE statement of u)
//     r  = (wd == 0 and not always_adapt) ? 1 : ((|p| > 0 and |u| > 0) ? |p| / |u| : 1),  with trust_clip min(r, 1)      (lamb_ratio)
//     p  = p - lr r u
// |.| is the 2-norm over the whole tensor.  Three passes (optimizer.hip): lamb_moments_piece writes m, v and returns the piece's sums
// of p^2 and u^2; lamb_ratio turns a tensor's sums into r; lamb_apply_piece forms u again from the m, v it reads and the old p -
// through lamb_u, whose two multiply-adds are fmaf by name, so that both passes get the same bits whatever the compiler may contract.
struct LambCoef { float lr, b1, b2, eps, wd, bc1, inv_sqrt_bc2; int adapt, trust_clip; };

OPTIM_FN LambCoef lamb_coef(const float* hg, float step) {
    LambCoef k;
    k.lr = hg[0]; k.b1 = hg[1]; k.b2 = hg[2]; k.eps = hg[3]; k.wd = hg[4];
    k.adapt = hg[4] != 0.f || hg[5] != 0.f; k.trust_clip = hg[6] != 0.f;
    // the bias corrections in fp64, once per workgroup: in fp32, 1 - b2^t cancels (b2 = 0.999, t = 2: 2^-24 of 0.998 is 1.5e-5 of
    // 0.002), which every element of u and with them the trust ratio would inherit as one common error
    k.bc1 = (float)(1.0 - pow((double)k.b1, (double)step));
    k.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)k.b2, (double)step)));
    return k;
}

OPTIM_FN float lamb_u(float m, float v, float p, const LambCoef& k) {
    const float denom = fmaf(sqrtf(v), k.inv_sqrt_bc2, k.eps);
    return fmaf(k.wd, p, (m / k.bc1) / denom);
}

// sum_p, sum_u: the tensor's sums of p^2 and u^2.
OPTIM_FN float lamb_ratio(float sum_p, float sum_u, const LambCoef& k) {
    if (!k.adapt) return 1.0f;
    const float pn = sqrtf(sum_p), un = sqrtf(sum_u);
    float r = (pn > 0.f && un > 0.f) ? pn / un : 1.0f;
    if (k.trust_clip) r = r < 1.0f ? r : 1.0f;
    return r;
}

// Pass 1 on elements [o, o + n) (n, wide as adamw_piece): new m and v are written, p and g only read; *sp and *su are advanced by the
// piece's p^2 and u^2, element after element.
OPTIM_FN void lamb_moments_piece(const float* p, const float* g, float* m, float* v, int64_t o, int n, bool wide, const LambCoef& k,
                                 float clip, float* sp, float* su) {
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
    float s_p = *sp, s_u = *su;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ge = gv[e] * clip;
        mv[e] = mv[e] + (ge - mv[e]) * (1.0f - k.b1);
        vv[e] = vv[e] * k.b2 + (1.0f - k.b2) * ge * ge;
        const float u = e < n ? lamb_u(mv[e], vv[e], pv[e], k) : 0.f;
        s_p += pv[e] * pv[e];
        s_u += u * u;
    }
    *sp = s_p; *su = s_u;
    if (wide) {
        *(OptimVec4*)(m + o) = OptimVec4{{mv[0], mv[1], mv[2], mv[3]}};
        *(OptimVec4*)(v + o) = OptimVec4{{vv[0], vv[1], vv[2], vv[3]}};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) { m[o + e] = mv[e]; v[o + e] = vv[e]; }
    }
}

// Pass 3: p = p - step_size u with step_size = lr r, u from the moments pass 1 wrote and the p it read; m and v are only read, g is
// only zeroed.  pn as adamw_piece.
OPTIM_FN void lamb_apply_piece(float* p, float* g, const float* m, const float* v, int64_t o, int n, bool wide, const LambCoef& k,
                               float step_size, int zero_grad, float* pn) {
    float pv[4], mv[4], vv[4];
    if (wide) {
        const OptimVec4 qp = *(const OptimVec4*)(p + o), qm = *(const OptimVec4*)(m + o), qv = *(const OptimVec4*)(v + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) { pv[e] = qp.v[e]; mv[e] = qm.v[e]; vv[e] = qv.v[e]; }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = e < n;
            pv[e] = in ? p[o + e] : 0.f; mv[e] = in ? m[o + e] : 0.f; vv[e] = in ? v[o + e] : 0.f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) pn[e] = pv[e] - step_size * lamb_u(mv[e], vv[e], pv[e], k);
    if (wide) {
        *(OptimVec4*)(p + o) = OptimVec4{{pn[0], pn[1], pn[2], pn[3]}};
        if (zero_grad) *(OptimVec4*)(g + o) = OptimVec4{{0.f, 0.f, 0.f, 0.f}};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) { p[o + e] = pn[e]; if (zero_grad) g[o + e] = 0.f; }
    }
}

// ---- Lion (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms", with timm's Lion conventions) ----------------------------
// Group words {lr, b1, b2, -, wd, -, -, -}; c the clip coefficient.  One moment, no step count, no bias correction:
//     g' = g c
//     pe = p (1 - lr wd)                       decoupled decay (timm: p.mul_(1 - lr * wd))
//     cc = b1 m + (1 - b1) g'                  (timm: exp_avg.mul(b1).add_(grad, alpha=1 - b1))
//     s  = sign(cc)                            +1, -1, 0 for cc == 0, NaN for NaN
//     p' = pe - lr s
//     m' = m + (g' - m)(1 - b2)                (timm: exp_avg.lerp_(grad, 1 - b2))
// Every product - g c, lr wd, p (1 - lr wd), b1 m, (1 - b1) g', (g' - m)(1 - b2) - is rounded on its own (lion_product), never
// contracted into an fma with the sum or difference that follows: sign(cc) is decided by rounding exactly where the two terms nearly
// cancel, and with the rule pinned the kernel, the host build and an fp32 restatement in separate torch ops give the same bits.
struct LionCoef { float lr, b1, b2, omb1, omb2, decay; };

OPTIM_FN float lion_product(float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float r = OPTIM_MUL_RN(a, b);
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(r));                          // the value barrier of ema_blend: the product is a value of its own
#endif
    return r;
}

OPTIM_FN LionCoef lion_coef(const float* hg) {
    LionCoef k;
    k.lr = hg[0]; k.b1 = hg[1]; k.b2 = hg[2];
    k.omb1 = 1.0f - k.b1; k.omb2 = 1.0f - k.b2;
    k.decay = 1.0f - lion_product(k.lr, hg[4]);
    return k;
}

OPTIM_FN float lion_sign(float c) {
    return c > 0.f ? 1.0f : (c < 0.f ? -1.0f : (c == 0.f ? 0.f : c));
}

// n, wide, pn as adamw_piece.
OPTIM_FN void lion_piece(float* p, float* g, float* m, int64_t o, int n, bool wide, const LionCoef& k, float clip, int zero_grad,
                         float* pn) {
    float gv[4], pv[4], mv[4];
    if (wide) {
        const OptimVec4 qg = *(const OptimVec4*)(g + o), qp = *(const OptimVec4*)(p + o), qm = *(const OptimVec4*)(m + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) { gv[e] = qg.v[e]; pv[e] = qp.v[e]; mv[e] = qm.v[e]; }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = e < n;
            gv[e] = in ? g[o + e] : 0.f; pv[e] = in ? p[o + e] : 0.f; mv[e] = in ? m[o + e] : 0.f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ge = lion_product(gv[e], clip);
        const float pe = lion_product(pv[e], k.decay);
        const float cc = lion_product(k.b1, mv[e]) + lion_product(k.omb1, ge);
        pn[e] = pe - k.lr * lion_sign(cc);      // lr s is exact (+lr, -lr, 0): an fma here changes no bit
        mv[e] = mv[e] + lion_product(ge - mv[e], k.omb2);
    }
    if (wide) {
        *(OptimVec4*)(p + o) = OptimVec4{{pn[0], pn[1], pn[2], pn[3]}};
        *(OptimVec4*)(m + o) = OptimVec4{{mv[0], mv[1], mv[2], mv[3]}};
        if (zero_grad) *(OptimVec4*)(g + o) = OptimVec4{{0.f, 0.f, 0.f, 0.f}};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) { p[o + e] = pn[e]; m[o + e] = mv[e]; if (zero_grad) g[o + e] = 0.f; }
    }
}

// A skipped update: only the gradient is touched.
OPTIM_FN void skipped_piece(float* g, int64_t o, int n, bool wide, int zero_grad) {
    if (!zero_grad) return;
    if (wide) *(OptimVec4*)(g + o) = OptimVec4{{0.f, 0.f, 0.f, 0.f}};
    else
        for (int e = 0; e < n; ++e) g[o + e] = 0.f;
}

// ---- exponential moving average of the parameters (timm's ModelEmaV2 / --model-ema) --------------------------------------------------
// hyper[3] = d (the decay), hyper[4] = warmup flag, hyper[5] = n, the EMA updates done so far.  After an applied update produced p':
//     d_t = warmup ? min(d, (1 + n) / (10 + n)) : d            all fp32, n as fp32
//     e'  = fl( fl(d_t * e) + fl((1.0f - d_t) * p') )           both products rounded on their own: never an fma
// and n advances by one.  A skipped update leaves e and n alone.
#define OPTIM_EMA_DECAY 3
#define OPTIM_EMA_WARMUP 4
#define OPTIM_EMA_COUNT 5

OPTIM_FN float ema_decay_at(float d, float warmup, float n) {
    if (warmup != 0.f) {
        const float w = (1.0f + n) / (10.0f + n);
        d = w < d ? w : d;
    }
    return d;
}

OPTIM_FN float ema_blend(float dt, float e, float p) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float keep = OPTIM_MUL_RN(dt, e);
    float take = OPTIM_MUL_RN(1.0f - dt, p);
#if defined(__HIP_DEVICE_COMPILE__)
    // -ffp-contract=fast lets the backend fuse a product into the sum whatever the source says (pragma and __fmul_rn included): an
    // empty statement that "produces" both products makes them values of their own.  No instruction is emitted for it.
    asm("" : "+v"(keep), "+v"(take));
#endif
    return keep + take;
}

// Beside optim_decide, by the same one thread: an applied update is one EMA update.
OPTIM_FN void ema_decide(bool applied, float* hyper) {
    if (applied) hyper[OPTIM_EMA_COUNT] += 1.0f;
}

// The decay of the update whose decision ema_decide just recorded (every workgroup of the update kernel derives it alike).
OPTIM_FN float ema_decay_now(const float* hyper) {
    return ema_decay_at(hyper[OPTIM_EMA_DECAY], hyper[OPTIM_EMA_WARMUP], hyper[OPTIM_EMA_COUNT] - 1.0f);
}

// Elements [o, o + n) of the average, from the new parameter values pn the update piece just produced (same n / wide as there).
OPTIM_FN void ema_piece(float* ema, int64_t o, int n, bool wide, float dt, const float* pn) {
    if (wide) {
        const OptimVec4 qe = *(const OptimVec4*)(ema + o);
        *(OptimVec4*)(ema + o) = OptimVec4{{ema_blend(dt, qe.v[0], pn[0]), ema_blend(dt, qe.v[1], pn[1]), ema_blend(dt, qe.v[2], pn[2]),
                                            ema_blend(dt, qe.v[3], pn[3])}};
    } else {
        for (int e = 0; e < n; ++e) ema[o + e] = ema_blend(dt, ema[o + e], pn[e]);
    }
}

// vited_ema_swap: p <-> its slice of the average, element for element; pn receives what p now holds (for the bf16 shadows).
OPTIM_FN void swap_piece(float* p, float* ema, int64_t o, int n, bool wide, float* pn) {
    if (wide) {
        const OptimVec4 qp = *(const OptimVec4*)(p + o), qe = *(const OptimVec4*)(ema + o);
        *(OptimVec4*)(p + o) = qe;
        *(OptimVec4*)(ema + o) = qp;
#pragma unroll
        for (int e = 0; e < 4; ++e) pn[e] = qe.v[e];
    } else {
        for (int e = 0; e < n; ++e) {
            const float pv = p[o + e], ev = ema[o + e];
            p[o + e] = ev; ema[o + e] = pv; pn[e] = ev;
        }
    }
}
