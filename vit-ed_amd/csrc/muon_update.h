// Muon (Jordan et al. 2024; torch.optim.Muon's conventions) as the fused update states it: the elementwise bodies of muon.hip - momentum,
// pack (normalise, round to bf16, pad, transpose) and apply - on four consecutive elements of one parameter row, plus the two fp32
// expressions of the Newton-Schulz epilogues.  Plain C++ like optim_update.h, so that the same text runs inside the HIP kernels and in a
// host program under the sanitizers (tools/muon_host_check.cpp).
//
// Group words of a Muon group {lr, momentum, nesterov, eps, weight_decay, adjust, kind = 1, 0}; c the clip coefficient; (a, b, cc) the
// Newton-Schulz coefficients; per tensor [rows, cols]:
//     g'  = fl(g c)                                              a product of its own (lion_product), in both passes that form it
//     buf = fma(g' - buf, 1 - momentum, buf)                     torch.optim.Muon's lerp momentum                        (muon_buf)
//     u   = nesterov ? fma(buf - g', momentum, g') : buf                                                                  (muon_u)
//     X   = bf16(u / max(|u|_F, eps))                            one division, one rounding; |u|_F = sqrt of fp32 sums in a fixed order
//                                                                stored transposed when rows > cols: X is [m, n], m <= n
//     k times:  A = bf16(X X^T);  B = bf16(fl(fl(b A) + fl(cc S))), S = A A in fp32;  X = bf16(fl(fl(a X) + T)), T = B X in fp32
//     O   = X (transposed back when rows > cols)
//     p   = fl(fl(p (1 - lr wd)) - fl(fl(lr adj) O))
//     adj = sqrt(max(1, rows / cols))  (adjust == 0: torch's None / 'original'),  0.2 sqrt(max(rows, cols))  (adjust == 1: 'match_rms_adamw')
// The fp32 expressions of the two epilogues are SEPARATE rounded operations (muon_ns_poly, muon_ns_next), never an fma: every product
// goes through lion_product's value barrier, so a restatement in separate fp32 torch operations (tests/muon_cases.py) gives the same
// bits.  The matrix products themselves take bf16 operands and accumulate in fp32 on the matrix cores; bf16 roundings happen at the three
// stores only.  bf16 values are handled here as their 16 bits (round to nearest even, as the hardware conversion), so the host build
// needs no bf16 type.
#pragma once
#include "optim_update.h"

struct MuonCoef { float lr, momentum, omm, eps, decay, step; int nesterov; };

OPTIM_FN MuonCoef muon_coef(const float* hg, int64_t rows, int64_t cols) {
    MuonCoef k;
    k.lr = hg[0]; k.momentum = hg[1]; k.omm = 1.0f - hg[1]; k.nesterov = hg[2] != 0.f; k.eps = hg[3];
    k.decay = 1.0f - lion_product(k.lr, hg[4]);
    const float adj = hg[5] != 0.f ? 0.2f * sqrtf((float)(rows > cols ? rows : cols))
                                   : sqrtf(rows > cols ? (float)rows / (float)cols : 1.0f);
    k.step = lion_product(k.lr, adj);
    return k;
}

OPTIM_FN uint16_t muon_bf16_bits(float v) {           // round to nearest even; a NaN stays a (quiet) NaN
    uint32_t u;
    memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

OPTIM_FN float muon_bf16_value(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float v;
    memcpy(&v, &u, 4);
    return v;
}

OPTIM_FN float muon_buf(float ge, float buf, const MuonCoef& k) { return fmaf(ge - buf, k.omm, buf); }
OPTIM_FN float muon_u(float ge, float buf, const MuonCoef& k) { return k.nesterov ? fmaf(buf - ge, k.momentum, ge) : buf; }

// The denominator of the normalisation from the tensor's sum of u^2.
OPTIM_FN float muon_denom(float sum_u, const MuonCoef& k) {
    const float n = sqrtf(sum_u);
    return n > k.eps ? n : k.eps;                       // a NaN norm falls to eps; the NaN elements themselves stay NaN
}

// The fp32 expressions of the two Newton-Schulz epilogues (s, t: the fp32 accumulators of A A and B X).
OPTIM_FN float muon_ns_poly(float b, float a_old, float c, float s) { return lion_product(b, a_old) + lion_product(c, s); }
OPTIM_FN float muon_ns_next(float a, float x_old, float t) { return lion_product(a, x_old) + t; }

// Moments pass on elements [o, o + n) of a Muon tensor (n, wide as adamw_piece): the new buf is written, g only read; *su is advanced by
// the piece's u^2, element after element.
OPTIM_FN void muon_moments_piece(const float* g, float* buf, int64_t o, int n, bool wide, const MuonCoef& k, float clip, float* su) {
    float gv[4], bv[4];
    if (wide) {
        const OptimVec4 qg = *(const OptimVec4*)(g + o), qb = *(const OptimVec4*)(buf + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) { gv[e] = qg.v[e]; bv[e] = qb.v[e]; }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = e < n;
            gv[e] = in ? g[o + e] : 0.f; bv[e] = in ? buf[o + e] : 0.f;
        }
    }
    float s = *su;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ge = lion_product(gv[e], clip);
        bv[e] = muon_buf(ge, bv[e], k);
        const float u = e < n ? muon_u(ge, bv[e], k) : 0.f;
        s += u * u;
    }
    *su = s;
    if (wide) *(OptimVec4*)(buf + o) = OptimVec4{{bv[0], bv[1], bv[2], bv[3]}};
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) buf[o + e] = bv[e];
    }
}

// Pack pass: u again from g and the buf the moments pass wrote (through muon_u: the same bits), divided by denom and rounded to bf16.
// x receives four bf16 bit patterns; elements past n are 0, the padding of the image.  Nothing is written here.
OPTIM_FN void muon_pack_piece(const float* g, const float* buf, int64_t o, int n, bool wide, const MuonCoef& k, float clip, float denom,
                              uint16_t* x) {
    float gv[4], bv[4];
    if (wide) {
        const OptimVec4 qg = *(const OptimVec4*)(g + o), qb = *(const OptimVec4*)(buf + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) { gv[e] = qg.v[e]; bv[e] = qb.v[e]; }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = e < n;
            gv[e] = in ? g[o + e] : 0.f; bv[e] = in ? buf[o + e] : 0.f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float u = muon_u(lion_product(gv[e], clip), bv[e], k);
        x[e] = e < n ? muon_bf16_bits(u / denom) : (uint16_t)0;
    }
}

// Apply pass: p = p (1 - lr wd) - lr adj O on elements [o, o + n); ob: the four bf16 bit patterns of O there.  g is only zeroed.
// pn as adamw_piece.
OPTIM_FN void muon_apply_piece(float* p, float* g, const uint16_t* ob, int64_t o, int n, bool wide, const MuonCoef& k, int zero_grad,
                               float* pn) {
    float pv[4];
    if (wide) {
        const OptimVec4 qp = *(const OptimVec4*)(p + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) pv[e] = qp.v[e];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) pv[e] = e < n ? p[o + e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) pn[e] = lion_product(pv[e], k.decay) - lion_product(k.step, muon_bf16_value(ob[e]));
    if (wide) {
        *(OptimVec4*)(p + o) = OptimVec4{{pn[0], pn[1], pn[2], pn[3]}};
        if (zero_grad) *(OptimVec4*)(g + o) = OptimVec4{{0.f, 0.f, 0.f, 0.f}};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) { p[o + e] = pn[e]; if (zero_grad) g[o + e] = 0.f; }
    }
}

// ---- the scratch layout (host and device alike) -------------------------------------------------------------------------------------------
// A Muon tensor [rows, cols] has m = min(rows, cols), n = max(rows, cols), both padded up to the GEMM granule MUON_GRANULE: mp, np.  Its
// region of the bf16 scratch, from `base` (in elements): X0 [mp, np], X1, XT0 [np, mp], XT1, A [mp, mp], B [mp, mp].
#define MUON_GRANULE 64
#define MUON_MAX_SHORT_SIDE 1024
#define MUON_TILE_WORDS 8      // a row of a tile table: {tensor, tile row, tile column, base, mp, np, tall, 0}
#define MUON_TENSOR_WORDS 4    // a row of the tensor table: {base (-1: an aux tensor), mp, np, tall}
#define MUON_META_WORDS 5      // a row of the HOST table the entries check: {rows, cols, ndim, is_muon, group}

OPTIM_FN int64_t muon_pad(int64_t v) { return (v + MUON_GRANULE - 1) / MUON_GRANULE * MUON_GRANULE; }
OPTIM_FN int64_t muon_region_elems(int64_t mp, int64_t np) { return 4 * mp * np + 2 * mp * mp; }

#if defined(__HIPCC__)
// The launches of vited_muon_step that live in optimizer.hip, beside the tile body and the kernels they share with the other entries:
// sum of squares + decision, the moments pass (aux tensors finished as AdamW finishes them) and the apply pass.
void muon_launch_head(const float* grad_flat, int64_t grad_numel, float* hyper, float max_norm, float* norm_out, float* workspace,
                      int ema, hipStream_t s);
void muon_launch_moments(const int64_t* desc, int count, int64_t total_tiles, const float* res, const float* hyper, int zero_grad,
                         float* ema_flat, const float* grad_flat, const int64_t* tensor_tab, float* tile_sums, hipStream_t s);
void muon_launch_apply(const int64_t* desc, int count, int64_t total_tiles, const float* res, const float* hyper, int zero_grad,
                       float* ema_flat, const float* grad_flat, const int64_t* tensor_tab, const uint16_t* scratch, int final_img,
                       hipStream_t s);
bool muon_ema_buffer_ok(const float* ema_flat, int64_t ema_numel, int64_t grad_numel);
#endif
