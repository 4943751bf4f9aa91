// Fused gradient clip + optimizer update + bf16 weight-shadow refresh + gradient zeroing on the flat gradient buffer, for AdamW
// (vited_adamw_step) and Nesterov / momentum SGD (vited_sgd_step)
// (replaces clip_grad_norm_ + torch.optim.AdamW.step / SGD.step + vited_cast_weights + zero_grad:
// misc/utils.py:215-223, misc/optimizer.py:22-46, misc/engine.py:231).
//
//   launch 1  optim_sumsq_kernel : partial[b] = sum of squares of a slice of the flat gradient (fixed slices and a
//                                  fixed reduction order: deterministic).
//   launch 2  optim_decide_kernel: ONE workgroup reduces the partials (thread x adds partials x, x + 256, x + 512, x + 768, then
//                                  the block sum), takes the norm and the clip coefficient, decides whether the update is
//                                  applied (hyper[1] set and a non-finite norm: skipped), advances hyper[0] or hyper[2] and leaves
//                                  {norm, clip, applied, step count} behind the partials.  Both counters are written here and
//                                  read by the NEXT launch only, never by another workgroup of the same one.
//   launch 3  optim_update_kernel: one workgroup per 64 x 64 tile of one parameter (device descriptor table, as
//                                  vited_cast_weights).  Per element (optim_update.h)
//                                      g' = g * min(1, max_norm / (norm + 1e-6))
//                                    AdamW
//                                      p  = p * (1 - lr * wd);  m = lerp(m, g', 1 - b1);  v = b2 * v + (1 - b2) * g'^2
//                                      p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
//                                    SGD
//                                      g' += wd * p;  buf = momentum * buf + g';  p -= lr * (nesterov ? g' + momentum * buf : buf)
//                                  (torch.optim.AdamW's / SGD's update), the new p is also written to its bf16 [rows, cols] shadow
//                                  and, through an LDS tile, to the transposed bf16 [cols, rows] shadow, and g is zeroed.  A skipped
//                                  update zeroes g and touches nothing else.
// HBM traffic per element: AdamW 16 B read (g, p, m, v) + 16 B written + 4 B of shadows, SGD 12 B read (g, p, buf) + 12 B written
// + 4 B of shadows (8 + 8 + 4 without momentum) = the floor for these updates.
// All hyper-parameters that change between steps (learning rate per group, step count) live in a device array, so a
// hipGraph replay of the launches follows the scheduler.
//
// vited_adamw_step_ema / vited_sgd_step_ema: the same three launches with the exponential moving average of the parameters kept in
// the third one (optim_update_ema_kernel, the EMA instance of the same tile body: + 4 B read and 4 B written per element, on the
// fresh p it holds in registers); launch 2 advances the EMA counter hyper[5] beside hyper[0].  vited_ema_swap: the OPT_SWAP instance
// of that body, p <-> e and both shadows rewritten from the value now in p.  The entries without _ema launch optim_update_kernel,
// which instantiates the body without any of it.
//
// vited_lamb_step / vited_lamb_step_ema: LAMB, whose trust ratio needs the norms of a whole tensor before any of its elements may
// move - launches 1 and 2, then three more (at the end of this file), the last one the OPT_LAMB instance of the same tile body.
//
// vited_lion_step / vited_lion_step_ema: Lion (lion_piece), the OPT_LION instance of the tile body behind the same launches 1 and 2.
// One moment (descriptor word 2; word 3 is 0, as for SGD):  pe = p (1 - lr wd);  p' = pe - lr sign(b1 m + (1 - b1) g');
// m' = m + (g' - m)(1 - b2), every product rounded on its own.  12 B read (g, p, m) + 12 B written + 4 B of shadows per element.
//
// vited_muon_step / vited_muon_step_ema (muon.hip) launch two kernels of this file, at its end: the moments pass, whose aux tiles are the
// OPT_ADAMW instance of the tile body, and the apply pass, its OPT_MUON instance.
#include "common.h"
#include "optim_update.h"
#include "muon_update.h"

#define AD_DESC_WORDS 10   // {p, g, m, v, shadow, shadow_t, rows, cols, first_tile, group}
#define AD_HYPER_HEADER 8  // hyper[0] = updates applied (float), [1] = skip-non-finite flag, [2] = updates skipped, [3..5] = EMA decay, warmup flag, EMA updates (the *_ema entries only), [6..7] reserved; then 8 floats per group
#define AD_GROUP_WORDS 8   // AdamW {lr, beta1, beta2, eps, weight_decay, -, -, -}; SGD {lr, momentum, nesterov, -, weight_decay, -, -, -}; Lion {lr, beta1, beta2, -, weight_decay, -, -, -}
#define AD_PARTIALS 1024
#define AD_RESULT_WORDS 4  // behind the partials: {norm, clip, applied, step count}
enum { OPT_ADAMW = 0, OPT_SGD = 1, OPT_SWAP = 2, OPT_LAMB = 3, OPT_LION = 4, OPT_MUON = 5 };

// What the OPT_MUON instance of the tile body needs beside the family's arguments (muon.hip): the tensor table, the bf16 scratch and
// which of the two X images holds the result of the last Newton-Schulz step.
struct MuonApplyArgs { const int64_t* tensor_tab; const uint16_t* scratch; int final_img; };

__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    const float total = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return total;
}

__global__ void __launch_bounds__(256)
optim_sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ partials) {
    __shared__ float red[4];
    // fixed contiguous slice per block, so the sum does not depend on the launch
    const int64_t per = ((n + AD_PARTIALS - 1) / AD_PARTIALS + 3) & ~(int64_t)3;
    const int64_t lo = (int64_t)blockIdx.x * per;
    int64_t hi = lo + per;
    hi = hi < n ? hi : n;
    float s = 0.f;
    const bool al = ((uintptr_t)g & 15) == 0;
    if (al) {
        for (int64_t i = lo + (int64_t)threadIdx.x * 4; i < hi; i += 1024) {
            if (i + 3 < hi) {
                const f32x4 q = *(const f32x4*)(g + i);
                s += q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
            } else {
                for (int64_t j = i; j < hi; ++j) s += g[j] * g[j];
            }
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256) s += g[i] * g[i];
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256)
optim_decide_kernel(float* __restrict__ ws, float* __restrict__ hyper, float max_norm, float* __restrict__ norm_out, int ema) {
    __shared__ float red[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < AD_PARTIALS / 256; ++i) s += ws[threadIdx.x + 256 * i];
    const float norm = sqrtf(block_sum_256(s, red));
    if (threadIdx.x == 0) {
        optim_decide(norm, max_norm, hyper, ws + AD_PARTIALS);
        if (ema) ema_decide(ws[AD_PARTIALS + 2] != 0.f, hyper);    // the *_ema entries only: the others never touch hyper[3..5]
        if (norm_out) *norm_out = norm;
    }
}

// One 64 x 64 tile of one parameter.  OPT_ADAMW / OPT_SGD: the update; EMA adds e' = ema_blend(d_t, e, p') on the row's slice of
// ema_flat (at the offset of its g in grad_flat).  OPT_SWAP: p <-> e and the shadows rewritten from the value now in p (vited_ema_swap;
// res, hyper and zero_grad unused).  OPT_LAMB: LAMB's third launch (below), p -= lr r u with r = ratio[row], m and v only read.
// OPT_LION: Lion's update; m is its one moment, v unused (0).  OPT_MUON: Muon's apply pass on the Muon tensors of the table (an aux
// tensor was finished by the moments pass: its workgroups return at once), p = p (1 - lr wd) - lr adj O with O read from the scratch.
template <int OPT, bool EMA>
__device__ __forceinline__ void
optim_update_tile(const int64_t* __restrict__ desc, int count, const float* __restrict__ res, const float* __restrict__ hyper,
                  int zero_grad, float* __restrict__ ema_flat, const float* grad_flat, const float* __restrict__ ratio = nullptr,
                  MuonApplyArgs mu = MuonApplyArgs{}) {
    __shared__ bf16 tile[64][66];
    float clip = 1.0f, step = 0.f;
    bool applied = true;
    if constexpr (OPT != OPT_SWAP) {
        clip = res[1]; step = res[3];
        applied = res[2] != 0.f;                // the same word in every workgroup
    }
    if (!applied && !zero_grad) return;

    const int64_t blk = blockIdx.x;
    int lo = 0, hi = count - 1;     // last descriptor whose first_tile <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(int64_t)mid * AD_DESC_WORDS + 8] <= blk) lo = mid; else hi = mid - 1;
    }
    const int64_t* d = desc + (int64_t)lo * AD_DESC_WORDS;
    float* p = (float*)d[0];
    float* g = (float*)d[1];
    float* m = (float*)d[2];                    // SGD: the momentum buffer; Lion: exp_avg
    float* v = (float*)d[3];                    // SGD, Lion: unused (0)
    bf16* __restrict__ dst = (bf16*)d[4];
    bf16* __restrict__ dst_t = (bf16*)d[5];
    const int64_t rows = d[6], cols = d[7];
    MuonCoef km = {};
    const uint16_t* o_img = nullptr;            // Muon: the image of O in the orientation of p, leading dimension o_ld
    int64_t o_ld = 0;
    if constexpr (OPT == OPT_MUON) {
        const int64_t* tt = mu.tensor_tab + (int64_t)lo * MUON_TENSOR_WORDS;
        if (tt[0] < 0) return;                  // an aux tensor: the same decision in every thread of the workgroup
        // wide: O is X [mp, np] itself; tall: X is O transposed, so O is the XT image [np, mp] - either way [pad(rows), pad(cols)]
        o_img = mu.scratch + tt[0] + ((tt[3] ? 2 : 0) + mu.final_img) * tt[1] * tt[2];
        o_ld = muon_pad(cols);
    }
    AdamWCoef ka = {};
    SgdCoef ks = {};
    LambCoef kl = {};
    LionCoef kn = {};
    float lamb_step = 0.f;                      // LAMB: lr * r of this row
    if constexpr (OPT != OPT_SWAP) {
        const float* hg = hyper + AD_HYPER_HEADER + d[9] * AD_GROUP_WORDS;
        if constexpr (OPT == OPT_ADAMW) ka = adamw_coef(hg, step);
        else if constexpr (OPT == OPT_LAMB) {
            if (applied) { kl = lamb_coef(hg, step); lamb_step = kl.lr * ratio[lo]; }
        } else if constexpr (OPT == OPT_LION) kn = lion_coef(hg);
        else if constexpr (OPT == OPT_MUON) km = muon_coef(hg, rows, cols);
        else ks = sgd_coef(hg);
    }
    float* e = nullptr;                         // the row's slice of the average
    float dt = 0.f;
    if constexpr (EMA) e = ema_flat + (g - grad_flat);
    if constexpr (EMA && OPT != OPT_SWAP) dt = applied ? ema_decay_now(hyper) : 0.f;

    const int64_t t = blk - d[8], tiles_c = (cols + 63) >> 6;
    const int64_t r0 = (t / tiles_c) << 6, c0 = (t % tiles_c) << 6;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;   // 16 x 16: 4 columns x 4 rows per thread
    uintptr_t ptrs = (uintptr_t)p | (uintptr_t)g;
    if constexpr (OPT == OPT_ADAMW || OPT == OPT_LAMB) ptrs |= (uintptr_t)m | (uintptr_t)v;
    else if constexpr (OPT == OPT_LION) ptrs |= (uintptr_t)m;
    else if (OPT == OPT_SGD && ks.momentum != 0.f) ptrs |= (uintptr_t)m;
    if constexpr (EMA) ptrs |= (uintptr_t)e;
    const bool vec = (cols & 3) == 0 && (ptrs & 15) == 0;
    if (!applied) {                             // skipped update: zero the gradient tile, leave p, the state and the shadows alone
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t r = r0 + ty + 16 * j, c = c0 + tx * 4;
            if (r < rows && c < cols) {
                const int n = cols - c < 4 ? (int)(cols - c) : 4;
                skipped_piece(g, r * cols + c, n, vec && n == 4, zero_grad);
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int lr_ = ty + 16 * j;
        const int64_t r = r0 + lr_, c = c0 + tx * 4;
        float pn[4] = {0.f, 0.f, 0.f, 0.f};
        if (r < rows && c < cols) {
            const int n = cols - c < 4 ? (int)(cols - c) : 4;
            if constexpr (OPT == OPT_ADAMW) adamw_piece(p, g, m, v, r * cols + c, n, vec && n == 4, ka, clip, zero_grad, pn);
            else if constexpr (OPT == OPT_SGD) sgd_piece(p, g, m, r * cols + c, n, vec && n == 4, ks, clip, zero_grad, pn);
            else if constexpr (OPT == OPT_LION) lion_piece(p, g, m, r * cols + c, n, vec && n == 4, kn, clip, zero_grad, pn);
            else if constexpr (OPT == OPT_LAMB) lamb_apply_piece(p, g, m, v, r * cols + c, n, vec && n == 4, kl, lamb_step, zero_grad, pn);
            else if constexpr (OPT == OPT_MUON) {
                // four padded columns of one padded row: 8-byte aligned (o_ld and c are multiples of 4) and inside the image
                uint16_t ob[4];
                memcpy(ob, o_img + r * o_ld + c, 8);
                muon_apply_piece(p, g, ob, r * cols + c, n, vec && n == 4, km, zero_grad, pn);
            }
            else swap_piece(p, e, r * cols + c, n, vec && n == 4, pn);
            if constexpr (EMA && OPT != OPT_SWAP) ema_piece(e, r * cols + c, n, vec && n == 4, dt, pn);
        }
        if (!dst && !dst_t) continue;
        bf16 b[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { b[e] = (bf16)pn[e]; tile[lr_][tx * 4 + e] = b[e]; }
        if (dst && r < rows) {
            if ((cols & 3) == 0 && c + 3 < cols) *(bf16x4*)(dst + r * cols + c) = bf16x4{b[0], b[1], b[2], b[3]};
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (c + e < cols) dst[r * cols + c + e] = b[e];
            }
        }
    }
    if (!dst_t) return;
    __syncthreads();
    const bool vec_t = (rows & 3) == 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int lc = ty + 16 * j;                 // column of the source tile = row of the transposed shadow
        const int64_t c = c0 + lc, r = r0 + tx * 4;
        if (c >= cols) continue;
        bf16 b[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = tile[tx * 4 + e][lc];
        if (vec_t && r + 3 < rows) *(bf16x4*)(dst_t + c * rows + r) = bf16x4{b[0], b[1], b[2], b[3]};
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (r + e < rows) dst_t[c * rows + r + e] = b[e];
        }
    }
}

template <int OPT>
__global__ void __launch_bounds__(256)
optim_update_kernel(const int64_t* __restrict__ desc, int count, const float* __restrict__ res,
                    const float* __restrict__ hyper, int zero_grad) {
    optim_update_tile<OPT, false>(desc, count, res, hyper, zero_grad, nullptr, nullptr);
}

template <int OPT>
__global__ void __launch_bounds__(256)
optim_update_ema_kernel(const int64_t* __restrict__ desc, int count, const float* __restrict__ res,
                        const float* __restrict__ hyper, int zero_grad, float* __restrict__ ema_flat, const float* grad_flat) {
    optim_update_tile<OPT, true>(desc, count, res, hyper, zero_grad, ema_flat, grad_flat);
}

__global__ void __launch_bounds__(256)
ema_swap_kernel(const int64_t* __restrict__ desc, int count, float* __restrict__ ema_flat, const float* grad_flat) {
    optim_update_tile<OPT_SWAP, true>(desc, count, nullptr, nullptr, 0, ema_flat, grad_flat);
}

extern "C" int64_t vited_adamw_workspace_bytes(void) { return (int64_t)(AD_PARTIALS + AD_RESULT_WORDS) * sizeof(float); }

// ema_flat == nullptr: the update without the average (the instances vited_adamw_step / vited_sgd_step have always reached).
template <int OPT>
static int optim_step(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel, float* hyper,
                      float max_norm, int zero_grad, float* norm_out, float* workspace, int64_t workspace_bytes, float* ema_flat,
                      void* stream) {
    if (!desc || !grad_flat || !hyper || !workspace || count <= 0 || grad_numel <= 0 || total_tiles <= 0 || total_tiles > 0x7fffffff)
        return VITED_ERR_BAD_ARG;
    if (workspace_bytes < vited_adamw_workspace_bytes()) return VITED_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(AD_PARTIALS), dim3(256), 0, s, grad_flat, grad_numel, workspace);
    hipLaunchKernelGGL(optim_decide_kernel, dim3(1), dim3(256), 0, s, workspace, hyper, max_norm, norm_out, ema_flat ? 1 : 0);
    if (ema_flat)
        hipLaunchKernelGGL(optim_update_ema_kernel<OPT>, dim3((unsigned)total_tiles), dim3(256), 0, s, desc, count,
                           workspace + AD_PARTIALS, hyper, zero_grad, ema_flat, grad_flat);
    else
        hipLaunchKernelGGL(optim_update_kernel<OPT>, dim3((unsigned)total_tiles), dim3(256), 0, s, desc, count, workspace + AD_PARTIALS,
                           hyper, zero_grad);
    return vited_check_launch();
}

// The average must cover the gradient buffer and allow the 16-byte accesses the gradient slices allow.
static bool ema_buffer_ok(const float* ema_flat, int64_t ema_numel, int64_t grad_numel) {
    return ema_flat && ((uintptr_t)ema_flat & 15) == 0 && ema_numel >= grad_numel;
}

extern "C" int vited_adamw_step(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                                float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                                int64_t workspace_bytes, void* stream) {
    return optim_step<OPT_ADAMW>(desc, count, total_tiles, grad_flat, grad_numel, hyper, max_norm, zero_grad, norm_out, workspace,
                                 workspace_bytes, nullptr, stream);
}

extern "C" int vited_sgd_step(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                              float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                              int64_t workspace_bytes, void* stream) {
    return optim_step<OPT_SGD>(desc, count, total_tiles, grad_flat, grad_numel, hyper, max_norm, zero_grad, norm_out, workspace,
                               workspace_bytes, nullptr, stream);
}

extern "C" int vited_adamw_step_ema(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                                    float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                                    int64_t workspace_bytes, float* ema_flat, int64_t ema_numel, void* stream) {
    if (!ema_buffer_ok(ema_flat, ema_numel, grad_numel)) return VITED_ERR_BAD_ARG;
    return optim_step<OPT_ADAMW>(desc, count, total_tiles, grad_flat, grad_numel, hyper, max_norm, zero_grad, norm_out, workspace,
                                 workspace_bytes, ema_flat, stream);
}

extern "C" int vited_sgd_step_ema(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                                  float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                                  int64_t workspace_bytes, float* ema_flat, int64_t ema_numel, void* stream) {
    if (!ema_buffer_ok(ema_flat, ema_numel, grad_numel)) return VITED_ERR_BAD_ARG;
    return optim_step<OPT_SGD>(desc, count, total_tiles, grad_flat, grad_numel, hyper, max_norm, zero_grad, norm_out, workspace,
                               workspace_bytes, ema_flat, stream);
}

extern "C" int vited_lion_step(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                               float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                               int64_t workspace_bytes, void* stream) {
    return optim_step<OPT_LION>(desc, count, total_tiles, grad_flat, grad_numel, hyper, max_norm, zero_grad, norm_out, workspace,
                                workspace_bytes, nullptr, stream);
}

extern "C" int vited_lion_step_ema(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                                   float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                                   int64_t workspace_bytes, float* ema_flat, int64_t ema_numel, void* stream) {
    if (!ema_buffer_ok(ema_flat, ema_numel, grad_numel)) return VITED_ERR_BAD_ARG;
    return optim_step<OPT_LION>(desc, count, total_tiles, grad_flat, grad_numel, hyper, max_norm, zero_grad, norm_out, workspace,
                                workspace_bytes, ema_flat, stream);
}

// ---- LAMB (vited_lamb_step / vited_lamb_step_ema; the rule is optim_update.h's) ----------------------------------------------------------
// No element of a tensor may move before the 2-norms of the whole tensor's p and u are known, so the update takes three launches behind
// the sum of squares and the decision:
//   launch 3  lamb_moments_kernel: one workgroup per 64 x 64 tile (the table and tiling of optim_update_tile); reads g, p, m, v, writes
//                                  m, v, forms u in registers and leaves the tile's {sum p^2, sum u^2} in tile_sums[2 * tile ..].  Order:
//                                  a thread adds its 16 elements one after the other, then block_sum_256 (wave butterfly, 4 wave sums).
//   launch 4  lamb_ratio_kernel  : one wave per tensor; lane l adds the tensor's tiles l, l + 64, .. in ascending order, wave_sum, lane
//                                  0 writes r to ratio[row].  No atomics: the sums do not depend on scheduling.
//   launch 5  optim_update_kernel<OPT_LAMB> (or its EMA instance): the tile body above; u again through lamb_u from the m, v just
//                                  written and the old p, p -= lr r u, both shadows, the average, g zeroed.  g is never read here and
//                                  never used as scratch, so zero_grad == 0 leaves its bits alone.
// A skipped update returns at once from launches 3 and 4 (m, v, tile_sums and ratio keep their bits) and zeroes g in launch 5.
// HBM traffic per element: 28 B read (g, p, m, v; then p, m, v) + 16 B written (m, v; then p, g) + 4 B of shadows.
// Workspace (floats): [0, 1024) partials, 4 result words, ratio[count], tile_sums[2 * total_tiles].
#define LAMB_RATIO_AT (AD_PARTIALS + AD_RESULT_WORDS)

__global__ void __launch_bounds__(256)
lamb_moments_kernel(const int64_t* __restrict__ desc, int count, const float* __restrict__ res, const float* __restrict__ hyper,
                    float* __restrict__ tile_sums) {
    __shared__ float red[4];
    if (res[2] == 0.f) return;                  // skipped: the same word in every workgroup
    const float clip = res[1], step = res[3];
    const int64_t blk = blockIdx.x;
    int lo = 0, hi = count - 1;     // last descriptor whose first_tile <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(int64_t)mid * AD_DESC_WORDS + 8] <= blk) lo = mid; else hi = mid - 1;
    }
    const int64_t* d = desc + (int64_t)lo * AD_DESC_WORDS;
    const float* p = (const float*)d[0];
    const float* g = (const float*)d[1];
    float* m = (float*)d[2];
    float* v = (float*)d[3];
    const int64_t rows = d[6], cols = d[7];
    const LambCoef k = lamb_coef(hyper + AD_HYPER_HEADER + d[9] * AD_GROUP_WORDS, step);
    const int64_t t = blk - d[8], tiles_c = (cols + 63) >> 6;
    const int64_t r0 = (t / tiles_c) << 6, c0 = (t % tiles_c) << 6;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;   // 16 x 16: 4 columns x 4 rows per thread
    const bool vec = (cols & 3) == 0 && (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    float sp = 0.f, su = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t r = r0 + ty + 16 * j, c = c0 + tx * 4;
        if (r < rows && c < cols) {
            const int n = cols - c < 4 ? (int)(cols - c) : 4;
            lamb_moments_piece(p, g, m, v, r * cols + c, n, vec && n == 4, k, clip, &sp, &su);
        }
    }
    sp = block_sum_256(sp, red);
    su = block_sum_256(su, red);
    if (threadIdx.x == 0) { tile_sums[2 * blk] = sp; tile_sums[2 * blk + 1] = su; }
}

__global__ void __launch_bounds__(64)
lamb_ratio_kernel(const int64_t* __restrict__ desc, const float* __restrict__ res, const float* __restrict__ hyper,
                  const float* __restrict__ tile_sums, float* __restrict__ ratio) {
    if (res[2] == 0.f) return;
    const int64_t* d = desc + (int64_t)blockIdx.x * AD_DESC_WORDS;
    const int64_t tiles = ((d[6] + 63) >> 6) * ((d[7] + 63) >> 6);
    const float* sums = tile_sums + 2 * d[8];
    float sp = 0.f, su = 0.f;
    for (int64_t t = threadIdx.x; t < tiles; t += 64) { sp += sums[2 * t]; su += sums[2 * t + 1]; }
    sp = wave_sum(sp);
    su = wave_sum(su);
    if (threadIdx.x == 0) ratio[blockIdx.x] = lamb_ratio(sp, su, lamb_coef(hyper + AD_HYPER_HEADER + d[9] * AD_GROUP_WORDS, res[3]));
}

__global__ void __launch_bounds__(256)
lamb_apply_kernel(const int64_t* __restrict__ desc, int count, const float* __restrict__ res, const float* __restrict__ hyper,
                  int zero_grad, const float* __restrict__ ratio) {
    optim_update_tile<OPT_LAMB, false>(desc, count, res, hyper, zero_grad, nullptr, nullptr, ratio);
}

__global__ void __launch_bounds__(256)
lamb_apply_ema_kernel(const int64_t* __restrict__ desc, int count, const float* __restrict__ res, const float* __restrict__ hyper,
                      int zero_grad, float* __restrict__ ema_flat, const float* grad_flat, const float* __restrict__ ratio) {
    optim_update_tile<OPT_LAMB, true>(desc, count, res, hyper, zero_grad, ema_flat, grad_flat, ratio);
}

extern "C" int64_t vited_lamb_workspace_bytes(int64_t total_tiles, int count) {
    if (total_tiles <= 0 || total_tiles > 0x7fffffff || count <= 0) return 0;
    return (int64_t)(LAMB_RATIO_AT + (int64_t)count + 2 * total_tiles) * sizeof(float);
}

static int lamb_step(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel, float* hyper,
                     float max_norm, int zero_grad, float* norm_out, float* workspace, int64_t workspace_bytes, float* ema_flat,
                     void* stream) {
    if (!desc || !grad_flat || !hyper || !workspace || count <= 0 || grad_numel <= 0 || total_tiles <= 0 || total_tiles > 0x7fffffff)
        return VITED_ERR_BAD_ARG;
    if (workspace_bytes < vited_lamb_workspace_bytes(total_tiles, count)) return VITED_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const float* res = workspace + AD_PARTIALS;
    float* ratio = workspace + LAMB_RATIO_AT;
    float* tile_sums = ratio + count;
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(AD_PARTIALS), dim3(256), 0, s, grad_flat, grad_numel, workspace);
    hipLaunchKernelGGL(optim_decide_kernel, dim3(1), dim3(256), 0, s, workspace, hyper, max_norm, norm_out, ema_flat ? 1 : 0);
    hipLaunchKernelGGL(lamb_moments_kernel, dim3((unsigned)total_tiles), dim3(256), 0, s, desc, count, res, hyper, tile_sums);
    hipLaunchKernelGGL(lamb_ratio_kernel, dim3((unsigned)count), dim3(64), 0, s, desc, res, hyper, tile_sums, ratio);
    if (ema_flat)
        hipLaunchKernelGGL(lamb_apply_ema_kernel, dim3((unsigned)total_tiles), dim3(256), 0, s, desc, count, res, hyper, zero_grad,
                           ema_flat, grad_flat, ratio);
    else
        hipLaunchKernelGGL(lamb_apply_kernel, dim3((unsigned)total_tiles), dim3(256), 0, s, desc, count, res, hyper, zero_grad, ratio);
    return vited_check_launch();
}

extern "C" int vited_lamb_step(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                               float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                               int64_t workspace_bytes, void* stream) {
    return lamb_step(desc, count, total_tiles, grad_flat, grad_numel, hyper, max_norm, zero_grad, norm_out, workspace, workspace_bytes,
                     nullptr, stream);
}

extern "C" int vited_lamb_step_ema(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                                   float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                                   int64_t workspace_bytes, float* ema_flat, int64_t ema_numel, void* stream) {
    if (!ema_buffer_ok(ema_flat, ema_numel, grad_numel)) return VITED_ERR_BAD_ARG;
    return lamb_step(desc, count, total_tiles, grad_flat, grad_numel, hyper, max_norm, zero_grad, norm_out, workspace, workspace_bytes,
                     ema_flat, stream);
}

extern "C" int vited_ema_swap(const int64_t* desc, int count, int64_t total_tiles, float* ema_flat, const float* grad_flat,
                              void* stream) {
    if (!desc || !grad_flat || count <= 0 || total_tiles <= 0 || total_tiles > 0x7fffffff || !ema_buffer_ok(ema_flat, 0, 0))
        return VITED_ERR_BAD_ARG;
    hipLaunchKernelGGL(ema_swap_kernel, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, desc, count, ema_flat, grad_flat);
    return vited_check_launch();
}

// ---- Muon's two elementwise launches that share the tile body (the entries, the Newton-Schulz kernels and the rest are muon.hip's) ------
//   muon_moments_kernel: one workgroup per 64 x 64 tile.  A tile of an aux tensor (tensor table base < 0) IS vited_adamw_step's third
//                        launch - the OPT_ADAMW instance of optim_update_tile, skipped update and average included - so an aux tensor
//                        gets AdamW's bits.  A tile of a Muon tensor reads g and buf, writes buf and leaves its sum of u^2 in
//                        tile_sums[tile] (a thread adds its 16 elements one after the other, then block_sum_256); skipped: nothing.
//   muon_apply_kernel  : the OPT_MUON instance of the tile body; aux tiles return at once.
template <bool EMA>
__global__ void __launch_bounds__(256)
muon_moments_kernel(const int64_t* __restrict__ desc, int count, const float* __restrict__ res, const float* __restrict__ hyper,
                    int zero_grad, float* __restrict__ ema_flat, const float* grad_flat, const int64_t* __restrict__ tensor_tab,
                    float* __restrict__ tile_sums) {
    __shared__ float red[4];
    const int64_t blk = blockIdx.x;
    int lo = 0, hi = count - 1;     // last descriptor whose first_tile <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(int64_t)mid * AD_DESC_WORDS + 8] <= blk) lo = mid; else hi = mid - 1;
    }
    if (tensor_tab[(int64_t)lo * MUON_TENSOR_WORDS] < 0) {      // aux: the same word in every thread of the workgroup
        optim_update_tile<OPT_ADAMW, EMA>(desc, count, res, hyper, zero_grad, ema_flat, grad_flat);
        return;
    }
    if (res[2] == 0.f) return;                  // skipped
    const float clip = res[1];
    const int64_t* d = desc + (int64_t)lo * AD_DESC_WORDS;
    const float* g = (const float*)d[1];
    float* buf = (float*)d[2];
    const int64_t rows = d[6], cols = d[7];
    const MuonCoef k = muon_coef(hyper + AD_HYPER_HEADER + d[9] * AD_GROUP_WORDS, rows, cols);
    const int64_t t = blk - d[8], tiles_c = (cols + 63) >> 6;
    const int64_t r0 = (t / tiles_c) << 6, c0 = (t % tiles_c) << 6;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;   // 16 x 16: 4 columns x 4 rows per thread
    const bool vec = (cols & 3) == 0 && (((uintptr_t)g | (uintptr_t)buf) & 15) == 0;
    float su = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t r = r0 + ty + 16 * j, c = c0 + tx * 4;
        if (r < rows && c < cols) {
            const int n = cols - c < 4 ? (int)(cols - c) : 4;
            muon_moments_piece(g, buf, r * cols + c, n, vec && n == 4, k, clip, &su);
        }
    }
    su = block_sum_256(su, red);
    if (threadIdx.x == 0) tile_sums[blk] = su;
}

__global__ void __launch_bounds__(256)
muon_apply_kernel(const int64_t* __restrict__ desc, int count, const float* __restrict__ res, const float* __restrict__ hyper,
                  int zero_grad, MuonApplyArgs mu) {
    optim_update_tile<OPT_MUON, false>(desc, count, res, hyper, zero_grad, nullptr, nullptr, nullptr, mu);
}

__global__ void __launch_bounds__(256)
muon_apply_ema_kernel(const int64_t* __restrict__ desc, int count, const float* __restrict__ res, const float* __restrict__ hyper,
                      int zero_grad, float* __restrict__ ema_flat, const float* grad_flat, MuonApplyArgs mu) {
    optim_update_tile<OPT_MUON, true>(desc, count, res, hyper, zero_grad, ema_flat, grad_flat, nullptr, mu);
}

void muon_launch_head(const float* grad_flat, int64_t grad_numel, float* hyper, float max_norm, float* norm_out, float* workspace,
                      int ema, hipStream_t s) {
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(AD_PARTIALS), dim3(256), 0, s, grad_flat, grad_numel, workspace);
    hipLaunchKernelGGL(optim_decide_kernel, dim3(1), dim3(256), 0, s, workspace, hyper, max_norm, norm_out, ema);
}

void muon_launch_moments(const int64_t* desc, int count, int64_t total_tiles, const float* res, const float* hyper, int zero_grad,
                         float* ema_flat, const float* grad_flat, const int64_t* tensor_tab, float* tile_sums, hipStream_t s) {
    if (ema_flat)
        hipLaunchKernelGGL(muon_moments_kernel<true>, dim3((unsigned)total_tiles), dim3(256), 0, s, desc, count, res, hyper, zero_grad,
                           ema_flat, grad_flat, tensor_tab, tile_sums);
    else
        hipLaunchKernelGGL(muon_moments_kernel<false>, dim3((unsigned)total_tiles), dim3(256), 0, s, desc, count, res, hyper, zero_grad,
                           (float*)nullptr, (const float*)nullptr, tensor_tab, tile_sums);
}

void muon_launch_apply(const int64_t* desc, int count, int64_t total_tiles, const float* res, const float* hyper, int zero_grad,
                       float* ema_flat, const float* grad_flat, const int64_t* tensor_tab, const uint16_t* scratch, int final_img,
                       hipStream_t s) {
    const MuonApplyArgs mu = {tensor_tab, scratch, final_img};
    if (ema_flat)
        hipLaunchKernelGGL(muon_apply_ema_kernel, dim3((unsigned)total_tiles), dim3(256), 0, s, desc, count, res, hyper, zero_grad,
                           ema_flat, grad_flat, mu);
    else
        hipLaunchKernelGGL(muon_apply_kernel, dim3((unsigned)total_tiles), dim3(256), 0, s, desc, count, res, hyper, zero_grad, mu);
}

bool muon_ema_buffer_ok(const float* ema_flat, int64_t ema_numel, int64_t grad_numel) { return ema_buffer_ok(ema_flat, ema_numel, grad_numel); }
