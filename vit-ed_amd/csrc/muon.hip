// Muon in the fused update (vited_muon_step / vited_muon_step_ema; the rule is muon_update.h's): the momentum of every 2-D tensor of a
// Muon group is orthogonalised by k Newton-Schulz steps on the matrix cores and applied as the update; every tensor of another group
// takes vited_adamw_step's rule from the same tile body (Jordan's MuonWithAuxAdam arrangement in one flat buffer).
//
// Launches of one update, 6 + 3 k in all, every one over ALL tensors at once:
//   1, 2   optim_sumsq_kernel, optim_decide_kernel (optimizer.hip): the gradient norm, the clip and the skip decision of the family.
//   3      muon_moments_kernel (optimizer.hip): aux tiles are finished as AdamW finishes them; Muon tiles get buf and their sum of u^2.
//   4      muon_norm_kernel: one wave per tensor; lane l adds the tensor's tile sums l, l + 64, .. in ascending order, wave_sum, lane 0
//          writes max(|u|_F, eps) to denom[row].  No atomics.
//   5      muon_pack_kernel: one workgroup per 64 x 64 tile of the PADDED tensor: u again (muon_u on g and the new buf), divided,
//          rounded to bf16, written to the image in p's orientation and, through an LDS tile, to the transposed one; rows and columns
//          past the tensor are written as zeros on every update, so the scratch needs no initialisation.
//   6 ..   k times muon_ns_kernel<GRAM>, <POLY>, <NEXT>: one wave per 64 x 64 output tile, driven by a tile table the host built
//          (optim.muon_layout), 2 x 2 accumulators of v_mfma_f32_32x32x16_bf16.
//   last   muon_apply_kernel (optimizer.hip, the OPT_MUON instance of the tile body): p, both shadows, the average, g zeroed.
//
// B X without a transposed read: all three products are NT products with both operands K-contiguous, because every step keeps X^T
// beside X.  A = X X^T reads X [mp, np] twice; S = A A reads A twice (A is symmetric, so A A = A A^T); T = B X sums over X's row index,
// T[i][j] = sum_k B[i][k] XT[j][k], and reads XT [np, mp].  The NEXT epilogue holds four consecutive rows of one column in four
// registers, so X^T of the new X leaves as 8-byte stores next to the 2-byte row stores of X: one more image pair (4 mp np + 2 mp^2
// elements per tensor instead of 2 mp np + 2 mp^2) buys one GEMM kernel, fragments loaded straight from global memory in the MFMA's own
// lane map (lane l: row l & 31, k = 8 (l >> 5) .. + 7: one 16-byte load), no LDS and no bank or alignment rule to get wrong.
// The last step writes only the image in p's orientation, which the apply pass reads.
//
// Zero padding is invariant under the iteration (a zero row of X gives a zero row and column of A and B and stays zero), and every
// image is padded to the 64 granule in both dimensions, so the GEMM kernel has no tail code; only pack and apply see rows and cols.
// A skipped update: every launch behind the decision returns at once, except that aux tiles (launch 3) and Muon tiles (last launch)
// zero g when asked.  g is read by launches 1, 3 and 5 and written by the last one only (aux tensors: by launch 3, which is their last).
// Every sum has a fixed order; nothing here uses an atomic.
//
// Workspace: floats [0, 1024) partials, 4 result words, denom[count], tile_sums[total_tiles], padded to a multiple of 64 floats; then
// the bf16 scratch, a region per Muon tensor (muon_update.h: X0, X1, XT0, XT1, A, B).
#include "common.h"
#include "muon_update.h"

#define MU_PARTIALS 1024
#define MU_DENOM_AT (MU_PARTIALS + 4)
#define MU_DESC_WORDS 10
#define MU_HYPER_HEADER 8
#define MU_GROUP_WORDS 8
enum { NS_GRAM = 0, NS_POLY = 1, NS_NEXT = 2 };

static inline int64_t mu_scratch_at(int count, int64_t total_tiles) {       // in floats
    return (MU_DENOM_AT + (int64_t)count + total_tiles + 63) / 64 * 64;
}

__global__ void __launch_bounds__(64)
muon_norm_kernel(const int64_t* __restrict__ desc, const float* __restrict__ res, const float* __restrict__ hyper,
                 const int64_t* __restrict__ tensor_tab, const float* __restrict__ tile_sums, float* __restrict__ denom) {
    if (res[2] == 0.f) return;
    if (tensor_tab[(int64_t)blockIdx.x * MUON_TENSOR_WORDS] < 0) return;
    const int64_t* d = desc + (int64_t)blockIdx.x * MU_DESC_WORDS;
    const int64_t tiles = ((d[6] + 63) >> 6) * ((d[7] + 63) >> 6);
    const float* sums = tile_sums + d[8];
    float su = 0.f;
    for (int64_t t = threadIdx.x; t < tiles; t += 64) su += sums[t];
    su = wave_sum(su);
    if (threadIdx.x == 0) denom[blockIdx.x] = muon_denom(su, muon_coef(hyper + MU_HYPER_HEADER + d[9] * MU_GROUP_WORDS, d[6], d[7]));
}

__global__ void __launch_bounds__(256)
muon_pack_kernel(const int64_t* __restrict__ desc, int count, const float* __restrict__ res, const float* __restrict__ hyper,
                 const int64_t* __restrict__ tensor_tab, const float* __restrict__ denom, uint16_t* __restrict__ scratch) {
    __shared__ uint16_t tile[64][66];
    if (res[2] == 0.f) return;
    const int64_t blk = blockIdx.x;
    int lo = 0, hi = count - 1;     // last descriptor whose first_tile <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(int64_t)mid * MU_DESC_WORDS + 8] <= blk) lo = mid; else hi = mid - 1;
    }
    const int64_t* tt = tensor_tab + (int64_t)lo * MUON_TENSOR_WORDS;
    if (tt[0] < 0) return;
    const int64_t* d = desc + (int64_t)lo * MU_DESC_WORDS;
    const float* g = (const float*)d[1];
    const float* buf = (const float*)d[2];
    const int64_t rows = d[6], cols = d[7];
    const MuonCoef k = muon_coef(hyper + MU_HYPER_HEADER + d[9] * MU_GROUP_WORDS, rows, cols);
    const float clip = res[1], dn = denom[lo];
    // the image in p's orientation [rp, cp] and the transposed one [cp, rp]: X and XT of a wide tensor, XT and X of a tall one
    const int64_t rp = muon_pad(rows), cp = muon_pad(cols), img = tt[1] * tt[2];
    uint16_t* straight = scratch + tt[0] + (tt[3] ? 2 : 0) * img;
    uint16_t* turned = scratch + tt[0] + (tt[3] ? 0 : 2) * img;
    const int64_t t = blk - d[8], tiles_c = (cols + 63) >> 6;     // = cp / 64: the padded tensor has the tiles of the tensor
    const int64_t r0 = (t / tiles_c) << 6, c0 = (t % tiles_c) << 6;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const bool vec = (cols & 3) == 0 && (((uintptr_t)g | (uintptr_t)buf) & 15) == 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int lr_ = ty + 16 * j;
        const int64_t r = r0 + lr_, c = c0 + tx * 4;
        uint16_t x[4] = {0, 0, 0, 0};
        if (r < rows && c < cols) {
            const int n = cols - c < 4 ? (int)(cols - c) : 4;
            muon_pack_piece(g, buf, r * cols + c, n, vec && n == 4, k, clip, dn, x);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[lr_][tx * 4 + e] = x[e];
        // r < rp and c + 3 < cp always: the tile lies inside the padded image
        *(uint2*)(straight + r * cp + c) = uint2{(uint32_t)x[0] | ((uint32_t)x[1] << 16), (uint32_t)x[2] | ((uint32_t)x[3] << 16)};
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int lc = ty + 16 * j;
        const int64_t c = c0 + lc, r = r0 + tx * 4;
        uint16_t x[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = tile[tx * 4 + e][lc];
        *(uint2*)(turned + c * rp + r) = uint2{(uint32_t)x[0] | ((uint32_t)x[1] << 16), (uint32_t)x[2] | ((uint32_t)x[3] << 16)};
    }
}

// One wave per 64 x 64 tile (ti, tj) of C = P Q^T, P [.., K] and Q [.., K] row-major bf16, K a multiple of 64.
//   NS_GRAM  A = bf16(X X^T)                 P = Q = X[parity] (ld np), K = np
//   NS_POLY  B = bf16(b A + c (A A))         P = Q = A (ld mp), K = mp
//   NS_NEXT  X' = bf16(a X + B X)            P = B (ld mp), Q = XT[parity] (ld mp), K = mp; writes X[parity ^ 1] and XT[parity ^ 1]
//            (last != 0: only the one in p's orientation)
// Accumulator register e of lane l (guide: C/D map of 32x32x16): column l & 31, row (e & 3) + 8 (e >> 2) + 4 (l >> 5).
template <int EPI>
__global__ void __launch_bounds__(64)
muon_ns_kernel(const int64_t* __restrict__ tab, bf16* __restrict__ scratch, const float* __restrict__ res, int parity, int last,
               float ca, float cb, float cc) {
    if (res[2] == 0.f) return;
    const int64_t* t = tab + (int64_t)blockIdx.x * MUON_TILE_WORDS;
    const int64_t ti = t[1], tj = t[2], mp = t[4], np = t[5], tall = t[6], img = mp * np;
    bf16* base = scratch + t[3];
    bf16* A = base + 4 * img;
    bf16* B = A + mp * mp;
    const bf16* P;
    const bf16* Q;
    int64_t ldp, ldq, K;
    if constexpr (EPI == NS_GRAM) { P = Q = base + parity * img; ldp = ldq = np; K = np; }
    else if constexpr (EPI == NS_POLY) { P = Q = A; ldp = ldq = mp; K = mp; }
    else { P = B; Q = base + (2 + parity) * img; ldp = ldq = mp; K = mp; }
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const bf16* pa = P + (ti * 64 + r) * ldp + 8 * h;
    const bf16* pb = Q + (tj * 64 + r) * ldq + 8 * h;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    for (int64_t k0 = 0; k0 < K; k0 += 64) {
        bf16x8 a[4][2], b[4][2];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            a[s][0] = *(const bf16x8*)(pa + k0 + 16 * s);
            a[s][1] = *(const bf16x8*)(pa + 32 * ldp + k0 + 16 * s);
            b[s][0] = *(const bf16x8*)(pb + k0 + 16 * s);
            b[s][1] = *(const bf16x8*)(pb + 32 * ldq + k0 + 16 * s);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s][i], b[s][j], acc[i][j], 0, 0, 0);
    }
    const bf16* xold = base + parity * img;
    bf16* xnew = base + (parity ^ 1) * img;
    bf16* xtnew = base + (2 + (parity ^ 1)) * img;
    const bool write_x = !last || !tall, write_xt = !last || tall;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t col = tj * 64 + 32 * j + r;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t row = ti * 64 + 32 * i + 8 * q + 4 * h;
                bf16 o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float s = acc[i][j][4 * q + e];
                    if constexpr (EPI == NS_GRAM) o[e] = (bf16)s;
                    else if constexpr (EPI == NS_POLY) o[e] = (bf16)muon_ns_poly(cb, (float)A[(row + e) * mp + col], cc, s);
                    else o[e] = (bf16)muon_ns_next(ca, (float)xold[(row + e) * np + col], s);
                }
                if constexpr (EPI == NS_GRAM) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) A[(row + e) * mp + col] = o[e];
                } else if constexpr (EPI == NS_POLY) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) B[(row + e) * mp + col] = o[e];
                } else {
                    if (write_x) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) xnew[(row + e) * np + col] = o[e];
                    }
                    if (write_xt) *(bf16x4*)(xtnew + col * mp + row) = bf16x4{o[0], o[1], o[2], o[3]};
                }
            }
        }
}

// HOST table rows {rows, cols, ndim, is_muon, group} and the HOST copy of the groups' kind words (word 6 of a group's 8): the counts the
// device tables must have, the scratch size, and the entries' refusals - among them a tensor whose is_muon disagrees with the kind of
// its group, whose coefficients the kernels would otherwise read as the other rule's.
struct MuonPlan { int64_t total_tiles, sq_tiles, x_tiles, scratch_elems; int muon_tensors; };

static int muon_plan(int count, const int64_t* meta, const int64_t* kinds, int groups, MuonPlan* out) {
    MuonPlan pl = {0, 0, 0, 0, 0};
    for (int i = 0; i < count; ++i) {
        const int64_t rows = meta[i * MUON_META_WORDS], cols = meta[i * MUON_META_WORDS + 1], ndim = meta[i * MUON_META_WORDS + 2];
        const int64_t group = meta[i * MUON_META_WORDS + 4];
        if (rows <= 0 || cols <= 0 || group < 0 || group >= groups) return VITED_ERR_BAD_ARG;
        if ((meta[i * MUON_META_WORDS + 3] != 0) != (kinds[group] != 0)) return VITED_ERR_BAD_ARG;
        pl.total_tiles += ((rows + 63) / 64) * ((cols + 63) / 64);
        if (!meta[i * MUON_META_WORDS + 3]) continue;
        if (ndim != 2) return VITED_ERR_BAD_ARG;
        const int64_t m = rows < cols ? rows : cols, n = rows < cols ? cols : rows;
        if (m > MUON_MAX_SHORT_SIDE) return VITED_ERR_UNSUPPORTED;
        const int64_t mp = muon_pad(m), np = muon_pad(n);
        pl.sq_tiles += (mp / 64) * (mp / 64);
        pl.x_tiles += (mp / 64) * (np / 64);
        pl.scratch_elems += muon_region_elems(mp, np);
        ++pl.muon_tensors;
    }
    if (pl.total_tiles > 0x7fffffff || pl.sq_tiles > 0x7fffffff || pl.x_tiles > 0x7fffffff) return VITED_ERR_UNSUPPORTED;
    *out = pl;
    return VITED_OK;
}

extern "C" int64_t vited_muon_workspace_bytes(int count, const int64_t* rows, const int64_t* cols, const int64_t* is_muon) {
    if (count <= 0 || !rows || !cols || !is_muon) return 0;
    int64_t total_tiles = 0, elems = 0;
    for (int i = 0; i < count; ++i) {
        if (rows[i] <= 0 || cols[i] <= 0) return 0;
        total_tiles += ((rows[i] + 63) / 64) * ((cols[i] + 63) / 64);
        if (!is_muon[i]) continue;
        const int64_t m = rows[i] < cols[i] ? rows[i] : cols[i], n = rows[i] < cols[i] ? cols[i] : rows[i];
        if (m > MUON_MAX_SHORT_SIDE) return 0;
        elems += muon_region_elems(muon_pad(m), muon_pad(n));
    }
    if (total_tiles > 0x7fffffff) return 0;
    return mu_scratch_at(count, total_tiles) * (int64_t)sizeof(float) + elems * 2;
}

static int muon_step(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel, float* hyper,
                     float max_norm, int zero_grad, float* norm_out, float* workspace, int64_t workspace_bytes, float* ema_flat,
                     void* stream, const int64_t* tiles_sq, int64_t n_sq, const int64_t* tiles_x, int64_t n_x, const int64_t* tensor_tab,
                     const int64_t* host_meta, const int64_t* host_kinds, int groups, int ns_steps, float ns_a, float ns_b,
                     float ns_c) {
    if (!desc || !grad_flat || !hyper || !workspace || !tensor_tab || !host_meta || !host_kinds || groups <= 0 || count <= 0 ||
        grad_numel <= 0 || total_tiles <= 0 || total_tiles > 0x7fffffff)
        return VITED_ERR_BAD_ARG;
    if ((((uintptr_t)desc | (uintptr_t)tiles_sq | (uintptr_t)tiles_x | (uintptr_t)tensor_tab | (uintptr_t)host_meta |
          (uintptr_t)host_kinds) & 7) ||
        (((uintptr_t)grad_flat | (uintptr_t)hyper) & 3) || ((uintptr_t)workspace & 15))
        return VITED_ERR_BAD_ARG;
    if (ns_steps < 1 || ns_steps > 16) return VITED_ERR_BAD_ARG;
    MuonPlan pl;
    const int rc = muon_plan(count, host_meta, host_kinds, groups, &pl);
    if (rc != VITED_OK) return rc;
    if (pl.total_tiles != total_tiles || pl.sq_tiles != n_sq || pl.x_tiles != n_x) return VITED_ERR_BAD_ARG;
    if (pl.muon_tensors && (!tiles_sq || !tiles_x)) return VITED_ERR_BAD_ARG;
    const int64_t scratch_at = mu_scratch_at(count, total_tiles);
    if (workspace_bytes < scratch_at * (int64_t)sizeof(float) + pl.scratch_elems * 2) return VITED_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const float* res = workspace + MU_PARTIALS;
    float* denom = workspace + MU_DENOM_AT;
    float* tile_sums = denom + count;
    bf16* scratch = (bf16*)(workspace + scratch_at);
    muon_launch_head(grad_flat, grad_numel, hyper, max_norm, norm_out, workspace, ema_flat ? 1 : 0, s);
    muon_launch_moments(desc, count, total_tiles, res, hyper, zero_grad, ema_flat, grad_flat, tensor_tab, tile_sums, s);
    if (pl.muon_tensors) {
        hipLaunchKernelGGL(muon_norm_kernel, dim3((unsigned)count), dim3(64), 0, s, desc, res, hyper, tensor_tab, tile_sums, denom);
        hipLaunchKernelGGL(muon_pack_kernel, dim3((unsigned)total_tiles), dim3(256), 0, s, desc, count, res, hyper, tensor_tab, denom,
                           (uint16_t*)scratch);
        for (int it = 0; it < ns_steps; ++it) {
            const int parity = it & 1, last = it == ns_steps - 1;
            hipLaunchKernelGGL(muon_ns_kernel<NS_GRAM>, dim3((unsigned)n_sq), dim3(64), 0, s, tiles_sq, scratch, res, parity, last, ns_a,
                               ns_b, ns_c);
            hipLaunchKernelGGL(muon_ns_kernel<NS_POLY>, dim3((unsigned)n_sq), dim3(64), 0, s, tiles_sq, scratch, res, parity, last, ns_a,
                               ns_b, ns_c);
            hipLaunchKernelGGL(muon_ns_kernel<NS_NEXT>, dim3((unsigned)n_x), dim3(64), 0, s, tiles_x, scratch, res, parity, last, ns_a,
                               ns_b, ns_c);
        }
        muon_launch_apply(desc, count, total_tiles, res, hyper, zero_grad, ema_flat, grad_flat, tensor_tab, (const uint16_t*)scratch,
                          ns_steps & 1, s);
    }
    return vited_check_launch();
}

extern "C" int vited_muon_step(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                               float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                               int64_t workspace_bytes, void* stream, const int64_t* tiles_sq, int64_t n_sq, const int64_t* tiles_x,
                               int64_t n_x, const int64_t* tensor_tab, const int64_t* host_meta, const int64_t* host_kinds, int groups,
                               int ns_steps, float ns_a, float ns_b, float ns_c) {
    return muon_step(desc, count, total_tiles, grad_flat, grad_numel, hyper, max_norm, zero_grad, norm_out, workspace, workspace_bytes,
                     nullptr, stream, tiles_sq, n_sq, tiles_x, n_x, tensor_tab, host_meta, host_kinds, groups, ns_steps, ns_a, ns_b,
                     ns_c);
}

extern "C" int vited_muon_step_ema(const int64_t* desc, int count, int64_t total_tiles, const float* grad_flat, int64_t grad_numel,
                                   float* hyper, float max_norm, int zero_grad, float* norm_out, float* workspace,
                                   int64_t workspace_bytes, float* ema_flat, int64_t ema_numel, void* stream, const int64_t* tiles_sq,
                                   int64_t n_sq, const int64_t* tiles_x, int64_t n_x, const int64_t* tensor_tab,
                                   const int64_t* host_meta, const int64_t* host_kinds, int groups, int ns_steps, float ns_a,
                                   float ns_b, float ns_c) {
    if (!muon_ema_buffer_ok(ema_flat, ema_numel, grad_numel)) return VITED_ERR_BAD_ARG;
    return muon_step(desc, count, total_tiles, grad_flat, grad_numel, hyper, max_norm, zero_grad, norm_out, workspace, workspace_bytes,
                     ema_flat, stream, tiles_sq, n_sq, tiles_x, n_x, tensor_tab, host_meta, host_kinds, groups, ns_steps, ns_a, ns_b,
                     ns_c);
}
