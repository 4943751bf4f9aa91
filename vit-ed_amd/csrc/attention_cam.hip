// Head-averaged attention relevancy maps (Chefer et al., rule 5; scripts/visualise_attentions.py avg_heads) without any
// per-head N x N tensor:
//
//   VITED_CAM_GRAD   cam[b, i, j] = (1/H) sum_h max(P_h[i, j] * dP_h[i, j], 0)
//   VITED_CAM_PROB   cam[b, i, j] = sum_h w[b, h] * P_h[i, j]                        (null w: 1/H)
//
// with P_h = exp(scale q_h . k_h - lse[b, h, i]) rebuilt from the forward's saved log-sum-exp and dP_h = dO_h . v_h.  Every
// operand already sits in HBM when the attention backward runs; the kernels below stop where the flash dQ kernel forms P and dP
// tile by tile, fold the heads in registers in the fixed order 0 .. H-1 (bit-reproducible, no atomics, nothing zero-initialised)
// and store each element of the [Nq, Nk] output exactly once.
//
//   MFMA kernel      bf16, head_dim 32 / 64.  One workgroup = 4 waves x 32 queries of one batch item and a run of 64-key tiles;
//                    outer loop over the key tiles, inner loop over the heads.  Scores are computed transposed like the flash
//                    kernels' (keys on accumulator rows, the query on the lane): -lse / scale of the lane's query is the INITIAL
//                    accumulator of the score chain, so P = exp2(scale log2(e) S') with no maximum, no rescale and no
//                    subtraction.  P and dP stay fp32 - they feed no further MFMA.  K / V tiles are staged exactly like the flash
//                    kernels' (register-staged, double buffered; attention_tiles.h); the next step's q / dO fragments and lse are
//                    fetched under the current step's MFMAs.
//                    STORE LAYOUT: the finished 32 x 64 tile of a wave is turned through a wave-private LDS patch so that the
//                    KEY sits on the lane for the store: one store instruction writes 64 consecutive keys of one query row,
//                    256 contiguous bytes (two whole 128-byte lines where the row is line-aligned).  Stored straight from the
//                    accumulators (query on the lane) an instruction would touch 16 rows x 64 bytes - sixteen half lines.  Rows
//                    of an odd-length output (Nk = 1025) are only 4-byte aligned, hence dword stores.
//   portable kernel  fp32 VALU, any head_dim, fp32 or bf16 storage, no alignment conditions: one workgroup = 16 queries x 64
//                    keys of one batch item, thread = 4 queries x 1 key (key on the lane: same 256-byte row stores).
#include "attention_tiles.h"

struct CamArgs {
    AttnArgs a;             // q, k, v, d_o (+ o_bs / o_ts = d_o's strides), lse, sizes, scale
    const float* w;         // PROB: [B, H] head weights, null = 1 / H
    float* cam;
    int64_t cam_bs, cam_ld;
    int tiles_per_wg;       // MFMA kernel: 64-key tiles per workgroup
};

// ------------------------------------------------------------------------------------------------
// bf16 MFMA kernel
// ------------------------------------------------------------------------------------------------
#define CAM_OS 68   // floats per row of the store patch (64 + 4: rows stay 16-byte aligned, f32x4 writes spread over the banks)

template <int HD, bool GRAD>
__global__ void __launch_bounds__(256)
attn_cam_mfma_kernel(CamArgs ca) {
    using C = SmallCfg<HD>;
    using F = FlashCfg<HD>;
    constexpr int STAGE_BYTES = (GRAD ? 2 : 1) * F::TILE_BYTES;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 stages][K tile (| V tile)] [4 waves][16][CAM_OS] f32
    const AttnArgs& a = ca.a;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int64_t b = blockIdx.z;
    const int nq = (int)a.nq, nk = (int)a.nk, H = a.heads;
    const int q0 = blockIdx.x * (64 * FL_W) + wave * (16 * FL_W);
    const bf16* qb = (const bf16*)a.q + b * a.q_bs;
    const bf16* kb = (const bf16*)a.k + b * a.k_bs;
    const bf16* vb = GRAD ? (const bf16*)a.v + b * a.v_bs : nullptr;
    const bf16* dob = GRAD ? (const bf16*)a.d_o + b * a.o_bs : nullptr;
    const float* lse_b = a.lse + b * H * (int64_t)nq;
    const float sc = a.scale * LOG2E;
    const float neg_inv_scale = -1.f / a.scale;
    const float inv_h = 1.f / (float)H;
    float* patch = (float*)(smem + 2 * STAGE_BYTES) + wave * (16 * CAM_OS);

    const int ntiles_all = (nk + FL_TILE - 1) / FL_TILE;
    const int t_begin = blockIdx.y * ca.tiles_per_wg;
    const int t_end = t_begin + ca.tiles_per_wg < ntiles_all ? t_begin + ca.tiles_per_wg : ntiles_all;
    const int steps = (t_end - t_begin) * H;      // one step = (key tile, head); >= H: the launcher starts no empty workgroup

    int qrow[FL_W];
#pragma unroll
    for (int w = 0; w < FL_W; ++w) {
        const int q = q0 + 16 * w + fr;
        qrow[w] = q < nq ? q : nq - 1;
    }
    // per-step row operands: fetched one step ahead
    bf16x8 qn[FL_W][C::KCH], don[FL_W][C::KCH];
    float c0n[FL_W];
    auto fetch_rows = [&](int h) {
#pragma unroll
        for (int w = 0; w < FL_W; ++w) {
            load_row_frags<HD>(qb + (int64_t)h * HD, a.q_ts, q0 + 16 * w, nq, fr, g, qn[w]);
            if constexpr (GRAD) load_row_frags<HD>(dob + (int64_t)h * HD, a.o_ts, q0 + 16 * w, nq, fr, g, don[w]);
            c0n[w] = lse_b[(int64_t)h * nq + qrow[w]];
        }
    };
    bf16x8 kr[F::PASSES], vr[F::PASSES];
    const TileMap<HD> mk(tid);
    auto fetch_tile = [&](int t, int h) {
        tile_to_regs<HD>(kb + (int64_t)h * HD, a.k_ts, t * FL_TILE, nk, mk, kr);
        if constexpr (GRAD) tile_to_regs<HD>(vb + (int64_t)h * HD, a.v_ts, t * FL_TILE, nk, mk, vr);
    };
    auto store_tile = [&](char* stage, int t) {
        regs_to_tile<HD>(stage, t * FL_TILE, nk, mk, kr);
        if constexpr (GRAD) regs_to_tile<HD>(stage + F::TILE_BYTES, t * FL_TILE, nk, mk, vr);
    };

    fetch_tile(t_begin, 0);
    fetch_rows(0);
    store_tile(smem, t_begin);
    __syncthreads();

    f32x4 acc[FL_W][4];
#pragma unroll
    for (int w = 0; w < FL_W; ++w)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) acc[w][kt] = f32x4{0.f, 0.f, 0.f, 0.f};

    int t = t_begin, h = 0;
    for (int s = 0; s < steps; ++s) {
        const char* ks = smem + (s & 1) * STAGE_BYTES;
        const char* vs = ks + F::TILE_BYTES;
        // this step's row operands (arrived under the previous step), then the next step's fetches
        bf16x8 qf[FL_W][C::KCH], dof[FL_W][C::KCH];
        float c0[FL_W];
#pragma unroll
        for (int w = 0; w < FL_W; ++w) {
#pragma unroll
            for (int c = 0; c < C::KCH; ++c) {
                qf[w][c] = qn[w][c];
                if constexpr (GRAD) dof[w][c] = don[w][c];
            }
            c0[w] = c0n[w] * neg_inv_scale;
        }
        float wh = inv_h;
        if constexpr (!GRAD) {
            if (ca.w) wh = ca.w[b * H + h];
        }
        const int hn = h + 1 < H ? h + 1 : 0;
        const int tn = h + 1 < H ? t : t + 1;
        const bool more = s + 1 < steps;   // wave-uniform
        if (more) {
            fetch_tile(tn, hn);
            fetch_rows(hn);
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            bf16x8 kf[C::KCH], vf[C::KCH];
            lds_row_frags<HD>(ks, kt, fr, g, kf);
            if constexpr (GRAD) lds_row_frags<HD>(vs, kt, fr, g, vf);
#pragma unroll
            for (int w = 0; w < FL_W; ++w) {
                f32x4 sv = {c0[w], c0[w], c0[w], c0[w]}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < C::KCH; ++c) {
                    sv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[c], qf[w][c], sv, 0, 0, 0);
                    if constexpr (GRAD) dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[c], dof[w][c], dp, 0, 0, 0);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pe = __builtin_amdgcn_exp2f(sv[e] * sc);
                    if constexpr (GRAD) acc[w][kt][e] += fmaxf(pe * dp[e], 0.f);
                    else acc[w][kt][e] = fmaf(wh, pe, acc[w][kt][e]);
                }
            }
        }
        if (more) store_tile(smem + ((s + 1) & 1) * STAGE_BYTES, tn);
        if (h + 1 == H) {   // the tile is complete: turn it through the patch and store rows of 64 consecutive keys
            const int key = t * FL_TILE + lane;
#pragma unroll
            for (int w = 0; w < FL_W; ++w) {
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    f32x4 v = acc[w][kt];
                    if constexpr (GRAD) v *= inv_h;
                    *(f32x4*)(patch + fr * CAM_OS + 16 * kt + 4 * g) = v;
                    acc[w][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                __syncthreads();
                const int qw = q0 + 16 * w;
                if (key < nk) {
                    float* dst = ca.cam + b * ca.cam_bs + (int64_t)qw * ca.cam_ld + key;
                    const int rows = nq - qw < 16 ? nq - qw : 16;      // <= 0 for a wave past the last query
                    for (int r = 0; r < rows; ++r) dst[(int64_t)r * ca.cam_ld] = patch[r * CAM_OS + lane];
                }
                __syncthreads();
            }
        }
        __syncthreads();
        h = hn;
        t = tn;
    }
}

template <int HD, bool GRAD>
static int launch_cam_mfma(CamArgs& ca, hipStream_t s) {
    const AttnArgs& a = ca.a;
    const int64_t qtiles = ceil_div64(a.nq, 64 * FL_W), ntiles = ceil_div64(a.nk, FL_TILE);
    // enough workgroups for two rounds of the chip before a workgroup takes a second key tile: each tile re-reads the query
    // tile's q / dO rows (cheap, L2), while a long run of tiles is one long chain of dependent loads
    int64_t per = qtiles * ntiles * a.batch / 512;
    per = per < 1 ? 1 : (per > ntiles ? ntiles : per);
    ca.tiles_per_wg = (int)per;
    const int64_t chunks = ceil_div64(ntiles, per);
    if (qtiles > 0x7fffffff || chunks > 65535) return VITED_ERR_UNSUPPORTED;
    dim3 grid((unsigned)qtiles, (unsigned)chunks, (unsigned)a.batch);
    const size_t lds = 2 * (GRAD ? 2 : 1) * FlashCfg<HD>::TILE_BYTES + 4 * 16 * CAM_OS * sizeof(float);
    hipLaunchKernelGGL((attn_cam_mfma_kernel<HD, GRAD>), grid, dim3(256), lds, s, ca);
    return vited_check_launch();
}

// ------------------------------------------------------------------------------------------------
// portable fp32 kernel
// ------------------------------------------------------------------------------------------------
#define CP_TQ 16   // queries per workgroup
#define CP_TK 64   // keys per workgroup (one per lane)
#define CP_DC 32   // head-dim chunk staged in LDS

template <typename T>
__device__ __forceinline__ void cam_stage(const T* base, int64_t ts, int64_t row0, int64_t n, int d0, int hd, int rows, float (*dst)[CP_DC + 1]) {
    for (int e = threadIdx.x; e < rows * CP_DC; e += 256) {
        const int r = e / CP_DC, d = e - r * CP_DC;
        const int64_t row = row0 + r;
        dst[r][d] = (row < n && d0 + d < hd) ? to_f32(base[row * ts + d0 + d]) : 0.f;
    }
}

template <typename T, bool GRAD>
__global__ void __launch_bounds__(256)
attn_cam_portable_kernel(CamArgs ca) {
    __shared__ float Qs[CP_TQ][CP_DC + 1], Ds[CP_TQ][CP_DC + 1], Ks[CP_TK][CP_DC + 1], Vs[CP_TK][CP_DC + 1];
    const AttnArgs& a = ca.a;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t b = blockIdx.z;
    const int64_t j0 = (int64_t)blockIdx.x * CP_TK, i0 = (int64_t)blockIdx.y * CP_TQ;
    const int hd = a.head_dim, H = a.heads;
    const float inv_h = 1.f / (float)H;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int h = 0; h < H; ++h) {
        const T* qb = (const T*)a.q + b * a.q_bs + (int64_t)h * hd;
        const T* kb = (const T*)a.k + b * a.k_bs + (int64_t)h * hd;
        float s[4] = {0.f, 0.f, 0.f, 0.f}, dp[4] = {0.f, 0.f, 0.f, 0.f};
        for (int d0 = 0; d0 < hd; d0 += CP_DC) {
            __syncthreads();
            cam_stage<T>(qb, a.q_ts, i0, a.nq, d0, hd, CP_TQ, Qs);
            cam_stage<T>(kb, a.k_ts, j0, a.nk, d0, hd, CP_TK, Ks);
            if constexpr (GRAD) {
                cam_stage<T>((const T*)a.d_o + b * a.o_bs + (int64_t)h * hd, a.o_ts, i0, a.nq, d0, hd, CP_TQ, Ds);
                cam_stage<T>((const T*)a.v + b * a.v_bs + (int64_t)h * hd, a.v_ts, j0, a.nk, d0, hd, CP_TK, Vs);
            }
            __syncthreads();
#pragma unroll 8
            for (int d = 0; d < CP_DC; ++d) {
                const float kd = Ks[tx][d];
                const float vd = GRAD ? Vs[tx][d] : 0.f;
#pragma unroll
                for (int qi = 0; qi < 4; ++qi) {
                    s[qi] = fmaf(Qs[4 * ty + qi][d], kd, s[qi]);
                    if constexpr (GRAD) dp[qi] = fmaf(Ds[4 * ty + qi][d], vd, dp[qi]);
                }
            }
        }
        float wh = inv_h;
        if constexpr (!GRAD) {
            if (ca.w) wh = ca.w[b * H + h];
        }
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) {
            int64_t i = i0 + 4 * ty + qi;
            i = i < a.nq ? i : a.nq - 1;
            const float p = __expf(fmaf(s[qi], a.scale, -a.lse[(b * H + h) * a.nq + i]));
            if constexpr (GRAD) acc[qi] += fmaxf(p * dp[qi], 0.f);
            else acc[qi] = fmaf(wh, p, acc[qi]);
        }
    }
    const int64_t j = j0 + tx;
    if (j < a.nk) {
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) {
            const int64_t i = i0 + 4 * ty + qi;
            if (i < a.nq) ca.cam[b * ca.cam_bs + i * ca.cam_ld + j] = GRAD ? acc[qi] * inv_h : acc[qi];
        }
    }
}

template <typename T, bool GRAD>
static int launch_cam_portable(const CamArgs& ca, hipStream_t s) {
    const AttnArgs& a = ca.a;
    const int64_t gx = ceil_div64(a.nk, CP_TK), gy = ceil_div64(a.nq, CP_TQ);
    if (gx > 0x7fffffff || gy > 65535) return VITED_ERR_UNSUPPORTED;
    dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)a.batch);
    hipLaunchKernelGGL((attn_cam_portable_kernel<T, GRAD>), grid, dim3(256), 0, s, ca);
    return vited_check_launch();
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" int vited_attention_cam(const void* q, int64_t q_bs, int64_t q_ts, const void* k, int64_t k_bs, int64_t k_ts,
                                   const void* v, int64_t v_bs, int64_t v_ts, const void* d_o, int64_t do_bs, int64_t do_ts,
                                   const float* lse, const float* head_weight, float* cam, int64_t cam_bs, int64_t cam_ld,
                                   int mode, int dtype, int64_t batch, int heads, int64_t nq, int64_t nk, int head_dim,
                                   float scale, void* stream) {
    if (mode != VITED_CAM_GRAD && mode != VITED_CAM_PROB) return VITED_ERR_BAD_ARG;
    const bool grad = mode == VITED_CAM_GRAD;
    if (!q || !k || !lse || !cam || (grad && (!v || !d_o))) return VITED_ERR_BAD_ARG;
    if (batch <= 0 || heads <= 0 || nq <= 0 || nk <= 0 || head_dim <= 0 || cam_ld < nk || cam_bs < 0) return VITED_ERR_BAD_ARG;
    if (dtype != VITED_F32 && dtype != VITED_BF16) return VITED_ERR_UNSUPPORTED;
    if (batch > 65535 || heads > 65535 || nq > (1 << 20) || nk > (1 << 20)) return VITED_ERR_UNSUPPORTED;
    CamArgs ca = {};
    AttnArgs& a = ca.a;
    a.q = q; a.k = k; a.v = v; a.d_o = d_o;
    a.q_bs = q_bs; a.q_ts = q_ts; a.k_bs = k_bs; a.k_ts = k_ts; a.v_bs = v_bs; a.v_ts = v_ts; a.o_bs = do_bs; a.o_ts = do_ts;
    a.lse = (float*)lse;
    a.batch = batch; a.heads = heads; a.nq = nq; a.nk = nk; a.head_dim = head_dim; a.scale = scale;
    ca.w = grad ? nullptr : head_weight;
    ca.cam = cam; ca.cam_bs = cam_bs; ca.cam_ld = cam_ld;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VITED_BF16 && scale > 0.f) {
        // attention_mfma_supported's conditions on the operands this mode reads (dO takes the place of o; PROB reads neither v nor dO)
        AttnArgs c = a;
        if (!grad) { c.v = k; c.v_bs = k_bs; c.v_ts = k_ts; c.o_bs = q_bs; c.o_ts = q_ts; }
        c.o = grad ? d_o : q;
        constexpr int64_t LIM = (int64_t)1 << 24;   // tile_to_regs: 32-bit byte offsets inside a 64-row tile
        if (attention_mfma_supported(c, false) && c.k_ts < LIM && c.v_ts < LIM) {
            attention_set_last_path(2);
            if (head_dim == 32) return grad ? launch_cam_mfma<32, true>(ca, s) : launch_cam_mfma<32, false>(ca, s);
            return grad ? launch_cam_mfma<64, true>(ca, s) : launch_cam_mfma<64, false>(ca, s);
        }
    }
    attention_set_last_path(1);
    if (dtype == VITED_F32) return grad ? launch_cam_portable<float, true>(ca, s) : launch_cam_portable<float, false>(ca, s);
    return grad ? launch_cam_portable<bf16, true>(ca, s) : launch_cam_portable<bf16, false>(ca, s);
}
