// Row-complete bf16 MFMA GEMM for the 768-wide residual stream (ViT-Base), with LayerNorm fused into the epilogue: the two modes
// of gemm_row.hip at twice the width.
//
//   MODE_FWD  y = residual + [row_scale[m] *] (A[M,K] . W[768,K]^T + bias)   (fp32)
//             h = LayerNorm(y; gamma, beta, eps) (bf16), mean, rstd           - or h == null: no LayerNorm
//   MODE_BWD  dh = dY[M,K] . Wt[768,K]^T                                      - on chip in fp32, never written
//             dx = dx_in + LN'(dh; x, mean, rstd, gamma) (fp32, + bf16 copy [lp_scale[m] *]), dgamma / dbeta column partials
//
// This file DUPLICATES gemm_row.hip's structure on purpose: the 384 kernels' code generation carries the
// shipped configurations' step times and is not touched; only the extern "C" entries there route N == 768 here.
//
// One 8-wave workgroup owns BM = 64 / 96 complete rows; wave w owns all BM rows x columns 96 w .. 96 w + 95
// (MT x 6 accumulators of v_mfma_f32_16x16x32_bf16, issued transposed so that a lane holds 4 consecutive columns of one row).
// A K = 64 tile of the 768-row W panel is 96 KB, so the 384 kernel's three A + two W buffers of 128-byte lines do not fit the
// 160 KB of LDS.  What gives is the second W buffer: a wave is the only reader of the W rows it stages, so it takes a tile's W
// fragments into registers (48) and refills its rows at once - no barrier on W, one barrier per tile for the double-buffered A
// (the schedule is described where it is written, below).  History, fused against two kernels at 41,544 rows, K = 3072 forward
// (DESIGN.md section 35):
//   1. K = 32 stages of 64-byte rows, two stages, one __syncthreads per stage (the plain pipeline): 328 us against 264;
//   2. the same stages with the W panel two stages ahead in a 3-buffer ring (counted vmcnt, raw s_barrier): 301;
//   3. this one, full 128-byte lines: 258 - 260.  The step is still set by the W panel's way from L2 into the LDS (96 KB per
//      64 / 96 rows x K = 64), not by the MFMAs.
// The epilogue is gemm_row.hip's: 32 rows per pass through an fp32 LDS scratch (32 x 772 floats, over the staging buffers), then
// the LayerNorm kernels' row loop - a 32-lane half-wave owns a row, 6 float4 per lane, all global traffic in full lines.
#include <mutex>
#include <type_traits>

#include "gemm_kernels.h"
#include "gemm_lds.h"
#include "gemm_row768.h"

#define R7_N ROW768_N
#define R7_LD 772        // floats per scratch row: 16-byte aligned rows; 772 mod 32 = 4 spreads the 8-lane groups of ds_write_b128 over the banks
#define R7_J 6           // float4 per lane of a half-wave's row; 16-column tiles per wave

enum { R7_MODE_FWD = 0, R7_MODE_BWD = 1 };

struct Row768Args {
    const bf16* A; int64_t lda;
    int seg_k; int64_t seg_stride;     // the contraction dim may be cut into segments of seg_k columns, segment j starting at A + j * seg_stride
    const bf16* W; int64_t ldw;
    int64_t M; int K;
    // forward
    const float* bias; const float* residual; int64_t ldr;
    float* y; int64_t ldy;
    const float* gamma; const float* beta; float eps;
    bf16* h; int64_t ldh; float* mean; float* rstd;
    // backward
    const float* x; int64_t ldx; const float* mean_in; const float* rstd_in;
    const float* dx_in; int64_t ldxi; float* dx; int64_t lddx; bf16* dx_lp; int64_t ldlp;
    float* partial;     // [tiles][2][768]
    // stochastic depth (SCALED instances only): fp32 [M], one value per row
    const float* row_scale;     // forward: y = residual + row_scale[m] * (a . w^T + bias)
    const float* lp_scale;      // backward: dx_lp = bf16(lp_scale[m] * dx) - the fp32 dx stays unscaled
};

template <int MT> struct Row768Cfg {
    static_assert(MT == 4 || MT == 6, "tile heights: 64 or 96 rows (the backward of a 128-row tile spills: 192 accumulators + the column sums)");
    static constexpr int BM = 16 * MT;
    static constexpr int A_BYTES = BM * 128;                             // one K = 64 tile of the A panel, full 128-byte lines: 8 / 12 KB
    static constexpr int W_BYTES = R7_N * 128;                           // ... of the whole W panel: 96 KB, ONE buffer (wave w's rows at 12 KB x w)
    static constexpr int W_WAVE_BYTES = 96 * 128;
    static constexpr int A_BASE = W_BYTES;                               // then two A buffers
    static constexpr int LDS_BYTES = W_BYTES + 2 * A_BYTES;              // 114,688 / 122,880
    static constexpr int A_PIECES = 2 * MT;                              // 8-row LDS-DMA pieces of an A tile: wave w takes w, w + 8
    static constexpr int PASS_SUB = 2;                                   // 16-row sub-tiles per epilogue pass
    static constexpr int PASS_ROWS = 16 * PASS_SUB;
    static constexpr int NPASS = MT / PASS_SUB;
    static constexpr int ROWS_PER_HALF = PASS_ROWS / 16;                 // rows of a pass per half-wave (16 half-waves)
    static_assert(MT % PASS_SUB == 0, "passes cover the tile");
    static_assert(A_PIECES <= 16, "at most two A pieces per wave");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
    static_assert(LDS_BYTES >= PASS_ROWS * R7_LD * 4, "epilogue scratch must fit the staging buffers");
    static_assert(LDS_BYTES >= 16 * 2 * R7_N * 4, "column-partial combine must fit the staging buffers");
};

// the same stores and loads as gemm_row.hip: outputs written once and read by a later kernel stream, the bf16 outputs are the very
// next kernel's operand, the row operands are read exactly once
#define R7_STORE(ptr, val) __builtin_nontemporal_store(val, ptr)
#define R7_STORE_LP(ptr, val) (*(ptr) = (val))
#define R7_LOAD(ptr) __builtin_nontemporal_load(ptr)

template <int MODE, int MT, bool SCALED>
__global__ void __launch_bounds__(512)
gemm_row768_kernel(const Row768Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using R = Row768Cfg<MT>;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t m0 = (int64_t)blockIdx.x * R::BM;

    f32x4 acc[MT][R7_J];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < R7_J; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- main loop: K = 64 tiles in full 128-byte lines ---------------------------------------------------------------------------
    // Every LDS-DMA piece is 8 rows x 128 B, FULL cache lines: in 16-row x 64-byte pieces (K = 32 stages, the first two forms of this
    // loop) the vector-memory path looks up twice the lines for the same bytes, and that look-up rate, not the MFMAs, set the step
    // (DESIGN.md section 35).  Lane (r8, c8) lands at row r8, 16-byte slot c8 of its piece and fetches source chunk c8 ^ swz(row),
    // swz(row) = (row >> 1) & 7 = 4 (piece & 1) + (r8 >> 1): gemm_row.hip's image.
    //
    // Two W buffers of 96 KB do not fit.  But wave w is the ONLY reader of W rows 96 w .. 96 w + 95, and it stages them itself: the W
    // panel needs no barrier at all.  Each wave reads its 12 fragments of tile t into registers, waits for them (lgkmcnt(0)) and
    // refills its own 12 KB with tile t + 1, which then lands under the MFMAs of tile t: one W buffer, used like two.  The A tile (read
    // by every wave, staged in pieces by all of them) is double buffered behind one workgroup barrier per tile.
    //   step t:  vmcnt(0) [own pieces of A(t), W(t)] ; barrier ; issue A(t+1) ; read W(t) fragments ; lgkmcnt(0) ; issue W(t+1) ;
    //            MT x (read 2 A fragments, 12 MFMAs)
    //   RAW  A(t): every wave's own wait, then the barrier, then the reads.  W(t): the reader's own wait.
    //   WAR  A buffer (t+1) & 1 was last read in step t-1, by MFMAs issued before barrier t.  W: the refill is issued after the
    //        lgkmcnt(0) that retires this wave's reads of it (the LDS-DMA comes from inline asm: the order is the program's).
    // Every wave passes the same nt barriers; nothing but the DMA issue depends on the wave.
    const int r8 = lane >> 3, c8 = lane & 7;
    const int cs_even = (c8 ^ (r8 >> 1)) * 8, cs_odd = (c8 ^ (r8 >> 1) ^ 4) * 8;
    const int nt = a.K / 64;
    // A: wave w stages pieces w and w + 8 of the tile's 2 MT (both of parity w & 1)
    const int cs_a = (wave & 1) ? cs_odd : cs_even;
    const bf16* pa[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        int64_t ar = m0 + 8 * (wave + 8 * k) + r8;
        ar = ar < a.M ? ar : a.M - 1;                           // rows past M are staged from the last row and never stored
        pa[k] = a.A + ar * a.lda + cs_a;
    }
    // W: the wave's own 12 pieces, even ones from pw_even, odd ones from pw_odd
    const bf16* pw_even = a.W + (int64_t)(96 * wave + r8) * a.ldw + cs_even;
    const bf16* pw_odd = a.W + (int64_t)(96 * wave + 8 + r8) * a.ldw + cs_odd;
    auto issue_a = [&](int t) {
        if (t >= nt) return;
        const int k0 = t * 64;
        const int seg = k0 / a.seg_k;                                         // scalar: which [M, seg_k] tensor this K-tile reads
        const int64_t ka = (int64_t)seg * a.seg_stride + (k0 - seg * a.seg_k);
        char* dst = smem + R::A_BASE + (t & 1) * R::A_BYTES + wave * 1024;
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (wave + 8 * k < R::A_PIECES) glds16_asm(pa[k] + ka, dst + k * 8192);
    };
    auto issue_w = [&](int t) {
        if (t >= nt) return;
        char* dst = smem + wave * R::W_WAVE_BYTES;
#pragma unroll
        for (int q = 0; q < R7_J; ++q) {
            glds16_asm(pw_even + (int64_t)(16 * q) * a.ldw + t * 64, dst + (2 * q) * 1024);
            glds16_asm(pw_odd + (int64_t)(16 * q) * a.ldw + t * 64, dst + (2 * q + 1) * 1024);
        }
    };
    // fragments: row (16 i + fr) of A / row (96 wave + 16 j + fr) of W, k-half kk -> 16-byte chunk 4 kk + fq; swz(row) = (fr >> 1) & 7
    const int fr = lane & 15, fq = lane >> 4;
    const int loff0 = fr * 128 + ((fq ^ ((fr >> 1) & 7)) << 4), loff1 = fr * 128 + (((4 + fq) ^ ((fr >> 1) & 7)) << 4);
    const char* sw = smem + wave * R::W_WAVE_BYTES;
    issue_a(0);
    issue_w(0);
    for (int t = 0; t < nt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();   // A(t) landed for every wave; everyone is done reading A(t-1)
        asm volatile("" ::: "memory");
        issue_a(t + 1);
        bf16x8 fb[R7_J][2];
#pragma unroll
        for (int j = 0; j < R7_J; ++j) {
            fb[j][0] = *(const bf16x8*)(sw + j * 2048 + loff0);
            fb[j][1] = *(const bf16x8*)(sw + j * 2048 + loff1);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the fragments are in registers: the wave's W rows may be refilled
        issue_w(t + 1);
        const char* sa = smem + R::A_BASE + (t & 1) * R::A_BYTES;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const bf16x8 fa0 = *(const bf16x8*)(sa + i * 2048 + loff0), fa1 = *(const bf16x8*)(sa + i * 2048 + loff1);
#pragma unroll
            for (int j = 0; j < R7_J; ++j) {  // transposed product: lane holds row (16 i + fr), columns 96 wave + 16 j + 4 fq + (0..3)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j][0], fa0, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j][1], fa1, acc[i][j], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: PASS_ROWS rows per pass through the fp32 scratch, then the LayerNorm row loop (half-wave per row) ---------------
    float* sc = (float*)smem;
    const int hl = lane & 31;
    const int hw = wave * 2 + (lane >> 5);          // half-wave 0..15: rows hw, hw + 16 of a pass
    const float inv_d = 1.0f / R7_N;
    f32x4 dg[R7_J], db[R7_J];
#pragma unroll
    for (int j = 0; j < R7_J; ++j) {
        dg[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        db[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // The per-column operands (bias, gamma, beta) are read where they are used (L1 / L2 hits, 3 KB each): held in registers next
    // to the accumulators of the passes still to come they would spill.
    // The row operand a row starts from (forward: the residual, backward: x): where the registers allow it, all of a pass's rows are
    // requested before the dump and its two barriers (a half-wave is one of only 16 per CU; gemm_row.hip measured the same).  The
    // backward of the 96-row tile has no room for it next to its column sums and fetches inside the row.
    constexpr bool PREFETCH = MODE == R7_MODE_FWD || MT == 4;
    auto fetch = [&](f32x4 (&v)[R7_J], int64_t m) {
        const float* src = MODE == R7_MODE_FWD ? a.residual + m * a.ldr : a.x + m * a.ldx;
        if (m < a.M) {                      // ONE branch around the six loads: a select per load makes hipcc wait for each in turn
#pragma unroll
            for (int j = 0; j < R7_J; ++j) v[j] = R7_LOAD((const f32x4*)(src + (j * 32 + hl) * 4));
        } else {
#pragma unroll
            for (int j = 0; j < R7_J; ++j) v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto row_fwd = [&](int r, int64_t m, f32x4 (&v)[R7_J]) {
        if (m >= a.M) return;
        float scale = 1.f;
        if constexpr (SCALED) scale = a.row_scale[m];
        f32x4 bs[R7_J];
        if (a.bias) {                       // (one branch, as in fetch)
#pragma unroll
            for (int j = 0; j < R7_J; ++j) bs[j] = *(const f32x4*)(a.bias + (j * 32 + hl) * 4);
        } else {
#pragma unroll
            for (int j = 0; j < R7_J; ++j) bs[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < R7_J; ++j) {
            const int c = (j * 32 + hl) * 4;
            f32x4 d = *(const f32x4*)(sc + r * R7_LD + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] += bs[j][e];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (SCALED) v[j][e] = v[j][e] + scale * d[e];      // the LayerNorm below sees the scaled y
                else v[j][e] = d[e] + v[j][e];
            }
            R7_STORE((f32x4*)(a.y + m * a.ldy + c), v[j]);
            s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        }
        if (!a.h) return;
        const float mu = half_wave_sum(s) * inv_d;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < R7_J; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[j][e] - mu;
                q = fmaf(d, d, q);
            }
        const float rs = rsqrtf(half_wave_sum(q) * inv_d + a.eps);
#pragma unroll
        for (int j = 0; j < R7_J; ++j) {
            const int c = (j * 32 + hl) * 4;
            const f32x4 gm = *(const f32x4*)(a.gamma + c), bt = *(const f32x4*)(a.beta + c);
            bf16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (bf16)((v[j][e] - mu) * rs * gm[e] + bt[e]);
            R7_STORE_LP((bf16x4*)(a.h + m * a.ldh + c), o);
        }
        if (hl == 0) {
            a.mean[m] = mu;
            a.rstd[m] = rs;
        }
    };
    // (the backward row keeps xhat alone across the row sums and forms dh * gamma again from the scratch and gamma afterwards: with
    // both held, the 96-row instance spills next to the column sums and the accumulators of the passes still to come)
    auto row_bwd = [&](int r, int64_t m, f32x4 (&xh)[R7_J]) {
        if (m >= a.M) return;
        const float mu = a.mean_in[m], rs = a.rstd_in[m];
        float lps = 1.f;
        if constexpr (SCALED) lps = a.lp_scale[m];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < R7_J; ++j) {
            const int c = (j * 32 + hl) * 4;
            const f32x4 d = *(const f32x4*)(sc + r * R7_LD + c);
            const f32x4 gm = *(const f32x4*)(a.gamma + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xh[j][e] = (xh[j][e] - mu) * rs;
                const float g = d[e] * gm[e];
                s1 += g;
                s2 = fmaf(g, xh[j][e], s2);
                dg[j][e] = fmaf(d[e], xh[j][e], dg[j][e]);
                db[j][e] += d[e];
            }
        }
        const float c1 = half_wave_sum(s1) * inv_d, c2 = half_wave_sum(s2) * inv_d;
        asm volatile("" ::: "memory");        // the second read of the scratch stays a read: not a value kept from the first
        auto write = [&](auto has_in) {      // ONE branch on dx_in around the whole sweep, not a select per load (see row_fwd)
#pragma unroll
            for (int j = 0; j < R7_J; ++j) {
                const int c = (j * 32 + hl) * 4;
                const f32x4 d = *(const f32x4*)(sc + r * R7_LD + c);
                const f32x4 gm = *(const f32x4*)(a.gamma + c);
                f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (decltype(has_in)::value) v = R7_LOAD((const f32x4*)(a.dx_in + m * a.ldxi + c));
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = rs * (d[e] * gm[e] - c1 - xh[j][e] * c2) + v[e];
                R7_STORE((f32x4*)(a.dx + m * a.lddx + c), v);
                if constexpr (SCALED) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] *= lps;
                }
                if (a.dx_lp) R7_STORE_LP((bf16x4*)(a.dx_lp + m * a.ldlp + c), (bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]}));
            }
        };
        if (a.dx_in) write(std::true_type{});
        else write(std::false_type{});
    };

#pragma unroll
    for (int p = 0; p < R::NPASS; ++p) {
        const int64_t mp = m0 + p * R::PASS_ROWS;
        f32x4 pre[R::ROWS_PER_HALF][R7_J];
        if constexpr (PREFETCH) {
#pragma unroll
            for (int k = 0; k < R::ROWS_PER_HALF; ++k) fetch(pre[k], mp + hw + 16 * k);
        }
        __syncthreads();       // every wave is done with the LDS (main loop's last stage / the previous pass's rows)
#pragma unroll
        for (int ii = 0; ii < R::PASS_SUB; ++ii) {
            const int i = R::PASS_SUB * p + ii;
#pragma unroll
            for (int j = 0; j < R7_J; ++j) *(f32x4*)(sc + (ii * 16 + fr) * R7_LD + wave * 96 + j * 16 + fq * 4) = acc[i][j];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < R::ROWS_PER_HALF; ++k) {
            const int r = hw + 16 * k;
            if constexpr (!PREFETCH) fetch(pre[k], mp + r);
            if constexpr (MODE == R7_MODE_FWD) row_fwd(r, mp + r, pre[k]);
            else row_bwd(r, mp + r, pre[k]);
        }
    }

    if (MODE == R7_MODE_BWD) {
        // the 16 half-waves' column partials -> one [2][768] row per workgroup (summed over workgroups by ln_bwd_finish)
        __syncthreads();
        float* my = sc + hw * 2 * R7_N;
#pragma unroll
        for (int j = 0; j < R7_J; ++j) {
            const int c = (j * 32 + hl) * 4;
            *(f32x4*)(my + c) = dg[j];
            *(f32x4*)(my + R7_N + c) = db[j];
        }
        __syncthreads();
        float* out = a.partial + (int64_t)blockIdx.x * 2 * R7_N;
        for (int c = threadIdx.x; c < 2 * R7_N; c += 512) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < 16; ++w) s += sc[w * 2 * R7_N + c];
            out[c] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------
static inline int row768_mt(int64_t M) {
    // rounds of 256 workgroups (one per CU) x rows per tile: the smallest makespan wins, the taller tile on a tie (the W panel is
    // staged once per tile).  13,824 rows (24 images of 576 tokens) = 216 x 64 (one round, where 144 x 96 leaves 112 CUs idle);
    // 41,544 (72 pairs of 577) = 433 x 96 (two rounds, where 650 x 64 needs three).
    static const int heights[] = {6, 4};
    int best = 6;
    int64_t cost = -1;
    for (int mt : heights) {
        const int64_t c = ceil_div64(ceil_div64(M, 16 * mt), 256) * mt;
        if (cost < 0 || c < cost) {
            cost = c;
            best = mt;
        }
    }
    return best;
}

int64_t row768_tiles(int64_t M) { return ceil_div64(M, 16 * row768_mt(M)); }

// What the kernels compute (the entries' shape check).  K >= 768: every Linear of a 768-wide model on the residual stream has K in
// {768, 1536, 2304, 3072, c_depth x 1536}.
bool row768_shape_ok(int64_t M, int64_t N, int64_t K) {
    return N == R7_N && K >= 768 && K % 64 == 0 && K <= (1 << 20) && M >= 1 && M < ((int64_t)1 << 31);
}

// Where they are FASTER than vited_gemm + vited_layernorm_fwd / _bwd, the part of vited_linear_layernorm_supported that speaks of
// speed (measured at a ViT-Base step's shapes: profiles/row768_probe.py; a class is in only where the fused
// kernel's whole range lay below the two-kernel form's):
//  * more rows than one round of 96-row tiles (M > 24,576).  At 13,824 rows - one partial round of 64-row tiles - the backward is
//    3 - 7 % slower at every K and the forward ties at K = 3072;
//  * K is not N or 4 N: the contractions of the FORWARD Linears on the residual stream (proj / cross-proj, fc2), whose fused form only
//    ties at 41,544 rows.  The predicate does not know the mode, so the backward products with those K (q, fc1) stay with the two
//    kernels too, although their fused form is 9 - 16 % faster there.
bool row768_pays(int64_t M, int64_t K) { return M > 256 * 96 && K != R7_N && K != 4 * R7_N; }

template <int MODE, int MT, bool SCALED>
static int row768_launch_scaled(const Row768Args& a, unsigned tiles, hipStream_t s) {
    auto kernel = gemm_row768_kernel<MODE, MT, SCALED>;
    static std::once_flag once;          // dynamic LDS above 64 KB needs the opt-in, once per kernel instance
    static hipError_t status = hipSuccess;
    std::call_once(once, [&] { status = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, Row768Cfg<MT>::LDS_BYTES); });
    if (status != hipSuccess) return VITED_ERR_LAUNCH;
    hipLaunchKernelGGL(kernel, dim3(tiles), dim3(512), Row768Cfg<MT>::LDS_BYTES, s, a);
    return vited_check_launch();
}

// a null scale takes the unscaled instance: the code of a model without stochastic depth
template <int MODE, int MT>
static int row768_launch_mt(const Row768Args& a, unsigned tiles, hipStream_t s) {
    if (MODE == R7_MODE_FWD ? a.row_scale != nullptr : a.lp_scale != nullptr) return row768_launch_scaled<MODE, MT, true>(a, tiles, s);
    return row768_launch_scaled<MODE, MT, false>(a, tiles, s);
}

template <int MODE>
static int row768_launch(const Row768Args& a, hipStream_t s) {
    const unsigned tiles = (unsigned)row768_tiles(a.M);
    switch (row768_mt(a.M)) {
        case 4: return row768_launch_mt<MODE, 4>(a, tiles, s);
        default: return row768_launch_mt<MODE, 6>(a, tiles, s);
    }
}

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int row768_fwd(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, const float* residual, int64_t ldr,
               const float* row_scale, float* y, int64_t ldy, const float* gamma, const float* beta, float eps, void* h, int64_t ldh,
               float* mean, float* rstd, int64_t M, int64_t N, int64_t K, void* stream) {
    if (!a || !w || !residual || !y || M <= 0 || N <= 0 || K <= 0 || lda < K || ldw < K || ldr < N || ldy < N) return VITED_ERR_BAD_ARG;
    if (h && (!gamma || !beta || !mean || !rstd || ldh < N)) return VITED_ERR_BAD_ARG;
    if (!row768_shape_ok(M, N, K)) return VITED_ERR_UNSUPPORTED;
    if ((lda & 7) || (ldw & 7) || (ldr & 3) || (ldy & 3) || (h && (ldh & 3))) return VITED_ERR_UNSUPPORTED;
    if (!al16(a) || !al16(w) || !al16(residual) || !al16(y) || !al16(bias) || !al16(gamma) || !al16(beta) || ((uintptr_t)h & 7))
        return VITED_ERR_BAD_ARG;
    Row768Args r = {};
    r.A = (const bf16*)a; r.lda = lda; r.seg_k = (int)K; r.seg_stride = 0; r.W = (const bf16*)w; r.ldw = ldw; r.M = M; r.K = (int)K;
    r.bias = bias; r.residual = residual; r.ldr = ldr; r.y = y; r.ldy = ldy;
    r.gamma = gamma; r.beta = beta; r.eps = eps; r.h = (bf16*)h; r.ldh = ldh; r.mean = mean; r.rstd = rstd;
    r.row_scale = row_scale;
    return row768_launch<R7_MODE_FWD>(r, (hipStream_t)stream);
}

// layernorm.hip
int ln_bwd_finish(const float* partial, int nparts, int dim, float* dgamma, float* dbeta, int accumulate, hipStream_t s);

int row768_bwd(const void* dy, int64_t lddy, int64_t seg_k, int64_t seg_stride, const void* wt, int64_t ldwt, const float* x, int64_t ldx,
               const float* gamma, const float* mean, const float* rstd, const float* dx_in, int64_t dx_in_ld, float* dx_out,
               int64_t dx_out_ld, void* dx_lp, int64_t dx_lp_ld, const float* lp_scale, float* dgamma, float* dbeta, int accumulate,
               int64_t M, int64_t N, int64_t K, float* workspace, int64_t workspace_bytes, void* stream) {
    if (lp_scale && !dx_lp) return VITED_ERR_BAD_ARG;
    if (!dy || !wt || !x || !gamma || !mean || !rstd || !dx_out || M <= 0 || N <= 0 || K <= 0) return VITED_ERR_BAD_ARG;
    if ((dgamma == nullptr) != (dbeta == nullptr)) return VITED_ERR_BAD_ARG;
    if (seg_k <= 0 || K % seg_k || lddy < seg_k || ldwt < K || ldx < N || dx_out_ld < N || (dx_in && dx_in_ld < N) || (dx_lp && dx_lp_ld < N))
        return VITED_ERR_BAD_ARG;
    if (!row768_shape_ok(M, N, K) || seg_k % 64 || (seg_stride & 7)) return VITED_ERR_UNSUPPORTED;
    if ((lddy & 7) || (ldwt & 7) || (ldx & 3) || (dx_out_ld & 3) || (dx_in && (dx_in_ld & 3)) || (dx_lp && (dx_lp_ld & 3))) return VITED_ERR_UNSUPPORTED;
    if (!al16(dy) || !al16(wt) || !al16(x) || !al16(gamma) || !al16(dx_in) || !al16(dx_out) || ((uintptr_t)dx_lp & 7)) return VITED_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < row768_tiles(M) * 2 * R7_N * (int64_t)sizeof(float)) return VITED_ERR_WORKSPACE;
    Row768Args r = {};
    r.A = (const bf16*)dy; r.lda = lddy; r.seg_k = (int)seg_k; r.seg_stride = seg_stride; r.W = (const bf16*)wt; r.ldw = ldwt; r.M = M; r.K = (int)K;
    r.gamma = gamma; r.x = x; r.ldx = ldx; r.mean_in = mean; r.rstd_in = rstd;
    r.dx_in = dx_in; r.ldxi = dx_in_ld; r.dx = dx_out; r.lddx = dx_out_ld; r.dx_lp = (bf16*)dx_lp; r.ldlp = dx_lp_ld;
    r.partial = workspace;
    r.lp_scale = lp_scale;
    const int rc = row768_launch<R7_MODE_BWD>(r, (hipStream_t)stream);
    if (rc != VITED_OK || !dgamma) return rc;     // dgamma == null: the caller keeps the partials and finishes several LayerNorms at once
    return ln_bwd_finish(workspace, (int)row768_tiles(M), R7_N, dgamma, dbeta, accumulate, (hipStream_t)stream);
}
