// NT GEMM for K = 384 with the A operand held in registers:  out = epilogue(A[M,384] . W[N,384]^T),  N % 128 == 0.
//
// Why: gemm_nt_mfma_kernel runs one workgroup per 256 x 128 output tile, so the N / 128 workgroups of one row block each pull the
// same 256 x 384 A panel L2 -> LDS and read it back as fragments: two thirds of the bytes that kernel stages (DESIGN.md section 5,
// round 4).  At K = 384 a wave's whole A operand for 32 rows is 2 row tiles x 12 K-steps x one bf16x8 = 96 VGPRs, so here every
// wave loads its A fragments ONCE, straight from global memory in the MFMA ownership (row = lane & 15, k-chunk = lane >> 4), and
// walks over the n-tiles of its row panel while only W goes through LDS.
//
// Geometry (template WAVES = 8 | 4): a workgroup owns a 32 * WAVES row panel; each wave a 32-row x 128-column tile = 2 x 8
// v_mfma_f32_16x16x32_bf16 accumulators, every element summed over k = 0, 32, ..., 352 in ascending order exactly as
// gemm_nt_mfma_kernel does, so the fp32 accumulators (and, through the shared epilogue code, the outputs) are bit-identical.
// Work split: the (row panel, n-tile) items, panel-major, are dealt in contiguous equal shares (+-1) to a launch of exactly the
// resident workgroup slots; a share that crosses into the next panel reloads A there.  xcd_remap keeps neighbouring shares on
// one XCD.
//
// W ring: a chunk = [128 n][64 k] of W = 16 KB in the BK = 64 swizzled image of gemm_lds.h (every LDS-DMA piece is 8 rows x 128 B,
// full cache lines), 6 chunks per item, S slots (6 with 8 waves = the whole W tile; 3 with 4 waves and under the 8-wave multiply
// epilogue; S divides 6, so a chunk's slot is its k-chunk % S), and the chunk sequence runs ACROSS items: step q of the workgroup's share (step = one chunk) issues chunk
// q + S - 1 behind its barrier, so S - 2 later chunks are in flight while chunk q is waited for - also under the epilogue, whose
// scratch is therefore a region of its own behind the ring.
// Synchronisation (inline-asm LDS-DMA, counted vmcnt, raw s_barrier; one barrier per chunk = per 32 MFMAs of a wave):
//   RAW: before barrier q every wave waits for its OWN pieces of chunk q: vmcnt(n) with n = the vector memory instructions it has
//        issued AFTER that chunk - vmcnt retires in issue order, loads and stores alike, on gfx9.  These are the PER LDS-DMA pieces
//        of each later chunk and, where the chunk was issued before the previous item's epilogue (k-chunk < S - 1), that epilogue's
//        stores (and multiplier loads): counted, they drain under this item's MFMAs instead of stalling its first barrier.  The
//        epilogue count E is exact only when no row of the wave tile is masked (rows >= M skip their accesses), so it is added only
//        for full wave tiles (wave-uniform); a smaller n only waits for more, never for less.  The compiler's own waits (A
//        fragments, multiplier rows) count only its own operations and are conservative for the same reason: the LDS-DMA it does
//        not see is older or extra.  E is checked against the ISA: 8 / 16 global stores per item (plain / GELU'), 8 stores + 8
//        multiplier loads (MUL; with 8 waves the 8 loads are LDS-DMA pieces that always issue, counted apart as AUXN).
//        The multiply epilogue's operand is the one HBM read of the epilogue: loaded where it is used, its latency is exposed
//        four times per item (dz 113 us at M = 65,536); as LDS-DMA issued an epilogue and S - 1 steps ahead, 93 us (issue_aux).
//   WAR: chunk q + S - 1 overwrites the slot of chunk q - 1 and is issued behind barrier q; every wave reaches that barrier after
//        the lgkmcnt(0) that retires its fragment reads of chunk q - 1 (the wait in front of the barrier).
//   The invariant E is a property of the compiled code, not of the source: `make check-k384` (csrc/Makefile) recompiles this file
//   with --save-temps and fails unless every gemm_nt_areg_kernel instance holds exactly the expected number of global stores
//   (all of them in the item loop's epilogue: 8, or 16 under GELU') and no scratch.  Run it after a compiler or epilogue change.
// Only vector memory instructions are used.
#include <mutex>
#include <type_traits>

#include "gemm_kernels.h"
#include "gemm_nt_epilogue.h"
#include "gemm_lds.h"

#define NT_AREG_CHUNK_BYTES (128 * 128)       // [128 n][64 k] bf16
#define NT_AREG_KSTEPS 12                     // K = 384
#define NT_AREG_MAX_N 2048                    // the bias vector's LDS image

// ring slots: the whole W tile with one 8-wave workgroup per CU (139 KB with scratch and bias), three chunks with two 4-wave
// workgroups per CU (73 KB each) and under the 8-wave multiply epilogue (155 KB with the multiplier rows)
static constexpr __host__ __device__ int nt_areg_slots(int waves, int epi) { return waves == 8 && epi != VITED_EPI_MUL ? 6 : 3; }
// EPI_MUL with 8 waves: the 32 x 128 multiplier rows of a wave's NEXT item go global -> LDS by LDS-DMA during the current item's
// epilogue (8 KB per wave behind the bias; the ring then has three slots) and are read back in that item's epilogue: held in
// registers across the MFMAs they do not fit (32 VGPRs), fetched in the epilogue their HBM latency is exposed four times per item
static constexpr __host__ __device__ bool nt_areg_aux_lds(int waves, int epi) { return waves == 8 && epi == VITED_EPI_MUL; }
#define NT_AREG_AUX_BYTES (32 * 128 * 2)
static constexpr __host__ __device__ int nt_areg_lds_bytes(int waves, int epi) {
    return nt_areg_slots(waves, epi) * NT_AREG_CHUNK_BYTES + waves * SCRATCH_BYTES + NT_AREG_MAX_N * 4 +
           (nt_areg_aux_lds(waves, epi) ? waves * NT_AREG_AUX_BYTES : 0);
}

template <int EPI, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(2, 2)))
gemm_nt_areg_kernel(const bf16* __restrict__ A, int64_t lda, const bf16* __restrict__ W, int64_t ldw, int64_t M, int64_t N,
                    int tiles_n, int nitems, EpiParams ep) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using C = NtCfg<64>;
    constexpr int PM = 32 * WAVES;                 // rows of a panel
    constexpr int PER = 16 / WAVES;                // LDS-DMA instructions per chunk per wave (8 rows each)
    constexpr int S = nt_areg_slots(WAVES, EPI), D = S - 1;   // ring slots; chunk q is issued in step q - D
    constexpr bool AUX_LDS = nt_areg_aux_lds(WAVES, EPI);
    static_assert(!AUX_LDS || D < 6, "a chunk issued behind the multiplier rows must be waited for before the epilogue");
    // vector memory instructions of one item's epilogue (4-wave MUL: with the next item's first multiplier loads)
    constexpr int E = EPI == VITED_EPI_STORE || AUX_LDS ? 8 : 16;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fq = lane >> 4;

    const int share = xcd_remap(blockIdx.x, gridDim.x);
    const int begin = (int)((int64_t)share * nitems / gridDim.x), end = (int)((int64_t)(share + 1) * nitems / gridDim.x);
    if (begin >= end) return;                      // whole workgroup: no barrier is left waiting

    // ---- W loader: this wave's PER pieces of a chunk; element offset of the lane inside the n-tile (row r, swizzled source chunk)
    unsigned woff[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int r = (wave * PER + j) * 8 + (lane >> 3);
        woff[j] = (unsigned)r * (unsigned)ldw + (unsigned)(((lane & 7) ^ C::swz(r)) << 3);
    }
    auto issue = [&](int nt, int kc) {             // chunk kc of n-tile nt into slot kc % S
        const bf16* base = W + (int64_t)nt * 128 * ldw + kc * 64;
        char* dst = smem + (kc % S) * NT_AREG_CHUNK_BYTES + wave * PER * 1024;
#pragma unroll
        for (int j = 0; j < PER; ++j) glds16_asm(base + woff[j], dst + j * 1024);
    };
    // ---- W fragment reads: row j * 16 + fr, chunk kk * 4 + fq; (row >> 1) & 7 = fr >> 1 for every j
    int boff[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) boff[kk] = C::off(fr, kk * 4 + fq);
    float* sc = (float*)(smem + S * NT_AREG_CHUNK_BYTES + wave * SCRATCH_BYTES);
    // the bias vector (zeros without one) sits in LDS for the whole launch: read from global memory in the epilogue, its vmcnt
    // wait would drain the ring once per item.  Visible to every wave behind the first chunk barrier.
    float* sbias = (float*)(smem + S * NT_AREG_CHUNK_BYTES + WAVES * SCRATCH_BYTES);
    for (int n = threadIdx.x; n < (int)N; n += 64 * WAVES) sbias[n] = ep.bias ? ep.bias[n] : 0.f;
    char* saux = smem + S * NT_AREG_CHUNK_BYTES + WAVES * SCRATCH_BYTES + NT_AREG_MAX_N * 4 + wave * NT_AREG_AUX_BYTES;

    // AUX_LDS: piece (sub-tile s, pc) of an item's multiplier rows = 8 rows x 128 B in the epilogue's ownership (row = lane >> 3, 8
    // columns at (lane & 7) * 8), lane-linear in LDS; rows >= M are clamped (their products are never stored), so all 8 instructions
    // always issue.  The pieces of item i + 1 are issued in the epilogue of item i, as soon as item i's have been read into registers
    // and in front of its stores: they then have an epilogue and D steps to come from HBM before the first wait that includes them
    // (vmcnt retires in order: chunk D of item i + 1, issued behind them in its step 0, is certified in step D, before its epilogue).
    auto issue_aux = [&](int panel_, int nt_) {
        const int64_t mt_ = (int64_t)panel_ * PM + wave * 32, n0_ = (int64_t)nt_ * 128;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int pc = 0; pc < 2; ++pc) {
                int64_t m = mt_ + (s & 1) * 16 + pc * 8 + (lane >> 3);
                m = m < M ? m : M - 1;
                glds16_asm((const bf16*)ep.aux + m * ep.ldo + n0_ + (s >> 1) * 64 + (lane & 7) * 8, saux + (s * 2 + pc) * 1024);
            }
    };
    int panel = begin / tiles_n, nt = begin - panel * tiles_n;
    int loaded = -1;
    bf16x8 a[2][NT_AREG_KSTEPS];
#pragma unroll
    for (int kc = 0; kc < D; ++kc) issue(nt, kc);
    if constexpr (AUX_LDS) issue_aux(panel, nt);
    bool prev_full = false;                        // the previous item's epilogue ran on a wave tile with no masked row
    for (int it = begin; it < end; ++it) {
        if (panel != loaded) {                     // wave-uniform: the first item, and a share that crosses into the next panel
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int64_t gm = (int64_t)panel * PM + wave * 32 + i * 16 + fr;
                gm = gm < M ? gm : M - 1;
                const bf16* arow = A + gm * lda + fq * 8;
#pragma unroll
                for (int ks = 0; ks < NT_AREG_KSTEPS; ++ks) a[i][ks] = *(const bf16x8*)(arow + ks * 32);
            }
            // drained here, once per panel, with a wait the compiler sees: left to its own bookkeeping it spreads vmcnt(23) ...
            // vmcnt(0) over the chunk loop of EVERY item, and those counts drain the W ring
            __builtin_amdgcn_s_waitcnt(0x0f70);    // vmcnt(0)
            loaded = panel;
        }
        int next_nt = nt + 1, next_panel = panel;
        if (next_nt == tiles_n) {
            next_nt = 0;
            ++next_panel;
        }
        const bool has_next = it + 1 < end;

        const int64_t mt = (int64_t)panel * PM + wave * 32, n0 = (int64_t)nt * 128;
        const bool full = mt + 32 <= M;
        const bool counted = prev_full && full;    // E more instructions sit behind the chunks issued before the last epilogue
        EpiPrefetch<EPI> pf[2];
        // the multiplier rows of the first sub-tile are fetched under the item's MFMAs, the other three at the start of the epilogue
        // (the W fragments' registers are free by then; all four held across the loop spill)
        if constexpr (EPI == VITED_EPI_MUL && !AUX_LDS) epilogue_prefetch_subtile<EPI>(ep, pf[0], 0, mt, n0, M, N, lane);
        f32x4 acc[2][8];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

        auto step = [&](auto kc_) {
            constexpr int kc = decltype(kc_)::value;
            // LDS-DMA chunks issued after chunk kc when its wait is reached: by the steps of the previous item (or the prologue)
            // behind the one that issued it, and by this item's steps lo .. kc - 1, of which those with s + D >= 6 reach into
            // the next item and issue only if there is one
            constexpr int lo = kc < D ? 0 : kc - D + 1;
            constexpr int before = kc < D ? D - kc - 1 : 0;
            constexpr int n_next = before + (kc - lo);
            constexpr int n_last = before + ((6 - D < kc ? 6 - D : kc) > lo ? (6 - D < kc ? 6 - D : kc) - lo : 0);
            // the item's 8 multiplier pieces sit behind the chunks issued before the previous epilogue (or in the prologue)
            constexpr int AUXN = AUX_LDS && kc < D ? 8 : 0;
            if (has_next) {
                if (kc < D && counted) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(n_next * PER + AUXN + E) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(n_next * PER + AUXN) : "memory");
            } else {
                if (kc < D && counted) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(n_last * PER + AUXN + E) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(n_last * PER + AUXN) : "memory");
            }
            __builtin_amdgcn_s_barrier();          // chunk kc landed for every wave; everyone is done reading the chunk before it
            asm volatile("" ::: "memory");
#ifndef NT_DBG_NO_W_DMA
            if constexpr (kc + D < 6) issue(nt, kc + D);
            else if (has_next) issue(next_nt, kc + D - 6);
#endif
            const char* sb = smem + (kc % S) * NT_AREG_CHUNK_BYTES;
            // The 8 W fragments of a K-step are requested as two groups of four, each one group of 8 MFMAs ahead of its use, and
            // the order is pinned: left to itself hipcc keeps two fragments live and waits lgkmcnt(0) in front of every 4 MFMAs.
            bf16x8 bfr[8];
            auto read4 = [&](int kk, int g) {
#pragma unroll
                for (int j = 0; j < 4; ++j) bfr[g * 4 + j] = *(const bf16x8*)(sb + (g * 4 + j) * 16 * C::ROW_BYTES + boff[kk]);
            };
            auto mfma8 = [&](int kk, int g) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        acc[i][g * 4 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][kc * 2 + kk], bfr[g * 4 + j], acc[i][g * 4 + j], 0, 0, 0);
            };
            read4(0, 0);
            read4(0, 1);
            __builtin_amdgcn_sched_barrier(0);
            mfma8(0, 0);
            __builtin_amdgcn_sched_barrier(0);
            read4(1, 0);
            __builtin_amdgcn_sched_barrier(0);
            mfma8(0, 1);
            __builtin_amdgcn_sched_barrier(0);
            read4(1, 1);
            __builtin_amdgcn_sched_barrier(0);
            mfma8(1, 0);
            mfma8(1, 1);
        };
        step(std::integral_constant<int, 0>{});
        step(std::integral_constant<int, 1>{});
        step(std::integral_constant<int, 2>{});
        step(std::integral_constant<int, 3>{});
        step(std::integral_constant<int, 4>{});
        step(std::integral_constant<int, 5>{});

#ifdef NT_DBG_NO_EPI
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) asm volatile("" ::"v"(acc[i][j]));
#else
        // ---- epilogue (gemm_nt_epilogue.h): the 32 x 128 wave tile as two 64-column halves x two 16-row sub-tiles through the
        // wave-private scratch, operands fetched one sub-tile ahead
        if constexpr (AUX_LDS) {
            // landed: chunk D of the item was issued, and has been waited for, behind them
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int pc = 0; pc < 2; ++pc) pf[s >> 1].aux[s & 1][pc] = *(const bf16x8*)(saux + (s * 2 + pc) * 1024 + lane * 16);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // WAR: the next item's pieces overwrite what was just read
            if (has_next) issue_aux(next_panel, next_nt);
        } else if constexpr (EPI == VITED_EPI_MUL) {
            epilogue_prefetch_subtile<EPI>(ep, pf[0], 1, mt, n0, M, N, lane);
            epilogue_prefetch_subtile<EPI>(ep, pf[1], 0, mt, n0 + 64, M, N, lane);
            epilogue_prefetch_subtile<EPI>(ep, pf[1], 1, mt, n0 + 64, M, N, lane);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float* bp = sbias + n0 + h * 64 + EpiTraits<EPI>::col(lane);
            pf[h].bias[0] = *(const f32x4*)bp;
            pf[h].bias[1] = *(const f32x4*)(bp + 4);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int h = s >> 1, i = s & 1;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) sc[(fq * 4 + e) * SCRATCH_LD + j * 16 + fr] = acc[i][h * 4 + j][e];
            // the scratch is wave-private and a wave's DS operations execute in order: only the compiler needs a fence
            asm volatile("" ::: "memory");
            epilogue_subtile<EPI>(ep, pf[h], sc, i, mt, n0 + h * 64, M, N, lane);
            asm volatile("" ::: "memory");
        }
#endif
        prev_full = full;
        panel = next_panel;
        nt = next_nt;
    }
}

bool gemm_nt_areg_supported(int64_t ldw, int64_t M, int64_t N, int64_t K, int epilogue) {
    if (epilogue != VITED_EPI_STORE && epilogue != VITED_EPI_MUL && epilogue != VITED_EPI_GELU_GRAD) return false;
    if (K != 32 * NT_AREG_KSTEPS || N % 128 || N < 768 || M < 8192) return false;
    // 32-bit arithmetic of the kernel: W offsets inside an n-tile, the item count
    return ldw < (1 << 20) && N <= NT_AREG_MAX_N && ceil_div64(M, 128) * (N / 128) < (1 << 30);
}

template <int EPI, int WAVES>
static int launch_areg(const bf16* a, int64_t lda, const bf16* w, int64_t ldw, int64_t M, int64_t N, const EpiParams& ep, hipStream_t s) {
    // ring + per-wave epilogue scratch + bias: 139 KB (8 waves, one workgroup per CU) / 73 KB (4 waves, two per CU)
    constexpr int LDS = nt_areg_lds_bytes(WAVES, EPI);
    auto kernel = gemm_nt_areg_kernel<EPI, WAVES>;
    static std::once_flag once;
    static hipError_t status = hipSuccess;
    std::call_once(once, [&] { status = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS); });
    if (status != hipSuccess) return VITED_ERR_LAUNCH;
    const int tiles_n = (int)(N / 128);
    const int nitems = (int)ceil_div64(M, 32 * WAVES) * tiles_n;
    const int slots = WAVES == 8 ? 256 : 512;      // resident workgroups of the chip: one launch round
    const int grid = nitems < slots ? nitems : slots;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * WAVES), LDS, s, a, lda, w, ldw, M, N, tiles_n, nitems, ep);
    return VITED_OK;
}

int gemm_nt_areg(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N, int epilogue, int waves,
                 const EpiParams& ep, hipStream_t s) {
    const bf16* a = (const bf16*)A;
    const bf16* w = (const bf16*)W;
    if (waves != 4 && waves != 8) return VITED_ERR_BAD_ARG;
    // the product build carries the two instances its dispatch takes; experiment builds all six (both geometries, three epilogues)
    if (epilogue == VITED_EPI_MUL && waves == 8) return launch_areg<VITED_EPI_MUL, 8>(a, lda, w, ldw, M, N, ep, s);
    if (epilogue == VITED_EPI_STORE && waves == 4) return launch_areg<VITED_EPI_STORE, 4>(a, lda, w, ldw, M, N, ep, s);
#ifdef VITED_TUNING
    switch (epilogue) {
        case VITED_EPI_STORE: return launch_areg<VITED_EPI_STORE, 8>(a, lda, w, ldw, M, N, ep, s);
        case VITED_EPI_MUL: return launch_areg<VITED_EPI_MUL, 4>(a, lda, w, ldw, M, N, ep, s);
        case VITED_EPI_GELU_GRAD:
            return waves == 8 ? launch_areg<VITED_EPI_GELU_GRAD, 8>(a, lda, w, ldw, M, N, ep, s)
                              : launch_areg<VITED_EPI_GELU_GRAD, 4>(a, lda, w, ldw, M, N, ep, s);
        default: break;
    }
#endif
    return VITED_ERR_UNSUPPORTED;
}
