// NT GEMM for K = 384 and 384-column groups with the WEIGHTS held in registers:
//   out[g] = A[M,384] . W[g * 384 : (g + 1) * 384, 384]^T (+ bias),  g < groups,  bf16 operands, fp32 accumulation, bf16 plain stores.
//
// Why: at N = 384 the tile kernel (gemm_nt_mfma_kernel) spends 48 MFMAs per wave behind a cold pipeline fill and an epilogue, 1,536
// times per launch, and every workgroup re-stages a 128 x 384 slice of W and of A (302 MB staged for 100 MB of traffic at
// M = 65,536); the A-in-registers kernel (gemm_nt_k384.hip) does not amortise its A load over three n-tiles.  The operand that is
// small and the same for every row is W: one group is 288 KB, 144 VGPRs per lane when 8 waves take 48 columns each.  Here a
// persistent workgroup loads its group's W ONCE, straight from global memory in the MFMA ownership (row = lane & 15,
// k-chunk = lane >> 4, the way gemm_nt_k384.hip loads A), keeps the bias in registers, and then only streams A through LDS and
// the result out.  With the group as a second work dimension one launch covers the qkv projection (three groups) and the decoder's
// stacked kv projection (2 L groups, functions.py: rt.kv_one_launch).
//
// Geometry: one 8-wave workgroup per CU.  Wave w owns columns 48 w .. 48 w + 47 of its group = 3 n-tiles x 12 K-steps of bf16x8
// fragments.  A step of the workgroup is a 32-row tile of A (two 16-row units of gemm_nt_wreg_split.h; a share of odd length ends
// with a half-used tile): 2 x 3 v_mfma_f32_16x16x32_bf16 accumulators per wave, the activation fragment as the A operand and the
// weight fragment as the B operand, every element summed over k = 0, 32, ..., 352 in ascending order exactly as
// gemm_nt_mfma_kernel and gemm_nt_areg_kernel do, and the same fp32 `acc + bias` (zero without one) rounded once to bf16: the
// outputs are bit-identical to theirs.
//
// A ring: a tile = [32 rows][384 k] = 24 KB as six [32][64] chunks in the BK = 64 swizzled image of gemm_lds.h; every LDS-DMA piece
// is 8 rows x 128 B (full cache lines), 24 pieces per tile, 3 per wave.  S = 5 slots (120 KB); tile t + S - 1 is issued behind
// the first barrier of step t.  Every wave reads its fragments with ds_read_b128, two K-steps ahead of the MFMAs that use them.
// Output: the 32 x 384 results go as bf16 into one LDS staging tile (rows padded to 784 B: the four row groups of a wave's
// fragment then fall on disjoint banks) and leave as full 768-byte rows of 16-byte stores, plain and cached like the tile
// kernel's EPI_STORE (the next kernel reads them).  Rows >= M are clamped on load and never stored; neither are the rows of a
// half-used tile that belong to the next share.
//
// Synchronisation (inline-asm LDS-DMA, counted vmcnt, raw s_barrier; two barriers per step, both in workgroup-uniform control
// flow; a workgroup with an empty share returns before the first):
//   RAW, ring:    before barrier 1 of step t every wave waits for its OWN pieces of tile t: vmcnt(3 n) with n = the tiles it has
//                 issued after tile t.  vmcnt retires in issue order, loads and stores alike, and ONLY the LDS-DMA pieces are
//                 counted: the output stores issued in between make the wait cover more, never less, so the count does not
//                 depend on how the stores compile.
//   WAR, ring:    tile t + S - 1 overwrites the slot of tile t - 1 and is issued behind barrier 1 of step t, which every wave
//                 reaches after the lgkmcnt(0) that retires its fragment reads of tile t - 1.
//   RAW, staging: lgkmcnt(0) + barrier 2 between the ds_writes and the row reads.
//   WAR, staging: step t + 1 writes the staging tile behind its barrier 1, which every wave reaches after the lgkmcnt(0) that
//                 retires its row reads of step t.
// Only vector memory instructions are used.
#include <mutex>

#include "gemm_kernels.h"
#include "gemm_lds.h"
#include "gemm_nt_wreg_split.h"

#define WREG_KSTEPS 12                          // K = 384
#define WREG_N 384                              // columns of a group
#define WREG_TILE_ROWS (2 * WREG_UNIT_ROWS)
#define WREG_CHUNK_BYTES (WREG_TILE_ROWS * 128) // [32 rows][64 k] bf16
#define WREG_TILE_BYTES (6 * WREG_CHUNK_BYTES)
#define WREG_SLOTS 5
#define WREG_STAGE_LD 784                       // bytes per staged output row: 768 + 16
#define WREG_STAGE_BYTES (WREG_TILE_ROWS * WREG_STAGE_LD)
#define WREG_LDS_BYTES (WREG_SLOTS * WREG_TILE_BYTES + WREG_STAGE_BYTES)   // 147,968 of the CU's 163,840
#define WREG_SLOTS_RESIDENT 256                 // one 8-wave workgroup per CU: one launch round

__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
gemm_nt_wreg_kernel(const bf16* __restrict__ A, int64_t lda, const bf16* __restrict__ W, int64_t ldw, const float* __restrict__ bias,
                    bf16* __restrict__ out, int64_t ldo, int64_t M, int per, int units, int groups_inner, int64_t group_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using C = NtCfg<64>;
    constexpr int S = WREG_SLOTS;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fq = lane >> 4;

    const WregShare sh = wreg_share((int)blockIdx.x, per, units);
    if (sh.unit_begin >= sh.unit_end) return;      // whole workgroup: no barrier is left waiting
    const int64_t row_begin = (int64_t)sh.unit_begin * WREG_UNIT_ROWS;
    const int64_t row_stop = (int64_t)sh.unit_end * WREG_UNIT_ROWS;
    const int64_t row_end = row_stop < M ? row_stop : M;
    const int nsteps = (sh.unit_end - sh.unit_begin + 1) >> 1;

    // ---- A loader: piece p = 3 wave + j of a tile is row block p & 3 of chunk p >> 2; the lane's row and swizzled source chunk
    int arow[3], acol[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int p = wave * 3 + j;
        arow[j] = (p & 3) * 8 + (lane >> 3);
        acol[j] = (p >> 2) * 64 + (((lane & 7) ^ C::swz(arow[j])) << 3);
    }
    auto issue = [&](int t, int slot) {            // tile t of the share into ring slot `slot`
        const int64_t r0 = row_begin + (int64_t)t * WREG_TILE_ROWS;
        char* dst = smem + slot * WREG_TILE_BYTES + wave * 3 * 1024;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            int64_t gm = r0 + arow[j];
            gm = gm < M ? gm : M - 1;
            glds16_asm(A + gm * lda + acol[j], dst + j * 1024);
        }
    };
#pragma unroll
    for (int p = 0; p < S - 1; ++p)
        if (p < nsteps) issue(p, p);

    // ---- the group's weights and bias, once: W fragment (n-tile j, K-step ks) = row 48 wave + 16 j + fr, k = 32 ks + 8 fq ..
    bf16x8 w[3][WREG_KSTEPS];
    float bv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int n = sh.group * WREG_N + wave * 48 + j * 16 + fr;
        const bf16* wrow = W + (int64_t)n * ldw + fq * 8;
#pragma unroll
        for (int ks = 0; ks < WREG_KSTEPS; ++ks) w[j][ks] = *(const bf16x8*)(wrow + ks * 32);
        bv[j] = bias ? bias[n] : 0.f;
    }
    // drained here, once, with a wait the compiler sees (as in gemm_nt_k384.hip): left to its own bookkeeping it spreads partial
    // vmcnt waits over the first step, and those counts would drain the ring
    __builtin_amdgcn_s_waitcnt(0x0f70);            // vmcnt(0)

    // fragment reads: row i * 16 + fr, chunk kk * 4 + fq of a [32][64] chunk; (row >> 1) & 7 = fr >> 1 for both i
    int aoff[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) aoff[kk] = C::off(fr, kk * 4 + fq);
    char* stage = smem + S * WREG_TILE_BYTES;
    // staging writes: accumulator (i, j) element e is row 16 i + 4 fq + e, column 48 wave + 16 j + fr
    char* swr = stage + (fq * 4) * WREG_STAGE_LD + (wave * 48 + fr) * 2;
    // row stores: piece q = thread + 512 jj is 16 bytes at column piece q % 48 of row q / 48
    int srow[3], scol[3];
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) {
        const int q = (int)threadIdx.x + 512 * jj;
        srow[jj] = q / 48;
        scol[jj] = q - srow[jj] * 48;
    }
    bf16* outg = out + (int64_t)(sh.group / groups_inner) * group_stride + (int64_t)(sh.group % groups_inner) * WREG_N;

    int slot = 0, islot = S - 1;                   // ring slots of tile t and of tile t + S - 1
    for (int t = 0; t < nsteps; ++t) {
        // LDS-DMA tiles issued behind tile t when its wait is reached: up to S - 2, fewer at the end of the share
        const int left = nsteps - 1 - t;
        if (left >= S - 2) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(3 * (S - 2)) : "memory");
        else if (left == 2) asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
        else if (left == 1) asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();              // tile t landed for every wave; everyone is done with tile t - 1 and the staging tile
        asm volatile("" ::: "memory");
        if (t + S - 1 < nsteps) issue(t + S - 1, islot);

        const char* sa = smem + slot * WREG_TILE_BYTES;
        f32x4 acc[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        // the four A fragments of a chunk (2 K-steps x 2 row tiles) are requested one chunk = 12 MFMAs ahead of their use, order pinned
        bf16x8 af[2][2][2];
        auto read4 = [&](int buf, int kc) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    af[buf][kk][i] = *(const bf16x8*)(sa + kc * WREG_CHUNK_BYTES + i * (16 * C::ROW_BYTES) + aoff[kk]);
        };
        read4(0, 0);
#pragma unroll
        for (int kc = 0; kc < 6; ++kc) {
            if (kc + 1 < 6) read4((kc + 1) & 1, kc + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kc & 1][kk][i], w[j][kc * 2 + kk], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }

        // ---- results -> staging tile (bf16) -> full rows
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    *(bf16*)(swr + (i * 16 + e) * WREG_STAGE_LD + j * 32) = (bf16)(acc[i][j][e] + bv[j]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();              // the staging tile is complete
        asm volatile("" ::: "memory");
        const int64_t r0 = row_begin + (int64_t)t * WREG_TILE_ROWS;
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) {
            const bf16x8 v = *(const bf16x8*)(stage + srow[jj] * WREG_STAGE_LD + scol[jj] * 16);
            const int64_t m = r0 + srow[jj];
            if (m < row_end) *(bf16x8*)(outg + m * ldo + scol[jj] * 8) = v;
        }
        slot = slot + 1 == S ? 0 : slot + 1;
        islot = islot + 1 == S ? 0 : islot + 1;
    }
}

bool gemm_nt_wreg_supported(int64_t lda, int64_t ldw, int64_t ldo, int64_t M, int groups, int groups_inner, int64_t group_stride) {
    if (M < 1 || M >= ((int64_t)1 << 31) || groups < 1 || groups > 4096 || groups_inner < 1 || group_stride < 0) return false;
    if (lda < 32 * WREG_KSTEPS || ldw < 32 * WREG_KSTEPS || ldo < (int64_t)WREG_N * groups_inner) return false;
    return lda % 8 == 0 && ldw % 8 == 0 && ldo % 8 == 0 && group_stride % 8 == 0;   // 16-byte pieces
}

int gemm_nt_wreg(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* out, int64_t ldo, int64_t M,
                 int groups, int groups_inner, int64_t group_stride, int workgroups, hipStream_t s) {
    if (workgroups < 0) return VITED_ERR_BAD_ARG;
    if (!gemm_nt_wreg_supported(lda, ldw, ldo, M, groups, groups_inner, group_stride)) return VITED_ERR_UNSUPPORTED;
    if (((uintptr_t)A | (uintptr_t)W | (uintptr_t)out) & 15 || (uintptr_t)bias & 3) return VITED_ERR_BAD_ARG;
    static std::once_flag once;
    static hipError_t status = hipSuccess;
    std::call_once(once, [&] {
        status = hipFuncSetAttribute((const void*)gemm_nt_wreg_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, WREG_LDS_BYTES);
    });
    if (status != hipSuccess) return VITED_ERR_LAUNCH;
    const int per = wreg_per_group(workgroups ? workgroups : WREG_SLOTS_RESIDENT, groups);
    hipLaunchKernelGGL(gemm_nt_wreg_kernel, dim3(per * groups), dim3(512), WREG_LDS_BYTES, s, (const bf16*)A, lda, (const bf16*)W, ldw,
                       bias, (bf16*)out, ldo, M, per, (int)wreg_units(M), groups_inner, group_stride);
    return vited_check_launch();
}
