// fp32 compute mode on the matrix cores: the GEMMs of gemm_portable.hip on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate).
// The instruction is bit for bit a k-ordered fmaf chain (D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), one rounding per product), which
// is what the portable kernels accumulate, so these kernels give the portable kernels' bits as long as every output element is ONE
// chain from +0 over the same products in the same order, zero products of the padding included:
//   * the reduction is walked in slabs of 16, the portable kernels' slab, padded with 0.f to a multiple of 16 and no further
//     (fma(0, 0, -0) is +0: one slab of padding more or less can flip the sign of a zero);
//   * no split of the reduction beyond the portable kernel's own, no second accumulator per output, slot 0 of an instruction is
//     the even k and slot 1 the odd one;
//   * the epilogue is epilogue_store<T, EPI> itself.
// BT x BT block (BT = 128 or 64), 256 threads, wave (wm, wn) of a 2 x 2 arrangement owns BT/2 x BT/2 outputs: 2 x 2 accumulators
// of 32 x 32 at BT = 128 (the higher rate once the grid is several rounds of the chip), one at BT = 64 (a quarter of the chain
// latency per slab and four times the blocks: the form for grids of up to about two rounds).
// Operands are staged k-major in LDS, As[k][m] / Bs[k][n], with the even k in rows 0..7 and the odd k in rows 8..15, so that the two
// lane halves of a fragment read (row = lane & 31, k slot = lane >> 5) are 8 rows = 32 banks apart.  Two LDS buffers: the next
// slab's global loads are issued before the current slab's MFMAs and written to the other buffer after them, one barrier a slab.
#include "gemm_epilogue.h"
#include "gemm_kernels.h"

#define FM_BK 16
#define FM_SMALL_GRID 576  // up to this many 128 x 128 tiles the 64 x 64 tile is used (measured: level at 576, ahead below)
#define FM_LD(BT) ((BT) + 4)  // floats per LDS row: 8 rows = 32 banks (mod 64) for both tiles, 16-B aligned rows

__device__ __forceinline__ int fm_row(int k) { return (k & 1) * 8 + (k >> 1); }   // LDS row of reduction index k of a slab

template <typename T> __device__ __forceinline__ f32x4 fm_load4(const T* p);
template <> __device__ __forceinline__ f32x4 fm_load4<float>(const float* p) { return *(const f32x4*)p; }
template <> __device__ __forceinline__ f32x4 fm_load4<bf16>(const bf16* p) {
    const bf16x4 v = *(const bf16x4*)p;
    return f32x4{to_f32(v[0]), to_f32(v[1]), to_f32(v[2]), to_f32(v[3])};
}

// whether 4 consecutive elements at every (row * ld + 4 c) may be read as one vector
template <typename T> __device__ __forceinline__ bool fm_vec_ok(const T* p, int64_t ld) {
    return (ld & 3) == 0 && ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0;
}

// An operand whose reduction index is the CONTIGUOUS one: P[o * ld + k], o in [o0, o0 + BT), k in [k0, k0 + 16).
// Thread -> rows tid / 4 (and tid / 4 + 64 at BT = 128), k (tid % 4) * 4 .. + 3.  Everything past o_end / k_end is 0.f.
template <typename T, int BT>
__device__ __forceinline__ void fm_fetch_ok(f32x4 (&r)[BT / 64], const T* __restrict__ P, int64_t ld, bool vec, int64_t o0, int64_t o_end,
                                            int64_t k0, int64_t k_end, int tid) {
    const int64_t k = k0 + (tid & 3) * 4;
#pragma unroll
    for (int p = 0; p < BT / 64; ++p) {
        const int64_t o = o0 + (tid >> 2) + p * 64;
        if (vec && o < o_end && k + 3 < k_end) {
            r[p] = fm_load4<T>(P + o * ld + k);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) r[p][j] = (o < o_end && k + j < k_end) ? to_f32(P[o * ld + k + j]) : 0.f;
        }
    }
}
template <int BT>
__device__ __forceinline__ void fm_put_ok(float (*S)[FM_LD(BT)], const f32x4 (&r)[BT / 64], int tid) {
    const int kq = (tid & 3) * 4;
#pragma unroll
    for (int p = 0; p < BT / 64; ++p)
#pragma unroll
        for (int j = 0; j < 4; ++j) S[fm_row(kq + j)][(tid >> 2) + p * 64] = r[p][j];
}

// An operand whose OUTPUT index is the contiguous one: P[k * ld + o].  BT / 4 threads a row of the slab: thread -> k tid / (BT / 4)
// (and + 8 at BT = 128), o (tid % (BT / 4)) * 4 .. + 3.
template <typename T, int BT>
__device__ __forceinline__ void fm_fetch_ko(f32x4 (&r)[BT / 64], const T* __restrict__ P, int64_t ld, bool vec, int64_t o0, int64_t o_end,
                                            int64_t k0, int64_t k_end, int tid) {
    constexpr int LPR = BT / 4;
    const int64_t o = o0 + (tid % LPR) * 4;
#pragma unroll
    for (int p = 0; p < BT / 64; ++p) {
        const int64_t k = k0 + tid / LPR + p * (256 / LPR);
        if (vec && k < k_end && o + 3 < o_end) {
            r[p] = fm_load4<T>(P + k * ld + o);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) r[p][j] = (k < k_end && o + j < o_end) ? to_f32(P[k * ld + o + j]) : 0.f;
        }
    }
}
template <int BT>
__device__ __forceinline__ void fm_put_ko(float (*S)[FM_LD(BT)], const f32x4 (&r)[BT / 64], int tid) {
    constexpr int LPR = BT / 4;
#pragma unroll
    for (int p = 0; p < BT / 64; ++p) *(f32x4*)&S[fm_row(tid / LPR + p * (256 / LPR))][(tid % LPR) * 4] = r[p];
}

// one slab: 8 instructions' worth of k per accumulator, k = 0, 1 | 2, 3 | ... in this order
template <int BT>
__device__ __forceinline__ void fm_slab(const float (*As)[FM_LD(BT)], const float (*Bs)[FM_LD(BT)], f32x16 (&acc)[BT / 64][BT / 64],
                                        int wm, int wn, int lane) {
    constexpr int WT = BT / 64;
    const int h8 = (lane >> 5) * 8, l = lane & 31;
#pragma unroll
    for (int s = 0; s < FM_BK / 2; ++s) {
        float a[WT], b[WT];
#pragma unroll
        for (int i = 0; i < WT; ++i) {
            a[i] = As[h8 + s][wm * (BT / 2) + i * 32 + l];
            b[i] = Bs[h8 + s][wn * (BT / 2) + i * 32 + l];
        }
#pragma unroll
        for (int i = 0; i < WT; ++i)
#pragma unroll
            for (int j = 0; j < WT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
}

// A [M, K] row-major (lda).  B: B_KN ? [K, N] (ldb) : [N, K] (ldb).
template <typename T, int EPI, bool B_KN, int BT>
__global__ void __launch_bounds__(256)
gemm_f32_mfma_kernel(const T* __restrict__ A, int64_t lda, const T* __restrict__ B, int64_t ldb, int64_t M, int64_t N, int64_t K,
                     EpiParams ep) {
    constexpr int WT = BT / 64;
    __shared__ __attribute__((aligned(16))) float As[2][FM_BK][FM_LD(BT)];
    __shared__ __attribute__((aligned(16))) float Bs[2][FM_BK][FM_LD(BT)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t m0 = (int64_t)blockIdx.y * BT, n0 = (int64_t)blockIdx.x * BT;
    const bool va = fm_vec_ok(A, lda), vb = fm_vec_ok(B, ldb);
    f32x4 ra[WT], rb[WT];
    auto fetch = [&](int64_t k0) {
        fm_fetch_ok<T, BT>(ra, A, lda, va, m0, M, k0, K, tid);
        if constexpr (B_KN) fm_fetch_ko<T, BT>(rb, B, ldb, vb, n0, N, k0, K, tid);
        else fm_fetch_ok<T, BT>(rb, B, ldb, vb, n0, N, k0, K, tid);
    };
    auto put = [&](int buf) {
        fm_put_ok<BT>(As[buf], ra, tid);
        if constexpr (B_KN) fm_put_ko<BT>(Bs[buf], rb, tid);
        else fm_put_ok<BT>(Bs[buf], rb, tid);
    };
    f32x16 acc[WT][WT] = {};
    fetch(0);
    put(0);
    __syncthreads();
    int buf = 0;
    for (int64_t k0 = 0; k0 < K; k0 += FM_BK) {
        const bool more = k0 + FM_BK < K;
        if (more) fetch(k0 + FM_BK);
        fm_slab<BT>(As[buf], Bs[buf], acc, wm, wn, lane);
        if (more) put(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    // C/D map of the 32 x 32 shapes: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int64_t m = m0 + wm * (BT / 2) + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            if (m >= M) continue;
            float rs = 1.f;
            if constexpr (EPI == EPI_RESIDUAL_SCALED) rs = ep.row_scale[m];
#pragma unroll
            for (int j = 0; j < WT; ++j) {
                const int64_t n = n0 + wn * (BT / 2) + j * 32 + (lane & 31);
                if (n < N) epilogue_store<T, EPI>(ep, m, n, acc[i][j][reg], rs);
            }
        }
}

// The 128-wide tile where its grid is more than FM_SMALL_GRID workgroups, else the 64-wide one (which wins where).
static inline int fm_tile(int64_t rows, int64_t cols) {
#ifdef FM_FORCE_TILE   // kernel experiments (make VARIANT=... EXTRA=-DFM_FORCE_TILE=64): one tile everywhere
    return FM_FORCE_TILE;
#else
    return ceil_div64(rows, 128) * ceil_div64(cols, 128) > FM_SMALL_GRID ? 128 : 64;
#endif
}

template <typename T, int EPI, int BT>
static void launch_f32_mfma_tile(const void* A, int64_t lda, const void* B, int64_t ldb, int b_layout, int64_t M, int64_t N, int64_t K,
                                 const EpiParams& ep, hipStream_t s) {
    dim3 grid((unsigned)ceil_div64(N, BT), (unsigned)ceil_div64(M, BT));
    if (b_layout == VITED_B_KN)
        hipLaunchKernelGGL((gemm_f32_mfma_kernel<T, EPI, true, BT>), grid, dim3(256), 0, s, (const T*)A, lda, (const T*)B, ldb, M, N, K, ep);
    else
        hipLaunchKernelGGL((gemm_f32_mfma_kernel<T, EPI, false, BT>), grid, dim3(256), 0, s, (const T*)A, lda, (const T*)B, ldb, M, N, K, ep);
}

template <typename T, int EPI>
static void launch_f32_mfma(const void* A, int64_t lda, const void* B, int64_t ldb, int b_layout, int64_t M, int64_t N, int64_t K,
                            const EpiParams& ep, hipStream_t s) {
    if (fm_tile(M, N) == 128) launch_f32_mfma_tile<T, EPI, 128>(A, lda, B, ldb, b_layout, M, N, K, ep, s);
    else launch_f32_mfma_tile<T, EPI, 64>(A, lda, B, ldb, b_layout, M, N, K, ep, s);
}

template <typename T>
static int dispatch_f32_mfma(const void* A, int64_t lda, const void* B, int64_t ldb, int b_layout, int64_t M, int64_t N, int64_t K,
                             int epilogue, const EpiParams& ep, hipStream_t s) {
    switch (epilogue) {
        case VITED_EPI_STORE: launch_f32_mfma<T, VITED_EPI_STORE>(A, lda, B, ldb, b_layout, M, N, K, ep, s); break;
        case VITED_EPI_GELU: launch_f32_mfma<T, VITED_EPI_GELU>(A, lda, B, ldb, b_layout, M, N, K, ep, s); break;
        case VITED_EPI_RESIDUAL: launch_f32_mfma<T, VITED_EPI_RESIDUAL>(A, lda, B, ldb, b_layout, M, N, K, ep, s); break;
        case VITED_EPI_MUL_GELU_GRAD: launch_f32_mfma<T, VITED_EPI_MUL_GELU_GRAD>(A, lda, B, ldb, b_layout, M, N, K, ep, s); break;
        case VITED_EPI_STORE_F32: launch_f32_mfma<T, VITED_EPI_STORE_F32>(A, lda, B, ldb, b_layout, M, N, K, ep, s); break;
        case VITED_EPI_MUL: launch_f32_mfma<T, VITED_EPI_MUL>(A, lda, B, ldb, b_layout, M, N, K, ep, s); break;
        case VITED_EPI_GELU_GRAD: launch_f32_mfma<T, VITED_EPI_GELU_GRAD>(A, lda, B, ldb, b_layout, M, N, K, ep, s); break;
        case EPI_RESIDUAL_SCALED: launch_f32_mfma<T, EPI_RESIDUAL_SCALED>(A, lda, B, ldb, b_layout, M, N, K, ep, s); break;
        default: return VITED_ERR_BAD_ARG;
    }
    return vited_check_launch();
}

// Host-only: the shapes that go to the matrix-core kernels (DESIGN.md section 37 has the measurements behind it).  A 32-wide
// accumulator tile that is mostly padding (the 4-logit head) stays on the vector-ALU kernel.
bool gemm_f32_mfma_supported(int64_t M, int64_t N, int64_t K, int b_layout, int epilogue) {
    if (b_layout != VITED_B_NK && b_layout != VITED_B_KN) return false;
    if (epilogue < VITED_EPI_STORE || epilogue > EPI_RESIDUAL_SCALED) return false;
    return M >= 64 && N >= 32 && K >= 1;
}

int gemm_f32_mfma(const void* A, int64_t lda, const void* B, int64_t ldb, int b_layout, int dtype, int64_t M, int64_t N, int64_t K,
                  int epilogue, const EpiParams& ep, hipStream_t s) {
    if (dtype == VITED_F32) return dispatch_f32_mfma<float>(A, lda, B, ldb, b_layout, M, N, K, epilogue, ep, s);
    if (dtype == VITED_BF16) return dispatch_f32_mfma<bf16>(A, lda, B, ldb, b_layout, M, N, K, epilogue, ep, s);
    return VITED_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------------
// weight gradient: dW[n, k] = sum_m dY[m, n] X[m, k], split over M exactly as gemm_tn_portable_kernel splits it: block z
// walks rows [z * rows_per_split, ...) in increasing m, in slabs of 16 padded with 0.f, and writes its BT x BT fp32 tile
// to slab z.  Both operands have the output index contiguous.
// ------------------------------------------------------------------------------------------------
template <typename T, int BT>
__global__ void __launch_bounds__(256)
gemm_tn_f32_mfma_kernel(const T* __restrict__ dY, int64_t lddy, const T* __restrict__ X, int64_t ldx, int64_t M, int64_t N, int64_t K,
                        int64_t rows_per_split, float* __restrict__ out) {
    constexpr int WT = BT / 64;
    __shared__ __attribute__((aligned(16))) float As[2][FM_BK][FM_LD(BT)];
    __shared__ __attribute__((aligned(16))) float Bs[2][FM_BK][FM_LD(BT)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t n0 = (int64_t)blockIdx.y * BT, kc0 = (int64_t)blockIdx.x * BT;
    const int64_t mb = (int64_t)blockIdx.z * rows_per_split;
    int64_t me = mb + rows_per_split;
    if (me > M) me = M;
    const bool va = fm_vec_ok(dY, lddy), vb = fm_vec_ok(X, ldx);
    f32x4 ra[WT], rb[WT];
    auto fetch = [&](int64_t r0) {
        fm_fetch_ko<T, BT>(ra, dY, lddy, va, n0, N, r0, me, tid);
        fm_fetch_ko<T, BT>(rb, X, ldx, vb, kc0, K, r0, me, tid);
    };
    auto put = [&](int buf) {
        fm_put_ko<BT>(As[buf], ra, tid);
        fm_put_ko<BT>(Bs[buf], rb, tid);
    };
    f32x16 acc[WT][WT] = {};
    fetch(mb);
    put(0);
    __syncthreads();
    int buf = 0;
    for (int64_t r0 = mb; r0 < me; r0 += FM_BK) {
        const bool more = r0 + FM_BK < me;
        if (more) fetch(r0 + FM_BK);
        fm_slab<BT>(As[buf], Bs[buf], acc, wm, wn, lane);
        if (more) put(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    float* o = out + (int64_t)blockIdx.z * N * K;
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int64_t n = n0 + wm * (BT / 2) + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            if (n >= N) continue;
#pragma unroll
            for (int j = 0; j < WT; ++j) {
                const int64_t k = kc0 + wn * (BT / 2) + j * 32 + (lane & 31);
                if (k < K) o[n * K + k] = acc[i][j][reg];
            }
        }
}

int gemm_tn_f32_mfma(const void* dY, int64_t lddy, const void* X, int64_t ldx, int dtype, int64_t M, int64_t N, int64_t K,
                     int64_t splits, float* out, hipStream_t s) {
    const int64_t rps = ceil_div64(ceil_div64(M, splits), FM_BK) * FM_BK;   // gemm_tn_portable's rounding
    if (dtype != VITED_F32 && dtype != VITED_BF16) return VITED_ERR_UNSUPPORTED;
    const bool f32 = dtype == VITED_F32;
    if (fm_tile(N, K * splits) == 128) {      // the splits are blocks of the grid like the tiles
        dim3 grid((unsigned)ceil_div64(K, 128), (unsigned)ceil_div64(N, 128), (unsigned)splits);
        if (f32) hipLaunchKernelGGL((gemm_tn_f32_mfma_kernel<float, 128>), grid, dim3(256), 0, s, (const float*)dY, lddy, (const float*)X, ldx, M, N, K, rps, out);
        else hipLaunchKernelGGL((gemm_tn_f32_mfma_kernel<bf16, 128>), grid, dim3(256), 0, s, (const bf16*)dY, lddy, (const bf16*)X, ldx, M, N, K, rps, out);
    } else {
        dim3 grid((unsigned)ceil_div64(K, 64), (unsigned)ceil_div64(N, 64), (unsigned)splits);
        if (f32) hipLaunchKernelGGL((gemm_tn_f32_mfma_kernel<float, 64>), grid, dim3(256), 0, s, (const float*)dY, lddy, (const float*)X, ldx, M, N, K, rps, out);
        else hipLaunchKernelGGL((gemm_tn_f32_mfma_kernel<bf16, 64>), grid, dim3(256), 0, s, (const bf16*)dY, lddy, (const bf16*)X, ldx, M, N, K, rps, out);
    }
    return vited_check_launch();
}
