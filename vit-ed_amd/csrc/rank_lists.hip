// Ranked neighbour lists of a distance matrix, by rows (vited_retrieval_topk): the first k elements of the
// order of rank_key.h - ascending by (order_bits(v), column): ties to the lower column, NaN after +inf - after the optional drop of
// its first element: the columns, the ranked values, and whether each hit has the row's label.  What
// similarity_matrix[col].nlargest(k + 1) / wi19_evaluate.get_sorted_retrievals(...)[:, :k] give on the host, without the n x n
// matrix 1 - S and with the order defined under ties.
//
// One workgroup of 256 threads per row, one launch, no workspace.  With K = k + skip the workgroup
//  1. radix-selects the K-th key: pass p counts, in an LDS histogram of up to 2,048 bins, digit p (rank_key.h: sel_pass) of the keys
//     that match the boundary prefix found so far, a block scan finds the bin that holds the K-th key (sel_cut), and the passes end
//     as soon as the keys ordered before that bin and the bin itself are at most SEL_CAND = 2,048 together.  The digits cover the whole
//     64-bit key, column included, and no two keys are equal, so the last possible pass leaves one key in the bin: at most K <= 1,025
//     candidates.  A row of one repeated value therefore never overflows the buffer - its value digits leave all n keys in the boundary
//     bin and its column digits cut that bin down to the lowest columns;
//  2. gathers the candidates into LDS in the fixed order of the row walk: per step a wave scan of every thread's count and the wave
//     totals give each thread its slots (no counter, no atomic);
//  3. bitonic-sorts them (at most 2,048 keys, as rank_rows_kernel does) and writes elements [skip, K) of the order; the value is
//     read again from the row, so that it is the ranked value bit for bit (-0 and NaN payloads included).
// Every pass re-reads the row (at most 80 KB at n = 20,000: L2-resident) with 16-byte loads behind an unaligned head and before a
// tail.  LDS: 16 KB of candidates + 8 KB of histogram + a few words.  The only atomics are the integer adds of the histogram, whose
// sums do not depend on their order; a thread merges a run of equal digits into one add, which is what a row of ties consists of.
// Every output element is written exactly once, and identical inputs give identical outputs.
#include "common.h"
#include "rank_key.h"
#include "rank_row.h"

namespace {

using namespace rank_key;
using namespace rank_row;

constexpr int THREADS = SEL_THREADS;
constexpr int WAVES = THREADS / 64;

// Walks the row in steps the whole workgroup takes together: the step of the head and tail elements (one per thread), then steps
// of one 16-byte vector per thread.  elem(key, e) runs for every element of the thread, e counting them within the step; step() runs
// once per step in every thread.
template <typename T, typename E, typename S>
__device__ __forceinline__ void walk_row(const T* row, int64_t n, bool sim, E elem, S step) {
    constexpr int VN = Vec<T>::N;
    const int t = threadIdx.x;
    const int64_t head = head_elements(row, n);
    const int64_t nvec = (n - head) / VN;
    const int64_t tail0 = head + nvec * VN;                  // head + (n - tail0) <= 2 (VN - 1) < THREADS
    auto key_of = [&](float v, int64_t j) { return make_key(rank_value<T>(v, sim), j); };
    if (t < head) elem(key_of(load_f32(row + t), t), 0);
    else if (tail0 + (t - head) < n) elem(key_of(load_f32(row + tail0 + (t - head)), tail0 + (t - head)), 0);
    step();
    for (int64_t q0 = 0; q0 < nvec; q0 += THREADS) {
        const int64_t q = q0 + t;
        if (q < nvec) {
            const typename Vec<T>::type raw = reinterpret_cast<const typename Vec<T>::type*>(row + head)[q];
            float v[VN];
            if constexpr (VN == 4) unpack(raw, v); else unpack_half<T>(raw, v);
#pragma unroll
            for (int e = 0; e < VN; ++e) elem(key_of(v[e], head + q * VN + e), e);
        }
        step();
    }
}

// Inclusive scan of x over the wave.
__device__ __forceinline__ uint32_t wave_inclusive(uint32_t x, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    return x;
}

template <typename T>
__global__ void __launch_bounds__(THREADS) topk_rows_kernel(const T* __restrict__ D, int64_t ld, int64_t n, int64_t r0,
                                                            const int* __restrict__ labels, int k, int skip, int from_similarity,
                                                            int* __restrict__ idx, float* __restrict__ val,
                                                            uint8_t* __restrict__ hit) {
    __shared__ uint64_t cand[SEL_CAND];
    __shared__ uint32_t hist[SEL_BINS];
    __shared__ uint32_t wave_tot[2][WAVES];
    __shared__ uint32_t cut[3];                    // the boundary bin, the matching keys in the bins before it, the keys in it

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t i = r0 + blockIdx.x;
    const T* row = D + i * ld;
    const bool sim = from_similarity != 0;
    const uint32_t K = (uint32_t)(k + skip);

    if (t < 3) cut[t] = 0u;
    uint64_t bound = 0;                            // the digits of the K-th key found so far
    uint32_t below = 0, in_bin = 0;                // keys ordered before the boundary bin; keys in it
    SelPass last = {0, 0};
    const int passes = sel_num_passes(n);
    for (int p = 0; p < passes; ++p) {
        const SelPass ps = sel_pass(p, n);
        for (int b = t; b < SEL_BINS; b += THREADS) hist[b] = 0u;
        __syncthreads();
        int run_digit = 0;
        uint32_t run = 0;                          // a run of equal digits is one add
        walk_row(row, n, sim, [&](uint64_t key, int) {
            if (!sel_match(key, bound, ps)) return;
            const int d = sel_digit(key, ps);
            if (run && d != run_digit) {
                atomicAdd(&hist[run_digit], run);
                run = 0;
            }
            run_digit = d;
            ++run;
        }, [] {});
        if (run) atomicAdd(&hist[run_digit], run);
        __syncthreads();

        // the cut: each thread owns SEL_PER_THREAD consecutive bins; the one whose bins hold the (K - below)-th matching key reports it
        uint32_t own = 0;
#pragma unroll
        for (int e = 0; e < SEL_PER_THREAD; ++e) own += hist[t * SEL_PER_THREAD + e];
        const uint32_t incl = wave_inclusive(own, lane);
        if (lane == 63) wave_tot[0][wave] = incl;
        __syncthreads();
        uint32_t base = incl - own;
        for (int w = 0; w < wave; ++w) base += wave_tot[0][w];
        int bin;
        uint32_t before;
        if (sel_cut(hist + t * SEL_PER_THREAD, SEL_PER_THREAD, base, K - below, &bin, &before)) {
            cut[0] = (uint32_t)(t * SEL_PER_THREAD + bin);
            cut[1] = before;
            cut[2] = hist[t * SEL_PER_THREAD + bin];
        }
        __syncthreads();
        bound |= (uint64_t)cut[0] << ps.shift;
        below += cut[1];
        in_bin = cut[2];
        last = ps;
        if (sel_fits(below, in_bin)) break;
    }

    // gather the candidates, in the order of the walk
    uint32_t gathered = 0;
    int parity = 0;
    uint64_t mine[Vec<T>::N];                      // the step's keys, and which of them are candidates
    uint32_t taken = 0;
    walk_row(row, n, sim, [&](uint64_t key, int e) {
        mine[e] = key;
        if (sel_take(key, bound, last)) taken |= 1u << e;
    }, [&] {
        const uint32_t cnt = (uint32_t)__popc(taken);
        const uint32_t incl = wave_inclusive(cnt, lane);
        if (lane == 63) wave_tot[parity][wave] = incl;
        __syncthreads();
        uint32_t slot = gathered + incl - cnt, total = 0;
        for (int w = 0; w < WAVES; ++w) {
            slot += w < wave ? wave_tot[parity][w] : 0u;
            total += wave_tot[parity][w];
        }
#pragma unroll
        for (int e = 0; e < Vec<T>::N; ++e) {
            const uint32_t at = slot + (uint32_t)__popc(taken & ((1u << e) - 1u));
            if ((taken >> e & 1u) && at < (uint32_t)SEL_CAND) cand[at] = mine[e];
        }
        gathered += total;
        parity ^= 1;
        taken = 0;
    });
    const int have = (int)min(gathered, (uint32_t)SEL_CAND);          // = below + in_bin >= K
    int p2 = 1;
    while (p2 < have) p2 <<= 1;
    for (int s = have + t; s < p2; s += THREADS) cand[s] = PAD_KEY;
    __syncthreads();
    for (int kk = 2; kk <= p2; kk <<= 1) {             // bitonic sort, ascending
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int q = t; q < p2 / 2; q += THREADS) {
                const int a = (q / j) * 2 * j + (q % j), b = a + j;
                const uint64_t ka = cand[a], kb = cand[b];
                const bool up = (a & kk) == 0;
                if ((ka > kb) == up) { cand[a] = kb; cand[b] = ka; }
            }
            __syncthreads();
        }
    }

    const int my_label = hit ? labels[i] : 0;
    for (int s = t; s < k; s += THREADS) {
        const int64_t o = (int64_t)blockIdx.x * k + s;
        const uint64_t key = s + skip < p2 ? cand[s + skip] : PAD_KEY;
        const int64_t j = (int64_t)(key & 0xffffffffu);
        const bool real = key != PAD_KEY && j < n;                      // always, by the count of the selection
        idx[o] = real ? (int)j : -1;
        val[o] = real ? rank_value<T>(load_f32(row + j), sim) : __uint_as_float(0x7fc00000u);
        if (hit) hit[o] = real && labels[j] == my_label ? 1 : 0;
    }
}

}  // namespace

extern "C" int vited_retrieval_topk(const void* D, int dtype, int64_t ld, int64_t n, int64_t r0, int64_t r1, const int* labels,
                                    int k, int remove_self_column, int from_similarity, int* idx, float* val, uint8_t* hit,
                                    void* stream) {
    if (!D || !idx || !val || (hit && !labels)) return VITED_ERR_BAD_ARG;
    if (n < 1 || n > INT32_MAX - 1 || ld < n) return VITED_ERR_BAD_ARG;
    if (r0 < 0 || r1 <= r0 || r1 > n) return VITED_ERR_BAD_ARG;
    if ((remove_self_column != 0 && remove_self_column != 1) || (from_similarity != 0 && from_similarity != 1)) return VITED_ERR_BAD_ARG;
    if (k < 1 || (int64_t)k + remove_self_column > n) return VITED_ERR_BAD_ARG;
    const int esize = dtype == VITED_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(D) % esize != 0) return VITED_ERR_BAD_ARG;
    if (k > SEL_MAX_K || r1 - r0 > INT32_MAX) return VITED_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(r1 - r0));
    switch (dtype) {
        case VITED_F32: hipLaunchKernelGGL(topk_rows_kernel<float>, grid, dim3(THREADS), 0, st, static_cast<const float*>(D), ld, n, r0, labels, k, remove_self_column, from_similarity, idx, val, hit); break;
        case VITED_BF16: hipLaunchKernelGGL(topk_rows_kernel<bf16>, grid, dim3(THREADS), 0, st, static_cast<const bf16*>(D), ld, n, r0, labels, k, remove_self_column, from_similarity, idx, val, hit); break;
        case VITED_F16: hipLaunchKernelGGL(topk_rows_kernel<f16>, grid, dim3(THREADS), 0, st, static_cast<const f16*>(D), ld, n, r0, labels, k, remove_self_column, from_similarity, idx, val, hit); break;
        default: return VITED_ERR_UNSUPPORTED;
    }
    return vited_check_launch();
}
