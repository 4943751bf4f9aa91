// Deterministic pair-score aggregation (the distance maps of michigan.py:188-209 of the reference).
//
// A record (i, j, score) adds d = 1 - score (fp32) to cell (i, j) and to cell (j, i) of an n x n grid; a diagonal record adds
// it twice to (i, i), as the reference's two appends do.  Per cell: count, mean, min and sample stdev; over the cells holding
// more than one value: the mean and the sample stdev of those stdevs.
//
// The result does not depend on how the records were batched or ordered, bit for bit, because no float value is ever combined
// in arrival order:
//  1. vited_pair_scores_add: every record is stored (i, j, d) and counted per cell with integer atomics;
//  2. vited_pair_scores_finish: an exclusive scan of the counts gives every cell a segment, the values are scattered into it
//     (the order inside a segment is arbitrary), and each cell's values are sorted by value - the sorted sequence is the same
//     whatever the arrival order - and reduced in that order in fp64 (sum, then a second pass over the squared deviations);
//  3. the stdev statistics are reduced over the cells in cell order by one workgroup.
// Cells of up to SMALL values are finished by one thread each (insertion sort in the segment), up to CAP values by a
// workgroup (bitonic sort in LDS), larger ones by a workgroup that places every value at its rank (a count over LDS chunks).
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int SCAN_TILE = THREADS * 8;      // cells per block of the count scan
constexpr int SMALL = 32;                   // values per cell finished by a single thread
constexpr int CAP = 8192;                   // values per cell sorted in LDS (32 KB)
constexpr int LARGE_BLOCKS = 1024;          // persistent grid over the cells above SMALL

typedef _Float16 f16;

__device__ __forceinline__ float load_score(const float* p, int64_t r) { return p[r]; }
__device__ __forceinline__ float load_score(const bf16* p, int64_t r) { return (float)p[r]; }
__device__ __forceinline__ float load_score(const f16* p, int64_t r) { return (float)p[r]; }

// Total order on the bit patterns of the values: -inf < ... < -0 < +0 < ... < +inf; NaNs at the ends by sign.  Equal images are
// equal bit patterns, so any two sorts of one multiset give the same sequence.
__device__ __forceinline__ uint32_t sort_bits(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_sort_bits(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

template <typename I, typename S>
__global__ void __launch_bounds__(THREADS) add_kernel(const I* __restrict__ pairs, int64_t ld, const S* __restrict__ scores,
                                                      int64_t m, int64_t n, int* __restrict__ counts, int* __restrict__ rec_cells,
                                                      float* __restrict__ rec_values, int* __restrict__ bad) {
    const int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (r >= m) return;
    const int64_t i = (int64_t)pairs[r * ld], j = (int64_t)pairs[r * ld + 1];
    const float d = 1.0f - load_score(scores, r);
    if (i < 0 || i >= n || j < 0 || j >= n) {
        rec_cells[2 * r] = -1;
        rec_cells[2 * r + 1] = -1;
        rec_values[r] = d;
        atomicOr(bad, 1);
        return;
    }
    rec_cells[2 * r] = (int)i;
    rec_cells[2 * r + 1] = (int)j;
    rec_values[r] = d;
    atomicAdd(&counts[i * n + j], 1);
    atomicAdd(&counts[j * n + i], 1);
}

// offsets[c] = sum of counts[0, c) within the tile, tile totals to tile_sum; cursors zeroed.
__global__ void __launch_bounds__(THREADS) scan_tiles_kernel(const int* __restrict__ counts, int64_t cells, int64_t* __restrict__ offsets,
                                                             int64_t* __restrict__ tile_sum, int* __restrict__ cursor) {
    __shared__ int64_t wave_tot[THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)t * 8;
    int64_t v[8], s = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int64_t c = c0 + e;
        v[e] = c < cells ? max(counts[c], 0) : 0;
        s += v[e];
        if (c < cells) cursor[c] = 0;
    }
    int64_t x = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) wave_tot[wave] = x;
    __syncthreads();
    int64_t base = x - s, total = 0;
    for (int w = 0; w < THREADS / 64; ++w) {
        base += w < wave ? wave_tot[w] : 0;
        total += wave_tot[w];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int64_t c = c0 + e;
        if (c < cells) offsets[c] = base;
        base += v[e];
    }
    if (t == 0) tile_sum[blockIdx.x] = total;
}

// Exclusive scan of the tile totals in place (one workgroup, tiles in order); offsets[cells] = the total.
__global__ void __launch_bounds__(THREADS) scan_totals_kernel(int64_t* __restrict__ tile_sum, int64_t tiles, int64_t* __restrict__ offsets,
                                                              int64_t cells) {
    __shared__ int64_t wave_tot[THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < tiles; b0 += THREADS) {
        const int64_t b = b0 + t;
        const int64_t s = b < tiles ? tile_sum[b] : 0;
        int64_t x = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        if (lane == 63) wave_tot[wave] = x;
        __syncthreads();
        int64_t base = carry + x - s, total = 0;
        for (int w = 0; w < THREADS / 64; ++w) {
            base += w < wave ? wave_tot[w] : 0;
            total += wave_tot[w];
        }
        if (b < tiles) tile_sum[b] = base;
        carry += total;
        __syncthreads();
    }
    if (t == 0) offsets[cells] = carry;
}

__global__ void __launch_bounds__(THREADS) scan_add_kernel(int64_t* __restrict__ offsets, int64_t cells, const int64_t* __restrict__ tile_sum) {
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c < cells) offsets[c] += tile_sum[c / SCAN_TILE];
}

__global__ void __launch_bounds__(THREADS) scatter_kernel(const int* __restrict__ rec_cells, const float* __restrict__ rec_values, int64_t m,
                                                          int64_t n, const int* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                          int* __restrict__ cursor, float* __restrict__ vals, int* __restrict__ bad) {
    const int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (r >= m) return;
    const int i = rec_cells[2 * r], j = rec_cells[2 * r + 1];
    if (i < 0 || i >= n || j < 0 || j >= n) return;
    const float d = rec_values[r];
    const int64_t cell[2] = {(int64_t)i * n + j, (int64_t)j * n + i};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = atomicAdd(&cursor[cell[h]], 1);
        const int64_t at = offsets[cell[h]] + p;
        if (p < counts[cell[h]] && at < 2 * m) vals[at] = d;
        else atomicOr(bad, 2);                            // counts and records disagree (never produced by the binding)
    }
}

__device__ __forceinline__ void write_cell(int64_t c, int cnt, double sum, double ss, float vmin, float* mean, float* minv, double* stdev) {
    const float nan = __uint_as_float(0x7fc00000u);
    mean[c] = cnt > 0 ? (float)(sum / cnt) : nan;
    minv[c] = cnt > 0 ? vmin : nan;
    stdev[c] = cnt > 1 ? sqrt(ss / (cnt - 1)) : (double)nan;
}

// One thread per cell: empty and single-value cells, and cells of up to SMALL values (insertion sort in the segment); larger
// cells go to the list of the workgroup pass.
__global__ void __launch_bounds__(THREADS) small_cells_kernel(const int* __restrict__ counts, int64_t cells, const int64_t* __restrict__ offsets,
                                                              float* __restrict__ vals, float* __restrict__ mean, float* __restrict__ minv,
                                                              double* __restrict__ stdev, int* __restrict__ large, int* __restrict__ nlarge,
                                                              int64_t nvals, int* __restrict__ bad) {
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c >= cells) return;
    int cnt = max(counts[c], 0);
    if (offsets[c] + cnt > nvals) {                      // counts and records disagree (never produced by the binding)
        atomicOr(bad, 2);
        cnt = 0;
    }
    if (cnt > SMALL) {
        large[atomicAdd(nlarge, 1)] = (int)c;             // the list's order varies; each cell's result does not
        return;
    }
    float* v = vals + offsets[c];
    for (int a = 1; a < cnt; ++a) {
        const float x = v[a];
        const uint32_t kx = sort_bits(x);
        int b = a - 1;
        while (b >= 0 && sort_bits(v[b]) > kx) {
            v[b + 1] = v[b];
            --b;
        }
        v[b + 1] = x;
    }
    double sum = 0.0, ss = 0.0;
    for (int a = 0; a < cnt; ++a) sum += (double)v[a];
    const double mu = cnt > 0 ? sum / cnt : 0.0;
    for (int a = 0; a < cnt; ++a) {
        const double dv = (double)v[a] - mu;
        ss += dv * dv;
    }
    write_cell(c, cnt, sum, ss, cnt > 0 ? v[0] : 0.0f, mean, minv, stdev);
}

// Sum of f(sorted[q]) over q < cnt in a fixed order: each thread a contiguous range, then a fixed tree.
template <typename F>
__device__ double block_ordered_sum(int cnt, double* red, F f) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (cnt + THREADS - 1) / THREADS;
    double s = 0.0;
    for (int q = t * per; q < min(cnt, (t + 1) * per); ++q) s += f(q);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
    __syncthreads();
    if (lane == 0) red[wave] = s;
    __syncthreads();
    double total = 0.0;
    for (int w = 0; w < THREADS / 64; ++w) total += red[w];
    return total;
}

// One workgroup per cell above SMALL values: bitonic sort in LDS up to CAP values, beyond that every value is written to its rank
// in `sorted` (rank = values below it + equal values before it in the segment: equal values are equal bits, so the sequence is
// the sorted one).  Then the two ordered fp64 passes.
__global__ void __launch_bounds__(THREADS) large_cells_kernel(const int* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                              const float* __restrict__ vals, float* __restrict__ sorted,
                                                              float* __restrict__ mean, float* __restrict__ minv, double* __restrict__ stdev,
                                                              const int* __restrict__ large, const int* __restrict__ nlarge) {
    __shared__ uint32_t key[CAP];
    __shared__ double red[THREADS / 64];
    const int t = threadIdx.x;
    const int total = *nlarge;
    for (int q = blockIdx.x; q < total; q += gridDim.x) {
        const int64_t c = large[q];
        const int cnt = counts[c];
        const int64_t off = offsets[c];
        const float* v = vals + off;
        double sum, ss;
        float vmin;
        if (cnt <= CAP) {
            int p2 = 1;
            while (p2 < cnt) p2 <<= 1;
            for (int s = t; s < p2; s += THREADS) key[s] = s < cnt ? sort_bits(v[s]) : 0xffffffffu;
            __syncthreads();
            for (int k = 2; k <= p2; k <<= 1) {
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int x = t; x < p2 / 2; x += THREADS) {
                        const int a = (x / j) * 2 * j + (x % j), b = a + j;
                        const uint32_t ka = key[a], kb = key[b];
                        if ((ka > kb) == ((a & k) == 0)) { key[a] = kb; key[b] = ka; }
                    }
                    __syncthreads();
                }
            }
            sum = block_ordered_sum(cnt, red, [&](int s) { return (double)from_sort_bits(key[s]); });
            const double mu = sum / cnt;
            ss = block_ordered_sum(cnt, red, [&](int s) { const double d = (double)from_sort_bits(key[s]) - mu; return d * d; });
            vmin = from_sort_bits(key[0]);
        } else {
            float* out = sorted + off;
            for (int a0 = 0; a0 < cnt; a0 += THREADS) {
                const int a = a0 + t;
                const uint32_t ka = a < cnt ? sort_bits(v[a]) : 0u;
                int rank = 0;
                for (int b0 = 0; b0 < cnt; b0 += CAP) {
                    const int nb = min(CAP, cnt - b0);
                    __syncthreads();
                    for (int s = t; s < nb; s += THREADS) key[s] = sort_bits(v[b0 + s]);
                    __syncthreads();
                    if (a < cnt)
                        for (int s = 0; s < nb; ++s) rank += key[s] < ka || (key[s] == ka && b0 + s < a);
                }
                if (a < cnt) out[rank] = v[a];
            }
            __threadfence_block();
            __syncthreads();
            sum = block_ordered_sum(cnt, red, [&](int s) { return (double)out[s]; });
            const double mu = sum / cnt;
            ss = block_ordered_sum(cnt, red, [&](int s) { const double d = (double)out[s] - mu; return d * d; });
            vmin = out[0];
        }
        if (t == 0) write_cell(c, cnt, sum, ss, vmin, mean, minv, stdev);
        __syncthreads();                                  // key / red are rewritten by the next cell
    }
}

// stats = {mean of the stdevs of the cells with more than one value, their sample stdev}: cells in a fixed order, fp64.
__global__ void __launch_bounds__(THREADS) std_stats_kernel(const int* __restrict__ counts, const double* __restrict__ stdev, int64_t cells,
                                                            double* __restrict__ stats) {
    __shared__ double part[2][THREADS];
    const int t = threadIdx.x;
    double s = 0.0, k = 0.0;
    for (int64_t c = t; c < cells; c += THREADS)
        if (counts[c] > 1) {
            s += stdev[c];
            k += 1.0;
        }
    part[0][t] = s;
    part[1][t] = k;
    __syncthreads();
    for (int h = THREADS / 2; h > 0; h >>= 1) {
        if (t < h) {
            part[0][t] += part[0][t + h];
            part[1][t] += part[1][t + h];
        }
        __syncthreads();
    }
    const double n_std = part[1][0], mu = part[0][0] / n_std;
    __syncthreads();
    double ss = 0.0;
    for (int64_t c = t; c < cells; c += THREADS)
        if (counts[c] > 1) {
            const double d = stdev[c] - mu;
            ss += d * d;
        }
    part[0][t] = ss;
    __syncthreads();
    for (int h = THREADS / 2; h > 0; h >>= 1) {
        if (t < h) part[0][t] += part[0][t + h];
        __syncthreads();
    }
    if (t == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        stats[0] = n_std > 0 ? mu : nan;
        stats[1] = n_std > 1 ? sqrt(part[0][0] / (n_std - 1)) : nan;
    }
}

struct Workspace {
    int64_t* offsets;      // [cells + 1]
    int64_t* tile_sum;     // [tiles]
    int* cursor;           // [cells]
    int* large;            // [cells]
    int* nlarge;           // [1] (+ padding)
    float* vals;           // [2 m]
    float* sorted;         // [2 m]
};

int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

int64_t carve(int64_t n, int64_t m, char* base, Workspace* w) {
    const int64_t cells = n * n, tiles = (cells + SCAN_TILE - 1) / SCAN_TILE;
    int64_t off = 0;
    auto take = [&](int64_t bytes) { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
    Workspace ws;
    ws.offsets = reinterpret_cast<int64_t*>(take(8 * (cells + 1)));
    ws.tile_sum = reinterpret_cast<int64_t*>(take(8 * tiles));
    ws.cursor = reinterpret_cast<int*>(take(4 * cells));
    ws.large = reinterpret_cast<int*>(take(4 * cells));
    ws.nlarge = reinterpret_cast<int*>(take(4));
    ws.vals = reinterpret_cast<float*>(take(4 * 2 * m));
    ws.sorted = reinterpret_cast<float*>(take(4 * 2 * m));
    if (w) *w = ws;
    return off;
}

unsigned blocks_for(int64_t items) { return (unsigned)((items + THREADS - 1) / THREADS); }

template <typename I, typename S>
void launch_add(const void* pairs, int64_t ld, const void* scores, int64_t m, int64_t n, int* counts, int* rec_cells, float* rec_values,
                int* bad, hipStream_t st) {
    hipLaunchKernelGGL((add_kernel<I, S>), dim3(blocks_for(m)), dim3(THREADS), 0, st, static_cast<const I*>(pairs), ld,
                       static_cast<const S*>(scores), m, n, counts, rec_cells, rec_values, bad);
}

template <typename I>
int dispatch_add(const void* pairs, int64_t ld, const void* scores, int score_dtype, int64_t m, int64_t n, int* counts, int* rec_cells,
                 float* rec_values, int* bad, hipStream_t st) {
    switch (score_dtype) {
        case VITED_F32: launch_add<I, float>(pairs, ld, scores, m, n, counts, rec_cells, rec_values, bad, st); return VITED_OK;
        case VITED_BF16: launch_add<I, bf16>(pairs, ld, scores, m, n, counts, rec_cells, rec_values, bad, st); return VITED_OK;
        case VITED_F16: launch_add<I, f16>(pairs, ld, scores, m, n, counts, rec_cells, rec_values, bad, st); return VITED_OK;
        default: return VITED_ERR_UNSUPPORTED;
    }
}

constexpr int64_t MAX_FRAGMENTS = 46340;    // n * n cells fit an int32 cell index

}  // namespace

extern "C" int64_t vited_pair_scores_workspace_bytes(int64_t n, int64_t m) {
    if (n < 1 || n > MAX_FRAGMENTS || m < 0) return -1;
    return carve(n, m, nullptr, nullptr);
}

extern "C" int vited_pair_scores_add(const void* pairs, int pair_dtype, int64_t pair_ld, const void* scores, int score_dtype, int64_t m,
                                     int64_t n, int* counts, int* rec_cells, float* rec_values, int* bad, void* stream) {
    if (!pairs || !scores || !counts || !rec_cells || !rec_values || !bad) return VITED_ERR_BAD_ARG;
    if (m < 1 || n < 1 || n > MAX_FRAGMENTS || pair_ld < 2 || m > INT32_MAX / 2) return VITED_ERR_BAD_ARG;
    const int isize = pair_dtype == VITED_I32 ? 4 : 8;
    if (reinterpret_cast<uintptr_t>(pairs) % isize != 0 || reinterpret_cast<uintptr_t>(scores) % (score_dtype == VITED_F32 ? 4 : 2) != 0)
        return VITED_ERR_BAD_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc;
    switch (pair_dtype) {
        case VITED_I32: rc = dispatch_add<int32_t>(pairs, pair_ld, scores, score_dtype, m, n, counts, rec_cells, rec_values, bad, st); break;
        case VITED_I64: rc = dispatch_add<int64_t>(pairs, pair_ld, scores, score_dtype, m, n, counts, rec_cells, rec_values, bad, st); break;
        default: return VITED_ERR_UNSUPPORTED;
    }
    if (rc != VITED_OK) return rc;
    return vited_check_launch();
}

extern "C" int vited_pair_scores_finish(const int* rec_cells, const float* rec_values, int64_t m, int64_t n, const int* counts, float* mean,
                                        float* minv, double* stdev, double* stats, int* bad, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
    if (!counts || !mean || !minv || !stdev || !stats || !bad || !workspace) return VITED_ERR_BAD_ARG;
    if (n < 1 || n > MAX_FRAGMENTS || m < 0 || m > INT32_MAX / 2 || (m > 0 && (!rec_cells || !rec_values))) return VITED_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return VITED_ERR_BAD_ARG;
    if (workspace_bytes < carve(n, m, nullptr, nullptr)) return VITED_ERR_WORKSPACE;
    Workspace w;
    carve(n, m, static_cast<char*>(workspace), &w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t cells = n * n, tiles = (cells + SCAN_TILE - 1) / SCAN_TILE;
    if (hipMemsetAsync(w.nlarge, 0, sizeof(int), st) != hipSuccess) return VITED_ERR_LAUNCH;
    hipLaunchKernelGGL(scan_tiles_kernel, dim3((unsigned)tiles), dim3(THREADS), 0, st, counts, cells, w.offsets, w.tile_sum, w.cursor);
    hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(THREADS), 0, st, w.tile_sum, tiles, w.offsets, cells);
    hipLaunchKernelGGL(scan_add_kernel, dim3(blocks_for(cells)), dim3(THREADS), 0, st, w.offsets, cells, w.tile_sum);
    if (m > 0)
        hipLaunchKernelGGL(scatter_kernel, dim3(blocks_for(m)), dim3(THREADS), 0, st, rec_cells, rec_values, m, n, counts, w.offsets,
                           w.cursor, w.vals, bad);
    hipLaunchKernelGGL(small_cells_kernel, dim3(blocks_for(cells)), dim3(THREADS), 0, st, counts, cells, w.offsets, w.vals, mean, minv,
                       stdev, w.large, w.nlarge, 2 * m, bad);
    hipLaunchKernelGGL(large_cells_kernel, dim3(LARGE_BLOCKS), dim3(THREADS), 0, st, counts, w.offsets, w.vals, w.sorted, mean, minv,
                       stdev, w.large, w.nlarge);
    hipLaunchKernelGGL(std_stats_kernel, dim3(1), dim3(THREADS), 0, st, counts, stdev, cells, stats);
    return vited_check_launch();
}
