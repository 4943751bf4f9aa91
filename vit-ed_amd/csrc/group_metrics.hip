// Group mAP / Pr@k of a distance matrix (misc/metric.calc_map_prak of the reference), by rows.
//
// Row i has the label a = labels[i].  A column j is CORRECT when labels[j] is one of a's positive labels P(a), and, when a
// negative relation is given, ELIGIBLE when labels[j] is in P(a) or in a's negative labels N(a); without one every column is
// eligible.  The eligible columns are ordered ascending by (D[i, j], j) (ties to the lower column, NaN last: a stable argsort),
// position 0 of that order is skipped whatever it is, and the AP / hits_k of the correct columns at positions 1.. follow.
// One workgroup per row, the scheme of retrieval.hip:
//  1. the keys of up to CHUNK correct columns are staged in LDS and bitonic-sorted;
//  2. the eligible columns are streamed once - the whole row with 16-byte loads, or with negatives the columns of P(a) and
//     N(a) \ P(a), gathered through the label -> column CSR - and every element adds one to bin u of an LDS histogram, u the
//     number of staged keys <= its key; an inclusive scan gives every staged column its rank among the eligible columns;
//  3. the row record accumulates from those ranks.
// Sets of correct columns larger than CHUNK repeat 1-3 per chunk, with a second histogram counting the correct columns of every
// chunk ordered before each staged one.  A second launch sums the row records in a fixed order: bit-identical run to run.
#include "rank_keys.h"

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = 2048;                  // correct columns per pass: 16 KB of keys + 2 x 8 KB of histograms in LDS
constexpr int MAX_K = 8;

struct KList { int k[MAX_K]; };              // the Pr@k cut-offs, passed by value

// LDS scratch of the label -> column enumeration below.
struct LabelBatch {
    int64_t pre[THREADS + 1];                // exclusive prefix of the column counts of the batch's labels
    int lab[THREADS];
    int64_t wave_tot[THREADS / 64];
};

// Is label b in the ascending list s[0, ns)?
__device__ __forceinline__ bool sorted_contains(const int* s, int ns, int b) {
    int lo = 0, hi = ns;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int v = s[mid];
        if (v == b) return true;
        if (v < b) lo = mid + 1; else hi = mid;
    }
    return false;
}

// Enumerates the columns of the labels lab[0, nl) (those also in the ascending list excl[0, nexcl) skipped) in a fixed flat
// order: label by label, each label's columns in col_members order.  fn(flat index, column) runs for the flat indexes in
// [lo, hi) only; the return value is the number of columns.  Called by the whole workgroup with uniform arguments.
template <typename F>
__device__ int64_t for_label_columns(const int* lab, int nl, const int* excl, int nexcl, const int* col_off, const int* col_mem,
                                     int num_labels, int64_t n, int64_t lo, int64_t hi, LabelBatch& sb, F fn) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int64_t base = 0;
    for (int b0 = 0; b0 < nl; b0 += THREADS) {
        const int q = b0 + t;
        int b = -1;
        int64_t cnt = 0;
        if (q < nl) {
            b = lab[q];
            if (b >= 0 && b < num_labels && !(nexcl > 0 && sorted_contains(excl, nexcl, b))) {
                const int64_t o0 = min((int64_t)max(col_off[b], 0), n), o1 = min((int64_t)max(col_off[b + 1], 0), n);
                cnt = max((int64_t)0, o1 - o0);
            }
        }
        int64_t x = cnt;                                  // inclusive scan over the wave, then over the waves
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        if (lane == 63) sb.wave_tot[wave] = x;
        __syncthreads();
        int64_t before = 0, total = 0;
        for (int w = 0; w < THREADS / 64; ++w) {
            before += w < wave ? sb.wave_tot[w] : 0;
            total += sb.wave_tot[w];
        }
        sb.pre[t] = before + x - cnt;
        sb.lab[t] = b;
        if (t == 0) sb.pre[THREADS] = total;
        __syncthreads();
        const int64_t a = max(lo, base), z = min(hi, base + total);
        for (int64_t f = a + t; f < z; f += THREADS) {
            const int64_t k = f - base;
            int u = 0;                                    // the last batch slot whose prefix is <= k
            for (int s = THREADS / 2; s > 0; s >>= 1)
                if (u + s < THREADS && sb.pre[u + s] <= k) u += s;
            const int bl = sb.lab[u];
            const int64_t j = col_mem[min((int64_t)max(col_off[bl], 0), n) + (k - sb.pre[u])];
            fn(f, j);
        }
        base += total;
        __syncthreads();                                  // sb is rewritten by the next batch
    }
    return base;
}

template <typename T>
__global__ void __launch_bounds__(THREADS) group_rows_kernel(const T* __restrict__ D, int64_t ld, int64_t n, int64_t r0,
                                                             const int* __restrict__ labels, int num_labels,
                                                             const int* __restrict__ col_off, const int* __restrict__ col_mem,
                                                             const int* __restrict__ pos_off, const int* __restrict__ pos_lab,
                                                             const int* __restrict__ neg_off, const int* __restrict__ neg_lab,
                                                             const KList ks, int nk, double* __restrict__ rows_out) {
    __shared__ uint64_t keys[CHUNK];
    __shared__ uint32_t below_all[CHUNK];      // eligible columns ordered before staged column s (after the scan)
    __shared__ uint32_t below_pos[CHUNK];      // correct columns ordered before staged column s (after the scan)
    __shared__ LabelBatch sb;
    __shared__ uint64_t wave_min[THREADS / 64];
    __shared__ uint32_t wave_tot[THREADS / 64];
    __shared__ double red_d[THREADS / 64];
    __shared__ int red_i[1 + MAX_K][THREADS / 64];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t i = r0 + blockIdx.x;
    const T* row = D + i * ld;
    const int a = labels[i];
    int pbeg = 0, pn = 0, nbeg = 0, nn = 0;
    if (a >= 0 && a < num_labels) {                 // the binding builds labels and the CSRs together; clamp for memory safety only
        pbeg = max(0, pos_off[a]);
        pn = max(0, pos_off[a + 1] - pbeg);
        if (neg_off) {
            nbeg = max(0, neg_off[a]);
            nn = max(0, neg_off[a + 1] - nbeg);
        }
    }
    const int* P = pos_lab + pbeg;
    const int* N = neg_lab ? neg_lab + nbeg : nullptr;
    const bool filtered = neg_off != nullptr;
    auto none = [](int64_t, int64_t) {};
    const int64_t npos = for_label_columns(P, pn, nullptr, 0, col_off, col_mem, num_labels, n, 0, 0, sb, none);
    const int nchunks = (int)((npos + CHUNK - 1) / CHUNK);
    constexpr int VN = Vec<T>::N;
    const int64_t head = min(n, (int64_t)(((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) / sizeof(T)));
    const int64_t nvec = (n - head) / VN;

    double ap = 0.0;
    int correct = 0, hits[MAX_K];
#pragma unroll
    for (int q = 0; q < MAX_K; ++q) hits[q] = 0;
    bool dropped_is_pos = false;

    for (int ch = 0; ch < nchunks; ++ch) {
        const int64_t cbeg = (int64_t)ch * CHUNK;
        const int cnt = (int)min((int64_t)CHUNK, npos - cbeg);
        int p2 = 1;
        while (p2 < cnt) p2 <<= 1;
        for (int s = t; s < p2; s += THREADS) {
            keys[s] = PAD_KEY;
            below_all[s] = 0u;
            below_pos[s] = 0u;
        }
        __syncthreads();
        for_label_columns(P, pn, nullptr, 0, col_off, col_mem, num_labels, n, cbeg, cbeg + cnt, sb, [&](int64_t f, int64_t j) {
            if (j >= 0 && j < n) keys[f - cbeg] = make_key(load_f32(row + j), j);
        });
        for (int k = 2; k <= p2; k <<= 1) {            // bitonic sort, ascending
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int q = t; q < p2 / 2; q += THREADS) {
                    const int x = (q / j) * 2 * j + (q % j), y = x + j;
                    const uint64_t kx = keys[x], ky = keys[y];
                    const bool up = (x & k) == 0;
                    if ((kx > ky) == up) { keys[x] = ky; keys[y] = kx; }
                }
                __syncthreads();
            }
        }

        // stream the eligible columns: bin u = number of staged keys <= this element's key
        uint64_t rmin = PAD_KEY;
        auto visit_key = [&](uint64_t k) {
            if (ch == 0) rmin = k < rmin ? k : rmin;
            const int u = count_le(keys, p2, k);
            if (u < cnt) atomicAdd(&below_all[u], 1u);
        };
        if (!filtered) {
            for (int64_t j = t; j < head; j += THREADS) visit_key(make_key(load_f32(row + j), j));
            for (int64_t q = t; q < nvec; q += THREADS) {
                const typename Vec<T>::type raw = reinterpret_cast<const typename Vec<T>::type*>(row + head)[q];
                float v[VN];
                if constexpr (VN == 4) unpack(raw, v); else unpack_half<T>(raw, v);
#pragma unroll
                for (int e = 0; e < VN; ++e) visit_key(make_key(v[e], head + q * VN + e));
            }
            for (int64_t j = head + nvec * VN + t; j < n; j += THREADS) visit_key(make_key(load_f32(row + j), j));
        } else {
            auto visit_col = [&](int64_t, int64_t j) {
                if (j >= 0 && j < n) visit_key(make_key(load_f32(row + j), j));
            };
            for_label_columns(P, pn, nullptr, 0, col_off, col_mem, num_labels, n, 0, INT64_MAX, sb, visit_col);
            for_label_columns(N, nn, P, pn, col_off, col_mem, num_labels, n, 0, INT64_MAX, sb, visit_col);
        }
        if (nchunks > 1) {                                // correct columns of every chunk ordered before each staged one
            for_label_columns(P, pn, nullptr, 0, col_off, col_mem, num_labels, n, 0, INT64_MAX, sb, [&](int64_t, int64_t j) {
                if (j < 0 || j >= n) return;
                const int u = count_le(keys, p2, make_key(load_f32(row + j), j));
                if (u < cnt) atomicAdd(&below_pos[u], 1u);
            });
        }
        if (ch == 0) {                                    // the first eligible element: skipped, whatever it is
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint64_t o = __shfl_xor(rmin, off, 64);
                rmin = o < rmin ? o : rmin;
            }
            if (lane == 0) wave_min[wave] = rmin;
        }
        __syncthreads();
        if (ch == 0) {
            uint64_t m = wave_min[0];
            for (int w = 1; w < THREADS / 64; ++w) m = wave_min[w] < m ? wave_min[w] : m;
            const int64_t jmin = (int64_t)(m & 0xffffffffu);
            dropped_is_pos = m != PAD_KEY && jmin < n && sorted_contains(P, pn, labels[jmin]);
        }
        block_inclusive_scan(below_all, cnt, wave_tot);
        if (nchunks > 1) block_inclusive_scan(below_pos, cnt, wave_tot);

        for (int s = t; s < cnt; s += THREADS) {
            if (keys[s] == PAD_KEY) continue;            // a member index out of range (never produced by the binding)
            const int64_t rank = below_all[s];
            if (rank == 0) continue;                      // this correct column is the skipped first element
            const int64_t pos = rank - 1;                 // 0-based position after the skip
            const int64_t m = (nchunks > 1 ? (int64_t)below_pos[s] : (int64_t)s) + 1 - (dropped_is_pos ? 1 : 0);
            ap += (double)m / (double)(pos + 1);
            ++correct;
#pragma unroll
            for (int q = 0; q < MAX_K; ++q) hits[q] += q < nk && pos < ks.k[q];
        }
        __syncthreads();                                  // keys / histograms are rewritten by the next chunk
    }

    // fixed-order block reduction of the row record
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ap += __shfl_xor(ap, off, 64);
        correct += __shfl_xor(correct, off, 64);
#pragma unroll
        for (int q = 0; q < MAX_K; ++q) hits[q] += __shfl_xor(hits[q], off, 64);
    }
    if (lane == 0) {
        red_d[wave] = ap;
        red_i[0][wave] = correct;
#pragma unroll
        for (int q = 0; q < MAX_K; ++q) red_i[1 + q][wave] = hits[q];
    }
    __syncthreads();
    if (t == 0) {
        double sum_ap = 0.0;
        int c = 0;
        for (int w = 0; w < THREADS / 64; ++w) {
            sum_ap += red_d[w];
            c += red_i[0][w];
        }
        double* rec = rows_out + (int64_t)blockIdx.x * (3 + nk);
        rec[0] = c > 0 ? sum_ap / c : 0.0;
        rec[1] = c > 0 ? 1.0 : 0.0;
        rec[2] = c;
        for (int q = 0; q < nk; ++q) {
            int h = 0;
            for (int w = 0; w < THREADS / 64; ++w) h += red_i[1 + q][w];
            rec[3 + q] = h;
        }
    }
}

// sums = {sum of AP over valid rows, valid rows, for every k: sum over valid rows of hits_k / min(correct, k)}.  A row without
// a correct retrieval adds nothing: the reference leaves it out of every mean.
__global__ void __launch_bounds__(THREADS) group_sum_kernel(const double* __restrict__ rows_out, int64_t rows,
                                                            const KList ks, int nk, double* __restrict__ sums) {
    __shared__ double part[2 + MAX_K][THREADS];
    const int t = threadIdx.x;
    double acc[2 + MAX_K];
#pragma unroll
    for (int f = 0; f < 2 + MAX_K; ++f) acc[f] = 0.0;
    for (int64_t r = t; r < rows; r += THREADS) {
        const double* rec = rows_out + r * (3 + nk);
        if (rec[1] == 0.0) continue;
        acc[0] += rec[0];
        acc[1] += 1.0;
#pragma unroll
        for (int q = 0; q < MAX_K; ++q)
            if (q < nk) acc[2 + q] += rec[3 + q] / fmin(rec[2], (double)ks.k[q]);
    }
    for (int f = 0; f < 2 + MAX_K; ++f) part[f][t] = acc[f];
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int f = 0; f < 2 + MAX_K; ++f) part[f][t] += part[f][t + s];
        __syncthreads();
    }
    if (t < 2 + nk) sums[t] = part[t][0];
}

template <typename T>
void launch_rows(const void* D, int64_t ld, int64_t n, int64_t r0, int64_t r1, const int* labels, int num_labels, const int* col_off,
                 const int* col_mem, const int* pos_off, const int* pos_lab, const int* neg_off, const int* neg_lab, const KList& ks,
                 int nk, double* rows_out, hipStream_t st) {
    hipLaunchKernelGGL(group_rows_kernel<T>, dim3((unsigned)(r1 - r0)), dim3(THREADS), 0, st, static_cast<const T*>(D), ld, n, r0,
                       labels, num_labels, col_off, col_mem, pos_off, pos_lab, neg_off, neg_lab, ks, nk, rows_out);
}

}  // namespace

extern "C" int vited_group_retrieval_metrics(const void* D, int dtype, int64_t ld, int64_t n, int64_t r0, int64_t r1,
                                             const int* labels, int num_labels, const int* col_offsets, const int* col_members,
                                             const int* pos_offsets, const int* pos_labels, const int* neg_offsets,
                                             const int* neg_labels, const int* ks, int nk, double* rows_out, double* sums,
                                             void* stream) {
    if (!D || !labels || !col_offsets || !col_members || !pos_offsets || !pos_labels || !ks || !rows_out || !sums)
        return VITED_ERR_BAD_ARG;
    if ((neg_offsets == nullptr) != (neg_labels == nullptr)) return VITED_ERR_BAD_ARG;
    if (n < 1 || n > INT32_MAX - 1 || ld < n || num_labels < 1 || num_labels > n) return VITED_ERR_BAD_ARG;
    if (r0 < 0 || r1 <= r0 || r1 > n) return VITED_ERR_BAD_ARG;
    if (nk < 1 || nk > MAX_K) return VITED_ERR_BAD_ARG;
    KList kl = {};
    for (int q = 0; q < nk; ++q) {
        if (ks[q] < 1) return VITED_ERR_BAD_ARG;
        kl.k[q] = ks[q];
    }
    const int esize = dtype == VITED_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(D) % esize != 0) return VITED_ERR_BAD_ARG;
    if (r1 - r0 > INT32_MAX) return VITED_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case VITED_F32: launch_rows<float>(D, ld, n, r0, r1, labels, num_labels, col_offsets, col_members, pos_offsets, pos_labels, neg_offsets, neg_labels, kl, nk, rows_out, st); break;
        case VITED_BF16: launch_rows<bf16>(D, ld, n, r0, r1, labels, num_labels, col_offsets, col_members, pos_offsets, pos_labels, neg_offsets, neg_labels, kl, nk, rows_out, st); break;
        case VITED_F16: launch_rows<f16>(D, ld, n, r0, r1, labels, num_labels, col_offsets, col_members, pos_offsets, pos_labels, neg_offsets, neg_labels, kl, nk, rows_out, st); break;
        default: return VITED_ERR_UNSUPPORTED;
    }
    int rc = vited_check_launch();
    if (rc != VITED_OK) return rc;
    hipLaunchKernelGGL(group_sum_kernel, dim3(1), dim3(THREADS), 0, st, rows_out, r1 - r0, kl, nk, sums);
    return vited_check_launch();
}
