// Retrieval metrics of a distance matrix (wi19_evaluate.get_metrics of the reference: mAP, top-1, Pr@10, Pr@100), by rows.
//
// Row i orders its n columns ascending by the composite key (D[i, j], j): ties go to the lower column, NaN after +inf, i.e.
// np.argsort(kind='stable').  Only the ranks of the row's same-class columns ("positives") matter, so one workgroup per row
//  1. stages the keys of up to CHUNK positives in LDS and bitonic-sorts them,
//  2. streams the whole row once (16-byte loads) and, for every element, adds one to bin u of an LDS histogram, where u is
//     the number of staged positives whose key is <= the element's key; an inclusive scan then gives every staged positive
//     its exact rank (the number of row elements ordered before it),
//  3. accumulates its row record from those ranks.
// Classes with more than CHUNK members repeat 1-3 per chunk of positives; a second histogram, filled from the positives of
// every chunk, then counts the positives ordered before each staged one.  The first element of the order (the row
// minimum, rank 0) is dropped when remove_self_column is set, whatever column it is, as the reference drops
// sorted_indexes[:, 1:].  A second launch sums the row records in a fixed order: the result is bit-identical run to run.
#include "rank_keys.h"

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = 2048;                  // positives per pass: 16 KB of keys + 2 x 8 KB of histograms in LDS
constexpr int REC = 5;                       // row record: AP sum, correct, top-1 hit, hits in the first 10, first 100
constexpr int SUMS = 7;

// The value the row is ranked by: D itself, or T(1 - S) (fp32 subtract, one rounding to T) when the matrix holds similarities.
template <typename T> __device__ __forceinline__ float rank_value(float v, bool from_similarity) {
    return from_similarity ? (float)(T)(1.0f - v) : v;
}

template <typename T>
__global__ void __launch_bounds__(THREADS) retrieval_rows_kernel(const T* __restrict__ D, int64_t ld, int64_t n, int64_t r0,
                                                                 const int* __restrict__ labels, const int* __restrict__ offsets,
                                                                 const int* __restrict__ members, int num_classes, int remove_self,
                                                                 int from_similarity, double* __restrict__ rows_out) {
    __shared__ uint64_t keys[CHUNK];
    __shared__ uint32_t below_all[CHUNK];      // elements of the row ordered before staged positive t (after the scan)
    __shared__ uint32_t below_pos[CHUNK];      // positives of the class ordered before staged positive t (after the scan)
    __shared__ uint64_t wave_min[THREADS / 64];
    __shared__ uint32_t wave_tot[THREADS / 64];
    __shared__ double red_d[THREADS / 64];
    __shared__ int red_i[4][THREADS / 64];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t i = r0 + blockIdx.x;
    const T* row = D + i * ld;
    const bool sim = from_similarity != 0;
    const int c = labels[i];
    int beg = 0, end = 0;
    if (c >= 0 && c < num_classes) {               // the binding builds labels and the CSR together; clamp for memory safety only
        beg = max(0, offsets[c]);
        end = min((int)n, offsets[c + 1]);
        end = max(beg, end);
    }
    const int npos = end - beg;
    const int nchunks = (npos + CHUNK - 1) / CHUNK;
    constexpr int VN = Vec<T>::N;                    // elements before the first 16-byte boundary, then whole vectors, then a tail
    const int64_t head = min(n, (int64_t)(((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) / sizeof(T)));
    const int64_t nvec = (n - head) / VN;

    double ap = 0.0;
    int correct = 0, top1 = 0, h10 = 0, h100 = 0;
    bool dropped_is_pos = false;

    for (int ch = 0; ch < nchunks; ++ch) {
        const int cbeg = beg + ch * CHUNK, cnt = min(CHUNK, end - cbeg);
        int p2 = 1;
        while (p2 < cnt) p2 <<= 1;
        for (int s = t; s < p2; s += THREADS) {
            uint64_t k = PAD_KEY;
            if (s < cnt) {
                const int j = members[cbeg + s];
                if (j >= 0 && j < n) k = make_key(rank_value<T>(load_f32(row + j), sim), j);
            }
            keys[s] = k;
            below_all[s] = 0u;
            below_pos[s] = 0u;
        }
        __syncthreads();
        for (int k = 2; k <= p2; k <<= 1) {            // bitonic sort, ascending
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int q = t; q < p2 / 2; q += THREADS) {
                    const int a = (q / j) * 2 * j + (q % j), b = a + j;
                    const uint64_t ka = keys[a], kb = keys[b];
                    const bool up = (a & k) == 0;
                    if ((ka > kb) == up) { keys[a] = kb; keys[b] = ka; }
                }
                __syncthreads();
            }
        }

        // stream the row: bin u = number of staged keys <= this element's key; the element is ordered before staged positives u..
        uint64_t rmin = PAD_KEY;
        auto visit = [&](float v, int64_t j) {
            const uint64_t k = make_key(rank_value<T>(v, sim), j);
            if (ch == 0) rmin = k < rmin ? k : rmin;
            const int u = count_le(keys, p2, k);
            if (u < cnt) atomicAdd(&below_all[u], 1u);
        };
        for (int64_t j = t; j < head; j += THREADS) visit(load_f32(row + j), j);
        for (int64_t q = t; q < nvec; q += THREADS) {
            const typename Vec<T>::type raw = reinterpret_cast<const typename Vec<T>::type*>(row + head)[q];
            float v[VN];
            if constexpr (VN == 4) unpack(raw, v); else unpack_half<T>(raw, v);
#pragma unroll
            for (int e = 0; e < VN; ++e) visit(v[e], head + q * VN + e);
        }
        for (int64_t j = head + nvec * VN + t; j < n; j += THREADS) visit(load_f32(row + j), j);
        if (nchunks > 1) {                                // positives of every chunk ordered before each staged one
            for (int s = t; s < npos; s += THREADS) {
                const int j = members[beg + s];
                if (j < 0 || j >= n) continue;
                const int u = count_le(keys, p2, make_key(rank_value<T>(load_f32(row + j), sim), j));
                if (u < cnt) atomicAdd(&below_pos[u], 1u);
            }
        }
        if (ch == 0) {                                    // the row minimum: the element dropped by remove_self_column
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
            dropped_is_pos = remove_self && jmin < n && labels[jmin] == c;
        }
        block_inclusive_scan(below_all, cnt, wave_tot);
        if (nchunks > 1) block_inclusive_scan(below_pos, cnt, wave_tot);

        for (int s = t; s < cnt; s += THREADS) {
            if (keys[s] == PAD_KEY) continue;            // a member index out of range (never produced by the binding)
            const int64_t rank = below_all[s];
            if (remove_self && rank == 0) continue;       // this positive is the dropped first element
            const int64_t pos = rank - (remove_self ? 1 : 0);                 // 0-based position after the drop
            const int64_t m = (nchunks > 1 ? (int64_t)below_pos[s] : (int64_t)s) + 1 - (dropped_is_pos ? 1 : 0);
            ap += (double)m / (double)(pos + 1);
            ++correct;
            top1 |= pos == 0;
            h10 += pos < 10;
            h100 += pos < 100;
        }
        __syncthreads();                                  // keys / histograms are rewritten by the next chunk
    }

    // fixed-order block reduction of the row record
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ap += __shfl_xor(ap, off, 64);
        correct += __shfl_xor(correct, off, 64);
        top1 += __shfl_xor(top1, off, 64);
        h10 += __shfl_xor(h10, off, 64);
        h100 += __shfl_xor(h100, off, 64);
    }
    if (lane == 0) {
        red_d[wave] = ap;
        red_i[0][wave] = correct;
        red_i[1][wave] = top1;
        red_i[2][wave] = h10;
        red_i[3][wave] = h100;
    }
    __syncthreads();
    if (t == 0) {
        double a = 0.0;
        int s[4] = {0, 0, 0, 0};
        for (int w = 0; w < THREADS / 64; ++w) {
            a += red_d[w];
            for (int f = 0; f < 4; ++f) s[f] += red_i[f][w];
        }
        double* rec = rows_out + (int64_t)blockIdx.x * REC;
        rec[0] = a;
        rec[1] = s[0];
        rec[2] = s[1] > 0 ? 1.0 : 0.0;
        rec[3] = s[2];
        rec[4] = s[3];
    }
}

// sums = {sum of AP over rows with a correct retrieval, those rows, top-1 hits, sum of Pr@10, sum of Pr@100,
//         rows without a correct retrieval, rows}.  Pr@k = hits_k / min(correct, k) is 0/0 = NaN on a row without one,
// exactly as in the reference, and the NaN carries into the sum.
__global__ void __launch_bounds__(THREADS) retrieval_sum_kernel(const double* __restrict__ rows_out, int64_t rows,
                                                                double* __restrict__ sums) {
    __shared__ double part[SUMS][THREADS];
    const int t = threadIdx.x;
    double acc[SUMS] = {0, 0, 0, 0, 0, 0, 0};
    for (int64_t r = t; r < rows; r += THREADS) {
        const double* rec = rows_out + r * REC;
        const double correct = rec[1];
        if (correct > 0) {
            acc[0] += rec[0] / correct;
            acc[1] += 1.0;
        } else {
            acc[5] += 1.0;
        }
        acc[2] += rec[2];
        acc[3] += rec[3] / fmin(correct, 10.0);
        acc[4] += rec[4] / fmin(correct, 100.0);
        acc[6] += 1.0;
    }
    for (int f = 0; f < SUMS; ++f) part[f][t] = acc[f];
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int f = 0; f < SUMS; ++f) part[f][t] += part[f][t + s];
        __syncthreads();
    }
    if (t < SUMS) sums[t] = part[t][0];
}

template <typename T>
void launch_rows(const void* D, int64_t ld, int64_t n, int64_t r0, int64_t r1, const int* labels, const int* offsets,
                 const int* members, int num_classes, int remove_self, int from_similarity, double* rows_out, hipStream_t st) {
    hipLaunchKernelGGL(retrieval_rows_kernel<T>, dim3((unsigned)(r1 - r0)), dim3(THREADS), 0, st, static_cast<const T*>(D), ld, n,
                       r0, labels, offsets, members, num_classes, remove_self, from_similarity, rows_out);
}

}  // namespace

extern "C" int vited_retrieval_metrics(const void* D, int dtype, int64_t ld, int64_t n, int64_t r0, int64_t r1, const int* labels,
                                       const int* offsets, const int* members, int num_classes, int remove_self_column,
                                       int from_similarity, double* rows_out, double* sums, void* stream) {
    if (!D || !labels || !offsets || !members || !rows_out || !sums) return VITED_ERR_BAD_ARG;
    if (n < 1 || n > INT32_MAX - 1 || ld < n || num_classes < 1 || num_classes > n) return VITED_ERR_BAD_ARG;
    if (r0 < 0 || r1 <= r0 || r1 > n) return VITED_ERR_BAD_ARG;
    if ((remove_self_column != 0 && remove_self_column != 1) || (from_similarity != 0 && from_similarity != 1)) return VITED_ERR_BAD_ARG;
    if (remove_self_column && n < 2) return VITED_ERR_BAD_ARG;       // no column would be left to retrieve
    const int esize = dtype == VITED_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(D) % esize != 0) return VITED_ERR_BAD_ARG;
    if (r1 - r0 > INT32_MAX) return VITED_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case VITED_F32: launch_rows<float>(D, ld, n, r0, r1, labels, offsets, members, num_classes, remove_self_column, from_similarity, rows_out, st); break;
        case VITED_BF16: launch_rows<bf16>(D, ld, n, r0, r1, labels, offsets, members, num_classes, remove_self_column, from_similarity, rows_out, st); break;
        case VITED_F16: launch_rows<f16>(D, ld, n, r0, r1, labels, offsets, members, num_classes, remove_self_column, from_similarity, rows_out, st); break;
        default: return VITED_ERR_UNSUPPORTED;
    }
    int rc = vited_check_launch();
    if (rc != VITED_OK) return rc;
    hipLaunchKernelGGL(retrieval_sum_kernel, dim3(1), dim3(THREADS), 0, st, rows_out, r1 - r0, sums);
    return vited_check_launch();
}
