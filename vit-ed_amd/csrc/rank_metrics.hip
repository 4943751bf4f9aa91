// Ranking metrics of a distance matrix, by rows: wi19_evaluate.get_metrics (mAP, top-1, Pr@10, Pr@100;
// vited_retrieval_metrics) and misc/metric.calc_map_prak (group mAP / Pr@k; vited_group_retrieval_metrics) of the reference.
//
// Row i orders its ELIGIBLE columns ascending by the composite key (D[i, j], j): ties go to the lower column, NaN after +inf,
// i.e. np.argsort(kind='stable').  Only the ranks of the row's CORRECT columns matter.  wi19 is the case where the correct
// columns are the row's class and every column is eligible; calc_map_prak takes the union of the columns of the row label's
// positive labels P(a), and with a negative relation only the columns of P(a) and N(a) are eligible.  One workgroup per row
//  1. stages the keys of up to CHUNK correct columns in LDS and bitonic-sorts them,
//  2. streams the eligible columns once (the whole row with 16-byte loads, or gathered through the label -> column CSR) and,
//     for every element, adds one to bin u of an LDS histogram, where u is the number of staged keys <= the element's key; an
//     inclusive scan then gives every staged column its exact rank (the number of eligible elements ordered before it),
//  3. accumulates its row record from those ranks.
// More than CHUNK correct columns repeat 1-3 per chunk; a second histogram, filled from the correct columns of every chunk,
// then counts the correct columns ordered before each staged one.  With skip_first the first element of the order (rank 0) is
// dropped whatever column it is, as the reference drops sorted_indexes[:, 1:].  A second launch sums the row records in a
// fixed order: the result is bit-identical run to run.  vited_retrieval_curves is the wi19 instance of the same kernel under the
// record policy CurveRecord: the positions of the correct columns counted per position (compute_roc / compute_fscore), one launch.
// The order itself (order_bits, make_key, rank_value) is rank_key.h's, shared with rank_lists.hip.
#include "common.h"
#include "rank_key.h"
#include "rank_row.h"

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = 2048;                  // correct columns per pass: 16 KB of keys + 2 x 8 KB of histograms in LDS
constexpr int MAX_K = 8;

using namespace rank_key;                    // order_bits, make_key, rank_value, PAD_KEY
using namespace rank_row;                    // f16, load_f32, Vec, unpack, unpack_half

// Number of keys[0, p2) that are <= k (keys ascending, padded with PAD_KEY to the power of two p2).
__device__ __forceinline__ int count_le(const uint64_t* keys, int p2, uint64_t k) {
    int pos = 0;
    for (int s = p2; s > 0; s >>= 1)
        if (pos + s <= p2 && keys[pos + s - 1] <= k) pos += s;
    return pos;
}

// Inclusive prefix sum of h[0, cnt) in place (cnt <= CHUNK = THREADS * 8): each thread scans 8 consecutive bins.
__device__ void block_inclusive_scan(uint32_t* h, int cnt, uint32_t* wave_tot) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t v[8], s = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int b = t * 8 + e;
        v[e] = b < cnt ? h[b] : 0u;
        s += v[e];
    }
    uint32_t x = s;                                     // inclusive scan of the thread totals over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) wave_tot[wave] = x;
    __syncthreads();
    uint32_t base = x - s;
    for (int w = 0; w < wave; ++w) base += wave_tot[w];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        base += v[e];
        const int b = t * 8 + e;
        if (b < cnt) h[b] = base;
    }
    __syncthreads();
}

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

// The two relations the row kernel ranks by.  Each is passed by value and holds the per-row state after select_row:
//  * npos, the number of correct columns, and for_correct(lo, hi, fn), fn(flat index, column) for the correct columns with
//    flat indexes in [lo, hi), called by the whole workgroup (out-of-range column indexes are possible; the kernel pads them);
//  * gather_eligible(fn): false when every column is eligible (the kernel streams the row), else fn(-, column) for each one;
//  * correct(b): whether a column of label b is correct;
//  * NH hit counters at the cut-offs cut(q), and write(rec, ...) of the row record, rec_len() doubles wide.

// wi19: the correct columns are the row's class, members[offsets[c], offsets[c + 1]); every column is eligible.
// Row record (5): AP sum, correct, top-1 hit, hits in the first 10, in the first 100.
struct ClassSlice {
    const int* offsets;
    const int* members;
    int num_classes;
    int c, beg;
    int64_t npos;

    static constexpr int NH = 3;
    __device__ static constexpr int cut(int q) { return q == 0 ? 1 : q == 1 ? 10 : 100; }
    __device__ static constexpr int rec_len() { return 5; }

    __device__ void select_row(int label, int64_t n) {
        c = label;
        beg = 0;
        npos = 0;
        if (c >= 0 && c < num_classes) {             // the binding builds labels and the CSR together; clamp for memory safety only
            beg = max(0, offsets[c]);
            npos = max(beg, min((int)n, offsets[c + 1])) - beg;
        }
    }
    template <typename F> __device__ void for_correct(int64_t lo, int64_t hi, F fn) const {
        for (int64_t f = lo + threadIdx.x; f < hi; f += THREADS) fn(f, (int64_t)members[beg + f]);
    }
    template <typename F> __device__ static bool gather_eligible(F) { return false; }
    __device__ bool correct(int b) const { return b == c; }
    __device__ void write(double* rec, double ap, const int* s) const {
        rec[0] = ap;
        rec[1] = s[0];
        rec[2] = s[1] > 0 ? 1.0 : 0.0;
        rec[3] = s[2];
        rec[4] = s[3];
    }
};

// LDS scratch of LabelSet::for_label_columns.
struct LabelBatch {
    int64_t pre[THREADS + 1];                // exclusive prefix of the column counts of the batch's labels
    int lab[THREADS];
    int64_t wave_tot[THREADS / 64];
};

// One LabelBatch per workgroup, whichever instantiations of for_label_columns use it.
__device__ __forceinline__ LabelBatch& label_batch() {
    __shared__ LabelBatch sb;
    return sb;
}

struct KList { int k[MAX_K]; };              // the Pr@k cut-offs, zero past nk

// calc_map_prak: the correct columns are those of the labels P(a), enumerated through the label -> column CSR; with a negative
// relation only the columns of P(a) and of N(a) \ P(a) are eligible.  Row record (3 + nk): AP mean, valid, correct, hits_k.
struct LabelSet {
    int num_labels;
    const int *col_off, *col_mem, *pos_off, *pos_lab, *neg_off, *neg_lab;
    KList ks;
    int nk;
    const int *P, *N;
    int pn, nn;
    int64_t n, npos;

    static constexpr int NH = MAX_K;
    __device__ int cut(int q) const { return ks.k[q]; }
    __device__ int rec_len() const { return 3 + nk; }

    __device__ void select_row(int a, int64_t n_) {
        n = n_;
        int pbeg = 0, nbeg = 0;
        pn = nn = 0;
        if (a >= 0 && a < num_labels) {              // the binding builds labels and the CSRs together; clamp for memory safety only
            pbeg = max(0, pos_off[a]);
            pn = max(0, pos_off[a + 1] - pbeg);
            if (neg_off) {
                nbeg = max(0, neg_off[a]);
                nn = max(0, neg_off[a + 1] - nbeg);
            }
        }
        P = pos_lab + pbeg;
        N = neg_lab ? neg_lab + nbeg : nullptr;
        npos = for_correct(0, 0, [](int64_t, int64_t) {});
    }
    template <typename F> __device__ int64_t for_correct(int64_t lo, int64_t hi, F fn) const {
        return for_label_columns(P, pn, nullptr, 0, lo, hi, fn);
    }
    template <typename F> __device__ bool gather_eligible(F fn) const {
        if (!neg_off) return false;
        for_correct(0, INT64_MAX, fn);
        for_label_columns(N, nn, P, pn, 0, INT64_MAX, fn);
        return true;
    }
    __device__ bool correct(int b) const { return sorted_contains(P, pn, b); }
    __device__ void write(double* rec, double ap, const int* s) const {
        rec[0] = s[0] > 0 ? ap / s[0] : 0.0;
        rec[1] = s[0] > 0 ? 1.0 : 0.0;
        rec[2] = s[0];
        for (int q = 0; q < nk; ++q) rec[3 + q] = s[1 + q];
    }

    // Enumerates the columns of the labels lab[0, nl) (those also in the ascending list excl[0, nexcl) skipped) in a fixed flat
    // order: label by label, each label's columns in col_mem order.  fn(flat index, column) runs for the flat indexes in [lo, hi)
    // only; the return value is the number of columns.  Called by the whole workgroup with uniform arguments.
    template <typename F>
    __device__ int64_t for_label_columns(const int* lab, int nl, const int* excl, int nexcl, int64_t lo, int64_t hi, F fn) const {
        LabelBatch& sb = label_batch();
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
};

// What else the row kernel records of the positions it finds.  NoRecord: nothing, the row record of the relation is all.
struct NoRecord {
    static constexpr bool ON = false;
};

// The wi19 curves (vited_retrieval_curves; compute_roc / compute_fscore of the reference): every correct column at 0-based position
// pos after the drop adds 1 to tp_at[pos] - 64-bit integer adds, whose sum does not depend on their order - and the row record is
// the int32 pair (correct retrievals, correct retrievals at positions < estimate[i]) instead of the relation's.
struct CurveRecord {
    static constexpr bool ON = true;
    unsigned long long* tp_at;               // [n - skip], added onto
    const int* estimate;                     // [n], or null: the second count stays 0
    int* rows;                               // [(r1 - r0) x 2]
};

template <typename T, typename Rel, typename Rec>
__global__ void __launch_bounds__(THREADS) rank_rows_kernel(const T* __restrict__ D, int64_t ld, int64_t n, int64_t r0,
                                                            const int* __restrict__ labels, Rel rel, int skip_first,
                                                            int from_similarity, double* __restrict__ rows_out, Rec rec) {
    __shared__ uint64_t keys[CHUNK];
    __shared__ uint32_t below_all[CHUNK];      // eligible elements ordered before staged column s (after the scan)
    __shared__ uint32_t below_pos[CHUNK];      // correct columns ordered before staged column s (after the scan)
    __shared__ uint64_t wave_min[THREADS / 64];
    __shared__ uint32_t wave_tot[THREADS / 64];
    __shared__ double red_d[THREADS / 64];
    __shared__ int red_i[1 + Rel::NH][THREADS / 64];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t i = r0 + blockIdx.x;
    const T* row = D + i * ld;
    const bool sim = from_similarity != 0;
    rel.select_row(labels[i], n);
    const int64_t npos = rel.npos;
    const int nchunks = (int)((npos + CHUNK - 1) / CHUNK);
    constexpr int VN = Vec<T>::N;                    // elements before the first 16-byte boundary, then whole vectors, then a tail
    const int64_t head = min(n, (int64_t)(((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) / sizeof(T)));
    const int64_t nvec = (n - head) / VN;
    auto key_of = [&](float v, int64_t j) { return make_key(rank_value<T>(v, sim), j); };
    auto key_at = [&](int64_t j) { return j >= 0 && j < n ? key_of(load_f32(row + j), j) : PAD_KEY; };

    double ap = 0.0;
    int correct = 0, hits[Rel::NH];
#pragma unroll
    for (int q = 0; q < Rel::NH; ++q) hits[q] = 0;
    bool dropped_is_pos = false;
    int in_estimate = 0;                             // CurveRecord only
    int64_t estimate = 0;
    if constexpr (Rec::ON) estimate = rec.estimate ? (int64_t)rec.estimate[i] : 0;

    for (int ch = 0; ch < nchunks; ++ch) {
        const int64_t cbeg = (int64_t)ch * CHUNK;
        const int cnt = (int)min((int64_t)CHUNK, npos - cbeg);
        int p2 = 1;
        while (p2 < cnt) p2 <<= 1;
        for (int s = t; s < p2; s += THREADS) {        // keys [0, cnt) are written by for_correct: no two writers per slot
            if (s >= cnt) keys[s] = PAD_KEY;
            below_all[s] = 0u;
            below_pos[s] = 0u;
        }
        rel.for_correct(cbeg, cbeg + cnt, [&](int64_t f, int64_t j) { keys[f - cbeg] = key_at(j); });
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

        // stream the eligible elements: bin u = number of staged keys <= this element's key; the element is ordered before
        // staged columns u..  A PAD_KEY (an out-of-range column) changes nothing.
        uint64_t rmin = PAD_KEY;
        auto visit = [&](uint64_t k) {
            if (ch == 0) rmin = k < rmin ? k : rmin;
            const int u = count_le(keys, p2, k);
            if (u < cnt) atomicAdd(&below_all[u], 1u);
        };
        if (!rel.gather_eligible([&](int64_t, int64_t j) { visit(key_at(j)); })) {
            for (int64_t j = t; j < head; j += THREADS) visit(key_of(load_f32(row + j), j));
            for (int64_t q = t; q < nvec; q += THREADS) {
                const typename Vec<T>::type raw = reinterpret_cast<const typename Vec<T>::type*>(row + head)[q];
                float v[VN];
                if constexpr (VN == 4) unpack(raw, v); else unpack_half<T>(raw, v);
#pragma unroll
                for (int e = 0; e < VN; ++e) visit(key_of(v[e], head + q * VN + e));
            }
            for (int64_t j = head + nvec * VN + t; j < n; j += THREADS) visit(key_of(load_f32(row + j), j));
        }
        if (nchunks > 1) {                                // correct columns of every chunk ordered before each staged one
            rel.for_correct(0, npos, [&](int64_t, int64_t j) {
                const int u = count_le(keys, p2, key_at(j));
                if (u < cnt) atomicAdd(&below_pos[u], 1u);
            });
        }
        if (ch == 0) {                                    // the row minimum: the element skip_first drops
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
            dropped_is_pos = skip_first && m != PAD_KEY && jmin < n && rel.correct(labels[jmin]);
        }
        block_inclusive_scan(below_all, cnt, wave_tot);
        if (nchunks > 1) block_inclusive_scan(below_pos, cnt, wave_tot);

        for (int s = t; s < cnt; s += THREADS) {
            if (keys[s] == PAD_KEY) continue;            // a column index out of range (never produced by the binding)
            const int64_t rank = below_all[s];
            if (skip_first && rank == 0) continue;        // this correct column is the dropped first element
            const int64_t pos = rank - (skip_first ? 1 : 0);                  // 0-based position after the drop
            const int64_t m = (nchunks > 1 ? (int64_t)below_pos[s] : (int64_t)s) + 1 - (dropped_is_pos ? 1 : 0);
            ap += (double)m / (double)(pos + 1);
            ++correct;
#pragma unroll
            for (int q = 0; q < Rel::NH; ++q) hits[q] += pos < rel.cut(q);
            if constexpr (Rec::ON) {
                if (pos < n - (skip_first ? 1 : 0)) atomicAdd(&rec.tp_at[pos], 1ull);
                in_estimate += pos < estimate;
            }
        }
        __syncthreads();                                  // keys / histograms are rewritten by the next chunk
    }

    // fixed-order block reduction of the row record
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ap += __shfl_xor(ap, off, 64);
        correct += __shfl_xor(correct, off, 64);
#pragma unroll
        for (int q = 0; q < Rel::NH; ++q) hits[q] += __shfl_xor(hits[q], off, 64);
    }
    if (lane == 0) {
        red_d[wave] = ap;
        red_i[0][wave] = correct;
#pragma unroll
        for (int q = 0; q < Rel::NH; ++q) red_i[1 + q][wave] = hits[q];
    }
    __syncthreads();
    if (t == 0) {
        double a = 0.0;
        int s[1 + Rel::NH] = {};
        for (int w = 0; w < THREADS / 64; ++w) {
            a += red_d[w];
            for (int f = 0; f < 1 + Rel::NH; ++f) s[f] += red_i[f][w];
        }
        if constexpr (!Rec::ON) rel.write(rows_out + (int64_t)blockIdx.x * rel.rec_len(), a, s);
        else rec.rows[(int64_t)blockIdx.x * 2] = s[0];
    }
    if constexpr (Rec::ON) {                          // the second count, summed like the first
        __shared__ int red_e[THREADS / 64];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) in_estimate += __shfl_xor(in_estimate, off, 64);
        if (lane == 0) red_e[wave] = in_estimate;
        __syncthreads();
        if (t == 0) {
            int e = 0;
            for (int w = 0; w < THREADS / 64; ++w) e += red_e[w];
            rec.rows[(int64_t)blockIdx.x * 2 + 1] = e;
        }
    }
}

// Fixed-order tree sum of every thread's acc over the workgroup; sums[0, nout) = the totals.
template <int F> __device__ void block_sums(const double (&acc)[F], double* sums, int nout) {
    __shared__ double part[F][THREADS];
    const int t = threadIdx.x;
    for (int f = 0; f < F; ++f) part[f][t] = acc[f];
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int f = 0; f < F; ++f) part[f][t] += part[f][t + s];
        __syncthreads();
    }
    if (t < nout) sums[t] = part[t][0];
}

// sums = {sum of AP over rows with a correct retrieval, those rows, top-1 hits, sum of Pr@10, sum of Pr@100,
//         rows without a correct retrieval, rows}.  Pr@k = hits_k / min(correct, k) is 0/0 = NaN on a row without one,
// exactly as in the reference, and the NaN carries into the sum.
__global__ void __launch_bounds__(THREADS) retrieval_sum_kernel(const double* __restrict__ rows_out, int64_t rows,
                                                                double* __restrict__ sums) {
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int64_t r = threadIdx.x; r < rows; r += THREADS) {
        const double* rec = rows_out + r * 5;
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
    block_sums(acc, sums, 7);
}

// sums = {sum of AP over valid rows, valid rows, for every k: sum over valid rows of hits_k / min(correct, k)}.  A row without
// a correct retrieval adds nothing: the reference leaves it out of every mean.
__global__ void __launch_bounds__(THREADS) group_sum_kernel(const double* __restrict__ rows_out, int64_t rows,
                                                            const KList ks, int nk, double* __restrict__ sums) {
    double acc[2 + MAX_K];
#pragma unroll
    for (int f = 0; f < 2 + MAX_K; ++f) acc[f] = 0.0;
    for (int64_t r = threadIdx.x; r < rows; r += THREADS) {
        const double* rec = rows_out + r * (3 + nk);
        if (rec[1] == 0.0) continue;
        acc[0] += rec[0];
        acc[1] += 1.0;
#pragma unroll
        for (int q = 0; q < MAX_K; ++q)
            if (q < nk) acc[2 + q] += rec[3 + q] / fmin(rec[2], (double)ks.k[q]);
    }
    block_sums(acc, sums, 2 + nk);
}

// The checks both entries share, then the row kernel for the dtype.  Entry-specific checks (all VITED_ERR_BAD_ARG) come first.
template <typename Rel, typename Rec = NoRecord>
int launch_rows(const void* D, int dtype, int64_t ld, int64_t n, int64_t r0, int64_t r1, const int* labels, int num_labels,
                const Rel& rel, int skip_first, int from_similarity, double* rows_out, double* sums, hipStream_t st,
                const Rec& rec = Rec()) {
    if (!D || !labels) return VITED_ERR_BAD_ARG;
    if (!Rec::ON && (!rows_out || !sums)) return VITED_ERR_BAD_ARG;
    if (n < 1 || n > INT32_MAX - 1 || ld < n || num_labels < 1 || num_labels > n) return VITED_ERR_BAD_ARG;
    if (r0 < 0 || r1 <= r0 || r1 > n) return VITED_ERR_BAD_ARG;
    const int esize = dtype == VITED_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(D) % esize != 0) return VITED_ERR_BAD_ARG;
    if (r1 - r0 > INT32_MAX) return VITED_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)(r1 - r0));
    switch (dtype) {
        case VITED_F32: hipLaunchKernelGGL((rank_rows_kernel<float, Rel, Rec>), grid, dim3(THREADS), 0, st, static_cast<const float*>(D), ld, n, r0, labels, rel, skip_first, from_similarity, rows_out, rec); break;
        case VITED_BF16: hipLaunchKernelGGL((rank_rows_kernel<bf16, Rel, Rec>), grid, dim3(THREADS), 0, st, static_cast<const bf16*>(D), ld, n, r0, labels, rel, skip_first, from_similarity, rows_out, rec); break;
        case VITED_F16: hipLaunchKernelGGL((rank_rows_kernel<f16, Rel, Rec>), grid, dim3(THREADS), 0, st, static_cast<const f16*>(D), ld, n, r0, labels, rel, skip_first, from_similarity, rows_out, rec); break;
        default: return VITED_ERR_UNSUPPORTED;
    }
    return vited_check_launch();
}

}  // namespace

extern "C" int vited_retrieval_metrics(const void* D, int dtype, int64_t ld, int64_t n, int64_t r0, int64_t r1, const int* labels,
                                       const int* offsets, const int* members, int num_classes, int remove_self_column,
                                       int from_similarity, double* rows_out, double* sums, void* stream) {
    if (!offsets || !members) return VITED_ERR_BAD_ARG;
    if ((remove_self_column != 0 && remove_self_column != 1) || (from_similarity != 0 && from_similarity != 1)) return VITED_ERR_BAD_ARG;
    if (remove_self_column && n < 2) return VITED_ERR_BAD_ARG;       // no column would be left to retrieve
    hipStream_t st = static_cast<hipStream_t>(stream);
    ClassSlice rel = {offsets, members, num_classes, 0, 0, 0};
    int rc = launch_rows(D, dtype, ld, n, r0, r1, labels, num_classes, rel, remove_self_column, from_similarity, rows_out, sums, st);
    if (rc != VITED_OK) return rc;
    hipLaunchKernelGGL(retrieval_sum_kernel, dim3(1), dim3(THREADS), 0, st, rows_out, r1 - r0, sums);
    return vited_check_launch();
}

extern "C" int vited_group_retrieval_metrics(const void* D, int dtype, int64_t ld, int64_t n, int64_t r0, int64_t r1,
                                             const int* labels, int num_labels, const int* col_offsets, const int* col_members,
                                             const int* pos_offsets, const int* pos_labels, const int* neg_offsets,
                                             const int* neg_labels, const int* ks, int nk, double* rows_out, double* sums,
                                             void* stream) {
    if (!col_offsets || !col_members || !pos_offsets || !pos_labels || !ks) return VITED_ERR_BAD_ARG;
    if ((neg_offsets == nullptr) != (neg_labels == nullptr)) return VITED_ERR_BAD_ARG;
    if (nk < 1 || nk > MAX_K) return VITED_ERR_BAD_ARG;
    LabelSet rel = {num_labels, col_offsets, col_members, pos_offsets, pos_labels, neg_offsets, neg_labels, {}, nk};
    for (int q = 0; q < nk; ++q) {
        if (ks[q] < 1) return VITED_ERR_BAD_ARG;
        rel.ks.k[q] = ks[q];
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = launch_rows(D, dtype, ld, n, r0, r1, labels, num_labels, rel, 1, 0, rows_out, sums, st);
    if (rc != VITED_OK) return rc;
    hipLaunchKernelGGL(group_sum_kernel, dim3(1), dim3(THREADS), 0, st, rows_out, r1 - r0, rel.ks, nk, sums);
    return vited_check_launch();
}

extern "C" int vited_retrieval_curves(const void* D, int dtype, int64_t ld, int64_t n, int64_t r0, int64_t r1, const int* labels,
                                      const int* offsets, const int* members, int num_classes, int remove_self_column,
                                      int from_similarity, const int* estimate, uint64_t* tp_at, int* rows_out, void* stream) {
    if (!offsets || !members || !tp_at || !rows_out) return VITED_ERR_BAD_ARG;
    if ((remove_self_column != 0 && remove_self_column != 1) || (from_similarity != 0 && from_similarity != 1)) return VITED_ERR_BAD_ARG;
    if (remove_self_column && n < 2) return VITED_ERR_BAD_ARG;       // no column would be left to retrieve
    if (reinterpret_cast<uintptr_t>(tp_at) % 8 != 0) return VITED_ERR_BAD_ARG;
    ClassSlice rel = {offsets, members, num_classes, 0, 0, 0};
    CurveRecord rec = {reinterpret_cast<unsigned long long*>(tp_at), estimate, rows_out};
    return launch_rows(D, dtype, ld, n, r0, r1, labels, num_classes, rel, remove_self_column, from_similarity, nullptr, nullptr,
                       static_cast<hipStream_t>(stream), rec);
}
