// Pair mining behind vited_mine_pairs: writer ids [n] + one fp32 key per ordered cell c = i * n + j  ->  the pair list (every
// same-id cell with i < j in ascending cell order, then the `keep` different-id candidates with the smallest (key, cell)), labels,
// validity weights, padding up to a fixed capacity, the PairSegments tables of column 1 and five counts.  This header holds the
// index arithmetic and the per-lane bodies of the kernel's three phases as plain C++ (a wave's ballot comes in as a 64-bit mask)
// so that the same text runs inside the HIP kernel (pair_mine.hip) and in a host program under the sanitizers
// (tools/mine_host_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MINE_FN __host__ __device__ __forceinline__
#else
#define MINE_FN inline
#endif

#define MINE_MAX_IMAGES 128
#define MINE_MAX_CAPACITY 24576      // 3 * 128 * 127 / 2 + 1 = 24,385 rounded up to a multiple of 1,024: one byte of LDS per row
#define MINE_THREADS 1024
#define MINE_WAVE 64
#define MINE_WAVES (MINE_THREADS / MINE_WAVE)
#define MINE_MIN_SORT 64

enum { MINE_POS = 1, MINE_CAND = 2 };

struct MineArgs {
    const int64_t* targets;   // [n]
    const float* keys;        // [n * n]
    int n, ordered, capacity;
    double neg_per_pos;
    int64_t* groups;          // [capacity][2]
    float* labels;            // [capacity]
    float* weights;           // [capacity]
    int64_t* seg_index;       // [capacity] = groups[:, 1]
    int64_t* seg_order;       // [capacity]
    int64_t* seg_offsets;     // [n + 1]
    int32_t* counts;          // [5]
};

// number of 64-bit words the sort runs over: the next power of two of n * n (at least one wave's worth)
MINE_FN int mine_sort_size(int n) {
    int s = MINE_MIN_SORT;
    while (s < n * n) s <<= 1;
    return s;
}

MINE_FN void mine_cell_ij(int c, int n, int& i, int& j) {
    i = c / n;
    j = c - i * n;
}

// MINE_POS: i < j with equal ids.  MINE_CAND: different ids, i < j (or any i != j when `ordered`).  0: everything else, the
// cells past n * n of the sort's padding included.
MINE_FN int mine_classify(const int64_t* tgt, int n, int ordered, int c) {
    if (c < 0 || c >= n * n) return 0;
    int i, j;
    mine_cell_ij(c, n, i, j);
    if (i == j) return 0;
    if (tgt[i] == tgt[j]) return i < j ? MINE_POS : 0;
    return (ordered || i < j) ? MINE_CAND : 0;
}

// (key, cell) as one word whose unsigned order is the order of the key AS A FLOAT, then of the cell: the usual sign flip, after
// key + 0 has turned -0 into +0.  A cell that is no candidate is all-ones and sorts behind every candidate.
MINE_FN uint64_t mine_sort_word(float key, int c, bool cand) {
    if (!cand) return ~(uint64_t)0;
    uint32_t b = __builtin_bit_cast(uint32_t, key + 0.0f);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)b << 32) | (uint32_t)c;
}

// rank of `lane` among the set bits of a wave's ballot
MINE_FN int mine_rank(uint64_t mask, int lane) { return __builtin_popcountll(mask & (((uint64_t)1 << lane) - 1)); }

struct MineCounts {
    int pos_rows, neg_rows, rows;   // what is emitted
    int32_t out[5];                 // positives found, candidates found, negatives emitted, pairs emitted, pairs dropped
};

// keep = min(#candidates, int(neg_per_pos * #positives)): the product in double, truncated like Python's int(); a product that
// is negative or NaN keeps nothing.  Then the truncation to the capacity: negatives go first, from the end, then positives.
MINE_FN MineCounts mine_counts(int npos, int ncand, double neg_per_pos, int capacity) {
    const double want = neg_per_pos * (double)npos;
    const int keep = !(want > 0.0) ? 0 : (want >= (double)ncand ? ncand : (int)want);
    MineCounts m;
    m.pos_rows = npos < capacity ? npos : capacity;
    m.neg_rows = keep < capacity - m.pos_rows ? keep : capacity - m.pos_rows;
    m.rows = m.pos_rows + m.neg_rows;
    m.out[0] = npos;
    m.out[1] = ncand;
    m.out[2] = m.neg_rows;
    m.out[3] = m.rows;
    m.out[4] = npos + keep - m.rows;
    return m;
}

// One output row; row_item[r] keeps column 1 (< 128) for the counting pass.  A row outside [0, capacity) is dropped here.
MINE_FN void mine_write_row(const MineArgs& a, uint8_t* row_item, int r, int i, int j, float label, float weight) {
    if (r < 0 || r >= a.capacity) return;
    a.groups[2 * (int64_t)r] = i;
    a.groups[2 * (int64_t)r + 1] = j;
    a.labels[r] = label;
    a.weights[r] = weight;
    a.seg_index[r] = j;
    row_item[r] = (uint8_t)j;
}

// Phase 1, one cell: the positive whose ballot rank puts it at row `row` is written at once (label 1, weight 1).
MINE_FN void mine_emit_positive(const MineArgs& a, uint8_t* row_item, int c, int row) {
    int i, j;
    mine_cell_ij(c, a.n, i, j);
    mine_write_row(a, row_item, row, i, j, 1.0f, 1.0f);
}

// Phase 2, compare-exchange number t (0 <= t < size / 2) of the bitonic stage (k, j), j < k powers of two.
MINE_FN void mine_bitonic_pair(uint64_t* w, int t, int k, int j) {
    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    const int hi = lo | j;
    const uint64_t x = w[lo], y = w[hi];
    if ((x > y) == ((lo & k) == 0)) {
        w[lo] = y;
        w[hi] = x;
    }
}

// Phase 3, row r in [pos_rows, capacity): the kept negative number r - pos_rows of the sorted words (label 0, weight 1), or a
// padding row (0, 0) with label 0 and weight 0.
MINE_FN void mine_emit_tail(const MineArgs& a, const MineCounts& m, const uint64_t* sorted, uint8_t* row_item, int r) {
    int i = 0, j = 0;
    bool real = false;
    if (r >= m.pos_rows && r < m.rows) {
        const uint32_t c = (uint32_t)sorted[r - m.pos_rows];
        if (c < (uint32_t)(a.n * a.n)) {
            mine_cell_ij((int)c, a.n, i, j);
            real = true;
        }
    }
    mine_write_row(a, row_item, r, i, j, 0.0f, real ? 1.0f : 0.0f);
}

// Counting pass, step 1 (one thread): offsets[g + 1] = offsets[g] + count[g]; `start` (n + 1 ints) keeps them for step 2.
MINE_FN void mine_scan_offsets(const MineArgs& a, const int* count, int* start) {
    int run = 0;
    for (int g = 0; g < a.n; ++g) {
        start[g] = run;
        a.seg_offsets[g] = run;
        run += count[g];
    }
    start[a.n] = run;
    a.seg_offsets[a.n] = run;
}

// Counting pass, step 2, one lane: row r belongs to the item whose group starts at `base` (rows before r already counted in it)
// and is number mine_rank(mask, lane) of this wave's 64 rows of that item: ascending pair number inside an item.
MINE_FN void mine_place_row(const MineArgs& a, int base, uint64_t mask, int lane, int r) {
    const int slot = base + mine_rank(mask, lane);
    if (slot < 0 || slot >= a.capacity) return;
    a.seg_order[slot] = r;
}
