// The order every ranking kernel shares (rank_metrics.hip, rank_lists.hip; DESIGN.md sections 12 and 30), and the arithmetic of the
// exact selection of rank_lists.hip, written so that the device kernels and a host program under the sanitizers
// (tools/ranklists_host_check.cpp) compile the same text.
//
// Row i ranks its columns ascending by the 64-bit key (order_bits(v) << 32) | j: v = D[i, j], or T(1 - S[i, j]) when the matrix holds
// similarities (fp32 subtract, one rounding to the matrix dtype T).  Ties go to the lower column, every NaN sorts after +inf (all
// NaNs tie), -0 ties with +0: np.argsort(kind='stable').  No two keys of a row are equal, because no two columns are.
//
// The selection finds the first K keys of that order by a radix select.  Pass p histograms the digit (shift, bits) = sel_pass(p, n)
// of the keys that still match the boundary prefix found so far; sel_cut finds the bin that holds the K-th key; the passes end as
// soon as the keys ordered before that bin and the bin itself fit the candidate buffer together (sel_fits), and the candidates are
// the keys sel_take accepts.  The digits walk order_bits from the top (11, 11, 10 bits) and then the column, from the highest bit a
// column below n can have; the column bits above it are zero in every key and are never a digit.  The last pass ends at bit 0, where
// a bin holds one key, so the passes always end with at most K <= SEL_MAX_K + 1 candidates - whatever the ties.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define RK_FN __host__ __device__ __forceinline__
#else
#define RK_FN inline
#endif

namespace rank_key {

// Order-preserving 32-bit image of a float: every NaN maps above +inf (to one value, so NaNs tie and fall back to the column
// order), -0 ties with +0.
RK_FN uint32_t order_bits(float v) {
    if (v != v) return 0xffffffffu;
    if (v == 0.0f) v = 0.0f;
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

RK_FN uint64_t make_key(float v, int64_t j) { return ((uint64_t)order_bits(v) << 32) | (uint32_t)j; }

// The value the row is ranked by: D itself, or T(1 - S) (fp32 subtract, one rounding to T) when the matrix holds similarities.
template <typename T> RK_FN float rank_value(float v, bool from_similarity) {
    return from_similarity ? (float)(T)(1.0f - v) : v;
}

constexpr uint64_t PAD_KEY = ~0ull;          // above every real key (a real key's low word is a column index < 2^31)

// ---- the exact selection of rank_lists.hip
constexpr int SEL_THREADS = 256;
constexpr int SEL_DIGIT = 11;                // bits of a full digit
constexpr int SEL_BINS = 1 << SEL_DIGIT;     // 8 KB of LDS counters
constexpr int SEL_PER_THREAD = SEL_BINS / SEL_THREADS;
constexpr int SEL_CAND = 2048;               // candidate keys: 16 KB of LDS, one bitonic sort
constexpr int SEL_MAX_K = 1024;

struct SelPass { int shift, bits; };

// Bits a column index below n can have (at least 1).
RK_FN int sel_column_bits(int64_t n) {
    int c = 1;
    while (c < 31 && ((int64_t)1 << c) < n) ++c;
    return c;
}

RK_FN int sel_num_passes(int64_t n) { return 3 + (sel_column_bits(n) + SEL_DIGIT - 1) / SEL_DIGIT; }

// Digit p, from the top of the key down: order_bits in 11 + 11 + 10 bits, then the column's sel_column_bits(n) bits in digits of up to 11.
RK_FN SelPass sel_pass(int p, int64_t n) {
    if (p == 0) return {53, 11};
    if (p == 1) return {42, 11};
    if (p == 2) return {32, 10};
    const int left = sel_column_bits(n) - SEL_DIGIT * (p - 3);     // column bits not yet a digit
    const int bits = left < SEL_DIGIT ? left : SEL_DIGIT;
    return {left - bits, bits};
}

// Does the key agree with the boundary `bound` (the digits found so far, zero below them) above the digit of pass ps?
RK_FN bool sel_match(uint64_t key, uint64_t bound, SelPass ps) {
    const int hi = ps.shift + ps.bits;
    return hi >= 64 || (key >> hi) == (bound >> hi);
}

RK_FN int sel_digit(uint64_t key, SelPass ps) { return (int)((key >> ps.shift) & (((uint64_t)1 << ps.bits) - 1)); }

// One thread's part of the cut: h[0, cnt) are consecutive bins of which `base` keys lie in the bins before them.  When the need-th
// key (1-based, among the matching keys) falls into one of them: true, *bin = its offset in h, *before = the keys in earlier bins.
RK_FN bool sel_cut(const uint32_t* h, int cnt, uint32_t base, uint32_t need, int* bin, uint32_t* before) {
    for (int e = 0; e < cnt; ++e) {
        if (base < need && need - base <= h[e]) {
            *bin = e;
            *before = base;
            return true;
        }
        base += h[e];
    }
    return false;
}

// The passes end when the keys before the boundary bin and the bin itself fit the candidate buffer.
RK_FN bool sel_fits(uint32_t below, uint32_t in_bin) { return (uint64_t)below + in_bin <= (uint64_t)SEL_CAND; }

// A candidate: ordered before the boundary bin of the last pass, or inside it.
RK_FN bool sel_take(uint64_t key, uint64_t bound, SelPass last) { return (key >> last.shift) <= (bound >> last.shift); }

}  // namespace rank_key
