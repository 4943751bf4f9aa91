// Host check of the exact selection of csrc/rank_lists.hip: the text of csrc/rank_key.h (order_bits / make_key / rank_value and the
// digit, bin and cut arithmetic) driven in the kernel's schedule - the passes of sel_pass, a histogram of SEL_BINS counters, the cut
// by SEL_THREADS threads of SEL_PER_THREAD bins each, the stop rule, the gather in the order of the row walk into a buffer of exactly
// SEL_CAND keys - over exactly-sized heap blocks, against std::stable_sort with a comparator written on the floats themselves.
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vit-ed_amd/csrc tools/ranklists_host_check.cpp
//
// A stand-alone program with its own main: it never goes through Python and never runs on a GPU.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <numeric>
#include <vector>

#include "rank_key.h"

using namespace rank_key;

static int failures = 0;

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            ++failures;                           \
            std::printf("FAILED %s: ", #cond);    \
            std::printf(__VA_ARGS__);             \
            std::printf("\n");                    \
        }                                         \
    } while (0)

// a < b in the order of the lists: NaN after everything, -0 == +0; ties are left to the stable sort
static bool value_less(float a, float b) {
    if (std::isnan(a)) return false;
    if (std::isnan(b)) return true;
    return a < b;
}

struct Lists {
    std::vector<int> idx;
    std::vector<uint32_t> val_bits;
    int passes = 0, candidates = 0;
};

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

// The kernel's schedule for one row.  T: the matrix dtype; head / vn: the unaligned head of the row and the elements of a 16-byte vector.
template <typename T> static Lists select_row(const std::vector<T>& row, bool sim, int k, int skip, int head, int vn) {
    const int64_t n = (int64_t)row.size();
    const uint32_t K = (uint32_t)(k + skip);
    auto key_at = [&](int64_t j) { return make_key(rank_value<T>((float)row[(size_t)j], sim), j); };
    Lists out;
    uint64_t bound = 0;
    uint32_t below = 0, in_bin = 0;
    SelPass last = {0, 0};
    const int passes = sel_num_passes(n);
    for (int p = 0; p < passes; ++p) {
        const SelPass ps = sel_pass(p, n);
        CHECK(ps.bits >= 1 && ps.bits <= SEL_DIGIT && ps.shift >= 0 && ps.shift + ps.bits <= 64, "pass %d of n %lld: shift %d bits %d", p,
              (long long)n, ps.shift, ps.bits);
        std::unique_ptr<uint32_t[]> hist(new uint32_t[SEL_BINS]());
        for (int64_t j = 0; j < n; ++j) {
            const uint64_t key = key_at(j);
            if (sel_match(key, bound, ps)) ++hist[sel_digit(key, ps)];
        }
        int found = 0, cut_bin = 0;
        uint32_t base = 0, cut_before = 0;
        for (int t = 0; t < SEL_THREADS; ++t) {
            int bin;
            uint32_t before;
            if (sel_cut(hist.get() + t * SEL_PER_THREAD, SEL_PER_THREAD, base, K - below, &bin, &before)) {
                ++found;
                cut_bin = t * SEL_PER_THREAD + bin;
                cut_before = before;
            }
            for (int e = 0; e < SEL_PER_THREAD; ++e) base += hist[t * SEL_PER_THREAD + e];
        }
        CHECK(found == 1, "pass %d: %d threads report the cut", p, found);
        if (found != 1) return out;
        bound |= (uint64_t)cut_bin << ps.shift;
        below += cut_before;
        in_bin = hist[cut_bin];
        last = ps;
        ++out.passes;
        if (sel_fits(below, in_bin)) break;
    }
    CHECK(sel_fits(below, in_bin) && below < K && below + in_bin >= K, "n %lld K %u: below %u in_bin %u after %d passes", (long long)n, K,
          below, in_bin, out.passes);

    // gather in the order of the walk: the head / tail step, then steps of SEL_THREADS vectors
    std::unique_ptr<uint64_t[]> cand(new uint64_t[SEL_CAND]);
    uint32_t gathered = 0;
    bool overflow = false;
    std::vector<char> seen((size_t)n, 0);
    auto take = [&](int64_t j) {
        CHECK(j >= 0 && j < n && !seen[(size_t)j], "column %lld walked twice or out of range", (long long)j);
        if (j < 0 || j >= n) return;
        seen[(size_t)j] = 1;
        const uint64_t key = key_at(j);
        if (!sel_take(key, bound, last)) return;
        if (gathered < (uint32_t)SEL_CAND) cand[gathered++] = key; else overflow = true;
    };
    const int64_t h = std::min<int64_t>(n, head), nvec = (n - h) / vn, tail0 = h + nvec * vn;
    CHECK(h + (n - tail0) <= SEL_THREADS, "head + tail exceed one step");
    for (int t = 0; t < SEL_THREADS; ++t) {
        if (t < h) take(t);
        else if (tail0 + (t - h) < n) take(tail0 + (t - h));
    }
    for (int64_t q0 = 0; q0 < nvec; q0 += SEL_THREADS)
        for (int t = 0; t < SEL_THREADS; ++t)
            if (q0 + t < nvec)
                for (int e = 0; e < vn; ++e) take(h + (q0 + t) * vn + e);
    CHECK(std::all_of(seen.begin(), seen.end(), [](char c) { return c == 1; }), "a column was not walked");
    CHECK(!overflow && gathered == below + in_bin, "gathered %u, expected %u", gathered, below + in_bin);
    out.candidates = (int)gathered;
    std::sort(cand.get(), cand.get() + gathered);
    for (uint32_t s = (uint32_t)skip; s < K && s < gathered; ++s) {
        const int64_t j = (int64_t)(cand[s] & 0xffffffffu);
        out.idx.push_back((int)j);
        out.val_bits.push_back(bits_of(rank_value<T>((float)row[(size_t)j], sim)));
    }
    return out;
}

template <typename T> static void check_row(const char* name, const std::vector<T>& row, bool sim, int k, int skip) {
    const int n = (int)row.size();
    std::vector<float> v((size_t)n);
    for (int j = 0; j < n; ++j) v[(size_t)j] = sim ? (float)(T)(1.0f - (float)row[(size_t)j]) : (float)row[(size_t)j];
    std::vector<int> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return value_less(v[(size_t)a], v[(size_t)b]); });
    const int vn = 16 / (int)sizeof(T);
    for (int head : {0, 1, vn - 1}) {
        const Lists got = select_row(row, sim, k, skip, head, vn);
        CHECK((int)got.idx.size() == k, "%s: %zu of %d elements", name, got.idx.size(), k);
        CHECK(got.passes <= sel_num_passes(n) && got.candidates <= SEL_CAND, "%s: %d passes, %d candidates", name, got.passes, got.candidates);
        for (int s = 0; s < k && s < (int)got.idx.size(); ++s) {
            const int want = order[(size_t)(s + skip)];
            if (got.idx[(size_t)s] != want || got.val_bits[(size_t)s] != bits_of(v[(size_t)want])) {
                CHECK(false, "%s (head %d, sim %d): position %d is column %d, expected %d", name, head, (int)sim, s, got.idx[(size_t)s], want);
                break;
            }
        }
    }
    std::printf("%-44s n %6d k %4d skip %d sim %d ok\n", name, n, k, skip, (int)sim);
}

static uint32_t rng_state = 20261020u;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

template <typename T> static std::vector<T> random_row(int n, int levels) {
    std::vector<T> r((size_t)n);
    for (auto& x : r) x = (T)((float)(rnd() % (uint32_t)levels) / (float)levels);
    return r;
}

template <typename T> static void cases(const char* tname) {
    char name[128];
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int sim = 0; sim < 2; ++sim) {
        for (int skip = 0; skip < 2; ++skip) {
            for (int n : {2, 7, 8 * 256 + 3}) {
                for (int k : {1, n - skip}) {
                    if (k > SEL_MAX_K || k < 1) continue;
                    std::snprintf(name, sizeof name, "%s random", tname);
                    check_row(name, random_row<T>(n, 1000), sim != 0, k, skip);
                }
            }
            std::snprintf(name, sizeof name, "%s random, coarse levels", tname);
            check_row(name, random_row<T>(8 * 256 + 3, 5), sim != 0, 300, skip);
            std::snprintf(name, sizeof name, "%s k = 1024 at n = 1500", tname);
            check_row(name, random_row<T>(1500, 700), sim != 0, SEL_MAX_K, skip);
            std::snprintf(name, sizeof name, "%s one repeated value", tname);
            check_row(name, std::vector<T>(5000, (T)0.25f), sim != 0, 100, skip);
            check_row(name, std::vector<T>(70000, (T)1.0f), sim != 0, SEL_MAX_K, skip);       // two column digits
            check_row(name, std::vector<T>(2048, (T)1.0f), sim != 0, 7, skip);                // the whole row fits the buffer
            check_row(name, std::vector<T>(2049, (T)1.0f), sim != 0, 7, skip);                // ... and just does not
            {
                std::vector<T> r = random_row<T>(5000, 900);                                  // 4,000 of 5,000 equal, below some and above others
                for (int j = 0; j < 5000; ++j)
                    if (j % 5) r[(size_t)j] = (T)0.5f;
                std::snprintf(name, sizeof name, "%s 4000 of 5000 equal", tname);
                check_row(name, r, sim != 0, 100, skip);
                check_row(name, r, sim != 0, SEL_MAX_K, skip);
            }
            {
                std::vector<T> r(3000);                                                       // scores saturated to exactly 0 and 1
                for (int j = 0; j < 3000; ++j) r[(size_t)j] = (T)((rnd() % 100) < 3 ? 1.0f : 0.0f);
                std::snprintf(name, sizeof name, "%s saturated 0 / 1", tname);
                check_row(name, r, sim != 0, 10, skip);
                check_row(name, r, sim != 0, 200, skip);
            }
            {
                std::vector<T> r = random_row<T>(300, 50);                                    // special values, the minimum off the diagonal
                const float special[] = {nan, inf, -inf, -0.0f, 0.0f, nan, -1.5f, inf, -0.0f};
                for (int j = 0; j < 300; j += 3) r[(size_t)j] = (T)special[(j / 3) % 9];
                std::snprintf(name, sizeof name, "%s NaN, inf, -inf, -0", tname);
                check_row(name, r, sim != 0, 1, skip);
                check_row(name, r, sim != 0, 300 - skip, skip);
                check_row(name, std::vector<T>(9, (T)nan), sim != 0, 9 - skip, skip);
            }
        }
    }
}

int main() {
    // the digit schedule: covers order_bits and every column bit, top down, without a gap inside either word
    for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)2048, (int64_t)2049, (int64_t)20000, (int64_t)(1 << 22) + 1, (int64_t)INT32_MAX - 1}) {
        const int c = sel_column_bits(n);
        CHECK(c >= 1 && c <= 31 && (((int64_t)1 << c) >= n) && (c == 1 || ((int64_t)1 << (c - 1)) < n), "column bits of %lld: %d", (long long)n, c);
        int next = 64;
        for (int p = 0; p < sel_num_passes(n); ++p) {
            const SelPass ps = sel_pass(p, n);
            if (p == 3) {
                CHECK(next == 32, "the value digits end at bit %d", next);
                next = c;
            }
            CHECK(ps.shift + ps.bits == next && ps.bits >= 1, "n %lld pass %d: shift %d bits %d, expected the top at %d", (long long)n, p,
                  ps.shift, ps.bits, next);
            next = ps.shift;
        }
        CHECK(next == 0, "n %lld: the digits end at bit %d", (long long)n, next);
    }
    CHECK(order_bits(-0.0f) == order_bits(0.0f) && order_bits(std::nanf("")) == 0xffffffffu, "order_bits of -0 / NaN");
    CHECK(order_bits(std::numeric_limits<float>::infinity()) < 0xffffffffu && order_bits(-1.0f) < order_bits(-0.5f), "order_bits order");

    cases<float>("fp32");
    cases<_Float16>("fp16");
    if (failures) {
        std::printf("ranklists_host_check FAILED: %d\n", failures);
        return 1;
    }
    std::printf("ranklists_host_check ok\n");
    return 0;
}
