// Host build of the pair mining of vited_mine_pairs (csrc/pair_mine.h) for the address and undefined-behaviour sanitizers: the
// very text the HIP kernel runs, driven lane by lane the way pair_mine.hip drives it (1,024 threads, ballots formed over 64
// lanes, the same loops), over the cases of tests/mine_cases.py with exactly-sized heap buffers, and compared with a naive double
// loop plus std::stable_sort.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vit-ed_amd/csrc tools/mine_host_check.cpp -o mine_host_check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pair_mine.h"

struct Result {
    std::vector<int64_t> groups, seg_index, seg_order, seg_offsets;
    std::vector<float> labels, weights;
    int32_t counts[5];
};

// the kernel's schedule on the host: exactly-sized heap blocks stand in for the outputs and for every LDS array
static void run_phases(const std::vector<int64_t>& targets, const std::vector<float>& keys, double neg_per_pos, int ordered, int capacity,
                       Result& out) {
    const int n = (int)targets.size(), size = mine_sort_size(n);
    int64_t* groups = (int64_t*)malloc(sizeof(int64_t) * 2 * capacity);
    float* labels = (float*)malloc(sizeof(float) * capacity);
    float* weights = (float*)malloc(sizeof(float) * capacity);
    int64_t* seg_index = (int64_t*)malloc(sizeof(int64_t) * capacity);
    int64_t* seg_order = (int64_t*)malloc(sizeof(int64_t) * capacity);
    int64_t* seg_offsets = (int64_t*)malloc(sizeof(int64_t) * (n + 1));
    int32_t* counts = (int32_t*)malloc(sizeof(int32_t) * 5);
    memset(groups, 0xff, sizeof(int64_t) * 2 * capacity);      // -1 / NaN: an unwritten element shows
    memset(labels, 0xff, sizeof(float) * capacity);
    memset(weights, 0xff, sizeof(float) * capacity);
    memset(seg_index, 0xff, sizeof(int64_t) * capacity);
    memset(seg_order, 0xff, sizeof(int64_t) * capacity);
    memset(seg_offsets, 0xff, sizeof(int64_t) * (n + 1));
    memset(counts, 0xff, sizeof(int32_t) * 5);
    uint64_t* words = (uint64_t*)malloc(sizeof(uint64_t) * size);
    int64_t* tgt = (int64_t*)malloc(sizeof(int64_t) * n);
    float* key = (float*)malloc(sizeof(float) * n * n);
    int* count = (int*)calloc(n, sizeof(int));
    int* start = (int*)malloc(sizeof(int) * (n + 1));
    uint8_t* row_item = (uint8_t*)malloc(capacity);
    memcpy(tgt, targets.data(), sizeof(int64_t) * n);
    memcpy(key, keys.data(), sizeof(float) * n * n);

    MineArgs a = {};
    a.targets = tgt; a.keys = key; a.n = n; a.ordered = ordered; a.capacity = capacity; a.neg_per_pos = neg_per_pos;
    a.groups = groups; a.labels = labels; a.weights = weights; a.seg_index = seg_index; a.seg_order = seg_order;
    a.seg_offsets = seg_offsets; a.counts = counts;

    // phase 1
    int npos = 0, ncand = 0;
    std::vector<int> kind(MINE_THREADS);
    for (int base = 0; base < size; base += MINE_THREADS) {
        int wave_total[MINE_WAVES] = {};
        uint64_t pos_mask[MINE_WAVES] = {};
        for (int t = 0; t < MINE_THREADS; ++t) {
            const int c = base + t;
            kind[t] = c < size ? mine_classify(tgt, n, ordered, c) : 0;
            if (c < size) words[c] = mine_sort_word(kind[t] == MINE_CAND ? key[c] : 0.0f, c, kind[t] == MINE_CAND);
            if (kind[t] == MINE_POS) pos_mask[t / MINE_WAVE] |= (uint64_t)1 << (t % MINE_WAVE);
            ncand += kind[t] == MINE_CAND;
        }
        for (int w = 0; w < MINE_WAVES; ++w) wave_total[w] = __builtin_popcountll(pos_mask[w]);
        int all = 0;
        for (int t = 0; t < MINE_THREADS; ++t) {
            const int wave = t / MINE_WAVE, lane = t % MINE_WAVE;
            int before = 0;
            all = 0;
            for (int w = 0; w < MINE_WAVES; ++w) {
                before += w < wave ? wave_total[w] : 0;
                all += wave_total[w];
            }
            if (kind[t] == MINE_POS) mine_emit_positive(a, row_item, base + t, npos + before + mine_rank(pos_mask[wave], lane));
        }
        npos += all;
    }
    const MineCounts m = mine_counts(npos, ncand, neg_per_pos, capacity);
    // phase 2
    if (m.neg_rows > 0)
        for (int k = 2; k <= size; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1)
                for (int p = 0; p < size / 2; ++p) mine_bitonic_pair(words, p, k, j);
    // phase 3
    for (int r = m.pos_rows; r < capacity; ++r) mine_emit_tail(a, m, words, row_item, r);
    for (int e = 0; e < 5; ++e) counts[e] = m.out[e];
    for (int r = 0; r < capacity; ++r) count[row_item[r]] += 1;
    mine_scan_offsets(a, count, start);
    for (int g = 0; g < n; ++g) {
        int base = start[g];
        for (int b = 0; b < capacity; b += MINE_WAVE) {
            uint64_t mask = 0;
            for (int lane = 0; lane < MINE_WAVE; ++lane)
                if (b + lane < capacity && row_item[b + lane] == g) mask |= (uint64_t)1 << lane;
            for (int lane = 0; lane < MINE_WAVE; ++lane)
                if ((mask >> lane) & 1) mine_place_row(a, base, mask, lane, b + lane);
            base += __builtin_popcountll(mask);
        }
    }

    out.groups.assign(groups, groups + 2 * capacity);
    out.labels.assign(labels, labels + capacity);
    out.weights.assign(weights, weights + capacity);
    out.seg_index.assign(seg_index, seg_index + capacity);
    out.seg_order.assign(seg_order, seg_order + capacity);
    out.seg_offsets.assign(seg_offsets, seg_offsets + n + 1);
    memcpy(out.counts, counts, sizeof(out.counts));
    free(groups); free(labels); free(weights); free(seg_index); free(seg_order); free(seg_offsets); free(counts);
    free(words); free(tgt); free(key); free(count); free(start); free(row_item);
}

// the rule restated: a double loop, std::stable_sort of the candidates by key, truncation, a stable grouping by item
static void naive(const std::vector<int64_t>& targets, const std::vector<float>& keys, double neg_per_pos, int ordered, int capacity,
                  Result& out) {
    const int n = (int)targets.size();
    std::vector<int> pos, cand;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            if (i == j) continue;
            if (targets[i] == targets[j]) {
                if (i < j) pos.push_back(i * n + j);
            } else if (ordered || i < j) {
                cand.push_back(i * n + j);
            }
        }
    std::stable_sort(cand.begin(), cand.end(), [&](int x, int y) { return keys[x] < keys[y]; });
    const double want = neg_per_pos * (double)pos.size();
    long keep = want > 0 ? (want >= (double)cand.size() ? (long)cand.size() : (long)want) : 0;
    const int pos_rows = std::min<long>((long)pos.size(), capacity), neg_rows = (int)std::min<long>(keep, capacity - pos_rows);
    out.groups.assign(2 * capacity, 0);
    out.labels.assign(capacity, 0.f);
    out.weights.assign(capacity, 0.f);
    for (int r = 0; r < pos_rows + neg_rows; ++r) {
        const int c = r < pos_rows ? pos[r] : cand[r - pos_rows];
        out.groups[2 * r] = c / n;
        out.groups[2 * r + 1] = c % n;
        out.labels[r] = r < pos_rows ? 1.f : 0.f;
        out.weights[r] = 1.f;
    }
    out.seg_index.resize(capacity);
    for (int r = 0; r < capacity; ++r) out.seg_index[r] = out.groups[2 * r + 1];
    out.seg_order.clear();
    out.seg_offsets.assign(n + 1, 0);
    for (int g = 0; g < n; ++g) {
        for (int r = 0; r < capacity; ++r)
            if (out.seg_index[r] == g) out.seg_order.push_back(r);
        out.seg_offsets[g + 1] = (int64_t)out.seg_order.size();
    }
    out.counts[0] = (int32_t)pos.size();
    out.counts[1] = (int32_t)cand.size();
    out.counts[2] = neg_rows;
    out.counts[3] = pos_rows + neg_rows;
    out.counts[4] = (int32_t)(pos.size() + keep) - pos_rows - neg_rows;
}

static std::vector<float> make_keys(int n, unsigned seed, int levels) {
    std::vector<float> k((size_t)n * n);
    unsigned s = seed;
    for (auto& v : k) {
        s = s * 1664525u + 1013904223u;
        v = levels > 0 ? (float)((s >> 16) % (unsigned)levels) / (float)levels : (levels < 0 ? 0.f : (float)(s >> 8) / 16777216.f);
    }
    return k;
}

static int run_case(const char* name, const std::vector<int64_t>& targets, double neg_per_pos, int ordered, const int want[4]) {
    const int n = (int)targets.size();
    int bad = 0;
    Result ref0;
    naive(targets, make_keys(n, 7u + n, 0), neg_per_pos, ordered, MINE_MAX_CAPACITY, ref0);
    const int pairs = ref0.counts[3];
    if (ref0.counts[0] != want[0] || ref0.counts[1] != want[1] || ref0.counts[2] != want[2] || pairs != want[3]) {
        printf("%-34s counts %d / %d / %d -> %d, expected %d / %d / %d -> %d\n", name, ref0.counts[0], ref0.counts[1], ref0.counts[2], pairs,
               want[0], want[1], want[2], want[3]);
        ++bad;
    }
    std::vector<int> capacities = {std::max(pairs, 1), pairs + 5};
    if (ref0.counts[2] > 1) capacities.push_back(pairs - ref0.counts[2] / 2);       // cuts into the negatives
    if (ref0.counts[0] > 1) capacities.push_back(ref0.counts[0] - 1);               // cuts into the positives
    for (int levels : {0, 4, -1})                                                    // uniform keys, four values, all zero
        for (int capacity : capacities) {
            const std::vector<float> keys = make_keys(n, 7u + n, levels);
            Result got, ref;
            run_phases(targets, keys, neg_per_pos, ordered, capacity, got);
            naive(targets, keys, neg_per_pos, ordered, capacity, ref);
            const bool same = got.groups == ref.groups && got.seg_index == ref.seg_index && got.seg_order == ref.seg_order &&
                              got.seg_offsets == ref.seg_offsets && memcmp(got.counts, ref.counts, sizeof(ref.counts)) == 0 &&
                              memcmp(got.labels.data(), ref.labels.data(), sizeof(float) * capacity) == 0 &&
                              memcmp(got.weights.data(), ref.weights.data(), sizeof(float) * capacity) == 0;
            if (!same) {
                printf("%-34s capacity %d key levels %d: MISMATCH\n", name, capacity, levels);
                ++bad;
            }
        }
    printf("%-34s %d / %d / %d -> %d pairs: %s\n", name, ref0.counts[0], ref0.counts[1], ref0.counts[2], pairs, bad ? "FAILED" : "ok");
    return bad;
}

int main() {
    auto classes = [](int n, int k, bool blocks) {
        std::vector<int64_t> t(n);
        for (int i = 0; i < n; ++i) t[i] = blocks ? i / (n / k) : i % k;
        return t;
    };
    int bad = 0;
    { const int w[4] = {24, 252, 48, 72}; bad += run_case("24 = 8 x 3, hisfrag", classes(24, 8, true), 2.0, 0, w); }
    { const int w[4] = {24, 504, 24, 48}; bad += run_case("24 = 8 x 3, michigan", classes(24, 8, true), 1.0, 1, w); }
    { const int w[4] = {9, 12, 12, 21}; bad += run_case("7, 2 classes alternating", classes(7, 2, false), 2.0, 0, w); }
    { const int w[4] = {0, 10, 0, 0}; bad += run_case("5 of 5 classes", classes(5, 5, false), 2.0, 0, w); }
    { const int w[4] = {15, 0, 0, 15}; bad += run_case("6 of one class", std::vector<int64_t>(6, 3), 2.0, 0, w); }
    { const int w[4] = {0, 0, 0, 0}; bad += run_case("1 image", {9}, 2.0, 0, w); }
    { const int w[4] = {2, 4, 4, 6}; bad += run_case("[0, 0, 1, 1]", {0, 0, 1, 1}, 2.0, 0, w); }
    { const int w[4] = {4, 11, 8, 12};
      bad += run_case("ids below 0 and above 2^32", {-5, (int64_t)1 << 40, -5, 7, (int64_t)1 << 40, -5}, 2.0, 0, w); }
    { const int w[4] = {4032, 8192, 8064, 12096}; bad += run_case("128, 2 classes, ordered", classes(128, 2, false), 2.0, 1, w); }
    { const int w[4] = {4032, 4096, 4096, 8128}; bad += run_case("128, 2 classes, upper", classes(128, 2, false), 2.0, 0, w); }
    { const int w[4] = {0, 21, 0, 0}; bad += run_case("7 of 7 classes (49 cells)", classes(7, 7, false), 2.0, 0, w); }
    { const int w[4] = {6, 9, 9, 15}; bad += run_case("6, 2 classes (36 cells)", classes(6, 2, false), 2.0, 0, w); }
    printf(bad ? "mine_host_check FAILED\n" : "mine_host_check ok\n");
    return bad ? 1 : 0;
}
