// Host build of the patch-dropout index arithmetic (csrc/patch_keep.h) for the address and undefined-behaviour sanitizers: the very
// text the HIP kernels run, driven the way patch_keep.hip drives it - 256 "threads" striding over a row - on exactly-sized heap
// blocks: the ranking against std::stable_sort (random keys, planted ties, a constant row, -0 / +0, NaN), the patch of every kept
// row in both forms, hostile tables (indices far outside the range) and the inverse table.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vit-ed_amd/csrc tools/patchkeep_host_check.cpp -o patchkeep_host_check
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <vector>

#include "patch_keep.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {      // xorshift64*, in [-1, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) / (double)(1ull << 52) - 1.0;
}

static int failures = 0;
static void expect(bool ok, const char* what, int a, int b, long got, long want) {
    if (!ok) {
        ++failures;
        fprintf(stderr, "FAIL %s (%d, %d): got %ld want %ld\n", what, a, b, got, want);
    }
}

constexpr int THREADS = 256;

// kind: 0 random, 1 planted ties, 2 constant, 3 signed zeros, 4 some NaN, 5 descending
static void check_ranking(int L, int K, int kind) {
    float* keys = (float*)malloc(sizeof(float) * L);
    int* keep = (int*)malloc(sizeof(int) * K);
    for (int i = 0; i < K; ++i) keep[i] = -7;
    for (int i = 0; i < L; ++i) {
        float v = (float)(3.0 * uniform());
        if (kind == 1 && i % 3) v = (float)(i % 5);
        if (kind == 2) v = 0.25f;
        if (kind == 3) v = i % 2 ? -0.0f : 0.0f;
        if (kind == 4 && i % 4 == 1) v = std::numeric_limits<float>::quiet_NaN();
        if (kind == 5) v = (float)(L - i);
        keys[i] = v;
    }
    for (int t = 0; t < THREADS; ++t)               // keep_from_keys_kernel's loop, thread by thread
        for (int i = t; i < L; i += THREADS) {
            const int rank = pk_rank(keys, L, i);
            expect(rank >= 0 && rank < L, "rank in range", L, kind, rank, 0);
            if (rank < K) keep[rank] = i;
        }
    std::vector<int> order(L);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {        // torch's order: ascending, NaN last
        const bool an = std::isnan(keys[a]), bn = std::isnan(keys[b]);
        return an || bn ? (!an && bn) : keys[a] < keys[b];
    });
    for (int r = 0; r < K; ++r) expect(keep[r] == order[r], "keep == stable argsort", L, kind, keep[r], order[r]);
    free(keys);
    free(keep);
}

static void check_tables(int n_patches, int K, int lead, bool hostile) {
    const int batch = 5, R = pk_rows(K, lead), L = n_patches - lead;
    int* keep = (int*)malloc(sizeof(int) * batch * K);
    int* inv = (int*)malloc(sizeof(int) * batch * n_patches);
    for (int b = 0; b < batch; ++b) {
        std::vector<int> perm(L);
        std::iota(perm.begin(), perm.end(), 0);
        for (int i = L - 1; i > 0; --i) std::swap(perm[i], perm[(int)((uniform() + 1.0) * 0.5 * (i + 1)) % (i + 1)]);
        for (int r = 0; r < K; ++r) keep[b * K + r] = perm[r];
        if (hostile) {
            keep[b * K] = 0x7fffff00;
            keep[b * K + K - 1] = -0x7fffff00;
        }
    }
    for (int b = 0; b < batch; ++b) {
        int* mine = inv + b * n_patches;
        for (int t = 0; t < THREADS; ++t) pk_inverse_clear(mine, n_patches, t, THREADS);        // the barrier sits between the two loops
        for (int t = 0; t < THREADS; ++t) pk_inverse_fill(mine, keep + b * K, K, lead, n_patches, t, THREADS);
        int kept = 0;
        for (int r = 0; r < R; ++r) {
            const int p = pk_patch(keep + b * K, lead, r, n_patches);
            expect(p >= 0 && p < n_patches, "patch in range", n_patches, lead, p, 0);
            if (!hostile) {
                const int want = lead ? (r == 0 ? 0 : 1 + keep[b * K + r - 1]) : keep[b * K + r];
                expect(p == want, "patch of a kept row", n_patches, lead, p, want);
                expect(mine[p] == r, "inverse of a kept patch", n_patches, lead, mine[p], r);
            }
        }
        for (int p = 0; p < n_patches; ++p) {
            expect(mine[p] >= -1 && mine[p] < R, "inverse entry in range", n_patches, lead, mine[p], -1);
            kept += mine[p] >= 0;
        }
        if (!hostile) expect(kept == R, "kept patches counted", n_patches, lead, kept, R);
        if (lead) expect(mine[0] == 0 || hostile, "patch 0 leads", n_patches, lead, mine[0], 0);
    }
    free(keep);
    free(inv);
}

int main() {
    const int shapes[][2] = {{1, 1}, {3, 1}, {3, 3}, {63, 31}, {64, 44}, {64, 6}, {257, 100}, {1023, 511}, {1024, 512}, {4096, 409}};
    int rows = 0;
    for (const auto& s : shapes)
        for (int kind = 0; kind < 6; ++kind, ++rows) check_ranking(s[0], s[1], kind);
    const int grids[] = {4, 64, 1024};
    int tables = 0;
    for (int n : grids)
        for (int lead = 0; lead < 2; ++lead)
            for (int K : {1, (n - lead) / 2, n - lead})
                if (K >= 1)
                    for (int hostile = 0; hostile < 2; ++hostile, ++tables) check_tables(n, K, lead, hostile);
    if (failures) {
        fprintf(stderr, "patchkeep_host_check: %d failures\n", failures);
        return 1;
    }
    printf("patchkeep_host_check ok: %d ranked rows, %d keep tables (both forms, hostile indices included)\n", rows, tables);
    return 0;
}
