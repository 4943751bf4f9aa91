// Host build of elementwise token dropout (csrc/token_dropout.h) for the address and undefined-behaviour sanitizers: the very text the
// HIP kernel runs - Philox, the address arithmetic, the per-lane body - driven in the kernel's schedule (td_walk: "threads" of a
// grid striding over the pieces; a grid of ONE workgroup of 256 and a grid of several) over exactly-sized heap buffers whose outputs
// are pre-filled with 0xff bytes, against a double loop over a scalar Philox written out independently below:
//   the three known answers of Philox4x32-10; an element address above 2^34 (hi32 of the group index non-zero), which no tensor in
//   a test can reach; both dtypes, with and without a keep table, both lead values, in place and out of place, strided rows.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vit-ed_amd/csrc tools/tokendrop_host_check.cpp -o tokendrop_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "token_dropout.h"

static int failures = 0;
static void expect(bool ok, const char* what, long a, long b, long c) {
    if (!ok && ++failures <= 20) fprintf(stderr, "FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
}

// ---- the rule once more, one element at a time, sharing nothing with the header but the constants of the paper --------------------
static void philox_scalar(const uint32_t c[4], const uint32_t k[2], uint32_t out[4]) {
    uint32_t x0 = c[0], x1 = c[1], x2 = c[2], x3 = c[3], k0 = k[0], k1 = k[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t a = 0xD2511F53ull * x0, b = 0xCD9E8D57ull * x2;
        const uint32_t hi0 = (uint32_t)(a >> 32), lo0 = (uint32_t)a, hi1 = (uint32_t)(b >> 32), lo1 = (uint32_t)b;
        const uint32_t y0 = hi1 ^ x1 ^ k0, y1 = lo1, y2 = hi0 ^ x3 ^ k1, y3 = lo0;
        x0 = y0; x1 = y1; x2 = y2; x3 = y3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = x0; out[1] = x1; out[2] = x2; out[3] = x3;
}

static bool kept_scalar(int64_t e, uint32_t stream, uint64_t seed, uint32_t thr) {
    const uint64_t g = (uint64_t)e >> 2;
    const uint32_t c[4] = {(uint32_t)(g & 0xffffffffu), (uint32_t)(g >> 32), stream, 0u}, k[2] = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
    uint32_t w[4];
    philox_scalar(c, k, w);
    return w[e & 3] >= thr;
}

static void check_known_answers() {
    const uint32_t cases[3][10] = {
        {0, 0, 0, 0, 0, 0, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
        {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
        {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};
    for (int i = 0; i < 3; ++i) {
        uint32_t w[4] = {cases[i][0], cases[i][1], cases[i][2], cases[i][3]}, s[4];
        td_philox(w, cases[i][4], cases[i][5]);
        philox_scalar(cases[i], cases[i] + 4, s);
        for (int j = 0; j < 4; ++j) {
            expect(w[j] == cases[i][6 + j], "known answer (header)", i, j, w[j]);
            expect(s[j] == cases[i][6 + j], "known answer (scalar)", i, j, s[j]);
        }
    }
}

// ---- element addresses no tensor reaches: hi32(g) != 0 from e = 2^34 on -------------------------------------------------------------
static void check_far_addresses() {
    const uint64_t seed = 0x0123456789abcdefull;
    int differ = 0;
    for (int64_t e : {(int64_t)1 << 34, ((int64_t)1 << 34) + 4, ((int64_t)1 << 40) + 12, ((int64_t)3 << 45) + 8, INT64_MAX - 3}) {
        uint32_t w[4], lo[4];
        td_words(e, 1u, seed, w);
        td_words(e & 0x3ffffffffll, 1u, seed, lo);        // the same low bits with hi32(g) = 0: another counter, other words
        differ += memcmp(w, lo, sizeof w) != 0;
        for (int j = 0; j < 4; ++j)
            expect((w[j] >= 0x40000000u) == kept_scalar((e & ~(int64_t)3) + j, 1u, seed, 0x40000000u), "far address", (long)(e >> 32), j, w[j]);
    }
    expect(differ == 5, "hi32 of the group index reaches the counter", differ, 0, 0);
    // the address of the last channel group of a stream of 2^22 samples x 1025 tokens x 1024 channels: above 2^42, computed in int64
    const int64_t e = td_address(((int64_t)1 << 22) - 1, 1025, 1024, 1024, 1020);
    expect(e == ((((int64_t)1 << 22) - 1) * 1025 + 1024) * 1024 + 1020, "address arithmetic", (long)(e >> 32), 0, 0);
}

// ---- the schedule over real buffers -----------------------------------------------------------------------------------------------
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {      // xorshift64*, in [-1, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) / (double)(1ull << 52) - 1.0;
}

static float value_of(float v) { return v; }
static float value_of(uint16_t v) { return td_bf16_to_f32(v); }
static void make(float& o, float v) { o = v; }
static void make(uint16_t& o, float v) { o = td_f32_to_bf16(v); }
static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }
static bool same_bits(uint16_t a, uint16_t b) { return a == b; }

// T: float or uint16_t (bf16 bits); GROUPS as the launcher picks it; pad: extra elements per row (a row stride above dim)
template <typename T, typename Vec, int GROUPS>
static void check_walk(int64_t batch, int rows, int dim, int tokens, int K, int lead, bool table, bool in_place, int pad, int64_t threads,
                       uint32_t thr, float scale, uint64_t seed, uint32_t stream) {
    const int64_t rs = dim + pad, bs = (int64_t)(rows - 1) * rs + dim + pad, count = (batch - 1) * bs + (int64_t)(rows - 1) * rs + dim;
    T* in = (T*)aligned_alloc(16, (size_t)((count * sizeof(T) + 15) / 16 * 16));
    T* out = in_place ? in : (T*)aligned_alloc(16, (size_t)((count * sizeof(T) + 15) / 16 * 16));
    std::vector<T> orig((size_t)count);
    if (!in_place) memset(out, 0xff, (size_t)count * sizeof(T));
    for (int64_t i = 0; i < count; ++i) {
        float v = (float)(4.0 * uniform());
        if (i % 97 == 5) v = INFINITY;
        if (i % 101 == 7) v = -INFINITY;
        if (i % 103 == 9) v = NAN;
        make(in[i], v);
        orig[(size_t)i] = in[i];
    }
    int* keep = nullptr;
    if (table) {
        keep = (int*)malloc(sizeof(int) * (size_t)(batch * K));
        const int range = lead ? tokens - 1 : tokens - 1;       // indices behind the prefix slot
        for (int64_t b = 0; b < batch; ++b)
            for (int r = 0; r < K; ++r) keep[b * K + r] = (int)((7 * r + 3 * b + 1) % range);
        keep[0] = 0x7fffff00;                                   // hostile entries are clamped, never followed
        if (batch * K > 1) keep[batch * K - 1] = -5;
    }
    for (int64_t t = 0; t < threads; ++t)                       // token_dropout_kernel, thread by thread
        td_walk<T, Vec, GROUPS>(in, bs, rs, out, bs, rs, batch, rows, dim, tokens, stream, keep, K, lead, seed, thr, scale, t, threads);
    for (int64_t b = 0; b < batch; ++b)
        for (int r = 0; r < rows; ++r) {
            int t = r;
            if (table && r > 0) {                               // the rows as vited_tokens_kept lays them out, clamped
                const int n = lead ? tokens : tokens - 1;
                int p = keep[b * K + r - 1] + (lead ? 1 : 0);
                p = p < 0 ? 0 : (p > n - 1 ? n - 1 : p);
                t = lead ? p : p + 1;
            }
            for (int d = 0; d < dim; ++d) {
                const int64_t at = b * bs + (int64_t)r * rs + d;
                const bool kept = kept_scalar((b * tokens + t) * (int64_t)dim + d, stream, seed, thr);
                T want;
                make(want, kept ? value_of(orig[(size_t)at]) * scale : 0.0f);
                const bool nan_both = kept && std::isnan(value_of(want)) && std::isnan(value_of(out[at]));
                expect(nan_both || same_bits(out[at], want), "element", (long)b, r, d);
            }
            for (int d = dim; d < dim + pad && (b * bs + (int64_t)r * rs + d) < count; ++d) {     // the gaps between rows are not touched
                const int64_t at = b * bs + (int64_t)r * rs + d;
                T ff;
                memset(&ff, 0xff, sizeof ff);
                expect(same_bits(out[at], in_place ? orig[(size_t)at] : ff), "gap untouched", (long)b, r, d);
            }
        }
    free(keep);
    if (!in_place) free(out);
    free(in);
}

int main() {
    check_known_answers();
    check_far_addresses();
    int runs = 0;
    const uint32_t thr10 = 429496729u, thr50 = 2147483648u;
    const float s10 = (float)(1.0 / (1.0 - 0.1)), s50 = 2.0f;
    for (int in_place = 0; in_place < 2; ++in_place)
        for (int64_t threads : {256, 1024}) {                   // one workgroup; four
            // fp32: [3, 5, 36] (dim % 8 != 0, less than a wave), [2, 65, 384], [1, 3, 1024]; padded rows
            check_walk<float, TdF32x4, 1>(3, 5, 36, 5, 0, 0, false, in_place, 0, threads, thr10, s10, 0x1111ull, 0), ++runs;
            check_walk<float, TdF32x4, 1>(2, 65, 384, 65, 0, 0, false, in_place, 0, threads, thr50, s50, 0xfedcba9876543210ull, 1), ++runs;
            check_walk<float, TdF32x4, 1>(1, 3, 1024, 3, 0, 0, false, in_place, 8, threads, thr10, s10, ~0ull, 1), ++runs;
            // bf16: one group per lane (dim % 8 != 0) and two
            check_walk<uint16_t, TdBf16x4, 1>(3, 5, 36, 5, 0, 0, false, in_place, 4, threads, thr50, s50, 77ull, 0), ++runs;
            check_walk<uint16_t, TdBf16x4, 2>(2, 65, 384, 65, 0, 0, false, in_place, 0, threads, thr10, s10, 0x8000000000000000ull, 1), ++runs;
            check_walk<uint16_t, TdBf16x4, 2>(1, 3, 1024, 3, 0, 0, false, in_place, 8, threads, thr10, s10, 5ull, 0), ++runs;
            // keep tables [2, 3] over 9 tokens (4 rows), both forms, both dtypes; and [3, 31] over 64
            for (int lead = 0; lead < 2; ++lead) {
                check_walk<float, TdF32x4, 1>(2, 4, 36, 9, 3, lead, true, in_place, 0, threads, thr50, s50, 99ull, (uint32_t)(1 - lead)), ++runs;
                check_walk<uint16_t, TdBf16x4, 2>(2, 4, 64, 9, 3, lead, true, in_place, 0, threads, thr10, s10, 98ull, (uint32_t)(1 - lead)), ++runs;
                check_walk<float, TdF32x4, 1>(3, 32, 384, 64, 31, lead, true, in_place, 4, threads, thr10, s10, 97ull, (uint32_t)(1 - lead)), ++runs;
            }
        }
    if (failures) {
        fprintf(stderr, "tokendrop_host_check: %d failures\n", failures);
        return 1;
    }
    printf("tokendrop_host_check ok: 3 known answers, far addresses, %d streams (fp32 / bf16, tables in both forms, in place and apart)\n", runs);
    return 0;
}
