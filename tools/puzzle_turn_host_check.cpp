// Stand-alone host program: the index rules of csrc/puzzle_turn.h - the text the kernels of csrc/puzzle_turn.hip and the turned-pair
// scatter of csrc/puzzle_compat.hip run - over the cases of a binary case file, for a build under the sanitizers
// (tests/test_puzzle_rot.py compiles it with -fsanitize=address,undefined).
//
//   puzzle_turn_host_check cases.bin out.bin
//
// cases.bin (little endian): int32 geometries, then per geometry 3 int32 (chans, S, p); int32 puzzles, then per puzzle int64 n, int64 m
// and m pairs (i, jt) int64.
// out.bin: per geometry and turn k = 0..3 the int64 array [G * G, chans p p] (G = S / p) that patchify writes for the turned image,
//   each entry the source element of the upright [chans, S, S] image (every strip element is placed through
//   strip_element; the program itself refuses an element outside the image or the strip, and a strip that is not filled exactly once);
//   then 4 x 4 x 2 int32: (si, sj) of every (k, bin), 4 x 4 int32: pair_turn(si, sj), 4 x 4 int32: moved_side(s, k);
//   per puzzle and pair int32 in-range flag and 4 int64 Dq2 offsets of its bins (-1 where the pair is refused).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "puzzle_turn.h"

namespace pt = puzzle_turn;

template <typename T> static bool get(FILE* f, std::vector<T>& v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}

template <typename T> static bool put(FILE* f, const std::vector<T>& v) {
    return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
    if (argc != 3) return fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]), 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return fprintf(stderr, "cannot open the files\n"), 2;
    std::vector<int32_t> head;
    if (!get(in, head, 1)) return fprintf(stderr, "empty case file\n"), 2;
    const int geometries = head[0];
    for (int q = 0; q < geometries; ++q) {
        if (!get(in, head, 3)) return fprintf(stderr, "geometry %d: short header\n", q), 2;
        const int chans = head[0], S = head[1], p = head[2];
        if (chans < 1 || S < 1 || p < 1 || S % p) return fprintf(stderr, "geometry %d: bad sizes\n", q), 2;
        const int G = S / p, Kp = chans * p * p, total = chans * p * S;
        const int64_t image = (int64_t)chans * S * S;
        for (int k = 0; k < 4; ++k) {
            std::vector<int64_t> rows((size_t)G * G * Kp, -1);
            for (int py = 0; py < G; ++py) {
                int64_t* strip = rows.data() + (size_t)py * G * Kp;
                for (int e = 0; e < total; ++e) {
                    const pt::StripElement at = pt::strip_element(chans, S, p, k, py, e);
                    if (at.src < 0 || at.src >= image || at.dst < 0 || at.dst >= (int64_t)G * Kp || at.c < 0 || at.c >= chans)
                        return fprintf(stderr, "geometry %d turn %d strip %d element %d leaves its array\n", q, k, py, e), 1;
                    if (at.src / ((int64_t)S * S) != at.c) return fprintf(stderr, "geometry %d: element %d changes its channel\n", q, e), 1;
                    if (strip[at.dst] != -1) return fprintf(stderr, "geometry %d turn %d strip %d: element %d written twice\n", q, k, py, e), 1;
                    strip[at.dst] = at.src;
                }
            }
            for (int64_t v : rows)
                if (v < 0) return fprintf(stderr, "geometry %d turn %d: an output element is never written\n", q, k), 1;
            if (!put(out, rows)) return fprintf(stderr, "write failed\n"), 2;
        }
    }
    std::vector<int32_t> sides, turns, moved;
    for (int k = 0; k < 4; ++k)
        for (int b = 0; b < 4; ++b) sides.push_back(pt::bin_side_i(b)), sides.push_back(pt::bin_side_j(b, k));
    for (int si = 0; si < 4; ++si)
        for (int sj = 0; sj < 4; ++sj) turns.push_back(pt::pair_turn(si, sj));
    for (int s = 0; s < 4; ++s)
        for (int k = 0; k < 4; ++k) moved.push_back(pt::moved_side(s, k));
    if (!put(out, sides) || !put(out, turns) || !put(out, moved)) return fprintf(stderr, "write failed\n"), 2;

    if (!get(in, head, 1)) return fprintf(stderr, "no puzzle count\n"), 2;
    const int puzzles = head[0];
    for (int q = 0; q < puzzles; ++q) {
        std::vector<int64_t> size, pairs;
        if (!get(in, size, 2) || size[0] < 2 || size[1] < 0 || !get(in, pairs, (size_t)(2 * size[1])))
            return fprintf(stderr, "puzzle %d: short or bad data\n", q), 2;
        const int64_t n = size[0], m = size[1];
        std::vector<int32_t> dq2((size_t)(16 * n * n), 0);         // the array a slot must stay inside: the sanitizer watches the store
        for (int64_t r = 0; r < m; ++r) {
            const int64_t i = pairs[2 * r], jt = pairs[2 * r + 1];
            std::vector<int32_t> ok(1, pt::pair_in_range(i, jt, n) ? 1 : 0);
            std::vector<int64_t> slots(4, -1);
            if (ok[0])
                for (int b = 0; b < 4; ++b) {
                    slots[b] = pt::dq2_slot(n, i, jt, b);
                    dq2[(size_t)slots[b]] += 1;
                }
            if (!put(out, ok) || !put(out, slots)) return fprintf(stderr, "write failed\n"), 2;
        }
    }
    fclose(in);
    if (fclose(out) != 0) return fprintf(stderr, "write failed\n"), 2;
    printf("puzzle_turn_host_check ok: %d geometries, %d puzzles\n", geometries, puzzles);
    return 0;
}
