// Stand-alone host program: the type-2 rules of csrc/puzzle_pixels.h - the text the kernels of csrc/puzzle_pixels.hip run - over the cases
// of a binary case file, for a build under the sanitizers (tests/test_puzzle_type2.py compiles it with -fsanitize=address,undefined).
//
//   puzzle_type2_host_check cases.bin out.bin
//
// cases.bin (little endian): int32 count, then per case 6 int32 (n, We, P, rows, cols, marker), the pieces uint8 [n, We, We, 3], cells
// int32 [rows * cols] and rotations int32 [rows * cols].  Per case out.bin receives Dq2 int32 [4, n, n, 4] (the three kinds of strips,
// then every pairing through pairing_reversed and strip_distance) and the board uint8 [rows P, cols P, 3] of board_byte_rotated.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "puzzle_pixels.h"

namespace pp = puzzle_pixels;

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
    const int count = head[0];
    for (int q = 0; q < count; ++q) {
        if (!get(in, head, 6)) return fprintf(stderr, "case %d: short header\n", q), 2;
        const int64_t n = head[0], rows = head[3], cols = head[4];
        const int We = head[1], P = head[2], marker = head[5];
        if (n < 2 || We < 2 || P < We || rows * cols != n) return fprintf(stderr, "case %d: bad sizes\n", q), 2;
        std::vector<uint8_t> pieces;
        std::vector<int32_t> cells, rotations;
        if (!get(in, pieces, (size_t)(n * We * We * 3)) || !get(in, cells, (size_t)n) || !get(in, rotations, (size_t)n))
            return fprintf(stderr, "case %d: short data\n", q), 2;

        const int padded = pp::strip_padded(We);
        std::vector<uint16_t> strips((size_t)(3 * 4 * n * padded));
        for (int kind = 0; kind < 3; ++kind)
            for (int s = 0; s < 4; ++s)
                for (int64_t i = 0; i < n; ++i)
                    for (int k = 0; k < padded; ++k) {
                        const uint8_t* piece = pieces.data() + i * We * We * 3;
                        strips[(size_t)(((kind * 4 + s) * n + i) * padded + k)] =
                            kind == 0 ? pp::strip_prediction(piece, We, s, k)
                                      : (kind == 1 ? pp::strip_border(piece, We, s, k) : pp::strip_border_reversed(piece, We, s, k));
                    }
        std::vector<int32_t> dq2((size_t)(16 * n * n));
        for (int si = 0; si < 4; ++si)
            for (int64_t i = 0; i < n; ++i)
                for (int64_t j = 0; j < n; ++j)
                    for (int sj = 0; sj < 4; ++sj) {
                        const int kind = pp::pairing_reversed(si, sj) ? 2 : 1;
                        dq2[(size_t)(((si * n + i) * n + j) * 4 + sj)] =
                            i == j ? pp::DQ_UNSET
                                   : pp::strip_distance(strips.data() + (si * n + i) * padded, strips.data() + ((kind * 4 + sj) * n + j) * padded, padded);
                    }

        std::vector<uint8_t> board((size_t)(rows * P * cols * P * 3));
        for (int64_t Y = 0; Y < rows * P; ++Y)
            for (int64_t X = 0; X < cols * P; ++X)
                for (int c = 0; c < 3; ++c)
                    board[(size_t)((Y * cols * P + X) * 3 + c)] =
                        pp::board_byte_rotated(pieces.data(), n, We, P, cells.data(), rotations.data(), cols, marker, Y, X, c);

        if (!put(out, dq2) || !put(out, board)) return fprintf(stderr, "case %d: write failed\n", q), 2;
    }
    fclose(in);
    if (fclose(out) != 0) return fprintf(stderr, "write failed\n"), 2;
    printf("puzzle_type2_host_check ok: %d cases\n", count);
    return 0;
}
