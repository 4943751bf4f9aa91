// Stand-alone host program: csrc/puzzle_pixels.h - the text the kernels of csrc/puzzle_pixels.hip run - over the cases of a binary case
// file, for a build under the sanitizers (tests/test_puzzle_pixels.py compiles it with -fsanitize=address,undefined).
//
//   puzzle_pixels_host_check cases.bin out.bin
//
// cases.bin (little endian): int32 count, then per case 10 int32 (H, W, P, We, n, rows, cols, S, marker, has_order), the image uint8
// [H, W, 3], order int32 [n] (when has_order), cells int32 [rows * cols].  Per case out.bin receives pieces uint8 [n, We, We, 3], Dq
// int32 [4, n, n], the resized pieces uint8 [n, 3, S, S] and the board uint8 [rows P, cols P, 3], and stdout one line with the 64-bit
// FNV-1a hash of each.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "puzzle_pixels.h"

namespace pp = puzzle_pixels;

static uint64_t fnv(const void* data, size_t bytes) {
    uint64_t h = 1469598103934665603ull;
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

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
        if (!get(in, head, 10)) return fprintf(stderr, "case %d: short header\n", q), 2;
        const int64_t H = head[0], W = head[1];
        const int P = head[2], We = head[3], S = head[7], marker = head[8];
        const int64_t n = head[4], rows = head[5], cols = head[6];
        std::vector<uint8_t> image;
        std::vector<int32_t> order, cells;
        if (!get(in, image, (size_t)(H * W * 3)) || !get(in, order, head[9] ? (size_t)n : 0) || !get(in, cells, (size_t)(rows * cols)))
            return fprintf(stderr, "case %d: short data\n", q), 2;
        const pp::Cut g = pp::cut_geometry(H, W, P, We);
        if (We < 2 || P < We || g.rows * g.cols != n || rows * cols != n || S < We) return fprintf(stderr, "case %d: bad sizes\n", q), 2;

        std::vector<uint8_t> pieces((size_t)(n * We * We * 3));
        for (int64_t k = 0; k < n; ++k)
            for (int y = 0; y < We; ++y)
                for (int x = 0; x < We; ++x) {
                    const uint8_t* src = image.data() + pp::cut_source(g, head[9] ? order[(size_t)k] : k, y, x);
                    uint8_t* dst = pieces.data() + ((k * We + y) * We + x) * 3;
                    dst[0] = src[0], dst[1] = src[1], dst[2] = src[2];
                }

        const int padded = pp::strip_padded(We);
        std::vector<uint16_t> strips((size_t)(2 * 4 * n * padded));
        for (int kind = 0; kind < 2; ++kind)
            for (int s = 0; s < 4; ++s)
                for (int64_t i = 0; i < n; ++i)
                    for (int k = 0; k < padded; ++k) {
                        const uint8_t* piece = pieces.data() + i * We * We * 3;
                        strips[(size_t)(((kind * 4 + s) * n + i) * padded + k)] =
                            kind ? pp::strip_border(piece, We, s, k) : pp::strip_prediction(piece, We, s, k);
                    }
        std::vector<int32_t> dq((size_t)(4 * n * n));
        for (int s = 0; s < 4; ++s)
            for (int64_t i = 0; i < n; ++i)
                for (int64_t j = 0; j < n; ++j)
                    dq[(size_t)((s * n + i) * n + j)] =
                        i == j ? pp::DQ_UNSET
                               : pp::strip_distance(strips.data() + (s * n + i) * padded, strips.data() + ((4 + (s + 2) % 4) * n + j) * padded, padded);

        std::vector<pp::Taps> taps((size_t)S);
        for (int x = 0; x < S; ++x) taps[(size_t)x] = pp::resample_taps(We, S, x);
        std::vector<uint8_t> resized((size_t)(n * 3 * S * S));
        for (int64_t k = 0; k < n; ++k)
            for (int c = 0; c < 3; ++c)
                for (int y = 0; y < S; ++y)
                    for (int x = 0; x < S; ++x)
                        resized[(size_t)(((k * 3 + c) * S + y) * S + x)] =
                            pp::resample_pixel(pieces.data() + k * We * We * 3, We, taps[(size_t)y], taps[(size_t)x], c);

        std::vector<uint8_t> board((size_t)(rows * P * cols * P * 3));
        for (int64_t Y = 0; Y < rows * P; ++Y)
            for (int64_t X = 0; X < cols * P; ++X)
                for (int c = 0; c < 3; ++c)
                    board[(size_t)((Y * cols * P + X) * 3 + c)] = pp::board_byte(pieces.data(), n, We, P, cells.data(), cols, marker, Y, X, c);

        if (!put(out, pieces) || !put(out, dq) || !put(out, resized) || !put(out, board)) return fprintf(stderr, "case %d: write failed\n", q), 2;
        printf("%d pieces %016llx dq %016llx resized %016llx board %016llx\n", q, (unsigned long long)fnv(pieces.data(), pieces.size()),
               (unsigned long long)fnv(dq.data(), dq.size() * 4), (unsigned long long)fnv(resized.data(), resized.size()),
               (unsigned long long)fnv(board.data(), board.size()));
    }
    fclose(in);
    if (fclose(out) != 0) return fprintf(stderr, "write failed\n"), 2;
    printf("puzzle_pixels_host_check ok: %d cases\n", count);
    return 0;
}
