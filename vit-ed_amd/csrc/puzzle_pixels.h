// The pixel rules of the classical Paikin-Tal baseline (solver_driver.py): the cut of an image into eroded
// pieces (Puzzle.make_pieces), the prediction-based border distance (PuzzlePiece.calculate_asymmetric_distance), Pillow's 8-bit
// bilinear upscale of a piece (TwoImgSyncEval's Resize) and the reconstructed board (Puzzle.reconstruct_from_pieces), written so that
// the device kernels (puzzle_pixels.hip) and a host program under the sanitizers (tools/puzzle_pixels_host_check.cpp) compile the
// same text.  Everything is 8-bit / integer arithmetic, except the resample coefficients, which are Pillow's fp64 expressions.
// The rules of type-2 puzzles (any side against any side, rotated pieces on the board) follow those of type 1.
//
// Images and pieces are uint8, HWC with 3 channels.  Sides: top 0, right 1, bottom 2, left 3; side s faces side (s + 2) % 4.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PP_FN __host__ __device__ __forceinline__
#else
#define PP_FN inline
#endif

namespace puzzle_pixels {

constexpr int CHANNELS = 3;
constexpr int DQ_UNSET = 2147483647;       // the diagonal of Dq, as vited_puzzle_distances_from_logits' caller fills it
// A strip value lies in [0, 765] and a strip holds 3 We of them: 765 * 3 * We <= 2^31 - 1 holds up to this eroded width.
constexpr int64_t MAX_ERODED = 935722;
constexpr int64_t MAX_PIECES = 46340;      // 4 n^2 int32 indices and the solver's own bound (vited_puzzle_compat_init)

// ---- the cut -----------------------------------------------------------------------------------------------------------------------
// rows = H / P, cols = W / P; the grid is centred: origin ((H - rows P) / 2, (W - cols P) / 2).  Cell (r, c) is the P x P block at
// origin + (r P, c P); a piece is its centre crop of We x We at offset int(round((P - We) / 2.0)), Python's round: half to even.
struct Cut {
    int64_t H, W;
    int P, We;
    int64_t rows, cols, top, left;
    int crop;
};

PP_FN int crop_offset(int P, int We) {
    const int d = P - We, h = d >> 1;
    return (d & 1) ? h + (h & 1) : h;       // d / 2 exactly, or h + 0.5 rounded to the even neighbour
}

PP_FN Cut cut_geometry(int64_t H, int64_t W, int P, int We) {
    Cut g;
    g.H = H, g.W = W, g.P = P, g.We = We;
    g.rows = H / P, g.cols = W / P;
    g.top = (H - g.rows * P) / 2, g.left = (W - g.cols * P) / 2;
    g.crop = crop_offset(P, We);
    return g;
}

// byte offset in the image of pixel (y, x) of the piece cut from cell `cell` (row-major)
PP_FN int64_t cut_source(const Cut& g, int64_t cell, int y, int x) {
    const int64_t r = cell / g.cols, c = cell % g.cols;
    return ((g.top + r * g.P + g.crop + y) * g.W + g.left + c * g.P + g.crop + x) * CHANNELS;
}

// ---- the distance --------------------------------------------------------------------------------------------------------------------
// Line `depth` (0: the border, 1: the line next to it) of side s, position t along it: top / bottom in column order, left / right in
// row order.  Returns the pixel's index y * We + x.
PP_FN int64_t side_pixel(int We, int s, int t, int depth) {
    const int64_t w = We;
    switch (s) {
        case 0: return depth * w + t;
        case 1: return t * w + (We - 1 - depth);
        case 2: return (We - 1 - depth) * w + t;
        default: return t * w + depth;
    }
}

// A strip is the 3 We values of one side of one piece in (position, channel) order, as uint16, zero-padded to strip_padded(We).
// prediction: 2 B - B' + 255 in [0, 765]; facing border: B + 255 in [255, 510].  The shared + 255 cancels in the difference, and the
// equal padding adds |0 - 0|.
PP_FN int strip_padded(int We) { return (CHANNELS * We + 3) & ~3; }

PP_FN uint16_t strip_prediction(const uint8_t* piece, int We, int s, int k) {
    if (k >= CHANNELS * We) return 0;
    const int t = k / CHANNELS, c = k % CHANNELS;
    const int b = piece[side_pixel(We, s, t, 0) * CHANNELS + c], b2 = piece[side_pixel(We, s, t, 1) * CHANNELS + c];
    return (uint16_t)(2 * b - b2 + 255);
}

PP_FN uint16_t strip_border(const uint8_t* piece, int We, int s, int k) {
    if (k >= CHANNELS * We) return 0;
    return (uint16_t)(piece[side_pixel(We, s, k / CHANNELS, 0) * CHANNELS + k % CHANNELS] + 255);
}

// acc + |a.lo - b.lo| + |a.hi - b.hi| over the two uint16 halves of a and b: v_sad_u16 on the device
PP_FN uint32_t sad2(uint32_t a, uint32_t b, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u16(a, b, acc);
#else
    const uint32_t al = a & 0xffffu, bl = b & 0xffffu, ah = a >> 16, bh = b >> 16;
    return acc + (al > bl ? al - bl : bl - al) + (ah > bh ? ah - bh : bh - ah);
#endif
}

// Dq[s, i, j] from the prediction strip of side s of piece i and the border strip of side (s + 2) % 4 of piece j
PP_FN int strip_distance(const uint16_t* prediction, const uint16_t* border, int padded) {
    uint32_t acc = 0;
    for (int k = 0; k < padded; k += 2) {
        uint32_t a, b;
        memcpy(&a, prediction + k, 4);
        memcpy(&b, border + k, 4);
        acc = sad2(a, b, acc);
    }
    return (int)acc;
}

// ---- type 2: any side of piece i against any side of piece j ---------------------------------------------------------------------------
// calculate_asymmetric_distance reads j's border in reversed pixel order (channels keep their order) when the two sides are the same,
// or (si, sj) is (right, top), (top, right), (left, bottom) or (bottom, left); the prediction of i is never reversed.  A pairing
// (s, (s + 2) % 4) is not reversed: it is the type-1 distance.
PP_FN bool pairing_reversed(int si, int sj) { return si == sj || (si ^ sj) == 1; }

// The border strip of side s read from its far end: value k is channel k % 3 of position We - 1 - k / 3, the same zero padding behind.
PP_FN uint16_t strip_border_reversed(const uint8_t* piece, int We, int s, int k) {
    if (k >= CHANNELS * We) return 0;
    return (uint16_t)(piece[side_pixel(We, s, We - 1 - k / CHANNELS, 0) * CHANNELS + k % CHANNELS] + 255);
}

// ---- Pillow's 8-bit bilinear resample, upscaling (libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, the horizontal
// pass into an 8-bit intermediate, then the vertical pass) ------------------------------------------------------------------------------
constexpr int RESAMPLE_TAPS = 3;           // support 1, ksize 3
constexpr int RESAMPLE_BITS = 22;          // PRECISION_BITS = 32 - 8 - 2

struct Taps {
    int first;                             // the first input index
    int k[RESAMPLE_TAPS];                  // fixed-point weights of first, first + 1, first + 2 (0 where the tap is outside)
};

// Taps of output index xx of an axis resampled from `in` to `out` >= in samples.  The weights are 1 - |x| of whole and half distances
// divided by their sum, all in fp64 as Pillow forms them; the products by 2^22 are exact, so the one rounding is the division's.
PP_FN Taps resample_taps(int in, int out, int xx) {
    const double scale = (double)in / (double)out;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - 1.0 + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + 1.0 + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    double w[RESAMPLE_TAPS] = {0.0, 0.0, 0.0}, ww = 0.0;
    for (int x = 0; x < xmax && x < RESAMPLE_TAPS; ++x) {
        double d = (double)(x + xmin) - center + 0.5;
        if (d < 0.0) d = -d;
        w[x] = d < 1.0 ? 1.0 - d : 0.0;
        ww += w[x];
    }
    Taps t;
    t.first = xmin;
    for (int x = 0; x < RESAMPLE_TAPS; ++x) {
        const double v = (x < xmax && ww != 0.0) ? w[x] / ww : w[x];
        t.k[x] = (int)(0.5 + v * (double)(1 << RESAMPLE_BITS));
    }
    return t;
}

PP_FN int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
PP_FN int resample_round(int acc) { return clip8((acc + (1 << (RESAMPLE_BITS - 1))) >> RESAMPLE_BITS); }

// channel c of output pixel of a We x We piece under the column taps tx and the row taps ty
PP_FN uint8_t resample_pixel(const uint8_t* piece, int We, const Taps& ty, const Taps& tx, int c) {
    int acc = 0;
    for (int j = 0; j < RESAMPLE_TAPS; ++j) {
        if (ty.k[j] == 0) continue;                        // a zero weight adds nothing: the row is not fetched (it may lie outside)
        int row = 0;
        for (int i = 0; i < RESAMPLE_TAPS; ++i)
            if (tx.k[i] != 0) row += tx.k[i] * piece[((ty.first + j) * We + tx.first + i) * CHANNELS + c];
        acc += ty.k[j] * resample_round(row);              // the horizontal pass leaves 8 bits
    }
    return (uint8_t)resample_round(acc);
}

// ---- the board -----------------------------------------------------------------------------------------------------------------------
// cells[r * cols + c]: -1 for an empty cell, else 2 * piece + framed.  A piece sits at (r P + pad, c P + pad), pad = (P - We) / 2; a
// framed one (misplaced, and a marker colour given) has a one-pixel ring of the marker around it, which needs pad >= 1; everything
// else is black.  `marker` < 0: no frames; else the colour's bytes, channel c in bits 8 c .. 8 c + 7.
PP_FN uint8_t board_byte(const uint8_t* pieces, int64_t n, int We, int P, const int* cells, int64_t cols, int marker, int64_t Y, int64_t X,
                         int c) {
    const int64_t r = Y / P, col = X / P;
    const int cell = cells[r * cols + col];
    if (cell < 0 || (cell >> 1) >= n) return 0;
    const int pad = (P - We) / 2;
    const int y = (int)(Y - r * P) - pad, x = (int)(X - col * P) - pad;
    if (y >= 0 && y < We && x >= 0 && x < We) return pieces[(((int64_t)(cell >> 1) * We + y) * We + x) * CHANNELS + c];
    if ((cell & 1) && marker >= 0 && y >= -1 && y <= We && x >= -1 && x <= We) return (uint8_t)(marker >> (8 * c));
    return 0;
}

// Pixel (y, x) of numpy.rot90(piece, r) (r quarter turns counter-clockwise) as a pixel index y' * We + x' of the piece itself.
PP_FN int64_t rotated_source(int We, int r, int y, int x) {
    const int64_t w = We;
    switch (r & 3) {
        case 0: return y * w + x;
        case 1: return x * w + (We - 1 - y);
        case 2: return (We - 1 - y) * w + (We - 1 - x);
        default: return (We - 1 - x) * w + y;
    }
}

// board_byte for a type-2 solution: the piece of cell (r, col) enters as numpy.rot90(piece, rotations[r * cols + col]).  The padding
// and the frame are the same on all four sides, so they turn into themselves.
PP_FN uint8_t board_byte_rotated(const uint8_t* pieces, int64_t n, int We, int P, const int* cells, const int* rotations, int64_t cols,
                                 int marker, int64_t Y, int64_t X, int c) {
    const int64_t r = Y / P, col = X / P;
    const int cell = cells[r * cols + col];
    if (cell < 0 || (cell >> 1) >= n) return 0;
    const int pad = (P - We) / 2;
    const int y = (int)(Y - r * P) - pad, x = (int)(X - col * P) - pad;
    if (y >= 0 && y < We && x >= 0 && x < We)
        return pieces[((int64_t)(cell >> 1) * We * We + rotated_source(We, rotations[r * cols + col], y, x)) * CHANNELS + c];
    if ((cell & 1) && marker >= 0 && y >= -1 && y <= We && x >= -1 && x <= We) return (uint8_t)(marker >> (8 * c));
    return 0;
}

}  // namespace puzzle_pixels
