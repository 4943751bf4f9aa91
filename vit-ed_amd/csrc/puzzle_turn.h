// The index rules of the learned type-2 puzzle path: a piece turned by quarter turns under the pair model, and
// where the four logits of one (piece i, turned piece j) forward land in Dq2 [4, n, n, 4].  Written so that the device kernels
// (puzzle_turn.hip, puzzle_compat.hip) and a host program under the sanitizers (tools/puzzle_turn_host_check.cpp) compile the same text.
//
// Sides: top 0, right 1, bottom 2, left 3, clockwise; side s faces side (s + 2) % 4.  A turn k in 0..3 is k CLOCKWISE quarter turns:
// turn_k(x) = numpy.rot90(x, -k) over the two pixel axes, and the border that was side s becomes side (s + k) % 4.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PT_FN __host__ __device__ __forceinline__
#else
#define PT_FN inline
#endif

namespace puzzle_turn {

// ---- pixels ------------------------------------------------------------------------------------------------------------------------
// Pixel (y, x) of turn_k(image) as the pixel index y' * S + x' of the upright S x S image.
PT_FN int64_t turned_source(int S, int k, int y, int x) {
    const int64_t w = S;
    switch (k & 3) {
        case 0: return y * w + x;
        case 1: return (S - 1 - x) * w + y;
        case 2: return (S - 1 - y) * w + (S - 1 - x);
        default: return x * w + (S - 1 - y);
    }
}

PT_FN int moved_side(int s, int k) { return (s + k) & 3; }

// Element e of the strip of patch row py - (channel c, row i of the patch row, column x of the image), x fastest, as patchify_kernel
// (elementwise.hip) walks it.  `src` is the element's offset in the upright [C, S, S] image turned by k, `dst` its offset in the G patch
// rows [G, C p p] that the strip fills, 0 <= e < C p S.
struct StripElement {
    int64_t src, dst;
    int c;
};

PT_FN StripElement strip_element(int chans, int S, int p, int k, int py, int e) {
    const int x = e % S, ci = e / S;            // ci = c * p + i
    const int i = ci % p, c = ci / p;
    const int px = x / p, j = x - px * p;
    StripElement r;
    r.c = c;
    r.src = (int64_t)c * S * S + turned_source(S, k, py * p + i, x);
    r.dst = (int64_t)px * chans * p * p + (int64_t)ci * p + j;
    return r;
}

// ---- pairings ----------------------------------------------------------------------------------------------------------------------
// Side sj of piece j faces side si of piece i once j is turned by pair_turn(si, sj).
PT_FN int pair_turn(int si, int sj) { return (si + 2 - sj) & 3; }

// The model's bin b of the pair (i, turn_k(j)) speaks of side bin_side_i(b) of piece i (the type-1 rule: side s reads bin (s + 3) % 4)
// and of side bin_side_j(b, k) of the upright piece j.
PT_FN int bin_side_i(int b) { return (b + 1) & 3; }
PT_FN int bin_side_j(int b, int k) { return (bin_side_i(b) + 2 - k) & 3; }

// jt = k * n + j in [0, 4 n): the row of turn_k(piece j) in the image-2 token cache of the 4 n turned pieces.
PT_FN bool pair_in_range(int64_t i, int64_t jt, int64_t n) { return i >= 0 && i < n && jt >= 0 && jt < 4 * n && jt % n != i; }

PT_FN int64_t dq2_index(int64_t n, int si, int64_t i, int64_t j, int sj) { return (((int64_t)si * n + i) * n + j) * 4 + sj; }

// Where bin b of the pair (i, jt) goes in Dq2 [4, n, n, 4]; the pair must be pair_in_range.
PT_FN int64_t dq2_slot(int64_t n, int64_t i, int64_t jt, int b) {
    const int k = (int)(jt / n);
    return dq2_index(n, bin_side_i(b), i, jt % n, bin_side_j(b, k));
}

}  // namespace puzzle_turn
