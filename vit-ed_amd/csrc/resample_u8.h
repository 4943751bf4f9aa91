// Pillow's Image.resize for 8-bit RGB, bilinear, at any scale (antialiased where it shrinks), from the resident image store
// (resample_u8.hip), written so that the device kernel and a host program under the sanitizers
// (tools/resample_host_check.cpp) compile the same text: the sample's geometry, the two passes, the band schedule and its plan.
//
// Per sample a window (top, left, h, w) of image `image[b]` (pixels outside the image are `fill`) is resized to Rh x Rw and the
// S x S crop at (crop_top, crop_left) of that is written as planes [3, S, S].  The taps come from tables computed in fp64 outside
// (ops_resample.resample_taps restates Pillow's precompute_coeffs + normalize_coeffs_8bpc): per axis int32 [classes, R, 2 + ks],
// entry (class, o) = (first tap in window coordinates, tap count, ks 22-bit weights, unused ones 0); a sample names its class per
// axis.  Both passes are  clip8((2^21 + sum_j pixel[first + j] k[j]) >> 22), horizontal first into a uint8 intermediate.
//
// Schedule: one workgroup of RS_THREADS covers one sample and one band of `band_rows` output rows.  Pass 1 resamples the source rows
// the band's vertical taps reach along x into `lds` - planar, [row][channel][Sp] bytes, Sp = S rounded up to 4 - pass 2 (behind a
// barrier) resamples those along y, four x per lane from one LDS dword per tap, and stores four output bytes per channel.
// Everything read from device memory that steers an address (image index, class, first tap, count, window) is clamped or guarded:
// a hostile table gives wrong pixels, never an access outside the store, the tables, the LDS band or the output.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define RS_FN __host__ __device__ __forceinline__
#else
#define RS_FN inline
#endif

#define RS_MAX_OUT 1024         // PUZZLE_MAX_SIZE: the longest output axis
#define RS_MAX_RATIO 8          // in_len / out_len
#define RS_MAX_TAPS 17          // ksize = ceil(max(ratio, 1)) * 2 + 1
#define RS_BITS 22              // Pillow's PRECISION_BITS for 8-bit images
#define RS_THREADS 256
#define RS_LDS_BYTES 65536      // the band's budget: two workgroups on a CU's 160 KiB
#define RS_MAX_BAND 16          // output rows per workgroup at most

struct RsArgs {
    const uint8_t* store;       // HWC images back to back
    const int64_t* img_off;     // [n_images] byte offsets
    const int* img_hw;          // [n_images, 2] (H, W)
    int n_images;
    const int* image;           // [n]
    const int* windows;         // [n, 4] (top, left, h, w) or null: whole images
    int fill;
    const int* xtab;            // [ncx, Rw, 2 + ksx]
    const int* xcls;            // [n]
    int ncx, ksx;
    const int* ytab;            // [ncy, Rh, 2 + ksy]
    const int* ycls;            // [n]
    int ncy, ksy;
    int Rh, Rw, crop_top, crop_left, S;
    uint8_t* out;               // [n] x [3, S, S], sample b at out + b out_bs
    int64_t out_bs;
    int band_rows, lds_rows, Sp, dwords;        // the plan
};

struct RsPlan {
    int band_rows, lds_rows, Sp, bands;
    int64_t lds_bytes;
};

// Source rows a band of `band` output rows can reach: first(y) moves by at most ceil((band - 1) scale) + 1 over the band (a
// truncation at each end), and the last row's taps add at most ks.
RS_FN int rs_band_source_rows(int band, int max_h, int Rh, int ksy) {
    const int64_t reach = ((int64_t)(band - 1) * max_h + Rh - 1) / Rh;      // ceil((band - 1) max_h / Rh)
    return (int)reach + 1 + ksy;
}

// The tallest band (up to RS_MAX_BAND rows) whose intermediate rows fit RS_LDS_BYTES; false if not even one row does.
RS_FN bool rs_make_plan(int max_h, int Rh, int ksy, int S, RsPlan* p) {
    p->Sp = (S + 3) / 4 * 4;
    int band = S < RS_MAX_BAND ? S : RS_MAX_BAND;
    while (band > 1 && (int64_t)rs_band_source_rows(band, max_h, Rh, ksy) * 3 * p->Sp > RS_LDS_BYTES) --band;
    p->band_rows = band;
    p->lds_rows = rs_band_source_rows(band, max_h, Rh, ksy);
    p->lds_bytes = (int64_t)p->lds_rows * 3 * p->Sp;
    p->bands = (S + band - 1) / band;
    return p->lds_bytes <= RS_LDS_BYTES;
}

RS_FN int rs_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// clip8((2^21 + acc) >> 22) of an accumulator that wraps on absurd coefficients instead of overflowing
RS_FN uint32_t rs_round(uint32_t acc) {
    const int v = (int)(acc + (1u << (RS_BITS - 1))) >> RS_BITS;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

struct RsSample {
    const uint8_t* img;         // the sample's image, HWC
    int H, W;
    int64_t top, left;          // of the window, in image coordinates
    int h, w;                   // the window's size
    const int* xt;              // the sample's tables: entry o at xt + o (2 + ksx)
    const int* yt;
};

RS_FN RsSample rs_sample(const RsArgs& a, int64_t b) {
    RsSample s;
    const int idx = rs_clamp(a.image[b], 0, a.n_images - 1);
    s.H = a.img_hw[2 * idx], s.W = a.img_hw[2 * idx + 1];
    s.img = a.store + a.img_off[idx];
    if (a.windows) {
        s.top = a.windows[4 * b], s.left = a.windows[4 * b + 1], s.h = a.windows[4 * b + 2], s.w = a.windows[4 * b + 3];
    } else {
        s.top = 0, s.left = 0, s.h = s.H, s.w = s.W;
    }
    s.xt = a.xtab + (int64_t)rs_clamp(a.xcls[b], 0, a.ncx - 1) * a.Rw * (2 + a.ksx);
    s.yt = a.ytab + (int64_t)rs_clamp(a.ycls[b], 0, a.ncy - 1) * a.Rh * (2 + a.ksy);
    return s;
}

// [r0, r0 + rows) of the window rows that the band of output rows [y0, y1) reads, rows at most lds_rows
RS_FN void rs_band_rows(const RsArgs& a, const RsSample& s, int y0, int y1, int* r0, int* rows) {
    const int* lo = s.yt + (int64_t)(a.crop_top + y0) * (2 + a.ksy);
    const int* hi = s.yt + (int64_t)(a.crop_top + y1 - 1) * (2 + a.ksy);
    *r0 = lo[0];
    const int64_t n = (int64_t)hi[0] + rs_clamp(hi[1], 0, a.ksy) - lo[0];
    *rows = n < 0 ? 0 : (n > a.lds_rows ? a.lds_rows : (int)n);
}

// Pass 1, one lane: item i of rows * Sp is column x = i % Sp of intermediate row i / Sp, all three channels.
RS_FN void rs_hpass_item(const RsArgs& a, const RsSample& s, int r0, int i, uint8_t* lds) {
    const int r = i / a.Sp, x = i - r * a.Sp;
    uint32_t acc[3] = {0u, 0u, 0u};
    if (x < a.S) {
        const int* e = s.xt + (int64_t)(a.crop_left + x) * (2 + a.ksx);
        const int64_t first = e[0];
        const int count = rs_clamp(e[1], 0, a.ksx);
        const int64_t v = (int64_t)r0 + r, Y = v + s.top;
        const bool row_in = v >= 0 && v < s.h && Y >= 0 && Y < s.H;
        const uint8_t* row = s.img + (row_in ? Y : 0) * (int64_t)s.W * 3;
        for (int j = 0; j < count; ++j) {
            const int64_t u = first + j, X = u + s.left;
            const uint32_t k = (uint32_t)e[2 + j];
            if (row_in && u >= 0 && u < s.w && X >= 0 && X < s.W) {
                const uint8_t* q = row + X * 3;
                acc[0] += k * q[0], acc[1] += k * q[1], acc[2] += k * q[2];
            } else {
                acc[0] += k * (uint32_t)a.fill, acc[1] += k * (uint32_t)a.fill, acc[2] += k * (uint32_t)a.fill;
            }
        }
        acc[0] = rs_round(acc[0]), acc[1] = rs_round(acc[1]), acc[2] = rs_round(acc[2]);
    }
    uint8_t* o = lds + (int64_t)r * 3 * a.Sp + x;        // the pad columns S .. Sp - 1 hold zeros: pass 2 reads whole dwords
    o[0] = (uint8_t)acc[0], o[a.Sp] = (uint8_t)acc[1], o[2 * a.Sp] = (uint8_t)acc[2];
}

// Pass 2, one lane: item i of (y1 - y0) * 3 * (Sp / 4) is the four pixels from x = 4 (i % G) of channel (i / G) % 3 of output row
// y0 + i / (3 G), G = Sp / 4.
RS_FN void rs_vpass_item(const RsArgs& a, const RsSample& s, int64_t b, int y0, int r0, int rows, int i, const uint8_t* lds) {
    const int G = a.Sp / 4;
    const int g = i % G, c = (i / G) % 3, y = y0 + i / (3 * G);
    const int* e = s.yt + (int64_t)(a.crop_top + y) * (2 + a.ksy);
    const int64_t first = e[0];
    const int count = rs_clamp(e[1], 0, a.ksy);
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
    for (int j = 0; j < count; ++j) {
        const int64_t r = first + j - r0;
        if (r < 0 || r >= rows) continue;                 // no valid table gets here
        uint32_t px;
        memcpy(&px, __builtin_assume_aligned(lds + (r * 3 + c) * a.Sp + 4 * g, 4), 4);      // one LDS dword
        const uint32_t k = (uint32_t)e[2 + j];
        acc[0] += k * (px & 255u), acc[1] += k * ((px >> 8) & 255u), acc[2] += k * ((px >> 16) & 255u), acc[3] += k * (px >> 24);
    }
    const uint32_t pk = rs_round(acc[0]) | rs_round(acc[1]) << 8 | rs_round(acc[2]) << 16 | rs_round(acc[3]) << 24;
    uint8_t* o = a.out + b * a.out_bs + ((int64_t)c * a.S + y) * a.S + 4 * g;
    if (a.dwords) {
        memcpy(__builtin_assume_aligned(o, 4), &pk, 4);                             // S % 4 == 0 and an aligned destination: every item is whole
    } else {
        for (int q = 0; q < 4 && 4 * g + q < a.S; ++q) o[q] = (uint8_t)(pk >> (8 * q));
    }
}

// What "thread" tid of `threads` does in each pass of (sample b, band): the kernel puts a barrier between the two.
RS_FN void rs_hpass(const RsArgs& a, int64_t b, int band, int tid, int threads, uint8_t* lds) {
    const RsSample s = rs_sample(a, b);
    const int y0 = band * a.band_rows, y1 = y0 + a.band_rows < a.S ? y0 + a.band_rows : a.S;
    int r0, rows;
    rs_band_rows(a, s, y0, y1, &r0, &rows);
    for (int i = tid; i < rows * a.Sp; i += threads) rs_hpass_item(a, s, r0, i, lds);
}

RS_FN void rs_vpass(const RsArgs& a, int64_t b, int band, int tid, int threads, const uint8_t* lds) {
    const RsSample s = rs_sample(a, b);
    const int y0 = band * a.band_rows, y1 = y0 + a.band_rows < a.S ? y0 + a.band_rows : a.S;
    int r0, rows;
    rs_band_rows(a, s, y0, y1, &r0, &rows);
    for (int i = tid; i < (y1 - y0) * 3 * (a.Sp / 4); i += threads) rs_vpass_item(a, s, b, y0, r0, rows, i, lds);
}
