// Host build of the Pillow-exact resize (csrc/resample_u8.h) for the address and undefined-behaviour sanitizers: the very text the HIP
// kernel runs - the sample's geometry, both passes, the band plan - driven in the kernel's schedule (per sample and band, RS_THREADS
// "threads" through pass 1, then, where the kernel has its barrier, through pass 2) over exactly-sized heap buffers: the store, the
// tables, the band's intermediate rows (plan.lds_bytes, freshly allocated per band) and an output pre-filled with 0xA5.  The result is
// compared against a second, scalar statement written out below, which shares nothing with the header: its own coefficients
// (Pillow's precompute_coeffs in double), its own window fetch, whole-image passes without bands.
//   windows hanging over all four edges and lying wholly outside, both fills, store offsets of every residue mod 4, ksize 17 (8x), a
//   partial last band, S % 4 != 0 (byte stores), a crop inside the resized image, a batch-strided output whose gaps stay 0xA5, and
//   hostile tables and classes (clamped or skipped, never followed).
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vit-ed_amd/csrc tools/resample_host_check.cpp -o resample_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "resample_u8.h"

static int failures = 0;
static void expect(bool ok, const char* what, long a, long b, long c) {
    if (!ok && ++failures <= 20) fprintf(stderr, "FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {      // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 33);
}

// ---- the rule once more ------------------------------------------------------------------------------------------------------------
struct Coeffs {
    int ksize;
    std::vector<int> first, count;
    std::vector<int> k;      // [out, ksize]
};

static Coeffs coeffs(int in_len, int out_len) {
    Coeffs c;
    const double scale = (double)in_len / (double)out_len;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    c.ksize = (int)ceil(support) * 2 + 1;
    const double ss = 1.0 / fs;
    c.first.resize(out_len), c.count.resize(out_len), c.k.assign((size_t)out_len * c.ksize, 0);
    std::vector<double> w(c.ksize);
    for (int xx = 0; xx < out_len; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_len) xmax = in_len;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            w[x] = a < 1.0 ? 1.0 - a : 0.0;
            ww += w[x];
        }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) w[x] /= ww;
            c.k[(size_t)xx * c.ksize + x] = w[x] < 0 ? (int)(-0.5 + w[x] * (1 << 22)) : (int)(0.5 + w[x] * (1 << 22));
        }
        c.first[xx] = xmin, c.count[xx] = xmax;
    }
    return c;
}

static int clip8(int64_t v) { return v < 0 ? 0 : (v > 255 ? 255 : (int)v); }

// window -> resize to Rh x Rw, whole image at a time: out[(y Rw + x) 3 + c]
static std::vector<uint8_t> resize_scalar(const uint8_t* img, int H, int W, int top, int left, int h, int w, int fill, int Rh, int Rw) {
    std::vector<uint8_t> win((size_t)h * w * 3);
    for (int v = 0; v < h; ++v)
        for (int u = 0; u < w; ++u)
            for (int c = 0; c < 3; ++c) {
                const int64_t Y = (int64_t)v + top, X = (int64_t)u + left;
                win[((size_t)v * w + u) * 3 + c] = (Y >= 0 && Y < H && X >= 0 && X < W) ? img[(Y * W + X) * 3 + c] : (uint8_t)fill;
            }
    const Coeffs cx = coeffs(w, Rw), cy = coeffs(h, Rh);
    std::vector<uint8_t> mid((size_t)h * Rw * 3), out((size_t)Rh * Rw * 3);
    for (int v = 0; v < h; ++v)
        for (int x = 0; x < Rw; ++x)
            for (int c = 0; c < 3; ++c) {
                int64_t acc = 1 << 21;
                for (int j = 0; j < cx.count[x]; ++j) acc += (int64_t)win[((size_t)v * w + cx.first[x] + j) * 3 + c] * cx.k[(size_t)x * cx.ksize + j];
                mid[((size_t)v * Rw + x) * 3 + c] = (uint8_t)clip8(acc >> 22);
            }
    for (int y = 0; y < Rh; ++y)
        for (int x = 0; x < Rw; ++x)
            for (int c = 0; c < 3; ++c) {
                int64_t acc = 1 << 21;
                for (int j = 0; j < cy.count[y]; ++j) acc += (int64_t)mid[((size_t)(cy.first[y] + j) * Rw + x) * 3 + c] * cy.k[(size_t)y * cy.ksize + j];
                out[((size_t)y * Rw + x) * 3 + c] = (uint8_t)clip8(acc >> 22);
            }
    return out;
}

// ---- the kernel's tables and schedule -----------------------------------------------------------------------------------------------
struct Tables {
    std::vector<int> lens;
    int ks = 0, max_len = 0, out_len = 0;
    int* tab = nullptr;      // exactly [classes, out_len, 2 + ks]
    int cls(int len) const {
        for (size_t i = 0; i < lens.size(); ++i)
            if (lens[i] == len) return (int)i;
        return 0;
    }
};

static Tables make_tables(std::vector<int> lens, int out_len) {
    Tables t;
    t.lens = lens, t.out_len = out_len;
    for (int n : lens) {
        const int ks = coeffs(n, out_len).ksize;
        if (ks > t.ks) t.ks = ks;
        if (n > t.max_len) t.max_len = n;
    }
    const int stride = 2 + t.ks;
    t.tab = (int*)calloc(lens.size() * (size_t)out_len * stride, sizeof(int));
    for (size_t c = 0; c < lens.size(); ++c) {
        const Coeffs co = coeffs(lens[c], out_len);
        for (int o = 0; o < out_len; ++o) {
            int* e = t.tab + (c * out_len + o) * stride;
            e[0] = co.first[o], e[1] = co.count[o];
            for (int j = 0; j < co.ksize; ++j) e[2 + j] = co.k[(size_t)o * co.ksize + j];
        }
    }
    return t;
}

struct Image { int H, W; };

// One "launch": n samples of the given images and windows, resized to R x R, cropped to S at (ct, cl), into a batch-strided output.
// hostile: scribble over the copies of the tables and classes the schedule reads (the result is then not compared, only its accesses).
static void check_launch(const char* what, const std::vector<Image>& images, int lead, const std::vector<int>& image, const int* windows,
                         int fill, int R, int ct, int cl, int S, int64_t gap, bool hostile) {
    const int n = (int)image.size();
    // the store: `lead` bytes in front so that the offsets take every residue, exactly sized
    std::vector<int64_t> off(images.size());
    std::vector<int> hw(images.size() * 2);
    int64_t bytes = lead;
    for (size_t i = 0; i < images.size(); ++i) {
        off[i] = bytes, hw[2 * i] = images[i].H, hw[2 * i + 1] = images[i].W;
        bytes += (int64_t)images[i].H * images[i].W * 3;
    }
    uint8_t* store = (uint8_t*)malloc((size_t)bytes);
    for (int64_t i = 0; i < bytes; ++i) store[i] = (uint8_t)rnd();
    int64_t* off_h = (int64_t*)malloc(sizeof(int64_t) * off.size());
    int* hw_h = (int*)malloc(sizeof(int) * hw.size());
    int* image_h = (int*)malloc(sizeof(int) * n);
    memcpy(off_h, off.data(), sizeof(int64_t) * off.size()), memcpy(hw_h, hw.data(), sizeof(int) * hw.size()), memcpy(image_h, image.data(), sizeof(int) * n);
    int* win_h = nullptr;
    if (windows) {
        win_h = (int*)malloc(sizeof(int) * 4 * n);
        memcpy(win_h, windows, sizeof(int) * 4 * n);
    }
    std::vector<int> hs, ws;
    for (int b = 0; b < n; ++b) {
        hs.push_back(windows ? windows[4 * b + 2] : images[image[b]].H);
        ws.push_back(windows ? windows[4 * b + 3] : images[image[b]].W);
    }
    Tables xt = make_tables(ws, R), yt = make_tables(hs, R);
    int* xcls = (int*)malloc(sizeof(int) * n);
    int* ycls = (int*)malloc(sizeof(int) * n);
    for (int b = 0; b < n; ++b) xcls[b] = xt.cls(ws[b]), ycls[b] = yt.cls(hs[b]);
    if (hostile) {
        const size_t nx = xt.lens.size() * (size_t)R * (2 + xt.ks), ny = yt.lens.size() * (size_t)R * (2 + yt.ks);
        for (size_t i = 0; i < nx; i += 3) xt.tab[i] = (int)rnd() - (1 << 30);
        for (size_t i = 0; i < ny; i += 5) yt.tab[i] = (int)rnd() - (1 << 30);
        xt.tab[0] = INT32_MAX, xt.tab[1] = INT32_MAX, yt.tab[0] = INT32_MIN, yt.tab[1] = INT32_MIN;
        xcls[0] = INT32_MAX, ycls[0] = INT32_MIN, image_h[0] = INT32_MAX;
        if (n > 1) image_h[n - 1] = -7;
        if (win_h) win_h[0] = INT32_MIN, win_h[1] = INT32_MAX, win_h[2] = INT32_MAX, win_h[3] = INT32_MAX;
    }
    RsPlan plan;
    const bool fits = rs_make_plan(yt.max_len, R, yt.ks, S, &plan);
    expect(fits && plan.lds_bytes <= RS_LDS_BYTES && plan.band_rows >= 1, "plan", plan.band_rows, plan.lds_rows, (long)plan.lds_bytes);
    const int64_t out_bs = (int64_t)3 * S * S + gap, out_bytes = (n - 1) * out_bs + (int64_t)3 * S * S;
    uint8_t* out = (uint8_t*)malloc((size_t)out_bytes);
    memset(out, 0xA5, (size_t)out_bytes);
    RsArgs a;
    a.store = store, a.img_off = off_h, a.img_hw = hw_h, a.n_images = (int)images.size(), a.image = image_h, a.windows = win_h, a.fill = fill;
    a.xtab = xt.tab, a.xcls = xcls, a.ncx = (int)xt.lens.size(), a.ksx = xt.ks, a.ytab = yt.tab, a.ycls = ycls, a.ncy = (int)yt.lens.size(), a.ksy = yt.ks;
    a.Rh = R, a.Rw = R, a.crop_top = ct, a.crop_left = cl, a.S = S, a.out = out, a.out_bs = out_bs;
    a.band_rows = plan.band_rows, a.lds_rows = plan.lds_rows, a.Sp = plan.Sp;
    a.dwords = S % 4 == 0 && (uintptr_t)out % 4 == 0 && out_bs % 4 == 0;
    int widest = 0;
    for (int b = 0; b < n && fits; ++b)
        for (int band = 0; band < plan.bands; ++band) {       // resample_u8_kernel, workgroup by workgroup
            uint8_t* lds = (uint8_t*)malloc((size_t)plan.lds_bytes);
            memset(lds, 0x5A, (size_t)plan.lds_bytes);
            for (int t = 0; t < RS_THREADS; ++t) rs_hpass(a, b, band, t, RS_THREADS, lds);
            for (int t = 0; t < RS_THREADS; ++t) rs_vpass(a, b, band, t, RS_THREADS, lds);
            free(lds);
            if (!hostile) {                                   // the plan's row bound holds for every band of a real table
                const RsSample s = rs_sample(a, b);
                const int y0 = band * plan.band_rows, y1 = y0 + plan.band_rows < S ? y0 + plan.band_rows : S;
                const int* lo = s.yt + (size_t)(ct + y0) * (2 + a.ksy);
                const int* hi = s.yt + (size_t)(ct + y1 - 1) * (2 + a.ksy);
                const int rows = hi[0] + hi[1] - lo[0];
                expect(rows <= plan.lds_rows, "band rows within the plan", b, band, rows);
                if (rows > widest) widest = rows;
            }
        }
    if (!hostile)
        for (int b = 0; b < n; ++b) {
            const Image& im = images[image[b]];
            const int top = windows ? windows[4 * b] : 0, left = windows ? windows[4 * b + 1] : 0;
            const std::vector<uint8_t> want = resize_scalar(store + off[image[b]], im.H, im.W, top, left, hs[b], ws[b], fill, R, R);
            for (int c = 0; c < 3; ++c)
                for (int y = 0; y < S; ++y)
                    for (int x = 0; x < S; ++x)
                        expect(out[b * out_bs + ((int64_t)c * S + y) * S + x] == want[((size_t)(y + ct) * R + x + cl) * 3 + c], what, b, y, x);
            for (int64_t g = 0; g < gap && b + 1 < n; ++g) expect(out[b * out_bs + (int64_t)3 * S * S + g] == 0xA5, "gap untouched", b, (long)g, 0);
        }
    free(out), free(xcls), free(ycls), free(xt.tab), free(yt.tab), free(win_h), free(image_h), free(hw_h), free(off_h), free(store);
}

int main() {
    int runs = 0;
    const std::vector<Image> images = {{5, 5}, {7, 9}, {16, 16}, {33, 37}, {64, 64}, {100, 100}, {128, 128}, {41, 23}};
    for (int lead = 0; lead < 4; ++lead) {                    // 75 + 189 + ... bytes per image: with the lead every residue mod 4
        // whole square images to 16 (3.2x up, identity, 6.25x, 8x with 17 taps) and to 32, S = R
        check_launch("whole to 16", images, lead, {0, 2, 4, 5, 6}, nullptr, 0, 16, 0, 0, 16, 0, false), ++runs;
        check_launch("whole to 32", images, lead, {6, 5, 0, 2}, nullptr, 255, 32, 0, 0, 32, 5, false), ++runs;
    }
    // a partial last band (S = 21 is no multiple of the band) with byte stores, a crop inside the resized image, non-square images
    check_launch("crop 21 of 37", images, 1, {3, 1, 7}, nullptr, 0, 37, 9, 11, 21, 3, false), ++runs;
    check_launch("crop 20 of 24", images, 2, {1, 3, 7, 5}, nullptr, 0, 24, 4, 0, 20, 0, false), ++runs;
    // windows over all four edges, around the whole image, and wholly outside it; both fills
    const int windows[8][4] = {{-5, -7, 40, 40}, {20, 25, 40, 40}, {-10, 10, 40, 40}, {10, -10, 40, 40}, {-30, -30, 100, 100}, {200, 3, 40, 40},
                               {3, -300, 40, 40}, {0, 0, 33, 37}};
    for (int fill : {0, 255}) {
        check_launch("windows -> 115 crop 100", images, 3, {3, 3, 3, 3, 3, 3, 3, 3}, &windows[0][0], fill, 115, 7, 8, 100, 1, false), ++runs;
        check_launch("windows -> 13", images, 0, {3, 1, 4, 7, 0, 2, 5, 6}, &windows[0][0], fill, 13, 0, 0, 13, 0, false), ++runs;
    }
    // the widest rows: 64 -> 1024 (S = 1024: bands of 16 rows of 3 KB), one sample
    check_launch("64 to 1024", images, 1, {4}, nullptr, 0, 1024, 0, 0, 1024, 0, false), ++runs;
    // hostile tables, classes, indices and windows: only the accesses are checked
    check_launch("hostile", images, 1, {3, 1, 7}, nullptr, 0, 37, 9, 11, 21, 3, true), ++runs;
    check_launch("hostile windows", images, 2, {3, 3, 3, 3, 3, 3, 3, 3}, &windows[0][0], 255, 13, 0, 0, 13, 0, true), ++runs;
    // the plan: 8x down to 1024 columns still fits one row per band; the largest band the budget takes
    RsPlan p;
    expect(rs_make_plan(8192, 1024, 17, 1024, &p) && p.band_rows == 1 && p.lds_bytes == 18 * 3 * 1024, "plan 8192 -> 1024", p.band_rows, p.lds_rows, (long)p.lds_bytes);
    expect(rs_make_plan(2048, 512, 9, 512, &p) && p.band_rows == 9 && p.lds_rows == 42, "plan 2048 -> 512", p.band_rows, p.lds_rows, (long)p.lds_bytes);
    expect(rs_make_plan(512, 588, 3, 512, &p) && p.band_rows == 16 && p.lds_rows == 18, "plan 512 -> 588", p.band_rows, p.lds_rows, (long)p.lds_bytes);
    if (failures) {
        fprintf(stderr, "resample_host_check: %d failures\n", failures);
        return 1;
    }
    printf("resample_host_check ok: %d launches (windows over every edge, offsets of every residue, 17 taps, partial bands, hostile tables), 3 plans\n", runs);
    return 0;
}
