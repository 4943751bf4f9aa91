// Config A input pipeline on the device (data/datasets/div2k_patch.py:84-111): the decoded DIV2K images stay resident in one
// uint8 store and every sample's (2 S) x (3 S) region - flips, ShiftScaleRotate, RGBShift, RandomCrop - is produced here, so only
// the window that the crop keeps is ever warped.  The output is what vited_crop_pairs_u8 (elementwise.hip) takes.  DESIGN.md
// section 16 has the per-pixel definition; tests/div2k_feed_cases.py restates it in numpy and the kernel equals it bit for bit.
//
// The fixed-point coordinates are sums of separately rounded fp64 terms: nothing in this file may be contracted into an fma
// (the Makefile builds it with -ffp-contract=off as well).
#pragma STDC FP_CONTRACT OFF
#include "common.h"

namespace {

constexpr int FEED_THREADS = 256;
constexpr int FEED_BAND_ROWS = 16;    // window rows per workgroup: S = 64 gives 8 bands of 768 four-pixel items

// rint(t * 1024) as an integer, saturated like cv2's saturate_cast<int> (NaN gives INT_MIN)
__device__ __forceinline__ int64_t fixed1024(double t) {
    const double r = rint(t * 1024.0);
    return (int64_t)(int)fmin(fmax(r, -2147483648.0), 2147483647.0);
}

// BORDER_REFLECT_101 (-i below 0, 2 (n - 1) - i at or above n, until in range) in closed form
__device__ __forceinline__ int reflect101(int64_t i, int n) {
    if (n <= 1) return 0;
    const int64_t p = 2 * (int64_t)(n - 1);
    i %= p;
    if (i < 0) i += p;
    return (int)(i < n ? i : p - i);
}

struct FeedSample {
    const uint8_t* img;     // the sample's image, HWC
    int H, W, top, left;
    bool hflip, vflip, warp, colour;
    double m[6];
    float shift[3];
};

__device__ __forceinline__ int colour_lut(int p, float shift) {
    return (int)floorf(fminf(fmaxf((float)p + shift, 0.0f), 255.0f));
}

// One window pixel, all three channels.  INSIDE: every tap of the band lies in the image (no reflection, the two taps of a row
// are 6 contiguous bytes).  With the warp off the pixel is the one tap at (X, Y): the caller passes Y as yterm_y.
template <bool INSIDE>
__device__ __forceinline__ void feed_pixel(const FeedSample& s, int X, int64_t xterm_y, int64_t yterm_y, int out[3]) {
    if (!s.warp) {
        int u = INSIDE ? X : reflect101(X, s.W), v = INSIDE ? (int)yterm_y : reflect101(yterm_y, s.H);
        if (s.hflip) u = s.W - 1 - u;
        if (s.vflip) v = s.H - 1 - v;
        const uint8_t* q = s.img + ((int64_t)v * s.W + u) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = s.colour ? colour_lut(q[c], s.shift[c]) : q[c];
        return;
    }
    const int64_t Xq = (fixed1024(s.m[0] * (double)X) + xterm_y + 16) >> 5;
    const int64_t Yq = (fixed1024(s.m[3] * (double)X) + yterm_y + 16) >> 5;
    const int64_t u0 = Xq >> 5, v0 = Yq >> 5;
    const int a = (int)(Xq & 31), b = (int)(Yq & 31);
    int ua, ub, va, vb;                // columns of the taps u0, u0 + 1 and rows of v0, v0 + 1 in the stored image
    if (INSIDE) {
        ua = (int)u0, ub = ua + 1, va = (int)v0, vb = va + 1;
    } else {
        ua = reflect101(u0, s.W), ub = reflect101(u0 + 1, s.W);
        va = reflect101(v0, s.H), vb = reflect101(v0 + 1, s.H);
    }
    if (s.hflip) ua = s.W - 1 - ua, ub = s.W - 1 - ub;
    if (s.vflip) va = s.H - 1 - va, vb = s.H - 1 - vb;
    const uint8_t* ra = s.img + (int64_t)va * s.W * 3;
    const uint8_t* rb = s.img + (int64_t)vb * s.W * 3;
    const int w00 = (32 - a) * (32 - b) * 32, w01 = a * (32 - b) * 32, w10 = (32 - a) * b * 32, w11 = a * b * 32;
    int p00[3], p01[3], p10[3], p11[3];
    if (INSIDE) {
        const int lo = ua < ub ? ua : ub;                  // ub = ua -+ 1: one 6-byte run per tap row
        const int ia = ua < ub ? 0 : 3, ib = 3 - ia;
        const uint8_t* qa = ra + (int64_t)lo * 3;
        const uint8_t* qb = rb + (int64_t)lo * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) p00[c] = qa[ia + c], p01[c] = qa[ib + c], p10[c] = qb[ia + c], p11[c] = qb[ib + c];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p00[c] = ra[(int64_t)ua * 3 + c], p01[c] = ra[(int64_t)ub * 3 + c];
            p10[c] = rb[(int64_t)ua * 3 + c], p11[c] = rb[(int64_t)ub * 3 + c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int v = (w00 * p00[c] + w01 * p01[c] + w10 * p10[c] + w11 * p11[c] + 16384) >> 15;
        if (s.colour) v = colour_lut(v, s.shift[c]);
        out[c] = v;
    }
}

template <bool INSIDE>
__device__ __forceinline__ void feed_band(const FeedSample& s, uint8_t* __restrict__ o, int S, int y0, int y1, bool dwords) {
    const int W3 = 3 * S, groups = (W3 + 3) / 4;
    const int64_t plane = (int64_t)2 * S * W3;
    for (int i = threadIdx.x; i < (y1 - y0) * groups; i += FEED_THREADS) {
        const int y = y0 + i / groups, x0 = (i % groups) * 4;
        const int Y = y + s.top;
        int64_t xterm_y = 0, yterm_y = Y;
        if (s.warp) {
            xterm_y = fixed1024(s.m[1] * (double)Y + s.m[2]);       // two roundings: this file is built without contraction
            yterm_y = fixed1024(s.m[4] * (double)Y + s.m[5]);
        }
        uint32_t pk[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0 + j < W3) {
                int px[3];
                feed_pixel<INSIDE>(s, x0 + j + s.left, xterm_y, yterm_y, px);
#pragma unroll
                for (int c = 0; c < 3; ++c) pk[c] |= (uint32_t)px[c] << (8 * j);
            }
        }
        uint8_t* row = o + (int64_t)y * W3 + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (dwords) {
                *reinterpret_cast<uint32_t*>(row + c * plane) = pk[c];        // 3 S % 4 == 0: every group is whole and aligned
            } else {
                for (int j = 0; j < 4 && x0 + j < W3; ++j) row[c * plane + j] = (uint8_t)(pk[c] >> (8 * j));
            }
        }
    }
}

__global__ void __launch_bounds__(FEED_THREADS)
div2k_regions_u8_kernel(const uint8_t* __restrict__ store, const int64_t* __restrict__ img_off, const int* __restrict__ img_hw,
                        int n_images, const int* __restrict__ image, const int* __restrict__ flags,
                        const double* __restrict__ minv, const float* __restrict__ rgb, const int* __restrict__ crop,
                        uint8_t* __restrict__ out, int S, int dwords) {
    const int64_t b = blockIdx.y;                             // everything about the sample is uniform over the workgroup
    int idx = image[b];
    idx = idx < 0 ? 0 : (idx >= n_images ? n_images - 1 : idx);     // device-side arguments: clamp instead of reading out of bounds
    FeedSample s;
    s.H = img_hw[2 * idx], s.W = img_hw[2 * idx + 1];
    s.img = store + img_off[idx];
    const int f = flags[b];
    s.hflip = f & 1, s.vflip = f & 2, s.warp = f & 4, s.colour = f & 8;
#pragma unroll
    for (int k = 0; k < 6; ++k) s.m[k] = minv[b * 6 + k];
#pragma unroll
    for (int c = 0; c < 3; ++c) s.shift[c] = rgb[b * 3 + c];
    const int tmax = s.H - 2 * S > 0 ? s.H - 2 * S : 0, lmax = s.W - 3 * S > 0 ? s.W - 3 * S : 0;
    const int top = crop[2 * b], left = crop[2 * b + 1];
    s.top = top < 0 ? 0 : (top > tmax ? tmax : top);
    s.left = left < 0 ? 0 : (left > lmax ? lmax : left);
    const int y0 = blockIdx.x * FEED_BAND_ROWS;
    const int y1 = y0 + FEED_BAND_ROWS < 2 * S ? y0 + FEED_BAND_ROWS : 2 * S;
    uint8_t* o = out + b * (int64_t)18 * S * S;
    if (s.H < 1 || s.W < 1) return;

    // Both fixed-point coordinates are a term monotone in X plus a term monotone in Y, so over the band's rectangle their
    // extremes are at its corners: the band takes the unreflected path when the taps of all four corners are inside the image.
    const int Xa = s.left, Xb = s.left + 3 * S - 1, Ya = s.top + y0, Yb = s.top + y1 - 1;
    int64_t ulo = Xa, uhi = Xb, vlo = Ya, vhi = Yb;
    if (s.warp) {
        const int64_t xa = fixed1024(s.m[0] * (double)Xa), xb = fixed1024(s.m[0] * (double)Xb);
        const int64_t xc = fixed1024(s.m[1] * (double)Ya + s.m[2]), xd = fixed1024(s.m[1] * (double)Yb + s.m[2]);
        const int64_t ya = fixed1024(s.m[3] * (double)Xa), yb = fixed1024(s.m[3] * (double)Xb);
        const int64_t yc = fixed1024(s.m[4] * (double)Ya + s.m[5]), yd = fixed1024(s.m[4] * (double)Yb + s.m[5]);
        ulo = ((xa < xb ? xa : xb) + (xc < xd ? xc : xd) + 16) >> 10;
        uhi = (((xa < xb ? xb : xa) + (xc < xd ? xd : xc) + 16) >> 10) + 1;
        vlo = ((ya < yb ? ya : yb) + (yc < yd ? yc : yd) + 16) >> 10;
        vhi = (((ya < yb ? yb : ya) + (yc < yd ? yd : yc) + 16) >> 10) + 1;
    }
    const bool inside = ulo >= 0 && uhi <= s.W - 1 && vlo >= 0 && vhi <= s.H - 1;
    if (inside)
        feed_band<true>(s, o, S, y0, y1, dwords != 0);
    else
        feed_band<false>(s, o, S, y0, y1, dwords != 0);
}

}  // namespace

extern "C" int vited_div2k_regions_u8(const uint8_t* store, const int64_t* img_off, const int* img_hw, int n_images, const int* image,
                                      const int* flags, const double* minv, const float* rgb, const int* crop, uint8_t* out,
                                      int64_t batch, int img_size, void* stream) {
    if (!store || !img_off || !img_hw || !image || !flags || !minv || !rgb || !crop || !out) return VITED_ERR_BAD_ARG;
    if (n_images <= 0 || batch < 1 || batch > 65535 || img_size <= 0 || img_size > 4096) return VITED_ERR_BAD_ARG;
    const int S = img_size;
    const int dwords = (3 * S) % 4 == 0 && ((uintptr_t)out & 3) == 0;
    dim3 grid((unsigned)((2 * S + FEED_BAND_ROWS - 1) / FEED_BAND_ROWS), (unsigned)batch);
    hipLaunchKernelGGL(div2k_regions_u8_kernel, grid, dim3(FEED_THREADS), 0, (hipStream_t)stream, store, img_off, img_hw, n_images,
                       image, flags, minv, rgb, crop, out, S, dwords);
    return vited_check_launch();
}
