// Config H input pipeline on the device (hisfrag.py:63-81): the decoded fragments stay resident in the uint8 store of div2k_feed.hip
// and every sample's S x S crop is produced here - RandomAffine (Pillow's 16.16 nearest transform), A.ShiftScaleRotate (cv2's
// fixed-point linear warp, constant border), RandomCrop with padding, ColorJitter (Pillow's ImageEnhance and HSV arithmetic) and
// GaussianBlur - so only the window that the crop keeps is ever computed.  The output is what vited_patchify_u8 takes.  DESIGN.md
// section 17 has the per-pixel definition; tests/hisfrag_feed_cases.py restates it in numpy and the kernels equal it bit for bit.
//
// The fixed-point coordinates are sums of separately rounded fp64 terms and the colour arithmetic is Pillow's separate fp32
// multiply and add: nothing in this file may be contracted into an fma (the Makefile builds it with -ffp-contract=off as well).
#pragma STDC FP_CONTRACT OFF
#include "u8_items.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// per-pixel arithmetic
// ---------------------------------------------------------------------------------------------------------------------------
enum : int { HF_AFFINE = 1, HF_WARP = 2, HF_JITTER = 4, HF_BLUR = 8 };

// rint(t * 1024) as an integer, saturated like cv2's saturate_cast<int> (NaN gives INT_MIN)
__device__ __forceinline__ int64_t fixed1024(double t) {
    const double r = rint(t * 1024.0);
    return (int64_t)(int)fmin(fmax(r, -2147483648.0), 2147483647.0);
}

struct WindowSample {
    const uint8_t* img;     // the sample's image, HWC
    int H, W;
    int64_t top, left;      // of the window, in unpadded image coordinates
    bool affine, warp;
    int64_t a[6];           // Pillow's 16.16 coefficients
    double m[6];            // inverse warp map
};

// A(u, v): the image after RandomAffine, 0 outside the image and wherever the 16.16 transform points outside it.  The products
// wrap (unsigned) on absurd coefficients instead of overflowing; the result is bounds-checked either way.
__device__ __forceinline__ void stage_a(const WindowSample& s, int64_t u, int64_t v, int px[3]) {
    px[0] = px[1] = px[2] = 0;
    if (u < 0 || u >= s.W || v < 0 || v >= s.H) return;
    int64_t xi = u, yi = v;
    if (s.affine) {
        xi = (int64_t)((uint64_t)s.a[2] + (uint64_t)u * (uint64_t)s.a[0] + (uint64_t)v * (uint64_t)s.a[1]) >> 16;
        yi = (int64_t)((uint64_t)s.a[5] + (uint64_t)u * (uint64_t)s.a[3] + (uint64_t)v * (uint64_t)s.a[4]) >> 16;
        if (xi < 0 || xi >= s.W || yi < 0 || yi >= s.H) return;
    }
    const uint8_t* q = s.img + (yi * s.W + xi) * 3;
    px[0] = q[0], px[1] = q[1], px[2] = q[2];
}

// T(X, Y): one window pixel, all three channels.  xterm_y / yterm_y are the row's fixed1024(m1 Y + m2) / fixed1024(m4 Y + m5).
__device__ __forceinline__ void window_pixel(const WindowSample& s, int64_t X, int64_t Y, int64_t xterm_y, int64_t yterm_y, int out[3]) {
    if (!s.warp) {
        stage_a(s, X, Y, out);
        return;
    }
    out[0] = out[1] = out[2] = 0;
    if (X < 0 || X >= s.W || Y < 0 || Y >= s.H) return;          // the pad comes after the warp
    const int64_t Xq = (fixed1024(s.m[0] * (double)X) + xterm_y + 16) >> 5;
    const int64_t Yq = (fixed1024(s.m[3] * (double)X) + yterm_y + 16) >> 5;
    const int64_t u0 = Xq >> 5, v0 = Yq >> 5;
    const int a = (int)(Xq & 31), b = (int)(Yq & 31);
    int p00[3], p01[3], p10[3], p11[3];
    stage_a(s, u0, v0, p00);
    stage_a(s, u0 + 1, v0, p01);
    stage_a(s, u0, v0 + 1, p10);
    stage_a(s, u0 + 1, v0 + 1, p11);
    const int w00 = (32 - a) * (32 - b) * 32, w01 = a * (32 - b) * 32, w10 = (32 - a) * b * 32, w11 = a * b * 32;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (w00 * p00[c] + w01 * p01[c] + w10 * p10[c] + w11 * p11[c] + 16384) >> 15;
}

// Image.blend(degenerate, image, f) on one byte: interpolation truncates, extrapolation clips
__device__ __forceinline__ int blend(int d, int p, float f) {
    const float t = (float)d + f * ((float)p - (float)d);
    if (f >= 0.0f && f <= 1.0f) return (int)t;
    return !(t > 0.0f) ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// Pillow's rgb2hsv_row, with its mix of fp32 and fp64 steps
__device__ __forceinline__ void rgb2hsv(int r, int g, int b, int& H, int& S, int& V) {
    const int mx = r > g ? (r > b ? r : b) : (g > b ? g : b), mn = r < g ? (r < b ? r : b) : (g < b ? g : b);
    V = mx;
    if (mx == mn) {
        H = S = 0;
        return;
    }
    const float cr = (float)(mx - mn);
    S = clip8((int)((cr / (float)mx) * 255.0f));
    const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
    float h;
    if (r == mx)
        h = bc - gc;
    else if (g == mx)
        h = (float)((2.0 + (double)rc) - (double)bc);
    else
        h = (float)((4.0 + (double)gc) - (double)rc);
    const double t = (double)h / 6.0 + 1.0;                      // in [5/6, 11/6]: fmod(t, 1) is t - floor(t), exactly
    h = (float)(t - floor(t));
    H = clip8((int)((double)h * 255.0));
}

__device__ __forceinline__ int round8(float x) { return (int)fminf(fmaxf(floorf(x + 0.5f), 0.0f), 255.0f); }

// Pillow's hsv2rgb
__device__ __forceinline__ void hsv2rgb(int H, int S, int V, int& r, int& g, int& b) {
    if (S == 0) {
        r = g = b = V;
        return;
    }
    const float h = (float)H * 6.0f / 255.0f, fs = (float)S / 255.0f;
    const float fi = floorf(h), f = h - fi, v = (float)V;
    const int p = round8(v * (1.0f - fs)), q = round8(v * (1.0f - fs * f)), t = round8(v * (1.0f - fs * (1.0f - f)));
    switch ((int)fi % 6) {
        case 0: r = V, g = t, b = p; break;
        case 1: r = q, g = V, b = p; break;
        case 2: r = p, g = V, b = t; break;
        case 3: r = p, g = q, b = V; break;
        case 4: r = t, g = p, b = V; break;
        default: r = V, g = p, b = q; break;
    }
}

struct JitterSample {
    int order[4];           // 0 brightness, 1 contrast, 2 saturation, 3 hue; anything else does nothing
    float fb, fc, fs;
    int hue;                // added to H, mod 256
};

// The sample's operations in their order on one pixel.  mean < 0: stop in front of the contrast (the pass that sums L for its
// mean) and return true if there is one; otherwise blend towards `mean` there.
__device__ __forceinline__ bool jitter_pixel(const JitterSample& j, int mean, int& r, int& g, int& b) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        switch (j.order[k]) {
            case 0: r = blend(0, r, j.fb), g = blend(0, g, j.fb), b = blend(0, b, j.fb); break;
            case 1:
                if (mean < 0) return true;
                r = blend(mean, r, j.fc), g = blend(mean, g, j.fc), b = blend(mean, b, j.fc);
                break;
            case 2: {
                const int l = luma(r, g, b);
                r = blend(l, r, j.fs), g = blend(l, g, j.fs), b = blend(l, b, j.fs);
                break;
            }
            case 3: {
                int H, S, V;
                rgb2hsv(r, g, b, H, S, V);
                hsv2rgb((H + j.hue) & 255, S, V, r, g, b);
                break;
            }
            default: break;
        }
    }
    return false;
}

// int(mean of L + 0.5), ImageStat's mean being a double division
__device__ __forceinline__ int contrast_mean(int64_t sum, int S) { return (int)floor((double)sum / (double)((int64_t)S * S) + 0.5); }

// One blurred byte: p[i][j] the 3 x 3 neighbourhood (already reflected), k = (k_edge, k_mid, k_edge).  Nine fp32 products with the
// weights k[i] k[j], added in row-major order from 0.
__device__ __forceinline__ int blur_value(const int p[3][3], const float k[3]) {
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc = acc + (k[i] * k[j]) * (float)p[i][j];
    return (int)fminf(fmaxf(rintf(acc), 0.0f), 255.0f);
}

// reflection without repeating the edge, for one step past it (S >= 2)
__device__ __forceinline__ int reflect_one(int i, int S) { return i < 0 ? -i : (i >= S ? 2 * (S - 1) - i : i); }

// ---------------------------------------------------------------------------------------------------------------------------
// kernels: one workgroup per (sample, band of rows); a lane owns four consecutive x of one row for all three channels
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int HF_THREADS = 256;
constexpr int HF_BAND_ROWS = 8;       // S = 512: 64 bands of 1,024 four-pixel items per sample

__global__ void __launch_bounds__(HF_THREADS)
hisfrag_windows_u8_kernel(const uint8_t* __restrict__ store, const int64_t* __restrict__ img_off, const int* __restrict__ img_hw,
                          int n_images, const int* __restrict__ image, const int* __restrict__ flags, const int64_t* __restrict__ afix,
                          const double* __restrict__ minv, const int* __restrict__ origin, uint8_t* __restrict__ out, int S, int dwords) {
    const int64_t b = blockIdx.y;                             // everything about the sample is uniform over the workgroup
    int idx = image[b];
    idx = idx < 0 ? 0 : (idx >= n_images ? n_images - 1 : idx);     // device-side arguments: clamp instead of reading out of bounds
    WindowSample s;
    s.H = img_hw[2 * idx], s.W = img_hw[2 * idx + 1];
    s.img = store + img_off[idx];
    const int f = flags[b];
    s.affine = f & HF_AFFINE, s.warp = f & HF_WARP;
#pragma unroll
    for (int k = 0; k < 6; ++k) s.a[k] = afix[b * 6 + k], s.m[k] = minv[b * 6 + k];
    s.top = origin[2 * b], s.left = origin[2 * b + 1];
    const int y0 = blockIdx.x * HF_BAND_ROWS;
    const int y1 = y0 + HF_BAND_ROWS < S ? y0 + HF_BAND_ROWS : S;
    const int groups = (S + 3) / 4;
    const int64_t plane = (int64_t)S * S;
    uint8_t* o = out + b * 3 * plane;
    for (int i = threadIdx.x; i < (y1 - y0) * groups; i += HF_THREADS) {
        const int y = y0 + i / groups, x0 = (i % groups) * 4;
        const int64_t Y = y + s.top;
        int64_t xterm_y = 0, yterm_y = 0;
        if (s.warp) {
            xterm_y = fixed1024(s.m[1] * (double)Y + s.m[2]);       // two roundings: this file is built without contraction
            yterm_y = fixed1024(s.m[4] * (double)Y + s.m[5]);
        }
        uint32_t pk[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0 + j < S) {
                int px[3];
                window_pixel(s, x0 + j + s.left, Y, xterm_y, yterm_y, px);
#pragma unroll
                for (int c = 0; c < 3; ++c) pk[c] |= (uint32_t)px[c] << (8 * j);
            }
        }
        store_item(o, plane, S, y, x0, pk, dwords != 0);
    }
}

__device__ __forceinline__ JitterSample load_jitter(const int* __restrict__ order, const float* __restrict__ factors,
                                                    const int* __restrict__ hue, int64_t b) {
    JitterSample j;
#pragma unroll
    for (int k = 0; k < 4; ++k) j.order[k] = order[b * 4 + k];
    j.fb = factors[b * 3], j.fc = factors[b * 3 + 1], j.fs = factors[b * 3 + 2];
    j.hue = hue[b] & 255;
    return j;
}

// sums[b] += the L of every pixel of the band as it stands when contrast's turn comes (integer: independent of the launch split)
__global__ void __launch_bounds__(HF_THREADS)
hisfrag_luma_sums_kernel(const uint8_t* __restrict__ in, const int* __restrict__ flags, const int* __restrict__ order,
                         const float* __restrict__ factors, const int* __restrict__ hue, unsigned long long* __restrict__ sums, int S,
                         int dwords) {
    const int64_t b = blockIdx.y;
    if (!(flags[b] & HF_JITTER)) return;
    const JitterSample j = load_jitter(order, factors, hue, b);
    if (j.order[0] != 1 && j.order[1] != 1 && j.order[2] != 1 && j.order[3] != 1) return;
    const int y0 = blockIdx.x * HF_BAND_ROWS;
    const int y1 = y0 + HF_BAND_ROWS < S ? y0 + HF_BAND_ROWS : S;
    const int groups = (S + 3) / 4;
    const int64_t plane = (int64_t)S * S;
    const uint8_t* src = in + b * 3 * plane;
    unsigned long long sum = 0;
    for (int i = threadIdx.x; i < (y1 - y0) * groups; i += HF_THREADS) {
        const int y = y0 + i / groups, x0 = (i % groups) * 4;
        uint32_t pk[3];
        load_item(src, plane, S, y, x0, pk, dwords != 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (x0 + q < S) {
                int r = (pk[0] >> (8 * q)) & 255, g = (pk[1] >> (8 * q)) & 255, bl = (pk[2] >> (8 * q)) & 255;
                jitter_pixel(j, -1, r, g, bl);
                sum += (unsigned long long)luma(r, g, bl);
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if ((threadIdx.x & 63) == 0 && sum != 0) atomicAdd(&sums[b], sum);
}

__global__ void __launch_bounds__(HF_THREADS)
hisfrag_jitter_u8_kernel(const uint8_t* in, const int* __restrict__ flags, const int* __restrict__ order,
                         const float* __restrict__ factors, const int* __restrict__ hue, const unsigned long long* __restrict__ sums,
                         uint8_t* out, int S, int dwords) {            // in may be out: every item is read, then written, by one lane
    const int64_t b = blockIdx.y;
    const bool on = flags[b] & HF_JITTER;
    const JitterSample j = load_jitter(order, factors, hue, b);
    const int mean = clip8(contrast_mean((int64_t)sums[b], S));
    const int y0 = blockIdx.x * HF_BAND_ROWS;
    const int y1 = y0 + HF_BAND_ROWS < S ? y0 + HF_BAND_ROWS : S;
    const int groups = (S + 3) / 4;
    const int64_t plane = (int64_t)S * S;
    for (int i = threadIdx.x; i < (y1 - y0) * groups; i += HF_THREADS) {
        const int y = y0 + i / groups, x0 = (i % groups) * 4;
        uint32_t pk[3];
        load_item(in + b * 3 * plane, plane, S, y, x0, pk, dwords != 0);
        if (on) {
            uint32_t res[3] = {0u, 0u, 0u};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int r = (pk[0] >> (8 * q)) & 255, g = (pk[1] >> (8 * q)) & 255, bl = (pk[2] >> (8 * q)) & 255;
                jitter_pixel(j, mean, r, g, bl);
                res[0] |= (uint32_t)(r & 255) << (8 * q), res[1] |= (uint32_t)(g & 255) << (8 * q), res[2] |= (uint32_t)(bl & 255) << (8 * q);
            }
            pk[0] = res[0], pk[1] = res[1], pk[2] = res[2];
        }
        store_item(out + b * 3 * plane, plane, S, y, x0, pk, dwords != 0);
    }
}

__global__ void __launch_bounds__(HF_THREADS)
hisfrag_blur_u8_kernel(const uint8_t* __restrict__ in, const int* __restrict__ flags, const float* __restrict__ weights,
                       uint8_t* __restrict__ out, int S, int dwords) {
    const int64_t b = blockIdx.y;
    const bool on = flags[b] & HF_BLUR;
    const float k[3] = {weights[2 * b], weights[2 * b + 1], weights[2 * b]};
    const int y0 = blockIdx.x * HF_BAND_ROWS;
    const int y1 = y0 + HF_BAND_ROWS < S ? y0 + HF_BAND_ROWS : S;
    const int groups = (S + 3) / 4;
    const int64_t plane = (int64_t)S * S;
    const uint8_t* src = in + b * 3 * plane;
    for (int i = threadIdx.x; i < (y1 - y0) * groups; i += HF_THREADS) {
        const int y = y0 + i / groups, x0 = (i % groups) * 4;
        uint32_t pk[3];
        if (!on) {
            load_item(src, plane, S, y, x0, pk, dwords != 0);
        } else {
            const int ya[3] = {reflect_one(y - 1, S), y, reflect_one(y + 1, S)};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                int col[3][6];                                   // rows y - 1 .. y + 1, columns x0 - 1 .. x0 + 4
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        const int x = x0 - 1 + q;
                        col[r][q] = x <= S ? src[c * plane + (int64_t)ya[r] * S + reflect_one(x, S)] : 0;      // x = S still reflects inside
                    }
                pk[c] = 0u;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (x0 + q < S) {
                        const int p[3][3] = {{col[0][q], col[0][q + 1], col[0][q + 2]}, {col[1][q], col[1][q + 1], col[1][q + 2]},
                                             {col[2][q], col[2][q + 1], col[2][q + 2]}};
                        pk[c] |= (uint32_t)blur_value(p, k) << (8 * q);
                    }
                }
            }
        }
        store_item(out + b * 3 * plane, plane, S, y, x0, pk, dwords != 0);
    }
}

inline bool bad_batch(int64_t batch, int img_size) { return batch < 1 || batch > 65535 || img_size < 2 || img_size > 4096; }

inline dim3 band_grid(int64_t batch, int S) { return dim3((unsigned)((S + HF_BAND_ROWS - 1) / HF_BAND_ROWS), (unsigned)batch); }

}  // namespace

extern "C" int vited_hisfrag_windows_u8(const uint8_t* store, const int64_t* img_off, const int* img_hw, int n_images, const int* image,
                                        const int* flags, const int64_t* afix, const double* minv, const int* origin, uint8_t* out,
                                        int64_t batch, int img_size, void* stream) {
    if (!store || !img_off || !img_hw || !image || !flags || !afix || !minv || !origin || !out) return VITED_ERR_BAD_ARG;
    if (n_images <= 0 || bad_batch(batch, img_size)) return VITED_ERR_BAD_ARG;
    const int S = img_size;
    const int dwords = S % 4 == 0 && ((uintptr_t)out & 3) == 0;
    hipLaunchKernelGGL(hisfrag_windows_u8_kernel, band_grid(batch, S), dim3(HF_THREADS), 0, (hipStream_t)stream, store, img_off, img_hw,
                       n_images, image, flags, afix, minv, origin, out, S, dwords);
    return vited_check_launch();
}

extern "C" int vited_hisfrag_jitter_u8(const uint8_t* in, const int* flags, const int* order, const float* factors, const int* hue,
                                       int64_t* sums, uint8_t* out, int64_t batch, int img_size, void* stream) {
    if (!in || !flags || !order || !factors || !hue || !sums || !out) return VITED_ERR_BAD_ARG;
    if (bad_batch(batch, img_size) || ((uintptr_t)sums & 7)) return VITED_ERR_BAD_ARG;
    const int S = img_size;
    const int dwords = S % 4 == 0 && (((uintptr_t)in | (uintptr_t)out) & 3) == 0;
    if (hipMemsetAsync(sums, 0, (size_t)batch * sizeof(int64_t), (hipStream_t)stream) != hipSuccess) return VITED_ERR_LAUNCH;
    hipLaunchKernelGGL(hisfrag_luma_sums_kernel, band_grid(batch, S), dim3(HF_THREADS), 0, (hipStream_t)stream, in, flags, order, factors,
                       hue, reinterpret_cast<unsigned long long*>(sums), S, dwords);
    hipLaunchKernelGGL(hisfrag_jitter_u8_kernel, band_grid(batch, S), dim3(HF_THREADS), 0, (hipStream_t)stream, in, flags, order, factors,
                       hue, reinterpret_cast<const unsigned long long*>(sums), out, S, dwords);
    return vited_check_launch();
}

extern "C" int vited_hisfrag_blur_u8(const uint8_t* in, const int* flags, const float* weights, uint8_t* out, int64_t batch, int img_size,
                                     void* stream) {
    if (!in || !flags || !weights || !out || in == out) return VITED_ERR_BAD_ARG;
    if (bad_batch(batch, img_size)) return VITED_ERR_BAD_ARG;
    const int S = img_size;
    const int dwords = S % 4 == 0 && (((uintptr_t)in | (uintptr_t)out) & 3) == 0;
    hipLaunchKernelGGL(hisfrag_blur_u8_kernel, band_grid(batch, S), dim3(HF_THREADS), 0, (hipStream_t)stream, in, flags, weights, out, S,
                       dwords);
    return vited_check_launch();
}
