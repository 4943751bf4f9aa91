// michigan.py's input pipeline on the device (michigan.py:68-101): the decoded fragments stay resident in the uint8 store of
// div2k_feed.hip and every sample's S x S crop is produced here - RandomCrop with a white pad, RandomResizedCrop (Pillow's two-pass
// 8-bit bilinear resample from per-sample tap tables), CoarseDropout, both flips - then, behind vited_hisfrag_jitter_u8, Pillow's
// GaussianBlur (three box-blur passes per axis) and RandomGrayscale.  The output is what vited_patchify_u8 takes.  DESIGN.md section
// 18 has the per-pixel definition; tests/michigan_feed_cases.py restates it in numpy and the kernels equal it bit for bit.
//
// Everything in this file is integer arithmetic: the plan (engine.michigan_augment_plan) computes every coefficient.
#include "u8_items.h"

namespace {

enum : int { MF_DROPOUT = 1, MF_HFLIP = 2, MF_BLUR = 8, MF_VFLIP = 16, MF_GRAY = 32 };      // bit 2 is the jitter's (hisfrag_feed.hip)

constexpr int MF_THREADS = 256;
constexpr int MF_BAND_ROWS = 8;       // S = 512: 64 bands of 1,024 four-pixel items per sample
constexpr int MF_MAX_HOLES = 16;
constexpr int MF_TAPS = 3;            // upscaling only: Pillow's bilinear support is 1, ksize 3
constexpr int MF_BITS = 22;           // Pillow's PRECISION_BITS for 8-bit images

// ---------------------------------------------------------------------------------------------------------------------------
// geometry
// ---------------------------------------------------------------------------------------------------------------------------
struct WindowSample {
    const uint8_t* img;     // the sample's image, HWC
    int H, W, S;
    int64_t top, left;      // of the window, in unpadded image coordinates
};

// Wd(u, v): the padded RandomCrop window; 255 outside the image and, for tap indices no plan produces, outside the window itself
__device__ __forceinline__ void window_pixel(const WindowSample& s, int64_t u, int64_t v, int px[3]) {
    px[0] = px[1] = px[2] = 255;
    if (u < 0 || u >= s.S || v < 0 || v >= s.S) return;
    const int64_t X = u + s.left, Y = v + s.top;
    if (X < 0 || X >= s.W || Y < 0 || Y >= s.H) return;
    const uint8_t* q = s.img + (Y * s.W + X) * 3;
    px[0] = q[0], px[1] = q[1], px[2] = q[2];
}

// clip8((2^21 + acc) >> 22) of an accumulator that wraps on absurd coefficients instead of overflowing
__device__ __forceinline__ int resample_round(uint32_t acc) { return clip8((int)(acc + (1u << (MF_BITS - 1))) >> MF_BITS); }

// One workgroup per (sample, band of output rows); a lane owns four consecutive x of one row for all three channels.  The taps of
// neighbouring outputs overlap almost entirely and a pixel's three channels are adjacent bytes, so the source rows are left to
// the cache: an LDS stage would need the band's whole tap span (up to S x 10 pixels, 120 KB at S = 4096) for reads that the
// vector cache already serves from one or two lines per wave instruction.
__global__ void __launch_bounds__(MF_THREADS)
michigan_windows_u8_kernel(const uint8_t* __restrict__ store, const int64_t* __restrict__ img_off, const int* __restrict__ img_hw,
                           int n_images, const int* __restrict__ image, const int* __restrict__ flags, const int* __restrict__ origin,
                           const int* __restrict__ x0, const int* __restrict__ kx, const int* __restrict__ y0,
                           const int* __restrict__ ky, const int* __restrict__ holes, const int* __restrict__ n_holes,
                           uint8_t* __restrict__ out, int S, int dwords) {
    const int64_t b = blockIdx.y;                             // everything about the sample is uniform over the workgroup
    int idx = image[b];
    idx = idx < 0 ? 0 : (idx >= n_images ? n_images - 1 : idx);     // device-side arguments: clamp instead of reading out of bounds
    WindowSample s;
    s.H = img_hw[2 * idx], s.W = img_hw[2 * idx + 1], s.S = S;
    s.img = store + img_off[idx];
    s.top = origin[2 * b], s.left = origin[2 * b + 1];
    const int f = flags[b];
    const bool fx = f & MF_HFLIP, fy = f & MF_VFLIP;
    int nh = (f & MF_DROPOUT) ? n_holes[b] : 0;
    nh = nh < 0 ? 0 : (nh > MF_MAX_HOLES ? MF_MAX_HOLES : nh);
    const int* hole = holes + b * MF_MAX_HOLES * 4;
    const int* x0b = x0 + b * S;
    const int* y0b = y0 + b * S;
    const int* kxb = kx + b * S * MF_TAPS;
    const int* kyb = ky + b * S * MF_TAPS;
    const int band0 = blockIdx.x * MF_BAND_ROWS;
    const int band1 = band0 + MF_BAND_ROWS < S ? band0 + MF_BAND_ROWS : S;
    const int groups = (S + 3) / 4;
    const int64_t plane = (int64_t)S * S;
    uint8_t* o = out + b * 3 * plane;
    for (int i = threadIdx.x; i < (band1 - band0) * groups; i += MF_THREADS) {
        const int y = band0 + i / groups, xg = (i % groups) * 4;
        const int ry = fy ? S - 1 - y : y;                    // the flips act on the fetch: holes and tables are in pre-flip coordinates
        const int64_t v0 = y0b[ry];
        const int kyv[MF_TAPS] = {kyb[ry * MF_TAPS], kyb[ry * MF_TAPS + 1], kyb[ry * MF_TAPS + 2]};
        uint32_t pk[3] = {0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int x = xg + q;
            if (x >= S) break;
            const int rx = fx ? S - 1 - x : x;
            bool holed = false;
            for (int h = 0; h < nh; ++h)
                holed |= rx >= hole[4 * h] && ry >= hole[4 * h + 1] && rx < hole[4 * h + 2] && ry < hole[4 * h + 3];
            int px[3] = {255, 255, 255};
            if (!holed) {
                const int64_t u0 = x0b[rx];
                const int kxv[MF_TAPS] = {kxb[rx * MF_TAPS], kxb[rx * MF_TAPS + 1], kxb[rx * MF_TAPS + 2]};
                uint32_t acc[3] = {0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < MF_TAPS; ++j) {
                    if (kyv[j] == 0) continue;                // a zero weight adds nothing: the row is not fetched
                    uint32_t row[3] = {0u, 0u, 0u};
#pragma unroll
                    for (int t = 0; t < MF_TAPS; ++t) {
                        if (kxv[t] == 0) continue;
                        int p[3];
                        window_pixel(s, u0 + t, v0 + j, p);
#pragma unroll
                        for (int c = 0; c < 3; ++c) row[c] += (uint32_t)kxv[t] * (uint32_t)p[c];
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] += (uint32_t)kyv[j] * (uint32_t)resample_round(row[c]);      // 8-bit intermediate
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) px[c] = resample_round(acc[c]);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) pk[c] |= (uint32_t)px[c] << (8 * q);
        }
        store_item(o, plane, S, y, xg, pk, dwords != 0);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// ImageFilter.GaussianBlur(radius <= 1) and RandomGrayscale
// ---------------------------------------------------------------------------------------------------------------------------
// A workgroup owns a tile of MB_TH x MB_TW pixels, all three channels, and runs the six passes (three along x, then three along y,
// an 8-bit intermediate after each) between two uint8 buffers in LDS.  The tile carries a halo of three pixels on every side; what a
// pass writes there is right one pixel less far out than what it read, so after six passes the tile itself is right.  At the
// crop's border every pass clamps its reads to the crop (Pillow replicates the edge of each pass's own input).  A row of a buffer is
// MB_STRIDE bytes, tile column 0 at byte 4: a lane works on one aligned dword of four pixels, consecutive lanes on consecutive
// dwords (no bank conflicts).
constexpr int MB_TH = 16, MB_TW = 128, MB_HALO = 3;
constexpr int MB_ROWS = MB_TH + 2 * MB_HALO;                  // 22
constexpr int MB_STRIDE = MB_TW + 8;                          // 136 bytes: columns x0 - 4 .. x0 + 131
constexpr int MB_GROUPS = MB_STRIDE / 4;                      // 34 dwords
constexpr int MB_PLANE = MB_ROWS * MB_GROUPS;                 // dwords per channel
constexpr int MB_ITEMS = 3 * MB_PLANE;                        // 2,244 dwords per buffer, 17,952 bytes for the pair

__device__ __forceinline__ uint32_t box3(uint32_t c, uint32_t l, uint32_t r, uint32_t ww, uint32_t fw) {
    return (c * ww + (l + r) * fw + (1u << 23)) >> 24;        // unsigned: at most 255 * 2^24 for the plan's weights, 8 bits for any
}

// one pass along x: lo / hi are the byte columns of the crop's first and last pixel that the buffer holds
__device__ __forceinline__ void blur_pass_x(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int lo, int hi, uint32_t ww,
                                            uint32_t fw) {
    const uint8_t* src8 = reinterpret_cast<const uint8_t*>(src);
    for (int i = threadIdx.x; i < MB_ITEMS; i += MF_THREADS) {
        const int g = i % MB_GROUPS, li = 4 * g;
        const uint8_t* row8 = src8 + (i - g) * 4;
        const uint32_t cur = src[i];
        const int il = li - 1 > lo ? li - 1 : lo, ir = li + 4 < hi ? li + 4 : hi;          // both inside 0 .. MB_STRIDE - 1
        const uint32_t left = row8[il], right = row8[ir];
        int last = hi - li;                                   // the byte of this dword that holds the crop's last column, if any
        last = last < 0 ? 0 : last;
        uint32_t res = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t c = (cur >> (8 * j)) & 255u;
            const uint32_t l = j > 0 ? (cur >> (8 * (j - 1))) & 255u : left;
            const int rs = j + 1 < last ? j + 1 : last;
            const uint32_t r = rs >= 4 ? right : (cur >> (8 * rs)) & 255u;
            res |= box3(c, l, r, ww, fw) << (8 * j);
        }
        dst[i] = res;
    }
}

// one pass along y: lo / hi are the buffer rows of the crop's first and last row that the buffer holds
__device__ __forceinline__ void blur_pass_y(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int lo, int hi, uint32_t ww,
                                            uint32_t fw) {
    for (int i = threadIdx.x; i < MB_ITEMS; i += MF_THREADS) {
        const int c = i / MB_PLANE, r = (i % MB_PLANE) / MB_GROUPS, g = i % MB_GROUPS;
        const int ru = r - 1 > lo ? r - 1 : lo, rd = r + 1 < hi ? r + 1 : hi;              // both inside 0 .. MB_ROWS - 1
        const uint32_t cur = src[i], up = src[c * MB_PLANE + ru * MB_GROUPS + g], down = src[c * MB_PLANE + rd * MB_GROUPS + g];
        uint32_t res = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            res |= box3((cur >> (8 * j)) & 255u, (up >> (8 * j)) & 255u, (down >> (8 * j)) & 255u, ww, fw) << (8 * j);
        dst[i] = res;
    }
}

__device__ __forceinline__ void gray_item(uint32_t pk[3]) {
    uint32_t res = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        res |= (uint32_t)luma((pk[0] >> (8 * j)) & 255, (pk[1] >> (8 * j)) & 255, (pk[2] >> (8 * j)) & 255) << (8 * j);
    pk[0] = pk[1] = pk[2] = res;
}

__global__ void __launch_bounds__(MF_THREADS)
michigan_blur_gray_u8_kernel(const uint8_t* __restrict__ in, const int* __restrict__ flags, const int* __restrict__ weights,
                             uint8_t* __restrict__ out, int S, int tiles_x, int dwords) {
    __shared__ uint32_t buf[2][MB_ITEMS];
    const int64_t b = blockIdx.y;                             // the flags are uniform over the workgroup: so is every branch on them
    const int f = flags[b];
    const bool blur = f & MF_BLUR, gray = f & MF_GRAY;
    const uint32_t ww = (uint32_t)weights[2 * b], fw = (uint32_t)weights[2 * b + 1];
    const int ty0 = (int)(blockIdx.x / tiles_x) * MB_TH, tx0 = (int)(blockIdx.x % tiles_x) * MB_TW;
    const int64_t plane = (int64_t)S * S;
    const uint8_t* src = in + b * 3 * plane;
    uint8_t* dst = out + b * 3 * plane;
    if (blur) {
        // the tile with its halo, zeros outside the crop (never read by a clamped tap)
        for (int i = threadIdx.x; i < MB_ITEMS; i += MF_THREADS) {
            const int c = i / MB_PLANE, r = (i % MB_PLANE) / MB_GROUPS, g = i % MB_GROUPS;
            const int y = ty0 - MB_HALO + r, x = tx0 - 4 + 4 * g;
            uint32_t v = 0u;
            if (y >= 0 && y < S) {
                const uint8_t* row = src + c * plane + (int64_t)y * S;
                if (dwords && x >= 0 && x + 3 < S) {
                    v = *reinterpret_cast<const uint32_t*>(row + x);
                } else {
                    for (int j = 0; j < 4; ++j)
                        if (x + j >= 0 && x + j < S) v |= (uint32_t)row[x + j] << (8 * j);
                }
            }
            buf[0][i] = v;
        }
        const int xlo = tx0 == 0 ? 4 : 0, xhi = S - 1 - tx0 + 4 < MB_STRIDE - 1 ? S - 1 - tx0 + 4 : MB_STRIDE - 1;
        const int ylo = ty0 < MB_HALO ? MB_HALO - ty0 : 0, yhi = S - 1 - ty0 + MB_HALO < MB_ROWS - 1 ? S - 1 - ty0 + MB_HALO : MB_ROWS - 1;
        __syncthreads();
        blur_pass_x(buf[0], buf[1], xlo, xhi, ww, fw);
        __syncthreads();
        blur_pass_x(buf[1], buf[0], xlo, xhi, ww, fw);
        __syncthreads();
        blur_pass_x(buf[0], buf[1], xlo, xhi, ww, fw);
        __syncthreads();
        blur_pass_y(buf[1], buf[0], ylo, yhi, ww, fw);
        __syncthreads();
        blur_pass_y(buf[0], buf[1], ylo, yhi, ww, fw);
        __syncthreads();
        blur_pass_y(buf[1], buf[0], ylo, yhi, ww, fw);
        __syncthreads();
    }
    for (int i = threadIdx.x; i < MB_TH * (MB_TW / 4); i += MF_THREADS) {
        const int r = i / (MB_TW / 4), g = i % (MB_TW / 4);
        const int y = ty0 + r, x = tx0 + 4 * g;
        if (y >= S || x >= S) continue;
        uint32_t pk[3];
        if (blur) {
#pragma unroll
            for (int c = 0; c < 3; ++c) pk[c] = buf[0][c * MB_PLANE + (r + MB_HALO) * MB_GROUPS + g + 1];
        } else {
            load_item(src, plane, S, y, x, pk, dwords != 0);
        }
        if (gray) gray_item(pk);
        store_item(dst, plane, S, y, x, pk, dwords != 0);
    }
}

inline bool bad_batch(int64_t batch, int img_size) { return batch < 1 || batch > 65535 || img_size < 2 || img_size > 4096; }

}  // namespace

extern "C" int vited_michigan_windows_u8(const uint8_t* store, const int64_t* img_off, const int* img_hw, int n_images, const int* image,
                                         const int* flags, const int* origin, const int* x0, const int* kx, const int* y0, const int* ky,
                                         const int* holes, const int* n_holes, uint8_t* out, int64_t batch, int img_size, void* stream) {
    if (!store || !img_off || !img_hw || !image || !flags || !origin || !x0 || !kx || !y0 || !ky || !holes || !n_holes || !out)
        return VITED_ERR_BAD_ARG;
    if (n_images <= 0 || bad_batch(batch, img_size)) return VITED_ERR_BAD_ARG;
    const int S = img_size;
    const int dwords = S % 4 == 0 && ((uintptr_t)out & 3) == 0;
    const dim3 grid((unsigned)((S + MF_BAND_ROWS - 1) / MF_BAND_ROWS), (unsigned)batch);
    hipLaunchKernelGGL(michigan_windows_u8_kernel, grid, dim3(MF_THREADS), 0, (hipStream_t)stream, store, img_off, img_hw, n_images, image,
                       flags, origin, x0, kx, y0, ky, holes, n_holes, out, S, dwords);
    return vited_check_launch();
}

extern "C" int vited_michigan_blur_gray_u8(const uint8_t* in, const int* flags, const int* weights, uint8_t* out, int64_t batch,
                                           int img_size, void* stream) {
    if (!in || !flags || !weights || !out || in == out) return VITED_ERR_BAD_ARG;
    if (bad_batch(batch, img_size)) return VITED_ERR_BAD_ARG;
    const int S = img_size;
    const int dwords = S % 4 == 0 && (((uintptr_t)in | (uintptr_t)out) & 3) == 0;
    const int tiles_x = (S + MB_TW - 1) / MB_TW, tiles_y = (S + MB_TH - 1) / MB_TH;
    hipLaunchKernelGGL(michigan_blur_gray_u8_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)batch), dim3(MF_THREADS), 0,
                       (hipStream_t)stream, in, flags, weights, out, S, tiles_x, dwords);
    return vited_check_launch();
}
