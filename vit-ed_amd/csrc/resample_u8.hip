// Pillow-exact Image.resize on the device:
//   vited_resample_u8   window of a resident image -> resize to Rh x Rw (8-bit, bilinear, antialiased where it shrinks) -> S x S crop
// The geometry, both passes and the band schedule are resample_u8.h (shared with tools/resample_host_check.cpp); the tap tables are
// computed outside in fp64, so this file is integer arithmetic only.  One workgroup per (sample, band of output rows): pass 1 from
// global memory into the band's uint8 intermediate rows in LDS, a barrier, pass 2 from LDS to the planar output.
//
// LDS: dynamic, lds_rows x 3 x Sp bytes, at most RS_LDS_BYTES = 64 KiB, so two workgroups share a CU's 160 KiB at the largest bands
// and eight and more at the sizes the loaders use.  The source is read a byte at a time: a pixel's channels are adjacent, the taps
// of neighbouring lanes overlap, and an image starts at any byte offset of the store, so no wider load is aligned; nothing is read
// that a tap does not name.
#include "common.h"
#include "resample_u8.h"

namespace {

__global__ void __launch_bounds__(RS_THREADS) resample_u8_kernel(const RsArgs a) {
    extern __shared__ __align__(16) uint8_t rs_lds[];
    const int64_t b = blockIdx.y;
    const int band = blockIdx.x;
    rs_hpass(a, b, band, threadIdx.x, RS_THREADS, rs_lds);
    __syncthreads();
    rs_vpass(a, b, band, threadIdx.x, RS_THREADS, rs_lds);
}

// taps per output the tables must hold for windows of up to max_len pixels resized to out_len
inline int taps_needed(int max_len, int out_len) { return ((max_len > out_len ? (max_len + out_len - 1) / out_len : 1)) * 2 + 1; }

}  // namespace

extern "C" int vited_resample_u8(const uint8_t* store, const int64_t* img_off, const int* img_hw, int n_images, const int* image,
                                 const int* windows, int fill, const int* xtab, const int* xcls, int ncx, int ksx, const int* ytab,
                                 const int* ycls, int ncy, int ksy, int max_h, int max_w, int Rh, int Rw, int crop_top, int crop_left,
                                 int img_size, uint8_t* out, int64_t out_bs, int64_t batch, void* stream) {
    if (!store || !img_off || !img_hw || !image || !xtab || !xcls || !ytab || !ycls || !out) return VITED_ERR_BAD_ARG;
    if (((uintptr_t)img_off % 8) || (((uintptr_t)img_hw | (uintptr_t)image | (uintptr_t)windows | (uintptr_t)xtab | (uintptr_t)xcls |
                                      (uintptr_t)ytab | (uintptr_t)ycls) % 4))
        return VITED_ERR_BAD_ARG;
    const int S = img_size;
    if (n_images <= 0 || batch < 1 || batch > 65535 || fill < 0 || fill > 255 || ncx <= 0 || ncy <= 0 || ksx <= 0 || ksy <= 0) return VITED_ERR_BAD_ARG;
    if (S < 1 || Rh < 1 || Rw < 1 || max_h < 1 || max_w < 1) return VITED_ERR_BAD_ARG;
    if (crop_top < 0 || crop_left < 0 || crop_top > Rh - S || crop_left > Rw - S) return VITED_ERR_BAD_ARG;      // the crop lies inside the resized image
    if (batch > 1 && out_bs < (int64_t)3 * S * S) return VITED_ERR_BAD_ARG;                                       // samples would overlap
    if (Rh > RS_MAX_OUT || Rw > RS_MAX_OUT) return VITED_ERR_UNSUPPORTED;
    if (max_h > (int64_t)RS_MAX_RATIO * Rh || max_w > (int64_t)RS_MAX_RATIO * Rw || ksx > RS_MAX_TAPS || ksy > RS_MAX_TAPS) return VITED_ERR_UNSUPPORTED;
    if (ksx < taps_needed(max_w, Rw) || ksy < taps_needed(max_h, Rh)) return VITED_ERR_BAD_ARG;                   // tables too narrow for max_h / max_w
    RsPlan plan;
    if (!rs_make_plan(max_h, Rh, ksy, S, &plan)) return VITED_ERR_UNSUPPORTED;
    RsArgs a;
    a.store = store, a.img_off = img_off, a.img_hw = img_hw, a.n_images = n_images, a.image = image, a.windows = windows, a.fill = fill;
    a.xtab = xtab, a.xcls = xcls, a.ncx = ncx, a.ksx = ksx, a.ytab = ytab, a.ycls = ycls, a.ncy = ncy, a.ksy = ksy;
    a.Rh = Rh, a.Rw = Rw, a.crop_top = crop_top, a.crop_left = crop_left, a.S = S, a.out = out, a.out_bs = out_bs;
    a.band_rows = plan.band_rows, a.lds_rows = plan.lds_rows, a.Sp = plan.Sp;
    a.dwords = S % 4 == 0 && (uintptr_t)out % 4 == 0 && out_bs % 4 == 0;
    hipLaunchKernelGGL(resample_u8_kernel, dim3((unsigned)plan.bands, (unsigned)batch), dim3(RS_THREADS), (size_t)plan.lds_bytes,
                       (hipStream_t)stream, a);
    return vited_check_launch();
}
