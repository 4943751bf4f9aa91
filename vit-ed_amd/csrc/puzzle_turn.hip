// Learned type-2 puzzles: the patch extraction of a piece turned by quarter turns.
//   vited_patchify_turned(_u8)   vited_patchify(_u8) of turn_k(image), k per image, gathered from the upright resident image: one
//                                copy of a puzzle's pieces serves all four turns, and no turned image is ever written
// The scatter of a turned pair's four logits into Dq2 (vited_puzzle_distances2_from_logits) sits beside the type-1 scatter in
// puzzle_compat.hip, on the same quantisation.  All index arithmetic is puzzle_turn.h (shared with tools/puzzle_turn_host_check.cpp).
#include "common.h"
#include "puzzle_turn.h"

namespace {

struct TurnNorm { float scale[4], shift[4]; };

// One workgroup per (image, patch row py), walking the strip in the element order of patchify_kernel / patchify_u8_kernel
// (elementwise.hip) with their arithmetic, so a row is bit-equal to the row those kernels write for the physically turned image.  The
// writes run along the patch row as theirs do; under an odd turn the reads walk down a column of the upright image (stride S), p
// neighbouring columns per strip, which the 64-byte lines of a piece a few KiB large serve from cache.
template <typename S, typename D>
__global__ void __launch_bounds__(256)
patchify_turned_kernel(const S* __restrict__ img, int64_t img_bs, const int64_t* __restrict__ bidx, const int* __restrict__ turn, int turn_all,
                       D* __restrict__ out, int chans, int size, int p, TurnNorm nrm) {
    const int G = size / p;
    const int64_t b = blockIdx.x;
    const int py = blockIdx.y;
    const int k = (turn ? turn[b] : turn_all) & 3;          // two bits: whatever the value, the source stays inside the image
    const int64_t src_b = bidx ? bidx[b] : b;
    const S* base = img + src_b * img_bs;
    const int Kp = chans * p * p;
    const int total = chans * p * size;
    D* obase = out + (b * G * G + (int64_t)py * G) * Kp;
    for (int e = threadIdx.x; e < total; e += blockDim.x) {
        const puzzle_turn::StripElement at = puzzle_turn::strip_element(chans, size, p, k, py, e);
        const S raw = base[at.src];
        float v;
        if constexpr (sizeof(S) == 1) v = fmaf((float)raw, nrm.scale[at.c], nrm.shift[at.c]);
        else v = raw;
        obase[at.dst] = from_f32<D>(v);
    }
}

int turned_args(const void* img, const void* out, int turn_all, int64_t batch, int chans, int img_size, int patch) {
    if (!img || !out || batch <= 0 || batch > 0x7fffffff || chans <= 0 || img_size <= 0 || patch <= 0 || img_size % patch)
        return VITED_ERR_BAD_ARG;
    if (turn_all < 0 || turn_all > 3) return VITED_ERR_BAD_ARG;
    if (img_size / patch > 65535 || (int64_t)chans * patch * img_size > 0x7fffffff) return VITED_ERR_UNSUPPORTED;
    return VITED_OK;
}

template <typename S>
int launch_turned(const S* img, int64_t img_bs, const int64_t* batch_index, const int32_t* turn, int turn_all, void* out, int out_dtype,
                  int64_t batch, int chans, int img_size, int patch, const TurnNorm& nrm, void* stream) {
    dim3 grid((unsigned)batch, (unsigned)(img_size / patch));
    hipStream_t s = (hipStream_t)stream;
    if (out_dtype == VITED_BF16)
        hipLaunchKernelGGL((patchify_turned_kernel<S, bf16>), grid, dim3(256), 0, s, img, img_bs, batch_index, turn, turn_all, (bf16*)out, chans,
                           img_size, patch, nrm);
    else if (out_dtype == VITED_F32)
        hipLaunchKernelGGL((patchify_turned_kernel<S, float>), grid, dim3(256), 0, s, img, img_bs, batch_index, turn, turn_all, (float*)out,
                           chans, img_size, patch, nrm);
    else
        return VITED_ERR_UNSUPPORTED;
    return vited_check_launch();
}

}  // namespace

extern "C" int vited_patchify_turned(const float* img, int64_t img_bs, const int64_t* batch_index, const int32_t* turn, int turn_all,
                                     void* out, int out_dtype, int64_t batch, int chans, int img_size, int patch, void* stream) {
    if (int err = turned_args(img, out, turn_all, batch, chans, img_size, patch)) return err;
    if (((uintptr_t)img | (uintptr_t)turn) % 4) return VITED_ERR_BAD_ARG;
    return launch_turned(img, img_bs, batch_index, turn, turn_all, out, out_dtype, batch, chans, img_size, patch, TurnNorm{}, stream);
}

extern "C" int vited_patchify_turned_u8(const uint8_t* img, int64_t img_bs, const int64_t* batch_index, const int32_t* turn, int turn_all,
                                        void* out, int out_dtype, int64_t batch, int chans, int img_size, int patch, const float* mean,
                                        const float* std, void* stream) {
    if (int err = turned_args(img, out, turn_all, batch, chans, img_size, patch)) return err;
    if (!mean || !std || chans > 4 || (uintptr_t)turn % 4) return VITED_ERR_BAD_ARG;
    TurnNorm nrm = {};
    for (int c = 0; c < chans; ++c) {       // the folding of vited_patchify_u8, to the bit
        if (!(std[c] > 0.f)) return VITED_ERR_BAD_ARG;
        nrm.scale[c] = 1.0f / (255.0f * std[c]);
        nrm.shift[c] = -mean[c] / std[c];
    }
    return launch_turned(img, img_bs, batch_index, turn, turn_all, out, out_dtype, batch, chans, img_size, patch, nrm, stream);
}
