// Elementwise token dropout (timm's pos_drop = nn.Dropout(pos_drop_rate) at the end of _pos_embed):
//   vited_token_dropout   out = keep(e) ? x * scale : 0 over a stream [batch, rows, dim], the mask from a counter-based generator
// The mask rule, the address arithmetic and the per-lane body are token_dropout.h (shared with tools/tokendrop_host_check.cpp).
// Nothing but the seed is read besides x: the backward calls the same entry on the gradient with the same seed.  A lane moves 16
// bytes (fp32: one group of four channels, one Philox call; bf16: two groups where dim allows, else one of 8 bytes), a grid-stride
// loop covers any size from any grid, every output element is written.
#include "common.h"
#include "token_dropout.h"

template <typename T, typename Vec, int GROUPS>
__global__ void __launch_bounds__(256)
token_dropout_kernel(const T* in, int64_t in_bs, int64_t in_rs, T* out, int64_t out_bs, int64_t out_rs, int64_t batch, int rows, int dim,
                     int tokens, uint32_t stream_id, const int* __restrict__ keep, int K, int lead, const int64_t* __restrict__ seed,
                     uint32_t thr, float scale) {
    td_walk<T, Vec, GROUPS>(in, in_bs, in_rs, out, out_bs, out_rs, batch, rows, dim, tokens, stream_id, keep, K, lead, (uint64_t)*seed, thr,
                            scale, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// [first, last) of the bytes an operand [batch, rows, dim] with these strides spans
static void td_span(const void* p, int64_t bs, int64_t rs, int64_t batch, int rows, int dim, int elem, uintptr_t* first, uintptr_t* last) {
    *first = (uintptr_t)p;
    *last = *first + (uintptr_t)(((batch - 1) * bs + (rows - 1) * rs + dim) * elem);
}

extern "C" int vited_token_dropout(const void* x, int64_t x_bs, int64_t x_rs, void* out, int64_t out_bs, int64_t out_rs, int dtype,
                                   int64_t batch, int rows, int dim, int tokens, int stream_id, const int32_t* keep, int K, int lead,
                                   const int64_t* seed, int64_t thr, float scale, void* stream) {
    if (!x || !out || !seed || batch <= 0 || rows <= 0 || dim <= 0 || tokens <= 0 || dim % 4) return VITED_ERR_BAD_ARG;
    if (thr < 0 || thr > 0xffffffffll || (stream_id != 0 && stream_id != 1) || (lead != 0 && lead != 1)) return VITED_ERR_BAD_ARG;
    if (keep ? (K <= 0 || K + 1 != rows || rows > tokens || (uintptr_t)keep % 4) : rows != tokens) return VITED_ERR_BAD_ARG;
    if (batch > (INT64_MAX / 4) / ((int64_t)tokens * dim)) return VITED_ERR_BAD_ARG;       // the element address stays an int64
    if (dtype != VITED_F32 && dtype != VITED_BF16) return VITED_ERR_UNSUPPORTED;
    if (dim > TD_MAX_DIM) return VITED_ERR_UNSUPPORTED;
    const int elem = dtype == VITED_F32 ? 4 : 2;
    const int64_t far = (int64_t)1 << 46;       // no stride of a real tensor; keeps the span arithmetic below inside an int64
    if (x_rs > far || out_rs > far || x_bs > far || out_bs > far || batch > far) return VITED_ERR_BAD_ARG;
    // rows and samples lie apart, and every piece of four channels is one aligned vector
    if (x_rs < dim || out_rs < dim || x_bs < (rows - 1) * x_rs + dim || out_bs < (rows - 1) * out_rs + dim) return VITED_ERR_BAD_ARG;
    if ((x_rs | x_bs | out_rs | out_bs) % 4 || ((uintptr_t)x | (uintptr_t)out) % (4 * elem) || (uintptr_t)seed % 8) return VITED_ERR_BAD_ARG;
    if (x != out || x_bs != out_bs || x_rs != out_rs) {        // in place is the same layout at the same address; anything else lies apart
        uintptr_t x0, x1, o0, o1;
        td_span(x, x_bs, x_rs, batch, rows, dim, elem, &x0, &x1);
        td_span(out, out_bs, out_rs, batch, rows, dim, elem, &o0, &o1);
        if (x0 < o1 && o0 < x1) return VITED_ERR_BAD_ARG;
    }
    const bool wide = dtype == VITED_BF16 && dim % 8 == 0 && (x_rs | x_bs | out_rs | out_bs) % 8 == 0 && ((uintptr_t)x | (uintptr_t)out) % 16 == 0;
    const int64_t total = batch * rows * (dim / (wide ? 8 : 4));
    int64_t blocks = ceil_div64(total, 256);
    if (blocks > 2048) blocks = 2048;       // 256 CUs x 8 workgroups; the loop strides over the rest
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t sid = (uint32_t)stream_id, t32 = (uint32_t)thr;
    if (dtype == VITED_F32)
        hipLaunchKernelGGL((token_dropout_kernel<float, TdF32x4, 1>), grid, block, 0, s, (const float*)x, x_bs, x_rs, (float*)out, out_bs, out_rs,
                           batch, rows, dim, tokens, sid, keep, K, lead, seed, t32, scale);
    else if (wide)
        hipLaunchKernelGGL((token_dropout_kernel<uint16_t, TdBf16x4, 2>), grid, block, 0, s, (const uint16_t*)x, x_bs, x_rs, (uint16_t*)out,
                           out_bs, out_rs, batch, rows, dim, tokens, sid, keep, K, lead, seed, t32, scale);
    else
        hipLaunchKernelGGL((token_dropout_kernel<uint16_t, TdBf16x4, 1>), grid, block, 0, s, (const uint16_t*)x, x_bs, x_rs, (uint16_t*)out,
                           out_bs, out_rs, batch, rows, dim, tokens, sid, keep, K, lead, seed, t32, scale);
    return vited_check_launch();
}
