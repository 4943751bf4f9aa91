// Second half of vited_attention_bwd_indexed: per-pair dK / dV terms (workspace) -> per-item dK / dV.  Bandwidth-bound: every
// thread owns one 16-byte piece of one output row, walks its item's pairs in ascending pair order (pair_segsum.h) and stores
// once - no atomics, every output element written exactly once, the same bits on every call.
#include "attention_kernels.h"
#include "pair_segsum.h"

#define SEGSUM_THREADS 256

template <typename T, int V>
__global__ void __launch_bounds__(SEGSUM_THREADS)
attn_segsum_kernel(SegSumArgs a) {
    const int64_t chunk = (int64_t)blockIdx.x * SEGSUM_THREADS + threadIdx.x;
    if (chunk >= a.nk * (a.width / V)) return;
    segsum_chunk<T, V>(a, blockIdx.y, blockIdx.z, chunk);
}

template <typename T>
static int launch_segsum(const SegSumArgs& a, hipStream_t s) {
    constexpr int V = 16 / sizeof(T);
    auto al = [](const void* p) { return ((uintptr_t)p % 16) == 0; };
    bool wide = a.width % V == 0 && al(a.ws) && al(a.out[0]) && al(a.out[1]);
    for (int i = 0; i < 2; ++i) wide = wide && a.out_bs[i] % V == 0 && a.out_ts[i] % V == 0;
    const int64_t chunks = a.nk * (a.width / (wide ? V : 1));
    const int64_t blocks = ceil_div64(chunks, SEGSUM_THREADS);
    if (blocks > 0x7fffffff) return VITED_ERR_UNSUPPORTED;
    dim3 grid((unsigned)blocks, (unsigned)a.items, 2);
    if (wide) hipLaunchKernelGGL((attn_segsum_kernel<T, V>), grid, dim3(SEGSUM_THREADS), 0, s, a);
    else hipLaunchKernelGGL((attn_segsum_kernel<T, 1>), grid, dim3(SEGSUM_THREADS), 0, s, a);
    return vited_check_launch();
}

int attention_segsum(const SegSumArgs& a, int dtype, hipStream_t s) {
    if (dtype == VITED_F32) return launch_segsum<float>(a, s);
    if (dtype == VITED_BF16) return launch_segsum<bf16>(a, s);
    return VITED_ERR_UNSUPPORTED;
}
