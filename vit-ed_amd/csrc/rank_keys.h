// Row-ranking helpers shared by the retrieval kernels (retrieval.hip, group_metrics.hip): 64-bit keys (order bits of the value,
// column) that reproduce np.argsort(kind='stable') with NaN last, the binary search against a sorted LDS key array, 16-byte row
// loads and the LDS histogram scan.
#pragma once
#include "common.h"

namespace {

constexpr uint64_t PAD_KEY = ~0ull;          // above every real key (a real key's low word is a column index < 2^31)

typedef _Float16 f16;

__device__ __forceinline__ float load_f32(const float* p) { return *p; }
__device__ __forceinline__ float load_f32(const bf16* p) { return (float)*p; }
__device__ __forceinline__ float load_f32(const f16* p) { return (float)*p; }

// Order-preserving 32-bit image of a float: every NaN maps above +inf (to one value, so NaNs tie and fall back to the column
// order), -0 ties with +0.
__device__ __forceinline__ uint32_t order_bits(float v) {
    if (v != v) return 0xffffffffu;
    if (v == 0.0f) v = 0.0f;
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint64_t make_key(float v, int64_t j) { return ((uint64_t)order_bits(v) << 32) | (uint32_t)j; }

// Number of keys[0, p2) that are <= k (keys ascending, padded with PAD_KEY to the power of two p2).
__device__ __forceinline__ int count_le(const uint64_t* keys, int p2, uint64_t k) {
    int pos = 0;
    for (int s = p2; s > 0; s >>= 1)
        if (pos + s <= p2 && keys[pos + s - 1] <= k) pos += s;
    return pos;
}

template <typename T> struct Vec;          // 16-byte loads: 4 fp32 or 8 half-width values
template <> struct Vec<float> { static constexpr int N = 4; typedef float4 type; };
template <> struct Vec<bf16> { static constexpr int N = 8; typedef uint4 type; };
template <> struct Vec<f16> { static constexpr int N = 8; typedef uint4 type; };

__device__ __forceinline__ void unpack(const float4& v, float* out) { out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w; }
template <typename T> __device__ __forceinline__ void unpack_half(const uint4& v, float* out) {
    const T* h = reinterpret_cast<const T*>(&v);
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = (float)h[e];
}

// Inclusive prefix sum of h[0, cnt) in place (cnt <= CHUNK = THREADS * 8): each thread scans 8 consecutive bins.
__device__ void block_inclusive_scan(uint32_t* h, int cnt, uint32_t* wave_tot) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t v[8], s = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int b = t * 8 + e;
        v[e] = b < cnt ? h[b] : 0u;
        s += v[e];
    }
    uint32_t x = s;                                     // inclusive scan of the thread totals over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) wave_tot[wave] = x;
    __syncthreads();
    uint32_t base = x - s;
    for (int w = 0; w < wave; ++w) base += wave_tot[w];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        base += v[e];
        const int b = t * 8 + e;
        if (b < cnt) h[b] = base;
    }
    __syncthreads();
}

}  // namespace
