// How the ranking kernels (rank_metrics.hip, rank_lists.hip) read a matrix row: element loads widened to fp32, and the 16-byte
// vectors the bulk of a row is read with, behind an unaligned head and before a tail.  Device code only.
#pragma once
#include "common.h"

namespace rank_row {

typedef _Float16 f16;

__device__ __forceinline__ float load_f32(const float* p) { return *p; }
__device__ __forceinline__ float load_f32(const bf16* p) { return (float)*p; }
__device__ __forceinline__ float load_f32(const f16* p) { return (float)*p; }

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

// Elements of a row of n before the first 16-byte boundary (all of them when the row ends first).
template <typename T> __device__ __forceinline__ int64_t head_elements(const T* row, int64_t n) {
    return min(n, (int64_t)(((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) / sizeof(T)));
}

}  // namespace rank_row
