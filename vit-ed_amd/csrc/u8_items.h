// Four-pixel items of the planar uint8 crops [3, S, S] that the device feeds write (hisfrag_feed.hip, michigan_feed.hip): a lane owns
// four consecutive x of one row for all three channels, one packed dword per channel.
#pragma once
#include "common.h"

__device__ __forceinline__ int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 32768) >> 16; }

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ void store_item(uint8_t* __restrict__ o, int64_t plane, int S, int y, int x0, const uint32_t pk[3], bool dwords) {
    uint8_t* row = o + (int64_t)y * S + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (dwords) {
            *reinterpret_cast<uint32_t*>(row + c * plane) = pk[c];            // S % 4 == 0: every item is whole and aligned
        } else {
            for (int j = 0; j < 4 && x0 + j < S; ++j) row[c * plane + j] = (uint8_t)(pk[c] >> (8 * j));
        }
    }
}

__device__ __forceinline__ void load_item(const uint8_t* __restrict__ in, int64_t plane, int S, int y, int x0, uint32_t pk[3], bool dwords) {
    const uint8_t* row = in + (int64_t)y * S + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (dwords) {
            pk[c] = *reinterpret_cast<const uint32_t*>(row + c * plane);
        } else {
            pk[c] = 0u;
            for (int j = 0; j < 4 && x0 + j < S; ++j) pk[c] |= (uint32_t)row[c * plane + j] << (8 * j);
        }
    }
}
