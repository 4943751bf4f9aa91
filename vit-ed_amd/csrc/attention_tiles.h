// Shared device helpers of the bf16 MFMA attention kernels (attention_mfma.hip: short sequences,
// attention_flash.hip: tiled online-softmax for long sequences).
#pragma once
#include "attention_kernels.h"

#define SM_MAX_TILES 5  // 5 x 16 = 80 tokens

__device__ __forceinline__ bf16x4 tr_read4(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)p);
}

template <int HD> struct SmallCfg {
    static constexpr int ROW_BYTES = HD * 2;          // one token's head slice
    static constexpr int KCH = HD / 32;               // 32-wide k-steps of a q.k dot product
    static constexpr int DT = HD / 16;                // 16-wide tiles of the head dim
    static constexpr int TILE_BYTES = (SM_MAX_TILES + 1) * 16 * ROW_BYTES;  // +1: zero phantom tile of an odd last k-step
    // XOR on the 32-byte slot index so the 8 rows x 32 B a half-wave reads per tr-read hit 64 distinct banks
    __device__ static __forceinline__ int swz(int r) { return HD == 32 ? ((r >> 2) & 1) << 5 : ((r >> 1) & 3) << 5; }
    __device__ static __forceinline__ int off(int r, int byte_in_row) { return r * ROW_BYTES + (byte_in_row ^ swz(r)); }
};

// 16-row x HD tile -> registers in MFMA row-fragment form (lane: row fr, 8 elements at 8*(g + 4*c)),
// rows clamped to n-1.
template <int HD>
__device__ __forceinline__ void load_row_frags(const bf16* base, int64_t ts, int row0, int n, int fr, int g,
                                               bf16x8 (&f)[HD / 32]) {
    int r = row0 + fr;
    r = r < n ? r : n - 1;
#pragma unroll
    for (int c = 0; c < HD / 32; ++c) f[c] = *(const bf16x8*)(base + (int64_t)r * ts + 8 * (g + 4 * c));
}

template <int HD>
__device__ __forceinline__ void stage_tile(char* lds, int row0, int n, int fr, int g, const bf16x8 (&f)[HD / 32]) {
    const int r = row0 + fr;
#pragma unroll
    for (int c = 0; c < HD / 32; ++c) {
        bf16x8 v = f[c];
        if (r >= n) v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        *(bf16x8*)(lds + SmallCfg<HD>::off(r, 16 * (g + 4 * c))) = v;
    }
}

// transposed operand: 16 (head-dim) x 32 (token) fragment for k-step ks of tile image `lds`, with the
// in-step token order (4g..4g+3 of the even tile, then 4g..4g+3 of the odd tile) that matches an
// accumulator pair used as the other operand.
template <int HD>
__device__ __forceinline__ bf16x8 tr_frag(const char* lds, int ks, int dt, int g, int qq, int p) {
    const int r0 = 32 * ks + 4 * g + qq, r1 = r0 + 16;
    const bf16x4 lo = tr_read4(lds + SmallCfg<HD>::off(r0, dt * 32 + 8 * p));
    const bf16x4 hi = tr_read4(lds + SmallCfg<HD>::off(r1, dt * 32 + 8 * p));
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

__device__ __forceinline__ bf16x8 pack_pair(const f32x4& a, const f32x4& b) {
    return bf16x8{(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)b[0], (bf16)b[1], (bf16)b[2], (bf16)b[3]};
}

__device__ __forceinline__ float group_max4(float v) {  // over the 4 lanes that share lane & 15
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum4(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

#define LOG2E 1.4426950408889634f
#define LN2 0.6931471805599453f

// ---- 64-row tiles of the long-sequence kernels (attention_flash.hip, attention_cam.hip): staging and fragment helpers ----
#define FL_TILE 64   // keys (or queries) per LDS tile
#ifndef FL_W
#define FL_W 2       // 16-row tiles per wave
#endif

template <int HD> struct FlashCfg {
    using C = SmallCfg<HD>;
    static constexpr int TILE_BYTES = FL_TILE * C::ROW_BYTES;
    static constexpr int CHUNKS_PER_ROW = HD / 8;
    static constexpr int PASSES = FL_TILE * CHUNKS_PER_ROW / 256;   // 16-byte chunks per thread and tile
};

// This thread's 16-byte chunks of a 64-row tile: what does not change from tile to tile (the loops below are VALU-bound - PMC:
// 8 vector instructions per MFMA in the forward - and the staging arithmetic redone per tile was a third of them: row clamp as
// compare + select, 64-bit row * stride, the swizzle, a select per stored dword).
template <int HD> struct TileMap {
    int row[FlashCfg<HD>::PASSES];   // row inside the tile
    int col2[FlashCfg<HD>::PASSES];  // column, in bytes
    int loff[FlashCfg<HD>::PASSES];  // byte offset inside the swizzled LDS image
    __device__ __forceinline__ TileMap(int tid) {
#pragma unroll
        for (int c = 0; c < FlashCfg<HD>::PASSES; ++c) {
            const int idx = tid + 256 * c;
            const int ch = idx % FlashCfg<HD>::CHUNKS_PER_ROW;
            row[c] = idx / FlashCfg<HD>::CHUNKS_PER_ROW;
            col2[c] = ch * 16;
            loff[c] = SmallCfg<HD>::off(row[c], ch * 16);
        }
    }
};
// cooperative tile copy, global -> registers.  Rows past n - 1 re-read row n - 1 (finite values; regs_to_tile zeroes them): the
// clamp is one v_min against a wave-uniform bound and the address is a 64-bit uniform tile base + a 32-bit per-lane byte offset
// (attention_fwd_flash / attention_bwd_flash refuse token strides of 2^24 elements or more) ...
template <int HD>
__device__ __forceinline__ void tile_to_regs(const bf16* base, int64_t ts, int row0, int n, const TileMap<HD>& m, bf16x8 (&r)[FlashCfg<HD>::PASSES]) {
    const char* tb = (const char*)(base + (int64_t)row0 * ts);   // wave-uniform
    const int last = n - 1 - row0;                               // >= 0: a tile is only staged when it holds a valid row
    const unsigned ts2 = (unsigned)ts * 2u;
#pragma unroll
    for (int c = 0; c < FlashCfg<HD>::PASSES; ++c) {
        const unsigned rr = (unsigned)(m.row[c] < last ? m.row[c] : last);
        r[c] = *(const bf16x8*)(tb + (rr * ts2 + (unsigned)m.col2[c]));
    }
}
// ... and registers -> LDS image (rows >= n zeroed; only the ragged last tile pays for the selects)
template <int HD>
__device__ __forceinline__ void regs_to_tile(char* lds, int row0, int n, const TileMap<HD>& m, const bf16x8 (&r)[FlashCfg<HD>::PASSES]) {
    if (row0 + FL_TILE > n) {   // wave-uniform
        asm volatile("" ::: "memory");   // keep this a branch: if-converted it costs a select per stored dword on EVERY tile
#pragma unroll
        for (int c = 0; c < FlashCfg<HD>::PASSES; ++c) {
            bf16x8 v = r[c];
            if (row0 + m.row[c] >= n) v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            *(bf16x8*)(lds + m.loff[c]) = v;
        }
    } else {
#pragma unroll
        for (int c = 0; c < FlashCfg<HD>::PASSES; ++c) *(bf16x8*)(lds + m.loff[c]) = r[c];
    }
}
// MFMA row fragment (row fr of 16-row tile t, k chunk g + 4c) out of an LDS image
template <int HD>
__device__ __forceinline__ void lds_row_frags(const char* lds, int t, int fr, int g, bf16x8 (&f)[HD / 32]) {
#pragma unroll
    for (int c = 0; c < HD / 32; ++c) f[c] = *(const bf16x8*)(lds + SmallCfg<HD>::off(16 * t + fr, 16 * (g + 4 * c)));
}
