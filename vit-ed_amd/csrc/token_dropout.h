// The mask rule of elementwise token dropout (token_dropout.hip; timm's pos_drop = nn.Dropout(pos_drop_rate)),
// written so that the device kernel and a host program under the sanitizers (tools/tokendrop_host_check.cpp) compile the same text.
//
// An element of a stream [batch, T, D] has the address e = (b T + t) D + d (int64), t being the token's ORIGINAL index in the stream -
// under a patch-dropout keep table the kept row's token, so a kept token carries the mask it would have had with every token present
// (timm drops before it selects).  The four elements of g = e >> 2 share one Philox4x32-10 call with the counter
// (lo32(g), hi32(g), stream, 0) and the key (lo32(seed), hi32(seed)); element e reads output word e & 3 and is KEPT iff word >= thr,
// thr = min(2^32 - 1, int(p 2^32)).  A kept element becomes x * scale (one fp32 multiply, rounded once to the output type), a
// dropped one 0 by selection, whatever it held.  Nothing is stored: the backward regenerates the mask from the seed.
#pragma once
#include <stdint.h>
#include <string.h>

#include "patch_keep.h"

#if defined(__HIPCC__)
#define TD_FN __host__ __device__ __forceinline__
#else
#define TD_FN inline
#endif

#define TD_MAX_DIM 1024         // the LayerNorm kernels' range: no stream of this model is wider

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of two 32 x 32 -> 64 bit
// products, the key bumped by the Weyl constants between rounds.  ctr is replaced by the output.
TD_FN void td_philox(uint32_t ctr[4], uint32_t k0, uint32_t k1) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * ctr[0], p1 = (uint64_t)0xCD9E8D57u * ctr[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ ctr[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ ctr[3] ^ k1;
        ctr[1] = (uint32_t)p1;
        ctr[3] = (uint32_t)p0;
        ctr[0] = n0;
        ctr[2] = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// the four words of the group that holds element e (e & 3 selects among them)
TD_FN void td_words(int64_t e, uint32_t stream, uint64_t seed, uint32_t w[4]) {
    const uint64_t g = (uint64_t)e >> 2;
    w[0] = (uint32_t)g;
    w[1] = (uint32_t)(g >> 32);
    w[2] = stream;
    w[3] = 0u;
    td_philox(w, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// original token of row r of a sample: r itself without a table; with one (keep: the sample's K indices) the prefix token 0 for
// r = 0 and the kept patch's token behind it, as vited_tokens_kept lays the rows out (lead = 1: patch 0 is the prefix and token
// = patch; lead = 0: the cls token is, and token = patch + 1).  Clamped into [0, tokens) like every table lookup.
TD_FN int td_token(const int* keep, int lead, int r, int tokens) {
    if (!keep || r == 0) return r < tokens ? r : tokens - 1;
    return lead ? pk_patch(keep, 1, r, tokens) : 1 + pk_patch(keep, 0, r - 1, tokens - 1);
}

// element address of channel c of token t of sample b
TD_FN int64_t td_address(int64_t b, int tokens, int t, int dim, int c) { return (b * tokens + t) * (int64_t)dim + c; }

// bf16 <-> fp32 on the bits: round to nearest even, NaN to the quiet NaN 0x7fc0 (what torch's conversion gives)
TD_FN float td_bf16_to_f32(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
TD_FN uint16_t td_f32_to_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

struct alignas(16) TdF32x4 { float v[4]; };
struct alignas(8) TdBf16x4 { uint16_t v[4]; };
// what one lane moves at a time: GROUPS groups of four channels as ONE aligned vector (16 bytes for fp32 x 1 and bf16 x 2)
template <typename Vec, int GROUPS> struct alignas(sizeof(Vec) * GROUPS) TdPack { Vec g[GROUPS]; };

TD_FN float td_load(const float& x) { return x; }
TD_FN float td_load(const uint16_t& x) { return td_bf16_to_f32(x); }
TD_FN void td_store(float& o, float v) { o = v; }
TD_FN void td_store(uint16_t& o, float v) { o = td_f32_to_bf16(v); }

// One lane's work: GROUPS consecutive groups of four channels starting at element address e (a multiple of 4), read from `in` and
// written to `out` (which may be `in`) as whole vectors.  Vec is TdF32x4 or TdBf16x4.
template <typename Vec, int GROUPS>
TD_FN void td_lane(const Vec* in, Vec* out, int64_t e, uint32_t stream, uint64_t seed, uint32_t thr, float scale) {
    TdPack<Vec, GROUPS> x = *(const TdPack<Vec, GROUPS>*)in;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int g = 0; g < GROUPS; ++g) {
        uint32_t w[4];
        td_words(e + 4 * g, stream, seed, w);
        for (int j = 0; j < 4; ++j) {
            const float scaled = td_load(x.g[g].v[j]) * scale;
            td_store(x.g[g].v[j], w[j] >= thr ? scaled : 0.0f);
        }
    }
    *(TdPack<Vec, GROUPS>*)out = x;
}

// The schedule: work item i of batch * rows * (dim / (4 GROUPS)) is the piece of 4 GROUPS channels at column c of row r of sample b;
// a "thread" `first` of `step` walks i = first, first + step, ...  Pointers and strides in elements of T (float or uint16_t).
template <typename T, typename Vec, int GROUPS>
TD_FN void td_walk(const T* in, int64_t in_bs, int64_t in_rs, T* out, int64_t out_bs, int64_t out_rs, int64_t batch, int rows, int dim,
                   int tokens, uint32_t stream, const int* keep, int K, int lead, uint64_t seed, uint32_t thr, float scale, int64_t first,
                   int64_t step) {
    const int pieces = dim / (4 * GROUPS);
    const int64_t total = batch * rows * pieces;
    for (int64_t i = first; i < total; i += step) {
        const int64_t row = i / pieces;
        const int c = (int)(i - row * pieces) * (4 * GROUPS);
        const int64_t b = row / rows;
        const int r = (int)(row - b * rows);
        const int t = td_token(keep ? keep + b * K : nullptr, lead, r, tokens);
        td_lane<Vec, GROUPS>((const Vec*)(in + b * in_bs + r * in_rs + c), (Vec*)(out + b * out_bs + r * out_rs + c),
                             td_address(b, tokens, t, dim, c), stream, seed, thr, scale);
    }
}
