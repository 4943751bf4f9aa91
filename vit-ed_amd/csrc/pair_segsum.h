// Segmented sum behind vited_attention_bwd_indexed: the attention backward kernels leave one dK / dV term per PAIR in a
// workspace, this reduction adds the terms of the pairs that share a key/value item, in ascending pair order, into that item's
// dK / dV.  The body is plain C++ (one call = one 16-byte piece of one output row) so that the same text runs inside the HIP
// kernel (attention_segsum.hip) and in a host program under the sanitizers (tools/segsum_host_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SEGSUM_FN __host__ __device__ __forceinline__
#else
#define SEGSUM_FN inline
#endif

struct SegSumArgs {
    const void* ws;           // per-pair terms [batch][nk][2 * width]: dK in columns [0, width), dV in [width, 2 width)
    void* out[2];             // dK, dV of the items: element (g, row, c) at out + g * out_bs + row * out_ts + c
    int64_t out_bs[2], out_ts[2];
    const int64_t* order;     // [batch]: pair numbers grouped by item, ascending inside a group
    const int64_t* offsets;   // [items + 1]: group g is order[offsets[g] .. offsets[g + 1])
    int64_t batch, items, nk;
    int width;                // heads * head_dim
};

template <typename T, int V> struct alignas(sizeof(T) * V) SegSumVec { T v[V]; };

// Output piece `chunk` (V elements: chunk = row * (width / V) + piece) of dK (which = 0) or dV (which = 1) of item g.  fp32
// accumulation seeded with the first term (so that a single term passes through bit for bit, -0 included), one rounding to T;
// an item without pairs is written as zeros.  Offsets and pair numbers outside the tables' ranges are skipped, never followed.
template <typename T, int V>
SEGSUM_FN void segsum_chunk(const SegSumArgs& a, int64_t g, int which, int64_t chunk) {
    typedef SegSumVec<T, V> Vec;
    const int cpr = a.width / V;
    const int64_t row = chunk / cpr;
    const int col = (int)(chunk - row * cpr) * V;
    const int64_t ws_ts = 2 * (int64_t)a.width, ws_bs = a.nk * ws_ts;
    int64_t s0 = a.offsets[g], s1 = a.offsets[g + 1];
    s0 = s0 < 0 ? 0 : (s0 > a.batch ? a.batch : s0);
    s1 = s1 < s0 ? s0 : (s1 > a.batch ? a.batch : s1);
    float acc[V];
    bool first = true;
    for (int64_t s = s0; s < s1; ++s) {
        const int64_t b = a.order[s];
        if (b < 0 || b >= a.batch) continue;
        const Vec t = *(const Vec*)((const T*)a.ws + b * ws_bs + row * ws_ts + (int64_t)which * a.width + col);
        if (first) {
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] = (float)t.v[e];
            first = false;
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] += (float)t.v[e];
        }
    }
    Vec r;
#pragma unroll
    for (int e = 0; e < V; ++e) r.v[e] = first ? (T)0.f : (T)acc[e];
    *(Vec*)((T*)a.out[which] + g * a.out_bs[which] + row * a.out_ts[which] + col) = r;
}
