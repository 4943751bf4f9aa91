// Host build of the segmented sum of vited_attention_bwd_indexed (csrc/pair_segsum.h) for the address and undefined-behaviour
// sanitizers: the very text the HIP kernel runs, driven over the index tables of tests/test_gpu_pair_index.py with exactly-sized
// heap buffers, every output piece visited once like the kernel's grid does, and compared with a plain double loop.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vit-ed_amd/csrc tools/segsum_host_check.cpp -o segsum_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pair_segsum.h"

template <typename T>
static int run_case(const char* name, std::vector<int64_t> index, int64_t items, int64_t nk, int width, bool wide) {
    const int64_t batch = (int64_t)index.size();
    std::vector<int64_t> order, offsets(items + 1, 0);
    for (int64_t g = 0; g < items; ++g) {          // stable grouping: ascending pair number inside an item
        for (int64_t b = 0; b < batch; ++b)
            if (index[b] == g) order.push_back(b);
        offsets[g + 1] = (int64_t)order.size();
    }
    // exactly-sized allocations (aligned_alloc: the 16-byte pieces need it), so that any step outside them is an ASan report
    const size_t ws_n = (size_t)(batch * nk * 2 * width), out_n = (size_t)(items * nk * 2 * width);
    T* ws = (T*)aligned_alloc(16, ws_n * sizeof(T));           // multiples of 16 bytes in every case below
    T* out = (T*)aligned_alloc(16, out_n * sizeof(T));
    unsigned s = 12345u + (unsigned)batch;
    for (size_t i = 0; i < ws_n; ++i) {
        s = s * 1664525u + 1013904223u;
        ws[i] = (T)(((int)(s >> 20) % 2001 - 1000) / 256.0f);
    }
    memset(out, 0xff, out_n * sizeof(T));           // NaN bit patterns: an unwritten element shows
    SegSumArgs a = {};
    a.ws = ws;
    a.out[0] = out;                                  // dK / dV as column views of a packed [items][nk][2 width] tensor
    a.out[1] = out + width;
    a.out_bs[0] = a.out_bs[1] = nk * 2 * width;
    a.out_ts[0] = a.out_ts[1] = 2 * width;
    a.order = order.data();
    a.offsets = offsets.data();
    a.batch = batch; a.items = items; a.nk = nk; a.width = width;
    constexpr int V = 16 / sizeof(T);
    const int64_t chunks = nk * (width / (wide ? V : 1));
    for (int which = 0; which < 2; ++which)
        for (int64_t g = 0; g < items; ++g)
            for (int64_t c = 0; c < chunks; ++c) {
                if (wide) segsum_chunk<T, V>(a, g, which, c);
                else segsum_chunk<T, 1>(a, g, which, c);
            }
    int bad = 0;
    for (int64_t g = 0; g < items; ++g)
        for (int64_t r = 0; r < nk; ++r)
            for (int c = 0; c < 2 * width; ++c) {
                float acc = 0.f;
                bool first = true;
                for (int64_t b = 0; b < batch; ++b)
                    if (index[b] == g) {
                        const float t = (float)ws[(b * nk + r) * 2 * width + c];
                        acc = first ? t : acc + t;
                        first = false;
                    }
                const T want = first ? (T)0.f : (T)acc;
                const T got = out[(g * nk + r) * 2 * width + c];
                if (memcmp(&want, &got, sizeof(T)) != 0) ++bad;
            }
    printf("%-28s %s V=%d: %s\n", name, sizeof(T) == 2 ? "bf16" : "fp32", wide ? V : 1, bad ? "MISMATCH" : "ok");
    free(ws);
    free(out);
    return bad;
}

template <typename T>
static int run_all() {
    int bad = 0;
    for (int wide = 0; wide < 2; ++wide) {
        bad += run_case<T>("[2,0,2,2,0] over 3, Nk 64", {2, 0, 2, 2, 0}, 3, 64, 384, wide);
        bad += run_case<T>("[1,1,0,1] over 2, Nk 256", {1, 1, 0, 1}, 2, 256, 384, wide);
        bad += run_case<T>("[3,1,0,2] over 4, Nk 65", {3, 1, 0, 2}, 4, 65, 128, wide);
        bad += run_case<T>("[1,3,1,2,3,3,1] over 4, Nk 64", {1, 3, 1, 2, 3, 3, 1}, 4, 64, 384, wide);
        bad += run_case<T>("[0,2,1,2,0] over 3, Nk 256", {0, 2, 1, 2, 0}, 3, 256, 384, wide);
    }
    return bad;
}

int main() {
    const int bad = run_all<float>() + run_all<__bf16>();
    printf(bad ? "segsum_host_check FAILED\n" : "segsum_host_check ok\n");
    return bad ? 1 : 0;
}
