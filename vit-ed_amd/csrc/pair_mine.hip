// vited_mine_pairs: the pair mining of the two-stage training step (hisfrag.py:117-145, michigan.py:120-150) in ONE launch of
// ONE workgroup, with a fixed-shape result and no host read: pairs, labels, validity weights, the PairSegments tables of the
// image-1 column and five counts (pair_mine.h holds the rule and the per-lane bodies).
//   phase 1  classify the n * n cells, 1,024 per round in ascending cell order; a wave ballot + the 16 wave totals give every
//            positive its output row, which is written at once; every cell's sort word goes to LDS; candidates are counted
//   phase 2  bitonic sort of the (key, cell) words in LDS (the next power of two of n * n entries; non-candidates are all-ones)
//   phase 3  the kept negatives and the padding rows; then a stable counting pass over column 1: per-item counts (LDS atomics),
//            a scan, and per item a ballot walk over the rows in order (16 waves take the items in turn)
// Every output element is written on every call by an ordinary vector store; nothing in global memory is read back or updated
// atomically, so two calls on the same operands give the same bits.
#include <mutex>

#include "common.h"
#include "pair_mine.h"

namespace {

// dynamic LDS: [sort words: size x 8][targets: 128 x 8][count: 128 x 4][start: 132 x 4][wave totals: 2 x 16 x 4][candidates: 16 x 4]
// [row_item: capacity x 1]; every offset a multiple of 16
constexpr int LDS_TARGETS = MINE_MAX_IMAGES * 8;
constexpr int LDS_COUNT = MINE_MAX_IMAGES * 4;
constexpr int LDS_START = (MINE_MAX_IMAGES + 4) * 4;
constexpr int LDS_WAVE = 2 * MINE_WAVES * 4;
constexpr int LDS_CAND = MINE_WAVES * 4;
constexpr int LDS_FIXED = LDS_TARGETS + LDS_COUNT + LDS_START + LDS_WAVE + LDS_CAND;
static_assert(LDS_FIXED % 16 == 0, "LDS carve offsets are multiples of 16");
constexpr int LDS_MAX = MINE_MAX_IMAGES * MINE_MAX_IMAGES * 8 + LDS_FIXED + MINE_MAX_CAPACITY;
static_assert(LDS_MAX <= 160 * 1024, "one workgroup may declare 160 KiB");

static size_t lds_bytes(int n, int capacity) { return (size_t)mine_sort_size(n) * 8 + LDS_FIXED + (size_t)((capacity + 15) / 16 * 16); }

__global__ void __launch_bounds__(MINE_THREADS) mine_pairs_kernel(MineArgs a, int size) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* words = (uint64_t*)smem;
    int64_t* tgt = (int64_t*)(smem + (size_t)size * 8);
    int* count = (int*)((char*)tgt + LDS_TARGETS);
    int* start = (int*)((char*)count + LDS_COUNT);
    int* wave_pos = (int*)((char*)start + LDS_START);          // [2][MINE_WAVES]
    int* wave_cand = (int*)((char*)wave_pos + LDS_WAVE);        // [MINE_WAVES]
    uint8_t* row_item = (uint8_t*)((char*)wave_cand + LDS_CAND);
    const int t = threadIdx.x, lane = t % MINE_WAVE, wave = t / MINE_WAVE;

    if (t < MINE_MAX_IMAGES) {
        tgt[t] = t < a.n ? a.targets[t] : 0;
        count[t] = 0;
    }
    __syncthreads();

    // ---- phase 1 ----
    int npos = 0, cand_here = 0;                                // npos: uniform; cand_here: this wave's candidates so far
    for (int base = 0, round = 0; base < size; base += MINE_THREADS, ++round) {
        const int c = base + t;
        const int kind = c < size ? mine_classify(tgt, a.n, a.ordered, c) : 0;
        if (c < size) words[c] = mine_sort_word(kind == MINE_CAND ? a.keys[c] : 0.0f, c, kind == MINE_CAND);
        const uint64_t pos_mask = __ballot(kind == MINE_POS);
        cand_here += __builtin_popcountll(__ballot(kind == MINE_CAND));
        int* totals = wave_pos + (round & 1) * MINE_WAVES;      // two buffers: the next round's writes need no second barrier
        if (lane == 0) totals[wave] = __builtin_popcountll(pos_mask);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < MINE_WAVES; ++w) {
            const int v = totals[w];
            before += w < wave ? v : 0;
            all += v;
        }
        if (kind == MINE_POS) mine_emit_positive(a, row_item, c, npos + before + mine_rank(pos_mask, lane));
        npos += all;
    }
    if (lane == 0) wave_cand[wave] = cand_here;
    __syncthreads();                                            // also: every sort word is in place
    int ncand = 0;
#pragma unroll
    for (int w = 0; w < MINE_WAVES; ++w) ncand += wave_cand[w];
    const MineCounts m = mine_counts(npos, ncand, a.neg_per_pos, a.capacity);

    // ---- phase 2 ---- (nothing to order when no negative is emitted)
    if (m.neg_rows > 0) {
        for (int k = 2; k <= size; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int p = t; p < size / 2; p += MINE_THREADS) mine_bitonic_pair(words, p, k, j);
                __syncthreads();
            }
    }

    // ---- phase 3 ----
    for (int r = m.pos_rows + t; r < a.capacity; r += MINE_THREADS) mine_emit_tail(a, m, words, row_item, r);
    if (t == 0) {
#pragma unroll
        for (int e = 0; e < 5; ++e) a.counts[e] = m.out[e];
    }
    __syncthreads();                                            // row_item is complete
    for (int r = t; r < a.capacity; r += MINE_THREADS) atomicAdd(&count[row_item[r]], 1);
    __syncthreads();
    if (t == 0) mine_scan_offsets(a, count, start);
    __syncthreads();
    for (int g = wave; g < a.n; g += MINE_WAVES) {
        int base = start[g];
        for (int b = 0; b < a.capacity; b += MINE_WAVE) {
            const int r = b + lane;
            const bool mine = r < a.capacity && row_item[r] == g;
            const uint64_t mask = __ballot(mine);
            if (mine) mine_place_row(a, base, mask, lane, r);
            base += __builtin_popcountll(mask);
        }
    }
}

}  // namespace

extern "C" int vited_mine_pairs_max_images(void) { return MINE_MAX_IMAGES; }

extern "C" int vited_mine_pairs(const int64_t* targets, int n, const float* keys, double neg_per_pos, int ordered_negatives,
                                int64_t capacity, int64_t* groups, float* labels, float* weights, int64_t* seg_index, int64_t* seg_order,
                                int64_t* seg_offsets, int32_t* counts, void* stream) {
    if (!targets || !keys || !groups || !labels || !weights || !seg_index || !seg_order || !seg_offsets || !counts)
        return VITED_ERR_BAD_ARG;
    if (n <= 0 || capacity <= 0) return VITED_ERR_BAD_ARG;
    if (n > MINE_MAX_IMAGES || capacity > MINE_MAX_CAPACITY) return VITED_ERR_UNSUPPORTED;
    static std::once_flag once;
    static hipError_t status = hipSuccess;
    std::call_once(once, [&] { status = hipFuncSetAttribute((const void*)mine_pairs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX); });
    if (status != hipSuccess) return VITED_ERR_LAUNCH;
    MineArgs a = {};
    a.targets = targets;
    a.keys = keys;
    a.n = n;
    a.ordered = ordered_negatives != 0;
    a.capacity = (int)capacity;
    a.neg_per_pos = neg_per_pos;
    a.groups = groups;
    a.labels = labels;
    a.weights = weights;
    a.seg_index = seg_index;
    a.seg_order = seg_order;
    a.seg_offsets = seg_offsets;
    a.counts = counts;
    hipLaunchKernelGGL(mine_pairs_kernel, dim3(1), dim3(MINE_THREADS), lds_bytes(n, (int)capacity), static_cast<hipStream_t>(stream), a,
                       mine_sort_size(n));
    return vited_check_launch();
}
