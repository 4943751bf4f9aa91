// vited_mined_bce: the BCE-with-logits loss of the two-stage training step over the rows of a mined pair list (vited_mine_pairs),
// and its gradient, in ONE launch of one workgroup.  Everything it reads lies in device memory, the pair count
// included, so a captured hipGraph follows whatever the mining launch in front of it left.
//
// The rule, per element (r, c) of logits [rows, classes] with x = logits[r, c], y = labels[r], w = weights[r]:
//   term    = (1 - y) x + m + log(exp(-m) + exp(-x - m)),  m = max(-x, 0)       the stable form of cls_metrics.hip
//   sigma-y = (1 - y) - q  for x >= 0,  q - y  for x < 0,  q = e / (1 + e),  e = exp(-|x|)     (sigmoid(x) - y without cancellation)
//   denom   = (float)max(counts[3], 1) * (float)classes  for the mean,  1  for the sum
//   loss    = (scale * sum over the elements of (w != 0 ? w * term : +0)) / denom
//   dlogits = w != 0 ? ((scale * w) * (sigma-y)) / denom : +0
// The weight is a SELECT: a row with weight 0 (padding) gives an exact +0 term and an exact +0 gradient whatever its logit holds, NaN
// and inf included.  A NaN or inf logit in a weighted row reaches the loss (fmaxf drops a NaN from m, (1 - y) x keeps it), as torch's does.
//
// Order of the sum: thread t of 256 adds the flattened elements t, t + 256, ... in ascending order, a wave's 64 sums meet in a
// butterfly (every lane the same bits), and lane 0 adds the four wave sums in wave order.  No atomics: the same bits on every call,
// and - the padding rows lying behind the pairs and adding +0 - the same bits whatever the capacity.  Contraction is off, so that
// every product and sum above rounds on its own.
#include "common.h"
#include "pair_mine.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / VITED_WAVE;
constexpr int MAX_CLASSES = 64;

__global__ void __launch_bounds__(THREADS) mined_bce_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                            const float* __restrict__ weights, const int32_t* __restrict__ counts,
                                                            int rows, int classes, int mean, float scale, float* __restrict__ loss,
                                                            float* __restrict__ dlogits) {
    __shared__ float wave_loss[WAVES];
    const int t = threadIdx.x;
    const int pairs = counts[3];
    const float denom = mean ? (float)(pairs > 1 ? pairs : 1) * (float)classes : 1.0f;
    const int total = rows * classes;                                    // <= 24,576 * 64
    float sum = 0.0f;
    for (int e = t; e < total; e += THREADS) {
        const int r = e / classes;
        const float x = logits[e], y = labels[r], w = weights[r];
        const float m = fmaxf(-x, 0.0f);
        const float term = (1.0f - y) * x + m + logf(expf(-m) + expf(-x - m));
        const float ex = expf(-fabsf(x));
        const float q = ex / (1.0f + ex);
        const float g = x >= 0.0f ? (1.0f - y) - q : q - y;              // a NaN logit: q is NaN either way
        const bool live = w != 0.0f;
        sum = sum + (live ? w * term : 0.0f);
        dlogits[e] = live ? ((scale * w) * g) / denom : 0.0f;
    }
    sum = wave_sum(sum);
    if (t % VITED_WAVE == 0) wave_loss[t / VITED_WAVE] = sum;
    __syncthreads();
    if (t == 0) {
        float all = wave_loss[0];
        for (int v = 1; v < WAVES; ++v) all = all + wave_loss[v];
        loss[0] = (scale * all) / denom;
    }
}

}  // namespace

extern "C" int vited_mined_bce(const float* logits, const float* labels, const float* weights, const int32_t* counts, int64_t rows,
                               int64_t classes, int mean, float scale, float* loss, float* dlogits, void* stream) {
    if (!logits || !labels || !weights || !counts || !loss || !dlogits) return VITED_ERR_BAD_ARG;
    if (rows < 1 || classes < 1 || !(scale == scale) || scale - scale != 0.0f) return VITED_ERR_BAD_ARG;
    if (rows > MINE_MAX_CAPACITY || classes > MAX_CLASSES) return VITED_ERR_UNSUPPORTED;
    if (((uintptr_t)logits | (uintptr_t)labels | (uintptr_t)weights | (uintptr_t)counts | (uintptr_t)loss | (uintptr_t)dlogits) % 4)
        return VITED_ERR_BAD_ARG;
    hipLaunchKernelGGL(mined_bce_kernel, dim3(1), dim3(THREADS), 0, static_cast<hipStream_t>(stream), logits, labels, weights, counts,
                       (int)rows, (int)classes, mean != 0, scale, loss, dlogits);
    return vited_check_launch();
}
