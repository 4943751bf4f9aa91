// Validation metrics of one multi-output binary classification batch (main.py:49-132, DefaultTrainer.validate): the
// BCE-with-logits loss, and per output column sklearn's accuracy_score and macro f1 / precision / recall of pred = logit > 0,
// folded into device AverageMeters.  One workgroup per batch: config A is 1,024 x 4 elements.
//
// Bit-identical from run to run: the counts are integer (LDS atomics), the fp32 loss is summed in a fixed order (each lane a
// compensated sum in element order, so that its error does not grow with the batch; then a butterfly inside the wave and the
// waves in order), and the fp64 finish runs on one lane per column and then on
// one lane for the column averages.  Contraction is off so that  sum + val * B  rounds twice, as in Python.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / VITED_WAVE;
constexpr int MAX_CLASSES = 64;
constexpr int METERS = 5;          // loss, acc, f1, precision, recall

// sklearn 1.7's per-label value over the labels present in unique(gt U pred) ({0, 1} at most), then the macro mean in label
// order: (v0 + v1) / 2, or the one value.
__device__ __forceinline__ double macro_mean(bool has0, double v0, bool has1, double v1) {
    if (has0 && has1) return (v0 + v1) / 2.0;
    return has0 ? v0 : v1;
}

__device__ __forceinline__ double ratio_or_zero(int64_t num, int64_t den) { return den ? (double)num / (double)den : 0.0; }

__global__ void __launch_bounds__(THREADS) cls_metrics_kernel(const float* __restrict__ logits, int64_t ld_logits,
                                                              const float* __restrict__ targets, int64_t ld_targets, int batch,
                                                              int classes, double* __restrict__ meters, double* __restrict__ last,
                                                              int* __restrict__ bad) {
    __shared__ int n_true[MAX_CLASSES], n_pred[MAX_CLASSES], n_tp[MAX_CLASSES];
    __shared__ float wave_loss[WAVES];
    __shared__ double column[4][MAX_CLASSES];        // acc, f1, precision, recall of each column
    const int t = threadIdx.x;
    if (t < MAX_CLASSES) n_true[t] = n_pred[t] = n_tp[t] = 0;
    __syncthreads();

    // BCEWithLogits of one element in the stable form (1 - y) x + m + log(exp(-m) + exp(-x - m)), m = max(-x, 0); a NaN logit
    // gives a NaN loss (fmaxf drops the NaN from m, (1 - y) x keeps it) and pred 0.
    const int64_t total = (int64_t)batch * classes;
    float loss = 0.0f, carry = 0.0f;                 // each lane: a compensated (Kahan) sum over its elements
    bool flagged = false;
    for (int64_t e = t; e < total; e += THREADS) {
        const int r = (int)(e / classes), c = (int)(e - (int64_t)r * classes);
        const float x = logits[r * ld_logits + c], y = targets[r * ld_targets + c];
        const float m = fmaxf(-x, 0.0f);
        const float term = (1.0f - y) * x + m + logf(expf(-m) + expf(-x - m)) - carry;
        const float next = loss + term;
        carry = isfinite(next) ? (next - loss) - term : 0.0f;   // an inf element loss stays inf (inf - inf would be NaN)
        loss = next;
        if (y != 0.0f && y != 1.0f) {
            flagged = true;                          // not a class label: reported, not counted
            continue;
        }
        const bool truth = y == 1.0f, pred = x > 0.0f;
        if (truth) atomicAdd(&n_true[c], 1);
        if (pred) atomicAdd(&n_pred[c], 1);
        if (truth && pred) atomicAdd(&n_tp[c], 1);
    }
    if (flagged) atomicOr(bad, 1);
    loss = wave_sum(loss);
    if (t % VITED_WAVE == 0) wave_loss[t / VITED_WAVE] = loss;
    __syncthreads();

    if (t < classes) {
        const int64_t b = batch, nt1 = n_true[t], np1 = n_pred[t], tp1 = n_tp[t];
        const int64_t nt0 = b - nt1, np0 = b - np1, tp0 = b - nt1 - np1 + tp1;
        const bool has0 = nt0 > 0 || np0 > 0, has1 = nt1 > 0 || np1 > 0;
        column[0][t] = (double)(tp0 + tp1) / (double)b * 100.0;
        column[1][t] = macro_mean(has0, 2.0 * (double)tp0 / (double)(nt0 + np0), has1, 2.0 * (double)tp1 / (double)(nt1 + np1));
        column[2][t] = macro_mean(has0, ratio_or_zero(tp0, np0), has1, ratio_or_zero(tp1, np1));
        column[3][t] = macro_mean(has0, ratio_or_zero(tp0, nt0), has1, ratio_or_zero(tp1, nt1));
    }
    __syncthreads();

    if (t == 0) {
        float loss_sum = wave_loss[0];
        for (int w = 1; w < WAVES; ++w) loss_sum = loss_sum + wave_loss[w];
        double value[METERS];
        value[0] = (double)(loss_sum / (float)total);             // loss.item() of the fp32 mean
        for (int k = 0; k < 4; ++k) {                              // Python's sum(list) / len(list), columns in order
            double s = 0.0;
            for (int c = 0; c < classes; ++c) s = s + column[k][c];
            value[k + 1] = s / (double)classes;
        }
        const double n = (double)batch;
        for (int k = 0; k < METERS; ++k) {                         // AverageMeter.update(val, n=B)
            meters[2 * k] = meters[2 * k] + value[k] * n;
            meters[2 * k + 1] = meters[2 * k + 1] + n;
            last[k] = value[k];
        }
    }
}

}  // namespace

extern "C" int vited_cls_metrics_update(const float* logits, int64_t ld_logits, const float* targets, int64_t ld_targets, int64_t batch,
                                        int64_t classes, double* meters, double* last, int* bad, void* stream) {
    if (!logits || !targets || !meters || !last || !bad) return VITED_ERR_BAD_ARG;
    if (batch < 1 || batch > INT32_MAX || classes < 1 || classes > MAX_CLASSES) return VITED_ERR_BAD_ARG;
    if (ld_logits < classes || ld_targets < classes) return VITED_ERR_BAD_ARG;
    if ((batch - 1) > (INT64_MAX - classes) / ld_logits || (batch - 1) > (INT64_MAX - classes) / ld_targets) return VITED_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(logits) % alignof(float) || reinterpret_cast<uintptr_t>(targets) % alignof(float) ||
        reinterpret_cast<uintptr_t>(meters) % alignof(double) || reinterpret_cast<uintptr_t>(last) % alignof(double) ||
        reinterpret_cast<uintptr_t>(bad) % alignof(int))
        return VITED_ERR_BAD_ARG;
    hipLaunchKernelGGL(cls_metrics_kernel, dim3(1), dim3(THREADS), 0, static_cast<hipStream_t>(stream), logits, ld_logits, targets,
                       ld_targets, (int)batch, (int)classes, meters, last, bad);
    return vited_check_launch();
}
