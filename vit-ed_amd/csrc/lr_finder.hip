// The learning-rate range test recorded on the device (engine/lr_finder.py):
//   vited_lr_finder_step   row i of the history from *loss, the smoothed and the best loss, the halt decision, and the rate of iteration
//                          i + 1 into every group's rate word - 0.0f once halted, after which nothing but those words is written
// One launch of one workgroup, queued behind the training step whose loss it reads.  The loss, the state, the history and the sweep's
// ends all lie in device memory, so an eager launch and a replayed one see the same thing and the host never reads a loss or sets a
// rate.  The rule is lr_finder.h (shared with tools/lrfinder_host_check.cpp), in fp64; this file is compiled with -ffp-contract=off.
#include "common.h"
#include "lr_finder.h"

#define LRF_THREADS 64

__global__ void __launch_bounds__(LRF_THREADS)
lr_finder_step_kernel(const float* __restrict__ loss_ptr, int64_t* state, double* history, const double* __restrict__ start,
                      const double* __restrict__ end, int groups, int64_t num_iter, double smooth_f, double diverge_th, float* dst,
                      int64_t first, int64_t stride) {
    double* stats = reinterpret_cast<double*>(state + LRF_SMOOTHED);
    const int64_t i = state[LRF_ROWS];
    if (!lr_finder_live(i, state[LRF_STATE], num_iter)) {          // uniform: every lane read the same two words
        lr_finder_write_rates(threadIdx.x, LRF_THREADS, false, 0, num_iter, start, end, groups, dst, first, stride);
        return;
    }
    const double loss = (double)*loss_ptr;
    const LrfDecision d = lr_finder_decide(loss, i, stats[0], stats[1], num_iter, smooth_f, diverge_th);
    __syncthreads();       // every lane has read the state
    if (threadIdx.x == 0) lr_finder_commit(i, loss, d, state, stats, history, start[0], end[0], num_iter);
    lr_finder_write_rates(threadIdx.x, LRF_THREADS, d.state == LRF_RUNNING, i + 1, num_iter, start, end, groups, dst, first, stride);
}

extern "C" int vited_lr_finder_step(const float* loss, int64_t* state, double* history, int64_t capacity, const double* start,
                                    const double* end, int groups, int64_t num_iter, double smooth_f, double diverge_th, float* dst,
                                    int64_t dst_words, int64_t first, int64_t stride, void* stream) {
    if (!loss || !state || !history || !start || !end || !dst) return VITED_ERR_BAD_ARG;
    if (groups <= 0 || groups > LRF_MAX_GROUPS || dst_words <= 0 || first < 0 || stride < 1) return VITED_ERR_BAD_ARG;
    if (num_iter < 1 || num_iter > capacity) return VITED_ERR_BAD_ARG;                 // every row the sweep can write lies in history
    if (!(smooth_f >= 0.0 && smooth_f <= 1.0) || !(diverge_th > 1.0)) return VITED_ERR_BAD_ARG;      // a NaN fails both
    const int64_t room = dst_words - 1 - first;                                        // words of dst behind the first group's
    if (room < 0 || (groups > 1 && stride > room / (groups - 1))) return VITED_ERR_BAD_ARG;      // the last group's word lies inside dst
    if (((uintptr_t)state | (uintptr_t)history | (uintptr_t)start | (uintptr_t)end) % 8 || ((uintptr_t)loss | (uintptr_t)dst) % 4)
        return VITED_ERR_BAD_ARG;
    hipLaunchKernelGGL(lr_finder_step_kernel, dim3(1), dim3(LRF_THREADS), 0, (hipStream_t)stream, loss, state, history, start, end, groups,
                       num_iter, smooth_f, diverge_th, dst, first, stride);
    return vited_check_launch();
}
