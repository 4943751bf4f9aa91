// The per-iteration learning-rate schedule stepped on the device (lr_scheduler.py):
//   vited_lr_schedule_step   dst[first + stride g] = (float)(lr_schedule_value(table, base[g], t) * scale[g]),  t = *counter,  *counter = t + 1
// One launch of one workgroup, queued directly behind the optimizer update: update n runs with the rate the launch after update n - 1
// left, as the reference's loop does (misc/engine.py:228).  Everything the kernel reads lies in device memory, so a captured hipGraph
// follows a loaded schedule and a resumed counter.  The rules are lr_schedule.h (shared with tools/lrsched_host_check.cpp), in fp64;
// this file is compiled with -ffp-contract=off.
#include "common.h"
#include "lr_schedule.h"

#define LRS_THREADS 64

__global__ void __launch_bounds__(LRS_THREADS)
lr_schedule_step_kernel(const double* __restrict__ table, const double* __restrict__ base, const double* __restrict__ scale, int groups,
                        int64_t* counter, float* dst, int64_t first, int64_t stride, float* last_lr) {
    const int64_t t = *counter;
    for (int g = threadIdx.x; g < groups; g += LRS_THREADS) {
        const float lr = (float)(lr_schedule_value(table, base[g], t) * scale[g]);
        dst[first + stride * g] = lr;
        if (last_lr) last_lr[g] = lr;
    }
    __syncthreads();       // every lane has read the counter
    if (threadIdx.x == 0) *counter = t + 1;
}

extern "C" int vited_lr_schedule_step(const double* table, const double* base, const double* scale, int groups, int64_t* counter,
                                      float* dst, int64_t dst_words, int64_t first, int64_t stride, float* last_lr, void* stream) {
    if (!table || !base || !scale || !counter || !dst) return VITED_ERR_BAD_ARG;
    if (groups <= 0 || groups > LRS_MAX_GROUPS || dst_words <= 0 || first < 0 || stride < 1) return VITED_ERR_BAD_ARG;
    const int64_t room = dst_words - 1 - first;                                    // words of dst behind the first group's
    if (room < 0 || (groups > 1 && stride > room / (groups - 1))) return VITED_ERR_BAD_ARG;      // the last group's word lies inside dst
    if (((uintptr_t)table | (uintptr_t)base | (uintptr_t)scale | (uintptr_t)counter) % 8 || ((uintptr_t)dst | (uintptr_t)last_lr) % 4)
        return VITED_ERR_BAD_ARG;
    if (last_lr) {                                                                 // the mirror lies apart from the words written
        const uintptr_t d0 = (uintptr_t)(dst + first), d1 = (uintptr_t)(dst + first + stride * (groups - 1) + 1);
        const uintptr_t l0 = (uintptr_t)last_lr, l1 = (uintptr_t)(last_lr + groups);
        if (d0 < l1 && l0 < d1) return VITED_ERR_BAD_ARG;
    }
    hipLaunchKernelGGL(lr_schedule_step_kernel, dim3(1), dim3(LRS_THREADS), 0, (hipStream_t)stream, table, base, scale, groups, counter,
                       dst, first, stride, last_lr);
    return vited_check_launch();
}
