// The per-iteration learning-rate rules of lr_scheduler.py (the reference's misc/lr_scheduler.py over timm.scheduler; DESIGN.md
// section 28) in fp64, operation for operation in Python's order, as plain C++: the same text runs in the one-workgroup kernel of
// lr_schedule.hip and in the host program under the sanitizers (tools/lrsched_host_check.cpp).  Compile with -ffp-contract=off:
// Python multiplies and adds separately.
//
// A schedule is a table of LRS_TABLE_WORDS doubles (the integers among them are exact in a double):
//   [LRS_KIND]           LRS_COSINE / LRS_LINEAR / LRS_STEP / LRS_MULTISTEP
//   [LRS_WARMUP_T]       warm-up updates; t < warmup_t gives  warmup_lr_init + t * ((base - warmup_lr_init) / warmup_t)
//   [LRS_WARMUP_LR_INIT]
//   [LRS_T_INITIAL]      cosine: the cycle length; linear: the update at which lr_min_rate * base is reached
//   [LRS_LR_MIN] [LRS_CYCLE_LIMIT] [LRS_WARMUP_PREFIX]     cosine; the prefix flag also shifts t for step
//   [LRS_LR_MIN_RATE]    linear
//   [LRS_DECAY_T] [LRS_DECAY_RATE]                          step
//   [LRS_GAMMA] [LRS_MILESTONES] = count, then the ascending milestones themselves (at most LRS_MAX_MILESTONES)
// A period of zero (t_initial, decay_t, linear's t_initial - warmup_t), where Python would raise ZeroDivisionError, gives the base
// rate here: the callers refuse such a table before it reaches a device.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LRS_FN __host__ __device__ inline
#else
#define LRS_FN inline
#endif

#define LRS_COSINE 0
#define LRS_LINEAR 1
#define LRS_STEP 2
#define LRS_MULTISTEP 3

#define LRS_KIND 0
#define LRS_WARMUP_T 1
#define LRS_WARMUP_LR_INIT 2
#define LRS_T_INITIAL 3
#define LRS_LR_MIN 4
#define LRS_CYCLE_LIMIT 5
#define LRS_WARMUP_PREFIX 6
#define LRS_LR_MIN_RATE 7
#define LRS_DECAY_T 8
#define LRS_DECAY_RATE 9
#define LRS_GAMMA 10
#define LRS_MILESTONES 11
#define LRS_FIRST_MILESTONE 12
#define LRS_MAX_MILESTONES 32
#define LRS_TABLE_WORDS (LRS_FIRST_MILESTONE + LRS_MAX_MILESTONES)
#define LRS_MAX_GROUPS 4096             // parameter groups one launch steps

#define LRS_PI 3.141592653589793        // math.pi

// Python's t // d for d > 0 (C++ truncates, Python floors: they differ for t < 0)
LRS_FN int64_t lrs_floor_div(int64_t t, int64_t d) {
    const int64_t q = t / d;
    return (t % d != 0 && t < 0) ? q - 1 : q;
}

// bisect.bisect_right(milestones, t): the number of leading milestones <= t
LRS_FN int lrs_bisect_right(const double* milestones, int count, double t) {
    int lo = 0, hi = count;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (t < milestones[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// _get_lr(t) of one parameter group whose base rate is `base`, before the group's lr_scale
LRS_FN double lr_schedule_value(const double* table, double base, int64_t t) {
    const int kind = (int)table[LRS_KIND];
    const int64_t warmup_t = (int64_t)table[LRS_WARMUP_T];
    const double warmup_lr_init = table[LRS_WARMUP_LR_INIT];
    if (t < warmup_t) {
        const double warmup_step = (base - warmup_lr_init) / (double)warmup_t;        // warmup_t > t >= 0 here, or t < 0
        return warmup_lr_init + (double)t * warmup_step;
    }
    const bool prefix = table[LRS_WARMUP_PREFIX] != 0.0;
    if (kind == LRS_COSINE) {
        const int64_t t_initial = (int64_t)table[LRS_T_INITIAL];
        const double lr_min = table[LRS_LR_MIN];
        if (t_initial <= 0) return base;
        if (prefix) t -= warmup_t;
        const int64_t i = lrs_floor_div(t, t_initial);
        const int64_t t_curr = t - t_initial * i;
        if (i < (int64_t)table[LRS_CYCLE_LIMIT])                                       // cycle_decay = 1: base * 1.0 ** i is base
            return lr_min + 0.5 * (base - lr_min) * (1.0 + cos(LRS_PI * (double)t_curr / (double)t_initial));
        return lr_min;
    }
    if (kind == LRS_LINEAR) {
        const int64_t total = (int64_t)table[LRS_T_INITIAL] - warmup_t;
        if (total == 0) return base;
        t -= warmup_t;
        return base - (base - base * table[LRS_LR_MIN_RATE]) * ((double)t / (double)total);
    }
    if (kind == LRS_STEP) {
        const int64_t decay_t = (int64_t)table[LRS_DECAY_T];
        if (decay_t <= 0) return base;
        if (prefix) t -= warmup_t;
        return base * pow(table[LRS_DECAY_RATE], (double)lrs_floor_div(t, decay_t));
    }
    int count = (int)table[LRS_MILESTONES];
    if (count < 0) count = 0;
    if (count > LRS_MAX_MILESTONES) count = LRS_MAX_MILESTONES;
    return base * pow(table[LRS_GAMMA], (double)lrs_bisect_right(table + LRS_FIRST_MILESTONE, count, (double)t));
}
