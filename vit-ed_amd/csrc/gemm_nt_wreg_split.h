// Work split of gemm_nt_wreg_kernel (gemm_nt_wreg.hip): which column group and which run of 16-row units a workgroup takes.
// Plain C++, so that the same text runs inside the kernel and in a host program (tools/wreg_split_host_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define WREG_FN __host__ __device__ __forceinline__
#else
#define WREG_FN inline
#endif

#define WREG_UNIT_ROWS 16

struct WregShare {
    int group;            // column group: rows [group * 384, group * 384 + 384) of W
    int unit_begin;       // 16-row units [unit_begin, unit_end) of that group; empty when the group has fewer units than workgroups
    int unit_end;
};

WREG_FN int64_t wreg_units(int64_t M) { return (M + WREG_UNIT_ROWS - 1) / WREG_UNIT_ROWS; }

// Workgroups per group: the wanted count divided over the groups as evenly as it allows (256 over 1 / 2 / 16 groups, 85 each of
// 255 over 3), at least one.  The launch has wreg_per_group * groups workgroups.
WREG_FN int wreg_per_group(int workgroups, int groups) {
    const int per = workgroups / groups;
    return per < 1 ? 1 : per;
}

// Workgroup wg of the launch.  The workgroups of one group are neighbours (wg / per), so that workgroups wg, wg + per, ... - the
// same rows of every group - are congruent modulo 8 whenever per is a multiple of 8 and meet in one XCD's L2.  Inside a group the
// units are dealt in contiguous shares that differ by at most one unit: with 16-row units the longest share of 66,560 rows over
// 256 workgroups is 17 units against a mean of 16.25 (4.6 % over; 32-row units: 9 against 8.125, 10.7 % over).
WREG_FN WregShare wreg_share(int wg, int per, int64_t units) {
    WregShare s;
    s.group = wg / per;
    const int64_t i = wg - s.group * per;
    s.unit_begin = (int)(i * units / per);
    s.unit_end = (int)((i + 1) * units / per);
    return s;
}
