// Host build of the work split of gemm_nt_wreg_kernel (csrc/gemm_nt_wreg_split.h): the very text the HIP kernel runs, driven over a
// list of (rows, groups, wanted workgroups).  Every (group, 16-row unit) must be covered exactly once, every workgroup's share must
// be one contiguous run inside one group, the shares of a group must differ by at most one unit, and at 66,560 rows and one group
// the longest share must stay within 5 % of the mean.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vit-ed_amd/csrc tools/wreg_split_host_check.cpp -o wreg_split_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gemm_nt_wreg_split.h"

static int run_case(int64_t M, int groups, int workgroups) {
    const int64_t units = wreg_units(M);
    const int per = wreg_per_group(workgroups, groups);
    const int grid = per * groups;
    int bad = 0;
    if (per < 1 || (workgroups >= groups && (grid > workgroups || grid + groups <= workgroups))) ++bad;   // as evenly as the count allows
    if (units * WREG_UNIT_ROWS < M || (units - 1) * WREG_UNIT_ROWS >= M) ++bad;
    // exactly-sized table: a unit or group outside its range is an ASan report
    std::vector<unsigned char> seen((size_t)(groups * units), 0);
    int64_t longest = 0, shortest = units;
    for (int wg = 0; wg < grid; ++wg) {
        const WregShare s = wreg_share(wg, per, units);
        if (s.group < 0 || s.group >= groups || s.unit_begin < 0 || s.unit_end < s.unit_begin || s.unit_end > units) {
            ++bad;
            continue;
        }
        if (wg % per != 0) {             // contiguous with the share in front of it inside the group
            const WregShare prev = wreg_share(wg - 1, per, units);
            if (prev.group != s.group || prev.unit_end != s.unit_begin) ++bad;
        } else if (s.unit_begin != 0) {
            ++bad;
        }
        if (wg % per == per - 1 && s.unit_end != units) ++bad;
        for (int u = s.unit_begin; u < s.unit_end; ++u) ++seen.at((size_t)(s.group * units + u));
        const int64_t len = s.unit_end - s.unit_begin;
        longest = len > longest ? len : longest;
        shortest = len < shortest ? len : shortest;
    }
    for (unsigned char c : seen)
        if (c != 1) ++bad;
    if (longest - shortest > 1) ++bad;
    const double mean = (double)units / per;
    if (M == 66560 && groups == 1 && workgroups >= 255 && (double)longest > 1.05 * mean) ++bad;
    printf("M %7lld groups %2d workgroups %3d: grid %3d, shares %lld..%lld units (mean %.3f): %s\n", (long long)M, groups, workgroups, grid,
           (long long)shortest, (long long)longest, mean, bad ? "BAD" : "ok");
    return bad;
}

int main() {
    int bad = 0, cases = 0;
    const int64_t big[] = {65536, 66560, 73800, 24576};
    const int group_counts[] = {1, 2, 3, 16};
    const int slots[] = {255, 256};
    for (int64_t M : big)
        for (int g : group_counts)
            for (int w : slots) {
                bad += run_case(M, g, w);
                ++cases;
            }
    const int64_t small[] = {1, 15, 16, 17, 4096, 4113, 8247};
    for (int64_t M : small)
        for (int g : group_counts) {
            if (g == 16 && M > 4113) continue;
            bad += run_case(M, g, 256);
            ++cases;
        }
    const int few[] = {1, 3, 8};
    for (int w : few)
        for (int g : group_counts) {
            bad += run_case(2003, g, w);
            ++cases;
        }
    bad += run_case(((int64_t)1 << 31) - 1, 1, 256);      // the largest M the kernel takes: 32-bit unit numbers
    ++cases;
    if (bad) printf("wreg_split_host_check FAILED\n");
    else printf("wreg_split_host_check ok: %d cases\n", cases);
    return bad ? 1 : 0;
}
