// The index arithmetic of patch dropout (patch_keep.hip; timm PatchDropout as the reference constructs it),
// written so that the device kernels and a host program under the sanitizers (tools/patchkeep_host_check.cpp) compile the same text.
//
// A keep table is int32 [B, K]: the indices timm's argsort kept, relative to the tokens BEHIND the prefix slot, in keep order.
//   x2 form (lead = 0): the prefix is the cls token; the kept patch rows of sample b are  patch(b, r) = keep[b, r],      r < K.
//   x1 form (lead = 1): there is no cls token, so the prefix slot falls on patch 0, which is always kept and leads:
//                       patch(b, 0) = 0,  patch(b, r) = 1 + keep[b, r - 1],  r < 1 + K.
// Indices are device data: whatever a table holds, pk_patch clamps into [0, n_patches), so no kernel reads or writes outside its
// operands because of one.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PK_FN __host__ __device__ __forceinline__
#else
#define PK_FN inline
#endif

#define PK_MAX_KEYS 4096        // keys of one row held in LDS by the ranking kernel

// kept patch rows per sample
PK_FN int pk_rows(int K, int lead) { return K + (lead ? 1 : 0); }

// the patch behind kept row r (r < pk_rows) of a sample whose keep row is `keep`
PK_FN int pk_patch(const int* keep, int lead, int r, int n_patches) {
    if (lead && r == 0) return 0;
    int p = keep[r - (lead ? 1 : 0)] + (lead ? 1 : 0);
    p = p < 0 ? 0 : p;
    return p < n_patches ? p : n_patches - 1;
}

// The order of the ranking: ascending keys, NaN after every number (torch.sort's order), equal keys (and -0 == +0) by index.
PK_FN bool pk_before(float a, int ia, float b, int ib) {
    const bool a_nan = a != a, b_nan = b != b;
    if (a_nan || b_nan) return a_nan == b_nan ? ia < ib : b_nan;
    return a < b || (a == b && ia < ib);
}

// rank of key i among the L keys of a row: how many come before it.  Distinct for distinct i, so the ranks are a permutation.
PK_FN int pk_rank(const float* keys, int L, int i) {
    const float k = keys[i];
    int rank = 0;
    for (int j = 0; j < L; ++j) rank += pk_before(keys[j], j, k, i) ? 1 : 0;
    return rank;
}

// inverse table of one sample: inv[p] = the kept row of patch p, or -1.  `inv` holds n_patches entries.
PK_FN void pk_inverse_clear(int* inv, int n_patches, int first, int step) {
    for (int p = first; p < n_patches; p += step) inv[p] = -1;
}
PK_FN void pk_inverse_fill(int* inv, const int* keep, int K, int lead, int n_patches, int first, int step) {
    for (int r = first; r < pk_rows(K, lead); r += step) inv[pk_patch(keep, lead, r, n_patches)] = r;
}
