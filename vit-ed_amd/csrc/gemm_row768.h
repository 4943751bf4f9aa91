// Row-complete Linear + LayerNorm kernels for the 768-wide residual stream (gemm_row768.hip), as the extern "C" entries of
// gemm_row.hip reach them: the same arguments, argument checks and return codes as the 384-wide forms there.
#pragma once
#include <stdint.h>

#define ROW768_N 768

bool row768_shape_ok(int64_t M, int64_t N, int64_t K);      // what the kernels compute: the entries' shape check
bool row768_pays(int64_t M, int64_t K);                      // ... and where they beat the two-kernel form (measured)
int64_t row768_tiles(int64_t M);          // workgroups of a launch = rows of the [tiles][2][768] column partials

int row768_fwd(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, const float* residual, int64_t ldr,
               const float* row_scale, float* y, int64_t ldy, const float* gamma, const float* beta, float eps, void* h, int64_t ldh,
               float* mean, float* rstd, int64_t M, int64_t N, int64_t K, void* stream);

int row768_bwd(const void* dy, int64_t lddy, int64_t seg_k, int64_t seg_stride, const void* wt, int64_t ldwt, const float* x, int64_t ldx,
               const float* gamma, const float* mean, const float* rstd, const float* dx_in, int64_t dx_in_ld, float* dx_out,
               int64_t dx_out_ld, void* dx_lp, int64_t dx_lp_ld, const float* lp_scale, float* dgamma, float* dbeta, int accumulate,
               int64_t M, int64_t N, int64_t K, float* workspace, int64_t workspace_bytes, void* stream);
