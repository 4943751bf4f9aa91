// C-ABI attention entry points: validation + dispatch (bf16 MFMA kernels when the shape is
// covered, otherwise the fp32 kernels: portable fp32-VALU, or the same chains on the f32-input matrix-core instruction).
#include "attention_kernels.h"
#include "pair_segsum.h"

static thread_local int g_last_attn_path = 0;
extern "C" int vited_last_attention_path(void) { return g_last_attn_path; }
void attention_set_last_path(int path) { g_last_attn_path = path; }

// Path 1 has two sets of kernels that compute the same bits: the vector-ALU ones (attention_portable.hip) and the matrix-core ones
// (attention_f32_mfma.hip).  Which of them the last path-1 call on this thread ran, and a process-wide switch that keeps every call
// on the vector-ALU ones (tests and the probe run both in one process).
static thread_local int g_last_fp32_attn_kernel = 0;
static int g_fp32_attn_select = 0;
extern "C" int vited_last_fp32_attention_kernel(void) { return g_last_fp32_attn_kernel; }
extern "C" int vited_fp32_attention_select(int mode) {
    if (mode != 0 && mode != 1) return VITED_ERR_BAD_ARG;
    return __atomic_exchange_n(&g_fp32_attn_select, mode, __ATOMIC_RELAXED);
}
extern "C" int vited_attention_f32_mfma_supported(int dtype, int64_t batch, int heads, int64_t nq, int64_t nk, int head_dim,
                                                  int backward) {
    return attention_f32_mfma_supported(dtype, batch, heads, nq, nk, head_dim, backward != 0) ? 1 : 0;
}
static inline bool fp32_attn_on_matrix_cores(const AttnArgs& a, int dtype, bool backward) {
    return __atomic_load_n(&g_fp32_attn_select, __ATOMIC_RELAXED) == 0 &&
           attention_f32_mfma_supported(dtype, a.batch, a.heads, a.nq, a.nk, a.head_dim, backward);
}

static int check_common(const AttnArgs& a, int dtype) {
    if (!a.q || !a.k || !a.v || !a.o || !a.lse) return VITED_ERR_BAD_ARG;
    if (a.batch <= 0 || a.heads <= 0 || a.nq <= 0 || a.nk <= 0 || a.head_dim <= 0) return VITED_ERR_BAD_ARG;
    if (dtype != VITED_F32 && dtype != VITED_BF16) return VITED_ERR_UNSUPPORTED;
    if (a.batch > 65535 || a.heads > 65535) return VITED_ERR_UNSUPPORTED;
    return VITED_OK;
}

extern "C" int vited_attention_fwd(const void* q, int64_t q_bs, int64_t q_ts, const void* k, int64_t k_bs, int64_t k_ts,
                                   const void* v, int64_t v_bs, int64_t v_ts, void* o, int64_t o_bs, int64_t o_ts,
                                   float* lse, int dtype, int64_t batch, int heads, int64_t nq, int64_t nk, int head_dim,
                                   float scale, void* stream) {
    return vited_attention_fwd_indexed(q, q_bs, q_ts, k, k_bs, k_ts, v, v_bs, v_ts, nullptr, o, o_bs, o_ts, lse, dtype, batch, heads, nq,
                                       nk, head_dim, scale, stream);
}

extern "C" int vited_attention_fwd_indexed(const void* q, int64_t q_bs, int64_t q_ts, const void* k, int64_t k_bs, int64_t k_ts,
                                           const void* v, int64_t v_bs, int64_t v_ts, const int64_t* kv_index, void* o, int64_t o_bs,
                                           int64_t o_ts, float* lse, int dtype, int64_t batch, int heads, int64_t nq, int64_t nk,
                                           int head_dim, float scale, void* stream) {
    AttnArgs a = {};
    a.q = q; a.k = k; a.v = v;
    a.kv_index = kv_index;
    a.q_bs = q_bs; a.q_ts = q_ts; a.k_bs = k_bs; a.k_ts = k_ts; a.v_bs = v_bs; a.v_ts = v_ts;
    a.o = o; a.o_bs = o_bs; a.o_ts = o_ts;
    a.lse = lse;
    a.batch = batch; a.heads = heads; a.nq = nq; a.nk = nk; a.head_dim = head_dim; a.scale = scale;
    int rc = check_common(a, dtype);
    if (rc != VITED_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VITED_BF16 && attention_mfma_supported(a, false)) {
        g_last_attn_path = 2;
        return attention_fwd_mfma(a, s);
    }
    g_last_attn_path = 1;
    if (fp32_attn_on_matrix_cores(a, dtype, false)) {
        g_last_fp32_attn_kernel = 2;
        return attention_fwd_f32_mfma(a, dtype, s);
    }
    g_last_fp32_attn_kernel = 1;
    return attention_fwd_portable(a, dtype, s);
}

static int bwd_dispatch(const AttnArgs& a, int dtype, hipStream_t s) {
    if (dtype == VITED_BF16 && attention_mfma_supported(a, true)) {
        g_last_attn_path = 2;
        return attention_bwd_mfma(a, s);
    }
    g_last_attn_path = 1;
    if (fp32_attn_on_matrix_cores(a, dtype, true)) {
        g_last_fp32_attn_kernel = 2;
        return attention_bwd_f32_mfma(a, dtype, s);
    }
    g_last_fp32_attn_kernel = 1;
    return attention_bwd_portable(a, dtype, s);
}

extern "C" int vited_attention_bwd(const void* q, int64_t q_bs, int64_t q_ts, const void* k, int64_t k_bs, int64_t k_ts,
                                   const void* v, int64_t v_bs, int64_t v_ts, const void* o, const void* d_o, int64_t o_bs,
                                   int64_t o_ts, const float* lse, float* delta, void* dq, int64_t dq_bs, int64_t dq_ts,
                                   void* dk, int64_t dk_bs, int64_t dk_ts, void* dv, int64_t dv_bs, int64_t dv_ts, int dtype,
                                   int64_t batch, int heads, int64_t nq, int64_t nk, int head_dim, float scale, void* stream) {
    AttnArgs a = {};
    a.q = q; a.k = k; a.v = v;
    a.q_bs = q_bs; a.q_ts = q_ts; a.k_bs = k_bs; a.k_ts = k_ts; a.v_bs = v_bs; a.v_ts = v_ts;
    a.o = o; a.d_o = d_o; a.o_bs = o_bs; a.o_ts = o_ts;
    a.lse = (float*)lse; a.delta = delta;
    a.dq = dq; a.dk = dk; a.dv = dv;
    a.dq_bs = dq_bs; a.dq_ts = dq_ts; a.dk_bs = dk_bs; a.dk_ts = dk_ts; a.dv_bs = dv_bs; a.dv_ts = dv_ts;
    a.batch = batch; a.heads = heads; a.nq = nq; a.nk = nk; a.head_dim = head_dim; a.scale = scale;
    int rc = check_common(a, dtype);
    if (rc != VITED_OK) return rc;
    if (!d_o || !delta || !dq || !dk || !dv) return VITED_ERR_BAD_ARG;
    return bwd_dispatch(a, dtype, (hipStream_t)stream);
}

static int64_t elem_bytes(int dtype) { return dtype == VITED_BF16 ? 2 : 4; }

extern "C" int64_t vited_attention_bwd_indexed_workspace_bytes(int dtype, int64_t batch, int heads, int64_t nk, int head_dim) {
    if ((dtype != VITED_F32 && dtype != VITED_BF16) || batch <= 0 || heads <= 0 || nk <= 0 || head_dim <= 0) return -1;
    return batch * nk * 2 * (int64_t)heads * head_dim * elem_bytes(dtype);
}

extern "C" int vited_attention_bwd_indexed(const void* q, int64_t q_bs, int64_t q_ts, const void* k, int64_t k_bs, int64_t k_ts,
                                           const void* v, int64_t v_bs, int64_t v_ts, const int64_t* kv_index,
                                           const int64_t* seg_order, const int64_t* seg_offsets, int64_t kv_items, const void* o,
                                           const void* d_o, int64_t o_bs, int64_t o_ts, const float* lse, float* delta, void* dq,
                                           int64_t dq_bs, int64_t dq_ts, void* dk, int64_t dk_bs, int64_t dk_ts, void* dv,
                                           int64_t dv_bs, int64_t dv_ts, int dtype, int64_t batch, int heads, int64_t nq, int64_t nk,
                                           int head_dim, float scale, void* workspace, int64_t workspace_bytes, void* stream) {
    AttnArgs a = {};
    a.q = q; a.k = k; a.v = v;
    a.kv_index = kv_index;
    a.q_bs = q_bs; a.q_ts = q_ts; a.k_bs = k_bs; a.k_ts = k_ts; a.v_bs = v_bs; a.v_ts = v_ts;
    a.o = o; a.d_o = d_o; a.o_bs = o_bs; a.o_ts = o_ts;
    a.lse = (float*)lse; a.delta = delta;
    a.dq = dq; a.dq_bs = dq_bs; a.dq_ts = dq_ts;
    a.batch = batch; a.heads = heads; a.nq = nq; a.nk = nk; a.head_dim = head_dim; a.scale = scale;
    int rc = check_common(a, dtype);
    if (rc != VITED_OK) return rc;
    if (!d_o || !delta || !dq || !dk || !dv || !kv_index || !seg_order || !seg_offsets || !workspace) return VITED_ERR_BAD_ARG;
    if (kv_items <= 0 || ((uintptr_t)workspace % 16) != 0) return VITED_ERR_BAD_ARG;
    if (kv_items > 65535) return VITED_ERR_UNSUPPORTED;
    if (workspace_bytes < vited_attention_bwd_indexed_workspace_bytes(dtype, batch, heads, nk, head_dim)) return VITED_ERR_WORKSPACE;
    // the kernels of vited_attention_bwd write pair b's dK / dV term into the workspace, packed [batch][nk][dK | dV] like a kv
    // projection, while they read k / v of item kv_index[b] ...
    const int64_t width = (int64_t)heads * head_dim;
    a.dk = workspace;
    a.dv = (char*)workspace + width * elem_bytes(dtype);
    a.dk_ts = a.dv_ts = 2 * width;
    a.dk_bs = a.dv_bs = nk * 2 * width;
    hipStream_t s = (hipStream_t)stream;
    rc = bwd_dispatch(a, dtype, s);
    if (rc != VITED_OK) return rc;
    // ... and the segmented sum adds the terms of every item's pairs in ascending pair order
    SegSumArgs g = {};
    g.ws = workspace;
    g.out[0] = dk; g.out_bs[0] = dk_bs; g.out_ts[0] = dk_ts;
    g.out[1] = dv; g.out_bs[1] = dv_bs; g.out_ts[1] = dv_ts;
    g.order = seg_order; g.offsets = seg_offsets;
    g.batch = batch; g.items = kv_items; g.nk = nk; g.width = (int)width;
    return attention_segsum(g, dtype, s);
}
