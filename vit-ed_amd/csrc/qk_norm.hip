// q/k-norm: LayerNorm(head_dim, eps) of every head's query and key row before the attention scores are formed
// (models/vision_transformer.py:35-36,60 and :153-154,180 of the reference, `qk_norm=True`).  Streaming kernels, HBM is the roof.
//
// Mapping: a head row is head_dim = 32 or 64 elements, 64 - 256 bytes.  QKN_LANES = 8 lanes own one head row, each lane E = head_dim / 8
// consecutive elements (one 16-byte load at fp32 x 32 and bf16 x 64, one 8-byte load at bf16 x 32, two 16-byte loads at fp32 x 64),
// so a wave covers 8 head rows and, since the heads of a token row lie side by side, 512 - 2,048 contiguous bytes per load
// instruction.  The row sums are three DPP adds inside the 8-lane group (quad_perm xor 1, xor 2, row_half_mirror): no LDS and no
// ds_bpermute in the forward.  32 lanes per row (the LayerNorm kernels' mapping) would leave 24 of them without an element at
// head_dim 32; 16 lanes would halve the bytes per lane below a dword pair for bf16.
// q and k are the two "operands" of a launch, blockIdx.y picks one: each has its own pointer, row stride and row count (column
// slices of [M, 3D] / [M, 2D] / [M, D]; the cross-attention's q and k differ in rows).  A launch with one operand has gridDim.y 1.
//
// Backward: dy (= d q-hat / d k-hat as the attention backward left it) is overwritten by dx in place; xhat is recomputed from the
// saved pre-norm projection and the saved mean / rstd (never from the normalised values: gamma may be 0).  d gamma / d beta: a lane
// owns the same E columns of every head row it sees -> register partials -> one LDS combine per workgroup -> [blocks][2][head_dim]
// partial rows -> the LayerNorm kernels' fixed-order finishing pass (ln_bwd_finish: no atomics, so two runs give the same bits),
// which overwrites or adds onto the destinations.
#include "common.h"
#include "qk_norm.h"

int ln_bwd_finish(const float* partial, int nparts, int dim, float* dgamma, float* dbeta, int accumulate, hipStream_t s);   // layernorm.hip

#define QKN_THREADS 256
#define QKN_GROUPS (QKN_THREADS / QKN_LANES)      // head rows per workgroup and step: 32

struct QknFwdOp {
    const void* x; void* y; const float* gamma; const float* beta; float* mean; float* rstd;
    int64_t x_ld, y_ld, rows;
};
struct QknFwdArgs { QknFwdOp op[2]; };

struct QknBwdOp {
    void* dy; const void* x; const float* gamma; const float* mean; const float* rstd; float* partial;
    int64_t dy_ld, x_ld, rows;
};
struct QknBwdArgs { QknBwdOp op[2]; };

template <int N> __device__ __forceinline__ float qkn_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), N, 0xf, 0xf, true));
}
// sum over the 8 lanes of a head row's group; every lane gets it.  quad_perm [1,0,3,2], quad_perm [2,3,0,1], then row_half_mirror
// (lane i of 8 reads lane 7 - i, which sits in the other quad, and after the first two steps a quad's lanes all hold its sum)
__device__ __forceinline__ float group_sum(float v) {
    v += qkn_dpp<0xB1>(v);
    v += qkn_dpp<0x4E>(v);
    v += qkn_dpp<0x141>(v);
    return v;
}

template <typename T, int E> struct QknRow;
template <int E> struct QknRow<float, E> {
    static __device__ __forceinline__ void load(const float* p, float* v) {
#pragma unroll
        for (int e = 0; e < E; e += 4) {
            const f32x4 t = *(const f32x4*)(p + e);
            v[e] = t[0]; v[e + 1] = t[1]; v[e + 2] = t[2]; v[e + 3] = t[3];
        }
    }
    static __device__ __forceinline__ void store(float* p, const float* v) {
#pragma unroll
        for (int e = 0; e < E; e += 4) *(f32x4*)(p + e) = f32x4{v[e], v[e + 1], v[e + 2], v[e + 3]};
    }
};
template <> struct QknRow<bf16, 4> {
    static __device__ __forceinline__ void load(const bf16* p, float* v) {
        const bf16x4 t = *(const bf16x4*)p;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)t[e];
    }
    static __device__ __forceinline__ void store(bf16* p, const float* v) {
        *(bf16x4*)p = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
    }
};
template <> struct QknRow<bf16, 8> {
    static __device__ __forceinline__ void load(const bf16* p, float* v) {
        const bf16x8 t = *(const bf16x8*)p;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
    }
    static __device__ __forceinline__ void store(bf16* p, const float* v) {
        *(bf16x8*)p = bf16x8{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3], (bf16)v[4], (bf16)v[5], (bf16)v[6], (bf16)v[7]};
    }
};

// head row hr of an operand: token row hr / heads, head hr % heads; this lane's E elements start at column head * HD + lane * E
template <typename T, int E>
__global__ void __launch_bounds__(QKN_THREADS)
qk_norm_fwd_kernel(const QknFwdArgs a, int heads, float eps) {
    constexpr int HD = E * QKN_LANES;
    const QknFwdOp op = a.op[blockIdx.y];
    const int lane = threadIdx.x & (QKN_LANES - 1);
    const int64_t group = ((int64_t)blockIdx.x * QKN_THREADS + threadIdx.x) / QKN_LANES;
    const int64_t ngroups = (int64_t)gridDim.x * QKN_GROUPS;
    const int64_t n = op.rows * heads;
    float gm[E], bt[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        gm[e] = op.gamma[lane * E + e];
        bt[e] = op.beta[lane * E + e];
    }
    const float inv_d = 1.f / HD;
    for (int64_t hr = group; hr < n; hr += ngroups) {
        const int64_t row = hr / heads;
        const int col = (int)(hr - row * heads) * HD + lane * E;
        float v[E], y[E];
        QknRow<T, E>::load((const T*)op.x + row * op.x_ld + col, v);
        const float mu = group_sum(qkn_sum_part<E>(v)) * inv_d;
        const float rs = qkn_rstd(group_sum(qkn_sq_part<E>(v, mu)), inv_d, eps);
        qkn_fwd_out<E>(v, mu, rs, gm, bt, y);
        QknRow<T, E>::store((T*)op.y + row * op.y_ld + col, y);
        if (lane == 0) {
            op.mean[hr] = mu;
            op.rstd[hr] = rs;
        }
    }
}

template <typename T, int E>
__global__ void __launch_bounds__(QKN_THREADS)
qk_norm_bwd_kernel(const QknBwdArgs a, int heads) {
    constexpr int HD = E * QKN_LANES;
    __shared__ __attribute__((aligned(16))) float lds[QKN_GROUPS][2][HD];
    const QknBwdOp op = a.op[blockIdx.y];
    const int lane = threadIdx.x & (QKN_LANES - 1);
    const int gid = threadIdx.x / QKN_LANES;
    const int64_t group = (int64_t)blockIdx.x * QKN_GROUPS + gid;
    const int64_t ngroups = (int64_t)gridDim.x * QKN_GROUPS;
    const int64_t n = op.rows * heads;
    float gm[E], dg[E], db[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        gm[e] = op.gamma[lane * E + e];
        dg[e] = 0.f;
        db[e] = 0.f;
    }
    const float inv_d = 1.f / HD;
    for (int64_t hr = group; hr < n; hr += ngroups) {
        const int64_t row = hr / heads;
        const int col = (int)(hr - row * heads) * HD + lane * E;
        const float mu = op.mean[hr], rs = op.rstd[hr];
        T* dyp = (T*)op.dy + row * op.dy_ld + col;
        float d[E], x[E], xh[E], g[E], dx[E], s1, s2;
        QknRow<T, E>::load(dyp, d);
        QknRow<T, E>::load((const T*)op.x + row * op.x_ld + col, x);
        qkn_bwd_parts<E>(d, x, mu, rs, gm, xh, g, s1, s2, dg, db);
        const float c1 = group_sum(s1) * inv_d, c2 = group_sum(s2) * inv_d;
        qkn_bwd_out<E>(g, xh, c1, c2, rs, dx);
        QknRow<T, E>::store(dyp, dx);
    }
    // the 32 groups' column partials through LDS, summed in group order: one [2][HD] partial row per workgroup
#pragma unroll
    for (int e = 0; e < E; ++e) {
        lds[gid][0][lane * E + e] = dg[e];
        lds[gid][1][lane * E + e] = db[e];
    }
    __syncthreads();
    if (threadIdx.x < 2 * HD) {
        const int which = threadIdx.x / HD, c = threadIdx.x % HD;
        float acc = 0.f;
#pragma unroll
        for (int w = 0; w < QKN_GROUPS; ++w) acc += lds[w][which][c];
        op.partial[(size_t)blockIdx.x * 2 * HD + threadIdx.x] = acc;
    }
}

static inline int64_t qkn_blocks(int64_t head_rows, int64_t per_group, int64_t cap) {
    int64_t b = ceil_div64(head_rows, QKN_GROUPS * per_group);
    if (b > cap) b = cap;
    return b < 1 ? 1 : b;
}
// backward: >= 4 head rows per group, at most 1,024 partial rows per operand (4 workgroups per CU)
static inline int64_t qkn_bwd_blocks(int64_t q_rows, int64_t k_rows, int64_t heads) {
    const int64_t rows = q_rows > k_rows ? q_rows : k_rows;
    return qkn_blocks(rows * heads, 4, 1024);
}

// vector width of one lane's piece in bytes (what the pointers and row strides must be multiples of)
static inline int qkn_vec_bytes(int dtype, int64_t head_dim) {
    const int bytes = (int)(head_dim / QKN_LANES) * (dtype == VITED_BF16 ? 2 : 4);
    return bytes > 16 ? 16 : bytes;
}
static inline bool qkn_aligned(const void* p, int64_t ld, int dtype, int vec) {
    const int64_t elem = dtype == VITED_BF16 ? 2 : 4;
    return ((uintptr_t)p % vec) == 0 && (ld * elem) % vec == 0;
}

extern "C" int vited_qk_norm_fwd(const void* q, int64_t q_ld, int64_t q_rows, const void* k, int64_t k_ld, int64_t k_rows,
                                 const float* gamma_q, const float* beta_q, const float* gamma_k, const float* beta_k, void* q_out,
                                 int64_t q_out_ld, void* k_out, int64_t k_out_ld, float* q_mean, float* q_rstd, float* k_mean,
                                 float* k_rstd, int dtype, int64_t heads, int64_t head_dim, float eps, void* stream) {
    if (!q && !k) return VITED_ERR_BAD_ARG;
    if (heads <= 0 || head_dim <= 0) return VITED_ERR_BAD_ARG;
    if (head_dim != 32 && head_dim != 64) return VITED_ERR_UNSUPPORTED;
    if (dtype != VITED_BF16 && dtype != VITED_F32) return VITED_ERR_UNSUPPORTED;
    const int64_t width = heads * head_dim;
    const int vec = qkn_vec_bytes(dtype, head_dim);
    if (q && (!gamma_q || !beta_q || !q_out || !q_mean || !q_rstd || q_rows <= 0 || q_ld < width || q_out_ld < width)) return VITED_ERR_BAD_ARG;
    if (k && (!gamma_k || !beta_k || !k_out || !k_mean || !k_rstd || k_rows <= 0 || k_ld < width || k_out_ld < width)) return VITED_ERR_BAD_ARG;
    if (q && !(qkn_aligned(q, q_ld, dtype, vec) && qkn_aligned(q_out, q_out_ld, dtype, vec))) return VITED_ERR_BAD_ARG;
    if (k && !(qkn_aligned(k, k_ld, dtype, vec) && qkn_aligned(k_out, k_out_ld, dtype, vec))) return VITED_ERR_BAD_ARG;
    QknFwdArgs a = {};
    int count = 0;
    int64_t most = 0;
    if (q) {
        a.op[count++] = QknFwdOp{q, q_out, gamma_q, beta_q, q_mean, q_rstd, q_ld, q_out_ld, q_rows};
        most = q_rows;
    }
    if (k) {
        a.op[count++] = QknFwdOp{k, k_out, gamma_k, beta_k, k_mean, k_rstd, k_ld, k_out_ld, k_rows};
        if (k_rows > most) most = k_rows;
    }
    const dim3 grid((unsigned)qkn_blocks(most * heads, 2, 2048), (unsigned)count);
    hipStream_t s = (hipStream_t)stream;
#define L(T, E) hipLaunchKernelGGL((qk_norm_fwd_kernel<T, E>), grid, dim3(QKN_THREADS), 0, s, a, (int)heads, eps)
    if (dtype == VITED_BF16) {
        if (head_dim == 32) L(bf16, 4); else L(bf16, 8);
    } else {
        if (head_dim == 32) L(float, 4); else L(float, 8);
    }
#undef L
    return vited_check_launch();
}

extern "C" int64_t vited_qk_norm_bwd_workspace_bytes(int64_t q_rows, int64_t k_rows, int64_t heads, int64_t head_dim) {
    if (q_rows < 0 || k_rows < 0 || heads <= 0 || head_dim <= 0) return 0;
    return 2 * qkn_bwd_blocks(q_rows, k_rows, heads) * 2 * head_dim * (int64_t)sizeof(float);
}

extern "C" int vited_qk_norm_bwd(void* dq, int64_t dq_ld, const void* q, int64_t q_ld, const float* q_mean, const float* q_rstd,
                                 const float* gamma_q, float* dgamma_q, float* dbeta_q, int64_t q_rows, void* dk, int64_t dk_ld,
                                 const void* k, int64_t k_ld, const float* k_mean, const float* k_rstd, const float* gamma_k,
                                 float* dgamma_k, float* dbeta_k, int64_t k_rows, int dtype, int accumulate, int64_t heads,
                                 int64_t head_dim, float* workspace, int64_t workspace_bytes, void* stream) {
    if (!dq && !dk) return VITED_ERR_BAD_ARG;
    if (heads <= 0 || head_dim <= 0) return VITED_ERR_BAD_ARG;
    if (head_dim != 32 && head_dim != 64) return VITED_ERR_UNSUPPORTED;
    if (dtype != VITED_BF16 && dtype != VITED_F32) return VITED_ERR_UNSUPPORTED;
    const int64_t width = heads * head_dim;
    const int vec = qkn_vec_bytes(dtype, head_dim);
    if (dq && (!q || !q_mean || !q_rstd || !gamma_q || !dgamma_q || !dbeta_q || q_rows <= 0 || dq_ld < width || q_ld < width)) return VITED_ERR_BAD_ARG;
    if (dk && (!k || !k_mean || !k_rstd || !gamma_k || !dgamma_k || !dbeta_k || k_rows <= 0 || dk_ld < width || k_ld < width)) return VITED_ERR_BAD_ARG;
    if (dq && !(qkn_aligned(dq, dq_ld, dtype, vec) && qkn_aligned(q, q_ld, dtype, vec))) return VITED_ERR_BAD_ARG;
    if (dk && !(qkn_aligned(dk, dk_ld, dtype, vec) && qkn_aligned(k, k_ld, dtype, vec))) return VITED_ERR_BAD_ARG;
    if (!dq) q_rows = 0;
    if (!dk) k_rows = 0;
    if (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < vited_qk_norm_bwd_workspace_bytes(q_rows, k_rows, heads, head_dim))
        return VITED_ERR_WORKSPACE;
    const int64_t blocks = qkn_bwd_blocks(q_rows, k_rows, heads);
    float* part_q = workspace;
    float* part_k = workspace + blocks * 2 * head_dim;
    QknBwdArgs a = {};
    int count = 0;
    if (dq) a.op[count++] = QknBwdOp{dq, q, gamma_q, q_mean, q_rstd, part_q, dq_ld, q_ld, q_rows};
    if (dk) a.op[count++] = QknBwdOp{dk, k, gamma_k, k_mean, k_rstd, part_k, dk_ld, k_ld, k_rows};
    const dim3 grid((unsigned)blocks, (unsigned)count);
    hipStream_t s = (hipStream_t)stream;
#define L(T, E) hipLaunchKernelGGL((qk_norm_bwd_kernel<T, E>), grid, dim3(QKN_THREADS), 0, s, a, (int)heads)
    if (dtype == VITED_BF16) {
        if (head_dim == 32) L(bf16, 4); else L(bf16, 8);
    } else {
        if (head_dim == 32) L(float, 4); else L(float, 8);
    }
#undef L
    int rc = vited_check_launch();
    if (rc != VITED_OK) return rc;
    if (dq) rc = ln_bwd_finish(part_q, (int)blocks, (int)head_dim, dgamma_q, dbeta_q, accumulate, s);
    if (rc != VITED_OK) return rc;
    if (dk) rc = ln_bwd_finish(part_k, (int)blocks, (int)head_dim, dgamma_k, dbeta_k, accumulate, s);
    return rc;
}
