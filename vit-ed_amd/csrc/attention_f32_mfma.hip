// fp32 attention on the matrix cores: the three kernels of attention_portable.hip on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate).
// The instruction is bit for bit a k-ordered fmaf chain (D = fma(a_k1, b_k1, fma(a_k0, b_k0, C))), and every product of the portable
// kernels is such a chain, so these kernels give the portable kernels' bits:
//   * the score tile is computed TRANSPOSED, rows = the 32 keys (queries, in dK / dV) of an LDS tile, columns = the 32 queries (keys)
//     a wave owns: a lane holds 16 scores of ITS column, so max, alpha, p and ds are per-lane arithmetic plus one exchange between
//     the lane halves (v_permlane32_swap);
//   * operand row i of the first product carries tile row 2r + h, where (r, h) are the accumulator register and lane half row i lands
//     in: register t of the probability tile is then the B operand of instruction t of the second product (tile rows 2t, 2t + 1, in
//     this order), with no LDS round trip;
//   * forward: the even-d and odd-d chains of the portable kernel are two accumulators fed (4t, 4t + 2) and (4t + 1, 4t + 3); the
//     padded keys of the last tile are +0 rows whose (+0)(+0) products are part of the chain, as in the portable kernel;
//   * backward: one accumulator fed (2t, 2t + 1); the portable loops stop at the last key / query, so a padded tile row is staged as
//     -0.f and its p / ds are +0: a product of -0 leaves every accumulator as it is, -0 included.  Instructions whose two slots are
//     both padding are skipped.
// 256 threads = 4 waves x 32 columns, the portable kernels' 128 rows a workgroup; K / V (Q / dO, lse, delta) tiles of 32 rows are
// shared through two LDS buffers: the next tile's global loads are issued before the current tile's MFMAs and written to the other
// buffer after them, one barrier a tile.  A wave whose 32 columns are all out of range only helps staging.
#include "attention_kernels.h"

#define AF_THREADS 256
#define AF_ROWS 128   // rows (queries, or keys in dK / dV) per workgroup
#define AF_KT 32      // tile rows, the portable kernels' AP_KT
#define AF_LD(HD) ((HD) + 1)   // floats per LDS row: odd, so that both "lanes = rows" and "lanes = columns" reads spread over the banks

// tile row carried by operand row i of the first product: accumulator register r of lane half h holds row (r & 3) + 8 (r >> 2) + 4 h
__device__ __forceinline__ int af_tile_row(int i) { return 2 * ((i & 3) + 4 * (i >> 3)) + ((i >> 2) & 1); }

// x of the lower (lanes 0..31) and of the upper half's lane with the same column, in both of them
__device__ __forceinline__ void af_halves(float x, float& lo, float& hi) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    lo = __builtin_bit_cast(float, (unsigned)r[0]);
    hi = __builtin_bit_cast(float, (unsigned)r[1]);
}

template <typename T> __device__ __forceinline__ f32x4 af_load4(const T* p);
template <> __device__ __forceinline__ f32x4 af_load4<float>(const float* p) { return *(const f32x4*)p; }
template <> __device__ __forceinline__ f32x4 af_load4<bf16>(const bf16* p) {
    const bf16x4 v = *(const bf16x4*)p;
    return f32x4{to_f32(v[0]), to_f32(v[1]), to_f32(v[2]), to_f32(v[3])};
}
// whether 4 consecutive elements at every (row * ts + 4 c) may be moved as one vector
template <typename T> __device__ __forceinline__ bool af_vec_ok(const T* p, int64_t ts) {
    return (ts & 3) == 0 && ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0;
}
template <typename T> __device__ __forceinline__ void af_store4(T* p, bool vec, float x0, float x1, float x2, float x3);
template <> __device__ __forceinline__ void af_store4<float>(float* p, bool vec, float x0, float x1, float x2, float x3) {
    if (vec) *(f32x4*)p = f32x4{x0, x1, x2, x3};
    else { p[0] = x0; p[1] = x1; p[2] = x2; p[3] = x3; }
}
template <> __device__ __forceinline__ void af_store4<bf16>(bf16* p, bool vec, float x0, float x1, float x2, float x3) {
    if (vec) *(bf16x4*)p = bf16x4{from_f32<bf16>(x0), from_f32<bf16>(x1), from_f32<bf16>(x2), from_f32<bf16>(x3)};
    else { p[0] = from_f32<bf16>(x0); p[1] = from_f32<bf16>(x1); p[2] = from_f32<bf16>(x2); p[3] = from_f32<bf16>(x3); }
}

// elements d .. d + 3 of one row of a head slice, times mul (the portable load_row); zeros for a row that is out of range
template <typename T>
__device__ __forceinline__ f32x4 af_row4(const T* p, int d, bool vec, bool live, float mul) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        if (vec) v = af_load4<T>(p + d);
        else v = f32x4{to_f32(p[d]), to_f32(p[d + 1]), to_f32(p[d + 2]), to_f32(p[d + 3])};
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] * mul;
    }
    return v;
}
// a row as the B operand of the backward score products: slot h of instruction t is d = 2t + h
template <typename T, int HD>
__device__ __forceinline__ void af_row_pairs(const T* p, bool vec, bool live, float mul, int h, float (&r)[HD / 2]) {
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
        const f32x4 v = af_row4<T>(p, d, vec, live, mul);
        r[d / 2] = h ? v[1] : v[0];
        r[d / 2 + 1] = h ? v[3] : v[2];
    }
}

// rows [j0, j0 + 32) of a strided [n, HD] head slice -> registers (4 consecutive d a thread, HD / 32 times), pad past n
template <typename T, int HD>
__device__ __forceinline__ void af_fetch(f32x4 (&r)[HD / 32], const T* base, int64_t ts, bool vec, int64_t j0, int64_t n, float pad,
                                         int tid) {
#pragma unroll
    for (int p = 0; p < HD / 32; ++p) {
        const int e = tid + p * AF_THREADS;
        const int jj = e / (HD / 4), d = (e % (HD / 4)) * 4;
        const int64_t j = j0 + jj;
        if (j >= n) r[p] = f32x4{pad, pad, pad, pad};
        else if (vec) r[p] = af_load4<T>(base + j * ts + d);
        else {
#pragma unroll
            for (int c = 0; c < 4; ++c) r[p][c] = to_f32(base[j * ts + d + c]);
        }
    }
}
template <int HD>
__device__ __forceinline__ void af_put(float (*S)[AF_LD(HD)], const f32x4 (&r)[HD / 32], int tid) {
#pragma unroll
    for (int p = 0; p < HD / 32; ++p) {
        const int e = tid + p * AF_THREADS;
        const int jj = e / (HD / 4), d = (e % (HD / 4)) * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) S[jj][d + c] = r[p][c];
    }
}

#define AF_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// ------------------------------------------------------------------------------------------------
// forward: S^T = K Q~^T (rows keys, columns queries), O^T += V^T P^T
// ------------------------------------------------------------------------------------------------
template <typename T, int HD>
__global__ void __launch_bounds__(AF_THREADS)
attn_fwd_f32_mfma_kernel(AttnArgs a) {
    constexpr int NB = HD / 32;
    __shared__ float Ks[2][AF_KT][AF_LD(HD)];
    __shared__ float Vs[2][AF_KT][AF_LD(HD)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, c = lane & 31;
    const int64_t b = blockIdx.z;
    const int hd = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * AF_ROWS + wave * 32;
    const int64_t i = i0 + c;
    const bool live = i < a.nq, wave_live = i0 < a.nq;
    const int64_t bkv = a.kv_index ? a.kv_index[b] : b;
    const T* kb = (const T*)a.k + bkv * a.k_bs + (int64_t)hd * HD;
    const T* vb = (const T*)a.v + bkv * a.v_bs + (int64_t)hd * HD;
    const bool vk = af_vec_ok(kb, a.k_ts), vv = af_vec_ok(vb, a.v_ts);
    // this lane's share of its query: slot h of the instructions of the even-d chain (4t + 2h) and of the odd-d chain (4t + 1 + 2h)
    float qe[HD / 4], qo[HD / 4];
    {
        const T* qp = (const T*)a.q + b * a.q_bs + i * a.q_ts + (int64_t)hd * HD;
        const bool vq = af_vec_ok(qp - i * a.q_ts, a.q_ts);
#pragma unroll
        for (int t = 0; t < HD / 4; ++t) {
            const f32x4 v = af_row4<T>(qp, 4 * t, vq, live, a.scale);
            qe[t] = h ? v[2] : v[0];
            qo[t] = h ? v[3] : v[1];
        }
    }
    f32x16 acc[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int krow = af_tile_row(c);
    f32x4 rk[NB], rv[NB];
    af_fetch<T, HD>(rk, kb, a.k_ts, vk, 0, a.nk, 0.f, tid);
    af_fetch<T, HD>(rv, vb, a.v_ts, vv, 0, a.nk, 0.f, tid);
    af_put<HD>(Ks[0], rk, tid);
    af_put<HD>(Vs[0], rv, tid);
    __syncthreads();
    int buf = 0;
    for (int64_t j0 = 0; j0 < a.nk; j0 += AF_KT) {
        const bool more = j0 + AF_KT < a.nk;
        if (more) {
            af_fetch<T, HD>(rk, kb, a.k_ts, vk, j0 + AF_KT, a.nk, 0.f, tid);
            af_fetch<T, HD>(rv, vb, a.v_ts, vv, j0 + AF_KT, a.nk, 0.f, tid);
        }
        if (wave_live) {
            const int cnt = (int)((a.nk - j0) < AF_KT ? (a.nk - j0) : AF_KT);
            f32x16 se, so;
#pragma unroll
            for (int r = 0; r < 16; ++r) { se[r] = 0.f; so[r] = 0.f; }
#pragma unroll
            for (int t = 0; t < HD / 4; ++t) {
                se = AF_MFMA(Ks[buf][krow][4 * t + 2 * h], qe[t], se);
                so = AF_MFMA(Ks[buf][krow][4 * t + 1 + 2 * h], qo[t], so);
            }
            float s[16];
            float tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {   // register r of half h is key 2r + h of the tile
                s[r] = 2 * r + h < cnt ? se[r] + so[r] : -INFINITY;
                tmax = fmaxf(tmax, s[r]);
            }
            float lo, hi;
            af_halves(tmax, lo, hi);
            tmax = fmaxf(lo, hi);
            const float mn = fmaxf(m, tmax);
            const float alpha = __expf(m - mn);  // m = -inf on the first tile -> 0
            l *= alpha;
#pragma unroll
            for (int n = 0; n < NB; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[n][r] *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = __expf(s[r] - mn);  // masked keys: exp(-inf) = 0
                af_halves(s[r], lo, hi);   // keys 2r and 2r + 1: the sum stays in key order
                l += lo;
                l += hi;
            }
#pragma unroll
            for (int t = 0; t < 16; ++t)
#pragma unroll
                for (int n = 0; n < NB; ++n) acc[n] = AF_MFMA(Vs[buf][2 * t + h][n * 32 + c], s[t], acc[n]);
            m = mn;
        }
        if (more) {
            af_put<HD>(Ks[buf ^ 1], rk, tid);
            af_put<HD>(Vs[buf ^ 1], rv, tid);
        }
        __syncthreads();
        buf ^= 1;
    }
    if (live) {
        const float inv = 1.f / l;
        T* o = (T*)a.o + b * a.o_bs + i * a.o_ts + (int64_t)hd * HD;
        const bool vo = af_vec_ok(o - i * a.o_ts, a.o_ts);
        // C/D map: register r of half h is output row (r & 3) + 8 (r >> 2) + 4 h, here d
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                af_store4<T>(o + n * 32 + 8 * g + 4 * h, vo, acc[n][4 * g] * inv, acc[n][4 * g + 1] * inv, acc[n][4 * g + 2] * inv,
                             acc[n][4 * g + 3] * inv);
        if (h == 0) a.lse[(b * a.heads + hd) * a.nq + i] = m + __logf(l);
    }
}

// ------------------------------------------------------------------------------------------------
// dQ (+ delta): S^T = K Q~^T, dP^T = V dO^T, dQ^T += K^T dS^T
// ------------------------------------------------------------------------------------------------
template <typename T, int HD>
__global__ void __launch_bounds__(AF_THREADS)
attn_bwd_dq_f32_mfma_kernel(AttnArgs a) {
    constexpr int NB = HD / 32;
    __shared__ float Ks[2][AF_KT][AF_LD(HD)];
    __shared__ float Vs[2][AF_KT][AF_LD(HD)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, c = lane & 31;
    const int64_t b = blockIdx.z;
    const int hd = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * AF_ROWS + wave * 32;
    const int64_t i = i0 + c;
    const bool live = i < a.nq, wave_live = i0 < a.nq;
    const int64_t bkv = a.kv_index ? a.kv_index[b] : b;
    const T* kb = (const T*)a.k + bkv * a.k_bs + (int64_t)hd * HD;
    const T* vb = (const T*)a.v + bkv * a.v_bs + (int64_t)hd * HD;
    const bool vk = af_vec_ok(kb, a.k_ts), vv = af_vec_ok(vb, a.v_ts);
    float qs[HD / 2], dos[HD / 2];   // slot h of instruction t is d = 2t + h
    float delta = 0.f, lse = 0.f;
    {
        const T* qp = (const T*)a.q + b * a.q_bs + i * a.q_ts + (int64_t)hd * HD;
        af_row_pairs<T, HD>(qp, af_vec_ok(qp - i * a.q_ts, a.q_ts), live, a.scale, h, qs);
    }
    {
        const T* dop = (const T*)a.d_o + b * a.o_bs + i * a.o_ts + (int64_t)hd * HD;
        const T* op = (const T*)a.o + b * a.o_bs + i * a.o_ts + (int64_t)hd * HD;
        const bool vdo = af_vec_ok(dop - i * a.o_ts, a.o_ts), vo = af_vec_ok(op - i * a.o_ts, a.o_ts);
#pragma unroll
        for (int d = 0; d < HD; d += 4) {
            const f32x4 v = af_row4<T>(dop, d, vdo, live, 1.f), w = af_row4<T>(op, d, vo, live, 1.f);
#pragma unroll
            for (int j = 0; j < 4; ++j) delta = fmaf(v[j], w[j], delta);
            dos[d / 2] = h ? v[1] : v[0];
            dos[d / 2 + 1] = h ? v[3] : v[2];
        }
    }
    if (live) {
        lse = a.lse[(b * a.heads + hd) * a.nq + i];
        if (h == 0) a.delta[(b * a.heads + hd) * a.nq + i] = delta;
    }
    f32x16 dq[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[n][r] = 0.f;
    const int krow = af_tile_row(c);
    f32x4 rk[NB], rv[NB];
    // a key row past nk is -0.f: its products with ds = +0 leave dq as it is
    af_fetch<T, HD>(rk, kb, a.k_ts, vk, 0, a.nk, -0.f, tid);
    af_fetch<T, HD>(rv, vb, a.v_ts, vv, 0, a.nk, 0.f, tid);
    af_put<HD>(Ks[0], rk, tid);
    af_put<HD>(Vs[0], rv, tid);
    __syncthreads();
    int buf = 0;
    for (int64_t j0 = 0; j0 < a.nk; j0 += AF_KT) {
        const bool more = j0 + AF_KT < a.nk;
        if (more) {
            af_fetch<T, HD>(rk, kb, a.k_ts, vk, j0 + AF_KT, a.nk, -0.f, tid);
            af_fetch<T, HD>(rv, vb, a.v_ts, vv, j0 + AF_KT, a.nk, 0.f, tid);
        }
        if (wave_live) {
            const int cnt = (int)((a.nk - j0) < AF_KT ? (a.nk - j0) : AF_KT);
            f32x16 sc, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { sc[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int t = 0; t < HD / 2; ++t) {
                sc = AF_MFMA(Ks[buf][krow][2 * t + h], qs[t], sc);
                dp = AF_MFMA(Vs[buf][krow][2 * t + h], dos[t], dp);
            }
            float dsr[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __expf(sc[r] - lse);
                const float ds = p * (dp[r] - delta);
                dsr[r] = 2 * r + h < cnt ? ds : 0.f;   // a padded ds never reaches a product
            }
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (2 * t < cnt) {
#pragma unroll
                    for (int n = 0; n < NB; ++n) dq[n] = AF_MFMA(Ks[buf][2 * t + h][n * 32 + c], dsr[t], dq[n]);
                }
        }
        if (more) {
            af_put<HD>(Ks[buf ^ 1], rk, tid);
            af_put<HD>(Vs[buf ^ 1], rv, tid);
        }
        __syncthreads();
        buf ^= 1;
    }
    if (live) {
        T* o = (T*)a.dq + b * a.dq_bs + i * a.dq_ts + (int64_t)hd * HD;
        const bool vo = af_vec_ok(o - i * a.dq_ts, a.dq_ts);
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                af_store4<T>(o + n * 32 + 8 * g + 4 * h, vo, dq[n][4 * g] * a.scale, dq[n][4 * g + 1] * a.scale,
                             dq[n][4 * g + 2] * a.scale, dq[n][4 * g + 3] * a.scale);
    }
}

// ------------------------------------------------------------------------------------------------
// dK / dV: S = Q K~^T (rows queries, columns keys), dP = dO V^T, dV^T += dO^T P, dK^T += Q^T dS
// ------------------------------------------------------------------------------------------------
template <typename T, int HD>
__global__ void __launch_bounds__(AF_THREADS)
attn_bwd_dkv_f32_mfma_kernel(AttnArgs a) {
    constexpr int NB = HD / 32;
    __shared__ float Qs[2][AF_KT][AF_LD(HD)];
    __shared__ float Ds[2][AF_KT][AF_LD(HD)];
    __shared__ float Ls[2][AF_KT], Dl[2][AF_KT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, c = lane & 31;
    const int64_t b = blockIdx.z;
    const int hd = blockIdx.y;
    const int64_t jw = (int64_t)blockIdx.x * AF_ROWS + wave * 32;
    const int64_t j = jw + c;
    const bool live = j < a.nk, wave_live = jw < a.nk;
    const T* qb = (const T*)a.q + b * a.q_bs + (int64_t)hd * HD;
    const T* dob = (const T*)a.d_o + b * a.o_bs + (int64_t)hd * HD;
    const bool vq = af_vec_ok(qb, a.q_ts), vd = af_vec_ok(dob, a.o_ts);
    const float* lseb = a.lse + (b * a.heads + hd) * a.nq;
    const float* delb = a.delta + (b * a.heads + hd) * a.nq;
    float ks[HD / 2], vs[HD / 2];   // slot h of instruction t is d = 2t + h; ks carries the softmax scale
    {
        const int64_t bkv = a.kv_index ? a.kv_index[b] : b;
        const T* kp = (const T*)a.k + bkv * a.k_bs + j * a.k_ts + (int64_t)hd * HD;
        const T* vp = (const T*)a.v + bkv * a.v_bs + j * a.v_ts + (int64_t)hd * HD;
        af_row_pairs<T, HD>(kp, af_vec_ok(kp - j * a.k_ts, a.k_ts), live, a.scale, h, ks);
        af_row_pairs<T, HD>(vp, af_vec_ok(vp - j * a.v_ts, a.v_ts), live, 1.f, h, vs);
    }
    f32x16 dk[NB], dv[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[n][r] = 0.f; dv[n][r] = 0.f; }
    const int qrow = af_tile_row(c);
    f32x4 rq[NB], rd[NB];
    float rl = 0.f, rdl = 0.f;
    auto fetch = [&](int64_t i0) {
        // a query row past nq is -0.f: its products with p = ds = +0 leave dk / dv as they are
        af_fetch<T, HD>(rq, qb, a.q_ts, vq, i0, a.nq, -0.f, tid);
        af_fetch<T, HD>(rd, dob, a.o_ts, vd, i0, a.nq, -0.f, tid);
        if (tid < AF_KT) {
            const int64_t i = i0 + tid;
            rl = i < a.nq ? lseb[i] : 0.f;
            rdl = i < a.nq ? delb[i] : 0.f;
        }
    };
    auto put = [&](int bf) {
        af_put<HD>(Qs[bf], rq, tid);
        af_put<HD>(Ds[bf], rd, tid);
        if (tid < AF_KT) { Ls[bf][tid] = rl; Dl[bf][tid] = rdl; }
    };
    fetch(0);
    put(0);
    __syncthreads();
    int buf = 0;
    for (int64_t i0 = 0; i0 < a.nq; i0 += AF_KT) {
        const bool more = i0 + AF_KT < a.nq;
        if (more) fetch(i0 + AF_KT);
        if (wave_live) {
            const int cnt = (int)((a.nq - i0) < AF_KT ? (a.nq - i0) : AF_KT);
            f32x16 sc, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { sc[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int t = 0; t < HD / 2; ++t) {
                sc = AF_MFMA(Qs[buf][qrow][2 * t + h], ks[t], sc);
                dp = AF_MFMA(Ds[buf][qrow][2 * t + h], vs[t], dp);
            }
            float pr[16], dsr[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {   // register r of half h is query 2r + h of the tile
                const float p = __expf(sc[r] - Ls[buf][2 * r + h]);
                const float ds = p * (dp[r] - Dl[buf][2 * r + h]);
                pr[r] = 2 * r + h < cnt ? p : 0.f;
                dsr[r] = 2 * r + h < cnt ? ds : 0.f;
            }
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (2 * t < cnt) {
#pragma unroll
                    for (int n = 0; n < NB; ++n) {
                        dv[n] = AF_MFMA(Ds[buf][2 * t + h][n * 32 + c], pr[t], dv[n]);
                        dk[n] = AF_MFMA(Qs[buf][2 * t + h][n * 32 + c], dsr[t], dk[n]);
                    }
                }
        }
        if (more) put(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    if (live) {
        T* ok = (T*)a.dk + b * a.dk_bs + j * a.dk_ts + (int64_t)hd * HD;
        T* ov = (T*)a.dv + b * a.dv_bs + j * a.dv_ts + (int64_t)hd * HD;
        const bool vok = af_vec_ok(ok - j * a.dk_ts, a.dk_ts), vov = af_vec_ok(ov - j * a.dv_ts, a.dv_ts);
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                T* pk = ok + n * 32 + 8 * g + 4 * h;
                T* pv = ov + n * 32 + 8 * g + 4 * h;
                af_store4<T>(pk, vok, dk[n][4 * g] * a.scale, dk[n][4 * g + 1] * a.scale, dk[n][4 * g + 2] * a.scale,
                             dk[n][4 * g + 3] * a.scale);
                af_store4<T>(pv, vov, dv[n][4 * g], dv[n][4 * g + 1], dv[n][4 * g + 2], dv[n][4 * g + 3]);
            }
    }
}

template <typename T, int HD>
static int launch_fwd(const AttnArgs& a, hipStream_t s) {
    dim3 grid((unsigned)ceil_div64(a.nq, AF_ROWS), a.heads, (unsigned)a.batch);
    hipLaunchKernelGGL((attn_fwd_f32_mfma_kernel<T, HD>), grid, dim3(AF_THREADS), 0, s, a);
    return vited_check_launch();
}

template <typename T, int HD>
static int launch_bwd(const AttnArgs& a, hipStream_t s) {
    dim3 gq((unsigned)ceil_div64(a.nq, AF_ROWS), a.heads, (unsigned)a.batch);
    dim3 gk((unsigned)ceil_div64(a.nk, AF_ROWS), a.heads, (unsigned)a.batch);
    hipLaunchKernelGGL((attn_bwd_dq_f32_mfma_kernel<T, HD>), gq, dim3(AF_THREADS), 0, s, a);
    hipLaunchKernelGGL((attn_bwd_dkv_f32_mfma_kernel<T, HD>), gk, dim3(AF_THREADS), 0, s, a);
    return vited_check_launch();
}

// Host-only: the calls that go to the matrix-core kernels (DESIGN.md section 38 has the measurements behind it).
bool attention_f32_mfma_supported(int dtype, int64_t batch, int heads, int64_t nq, int64_t nk, int head_dim, bool backward) {
    if (dtype != VITED_F32 && dtype != VITED_BF16) return false;
    if (head_dim != 32 && head_dim != 64) return false;
    if (batch <= 0 || heads <= 0 || nq <= 0 || nk <= 0) return false;
    (void)backward;
    return true;
}

int attention_fwd_f32_mfma(const AttnArgs& a, int dtype, hipStream_t s) {
    if (dtype == VITED_F32) {
        if (a.head_dim == 32) return launch_fwd<float, 32>(a, s);
        if (a.head_dim == 64) return launch_fwd<float, 64>(a, s);
    } else if (dtype == VITED_BF16) {
        if (a.head_dim == 32) return launch_fwd<bf16, 32>(a, s);
        if (a.head_dim == 64) return launch_fwd<bf16, 64>(a, s);
    }
    return VITED_ERR_UNSUPPORTED;
}

int attention_bwd_f32_mfma(const AttnArgs& a, int dtype, hipStream_t s) {
    if (dtype == VITED_F32) {
        if (a.head_dim == 32) return launch_bwd<float, 32>(a, s);
        if (a.head_dim == 64) return launch_bwd<float, 64>(a, s);
    } else if (dtype == VITED_BF16) {
        if (a.head_dim == 32) return launch_bwd<bf16, 32>(a, s);
        if (a.head_dim == 64) return launch_bwd<bf16, 64>(a, s);
    }
    return VITED_ERR_UNSUPPORTED;
}
