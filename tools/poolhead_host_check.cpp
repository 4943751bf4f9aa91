// Host build of the pooled-head arithmetic (csrc/pool_head.h) for the address and undefined-behaviour sanitizers: the very text the
// HIP kernels run, driven lane by lane the way pool_head.hip drives it - 32 lanes per token row, each with its 16-byte vectors, the
// row sums formed in the order of the kernel's DPP half-wave sum, 8 row owners per chunk of 64 tokens, the owners' and the chunks' sums
// added in ascending order - over exactly-sized heap blocks, forward and backward, plain and with a LayerNorm, and compared with a
// long-double evaluation of the formulas.  tokens 2, 5, 65, 100 (99 pooled tokens: the chunks do not divide them), 1025; dim 32, 384, 1000.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vit-ed_amd/csrc tools/poolhead_host_check.cpp -o poolhead_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pool_head.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {      // xorshift64*, in [-1, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) / (double)(1ull << 52) - 1.0;
}

// what half_wave_sum (common.h) leaves in every lane: rotations by 8, 4, 2, 1 inside each 16-lane row, then the other row
static void half_wave_sum(float* v) {
    float t[POOL_LANES];
    for (int rot = 8; rot >= 1; rot >>= 1) {
        for (int l = 0; l < POOL_LANES; ++l) t[l] = v[l] + v[(l & 16) | ((l + rot) & 15)];
        memcpy(v, t, sizeof t);
    }
    for (int l = 0; l < POOL_LANES; ++l) t[l] = v[l] + v[l ^ 16];
    memcpy(v, t, sizeof t);
}

static int failures = 0;
static void expect(bool ok, const char* what, int tokens, int dim, int norm, double got, double want) {
    if (!ok && ++failures < 20) fprintf(stderr, "FAIL %s (tokens %d, dim %d, norm %d): got %.9g want %.9g\n", what, tokens, dim, norm, got, want);
}

// a lane's piece of a row, zeros past dim: what pool_load (pool_head.hip) produces
template <int VPL> static void load(const float* row, int dim, int lane, float* v) {
    for (int j = 0; j < VPL; ++j)
        for (int e = 0; e < 4; ++e) v[4 * j + e] = pool_col(j, lane) < dim ? row[pool_col(j, lane) + e] : 0.f;
}
template <int VPL> static void store(float* row, int dim, int lane, const float* v) {
    for (int j = 0; j < VPL; ++j)
        for (int e = 0; e < 4; ++e)
            if (pool_col(j, lane) < dim) row[pool_col(j, lane) + e] = v[4 * j + e];
}

template <int VPL> static void run(int items, int tokens, int first, int dim, bool norm) {
    const float eps = 1e-6f;
    const int64_t nsplit = pool_splits(tokens, first);
    const float count = (float)(tokens - first), inv_d = 1.f / dim;
    const size_t rows = (size_t)items * tokens;
    // exactly-sized heap blocks: an access one element past a row, an item or a partial row shows under the address sanitizer
    float* x = (float*)malloc(sizeof(float) * rows * dim);
    float* dx = (float*)malloc(sizeof(float) * rows * dim);
    float* g = (float*)malloc(sizeof(float) * items * dim);
    float* pooled = (float*)malloc(sizeof(float) * items * dim);
    float* gamma = (float*)malloc(sizeof(float) * dim);
    float* beta = (float*)malloc(sizeof(float) * dim);
    float* mean = (float*)malloc(sizeof(float) * rows);
    float* rstd = (float*)malloc(sizeof(float) * rows);
    float* part = (float*)malloc(sizeof(float) * items * nsplit * dim);          // the forward's partial rows
    float* part2 = (float*)malloc(sizeof(float) * items * nsplit * 2 * dim);     // the backward's [2][dim] partial rows
    float* lds = (float*)malloc(sizeof(float) * POOL_HALVES * 2 * dim);
    float* dgamma = (float*)malloc(sizeof(float) * dim);
    float* dbeta = (float*)malloc(sizeof(float) * dim);
    for (size_t i = 0; i < rows * dim; ++i) x[i] = (float)(2.0 * uniform() + 0.5);
    for (size_t i = 0; i < rows * dim; ++i) dx[i] = NAN;
    for (int i = 0; i < items * dim; ++i) g[i] = (float)uniform();
    for (int i = 0; i < dim; ++i) { gamma[i] = (float)(1.0 + 0.3 * uniform()); beta[i] = (float)(0.2 * uniform()); }

    // ---- forward: one "workgroup" per (item, chunk)
    for (int b = 0; b < items; ++b)
        for (int64_t sp = 0; sp < nsplit; ++sp) {
            int64_t t0, t1;
            pool_chunk(tokens, first, sp, t0, t1);
            for (int h = 0; h < POOL_HALVES; ++h) {
                std::vector<float> acc(POOL_LANES * VPL * 4, 0.f);
                for (int64_t t = t0 + h; t < t1; t += POOL_HALVES) {
                    const float* row = x + ((size_t)b * tokens + t) * dim;
                    float v[POOL_LANES][VPL * 4], s[POOL_LANES];
                    for (int l = 0; l < POOL_LANES; ++l) load<VPL>(row, dim, l, v[l]);
                    if (norm) {
                        for (int l = 0; l < POOL_LANES; ++l) s[l] = pool_sum_part<VPL>(v[l]);
                        half_wave_sum(s);
                        const float mu = s[0] * inv_d;
                        for (int l = 1; l < POOL_LANES; ++l) expect(s[l] == s[0], "lanes agree on the sum", tokens, dim, norm, s[l], s[0]);
                        for (int l = 0; l < POOL_LANES; ++l) s[l] = pool_sq_part<VPL>(v[l], mu, dim, l);
                        half_wave_sum(s);
                        const float rs = pool_rstd(s[0], inv_d, eps);
                        for (int l = 0; l < POOL_LANES; ++l) pool_acc_norm<VPL>(&acc[l * VPL * 4], v[l], mu, rs, dim, l);
                        mean[(size_t)b * tokens + t] = mu;
                        rstd[(size_t)b * tokens + t] = rs;
                    } else {
                        for (int l = 0; l < POOL_LANES; ++l) pool_acc_plain<VPL>(&acc[l * VPL * 4], v[l]);
                    }
                }
                for (int l = 0; l < POOL_LANES; ++l) store<VPL>(lds + (size_t)h * dim, dim, l, &acc[l * VPL * 4]);
            }
            for (int c = 0; c < dim; ++c) {
                const float s = pool_sum_ordered(lds + c, dim, POOL_HALVES);
                if (nsplit > 1) part[((size_t)b * nsplit + sp) * dim + c] = s;
                else pooled[(size_t)b * dim + c] = norm ? pool_finish_norm(s, count, gamma[c], beta[c]) : pool_finish(s, count);
            }
        }
    if (nsplit > 1)
        for (int b = 0; b < items; ++b)
            for (int c = 0; c < dim; ++c) {
                const float s = pool_sum_ordered(part + (size_t)b * nsplit * dim + c, dim, nsplit);
                pooled[(size_t)b * dim + c] = norm ? pool_finish_norm(s, count, gamma[c], beta[c]) : pool_finish(s, count);
            }

    // ---- backward
    for (int b = 0; b < items; ++b)
        for (int64_t sp = 0; sp < nsplit; ++sp) {
            int64_t t0, t1;
            pool_chunk(tokens, first, sp, t0, t1);
            float dy[POOL_LANES][VPL * 4], gg[POOL_LANES][VPL * 4], s[POOL_LANES];
            for (int l = 0; l < POOL_LANES; ++l) {
                load<VPL>(g + (size_t)b * dim, dim, l, dy[l]);
                load<VPL>(gamma, dim, l, gg[l]);
                for (int i = 0; i < VPL * 4; ++i) { dy[l][i] = pool_grad(dy[l][i], count); gg[l][i] *= dy[l][i]; }
                s[l] = pool_sum_part<VPL>(gg[l]);
            }
            half_wave_sum(s);
            const float c1 = s[0] * inv_d;
            if (sp == 0)
                for (int h = 0; h < POOL_HALVES; ++h)
                    for (int64_t t = h; t < first; t += POOL_HALVES) {
                        float zero[VPL * 4] = {};
                        for (int l = 0; l < POOL_LANES; ++l) store<VPL>(dx + ((size_t)b * tokens + t) * dim, dim, l, zero);
                    }
            for (int h = 0; h < POOL_HALVES; ++h) {
                std::vector<float> dg(POOL_LANES * VPL * 4, 0.f), db(POOL_LANES * VPL * 4, 0.f);
                for (int64_t t = t0 + h; t < t1; t += POOL_HALVES) {
                    float* out = dx + ((size_t)b * tokens + t) * dim;
                    for (int i = 0; i < dim; ++i) expect(std::isnan(out[i]), "dx is written once", tokens, dim, norm, out[i], NAN);
                    if (!norm) {
                        for (int l = 0; l < POOL_LANES; ++l) store<VPL>(out, dim, l, dy[l]);
                        continue;
                    }
                    const float* row = x + ((size_t)b * tokens + t) * dim;
                    const float mu = mean[(size_t)b * tokens + t], rs = rstd[(size_t)b * tokens + t];
                    float xh[POOL_LANES][VPL * 4], v[VPL * 4], o[VPL * 4], s2[POOL_LANES];
                    for (int l = 0; l < POOL_LANES; ++l) {
                        load<VPL>(row, dim, l, v);
                        s2[l] = pool_bwd_parts<VPL>(dy[l], gg[l], v, mu, rs, xh[l], &dg[l * VPL * 4], &db[l * VPL * 4], dim, l);
                    }
                    half_wave_sum(s2);
                    for (int l = 0; l < POOL_LANES; ++l) {
                        pool_bwd_out<VPL>(gg[l], xh[l], c1, s2[l] * inv_d, rs, o);
                        store<VPL>(out, dim, l, o);
                    }
                }
                for (int l = 0; l < POOL_LANES; ++l) {
                    store<VPL>(lds + (size_t)h * 2 * dim, dim, l, &dg[l * VPL * 4]);
                    store<VPL>(lds + (size_t)h * 2 * dim + dim, dim, l, &db[l * VPL * 4]);
                }
            }
            if (norm)
                for (int c = 0; c < 2 * dim; ++c) part2[((size_t)b * nsplit + sp) * 2 * dim + c] = pool_sum_ordered(lds + c, 2 * dim, POOL_HALVES);
        }
    if (norm)
        for (int c = 0; c < dim; ++c) {
            dgamma[c] = pool_sum_ordered(part2 + c, 2 * dim, items * nsplit);
            dbeta[c] = pool_sum_ordered(part2 + dim + c, 2 * dim, items * nsplit);
        }

    // ---- the long-double evaluation
    const long double n = tokens - first;
    std::vector<long double> want_dg(dim, 0.0L), want_db(dim, 0.0L);
    for (int b = 0; b < items; ++b) {
        std::vector<long double> want(dim, 0.0L);
        for (int t = 0; t < tokens; ++t) {
            const float* row = x + ((size_t)b * tokens + t) * dim;
            const float* out = dx + ((size_t)b * tokens + t) * dim;
            if (t < first) {
                for (int i = 0; i < dim; ++i) expect(out[i] == 0.f, "prefix rows get zero", tokens, dim, norm, out[i], 0.0);
                continue;
            }
            long double m = 0, var = 0, xmax = 0;
            for (int i = 0; i < dim; ++i) { m += row[i]; xmax = fmaxl(xmax, fabsl((long double)row[i])); }
            m /= dim;
            for (int i = 0; i < dim; ++i) var += (row[i] - m) * (row[i] - m);
            const long double rs = 1.0L / sqrtl(var / dim + (long double)eps);
            const long double xh_tol = 4e-6L * (1.0L + xmax * rs);
            long double c1 = 0, c2 = 0;
            for (int i = 0; i < dim; ++i) {
                const long double xh = (row[i] - m) * rs, gg = (long double)g[(size_t)b * dim + i] / n * gamma[i];
                c1 += gg;
                c2 += gg * xh;
            }
            c1 /= dim;
            c2 /= dim;
            for (int i = 0; i < dim; ++i) {
                const long double dy = (long double)g[(size_t)b * dim + i] / n;
                if (!norm) {
                    want[i] += row[i];
                    expect(fabsl(out[i] - dy) <= 1e-7L * fabsl(dy), "dx", tokens, dim, norm, out[i], (double)dy);
                    continue;
                }
                const long double xh = (row[i] - m) * rs;
                want[i] += xh * gamma[i] + beta[i];
                const long double wdx = rs * (dy * gamma[i] - c1 - xh * c2);
                expect(fabsl(out[i] - wdx) <= xh_tol * 8.0L * (fabsl(dy) + fabsl(wdx)) * fmaxl(1.0L, rs), "dx", tokens, dim, norm, out[i], (double)wdx);
                want_dg[i] += dy * xh;
                want_db[i] += dy;
            }
            if (norm) {
                const size_t r = (size_t)b * tokens + t;
                expect(fabsl(mean[r] - m) <= 1e-6L * (1.0L + xmax), "mean", tokens, dim, norm, mean[r], (double)m);
                expect(fabsl(rstd[r] - rs) <= 1e-5L * rs * (1.0L + xmax * rs), "rstd", tokens, dim, norm, rstd[r], (double)rs);
            }
        }
        // fp32 sums of n terms of magnitude <= 4: error <= n ulps of the running sum, far below this
        for (int i = 0; i < dim; ++i)
            expect(fabsl(pooled[(size_t)b * dim + i] - want[i] / n) <= 2e-5L, "pooled", tokens, dim, norm, pooled[(size_t)b * dim + i], (double)(want[i] / n));
    }
    if (norm)
        for (int i = 0; i < dim; ++i) {
            expect(fabsl(dgamma[i] - want_dg[i]) <= 2e-5L * items, "dgamma", tokens, dim, norm, dgamma[i], (double)want_dg[i]);
            expect(fabsl(dbeta[i] - want_db[i]) <= 2e-6L * items, "dbeta", tokens, dim, norm, dbeta[i], (double)want_db[i]);
        }
    free(x); free(dx); free(g); free(pooled); free(gamma); free(beta); free(mean); free(rstd); free(part); free(part2); free(lds);
    free(dgamma); free(dbeta);
}

static void run_dim(int items, int tokens, int first, int dim, bool norm) {
    switch ((dim + 127) / 128) {
        case 1: run<1>(items, tokens, first, dim, norm); break;
        case 3: run<3>(items, tokens, first, dim, norm); break;
        case 8: run<8>(items, tokens, first, dim, norm); break;
        default: fprintf(stderr, "no instance for dim %d\n", dim); ++failures;
    }
}

int main() {
    const int token_counts[] = {2, 5, 65, 100, 1025}, dims[] = {32, 384, 1000};
    int cases = 0;
    for (int tokens : token_counts)
        for (int dim : dims)
            for (int norm = 0; norm < 2; ++norm, ++cases) run_dim(tokens > 100 ? 1 : 2, tokens, 1, dim, norm != 0);
    run_dim(2, 70, 0, 384, true);        // no prefix: 70 pooled tokens = 64 + 6
    run_dim(2, 12, 3, 32, false);        // a longer prefix
    cases += 2;
    if (failures) {
        fprintf(stderr, "poolhead_host_check: %d failures\n", failures);
        return 1;
    }
    printf("poolhead_host_check ok: %d cases, forward and backward, plain and with a LayerNorm\n", cases);
    return 0;
}
