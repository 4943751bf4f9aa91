// Host build of the q/k-norm arithmetic (csrc/qk_norm.h) for the address and undefined-behaviour sanitizers: the very text the HIP
// kernels run, driven lane by lane the way qk_norm.hip drives it - 8 lanes per head row, each with head_dim / 8 elements, the row
// sums formed by the xor-1 / xor-2 / xor-4 butterfly of the kernel's DPP adds - over a few hundred random and structured head rows
// in exactly-sized heap blocks, forward and backward, and compared with a long-double evaluation of the formulas.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vit-ed_amd/csrc tools/qknorm_host_check.cpp -o qknorm_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "qk_norm.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {      // xorshift64*, in [-1, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) / (double)(1ull << 52) - 1.0;
}

// what group_sum (qk_norm.hip) leaves in every lane of an 8-lane group
static void butterfly(float* v) {
    for (int step = 1; step < QKN_LANES; step <<= 1) {
        float t[QKN_LANES];
        for (int l = 0; l < QKN_LANES; ++l) t[l] = v[l] + v[l ^ step];
        memcpy(v, t, sizeof t);
    }
}

struct Case { const char* name; int kind; };     // kind: 0 random, 1 equal values, 2 large offset, 3 tiny values, 4 one spike, 5 gamma 0

static int failures = 0;
static void expect(bool ok, const char* what, const char* name, int hd, double got, double want) {
    if (!ok) {
        ++failures;
        fprintf(stderr, "FAIL %s (%s, head_dim %d): got %.9g want %.9g\n", what, name, hd, got, want);
    }
}

template <int E> static void run_rows(const Case& c, int rows, float eps) {
    constexpr int HD = E * QKN_LANES;
    // exactly-sized heap blocks: an access one element past a row shows under the address sanitizer
    float* x = (float*)malloc(sizeof(float) * rows * HD);
    float* dy = (float*)malloc(sizeof(float) * rows * HD);
    float* y = (float*)malloc(sizeof(float) * rows * HD);
    float* dx = (float*)malloc(sizeof(float) * rows * HD);
    float* gamma = (float*)malloc(sizeof(float) * HD);
    float* beta = (float*)malloc(sizeof(float) * HD);
    float* mean = (float*)malloc(sizeof(float) * rows);
    float* rstd = (float*)malloc(sizeof(float) * rows);
    float* dgamma = (float*)calloc(HD, sizeof(float));
    float* dbeta = (float*)calloc(HD, sizeof(float));
    for (int i = 0; i < HD; ++i) {
        gamma[i] = c.kind == 5 ? 0.f : (float)(1.0 + 0.3 * uniform());
        beta[i] = (float)(0.2 * uniform());
    }
    for (int r = 0; r < rows; ++r) {
        const float level = (float)(3.0 * uniform());
        for (int i = 0; i < HD; ++i) {
            float v = (float)(2.0 * uniform());
            if (c.kind == 1) v = level;
            if (c.kind == 2) v = 1000.f + (float)uniform();
            if (c.kind == 3) v = (float)(1e-6 * uniform());
            if (c.kind == 4) v = i == (r % HD) ? 50.f : (float)(0.01 * uniform());
            x[r * HD + i] = v;
            dy[r * HD + i] = (float)uniform();
        }
    }
    const float inv_d = 1.f / HD;
    // forward, row by row, lane by lane
    for (int r = 0; r < rows; ++r) {
        float part[QKN_LANES];
        for (int l = 0; l < QKN_LANES; ++l) part[l] = qkn_sum_part<E>(x + r * HD + l * E);
        butterfly(part);
        const float mu = part[0] * inv_d;
        for (int l = 1; l < QKN_LANES; ++l) expect(part[l] == part[0], "lanes agree on the sum", c.name, HD, part[l], part[0]);
        for (int l = 0; l < QKN_LANES; ++l) part[l] = qkn_sq_part<E>(x + r * HD + l * E, mu);
        butterfly(part);
        const float rs = qkn_rstd(part[0], inv_d, eps);
        for (int l = 0; l < QKN_LANES; ++l) qkn_fwd_out<E>(x + r * HD + l * E, mu, rs, gamma + l * E, beta + l * E, y + r * HD + l * E);
        mean[r] = mu;
        rstd[r] = rs;
    }
    // backward: a lane keeps its E column sums over all rows, as in the kernel
    for (int r = 0; r < rows; ++r) {
        float xh[HD], g[HD], s1[QKN_LANES], s2[QKN_LANES];
        for (int l = 0; l < QKN_LANES; ++l)
            qkn_bwd_parts<E>(dy + r * HD + l * E, x + r * HD + l * E, mean[r], rstd[r], gamma + l * E, xh + l * E, g + l * E, s1[l], s2[l],
                             dgamma + l * E, dbeta + l * E);
        butterfly(s1);
        butterfly(s2);
        for (int l = 0; l < QKN_LANES; ++l) qkn_bwd_out<E>(g + l * E, xh + l * E, s1[l] * inv_d, s2[l] * inv_d, rstd[r], dx + r * HD + l * E);
    }
    // the long-double evaluation
    std::vector<long double> want_dg(HD, 0.0L), want_db(HD, 0.0L);
    for (int r = 0; r < rows; ++r) {
        long double m = 0, var = 0;
        for (int i = 0; i < HD; ++i) m += x[r * HD + i];
        m /= HD;
        for (int i = 0; i < HD; ++i) var += (x[r * HD + i] - m) * (x[r * HD + i] - m);
        var /= HD;
        const long double rs = 1.0L / sqrtl(var + (long double)eps);
        // how far fp32 can be off: a few ulps of the largest |x - mean| * rstd, plus the mean's own rounding carried through rstd
        long double xmax = 0;
        for (int i = 0; i < HD; ++i) xmax = fmaxl(xmax, fabsl((long double)x[r * HD + i]));
        const long double xh_tol = 4e-6L * (1.0L + xmax * rs);
        long double c1 = 0, c2 = 0;
        for (int i = 0; i < HD; ++i) {
            const long double xh = (x[r * HD + i] - m) * rs, gg = (long double)dy[r * HD + i] * gamma[i];
            c1 += gg;
            c2 += gg * xh;
        }
        c1 /= HD;
        c2 /= HD;
        for (int i = 0; i < HD; ++i) {
            const long double xh = (x[r * HD + i] - m) * rs;
            const long double wy = xh * gamma[i] + beta[i];
            expect(fabsl(y[r * HD + i] - wy) <= xh_tol * (1.0L + fabsl((long double)gamma[i])), "y", c.name, HD, y[r * HD + i], (double)wy);
            const long double gg = (long double)dy[r * HD + i] * gamma[i];
            const long double wdx = rs * (gg - c1 - xh * c2);
            expect(fabsl(dx[r * HD + i] - wdx) <= xh_tol * 8.0L * (1.0L + fabsl(wdx)) * fmaxl(1.0L, rs), "dx", c.name, HD, dx[r * HD + i], (double)wdx);
            want_dg[i] += (long double)dy[r * HD + i] * xh;
            want_db[i] += dy[r * HD + i];
            if (c.kind == 1) expect(y[r * HD + i] == beta[i], "equal values give exactly beta", c.name, HD, y[r * HD + i], beta[i]);
            if (c.kind == 5) {
                expect(y[r * HD + i] == beta[i], "gamma 0 gives exactly beta", c.name, HD, y[r * HD + i], beta[i]);
                expect(dx[r * HD + i] == 0.f, "gamma 0 gives dx 0", c.name, HD, dx[r * HD + i], 0.0);
            }
        }
        expect(fabsl(mean[r] - m) <= 1e-6L * (1.0L + xmax), "mean", c.name, HD, mean[r], (double)m);
        expect(fabsl(rstd[r] - rs) <= 1e-5L * rs * (1.0L + xmax * rs), "rstd", c.name, HD, rstd[r], (double)rs);
    }
    for (int i = 0; i < HD; ++i) {
        long double xs = 0;
        for (int r = 0; r < rows; ++r) xs = fmaxl(xs, fabsl((long double)x[r * HD + i]) * rstd[r]);
        expect(fabsl(dgamma[i] - want_dg[i]) <= 1e-5L * rows * (1.0L + xs), "dgamma", c.name, HD, dgamma[i], (double)want_dg[i]);
        expect(fabsl(dbeta[i] - want_db[i]) <= 1e-6L * rows, "dbeta", c.name, HD, dbeta[i], (double)want_db[i]);
    }
    free(x); free(dy); free(y); free(dx); free(gamma); free(beta); free(mean); free(rstd); free(dgamma); free(dbeta);
}

int main() {
    const Case cases[] = {{"random", 0}, {"equal values", 1}, {"large offset", 2}, {"tiny values", 3}, {"one spike", 4}, {"gamma 0", 5}};
    int rows_total = 0;
    for (const Case& c : cases) {
        const int rows = c.kind == 0 ? 160 : 40;
        run_rows<4>(c, rows, 1e-6f);
        run_rows<8>(c, rows, 1e-6f);
        rows_total += 2 * rows;
    }
    if (failures) {
        fprintf(stderr, "qknorm_host_check: %d failures\n", failures);
        return 1;
    }
    printf("qknorm_host_check ok: %d head rows, head_dim 32 and 64, forward and backward\n", rows_total);
    return 0;
}
