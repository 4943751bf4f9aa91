// Host build of LAMB's update bodies (csrc/optim_update.h: lamb_coef, lamb_u, lamb_ratio, lamb_moments_piece, lamb_apply_piece) for the
// address and undefined-behaviour sanitizers: the very text the HIP kernels run, driven the way vited_lamb_step's three launches drive
// it (64 x 64 tiles, 4 columns per thread, the same tail and alignment rules; per-tile sums, then the tensor's ratio, then the apply
// pass) over exactly-sized heap buffers, and compared with a plain double-precision loop.  Cases: decayed, undecayed (r = 1),
// always_adapt, trust_clip; p = 0 (r = 1); g = 0 with zero state (r = 1 / wd); p = 0 and g = 0 (r = 1, nothing non-finite); an odd-word
// start (no 16-byte accesses); gradients kept (their bits must stay).
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vit-ed_amd/csrc tools/lamb_host_check.cpp -o lamb_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "optim_update.h"

static unsigned rng_state = 2463534242u;
static float rnd() {                                   // uniform in [-1, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)((int)(rng_state >> 8) % 20001 - 10000) / 10000.0f;
}

// as tools/optim_host_check.cpp: rtol 1e-5 plus a few fp32 roundings of the largest operand
static const double ATOL_M = 5e-7, ATOL_V = 1e-8, ATOL_P = 2e-6;
static bool close_to(double got, double want, double atol) { return std::fabs(got - want) <= atol + 1e-5 * std::fabs(want); }

enum Fill { PLAIN, ZERO_P, ZERO_G, ZERO_BOTH };

static int run_case(int64_t rows, int64_t cols, int skew, float wd, int always_adapt, int trust_clip, Fill fill, int zero_grad, int steps) {
    const size_t n = (size_t)(rows * cols);
    std::vector<float*> blocks;
    auto exact = [&]() -> float* {                      // exactly n floats, ending at the end of the allocation
        char* raw = (char*)malloc(n * 4 + (size_t)skew * 4);
        blocks.push_back((float*)raw);
        return (float*)raw + skew;
    };
    float *p = exact(), *g = exact(), *m = exact(), *v = exact();
    std::vector<double> dp(n), dm(n, 0.0), dv(n, 0.0), du(n);
    for (size_t i = 0; i < n; ++i) {
        p[i] = (fill == ZERO_P || fill == ZERO_BOTH) ? 0.f : 0.1f * rnd();
        m[i] = v[i] = 0.f;
        dp[i] = p[i];
    }
    float hyper[16] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, /* group 0 */ 2e-3f, 0.9f, 0.999f, 1e-6f, wd, (float)always_adapt,
                       (float)trust_clip, 0.f};
    const float max_norm = 1.0f;
    int bad = 0;
    float r = NAN;
    for (int it = 0; it < steps; ++it) {
        std::vector<float> g0(n);
        for (size_t i = 0; i < n; ++i) g0[i] = g[i] = (fill == ZERO_G || fill == ZERO_BOTH) ? 0.f : 0.3f * rnd();
        const float norm = it == 1 ? 7.0f : 0.5f;       // the clip is active in the second update
        float res[4];
        optim_decide(norm, max_norm, hyper, res);
        const LambCoef k = lamb_coef(hyper + 8, res[3]);
        const bool vec = (cols & 3) == 0 && (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
        const int64_t tiles_r = (rows + 63) / 64, tiles_c = (cols + 63) / 64;
        float sum_p = 0.f, sum_u = 0.f;
        for (int64_t t = 0; t < tiles_r * tiles_c; ++t) {           // launch 3: one workgroup per tile, 256 threads, 4 pieces each
            float tile_p = 0.f, tile_u = 0.f;
            for (int tid = 0; tid < 256; ++tid) {
                float sp = 0.f, su = 0.f;
                for (int j = 0; j < 4; ++j) {
                    const int64_t rr = (t / tiles_c) * 64 + (tid >> 4) + 16 * j, c = (t % tiles_c) * 64 + (tid & 15) * 4;
                    if (rr >= rows || c >= cols) continue;
                    const int q = cols - c < 4 ? (int)(cols - c) : 4;
                    lamb_moments_piece(p, g, m, v, rr * cols + c, q, vec && q == 4, k, res[1], &sp, &su);
                }
                tile_p += sp; tile_u += su;
            }
            sum_p += tile_p; sum_u += tile_u;
        }
        r = lamb_ratio(sum_p, sum_u, k);                             // launch 4
        std::vector<float> pn_all(n, NAN);
        for (int64_t t = 0; t < tiles_r * tiles_c; ++t)              // launch 5
            for (int tid = 0; tid < 256; ++tid)
                for (int j = 0; j < 4; ++j) {
                    const int64_t rr = (t / tiles_c) * 64 + (tid >> 4) + 16 * j, c = (t % tiles_c) * 64 + (tid & 15) * 4;
                    if (rr >= rows || c >= cols) continue;
                    const int q = cols - c < 4 ? (int)(cols - c) : 4;
                    float pn[4] = {NAN, NAN, NAN, NAN};
                    lamb_apply_piece(p, g, m, v, rr * cols + c, q, vec && q == 4, k, k.lr * r, zero_grad, pn);
                    for (int e = 0; e < q; ++e) pn_all[rr * cols + c + e] = pn[e];
                }
        // the double-precision statement of the same update
        const double lr = hyper[8], b1 = hyper[9], b2 = hyper[10], eps = hyper[11], step = it + 1, clip = optim_clip_coef(norm, max_norm);
        double np2 = 0.0, nu2 = 0.0;
        for (size_t i = 0; i < n; ++i) {
            const double ge = (double)g0[i] * clip;
            dm[i] += (ge - dm[i]) * (1.0 - b1);
            dv[i] = dv[i] * b2 + (1.0 - b2) * ge * ge;
            du[i] = (dm[i] / (1.0 - std::pow(b1, step))) / (std::sqrt(dv[i]) / std::sqrt(1.0 - std::pow(b2, step)) + eps) + (double)wd * dp[i];
            np2 += dp[i] * dp[i]; nu2 += du[i] * du[i];
        }
        double dr = 1.0;
        if (wd != 0.f || always_adapt) {
            dr = (np2 > 0.0 && nu2 > 0.0) ? std::sqrt(np2) / std::sqrt(nu2) : 1.0;
            if (trust_clip && dr > 1.0) dr = 1.0;
        }
        if (!std::isfinite(r) || !close_to(r, dr, 0.0)) ++bad;
        for (size_t i = 0; i < n; ++i) {
            dp[i] -= lr * dr * du[i];
            if (!close_to(m[i], dm[i], ATOL_M) || !close_to(v[i], dv[i], ATOL_V) || !close_to(p[i], dp[i], ATOL_P)) ++bad;
            if (!std::isfinite(p[i]) || memcmp(&pn_all[i], &p[i], 4) != 0) ++bad;
            const float want_g = zero_grad ? 0.f : g0[i];
            if (memcmp(&g[i], &want_g, 4) != 0) ++bad;
        }
    }
    if (fill == ZERO_BOTH && r != 1.0f) ++bad;
    if (fill == ZERO_G && wd != 0.f && !trust_clip && !close_to(r, 1.0 / wd, 0.0)) ++bad;
    printf("[%3lld x %3lld] skew %d wd %-4g adapt %d clip %d fill %d zero %d: r %.7g %s\n", (long long)rows, (long long)cols, skew, wd,
           always_adapt, trust_clip, (int)fill, zero_grad, r, bad ? "MISMATCH" : "ok");
    for (float* b : blocks) free(b);
    return bad ? 1 : 0;
}

int main() {
    int bad = 0, cases = 0;
    const int64_t shapes[][2] = {{65, 67}, {128, 64}, {130, 4}, {1, 1}, {1, 3}, {1, 130}, {8, 12}};
    for (const auto& sh : shapes) {
        bad += run_case(sh[0], sh[1], 0, 0.05f, 0, 0, PLAIN, 1, 3); ++cases;
        bad += run_case(sh[0], sh[1], 1, 0.05f, 0, 0, PLAIN, 0, 2); ++cases;       // odd-word start, gradients kept
        bad += run_case(sh[0], sh[1], 0, 0.f, 0, 0, PLAIN, 1, 2); ++cases;         // no decay: r = 1
        bad += run_case(sh[0], sh[1], 0, 0.f, 1, 0, PLAIN, 1, 2); ++cases;         // always_adapt
        bad += run_case(sh[0], sh[1], 0, 0.05f, 0, 1, PLAIN, 1, 2); ++cases;       // trust_clip
        bad += run_case(sh[0], sh[1], 0, 0.05f, 0, 0, ZERO_P, 1, 2); ++cases;
        bad += run_case(sh[0], sh[1], 0, 0.05f, 0, 0, ZERO_G, 1, 2); ++cases;
        bad += run_case(sh[0], sh[1], 0, 0.05f, 0, 0, ZERO_BOTH, 1, 2); ++cases;
    }
    if (bad) printf("lamb_host_check FAILED: %d of %d cases\n", bad, cases);
    else printf("lamb_host_check ok: %d cases\n", cases);
    return bad ? 1 : 0;
}
