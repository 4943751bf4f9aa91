// Host build of the update bodies of vited_adamw_step / vited_sgd_step (csrc/optim_update.h) for the address and undefined-behaviour
// sanitizers: the very text the HIP kernels run, driven piece by piece the way optim_update_kernel drives it (64 x 64 tiles, 4
// columns per thread, the same tail and alignment rules) over exactly-sized heap buffers, and compared element by element with a
// plain double-precision loop.  Cases: AdamW; SGD with Nesterov, with plain momentum and with momentum 0 (buffer absent, and present
// but NaN-filled: it must be neither read nor written); an update that is skipped (everything but g keeps its bits) and one that is
// not; a parameter that starts on an odd word (no 16-byte accesses).
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vit-ed_amd/csrc tools/optim_host_check.cpp -o optim_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "optim_update.h"

enum Kind { ADAMW, SGD_NESTEROV, SGD_MOMENTUM, SGD_PLAIN_NOBUF, SGD_PLAIN_NANBUF };
static const char* kind_name[] = {"adamw", "sgd nesterov 0.9", "sgd momentum 0.9", "sgd momentum 0 (no buffer)", "sgd momentum 0 (NaN buffer)"};

static unsigned rng_state = 2463534242u;
static float rnd() {                                   // uniform in [-1, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)((int)(rng_state >> 8) % 20001 - 10000) / 10000.0f;
}

// rtol 1e-5 plus an absolute term for cancelled values: a few fp32 roundings (2^-24 relative each) of the largest operand, which is
// ~1 for the momentum buffer (gradients up to 0.3, 1 / (1 - 0.9) of them at most), 0.09 for exp_avg_sq and 0.1 for a parameter
static const double ATOL_M = 5e-7, ATOL_V = 1e-8, ATOL_P = 2e-6;
static bool close_to(float got, double want, double atol) { return std::fabs((double)got - want) <= atol + 1e-5 * std::fabs(want); }

static int run_case(Kind kind, int64_t rows, int64_t cols, int skew, float norm, float flag, int zero_grad, int steps) {
    const size_t n = (size_t)(rows * cols);
    const bool adam = kind == ADAMW, has_buf = kind != SGD_PLAIN_NOBUF;
    std::vector<float*> blocks;
    // exactly n floats each, ending at the end of the allocation (ASan's redzone follows the last element)
    auto exact = [&](bool present) -> float* {
        if (!present) return nullptr;
        // malloc's 16-byte aligned start + skew words; the allocation ends right behind element n - 1
        char* raw = (char*)malloc(n * 4 + (size_t)skew * 4);
        blocks.push_back((float*)raw);
        return (float*)raw + skew;
    };
    float *p = exact(true), *g = exact(true), *m = exact(has_buf), *v = exact(adam);
    std::vector<double> dp(n), dg(n), dm(n), dv(n);
    std::vector<float> p0(n), m0(n), v0(n);
    for (size_t i = 0; i < n; ++i) {
        p[i] = 0.1f * rnd();
        if (m) m[i] = kind == SGD_PLAIN_NANBUF ? NAN : (steps ? 0.f : 0.01f * rnd());
        if (v) v[i] = steps ? 0.f : 1e-4f * std::fabs(rnd());
        dp[i] = p[i]; dm[i] = (m && kind != SGD_PLAIN_NANBUF) ? m[i] : 0.0; dv[i] = v ? v[i] : 0.0;
    }
    float hyper[16] = {0.f, flag, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, /* group 0 */ 2e-3f, 0.f, 0.f, 0.f, 0.05f, 0.f, 0.f, 0.f};
    if (adam) { hyper[9] = 0.9f; hyper[10] = 0.98f; hyper[11] = 1e-8f; }
    else { hyper[9] = (kind == SGD_NESTEROV || kind == SGD_MOMENTUM) ? 0.9f : 0.f; hyper[10] = kind == SGD_NESTEROV ? 1.f : 0.f; }
    const float max_norm = 1.0f;
    int bad = 0;
    const int rounds = steps ? steps : 1;
    double applied_total = 0, skipped_total = 0;
    for (int it = 0; it < rounds; ++it) {
        for (size_t i = 0; i < n; ++i) { g[i] = 0.3f * rnd(); dg[i] = g[i]; p0[i] = p[i]; if (m) m0[i] = m[i]; if (v) v0[i] = v[i]; }
        float res[4] = {NAN, NAN, NAN, NAN};
        optim_decide(norm, max_norm, hyper, res);
        const bool applied = res[2] != 0.f;
        const bool want_applied = !(flag != 0.f && !std::isfinite(norm));
        applied_total += want_applied; skipped_total += !want_applied;
        if (applied != want_applied || hyper[0] != (float)applied_total || hyper[2] != (float)skipped_total || res[3] != hyper[0]
            || memcmp(&res[0], &norm, 4) != 0)
            ++bad;
        AdamWCoef ka = {};
        SgdCoef ks = {};
        if (adam) ka = adamw_coef(hyper + 8, res[3]);
        else ks = sgd_coef(hyper + 8);
        uintptr_t ptrs = (uintptr_t)p | (uintptr_t)g;
        if (adam) ptrs |= (uintptr_t)m | (uintptr_t)v;
        else if (ks.momentum != 0.f) ptrs |= (uintptr_t)m;
        const bool vec = (cols & 3) == 0 && (ptrs & 15) == 0;
        std::vector<float> pn_all(n, NAN);
        const int64_t tiles_r = (rows + 63) / 64, tiles_c = (cols + 63) / 64;
        for (int64_t t = 0; t < tiles_r * tiles_c; ++t)            // the kernel's grid: one workgroup per tile, 256 threads, 4 pieces each
            for (int tid = 0; tid < 256; ++tid)
                for (int j = 0; j < 4; ++j) {
                    const int64_t r = (t / tiles_c) * 64 + (tid >> 4) + 16 * j, c = (t % tiles_c) * 64 + (tid & 15) * 4;
                    if (r >= rows || c >= cols) continue;
                    const int k = cols - c < 4 ? (int)(cols - c) : 4;
                    float pn[4] = {NAN, NAN, NAN, NAN};
                    if (!applied) skipped_piece(g, r * cols + c, k, vec && k == 4, zero_grad);
                    else if (adam) adamw_piece(p, g, m, v, r * cols + c, k, vec && k == 4, ka, res[1], zero_grad, pn);
                    else sgd_piece(p, g, m, r * cols + c, k, vec && k == 4, ks, res[1], zero_grad, pn);
                    for (int e = 0; e < k; ++e) pn_all[r * cols + c + e] = pn[e];
                }
        // the double-precision statement of the same update
        const double lr = hyper[8], wd = hyper[12], clip = want_applied ? (double)optim_clip_coef(norm, max_norm) : 0.0;
        for (size_t i = 0; i < n; ++i) {
            if (!want_applied) {
                if (memcmp(&p[i], &p0[i], 4) || (m && memcmp(&m[i], &m0[i], 4)) || (v && memcmp(&v[i], &v0[i], 4))) ++bad;
                if (g[i] != (zero_grad ? 0.f : (float)dg[i])) ++bad;
                continue;
            }
            double ge = dg[i] * clip;
            if (adam) {
                const double b1 = hyper[9], b2 = hyper[10], eps = hyper[11], step = applied_total;
                dp[i] *= 1.0 - lr * wd;
                dm[i] += (ge - dm[i]) * (1.0 - b1);
                dv[i] = dv[i] * b2 + (1.0 - b2) * ge * ge;
                dp[i] -= lr / (1.0 - std::pow(b1, step)) * dm[i] / (std::sqrt(dv[i]) / std::sqrt(1.0 - std::pow(b2, step)) + eps);
                if (!close_to(m[i], dm[i], ATOL_M) || !close_to(v[i], dv[i], ATOL_V)) ++bad;
            } else {
                const double mom = hyper[9];
                ge += wd * dp[i];
                double d = ge;
                if (mom != 0.0) {
                    dm[i] = mom * dm[i] + ge;
                    d = hyper[10] != 0.f ? ge + mom * dm[i] : dm[i];
                    if (!close_to(m[i], dm[i], ATOL_M)) ++bad;
                } else if (m && memcmp(&m[i], &m0[i], 4)) ++bad;          // the NaN-filled buffer keeps its bits
                dp[i] -= lr * d;
            }
            if (!close_to(p[i], dp[i], ATOL_P) || memcmp(&pn_all[i], &p[i], 4) != 0) ++bad;
            if (g[i] != (zero_grad ? 0.f : (float)dg[i])) ++bad;
        }
    }
    printf("%-30s [%3lld x %3lld] skew %d norm %-4g flag %g zero %d x%d: %s\n", kind_name[kind], (long long)rows, (long long)cols, skew,
           norm, flag, zero_grad, rounds, bad ? "MISMATCH" : "ok");
    for (float* b : blocks) free(b);
    return bad ? 1 : 0;
}

int main() {
    int bad = 0, cases = 0;
    const int64_t shapes[][2] = {{65, 130}, {4, 384}, {1, 1}, {100, 36}, {7, 3}, {1, 384}};
    for (int kind = ADAMW; kind <= SGD_PLAIN_NANBUF; ++kind)
        for (const auto& sh : shapes) {
            bad += run_case((Kind)kind, sh[0], sh[1], 0, 0.5f, 0.f, 1, 3); ++cases;        // no clip, three updates from a zero state
            bad += run_case((Kind)kind, sh[0], sh[1], 0, 7.0f, 1.f, 1, 0); ++cases;        // clip active, flag set, warm state
            bad += run_case((Kind)kind, sh[0], sh[1], 1, 7.0f, 1.f, 0, 0); ++cases;        // odd-word start, gradients kept
            bad += run_case((Kind)kind, sh[0], sh[1], 0, NAN, 1.f, 1, 0); ++cases;         // skipped: NaN norm
            bad += run_case((Kind)kind, sh[0], sh[1], 1, INFINITY, 1.f, 1, 0); ++cases;    // skipped: inf norm, odd-word start
            bad += run_case((Kind)kind, sh[0], sh[1], 0, INFINITY, 1.f, 0, 0); ++cases;    // skipped, gradients kept: nothing is written
        }
    if (bad) printf("optim_host_check FAILED: %d of %d cases\n", bad, cases);
    else printf("optim_host_check ok: %d cases\n", cases);
    return bad ? 1 : 0;
}
