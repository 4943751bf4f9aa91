// Host build of the parameter-EMA rule of csrc/optim_update.h (ema_decay_at, ema_blend, ema_decide, ema_piece, swap_piece) for the
// address and undefined-behaviour sanitizers: the very text the HIP kernels run.
//   * the rule against the literal cases of tests/test_ema.py: the warmup crossover for d = 0.5 (d_t reaches d at n = 8) and for
//     d = 0.9999 (near n = 89990), the blend bit for bit against two products rounded through volatile floats (no fma), and 50 updates
//     of random data against d*e + (1-d)*p in double at rtol 1e-6;
//   * ema_piece behind adamw_piece / sgd_piece (momentum 0.9 with Nesterov, and momentum 0 without a buffer) and swap_piece, driven
//     piece by piece the way the update kernel drives them (64 x 64 tiles, 4 columns per thread, the same tail and alignment rules)
//     over exactly-sized heap buffers; a skipped update leaves the average and the counter alone; two swaps restore every bit.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vit-ed_amd/csrc tools/ema_host_check.cpp -o ema_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "optim_update.h"

static unsigned rng_state = 88172645u;
static float rnd() {                                   // uniform in [-1, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)((int)(rng_state >> 8) % 20001 - 10000) / 10000.0f;
}

static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

// fl(fl(dt * e) + fl((1 - dt) * p)) with every intermediate forced through memory
static float blend_rounded(float dt, float e, float p) {
    volatile float keep = dt * e;
    volatile float rest = 1.0f - dt;
    volatile float take = rest * p;
    volatile float sum = keep + take;
    return sum;
}

static int check_rule() {
    int bad = 0;
    // d = 0.5: (1 + n) / (10 + n) < 0.5 for n < 8, = 0.5 at n = 8
    for (int n = 0; n < 8; ++n) {
        const float want = (1.0f + (float)n) / (10.0f + (float)n);
        if (!same_bits(ema_decay_at(0.5f, 1.f, (float)n), want) || !(want < 0.5f)) ++bad;
    }
    if (!same_bits(ema_decay_at(0.5f, 1.f, 7.f), 8.0f / 17.0f)) ++bad;
    const float later[] = {8.f, 9.f, 100.f, 1e6f};
    for (float n : later)
        if (!same_bits(ema_decay_at(0.5f, 1.f, n), 0.5f)) ++bad;
    if (!same_bits(ema_decay_at(0.5f, 0.f, 0.f), 0.5f)) ++bad;
    // d = 0.9999: the ramp starts at 0.1, is below d at n = 80000 and has reached it within 60 updates of n = 89990
    const float d = 0.9999f;
    if (!same_bits(ema_decay_at(d, 1.f, 0.f), 1.0f / 10.0f) || !(ema_decay_at(d, 1.f, 80000.f) < d)) ++bad;
    int first = -1;
    for (int n = 80000; n < 100000 && first < 0; ++n)
        if (same_bits(ema_decay_at(d, 1.f, (float)n), d)) first = n;
    if (first < 0 || std::abs(first - 89990) > 60) ++bad;
    const float after[] = {(float)first, (float)first + 1.f, 95000.f, 1e7f};
    for (float n : after)
        if (!same_bits(ema_decay_at(d, 1.f, n), d)) ++bad;
    // the blend: bit for bit two rounded products and a rounded sum; 50 updates against double
    const float decays[] = {0.9999f, 0.99f, 0.5f, 0.0f};
    for (int k = 0; k < 4; ++k) {
        const float warm = (k == 1 || k == 2) ? 1.f : 0.f;
        std::vector<float> e(1024);
        std::vector<double> e64(1024);
        for (size_t i = 0; i < e.size(); ++i) { e[i] = rnd(); e64[i] = e[i]; }
        float hyper[8] = {0.f, 0.f, 0.f, decays[k], warm, 0.f, 0.f, 0.f};
        for (int it = 0; it < 50; ++it) {
            ema_decide(true, hyper);
            const float dt = ema_decay_now(hyper);
            if (!same_bits(dt, ema_decay_at(decays[k], warm, (float)it))) ++bad;
            for (size_t i = 0; i < e.size(); ++i) {
                const float p = rnd();
                const float got = ema_blend(dt, e[i], p);
                if (!same_bits(got, blend_rounded(dt, e[i], p))) ++bad;
                e64[i] = (double)dt * e64[i] + (1.0 - (double)dt) * (double)p;
                if (std::fabs((double)got - e64[i]) > 1e-6 + 1e-6 * std::fabs(e64[i])) ++bad;
                e[i] = got;
            }
        }
        ema_decide(false, hyper);                       // a skipped update does not count
        if (hyper[OPTIM_EMA_COUNT] != 50.f) ++bad;
    }
    printf("%-44s %s\n", "rule: crossover, blend, 50 updates", bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}

enum Kind { ADAMW, SGD_NESTEROV, SGD_PLAIN_NOBUF, SWAP };
static const char* kind_name[] = {"adamw + ema", "sgd nesterov 0.9 + ema", "sgd momentum 0 (no buffer) + ema", "swap"};

static int run_case(Kind kind, int64_t rows, int64_t cols, int skew, float norm, float warm) {
    const size_t n = (size_t)(rows * cols);
    std::vector<float*> blocks;
    // exactly n floats, ending at the end of the allocation (ASan's redzone follows the last element); skew: an odd-word start
    auto exact = [&](bool present) -> float* {
        if (!present) return nullptr;
        char* raw = (char*)malloc(n * 4 + (size_t)skew * 4);
        blocks.push_back((float*)raw);
        return (float*)raw + skew;
    };
    float *p = exact(true), *g = exact(true), *m = exact(kind == ADAMW || kind == SGD_NESTEROV), *v = exact(kind == ADAMW), *e = exact(true);
    for (size_t i = 0; i < n; ++i) {
        p[i] = 0.1f * rnd(); g[i] = 0.3f * rnd(); e[i] = kind == SWAP ? 0.1f * rnd() : p[i];
        if (m) m[i] = 0.f;
        if (v) v[i] = 0.f;
    }
    float hyper[16] = {0.f, 1.f, 0.f, 0.99f, warm, 0.f, 0.f, 0.f, /* group 0 */ 2e-3f, 0.f, 0.f, 0.f, 0.05f, 0.f, 0.f, 0.f};
    if (kind == ADAMW) { hyper[9] = 0.9f; hyper[10] = 0.98f; hyper[11] = 1e-8f; }
    else if (kind == SGD_NESTEROV) { hyper[9] = 0.9f; hyper[10] = 1.f; }
    int bad = 0;
    const int rounds = kind == SWAP ? 2 : 3;
    std::vector<float> p_first(p, p + n), e_first(e, e + n);
    for (int it = 0; it < rounds; ++it) {
        std::vector<float> e0(e, e + n), p0(p, p + n), pn_all(n, NAN);
        float res[4] = {NAN, NAN, 1.f, NAN};
        bool applied = true;
        float dt = 0.f;
        const float count0 = hyper[OPTIM_EMA_COUNT];
        if (kind != SWAP) {
            for (size_t i = 0; i < n; ++i) g[i] = 0.3f * rnd();
            optim_decide(norm, 1.0f, hyper, res);
            applied = res[2] != 0.f;
            ema_decide(applied, hyper);
            if (hyper[OPTIM_EMA_COUNT] != count0 + (applied ? 1.f : 0.f)) ++bad;
            if (applied) dt = ema_decay_now(hyper);
            if (applied && !same_bits(dt, ema_decay_at(0.99f, warm, count0))) ++bad;
        }
        AdamWCoef ka = {};
        SgdCoef ks = {};
        if (kind == ADAMW) ka = adamw_coef(hyper + 8, res[3]);
        else if (kind != SWAP) ks = sgd_coef(hyper + 8);
        uintptr_t ptrs = (uintptr_t)p | (uintptr_t)g | (uintptr_t)e;
        if (kind == ADAMW) ptrs |= (uintptr_t)m | (uintptr_t)v;
        else if (kind != SWAP && ks.momentum != 0.f) ptrs |= (uintptr_t)m;
        const bool vec = (cols & 3) == 0 && (ptrs & 15) == 0;
        const int64_t tiles_r = (rows + 63) / 64, tiles_c = (cols + 63) / 64;
        for (int64_t t = 0; t < tiles_r * tiles_c; ++t)            // the kernel's grid: one workgroup per tile, 256 threads, 4 pieces each
            for (int tid = 0; tid < 256; ++tid)
                for (int j = 0; j < 4; ++j) {
                    const int64_t r = (t / tiles_c) * 64 + (tid >> 4) + 16 * j, c = (t % tiles_c) * 64 + (tid & 15) * 4;
                    if (r >= rows || c >= cols) continue;
                    const int k = cols - c < 4 ? (int)(cols - c) : 4;
                    const int64_t o = r * cols + c;
                    float pn[4] = {NAN, NAN, NAN, NAN};
                    if (!applied) { skipped_piece(g, o, k, vec && k == 4, 1); continue; }
                    if (kind == ADAMW) adamw_piece(p, g, m, v, o, k, vec && k == 4, ka, res[1], 1, pn);
                    else if (kind == SWAP) swap_piece(p, e, o, k, vec && k == 4, pn);
                    else sgd_piece(p, g, m, o, k, vec && k == 4, ks, res[1], 1, pn);
                    if (kind != SWAP) ema_piece(e, o, k, vec && k == 4, dt, pn);
                    for (int q = 0; q < k; ++q) pn_all[o + q] = pn[q];
                }
        for (size_t i = 0; i < n; ++i) {
            if (!applied) {
                if (!same_bits(e[i], e0[i]) || !same_bits(p[i], p0[i])) ++bad;
            } else if (kind == SWAP) {
                if (!same_bits(p[i], e0[i]) || !same_bits(e[i], p0[i]) || !same_bits(pn_all[i], p[i])) ++bad;
            } else {
                if (!same_bits(pn_all[i], p[i]) || !same_bits(e[i], blend_rounded(dt, e0[i], p[i]))) ++bad;
            }
        }
    }
    if (kind == SWAP)
        for (size_t i = 0; i < n; ++i)
            if (!same_bits(p[i], p_first[i]) || !same_bits(e[i], e_first[i])) ++bad;
    printf("%-34s [%3lld x %3lld] skew %d norm %-4g warmup %g: %s\n", kind_name[kind], (long long)rows, (long long)cols, skew, norm, warm,
           bad ? "MISMATCH" : "ok");
    for (float* b : blocks) free(b);
    return bad ? 1 : 0;
}

int main() {
    int bad = check_rule(), cases = 1;
    // the parameter set of tests/ema_cases.py ([n] is one row of n columns, as the optimizers lay a 1-D parameter out)
    const int64_t shapes[][2] = {{1, 1}, {1, 65}, {64, 64}, {65, 63}, {130, 70}};
    for (int kind = ADAMW; kind <= SWAP; ++kind)
        for (const auto& sh : shapes) {
            bad += run_case((Kind)kind, sh[0], sh[1], 0, 0.5f, 0.f); ++cases;              // no clip
            bad += run_case((Kind)kind, sh[0], sh[1], 0, 7.0f, 1.f); ++cases;              // clip active, warmup
            bad += run_case((Kind)kind, sh[0], sh[1], 1, 7.0f, 1.f); ++cases;              // odd-word start: no 16-byte accesses
            if (kind != SWAP) { bad += run_case((Kind)kind, sh[0], sh[1], 0, INFINITY, 1.f); ++cases; }   // skipped: e and n stay
        }
    if (bad) printf("ema_host_check FAILED: %d of %d cases\n", bad, cases);
    else printf("ema_host_check ok: %d cases\n", cases);
    return bad ? 1 : 0;
}
