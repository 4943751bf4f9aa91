// Host build of Lion's update body (csrc/optim_update.h: lion_coef, lion_sign, lion_piece) for the address and undefined-behaviour
// sanitizers: the very text the HIP kernel runs, one 4-element piece at a time over exactly-sized heap blocks (a piece of n elements
// lies at the end of its allocation, so one element too many is a heap overflow), compared bit for bit with a second, scalar statement
// of the rule whose every intermediate is a volatile float - so nothing in it can be contracted either.  Cases: n = 1..4, the 16-byte
// path (n = 4, aligned) and the element path (n = 4 aligned, n = 4 from an odd word, n < 4), a piece behind four untouched elements,
// with and without decay, gradients zeroed and kept, p = 0, g = 0 with zero state (the parameter only decays), p = 0 and g = 0 (stays
// exactly 0).  Three updates each, the clip active in the second.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I vit-ed_amd/csrc tools/lion_host_check.cpp -o lion_host_check
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

static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

// The rule once more, one rounded operation per line.
static void scalar_rule(float p, float g, float m, float clip, float lr, float b1, float b2, float wd, float* p_out, float* m_out) {
    volatile float gc = g * clip;
    volatile float lw = lr * wd;
    volatile float decay = 1.0f - lw;
    volatile float pe = p * decay;
    volatile float keep = b1 * m;
    volatile float omb1 = 1.0f - b1;
    volatile float take = omb1 * gc;
    volatile float cc = keep + take;
    volatile float s = cc > 0.f ? 1.0f : (cc < 0.f ? -1.0f : 0.f);
    volatile float ls = lr * s;
    *p_out = pe - ls;
    volatile float diff = gc - m;
    volatile float omb2 = 1.0f - b2;
    volatile float scaled = diff * omb2;
    *m_out = m + scaled;
}

enum Fill { PLAIN, ZERO_P, ZERO_G, ZERO_BOTH };

// A piece of n elements at offset `lead` of blocks of exactly lead + n floats that start `skew` words behind a 16-byte boundary.
static int run_case(int n, bool wide, int skew, int lead, float wd, Fill fill, int zero_grad) {
    const size_t len = (size_t)(lead + n);
    std::vector<char*> blocks;
    auto exact = [&]() -> float* {
        char* raw = (char*)malloc((len + (size_t)skew) * 4);
        blocks.push_back(raw);
        return (float*)raw + skew;
    };
    float *p = exact(), *g = exact(), *m = exact();
    std::vector<float> rp(len), rm(len, 0.f), rg(len);
    for (size_t i = 0; i < len; ++i) {
        p[i] = (fill == ZERO_P || fill == ZERO_BOTH) ? 0.f : 0.1f * rnd();
        m[i] = 0.f;
        rp[i] = p[i];
    }
    float hyper[16] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, /* group 0 */ 2e-3f, 0.9f, 0.98f, 0.f, wd, 0.f, 0.f, 0.f};
    int bad = 0;
    if (wide && (n != 4 || ((((uintptr_t)(p + lead)) | ((uintptr_t)(g + lead)) | ((uintptr_t)(m + lead))) & 15) != 0)) ++bad;   // the case table's own error
    for (int it = 0; it < 3 && !bad; ++it) {
        for (size_t i = 0; i < len; ++i) rg[i] = g[i] = (fill == ZERO_G || fill == ZERO_BOTH) ? 0.f : 0.3f * rnd();
        float res[4];
        optim_decide(it == 1 ? 7.0f : 0.5f, 1.0f, hyper, res);
        const LionCoef k = lion_coef(hyper + 8);
        float pn[4] = {NAN, NAN, NAN, NAN};
        lion_piece(p, g, m, lead, n, wide, k, res[1], zero_grad, pn);
        for (int e = 0; e < n; ++e) {
            const size_t i = (size_t)lead + e;
            float wp, wm;
            scalar_rule(rp[i], rg[i], rm[i], res[1], hyper[8], hyper[9], hyper[10], wd, &wp, &wm);
            if (fill == ZERO_G || fill == ZERO_BOTH) {                // no gradient, no moment: the parameter only decays
                volatile float lw = hyper[8] * wd;
                volatile float decay = 1.0f - lw;
                volatile float only = rp[i] * decay;
                if (!same_bits(wp, only) || wm != 0.f) ++bad;
            }
            if (wd == 0.f) {                                          // without decay the step is exactly +lr, -lr or 0
                volatile float up = rp[i] + hyper[8], down = rp[i] - hyper[8];
                if (!same_bits(wp, up) && !same_bits(wp, down) && !same_bits(wp, rp[i])) ++bad;
            }
            rp[i] = wp; rm[i] = wm;
            if (!same_bits(p[i], wp) || !same_bits(m[i], wm) || !same_bits(pn[e], wp) || !std::isfinite(p[i])) ++bad;
            if (!same_bits(g[i], zero_grad ? 0.f : rg[i])) ++bad;
            if (fill == ZERO_BOTH && !same_bits(p[i], 0.f)) ++bad;
        }
        for (int i = 0; i < lead; ++i)                                // what lies in front of the piece is not the piece's
            if (!same_bits(p[i], rp[i]) || !same_bits(m[i], 0.f) || !same_bits(g[i], rg[i])) ++bad;
    }
    if (bad)
        printf("n %d wide %d skew %d lead %d wd %g fill %d zero %d: MISMATCH\n", n, (int)wide, skew, lead, wd, (int)fill, zero_grad);
    for (char* b : blocks) free(b);
    return bad ? 1 : 0;
}

int main() {
    int bad = 0, cases = 0;
    const Fill fills[] = {PLAIN, ZERO_P, ZERO_G, ZERO_BOTH};
    const float decays[] = {0.05f, 0.f};
    for (Fill fill : fills)
        for (float wd : decays)
            for (int zero_grad = 0; zero_grad < 2; ++zero_grad) {
                for (int n = 1; n <= 4; ++n)
                    for (int skew = 0; skew < 2; ++skew) { bad += run_case(n, false, skew, 0, wd, fill, zero_grad); ++cases; }
                bad += run_case(4, true, 0, 0, wd, fill, zero_grad); ++cases;       // the 16-byte path
                bad += run_case(4, true, 0, 4, wd, fill, zero_grad); ++cases;       // ... behind four elements that are not its own
                bad += run_case(3, false, 0, 4, wd, fill, zero_grad); ++cases;      // a row's tail
            }
    // the sign: +1, -1, 0 for either zero, NaN for NaN
    if (lion_sign(3.f) != 1.f || lion_sign(-1e-30f) != -1.f || !same_bits(lion_sign(0.f), 0.f) || !same_bits(lion_sign(-0.f), 0.f) ||
        !std::isnan(lion_sign(NAN))) ++bad;
    ++cases;
    if (bad) printf("lion_host_check FAILED: %d of %d cases\n", bad, cases);
    else printf("lion_host_check ok: %d cases\n", cases);
    return bad ? 1 : 0;
}
