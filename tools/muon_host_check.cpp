// Host build of Muon's elementwise bodies (csrc/muon_update.h: muon_coef, muon_moments_piece, muon_denom, muon_pack_piece,
// muon_apply_piece, the bf16 bit conversions and the two epilogue expressions) for the address and undefined-behaviour sanitizers: the
// very text the HIP kernels run, driven the way vited_muon_step's elementwise launches drive it (64 x 64 tiles, 4 columns per thread,
// the same tail and alignment rules; per-tile sums, then the tensor's denominator, then the pack pass into an exactly-sized padded image
// in p's orientation, then the apply pass reading O from it) and compared with a plain double-precision loop.  The transposed image is
// NOT covered here: its indexing is muon_pack_kernel's LDS tile in muon.hip, not a body of muon_update.h, and is held by the GPU tests
// alone (tall tensors (72, 16), (128, 64), (130, 4), whose X is the transposed image, and every wide tensor's B X, which reads it).
// The Newton-Schulz products are not part of this program: O is the packed X itself (zero steps).  Cases: wide, tall, tails in both
// dimensions, nesterov on and off, both adjust modes, an odd-word start (no 16-byte accesses), gradients kept (their bits must
// stay), u = 0 (denominator eps, nothing non-finite).
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vit-ed_amd/csrc tools/muon_host_check.cpp -o muon_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "muon_update.h"

static unsigned rng_state = 2463534242u;
static float rnd() {                                   // uniform in [-1, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)((int)(rng_state >> 8) % 20001 - 10000) / 10000.0f;
}

static bool close_to(double got, double want, double atol, double rtol) { return std::fabs(got - want) <= atol + rtol * std::fabs(want); }

static int run_case(int64_t rows, int64_t cols, int skew, int nesterov, int adjust, int zero_g, int zero_grad, int steps) {
    const size_t n = (size_t)(rows * cols);
    std::vector<char*> blocks;
    auto exact = [&](size_t bytes, int sk) -> char* {   // exactly `bytes`, ending at the end of the allocation
        char* raw = (char*)malloc(bytes + (size_t)sk * 4);
        blocks.push_back(raw);
        return raw + sk * 4;
    };
    float *p = (float*)exact(n * 4, skew), *g = (float*)exact(n * 4, skew), *buf = (float*)exact(n * 4, skew);
    const int64_t rp = muon_pad(rows), cp = muon_pad(cols);
    uint16_t* straight = (uint16_t*)exact((size_t)(rp * cp) * 2, 0);      // [rp, cp]: p's orientation
    memset(straight, 0xff, (size_t)(rp * cp) * 2);                        // NaN patterns: the pack pass must overwrite every element
    std::vector<double> dp(n), db(n, 0.0), du(n);
    for (size_t i = 0; i < n; ++i) { p[i] = 0.1f * rnd(); buf[i] = 0.f; dp[i] = p[i]; }
    float hyper[16] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, /* Muon group */ 2e-3f, 0.95f, (float)nesterov, 1e-7f, 0.05f, (float)adjust,
                       1.f, 0.f};
    const float max_norm = 1.0f;
    int bad = 0;
    for (int it = 0; it < steps; ++it) {
        std::vector<float> g0(n);
        for (size_t i = 0; i < n; ++i) g0[i] = g[i] = zero_g ? 0.f : 0.3f * rnd();
        const float norm = it == 1 ? 7.0f : 0.5f;       // the clip is active in the second update
        float res[4];
        optim_decide(norm, max_norm, hyper, res);
        const MuonCoef k = muon_coef(hyper + 8, rows, cols);
        const bool vec = (cols & 3) == 0 && (((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) == 0;
        const int64_t tiles_r = (rows + 63) / 64, tiles_c = (cols + 63) / 64;
        float sum_u = 0.f;
        for (int64_t t = 0; t < tiles_r * tiles_c; ++t) {           // the moments pass
            float tile_u = 0.f;
            for (int tid = 0; tid < 256; ++tid) {
                float su = 0.f;
                for (int j = 0; j < 4; ++j) {
                    const int64_t rr = (t / tiles_c) * 64 + (tid >> 4) + 16 * j, c = (t % tiles_c) * 64 + (tid & 15) * 4;
                    if (rr >= rows || c >= cols) continue;
                    const int q = cols - c < 4 ? (int)(cols - c) : 4;
                    muon_moments_piece(g, buf, rr * cols + c, q, vec && q == 4, k, res[1], &su);
                }
                tile_u += su;
            }
            sum_u += tile_u;
        }
        const float denom = muon_denom(sum_u, k);                    // one wave per tensor
        for (int64_t t = 0; t < tiles_r * tiles_c; ++t)              // the pack pass: the whole padded tile
            for (int tid = 0; tid < 256; ++tid)
                for (int j = 0; j < 4; ++j) {
                    const int64_t rr = (t / tiles_c) * 64 + (tid >> 4) + 16 * j, c = (t % tiles_c) * 64 + (tid & 15) * 4;
                    uint16_t x[4] = {0, 0, 0, 0};
                    if (rr < rows && c < cols) {
                        const int q = cols - c < 4 ? (int)(cols - c) : 4;
                        muon_pack_piece(g, buf, rr * cols + c, q, vec && q == 4, k, res[1], denom, x);
                    }
                    for (int e = 0; e < 4; ++e) straight[rr * cp + c + e] = x[e];
                }
        // the double-precision statement of momentum and normalisation
        const double clip = optim_clip_coef(norm, max_norm), mom = hyper[9];
        double nu2 = 0.0;
        for (size_t i = 0; i < n; ++i) {
            const double ge = (double)g0[i] * clip;
            db[i] += (ge - db[i]) * (1.0 - mom);
            du[i] = nesterov ? ge + (db[i] - ge) * mom : db[i];
            nu2 += du[i] * du[i];
        }
        const double dden = std::sqrt(nu2) > (double)hyper[11] ? std::sqrt(nu2) : (double)hyper[11];
        if (!close_to(denom, dden, 0.0, 1e-5)) ++bad;
        for (int64_t rr = 0; rr < rp; ++rr)
            for (int64_t c = 0; c < cp; ++c) {
                const uint16_t s = straight[rr * cp + c];
                if (rr >= rows || c >= cols) { if (s != 0) ++bad; continue; }
                const double want = du[rr * cols + c] / dden;
                if (!close_to(muon_bf16_value(s), want, 1e-9, 1.0 / 256 + 1e-4)) ++bad;      // half an ulp of bf16 is 2^-9 of the value
                if (!close_to(buf[rr * cols + c], db[rr * cols + c], 1e-8, 1e-5)) ++bad;
            }
        std::vector<float> pn_all(n, NAN);
        for (int64_t t = 0; t < tiles_r * tiles_c; ++t)              // the apply pass, O = the packed image
            for (int tid = 0; tid < 256; ++tid)
                for (int j = 0; j < 4; ++j) {
                    const int64_t rr = (t / tiles_c) * 64 + (tid >> 4) + 16 * j, c = (t % tiles_c) * 64 + (tid & 15) * 4;
                    if (rr >= rows || c >= cols) continue;
                    const int q = cols - c < 4 ? (int)(cols - c) : 4;
                    float pn[4] = {NAN, NAN, NAN, NAN};
                    uint16_t ob[4];
                    memcpy(ob, straight + rr * cp + c, 8);
                    muon_apply_piece(p, g, ob, rr * cols + c, q, vec && q == 4, k, zero_grad, pn);
                    for (int e = 0; e < q; ++e) pn_all[rr * cols + c + e] = pn[e];
                }
        const double lr = hyper[8], wd = hyper[12];
        const double adj = adjust ? 0.2 * std::sqrt((double)(rows > cols ? rows : cols)) : std::sqrt(rows > cols ? (double)rows / (double)cols : 1.0);
        for (size_t i = 0; i < n; ++i) {
            const double o = muon_bf16_value(straight[(i / cols) * cp + (i % cols)]);
            dp[i] = dp[i] * (1.0 - lr * wd) - lr * adj * o;
            if (!close_to(p[i], dp[i], 2e-6, 1e-5)) ++bad;
            if (!std::isfinite(p[i]) || memcmp(&pn_all[i], &p[i], 4) != 0) ++bad;
            const float want_g = zero_grad ? 0.f : g0[i];
            if (memcmp(&g[i], &want_g, 4) != 0) ++bad;
        }
    }
    printf("[%3lld x %3lld] skew %d nesterov %d adjust %d zero_g %d zero %d: %s\n", (long long)rows, (long long)cols, skew, nesterov, adjust,
           zero_g, zero_grad, bad ? "MISMATCH" : "ok");
    for (char* b : blocks) free(b);
    return bad ? 1 : 0;
}

static int check_scalars() {
    int bad = 0;
    // round to nearest even on the 16 dropped bits, ties included; the values survive the round trip
    const float one_plus_half_ulp = 1.0f + 1.0f / 256, one_plus_three_half_ulp = 1.0f + 3.0f / 256;
    if (muon_bf16_bits(1.0f) != 0x3f80 || muon_bf16_bits(one_plus_half_ulp) != 0x3f80 || muon_bf16_bits(one_plus_three_half_ulp) != 0x3f82) ++bad;
    if (muon_bf16_bits(-0.69140625f) != 0xbf31 || muon_bf16_value(0xbf31) != -0.69140625f) ++bad;
    if (muon_bf16_bits(0.f) != 0 || !std::isnan(muon_bf16_value(muon_bf16_bits(NAN)))) ++bad;
    // separate rounded operations: fl(fl(b A) + fl(c S)) and fl(fl(a X) + T)
    const float b = -4.7750f, c = 2.0315f, a = 3.4445f, A = 0.015625f, S = 0.000244140625f, X = 0.125f, T = -0.07177734375f;
    const float pb = b * A, pc = c * S, pa = a * X;
    if (muon_ns_poly(b, A, c, S) != pb + pc || muon_ns_next(a, X, T) != pa + T) ++bad;
    printf("scalars: %s\n", bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}

int main() {
    int bad = check_scalars(), cases = 1;
    const int64_t shapes[][2] = {{65, 67}, {128, 64}, {130, 4}, {4, 6}, {16, 40}, {72, 16}, {1, 3}};
    for (const auto& sh : shapes) {
        bad += run_case(sh[0], sh[1], 0, 1, 0, 0, 1, 3); ++cases;
        bad += run_case(sh[0], sh[1], 1, 1, 0, 0, 0, 2); ++cases;       // odd-word start, gradients kept
        bad += run_case(sh[0], sh[1], 0, 0, 1, 0, 1, 2); ++cases;       // plain momentum, match_rms_adamw
        bad += run_case(sh[0], sh[1], 0, 1, 1, 1, 1, 2); ++cases;       // u = 0
    }
    if (bad) printf("muon_host_check FAILED: %d of %d cases\n", bad, cases);
    else printf("muon_host_check ok: %d cases\n", cases);
    return bad ? 1 : 0;
}
