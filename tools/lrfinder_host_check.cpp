// Host check of csrc/lr_finder.h: the text the one-workgroup kernel of lr_finder.hip runs, driven here over scripted loss sequences
// exactly as the kernel drives it (one lane), checked against a second, scalar statement of the same arithmetic and printed as bits, so
// that a test can compare them with the numpy statement (tests/test_lr_finder.py) - same libm, same operation order.  A stand-alone
// program with its own main; build it with
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I vit-ed_amd/csrc
// The state, the history, the sweep's ends and the rate words live in exactly-sized heap buffers, so a row behind the last one or a
// word behind the last group's is reported.
//
// Input (argv[1]), one case per line:
//   num_iter  extra  smooth_f  diverge_th  groups  {start end} x groups  losses  {loss} x losses
// doubles as 16-digit and losses (fp32) as 8-digit hex bit patterns, the rest decimal; every loss is one launch, `extra` more launches
// follow on the last loss (they may move nothing but the rate words once the test has halted).
// Output per case:  "case rows state smoothed best", one "w" line per launch with every group's rate word, one "h" line per row.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "lr_finder.h"

static const int64_t FIRST = 8, STRIDE = 8;      // the optimizers' hyper array
static const uint32_t SENTINEL = 0x7fc12345u;    // every word of it that is no rate word

template <class T, class U>
static T bits_to(U u) {
    static_assert(sizeof(T) == sizeof(U), "same size");
    T t;
    memcpy(&t, &u, sizeof t);
    return t;
}

// a word of the state as bits, whichever kind it is
static uint64_t word(const int64_t* state, int w) {
    uint64_t u;
    memcpy(&u, reinterpret_cast<const char*>(state) + 8 * w, 8);
    return u;
}

// one launch as lr_finder_step_kernel makes it, with one lane
static void launch(const float* loss_ptr, int64_t* state, double* history, const double* start, const double* end, int groups,
                   int64_t num_iter, double smooth_f, double diverge_th, float* dst) {
    double* stats = reinterpret_cast<double*>(state + LRF_SMOOTHED);
    const int64_t i = state[LRF_ROWS];
    if (!lr_finder_live(i, state[LRF_STATE], num_iter)) {
        lr_finder_write_rates(0, 1, false, 0, num_iter, start, end, groups, dst, FIRST, STRIDE);
        return;
    }
    const double loss = (double)*loss_ptr;
    const LrfDecision d = lr_finder_decide(loss, i, stats[0], stats[1], num_iter, smooth_f, diverge_th);
    lr_finder_commit(i, loss, d, state, stats, history, start[0], end[0], num_iter);
    lr_finder_write_rates(0, 1, d.state == LRF_RUNNING, i + 1, num_iter, start, end, groups, dst, FIRST, STRIDE);
}

// the second statement: scalars only, no buffers
struct Scalar {
    int64_t rows = 0, state = 0;
    double s = 0.0, best = 0.0;
    bool record(double loss, int64_t num_iter, double f, double th) {       // whether this call recorded a row
        if (state != 0 || rows >= num_iter) return false;
        if (rows == 0) s = best = loss;
        else {
            s = f == 0.0 ? loss : f * loss + (1.0 - f) * s;
            if (s < best) best = s;
        }
        ++rows;
        if (isnan(loss) || isinf(loss)) state = 3;
        else if (s > th * best) state = 2;
        else if (rows == num_iter) state = 1;
        return true;
    }
};

static int fail(long c, const char* what) {
    fprintf(stderr, "case %ld: %s\n", c, what);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    long cases = 0;
    for (;; ++cases) {
        int64_t num_iter = 0, extra = 0, groups = 0, count = 0;
        uint64_t fb = 0, tb = 0;
        if (fscanf(f, "%" SCNd64, &num_iter) != 1) break;
        if (fscanf(f, "%" SCNd64 " %" SCNx64 " %" SCNx64 " %" SCNd64, &extra, &fb, &tb, &groups) != 4 || num_iter < 1 || extra < 0 ||
            groups < 1 || groups > LRF_MAX_GROUPS)
            return fail(cases, "bad header");
        const double smooth_f = bits_to<double>(fb), diverge_th = bits_to<double>(tb);
        std::unique_ptr<double[]> start(new double[groups]), end(new double[groups]);
        for (int64_t g = 0; g < groups; ++g) {
            uint64_t a = 0, b = 0;
            if (fscanf(f, "%" SCNx64 " %" SCNx64, &a, &b) != 2) return fail(cases, "incomplete ends");
            start[g] = bits_to<double>(a);
            end[g] = bits_to<double>(b);
        }
        if (fscanf(f, "%" SCNd64, &count) != 1 || count < 1) return fail(cases, "no losses");
        std::unique_ptr<float[]> losses(new float[count]);
        for (int64_t k = 0; k < count; ++k) {
            uint32_t u = 0;
            if (fscanf(f, "%" SCNx32, &u) != 1) return fail(cases, "incomplete losses");
            losses[k] = bits_to<float>(u);
        }
        // exactly-sized buffers; the state comes from malloc, which gives storage without a declared type for its two kinds of word
        int64_t* state = static_cast<int64_t*>(calloc(LRF_STATE_WORDS, 8));
        std::unique_ptr<double[]> history(new double[LRF_HISTORY_COLS * num_iter]);
        const int64_t words = FIRST + STRIDE * (groups - 1) + 1;
        std::unique_ptr<float[]> dst(new float[words]);
        if (!state) return fail(cases, "out of memory");
        for (int64_t k = 0; k < LRF_HISTORY_COLS * num_iter; ++k) history[k] = -1.0;
        for (int64_t w = 0; w < words; ++w) dst[w] = bits_to<float>(SENTINEL);
        Scalar ref;
        std::vector<uint32_t> lines;
        for (int64_t k = 0; k < count + extra; ++k) {
            const float* loss = &losses[k < count ? k : count - 1];
            const int64_t row = state[LRF_ROWS];
            uint64_t was[LRF_STATE_WORDS];
            memcpy(was, state, sizeof was);
            launch(loss, state, history.get(), start.get(), end.get(), (int)groups, num_iter, smooth_f, diverge_th, dst.get());
            const bool recorded = ref.record((double)*loss, num_iter, smooth_f, diverge_th);
            if (!recorded && memcmp(was, state, sizeof was)) return fail(cases, "a halted launch moved the state");
            if (state[LRF_ROWS] != ref.rows || state[LRF_STATE] != ref.state) return fail(cases, "rows or state differ from the scalar form");
            const double s = bits_to<double>(word(state, LRF_SMOOTHED)), best = bits_to<double>(word(state, LRF_BEST));
            if (ref.rows && (memcmp(&s, &ref.s, 8) || memcmp(&best, &ref.best, 8))) return fail(cases, "statistics differ from the scalar form");
            if (recorded) {
                const double want[3] = {start[0] * pow(end[0] / start[0], (double)row / (double)num_iter), (double)*loss, ref.s};
                if (memcmp(&history[LRF_HISTORY_COLS * row], want, sizeof want)) return fail(cases, "history row differs from the scalar form");
            }
            for (int64_t w = 0; w < words; ++w) {
                const bool rate = w >= FIRST && (w - FIRST) % STRIDE == 0;
                if (!rate) {
                    if (bits_to<uint32_t>(dst[w]) != SENTINEL) return fail(cases, "a word that is no rate word moved");
                    continue;
                }
                const int64_t g = (w - FIRST) / STRIDE;
                const float want = ref.state == 0 ? (float)(start[g] * pow(end[g] / start[g], (double)ref.rows / (double)num_iter)) : 0.0f;
                if (memcmp(&dst[w], &want, 4)) return fail(cases, "rate word differs from the scalar form");
                lines.push_back(bits_to<uint32_t>(dst[w]));
            }
        }
        printf("case %" PRId64 " %" PRId64 " %016" PRIx64 " %016" PRIx64 "\n", state[LRF_ROWS], state[LRF_STATE],
               word(state, LRF_SMOOTHED), word(state, LRF_BEST));
        for (int64_t k = 0; k < count + extra; ++k) {
            printf("w");
            for (int64_t g = 0; g < groups; ++g) printf(" %08" PRIx32, lines[k * groups + g]);
            printf("\n");
        }
        for (int64_t r = 0; r < state[LRF_ROWS]; ++r)
            printf("h %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits_to<uint64_t>(history[3 * r]), bits_to<uint64_t>(history[3 * r + 1]),
                   bits_to<uint64_t>(history[3 * r + 2]));
        free(state);
    }
    fclose(f);
    printf("lrfinder_host_check ok: %ld cases\n", cases);
    return 0;
}
