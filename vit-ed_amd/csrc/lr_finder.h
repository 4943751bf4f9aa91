// The learning-rate range test (the reference's lr_finder.py over ignite's FastaiLRFinder) in fp64 as plain C++:
// the same text runs in the one-workgroup kernel of lr_finder.hip and in the host program under the sanitizers
// (tools/lrfinder_host_check.cpp).  Compile with -ffp-contract=off: the numpy statement (ops_lrfinder.py) multiplies and adds separately.
//
// Rate.    Iteration i (0-based) of group g runs at  start_g * (end_g / start_g) ** (i / num_iter):  exactly start_g at i = 0, end_g
//          approached and never reached.
// Record.  Once per iteration, on the loss of the iteration that just ran:
//            s_0 = loss_0;  s_i = smooth_f * loss_i + (1 - smooth_f) * s_{i-1}   (smooth_f == 0: s_i = loss_i, the raw loss)
//            best = s_0, then best = s_i where s_i < best
//          history row i = (lr_i of group 0, loss_i, s_i)
// Halt.    After the row, in this order: a loss that is not finite -> LRF_NONFINITE;  s_i > diverge_th * best -> LRF_DIVERGED;
//          i + 1 == num_iter -> LRF_DONE.  While running every group's rate word receives (float)lr_{i+1}(g); a halted test writes 0.0f
//          and touches neither the history nor the state again.
//
// The state is LRF_STATE_WORDS 8-byte words: [LRF_ROWS] int64 rows written (the index of the next iteration), [LRF_STATE] int64 halt
// state, [LRF_SMOOTHED] fp64 s of the last row, [LRF_BEST] fp64 best.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LRF_FN __host__ __device__ inline
#else
#define LRF_FN inline
#endif

#define LRF_RUNNING 0
#define LRF_DONE 1
#define LRF_DIVERGED 2
#define LRF_NONFINITE 3

#define LRF_ROWS 0
#define LRF_STATE 1
#define LRF_SMOOTHED 2
#define LRF_BEST 3
#define LRF_STATE_WORDS 4
#define LRF_HISTORY_COLS 3
#define LRF_MAX_GROUPS 4096             // parameter groups one launch serves

struct LrfDecision {
    double smoothed, best;
    int64_t state;
};

// the rate of iteration i
LRF_FN double lr_finder_rate(double start, double end, int64_t i, int64_t num_iter) {
    return start * pow(end / start, (double)i / (double)num_iter);
}

// what the record of iteration i decides from the loss and the statistics behind row i - 1 (not read for i == 0)
LRF_FN LrfDecision lr_finder_decide(double loss, int64_t i, double s_prev, double best_prev, int64_t num_iter, double smooth_f,
                                    double diverge_th) {
    LrfDecision d;
    if (i == 0 || smooth_f == 0.0) d.smoothed = loss;
    else d.smoothed = smooth_f * loss + (1.0 - smooth_f) * s_prev;
    d.best = (i == 0 || d.smoothed < best_prev) ? d.smoothed : best_prev;
    if (!(fabs(loss) <= DBL_MAX)) d.state = LRF_NONFINITE;            // inf or NaN
    else if (d.smoothed > diverge_th * d.best) d.state = LRF_DIVERGED;
    else if (i + 1 == num_iter) d.state = LRF_DONE;
    else d.state = LRF_RUNNING;
    return d;
}

// whether a launch may still record: running, and the next row lies inside the sweep (a state somebody scribbled over records nothing)
LRF_FN bool lr_finder_live(int64_t rows, int64_t state, int64_t num_iter) {
    return state == LRF_RUNNING && rows >= 0 && rows < num_iter;
}

// one lane's share of the rate words: (float)lr_next(g) while running, 0.0f once halted
LRF_FN void lr_finder_write_rates(int lane, int lanes, bool running, int64_t next, int64_t num_iter, const double* start, const double* end,
                                  int groups, float* dst, int64_t first, int64_t stride) {
    for (int g = lane; g < groups; g += lanes)
        dst[first + stride * g] = running ? (float)lr_finder_rate(start[g], end[g], next, num_iter) : 0.0f;
}

// row i of the history and the state behind it: one lane's work
LRF_FN void lr_finder_commit(int64_t i, double loss, const LrfDecision& d, int64_t* counters, double* stats, double* history, double start0,
                             double end0, int64_t num_iter) {
    double* row = history + LRF_HISTORY_COLS * i;
    row[0] = lr_finder_rate(start0, end0, i, num_iter);
    row[1] = loss;
    row[2] = d.smoothed;
    stats[0] = d.smoothed;
    stats[1] = d.best;
    counters[LRF_ROWS] = i + 1;
    counters[LRF_STATE] = d.state;
}
