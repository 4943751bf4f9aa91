"""The learning-rate range test's rule (csrc/lr_finder.h) written out in numpy, the scripted loss sequences with
their hand-written answers, and the seeded random ones: shared by tests/test_lr_finder.py (CPU) and tests/test_gpu_lr_finder.py.

Rate of iteration i:  start * (end / start) ** (i / num_iter).  Record of iteration i: s = loss for i == 0 or smooth_f == 0, else
smooth_f * loss + (1 - smooth_f) * s_prev; best the smallest s so far; row i = (rate of group 0, loss, s).  Halt, after the row: a loss
that is not finite -> 3; s > diverge_th * best -> 2; i + 1 == num_iter -> 1.  Rate words: fp32(rate of i + 1) while running, 0 after."""
import math
import struct

import numpy as np

RUNNING, DONE, DIVERGED, NONFINITE = range(4)
HEADER, WORDS = 8, 8                     # the optimizers' hyper array: 8 header words, 8 per group, the rate first
NAN, INF = float('nan'), float('inf')


def rate(start, end, i, num_iter):
    """Python's doubles and libm's pow, which the host program shares; numpy's own pow is a vectorised one, an ulp off here and there."""
    start, end = float(start), float(end)
    return np.float64(start * math.pow(end / start, float(i) / float(num_iter)))


def run(case, launches=None):
    """The rule over ``case['losses']`` (rounded to fp32 first: the kernel reads an fp32 loss), one launch per loss and ``case['extra']``
    more on the last one.  Returns {'history': fp64 [rows, 3], 'rows', 'state', 'smoothed', 'best', 'words': per launch the fp64 value
    whose fp32 rounding every group's rate word holds (0.0 once halted)}."""
    losses = [np.float64(np.float32(v)) for v in case['losses']]
    losses += [losses[-1]] * case.get('extra', 0)
    num_iter, f, th = case['num_iter'], np.float64(case['smooth_f']), np.float64(case['diverge_th'])
    rows, state, s, best, history, words = 0, RUNNING, np.float64(0), np.float64(0), [], []
    for loss in losses[:launches]:
        if state == RUNNING and rows < num_iter:
            if rows == 0 or f == 0:
                s = loss
            else:
                s = f * loss + (np.float64(1) - f) * s
            best = s if rows == 0 or s < best else best
            history.append((rate(case['start'][0], case['end'][0], rows, num_iter), loss, s))
            rows += 1
            if not np.isfinite(loss):
                state = NONFINITE
            elif s > th * best:
                state = DIVERGED
            elif rows == num_iter:
                state = DONE
        words.append([rate(a, b, rows, num_iter) if state == RUNNING else np.float64(0) for a, b in zip(case['start'], case['end'])])
    return dict(history=np.array(history, dtype=np.float64).reshape(-1, 3), rows=rows, state=state, smoothed=s, best=best, words=words)


def _case(id, losses, num_iter, smooth_f=0.05, diverge_th=5.0, start=(1e-7,), end=(1e-2,), extra=0, **want):
    return dict(id=id, losses=list(losses), num_iter=num_iter, smooth_f=smooth_f, diverge_th=diverge_th, start=list(start), end=list(end),
                extra=extra, want=want)


# Hand-written answers: every number below is exact in binary, worked out on paper from the rule.
CASES = [
    # 4, 3, 2, 1 at smooth_f 1/2: 4; (3 + 4) / 2; (2 + 3.5) / 2; (1 + 2.75) / 2.  The last row reaches num_iter.
    _case('monotone', [4, 3, 2, 1], 4, smooth_f=0.5, start=(1.0,), end=(16.0,), rows=4, state=DONE, smoothed=[4, 3.5, 2.75, 1.875],
          best=1.875, lrs=[1, 2, 4, 8]),
    # 1, 1, 8: s_2 = (8 + 1) / 2 = 4.5 > 2 * 1 halts at row 2; the fourth loss and two more launches record nothing
    _case('diverges_at_row_2', [1, 1, 8, 100], 6, smooth_f=0.5, diverge_th=2.0, extra=2, rows=3, state=DIVERGED, smoothed=[1, 1, 4.5],
          best=1.0),
    # exactly at the threshold is not above it: s_1 = (5 + 1) / 2 = 3 = 3 * 1 goes on, s_2 = (5 + 3) / 2 = 4 > 3 halts
    _case('threshold_is_strict', [1, 5, 5, 5], 8, smooth_f=0.5, diverge_th=3.0, rows=3, state=DIVERGED, smoothed=[1, 3, 4], best=1.0),
    _case('nan_at_row_3', [2, 2, 2, NAN, 1], 8, smooth_f=0.5, extra=1, rows=4, state=NONFINITE, smoothed=[2, 2, 2, NAN], best=2.0),
    _case('inf_at_row_0', [INF, 1], 8, rows=1, state=NONFINITE, smoothed=[INF], best=INF),
    _case('num_iter_reached', [3, 3, 3, 3, 3], 3, smooth_f=0.25, extra=1, rows=3, state=DONE, smoothed=[3, 3, 3], best=3.0),
    _case('loader_ran_out', [3, 2], 5, smooth_f=0.5, rows=2, state=RUNNING, smoothed=[3, 2.5], best=2.5),
    # smooth_f 0 records the raw loss; 1 does too (1 * loss + 0 * s_prev)
    _case('smooth_f_0', [4, 1, 2, 9], 8, smooth_f=0.0, diverge_th=4.0, rows=4, state=DIVERGED, smoothed=[4, 1, 2, 9], best=1.0),
    _case('smooth_f_1', [4, 1, 2, 9], 8, smooth_f=1.0, diverge_th=4.0, rows=4, state=DIVERGED, smoothed=[4, 1, 2, 9], best=1.0),
    # two groups, the second with lr_scale 1/2: 1 -> 16 and 0.5 -> 8 over 4 iterations
    _case('two_groups', [4, 4, 4, 4], 4, smooth_f=0.5, start=(1.0, 0.5), end=(16.0, 8.0), rows=4, state=DONE, smoothed=[4, 4, 4, 4],
          best=4.0, lrs=[1, 2, 4, 8], words=[[2, 1], [4, 2], [8, 4], [0, 0]]),
    _case('one_iteration', [0.7], 1, rows=1, state=DONE, best=float(np.float32(0.7))),
]
BY_ID = {c['id']: c for c in CASES}


def random_cases(count=64, seed=1234):
    """Seeded sequences of 1 to 24 losses: drifting positive losses that now and then take off or turn non-finite, 1 to 3 groups, every
    kind of smooth_f, a sweep that is sometimes shorter than the sequence."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = int(rng.integers(1, 25))
        losses = np.exp(rng.normal(0.0, 0.3, n)).cumprod() * rng.uniform(0.1, 3.0)
        if rng.random() < 0.5 and n > 3:
            at = int(rng.integers(2, n))
            losses[at:] *= np.exp(np.arange(n - at) * rng.uniform(0.5, 3.0))
        if rng.random() < 0.2:
            losses[int(rng.integers(0, n))] = [NAN, INF, -INF][int(rng.integers(0, 3))]
        groups = int(rng.integers(1, 4))
        start = 10.0 ** rng.uniform(-8, -4, groups)
        end = start * 10.0 ** rng.uniform(1, 6, groups)
        out.append(_case(f'random{k}', losses.tolist(), int(rng.integers(max(1, n - 4), n + 5)),
                         smooth_f=float([0.0, 1.0, 0.05, rng.uniform(0, 1)][int(rng.integers(0, 4))]),
                         diverge_th=float(rng.uniform(1.5, 6.0)), start=start.tolist(), end=end.tolist(), extra=int(rng.integers(0, 3))))
    return out


def bits64(v):
    return struct.unpack('<Q', struct.pack('<d', float(v)))[0]


def bits32(v):
    return struct.unpack('<I', struct.pack('<f', float(np.float32(v))))[0]


def ulps64(a, b):
    """The distance of two finite positive doubles in units of the last place."""
    return abs(bits64(a) - bits64(b))


def fp32_matches(got, want64):
    """The device's fp64 pow is a few fp64 ulp off libm's, which can only move a value across an fp32 rounding boundary: the word is
    numpy's value rounded to fp32 or its neighbour (the allowance of tests/test_gpu_lr_scheduler.py for the pow branch)."""
    want = np.float32(want64)
    return np.float32(got) in (want, np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(-np.inf)))
