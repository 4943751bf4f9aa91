"""Functional wrapper of the learning-rate range test's record (csrc/lr_finder.hip), re-exported by ``ops``, the
same rule restated in numpy for CPU tensors, and the suggestion that is read off the history on the host.

``lr_finder_step`` on CUDA tensors is an ``ops`` function in every respect - each tensor goes through ``ops._check`` before its pointer
reaches ``ops._lib.call``, the launch goes to torch's current stream, nothing synchronises - kept in a module of its own; everything is
looked up on ``ops`` at call time, so whatever replaces the library or the device gate there holds here too.

The rule (csrc/lr_finder.h states it for the kernel), with i the rows written so far:
  rate     iteration i of group g runs at ``start[g] * (end[g] / start[g]) ** (i / num_iter)``
  record   ``s = loss`` for i == 0 or smooth_f == 0, else ``smooth_f * loss + (1 - smooth_f) * s_prev``; ``best`` the smallest s so far;
           history row i = (rate of group 0, loss, s)
  halt     LRF_NONFINITE for a loss that is not finite, else LRF_DIVERGED where ``s > diverge_th * best``, else LRF_DONE where
           ``i + 1 == num_iter``; the row of the halting iteration stays
  words    while running ``fp32(rate of iteration i + 1)`` into every group's rate word; 0.0 once halted, and then nothing else moves"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops as _o

LRF_RUNNING, LRF_DONE, LRF_DIVERGED, LRF_NONFINITE = range(4)                 # the halt states
LRF_ROWS, LRF_STATE, LRF_SMOOTHED, LRF_BEST = range(4)                        # the state words: int64, int64, fp64 bits, fp64 bits
LRF_STATE_WORDS = 4
LRF_HISTORY_COLS = 3
LRF_MAX_GROUPS = 4096
_f32, _f64, _i64 = torch.float32, torch.float64, torch.int64


def lr_finder_rate(start: float, end: float, i: int, num_iter: int) -> float:
    """The rate of iteration i in Python's doubles: exactly ``start`` at i == 0, ``end`` never reached."""
    start, end = float(start), float(end)
    return start * math.pow(end / start, float(i) / float(num_iter))


def _record_numpy(loss, state, history, start, end, num_iter, smooth_f, diverge_th, dst, first, stride):
    """The rule on CPU tensors, in place, word for word what the kernel does."""
    counters = state.numpy()
    stats = state[LRF_SMOOTHED:].view(_f64).numpy()
    hist, words = history.numpy().reshape(-1, LRF_HISTORY_COLS), dst.numpy().reshape(-1)
    starts, ends = start.tolist(), end.tolist()
    at = [first + stride * g for g in range(len(starts))]
    i = int(counters[LRF_ROWS])
    if counters[LRF_STATE] != LRF_RUNNING or not 0 <= i < num_iter:
        words[at] = np.float32(0.0)
        return
    value = float(loss.reshape(-1)[0])
    s = value if i == 0 or smooth_f == 0.0 else smooth_f * value + (1.0 - smooth_f) * float(stats[0])
    best = s if i == 0 or s < float(stats[1]) else float(stats[1])
    if not math.isfinite(value):
        halt = LRF_NONFINITE
    elif s > diverge_th * best:
        halt = LRF_DIVERGED
    else:
        halt = LRF_DONE if i + 1 == num_iter else LRF_RUNNING
    hist[i] = (lr_finder_rate(starts[0], ends[0], i, num_iter), value, s)
    stats[0], stats[1] = s, best
    counters[LRF_ROWS], counters[LRF_STATE] = i + 1, halt
    for w, a, b in zip(at, starts, ends):
        words[w] = np.float32(lr_finder_rate(a, b, i + 1, num_iter)) if halt == LRF_RUNNING else np.float32(0.0)


def lr_finder_step(loss: torch.Tensor, state: torch.Tensor, history: torch.Tensor, start: torch.Tensor, end: torch.Tensor, num_iter: int,
                   smooth_f: float, diverge_th: float, dst: torch.Tensor, first: int, stride: int):
    """One record of the range test (``vited_lr_finder_step``), all on the device, in one launch on the current stream: row
    ``state[0]`` of ``history`` from ``loss``, the smoothed and the best loss, the halt state, and the next iteration's rate into
    ``dst[first + stride * g]`` of every group g - 0.0 once halted, after which only those words are written.  ``loss`` fp32, one
    element; ``state`` int64 [LRF_STATE_WORDS] (words 2 and 3 hold fp64 bits), zero before the first record; ``history`` fp64
    [capacity, 3] with capacity >= num_iter; ``start`` / ``end`` fp64 [groups], positive and finite (the caller's check: they may live on
    the device); ``dst`` a contiguous fp32 buffer that holds the last group's word.  On CPU tensors the same rule runs in numpy."""
    op = 'lr_finder_step'
    num_iter, smooth_f, diverge_th, first, stride = int(num_iter), float(smooth_f), float(diverge_th), int(first), int(stride)
    tensors = (loss, state, history, start, end, dst)
    cpu = all(torch.is_tensor(t) and not t.is_cuda for t in tensors)
    if not cpu:
        _o._need_gpu(*[t for t in tensors if torch.is_tensor(t)])
    dev = next((t.device for t in (dst, state, loss) if torch.is_tensor(t)), None)         # dst's; a missing dst is refused by name below
    _o._check(op, 'loss', loss, _f32, 1, dev)
    _o._check(op, 'state', state, _i64, (LRF_STATE_WORDS,), dev)
    _o._check(op, 'history', history, _f64, (_o._Min(1), LRF_HISTORY_COLS), dev)
    _o._check(op, 'start', start, _f64, (_o._Min(1),), dev)
    groups = start.shape[0]
    _o._check(op, 'end', end, _f64, (groups,), dev, like='start')
    if groups > LRF_MAX_GROUPS or first < 0 or stride < 1:
        raise ValueError(f'{op}: {groups} groups (at most {LRF_MAX_GROUPS}) at word {first} with stride {stride} (>= 0 and >= 1)')
    if not 1 <= num_iter <= history.shape[0]:
        raise ValueError(f'{op}: num_iter {num_iter} is outside [1, {history.shape[0]}], the rows of history')
    if not 0.0 <= smooth_f <= 1.0 or not diverge_th > 1.0:
        raise ValueError(f'{op}: smooth_f {smooth_f} must lie in [0, 1] and diverge_th {diverge_th} above 1')
    _o._check(op, 'dst', dst, _f32, _o._Min(first + stride * (groups - 1) + 1), dev)
    if cpu:
        return _record_numpy(loss, state, history, start, end, num_iter, smooth_f, diverge_th, dst, first, stride)
    _o._lib.call('vited_lr_finder_step', _o._ptr(loss), _o._ptr(state), _o._ptr(history), history.shape[0], _o._ptr(start), _o._ptr(end),
                 groups, num_iter, smooth_f, diverge_th, _o._ptr(dst), dst.numel(), first, stride, _o._stream())


def lr_suggestion(lrs, smoothed, skip_start: int = 0, skip_end: int = 0) -> float:
    """The rate at the steepest descent of the smoothed loss (FastaiLRFinder.lr_suggestion): after ``skip_start`` leading and
    ``skip_end`` trailing rows are dropped, ``d_k = s_k - s_{k-1}`` for k = 1 .. rows - 1, and the answer is the rate of the first k with
    the smallest ``d_k``.  Fewer than two rows left raise ValueError."""
    skip_start, skip_end = int(skip_start), int(skip_end)
    if skip_start < 0 or skip_end < 0:
        raise ValueError(f'lr_suggestion: skip_start {skip_start} and skip_end {skip_end} must not be negative')
    lrs, smoothed = np.asarray(lrs, dtype=np.float64).reshape(-1), np.asarray(smoothed, dtype=np.float64).reshape(-1)
    if lrs.shape != smoothed.shape:
        raise ValueError(f'lr_suggestion: {lrs.shape[0]} rates for {smoothed.shape[0]} losses')
    stop = lrs.shape[0] - skip_end
    lrs, smoothed = lrs[skip_start:stop], smoothed[skip_start:stop]
    if lrs.shape[0] < 2:
        raise ValueError(f'lr_suggestion: {lrs.shape[0]} rows are left, the steepest descent needs two')
    return float(lrs[int(np.argmin(smoothed[1:] - smoothed[:-1])) + 1])
