"""Functional wrapper of the device-stepped learning-rate schedule (csrc/lr_schedule.hip) and the layout of
its rule table (csrc/lr_schedule.h).

``lr_schedule_step`` is an ``ops`` function in every respect - each tensor goes through ``ops._check`` before its pointer reaches
``ops._lib.call``, the launch goes to torch's current stream, nothing synchronises - kept in a module of its own; everything is looked
up on ``ops`` at call time, so whatever replaces the library or the device gate there holds here too."""
from __future__ import annotations

import torch

from . import ops as _o

# the words of the fp64 rule table (the LRS_* of csrc/lr_schedule.h)
(LR_KIND, LR_WARMUP_T, LR_WARMUP_LR_INIT, LR_T_INITIAL, LR_LR_MIN, LR_CYCLE_LIMIT, LR_WARMUP_PREFIX, LR_LR_MIN_RATE, LR_DECAY_T,
 LR_DECAY_RATE, LR_GAMMA, LR_MILESTONES, LR_FIRST_MILESTONE) = range(13)
LR_MAX_MILESTONES = 32
LR_TABLE_WORDS = LR_FIRST_MILESTONE + LR_MAX_MILESTONES
LR_MAX_GROUPS = 4096
_f32, _f64, _i64 = torch.float32, torch.float64, torch.int64


def lr_schedule_step(table: torch.Tensor, base: torch.Tensor, scale: torch.Tensor, counter: torch.Tensor, dst: torch.Tensor, first: int,
                     stride: int, last_lr: torch.Tensor | None = None):
    """One schedule step (``vited_lr_schedule_step``): with t = counter[0], ``dst[first + stride * g] = fp32(rule(table, base[g], t) *
    scale[g])`` for every group g, the same values into ``last_lr`` when given, then ``counter[0] = t + 1`` - all on the device, in one
    launch on the current stream.  ``table`` fp64 [LR_TABLE_WORDS], ``base`` / ``scale`` fp64 [groups], ``counter`` int64 [1], ``dst``
    a contiguous fp32 buffer that holds the last group's word, ``last_lr`` fp32 [groups] apart from ``dst``."""
    op = 'lr_schedule_step'
    _o._need_gpu(table, base, scale, counter, dst, last_lr)
    dev = next((t.device for t in (dst, table, counter) if torch.is_tensor(t)), None)      # dst's; a missing dst is refused by name below
    _o._check(op, 'table', table, _f64, (LR_TABLE_WORDS,), dev)
    _o._check(op, 'base', base, _f64, (_o._Min(1),), dev)
    groups = base.shape[0]
    _o._check(op, 'scale', scale, _f64, (groups,), dev, like='base')
    _o._check(op, 'counter', counter, _i64, 1, dev)
    first, stride = int(first), int(stride)
    if groups > LR_MAX_GROUPS or first < 0 or stride < 1:
        raise ValueError(f'{op}: {groups} groups (at most {LR_MAX_GROUPS}) at word {first} with stride {stride} (>= 0 and >= 1)')
    _o._check(op, 'dst', dst, _f32, _o._Min(first + stride * (groups - 1) + 1), dev)
    _o._check(op, 'last_lr', last_lr, _f32, (groups,), dev, optional=True, like='base')
    _o._lib.call('vited_lr_schedule_step', _o._ptr(table), _o._ptr(base), _o._ptr(scale), groups, _o._ptr(counter), _o._ptr(dst),
                 dst.numel(), first, stride, _o._ptr(last_lr), _o._stream())
