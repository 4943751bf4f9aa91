"""Functional wrapper of the exchange of parameters and their moving averages (``vited_ema_swap``, csrc/optimizer.hip; DESIGN.md
section 39).

``ema_swap`` is an ``ops`` function in every respect - each tensor goes through ``ops._check`` before its pointer reaches
``ops._lib.call``, the launch goes to torch's current stream, nothing synchronises - kept in a module of its own; everything is looked
up on ``ops`` at call time, so whatever replaces the library or the device gate there holds here too.  The update entries that keep
the average (``vited_adamw_step_ema`` / ``vited_sgd_step_ema``) are called by ``optim.py``, beside the entries without it."""
from __future__ import annotations

import torch

from . import ops as _o

_f32, _i64 = torch.float32, torch.int64


def ema_swap(desc: torch.Tensor, total_tiles: int, ema: torch.Tensor, grad_flat: torch.Tensor):
    """p <-> its slice of ``ema`` for every row of ``desc`` (the int64 [count, 10] descriptor table of the fused optimizers, whose
    gradient pointers lie in ``grad_flat``), and the rows' bf16 shadows rewritten from the value now in p.  ``ema`` fp32, as long as
    ``grad_flat`` and 16-byte aligned.  One launch; calling it twice restores every bit.  Raises before anything is launched, every
    message beginning with ``ema_swap: ``."""
    op = 'ema_swap'
    _o._need_gpu(desc, ema, grad_flat)
    dev = grad_flat.device
    _o._check(op, 'desc', desc, _i64, (_o._Min(1), 10), dev)
    _o._check(op, 'grad_flat', grad_flat, _f32, _o._Min(1), dev)
    _o._check(op, 'ema', ema, _f32, grad_flat.numel(), dev, like='grad_flat')
    if _o._ptr(ema) % 16:
        raise ValueError(f'{op}: ema must be 16-byte aligned')
    if not 1 <= int(total_tiles) <= 0x7fffffff:
        raise ValueError(f'{op}: total_tiles must lie in [1, 2^31), got {total_tiles}')
    _o._lib.call('vited_ema_swap', _o._ptr(desc), desc.shape[0], int(total_tiles), _o._ptr(ema), _o._ptr(grad_flat), _o._stream())
