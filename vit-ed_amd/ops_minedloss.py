"""Functional wrapper of the fused mined-pair loss (csrc/mined_bce.hip).

``mined_bce`` is an ``ops`` function in every respect - each tensor goes through ``ops._check`` before its pointer reaches
``ops._lib.call``, the launch goes to torch's current stream, nothing synchronises - kept in a module of its own; everything is looked
up on ``ops`` at call time, so whatever replaces the library or the device gate there holds here too."""
from __future__ import annotations

import math

import torch

from . import ops as _o

MINED_BCE_MAX_CLASSES = 64
_f32, _i32 = torch.float32, torch.int32


def mined_bce(logits: torch.Tensor, labels: torch.Tensor, weights: torch.Tensor, counts: torch.Tensor, reduction: str = 'mean',
              scale: float = 1.0):
    """BCE-with-logits over a mined pair list and its gradient in one launch (``vited_mined_bce``; include/vited.h states the rule):
    ``logits`` fp32 [R, C] with dense rows (1 <= R <= ``ops.MINE_MAX_CAPACITY``, 1 <= C <= 64), ``labels`` / ``weights`` fp32 [R, 1] and
    ``counts`` int32 [5] as ``MinedPairs`` holds them.  Returns (loss fp32 [1], dlogits fp32 [R, C]), every element written:
    loss = scale * sum(w * term) / denom and dlogits = scale * w * (sigmoid(x) - y) / denom, with denom = max(counts[3], 1) * C for
    'mean' (read on the device) and 1 for 'sum'; a row of weight 0 gives exact zeros whatever its logit holds.  Bitwise reproducible.
    Raises before anything is launched, every message beginning with ``mined_bce: ``."""
    op = 'mined_bce'
    if reduction not in ('mean', 'sum'):
        raise ValueError(f"{op}: reduction must be 'mean' or 'sum', got {reduction!r}")
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError(f'{op}: scale must be a finite number, got {scale}')
    dev = logits.device if torch.is_tensor(logits) else None
    _o._check(op, 'logits', logits, _f32, (_o._Min(1), _o._Min(1)), dev)
    rows, classes = logits.shape
    if rows > _o.MINE_MAX_CAPACITY or classes > MINED_BCE_MAX_CLASSES:
        raise ValueError(f'{op}: logits [{rows}, {classes}]: at most {_o.MINE_MAX_CAPACITY} rows (the largest mining capacity) of at most '
                         f'{MINED_BCE_MAX_CLASSES} outputs')
    _o._check(op, 'labels', labels, _f32, (rows, 1), dev, like='logits')
    _o._check(op, 'weights', weights, _f32, (rows, 1), dev, like='logits')
    _o._check(op, 'counts', counts, _i32, (5,), dev)
    try:
        _o._need_gpu(logits)
    except RuntimeError as err:
        raise RuntimeError(f'{op}: {err}') from None
    loss = torch.empty(1, dtype=_f32, device=dev)
    dlogits = torch.empty((rows, classes), dtype=_f32, device=dev)
    _o._lib.call('vited_mined_bce', _o._ptr(logits), _o._ptr(labels), _o._ptr(weights), _o._ptr(counts), rows, classes,
                 int(reduction == 'mean'), scale, _o._ptr(loss), _o._ptr(dlogits), _o._stream())
    return loss, dlogits
