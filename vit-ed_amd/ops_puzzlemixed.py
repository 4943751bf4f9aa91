"""Functional wrapper of the point lookups of the mutual compatibility (csrc/puzzle_compat.hip), re-exported by
``ops``: what the placement loop of a mixed-bag or unknown-dimension puzzle reads of M, fetched on the device.

It is an ``ops`` function in every respect, kept in a module of its own as ``ops_puzzle2`` is: each tensor goes through ``ops._check``
before its pointer reaches ``ops._lib.call``, the launch goes to torch's current stream, nothing synchronises, and everything is
looked up on ``ops`` at call time."""
from __future__ import annotations

import torch

from . import ops as _o

_i32, _f32 = torch.int32, torch.float32


def puzzle_mutual_gather(mutual: torch.Tensor, lookups: torch.Tensor, out: torch.Tensor | None = None,
                         bad: torch.Tensor | None = None) -> torch.Tensor:
    """out[r] = mutual[side, p, q] for lookups int32 [m, 3] = (side, p, q) into a type-1 mutual float32 [4, n, n], or
    mutual[side_p, p, q, side_q] for lookups int32 [m, 4] = (side_p, p, q, side_q) into a type-2 mutual float32 [4, n, n, 4]
    (``vited_puzzle_mutual_gather`` / ``vited_puzzle_mutual_gather2``): the bits of M unchanged.  A lookup outside the tensor leaves
    out[r] as it was and sets bad int32 [1], which the caller zeroes and reads (None: a fresh zero word, not returned)."""
    _o._need_gpu(mutual, lookups, out, bad)
    op = 'puzzle_mutual_gather'
    shape = tuple(getattr(mutual, 'shape', ()))
    if len(shape) not in (3, 4) or shape[1] < 2:
        raise ValueError(f'{op}: mutual must be [4, n, n] or [4, n, n, 4] with n >= 2, got shape {list(shape)}')
    n, dev, width = shape[1], mutual.device, len(shape)
    m = lookups.shape[0] if getattr(lookups, 'dim', lambda: 0)() == 2 else 0
    _o._check(op, 'mutual', mutual, _f32, (4, n, n) if width == 3 else (4, n, n, 4), dev)
    _o._check(op, 'lookups', lookups, _i32, (m, width), dev)
    out = _o._out(op, 'out', out, _f32, (m,), dev)
    if bad is None:
        bad = torch.zeros(1, dtype=_i32, device=dev)
    _o._check(op, 'bad', bad, _i32, (1,), dev)
    _o._lib.call('vited_puzzle_mutual_gather' if width == 3 else 'vited_puzzle_mutual_gather2', _o._ptr(mutual), n, _o._ptr(lookups), m,
                 _o._ptr(out), _o._ptr(bad), _o._stream())
    return out
