"""Functional wrappers of the learned type-2 puzzle entry points (pieces turned by quarter turns under the pair model:
csrc/puzzle_turn.hip, csrc/puzzle_compat.hip), re-exported by ``ops``: the patch extraction of a turned image and
the scatter of a turned pair's four logits into Dq2.

They are ``ops`` functions in every respect, kept in a module of their own as ``ops_puzzle2`` is: each tensor goes through
``ops._check`` before its pointer reaches ``ops._lib.call``, the launch goes to torch's current stream, and everything is looked up on
``ops`` at call time.  A turn k in 0..3 is k clockwise quarter turns, ``torch.rot90(x, -k, (-2, -1))``; an integer turn never
synchronises, a tensor of turns is read back once to be refused when a value lies outside 0..3."""
from __future__ import annotations

import ctypes as C

import torch

from . import ops as _o
from . import ops_puzzlepixels as _pp

_i32, _i64, _u8, _f32 = torch.int32, torch.int64, torch.uint8, torch.float32


def _turns(op, turn, batch, dev):
    """(turn int32 [batch] on ``dev`` | None, the turn of every image) of ``turn``: an int 0..3, or an int32 / int64 tensor [batch]."""
    if torch.is_tensor(turn):
        _o._check(op, 'turn', turn, (_i32, _i64), (batch,), dev, None)
        if batch and bool(((turn < 0) | (turn > 3)).any()):
            raise ValueError(f'{op}: turn must hold quarter turns 0..3, got {int(turn.min())} .. {int(turn.max())}')
        return turn.to(_i32).contiguous(), 0
    if isinstance(turn, bool) or not isinstance(turn, int) or not 0 <= turn <= 3:
        raise ValueError(f'{op}: turn must be a quarter turn 0..3 or an int tensor [{batch}] of them, got {turn!r}')
    return None, turn


def patchify_turned(img: torch.Tensor, patch: int, dtype: torch.dtype, turn, batch_index: torch.Tensor | None = None,
                    mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)) -> torch.Tensor:
    """``ops.patchify(torch.rot90(img, -k, (2, 3)), ...)`` bit for bit, gathered from the upright ``img`` (``vited_patchify_turned`` /
    ``_u8``): img uint8 / fp32 [B, C, S, S] (any batch stride, dense [C, S, S]) -> [nb * (S/p)^2, C*p*p].  ``turn``: an int 0..3 for
    every image, or an int tensor [nb] with one turn per OUTPUT image (nb = B, or the length of ``batch_index``)."""
    _o._need_gpu(img, batch_index, turn if torch.is_tensor(turn) else None)
    op = 'patchify_turned'
    dev = getattr(img, 'device', None)
    _o._check(op, 'img', img, (_u8, _f32), (None, None, None, None), dev, None)
    if img.stride()[1:] != (img.shape[2] * img.shape[3], img.shape[3], 1):
        img = img.contiguous()
    _o._check(op, 'img', img, (_u8, _f32), (None, None) + tuple(img.shape[2:3]) * 2, dev, _o.DENSE_ITEMS)     # [B, C, S, S]
    b, c, s, _ = img.shape
    _o._check(op, 'batch_index', batch_index, _i64, None, dev, optional=True)
    nb = b if batch_index is None else batch_index.numel()
    if not isinstance(patch, int) or patch < 1 or s % patch:
        raise ValueError(f'{op}: img is {s} x {s}, which {patch} x {patch} patches do not tile')
    if nb < 1:
        raise ValueError(f'{op}: img must hold at least one image, got {nb}')
    turns, turn_all = _turns(op, turn, nb, dev)
    g = s // patch
    out = torch.empty((nb * g * g, c * patch * patch), dtype=dtype, device=dev)
    if img.dtype == _u8:
        if not 1 <= c <= 4:
            raise ValueError(f'{op}: img of uint8 must have 1..4 channels, got {c}')
        mean, std = ([float(v) for v in list(t)[:c]] for t in (mean, std))
        _o._lib.call('vited_patchify_turned_u8', _o._ptr(img), img.stride(0), _o._ptr(batch_index), _o._ptr(turns), turn_all, _o._ptr(out),
                     _o._code(dtype), nb, c, s, patch, _o._host_array(C.c_float, mean, c), _o._host_array(C.c_float, std, c), _o._stream())
    else:
        _o._lib.call('vited_patchify_turned', _o._ptr(img), img.stride(0), _o._ptr(batch_index), _o._ptr(turns), turn_all, _o._ptr(out),
                     _o._code(dtype), nb, c, s, patch, _o._stream())
    return out


def puzzle_distances2_from_logits(logits: torch.Tensor, pi: torch.Tensor, pjt: torch.Tensor, dq2: torch.Tensor, bad: torch.Tensor):
    """dq2[si, pi[r], j, sj] = uint32(trunc(fp32(fp32(1 - sigmoid(logits[r, b])) * 1000))) for the bins b = 0..3 of the pair (piece
    pi[r], piece j turned by k clockwise quarter turns), pjt[r] = k * n + j: si = (b + 1) % 4, sj = (si + 2 - k) % 4
    (``vited_puzzle_distances2_from_logits``).  logits float32 [m, 4], pi / pjt int64 [m], dq2 int32 [4, n, n, 4]; a pair with pi
    outside [0, n), pjt outside [0, 4 n) or j == pi sets bad int32 [1] and writes nothing."""
    _o._need_gpu(logits, pi, pjt, dq2, bad)
    op = 'puzzle_distances2_from_logits'
    shape = tuple(getattr(dq2, 'shape', ()))
    if len(shape) != 4 or shape[0] != 4 or shape[3] != 4 or shape[1] != shape[2] or not 2 <= shape[1] <= _pp.PUZZLE_MAX_PIECES:
        raise ValueError(f'{op}: dq2 must be [4, n, n, 4] with 2 <= n <= {_pp.PUZZLE_MAX_PIECES}, got shape {list(shape)}')
    n, dev, m = shape[1], dq2.device, getattr(pi, 'numel', lambda: 0)()
    for name, t, dtype, extent in (('dq2', dq2, _i32, (4, n, n, 4)), ('logits', logits, _f32, (m, 4)), ('pi', pi, _i64, (m,)),
                                   ('pjt', pjt, _i64, (m,)), ('bad', bad, _i32, (1,))):
        _o._check(op, name, t, dtype, extent, dev)
    _o._lib.call('vited_puzzle_distances2_from_logits', _o._ptr(logits), _o._ptr(pi), _o._ptr(pjt), m, n, _o._ptr(dq2), _o._ptr(bad),
                 _o._stream())
