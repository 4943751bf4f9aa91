"""Functional wrappers of the ranked-list and curve entry points (csrc/rank_lists.hip, the curve record of csrc/rank_metrics.hip;
DESIGN.md section 30), re-exported by ``ops``.

They are ``ops`` functions in every respect - each tensor goes through ``ops._check`` before its pointer reaches ``ops._lib.call``, the
launch goes to torch's current stream, nothing synchronises - kept in a module of their own; everything is looked up on ``ops`` at
call time, so whatever replaces the library or the device gate there (tests/test_ops_args.py does) holds here too."""
from __future__ import annotations

import torch

from . import ops as _o

TOPK_MAX_K = 1024          # SEL_MAX_K of csrc/rank_key.h: k + 1 keys fit the kernel's candidate buffer twice over
_f32, _i32, _i64, _u8 = torch.float32, torch.int32, torch.int64, torch.uint8


def _flags(remove_self_column, from_similarity):
    return int(bool(remove_self_column)), int(bool(from_similarity))


def retrieval_topk_rows(matrix: torch.Tensor, k: int, rows: tuple[int, int], labels=None, *, remove_self_column: bool = True,
                        from_similarity: bool = False):
    """(idx int32 [r1 - r0, k], val float32 [r1 - r0, k], hit uint8 [r1 - r0, k] | None): the first ``k`` retrievals of the rows
    [r0, r1) of the [n, n] matrix in the stable order of the retrieval metrics (ascending by (value, column); with
    ``remove_self_column`` behind the dropped first element), the values they were ranked by (the matrix' own, or dtype(1 - S) with
    ``from_similarity``), and with ``labels`` int32 [n] whether each hit has the row's label (``vited_retrieval_topk``).
    1 <= k <= 1024 and k + skip <= n."""
    _o._need_gpu(matrix, labels)
    op = 'retrieval_topk_rows'
    if labels is None:
        if matrix.dtype not in _o._FLOATS:
            raise TypeError(f'{op}: matrix must be float32, bfloat16 or float16, got {matrix.dtype}')
        if matrix.dim() != 2 or matrix.shape[0] != matrix.shape[1]:
            raise ValueError(f'{op}: matrix must be a square [n, n] matrix, got shape {tuple(matrix.shape)}')
        n = matrix.shape[0]
        ld = _o._rows(op, 'matrix', matrix, _o._FLOATS, matrix.device, n, n)
        dt, r0, r1 = _o._DTYPE[matrix.dtype], int(rows[0]), int(rows[1])
        if not 0 <= r0 < r1 <= n:
            raise ValueError(f'{op}: rows ({r0}, {r1}) is not a non-empty range inside [0, {n})')
    else:
        dt, ld, n, r0, r1 = _o._ranking_args(op, 'retrieval', matrix, labels, rows)
    k = int(k)
    skip, sim = _flags(remove_self_column, from_similarity)
    if k < 1 or k + skip > n:
        raise ValueError(f'{op}: k must be in [1, {n - skip}] for a row of {n} columns{" behind the dropped one" if skip else ""}, got {k}')
    if k > TOPK_MAX_K:
        raise ValueError(f'{op}: k must be at most {TOPK_MAX_K}, got {k}')
    dev = matrix.device
    idx = torch.empty((r1 - r0, k), dtype=_i32, device=dev)
    val = torch.empty((r1 - r0, k), dtype=_f32, device=dev)
    hit = torch.empty((r1 - r0, k), dtype=_u8, device=dev) if labels is not None else None
    _o._lib.call('vited_retrieval_topk', _o._ptr(matrix), dt, ld, n, r0, r1, _o._ptr(labels), k, skip, sim, _o._ptr(idx), _o._ptr(val),
                 _o._ptr(hit), _o._stream())
    return idx, val, hit


def retrieval_curve_rows(matrix: torch.Tensor, labels: torch.Tensor, offsets: torch.Tensor, members: torch.Tensor,
                         rows: tuple[int, int], *, remove_self_column: bool = True, from_similarity: bool = False, estimate=None,
                         tp_at=None):
    """(tp_at int64 [n - skip], records int32 [r1 - r0, 2]) for the rows [r0, r1) of the [n, n] matrix (``vited_retrieval_curves``):
    tp_at[p] = the rows whose retrieval at 0-based position p (after the drop) is correct - ``sorted_retrievals.sum(axis=0)`` of the
    reference - and per row (correct retrievals, correct retrievals at positions < estimate[i]).  ``labels`` / ``offsets`` /
    ``members`` as ``retrieval_metrics_rows`` takes them.  ``estimate`` int32 [n] optional (the second count is 0 without it).  A
    given ``tp_at`` is ADDED onto (further shares of the same matrix); otherwise a zeroed one is made."""
    _o._need_gpu(matrix, labels, offsets, members, estimate, tp_at)
    op = 'retrieval_curve_rows'
    dt, ld, n, r0, r1 = _o._ranking_args(op, 'retrieval curve', matrix, labels, rows)
    dev = matrix.device
    _o._check(op, 'members', members, _i32, (n,), dev)
    _o._check(op, 'offsets', offsets, _i32, (None,), dev)
    _o._check(op, 'estimate', estimate, _i32, (n,), dev, optional=True)
    skip, sim = _flags(remove_self_column, from_similarity)
    if n - skip < 1:
        raise ValueError(f'{op}: matrix leaves no column to retrieve behind the dropped one (n = {n})')
    if tp_at is None:
        tp_at = torch.zeros(n - skip, dtype=_i64, device=dev)
    _o._check(op, 'tp_at', tp_at, _i64, (n - skip,), dev)
    records = torch.empty((r1 - r0, 2), dtype=_i32, device=dev)
    _o._lib.call('vited_retrieval_curves', _o._ptr(matrix), dt, ld, n, r0, r1, _o._ptr(labels), _o._ptr(offsets), _o._ptr(members),
                 offsets.numel() - 1, skip, sim, _o._ptr(estimate), _o._ptr(tp_at), _o._ptr(records), _o._stream())
    return tp_at, records
