"""Functional wrapper of the 384-column NT products with the weights held in registers (``vited_gemm_nt_wreg``,
csrc/gemm_nt_wreg.hip).

``gemm_nt_wreg`` is an ``ops`` function in every respect - each tensor goes through ``ops._check`` before its pointer reaches
``ops._lib.call``, the launch goes to torch's current stream, nothing synchronises - kept in a module of its own; everything is looked
up on ``ops`` at call time, so whatever replaces the library or the device gate there holds here too."""
from __future__ import annotations

import contextlib

import torch

from . import ops as _o

_f32, _bf16 = torch.float32, torch.bfloat16
WREG_WIDTH = 384          # columns of a group, and K


def gemm_nt_wreg_supported(m: int, groups: int, groups_inner: int = 1, lda: int = WREG_WIDTH, ldw: int = WREG_WIDTH,
                           ldo: int | None = None, group_stride: int | None = None) -> bool:
    """Whether ``gemm_nt_wreg`` takes ``groups`` 384-column groups of an [m, 384] operand with these strides (defaults: dense).
    Host-only."""
    ldo = WREG_WIDTH * groups_inner if ldo is None else ldo
    group_stride = m * ldo if group_stride is None else group_stride
    return bool(_o._lib.load().vited_gemm_nt_wreg_supported(int(lda), int(ldw), int(ldo), int(m), int(groups), int(groups_inner),
                                                             int(group_stride)))


def gemm_nt_wreg(a: torch.Tensor, w: torch.Tensor, bias=None, out=None, *, groups: int | None = None, workgroups: int = 0):
    """out_g = a[M,384] . w[384 g : 384 (g + 1)]^T + bias[384 g : 384 (g + 1)] for every 384-row group g of the stacked bf16 weights
    ``w`` [384 G, 384], in ONE launch with the weights held in registers; bit-identical to ``ops.gemm`` per group.
    ``out``: bf16 [M, 384 G] (the groups side by side), or [G / i, M, 384 i] (``i`` groups side by side in each of G / i tensors with
    dense rows: the decoder's kv_all [L, Mc, 768]); a dense last dim, any row / tensor stride.  ``groups``: G, when given, checked
    against ``w``.  ``workgroups``: 0 = one per CU; a small count gives long shares of few rows (tests).  Returns ``out``.  Raises
    before anything is launched, every message beginning with ``gemm_nt_wreg: ``."""
    _o._need_gpu(a, w, bias, out)
    op, dev = 'gemm_nt_wreg', a.device
    lda = _o._rows(op, 'a', a, _bf16, dev, cols=WREG_WIDTH)
    m = a.shape[0]
    ldw = _o._rows(op, 'w', w, _bf16, dev, cols=WREG_WIDTH, like='a')
    g = w.shape[0] // WREG_WIDTH
    if g < 1 or w.shape[0] != g * WREG_WIDTH or (groups is not None and groups != g):
        raise ValueError(f'{op}: w has {w.shape[0]} rows, which are not {"whole" if groups is None else groups} groups of {WREG_WIDTH}')
    if out is None:
        out = torch.empty((m, g * WREG_WIDTH), dtype=_bf16, device=dev)
    if torch.is_tensor(out) and out.dim() == 3:
        _o._check(op, 'out', out, _bf16, (None, m, None), dev, _o.DENSE_LAST)
        outer, width, ldo, group_stride = out.shape[0], out.shape[2], out.stride(1), out.stride(0) if out.shape[0] > 1 else 0
    else:
        _o._check(op, 'out', out, _bf16, (m, None), dev, _o.DENSE_LAST)
        outer, width, ldo, group_stride = 1, out.shape[1], out.stride(0), 0
    inner = width // WREG_WIDTH
    if inner < 1 or width != inner * WREG_WIDTH or outer * inner != g:
        raise ValueError(f'{op}: out {list(out.shape)} does not hold {g} groups of {WREG_WIDTH} columns')
    if m == 1:
        lda, ldo = max(lda, WREG_WIDTH), max(ldo, width)              # the stride of a single row says nothing
    _o._check(op, 'bias', bias, _f32, g * WREG_WIDTH, dev, optional=True)
    if workgroups < 0:
        raise ValueError(f'{op}: workgroups must be >= 0, got {workgroups}')
    _o._lib.call('vited_gemm_nt_wreg', _o._ptr(a), lda, _o._ptr(w), ldw, _o._ptr(bias), _o._ptr(out), ldo, m, g, inner, group_stride,
                 int(workgroups), _o._stream())
    return out


@contextlib.contextmanager
def gemm_nt_wreg_dispatch(enabled: bool):
    """Within the block ``ops.gemm`` hands (``True``, the default of the process) or never hands (``False``) the shapes its dispatch
    names to the weights-in-registers kernel; the previous mode returns on exit.  Both give the same bits.  Process-wide."""
    select = _o._lib.load().vited_gemm_nt_wreg_select       # returns the previous mode, not a status: only valid modes are passed
    previous = select(0 if enabled else 1)
    try:
        yield
    finally:
        select(previous)
