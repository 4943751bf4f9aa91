"""The host side of the matrix-core fp32 attention kernels (csrc/attention_f32_mfma.hip): the shape predicate,
the per-thread record of which kernels ran, and the process-wide selection between them.

Attention path 1 (the fp32 compute mode, and the bf16 operands the bf16 MFMA attention refuses) has the vector-ALU kernels and, where
``fp32_attention_supported`` says so, kernels on ``v_mfma_f32_32x32x2_f32`` that give the same bits.  Nothing here launches a kernel;
the library is looked up on ``ops`` at call time, so whatever replaces it there holds here too."""
from __future__ import annotations

import contextlib

import torch

from . import ops as _o

_FP32_ATTENTION_MODES = {'auto': 0, 'valu': 1}


def _dtype_code(dtype) -> int:
    if isinstance(dtype, torch.dtype):
        return {torch.float32: 0, torch.bfloat16: 1}.get(dtype, -1)       # VITED_F32 / VITED_BF16; anything else is no attention dtype
    return int(dtype)


def fp32_attention_supported(batch: int, heads: int, nq: int, nk: int, head_dim: int, *, backward: bool = False,
                             dtype=torch.float32) -> bool:
    """Whether ``attention_fwd`` (``backward=False``) or ``attention_bwd`` of that shape, once it is on attention path 1, takes the
    matrix-core kernels under ``'auto'``.  ``dtype`` is the storage type (a torch dtype or a VITED_* code).  Host-only."""
    return bool(_o._lib.load().vited_attention_f32_mfma_supported(_dtype_code(dtype), int(batch), int(heads), int(nq), int(nk),
                                                                  int(head_dim), int(bool(backward))))


def last_fp32_attention_kernel() -> int:
    """Which kernels the last path-1 attention call of this thread ran: 0 none yet, 1 vector-ALU, 2 matrix-core."""
    return _o._lib.load().vited_last_fp32_attention_kernel()


@contextlib.contextmanager
def fp32_attention_kernels(mode: str):
    """Within the block, path-1 attention calls pick their kernels automatically (``'auto'``, the default of the process) or stay on
    the vector-ALU kernels (``'valu'``); the previous mode returns on exit, also on an exception.  Both give the same bits.
    Process-wide, and separate from ``fp32_gemm_kernels``."""
    if mode not in _FP32_ATTENTION_MODES:
        raise ValueError(f"fp32_attention_kernels: mode is 'auto' or 'valu', not {mode!r}")
    select = _o._lib.load().vited_fp32_attention_select    # returns the previous mode, not a status: only valid modes are passed
    previous = select(_FP32_ATTENTION_MODES[mode])
    try:
        yield
    finally:
        select(previous)
