"""CPU: the host side of the matrix-core fp32 attention (attention_f32_mfma.hip): the three C entries, the shape predicate and the
process-wide kernel selection.  No kernel is launched."""
import ctypes
import re
import threading

import pytest
import torch

ENTRIES = ('vited_attention_f32_mfma_supported', 'vited_last_fp32_attention_kernel', 'vited_fp32_attention_select')


def test_entries_are_in_the_header_the_binding_and_the_library(vited):
    i, i64 = ctypes.c_int, ctypes.c_int64
    text = re.sub(r'/\*.*?\*/', ' ', open(vited._lib.HEADER_PATH).read(), flags=re.S)
    lib = vited._lib.load()
    for name in ENTRIES:
        assert re.search(rf'\bint {name}\s*\(', text), f'{name} is not declared in include/vited.h'
        assert name in vited._lib.SIGNATURES and hasattr(lib, name)
    assert vited._lib.SIGNATURES['vited_attention_f32_mfma_supported'] == (i, [i, i64, i, i64, i64, i, i])
    assert vited._lib.SIGNATURES['vited_last_fp32_attention_kernel'] == (i, [])
    assert vited._lib.SIGNATURES['vited_fp32_attention_select'] == (i, [i])
    assert lib.vited_abi_version() == 1                  # additions leave the ABI version where it is
    for name in ('fp32_attention_supported', 'last_fp32_attention_kernel', 'fp32_attention_kernels'):
        assert callable(getattr(vited.ops, name))


def test_other_head_dims_and_dtypes_are_not_covered(vited):
    ops, lib = vited.ops, vited._lib.load()
    for backward in (False, True):
        assert not ops.fp32_attention_supported(4, 8, 257, 257, 48, backward=backward)
        assert not ops.fp32_attention_supported(4, 8, 257, 257, 16, backward=backward)
        assert not ops.fp32_attention_supported(4, 6, 257, 257, 64, backward=backward, dtype=torch.float16)
        assert not ops.fp32_attention_supported(4, 6, 257, 257, 64, backward=backward, dtype=2)
        assert lib.vited_attention_f32_mfma_supported(-1, 4, 6, 257, 257, 64, int(backward)) == 0
        # what is no attention at all is not covered either
        assert not ops.fp32_attention_supported(0, 6, 257, 257, 64, backward=backward)
        assert not ops.fp32_attention_supported(4, 6, 0, 257, 64, backward=backward)
        assert not ops.fp32_attention_supported(4, 6, 257, 0, 64, backward=backward)


# the shapes DESIGN.md section 38 lists as taken: (batch, heads, nq, nk, head_dim)
TAKEN = [(256, 12, 64, 64, 32), (128, 12, 65, 65, 32), (16, 12, 64, 64, 32), (8, 12, 65, 65, 32), (8, 6, 256, 256, 64),
         (4, 6, 257, 257, 64), (4, 12, 257, 257, 32), (8, 6, 576, 576, 64), (4, 6, 577, 577, 64), (4, 6, 1024, 1024, 64),
         (2, 6, 1025, 1025, 64)]


@pytest.mark.parametrize('shape', TAKEN, ids=['x'.join(map(str, s)) for s in TAKEN])
def test_the_measured_shapes_are_covered(vited, shape):
    ops = vited.ops
    for dtype in (torch.float32, torch.bfloat16):        # the storage type does not enter: bf16 reaches path 1 by its layout
        assert ops.fp32_attention_supported(*shape, dtype=dtype)
        assert ops.fp32_attention_supported(*shape, backward=True, dtype=dtype)


def test_select_round_trips_and_rejects_other_modes(vited):
    lib = vited._lib.load()
    first = lib.vited_fp32_attention_select(0)
    gemm = lib.vited_fp32_gemm_select(0)
    try:
        assert first in (0, 1)
        assert lib.vited_fp32_attention_select(1) == 0
        assert lib.vited_fp32_attention_select(1) == 1
        assert lib.vited_fp32_gemm_select(0) == 0                     # the GEMM selection is a switch of its own
        assert lib.vited_fp32_attention_select(0) == 1
        assert lib.vited_fp32_attention_select(0) == 0
        for bad in (2, -1, 7):
            assert lib.vited_fp32_attention_select(bad) == 1          # VITED_ERR_BAD_ARG
            assert lib.vited_fp32_attention_select(0) == 0            # ... and nothing changed
        assert lib.vited_fp32_gemm_select(1) == 0
        assert lib.vited_fp32_attention_select(0) == 0
    finally:
        lib.vited_fp32_attention_select(first)
        lib.vited_fp32_gemm_select(gemm)


def test_the_context_manager_restores_the_mode(vited):
    ops, lib = vited.ops, vited._lib.load()

    def mode():
        m = lib.vited_fp32_attention_select(0)
        lib.vited_fp32_attention_select(m)
        return m

    assert mode() == 0                                           # automatic is the default of the process
    with ops.fp32_attention_kernels('valu'):
        assert mode() == 1
        with ops.fp32_attention_kernels('auto'):
            assert mode() == 0
        assert mode() == 1
    assert mode() == 0
    with pytest.raises(KeyError, match='inside'):
        with ops.fp32_attention_kernels('valu'):
            raise KeyError('inside')
    assert mode() == 0
    with pytest.raises(ValueError, match="'auto' or 'valu'"):
        with ops.fp32_attention_kernels('mfma'):
            pass
    assert mode() == 0


def test_no_kernel_is_reported_before_a_call(vited):
    """The record is per thread: a thread that has issued no attention reads 0, whatever other threads have run."""
    seen = []
    t = threading.Thread(target=lambda: seen.append(vited.ops.last_fp32_attention_kernel()))
    t.start()
    t.join()
    assert seen == [0]
    assert vited.ops.last_fp32_attention_kernel() in (0, 1, 2)
