"""CPU: the host side of the matrix-core fp32 GEMMs (gemm_f32_mfma.hip): the three C entries, the shape predicate and the
process-wide kernel selection.  No kernel is launched."""
import ctypes
import re
import threading

import pytest

ENTRIES = ('vited_gemm_f32_mfma_supported', 'vited_last_fp32_gemm_kernel', 'vited_fp32_gemm_select')


def test_entries_are_in_the_header_the_binding_and_the_library(vited):
    i, i64 = ctypes.c_int, ctypes.c_int64
    text = re.sub(r'/\*.*?\*/', ' ', open(vited._lib.HEADER_PATH).read(), flags=re.S)
    lib = vited._lib.load()
    for name in ENTRIES:
        assert re.search(rf'\bint {name}\s*\(', text), f'{name} is not declared in include/vited.h'
        assert name in vited._lib.SIGNATURES and hasattr(lib, name)
    assert vited._lib.SIGNATURES['vited_gemm_f32_mfma_supported'] == (i, [i64, i64, i64, i, i])
    assert vited._lib.SIGNATURES['vited_last_fp32_gemm_kernel'] == (i, [])
    assert vited._lib.SIGNATURES['vited_fp32_gemm_select'] == (i, [i])
    assert lib.vited_abi_version() == 1                  # additions leave the ABI version where it is


def test_the_head_stays_on_the_vector_alu_kernel(vited):
    ops = vited.ops
    assert not ops.fp32_gemm_supported(33, 4, 384)
    assert not ops.fp32_gemm_supported(33, 4, 384, b_layout=ops.B_KN, epilogue=ops.EPI_STORE_F32)


def test_a_block_shape_is_covered_in_both_layouts_and_every_epilogue(vited):
    ops = vited.ops
    epilogues = (ops.EPI_STORE, ops.EPI_GELU, ops.EPI_RESIDUAL, ops.EPI_MUL_GELU_GRAD, ops.EPI_STORE_F32, ops.EPI_MUL, ops.EPI_GELU_GRAD)
    assert sorted(epilogues) == list(range(7))
    for layout in (ops.B_NK, ops.B_KN):
        for epi in epilogues:
            assert ops.fp32_gemm_supported(128, 384, 384, b_layout=layout, epilogue=epi), (layout, epi)
    # what is no GEMM at all is not covered either
    assert not ops.fp32_gemm_supported(128, 384, 384, b_layout=2)
    assert not ops.fp32_gemm_supported(128, 384, 384, epilogue=7) and not ops.fp32_gemm_supported(128, 384, 384, epilogue=-1)
    assert not ops.fp32_gemm_supported(0, 384, 384) and not ops.fp32_gemm_supported(128, 384, 0)


def test_select_round_trips_and_rejects_other_modes(vited):
    lib = vited._lib.load()
    first = lib.vited_fp32_gemm_select(0)
    try:
        assert first in (0, 1)
        assert lib.vited_fp32_gemm_select(1) == 0
        assert lib.vited_fp32_gemm_select(1) == 1
        assert lib.vited_fp32_gemm_select(0) == 1
        assert lib.vited_fp32_gemm_select(0) == 0
        for bad in (2, -1, 7):
            assert lib.vited_fp32_gemm_select(bad) == 1          # VITED_ERR_BAD_ARG
            assert lib.vited_fp32_gemm_select(0) == 0            # ... and nothing changed
    finally:
        lib.vited_fp32_gemm_select(first)


def test_the_context_manager_restores_the_mode(vited):
    ops, lib = vited.ops, vited._lib.load()

    def mode():
        m = lib.vited_fp32_gemm_select(0)
        lib.vited_fp32_gemm_select(m)
        return m

    assert mode() == 0                                           # automatic is the default of the process
    with ops.fp32_gemm_kernels('valu'):
        assert mode() == 1
        with ops.fp32_gemm_kernels('auto'):
            assert mode() == 0
        assert mode() == 1
    assert mode() == 0
    with pytest.raises(KeyError, match='inside'):
        with ops.fp32_gemm_kernels('valu'):
            raise KeyError('inside')
    assert mode() == 0
    with pytest.raises(ValueError, match="'auto' or 'valu'"):
        with ops.fp32_gemm_kernels('mfma'):
            pass
    assert mode() == 0


def test_no_kernel_is_reported_before_a_call(vited):
    """The record is per thread: a thread that has issued no GEMM reads 0, whatever other threads have run."""
    seen = []
    t = threading.Thread(target=lambda: seen.append(vited.ops.last_fp32_gemm_kernel()))
    t.start()
    t.join()
    assert seen == [0]
    assert vited.ops.last_fp32_gemm_kernel() in (0, 1, 2)
