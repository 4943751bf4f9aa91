"""The K = 384 NT GEMM shapes (M >= 8,192, N >= 768, N % 128 == 0; plain-store, multiply and GELU' epilogues) that the kernel
with the A operand in registers (gemm_nt_k384.hip) covers; which of them the dispatch gives it is a measured choice (gemm_mfma.hip,
nt_areg_waves).  last_paths() is 2 for both kernels, so which one ran follows from the dispatch alone.  In a product build the
new kernel runs:
  * EPI_MUL at every case of this file (all N, all M >= 8,192), on 8-wave workgroups (gemm_nt_areg_kernel<EPI_MUL, 8>);
  * EPI_STORE (with and without bias) for N >= 1152 and M >= 65,536, on 4-wave workgroups (<EPI_STORE, 4>): here M = 66,560
    (whole panels) and the ragged M = 65,613 and 73,800 (config H's decoder rows) at N = 1152 and 1536, contiguous and strided;
  * nothing else: EPI_GELU_GRAD, N = 768 plain store and every plain store below 65,536 rows compare the tile kernel with itself.
The other four instances (both geometries of every epilogue) exist only in an experiment build, which runs this whole file over
them on every shape:
    make -C vit-ed_amd/csrc VARIANT=t EXTRA=-DVITED_TUNING
    VITED_LIB=$PWD/vit-ed_amd/libvited_hip_t.so VITED_NT_AREG=8 python -m pytest -m gpu tests/test_gpu_gemm_k384.py     (and =4)
A change of the thresholds in nt_areg_waves moves this coverage: keep the list above and the row counts below in step with it.

Every output element against fp64 on the same bf16-rounded operands, and BIT-equal to gemm_nt_mfma_kernel: a GEMM row depends on
no other row and launches of fewer than 8,192 rows take the unchanged 128 x 128 tile kernel, so the large launch is compared with
launches on row slices of 8,000 rows (which straddle the 128- / 256-row panel boundaries and end in the ragged tail).  Both kernels
sum every element over k = 0, 32, ..., 352 in ascending order with the same MFMA and share the epilogue arithmetic.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16_OUT = dict(rtol=1e-2, atol=1e-2)   # the bound of tests/test_gpu_ops.py
K = 384
SLICE = 8000                             # < 8,192 rows: the old kernel; not a multiple of 128: slices straddle panel boundaries


def _rand(shape, dev, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev).to(dtype)


def _operands(M, N, gpu):
    a = _rand((M, K), gpu, 31, dtype=torch.bfloat16)
    w = _rand((N, K), gpu, 32, 1 / math.sqrt(K), dtype=torch.bfloat16)
    bias = _rand((N,), gpu, 33)
    aux = _rand((M, N), gpu, 34, dtype=torch.bfloat16)
    return a, w, bias, aux


def _launches(ops, L, a, w, bias, aux):
    """name -> outputs of the four launches of the issue: plain store with and without bias, multiply, GELU' (both outputs)."""
    out = {}
    out['store+bias'] = (ops.gemm(a, w, bias=bias),)
    assert ops.last_paths()[0] == 2
    out['store'] = (ops.gemm(a, w),)
    assert ops.last_paths()[0] == 2
    out['mul'] = (ops.gemm(a, w, epilogue=L.EPI_MUL, aux=aux),)
    assert ops.last_paths()[0] == 2
    out['gelu_grad'] = tuple(ops.gemm(a, w, epilogue=L.EPI_GELU_GRAD, bias=bias))
    assert ops.last_paths()[0] == 2
    return out


@pytest.mark.parametrize('N', [768, 1152, 1536])
# 65,613 = 65,536 + 77 and 73,800: ragged row counts at which the plain-store launches take the new kernel (a wave tile partly and
# wholly past M, a share that crosses from a full panel into the ragged one)
@pytest.mark.parametrize('M', [8192, 16640, 16555, 66560, 65613, 73800])
def test_k384_gemm_against_fp64_and_bit_equal_to_the_tile_kernel(vited, gpu, M, N):
    ops, L = vited.ops, vited._lib
    a, w, bias, aux = _operands(M, N, gpu)
    got = _launches(ops, L, a, w, bias, aux)

    acc = a.double() @ w.double().t()
    ref = acc + bias.double()
    torch.testing.assert_close(got['store+bias'][0].double(), ref, **BF16_OUT)
    torch.testing.assert_close(got['store'][0].double(), acc, **BF16_OUT)
    torch.testing.assert_close(got['mul'][0].double(), acc * aux.double(), **BF16_OUT)
    zg = ref.clone().requires_grad_()
    F.gelu(zg).sum().backward()
    torch.testing.assert_close(got['gelu_grad'][0].double(), zg.grad, **BF16_OUT)
    torch.testing.assert_close(got['gelu_grad'][1].double(), F.gelu(ref), **BF16_OUT)
    del acc, ref, zg

    # bit-equal to the old kernel on every row
    for r0 in range(0, M, SLICE):
        r1 = min(M, r0 + SLICE)
        part = _launches(ops, L, a[r0:r1], w, bias, aux[r0:r1])
        for name, outs in got.items():
            for full, sl in zip(outs, part[name]):
                assert torch.equal(full[r0:r1], sl), (name, M, N, r0, r1)

    # the same bits on every launch (race screen for the W ring), unrelated memory traffic in between
    noise = torch.empty(16 << 20, device=gpu)
    for it in range(4):
        noise.fill_(float(it))
        again = _launches(ops, L, a, w, bias, aux)
        for name, outs in got.items():
            for first, t in zip(outs, again[name]):
                assert torch.equal(first, t), (name, M, N, it)


@pytest.mark.parametrize('M,N', [(16555, 1152), (8192, 1536), (65613, 1152), (73800, 1536)])
def test_k384_gemm_row_strides(vited, gpu, M, N):
    """Operand and output rows that are not contiguous (lda > K, ldo > N): the same bits as the contiguous launch."""
    ops, L = vited.ops, vited._lib
    a, w, bias, aux = _operands(M, N, gpu)
    want = _launches(ops, L, a, w, bias, aux)
    a_wide = torch.zeros((M, K + 16), device=gpu, dtype=torch.bfloat16)
    a_wide[:, :K] = a
    aux_wide = torch.zeros((M, N + 64), device=gpu, dtype=torch.bfloat16)
    aux_wide[:, :N] = aux
    a_s, aux_s = a_wide[:, :K], aux_wide[:, :N]

    def buf():
        return torch.full((M, N + 64), 7.0, device=gpu, dtype=torch.bfloat16)

    o = buf()
    ops.gemm(a_s, w, bias=bias, out=o[:, :N])
    assert ops.last_paths()[0] == 2
    assert torch.equal(o[:, :N], want['store+bias'][0]) and bool((o[:, N:] == 7.0).all())
    o = buf()
    ops.gemm(a_s, w, out=o[:, :N])
    assert ops.last_paths()[0] == 2
    assert torch.equal(o[:, :N], want['store'][0]) and bool((o[:, N:] == 7.0).all())
    o = buf()
    ops.gemm(a_s, w, epilogue=L.EPI_MUL, aux=aux_s, out=o[:, :N])
    assert ops.last_paths()[0] == 2
    assert torch.equal(o[:, :N], want['mul'][0]) and bool((o[:, N:] == 7.0).all())
    o, o2 = buf(), buf()
    ops.gemm(a_s, w, epilogue=L.EPI_GELU_GRAD, bias=bias, out=o[:, :N], out2=o2[:, :N])
    assert torch.equal(o[:, :N], want['gelu_grad'][0]) and torch.equal(o2[:, :N], want['gelu_grad'][1])
    assert bool((o[:, N:] == 7.0).all()) and bool((o2[:, N:] == 7.0).all())
