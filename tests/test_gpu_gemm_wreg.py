"""The 384-column NT products with the weights held in registers (csrc/gemm_nt_wreg.hip), called through ops.gemm_nt_wreg so that the
shapes can be small: the kernel's paths depend on how many 16-row units a workgroup gets, not on the row count itself.

  * default workgroups (one per CU, divided over the groups): M = 1, 15, 16, 17 (one ragged / whole / whole + ragged unit: every
    workgroup but one or two returns at once), 4,096 (256 units: one each at one group), 4,113 and 8,247 (unequal shares, a share of
    odd length whose last tile is half used, a ragged last unit);
  * few workgroups at M = 2,003: shares of 126 / 42 / 15-16 units = up to 63 steps through the 5-slot ring;
  * groups = 1 ([M, 384]), 3 ([M, 1152], side by side), 2 and 16 in the decoder's kv addressing ([G / 2, M, 768], dense).

Every element against fp64 on the same bf16 operands, and BIT-equal to ops.gemm on each group's weight slice: a GEMM row depends on
no other row, and launches of at most 8,000 rows are far below the row counts from which ops.gemm's own dispatch uses this kernel
(NT_WREG_MIN_M = 32,768 at N = 384, NT_WREG_QKV_MIN_M = 65,536 at N = 1152: gemm_mfma.hip), so they run the 128 x 128 tile kernel.  Both
sum every element over k = 0, 32, ..., 352 in ascending order with the same MFMA and round acc + bias once.  (Through the dispatch
itself the kernel is reached by tests/test_gpu_gemm_k384.py: its plain-store launches at N = 1152 from 65,536 rows, three groups.)
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16_OUT = dict(rtol=1e-2, atol=1e-2)   # the bound of tests/test_gpu_ops.py
K = W = 384
SLICE = 8000


def _rand(shape, dev, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev).to(dtype)


def _operands(M, groups, gpu):
    a = _rand((M, K), gpu, 41, dtype=torch.bfloat16)
    w = _rand((groups * W, K), gpu, 42, 1 / math.sqrt(K), dtype=torch.bfloat16)
    bias = _rand((groups * W,), gpu, 43)
    return a, w, bias


def _empty_out(M, groups, gpu):
    """groups 2 and 16: the kv addressing, L dense [M, 768] tensors; 1 and 3: the groups side by side in one [M, 384 G]."""
    shape = (groups // 2, M, 2 * W) if groups % 2 == 0 else (M, groups * W)
    return torch.empty(shape, device=gpu, dtype=torch.bfloat16)


def _group(out, g):
    """The [M, 384] block of group g."""
    if out.dim() == 3:
        return out[g // 2, :, (g % 2) * W:(g % 2 + 1) * W]
    return out[:, g * W:(g + 1) * W]


def _check_all(ops, gpu, M, groups, with_bias, workgroups=0):
    a, w, bias = _operands(M, groups, gpu)
    bias = bias if with_bias else None
    got = ops.gemm_nt_wreg(a, w, bias, _empty_out(M, groups, gpu), groups=groups, workgroups=workgroups)
    assert ops.last_paths()[0] == 2
    ref = a.double() @ w.double().t()
    if with_bias:
        ref += bias.double()
    for g in range(groups):
        torch.testing.assert_close(_group(got, g).double(), ref[:, g * W:(g + 1) * W], **BF16_OUT)
        # bit-equal to the tile kernel on every row
        for r0 in range(0, M, SLICE):
            r1 = min(M, r0 + SLICE)
            part = ops.gemm(a[r0:r1], w[g * W:(g + 1) * W], bias=None if bias is None else bias[g * W:(g + 1) * W])
            assert torch.equal(_group(got, g)[r0:r1], part), (M, groups, g, r0)
    # the same bits on every launch (race screen for the A ring and the staging tile), unrelated memory traffic in between
    noise = torch.empty(16 << 20, device=gpu)
    for it in range(4):
        noise.fill_(float(it))
        again = ops.gemm_nt_wreg(a, w, bias, _empty_out(M, groups, gpu), groups=groups, workgroups=workgroups)
        assert torch.equal(got, again), (M, groups, it)


@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('M,groups', [(M, g) for M in (1, 15, 16, 17, 4096, 4113, 8247) for g in (1, 2, 3, 16)
                                      if g < 16 or M <= 4113])          # 16 groups up to 4,113 rows
def test_wreg_against_fp64_and_bit_equal_to_the_tile_kernel(vited, gpu, M, groups, with_bias):
    _check_all(vited.ops, gpu, M, groups, with_bias)


@pytest.mark.parametrize('groups', [1, 2])
@pytest.mark.parametrize('workgroups', [1, 3, 8])
def test_wreg_long_shares_wrap_the_ring(vited, gpu, workgroups, groups):
    """2,003 rows = 126 units on 1 / 3 / 8 workgroups (per group: 1 / 1 / 4 with two groups): many times the ring's five slots."""
    _check_all(vited.ops, gpu, 2003, groups, True, workgroups=workgroups)


@pytest.mark.parametrize('M,groups', [(17, 2), (4113, 4), (2003, 1), (8247, 3)])
def test_wreg_row_strides_and_guards(vited, gpu, M, groups):
    """lda > 384, ldo > 384 groups_inner and tensors that are not back to back: the same bits as the dense launch, guard columns and
    guard rows (prefilled with 7.0) untouched."""
    ops = vited.ops
    a, w, bias = _operands(M, groups, gpu)
    want = ops.gemm_nt_wreg(a, w, bias, _empty_out(M, groups, gpu), groups=groups)
    a_wide = torch.zeros((M, K + 16), device=gpu, dtype=torch.bfloat16)
    a_wide[:, :K] = a
    shape = want.shape
    buf = torch.full((*shape[:-2], M + 3, shape[-1] + 64), 7.0, device=gpu, dtype=torch.bfloat16)
    view = buf[..., :M, :shape[-1]]
    ops.gemm_nt_wreg(a_wide[:, :K], w, bias, view, groups=groups)
    assert ops.last_paths()[0] == 2
    assert torch.equal(view, want)
    assert bool((buf[..., M:, :] == 7.0).all()) and bool((buf[..., shape[-1]:] == 7.0).all())


@pytest.mark.parametrize('M,N', [(32771, 384), (65613, 1152)])
def test_dispatch_hands_the_measured_shapes_over(vited, gpu, M, N):
    """ops.gemm at the shapes its dispatch gives to this kernel (N = 384 from 32,768 rows, N = 1152 from 65,536), into a column slice
    of a wider buffer: the same bits as with the hand-over switched off, guard columns untouched."""
    ops = vited.ops
    a, w, bias = _operands(M, N // W, gpu)
    buf = torch.full((M, N + 64), 7.0, device=gpu, dtype=torch.bfloat16)
    ops.gemm(a, w, bias=bias, out=buf[:, :N])
    assert ops.last_paths()[0] == 2
    with ops.gemm_nt_wreg_dispatch(False):
        want = ops.gemm(a, w, bias=bias)
    assert torch.equal(buf[:, :N], want) and bool((buf[:, N:] == 7.0).all())
    assert torch.equal(ops.gemm_nt_wreg(a, w, bias), want)


def test_wreg_refuses_what_it_cannot_address(vited, gpu):
    ops = vited.ops
    a, w, bias = _operands(32, 2, gpu)
    with pytest.raises(ValueError, match=r'^gemm_nt_wreg: w '):
        ops.gemm_nt_wreg(a, w[:500], bias)
    with pytest.raises(ValueError, match=r'^gemm_nt_wreg: w '):
        ops.gemm_nt_wreg(a, w, bias, groups=3)
    with pytest.raises(ValueError, match=r'^gemm_nt_wreg: out '):
        ops.gemm_nt_wreg(a, w, bias, torch.empty((32, 3 * W), device=gpu, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match=r'^gemm_nt_wreg: bias '):
        ops.gemm_nt_wreg(a, w, bias[:W])
    with pytest.raises(ValueError, match=r'^gemm_nt_wreg: a '):
        ops.gemm_nt_wreg(a.float(), w, bias)


def test_model_kv_in_one_launch_equals_the_loop(vited, gpu):
    """A config-A model at batch 2: the decoder's keys / values of all blocks from one grouped launch against one GEMM per block
    (rt.kv_one_launch = True against False, the default).  Loss and every gradient bit for bit."""
    from oracle import vited_oracle as vo
    s = vo.ViTEDShape()
    torch.manual_seed(5)
    model = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, num_classes=s.num_classes, embed_dim=s.embed_dim,
                                          depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads).to(gpu)
    model.compute_dtype = torch.bfloat16
    rt = model.runtime(torch.bfloat16)
    assert rt.fold_context
    default = rt.kv_one_launch
    x = torch.randn(2, 2, 3, s.img_size, s.img_size, device=gpu).clamp(-1, 1)
    y = (torch.rand(2, s.num_classes, device=gpu) > 0.5).float()
    seen = []
    real = vited.ops.gemm_nt_wreg

    def spy(*args, **kwargs):
        seen.append(kwargs.get('groups'))
        return real(*args, **kwargs)

    results = []
    for one_launch in (True, False):
        rt.kv_one_launch = one_launch
        model.zero_grad(set_to_none=True)
        vited.ops.gemm_nt_wreg = spy
        try:
            loss = torch.nn.functional.binary_cross_entropy_with_logits(model(x), y)
            loss.backward()
        finally:
            vited.ops.gemm_nt_wreg = real
        results.append((loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    rt.kv_one_launch = default
    assert seen == [2 * s.c_depth]                       # the grouped launch ran in the first pass and only there
    (loss1, grads1), (loss0, grads0) = results
    assert torch.equal(loss1, loss0) and grads1 and grads1.keys() == grads0.keys()
    for name, g in grads1.items():
        assert torch.equal(g, grads0[name]), name
