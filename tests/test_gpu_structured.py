"""Parity on structured VALUES.  The other GPU tests draw every operand from randn and vary the shapes; these hold the shapes
small and vary what the numbers look like, because several hot-path kernels have code that only runs, or only matters, away
from N(0, 1): the O / l rescale of the tiled attention forward (never taken after the first key tile on randn scores), the
exact-delta correction of the tiled dQ kernel (~1e-4 on randn V), the two-pass variance of the three LayerNorm implementations
(a one-pass E[x^2] - mu^2 is fine on zero-mean rows), the tails of the fast GELU (randn pre-activations stay inside |z| < 5).

Attention is compared with fp64 softmax attention of the same operands under ELEMENTWISE bounds built from the operands
(structured_cases.attention_truth: rounding units over absolute sums, no blanket tolerance); tests/test_structured_cases.py
shows on the CPU that a faithful model of the arithmetic stays inside them and that two one-line mutants do not.  LayerNorm and
GELU keep the tolerances of the existing tests of the same ops / the accuracy the kernels' comments claim.

Every test prints its measured maximum of error / bound before asserting (pytest -s shows them; DESIGN.md records them).
"""
import math

import pytest
import torch
import torch.nn.functional as F

import structured_cases as sc

pytestmark = pytest.mark.gpu
BF16_OUT = dict(rtol=1e-2, atol=1e-2)   # the bound of tests/test_gpu_ops.py
PORTABLE, MFMA = 1, 2                   # ops.last_paths()[1]
SHORT_MAX = 80                          # attention_mfma.hip: 16 * SM_MAX_TILES


def _tiled(nq, nk, hd, backward):
    """ops.last_paths() tells the bf16 MFMA kernels from the portable ones and nothing more: inside the MFMA path the dispatcher
    (small_ok, attention_mfma.hip) takes the short-sequence kernels for nk <= 80 - the backward only with hd 32 and nq <= 80 - and
    the tiled ones otherwise.  The cases below are tied to their kernel by this shape rule, restated here so that each test asserts
    which side it means to be on; a dispatcher that moves the limit has to move SHORT_MAX with it."""
    return nk > SHORT_MAX or (backward and (hd != 32 or nq > SHORT_MAX))
UNIT = {torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -18}


def _seed(*parts):
    return sum((i + 1) * 7919 * (sum(map(ord, p)) if isinstance(p, str) else int(p)) for i, p in enumerate(parts)) % (2 ** 31)


def _on_gpu(case, gpu, dtype):
    """The operands the way the model lays them out: packed qkv [B, N, 3 D] consumed in place when self-shaped, q + packed kv
    otherwise; gradients are written into views of the same packing."""
    q, k, v, do = case
    D = q.shape[2]
    if q.shape[:2] == k.shape[:2]:
        qkv = torch.cat([q, k, v], -1).to(gpu).to(dtype)
        views = qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:]
        dqkv = torch.full_like(qkv, float('nan'))
        grads = dqkv[:, :, :D], dqkv[:, :, D:2 * D], dqkv[:, :, 2 * D:]
    else:
        qd = q.to(gpu).to(dtype)
        kv = torch.cat([k, v], -1).to(gpu).to(dtype)
        views = qd, kv[:, :, :D], kv[:, :, D:]
        dkv = torch.full_like(kv, float('nan'))
        grads = torch.full_like(qd, float('nan')), dkv[:, :, :D], dkv[:, :, D:]
    return views, do.to(gpu).to(dtype), grads


def _attention_ratios(ops, gpu, kind, B, H, nq, nk, hd, dtype, path, backward=True):
    """Forward (+ backward) through ops.attention_fwd / attention_bwd -> {tensor: max err / bound}, lse against rtol = atol = 1e-4."""
    scale = hd ** -0.5
    case = sc.attention_case(kind, B, B, H, nq, nk, hd, _seed(kind, nq, nk, hd))
    (q, k, v), do, (dq, dk, dv) = _on_gpu(case, gpu, dtype)
    truth, bound = sc.attention_truth(*(t.to(gpu) for t in case), H, scale, UNIT[dtype])
    o, lse = ops.attention_fwd(q, k, v, H, scale)
    assert ops.last_paths()[1] == path
    out = dict(o=sc.ratio(o, truth['o'], bound['o']), lse=sc.lse_ratio(lse, truth['lse']))
    if backward:
        # the kernels consume the SAVED (storage-dtype) output o, like the reference's SDPA backward
        ops.attention_bwd(q, k, v, o, do, lse, H, scale, dq, dk, dv)
        assert ops.last_paths()[1] == path
        for name, got in (('dq', dq), ('dk', dk), ('dv', dv)):
            out[name] = sc.ratio(got, truth[name], bound[name])
    return out


def _report(tag, kind, nq, nk, hd, ratios):
    print(f'\nvalue-parity {tag} {kind} nq={nq} nk={nk} hd={hd} ' + ' '.join(f'{n}={r:.3f}' for n, r in ratios.items()))
    assert all(r <= 1.0 for r in ratios.values()), (tag, kind, nq, nk, hd, ratios)


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('nq,nk', [(129, 321), (257, 1024), (1025, 1025), (65, 130)])
@pytest.mark.parametrize('kind', sc.ATTENTION_KINDS)
def test_tiled_attention_on_structured_values(vited, gpu, kind, nq, nk, hd):
    """bf16, nk > 80: the tiled online-softmax forward and the two tiled backward kernels.  'rising' makes the forward rescale
    O and l with a finite old maximum in every 16-query group (and leaves lazy steps in between); 'voffset' makes the delta
    estimated from the bf16 O wrong by ~0.5, which the dQ epilogue has to take out again."""
    assert _tiled(nq, nk, hd, False) and _tiled(nq, nk, hd, True)
    B, H = (2, 2) if nq > 1000 else (2, 3)
    _report('tiled', kind, nq, nk, hd, _attention_ratios(vited.ops, gpu, kind, B, H, nq, nk, hd, torch.bfloat16, MFMA))


@pytest.mark.parametrize('nq,nk', [(65, 65), (65, 64), (1, 65)])
@pytest.mark.parametrize('kind', ['onehot', 'uniform', 'voffset'])
def test_short_attention_on_structured_values(vited, gpu, kind, nq, nk):
    """bf16, nq and nk <= 80, hd 32: the short-sequence forward and the one-wave-per-head backward, which takes delta from its own
    P and dP."""
    assert not _tiled(nq, nk, 32, False) and not _tiled(nq, nk, 32, True)
    _report('short', kind, nq, nk, 32, _attention_ratios(vited.ops, gpu, kind, 3, 3, nq, nk, 32, torch.bfloat16, MFMA))


@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('nq,nk', [(129, 321), (65, 65)])
@pytest.mark.parametrize('kind', sc.ATTENTION_KINDS)
def test_portable_attention_on_structured_values(vited, gpu, kind, nq, nk, hd):
    """fp32 activations: the portable kernels, same formulas with the rounding unit 2^-18 in place of 2^-7."""
    _report('portable', kind, nq, nk, hd, _attention_ratios(vited.ops, gpu, kind, 2, 2, nq, nk, hd, torch.float32, PORTABLE))


@pytest.mark.parametrize('dtype,path', [(torch.bfloat16, MFMA), (torch.float32, PORTABLE)])
@pytest.mark.parametrize('nq,nk,hd', [(129, 321, 32), (129, 321, 64), (65, 65, 32)])
def test_indexed_forward_on_rising_scores(vited, gpu, nq, nk, hd, dtype, path):
    """ops.attention_fwd(..., kv_index=...) with a repeating, non-identity index: batch item b attends over k / v item index[b]."""
    ops = vited.ops
    B, KV, H, scale = 4, 3, 2, hd ** -0.5
    index = torch.tensor([2, 0, 2, 1], device=gpu)
    q, k, v, do = sc.attention_case('rising', B, KV, H, nq, nk, hd, _seed('indexed', nq, nk, hd))
    truth, bound = sc.attention_truth(q.to(gpu), k.to(gpu), v.to(gpu), do.to(gpu), H, scale, UNIT[dtype], kv_index=index)
    D = H * hd
    kv = torch.cat([k, v], -1).to(gpu).to(dtype)
    o, lse = ops.attention_fwd(q.to(gpu).to(dtype), kv[:, :, :D], kv[:, :, D:], H, scale, kv_index=index)
    assert ops.last_paths()[1] == path
    _report('indexed-' + ('bf16' if dtype == torch.bfloat16 else 'fp32'), 'rising', nq, nk, hd,
            dict(o=sc.ratio(o, truth['o'], bound['o']), lse=sc.lse_ratio(lse, truth['lse'])))


@pytest.mark.parametrize('nq,nk,hd', [(129, 321, 32), (129, 321, 64), (257, 1024, 64), (65, 130, 32), (65, 65, 32), (65, 65, 64)])
def test_value_offset_does_not_move_dq_dk(vited, gpu, nq, nk, hd):
    """Softmax backward is invariant to a constant added to every row of V.  dQ and dK computed with v = 16 + randn and with
    v - 16 (same dO; o and lse each from its own forward) agree within the sum of their two bounds: the 'exact delta' of the
    bf16 backward stated as a test.  (65, 65, 32) runs the short-sequence forward and backward, (65, 65, 64) the short-sequence
    forward and the tiled backward (the short backward is hd 32 only), every other shape the tiled kernels throughout."""
    ops = vited.ops
    assert _tiled(nq, nk, hd, True) == ((nq, nk, hd) != (65, 65, 32)) and _tiled(nq, nk, hd, False) == (nk > SHORT_MAX)
    B, H, scale = 2, 2, hd ** -0.5
    q, k, v, do = sc.attention_case('voffset', B, B, H, nq, nk, hd, _seed('offset', nq, nk, hd))
    got, bounds = [], []
    for vv in (v, v - sc.V_OFFSET):
        assert torch.equal(vv, sc.bf(vv))
        (qd, kd, vd), dod, (dq, dk, dv) = _on_gpu((q, k, vv, do), gpu, torch.bfloat16)
        o, lse = ops.attention_fwd(qd, kd, vd, H, scale)
        ops.attention_bwd(qd, kd, vd, o, dod, lse, H, scale, dq, dk, dv)
        assert ops.last_paths()[1] == MFMA
        got.append((dq.double(), dk.double()))
        bounds.append(sc.attention_truth(q.to(gpu), k.to(gpu), vv.to(gpu), do.to(gpu), H, scale, UNIT[torch.bfloat16])[1])
    ratios = {}
    for i, name in enumerate(('dq', 'dk')):
        assert bool(torch.isfinite(got[0][i]).all()) and bool(torch.isfinite(got[1][i]).all())
        ratios[name] = float(((got[0][i] - got[1][i]).abs() / (bounds[0][name] + bounds[1][name])).max())
    _report('offset-invariance', 'voffset', nq, nk, hd, ratios)


# ---------------------------------------------------------------------------------------------
# LayerNorm on structured rows: the three forward implementations, the two backward ones
# ---------------------------------------------------------------------------------------------
D = 384
LN_ROWS = [65 * 3 + 1, 640 + 17]


def _finite(**tensors):
    for name, t in tensors.items():
        assert bool(torch.isfinite(t).all()), f'{name} holds a NaN or an inf'


def _ln_truth(x, gamma, beta):
    """fp64 LayerNorm of the fp32 rows x -> (y, mean, rstd)."""
    xd = x.double()
    return (F.layer_norm(xd, (D,), gamma.double(), beta.double(), 1e-6), xd.mean(1),
            (xd.var(1, unbiased=False) + 1e-6).rsqrt())


def _affine(gpu, seed):
    gen = torch.Generator().manual_seed(seed)
    return (1 + 0.2 * torch.randn(D, generator=gen)).to(gpu), (0.1 * torch.randn(D, generator=gen)).to(gpu)


def _within(name, got, want, rtol, atol, extra=None):
    """|got - want| <= atol + rtol |want| (+ extra), elementwise; prints the largest err / allowance."""
    allow = atol + rtol * want.abs()
    if extra is not None:
        allow = allow + extra
    r = float(((got.double() - want).abs() / allow).max())
    print(f'value-parity layernorm {name} err/allowance={r:.3f}')
    assert r <= 1.0, (name, r)


def _mean_slack(kinds, mean, gpu):
    """2 ulp(|mu|) on the rows '1024 + round(8 randn) / 8', 0 elsewhere.  Those rows hold 13-bit values, so the fp32 sum of 384 of
    them is exact in any order and the only fp32 error in the mean is mu = fl(fl(sum) * fl(1 / d)): at most 2 ulp."""
    big = torch.tensor([k == 'mean1024' for k in kinds], device=gpu)
    return torch.where(big, 2 * sc.ulp32(mean), torch.zeros_like(mean))


@pytest.mark.parametrize('rows', LN_ROWS)
def test_layernorm_fwd_on_structured_rows(vited, gpu, rows):
    """ops.layernorm_fwd (layernorm.hip) against fp64 with the tolerances of test_layernorm_fwd_bwd (y fp32 1e-5 / 1e-5, mean
    1e-5 / 1e-6, y bf16 1e-2 / 1e-2) and of test_linear_residual_layernorm_fwd for rstd (1e-4 / 1e-6: the same arithmetic, bit for
    bit).  The fp32 outputs of the large-mean rows get the extra 2 ulp(|mu|) rstd |gamma| that the rounding of the mean itself
    costs; a one-pass variance is hundreds of times outside it."""
    ops = vited.ops
    xc, kinds = sc.layernorm_rows(rows, D, 31 + rows)
    x = xc.to(gpu)
    gamma, beta = _affine(gpu, 32)
    y_ref, mean_ref, rstd_ref = _ln_truth(x, gamma, beta)
    slack = _mean_slack(kinds, mean_ref, gpu)
    y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, 1e-6, torch.float32)
    y16, mean16, rstd16 = ops.layernorm_fwd(x, gamma, beta, 1e-6, torch.bfloat16)
    _finite(y=y, mean=mean, rstd=rstd, y16=y16, mean16=mean16, rstd16=rstd16)
    _within('fwd y fp32', y, y_ref, 1e-5, 1e-5, (slack * rstd_ref)[:, None] * gamma.double().abs())
    _within('fwd mean', mean, mean_ref, 1e-5, 1e-6, slack)
    _within('fwd rstd', rstd, rstd_ref, 1e-4, 1e-6)
    _within('fwd y bf16', y16, y_ref, **BF16_OUT)
    assert torch.equal(mean16, mean) and torch.equal(rstd16, rstd)


@pytest.mark.parametrize('rows', LN_ROWS)
def test_layernorm_bwd_on_structured_rows(vited, gpu, rows):
    """ops.layernorm_bwd with the tolerances of test_layernorm_fwd_bwd, unchanged.  The saved statistics are the fp64 ones rounded
    to fp32 (as test_linear_layernorm_bwd passes them) and the fp64 reference is evaluated AT those fp32 numbers
    (structured_cases.layernorm_bwd_ref; tests/test_structured_cases.py shows it equal to autograd through F.layer_norm at the
    row's own statistics).  On the rows around 1024 the fp32 mean is up to ulp(1024) / 2 = 6e-5 away from the exact one, which alone
    moves dx by ~1e-5: a reference at the exact mean would judge the operand, not the kernel."""
    ops = vited.ops
    xc, _ = sc.layernorm_rows(rows, D, 41 + rows)
    x = xc.to(gpu)
    gamma, beta = _affine(gpu, 42)
    gen = torch.Generator().manual_seed(43)
    dy, dx_in = torch.randn(rows, D, generator=gen).to(gpu), torch.randn(rows, D, generator=gen).to(gpu)
    _, mean_ref, rstd_ref = _ln_truth(x, gamma, beta)
    mean, rstd = mean_ref.float(), rstd_ref.float()
    dx_ref, dg_ref, db_ref = sc.layernorm_bwd_ref(dy, x, gamma, mean, rstd)
    dx, lp, dg, db = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx_in=dx_in, want_lp=True)
    _finite(dx=dx, lp=lp, dg=dg, db=db)
    _within('bwd dx', dx, dx_ref + dx_in.double(), 1e-4, 1e-5)
    assert torch.equal(lp, dx.to(torch.bfloat16))
    _within('bwd dgamma', dg, dg_ref, 1e-4, 1e-4 * math.sqrt(rows))
    _within('bwd dbeta', db, db_ref, 1e-4, 1e-4 * math.sqrt(rows))


@pytest.mark.parametrize('K', [384, 1536])
@pytest.mark.parametrize('rows', LN_ROWS)
def test_linear_residual_layernorm_fwd_on_structured_rows(vited, gpu, rows, K):
    """gemm_row.hip: the structured rows are the fp32 RESIDUAL, which is how such rows arise in the model, with a small a w^T on
    top whose every product and sum is exact in fp32 (integers times sixteenths on eight input channels; the rows of a are zero
    under the constant rows, which therefore stay constant).  y, h, mean, rstd against fp64 of the same operands with the
    tolerances of test_linear_residual_layernorm_fwd."""
    ops = vited.ops
    res_c, kinds = sc.layernorm_rows(rows, D, 51 + rows)
    gen = torch.Generator().manual_seed(52 + K)
    a = torch.zeros(rows, K)
    a[:, :8] = torch.round(torch.randn(rows, 8, generator=gen))
    a[[k.startswith('const') for k in kinds]] = 0
    w = torch.zeros(D, K)
    w[:, :8] = torch.round(2 * torch.randn(D, 8, generator=gen)) / 16
    a, w, res = a.to(gpu).to(torch.bfloat16), w.to(gpu).to(torch.bfloat16), res_c.to(gpu)
    gamma, beta = _affine(gpu, 53)
    assert ops.linear_layernorm_supported(rows, D, K, torch.bfloat16)
    y, h, mean, rstd = ops.linear_residual_layernorm_fwd(a, w, None, res, gamma, beta, 1e-6)
    _finite(y=y, h=h, mean=mean, rstd=rstd)
    y_ref = res.double() + a.double() @ w.double().t()
    _within('fused fwd y', y, y_ref, 1e-5, 2e-5 * K ** 0.5)
    h_ref, mean_ref, rstd_ref = _ln_truth(y_ref.float(), gamma, beta)
    _within('fused fwd mean', mean, mean_ref, 1e-5, 1e-5)
    _within('fused fwd rstd', rstd, rstd_ref, 1e-4, 1e-6)
    _within('fused fwd h', h, h_ref, **BF16_OUT)


@pytest.mark.parametrize('K', [384, 1536])
@pytest.mark.parametrize('rows', LN_ROWS)
def test_linear_layernorm_bwd_on_structured_rows(vited, gpu, rows, K):
    """gemm_row.hip backward: dx = dx_in + LN'(dy Wt^T) on structured x against fp64 autograd, tolerances of
    test_linear_layernorm_bwd (which scale the absolute part by the largest reference value)."""
    ops = vited.ops
    xc, _ = sc.layernorm_rows(rows, D, 61 + rows)
    x = xc.to(gpu)
    gen = torch.Generator().manual_seed(62 + K)
    dy = torch.randn(rows, K, generator=gen).to(gpu).to(torch.bfloat16)
    wt = (torch.randn(D, K, generator=gen) * K ** -0.5).to(gpu).to(torch.bfloat16)
    dx_in = torch.randn(rows, D, generator=gen).to(gpu)
    gamma, beta = _affine(gpu, 63)
    xd, gd, bd = (t.double().requires_grad_() for t in (x, gamma, beta))
    F.layer_norm(xd, (D,), gd, bd, 1e-6).backward(dy.double() @ wt.double().t())
    _, mean_ref, rstd_ref = _ln_truth(x, gamma, beta)
    dx, lp, dg, db = ops.linear_layernorm_bwd(dy, wt, x, gamma, mean_ref.float(), rstd_ref.float(), dx_in=dx_in, want_lp=True)
    _finite(dx=dx, lp=lp, dg=dg, db=db)
    want = xd.grad + dx_in.double()
    _within('fused bwd dx', dx, want, 1e-4, 1e-5 * float(want.abs().max()))
    assert torch.equal(lp, dx.to(torch.bfloat16))
    _within('fused bwd dgamma', dg, gd.grad, 1e-4, 1e-5 * float(gd.grad.abs().max()) * rows ** 0.5)
    _within('fused bwd dbeta', db, bd.grad, 1e-4, 1e-5 * float(bd.grad.abs().max()) * rows ** 0.5)


@pytest.mark.parametrize('rows', LN_ROWS)
def test_mlp_fused_layernorm_on_structured_rows(vited, gpu, rows):
    """mlp_fused.hip: saved mean, rstd and h = LayerNorm(x) (bf16) on structured x against fp64, tolerances of
    test_mlp_fused_forward_and_saved_tensors (mean 1e-5 / 1e-6 plus the 2 ulp of the large-mean rows, rstd 1e-5 / 1e-6, h 1e-2)."""
    ops = vited.ops
    xc, kinds = sc.layernorm_rows(rows, D, 71 + rows)
    x = xc.to(gpu)
    gamma, beta = _affine(gpu, 72)
    gen = torch.Generator().manual_seed(73)
    w1, b1 = (0.06 * torch.randn(1536, D, generator=gen)).to(gpu).to(torch.bfloat16), (0.1 * torch.randn(1536, generator=gen)).to(gpu)
    w2, b2 = (0.03 * torch.randn(D, 1536, generator=gen)).to(gpu).to(torch.bfloat16), (0.1 * torch.randn(D, generator=gen)).to(gpu)
    y, (mean, rstd, h, gd, u) = ops.mlp_fwd(x, gamma, beta, w1, b1, w2, b2, 1e-6, save=True)
    _finite(y=y, mean=mean, rstd=rstd, h=h, gd=gd, u=u)
    h_ref, mean_ref, rstd_ref = _ln_truth(x, gamma, beta)
    _within('mlp mean', mean, mean_ref, 1e-5, 1e-6, _mean_slack(kinds, mean_ref, gpu))
    _within('mlp rstd', rstd, rstd_ref, 1e-5, 1e-6)
    _within('mlp h', h, h_ref, **BF16_OUT)


# ---------------------------------------------------------------------------------------------
# GELU epilogues on a value grid
# ---------------------------------------------------------------------------------------------
def _gelu_allow(ref, z, dtype):
    """bf16 outputs: one output rounding (2^-8 |ref|) plus the cdf error the fast GELU claims (3e-7, times |z| where z
    multiplies it); fp32 outputs: 1e-6 max(1, |z|)."""
    zmag = z.double().abs().clamp_min(1.0)
    return 1e-6 * zmag if dtype == torch.float32 else 2.0 ** -8 * ref.abs() + 3e-7 * zmag


def _gelu_check(name, got, ref, z, dtype):
    _finite(**{name: got})
    r = (got.double() - ref).abs() / _gelu_allow(ref, z, dtype)
    worst = int(r.argmax())
    print(f'value-parity gelu {name} {dtype} err/allowance={float(r.max()):.3f} at z={float(z.flatten()[worst])!r}')
    assert float(r.max()) <= 1.0, (name, float(z.flatten()[worst]), float(got.flatten()[worst]), float(ref.flatten()[worst]))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('N,K', [(1536, 384), (64, 64), (32, 32)])
def test_gelu_epilogues_on_a_value_grid(vited, gpu, dtype, N, K):
    """ops.gemm with EPI_GELU, EPI_GELU_GRAD and EPI_MUL_GELU_GRAD, driven so that the pre-activation takes prescribed values:
    a[m, 0] = grid value m, w[n, 0] = 1, everything else 0, so acc[m, n] = grid[m] exactly and z = fl32(grid[m] + bias[n]) with
    bias a second, fine grid.  The multiplying epilogue takes the grid as its saved pre-activation.
    (1536, 384) is fc1 of the model; (32, 32) takes the portable kernel in bf16 too.

    -0 reaches the GELU code ONLY through the aux of EPI_MUL_GELU_GRAD (asserted below): in EPI_GELU / EPI_GELU_GRAD, and in the
    fused MLP, the accumulator starts at +0 and +0 + -0 = +0, so the grid's -0 arrives there as +0 (same value, other sign)."""
    ops, L = vited.ops, vited._lib
    grid = sc.gelu_grid().to(gpu)
    M = grid.numel()
    a = torch.zeros(M, K, device=gpu)
    a[:, 0] = grid
    w = torch.zeros(N, K, device=gpu)
    w[:, 0] = 1.0
    a, w = a.to(dtype), w.to(dtype)
    bias = ((torch.arange(N, device=gpu) % 16) - 8).float() / 64
    bias[::5] = 0.0
    z = grid[:, None] + bias[None, :]                                   # fp32: the one rounding the kernel makes too
    u_ref, g_ref = sc.gelu_ref(z)
    path = MFMA if dtype == torch.bfloat16 and K % 64 == 0 and N % 16 == 0 else PORTABLE
    zo, u = ops.gemm(a, w, epilogue=L.EPI_GELU, bias=bias)
    assert ops.last_paths()[0] == path
    torch.testing.assert_close(zo.double(), z.double(), rtol=2.0 ** -8 if dtype == torch.bfloat16 else 0, atol=0)
    _gelu_check('EPI_GELU u', u, u_ref, z, dtype)
    gd, u2 = ops.gemm(a, w, epilogue=L.EPI_GELU_GRAD, bias=bias)
    assert ops.last_paths()[0] == path
    _gelu_check('EPI_GELU_GRAD gd', gd, g_ref, z, dtype)
    _gelu_check('EPI_GELU_GRAD u', u2, u_ref, z, dtype)
    # acc = 1 everywhere, the saved pre-activation walks the grid along the rows and the columns
    ones = torch.zeros(M, K, device=gpu)
    ones[:, 0] = 1.0
    aux = grid[(torch.arange(M, device=gpu)[:, None] * 7 + torch.arange(N, device=gpu)[None, :]) % M].to(dtype)
    assert int((torch.signbit(aux.float()) & (aux.float() == 0)).sum()) > 0
    dz = ops.gemm(ones.to(dtype), w, epilogue=L.EPI_MUL_GELU_GRAD, aux=aux)
    assert ops.last_paths()[0] == path
    _gelu_check('EPI_MUL_GELU_GRAD dz', dz, sc.gelu_ref(aux.float())[1], aux.float(), dtype)


def test_mlp_fused_gelu_on_a_value_grid(vited, gpu):
    """ops.mlp_fwd's saved gd = gelu'(z) and u = gelu(z) with fc1's weight zero and its bias walking the grid: z = b1 in value
    (the -0 of the grid becomes +0 when it is added to the +0 accumulator; test_gelu_epilogues_on_a_value_grid carries the -0 case)."""
    ops = vited.ops
    grid = sc.gelu_grid()
    b1 = torch.cat([grid[:8], grid[8:][torch.linspace(0, grid.numel() - 9, 1536 - 8).round().long()]]).to(gpu)
    rows = 65
    xc, _ = sc.layernorm_rows(rows, D, 81)
    gamma, beta = _affine(gpu, 82)
    gen = torch.Generator().manual_seed(83)
    w1 = torch.zeros(1536, D, device=gpu, dtype=torch.bfloat16)
    w2, b2 = (0.03 * torch.randn(D, 1536, generator=gen)).to(gpu).to(torch.bfloat16), (0.1 * torch.randn(D, generator=gen)).to(gpu)
    y, (mean, rstd, h, gd, u) = ops.mlp_fwd(xc.to(gpu), gamma, beta, w1, b1, w2, b2, 1e-6, save=True)
    _finite(y=y, mean=mean, rstd=rstd, h=h)
    z = b1[None, :].expand(rows, 1536)
    u_ref, g_ref = sc.gelu_ref(z)
    _gelu_check('mlp_fwd gd', gd, g_ref, z, torch.bfloat16)
    _gelu_check('mlp_fwd u', u, u_ref, z, torch.bfloat16)
