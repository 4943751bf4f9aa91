"""The exact operands of tests/exact_cases.py do what they claim - no GPU needed.

  * The truth is order-free: the same contraction evaluated in fp32 in three different orders (ascending k-panels of 32, descending
    panels of 64, split-K slabs summed afterwards) equals the fp64 product bit for bit, for the NT operands and for the
    weight-gradient operands.  That is what lets tests/test_gpu_exact.py hold every GEMM kernel to torch.equal.
  * The comparison is meaningful: most outputs are NOT bf16 numbers (the store has to round) and a good share are exact ties
    (round-to-even has to decide).
  * Seven torch-restated kernel defects each differ from the truth; the four that are pure rounding defects pass the suite's
    rtol = atol = 1e-2 against fp64 on randn operands, which is why the exact tests exist.
"""
import functools

import pytest
import torch

import exact_cases as ec

M, N, K = 257, 768, 384
BF16_OUT = dict(rtol=1e-2, atol=1e-2)   # the bound of tests/test_gpu_ops.py


@functools.lru_cache(maxsize=None)
def _nt(scale='wide'):
    ops = ec.nt_operands(M, N, K, 7, scale)
    ops['aux'] = ec.mul_aux(M, N, 8)
    ec.guard_nt(ops['a'], ops['w'], ops['bias'], ops['residual'], ops['aux'])
    ops['z'] = ec.nt_truth(ops['a'], ops['w'], ops['bias'])
    return ops


@functools.lru_cache(maxsize=None)
def _wgrad():
    dy, x = ec.wgrad_operands(1000, 200, 136, 9)
    ec.guard_wgrad(dy, x)
    return dy, x


@functools.lru_cache(maxsize=None)
def _randn():
    """The operands of the other GPU tests: bf16-rounded randn, outputs about 1 in size."""
    gen = torch.Generator().manual_seed(10)
    a = ec.bf(torch.randn(M, K, generator=gen))
    w = ec.bf(torch.randn(N, K, generator=gen) * K ** -0.5)
    bias = torch.randn(N, generator=gen)
    aux = ec.bf(torch.randn(M, N, generator=gen))
    z = a.double() @ w.double().t() + bias.double()
    return dict(a=a, w=w, bias=bias, aux=aux, z=z)


def _panels(a, w, width, descending):
    """fp32 a w^T accumulated panel by panel along k."""
    acc = torch.zeros(a.shape[0], w.shape[0])
    starts = list(range(0, a.shape[1], width))
    for k0 in (reversed(starts) if descending else starts):
        acc = acc + a[:, k0:k0 + width] @ w[:, k0:k0 + width].t()
    return acc


def _split_k(a, w, splits):
    """fp32 partial products over ``splits`` slabs of k, summed afterwards (last slab first)."""
    step = -(-a.shape[1] // splits)
    slabs = [a[:, k0:k0 + step] @ w[:, k0:k0 + step].t() for k0 in range(0, a.shape[1], step)]
    acc = torch.zeros_like(slabs[0])
    for s in reversed(slabs):
        acc = acc + s
    return acc


def _orders(a, w):
    return dict(ascending_32=_panels(a, w, 32, False), descending_64=_panels(a, w, 64, True), split_k_3=_split_k(a, w, 3),
                split_k_7=_split_k(a, w, 7))


@pytest.mark.parametrize('scale', ['wide', 'gelu'])
def test_nt_truth_is_the_same_in_every_order(scale):
    c = _nt(scale)
    truth = ec.nt_truth(c['a'], c['w'], c['bias'], c['residual'])
    for name, acc in _orders(c['a'], c['w']).items():
        assert acc.dtype == torch.float32
        assert torch.equal(acc.double(), ec.nt_truth(c['a'], c['w'])), name
        # the epilogue's two fp32 additions, in both orders
        assert torch.equal(((acc + c['bias']) + c['residual']).double(), truth), name
        assert torch.equal((acc + (c['bias'] + c['residual'])).double(), truth), name


def test_weight_gradient_truth_is_the_same_in_every_order():
    dy, x = _wgrad()
    dw, db = ec.wgrad_truth(dy, x)
    # dW = dy^T x contracts over the ROWS: panels and split-K slabs of rows
    for name, acc in _orders(dy.t().contiguous(), x.t().contiguous()).items():
        assert torch.equal(acc.double(), dw), name
    for step in (32, 64, 334):
        parts = [dy[r0:r0 + step].sum(0) for r0 in range(0, dy.shape[0], step)]
        assert torch.equal(torch.stack(parts[::-1]).sum(0).double(), db), step
    # accumulated onto integer-valued content
    gen = torch.Generator().manual_seed(11)
    dw0, db0 = ec.ints(dw.shape, 64, gen), ec.ints(db.shape, 64, gen)
    ec.guard_wgrad(dy, x, dw0, db0)
    dw1, db1 = ec.wgrad_truth(dy, x, dw0, db0)
    assert torch.equal((dw0 + _split_k(dy.t().contiguous(), x.t().contiguous(), 3)).double(), dw1)
    assert torch.equal((db0 + dy.sum(0)).double(), db1)


def test_layernorm_bwd_column_sums_are_the_same_in_every_order():
    dy, wt = ec.ln_bwd_operands(1000, 384, 384, 12)
    ec.guard_nt(dy, wt)
    dh = ec.nt_truth(dy, wt)
    ec.guard_colsum(dh)
    dh32 = _panels(dy, wt, 32, False)
    assert torch.equal(dh32.double(), dh)
    for tile in (96, 128, 144, 160):
        parts = [dh32[r0:r0 + tile].sum(0) for r0 in range(0, 1000, tile)]
        assert torch.equal(torch.stack(parts).sum(0).double(), dh.sum(0)), tile


def test_guard_refuses_operands_that_can_round():
    c = _nt()
    with pytest.raises(AssertionError, match='bf16'):
        ec.guard_nt(c['a'] + 1 / 512, c['w'])
    with pytest.raises(AssertionError, match='multiple'):
        ec.guard_nt(c['a'], c['w'], residual=c['residual'] + 1 / 32)
    with pytest.raises(AssertionError, match='partial sum'):
        ec.guard_nt(c['a'] * 1024, c['w'])
    with pytest.raises(AssertionError, match='fp32'):
        # z = 255 * 509 / 16 has 17 significant bits, aux = 255 / 128 eight: the product needs 25
        ec.guard_nt(torch.tensor([[255.0, 255.0]]), torch.tensor([[255.0, 254.0]]) / 16, aux=torch.tensor([[255.0 / 128]]))
    dy, x = _wgrad()
    with pytest.raises(AssertionError, match='partial sum'):
        ec.guard_wgrad(dy * 128, x)
    with pytest.raises(AssertionError, match='partial sum'):
        ec.guard_colsum(dy * 1024)


def test_outputs_need_rounding_and_hit_ties():
    """Measured on these operands: 72 % of the outputs are not bf16 numbers, 16 % are exact ties."""
    c = _nt()
    z32 = ec.as_f32(c['z'])
    assert torch.equal(z32.double(), c['z'])
    rounded, ties = float(ec.needs_rounding(z32).float().mean()), float(ec.is_tie(z32).float().mean())
    print(f'\nexact operands ({M}, {N}, {K}): {100 * rounded:.1f} % of the outputs need rounding, {100 * ties:.1f} % are ties')
    assert rounded >= 0.5 and ties >= 0.01
    # ties go to even: the kept mantissa bit of the result is 0 on every tie
    t = ec.is_tie(z32)
    kept = ec.as_bf16(c['z']).float().view(torch.int32) >> 16
    assert bool(((kept[t] & 1) == 0).all())
    # the GELU scale keeps the pre-activations where the GELU is neither 0 nor the identity
    zg = _nt('gelu')['z']
    print(f'gelu scale: pre-activation spread {float(zg.std()):.2f}')
    assert 3.0 < float(zg.std()) < 6.0


def _rounding_mutants(c):
    """name -> (mutant output, true output) of the four pure rounding defects, on operands c (exact or randn)."""
    z32 = c['z'].float()
    acc = c['a'].double() @ c['w'].double().t()
    return {
        'truncating store': (ec.store_truncating(z32), ec.as_bf16(c['z'])),
        'round half away from zero': (ec.store_half_away(z32), ec.as_bf16(c['z'])),
        'bf16 z before the EPI_MUL multiply': (ec.mul_double_rounding(z32, c['aux']), (z32 * c['aux']).bfloat16()),
        'bf16 hand-off between the K halves': (ec.k_halves_through_bf16(c['a'], c['w']), acc.float().bfloat16()),
    }


def test_rounding_mutants_differ_on_exact_operands_and_pass_the_old_bound_on_randn():
    exact = _nt()
    assert torch.equal(ec.mul_truth(exact['z'], exact['aux']), (exact['z'].float() * exact['aux']).bfloat16())
    for name, (got, want) in _rounding_mutants(exact).items():
        frac = float((got != want).float().mean())
        print(f'\n{name}: {100 * frac:.1f} % of the exact outputs differ')
        assert not torch.equal(got, want), name
        assert frac > 0.05, (name, frac)
    r = _randn()
    acc = r['a'].double() @ r['w'].double().t()
    fp64 = {'truncating store': r['z'], 'round half away from zero': r['z'], 'bf16 z before the EPI_MUL multiply': r['z'] * r['aux'].double(),
            'bf16 hand-off between the K halves': acc}
    for name, (got, _) in _rounding_mutants(r).items():
        torch.testing.assert_close(got.double(), fp64[name], **BF16_OUT)     # invisible to the randn tests


def test_indexing_mutants_differ_on_exact_operands():
    c = _nt()
    want = ec.as_bf16(c['z'])
    got = ec.ragged_tile_drops_k(c['a'], c['w'], c['bias'])
    assert M % 128 != 0 and torch.equal(got[:M // 128 * 128], want[:M // 128 * 128]) and not torch.equal(got[M // 128 * 128:], want[M // 128 * 128:])
    dy, x = _wgrad()
    dw, db = ec.wgrad_truth(dy, x)
    assert not torch.equal(ec.wgrad_last_row_twice(dy, x), ec.as_f32(dw))
    for row in (0, 511, dy.shape[0] - 1):
        assert not torch.equal(ec.bias_grad_row_left_out(dy, row), ec.as_f32(db)), row
