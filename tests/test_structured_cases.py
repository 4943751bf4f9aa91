"""The value-structured inputs do what they claim, and a faithful fp32 model of the tiled attention arithmetic stays inside the
elementwise bounds that tests/test_gpu_structured.py asserts of the kernels - no GPU needed.

The model (structured_cases.model_fwd / model_bwd) is test code: 64-key tiles, 16-query groups sharing one branch, the reference
maximum that moves only past + 8 log2 units, bf16 P into P V, dQ with the delta estimated from the bf16 O and corrected at the
end.  Its two mutants (no l rescale; correction added instead of subtracted) are far outside the bounds on the inputs built for
them and indistinguishable on randn: the inputs, not the tolerance, are what catches them.
"""
import functools

import pytest
import torch

import structured_cases as sc

SHAPES = [(129, 321), (257, 1024)]


@functools.lru_cache(maxsize=None)
def _case(kind, nq, nk, hd):
    """One head: operands, fp64 truth and bounds, the model's outputs."""
    gen = torch.Generator().manual_seed(1000 * hd + nq + len(kind))
    q, k, v = sc.attention_operands(kind, nq, nk, hd, gen)
    do = sc.bf(torch.randn(nq, hd, generator=gen))
    scale = hd ** -0.5
    truth, bound = sc.attention_truth(q[None], k[None], v[None], do[None], 1, scale, 2.0 ** -7)
    truth = {n: t[0] for n, t in truth.items()}
    bound = {n: t[0] for n, t in bound.items()}
    o, lse, rescales = sc.model_fwd(q, k, v, scale)
    return dict(q=q, k=k, v=v, do=do, scale=scale, truth=truth, bound=bound, o=o, lse=lse, rescales=rescales)


@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('nq,nk', SHAPES)
@pytest.mark.parametrize('kind', sc.ATTENTION_KINDS)
def test_model_is_inside_every_bound(kind, nq, nk, hd):
    c = _case(kind, nq, nk, hd)
    t, b = c['truth'], c['bound']
    dq, dk, dv = sc.model_bwd(c['q'], c['k'], c['v'], c['o'], c['do'], c['lse'], c['scale'])
    ratios = dict(o=sc.ratio(c['o'], t['o'], b['o']), lse=sc.lse_ratio(c['lse'], t['lse'][0]), dq=sc.ratio(dq, t['dq'], b['dq']),
                  dk=sc.ratio(dk, t['dk'], b['dk']), dv=sc.ratio(dv, t['dv'], b['dv']))
    print(kind, nq, nk, hd, {n: round(r, 3) for n, r in ratios.items()})
    assert all(r <= 1.0 for r in ratios.values()), ratios


@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('nq,nk', SHAPES)
@pytest.mark.parametrize('kind', sc.ATTENTION_KINDS)
def test_inputs_do_what_they_claim(kind, nq, nk, hd):
    c = _case(kind, nq, nk, hd)
    for name in ('q', 'k', 'v', 'do'):
        assert torch.equal(c[name], sc.bf(c[name])), name            # bf16 round trip
    rescales = c['rescales']
    assert rescales.numel() == (nq + 15) // 16
    s_max = float((c['q'].double() @ c['k'].double().t()).abs().max()) * c['scale']
    if kind in ('randn', 'uniform', 'voffset'):
        assert int(rescales.sum()) == 0                               # after tile 0 the reference maximum never moves
    if kind == 'rising':
        assert bool((rescales > 0).all()), rescales                   # every 16-query group rescales with a finite maximum
        steps = sc.tile_steps(c['q'], c['k'], c['scale'])
        up = steps[::8]                                               # the rows with b = 1: their tile maxima follow RISING_STEPS
        assert bool((up > sc.LAZY_NATS + 0.5).any()) and bool(((up > 1.0) & (up < sc.LAZY_NATS - 0.5)).any())
        assert bool((steps < -1.0).any()) and bool((steps.abs() < 0.6).any())     # falling rows, flat rows
    if kind == 'onehot':
        assert s_max > 88.0                                           # exp overflows fp32 without the maximum subtraction
        p_max = torch.softmax((c['q'].double() @ c['k'].double().t()) * c['scale'], -1).amax(1)
        assert float(p_max.min()) > 0.5
    if kind == 'uniform':
        s = (c['q'].double() @ c['k'].double().t()) * c['scale']
        assert torch.equal(s, s[:, :1].expand_as(s))                  # identical keys: P = 1 / nk exactly
        torch.testing.assert_close(c['truth']['o'], c['v'].double().mean(0).expand(nq, hd), rtol=1e-12, atol=1e-12)
    if kind == 'voffset':
        assert float(c['truth']['o'].abs().min()) > 12.0


@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('nq,nk', SHAPES)
def test_forgotten_l_rescale_needs_rising_maxima(nq, nk, hd):
    """Mutant (a): l is not multiplied by alpha.  Bit-identical to the model on randn, outside the o bound and the lse
    tolerance on 'rising'."""
    c = _case('randn', nq, nk, hd)
    o, lse, _ = sc.model_fwd(c['q'], c['k'], c['v'], c['scale'], rescale_l=False)
    assert torch.equal(o, c['o']) and torch.equal(lse, c['lse'])
    c = _case('rising', nq, nk, hd)
    o, lse, _ = sc.model_fwd(c['q'], c['k'], c['v'], c['scale'], rescale_l=False)
    r_o, r_lse = sc.ratio(o, c['truth']['o'], c['bound']['o']), sc.lse_ratio(lse, c['truth']['lse'][0])
    print('no l rescale, rising', nq, nk, hd, 'o', round(r_o, 1), 'lse', round(r_lse, 1))
    assert r_o > 10.0 and r_lse > 100.0


@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('nq,nk', SHAPES)
def test_delta_correction_sign_needs_a_value_offset(nq, nk, hd):
    """Mutant (b): dq + corr * bq.  On randn it passes the rtol = atol = 2e-2 of test_attention_fwd_bwd and stays inside the
    elementwise bound; with v = 16 + randn it is outside both."""
    c = _case('randn', nq, nk, hd)
    dq, _, _ = sc.model_bwd(c['q'], c['k'], c['v'], c['o'], c['do'], c['lse'], c['scale'], corr_sign=-1.0)
    assert torch.allclose(dq.double(), c['truth']['dq'], rtol=2e-2, atol=2e-2)
    assert sc.ratio(dq, c['truth']['dq'], c['bound']['dq']) <= 1.0
    c = _case('voffset', nq, nk, hd)
    dq, _, _ = sc.model_bwd(c['q'], c['k'], c['v'], c['o'], c['do'], c['lse'], c['scale'], corr_sign=-1.0)
    r = sc.ratio(dq, c['truth']['dq'], c['bound']['dq'])
    print('+ corr * bq, voffset', nq, nk, hd, round(r, 1))
    assert r > 5.0 and not torch.allclose(dq.double(), c['truth']['dq'], rtol=2e-2, atol=2e-2)


def test_value_offset_leaves_dq_and_dk_where_they_are():
    """Softmax backward is invariant to a constant added to every row of V: the fp64 dQ and dK of v and of v - 16 agree."""
    c = _case('voffset', 129, 321, 32)
    t0, _ = sc.attention_truth(c['q'][None], c['k'][None], (c['v'] - sc.V_OFFSET)[None], c['do'][None], 1, c['scale'], 2.0 ** -7)
    for name in ('dq', 'dk'):
        torch.testing.assert_close(t0[name][0], c['truth'][name], rtol=0, atol=1e-12)


def test_layernorm_rows_and_the_exact_mean_allowance():
    """Rows 1024 + round(8 randn) / 8: an fp32 two-pass LayerNorm is inside (existing tolerance + 2 ulp(|mu|) rstd |gamma|), a
    one-pass E[x^2] - mu^2 variance is far outside; constant rows give y = beta and rstd = eps^-1/2 exactly in fp32."""
    d = 384
    x, kinds = sc.layernorm_rows(657, d, 7)
    assert {'mean1024', 'spike', 'const0', 'const1', 'const2', 'randn'} == set(kinds)
    gen = torch.Generator().manual_seed(8)
    g, b = 1 + 0.2 * torch.randn(d, generator=gen), 0.1 * torch.randn(d, generator=gen)
    ref = torch.nn.functional.layer_norm(x.double(), (d,), g.double(), b.double(), 1e-6)
    mu64 = x.double().mean(1, keepdim=True)
    rstd64 = (x.double().var(1, unbiased=False, keepdim=True) + 1e-6).rsqrt()
    mu = x.sum(1, keepdim=True) * torch.tensor(1.0 / d)
    dd = x - mu
    y2 = dd * torch.rsqrt((dd * dd).sum(1, keepdim=True) * torch.tensor(1.0 / d) + 1e-6) * g + b
    y1 = dd * torch.rsqrt((x * x).sum(1, keepdim=True) * torch.tensor(1.0 / d) - mu * mu + 1e-6) * g + b
    big = torch.tensor([k == 'mean1024' for k in kinds])
    allow = 1e-5 + 1e-5 * ref.abs() + 2 * sc.ulp32(mu64) * rstd64 * g.double().abs()
    assert float(((mu.double() - mu64).abs() / sc.ulp32(mu64))[big].max()) <= 2.0
    assert float(((y2.double() - ref).abs() / allow)[big].max()) <= 1.0
    one_pass = (y1.double() - ref).abs() / allow
    assert not bool(torch.isfinite(y1[big]).all()) or float(one_pass[big].max()) > 50.0
    const = torch.tensor([k.startswith('const') for k in kinds])
    assert torch.equal(y2[const], b.expand(int(const.sum()), d))
    torch.testing.assert_close(rstd64[const], torch.full_like(rstd64[const], 1e3), rtol=1e-12, atol=0)


def test_layernorm_backward_reference_is_taken_at_the_statistics_passed_in():
    """structured_cases.layernorm_bwd_ref equals fp64 autograd through F.layer_norm at the row's own statistics.  Handed the fp32
    roundings of those statistics - what the GPU test passes to the kernels - an fp32 evaluation of the same formula stays inside
    the plain tolerances of test_layernorm_fwd_bwd against the reference AT those numbers, while fp32 PyTorch autograd, judged
    against fp64 autograd at the exact mean, is several times outside on the rows around 1024: that comparison would measure the
    rounding of the operand."""
    d = 384
    for rows in (196, 657):
        x, kinds = sc.layernorm_rows(rows, d, 41 + rows)
        gen = torch.Generator().manual_seed(42)
        g, b = 1 + 0.2 * torch.randn(d, generator=gen), 0.1 * torch.randn(d, generator=gen)
        dy = torch.randn(rows, d, generator=torch.Generator().manual_seed(43))
        xd, gd, bd = (t.double().requires_grad_() for t in (x, g, b))
        torch.nn.functional.layer_norm(xd, (d,), gd, bd, 1e-6).backward(dy.double())
        mean64 = x.double().mean(1)
        rstd64 = (x.double().var(1, unbiased=False) + 1e-6).rsqrt()
        dx, dg, db = sc.layernorm_bwd_ref(dy, x, g, mean64, rstd64)
        torch.testing.assert_close(dx, xd.grad, rtol=1e-9, atol=1e-9)
        torch.testing.assert_close(dg, gd.grad, rtol=1e-9, atol=1e-9)
        torch.testing.assert_close(db, bd.grad, rtol=1e-9, atol=1e-9)
        mean, rstd = mean64.float(), rstd64.float()
        dx_ref, dg_ref, _ = sc.layernorm_bwd_ref(dy, x, g, mean, rstd)
        xhat = (x - mean[:, None]) * rstd[:, None]                  # fp32, the formula of the kernels
        gg = dy * g
        c1, c2 = gg.sum(1, keepdim=True) * torch.tensor(1.0 / d), (gg * xhat).sum(1, keepdim=True) * torch.tensor(1.0 / d)
        dx32 = rstd[:, None] * (gg - c1 - xhat * c2)
        plain = lambda got, want: float(((got.double() - want).abs() / (1e-5 + 1e-4 * want.abs())).max())
        assert plain(dx32, dx_ref) <= 1.0
        assert float((((dy * xhat).sum(0).double() - dg_ref).abs() / (1e-4 * rows ** 0.5 + 1e-4 * dg_ref.abs())).max()) <= 1.0
        x32 = x.clone().requires_grad_()
        torch.nn.functional.layer_norm(x32, (d,), g, b, 1e-6).backward(dy)
        big = torch.tensor([k == 'mean1024' for k in kinds])
        assert plain(x32.grad[big], xd.grad[big]) > 2.0


def test_gelu_grid_covers_the_tails_and_both_zeros():
    z = sc.gelu_grid()
    assert torch.equal(z, sc.bf(z))
    zeros = z[z == 0]
    assert zeros.numel() == 3 and int(torch.signbit(zeros).sum()) == 1
    assert float(z.abs().max()) > 9e3 and bool(((z.abs() > 5) & (z.abs() <= 12)).sum() > 100)
    u, g = sc.gelu_ref(z)
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(g).all())
    assert float(g[torch.signbit(z) & (z == 0)]) == 0.5
