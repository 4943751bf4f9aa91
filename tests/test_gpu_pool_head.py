"""The pooled head on the MI355X: the kernels of csrc/pool_head.hip against the fp64 formula evaluated on the values they read, the
exact identities the arithmetic allows, and models with global_pool='avg' / fc_norm - training, the two-stage and pair-indexed forms,
the pair caches, puzzle distances, captured training steps, combined with stochastic depth, q/k-norm and patch dropout - against the
restatement of tests/pool_cases.py.

Operator tolerances are those of tests/test_gpu_qknorm.py: fp32 outputs rtol 1e-5 / atol 1e-5, a bf16 copy rtol 2^-8 on top, and every
column of d gamma / d beta within 1e-5 x the sum of the |terms| it adds.  Model tolerances are test_gpu_droppath._check_values'."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import droppath_cases as dc
import patchdrop_cases as pc
import pool_cases as plc
import qknorm_cases as qc
from oracle import vited_oracle as vo
from test_gpu_droppath import _check_values, _grads
from test_gpu_puzzle import near_integer, quantise_numpy

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
VARIANTS = list(plc.VARIANTS)
BCE = F.binary_cross_entropy_with_logits
EPS = 1e-6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pool_head.npz')
PATTERN = -1536.0        # exactly representable in bf16 and fp32


# ---------------------------------------------------------------------------------------------
# operator level
# ---------------------------------------------------------------------------------------------
def _rand(shape, gpu, seed, dtype=torch.float32, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return (offset + scale * torch.randn(shape, generator=g)).to(dtype).to(gpu)


def _tol(dtype):
    return dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=2 ** -8, atol=1e-5)


def _ref(x, first, gamma=None, beta=None, g=None):
    """fp64: pooled = mean over t >= first of x[:, t] or of LayerNorm(x[:, t]); with ``g`` also (dx, dgamma, dbeta, the per-column sums of
    |dy xhat| and |dy|) and without it the rows' (mean, rstd)."""
    grad = g is not None
    xd = x.double().clone().requires_grad_(grad)
    y, gd, bd, xhat = xd, None, None, None
    mean = rstd = None
    if gamma is not None:
        gd, bd = gamma.double().clone().requires_grad_(grad), beta.double().clone().requires_grad_(grad)
        mean = xd.mean(-1, keepdim=True)
        rstd = (((xd - mean) ** 2).mean(-1, keepdim=True) + EPS).rsqrt()
        xhat = (xd - mean) * rstd
        y = xhat * gd + bd
    pooled = y[:, first:].mean(1)
    if not grad:
        return pooled.detach(), (mean.detach().squeeze(-1), rstd.detach().squeeze(-1)) if gamma is not None else None
    pooled.backward(g.double())
    if gamma is None:
        return xd.grad, None, None, None, None
    dy = (g.double() / (x.shape[1] - first)).unsqueeze(1)
    return xd.grad, gd.grad, bd.grad, (dy * xhat.detach()[:, first:]).abs().sum((0, 1)), (dy.abs() * (x.shape[1] - first)).sum((0, 1))


def _strided(gpu, items, tokens, d, seed=None, dtype=torch.float32):
    """([items, tokens, d] view, the buffer behind it): rows 1 .. tokens and columns 4 .. 4 + d of a [items, tokens + 2, d + 8] buffer -
    random, or filled with PATTERN when no seed is given."""
    shape = (items, tokens + 2, d + 8)
    buf = _rand(shape, gpu, seed, dtype) if seed is not None else torch.full(shape, PATTERN, dtype=dtype, device=gpu)
    return buf[:, 1:1 + tokens, 4:4 + d], buf


def _untouched_outside(buf, items, tokens, d):
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[:, 1:1 + tokens, 4:4 + d] = True
    return bool((buf[~inside] == PATTERN).all()) and not bool((buf[inside] == PATTERN).any())


def _run_case(vited, gpu, items, tokens, d, norm, lp_dtype, scaled, seed):
    ops = vited.ops
    first = 1
    x, xbuf = _strided(gpu, items, tokens, d, seed)
    before = xbuf.clone()
    gamma, beta = (_rand((d,), gpu, seed + 1, offset=1.0, scale=0.3), _rand((d,), gpu, seed + 2, scale=0.2)) if norm else (None, None)
    pbuf = torch.full((items, d + 8), PATTERN, device=gpu)
    out = pbuf[:, 4:4 + d]
    pooled, mean, rstd = ops.token_pool_fwd(x, first, gamma, beta, EPS, save_stats=norm, out=out)
    assert pooled is out and torch.equal(xbuf, before), 'the forward wrote into its input'
    assert bool((pbuf[:, :4] == PATTERN).all()) and bool((pbuf[:, 4 + d:] == PATTERN).all()) and not bool((out == PATTERN).any())
    want, stats = _ref(x, first, gamma, beta)
    print(f'{items} x {tokens} x {d} norm={norm}: pooled max|d| = {float((pooled.double() - want).abs().max()):.3e}')
    torch.testing.assert_close(pooled.double(), want, **_tol(torch.float32))
    if norm:
        assert mean.shape == rstd.shape == (items * tokens,)
        torch.testing.assert_close(mean.view(items, tokens)[:, first:].double(), stats[0][:, first:], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(rstd.view(items, tokens)[:, first:].double(), stats[1][:, first:], rtol=1e-5, atol=0)
        assert torch.equal(ops.token_pool_fwd(x, first, gamma, beta, EPS)[0], pooled)          # inference: no statistics, the same bits
    assert torch.equal(ops.token_pool_fwd(x, first, gamma, beta, EPS, out=torch.empty_like(pooled))[0], pooled)      # two runs

    g = _rand((items, d), gpu, seed + 3)
    lp_scale = _rand((items,), gpu, seed + 4, offset=1.5, scale=0.25) if scaled else None
    extra = dict(x=x, gamma=gamma, mean=mean, rstd=rstd) if norm else {}

    def backward(**kw):
        dx, dbuf = _strided(gpu, items, tokens, d)
        lp, lbuf = _strided(gpu, items, tokens, d, dtype=lp_dtype) if lp_dtype is not None else (None, None)
        got = ops.token_pool_bwd(g, tokens, first, dx=dx, dx_lp=lp, lp_scale=lp_scale, **extra, **kw)
        assert got[0] is dx and got[1] is lp
        assert _untouched_outside(dbuf, items, tokens, d), 'dx: a byte outside the region was written, or one inside was not'
        assert lp is None or _untouched_outside(lbuf, items, tokens, d), 'dx_lp: outside written, or inside not'
        return got

    dx, lp, dg, db = backward()
    assert torch.equal(xbuf, before)
    dx_ref, dg_ref, db_ref, sum_g, sum_b = _ref(x, first, gamma, beta, g)
    print(f'    dx max|d| = {float((dx.double() - dx_ref).abs().max()):.3e}')
    torch.testing.assert_close(dx.double(), dx_ref, **_tol(torch.float32))
    assert int(torch.count_nonzero(dx[:, :first])) == 0
    if lp is not None:
        assert int(torch.count_nonzero(lp[:, :first])) == 0
        scale = lp_scale.double().view(-1, 1, 1) if scaled else 1.0
        torch.testing.assert_close(lp.double(), dx_ref * scale, **_tol(lp_dtype))
        # the copy is the rounded, scaled dx itself
        assert torch.equal(lp, (dx * lp_scale.view(-1, 1, 1) if scaled else dx).to(lp_dtype))
    if norm:
        print(f'    dgamma max|d| = {float((dg.double() - dg_ref).abs().max()):.3e} (bound {float(1e-5 * sum_g.max()):.1e}), '
              f'dbeta max|d| = {float((db.double() - db_ref).abs().max()):.3e}')
        assert bool(((dg.double() - dg_ref).abs() <= 1e-5 * sum_g).all())
        assert bool(((db.double() - db_ref).abs() <= 1e-5 * sum_b).all())
    else:
        assert dg is None and db is None
    again = backward()
    for a, b in zip(again, (dx, lp, dg, db)):
        assert (a is None and b is None) or torch.equal(a, b)
    if norm:        # accumulation: onto given destinations the sums are ADDED - twice gives base + 2 x
        dest = [_rand((d,), gpu, seed + 5), _rand((d,), gpu, seed + 6)]
        base = [t.clone() for t in dest]
        for _ in range(2):
            got = backward(dgamma=dest[0], dbeta=dest[1])
            assert got[2] is dest[0] and got[3] is dest[1]
        for t, b0, s in zip(dest, base, (dg, db)):
            assert torch.equal(t, (b0 + s) + s)


# 3 x 2: one pooled token; 3 x 5; 7 x 65: one chunk of 64 tokens; 2 x 1025: 16 chunks per item and the fixed-order combine
SHAPES = [(3, 2), (3, 5), (7, 65), (2, 1025)]


@pytest.mark.parametrize('d', [32, 384, 768, 1000])
@pytest.mark.parametrize('items,tokens', SHAPES)
def test_forward_backward_against_fp64(vited, gpu, items, tokens, d):
    """Plain and with a LayerNorm; the low-precision copy bf16 with a per-item scale, fp32 without one (and absent, scaled fp32 and
    unscaled bf16 at D = 384)."""
    for norm in (False, True):
        _run_case(vited, gpu, items, tokens, d, norm, torch.bfloat16, True, seed=items + tokens + d)
        _run_case(vited, gpu, items, tokens, d, norm, torch.float32, False, seed=items + tokens + d + 50)
        if d == 384:
            _run_case(vited, gpu, items, tokens, d, norm, None, False, seed=items + tokens + d + 100)
            _run_case(vited, gpu, items, tokens, d, norm, torch.float32, True, seed=items + tokens + d + 150)
            _run_case(vited, gpu, items, tokens, d, norm, torch.bfloat16, False, seed=items + tokens + d + 200)


def test_chunks_that_do_not_divide_the_tokens(vited, gpu):
    """100 tokens behind no prefix and 131 behind one: 64 + 36 and 64 + 64 + 2 pooled tokens; a prefix of 3 rows."""
    _run_case(vited, gpu, 3, 131, 384, True, torch.bfloat16, True, seed=7)
    ops = vited.ops
    for first, tokens in ((0, 100), (3, 12)):
        x = _rand((2, tokens, 64), gpu, 8 + first)
        gamma, beta = _rand((64,), gpu, 9, offset=1.0, scale=0.3), _rand((64,), gpu, 10, scale=0.2)
        for gm, bt in ((None, None), (gamma, beta)):
            pooled, mean, rstd = ops.token_pool_fwd(x, first, gm, bt, EPS, save_stats=gm is not None)
            torch.testing.assert_close(pooled.double(), _ref(x, first, gm, bt)[0], **_tol(torch.float32))
            g = _rand((2, 64), gpu, 11)
            kw = dict(x=x, gamma=gm, mean=mean, rstd=rstd) if gm is not None else {}
            dx = ops.token_pool_bwd(g, tokens, first, **kw)[0]
            torch.testing.assert_close(dx.double(), _ref(x, first, gm, bt, g)[0], **_tol(torch.float32))
            assert int(torch.count_nonzero(dx[:, :first])) == 0


@pytest.mark.parametrize('tokens', [65, 1025])
def test_exact_mean_of_dyadic_values(vited, gpu, tokens):
    """Inputs that are multiples of 2^-8 in [-1, 1] with 64 and 1,024 pooled tokens: every partial sum is a multiple of 2^-8 below 2^11,
    exact in fp32 in any order, and so is the division by a power of two - the plain mean equals the fp64 one bit for bit; so does the
    backward's g / count."""
    ops = vited.ops
    gen = torch.Generator().manual_seed(tokens)
    x = (torch.randint(-256, 257, (3, tokens, 384), generator=gen).float() / 256).to(gpu)
    pooled, _, _ = ops.token_pool_fwd(x, 1)
    want = x.double()[:, 1:].mean(1)
    assert torch.equal(pooled.double(), want) and float(want.abs().max()) > 0
    g = (torch.randint(-256, 257, (3, 384), generator=gen).float() / 256).to(gpu)
    dx, lp, _, _ = ops.token_pool_bwd(g, tokens, 1, lp_dtype=torch.float32)
    assert torch.equal(dx[:, 1:].double(), (g.double() / (tokens - 1)).unsqueeze(1).expand(-1, tokens - 1, -1)) and torch.equal(lp, dx)
    assert int(torch.count_nonzero(dx[:, 0])) == 0


def test_bad_arguments_raise(vited, gpu):
    ops = vited.ops
    x = torch.zeros(2, 5, 32, device=gpu)
    g = torch.zeros(2, 32, device=gpu)
    w = torch.ones(32, device=gpu)
    with pytest.raises(ValueError, match='x '):
        ops.token_pool_fwd(x.bfloat16())
    with pytest.raises(ValueError, match='x '):
        ops.token_pool_fwd(x[0])                                    # rank
    with pytest.raises(ValueError, match='x '):
        ops.token_pool_fwd(torch.zeros(2, 32, 5, device=gpu).transpose(1, 2))      # the last dim is not dense
    with pytest.raises(ValueError, match='x '):
        ops.token_pool_fwd(torch.zeros(2, 5, 34, device=gpu)[:, :, 2:])             # 8 bytes into a 16-byte line
    with pytest.raises(ValueError, match='nothing to pool'):
        ops.token_pool_fwd(x, first=5)
    with pytest.raises(ValueError, match='dim 1028'):
        ops.token_pool_fwd(torch.zeros(1, 2, 1028, device=gpu))
    with pytest.raises(ValueError, match='gamma and beta'):
        ops.token_pool_fwd(x, 1, w, None)
    with pytest.raises(ValueError, match='gamma'):
        ops.token_pool_fwd(x, 1, torch.ones(16, device=gpu), torch.ones(16, device=gpu))
    with pytest.raises(ValueError, match='save_stats'):
        ops.token_pool_fwd(x, 1, save_stats=True)
    with pytest.raises(ValueError, match='workspace'):
        ops.token_pool_fwd(torch.zeros(2, 130, 32, device=gpu), 1, workspace=torch.zeros(8, device=gpu))
    with pytest.raises(RuntimeError, match='CPU tensor'):
        ops.token_pool_fwd(x, 1, w.cpu(), w.cpu())
    with pytest.raises(ValueError, match='g '):
        ops.token_pool_bwd(g.bfloat16(), 5)
    with pytest.raises(ValueError, match='dx '):
        ops.token_pool_bwd(g, 5, dx=torch.zeros(2, 4, 32, device=gpu))
    with pytest.raises(ValueError, match='lp_scale'):
        ops.token_pool_bwd(g, 5, lp_scale=torch.ones(2, device=gpu))
    with pytest.raises(ValueError, match='lp_scale'):
        ops.token_pool_bwd(g, 5, lp_dtype=torch.bfloat16, lp_scale=torch.ones(3, device=gpu))
    with pytest.raises(ValueError, match='mean'):
        ops.token_pool_bwd(g, 5, x=x, gamma=w, mean=torch.zeros(4, device=gpu), rstd=torch.zeros(10, device=gpu))
    with pytest.raises(ValueError, match='go with gamma'):
        ops.token_pool_bwd(g, 5, mean=torch.zeros(10, device=gpu))
    with pytest.raises((ValueError, TypeError), match='dx_lp'):
        ops.token_pool_bwd(g, 5, dx_lp=torch.zeros(2, 5, 32, device=gpu, dtype=torch.float16))


# ---------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------
def _options(variant):
    global_pool, fc_norm = plc.VARIANTS[variant]
    return dict(global_pool=global_pool, fc_norm=fc_norm)


def _hip_model(vited, s, gpu, dtype, variant, state=None, **kw):
    m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                      embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads,
                                      mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, **_options(variant), **kw)
    m.compute_dtype = dtype
    if state is not None:
        m.load_state_dict(state)
    return m.to(gpu)


def _random_oracle(s, seed, variant, qk=False):
    """The oracle's init with the head's norm (and the q/k-norms) moved off weight 1 / bias 0, which would hide a swapped parameter."""
    torch.manual_seed(seed)
    m = (plc.PoolQKNormViTED if qk else plc.PoolViTED)(s, **_options(variant))
    gen = torch.Generator().manual_seed(seed + 1000)
    if qk:
        qc.randomize_norms_(m, gen)
    norm = m.fc_norm if m.use_fc_norm else m.norm
    with torch.no_grad():
        norm.weight.copy_(1.0 + 0.2 * torch.randn(norm.weight.shape, generator=gen))
        norm.bias.copy_(0.1 * torch.randn(norm.bias.shape, generator=gen))
    return m


def _batch(s, batch, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(batch, 2, 3, s.img_size, s.img_size, generator=g).clamp(-1, 1),
            (torch.rand(batch, s.num_classes, generator=g) > 0.6).float())


def _one_shot(vited, gpu, dtype, s, batch, seed, variant, prepare=None):
    oracle = _random_oracle(s, seed, variant)
    model = _hip_model(vited, s, gpu, dtype, variant, state=oracle.state_dict()).train()
    if prepare is not None:
        prepare(model)
    x, y = _batch(s, batch, seed + 1)
    lo = oracle(x)
    _, go = plc.loss_and_grads(oracle, lo, y)
    lh = model(x.to(gpu))
    BCE(lh, y.to(gpu)).backward()
    gh = _grads(model)
    assert set(gh) == set(go)
    return model, lh.detach().cpu(), gh, lo.detach(), go


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('variant', VARIANTS)
def test_small_model_against_the_restatement(vited, gpu, variant, which, dtype):
    """The golden geometries (5 tokens; 1 + 2 blocks at head_dim 32, 2 + 1 at head_dim 64, where the only decoder block is the last)."""
    s = plc.GOLDEN_SHAPES[which]
    model, lh, gh, lo, go = _one_shot(vited, gpu, dtype, s, plc.GOLDEN_BATCH, 10 * which + VARIANTS.index(variant), variant)
    assert model.runtime().cls_tail is (variant == 'token_fc')
    _check_values(dtype, lh, gh, lo, go)


@pytest.mark.parametrize('variant', VARIANTS)
def test_small_model_against_the_reference_fixture(vited, gpu, variant):
    """Golden shape 0 in fp32 on the fixture's closed-form weights and inputs: the logits the reference's own class gave."""
    fx = np.load(GOLDEN)
    s = plc.GOLDEN_SHAPES[0]
    state = plc.fill_closed_form_(plc.PoolViTED(s, **_options(variant))).state_dict()
    model = _hip_model(vited, s, gpu, torch.float32, variant, state=state)
    x, y = plc.golden_inputs(s)
    lh = model(x.to(gpu))
    loss = BCE(lh, y.to(gpu))
    torch.testing.assert_close(lh.detach().cpu().double(), torch.from_numpy(fx[f'logits_{variant}0']), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(float(loss), float(fx[f'loss_{variant}0']), rtol=1e-4)


class _Recorder:
    """Records (entry point, its small integer arguments: sizes, strides, codes - never a pointer) of every call that reaches the library."""

    def __init__(self, vited):
        self.lib, self.real, self.calls = vited._lib, vited._lib.call, []

    def __enter__(self):
        def call(name, *args):
            self.calls.append((name, tuple(a for a in args if isinstance(a, int) and not isinstance(a, bool) and 0 < a < 1 << 24)))
            return self.real(name, *args)
        self.lib.call = call
        return self

    def __exit__(self, *exc):
        self.lib.call = self.real
        return False

    def names(self):
        return [n for n, _ in self.calls]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('variant', ['avg', 'avg_nofc'])
def test_config_a_geometry(vited, gpu, variant, dtype):
    """D 384, 12 heads, 64 / 65 tokens, 1 + 2 blocks, B 8: under 'avg' no decoder block runs on the cls rows alone, and the pooling
    kernels are reached once each way."""
    s = vo.ViTEDShape(depth=1, c_depth=2)
    F_ = vited.functions
    cls_only = []
    real_f, real_b = F_._dec_self_fwd, F_._dec_self_bwd
    F_._dec_self_fwd = lambda rt, x, P, batch, n, cls, **k: cls_only.append(cls) or real_f(rt, x, P, batch, n, cls, **k)
    F_._dec_self_bwd = lambda rt, dx, dx_lp, x, P, saved, batch, n, cls, **k: cls_only.append(cls) or real_b(rt, dx, dx_lp, x, P, saved, batch, n, cls, **k)
    try:
        with _Recorder(vited) as rec:
            model, lh, gh, lo, go = _one_shot(vited, gpu, dtype, s, 8, 20 + VARIANTS.index(variant), variant)
    finally:
        F_._dec_self_fwd, F_._dec_self_bwd = real_f, real_b
    assert cls_only == [False] * 4 and not model.runtime().cls_tail
    names = rec.names()
    assert names.count('vited_token_pool_fwd') == 1 and names.count('vited_token_pool_bwd') == 1
    _check_values(dtype, lh, gh, lo, go)
    # the default model on the same geometry does take the cls-only last block
    cls_only.clear()
    F_._dec_self_fwd = lambda rt, x, P, batch, n, cls, **k: cls_only.append(cls) or real_f(rt, x, P, batch, n, cls, **k)
    try:
        with torch.no_grad():
            vited.VisionTransformerCustom(img_size=64, patch_size=8, num_classes=4, embed_dim=384, depth=1, c_depth=2, num_heads=12).to(gpu)(
                torch.zeros(2, 2, 3, 64, 64, device=gpu))
    finally:
        F_._dec_self_fwd = real_f
    assert cls_only == [False, True]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('variant', VARIANTS)
def test_with_stochastic_depth(vited, gpu, variant, dtype):
    """Forced scales, 2 + 2 blocks, B 8: the last block's MLP scale rides on the pooled backward's low-precision copy, per sample."""
    s = vo.ViTEDShape(depth=2, c_depth=2)
    oracle = _random_oracle(s, 30, variant)
    model = _hip_model(vited, s, gpu, dtype, variant, state=oracle.state_dict(), drop_path_rate=0.5).train()
    x, y = _batch(s, 8, 31)
    enc, dec = dc.irregular_scales(0.5, s.depth, 2, 8, salt=3), dc.irregular_scales(0.5, s.c_depth, 3, 8, salt=5)
    lo = plc.forward(oracle, x, enc=enc, dec=dec)
    _, go = plc.loss_and_grads(oracle, lo, y)
    seen = []
    ops = vited.ops
    real = ops.token_pool_bwd
    ops.token_pool_bwd = lambda *a, **k: seen.append(k.get('lp_scale')) or real(*a, **k)
    try:
        lh = model(x.to(gpu), drop_path=vited.DropPathScales(enc.to(gpu), dec.to(gpu)))
        BCE(lh, y.to(gpu)).backward()
    finally:
        ops.token_pool_bwd = real
    if variant != 'token_fc':
        assert len(seen) == 1 and seen[0] is not None and tuple(seen[0].shape) == (8,) and torch.equal(seen[0].cpu(), dec[1, 2])
    _check_values(dtype, lh.detach().cpu(), _grads(model), lo.detach(), go)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('variant', ['avg', 'avg_nofc'])
def test_with_qk_norm(vited, gpu, variant, dtype):
    s = plc.GOLDEN_SHAPES[0]
    oracle = _random_oracle(s, 40, variant, qk=True)
    model = _hip_model(vited, s, gpu, dtype, variant, state=oracle.state_dict(), qk_norm=True).train()
    x, y = _batch(s, 3, 41)
    lo = oracle(x)
    _, go = plc.loss_and_grads(oracle, lo, y)
    lh = model(x.to(gpu))
    BCE(lh, y.to(gpu)).backward()
    gh = _grads(model)
    zero = [n for n in go if n.endswith('k_norm.bias')]       # zero in exact arithmetic (tests/test_qknorm.py): noise against the weight's gradient
    tol = 1e-3 if dtype == torch.float32 else 5e-2
    for n in zero:
        assert float(gh[n].norm()) <= tol * float(go[n.replace('.bias', '.weight')].norm()), n
    _check_values(dtype, lh.detach().cpu(), {n: g for n, g in gh.items() if n not in zero}, lo.detach(), {n: g for n, g in go.items() if n not in zero})


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('variant', ['avg', 'avg_nofc'])
def test_with_patch_dropout(vited, gpu, variant, dtype):
    """patch_drop_rate 0.5 with forced keep indices on 64-pixel images: the decoder runs on 1 + 32 tokens and the mean is over the 32
    kept ones.  Against the restatement (the reference's own class is not run with patch dropout anywhere in this suite)."""
    s = vo.ViTEDShape(depth=1, c_depth=2)
    oracle = _random_oracle(s, 50, variant)
    model = _hip_model(vited, s, gpu, dtype, variant, state=oracle.state_dict(), patch_drop_rate=0.5).train()
    x, y = _batch(s, 4, 51)
    k1, k2 = model.patch_keep_counts
    assert (k1, k2) == (pc.keep_count(s.n1 - 1, 0.5), pc.keep_count(s.n1, 0.5)) == (31, 32)
    keep1, keep2 = pc.closed_form_keep(4, s.n1 - 1, k1, salt=1), pc.closed_form_keep(4, s.n1, k2, salt=2)
    lo = plc.forward(oracle, x, keep1=keep1, keep2=keep2)
    _, go = plc.loss_and_grads(oracle, lo, y)
    with _Recorder(vited) as rec:
        lh = model(x.to(gpu), patch_keep=vited.PatchKeep(keep1.to(gpu), keep2.to(gpu)))
        BCE(lh, y.to(gpu)).backward()
    pool = [a for n, a in rec.calls if n == 'vited_token_pool_fwd']
    assert len(pool) == 1 and 1 + k2 in pool[0] and s.n2 not in pool[0], pool       # tokens = 1 + K
    _check_values(dtype, lh.detach().cpu(), _grads(model), lo.detach(), go)
    # it is the mean over the KEPT tokens: the restatement on all tokens gives other logits
    assert not torch.allclose(plc.forward(oracle, x).detach(), lo.detach(), rtol=1e-2, atol=1e-3)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('variant', VARIANTS)
def test_two_stage_equals_one_shot(vited, gpu, variant, dtype):
    """model(x) and model(model(x1, forward_first_part=True), x2): the same launches, the same bits, logits and gradients."""
    s = plc.GOLDEN_SHAPES[1]
    model = _hip_model(vited, s, gpu, dtype, variant, state=_random_oracle(s, 60, variant).state_dict()).train()
    x, y = _batch(s, 4, 61)
    x, y = x.to(gpu), y.to(gpu)
    l1 = model(x)
    BCE(l1, y).backward()
    g1 = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    l2 = model(model(x[:, 0], forward_first_part=True), x[:, 1])
    BCE(l2, y).backward()
    assert torch.equal(l1, l2)
    for n, p in model.named_parameters():
        assert torch.equal(p.grad, g1[n]), n


@pytest.mark.parametrize('dtype', DTYPES)
def test_pair_indexed_form_equals_the_gathered_form(vited, gpu, dtype):
    """hisfrag_prepare_indexed's batch (4 images of 2 writers, 2 + 2 blocks) under 'avg': logits and gradients of the pair-indexed form
    against model(feats[i], x[j]) on the same model, at the figures tests/test_gpu_qknorm.py asks of the two forms; two runs, same bits."""
    s = vo.ViTEDShape(img_size=16, patch_size=8, num_classes=1, embed_dim=128, num_heads=2, depth=2, c_depth=2)
    E = vited.engine
    exact = dtype == torch.float32
    model = _hip_model(vited, s, gpu, dtype, 'avg', state=_random_oracle(s, 70, 'avg').state_dict()).train()
    samples = torch.randn(4, 3, s.img_size, s.img_size, generator=torch.Generator().manual_seed(71)).clamp(-1, 1).to(gpu)
    targets = torch.tensor([0, 0, 1, 1], device=gpu)
    (x, feats, j_idx, seg), labels = E.hisfrag_prepare_indexed(model, samples, targets, amp=not exact,
                                                               generator=torch.Generator(device=gpu).manual_seed(1))
    labels = labels.reshape(-1, 1).float()
    feats = feats.detach().float()

    def indexed():
        model.zero_grad(set_to_none=True)
        f = feats.clone().requires_grad_()
        logits = model(f, samples, x2_index=j_idx, x1_index=seg)
        BCE(logits, labels).backward()
        return logits.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}, f.grad.clone()

    l1, g1, df1 = indexed()
    l2, g2, df2 = indexed()
    assert torch.equal(l1, l2) and torch.equal(df1, df2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    model.zero_grad(set_to_none=True)
    f = feats.clone().requires_grad_()
    lg = model(f[seg.index], samples[j_idx])
    BCE(lg, labels).backward()
    gg = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert set(gg) == set(g1) and 'fc_norm.weight' in g1
    torch.testing.assert_close(l1, lg.detach(), **(dict(rtol=1e-3, atol=1e-5) if exact else dict(rtol=3e-2, atol=3e-2)))
    tol = 1e-3 if exact else 5e-2
    for n in gg:
        err = float((g1[n] - gg[n]).norm() / (gg[n].norm() + 1e-12))
        assert err <= tol, (n, err)
    assert float((df1 - f.grad).norm() / f.grad.norm()) <= tol


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('variant,c_depth', [('avg', 2), ('avg_nofc', 2), ('avg', 1)])
def test_pair_caches(vited, gpu, variant, c_depth, dtype):
    """6 images: pairwise_similarity from the caches equals the uncached form at tests/test_gpu_model.py's rtol / atol 1e-2, and both the
    restatement at that file's 2e-3 (fp32) / 3e-2 (bf16).  c_depth 1: the cached first block is also the last one, on all rows."""
    s = vo.ViTEDShape(img_size=16, patch_size=8, num_classes=1, embed_dim=128, num_heads=2, depth=1, c_depth=c_depth)
    oracle = _random_oracle(s, 80 + c_depth, variant).eval()
    model = _hip_model(vited, s, gpu, dtype, variant, state=oracle.state_dict()).eval()
    n = 6
    imgs = torch.randn(n, 3, 16, 16, generator=torch.Generator().manual_seed(82)).clamp(-1, 1)
    amp = dtype == torch.bfloat16
    sim = vited.engine.pairwise_similarity(model, imgs.to(gpu), block=2, pair_batch=4, amp=amp)
    plain = vited.engine.pairwise_similarity(model, imgs.to(gpu), block=2, pair_batch=4, amp=amp, pair_cache=False)
    torch.testing.assert_close(sim.float(), plain.float(), rtol=1e-2, atol=1e-2)
    i, j = torch.triu_indices(n, n)
    with torch.no_grad():
        ref = oracle(torch.stack([imgs[i], imgs[j]], dim=1)).reshape(-1)
    tol = dict(rtol=2e-3, atol=2e-3) if dtype == torch.float32 else dict(rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(sim[i, j].float().cpu(), ref, **tol)
    torch.testing.assert_close(plain[i, j].float().cpu(), ref, **tol)
    assert float(ref.std()) > 1e-3


def test_puzzle_distances(vited, gpu):
    """6 pieces, fp32, 'avg': puzzle_distances' logits are the restatement's and its integer distances the quantised restatement's,
    off by one at most (tests/test_gpu_qknorm.py's form of the check)."""
    s = vo.ViTEDShape(img_size=16, patch_size=8, num_classes=4, embed_dim=64, num_heads=2, depth=1, c_depth=2)
    n = 6
    pieces = torch.randint(0, 256, (n, 3, 16, 16), dtype=torch.uint8, generator=torch.Generator().manual_seed(92))
    ii, jj = np.nonzero(~np.eye(n, dtype=bool))
    x = (pieces.float() / 255 - 0.5) / 0.5
    stacked = torch.stack([x[ii], x[jj]], dim=1)
    for seed in range(91, 99):       # a seed at which no entry of the reference itself sits on a quantisation boundary (decided on the CPU)
        oracle = _random_oracle(s, seed, 'avg').eval()
        with torch.no_grad():
            ref32 = oracle(stacked).numpy()
            ref64 = oracle.double()(stacked.double()).numpy()
        oracle.float()
        if not near_integer(ref64).any() and (quantise_numpy(ref32) == quantise_numpy(ref64.astype(np.float32))).all():
            break
    else:
        raise AssertionError('no seed in 91..98 keeps the reference off the quantisation boundaries')
    model = _hip_model(vited, s, gpu, torch.float32, 'avg', state=oracle.state_dict()).eval()
    dq, logits = vited.engine.puzzle_distances(model, pieces, pair_batch=7, block=4, amp=False, return_logits=True)
    np.testing.assert_allclose(logits[ii, jj].cpu().numpy(), ref32, rtol=1e-3, atol=1e-5)
    dqn = dq.cpu().numpy()
    for side in range(4):
        want = quantise_numpy(ref32[:, (side + 3) % 4]).astype(np.int64)
        assert np.abs(dqn[side, ii, jj].astype(np.int64) - want).max() <= 1, side


def test_pair_relevancy_is_refused_under_avg(vited, gpu):
    s = plc.GOLDEN_SHAPES[0]
    model = _hip_model(vited, s, gpu, torch.float32, 'avg')
    x = vo.closed_form_pairs(2, s).to(gpu)
    with pytest.raises(NotImplementedError, match='global_pool'):
        vited.engine.pair_relevancy(model, x, amp=False)
    assert model.keep_cam is False and all(p.grad is None for p in model.parameters())
    model.keep_attn = True              # the attention maps themselves stay available: that path already runs all rows
    for blk in model.cross_blocks:
        blk.attn.keep_attn = blk.cross_attn.keep_attn = True
    out = model(x)
    assert tuple(model.cross_blocks[-1].attn.get_attn().shape) == (2, s.num_heads, s.n2, s.n2) and bool(torch.isfinite(out).all())


def _train_steps(vited, gpu, s, state, use_graph, optimizer, variant):
    m = _hip_model(vited, s, gpu, None, variant, state=state).train()
    groups = vited.engine.param_groups_no_decay_1d(m)
    if optimizer == 'adamw':
        opt = vited.optim.FlatAdamW(groups, lr=1e-3, weight_decay=0.05)
    else:
        opt = vited.optim.FlatSGD(groups, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.05)
    return m, vited.engine.TrainStep(m, opt, clip_grad=5.0, amp=True, use_graph=use_graph)


@pytest.mark.parametrize('variant,optimizer', [('avg', 'adamw'), ('avg_nofc', 'sgd')])
def test_train_step_captured_equals_eager(vited, gpu, variant, optimizer):
    """Config-A geometry, 1 + 2 blocks, B 16, bf16: three steps of the captured graphs against the eagerly launched step - the same
    loss at every step and the same parameters at the end, bit for bit - and the head's norm has moved."""
    s = vo.ViTEDShape(depth=1, c_depth=2)
    state = _random_oracle(s, 100, variant).state_dict()
    (me, eager), (mg, graph) = (_train_steps(vited, gpu, s, state, False, optimizer, variant),
                                _train_steps(vited, gpu, s, state, True, optimizer, variant))
    g = torch.Generator().manual_seed(101)
    for it in range(3):
        x = torch.randn(16, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
        y = (torch.rand(16, 4, generator=g) > 0.6).float().to(gpu)
        le, lg = float(eager.step(x, y)), float(graph.step(x, y))
        assert le == lg, (it, le, lg)
    for (n, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(pe, pg), n
    key = 'fc_norm' if mg.use_fc_norm else 'norm'
    for n in (key + '.weight', key + '.bias'):
        assert not torch.equal(dict(mg.named_parameters())[n].detach().cpu(), state[n]), f'{n} never moved'


@pytest.mark.parametrize('dtype', DTYPES)
def test_off_is_off(vited, gpu, dtype):
    """The default model and one built with global_pool='token', fc_norm=False: the same calls reach the library with the same sizes, in
    the same order, none of them a pooling kernel, and logits and gradients agree bit for bit."""
    s = vo.ViTEDShape(depth=2, c_depth=2)
    torch.manual_seed(111)
    state = vo.OracleViTED(s).state_dict()
    x, y = _batch(s, 8, 112)
    x, y = x.to(gpu), y.to(gpu)
    outs = []
    for kw in ({}, dict(global_pool='token', fc_norm=False)):
        m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, num_classes=s.num_classes, embed_dim=s.embed_dim,
                                          depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads, **kw)
        m.compute_dtype = dtype
        m.load_state_dict(state)
        m = m.to(gpu).train()
        with _Recorder(vited) as rec:
            logits = m(x)
            BCE(logits, y).backward()
            with torch.no_grad():            # and the pair caches
                m.eval()
                kvs = m.cache_context_kv(m(x[:, 0].contiguous(), forward_first_part=True))
                tokens2, q0 = m.cache_image2_tokens(x[:, 1].contiguous())
                idx = torch.arange(8, device=gpu)
                cached = m.forward_pairs_cached(tokens2, idx, kvs, idx, q0)
        outs.append((rec.calls, logits.detach(), _grads(m), cached))
    (c0, l0, g0, k0), (c1, l1, g1, k1) = outs
    assert c0 == c1 and len(c0) > 50 and not any('token_pool' in n for n, _ in c0)
    assert torch.equal(l0, l1) and torch.equal(k0, k1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
