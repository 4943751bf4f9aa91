"""q/k-norm on the MI355X: the kernels of csrc/qk_norm.hip against the fp64 formula evaluated on the values they read (bf16 inputs
upcast), the exact identities the arithmetic allows, and a ``qk_norm=True`` model - training, pair-indexed training, the pair
caches, puzzle distances, relevancy maps, captured training steps - against the restatement of tests/qknorm_cases.py.

Operator tolerances come from the number formats.  A normalised element is of order one and the fp32 arithmetic behind it is a
dozen roundings of 2^-24, so fp32 outputs hold rtol 1e-5 / atol 1e-5; a bf16 output adds its own rounding, half an ulp = 2^-9
relative, so bf16 holds rtol 2^-8 on top.  The parameter gradients are fp32 sums over all head rows: the error of such a sum is
bounded by (number of roundings) x 2^-24 x the sum of the |terms|, and each column's bound here is 1e-5 x sum |terms| - a few hundred
roundings' worth, the depth of the reduction (lane partials, LDS combine, finishing pass) rather than the row count.

Model tolerances are those of tests/test_gpu_droppath.py::_check_values.  The gradient of every ``k_norm.bias`` is zero in exact
arithmetic (tests/test_qknorm.py's docstring), so those tensors are held to the same figure times the norm of the module's weight
gradient instead of a relative error against a reference that is itself rounding noise."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import qknorm_cases as qc
from oracle import vited_oracle as vo
from test_gpu_droppath import _check_values, _grads
from test_gpu_puzzle import near_integer, quantise_numpy
from test_gpu_relevancy import SLOW_PATH_R_QI_DISTANCE, _avg_heads, _dist

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
BCE = F.binary_cross_entropy_with_logits
EPS = 1e-6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'qk_norm.npz')


# ---------------------------------------------------------------------------------------------
# operator level
# ---------------------------------------------------------------------------------------------
def _rand(shape, gpu, seed, dtype=torch.float32, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return (offset + scale * torch.randn(shape, generator=g)).to(dtype).to(gpu)


def _params(hd, gpu, seed):
    return (_rand((hd,), gpu, seed, offset=1.0, scale=0.3), _rand((hd,), gpu, seed + 1, scale=0.2))


def _ref(x, gamma, beta, heads, dy=None):
    """fp64 LayerNorm over every head's head_dim elements of x [rows, heads * hd] (the values the kernel read, upcast); with ``dy`` also
    (dx, dgamma, dbeta, per-column sum of |dy * xhat|, of |dy|)."""
    rows, d = x.shape
    xd = x.double().reshape(rows, heads, d // heads).clone().requires_grad_(dy is not None)
    g, b = gamma.double().clone().requires_grad_(dy is not None), beta.double().clone().requires_grad_(dy is not None)
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + EPS).rsqrt()
    xhat = (xd - mean) * rstd
    y = (xhat * g + b).reshape(rows, d)
    if dy is None:
        return y.detach(), mean.detach().reshape(rows, heads), rstd.detach().reshape(rows, heads)
    dyd = dy.double()
    y.backward(dyd)
    t = dyd.reshape(rows, heads, -1)
    return xd.grad.reshape(rows, d), g.grad, b.grad, (t * xhat.detach()).abs().sum((0, 1)), t.abs().sum((0, 1))


def _tol(dtype):
    return dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=2 ** -8, atol=1e-5)


PATTERN = -1536.0        # exactly representable in bf16 and fp32


def _layout(layout, gpu, dtype, rows_q, rows_k, heads, hd, seed):
    """(q view | None, k view | None, the buffers behind them) for one of the layouts the model uses: 'packed3' q / k are column
    slices of [M, 3D]; 'cross' q is a dense [Mq, D], k the first half of [Mk, 2D] with another row count; 'q_only' / 'k_only' one
    operand alone, as the pair caches call it."""
    d = heads * hd
    if layout == 'packed3':
        buf = _rand((rows_q, 3 * d), gpu, seed, dtype)
        return buf[:, 0:d], buf[:, d:2 * d], [buf]
    qb, kb = _rand((rows_q, d), gpu, seed, dtype), _rand((rows_k, 2 * d), gpu, seed + 1, dtype)
    if layout == 'cross':
        return qb, kb[:, 0:d], [qb, kb]
    return (qb, None, [qb]) if layout == 'q_only' else (None, kb[:, 0:d], [kb])


def _run_case(vited, gpu, dtype, batch, n, heads, hd, layout, seed=0):
    ops = vited.ops
    d = heads * hd
    rows_q, rows_k = (batch * n, batch * n) if layout == 'packed3' else (batch * (n + 1), batch * n)
    q, k, bufs = _layout(layout, gpu, dtype, rows_q, rows_k, heads, hd, seed)
    before = [b.clone() for b in bufs]
    (gq, bq), (gk, bk) = _params(hd, gpu, seed + 10), _params(hd, gpu, seed + 20)
    # outputs: column slices of pattern-filled buffers wider than what is written
    out = torch.full((max(rows_q, rows_k), 3 * d + 16), PATTERN, dtype=dtype, device=gpu)
    qo = out[:rows_q, 0:d] if q is not None else None
    ko = out[:rows_k, d:2 * d] if k is not None else None
    got_q, got_k, sq, sk = ops.qk_norm_fwd(q, k, gq if q is not None else None, bq if q is not None else None, gk if k is not None else None,
                                           bk if k is not None else None, heads, EPS, out=(qo, ko))
    for b, b0 in zip(bufs, before):
        assert torch.equal(b, b0), 'the forward wrote into its input'
    written = torch.zeros_like(out, dtype=torch.bool)
    for t, rows, c0 in ((q, rows_q, 0), (k, rows_k, d)):
        if t is not None:
            written[:rows, c0:c0 + d] = True
    assert bool((out[~written] == PATTERN).all()), 'the forward wrote outside its slices'
    assert (got_q is None) == (q is None) and (got_k is None) == (k is None) and (sq is None) == (q is None) and (sk is None) == (k is None)
    for name, x, g, b, got, st in (('q', q, gq, bq, got_q, sq), ('k', k, gk, bk, got_k, sk)):
        if x is None:
            continue
        y, mean, rstd = _ref(x, g, b, heads)
        print(f'{dtype} {layout} {name}: y max|d| = {float((got.double() - y).abs().max()):.3e}')
        torch.testing.assert_close(got.double(), y, **_tol(dtype))
        assert st[0].shape == st[1].shape == (x.shape[0], heads)
        torch.testing.assert_close(st[0].double(), mean, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(st[1].double(), rstd, rtol=1e-5, atol=0)

    # backward: d(out) sits in the q / k columns of pattern-filled gradient buffers and is overwritten in place
    dbuf = torch.full((max(rows_q, rows_k), 3 * d + 8), PATTERN, dtype=dtype, device=gpu)
    dq = dbuf[:rows_q, 0:d] if q is not None else None
    dk = dbuf[:rows_k, d:2 * d] if k is not None else None
    dys = {}
    for name, t, sd in (('q', dq, seed + 30), ('k', dk, seed + 31)):
        if t is not None:
            t.copy_(_rand(tuple(t.shape), gpu, sd, dtype))
            dys[name] = t.clone()
    start = dbuf.clone()

    def backward():
        dbuf.copy_(start)
        return ops.qk_norm_bwd(dq, q, sq, gq if q is not None else None, dk, k, sk, gk if k is not None else None, heads)

    grads = backward()
    assert bool((dbuf[~written[:, :3 * d + 8]] == PATTERN).all()), 'the backward wrote outside its slices'
    for b, b0 in zip(bufs, before):
        assert torch.equal(b, b0)
    kept = (dbuf.clone(), [g.clone() if g is not None else None for g in grads])
    for name, x, g, b, dx, st, (dg, db) in (('q', q, gq, bq, dq, sq, grads[0:2]), ('k', k, gk, bk, dk, sk, grads[2:4])):
        if x is None:
            assert dg is None and db is None
            continue
        dx_ref, dg_ref, db_ref, sum_g, sum_b = _ref(x, g, b, heads, dys[name])
        print(f'{dtype} {layout} d{name}: dx max|d| = {float((dx.double() - dx_ref).abs().max()):.3e}, dgamma max|d| = '
              f'{float((dg.double() - dg_ref).abs().max()):.3e} (bound {float(1e-5 * sum_g.max()):.1e}), dbeta max|d| = '
              f'{float((db.double() - db_ref).abs().max()):.3e}')
        torch.testing.assert_close(dx.double(), dx_ref, **_tol(dtype))
        assert bool(((dg.double() - dg_ref).abs() <= 1e-5 * sum_g).all())
        assert bool(((db.double() - db_ref).abs() <= 1e-5 * sum_b).all())
    # two runs: identical bits
    again = backward()
    assert torch.equal(dbuf, kept[0])
    for a, b in zip(again, kept[1]):
        assert (a is None and b is None) or torch.equal(a, b)
    # accumulation: onto given destinations the sums are ADDED - twice gives base + 2 x
    present = [g for g in grads if g is not None]
    dest = [_rand((hd,), gpu, seed + 40 + i) for i in range(len(present))]
    base = [t.clone() for t in dest]
    names = (['dgq', 'dbq'] if q is not None else []) + (['dgk', 'dbk'] if k is not None else [])
    for _ in range(2):
        dbuf.copy_(start)
        ops.qk_norm_bwd(dq, q, sq, gq if q is not None else None, dk, k, sk, gk if k is not None else None, heads, **dict(zip(names, dest)))
    for t, b0, g in zip(dest, base, present):
        assert torch.equal(t, (b0 + g) + g)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('layout', ['packed3', 'cross', 'q_only', 'k_only'])
@pytest.mark.parametrize('heads,hd', [(2, 32), (3, 32), (2, 64), (3, 64)])
def test_forward_backward_against_fp64(vited, gpu, dtype, layout, heads, hd):
    """B 3, N 5: 15 / 18 token rows, 30 - 54 head rows - no multiple of the 8 head rows of a wave nor of the 32 of a workgroup."""
    _run_case(vited, gpu, dtype, 3, 5, heads, hd, layout, seed=heads * hd)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('layout', ['packed3', 'cross'])
def test_grid_stride_loop_runs_more_than_once(vited, gpu, dtype, layout):
    """B 7, N 65, 6 heads: 2,730 head rows on 43 (forward) / 22 (backward) workgroups of 32 groups."""
    _run_case(vited, gpu, dtype, 7, 65, 6, 32, layout, seed=7)


@pytest.mark.parametrize('hd', [32, 64])
def test_exact_identities(vited, gpu, hd):
    """fp32, bit for bit: a head row of equal values gives exactly beta; gamma = 0 gives exactly beta, and in the backward dx = 0 while
    dgamma still is sum dy * xhat (the backward never divides by gamma)."""
    ops = vited.ops
    heads, rows = 3, 11
    d = heads * hd
    (g, b), (g2, b2) = _params(hd, gpu, 1), _params(hd, gpu, 3)
    level = _rand((rows, heads, 1), gpu, 5, scale=3.0)
    x = level.expand(rows, heads, hd).reshape(rows, d).contiguous()
    k = _rand((rows, d), gpu, 6)
    yq, yk, _, _ = ops.qk_norm_fwd(x, k, g, b, g2, b2, heads, EPS)
    assert torch.equal(yq, b.repeat(rows, heads)), 'equal values: exactly beta'
    zero = torch.zeros_like(g)
    yq, yk0, sq, sk = ops.qk_norm_fwd(k, k, zero, b, g2, b2, heads, EPS)
    assert torch.equal(yq, b.repeat(rows, heads)), 'gamma = 0: exactly beta'
    assert torch.equal(yk0, yk), 'the other operand of the launch is untouched by it'
    dy = _rand((rows, d), gpu, 8)
    dq, dk = dy.clone(), dy.clone()
    dgq, dbq, dgk, dbk = ops.qk_norm_bwd(dq, k, sq, zero, dk, k, sk, g2, heads)
    assert int(torch.count_nonzero(dq)) == 0, 'gamma = 0: dx = 0'
    assert int(torch.count_nonzero(dk)) > 0
    _, dg_ref, db_ref, sum_g, sum_b = _ref(k, g2, b2, heads, dy)
    assert torch.equal(dgq, dgk) and torch.equal(dbq, dbk), 'dgamma / dbeta do not depend on gamma'
    assert bool(((dgq.double() - dg_ref).abs() <= 1e-5 * sum_g).all()) and float(dgq.abs().max()) > 0.1
    assert bool(((dbq.double() - db_ref).abs() <= 1e-5 * sum_b).all())


def test_bad_arguments_raise(vited, gpu):
    ops = vited.ops
    g = torch.ones(32, device=gpu)
    x = torch.zeros(4, 64, device=gpu)
    with pytest.raises(ValueError):
        ops.qk_norm_fwd(None, None, None, None, None, None, 2, EPS)
    with pytest.raises(RuntimeError, match='unsupported'):
        ops.qk_norm_fwd(torch.zeros(4, 32, device=gpu), None, torch.ones(16, device=gpu), torch.ones(16, device=gpu), None, None, 2, EPS)
    with pytest.raises(RuntimeError):
        ops.qk_norm_fwd(torch.zeros(4, 64), None, g.cpu(), g.cpu(), None, None, 2, EPS)          # no CPU fallback
    with pytest.raises(ValueError):
        ops.qk_norm_fwd(x.t(), None, g, g, None, None, 2, EPS)                                   # the last dim must be dense
    with pytest.raises(RuntimeError, match='vited_qk_norm_fwd failed'):
        ops.qk_norm_fwd(torch.zeros(4, 66, device=gpu)[:, 2:], None, g, g, None, None, 2, EPS)   # misaligned for 16-byte vectors


@pytest.mark.parametrize('dtype', DTYPES)
def test_custom_operator_forward_and_autograd(vited, gpu, dtype):
    heads, hd = 3, 32
    q = _rand((2, 5, heads * hd), gpu, 1, dtype).requires_grad_()
    kv = _rand((2, 4, 2 * heads * hd), gpu, 2, dtype).requires_grad_()
    (gq, bq), (gk, bk) = _params(hd, gpu, 3), _params(hd, gpu, 5)
    params = [t.requires_grad_() for t in (gq, bq, gk, bk)]
    qo, ko, *_ = torch.ops.vited.qk_norm(q, kv[:, :, :heads * hd], *params, heads, EPS)
    assert qo.dtype == ko.dtype == dtype and qo.shape == q.shape and ko.shape == (2, 4, heads * hd)
    wq, wk = _rand(tuple(qo.shape), gpu, 7), _rand(tuple(ko.shape), gpu, 8)
    ((qo.float() * wq).sum() + (ko.float() * wk).sum()).backward()
    ref_in = [t.detach().double().requires_grad_() for t in (q, kv, *params)]
    rq, rkv, rgq, rbq, rgk, rbk = ref_in
    ro_q = F.layer_norm(rq.view(2, 5, heads, hd), (hd,), rgq, rbq, EPS).view(2, 5, -1)
    ro_k = F.layer_norm(rkv[:, :, :heads * hd].reshape(2, 4, heads, hd), (hd,), rgk, rbk, EPS).view(2, 4, -1)
    torch.testing.assert_close(qo.double(), ro_q, **_tol(dtype))
    torch.testing.assert_close(ko.double(), ro_k, **_tol(dtype))
    # the upstream gradient reaches the kernel in the activation dtype: in bf16 it is rounded before it is used
    ((ro_q * wq.to(dtype).double()).sum() + (ro_k * wk.to(dtype).double()).sum()).backward()
    tol = dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    for got, want in zip((q, kv, *params), ref_in):
        assert got.grad is not None and got.grad.shape == got.shape
        torch.testing.assert_close(got.grad.double(), want.grad, **tol)
    assert int(torch.count_nonzero(kv.grad[:, :, heads * hd:])) == 0          # the V half never entered


# ---------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------
def _hip_model(vited, s, gpu, dtype, state=None, qk_norm=True, **kw):
    m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                      embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads,
                                      mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, qk_norm=qk_norm, **kw)
    m.compute_dtype = dtype
    if state is not None:
        m.load_state_dict(state)
    return m.to(gpu)


def _random_oracle(s, seed):
    """The oracle's init with the q/k-norm parameters moved off 1 / 0."""
    torch.manual_seed(seed)
    return qc.randomize_norms_(qc.QKNormViTED(s), torch.Generator().manual_seed(seed + 1000))


def _check(dtype, lh, gh, lo, go):
    """test_gpu_droppath._check_values; the k_norm.bias gradients (zero in exact arithmetic) against tolerance x |d k_norm.weight|."""
    zero = [n for n in go if n.endswith('k_norm.bias')]
    tol = 1e-3 if dtype == torch.float32 else 5e-2
    for n in zero:
        scale = float(go[n.replace('.bias', '.weight')].norm())
        got = float(gh[n].norm())
        print(f'{dtype}: {n} |g| = {got:.3e} (exactly 0 in exact arithmetic; reference {float(go[n].norm()):.1e}, bound {tol * scale:.3e})')
        assert got <= tol * scale, n
    _check_values(dtype, lh, {n: g for n, g in gh.items() if n not in zero}, lo, {n: g for n, g in go.items() if n not in zero})


def _one_shot(vited, gpu, dtype, s, batch, seed, prepare=None):
    oracle = _random_oracle(s, seed)
    model = _hip_model(vited, s, gpu, dtype, state=oracle.state_dict()).train()
    if prepare is not None:
        prepare(model)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(batch, 2, 3, s.img_size, s.img_size, generator=g).clamp(-1, 1)
    y = (torch.rand(batch, s.num_classes, generator=g) > 0.6).float()
    lo = oracle(x)
    _, go = qc.loss_and_grads(oracle, lo, y)
    lh = model(x.to(gpu))
    BCE(lh, y.to(gpu)).backward()
    gh = _grads(model)
    assert set(gh) == set(go)
    return model, lh.detach().cpu(), gh, lo.detach(), go


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('which', [0, 1])
def test_small_model_against_the_restatement(vited, gpu, dtype, which):
    """The golden geometries (head_dim 32 / 64, 4 / 5 tokens, 2 + 2 blocks, B 3): portable kernels in fp32, tile kernels in bf16."""
    s = qc.GOLDEN_SHAPES[which]
    _, lh, gh, lo, go = _one_shot(vited, gpu, dtype, s, qc.GOLDEN_BATCH, seed=which)
    _check(dtype, lh, gh, lo, go)


def test_small_model_against_the_reference_fixture(vited, gpu):
    """Golden shape 0 in fp32 on the fixture's closed-form weights and inputs: the logits the reference's own classes gave."""
    fx = np.load(GOLDEN)
    s = qc.GOLDEN_SHAPES[0]
    state = qc.fill_closed_form_(qc.QKNormViTED(s)).state_dict()
    model = _hip_model(vited, s, gpu, torch.float32, state=state)
    x, y = qc.golden_inputs(s)
    lh = model(x.to(gpu))
    loss = BCE(lh, y.to(gpu))
    torch.testing.assert_close(lh.detach().cpu().double(), torch.from_numpy(fx['logits0']), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(float(loss), float(fx['loss0']), rtol=1e-4)


@pytest.mark.parametrize('dtype', DTYPES)
def test_config_a_geometry(vited, gpu, dtype):
    """D 384, 12 heads x 32, 64 / 65 tokens, 2 + 2 blocks, B 8: the short-sequence attention kernels, the row-complete Linear +
    LayerNorm kernels around them, the folded context keys / values (bf16) and the cls-only last block."""
    s = vo.ViTEDShape(depth=2, c_depth=2)
    ops = vited.ops
    calls = []
    real = ops.qk_norm_fwd

    def spy(q, k, *a, **kw):
        calls.append((None if q is None else tuple(q.shape), None if k is None else tuple(k.shape)))
        return real(q, k, *a, **kw)

    ops.qk_norm_fwd = spy
    try:
        model, lh, gh, lo, go = _one_shot(vited, gpu, dtype, s, 8, seed=3)
    finally:
        ops.qk_norm_fwd = real
    assert model.runtime().cls_tail
    assert ((8, 384), (8 * 65, 384)) in calls, calls          # the cls-only last block: query 0 of every sample, every key
    assert ((8 * 64, 384), (8 * 64, 384)) in calls and ((8 * 65, 384), (8 * 65, 384)) in calls
    _check(dtype, lh, gh, lo, go)


@pytest.mark.parametrize('dtype,img,path', [(torch.float32, 16, 1), (torch.bfloat16, 16, 2), (torch.bfloat16, 80, 2)])
def test_each_attention_path(vited, gpu, dtype, img, path):
    """1 + 1 blocks, head_dim 64.  vited_last_attention_path reports 1 (portable fp32) or 2 (bf16 MFMA); the MFMA dispatch has a
    short-sequence form (up to 80 keys; its backward at head_dim 32 only) and the flash form: 16-pixel images give 4 / 5 tokens,
    80-pixel images 100 / 101 tokens, the shortest patch-8 sequence past 80 keys, so forward and backward are the flash kernels."""
    s = vo.ViTEDShape(img_size=img, patch_size=8, num_classes=4, embed_dim=128, num_heads=2, depth=1, c_depth=1)
    ops = vited.ops
    seen = []
    real_f, real_b = ops.attention_fwd, ops.attention_bwd

    def spy_f(*a, **k):
        out = real_f(*a, **k)
        seen.append(ops.last_paths()[1])
        return out

    def spy_b(*a, **k):
        out = real_b(*a, **k)
        seen.append(ops.last_paths()[1])
        return out

    ops.attention_fwd, ops.attention_bwd = spy_f, spy_b
    try:
        _, lh, gh, lo, go = _one_shot(vited, gpu, dtype, s, 3, seed=4 + img)
    finally:
        ops.attention_fwd, ops.attention_bwd = real_f, real_b
    assert len(seen) == 6 and set(seen) == {path}, seen
    _check(dtype, lh, gh, lo, go)


@pytest.mark.parametrize('dtype', DTYPES)
def test_pair_indexed_form_equals_the_gathered_form(vited, gpu, dtype):
    """The two-stage step on hisfrag_prepare_indexed's batch (4 images of 2 writers, 2 + 2 blocks; in bf16 the folded keys / values of
    all blocks): k_norm runs once per IMAGE and its backward on the per-image d(k) after the segmented sum.  Logits and gradients
    against the gathered form model(feats[i], x[j]) on the same model: in fp32 at the 1e-3 relative that tests/test_gpu_pair_index.py
    asks of the two forms, in bf16 (where the two forms round d(k) at different places: per pair, or once per image) at the bf16
    figures of _check_values; two runs give the same bits."""
    s = vo.ViTEDShape(img_size=16, patch_size=8, num_classes=1, embed_dim=128, num_heads=2, depth=2, c_depth=2)
    E = vited.engine
    exact = dtype == torch.float32
    oracle = _random_oracle(s, 11)
    model = _hip_model(vited, s, gpu, dtype, state=oracle.state_dict()).train()
    samples = torch.randn(4, 3, s.img_size, s.img_size, generator=torch.Generator().manual_seed(12)).clamp(-1, 1).to(gpu)
    targets = torch.tensor([0, 0, 1, 1], device=gpu)
    (x, feats, j_idx, seg), labels = E.hisfrag_prepare_indexed(model, samples, targets, amp=not exact,
                                                               generator=torch.Generator(device=gpu).manual_seed(1))
    assert x is samples and isinstance(seg, vited.ops.PairSegments) and j_idx.numel() == labels.shape[0] >= 2
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
    assert torch.equal(l1, l2) and torch.equal(df1, df2) and set(g1) == set(g2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    model.zero_grad(set_to_none=True)
    f = feats.clone().requires_grad_()
    lg = model(f[seg.index], samples[j_idx])
    BCE(lg, labels).backward()
    gg = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert set(gg) == set(g1) and any(qc.is_qk_norm_key(n) for n in g1) and not any(n.startswith('blocks.') for n in g1)
    print(f'indexed vs gathered: logits max|d| = {float((l1 - lg).abs().max()):.3e}')
    torch.testing.assert_close(l1, lg.detach(), **(dict(rtol=1e-3, atol=1e-5) if exact else dict(rtol=3e-2, atol=3e-2)))
    tol = 1e-3 if exact else 5e-2
    for n in gg:
        if n.endswith('k_norm.bias'):            # zero in exact arithmetic: noise against the weight's gradient
            assert float(g1[n].norm()) <= tol * float(gg[n.replace('.bias', '.weight')].norm()), n
            continue
        err = float((g1[n] - gg[n]).norm() / (gg[n].norm() + 1e-12))
        assert err <= tol, (n, err)
    assert float((df1 - f.grad).norm() / f.grad.norm()) <= tol


@pytest.mark.parametrize('dtype', DTYPES)
def test_pair_caches(vited, gpu, dtype):
    """5 images, 1 + 2 blocks (the cached first block, the cls-only last one): pairwise_similarity from the caches - normalised q0,
    normalised cached keys - equals the uncached form at test_gpu_model.py's rtol / atol 1e-2, and both the restatement at that
    file's 2e-3 (fp32) / 3e-2 (bf16; scores are stored as fp16)."""
    s = vo.ViTEDShape(img_size=16, patch_size=8, num_classes=1, embed_dim=128, num_heads=2, depth=1, c_depth=2)
    oracle = _random_oracle(s, 21).eval()
    model = _hip_model(vited, s, gpu, dtype, state=oracle.state_dict()).eval()
    n = 5
    imgs = torch.randn(n, 3, 16, 16, generator=torch.Generator().manual_seed(22)).clamp(-1, 1)
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
    """4 pieces, fp32: puzzle_distances' logits are the restatement's, and its integer distances are the quantised restatement's
    logits - off by one at most where a logit sits on a quantisation boundary.  The seed is one at which the fp32 restatement
    quantises like the fp64 one everywhere (asserted here, on the CPU), so no entry of the reference itself is on a boundary."""
    s = vo.ViTEDShape(img_size=16, patch_size=8, num_classes=4, embed_dim=64, num_heads=2, depth=1, c_depth=2)
    oracle = _random_oracle(s, 31).eval()
    n = 4
    pieces = torch.randint(0, 256, (n, 3, 16, 16), dtype=torch.uint8, generator=torch.Generator().manual_seed(32))
    ii, jj = np.nonzero(~np.eye(n, dtype=bool))
    x = (pieces.float() / 255 - 0.5) / 0.5
    stacked = torch.stack([x[ii], x[jj]], dim=1)
    with torch.no_grad():
        ref32 = oracle(stacked).numpy()
        ref64 = oracle.double()(stacked.double()).numpy()
    oracle.float()
    assert not near_integer(ref64).any() and (quantise_numpy(ref32) == quantise_numpy(ref64.astype(np.float32))).all()
    model = _hip_model(vited, s, gpu, torch.float32, state=oracle.state_dict()).eval()
    dq, logits = vited.engine.puzzle_distances(model, pieces, pair_batch=5, block=3, amp=False, return_logits=True)
    got = logits[ii, jj].cpu().numpy()
    np.testing.assert_allclose(got, ref32, rtol=1e-3, atol=1e-5)
    dqn = dq.cpu().numpy()
    off = 0
    for side in range(4):
        want = quantise_numpy(ref32[:, (side + 3) % 4]).astype(np.int64)
        diff = np.abs(dqn[side, ii, jj].astype(np.int64) - want)
        assert diff.max() <= 1, (side, diff.max())
        off += int((diff != 0).sum())
        assert (np.diagonal(dqn[side]) == 2 ** 31 - 1).all()
    print(f'puzzle distances: {off} of {4 * ii.size} entries differ by one ({off / (4 * ii.size):.1%})')


def test_pair_relevancy(vited, gpu):
    """pair_relevancy(method='relevance') on a qk_norm=True model against the restatement with hooks - its softmax maps are formed
    from the NORMALISED q / k, their gradients taken by autograd, in fp64 - propagated by the same relevancy_from_cams, at the
    distance tests/test_gpu_relevancy.py allows pair_relevancy: twice the slow path's."""
    s = qc.GOLDEN_SHAPES[0]
    engine = vited.engine
    oracle = qc.fill_closed_form_(qc.QKNormViTED(s)).double()
    x = vo.closed_form_pairs(2, s)
    oracle.maps = {}
    logits = oracle(x.double())
    target = logits.argmax(-1)
    logits.backward(torch.zeros_like(logits).scatter_(1, target.unsqueeze(1), 1.0))
    cams = [[_avg_heads(oracle.maps[(kind, i, which)]['attn'].detach(), oracle.maps[(kind, i, which)]['attn'].grad).to(gpu)
             for i in range(depth)] for kind, which, depth in (('blocks', 'attn', s.depth), ('cross_blocks', 'attn', s.c_depth),
                                                                ('cross_blocks', 'cross_attn', s.c_depth))]
    want = engine.relevancy_from_cams(*cams)
    model = _hip_model(vited, s, gpu, torch.float32, state={k: v.float() for k, v in oracle.state_dict().items()})
    rel, out = engine.pair_relevancy(model, x.to(gpu), target=target.to(gpu), amp=False)
    torch.testing.assert_close(out.cpu().double(), logits.detach(), rtol=1e-3, atol=1e-4)
    d = _dist(rel, want[:, 1:])
    print(f'R_qi distance from the restatement: {d:.3e} (allowed {2 * SLOW_PATH_R_QI_DISTANCE:.3e})')
    assert tuple(rel.shape) == (2, s.n2 - 1, s.n1) and d <= 2 * SLOW_PATH_R_QI_DISTANCE
    assert all(p.grad is None for p in model.parameters())


def _train_steps(vited, gpu, s, state, use_graph, optimizer):
    m = _hip_model(vited, s, gpu, None, state=state).train()
    groups = vited.engine.param_groups_no_decay_1d(m)
    if optimizer == 'adamw':
        opt = vited.optim.FlatAdamW(groups, lr=1e-3, weight_decay=0.05)
    else:
        opt = vited.optim.FlatSGD(groups, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.05)
    return m, vited.engine.TrainStep(m, opt, clip_grad=5.0, amp=True, use_graph=use_graph)


@pytest.mark.parametrize('optimizer', ['adamw', 'sgd'])
def test_train_step_captured_equals_eager(vited, gpu, optimizer):
    """Config-A geometry, 2 + 2 blocks, B 16, bf16: four steps of the captured graphs against the eagerly launched step - the same
    loss at every step and the same parameters at the end, bit for bit - and the norm parameters have moved."""
    s = vo.ViTEDShape(depth=2, c_depth=2)
    state = _random_oracle(s, 41).state_dict()
    (me, eager), (mg, graph) = _train_steps(vited, gpu, s, state, False, optimizer), _train_steps(vited, gpu, s, state, True, optimizer)
    g = torch.Generator().manual_seed(42)
    for it in range(4):
        x = torch.randn(16, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
        y = (torch.rand(16, 4, generator=g) > 0.6).float().to(gpu)
        le, lg = float(eager.step(x, y)), float(graph.step(x, y))
        assert le == lg, (it, le, lg)
    assert graph._g1 is not None and graph._g2 is not None
    for (n, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(pe, pg), n
    for n, p in mg.named_parameters():
        if qc.is_qk_norm_key(n) and not n.endswith('k_norm.bias'):
            assert not torch.equal(p.detach().cpu(), state[n]), f'{n} never moved'


@pytest.mark.parametrize('dtype', DTYPES)
def test_off_is_off(vited, gpu, dtype):
    """A qk_norm=False model never reaches the kernel, and its logits and gradients are those of a second such model, bit for bit."""
    s = vo.ViTEDShape(depth=2, c_depth=2)
    torch.manual_seed(51)
    state = vo.OracleViTED(s).state_dict()
    ops = vited.ops
    calls = []
    real_f, real_b = ops.qk_norm_fwd, ops.qk_norm_bwd
    ops.qk_norm_fwd = lambda *a, **k: calls.append('fwd') or real_f(*a, **k)
    ops.qk_norm_bwd = lambda *a, **k: calls.append('bwd') or real_b(*a, **k)
    try:
        a, b = (_hip_model(vited, s, gpu, dtype, state=state, qk_norm=q).train() for q in (False, False))
        assert not a.runtime().qk_norm
        g = torch.Generator().manual_seed(52)
        x = torch.randn(8, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
        y = (torch.rand(8, 4, generator=g) > 0.6).float().to(gpu)
        outs = []
        for m in (a, b):
            logits = m(x)
            BCE(logits, y).backward()
            outs.append((logits.detach(), _grads(m)))
        with torch.no_grad():            # the pair caches of the off model
            a.eval()
            kvs = a.cache_context_kv(a(x[:, 0].contiguous(), forward_first_part=True))
            tokens2, q0 = a.cache_image2_tokens(x[:, 1].contiguous())
            idx = torch.arange(8, device=gpu)
            cached = a.forward_pairs_cached(tokens2, idx, kvs, idx, q0)
        assert calls == [] and cached.shape == (8, 4) and bool(torch.isfinite(cached).all())
        on = _hip_model(vited, s, gpu, dtype, qk_norm=True).train()
        BCE(on(x), y).backward()
        assert calls.count('fwd') >= 2 * 2 + 2 * 2 and calls.count('bwd') == 2 + 2 * 2, calls
    finally:
        ops.qk_norm_fwd, ops.qk_norm_bwd = real_f, real_b
    assert torch.equal(outs[0][0], outs[1][0])
    for n in outs[0][1]:
        assert torch.equal(outs[0][1][n], outs[1][1][n]), n
