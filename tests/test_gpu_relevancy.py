"""Attention relevancy maps on the GPU: ops.attention_cam (csrc/attention_cam.hip), model.keep_cam and engine.pair_relevancy.

The kernel's reference is fp64 PyTorch on the SAME stored-dtype operands: P_h = softmax(scale q_h k_h^T), dP_h = dO_h v_h^T,
cam = mean_h max(P_h o dP_h, 0) (avg_heads of scripts/visualise_attentions.py) or sum_h w_h P_h.  Nothing in either kernel is
rounded to bf16 after the loads, so ONE tolerance serves fp32 and bf16 operands: the fp32 backward tolerance of
test_gpu_ops.test_attention_fwd_bwd, rtol 2e-4 with atol 2e-5 x max|expected| (the maps of a thousand-key attention are of order
1e-3 and below, hence the scaled atol).  Model-level checks read tests/golden/relevancy.npz (tools/make_relevancy_golden.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import vited_oracle as vo

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'relevancy.npz')
DTYPES = [torch.float32, torch.bfloat16]
# the issue's shapes, then two of this file's own: a batch large enough that a workgroup of the MFMA kernel takes TWO 64-key tiles
# (one head, and two heads: the step that moves to the next tile after the last head)
SHAPES = [(2, 12, 65, 65, 32), (2, 12, 65, 64, 32), (2, 1, 5, 4, 32), (1, 2, 1, 1, 64), (2, 3, 200, 130, 32), (1, 6, 257, 256, 64),
          (1, 6, 1025, 1024, 64), (3, 5, 64, 65, 32), (64, 1, 5, 1100, 32), (64, 2, 5, 1100, 64)]


def _rand(shape, dev, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev).to(dtype)


def _operands(gpu, dtype, B, H, Nq, Nk, hd, seed=0):
    """As test_attention_fwd_bwd: packed qkv for self-attention, q + packed kv for cross-attention; dO dense."""
    D = H * hd
    if Nq == Nk:
        qkv = _rand((B, Nq, 3 * D), gpu, seed + 1, dtype=dtype)
        q, k, v = qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:]
    else:
        q = _rand((B, Nq, D), gpu, seed + 1, dtype=dtype)
        kv = _rand((B, Nk, 2 * D), gpu, seed + 2, dtype=dtype)
        k, v = kv[:, :, :D], kv[:, :, D:]
    return q, k, v, _rand((B, Nq, D), gpu, seed + 3, dtype=dtype)


def _heads64(t, H):
    b, n, d = t.shape
    return t.double().reshape(b, n, H, d // H).transpose(1, 2)


def _maps(q, k, v, do, H, scale):
    """fp64 P [B, H, Nq, Nk] and dP (None without v / do)."""
    p = torch.softmax((_heads64(q, H) @ _heads64(k, H).transpose(-1, -2)) * scale, dim=-1)
    dp = _heads64(do, H) @ _heads64(v, H).transpose(-1, -2) if v is not None else None
    return p, dp


def _cam_ref(q, k, v, do, H, scale):
    p, dp = _maps(q, k, v, do, H, scale)
    return (p * dp).clamp(min=0).mean(dim=1)


def _close(got, want, what=''):
    want = want.double()
    atol = 2e-5 * float(want.abs().max())
    err = float((got.double() - want).abs().max())
    print(f'{what} max|err| {err:.3e}  max|expected| {float(want.abs().max()):.3e}  atol {atol:.3e}')
    torch.testing.assert_close(got.double(), want, rtol=2e-4, atol=atol)


# ---------------------------------------------------------------------------------------------
# 1. the op against fp64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,H,Nq,Nk,hd', SHAPES)
def test_cam_grad_against_fp64(vited, gpu, dtype, B, H, Nq, Nk, hd):
    ops, scale = vited.ops, hd ** -0.5
    q, k, v, do = _operands(gpu, dtype, B, H, Nq, Nk, hd)
    _, lse = ops.attention_fwd(q, k, v, H, scale)
    cam = ops.attention_cam(q, k, v, do, lse, H, scale, mode='grad')
    assert ops.last_paths()[1] == (2 if dtype == torch.bfloat16 else 1)
    assert cam.dtype == torch.float32 and tuple(cam.shape) == (B, Nq, Nk)
    _close(cam, _cam_ref(q, k, v, do, H, scale), f'grad {dtype} {(B, H, Nq, Nk, hd)}')


# ---------------------------------------------------------------------------------------------
# 2. PROB mode
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,H,Nq,Nk,hd', [(2, 12, 65, 64, 32), (1, 6, 257, 256, 64)])
def test_cam_prob(vited, gpu, dtype, B, H, Nq, Nk, hd):
    ops, scale = vited.ops, hd ** -0.5
    q, k, v, _ = _operands(gpu, dtype, B, H, Nq, Nk, hd, seed=10)
    _, lse = ops.attention_fwd(q, k, v, H, scale)
    p, _ = _maps(q, k, None, None, H, scale)
    mean = ops.attention_cam(q, k, None, None, lse, H, scale, mode='prob')
    assert ops.last_paths()[1] == (2 if dtype == torch.bfloat16 else 1)
    _close(mean, p.mean(dim=1), 'prob, null weights')
    assert float((mean.double().sum(-1) - 1).abs().max()) < 1e-5            # the head mean of a softmax: every row sums to 1
    w = _rand((B, H), gpu, 11)                                              # signed
    weighted = ops.attention_cam(q, k, v, None, lse, H, scale, mode='prob', head_weight=w)   # v is ignored in this mode
    _close(weighted, (p * w.double()[:, :, None, None]).sum(dim=1), 'prob, signed weights')


# ---------------------------------------------------------------------------------------------
# 3. structured values with closed-form answers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_zero_output_gradient_gives_an_exactly_zero_map(vited, gpu, dtype):
    ops, (B, H, Nq, Nk, hd) = vited.ops, (2, 3, 200, 130, 32)
    q, k, v, do = _operands(gpu, dtype, B, H, Nq, Nk, hd, seed=20)
    _, lse = ops.attention_fwd(q, k, v, H, hd ** -0.5)
    cam = ops.attention_cam(q, k, v, torch.zeros_like(do), lse, H, hd ** -0.5, mode='grad')
    assert torch.count_nonzero(cam) == 0


@pytest.mark.parametrize('dtype', DTYPES)
def test_zero_queries_give_uniform_attention(vited, gpu, dtype):
    """q = 0: P = 1 / Nk for every head, so cam = mean_h max(dP_h, 0) / Nk."""
    ops, (B, H, Nq, Nk, hd) = vited.ops, (2, 3, 70, 130, 64)
    q, k, v, do = _operands(gpu, dtype, B, H, Nq, Nk, hd, seed=30)
    q = torch.zeros_like(q)
    _, lse = ops.attention_fwd(q, k, v, H, hd ** -0.5)
    cam = ops.attention_cam(q, k, v, do, lse, H, hd ** -0.5, mode='grad')
    dp = _heads64(do, H) @ _heads64(v, H).transpose(-1, -2)
    _close(cam, dp.clamp(min=0).mean(dim=1) / Nk, 'q = 0')


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_head_with_negative_gradient_everywhere_drops_out(vited, gpu, dtype):
    """Head 1: v >= 0 and dO <= 0, so dP_1 < 0 for every (query, key) and max(P_1 dP_1, 0) = 0: the map is the other heads' sum / H."""
    ops, (B, H, Nq, Nk, hd) = vited.ops, (2, 3, 70, 130, 32)
    q, k, v, do = _operands(gpu, dtype, B, H, Nq, Nk, hd, seed=40)
    v, do = v.clone(), do.clone()
    v[:, :, hd:2 * hd] = v[:, :, hd:2 * hd].abs() + 0.125
    do[:, :, hd:2 * hd] = -do[:, :, hd:2 * hd].abs() - 0.125
    _, lse = ops.attention_fwd(q, k, v, H, hd ** -0.5)
    cam = ops.attention_cam(q, k, v, do, lse, H, hd ** -0.5, mode='grad')
    p, dp = _maps(q, k, v, do, H, hd ** -0.5)
    assert float(dp[:, 1].max()) < 0
    others = (p[:, [0, 2]] * dp[:, [0, 2]]).clamp(min=0).sum(dim=1) / H
    _close(cam, others, 'one head negative')


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_dominant_key_owns_the_map(vited, gpu, dtype):
    """Every query scores key 37 sixty above the other keys (q = 2.5, k_37 = 3, the other keys 0: sqrt(64) x 2.5 x 3 = 60, exact in
    bf16), so P is 1 in that column and e^-60 elsewhere: the map is max(dP, 0) of that column and zero within tolerance elsewhere."""
    ops, (B, H, Nq, Nk, hd) = vited.ops, (2, 3, 70, 130, 64)
    _, _, v, do = _operands(gpu, dtype, B, H, Nq, Nk, hd, seed=50)
    q = torch.full((B, Nq, H * hd), 2.5, dtype=dtype, device=gpu)
    k = torch.zeros((B, Nk, H * hd), dtype=dtype, device=gpu)
    k[:, 37] = 3.0
    _, lse = ops.attention_fwd(q, k, v, H, hd ** -0.5)
    cam = ops.attention_cam(q, k, v, do, lse, H, hd ** -0.5, mode='grad')
    want = _cam_ref(q, k, v, do, H, hd ** -0.5)
    _close(cam, want, 'dominant key')
    column = torch.zeros_like(want)
    column[:, :, 37] = (_heads64(do, H) @ _heads64(v, H).transpose(-1, -2))[:, :, :, 37].clamp(min=0).mean(dim=1)
    _close(cam, column, 'dominant key, closed form')
    assert torch.count_nonzero(cam[:, :, 37]) > 0
    rest = torch.cat([cam[:, :, :37], cam[:, :, 38:]], dim=2)
    assert float(rest.abs().max()) <= 2e-5 * float(want.abs().max())


# ---------------------------------------------------------------------------------------------
# 4. output contract
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,H,Nq,Nk,hd', [(2, 3, 200, 130, 32), (64, 2, 5, 1100, 64)])
def test_padded_output_is_written_inside_only_and_reproducibly(vited, gpu, dtype, B, H, Nq, Nk, hd):
    ops, scale = vited.ops, hd ** -0.5
    q, k, v, do = _operands(gpu, dtype, B, H, Nq, Nk, hd, seed=60)
    _, lse = ops.attention_fwd(q, k, v, H, scale)
    sentinel = -7.25
    buf = torch.full((B, Nq + 1, Nk + 3), sentinel, dtype=torch.float32, device=gpu)      # cam_ld = nk + 3, a guard row per item
    cam = ops.attention_cam(q, k, v, do, lse, H, scale, mode='grad', out=buf[:, :Nq, :])
    assert cam.data_ptr() == buf.data_ptr() and tuple(cam.shape) == (B, Nq, Nk) and cam.stride() == ((Nq + 1) * (Nk + 3), Nk + 3, 1)
    assert bool((buf[:, :Nq, Nk:] == sentinel).all()) and bool((buf[:, Nq, :] == sentinel).all())
    assert bool((cam >= 0).all())                                                         # every inside element was written
    again = ops.attention_cam(q, k, v, do, lse, H, scale, mode='grad')
    assert torch.equal(again, cam)
    _close(cam, _cam_ref(q, k, v, do, H, scale), 'padded output')


def test_misaligned_bf16_view_takes_the_portable_kernel(vited, gpu):
    ops, (B, H, Nq, Nk, hd) = vited.ops, (2, 3, 70, 130, 32)
    D, scale = H * hd, hd ** -0.5
    flat = _rand((B * Nq * D + 8,), gpu, 70, dtype=torch.bfloat16)
    q = flat[1:1 + B * Nq * D].view(B, Nq, D)                                             # 2 bytes off a 16-byte boundary
    _, k, v, do = _operands(gpu, torch.bfloat16, B, H, Nq, Nk, hd, seed=71)
    _, lse = ops.attention_fwd(q, k, v, H, scale)
    cam = ops.attention_cam(q, k, v, do, lse, H, scale, mode='grad')
    assert ops.last_paths()[1] == 1
    _close(cam, _cam_ref(q, k, v, do, H, scale), 'misaligned view')
    aligned = ops.attention_cam(q.clone(), k, v, do, lse, H, scale, mode='grad')
    assert ops.last_paths()[1] == 2
    _close(aligned, cam, 'MFMA against portable')


def test_argument_errors(vited, gpu):
    ops, (B, H, Nq, Nk, hd) = vited.ops, (1, 2, 5, 4, 32)
    q, k, v, do = _operands(gpu, torch.float32, B, H, Nq, Nk, hd, seed=80)
    _, lse = ops.attention_fwd(q, k, v, H, hd ** -0.5)
    call = lambda *a, **kw: ops.attention_cam(*a, H, hd ** -0.5, **kw)
    with pytest.raises(ValueError, match='mode'):
        call(q, k, v, do, lse, mode='both')
    with pytest.raises(ValueError, match='needs v and do'):
        call(q, k, None, do, lse, mode='grad')
    with pytest.raises(ValueError, match='head_weight'):
        call(q, k, v, do, lse, mode='grad', head_weight=torch.ones(B, H, device=gpu))
    with pytest.raises(ValueError, match='lse'):
        call(q, k, v, do, lse[:, :, :4], mode='grad')
    with pytest.raises(ValueError, match='out must be'):
        call(q, k, v, do, lse, mode='grad', out=torch.empty(B, Nq, Nk - 1, device=gpu))
    with pytest.raises(ValueError, match='does not match q'):
        call(q, k.bfloat16(), v, do, lse, mode='grad')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        call(q.cpu(), k, v, do, lse, mode='grad')


# ---------------------------------------------------------------------------------------------
# 5. - 7. the model switch and engine.pair_relevancy
# ---------------------------------------------------------------------------------------------
def _hip_model(vited, s, gpu, dtype, **kw):
    m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                      embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads, **kw)
    m.compute_dtype = dtype
    return m.to(gpu)


def _holders(model):
    return ([blk.attn for blk in model.blocks], [blk.attn for blk in model.cross_blocks], [blk.cross_attn for blk in model.cross_blocks])


def _avg_heads(attn, grad):
    """avg_heads of the script for every sample of a batch: [B, h, Nq, Nk] x 2 -> [B, Nq, Nk]."""
    return (attn * grad).clamp(min=0).mean(dim=1)


def test_fused_cam_equals_the_materialised_maps(vited, gpu):
    s = vo.ViTEDShape(depth=1, c_depth=1)
    torch.manual_seed(6)
    model = _hip_model(vited, s, gpu, torch.bfloat16, keep_attn=True)
    with pytest.raises(RuntimeError, match='no attention map recorded'):
        model.blocks[0].attn.get_attn_cam()
    model.keep_cam = True
    x = torch.randn(3, 2, 3, 64, 64).clamp(-1, 1).to(gpu)
    y = (torch.rand(3, 4) > 0.5).float().to(gpu)
    torch.nn.functional.binary_cross_entropy_with_logits(model(x), y).backward()
    assert all(p.grad is None for p in model.parameters())          # a keep_cam backward hands no parameter gradient on
    for group in _holders(model):
        for holder in group:
            cam = holder.get_attn_cam()
            attn, grad = holder.get_attn(), holder.get_attn_gradients()
            assert tuple(cam.shape) == (3,) + tuple(attn.shape[2:]) and cam.dtype == torch.float32
            _close(cam, _avg_heads(attn.double(), grad.double()), f'model cam {holder._key}')


def _one_hot_backward(model, x, target):
    logits = model(x)
    logits.backward(torch.zeros_like(logits).scatter_(1, target.unsqueeze(1), 1.0))
    return logits.detach()


def _dist(a, b):
    """max |a - b| over max |b|."""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


# Distance (_dist) of the SLOW path's R_qi from the fixture's, measured once on an MI355X: keep_attn maps -> avg_heads ->
# relevancy_from_cams in fp64, fp32 kernels, closed-form 2 + 2 block model: 3.741e-06 (pair_relevancy in the same run: 3.938e-06).
# pair_relevancy may be twice as far.
SLOW_PATH_R_QI_DISTANCE = 3.741e-06


def test_model_against_the_reference_fixture(vited, gpu):
    fx = np.load(GOLDEN)
    img, p, c, ncls, d, depth, cdepth, heads = [int(v) for v in fx['shape']]
    s = vo.ViTEDShape(img_size=img, patch_size=p, in_chans=c, num_classes=ncls, embed_dim=d, depth=depth, c_depth=cdepth, num_heads=heads)
    engine = vited.engine
    model = vo.fill_closed_form_(_hip_model(vited, s, gpu, torch.float32))
    x = vo.closed_form_pairs(2, s).to(gpu)
    target = torch.from_numpy(fx['target']).to(gpu)
    # the six head-averaged maps
    model.keep_cam = True
    logits = _one_hot_backward(model, x, target)
    np.testing.assert_allclose(logits.cpu().numpy(), fx['logits'], rtol=1e-3, atol=1e-4)
    assert torch.equal(logits.argmax(-1), target)
    for holders, name in zip(_holders(model), ('enc', 'dec_self', 'dec_cross')):
        for i, holder in enumerate(holders):
            want = fx[f'{name}_cams'][i]
            got = holder.get_attn_cam().cpu().numpy()
            print(f'{name}[{i}] max|err| {np.abs(got - want).max():.3e} of {np.abs(want).max():.3e}')
            np.testing.assert_allclose(got, want, rtol=2e-3, atol=1e-6 * float(np.abs(want).max()) + 1e-9)
    model.keep_cam = False
    model._attn_store.clear()
    # the slow path on the same fixture: materialised maps -> avg_heads -> the same propagation
    slow = vo.fill_closed_form_(_hip_model(vited, s, gpu, torch.float32, keep_attn=True))
    _one_hot_backward(slow, x, target)
    cams = [[_avg_heads(h.get_attn(), h.get_attn_gradients()).double() for h in group] for group in _holders(slow)]
    want = torch.from_numpy(fx['r_qi']).to(gpu)
    r_slow = engine.relevancy_from_cams(*cams)
    rel, out = engine.pair_relevancy(model, x, amp=False)
    assert tuple(rel.shape) == (2, s.n2 - 1, s.n1) and rel.dtype == torch.float32 and torch.equal(out, logits)
    d_slow, d_fused = _dist(r_slow[:, 1:], want[:, 1:]), _dist(rel, want[:, 1:])
    print(f'R_qi distance from the fixture: slow path {d_slow:.3e}, pair_relevancy {d_fused:.3e}')
    assert d_fused <= 2 * SLOW_PATH_R_QI_DISTANCE
    with_cls, _ = engine.pair_relevancy(model, x, amp=False, include_cls=True, target=2)
    assert tuple(with_cls.shape) == (2, s.n2, s.n1) and torch.equal(with_cls[:, 1:], rel)
    # 'raw' and 'gradcam' against the same quantities from the materialised maps of the last cross-attention
    last = slow.cross_blocks[-1].cross_attn
    attn, grad = last.get_attn().double(), last.get_attn_gradients().double()
    raw, _ = engine.pair_relevancy(model, x, amp=False, method='raw')
    gradcam, _ = engine.pair_relevancy(model, x, amp=False, method='gradcam')
    assert tuple(raw.shape) == tuple(gradcam.shape) == (2, s.n1)
    _close(raw, attn.mean(dim=1)[:, 0, :], 'raw')
    _close(gradcam, (attn * grad.mean(dim=(2, 3), keepdim=True)).mean(dim=1).clamp(min=0)[:, 0, :], 'gradcam')


def test_pair_relevancy_leaves_training_state_alone(vited, gpu):
    """Two twins train side by side (two micro-batches per update, bf16): one of them explains a batch between the micro-batches.
    Its flat gradient buffer and every p.grad must keep their bits, its switches and store must be as before, and its losses must
    stay those of the undisturbed twin - through the update that consumes the accumulated gradients and one step further.
    (Two decoder blocks: with one, only the cls query's row of the decoder self map is non-zero, every other row of R_qq is still
    the identity at rule 10, handle_residual gives 0 / 0 and the whole R_qi is 0 - the reference's result for such a model too.)"""
    s = vo.ViTEDShape(depth=1, c_depth=2)
    torch.manual_seed(3)
    engine = vited.engine
    models = [_hip_model(vited, s, gpu, None) for _ in range(2)]
    models[1].load_state_dict(models[0].state_dict())
    steps = [engine.TrainStep(m, vited.optim.FlatAdamW(engine.param_groups_no_decay_1d(m), lr=1e-3, weight_decay=0.05), amp=True,
                              accumulation_steps=2) for m in models]
    g = torch.Generator().manual_seed(9)
    batches = [(torch.randn(8, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu), (torch.rand(8, 4, generator=g) > 0.6).float().to(gpu))
               for _ in range(4)]
    for step in steps:
        step.step(*batches[0])
    model, flat = models[0], steps[0].flat.flat
    assert float(flat.abs().max()) > 0                              # gradients of the first micro-batch wait in the flat buffer
    before_flat = flat.clone()
    before_grads = [p.grad.clone() for p in model.parameters()]
    pairs = torch.randn(3, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
    rel, logits = engine.pair_relevancy(model, pairs, amp=True)
    assert tuple(rel.shape) == (3, s.n2 - 1, s.n1) and tuple(logits.shape) == (3, 4) and bool(torch.isfinite(rel).all())
    assert float(rel.abs().max()) > 0
    assert torch.equal(flat, before_flat)
    assert all(torch.equal(p.grad, b) for p, b in zip(model.parameters(), before_grads))
    assert model.keep_cam is False and model.keep_attn is False and model._attn_store == {}
    with pytest.raises(RuntimeError, match='no attention map recorded'):
        model.blocks[0].attn.get_attn_cam()
    # chunked == unchunked, bit for bit
    one_by_one, logits1 = engine.pair_relevancy(model, pairs, amp=True, chunk=1)
    assert torch.equal(one_by_one, rel) and torch.equal(logits1, logits)
    assert torch.equal(flat, before_flat)
    # the switches a caller had set come back too
    model.keep_attn = True
    engine.pair_relevancy(model, pairs[:1], amp=True, method='raw')
    assert model.keep_attn is True and model.keep_cam is False and model._attn_store == {}
    model.keep_attn = False
    for batch in batches[1:]:
        losses = [step.step(*batch) for step in steps]
        assert torch.equal(losses[0], losses[1])
