"""The pair-indexed decoder on the MI355X: vited_attention_bwd_indexed (per-pair dK / dV terms + segmented sum) against the fp64 SDPA
on gathered keys / values, and model(feats, x2, x2_index=j, x1_index=i) under autograd against the CPU oracle's
oracle(feats[i], imgs[j]).

Op tolerances are those of test_attention_fwd_bwd (tests/test_gpu_ops.py); an item's dK / dV is a sum of per-pair terms, each within
the per-pair tolerance, so its absolute bound is that tolerance times the largest number of pairs on one item.  Model tolerances
are those of tests/test_gpu_droppath.py::_check_values."""
import pytest
import torch

import droppath_cases as dc
from oracle import vited_oracle as vo
from test_gpu_droppath import _check_values, _grads, _hip_model
from test_gpu_ops import _rand, _sdpa_ref

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
BCE = torch.nn.functional.binary_cross_entropy_with_logits

OP_CASES = [
    (3, 12, 65, 64, 32, [2, 0, 2, 2, 0]),      # short-sequence kernel, an item nobody reads (exact zeros), three summands
    (3, 12, 1, 64, 32, [2, 0, 2, 2, 0]),       # the cls-only last block
    (2, 6, 257, 256, 64, [1, 1, 0, 1]),        # flash kernels, ragged last tile
    (4, 2, 65, 65, 64, [3, 1, 0, 2]),          # one pair per item
]


def _indexed_bwd(ops, q, kv, o, do, lse, H, scale, seg):
    D = q.shape[2]
    dq = torch.empty_like(q)
    dkv = torch.full_like(kv, float('nan'))
    ops.attention_bwd(q, kv[:, :, :D], kv[:, :, D:], o, do, lse, H, scale, dq, dkv[:, :, :D], dkv[:, :, D:], segments=seg)
    return dq, dkv


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('items,H,Nq,Nk,hd,index', OP_CASES)
def test_attention_bwd_indexed(vited, gpu, dtype, items, H, Nq, Nk, hd, index):
    ops = vited.ops
    D, P, scale = H * hd, len(index), hd ** -0.5
    path = 1 if dtype == torch.float32 else 2                     # fp32: portable kernels; bf16: short-sequence MFMA or flash
    idx = torch.tensor(index, device=gpu)
    seg = ops.pair_segments(idx, items)
    q = _rand((P, Nq, D), gpu, 1, dtype=dtype)
    kv = _rand((items, Nk, 2 * D), gpu, 2, dtype=dtype)            # packed kv projection, k / v consumed in place
    do = _rand((P, Nq, D), gpu, 3, dtype=dtype)
    o, lse = ops.attention_fwd(q, kv[:, :, :D], kv[:, :, D:], H, scale, kv_index=idx)
    dq, dkv = _indexed_bwd(ops, q, kv, o, do, lse, H, scale, seg)
    assert ops.last_paths()[1] == path
    dk, dv = dkv[:, :, :D], dkv[:, :, D:]
    assert bool(torch.isfinite(dkv.float()).all())                 # every element of the NaN-filled outputs was written

    # the gathered form: the same kernels on materialised kv[index]
    kvg = kv[idx].contiguous()
    og, lseg = ops.attention_fwd(q, kvg[:, :, :D], kvg[:, :, D:], H, scale)
    assert torch.equal(og, o) and torch.equal(lseg, lse)
    dqg, dkvg = torch.empty_like(q), torch.empty_like(kvg)
    ops.attention_bwd(q, kvg[:, :, :D], kvg[:, :, D:], o, do, lse, H, scale, dqg, dkvg[:, :, :D], dkvg[:, :, D:])
    assert ops.last_paths()[1] == path
    assert torch.equal(dq, dqg)                                    # dq is per pair: bit for bit

    # fp64 SDPA on gathered K / V, its gradients summed per item
    qr, kr, vr = (t.double().clone().requires_grad_() for t in (q, kvg[:, :, :D], kvg[:, :, D:]))
    o_ref, _ = _sdpa_ref(qr, kr, vr, H, scale)
    o_ref.backward(do.double())
    dk_ref = torch.zeros((items, Nk, D), dtype=torch.float64, device=gpu).index_add_(0, idx, kr.grad)
    dv_ref = torch.zeros((items, Nk, D), dtype=torch.float64, device=gpu).index_add_(0, idx, vr.grad)
    counts = torch.bincount(idx, minlength=items)
    most = int(counts.max())
    rtol, atol = (2e-4, 2e-5) if dtype == torch.float32 else (2e-2, 2e-2)
    for name, got, ref, a in (('dq', dq, qr.grad, atol), ('dk', dk, dk_ref, atol * most), ('dv', dv, dv_ref, atol * most)):
        print(f'{dtype} {name}: max|d| = {float((got.double() - ref).abs().max()):.3e} (atol {a:.1e})')
    torch.testing.assert_close(dq.double(), qr.grad, rtol=rtol, atol=atol)
    torch.testing.assert_close(dk.double(), dk_ref, rtol=rtol, atol=atol * most)
    torch.testing.assert_close(dv.double(), dv_ref, rtol=rtol, atol=atol * most)
    for g in (counts == 0).nonzero().view(-1).tolist():
        assert not bool(dkv[g].any()), f'item {g} has no pair: its dk / dv must be exact zeros'
    if most == 1 and int(counts.min()) == 1:                       # a permutation: one term per item passes through unchanged
        assert torch.equal(dkv[idx], dkvg)
    # no atomics: a second call gives the same bits
    dq2, dkv2 = _indexed_bwd(ops, q, kv, o, do, lse, H, scale, seg)
    assert torch.equal(dq2, dq) and torch.equal(dkv2, dkv)


def test_attention_bwd_indexed_checks_its_tables(vited, gpu):
    ops = vited.ops
    H, hd, D = 2, 32, 64
    q, kv = _rand((3, 5, D), gpu, 1), _rand((2, 4, 2 * D), gpu, 2)
    idx = torch.tensor([1, 0, 1], device=gpu)
    o, lse = ops.attention_fwd(q, kv[:, :, :D], kv[:, :, D:], H, 0.2, kv_index=idx)
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    args = (q, kv[:, :, :D], kv[:, :, D:], o, torch.ones_like(o), lse, H, 0.2, dq, dkv[:, :, :D], dkv[:, :, D:])
    with pytest.raises(ValueError, match='outside'):
        ops.attention_bwd(*args, kv_index=torch.tensor([1, 2, 1], device=gpu))          # an index past the items never reaches a kernel
    with pytest.raises(ValueError, match='offsets'):
        ops.attention_bwd(*args, segments=ops.pair_segments(idx, 3))                    # tables of another item count
    with pytest.raises(ValueError, match='segments'):
        ops.attention_bwd(*args, segments=ops.pair_segments(idx.cpu(), 2))              # host tables
    ops.attention_bwd(*args, kv_index=idx)                                              # builds its tables itself
    ref = dkv.clone()
    ops.attention_bwd(*args, segments=ops.pair_segments(idx, 2))
    assert torch.equal(dkv, ref)


# ---------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------
def _oracle_two_stage(oracle, imgs, i, j, y, enc=None, dec=None):
    """oracle encoder on the images, oracle(feats[i], imgs[j]), BCE, all gradients (+ d feats)."""
    oracle.zero_grad(set_to_none=True)
    feats = oracle(imgs, forward_first_part=True) if enc is None else dc.encoder_scaled(oracle, imgs, enc)
    feats.retain_grad()
    lo = oracle(feats[i], imgs[j]) if dec is None else dc.decoder_scaled(oracle, feats[i], imgs[j], dec)
    _, go = dc.loss_and_grads(oracle, lo, y)
    return lo.detach(), go, feats.grad.detach().clone()


def _indexed_two_stage(vited, model, imgs, i, j, y, enc=None, dec=None, detach=False):
    model.zero_grad(set_to_none=True)
    kw1 = {} if enc is None else dict(drop_path=vited.DropPathScales(enc, None))
    kw2 = {} if dec is None else dict(drop_path=vited.DropPathScales(None, dec))
    feats = model(imgs, forward_first_part=True, **kw1)
    if detach:
        feats = feats.detach()
    else:
        feats.retain_grad()
    lh = model(feats, imgs, x2_index=j, x1_index=i, **kw2)
    BCE(lh, y).backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return lh.detach(), grads, None if detach else feats.grad.detach().clone()


def _gathered_two_stage(model, imgs, i, j, y):
    model.zero_grad(set_to_none=True)
    feats = model(imgs, forward_first_part=True)
    lh = model(feats[i], imgs[j])
    BCE(lh, y).backward()
    return lh.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _print_gap_to_gathered(model, imgs, i, j, y, lh, gh):
    lg, gg = _gathered_two_stage(model, imgs, i, j, y)
    worst = max(float((gh[n] - gg[n]).norm() / (gg[n].norm() + 1e-12)) for n in gg)
    print(f'indexed vs gathered HIP form: logits max|d| = {float((lh - lg).abs().max()):.3e}, worst gradient tensor rel err {worst:.3e}')


def _setup(vited, gpu, dtype, s, n_img, pairs, seed):
    torch.manual_seed(seed)
    oracle = vo.OracleViTED(s)
    model = _hip_model(vited, s, gpu, dtype, state=oracle.state_dict()).train()
    imgs = torch.randn(n_img, 3, s.img_size, s.img_size).clamp(-1, 1)
    y = (torch.rand(pairs, s.num_classes) > 0.5).float()
    return oracle, model, imgs, y


A_I, A_J = [1, 3, 1, 2, 3, 3, 1], [0, 1, 2, 0, 2, 3, 3]         # image 0 is never image 1


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('depth,c_depth', [(1, 1), (2, 3)])
def test_config_a_geometry_against_the_oracle(vited, gpu, dtype, depth, c_depth):
    """D 384, 12 heads, 64 / 65 tokens, 4 images, 7 pairs.  (1, 1): norm_context + kv inside the block (unfolded) and the cross-attention
    of the cls-only last block (Nq = 1); (2, 3) in bf16: the folded kv of all blocks, in fp32 the unfolded exact path at depth."""
    s = vo.ViTEDShape(depth=depth, c_depth=c_depth)
    oracle, model, imgs, y = _setup(vited, gpu, dtype, s, 4, 7, seed=depth)
    i, j = torch.tensor(A_I), torch.tensor(A_J)
    lo, go, dfo = _oracle_two_stage(oracle, imgs, i, j, y)
    g_imgs, gi, gj, gy = imgs.to(gpu), i.to(gpu), j.to(gpu), y.to(gpu)
    lh, gh, dfh = _indexed_two_stage(vited, model, g_imgs, gi, gj, gy)
    assert lh.shape == (7, s.num_classes)
    assert set(gh) == set(go)
    _check_values(dtype, lh.cpu(), {**{n: g.cpu() for n, g in gh.items()}, 'd feats': dfh.cpu()}, lo, {**go, 'd feats': dfo})
    assert not bool(dfh[0].any()), 'image 0 is never image 1: its rows of d feats are exact zeros'
    assert bool(dfh[1:].flatten(1).any(1).all())
    _print_gap_to_gathered(model, g_imgs, gi, gj, gy, lh, gh)
    # under no_grad, from an int64 index or from prepared tables, the same logits
    with torch.no_grad():
        feats = model(g_imgs, forward_first_part=True)
        l1 = model(feats, g_imgs, x2_index=gj, x1_index=gi)
        l2 = model.forward_second_part_head(feats, g_imgs, x2_index=gj, x1_index=vited.ops.pair_segments(gi, 4))
    assert torch.equal(l1, lh) and torch.equal(l2, lh)


@pytest.mark.parametrize('dtype', DTYPES)
def test_flash_geometry_against_the_oracle_plain_and_scaled(vited, gpu, dtype):
    """256-pixel images, patch 16, 6 heads x 64, 2 + 2 blocks (257 / 256 tokens: the flash kernels), 3 images, 5 pairs - once plain,
    once with forced stochastic-depth scales (per image in the encoder, per PAIR in the decoder) against droppath_cases' composition."""
    s = vo.ViTEDShape(img_size=256, patch_size=16, num_classes=1, num_heads=6, depth=2, c_depth=2)
    oracle, model, imgs, y = _setup(vited, gpu, dtype, s, 3, 5, seed=2)
    i, j = torch.tensor([0, 2, 1, 2, 0]), torch.tensor([1, 0, 2, 2, 1])
    g_imgs, gi, gj, gy = imgs.to(gpu), i.to(gpu), j.to(gpu), y.to(gpu)
    lo, go, dfo = _oracle_two_stage(oracle, imgs, i, j, y)
    lh, gh, dfh = _indexed_two_stage(vited, model, g_imgs, gi, gj, gy)
    _check_values(dtype, lh.cpu(), {**{n: g.cpu() for n, g in gh.items()}, 'd feats': dfh.cpu()}, lo, {**go, 'd feats': dfo})
    _print_gap_to_gathered(model, g_imgs, gi, gj, gy, lh, gh)
    enc = dc.irregular_scales(0.5, s.depth, 2, 3, salt=7)
    dec = dc.irregular_scales(0.5, s.c_depth, 3, 5, salt=9)
    lo, go, dfo = _oracle_two_stage(oracle, imgs, i, j, y, enc, dec)
    lh, gh, dfh = _indexed_two_stage(vited, model, g_imgs, gi, gj, gy, enc.to(gpu), dec.to(gpu))
    _check_values(dtype, lh.cpu(), {**{n: g.cpu() for n, g in gh.items()}, 'd feats': dfh.cpu()}, lo, {**go, 'd feats': dfo})


@pytest.mark.parametrize('dtype', DTYPES)
def test_indexed_step_is_reproducible_and_leaves_the_gathered_form_alone(vited, gpu, dtype):
    s = vo.ViTEDShape(depth=2, c_depth=3)
    torch.manual_seed(5)
    state = vo.OracleViTED(s).state_dict()
    model, other = (_hip_model(vited, s, gpu, dtype, state=state).train() for _ in range(2))
    g = torch.Generator().manual_seed(6)
    imgs = torch.randn(4, 3, s.img_size, s.img_size, generator=g).clamp(-1, 1).to(gpu)
    y = (torch.rand(7, s.num_classes, generator=g) > 0.5).float().to(gpu)
    gi, gj = torch.tensor(A_I, device=gpu), torch.tensor(A_J, device=gpu)
    # a call without x1_index on a model that never ran the indexed form ...
    l_other, g_other = _gathered_two_stage(other, imgs, gi, gj, y)
    # two indexed runs from the same state: the same bits, logits and every parameter's gradient
    l1, g1, df1 = _indexed_two_stage(vited, model, imgs, gi, gj, y)
    l2, g2, df2 = _indexed_two_stage(vited, model, imgs, gi, gj, y)
    assert torch.equal(l1, l2) and torch.equal(df1, df2)
    assert set(g1) == set(g2) == {n for n, _ in model.named_parameters()}
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    # ... gives the bits of the same call after it
    l_after, g_after = _gathered_two_stage(model, imgs, gi, gj, y)
    assert torch.equal(l_after, l_other)
    for n in g_other:
        assert torch.equal(g_after[n], g_other[n]), n
    # a frozen encoder (detached features): the same decoder gradients, nothing for the encoder
    l3, g3, _ = _indexed_two_stage(vited, model, imgs, gi, gj, y, detach=True)
    assert torch.equal(l3, l1)
    dec_only = {n for n, p in model.named_parameters() if any(p is q for q in vited.engine._decoder_only_parameters(model))}
    assert dec_only and dec_only <= set(g3)
    for n in dec_only:
        assert torch.equal(g3[n], g1[n]), n
    assert not any(n.startswith('blocks.') for n in g3)


def test_x1_index_argument_checks(vited, gpu):
    s = vo.SHAPE_T
    torch.manual_seed(0)
    model = _hip_model(vited, s, gpu, torch.float32).train()
    imgs = torch.randn(3, 3, s.img_size, s.img_size, device=gpu).clamp(-1, 1)
    feats = model(imgs, forward_first_part=True)
    j = torch.tensor([0, 1, 2, 2], device=gpu)
    with pytest.raises(ValueError, match='outside'):
        model(feats, imgs, x2_index=j, x1_index=torch.tensor([0, 3, 1, 1], device=gpu))
    with pytest.raises(ValueError, match='pairs'):
        model(feats, imgs, x2_index=j, x1_index=torch.tensor([0, 1], device=gpu))
    with pytest.raises(ValueError, match='items'):
        model(feats, imgs, x2_index=j, x1_index=vited.ops.pair_segments(torch.tensor([0, 1, 1, 0], device=gpu), 2))
    model.keep_cam = True
    try:
        with pytest.raises(NotImplementedError, match='x1_index'):
            model(feats, imgs, x2_index=j, x1_index=torch.tensor([0, 2, 1, 1], device=gpu))
    finally:
        model.keep_cam = False
    out = model(feats, imgs, x2_index=j, x1_index=torch.tensor([0, 2, 1, 1]))        # a host index is moved
    assert out.shape == (4, s.num_classes) and out.requires_grad


def test_indexed_two_stage_train_step(vited, gpu):
    """TrainStep(forward_fn=indexed two-stage, eager) with FlatAdamW on config T's geometry, fed by hisfrag_prepare_indexed for three
    steps: finite losses, every Linear weight moved, and the first step's gradient norm is the gathered step's from the same state."""
    s, E = vo.SHAPE_T, vited.engine
    torch.manual_seed(0)
    state = vo.OracleViTED(s).state_dict()
    samples = torch.randn(9, 3, s.img_size, s.img_size, device=gpu).clamp(-1, 1)
    targets = torch.arange(3, device=gpu).repeat_interleave(3)

    def make(forward_fn):
        m = _hip_model(vited, s, gpu, torch.float32, state=state).train()
        opt = vited.optim.FlatAdamW(E.param_groups_no_decay_1d(m), model=m, lr=1e-3, weight_decay=0.05)
        return m, E.TrainStep(m, opt, clip_grad=5.0, amp=False, use_graph=False, forward_fn=forward_fn)

    m, step = make(lambda mod, b: mod(b[1], b[0], x2_index=b[2], x1_index=b[3]))
    mg, step_g = make(lambda mod, b: mod(b[1], b[0]))
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    losses, norms = [], []
    for it in range(3):
        gen = torch.Generator(device=gpu).manual_seed(it)
        batch, labels = E.hisfrag_prepare_indexed(m, samples, targets, amp=False, generator=gen)
        assert batch[0] is samples and batch[2].dtype == torch.int64 and isinstance(batch[3], vited.ops.PairSegments)
        assert batch[1].shape[0] == 9 and batch[2].numel() == labels.shape[0] == batch[3].index.numel() == 9 + 18
        losses.append(float(step.step(batch, labels)))
        norms.append(float(step.last_norm))
        if it == 0:
            gen = torch.Generator(device=gpu).manual_seed(it)
            (x, feats), labels_g = E.hisfrag_prepare_data(mg, samples, targets, amp=False, generator=gen)
            assert torch.equal(labels_g, labels) and torch.equal(x, samples[batch[2]])
            loss_g = float(step_g.step((x, feats), labels_g))
            norm_g = float(step_g.last_norm)
            print(f'first step: indexed loss {losses[0]:.6f} norm {norms[0]:.6f}; gathered loss {loss_g:.6f} norm {norm_g:.6f}')
            assert abs(norms[0] - norm_g) <= 1e-3 * norm_g and abs(losses[0] - loss_g) <= 1e-3 * abs(loss_g)
    assert all(torch.isfinite(torch.tensor(losses + norms))), (losses, norms)
    stuck = [n for n, p in m.named_parameters() if p.ndim == 2 and torch.equal(p.detach(), before[n])]
    assert not stuck, stuck
    # michigan's rule through the same entry: as many negatives as positives, both orders among the candidates
    batch, labels = E.hisfrag_prepare_indexed(m, samples, targets, amp=False, neg_per_pos=1.0, ordered_negatives=True,
                                              generator=torch.Generator(device=gpu).manual_seed(9))
    assert labels.shape[0] == 18 and float(labels.sum()) == 9
    assert float(step.step(batch, labels)) > 0
