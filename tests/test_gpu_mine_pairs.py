"""Pair mining on the MI355X (vited_mine_pairs): the kernel against the CPU statement of the rule, exactly;
mining + loss inside one captured graph (which raises on any host read); the model on padded against exact pair lists."""
import pytest
import torch

import mine_cases as mc
from oracle import vited_oracle as vo
from test_gpu_droppath import _check_values, _hip_model
from test_gpu_pair_index import _oracle_two_stage

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]


def _kernel_with_sentinels(ops, case, keys, capacity, gpu):
    """ops.mine_pairs' launch into buffers filled with -1 / NaN: an element the kernel leaves alone shows."""
    n = len(case.targets)
    ints = lambda *shape: torch.full(shape, -1, dtype=torch.int64, device=gpu)
    nans = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=gpu)
    groups, labels, weights, index, order, offsets = ints(capacity, 2), nans(capacity, 1), nans(capacity, 1), ints(capacity), ints(capacity), ints(n + 1)
    counts = torch.full((5,), -1, dtype=torch.int32, device=gpu)
    ops.mine_pairs_out(torch.tensor(case.targets, device=gpu), keys.to(gpu), case.neg_per_pos, case.ordered, groups, labels, weights, index,
                       order, offsets, counts)
    c = lambda t: t.cpu().numpy()
    return dict(groups=c(groups), labels=c(labels), weights=c(weights), counts=c(counts), seg_index=c(index), seg_order=c(order),
                seg_offsets=c(offsets))


def _cpu(E, case, keys, capacity):
    return mc.as_numpy(E.mine_pairs_device(torch.tensor(case.targets), capacity, neg_per_pos=case.neg_per_pos, ordered_negatives=case.ordered,
                                           keys=keys))


@pytest.mark.parametrize('case', mc.CASES + mc.EXTRA_GPU_CASES, ids=lambda c: c.name)
def test_kernel_against_the_cpu_path(vited, gpu, case):
    n = len(case.targets)
    variants = [(mc.make_keys(n, seed=n), mc.capacities(case)), (mc.make_keys(n, seed=3, levels=4), mc.capacities(case)[:1]),
                (mc.make_keys(n, seed=0, levels=0), mc.capacities(case)[1:2])]
    if case.positives > 1:
        variants.append((mc.make_keys(n, seed=1), [('cut_positives', case.positives - 1)]))
    for keys, caps in variants:
        for label, capacity in caps:
            got = _kernel_with_sentinels(vited.ops, case, keys, capacity, gpu)
            mc.assert_same(got, _cpu(vited.engine, case, keys, capacity), f'{case.name} {label}')
    mined = vited.engine.mine_pairs_device(torch.tensor(case.targets, device=gpu), case.pairs + 5, neg_per_pos=case.neg_per_pos,
                                           ordered_negatives=case.ordered, keys=mc.make_keys(n, seed=n).to(gpu))
    mc.assert_same(mc.as_numpy(mined), _cpu(vited.engine, case, mc.make_keys(n, seed=n), case.pairs + 5), f'{case.name} through engine')


def test_more_than_128_images_never_launch(vited, gpu, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError('a bad argument reached the launch')

    monkeypatch.setattr(vited._lib, 'call', no_launch)
    t, k = torch.zeros(129, dtype=torch.int64, device=gpu), torch.zeros(129 * 129, device=gpu)
    with pytest.raises(ValueError, match='129 images'):
        vited.ops.mine_pairs(t, k, 2.0, False, 64)
    with pytest.raises(ValueError, match='capacity'):
        vited.ops.mine_pairs(t[:4], k[:16], 2.0, False, vited.ops.MINE_MAX_CAPACITY + 1)
    with pytest.raises(ValueError):
        vited.ops.mine_pairs(t[:4], k[:16].cpu(), 2.0, False, 6)


def test_default_keys_come_from_the_device_generator(vited, gpu):
    E, t = vited.engine, torch.tensor(mc.BY_NAME['hisfrag_24'].targets, device=gpu)
    a = E.mine_pairs_device(t, 72, generator=torch.Generator(device=gpu).manual_seed(4))
    b = E.mine_pairs_device(t, 72, keys=torch.rand(576, generator=torch.Generator(device=gpu).manual_seed(4), device=gpu))
    assert torch.equal(a.groups, b.groups) and a.counts.tolist() == [24, 252, 48, 72, 0]
    torch.manual_seed(7)
    c = E.mine_pairs_device(t, 72)
    torch.manual_seed(7)
    d = E.mine_pairs_device(t, 72)
    assert torch.equal(c.groups, d.groups) and not torch.equal(c.groups, a.groups)


def test_mining_and_loss_in_one_captured_graph(vited, gpu):
    """A host read inside mine_pairs_device or mined_bce_with_logits makes the capture raise."""
    E, capacity = vited.engine, 80
    batches = [(mc.BY_NAME['hisfrag_24'].targets, 5), ([c for c in range(6) for _ in range(4)], 6)]       # 72 pairs; 36 + 72 > 80
    static_t = torch.zeros(24, dtype=torch.int64, device=gpu)
    static_k, static_x = torch.zeros(576, device=gpu), torch.zeros(capacity, 1, device=gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            E.mined_bce_with_logits(static_x, E.mine_pairs_device(static_t, capacity=capacity, keys=static_k))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mined = E.mine_pairs_device(static_t, capacity=capacity, keys=static_k)
        loss = E.mined_bce_with_logits(static_x, mined)
    for targets, seed in batches:
        keys = mc.make_keys(24, seed=seed)
        logits = torch.randn(capacity, 1, generator=torch.Generator().manual_seed(seed)) * 2
        static_t.copy_(torch.tensor(targets))
        static_k.copy_(keys)
        static_x.copy_(logits)
        graph.replay()
        torch.cuda.synchronize()
        want = E.mine_pairs_device(torch.tensor(targets), capacity=capacity, keys=keys)
        mc.assert_same(mc.as_numpy(mined), mc.as_numpy(want), f'replay with seed {seed}')
        torch.testing.assert_close(loss.cpu(), E.mined_bce_with_logits(logits, want))
    assert mined.counts.tolist() == [36, 240, 44, 80, 28]


def _mined_two_stage(E, model, imgs, targets, capacity, seed):
    model.zero_grad(set_to_none=True)
    batch, mined = E.hisfrag_prepare_mined(model, imgs, targets, capacity, amp=False, generator=torch.Generator(device=imgs.device).manual_seed(seed))
    samples, feats, x2_index, segments = batch
    assert samples is imgs and x2_index.shape == (capacity,) and segments.index.shape == (capacity,) and segments.items == imgs.shape[0]
    feats.retain_grad()
    logits = model(feats, samples, x2_index=x2_index, x1_index=segments)
    E.mined_bce_with_logits(logits, mined).backward()
    grads = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
    return logits.detach(), grads, feats.grad.detach().clone(), mined


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('depth,c_depth', [(1, 1), (2, 3)])
def test_model_on_padded_against_exact_pairs(vited, gpu, dtype, depth, c_depth):
    """4 images [0, 0, 1, 1]: 2 positives + 4 negatives.  Capacity 8 adds two padding rows (pair (0, 0), weight 0) at the end of
    image 0's group - and image 0 is nobody's image 1 here, so its rows of d feats stay exact zeros."""
    E, s = vited.engine, vo.ViTEDShape(depth=depth, c_depth=c_depth)
    torch.manual_seed(depth)
    oracle = vo.OracleViTED(s)
    model = _hip_model(vited, s, gpu, dtype, state=oracle.state_dict()).train()
    imgs = torch.randn(4, 3, s.img_size, s.img_size).clamp(-1, 1)
    targets = torch.tensor([0, 0, 1, 1], device=gpu)
    l6, g6, df6, m6 = _mined_two_stage(E, model, imgs.to(gpu), targets, 6, seed=3)
    l8, g8, df8, m8 = _mined_two_stage(E, model, imgs.to(gpu), targets, 8, seed=3)
    assert m6.counts.tolist() == [2, 4, 4, 6, 0] == m8.counts.tolist() and torch.equal(m8.groups[:6], m6.groups)
    assert m8.groups[6:].tolist() == [[0, 0], [0, 0]] and m8.weights.flatten().tolist() == [1.] * 6 + [0.] * 2
    assert l8.shape == (8, s.num_classes) and torch.equal(l8[:6], l6), 'the logits of the real pairs do not depend on the padding'
    pairs = m8.groups[:6].cpu()
    y = m8.labels[:6].cpu().expand(6, s.num_classes).contiguous()
    lo, go, dfo = _oracle_two_stage(oracle, imgs, pairs[:, 1], pairs[:, 0], y)
    assert set(g8) == set(go)
    _check_values(dtype, l8[:6].cpu(), {**g8, 'd feats': df8.cpu()}, lo, {**go, 'd feats': dfo})
    assert 0 not in pairs[:, 1].tolist() and not bool(df8[0].any()), 'image 0 is never image 1: its rows of d feats are exact zeros'
    assert bool(df8[1:].flatten(1).any(1).all())


def test_mined_two_stage_train_step(vited, gpu):
    """One eager TrainStep fed by hisfrag_prepare_mined at capacity 8 (two padding rows) against the same step fed with the same six
    pairs in the same order in hisfrag_prepare_indexed's form: loss and gradient norm within that test's fp32 tolerances."""
    s, E = vo.SHAPE_T, vited.engine
    torch.manual_seed(0)
    state = vo.OracleViTED(s).state_dict()
    samples = torch.randn(4, 3, s.img_size, s.img_size, device=gpu).clamp(-1, 1)
    targets = torch.tensor([0, 0, 1, 1], device=gpu)
    forward = lambda mod, b: mod(b[1], b[0], x2_index=b[2], x1_index=b[3])

    def make(criterion):
        m = _hip_model(vited, s, gpu, torch.float32, state=state).train()
        opt = vited.optim.FlatAdamW(E.param_groups_no_decay_1d(m), model=m, lr=1e-3, weight_decay=0.05)
        return m, E.TrainStep(m, opt, clip_grad=5.0, amp=False, use_graph=False, forward_fn=forward, criterion=criterion)

    m, step = make(E.mined_bce_with_logits)
    mi, step_i = make(None)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    batch, mined = E.hisfrag_prepare_mined(m, samples, targets, 8, amp=False, generator=torch.Generator(device=gpu).manual_seed(1))
    loss = float(step.step(batch, mined))
    norm = float(step.last_norm)
    feats = mi(samples, forward_first_part=True)
    batch_i = (samples, feats, mined.groups[:6, 0].contiguous(), vited.ops.pair_segments(mined.groups[:6, 1].contiguous(), 4))
    loss_i = float(step_i.step(batch_i, mined.labels[:6]))
    norm_i = float(step_i.last_norm)
    print(f'mined (capacity 8) loss {loss:.6f} norm {norm:.6f}; indexed (6 pairs) loss {loss_i:.6f} norm {norm_i:.6f}')
    assert all(torch.isfinite(torch.tensor([loss, norm, loss_i, norm_i])))
    assert abs(norm - norm_i) <= 1e-3 * norm_i and abs(loss - loss_i) <= 1e-3 * abs(loss_i)
    stuck = [n for n, p in m.named_parameters() if p.ndim == 2 and torch.equal(p.detach(), before[n])]
    assert not stuck, stuck
