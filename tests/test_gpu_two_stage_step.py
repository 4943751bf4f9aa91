"""engine.TwoStageTrainStep on the MI355X: the replayed step against the eagerly launched one, bit for bit (the
pair-indexed decoder and the fused loss are bitwise reproducible, so equality is the bar); one eager step against the existing eager
path (hisfrag_prepare_mined's pieces + TrainStep + mined_bce_with_logits); live draws under replay; the refusals.

6 images of 64 x 64 at depth 1 + 1, one output, 384 wide (64 / 65 tokens: amp reaches the MFMA kernels); capacity is one row more than
any labeling of 6 images needs, so every batch carries padding.  The labels cycle through two balanced batches, one without any pair
(every row is padding: the loss is an exact 0 and so is every gradient) and one without a negative."""
import pytest
import torch

import lr_schedule_cases as lc
from oracle import vited_oracle as vo

pytestmark = pytest.mark.gpu
N = 6
LABELS = ([0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 2, 2], [0, 1, 2, 3, 4, 5], [0] * 6)
SHAPE = vo.ViTEDShape(depth=1, c_depth=1, num_classes=1)


def _model(vited, gpu, s=SHAPE, state=None, **kw):
    m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                      embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads, **kw)
    m.compute_dtype = None               # follows autocast
    if state is not None:
        m.load_state_dict(state)
    return m.to(gpu).train()


@pytest.fixture(scope='module')
def init(vited, gpu):
    torch.manual_seed(13)
    return {k: v.clone() for k, v in _model(vited, gpu).state_dict().items()}


def _optimizer(vited, m, kind, lr):
    groups = vited.engine.param_groups_no_decay_1d(m)
    if kind == 'adamw':
        return vited.optim.FlatAdamW(groups, lr=lr, weight_decay=0.05)
    return vited.optim.FlatSGD(groups, lr=lr, momentum=0.9, nesterov=True, weight_decay=0.05)


def _same_mined(a, b):
    return (torch.equal(a.groups, b.groups) and torch.equal(a.labels, b.labels) and torch.equal(a.weights, b.weights)
            and torch.equal(a.counts, b.counts) and all(torch.equal(s, t) for s, t in zip(a.segments, b.segments)))


@pytest.mark.parametrize('kind,amp,accum', [('adamw', False, 1), ('adamw', True, 1), ('adamw', False, 2), ('sgd', False, 1)])
def test_replay_equals_eager_bit_for_bit(vited, gpu, init, kind, amp, accum):
    E = vited.engine
    capacity = E.mined_pair_capacity(N) + 1
    case = lc.BY_ID['cosine_prefix_warm2']
    keys = torch.zeros(N * N, device=gpu)
    models, steps = [], []
    for use_graph in (False, True):
        m = _model(vited, gpu, state=init)
        opt = _optimizer(vited, m, kind, lc.BASE_LR)
        sched = E.build_scheduler(lc.config(case), opt, lc.N_ITER, step_warmup_prefix=case['step_warmup_prefix'])
        step = E.TwoStageTrainStep(m, opt, capacity=capacity, clip_grad=5.0, amp=amp, use_graph=use_graph, accumulation_steps=accum,
                                   lr_scheduler=sched, meters=True)
        assert step.lr_on_device
        step.mine_keys = keys            # both read the one tensor in place; the captured graph too
        models.append(m)
        steps.append(step)
    g = torch.Generator().manual_seed(17)
    seen = set()
    for it in range(7 * accum):
        samples = torch.randn(N, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
        targets = torch.tensor(LABELS[it % len(LABELS)], device=gpu)
        keys.copy_(torch.rand(N * N, generator=g))
        le = steps[0].step(samples, targets).clone()
        mined_e = steps[0].last_mined
        lg = steps[1].step(samples, targets)
        assert torch.equal(le, lg), (it, float(le), float(lg))
        assert _same_mined(mined_e, steps[1].last_mined), it
        assert mined_e.counts[3].item() < capacity and mined_e.weights[-1].item() == 0.0        # every batch carries padding
        seen.add(tuple(mined_e.counts.tolist()))
        if steps[0].last_norm is not None:
            assert torch.equal(steps[0].last_norm, steps[1].last_norm), it
    assert seen == {(6, 9, 9, 15, 0), (3, 12, 6, 9, 0), (0, 15, 0, 0, 0), (15, 0, 0, 15, 0)}
    assert steps[1]._g1 is not None and steps[1]._g2 is not None and steps[1]._g_opt is not None and steps[1].recaptures == 0
    assert steps[0]._g1 is None and steps[0].num_updates == steps[1].num_updates == 7
    assert steps[0].meters.values() == steps[1].meters.values() and steps[0].meters.values()['nonfinite'] == 0
    assert torch.equal(steps[0].meters.state, steps[1].meters.state)
    for (n, pe), (_, pg) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert torch.equal(pe, pg), f'{n}: graph replay differs from eager launches'
    assert not torch.equal(models[0].head.weight, init['head.weight'])
    if amp:
        x = torch.randn(4, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            after = [m.eval()(x) for m in models]
            want = _model(vited, gpu, state=models[1].state_dict()).eval()(x)
        assert torch.equal(after[0], want) and torch.equal(after[1], want), 'stale bf16 weight shadows after the last update'


def test_one_eager_step_against_the_existing_eager_path(vited, gpu, init):
    """The same pairs through mine_pairs_device(keys=...) + forward_first_part + TrainStep(forward_fn, mined_bce_with_logits): loss and
    gradient norm within 1e-3 relative, the fp32 tolerance test_mined_two_stage_train_step uses for this comparison."""
    E = vited.engine
    capacity = E.mined_pair_capacity(N) + 1
    g = torch.Generator().manual_seed(3)
    samples = torch.randn(N, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
    targets = torch.tensor(LABELS[1], device=gpu)
    keys = torch.rand(N * N, generator=g).to(gpu)

    m = _model(vited, gpu, state=init)
    step = E.TwoStageTrainStep(m, _optimizer(vited, m, 'adamw', 1e-3), capacity=capacity, clip_grad=5.0, amp=False, use_graph=False)
    step.mine_keys = keys
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    loss, norm = float(step.step(samples, targets)), float(step.last_norm)

    mo = _model(vited, gpu, state=init)
    old = E.TrainStep(mo, _optimizer(vited, mo, 'adamw', 1e-3), clip_grad=5.0, amp=False, use_graph=False,
                      forward_fn=lambda mod, b: mod(b[1], b[0], x2_index=b[2], x1_index=b[3]), criterion=E.mined_bce_with_logits)
    mined = E.mine_pairs_device(targets, capacity, keys=keys)
    assert _same_mined(mined, step.last_mined) and mined.counts.tolist() == [3, 12, 6, 9, 0]
    feats = mo(samples, forward_first_part=True)
    loss_o = float(old.step((samples, feats, mined.groups[:, 0].contiguous(), mined.segments), mined))
    norm_o = float(old.last_norm)
    print(f'two-stage step loss {loss:.7f} norm {norm:.7f}; existing eager path loss {loss_o:.7f} norm {norm_o:.7f}')
    assert all(torch.isfinite(torch.tensor([loss, norm, loss_o, norm_o]))) and norm_o > 0
    assert abs(loss - loss_o) <= 1e-3 * abs(loss_o) and abs(norm - norm_o) <= 1e-3 * norm_o
    stuck = [n for n, p in m.named_parameters() if p.ndim == 2 and torch.equal(p.detach(), before[n])]
    assert not stuck, stuck


def test_live_draws_under_replay(vited, gpu):
    """No forced keys: every replay mines anew and draws its stochastic depth, patch dropout and position dropout anew.  With one block
    per half the model's drop-path rule (linspace(0, rate, blocks)) gives every block the rate 0 and the scales could never differ, so
    this test alone runs at depth 2 + 2."""
    E = vited.engine
    s = vo.ViTEDShape(depth=2, c_depth=2, num_classes=1)
    torch.manual_seed(5)
    m = _model(vited, gpu, s, drop_path_rate=0.1, patch_drop_rate=0.25, pos_drop_rate=0.1)
    step = E.TwoStageTrainStep(m, _optimizer(vited, m, 'adamw', 1e-4), capacity=E.mined_pair_capacity(N) + 1, amp=True, use_graph=True)
    samples = torch.randn(N, 3, 64, 64, device=gpu).clamp(-1, 1)
    targets = torch.tensor(LABELS[1], device=gpu)
    want = E.mine_pairs_device(torch.tensor(LABELS[1]), step.capacity).counts
    seen = []
    for it in range(4):
        loss = step.step(samples, targets)
        if it < 2:
            assert step._g1 is None
            continue
        assert step._g1 is not None and bool(torch.isfinite(loss))
        mined, drop = step.last_mined, m.last_drop_path
        seen.append((mined.groups.clone(), mined.counts.clone(), drop.enc.clone(), drop.dec.clone(), m.last_patch_keep.x2.clone(),
                     m.last_pos_drop.x1.clone()))
    (ga, ca, ea, da, ka, pa), (gb, cb, eb, db, kb, pb) = seen
    assert torch.equal(ca.cpu(), want) and torch.equal(cb.cpu(), want) and want.tolist() == [3, 12, 6, 9, 0]
    assert torch.equal(ga[:3], gb[:3]) and not torch.equal(ga, gb), 'two replays mined the same negatives'
    assert not (torch.equal(ea, eb) and torch.equal(da, db)), 'two replays drew the same drop-path scales'
    assert da.shape == (2, 3, step.capacity) and ea.shape == (2, 2, N)          # per pair in the decoder, per image in the encoder
    assert not torch.equal(ka, kb) and not torch.equal(pa, pb)
    assert step.recaptures == 0


def test_refusals_on_the_gpu_model(vited, gpu, init, monkeypatch):
    E = vited.engine
    m = _model(vited, gpu, state=init)
    opt = _optimizer(vited, m, 'adamw', 1e-4)
    with pytest.raises(ValueError, match=r'^TwoStageTrainStep: capacity'):
        E.TwoStageTrainStep(m, opt, capacity=vited.ops.MINE_MAX_CAPACITY + 1)
    with pytest.raises(ValueError, match='capturable=True'):
        E.TwoStageTrainStep(m, torch.optim.AdamW(m.parameters(), lr=1e-4), capacity=16, use_graph=True)
    step = E.TwoStageTrainStep(m, opt, capacity=16, amp=False)

    def no_launch(*a, **k):
        raise AssertionError('a refused call reached a launch')

    monkeypatch.setattr(vited._lib, 'call', no_launch)
    samples, targets = torch.zeros(N, 3, 64, 64, device=gpu), torch.tensor(LABELS[0], device=gpu)
    step.drop_path = vited.DropPathScales(torch.ones(1, 2, N, device=gpu), torch.ones(1, 3, 16, device=gpu))
    with pytest.raises(ValueError, match=r'^TwoStageTrainStep: step\.drop_path'):
        step.step(samples, targets)
    step.drop_path = None
    many = vited.ops.mine_pairs_max_images() + 1
    with pytest.raises(ValueError, match=rf'^TwoStageTrainStep: samples holds {many} images'):
        step.step(torch.zeros(many, 3, 64, 64, device=gpu), torch.zeros(many, dtype=torch.int64, device=gpu))
    assert step.num_updates == 0 and step.last_mined is None
