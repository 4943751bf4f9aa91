"""Lion in the fused update on the MI355X (vited_lion_step / vited_lion_step_ema, optim.FlatLion): the parameter
bag of tests/lamb_cases.py against the rule restated in fp32 - bit for bit - and in fp64, the shadows, what must keep its bits, and - on
the smallest oracle geometry (1 + 1 blocks, batch 2) - everything the step does around an optimizer.

Tolerances.  Against the fp32 restatement (tests/lion_cases.py: every product and every sum an operation of its own, the clip coefficient
taken from the kernel's own norm) parameters and exp_avg are equal bit for bit.  Against the fp64 restatement, on the elements that
never come near a tie of the sign (lion_cases.near_tie; their share is capped at 0.1 %), |p - p64| <= 1e-7: the step lr s is exact, so
an update rounds twice, p (1 - lr wd) and the difference, by half an ulp each, 2^-27 at |p| < 0.25, which over 5 updates is 7.5e-8
(the rounded 1 - lr wd adds 3e-8 |p| per update, 1.8e-8 in all at |p| <= 0.12); exp_avg at the bounds tests/test_gpu_lamb.py holds the first
moment to, rtol 1e-5 / atol 1e-9.  Whatever compares two runs of the same kernels is bit for bit."""
import copy
import types

import numpy as np
import pytest
import torch

import ema_cases as ec
import lion_cases as nc
import lr_schedule_cases as sc
from oracle import vited_oracle as vo
from test_gpu_engine import _hip_model

pytestmark = pytest.mark.gpu
lc = nc.lc


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


class Bound:
    """A fused optimizer over the bag, bound to a flat buffer and to a Runtime that holds the bf16 shadows of the 2-D and 4-D tensors."""

    def __init__(self, V, dev, override=None, cls=None, **opt_kw):
        self.ps = [torch.nn.Parameter(t.to(dev)) for t in lc.initial_parameters()]
        groups = nc.param_groups(self.ps, **(override or {}))
        self.opt = V.optim.FlatLion(groups, **nc.HYPER, **opt_kw) if cls is None else cls(groups, **lc.HYPER, **opt_kw)
        self.flat = V.engine.FlatGradients(self.ps)
        self.view_of = {id(p): v for p, v in zip(self.flat.params, self.flat.views)}
        self.rt = V.functions.Runtime(img_size=64, patch_size=8, in_chans=3, num_classes=4, embed_dim=384, depth=1, c_depth=1, num_heads=12)
        self.shadow_n = {i: self.rt.weight(p) for i, p in enumerate(self.ps) if p.ndim in (2, 4)}
        self.shadow_t = {i: self.rt.weight_t(p)[0] for i, p in enumerate(self.ps) if p.ndim == 2}
        self.opt.bind_flat(self.flat, types.SimpleNamespace(_runtimes={torch.bfloat16: self.rt}))

    def set_gradient(self, step):
        for p, g in zip(self.ps, lc.gradients(step)):
            self.view_of[id(p)].copy_(g)

    def shadows_current(self):
        ok = all(torch.equal(sh, self.ps[i].detach().reshape(self.ps[i].shape[0], -1).to(torch.bfloat16)) and self.rt.weight(self.ps[i]) is sh
                 for i, sh in self.shadow_n.items())
        return ok and all(torch.equal(sh, self.ps[i].detach().t().contiguous().to(torch.bfloat16)) for i, sh in self.shadow_t.items())

    def record(self, norm):
        o = self.opt
        return dict(norm=norm.detach().cpu().clone().reshape(1), p=[p.detach().cpu().clone() for p in self.ps],
                    m=[o.state[p]['exp_avg'].cpu().clone() for p in self.ps], shadows=self.shadows_current(),
                    grad_max=float(self.flat.flat.abs().max()))


_RUNS = {}


def run(V, dev, variant='plain', fresh=False):
    """nc.UPDATES updates of the bag, one record per update; computed once per variant and shared between the tests."""
    kw = {'plain': {}, 'no_decay': dict(override=dict(weight_decay=0.0))}[variant]
    if fresh or variant not in _RUNS:
        b = Bound(V, dev, **kw)
        assert set(b.opt.state[b.ps[0]]) == {'exp_avg'} and b.opt.exp_avg.numel() == b.flat.flat.numel()       # installed at bind
        records = []
        for step in range(nc.UPDATES):
            b.set_gradient(step)
            records.append(b.record(b.opt.step_flat(nc.MAX_NORM)))
        assert b.opt.num_updates == nc.UPDATES and b.opt.skipped_updates == 0
        if fresh:
            return records
        _RUNS[variant] = records
    return _RUNS[variant]


# ---- the bag ---------------------------------------------------------------------------------------------------------------------
def test_bag_against_the_fp32_restatement_bit_for_bit(vited, gpu):
    records = run(vited, gpu)
    want = nc.run(torch.float32, norms=[float(rec['norm']) for rec in records])
    adamw = Bound(vited, gpu, cls=vited.optim.FlatAdamW)
    for step, (rec, w) in enumerate(zip(records, want)):
        adamw.set_gradient(step)
        assert same(rec['norm'], adamw.opt.step_flat(nc.MAX_NORM).reshape(1)), step         # the norm vited_adamw_step reports
        assert abs(float(rec['norm']) - float(lc.clip_coef(lc.gradients(step), nc.MAX_NORM, torch.float64)[0])) <= 1e-5 * float(rec['norm'])
        for i, shape in enumerate(nc.SHAPES):
            off = int((bits(rec['p'][i]) != bits(w['p'][i])).sum()), int((bits(rec['m'][i]) != bits(w['m'][i])).sum())
            assert off == (0, 0), f'update {step} {shape} ({nc.KINDS[i]}): {off[0]} parameters and {off[1]} moments differ in their bits'
        assert rec['shadows'], step                                                         # both shadows are bf16(p)
        assert rec['grad_max'] == 0.0                                                       # zero_grad fused in
    assert float(records[1]['norm']) > nc.MAX_NORM > float(records[2]['norm']) and float(records[3]['norm']) > nc.MAX_NORM


def test_bag_against_the_fp64_restatement(vited, gpu):
    records, f64 = run(vited, gpu), nc.run(torch.float64)
    near = nc.near_tie(f64)
    excluded = sum(int(t.sum()) for t in near)
    assert excluded <= nc.TIE_SHARE * nc.TOTAL
    worst = 0.0
    for step, (rec, w) in enumerate(zip(records, f64)):
        assert abs(float(rec['norm']) - w['norm']) <= 1e-5 * w['norm'] + 1e-7
        for i, shape in enumerate(nc.SHAPES):
            err = (rec['p'][i].double() - w['p'][i]).abs()[~near[i]]
            worst = max(worst, float(err.max()) if err.numel() else 0.0)
            torch.testing.assert_close(rec['m'][i].double(), w['m'][i], rtol=1e-5, atol=1e-9, msg=lambda m: f'update {step} exp_avg {shape}: {m}')
            assert bool(torch.isfinite(rec['p'][i]).all())
    print(f'excluded {excluded} of {nc.TOTAL} elements; worst |p - p64| elsewhere {worst:.2e}')
    assert worst <= 1e-7


def test_without_decay_every_element_moves_by_lr_or_not_at_all(vited, gpu):
    records = run(vited, gpu, 'no_decay')
    before = lc.initial_parameters()
    moved = {-1: 0, 0: 0, 1: 0}
    for rec in records:
        for i, p in enumerate(rec['p']):
            lr = torch.tensor(nc.group_settings(nc.GROUP_OF[i])['lr'], dtype=torch.float32)
            up, down, stay = bits(before[i] + lr) == bits(p), bits(before[i] - lr) == bits(p), bits(before[i]) == bits(p)
            assert bool((up | down | stay).all()), nc.SHAPES[i]
            moved[1] += int(up.sum()); moved[-1] += int(down.sum()); moved[0] += int((stay & ~up & ~down).sum())
        before = rec['p']
    assert moved[1] > 1000 and moved[-1] > 1000 and moved[0] == nc.UPDATES * sum(n for n, k in zip(nc.NUMEL, nc.KINDS) if k in ('zero_g', 'zero_both'))


def test_the_zero_kinds(vited, gpu):
    records = run(vited, gpu)
    kind = {k: nc.KINDS.index(k) for k in ('zero_p', 'zero_g', 'zero_both')}
    s = nc.group_settings(nc.GROUP_OF[kind['zero_g']])
    lr, wd = torch.tensor(s['lr'], dtype=torch.float32), torch.tensor(s['weight_decay'], dtype=torch.float32)
    decay = 1.0 - lr * wd
    p = lc.initial_parameters()[kind['zero_g']]
    for rec in records:
        p = p * decay                                                                       # no gradient: the parameter only decays
        assert same(rec['p'][kind['zero_g']], p) and float(rec['m'][kind['zero_g']].abs().max()) == 0.0
        assert not bits(rec['p'][kind['zero_both']]).any() and not bits(rec['m'][kind['zero_both']]).any()       # exactly +0
    assert bool((records[0]['p'][kind['zero_p']].abs() == lr).all())                        # p = 0 under a gradient: one step of lr


def test_kept_gradients_keep_their_bits(vited, gpu):
    b = Bound(vited, gpu)
    records = run(vited, gpu)
    for step in range(2):
        b.set_gradient(step)
        before = bits(b.flat.flat)
        b.opt.step_flat(nc.MAX_NORM, zero_grad=False)
        assert np.array_equal(bits(b.flat.flat), before) and before.any()
        assert all(same(p, w) for p, w in zip(b.ps, records[step]['p']))               # and the update is the one that zeroes them


def test_two_runs_give_the_same_bits(vited, gpu):
    first, second = run(vited, gpu), run(vited, gpu, fresh=True)
    for a, b in zip(first, second):
        assert all(same(x, y) for what in ('p', 'm') for x, y in zip(a[what], b[what])) and same(a['norm'], b['norm'])


# ---- the smallest oracle geometry ------------------------------------------------------------------------------------------------------
N, LABELS = 6, ([0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 2, 2], [0, 1, 2, 3, 4, 5], [0] * 6)       # the two-stage step's images and their classes


@pytest.fixture(scope='module')
def shape():
    return vo.ViTEDShape(depth=1, c_depth=1)


@pytest.fixture(scope='module')
def init(vited, gpu, shape):
    torch.manual_seed(19)
    return _hip_model(vited, shape, gpu, None).state_dict()


def _batches(n, dev, seed=5, nan_at=None):
    g = torch.Generator().manual_seed(seed)
    out = []
    for it in range(n):
        x = torch.randn(2, 2, 3, 64, 64, generator=g).clamp(-1, 1)
        y = (torch.rand(2, 4, generator=g) > 0.6).float()
        if it == nan_at:
            x[1, 0, 1, 17, 5] = float('nan')
        out.append((x.to(dev), y.to(dev)))
    return out


def _step(V, dev, shape, init, case=None, on_device=None, cls=None, lr=1e-4, load=None, two_stage=False, **kw):
    """model, optimizer and step on the shared initial weights; ``case``: a tests/lr_schedule_cases.py schedule; ``load``: (model state,
    optimizer state) loaded BEFORE the step binds the optimizer (the reference's resume order)."""
    m = _hip_model(V, shape, dev, None)
    m.load_state_dict(init if load is None else load[0])
    opt_kw = {k: kw.pop(k) for k in ('ema_decay', 'ema_warmup', 'skip_nonfinite') if k in kw}
    opt = (cls or V.optim.FlatLion)(V.engine.param_groups_no_decay_1d(m), lr=sc.BASE_LR if case else lr, weight_decay=0.05, model=m, **opt_kw)
    if load is not None:
        opt.load_state_dict(load[1])
        assert opt.flat is None
    if case:
        kw['lr_scheduler'] = V.engine.build_scheduler(sc.config(case), opt, sc.N_ITER, step_warmup_prefix=case['step_warmup_prefix'])
        if on_device is not None:
            kw['lr_scheduler'].on_device = on_device
    if two_stage:
        step = V.engine.TwoStageTrainStep(m, opt, capacity=V.engine.mined_pair_capacity(N) + 1, clip_grad=5.0, amp=True, **kw)
    else:
        step = V.engine.TrainStep(m, opt, clip_grad=5.0, amp=True, **kw)
    return m, opt, step


def _state_bits(opt):
    return [bits(opt._bufs[n]) for n in opt._state_names] + [bits(opt._hyper)]


def _shadow_bits(V, m):
    names = {id(p): n for n, p in m.named_parameters()}
    return {(names[pid], tag): bits(buf) for cache in V.functions.shadows_of(m) for pid, tags in cache.buffers().items()
            for tag, buf in tags.items()}


def _same_models(a, b):
    for (name, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert same(p, q), name


def test_replayed_step_equals_the_eager_one(vited, gpu, shape, init):
    runs = [_step(vited, gpu, shape, init, use_graph=ug) for ug in (False, True)]
    for x, y in _batches(3 + 2, gpu):                                                  # two eager steps and the capture, then 3 replays
        le, lg = [st.step(x, y) for _, _, st in runs]
        assert same(le.reshape(1), lg.reshape(1))
        assert same(runs[0][2].last_norm.reshape(1), runs[1][2].last_norm.reshape(1))
    (me, oe, se), (mg, og, sg) = runs
    assert se._g1 is None and sg._g_opt is not None and sg.recaptures == 0 and oe.num_updates == og.num_updates == 5
    _same_models(me, mg)
    assert not same(mg.head.weight, init['head.weight'])
    assert all(np.array_equal(a, b) for a, b in zip(_state_bits(oe), _state_bits(og)))
    assert _shadow_bits(vited, mg) and all(np.array_equal(a, _shadow_bits(vited, me)[k]) for k, a in _shadow_bits(vited, mg).items())


def test_captured_two_stage_step_equals_the_eager_one(vited, gpu):
    s = vo.ViTEDShape(depth=1, c_depth=1, num_classes=1)
    torch.manual_seed(23)
    start = _hip_model(vited, s, gpu, None).state_dict()
    runs = [_step(vited, gpu, s, start, two_stage=True, use_graph=ug) for ug in (False, True)]
    g = torch.Generator().manual_seed(17)
    keys = torch.rand(N * N, generator=g).to(gpu)
    for _, _, st in runs:
        st.mine_keys = keys
    for it in range(4):                                                                # two eager steps, the capture, one replayed step
        samples = torch.randn(N, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
        targets = torch.tensor(LABELS[it % 2], device=gpu)
        le, lg = [st.step(samples, targets).clone() for _, _, st in runs]
        assert same(le.reshape(1), lg.reshape(1)) and same(runs[0][2].last_norm.reshape(1), runs[1][2].last_norm.reshape(1)), it
    (me, oe, se), (mg, og, sg) = runs
    assert sg._g1 is not None and sg._g2 is not None and sg._g_opt is not None and sg.recaptures == 0 and se._g1 is None
    assert oe.num_updates == og.num_updates == 4
    _same_models(me, mg)
    assert not same(mg.head.weight, start['head.weight']) and all(np.array_equal(a, b) for a, b in zip(_state_bits(oe), _state_bits(og)))


def test_a_nan_batch_is_skipped_and_leaves_everything_alone(vited, gpu, shape, init):
    m, opt, step = _step(vited, gpu, shape, init, skip_nonfinite=True, ema_decay=0.9)

    def snapshot():
        return ([bits(p) for p in m.parameters()] + [bits(opt.exp_avg), bits(opt.ema)] + list(_shadow_bits(vited, m).values()),
                (opt.num_updates, opt.num_ema_updates, opt.skipped_updates))

    for it, (x, y) in enumerate(_batches(4, gpu, nan_at=2)):
        before = snapshot()
        step.step(x, y)
        after = snapshot()
        assert float(opt.flat.flat.abs().max()) == 0.0                                 # the gradients are zeroed either way
        if it == 2:
            assert not torch.isfinite(step.last_norm)
            assert len(before[0]) == len(after[0]) and all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
            assert after[1] == (before[1][0], before[1][1], before[1][2] + 1)
        else:
            assert any(not np.array_equal(a, b) for a, b in zip(before[0], after[0]))
            assert after[1] == (before[1][0] + 1, before[1][1] + 1, before[1][2])
    assert opt.num_updates == 3 and opt.skipped_updates == 1 and all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_the_average_follows_the_lion_updated_parameters(vited, gpu, shape, init):
    m, opt, step = _step(vited, gpu, shape, init, ema_decay=0.5, ema_warmup=True)
    plain = _step(vited, gpu, shape, init)
    params = list(opt.flat.params)
    assert all(same(opt.ema_of(p), p) for p in params)
    for n, (x, y) in enumerate(_batches(3, gpu)):
        e_before = [bits(opt.ema_of(p)).view(np.float32) for p in params]
        step.step(x, y)
        plain[2].step(x, y)
        for e, p in zip(e_before, params):
            want = ec.update(e, bits(p).view(np.float32), 0.5, True, n)[0]              # ema_blend's statement on the device's own new p
            assert np.array_equal(bits(opt.ema_of(p)), want.view(np.int32))
    assert opt.num_ema_updates == 3
    _same_models(m, plain[0])                                                          # keeping the average changes nothing else
    assert same(opt.exp_avg, plain[1].exp_avg)
    # the exchange for an evaluation, and back
    before = ([bits(p) for p in params], bits(opt.ema), _state_bits(opt))
    with opt.swap_ema():
        assert all(np.array_equal(bits(opt.ema_of(p)), w) for p, w in zip(params, before[0])) and not np.array_equal(bits(opt.ema), before[1])
    after = ([bits(p) for p in params], bits(opt.ema), _state_bits(opt))
    assert all(np.array_equal(a, b) for a, b in zip(before[0] + [before[1]] + before[2], after[0] + [after[1]] + after[2]))
    averaged = opt.ema_state_dict(m)
    assert list(averaged) == list(m.state_dict()) and not same(averaged['head.weight'], m.head.weight)


def test_device_stepped_schedule_equals_the_host_stepped_one(vited, gpu, shape, init):
    """linear_warm2: warm-up and linear decay, + - * / alone, which fp64 rounds alike on the host and the device - so the two runs see
    the same fp32 rates and must agree in every bit."""
    case = sc.BY_ID['linear_warm2']
    runs = [_step(vited, gpu, shape, init, case=case, on_device=od, use_graph=ug) for od, ug in ((None, True), (False, False))]
    assert [r[2].lr_on_device for r in runs] == [True, False]
    rates = [[], []]
    for x, y in _batches(12, gpu):                                                     # 10 warm-up iterations, then the decay
        ld, lh = [st.step(x, y) for _, _, st in runs]
        assert same(ld.reshape(1), lh.reshape(1))
        for r, seen in zip(runs, rates):
            seen.append(r[1]._hyper[8::8].tolist())
    assert rates[0][:-1] == rates[1][1:] and len({tuple(r) for r in rates[0]}) >= 10   # the host-stepped array holds what the update consumed
    assert runs[0][1].hyper_uploads == 1 and runs[1][1].hyper_uploads > 1 and runs[0][2].recaptures == 0
    _same_models(runs[0][0], runs[1][0])
    assert same(runs[0][1].exp_avg, runs[1][1].exp_avg) and not same(runs[0][0].head.weight, init['head.weight'])


def test_find_lr_sweeps_and_restores_bit_for_bit(vited, gpu, shape, init):
    m, opt, step = _step(vited, gpu, shape, init)
    for x, y in _batches(2, gpu):
        step.step(x, y)
    before = ([bits(p) for p in m.parameters()], _state_bits(opt), [g['lr'] for g in opt.param_groups])
    result = vited.engine.find_lr(step, _batches(3, gpu, seed=3), num_iter=3, start_lr=1e-6, end_lr=1e-3, restore=True)
    assert result.iterations == 3
    after = ([bits(p) for p in m.parameters()], _state_bits(opt), [g['lr'] for g in opt.param_groups])
    assert all(np.array_equal(a, b) for a, b in zip(before[0] + before[1], after[0] + after[1])) and before[2] == after[2]
    assert opt.num_updates == 2 and set(opt.state[opt.flat.params[0]]) == {'exp_avg'}
    kept = vited.engine.find_lr(step, _batches(3, gpu, seed=3), num_iter=3, start_lr=1e-6, end_lr=1e-3, restore=False)
    assert kept.iterations == 3 and opt.num_updates == 5 and any(not np.array_equal(bits(p), w) for p, w in zip(m.parameters(), before[0]))


def test_state_dict_round_trips_before_and_after_bind(vited, gpu, shape, init):
    ma, oa, sa = _step(vited, gpu, shape, init)
    data = _batches(3, gpu)
    for x, y in data[:2]:
        sa.step(x, y)
    saved, weights = copy.deepcopy(oa.state_dict()), copy.deepcopy(ma.state_dict())
    assert all(set(st) == {'exp_avg'} for st in saved['state'].values()) and len(saved['state']) == len(oa.flat.params)      # timm Lion's layout
    mb, ob, sb = _step(vited, gpu, shape, init, load=(weights, copy.deepcopy(saved)))   # loaded before the step binds the optimizer
    mc, oc, stc = _step(vited, gpu, shape, init)                                       # ... and into a bound one
    buffer = oc.exp_avg.data_ptr()
    mc.load_state_dict(weights)
    oc.load_state_dict(copy.deepcopy(saved))
    assert oc.exp_avg.data_ptr() == buffer
    for o in (ob, oc):
        final = o.state_dict()
        assert final['param_groups'] == saved['param_groups'] and set(final['state']) == set(saved['state'])
        assert all(set(st) == {'exp_avg'} and same(st['exp_avg'], saved['state'][k]['exp_avg']) for k, st in final['state'].items())
    x, y = data[2]                                                                     # and the resumed runs continue as the original
    la, lb, lc_ = sa.step(x, y), sb.step(x, y), stc.step(x, y)
    assert same(la.reshape(1), lb.reshape(1)) and same(la.reshape(1), lc_.reshape(1))
    _same_models(ma, mb)
    _same_models(ma, mc)
    assert same(oa.exp_avg, ob.exp_avg) and same(oa.exp_avg, oc.exp_avg)


def test_an_adamw_checkpoint_goes_in_after_bind_without_a_recapture(vited, gpu, shape, init):
    madam, oadam, sadam = _step(vited, gpu, shape, init, cls=vited.optim.FlatAdamW, lr=1e-3)
    data = _batches(5, gpu)
    for x, y in data[:2]:
        sadam.step(x, y)
    saved = copy.deepcopy(oadam.state_dict())
    assert set(saved['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'}
    runs = [_step(vited, gpu, shape, init, use_graph=ug) for ug in (False, True)]
    for x, y in data[:4]:                                                              # the graph run has captured and replayed
        for _, _, st in runs:
            st.step(x, y)
    for m, o, st in runs:
        buffer = o.exp_avg.data_ptr()
        o.load_state_dict(copy.deepcopy(saved))
        assert o.exp_avg.data_ptr() == buffer and same(o.exp_avg, oadam.exp_avg)       # copied INTO the buffer the graph reads
        assert all(set(s) == {'exp_avg'} for s in o.state.values()) and all(set(s) == {'exp_avg'} for s in o.state_dict()['state'].values())
        assert o.param_groups[0]['lr'] == 1e-3 and o.num_updates == 4                  # the groups are the checkpoint's, the count is this run's
    losses = [st.step(*data[4]) for _, _, st in runs]
    assert same(losses[0].reshape(1), losses[1].reshape(1)) and runs[1][2].recaptures == 0 and runs[1][2]._g_opt is not None
    _same_models(runs[0][0], runs[1][0])
    assert same(runs[0][1].exp_avg, runs[1][1].exp_avg) and not same(runs[1][1].exp_avg, oadam.exp_avg)


@pytest.mark.parametrize('name', ['lion', 'Lion'])
def test_build_optimizer_gives_flat_lion_on_a_gpu_model(vited, gpu, shape, name):
    m = _hip_model(vited, shape, gpu, None)
    o = types.SimpleNamespace(NAME=name, EPS=1e-6, BETAS=(0.95, 0.98), MOMENTUM=0.9)
    cfg = types.SimpleNamespace(TRAIN=types.SimpleNamespace(OPTIMIZER=o, BASE_LR=2e-4, WEIGHT_DECAY=0.5))
    for kw in (dict(), dict(fused_hip=True)):
        opt = vited.engine.build_optimizer(cfg, m, skip_nonfinite=True, ema_decay=0.99, **kw)
        assert type(opt) is vited.optim.FlatLion and opt.skip_nonfinite and opt.ema_decay == 0.99
        assert [g['weight_decay'] for g in opt.param_groups] == [0.5, 0.0]
        assert all(p.ndim == 1 for p in opt.param_groups[1]['params']) and all(p.ndim > 1 for p in opt.param_groups[0]['params'])
        assert opt.defaults['lr'] == 2e-4 and opt.defaults['betas'] == (0.95, 0.98) and 'eps' not in opt.defaults
    with pytest.raises(ValueError, match='unknown optimizer lion .*HIP optimizer only'):
        vited.engine.build_optimizer(cfg, m, fused_hip=False)
