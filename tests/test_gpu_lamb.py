"""LAMB in the fused update on the MI355X (vited_lamb_step / vited_lamb_step_ema, optim.FlatLAMB): the parameter
bag of tests/lamb_cases.py against the rule restated in fp64 and against torch.optim.AdamW, the trust ratios, the shadows, what must
keep its bits, and - on the smallest oracle geometry (1 + 1 blocks, batch 2) - everything the step does around an optimizer.

Tolerances.  Parameters, exp_avg and exp_avg_sq: those of tests/test_gpu_optim_sgd.py and of the AdamW parity test in
tests/test_gpu_engine.py - parameters rtol 2e-6 with atol 1e-3 * lr, exp_avg rtol 1e-5 / atol 1e-9, exp_avg_sq rtol 1e-5 / atol 1e-12, the
norm rtol 1e-5.  Trust ratios: relative (chain + 2) * 2^-24, where chain is the longest run of dependent fp32 additions between one
element's square and the tensor's sum in the reduction DESIGN.md section 40 states: a thread's 16 elements one after the other, 6 levels
of the wave butterfly, 3 additions over the 4 wave sums, ceil(tiles / 64) tile sums per lane, 6 levels again.  Whatever compares two runs
of the same kernels (replayed against eager, restored against untouched, one run against its repetition) is bit for bit."""
import copy
import types

import numpy as np
import pytest
import torch

import ema_cases as ec
import lamb_cases as lc
import lr_schedule_cases as sc
from oracle import vited_oracle as vo
from test_gpu_engine import _hip_model

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def chain(shape):
    rows = shape[0] if len(shape) > 1 else 1
    cols = int(np.prod(shape)) // rows
    tiles = ((rows + 63) // 64) * ((cols + 63) // 64)
    return 16 + 6 + 3 + (tiles + 63) // 64 + 6


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


class Bound:
    """FlatLAMB over the bag, bound to a flat buffer and to a Runtime that holds the bf16 shadows of the 2-D and 4-D tensors."""

    def __init__(self, V, dev, override=None, **opt_kw):
        self.ps = [torch.nn.Parameter(t.to(dev)) for t in lc.initial_parameters()]
        self.opt = V.optim.FlatLAMB(lc.param_groups(self.ps, **(override or {})), **lc.HYPER, **opt_kw)
        self.flat = V.engine.FlatGradients(self.ps)
        self.view_of = {id(p): v for p, v in zip(self.flat.params, self.flat.views)}
        self.rt = V.functions.Runtime(img_size=64, patch_size=8, in_chans=3, num_classes=4, embed_dim=384, depth=1, c_depth=1, num_heads=12)
        self.shadow_n = {i: self.rt.weight(p) for i, p in enumerate(self.ps) if p.ndim in (2, 4)}
        self.shadow_t = {i: self.rt.weight_t(p)[0] for i, p in enumerate(self.ps) if p.ndim == 2}
        self.opt.bind_flat(self.flat, types.SimpleNamespace(_runtimes={torch.bfloat16: self.rt}))
        self.key = lc.index_in_groups()

    def set_gradient(self, step):
        for p, g in zip(self.ps, lc.gradients(step)):
            self.view_of[id(p)].copy_(g)

    def shadows_current(self):
        ok = all(torch.equal(sh, self.ps[i].detach().reshape(self.ps[i].shape[0], -1).to(torch.bfloat16)) and self.rt.weight(self.ps[i]) is sh
                 for i, sh in self.shadow_n.items())
        return ok and all(torch.equal(sh, self.ps[i].detach().t().contiguous().to(torch.bfloat16)) for i, sh in self.shadow_t.items())

    def record(self, norm):
        o, r = self.opt, self.opt.trust_ratios()
        return dict(norm=float(norm), p=[p.detach().cpu().clone() for p in self.ps], m=[o.state[p]['exp_avg'].cpu().clone() for p in self.ps],
                    v=[o.state[p]['exp_avg_sq'].cpu().clone() for p in self.ps], r=[r[self.key[i]] for i in range(len(self.ps))],
                    shadows=self.shadows_current(), grad_max=float(self.flat.flat.abs().max()))


_RUNS = {}


def run(V, dev, variant='plain', fresh=False):
    """lc.UPDATES updates of the bag, one record per update; computed once per variant and shared between the tests."""
    kw = {'plain': {}, 'trust_clip': dict(trust_clip=True), 'always_adapt': dict(always_adapt=True)}[variant]
    if fresh or variant not in _RUNS:
        b = Bound(V, dev, **kw)
        records = []
        for step in range(lc.UPDATES):
            b.set_gradient(step)
            records.append(b.record(b.opt.step_flat(lc.MAX_NORM)))
        assert b.opt.num_updates == lc.UPDATES and b.opt.skipped_updates == 0
        if fresh:
            return records
        _RUNS[variant] = records
    return _RUNS[variant]


def check_against(records, ref, what):
    worst = dict(p=0.0, m=0.0, v=0.0, r=0.0)
    for step, (rec, want) in enumerate(zip(records, ref)):
        assert abs(rec['norm'] - want['norm']) <= 1e-5 * want['norm'] + 1e-7
        for i, shape in enumerate(lc.SHAPES):
            lr = lc.group_settings(lc.GROUP_OF[i])['lr']
            where = lambda m, n=None: f'{what} update {step} {n} {shape} ({lc.KINDS[i]}): {m}'
            for name, got, w, tol in (('p', rec['p'][i], want['p'][i], dict(rtol=2e-6, atol=1e-3 * lr)),
                                      ('m', rec['m'][i], want['m'][i], dict(rtol=1e-5, atol=1e-9)),
                                      ('v', rec['v'][i], want['v'][i], dict(rtol=1e-5, atol=1e-12))):
                err = float(((got.double() - w.double()).abs() / (tol['atol'] + tol['rtol'] * w.double().abs())).max())
                worst[name] = max(worst[name], err)
                torch.testing.assert_close(got.double(), w.double(), msg=lambda m, n=name: where(m, n), **tol)
                assert bool(torch.isfinite(got).all())
            r, wr = rec['r'][i], want['r'][i]
            worst['r'] = max(worst['r'], abs(r - wr) / wr / ((chain(shape) + 2) * U))
            assert abs(r - wr) <= (chain(shape) + 2) * U * wr, where(f'r {r!r} against {wr!r}, {abs(r - wr) / wr / U:.1f} x 2^-24 for {chain(shape) + 2}', 'r')
    print(f'{what}: worst error in units of its tolerance {worst}')


# ---- the bag ---------------------------------------------------------------------------------------------------------------------
def test_bag_against_the_fp64_restatement(vited, gpu):
    records = run(vited, gpu)
    check_against(records, lc.run(torch.float64), 'plain')
    kind = {k: lc.KINDS.index(k) for k in ('zero_p', 'zero_g', 'zero_both')}
    wd, zg = lc.HYPER['weight_decay'], kind['zero_g']
    assert records[0]['r'][kind['zero_p']] == 1.0                                      # |p| = 0 in the first update
    for rec in records:
        assert abs(rec['r'][zg] - 1.0 / wd) <= (chain(lc.SHAPES[zg]) + 2) * U / wd     # u = wd p
        assert float(rec['m'][zg].abs().max()) == 0.0 and float(rec['v'][zg].abs().max()) == 0.0
        assert rec['r'][kind['zero_both']] == 1.0 and float(rec['p'][kind['zero_both']].abs().max()) == 0.0        # |u| = 0, nothing non-finite
        assert all(r == 1.0 for r, g in zip(rec['r'], lc.GROUP_OF) if g == 1)          # no decay, not adapted
        assert rec['grad_max'] == 0.0                                                  # zero_grad fused in
    assert records[1]['norm'] > lc.MAX_NORM > records[2]['norm']                       # clipped and unclipped updates


def test_without_decay_it_is_torch_adamw(vited, gpu):
    b = Bound(vited, gpu, override=dict(weight_decay=0.0))
    ref = [torch.nn.Parameter(p.detach().clone()) for p in b.ps]
    topt = torch.optim.AdamW(lc.param_groups(ref, weight_decay=0.0), **{**lc.HYPER, 'weight_decay': 0.0})
    for step in range(lc.UPDATES):
        b.set_gradient(step)
        for q, g in zip(ref, lc.gradients(step)):
            q.grad = g.to(gpu)
        want_norm = torch.nn.utils.clip_grad_norm_(ref, lc.MAX_NORM)
        topt.step()
        norm = b.opt.step_flat(lc.MAX_NORM)
        torch.testing.assert_close(norm, want_norm, rtol=1e-5, atol=1e-7)
        for i, (p, q) in enumerate(zip(b.ps, ref)):
            lr = lc.group_settings(lc.GROUP_OF[i])['lr']
            torch.testing.assert_close(p, q, rtol=2e-6, atol=1e-3 * lr, msg=lambda m: f'update {step} {lc.SHAPES[i]}: {m}')
            torch.testing.assert_close(b.opt.state[p]['exp_avg'], topt.state[q]['exp_avg'], rtol=1e-5, atol=1e-9)
            torch.testing.assert_close(b.opt.state[p]['exp_avg_sq'], topt.state[q]['exp_avg_sq'], rtol=1e-5, atol=1e-12)
        assert set(b.opt.trust_ratios().values()) == {1.0} and b.shadows_current()
    sd, tsd = b.opt.state_dict(), topt.state_dict()
    assert set(sd['state']) == set(tsd['state']) and float(sd['state'][0]['step']) == lc.UPDATES


def test_trust_clip_keeps_every_ratio_at_or_below_one(vited, gpu):
    records, ref, free = run(vited, gpu, 'trust_clip'), lc.run(torch.float64, trust_clip=True), lc.run(torch.float64)
    check_against(records, ref, 'trust_clip')
    assert all(r <= 1.0 for rec in records for r in rec['r'])
    clipped = [(s, i) for s, rec in enumerate(free) for i, r in enumerate(rec['r']) if r > 1.5]
    assert clipped and all(records[s]['r'][i] == 1.0 for s, i in clipped if s == 0)     # the clip did act


def test_always_adapt_reaches_the_undecayed_group(vited, gpu):
    records = run(vited, gpu, 'always_adapt')
    check_against(records, lc.run(torch.float64, always_adapt=True), 'always_adapt')
    assert all(r != 1.0 for rec in records for r, g in zip(rec['r'], lc.GROUP_OF) if g == 1)


def test_both_shadows_follow_every_update(vited, gpu):
    for variant in ('plain', 'always_adapt'):
        assert all(rec['shadows'] for rec in run(vited, gpu, variant)), variant


def test_kept_gradients_keep_their_bits(vited, gpu):
    b = Bound(vited, gpu)
    records = run(vited, gpu)
    for step in range(2):
        b.set_gradient(step)
        before = bits(b.flat.flat)
        b.opt.step_flat(lc.MAX_NORM, zero_grad=False)
        assert np.array_equal(bits(b.flat.flat), before) and before.any()
        assert all(same(p, w) for p, w in zip(b.ps, records[step]['p']))               # and the update is the one that zeroes them


def test_two_runs_give_the_same_bits(vited, gpu):
    first, second = run(vited, gpu), run(vited, gpu, fresh=True)
    for a, b in zip(first, second):
        assert all(same(x, y) for what in ('p', 'm', 'v') for x, y in zip(a[what], b[what]))
        assert np.array_equal(np.float32(a['r']).view(np.int32), np.float32(b['r']).view(np.int32)) and a['norm'] == b['norm']


# ---- the smallest oracle geometry ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def shape():
    return vo.ViTEDShape(depth=1, c_depth=1)


@pytest.fixture(scope='module')
def init(vited, gpu, shape):
    torch.manual_seed(17)
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


def _step(V, dev, shape, init, scheduled=False, cls=None, lr=1e-3, **kw):
    m = _hip_model(V, shape, dev, None)
    m.load_state_dict(init)
    opt_kw = {k: kw.pop(k) for k in ('ema_decay', 'ema_warmup', 'skip_nonfinite') if k in kw}
    opt = (cls or V.optim.FlatLAMB)(V.engine.param_groups_no_decay_1d(m), lr=sc.BASE_LR if scheduled else lr, weight_decay=0.05, model=m, **opt_kw)
    if scheduled:
        case = sc.BY_ID['cosine_prefix_warm0']
        kw['lr_scheduler'] = V.engine.build_scheduler(sc.config(case), opt, sc.N_ITER, step_warmup_prefix=case['step_warmup_prefix'])
    return m, opt, V.engine.TrainStep(m, opt, clip_grad=5.0, amp=True, **kw)


def _state_bits(opt):
    return [bits(opt._bufs[n]) for n in opt._state_names] + [bits(opt._ws[1028: 1028 + len(opt.flat.params)]), bits(opt._hyper)]


def test_replayed_step_equals_the_eager_one(vited, gpu, shape, init):
    runs = [_step(vited, gpu, shape, init, scheduled=True, use_graph=ug, accumulation_steps=2) for ug in (False, True)]
    for x, y in _batches(8, gpu):
        le, lg = [st.step(x, y) for _, _, st in runs]
        assert same(le.reshape(1), lg.reshape(1))
    (me, oe, se), (mg, og, sg) = runs
    assert se._g1 is None and sg._g_opt is not None and sg.recaptures == 0 and se.lr_on_device and sg.lr_on_device
    assert oe.num_updates == og.num_updates == 4 and same(se.last_norm.reshape(1), sg.last_norm.reshape(1))
    for (name, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
        assert same(pe, pg), name
    assert not same(mg.head.weight, init['head.weight'])
    assert all(np.array_equal(a, b) for a, b in zip(_state_bits(oe), _state_bits(og)))
    ratios = og.trust_ratios()
    assert set(ratios) == {n for n, _ in mg.named_parameters()}                        # keyed by the model's names
    assert all(ratios[n] == 1.0 for n, p in mg.named_parameters() if p.ndim == 1) and ratios['head.weight'] not in (0.0, 1.0)


def test_a_nan_batch_is_skipped_and_leaves_everything_alone(vited, gpu, shape, init):
    m, opt, step = _step(vited, gpu, shape, init, skip_nonfinite=True)
    for it, (x, y) in enumerate(_batches(4, gpu, nan_at=2)):
        before = ([bits(p) for p in m.parameters()], _state_bits(opt), opt.num_updates)
        step.step(x, y)
        after = ([bits(p) for p in m.parameters()], _state_bits(opt), opt.num_updates)
        assert float(opt.flat.flat.abs().max()) == 0.0                                 # the gradients are zeroed either way
        if it == 2:
            assert not torch.isfinite(step.last_norm)
            assert all(np.array_equal(a, b) for a, b in zip(before[0] + before[1][:3], after[0] + after[1][:3])) and before[2] == after[2]
            assert opt.skipped_updates == 1
        else:
            assert any(not np.array_equal(a, b) for a, b in zip(before[0], after[0])) and after[2] == before[2] + 1
    assert opt.num_updates == 3 and all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_the_average_follows_the_lamb_updated_parameters(vited, gpu, shape, init):
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
    for (name, p), (_, q) in zip(m.named_parameters(), plain[0].named_parameters()):   # keeping the average changes nothing else
        assert same(p, q), name
    # the exchange for an evaluation, and back
    before = ([bits(p) for p in params], bits(opt.ema), _state_bits(opt))
    with opt.swap_ema():
        assert all(np.array_equal(bits(opt.ema_of(p)), w) for p, w in zip(params, before[0])) and not np.array_equal(bits(opt.ema), before[1])
    after = ([bits(p) for p in params], bits(opt.ema), _state_bits(opt))
    assert all(np.array_equal(a, b) for a, b in zip(before[0] + [before[1]] + before[2], after[0] + [after[1]] + after[2]))
    averaged = opt.ema_state_dict(m)
    assert list(averaged) == list(m.state_dict()) and not same(averaged['head.weight'], m.head.weight)


def test_find_lr_sweeps_and_restores_bit_for_bit(vited, gpu, shape, init):
    m, opt, step = _step(vited, gpu, shape, init)
    for x, y in _batches(2, gpu):
        step.step(x, y)
    before = ([bits(p) for p in m.parameters()], _state_bits(opt), [g['lr'] for g in opt.param_groups])
    result = vited.engine.find_lr(step, _batches(3, gpu, seed=3), num_iter=3, start_lr=1e-5, end_lr=1e-2, restore=True)
    assert result.iterations == 3
    after = ([bits(p) for p in m.parameters()], _state_bits(opt), [g['lr'] for g in opt.param_groups])
    assert all(np.array_equal(a, b) for a, b in zip(before[0] + before[1], after[0] + after[1])) and before[2] == after[2]      # ratios included
    assert opt.num_updates == 2
    kept = vited.engine.find_lr(step, _batches(3, gpu, seed=3), num_iter=3, start_lr=1e-5, end_lr=1e-2, restore=False)
    assert kept.iterations == 3 and opt.num_updates == 5 and any(not np.array_equal(bits(p), w) for p, w in zip(m.parameters(), before[0]))             # the sweep does move them


def test_state_dict_moves_to_flat_adamw_and_back(vited, gpu, shape, init):
    ma, oa, sa = _step(vited, gpu, shape, init)
    for x, y in _batches(2, gpu):
        sa.step(x, y)
    saved = copy.deepcopy(oa.state_dict())
    mb, ob, sb = _step(vited, gpu, shape, init, cls=vited.optim.FlatAdamW)
    ob.load_state_dict(copy.deepcopy(saved))
    assert ob.num_updates == 2
    through = copy.deepcopy(ob.state_dict())
    mc, oc, stc = _step(vited, gpu, shape, init)
    mc.load_state_dict(ma.state_dict())
    oc.load_state_dict(through)
    final = oc.state_dict()
    assert final['param_groups'] == saved['param_groups'] and set(final['state']) == set(saved['state'])
    for k, st in saved['state'].items():
        assert float(final['state'][k]['step']) == float(st['step']) == 2.0
        assert same(final['state'][k]['exp_avg'], st['exp_avg']) and same(final['state'][k]['exp_avg_sq'], st['exp_avg_sq'])
    x, y = _batches(3, gpu)[2]                                                          # and the resumed run continues as the original
    assert same(sa.step(x, y).reshape(1), stc.step(x, y).reshape(1))
    for (name, p), (_, q) in zip(ma.named_parameters(), mc.named_parameters()):
        assert same(p, q), name


@pytest.mark.parametrize('name', ['lamb', 'fused_lamb'])
def test_build_optimizer_gives_flat_lamb_on_a_gpu_model(vited, gpu, shape, name):
    m = _hip_model(vited, shape, gpu, None)
    o = types.SimpleNamespace(NAME=name, EPS=1e-6, BETAS=(0.9, 0.99), MOMENTUM=0.9)
    cfg = types.SimpleNamespace(TRAIN=types.SimpleNamespace(OPTIMIZER=o, BASE_LR=2e-3, WEIGHT_DECAY=0.05))
    opt = vited.engine.build_optimizer(cfg, m, skip_nonfinite=True, ema_decay=0.99)
    assert type(opt) is vited.optim.FlatLAMB and opt.skip_nonfinite and opt.ema_decay == 0.99
    assert [g['weight_decay'] for g in opt.param_groups] == [0.05, 0.0]
    assert all(p.ndim == 1 for p in opt.param_groups[1]['params']) and all(p.ndim > 1 for p in opt.param_groups[0]['params'])
    assert opt.defaults['lr'] == 2e-3 and opt.defaults['betas'] == (0.9, 0.99) and opt.defaults['eps'] == 1e-6
    assert not opt.defaults['always_adapt'] and not opt.defaults['trust_clip']
    with pytest.raises(ValueError, match='unknown optimizer'):
        vited.engine.build_optimizer(cfg, m, fused_hip=False)
