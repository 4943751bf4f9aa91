"""Muon in the fused update on the MI355X (vited_muon_step / vited_muon_step_ema, optim.FlatMuon).

Criteria.  (1) On exact-arithmetic operands (muon_cases.exact_u: every dot product has at most one non-zero term) O equals the rule
restated in the kernel's arithmetic bit for bit.  (2) On general operands e_hip = |O_hip - O_64|_F / |O_64|_F, O_64 the fp64 iteration
from the same u, must not exceed 2 e_torch, e_torch the same error of torch.optim.Muon's own bf16 iteration on the CPU: the kernel
differs from torch by one rounding at the normalisation instead of two and by the order of the fp32 sums, neither of which can move a
result by more than the bf16 roundings themselves do.  (3) Over five updates of the bag momentum_buffer agrees with torch.optim.Muon on
the CPU to rtol 1e-6 (atol 1e-9: the buffer's elements stay below 1e-2, where an fp32 ulp is 9e-10, and a lerp that cancels leaves an
ulp of its larger operand), every Muon tensor's step is held by criterion (2), and the aux tensors carry FlatAdamW's bits.  Whatever
compares two runs of the same kernels is bit for bit.

What pins O.  The bag's gradients (lamb_cases.gradients) are closed forms of rank 6 or so, on which the iteration is no contraction: both
e_hip and e_torch are 0.2 - 0.8 of the step there, so criterion (2) on the bag is the check the issue sets but a weak one - it shows
that the kernel is no worse than torch's bf16 iteration on ill-conditioned operands, and that a zero u gives O = 0, not that O is
right.  O itself is pinned by the exact-arithmetic tests and by the general-value test, whose operands (muon_cases.general_u) carry a
full-rank term and give e_torch of 1.3e-2 .. 1.7e-2; the bag then holds momentum_buffer, the apply pass, the aux tensors and the
family's behaviour around them."""
import copy
import types

import numpy as np
import pytest
import torch

import ema_cases as ec
import lamb_cases as lc
import lr_schedule_cases as sc
import muon_cases as mc
from oracle import vited_oracle as vo
from test_gpu_engine import _hip_model

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- 1, 2: one update from a given u ---------------------------------------------------------------------------------------------------
AUX_BETWEEN = [(5,), (1, 5, 8), (8, 3, 2, 2)]          # 1-D, 3-D and 4-D aux tensors between the Muon tensors in the flat buffer


def orthogonalize(V, dev, us, aux_between=False):
    """One FlatMuon update with momentum 0 (so u = g exactly), p = 0, lr = 1 and no decay on Muon tensors whose gradients are ``us``:
    [(O as the scratch holds it, the new p)] per tensor."""
    ws = [torch.nn.Parameter(torch.zeros(u.shape, device=dev)) for u in us]
    aux = [torch.nn.Parameter(torch.full(s, 0.25, device=dev)) for s in (AUX_BETWEEN if aux_between else [])]
    order = []
    for k, w in enumerate(ws):                          # w0 a0 w1 a1 w2 a2 w3 w4
        order.append(w)
        if k < len(aux):
            order.append(aux[k])
    groups = [{'params': ws, 'use_muon': True}] + ([{'params': aux}] if aux else [])
    opt = V.optim.FlatMuon(groups, lr=1.0, momentum=0.0, nesterov=True, weight_decay=0.0)
    flat = V.engine.FlatGradients(order)
    view_of = {id(p): v for p, v in zip(flat.params, flat.views)}
    opt.bind_flat(flat)
    for w, u in zip(ws, us):
        view_of[id(w)].copy_(u.to(dev))
    for a in aux:
        view_of[id(a)].fill_(0.5)
    opt.step_flat(None)
    assert float(flat.flat.abs().max()) == 0.0 and opt.num_updates == 1
    assert all(bool((a != 0.25).all()) and bool(torch.isfinite(a).all()) for a in aux)      # the aux tensors moved, by AdamW
    return [(opt.orthogonalized(w).cpu(), w.detach().cpu().clone()) for w in ws]


def _check_exact(got, us):
    for (o, p), u in zip(got, us):
        want = mc.newton_schulz_kernel(u)
        off = int((bits(o) != bits(want)).sum())
        assert off == 0, f'{tuple(u.shape)}: {off} elements of O differ in their bits'
        adj = torch.tensor(mc.adjust(u.shape[0], u.shape[1], None), dtype=torch.float32)
        torch.testing.assert_close(p, -adj * want.float(), rtol=1e-6, atol=0.0)            # p = 0 - lr adj O


@pytest.mark.parametrize('shape', mc.EXACT_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_exact_arithmetic_bit_for_bit_each_alone(vited, gpu, shape):
    us = [mc.exact_u(*shape)]
    _check_exact(orthogonalize(vited, gpu, us), us)


def test_exact_arithmetic_bit_for_bit_all_in_one_optimizer(vited, gpu):
    us = [mc.exact_u(*s) for s in mc.EXACT_SHAPES]
    got = orthogonalize(vited, gpu, us, aux_between=True)
    _check_exact(got, us)
    o = got[mc.EXACT_SHAPES.index((64, 96))][0].float()
    assert int((o != 0).sum()) == 64 and set(o.abs()[o != 0].tolist()) == {0.69140625}


def test_general_values_against_the_fp64_iteration(vited, gpu):
    us = [mc.general_u(*s) for s in mc.GENERAL_SHAPES]
    for (o, _), u in zip(orthogonalize(vited, gpu, us), us):
        e_hip, e_torch = mc.relative_error(o, mc.newton_schulz(u)), mc.torch_bf16_error(u)
        print(f'{tuple(u.shape)}: e_hip {e_hip:.3e} e_torch {e_torch:.3e} ratio {e_hip / e_torch:.2f}')
        assert e_hip <= 2 * e_torch, (tuple(u.shape), e_hip, e_torch)


# ---- 3, 4: the bag ---------------------------------------------------------------------------------------------------------------------
class Bound:
    """A fused optimizer over the bag, bound to a flat buffer and to a Runtime that holds the bf16 shadows of the 2-D and 4-D tensors."""

    def __init__(self, V, dev, cls=None, muon_override=None, **opt_kw):
        self.ps = [torch.nn.Parameter(t.to(dev)) for t in lc.initial_parameters()]
        if cls is None:
            self.opt = V.optim.FlatMuon(mc.param_groups(self.ps, **(muon_override or {})), **mc.HYPER, **opt_kw)
        else:       # FlatAdamW with the aux groups' settings on every tensor
            self.opt = cls(lc.param_groups(self.ps), lr=mc.HYPER['lr'], betas=mc.HYPER['betas'], eps=mc.HYPER['adam_eps'],
                           weight_decay=mc.HYPER['weight_decay'], **opt_kw)
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

    def state_of(self, i):
        return {k: v.detach().cpu().clone() for k, v in self.opt.state[self.ps[i]].items()}

    def record(self, norm):
        return dict(norm=norm.detach().cpu().clone().reshape(1), p=[p.detach().cpu().clone() for p in self.ps],
                    state=[self.state_of(i) for i in range(len(self.ps))], shadows=self.shadows_current(),
                    grad_max=float(self.flat.flat.abs().max()),
                    o=[self.opt.orthogonalized(p).cpu() if mu and hasattr(self.opt, 'orthogonalized') else None
                       for p, mu in zip(self.ps, mc.IS_MUON)])


VARIANTS = {'nesterov': dict(), 'plain_momentum': dict(nesterov=False), 'match_rms': dict(adjust_lr_fn='match_rms_adamw'),
            'plain_match_rms': dict(nesterov=False, adjust_lr_fn='match_rms_adamw')}
_RUNS = {}


def run(V, dev, variant='nesterov', fresh=False, **opt_kw):
    """lc.UPDATES updates of the bag, one record per update (each with the parameters before it); computed once per variant."""
    if fresh or variant not in _RUNS:
        b = Bound(V, dev, cls=V.optim.FlatAdamW if variant == 'adamw' else None, muon_override=VARIANTS.get(variant), **opt_kw)
        if variant != 'adamw':
            assert all(set(b.opt.state[p]) == ({'momentum_buffer'} if mu else {'exp_avg', 'exp_avg_sq'}) for p, mu in zip(b.ps, mc.IS_MUON))
        records = []
        for step in range(lc.UPDATES):
            before = [p.detach().cpu().clone() for p in b.ps]
            b.set_gradient(step)
            records.append(dict(b.record(b.opt.step_flat(lc.MAX_NORM)), p_before=before))
        assert b.opt.num_updates == lc.UPDATES and b.opt.skipped_updates == 0
        if fresh:
            return records
        _RUNS[variant] = records
    return _RUNS[variant]


def torch_reference(nesterov, adjust_lr_fn):
    """torch.optim.Muon on the bag's Muon tensors + torch.optim.AdamW on the others, fp32 on the CPU, the clip over all gradients."""
    ps = [torch.nn.Parameter(t.clone()) for t in lc.initial_parameters()]
    muon = torch.optim.Muon([p for p, mu in zip(ps, mc.IS_MUON) if mu], lr=mc.HYPER['lr'], momentum=mc.HYPER['momentum'], nesterov=nesterov,
                            weight_decay=mc.HYPER['weight_decay'], adjust_lr_fn=adjust_lr_fn, ns_coefficients=mc.NS_COEFFICIENTS,
                            ns_steps=mc.NS_STEPS, eps=mc.EPS)
    adamw = torch.optim.AdamW([{'params': [p for p, g in zip(ps, lc.GROUP_OF) if g == gi], **mc.AUX_GROUPS[gi - 1]} for gi in (1, 2)],
                              lr=mc.HYPER['lr'], betas=mc.HYPER['betas'], eps=mc.HYPER['adam_eps'], weight_decay=mc.HYPER['weight_decay'])
    out = []
    for step in range(lc.UPDATES):
        before = [p.detach().clone() for p in ps]
        for p, g in zip(ps, lc.gradients(step)):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(ps, lc.MAX_NORM)
        muon.step()
        adamw.step()
        out.append(dict(p_before=before, p=[p.detach().clone() for p in ps],
                        buf=[muon.state[p]['momentum_buffer'].clone() if mu else None for p, mu in zip(ps, mc.IS_MUON)]))
    return out


def _step_error(p_before, p, o64, lr, wd, adj):
    """(|step - step_64|_F, |step_64|_F) of one tensor in one update: step = p_new - p_old (1 - lr wd), step_64 = -lr adj O_64."""
    step = p.double() - p_before.double() * (1 - lr * wd)
    want = -lr * adj * o64
    return float((step - want).norm()), float(want.norm())


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_five_updates_of_the_bag_against_torch_on_the_cpu(vited, gpu, variant):
    nesterov, adjust_lr_fn = VARIANTS[variant].get('nesterov', True), VARIANTS[variant].get('adjust_lr_fn')
    records, ref, f64 = run(vited, gpu, variant), torch_reference(nesterov, adjust_lr_fn), mc.run_muon_tensors(torch.float64, nesterov, adjust_lr_fn)
    muon_at = [i for i, mu in enumerate(mc.IS_MUON) if mu]
    lr, wd = mc.HYPER['lr'], mc.HYPER['weight_decay']
    for step, (rec, r, w) in enumerate(zip(records, ref, f64)):
        assert abs(float(rec['norm']) - w['norm']) <= 1e-5 * w['norm'] + 1e-7
        assert rec['shadows'] and rec['grad_max'] == 0.0, step                             # both shadows are bf16(p); zero_grad fused in
        for k, i in enumerate(muon_at):
            shape = lc.SHAPES[i]
            torch.testing.assert_close(rec['state'][i]['momentum_buffer'], r['buf'][i], rtol=1e-6, atol=1e-9,
                                       msg=lambda m: f'update {step} momentum_buffer {shape}: {m}')
            assert bool(torch.isfinite(rec['p'][i]).all()) and bool(torch.isfinite(rec['o'][i].float()).all()), (step, shape)
            adj = mc.adjust(shape[0], shape[1], adjust_lr_fn)
            d_hip, n64 = _step_error(rec['p_before'][i], rec['p'][i], w['o'][k], lr, wd, adj)
            d_torch, _ = _step_error(r['p_before'][i], r['p'][i], w['o'][k], lr, wd, adj)
            if n64 == 0.0:                          # u = 0: O = 0, the parameter only decays: at |p| < 0.125 half an ulp of the product, 2^-27, and as much from the rounded 1 - lr wd
                assert not bits(rec['o'][i]).any() and d_hip <= 2.0 ** -26 * rec['p'][i].numel() ** 0.5, (step, shape, d_hip)
                continue
            print(f'{variant} update {step} {shape}: e_hip {d_hip / n64:.3e} e_torch {d_torch / n64:.3e} ratio {d_hip / d_torch:.2f}')
            assert d_hip <= 2 * d_torch, (step, shape, d_hip / n64, d_torch / n64)
        for i, mu in enumerate(mc.IS_MUON):
            if not mu:                              # against torch.optim.AdamW at the bounds tools/lamb_host_check.cpp holds p to
                torch.testing.assert_close(rec['p'][i], r['p'][i], rtol=1e-5, atol=2e-6, msg=lambda m: f'update {step} aux {lc.SHAPES[i]}: {m}')
    assert float(records[1]['norm']) > lc.MAX_NORM > float(records[2]['norm']) and float(records[3]['norm']) > lc.MAX_NORM


def test_aux_tensors_carry_flat_adamws_bits(vited, gpu):
    records, adamw = run(vited, gpu), run(vited, gpu, 'adamw')
    checked = 0
    for step, (rec, a) in enumerate(zip(records, adamw)):
        assert same(rec['norm'], a['norm'])
        for i, mu in enumerate(mc.IS_MUON):
            if not mu:
                assert same(rec['p'][i], a['p'][i]), (step, lc.SHAPES[i])
                assert all(same(rec['state'][i][n], a['state'][i][n]) for n in ('exp_avg', 'exp_avg_sq')), (step, lc.SHAPES[i])
                checked += 1
    assert checked == lc.UPDATES * (len(lc.BAG) - sum(mc.IS_MUON)) and checked > 0


def _all_bits(rec):
    return [bits(t) for t in rec['p']] + [bits(v) for st in rec['state'] for _, v in sorted(st.items())] + [bits(o) for o in rec['o'] if o is not None]


def test_two_runs_give_the_same_bits(vited, gpu):
    first, second = run(vited, gpu), run(vited, gpu, fresh=True)
    for a, b in zip(first, second):
        assert same(a['norm'], b['norm']) and all(np.array_equal(x, y) for x, y in zip(_all_bits(a), _all_bits(b)))


def test_kept_gradients_keep_their_bits(vited, gpu):
    b = Bound(vited, gpu)
    records = run(vited, gpu)
    for step in range(2):
        b.set_gradient(step)
        before = bits(b.flat.flat)
        b.opt.step_flat(lc.MAX_NORM, zero_grad=False)
        assert np.array_equal(bits(b.flat.flat), before) and before.any()
        assert all(same(p, w) for p, w in zip(b.ps, records[step]['p']))               # and the update is the one that zeroes them


def test_an_inf_gradient_is_skipped_and_leaves_every_buffer_alone(vited, gpu):
    b = Bound(vited, gpu, skip_nonfinite=True, ema_decay=0.9)
    b.set_gradient(0)
    b.opt.step_flat(lc.MAX_NORM)

    def snapshot():
        return [bits(p) for p in b.ps] + [bits(t) for t in b.opt._bufs.values()] + [bits(b.opt.ema), bits(b.opt._ws[1028:])] + \
               [bits(s) for s in list(b.shadow_n.values()) + list(b.shadow_t.values())]

    for zero_grad in (True, False):
        b.set_gradient(1)
        b.view_of[id(b.ps[1])][3, 5] = float('inf')                                     # in a Muon tensor
        before, g_before = snapshot(), bits(b.flat.flat)
        norm = b.opt.step_flat(lc.MAX_NORM, zero_grad=zero_grad)
        assert not bool(torch.isfinite(norm)) and all(np.array_equal(x, y) for x, y in zip(before, snapshot()))
        assert (float(b.flat.flat.abs().max()) == 0.0) if zero_grad else np.array_equal(bits(b.flat.flat), g_before)
    assert (b.opt.num_updates, b.opt.num_ema_updates, b.opt.skipped_updates) == (1, 1, 2)
    b.set_gradient(2)                                                                   # and the next finite one is applied
    before = snapshot()
    b.opt.step_flat(lc.MAX_NORM)
    assert b.opt.num_updates == 2 and all(bool(torch.isfinite(p).all()) for p in b.ps)
    assert sum(not np.array_equal(x, y) for x, y in zip(before, snapshot())) >= len(b.ps) - 2


def test_the_average_follows_the_updated_parameters_and_swaps(vited, gpu):
    b, plain = Bound(vited, gpu, ema_decay=0.5, ema_warmup=True), run(vited, gpu)
    assert all(same(b.opt.ema_of(p), p) for p in b.ps)
    for n in range(3):
        e_before = [bits(b.opt.ema_of(p)).view(np.float32) for p in b.ps]
        b.set_gradient(n)
        b.opt.step_flat(lc.MAX_NORM)
        for e, p in zip(e_before, b.ps):
            want = ec.update(e, bits(p).view(np.float32), 0.5, True, n)[0]              # e = d e + (1 - d) p on the device's own new p
            assert np.array_equal(bits(b.opt.ema_of(p)), want.view(np.int32))
        assert all(same(p, w) for p, w in zip(b.ps, plain[n]['p'])) and b.shadows_current()      # keeping the average changes nothing else
    assert b.opt.num_ema_updates == 3
    before = ([bits(p) for p in b.ps], bits(b.opt.ema), [bits(t) for t in b.opt._bufs.values()])
    with b.opt.swap_ema():
        assert all(np.array_equal(bits(b.opt.ema_of(p)), w) for p, w in zip(b.ps, before[0])) and not np.array_equal(bits(b.opt.ema), before[1])
        assert b.shadows_current()                                                       # the shadows follow the averaged weights
    after = ([bits(p) for p in b.ps], bits(b.opt.ema), [bits(t) for t in b.opt._bufs.values()])
    assert all(np.array_equal(x, y) for x, y in zip(before[0] + [before[1]] + before[2], after[0] + [after[1]] + after[2]))
    assert b.shadows_current()


def test_refusals_of_the_entry(vited, gpu):
    b = Bound(vited, gpu)
    b.set_gradient(0)
    lib, o = vited._lib.load(), b.opt
    desc = o._descriptors()
    head = (desc.data_ptr(), desc.shape[0], o._tiles, b.flat.flat.data_ptr(), b.flat.flat.numel(), o._hyper.data_ptr(), 0.0, 0, None,
            o._ws.data_ptr(), o._ws.numel() * 4, None)
    extras = list(o._entry_extras())
    call = lambda over, h=head: lib.vited_muon_step(*h, *[over.get(i, v) for i, v in enumerate(extras)])
    before = [bits(p) for p in b.ps] + [bits(b.flat.flat)]
    assert call({8: 0}) == 1 and call({8: 17}) == 1                                   # ns_steps
    assert call({1: extras[1] + 1}) == 1 and call({0: extras[0] + 4}) == 1              # a tile count off; a misaligned table
    meta = o._mu['meta'].clone()
    meta[lc.SHAPES.index((65, 67)), 2] = 3                                                  # a Muon tensor that is not 2-D
    assert call({5: meta.data_ptr()}) == 1
    meta = o._mu['meta'].clone()
    meta[lc.SHAPES.index((65, 67)), :2] = torch.tensor([1088, 2048])                        # a short side above 1024
    assert call({5: meta.data_ptr()}) == 2
    kinds = o._mu['kinds'].clone()
    assert kinds.tolist() == [1, 0, 0]
    kinds[0], kinds[1] = 0, 1                                                               # group kinds that contradict the tensor table
    assert call({6: kinds.data_ptr()}) == 1 and call({7: 1}) == 1 and call({6: None}) == 1
    meta = o._mu['meta'].clone()
    meta[0, 4] = 2                                                                          # a Muon tensor filed under an aux group
    assert call({5: meta.data_ptr()}) == 1
    assert call({}, head[:10] + (o._ws.numel() * 4 - 2, None)) == 4                            # a workspace too small
    torch.cuda.synchronize()
    assert all(np.array_equal(x, y) for x, y in zip(before, [bits(p) for p in b.ps] + [bits(b.flat.flat)]))      # refused before any launch


# ---- 5: under the steps -------------------------------------------------------------------------------------------------------------------
N, LABELS = 6, ([0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 2, 2])


@pytest.fixture(scope='module')
def init(vited, gpu):
    torch.manual_seed(19)
    return _hip_model(vited, vo.SHAPE_T, gpu, None).state_dict()


def _batches(n, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(2, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(dev), (torch.rand(2, 1, generator=g) > 0.6).float().to(dev)) for _ in range(n)]


def _config(lr):
    o = types.SimpleNamespace(NAME='muon', EPS=1e-6, BETAS=(0.9, 0.98), MOMENTUM=0.9)
    return types.SimpleNamespace(TRAIN=types.SimpleNamespace(OPTIMIZER=o, BASE_LR=lr, WEIGHT_DECAY=0.05))


def _step(V, dev, init, case=None, on_device=None, two_stage=False, load=None, **kw):
    """``load``: (model state, optimizer state) loaded BEFORE the step binds the optimizer (the reference's resume order)."""
    m = _hip_model(V, vo.SHAPE_T, dev, None)
    m.load_state_dict(init if load is None else load[0])
    opt = V.engine.build_optimizer(_config(sc.BASE_LR if case else 1e-3), m)
    if load is not None:
        opt.load_state_dict(load[1])
        assert opt.flat is None
    if case:
        kw['lr_scheduler'] = V.engine.build_scheduler(sc.config(case), opt, sc.N_ITER, step_warmup_prefix=case['step_warmup_prefix'])
        if on_device is not None:
            kw['lr_scheduler'].on_device = on_device
    cls = V.engine.TwoStageTrainStep if two_stage else V.engine.TrainStep
    extra = dict(capacity=V.engine.mined_pair_capacity(N) + 1) if two_stage else {}
    return m, opt, cls(m, opt, clip_grad=5.0, amp=True, **extra, **kw)


def _state_bits(opt):
    return [bits(opt._bufs[n]) for n in opt._state_names] + [bits(opt._hyper)]


def _same_models(a, b):
    for (name, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert same(p, q), name


def test_build_optimizer_gives_the_three_groups(vited, gpu):
    m = _hip_model(vited, vo.SHAPE_T, gpu, None)
    for name in ('muon', 'Muon'):
        cfg = _config(2e-4)
        cfg.TRAIN.OPTIMIZER.NAME = name
        opt = vited.engine.build_optimizer(cfg, m, skip_nonfinite=True, ema_decay=0.99)
        assert type(opt) is vited.optim.FlatMuon and opt.skip_nonfinite and opt.ema_decay == 0.99
        names = {id(p): n for n, p in m.named_parameters()}
        g_muon, g_decay, g_none = opt.param_groups
        assert [g['use_muon'] for g in opt.param_groups] == [True, False, False] and [g['weight_decay'] for g in opt.param_groups] == [0.05, 0.05, 0.0]
        assert g_muon['params'] and all(p.ndim == 2 and names[id(p)].startswith(('blocks.', 'cross_blocks.')) for p in g_muon['params'])
        assert {names[id(p)] for p in g_decay['params']} == {'head.weight', 'patch_embed.proj.weight', 'pos_embed', 'cls_token'}
        assert all(p.ndim == 1 or names[id(p)].endswith('.bias') for p in g_none['params'])
        assert sum(len(g['params']) for g in opt.param_groups) == len(list(m.parameters()))
        assert (g_muon['lr'], g_muon['momentum'], g_muon['nesterov'], g_muon['adjust_lr_fn']) == (2e-4, 0.95, True, 'match_rms_adamw')
        assert g_decay['betas'] == (0.9, 0.98) and g_decay['adam_eps'] == 1e-6 and opt.ns_steps == 5
    with pytest.raises(ValueError, match='unknown optimizer muon .*HIP optimizer only'):
        vited.engine.build_optimizer(_config(2e-4), m, fused_hip=False)


def test_replayed_step_equals_the_eager_one(vited, gpu, init):
    runs = [_step(vited, gpu, init, use_graph=ug) for ug in (False, True)]
    for x, y in _batches(3 + 3, gpu):                                                  # two eager steps and the capture, then 3 replays
        le, lg = [st.step(x, y) for _, _, st in runs]
        assert same(le.reshape(1), lg.reshape(1))
        assert same(runs[0][2].last_norm.reshape(1), runs[1][2].last_norm.reshape(1))
    (me, oe, se), (mg, og, sg) = runs
    assert se._g1 is None and sg._g_opt is not None and sg.recaptures == 0 and oe.num_updates == og.num_updates == 6
    _same_models(me, mg)
    w = next(p for n, p in mg.named_parameters() if n == 'blocks.0.attn.proj.weight')
    assert not same(w, init['blocks.0.attn.proj.weight']) and not same(mg.head.weight, init['head.weight'])
    assert all(np.array_equal(a, b) for a, b in zip(_state_bits(oe), _state_bits(og)))
    assert set(og.state[w]) == {'momentum_buffer'} and set(og.state[mg.head.weight]) == {'exp_avg', 'exp_avg_sq'}


def test_device_stepped_cosine_schedule_reaches_the_muon_groups_rate_word(vited, gpu, init):
    """cosine_prefix_warm2, stepped on the device, eager and replayed: after update n the rate word of every group - word 0 of the Muon
    group among them - holds the schedule's value at n (lr_schedule_cases.fp32_matches: exactly in the warm-up, else that fp32 value or
    a neighbour, the device's fp64 cos being a few ulp off libm's), the kind words stay, and the two runs agree in every bit."""
    case = sc.BY_ID['cosine_prefix_warm2']
    runs = [_step(vited, gpu, init, case=case, use_graph=ug) for ug in (False, True)]
    assert all(r[2].lr_on_device for r in runs)
    muon_word = []
    for n, (x, y) in enumerate(_batches(14, gpu)):                                     # 10 warm-up updates, then four on the cosine
        le, lg = [st.step(x, y) for _, _, st in runs]
        assert same(le.reshape(1), lg.reshape(1)), n
        for _, opt, _ in runs:
            words = opt._hyper[8:].reshape(3, 8).tolist()
            assert [w[6] for w in words] == [1.0, 0.0, 0.0], n                          # the kinds stayed
            for g, w in enumerate(words):
                assert sc.fp32_matches(w[0], sc.value(case, n), sc.exact_branch(case, n)), (n, g, w[0], sc.value(case, n))
        muon_word.append(runs[1][1]._hyper[8].item())
    assert len(set(muon_word)) == 14 and not sc.exact_branch(case, 13)                  # it moved in every update, the cosine branch included
    assert all(r[1].hyper_uploads == 1 for r in runs) and runs[1][2].recaptures == 0 and runs[1][2]._g_opt is not None
    _same_models(runs[0][0], runs[1][0])
    assert all(np.array_equal(a, b) for a, b in zip(_state_bits(runs[0][1]), _state_bits(runs[1][1])))


def test_device_stepped_linear_schedule_equals_the_host_stepped_one(vited, gpu, init):
    """linear_warm2 beside the cosine case above: + - * / alone, which fp64 rounds alike on the host and the device, so a host-stepped
    run sees the same fp32 rates and must agree in every bit."""
    case = sc.BY_ID['linear_warm2']
    runs = [_step(vited, gpu, init, case=case, on_device=od, use_graph=ug) for od, ug in ((None, True), (False, False))]
    assert [r[2].lr_on_device for r in runs] == [True, False]
    rates = [[], []]
    for x, y in _batches(12, gpu):
        ld, lh = [st.step(x, y) for _, _, st in runs]
        assert same(ld.reshape(1), lh.reshape(1))
        for r, seen in zip(runs, rates):
            seen.append(r[1]._hyper[8::8].tolist())
    assert rates[0][:-1] == rates[1][1:] and len({r[0] for r in rates[0]}) >= 10           # word 0 of the Muon group follows the schedule
    assert runs[0][1].hyper_uploads == 1 and runs[1][1].hyper_uploads > 1 and runs[0][2].recaptures == 0
    assert runs[0][1]._hyper[8 + 6].item() == 1.0 and runs[0][1]._hyper[16 + 6].item() == 0.0      # the kinds stayed
    _same_models(runs[0][0], runs[1][0])


def test_one_two_stage_update_runs(vited, gpu, init):
    m, opt, step = _step(vited, gpu, init, two_stage=True, use_graph=False)
    g = torch.Generator().manual_seed(17)
    step.mine_keys = torch.rand(N * N, generator=g).to(gpu)
    loss = step.step(torch.randn(N, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu), torch.tensor(LABELS[0], device=gpu))
    assert bool(torch.isfinite(loss)) and opt.num_updates == 1 and all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert not same(dict(m.named_parameters())['blocks.0.attn.proj.weight'], init['blocks.0.attn.proj.weight'])


def test_find_lr_accepts_it_and_restores_bit_for_bit(vited, gpu, init):
    m, opt, step = _step(vited, gpu, init)
    for x, y in _batches(2, gpu):
        step.step(x, y)
    before = ([bits(p) for p in m.parameters()], _state_bits(opt), [g['lr'] for g in opt.param_groups])
    result = vited.engine.find_lr(step, _batches(3, gpu, seed=3), num_iter=3, start_lr=1e-6, end_lr=1e-3, restore=True)
    assert result.iterations == 3
    after = ([bits(p) for p in m.parameters()], _state_bits(opt), [g['lr'] for g in opt.param_groups])
    assert all(np.array_equal(a, b) for a, b in zip(before[0] + before[1], after[0] + after[1])) and before[2] == after[2]
    assert opt.num_updates == 2


def test_state_dict_round_trips_before_and_after_bind(vited, gpu, init):
    ma, oa, sa = _step(vited, gpu, init, use_graph=True)
    data = _batches(5, gpu)
    for x, y in data[:4]:                                                              # captured and replayed
        sa.step(x, y)
    saved, weights = copy.deepcopy(oa.state_dict()), copy.deepcopy(ma.state_dict())
    muon_keys = {k for k, st in saved['state'].items() if set(st) == {'momentum_buffer'}}
    assert len(muon_keys) == len(oa.param_groups[0]['params']) and len(saved['state']) == len(oa.flat.params)
    assert all(set(st) == {'step', 'exp_avg', 'exp_avg_sq'} and float(st['step']) == 4.0 for k, st in saved['state'].items() if k not in muon_keys)
    mb, ob, sb = _step(vited, gpu, init, use_graph=True, load=(weights, copy.deepcopy(saved)))       # loaded before the step binds it
    # ... and into a bound one.  Eager: this run also reloads the MODEL's weights, which a captured forward would not see in its bf16
    # shadows; the load into an optimizer that has captured is the next test's, where the weights stay
    mc_, oc, sc_ = _step(vited, gpu, init, use_graph=False)
    for x, y in data[:3]:
        sc_.step(x, y)
    buffers = [oc._bufs[n].data_ptr() for n in oc._state_names]
    mc_.load_state_dict(weights)
    oc.load_state_dict(copy.deepcopy(saved))
    assert [oc._bufs[n].data_ptr() for n in oc._state_names] == buffers                # copied INTO the buffers the graph reads
    for o in (ob, oc):
        final = o.state_dict()
        assert final['param_groups'] == saved['param_groups'] and set(final['state']) == set(saved['state']) and o.num_updates == 4
        assert all(set(st) == set(saved['state'][k]) and all(same(st[n], saved['state'][k][n]) for n in st) for k, st in final['state'].items())
    x, y = data[4]                                                                     # and the resumed runs continue as the original
    la, lb, lc_ = sa.step(x, y), sb.step(x, y), sc_.step(x, y)
    assert same(la.reshape(1), lb.reshape(1)) and same(la.reshape(1), lc_.reshape(1))
    _same_models(ma, mb)
    _same_models(ma, mc_)
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(_state_bits(oa)[:2], _state_bits(ob)[:2], _state_bits(oc)[:2]))


def test_an_adamw_checkpoint_of_two_groups_goes_in_after_bind_without_a_recapture(vited, gpu, init):
    """The case a user hits: a run under NAME: adamw (two groups) resumed under NAME: muon (three), into a step that has captured."""
    madam = _hip_model(vited, vo.SHAPE_T, gpu, None)
    madam.load_state_dict(init)
    cfg = _config(1e-3)
    cfg.TRAIN.OPTIMIZER.NAME = 'adamw'
    oadam = vited.engine.build_optimizer(cfg, madam)
    sadam = vited.engine.TrainStep(madam, oadam, clip_grad=5.0, amp=True)
    data = _batches(5, gpu)
    for x, y in data[:2]:
        sadam.step(x, y)
    saved = copy.deepcopy(oadam.state_dict())
    assert len(saved['param_groups']) == 2 and type(oadam) is vited.optim.FlatAdamW
    runs = [_step(vited, gpu, init, use_graph=ug) for ug in (False, True)]
    for x, y in data[:4]:
        for _, _, st in runs:
            st.step(x, y)
    for m, o, st in runs:
        buffers = [o._bufs[n].data_ptr() for n in o._state_names]
        o.load_state_dict(copy.deepcopy(saved))
        assert [o._bufs[n].data_ptr() for n in o._state_names] == buffers and o.num_updates == 2
        for (name, p), (_, q) in zip(m.named_parameters(), madam.named_parameters()):
            want = oadam.state[q]
            if p.ndim == 2 and name.startswith(('blocks.', 'cross_blocks.')):
                assert set(o.state[p]) == {'momentum_buffer'} and same(o.state[p]['momentum_buffer'], want['exp_avg']), name
            else:
                assert same(o.state[p]['exp_avg'], want['exp_avg']) and same(o.state[p]['exp_avg_sq'], want['exp_avg_sq']), name
    losses = [st.step(*data[4]) for _, _, st in runs]
    assert same(losses[0].reshape(1), losses[1].reshape(1)) and runs[1][2].recaptures == 0 and runs[1][2]._g_opt is not None
    _same_models(runs[0][0], runs[1][0])
    assert all(np.array_equal(a, b) for a, b in zip(_state_bits(runs[0][1]), _state_bits(runs[1][1])))
