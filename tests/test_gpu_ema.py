"""The parameter EMA on the MI355X: the average kept by the update launch (vited_adamw_step_ema / vited_sgd_step_ema)
against the numpy rule of tests/ema_cases.py applied to the device's own parameters, what it must leave alone, skipped updates, a decay
changed between updates, graph replay, the exchange for evaluation (vited_ema_swap), the state round trip and the rate test's restore.

Everything here is compared BIT FOR BIT: the rule is three IEEE fp32 operations the header fixes the order of, numpy performs the same
three, and every other comparison is between two runs of the same kernels.

P: the five small tensors of ema_cases.SHAPES in two groups (2-D: decay, 1-D: none), the 2-D ones with both bf16 shadows.  The model runs
are config T's (configs/test/test_pjs_hisfrag20_patch32_64.yaml: 64 px, patch 32, width 32, 1 + 1 blocks)."""
import os
import types

import numpy as np
import pytest
import torch

import ema_cases as ec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_T = os.path.join(ROOT, 'configs', 'test', 'test_pjs_hisfrag20_patch32_64.yaml')
KINDS = {'adamw': dict(lr=2e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.05),
         'sgd_nesterov': dict(lr=2e-3, momentum=0.9, nesterov=True, weight_decay=0.05),
         'sgd_plain': dict(lr=2e-3, momentum=0.0, weight_decay=0.05)}
EMA = {'fixed': dict(ema_decay=0.9999, ema_warmup=False), 'warmup': dict(ema_decay=0.5, ema_warmup=True)}    # the ramp reaches 0.5 at n = 8
UPDATES = 12


def bits(t):
    """The bits of a float tensor (or numpy array) as a CPU integer array: equality of these is equality of every bit, NaNs included."""
    a = t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy() if torch.is_tensor(t) \
        else np.ascontiguousarray(t).view(np.int32)
    return a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


class Holder(torch.nn.Module):
    """P as a module: ``named_parameters`` / ``state_dict`` keys ps.0 .. ps.4."""

    def __init__(self, dev, only=None):
        super().__init__()
        arrays = ec.initial_parameters()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev))
                                          for i, a in enumerate(arrays) if only is None or i in only])


class Bound:
    """A fused optimizer over P, bound to a flat buffer and to a Runtime that holds both bf16 shadows of every 2-D tensor."""

    def __init__(self, vited, dev, kind, only=None, **extra):
        self.holder = Holder(dev, only)
        self.ps = list(self.holder.ps)
        groups = [{'params': [p for p in self.ps if p.ndim > 1]}, {'params': [p for p in self.ps if p.ndim <= 1], 'weight_decay': 0.0}]
        groups = [g for g in groups if g['params']]
        cls = vited.optim.FlatAdamW if kind == 'adamw' else vited.optim.FlatSGD
        self.opt = cls(groups, **KINDS[kind], **extra)
        self.flat = vited.engine.FlatGradients(self.ps)
        self.rt = vited.functions.Runtime(img_size=64, patch_size=8, in_chans=3, num_classes=4, embed_dim=384, depth=1, c_depth=1, num_heads=12)
        self.shadow_n = [self.rt.weight(p) for p in self.ps if p.ndim > 1]
        self.shadow_t = [self.rt.weight_t(p)[0] for p in self.ps if p.ndim > 1]
        self.opt.bind_flat(self.flat, types.SimpleNamespace(_runtimes={torch.bfloat16: self.rt}))

    def set_gradient(self, step, bad=None):
        g, at = ec.gradient(step), 0
        for p, view in zip(self.flat.params, self.flat.views):
            view.copy_(torch.from_numpy(g[at: at + p.numel()].reshape(p.shape)))
            at += p.numel()
        if bad is not None:
            self.flat.views[-1].view(-1)[1234] = bad

    def record(self, norm):
        o = self.opt
        return dict(p=[bits(p) for p in self.ps], bufs={n: bits(b) for n, b in o._bufs.items()}, shadow_n=[bits(s) for s in self.shadow_n],
                    shadow_t=[bits(s) for s in self.shadow_t], norm=bits(norm.reshape(1)), hyper=bits(o._hyper[:3]),
                    e=None if o.ema is None else [bits(o.ema_of(p)) for p in self.ps])


_RUNS = {}


def run(vited, dev, kind, ema):
    """12 updates on P (update 1 clipped), one record per update; computed once per (kind, ema) and shared between the tests."""
    key = (kind, ema)
    if key not in _RUNS:
        b = Bound(vited, dev, kind, **(EMA[ema] if ema else {}))
        records, counts = [], []
        if ema:
            assert all(same(b.opt.ema_of(p), p) for p in b.ps) and b.opt.num_ema_updates == 0            # e == p before the first update
        for step in range(UPDATES):
            b.set_gradient(step)
            records.append(b.record(b.opt.step_flat(1.0)))
            counts.append(b.opt.num_ema_updates)
        _RUNS[key] = records, counts
    return _RUNS[key]


def as_f32(b):
    return b.view(np.float32)


# 1. the rule, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ema', list(EMA))
@pytest.mark.parametrize('kind', list(KINDS))
def test_average_follows_the_rule_bit_for_bit(vited, gpu, kind, ema):
    records, counts = run(vited, gpu, kind, ema)
    d, warm = EMA[ema]['ema_decay'], EMA[ema]['ema_warmup']
    want = [a.copy() for a in ec.initial_parameters()]
    for step, rec in enumerate(records):
        for i, shape in enumerate(ec.SHAPES):
            p_new = as_f32(rec['p'][i])                  # the device's own new parameter
            assert step == 0 or not np.array_equal(rec['p'][i], records[step - 1]['p'][i]), (step, shape)     # it was updated
            want[i], _ = ec.update(want[i], p_new, d, warm, step)
            assert np.array_equal(rec['e'][i], bits(want[i])), f'update {step + 1}, parameter {shape}: average differs from the rule'
        assert counts[step] == step + 1
    assert ec.decay_at(d, warm, 7) < ec.decay_at(d, warm, 8) or not warm          # the run crossed the warmup's end


# 2. the average perturbs nothing --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', list(KINDS))
def test_everything_else_keeps_its_bits(vited, gpu, kind):
    plain, plain_counts = run(vited, gpu, kind, None)
    assert plain_counts == [0] * UPDATES and plain[0]['e'] is None
    for ema in EMA:
        with_ema, _ = run(vited, gpu, kind, ema)
        for step, (a, b) in enumerate(zip(plain, with_ema)):
            for what in ('p', 'shadow_n', 'shadow_t'):
                assert all(np.array_equal(x, y) for x, y in zip(a[what], b[what])), (ema, step, what)
            assert all(np.array_equal(a['bufs'][n], b['bufs'][n]) for n in a['bufs']) and set(a['bufs']) == set(b['bufs']), (ema, step)
            assert np.array_equal(a['norm'], b['norm']) and np.array_equal(a['hyper'], b['hyper']), (ema, step)
    assert as_f32(plain[-1]['hyper']).tolist() == [float(UPDATES), 0.0, 0.0]
    assert as_f32(plain[1]['norm'])[0] > 1.0 > as_f32(plain[2]['norm'])[0]        # update 2 was clipped, the others were not


# 3. skipped updates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['adamw', 'sgd_nesterov'])
def test_a_skipped_update_leaves_the_average_and_its_counter(vited, gpu, kind):
    b = Bound(vited, gpu, kind, skip_nonfinite=True, **EMA['warmup'])
    want = [a.copy() for a in ec.initial_parameters()]
    n, after = 0, []
    for step in range(5):
        b.set_gradient(step, bad=float('inf') if step == 2 else None)
        norm = b.opt.step_flat(1.0)
        rec = b.record(norm)
        after.append((rec, b.opt.num_ema_updates))
        if step == 2:
            assert not np.isfinite(as_f32(rec['norm'])[0])
            assert all(np.array_equal(x, y) for x, y in zip(rec['e'], after[1][0]['e'])) and after[2][1] == after[1][1] == 2
            assert all(np.array_equal(x, y) for x, y in zip(rec['p'], after[1][0]['p']))
        else:
            for i in range(len(want)):
                want[i], _ = ec.update(want[i], as_f32(rec['p'][i]), 0.5, True, n)
            n += 1
        assert all(np.array_equal(e, bits(w)) for e, w in zip(rec['e'], want)), step
        assert float(b.flat.flat.abs().max()) == 0.0                               # the gradients are zeroed either way
    assert b.opt.num_ema_updates == 4 and b.opt.num_updates == 4 and b.opt.skipped_updates == 1


# the config-T model -----------------------------------------------------------------------------------------------------------------
def _model(V, dev, state=None):
    m = V.build_model(V.config_from_yaml(CFG_T))
    if state is not None:
        m.load_state_dict(state)
    return m.to(dev).train()


@pytest.fixture(scope='module')
def init(vited, gpu):
    torch.manual_seed(41)
    return {k: v.clone() for k, v in _model(vited, gpu).state_dict().items()}


def _step(V, dev, init, kind='adamw', two_stage=False, **kw):
    m = _model(V, dev, init)
    groups = V.engine.param_groups_no_decay_1d(m)
    ema = {k: kw.pop(k) for k in ('ema_decay', 'ema_warmup') if k in kw}
    opt = (V.optim.FlatAdamW(groups, lr=1e-3, weight_decay=0.05, model=m, **ema) if kind == 'adamw' else
           V.optim.FlatSGD(groups, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.05, model=m, **ema))
    if two_stage:
        step = V.engine.TwoStageTrainStep(m, opt, capacity=8, neg_per_pos=1.0, clip_grad=5.0, **kw)
        step.mine_keys = torch.linspace(0, 1, 36, device=dev)
    else:
        step = V.engine.TrainStep(m, opt, clip_grad=5.0, **kw)
    return m, opt, step


def _batches(n, dev, two_stage=False, seed=7):
    g = torch.Generator().manual_seed(seed)
    if two_stage:
        return [(torch.randn(6, 3, 64, 64, generator=g).clamp(-1, 1).to(dev), torch.tensor([0, 0, 1, 1, 2, 2], device=dev)) for _ in range(n)]
    return [(torch.randn(4, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(dev), (torch.rand(4, 1, generator=g) > 0.5).float().to(dev))
            for _ in range(n)]


def _params(opt):
    return list(opt.flat.params)


def _shadow_bits(V, m):
    names = {id(p): n for n, p in m.named_parameters()}
    return {(names[pid], tag): bits(buf) for cache in V.functions.shadows_of(m) for pid, tags in cache.buffers().items()
            for tag, buf in tags.items()}


def _rule_step(opt, e_before, d, warm, n):
    """The rule applied to the device's own new parameters: what the averages must hold now."""
    return [bits(ec.update(as_f32(e), as_f32(bits(p)), d, warm, n)[0]) for e, p in zip(e_before, _params(opt))]


# 4. ema_decay changed between updates ---------------------------------------------------------------------------------------------
def test_decay_changed_between_eager_updates(vited, gpu):
    b = Bound(vited, gpu, 'adamw', ema_decay=0.9)
    want = [a.copy() for a in ec.initial_parameters()]
    for step, d in enumerate((0.9, 0.9, 0.25, 0.25, 0.0)):
        b.opt.ema_decay = d
        b.set_gradient(step)
        b.opt.step_flat(1.0)
        want = [ec.update(w, as_f32(bits(p)), d, False, step)[0] for w, p in zip(want, b.ps)]
        assert all(same(b.opt.ema_of(p), w) for p, w in zip(b.ps, want)), (step, d)
    assert all(same(b.opt.ema_of(p), p) for p in b.ps)                             # a decay of 0: the average IS the parameter
    assert b.opt.hyper_uploads == 1 + 3                                            # the groups once, the decay three times


def test_decay_changed_under_a_captured_step(vited, gpu, init):
    m, opt, step = _step(vited, gpu, init, use_graph=True, amp=True, ema_decay=0.9)
    batches = _batches(6, gpu)
    for x, y in batches[:4]:
        step.step(x, y)
    graph = step._g_opt
    assert graph is not None and step.recaptures == 0 and opt.num_ema_updates == 4
    for (x, y), d in zip(batches[4:], (0.25, 0.75)):
        e_before = [bits(opt.ema_of(p)) for p in _params(opt)]
        n = opt.num_ema_updates
        opt.ema_decay = d
        step.step(x, y)
        assert all(np.array_equal(bits(opt.ema_of(p)), w) for p, w in zip(_params(opt), _rule_step(opt, e_before, d, False, n))), d
    assert step._g_opt is graph and step.recaptures == 0 and opt.num_ema_updates == 6


# 5. captured = eager ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('two_stage,kind', [(False, 'adamw'), (False, 'sgd'), (True, 'adamw')])
def test_replayed_step_equals_the_eager_one(vited, gpu, init, two_stage, kind):
    runs = [_step(vited, gpu, init, kind, two_stage, use_graph=ug, amp=True, ema_decay=0.9, ema_warmup=True) for ug in (False, True)]
    for x, y in _batches(4, gpu, two_stage):
        le, lg = [st.step(x, y) for _, _, st in runs]
        assert same(le.reshape(1), lg.reshape(1))
    (me, oe, se), (mg, og, sg) = runs
    assert se._g1 is None and sg._g_opt is not None and sg.recaptures == 0
    assert oe.num_ema_updates == og.num_ema_updates == 4 and same(oe.ema, og.ema) and not same(oe.ema, oe.flat.flat)
    moved = 0
    for (name, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
        assert same(pe, pg), name
        assert same(oe.ema_of(pe), og.ema_of(pg)), name
        moved += not same(oe.ema_of(pe), pe)
    assert moved > 0
    sh_e, sh_g = _shadow_bits(vited, me), _shadow_bits(vited, mg)
    assert sh_e and set(sh_e) == set(sh_g) and all(np.array_equal(sh_e[k], sh_g[k]) for k in sh_e)


# 6. the swap, inside the block -----------------------------------------------------------------------------------------------------
def test_inside_the_block_the_model_evaluates_on_the_average(vited, gpu, init, monkeypatch):
    m, opt, step = _step(vited, gpu, init, amp=True, ema_decay=0.5)
    for x, y in _batches(3, gpu):
        step.step(x, y)
    averaged = opt.ema_state_dict(m)
    assert list(averaged) == list(m.state_dict()) and not same(averaged['head.weight'], m.head.weight)
    other = _model(vited, gpu, averaged).eval()
    x = _batches(1, gpu, seed=99)[0][0]
    raw = {n: bits(p) for n, p in m.named_parameters()}
    m.eval()
    for amp in (False, True):
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=amp):
            want, outside = other(x), m(x)
            with opt.swap_ema():
                assert opt.ema_swapped
                inside = m(x)
                assert all(same(p, averaged[n]) for n, p in m.named_parameters())
                assert all(same(opt.ema_of(p), as_f32(raw[n])) for n, p in m.named_parameters())      # the raw weights wait in ema
                inner = opt.ema_state_dict(m)
                assert all(same(inner[k], averaged[k]) for k in averaged)
                with pytest.raises(RuntimeError, match='nested use'):
                    with opt.swap_ema():
                        pass
                with pytest.raises(RuntimeError, match='step_flat: not inside'):
                    opt.step_flat(1.0)
                with pytest.raises(RuntimeError, match='TrainStep.step: not inside'):
                    step.step(*_batches(1, gpu)[0])
        assert same(inside, want) and not same(inside, outside), amp
        assert not opt.ema_swapped and all(same(p, as_f32(raw[n])) for n, p in m.named_parameters())
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='not during graph capture'):
        with opt.swap_ema():
            pass


# 7. the swap, after the block --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['adamw', 'sgd_nesterov'])
def test_after_the_block_every_bit_is_back_and_training_continues_alike(vited, gpu, kind):
    a, b = (Bound(vited, gpu, kind, **EMA['warmup']) for _ in range(2))
    for step in range(3):
        for t in (a, b):
            t.set_gradient(step)
            t.opt.step_flat(1.0)
    before, key, versions = a.record(a.opt._norm), a.opt._desc_key, [p._version for p in a.ps]
    with a.opt.swap_ema():
        for i, p in enumerate(a.ps):
            assert np.array_equal(bits(p), before['e'][i]) and np.array_equal(bits(a.opt.ema_of(p)), before['p'][i])
        assert all(p._version > v for p, v in zip(a.ps, versions))                 # published like an update
        for p, sh in zip([p for p in a.ps if p.ndim > 1], a.shadow_n):
            assert a.rt.weight(p) is sh and same(sh, p.detach().to(torch.bfloat16))            # current: no recast, and of the average
    after = a.record(a.opt._norm)
    for what in ('p', 'e', 'shadow_n', 'shadow_t'):
        assert all(np.array_equal(x, y) for x, y in zip(before[what], after[what])), what
    assert a.opt._desc_key == key and a.opt.num_ema_updates == 3
    for t in (a, b):
        t.set_gradient(3)
        t.opt.step_flat(1.0)
    ra, rb = a.record(a.opt._norm), b.record(b.opt._norm)
    for what in ('p', 'e', 'shadow_n', 'shadow_t'):
        assert all(np.array_equal(x, y) for x, y in zip(ra[what], rb[what])), what
    assert all(np.array_equal(ra['bufs'][n], rb['bufs'][n]) for n in ra['bufs']) and np.array_equal(ra['hyper'], rb['hyper'])


def test_swap_against_its_numpy_statement(vited, gpu):
    b = Bound(vited, gpu, 'adamw', only=(3, 4), ema_decay=0.5)                     # [65, 63] and [130, 70] alone
    b.set_gradient(0)
    b.opt.step_flat(1.0)
    p0, e0 = [as_f32(bits(p)) for p in b.ps], [as_f32(bits(b.opt.ema_of(p))) for p in b.ps]
    assert not any(np.array_equal(p, e) for p, e in zip(p0, e0))
    bf16 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16)
    with b.opt.swap_ema():
        for i, p in enumerate(b.ps):
            p1, e1, sh, sh_t = ec.swap(p0[i], e0[i])
            assert same(p, p1) and same(b.opt.ema_of(p), e1)
            assert same(b.shadow_n[i], bf16(sh)) and same(b.shadow_t[i], bf16(sh_t)) and b.shadow_t[i].shape == (p.shape[1], p.shape[0])
    for i, p in enumerate(b.ps):
        assert same(p, p0[i]) and same(b.opt.ema_of(p), e0[i])
        assert same(b.shadow_n[i], bf16(p0[i])) and same(b.shadow_t[i], bf16(p0[i].T))


# 8. state round trip -----------------------------------------------------------------------------------------------------------------
def test_state_round_trip_before_binding_after_binding_and_after_a_capture(vited, gpu, init):
    ema = dict(ema_decay=0.5, ema_warmup=True)
    batches = _batches(7, gpu)
    ma, oa, sa = _step(vited, gpu, init, amp=True, **ema)
    # c runs the same batches replayed (its parameters and moments are a's, bit for bit) but averages with another decay
    mc, oc, sc = _step(vited, gpu, init, amp=True, use_graph=True, ema_decay=0.125)
    for x, y in batches[:4]:
        sa.step(x, y)
        sc.step(x, y)
    assert sc._g_opt is not None and all(same(x, y) for x, y in zip(ma.parameters(), mc.parameters())) and not same(oa.ema, oc.ema)
    averaged, count = oa.ema_state_dict(ma), oa.num_ema_updates
    assert count == 4
    # b: a fresh optimizer, everything loaded before it is bound
    mb = _model(vited, gpu, ma.state_dict())
    ob = vited.optim.FlatAdamW(vited.engine.param_groups_no_decay_1d(mb), lr=1e-3, weight_decay=0.05, model=mb, **ema)
    ob.load_state_dict(oa.state_dict())
    ob.load_ema_state_dict(averaged, mb, num_ema_updates=count)
    assert ob.ema is None and ob.num_ema_updates == 4
    sb = vited.engine.TrainStep(mb, ob, clip_grad=5.0, amp=True)
    # c: loaded after binding and after the capture, into the buffer the graph reads
    graph, buffer = sc._g_opt, oc.ema.data_ptr()
    oc.ema_decay, oc.ema_warmup = 0.5, True
    oc.load_ema_state_dict(averaged, mc, num_ema_updates=count)
    assert oc.ema.data_ptr() == buffer
    for o in (ob, oc):
        assert o.num_ema_updates == 4 and same(o.ema, oa.ema)
    for x, y in batches[4:]:
        for st in (sa, sb, sc):
            st.step(x, y)
    assert sc._g_opt is graph and sc.recaptures == 0
    for (name, pa), (_, pb), (_, pc) in zip(ma.named_parameters(), mb.named_parameters(), mc.named_parameters()):
        assert same(pa, pb) and same(pa, pc), name
        assert same(oa.ema_of(pa), ob.ema_of(pb)) and same(oa.ema_of(pa), oc.ema_of(pc)), name
    assert oa.num_ema_updates == ob.num_ema_updates == oc.num_ema_updates == 7


# 9. the rate test's restore ------------------------------------------------------------------------------------------------------------
def test_find_lr_restores_the_average_and_its_counter(vited, gpu, init):
    m, opt, step = _step(vited, gpu, init, amp=True, ema_decay=0.5, ema_warmup=True)
    for x, y in _batches(2, gpu):
        step.step(x, y)
    e, p, hyper = bits(opt.ema), [bits(q) for q in _params(opt)], bits(opt._hyper)
    result = vited.engine.find_lr(step, _batches(6, gpu, seed=3), num_iter=6, start_lr=1e-5, end_lr=1e-2, restore=True)
    assert result.iterations >= 2
    assert np.array_equal(bits(opt.ema), e) and opt.num_ema_updates == 2 and np.array_equal(bits(opt._hyper), hyper)
    assert all(np.array_equal(bits(q), w) for q, w in zip(_params(opt), p))
    kept = vited.engine.find_lr(step, _batches(6, gpu, seed=3), num_iter=6, start_lr=1e-5, end_lr=1e-2, restore=False)
    assert opt.num_ema_updates == 8 and not np.array_equal(bits(opt.ema), e)      # the sweep does move it


# 10. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['adamw', 'sgd_nesterov'])
def test_entries_refuse_a_null_or_short_average_before_any_launch(vited, gpu, kind):
    b = Bound(vited, gpu, kind, **EMA['fixed'])
    b.set_gradient(0)
    o = b.opt
    o.sync_hyperparameters()
    desc = o._descriptors()
    before = (b.record(o._norm), bits(o._hyper), bits(b.flat.flat), bits(o.ema))
    lib, n = vited._lib.load(), b.flat.flat.numel()
    entry = getattr(lib, 'vited_adamw_step_ema' if kind == 'adamw' else 'vited_sgd_step_ema')
    args = [desc.data_ptr(), desc.shape[0], o._tiles, b.flat.flat.data_ptr(), n, o._hyper.data_ptr(), 1.0, 1, o._norm.data_ptr(), o._ws.data_ptr(),
            o._ws.numel() * 4]
    stream = torch.cuda.current_stream().cuda_stream
    assert entry(*args, None, n, stream) == 1                                      # VITED_ERR_BAD_ARG: null
    assert entry(*args, o.ema.data_ptr(), n - 1, stream) == 1                      # shorter than the gradient buffer
    assert entry(*args, o.ema.data_ptr() + 4, n, stream) == 1                      # not 16-byte aligned
    assert lib.vited_ema_swap(desc.data_ptr(), desc.shape[0], o._tiles, None, b.flat.flat.data_ptr(), stream) == 1
    assert lib.vited_ema_swap(desc.data_ptr(), desc.shape[0], o._tiles, o.ema.data_ptr() + 4, b.flat.flat.data_ptr(), stream) == 1
    with pytest.raises(ValueError, match='^ema_swap: ema '):
        vited.ops.ema_swap(desc, o._tiles, o.ema[:-16], b.flat.flat)
    torch.cuda.synchronize()
    after = (b.record(o._norm), bits(o._hyper), bits(b.flat.flat), bits(o.ema))
    for what in ('p', 'e', 'shadow_n', 'shadow_t'):
        assert all(np.array_equal(x, y) for x, y in zip(before[0][what], after[0][what])), what
    assert all(np.array_equal(before[0]['bufs'][k], after[0]['bufs'][k]) for k in before[0]['bufs'])
    assert all(np.array_equal(x, y) for x, y in zip(before[1:], after[1:])) and np.array_equal(before[0]['norm'], after[0]['norm'])
    assert o.num_ema_updates == 0 and o.num_updates == 0
