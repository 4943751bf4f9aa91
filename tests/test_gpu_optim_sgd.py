"""The tail of the training loop on the GPU: the fused clip + SGD kernel against torch.optim.SGD + clip_grad_norm_
(misc/optimizer.py:22-24, misc/utils.py:215-223), its hipGraph replay, state interchange with torch.optim.SGD, updates skipped on a
non-finite gradient norm (what GradScaler.step does for the reference, misc/utils.py:206-226) for both fused optimizers, a second
TrainStep on one optimizer, and the loop's meters on the device (misc/engine.py:221-222, 235).

Tolerances are those of test_gpu_engine.py's AdamW test: the kernels evaluate torch's expressions with other roundings, so parameters
agree to rtol 2e-6 (atol tied to lr), state buffers to rtol 1e-5; whatever compares two runs of the SAME kernels (graph replay against
eager launches, flagged against unflagged, skipped against untouched) is bit for bit.
"""
import copy
import types

import pytest
import torch

from oracle import vited_oracle as vo
from test_gpu_engine import _Sched, _hip_model

pytestmark = pytest.mark.gpu

SHAPES = [(384, 1152), (4, 384), (384, 3, 8, 8), (384,), (65, 130), (1536, 384), (1,), (1, 1, 384), (100, 36)]
SGD_VARIANTS = {'nesterov': dict(momentum=0.9, nesterov=True), 'momentum': dict(momentum=0.9), 'plain': dict(momentum=0.0)}
ADAMW_KW = dict(lr=2e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.05)
SGD_KW = dict(lr=2e-3, weight_decay=0.05)


def _groups(ps):
    return [{'params': [p for p in ps if p.ndim > 1]}, {'params': [p for p in ps if p.ndim <= 1], 'weight_decay': 0.0}]


def _twins(gpu, seed=0):
    torch.manual_seed(seed)
    mine = [torch.nn.Parameter(torch.randn(sh, device=gpu) * 0.1) for sh in SHAPES]
    return mine, [torch.nn.Parameter(p.detach().clone()) for p in mine]


class _Bound:
    """A fused optimizer over SHAPES, bound to a flat buffer with an ``early`` bucket and to a Runtime that holds bf16 shadows."""

    def __init__(self, vited, opt, mine):
        self.opt, self.mine = opt, mine
        self.flat = vited.engine.FlatGradients(mine, early=[mine[1], mine[3]])       # any layout of the flat buffer
        self.rt = vited.functions.Runtime(img_size=64, patch_size=8, in_chans=3, num_classes=4, embed_dim=384, depth=1, c_depth=1, num_heads=12)
        self.shadow_n = {i: self.rt.weight(mine[i]) for i in (0, 2, 5, 8)}
        self.shadow_t = {i: self.rt.weight_t(mine[i])[0] for i in (0, 4, 5)}
        opt.bind_flat(self.flat, types.SimpleNamespace(_runtimes={torch.bfloat16: self.rt}))

    def check_shadows(self):
        for i, sh in self.shadow_n.items():
            assert torch.equal(sh, self.mine[i].detach().reshape(self.mine[i].shape[0], -1).to(torch.bfloat16)), f'shadow of param {i}'
            assert self.rt.weight(self.mine[i]) is sh                       # the cache entry stays valid: no recast on the next forward
        for i, sh in self.shadow_t.items():
            assert torch.equal(sh, self.mine[i].detach().reshape(self.mine[i].shape[0], -1).t().contiguous().to(torch.bfloat16)), f'shadow_t of param {i}'

    def snapshot(self):
        state = [{k: v.clone() for k, v in self.opt.state[p].items() if torch.is_tensor(v)} for p in self.mine]
        return ([p.detach().clone() for p in self.mine], state, [s.clone() for s in self.shadow_n.values()],
                [s.clone() for s in self.shadow_t.values()])


def _gradients(mine, ref, it, generator, bad=None):
    """The same random gradients into the flat views and into the torch twin; ``bad``: one element of the largest parameter."""
    for i, (p, q) in enumerate(zip(mine, ref)):
        g = torch.randn(p.shape, device=p.device, generator=generator) * (3.0 if it == 1 else 0.01)     # step 1: the clip is active
        if bad is not None and i == 5:
            g.view(-1)[1234] = bad
        p.grad.copy_(g)
        if q is not None:
            q.grad = g.clone()


def _set_lr(opts, lr):
    for o in opts:
        for grp in o.param_groups:
            grp['lr'] = lr


def _assert_params_close(mine, ref, lr, what):
    for i, (p, q) in enumerate(zip(mine, ref)):
        torch.testing.assert_close(p, q, rtol=2e-6, atol=1e-3 * lr, msg=lambda m: f'{what} param {i} {tuple(p.shape)}: {m}')


def _assert_state_close(opt, topt, mine, ref, names):
    for p, q in zip(mine, ref):
        for name, atol in names:
            torch.testing.assert_close(opt.state[p][name], topt.state[q][name], rtol=1e-5, atol=atol)


# ---------------------------------------------------------------------------------------------
# 1. parity with torch.optim.SGD
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', list(SGD_VARIANTS))
def test_flat_sgd_matches_torch_sgd_and_refreshes_shadows(vited, gpu, variant):
    kw = dict(SGD_KW, **SGD_VARIANTS[variant])
    mine, ref = _twins(gpu)
    opt, topt = vited.optim.FlatSGD(_groups(mine), **kw), torch.optim.SGD(_groups(ref), **kw)
    b = _Bound(vited, opt, mine)
    assert opt.state_dict()['state'] == {}                                    # empty before the first update, as torch's
    gen = torch.Generator(device=gpu).manual_seed(1)
    for it in range(4):
        _gradients(mine, ref, it, gen)
        lr = 2e-3 / (1 + it)                                                  # per-iteration schedule
        _set_lr((opt, topt), lr)
        want_norm = torch.nn.utils.clip_grad_norm_(ref, 1.0)
        topt.step()
        norm = opt.step_flat(1.0)
        torch.testing.assert_close(norm, want_norm, rtol=1e-5, atol=1e-7)
        assert float(b.flat.flat.abs().max()) == 0.0                          # zero_grad fused in
        _assert_params_close(mine, ref, lr, f'step {it}')
        if kw['momentum']:
            _assert_state_close(opt, topt, mine, ref, [('momentum_buffer', 1e-9)])
        else:
            assert all(not opt.state[p] for p in mine) and all(not topt.state[q] for q in ref)
        b.check_shadows()
    assert opt.num_updates == 4 and opt.skipped_updates == 0
    sd, tsd = opt.state_dict(), topt.state_dict()                             # torch.optim.SGD-shaped state (misc/utils.py:130-142)
    assert set(sd['state']) == set(tsd['state']) and set(sd['param_groups'][0]) == set(tsd['param_groups'][0])
    if kw['momentum']:
        base = opt._bufs['momentum_buffer']
        assert all(opt.state[p]['momentum_buffer'].untyped_storage().data_ptr() == base.untyped_storage().data_ptr() for p in mine)


# ---------------------------------------------------------------------------------------------
# 2. graph replay equals eager launches
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('amp,accum', [(False, 1), (True, 1), (False, 2), (True, 2)])
def test_sgd_graph_replay_equals_eager_with_lr_schedule_and_accumulation(vited, gpu, amp, accum):
    """TrainStep(use_graph=True) with FlatSGD: a learning rate that changes after every update and (accum = 2) two micro-batches
    per update must give, bit for bit, the eagerly launched TrainStep's losses, norm and parameters; with bf16 the weight shadows
    are refreshed inside the update, so an eval forward right after training equals that of a freshly loaded copy."""
    s = vo.ViTEDShape(depth=1, c_depth=1)
    torch.manual_seed(3)
    init = _hip_model(vited, s, gpu, None).state_dict()
    models, steps = [], []
    for use_graph in (False, True):
        m = _hip_model(vited, s, gpu, None)
        m.load_state_dict(init)
        opt = vited.optim.FlatSGD(vited.engine.param_groups_no_decay_1d(m), lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.05)
        steps.append(vited.engine.TrainStep(m, opt, clip_grad=5.0, amp=amp, use_graph=use_graph, accumulation_steps=accum,
                                            lr_scheduler=_Sched(opt, 1e-2)))
        models.append(m)
    g = torch.Generator().manual_seed(9)
    for it in range(7 * accum):
        x = torch.randn(8, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
        y = (torch.rand(8, 4, generator=g) > 0.6).float().to(gpu)
        le, lg = [float(st.step(x, y)) for st in steps]
        assert le == lg, (it, le, lg)
    assert steps[1]._g1 is not None and steps[1]._g2 is not None and steps[0].num_updates == steps[1].num_updates == 7
    assert steps[1].recaptures == 0
    assert float(steps[0].last_norm) == float(steps[1].last_norm)
    assert steps[0].optimizer.num_updates == steps[1].optimizer.num_updates == 7
    for (n, pe), (_, pg) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert torch.equal(pe, pg), f'{n}: graph replay differs from eager launches'
    assert not torch.equal(models[0].head.weight, init['head.weight'])
    x = torch.randn(4, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=amp):
        after = [m.eval()(x) for m in models]
        fresh = _hip_model(vited, s, gpu, None)
        fresh.load_state_dict(models[1].state_dict())
        want = fresh.eval()(x)
    assert torch.equal(after[0], want) and torch.equal(after[1], want), 'stale bf16 weight shadows after the last update'


# ---------------------------------------------------------------------------------------------
# 3. state interchange with torch.optim.SGD
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('load_first', [True, False])
def test_sgd_state_moves_between_torch_and_flat(vited, gpu, load_first):
    """torch -> FlatSGD (loaded before or after bind_flat) -> torch: two updates each, against torch.optim.SGD all the way."""
    kw = dict(SGD_KW, momentum=0.9, nesterov=True)
    mine, ref = _twins(gpu)
    topt = torch.optim.SGD(_groups(ref), **kw)
    gen = torch.Generator(device=gpu).manual_seed(2)
    flat0 = vited.engine.FlatGradients(mine)            # only to give the twin's gradients a home during torch's two updates
    updates = 0

    def torch_update(params, o):
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        o.step()

    for it in range(2):
        _gradients(mine, ref, it, gen)
        _set_lr((topt,), 2e-3 / (1 + updates))
        torch_update(ref, topt)
        updates += 1
    for p, q in zip(mine, ref):
        p.data.copy_(q.data)                             # the checkpoint's parameters
    saved = copy.deepcopy(topt.state_dict())
    del flat0
    opt = vited.optim.FlatSGD(_groups(mine), **kw)
    if load_first:
        opt.load_state_dict(saved)
        b = _Bound(vited, opt, mine)
    else:
        b = _Bound(vited, opt, mine)
        opt.load_state_dict(saved)
    for it in range(2, 4):
        _gradients(mine, ref, it, gen)
        lr = 2e-3 / (1 + updates)
        _set_lr((opt, topt), lr)
        torch_update(ref, topt)
        opt.step_flat(1.0)
        updates += 1
        _assert_params_close(mine, ref, lr, f'after loading, step {it}')
        _assert_state_close(opt, topt, mine, ref, [('momentum_buffer', 1e-9)])
        b.check_shadows()
    # the other direction: FlatSGD's state into a fresh torch.optim.SGD over copies of FlatSGD's parameters
    back = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    topt2 = torch.optim.SGD(_groups(back), **kw)
    topt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    for it in range(4, 6):
        _gradients(mine, ref, it, gen)
        for q, r in zip(ref, back):
            r.grad = q.grad.clone()
        lr = 2e-3 / (1 + updates)
        _set_lr((opt, topt, topt2), lr)
        torch_update(ref, topt)
        torch_update(back, topt2)
        opt.step_flat(1.0)
        updates += 1
        _assert_params_close(back, ref, lr, f'torch resumed from FlatSGD, step {it}')
        _assert_params_close(mine, ref, lr, f'step {it}')
    # a torch state without buffers (saved before torch's first update, or momentum_buffer None) loads as zeros
    empty = torch.optim.SGD(_groups([torch.nn.Parameter(p.detach().clone()) for p in mine]), **kw).state_dict()
    opt.load_state_dict(empty)
    assert float(opt._bufs['momentum_buffer'].abs().max()) == 0.0


def test_load_state_dict_into_a_captured_train_step_keeps_replaying(vited, gpu):
    """load_state_dict copies INTO the flat momentum buffer the captured update graph reads: replays go on without a recapture and
    equal an eager TrainStep that loaded the same state."""
    s = vo.ViTEDShape(depth=1, c_depth=1)
    torch.manual_seed(4)
    init = _hip_model(vited, s, gpu, None).state_dict()
    models, steps = [], []
    for use_graph in (False, True):
        m = _hip_model(vited, s, gpu, None)
        m.load_state_dict(init)
        opt = vited.optim.FlatSGD(vited.engine.param_groups_no_decay_1d(m), lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.05)
        steps.append(vited.engine.TrainStep(m, opt, clip_grad=5.0, amp=True, use_graph=use_graph))
        models.append(m)
    g = torch.Generator().manual_seed(5)

    def batch():
        return (torch.randn(8, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu), (torch.rand(8, 4, generator=g) > 0.6).float().to(gpu))

    for it in range(4):
        x, y = batch()
        assert float(steps[0].step(x, y)) == float(steps[1].step(x, y))
    assert steps[1]._g_opt is not None
    graph = steps[1]._g_opt
    saved = copy.deepcopy(steps[0].optimizer.state_dict())
    for name, st in saved['state'].items():
        st['momentum_buffer'].mul_(0.5)                   # a state that differs from both runs' own
    for st in steps:
        st.optimizer.load_state_dict(copy.deepcopy(saved))
    for it in range(3):
        x, y = batch()
        assert float(steps[0].step(x, y)) == float(steps[1].step(x, y))
    assert steps[1]._g_opt is graph and steps[1].recaptures == 0
    for (n, pe), (_, pg) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert torch.equal(pe, pg), n
    p0 = next(iter(steps[1].optimizer.state))
    assert steps[1].optimizer.state[p0]['momentum_buffer'].untyped_storage().data_ptr() == \
        steps[1].optimizer._bufs['momentum_buffer'].untyped_storage().data_ptr()


# ---------------------------------------------------------------------------------------------
# 4. an update with a non-finite gradient norm is skipped
# ---------------------------------------------------------------------------------------------
def _fused_and_torch(vited, kind, mine, ref, **extra):
    if kind == 'adamw':
        return (vited.optim.FlatAdamW(_groups(mine), **ADAMW_KW, **extra), torch.optim.AdamW(_groups(ref), **ADAMW_KW),
                [('exp_avg', 1e-9), ('exp_avg_sq', 1e-12)])
    kw = dict(SGD_KW, momentum=0.9, nesterov=True)
    return vited.optim.FlatSGD(_groups(mine), **kw, **extra), torch.optim.SGD(_groups(ref), **kw), [('momentum_buffer', 1e-9)]


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
@pytest.mark.parametrize('kind', ['adamw', 'sgd'])
def test_nonfinite_gradient_skips_the_update(vited, gpu, kind, bad):
    mine, ref = _twins(gpu)
    opt, topt, names = _fused_and_torch(vited, kind, mine, ref, skip_nonfinite=True)
    b = _Bound(vited, opt, mine)
    gen = torch.Generator(device=gpu).manual_seed(1)
    for it in range(4):
        _gradients(mine, ref, it, gen, bad=bad if it == 1 else None)
        lr = 2e-3 / (1 + it)
        _set_lr((opt, topt), lr)
        want_norm = torch.nn.utils.clip_grad_norm_(ref, 1.0)
        before = b.snapshot()
        if it != 1:
            topt.step()                                   # GradScaler.step leaves optimizer.step() out in iteration 1
        norm = opt.step_flat(1.0)
        assert float(b.flat.flat.abs().max()) == 0.0      # the gradients are zeroed either way
        if it == 1:
            assert not torch.isfinite(norm) and not torch.isfinite(want_norm)
            after = b.snapshot()
            for x, y in zip(before[0] + before[2] + before[3], after[0] + after[2] + after[3]):
                assert torch.equal(x, y), 'a skipped update changed a parameter or a shadow'
            for sx, sy in zip(before[1], after[1]):
                assert sx.keys() == sy.keys() and all(torch.equal(sx[k], sy[k]) for k in sx), 'a skipped update changed the state'
        else:
            torch.testing.assert_close(norm, want_norm, rtol=1e-5, atol=1e-7)
            _assert_params_close(mine, ref, lr, f'step {it}')
            _assert_state_close(opt, topt, mine, ref, names)
        b.check_shadows()
    assert opt.num_updates == 3 and opt.skipped_updates == 1
    assert all(bool(torch.isfinite(p).all()) for p in mine)


@pytest.mark.parametrize('kind', ['adamw', 'sgd'])
def test_skip_flag_changes_no_bit_on_finite_gradients(vited, gpu, kind):
    runs = []
    for flag in (False, True):
        mine, _ = _twins(gpu)
        opt, _, names = _fused_and_torch(vited, kind, mine, mine, skip_nonfinite=flag)
        b = _Bound(vited, opt, mine)
        gen = torch.Generator(device=gpu).manual_seed(1)
        norms = []
        for it in range(4):
            _gradients(mine, [None] * len(mine), it, gen)
            _set_lr((opt,), 2e-3 / (1 + it))
            norms.append(float(opt.step_flat(1.0)))
        assert opt.num_updates == 4 and opt.skipped_updates == 0
        runs.append((norms, b.snapshot()))
    assert runs[0][0] == runs[1][0]
    (p0, s0, n0, t0), (p1, s1, n1, t1) = runs[0][1], runs[1][1]
    for x, y in zip(p0 + n0 + t0, p1 + n1 + t1):
        assert torch.equal(x, y)
    for sx, sy in zip(s0, s1):
        assert sx.keys() == sy.keys() and all(torch.equal(sx[k], sy[k]) for k in sx)


def test_unflagged_optimizer_still_lets_a_nan_through(vited, gpu):
    """With the flag clear the kernel does what it did before: the update is applied and counted, and the NaN gradient reaches its
    parameter (a NaN norm fails the ``clip < 1`` comparison, so the coefficient is 1 and the other elements stay finite)."""
    mine, _ = _twins(gpu)
    opt = vited.optim.FlatSGD(_groups(mine), **SGD_KW, momentum=0.9)
    b = _Bound(vited, opt, mine)
    _gradients(mine, [None] * len(mine), 0, torch.Generator(device=gpu).manual_seed(1), bad=float('nan'))
    assert not torch.isfinite(opt.step_flat(1.0))
    assert opt.num_updates == 1 and opt.skipped_updates == 0
    assert bool(torch.isnan(mine[5].view(-1)[1234])) and bool(torch.isnan(opt.state[mine[5]]['momentum_buffer'].view(-1)[1234]))
    assert int(torch.isnan(mine[5]).sum()) == 1 and bool(torch.isfinite(mine[0]).all())
    assert float(b.flat.flat.abs().max()) == 0.0


@pytest.mark.parametrize('kind', ['adamw', 'sgd'])
def test_captured_update_skips_a_nan_batch_and_trains_on(vited, gpu, kind):
    """Through TrainStep on the one-block model, a NaN in one batch's input: the replayed update skips (parameters keep their bits,
    the norm is not finite), the next replays train on, and the replayed run equals the eager one bit for bit throughout."""
    s = vo.ViTEDShape(depth=1, c_depth=1)
    torch.manual_seed(6)
    init = _hip_model(vited, s, gpu, None).state_dict()
    models, steps = [], []
    for use_graph in (False, True):
        m = _hip_model(vited, s, gpu, None)
        m.load_state_dict(init)
        groups = vited.engine.param_groups_no_decay_1d(m)
        if kind == 'adamw':
            opt = vited.optim.FlatAdamW(groups, lr=1e-3, weight_decay=0.05, skip_nonfinite=True)
        else:
            opt = vited.optim.FlatSGD(groups, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.05, skip_nonfinite=True)
        steps.append(vited.engine.TrainStep(m, opt, clip_grad=5.0, amp=True, use_graph=use_graph, lr_scheduler=_Sched(opt, opt.defaults['lr'])))
        models.append(m)
    g = torch.Generator().manual_seed(7)
    for it in range(6):
        x = torch.randn(8, 2, 3, 64, 64, generator=g).clamp(-1, 1)
        y = (torch.rand(8, 4, generator=g) > 0.6).float().to(gpu)
        if it == 4:
            x[3, 0, 1, 17, 5] = float('nan')
        x = x.to(gpu)
        before = [p.detach().clone() for p in models[1].parameters()]
        losses = [float(st.step(x, y)) for st in steps]
        if it == 4:
            assert steps[1]._g_opt is not None                                           # this update was a replay
            assert all(l != l for l in losses) and not torch.isfinite(steps[1].last_norm) and not torch.isfinite(steps[0].last_norm)
            for p, q in zip(models[1].parameters(), before):
                assert torch.equal(p, q), 'the skipped replay changed a parameter'
        else:
            assert losses[0] == losses[1] and losses[0] == losses[0], (it, losses)
            assert float(steps[0].last_norm) == float(steps[1].last_norm)
            assert any(not torch.equal(p, q) for p, q in zip(models[1].parameters(), before))
    for st in steps:
        assert st.num_updates == 6 and st.optimizer.num_updates == 5 and st.optimizer.skipped_updates == 1
    assert steps[1].recaptures == 0
    for (n, pe), (_, pg) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert torch.equal(pe, pg) and bool(torch.isfinite(pg).all()), n
    x = torch.randn(4, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        fresh = _hip_model(vited, s, gpu, None)
        fresh.load_state_dict(models[1].state_dict())
        assert torch.equal(models[1].eval()(x), fresh.eval()(x)), 'stale bf16 weight shadows'


# ---------------------------------------------------------------------------------------------
# 5. a second TrainStep on the same optimizer
# ---------------------------------------------------------------------------------------------
class _LinearInParameters(torch.nn.Module):
    """With the criterion mean(out * y) the gradient does not depend on the parameters, so the fused and the torch run see the same
    gradients bit for bit and only the optimizers differ."""

    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(130, 65)

    def forward(self, x):
        return self.fc(x)


def test_second_train_step_keeps_the_step_count(vited, gpu):
    torch.manual_seed(8)
    a, ref = _LinearInParameters().to(gpu), _LinearInParameters().to(gpu)
    ref.load_state_dict(a.state_dict())
    kw = dict(lr=2e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.05)
    opt = vited.optim.FlatAdamW(vited.engine.param_groups_no_decay_1d(a), **kw)
    topt = torch.optim.AdamW(vited.engine.param_groups_no_decay_1d(ref), **kw)
    crit = lambda out, y: (out * y).mean()
    g = torch.Generator().manual_seed(3)
    step = None
    for it in range(4):
        if it % 2 == 0:
            step = vited.engine.TrainStep(a, opt, clip_grad=5.0, amp=False, criterion=crit)      # it == 2: a second TrainStep, a new flat buffer
        x, y = torch.randn(16, 130, generator=g).to(gpu), torch.randn(16, 65, generator=g).to(gpu)
        step.step(x, y)
        topt.zero_grad()
        crit(ref(x), y).backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 5.0)
        topt.step()
    assert opt.num_updates == 4 and opt.skipped_updates == 0
    assert float(opt.state_dict()['state'][0]['step']) == 4.0
    for (n, p), (_, q) in zip(a.named_parameters(), ref.named_parameters()):
        torch.testing.assert_close(p, q, rtol=2e-6, atol=1e-3 * kw['lr'], msg=lambda m: f'{n}: {m}')
        torch.testing.assert_close(opt.state[p]['exp_avg'], topt.state[q]['exp_avg'], rtol=1e-5, atol=1e-9)
        torch.testing.assert_close(opt.state[p]['exp_avg_sq'], topt.state[q]['exp_avg_sq'], rtol=1e-5, atol=1e-12)


# ---------------------------------------------------------------------------------------------
# 6. the loop's meters on the device
# ---------------------------------------------------------------------------------------------
class _AverageMeter:
    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


@pytest.mark.parametrize('accum', [1, 2])
def test_train_step_meters_eager_and_captured(vited, gpu, accum):
    s = vo.ViTEDShape(depth=1, c_depth=1)
    torch.manual_seed(10)
    init = _hip_model(vited, s, gpu, None).state_dict()
    models, steps = [], []
    for use_graph, meters in ((False, True), (True, True), (False, False)):
        m = _hip_model(vited, s, gpu, None)
        m.load_state_dict(init)
        opt = vited.optim.FlatSGD(vited.engine.param_groups_no_decay_1d(m), lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.05)
        steps.append(vited.engine.TrainStep(m, opt, clip_grad=5.0, amp=True, use_graph=use_graph, accumulation_steps=accum, meters=meters))
        models.append(m)
    assert steps[2].meters is None
    lm, nm = [_AverageMeter(), _AverageMeter()], [_AverageMeter(), _AverageMeter()]
    g = torch.Generator().manual_seed(11)
    for it in range(5 * accum):
        x = torch.randn(8, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
        y = (torch.rand(8, 4, generator=g) > 0.6).float().to(gpu)
        for k, st in enumerate(steps):
            loss = st.step(x, y)
            if k < 2:
                lm[k].update(float(loss) * accum, y.shape[0])
                if (it + 1) % accum == 0:
                    nm[k].update(float(st.last_norm))
    assert steps[1]._g1 is not None and steps[1]._g_opt is not None
    for k in range(2):
        v = steps[k].meters.values()
        print(f'accum {accum} graph {bool(k)}: loss {v["loss"]} want ({lm[k].val}, {lm[k].avg}); norm {v["grad_norm"]} want ({nm[k].val}, {nm[k].avg})')
        for got, want in ((v['loss'].val, lm[k].val), (v['loss'].avg, lm[k].avg), (v['grad_norm'].val, nm[k].val), (v['grad_norm'].avg, nm[k].avg)):
            assert abs(got - want) <= 1e-12 * abs(want), (k, got, want)
        assert v['nonfinite'] == 0
        total = torch.tensor([lm[k].sum, lm[k].count], dtype=torch.float32).tolist()
        assert steps[k].meters.all_reduce() == total[0] / total[1]
    for other in (1, 2):                                 # metering changes nothing that is trained, eagerly or in replay
        for (n, p), (_, q) in zip(models[0].named_parameters(), models[other].named_parameters()):
            assert torch.equal(p, q), n
    steps[1].meters.reset()
    assert steps[1].meters.values()['loss'] == (0.0, 0.0)
