"""The device-stepped learning-rate schedule on the GPU (vited_lr_schedule_step, lr_scheduler.py): the kernel
alone over the whole case table, and through ``engine.TrainStep`` - eager, replayed, with accumulation and skipped updates, resumed
and re-bound.

Tolerance (tests/lr_schedule_cases.py: ``fp32_matches``): in the warm-up and linear branches and in cosine's constant tail the rate
words equal Python's value rounded to fp32 exactly - IEEE fp64 + - * / round identically on both sides; in the cos and pow branches
they may be the neighbouring fp32 value, because the device's fp64 cos / pow are a few fp64 ulp off libm's, which can only move a value
across a rounding boundary.  Runs of the same kernels against each other (graph against eager, resumed against uninterrupted) are
compared bit for bit."""
import copy

import pytest
import torch

import lr_schedule_cases as lc
from oracle import vited_oracle as vo
from test_gpu_engine import _hip_model

pytestmark = pytest.mark.gpu
HEADER, WORDS = 8, 8                     # the hyper array: 8 header words, 8 per group, the rate first


class _Recorded:
    """A host scheduler that only has step_update (the engine's host-stepped path): writes rates recorded elsewhere."""

    def __init__(self, opt, rates):
        self.opt, self.rates = opt, rates

    def step_update(self, n):
        for g, lr in zip(self.opt.param_groups, self.rates[n]):
            g['lr'] = lr


def _rate_words(opt):
    return opt._hyper[HEADER::WORDS].tolist()


def _check_rates(case, got, t, where):
    want = lc.group_rates(case, t) if t >= 0 else lc.initial_rates(case)
    for g, (a, b) in enumerate(zip(got, want)):
        assert lc.fp32_matches(a, b, t < 0 or lc.exact_branch(case, t)), (where, case['id'], t, g, a, b)


@pytest.fixture(scope='module')
def shape():
    return vo.ViTEDShape(depth=1, c_depth=1)


@pytest.fixture(scope='module')
def init(vited, gpu, shape):
    torch.manual_seed(11)
    return _hip_model(vited, shape, gpu, None).state_dict()


def _batches(n, gpu, nan_at=None):
    g = torch.Generator().manual_seed(21)
    out = []
    for it in range(n):
        x = torch.randn(8, 2, 3, 64, 64, generator=g).clamp(-1, 1)
        y = (torch.rand(8, 4, generator=g) > 0.6).float()
        if it == nan_at:
            x[3, 0, 1, 17, 5] = float('nan')
        out.append((x.to(gpu), y.to(gpu)))
    return out


def _setup(vited, gpu, shape, init, case, *, kind='adamw', on_device=None, scheduler='build', state=None, **step_kw):
    """model, optimizer, scheduler and TrainStep on the shared initial weights; ``scheduler``: 'build' (build_scheduler on the case) or
    a callable opt -> host scheduler (the groups are still initialised by the case's schedule); ``state``: (optimizer, scheduler)
    state_dicts to load before the TrainStep is built (the reference's resume order)."""
    m = _hip_model(vited, shape, gpu, None)
    m.load_state_dict(init if state is None else state[2])
    groups = vited.engine.param_groups_no_decay_1d(m)
    groups[1]['lr_scale'] = lc.LR_SCALES[1]
    skip = step_kw.pop('skip_nonfinite', False)
    if kind == 'adamw':
        opt = vited.optim.FlatAdamW(groups, lr=lc.BASE_LR, weight_decay=0.05, skip_nonfinite=skip)
    else:
        opt = vited.optim.FlatSGD(groups, lr=lc.BASE_LR, momentum=0.9, nesterov=True, weight_decay=0.05, skip_nonfinite=skip)
    sched = vited.engine.build_scheduler(lc.config(case), opt, lc.N_ITER, step_warmup_prefix=case['step_warmup_prefix'])
    if on_device is not None:
        sched.on_device = on_device
    if state is not None:
        opt.load_state_dict(state[0])
        sched.load_state_dict(state[1])
    used = sched if scheduler == 'build' else scheduler(opt)
    step = vited.engine.TrainStep(m, opt, clip_grad=5.0, lr_scheduler=used, **step_kw)
    return m, opt, sched, step


# ---- G1: the kernel alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['adamw', 'sgd'])
def test_kernel_follows_the_case_table_and_touches_nothing_else(vited, gpu, layout):
    ops = vited.ops
    f64, words = torch.float64, {'adamw': [0., 0.9, 0.999, 1e-8, 0.05, 0., 0., 0.], 'sgd': [0., 0.9, 1.0, 0., 0.05, 0., 0., 0.]}[layout]
    p = [[torch.nn.Parameter(torch.zeros(3))], [torch.nn.Parameter(torch.zeros(2))]]
    base = torch.tensor([lc.BASE_LR, lc.BASE_LR], dtype=f64, device=gpu)
    scale = torch.tensor([1.0, lc.LR_SCALES[1]], dtype=f64, device=gpu)
    for case in lc.CASES:
        sched = vited.lr_scheduler.build_scheduler(lc.config(case), torch.optim.SGD(lc.group_specs(p), lr=lc.BASE_LR), lc.N_ITER,
                                                   step_warmup_prefix=case['step_warmup_prefix'])
        table = torch.tensor(sched._table_words(), dtype=f64, device=gpu)
        hyper = torch.tensor([17., 1., 3., 0., 0., 0., 0., 0.] + [-1.] + words[1:] + [-2.] + words[1:4] + [0.] + words[5:], device=gpu)
        before = hyper.view(torch.int32).clone()
        rate = torch.zeros(HEADER + 2 * WORDS, dtype=torch.bool, device=gpu)
        rate[HEADER::WORDS] = True
        counter = torch.zeros(1, dtype=torch.int64, device=gpu)
        last = torch.full((2,), -3., device=gpu)
        for t in lc.T_VALUES:
            if t >= 40:
                counter.fill_(t)
            mirror = last if t % 2 == 0 else None                    # the mirror is optional
            if mirror is None:
                last.fill_(-3.)
            ops.lr_schedule_step(table, base, scale, counter, hyper, HEADER, WORDS, mirror)
            assert int(counter) == t + 1, (case['id'], t)
            got = hyper[HEADER::WORDS].tolist()
            _check_rates(case, got, t, 'kernel')
            assert last.tolist() == (got if mirror is not None else [-3., -3.]), (case['id'], t)
            assert torch.equal(hyper.view(torch.int32)[~rate], before[~rate]), (case['id'], t)      # header, betas, eps, decay: same bits
    with pytest.raises(ValueError, match='lr_schedule_step: dst'):
        ops.lr_schedule_step(table, base, scale, counter, hyper[:16], HEADER, WORDS)               # the second group's word is outside
    with pytest.raises(ValueError, match='lr_schedule_step: table'):
        ops.lr_schedule_step(table[:40], base, scale, counter, hyper, HEADER, WORDS)
    with pytest.raises(ValueError, match='lr_schedule_step: scale'):
        ops.lr_schedule_step(table, base, scale.float(), counter, hyper, HEADER, WORDS)


# ---- G2: eager TrainStep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,case_id', [('adamw', 'cosine_prefix_warm2'), ('adamw', 'cosine_prefix_warm0'), ('sgd', 'cosine_noprefix_warm0')])
def test_eager_step_consumes_what_the_kernel_wrote(vited, gpu, shape, init, kind, case_id):
    case, data = lc.BY_ID[case_id], _batches(8, gpu)
    m, opt, sched, step = _setup(vited, gpu, shape, init, case, kind=kind, amp=True)
    assert step.lr_on_device and sched.attached()
    recorded = []
    for n, (x, y) in enumerate(data):
        assert [g['lr'] for g in opt.param_groups] == (lc.group_rates(case, n - 1) if n else lc.initial_rates(case))
        step.step(x, y)
        got = _rate_words(opt)
        _check_rates(case, got, n, 'eager')
        assert sched.device_rates == got and sched.device_update == n + 1 == step.num_updates
        assert [g['lr'] for g in opt.param_groups] == lc.group_rates(case, n)           # the host mirror, in Python floats
        recorded.append(got)
    assert opt.hyper_uploads == 1 and opt.num_updates == 8
    assert opt.state_dict()['param_groups'][1]['lr'] == lc.group_rates(case, 7)[1]
    # the same run, host-stepped with the recorded device values: the update consumed exactly what the kernel wrote
    m2, opt2, _, step2 = _setup(vited, gpu, shape, init, case, kind=kind, amp=True, scheduler=lambda o: _Recorded(o, recorded))
    assert not step2.lr_on_device
    for x, y in data:
        step2.step(x, y)
    assert opt2.hyper_uploads > 1
    for (name, a), (_, b) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), name
    assert not torch.equal(m.head.weight, init['head.weight'])


# ---- G3: replayed -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('amp', [False, True])
def test_graph_replay_steps_the_schedule_like_eager_launches(vited, gpu, shape, init, amp):
    case, data = lc.BY_ID['cosine_prefix_warm0'], _batches(7, gpu)
    runs = [_setup(vited, gpu, shape, init, case, amp=amp, use_graph=ug, on_device=od) for ug, od in ((False, None), (True, None), (True, False))]
    assert [r[3].lr_on_device for r in runs] == [True, True, False]
    rates = [[], [], []]
    for n, (x, y) in enumerate(data):
        losses = [float(r[3].step(x, y)) for r in runs]
        assert losses[0] == losses[1], (n, losses)
        for r, seen in zip(runs, rates):
            seen.append(_rate_words(r[1]))
        _check_rates(case, rates[1][-1], n, 'replayed')
        # host-stepped, the array holds what update n consumed - step_update(n - 1)'s value, uploaded in front of update n - which is
        # what the device-stepped array held after update n - 1: the same schedule, one upload per iteration
        _check_rates(case, rates[2][-1], n - 1, 'host-stepped')
        if n:
            assert all(lc.fp32_matches(a, b, lc.exact_branch(case, n - 1)) for a, b in zip(rates[2][n], rates[1][n - 1])), n
        assert rates[0][-1] == rates[1][-1]
        assert [g['lr'] for g in runs[1][1].param_groups] == lc.group_rates(case, n)
    graph = runs[1][3]
    assert graph._g_opt is not None and graph.recaptures == 0 and runs[1][2].device_update == 7
    assert runs[0][1].hyper_uploads == 1 and runs[1][1].hyper_uploads == 1 and runs[2][1].hyper_uploads > 1
    for (name, a), (_, b) in zip(runs[0][0].named_parameters(), runs[1][0].named_parameters()):
        assert torch.equal(a, b), f'{name}: graph replay differs from eager launches'
    # a caller's set_lr between two replays is uploaded and holds for one update; the schedule step behind it takes over again
    graph.set_lr(3e-4)
    assert runs[1][1].hyper_uploads == 2 and _rate_words(runs[1][1]) == [float(torch.tensor(3e-4)), float(torch.tensor(3e-4 * 0.1))]
    graph.step(*data[0])
    _check_rates(case, _rate_words(runs[1][1]), 7, 'after set_lr')
    assert runs[1][1].hyper_uploads == 2 and graph.recaptures == 0


# ---- G4: the index ----------------------------------------------------------------------------------------------------------------
def test_index_counts_iterations_that_reach_the_update(vited, gpu, shape, init):
    case = lc.BY_ID['linear_warm0']
    m, opt, sched, step = _setup(vited, gpu, shape, init, case, amp=True, accumulation_steps=2)
    for call, (x, y) in enumerate(_batches(6, gpu)):
        step.step(x, y)
        done = (call + 1) // 2
        assert sched.device_update == done == step.num_updates
        if done:                                                     # the array is filled by the first update's upload
            _check_rates(case, _rate_words(opt), done - 1, 'accumulation')
    assert opt.num_updates == 3 and opt.hyper_uploads == 1
    m, opt, sched, step = _setup(vited, gpu, shape, init, case, amp=True, skip_nonfinite=True)
    for n, (x, y) in enumerate(_batches(4, gpu, nan_at=2)):
        step.step(x, y)
        _check_rates(case, _rate_words(opt), n, 'skipped update')
    assert sched.device_update == 4 == step.num_updates and opt.num_updates == 3 and opt.skipped_updates == 1
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


# ---- G5: resume -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case_id', ['cosine_prefix_warm2', 'cosine_prefix_warm0', 'step_noprefix_warm0'])
@pytest.mark.parametrize('use_graph', [False, True])
def test_resumed_run_continues_bit_for_bit(vited, gpu, shape, init, use_graph, case_id):
    """In the warm-up (the first case) the host's rate in the optimizer's state_dict is bit for bit the kernel's.  In the cos and pow
    branches (the other two) it may be the fp32 neighbour, so ``attach`` derives the resumed run's first rate again on the device, by
    one launch at ``start_update - 1``: the array then holds what the uninterrupted run's held, whichever branch."""
    case, data = lc.BY_ID[case_id], _batches(8, gpu)
    m, opt, sched, step = _setup(vited, gpu, shape, init, case, amp=True, use_graph=use_graph)
    whole, state = [], None
    for n, (x, y) in enumerate(data):
        step.step(x, y)
        whole.append(_rate_words(opt))
        if n == 3:
            state = copy.deepcopy((opt.state_dict(), sched.state_dict(), m.state_dict()))      # the moments are views: the run goes on
    m2, opt2, sched2, step2 = _setup(vited, gpu, shape, init, case, amp=True, use_graph=use_graph, state=state, start_update=4)
    assert opt2.num_updates == 4 and sched2.device_update == 4
    assert _rate_words(opt2) == whole[3] and sched2.device_rates == whole[3]          # the kernel's own value of update 3, again
    for n, (x, y) in enumerate(data[4:], 4):
        step2.step(x, y)
        assert _rate_words(opt2) == whole[n], n
    assert step2.num_updates == 8 == sched2.device_update and opt2.hyper_uploads == 1
    for (name, a), (_, b) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), name
    if use_graph and case_id == 'cosine_prefix_warm2':
        # a captured graph follows a loaded schedule and a moved counter without re-capture: both are copied INTO its buffers
        assert step2._g_opt is not None
        other = dict(sched2.state_dict(), warmup_lr_init=1e-6, warmup_steps=[(lc.BASE_LR - 1e-6) / 10] * 2)
        sched2.load_state_dict(other)
        sched2.attach(opt2, 2)
        step2.num_updates = 2
        step2.step(*data[0])
        want = 1e-6 + 2 * ((lc.BASE_LR - 1e-6) / 10)
        assert _rate_words(opt2) == [float(torch.tensor(want)), float(torch.tensor(want * 0.1))]
        assert step2.recaptures == 0 and sched2.device_update == 3


# ---- G6: re-bind ------------------------------------------------------------------------------------------------------------------
def test_second_trainstep_on_the_same_optimizer_reattaches(vited, gpu, shape, init):
    case, data = lc.BY_ID['multistep_warm2'], _batches(4, gpu)
    m, opt, sched, step = _setup(vited, gpu, shape, init, case, amp=True)
    for x, y in data[:2]:
        step.step(x, y)
    old = opt._hyper
    again = vited.engine.TrainStep(m, opt, clip_grad=5.0, amp=True, lr_scheduler=sched, start_update=step.num_updates)
    assert opt._hyper is not old and again.lr_on_device and sched.device_update == 2
    stale = old.clone()
    for n, (x, y) in enumerate(data[2:], 2):
        again.step(x, y)
        _check_rates(case, _rate_words(opt), n, 're-bound')
        assert sched.device_update == n + 1
    assert torch.equal(old, stale) and opt.num_updates == 4              # nothing wrote to the array of the first binding
    # the first step behind the re-binding ran with the right rate: one TrainStep over the same four batches ends on the same bits
    # (all four updates lie in the warm-up, whose arithmetic is exact on the host and on the device)
    m1, opt1, _, one = _setup(vited, gpu, shape, init, case, amp=True)
    for x, y in data:
        one.step(x, y)
    for (name, a), (_, b) in zip(m.named_parameters(), m1.named_parameters()):
        assert torch.equal(a, b), name
    # groups that hold something else than the schedule's last value (a caller's rate) keep it for the first update
    for g in opt.param_groups:
        g['lr'] = 7e-5
    third = vited.engine.TrainStep(m, opt, clip_grad=5.0, amp=True, lr_scheduler=sched, start_update=4)
    third._sync_lr()
    assert sched.device_update == 4 and _rate_words(opt) == [float(torch.tensor(7e-5))] * 2
