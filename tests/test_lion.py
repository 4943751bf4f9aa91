"""CPU: optim.FlatLion's constructor and checkpoint loading, engine.build_optimizer's refusal off the HIP path, the Lion entries of the C
ABI, the host build of the update body (tools/lion_host_check.cpp) under the address and undefined-behaviour sanitizers, and the
condition under which tests/lion_cases.py's fp64 restatement may be compared with an fp32 computation at all: how many of the bag's
elements ever come near a tie of the sign, and that fp32 and fp64 agree on every sign elsewhere."""
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import lion_cases as nc
from test_abi import _ensure_built

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the constructor ----------------------------------------------------------------------------------------------------------------
def test_flat_lion_constructor_checks(vited):
    p = [torch.nn.Parameter(torch.zeros(3, 3))]
    for kw, match in ((dict(lr=-1.0), 'Invalid learning rate: -1.0'), (dict(betas=(1.0, 0.9)), 'Invalid beta parameter at index 0: 1.0'),
                      (dict(betas=(0.9, -0.1)), 'Invalid beta parameter at index 1: -0.1'),
                      (dict(weight_decay=-0.1), 'Invalid weight_decay value: -0.1'), (dict(ema_decay=1.0), 'ema_decay')):
        with pytest.raises(ValueError, match=match):
            vited.optim.FlatLion(p, **kw)
    with pytest.raises(ValueError, match='FlatLion does not support maximize=True'):
        vited.optim.FlatLion([{'params': p, 'maximize': True}])
    opt = vited.optim.FlatLion(p)
    assert opt.defaults == dict(lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0, foreach=None, maximize=False)
    assert isinstance(opt, vited.optim._FlatOptimizer) and not isinstance(opt, vited.optim._FlatAdamMoments)
    assert opt._entry == 'vited_lion_step' and opt._state_names == ('exp_avg',) and opt._state_at_bind
    assert opt.num_updates == 0 and opt.skipped_updates == 0 and opt.exp_avg is None
    assert opt.state_dict()['state'] == {} and len(opt.state) == 0                         # empty before bind
    opt = vited.optim.FlatLion([{'params': p, 'weight_decay': 0.3}], lr=3e-4, betas=(0.95, 0.98), weight_decay=0.1)
    assert opt._group_words(opt.param_groups[0]) == [3e-4, 0.95, 0.98, 0.0, 0.3, 0.0, 0.0, 0.0]
    assert opt.hyper_lr_words() == (8, 8)                                        # the rate sits where the schedules and the range test write
    opt.param_groups[0]['maximize'] = True
    with pytest.raises(ValueError, match='maximize=True'):
        opt._group_words(opt.param_groups[0])
    opt.param_groups[0]['maximize'] = False
    with pytest.raises(RuntimeError, match='no CPU path'):
        opt.bind_flat(vited.engine.FlatGradients(p))
    with pytest.raises(RuntimeError, match='bind_flat'):
        opt.step_flat(1.0)
    with pytest.raises(RuntimeError, match='bind_flat'):                         # accepted as a fused optimizer: only the binding is missing
        vited.engine.LRRangeTest(opt, 10)


def _with_adam_state(opt, step=3.0):
    for i, q in enumerate(p for g in opt.param_groups for p in g['params']):
        opt.state[q] = dict(step=torch.tensor(step), exp_avg=torch.full_like(q, 0.25 + i), exp_avg_sq=torch.full_like(q, 0.5))
    return opt


def test_an_adamw_checkpoint_loads_and_leaves_only_exp_avg(vited):
    shapes = [(3, 3), (5,)]
    for source in (lambda ps: torch.optim.AdamW(ps, lr=1e-3, weight_decay=0.05), lambda ps: vited.optim.FlatAdamW(ps, lr=1e-3, weight_decay=0.05),
                   lambda ps: vited.optim.FlatLAMB(ps, lr=1e-3, weight_decay=0.05)):
        saved = _with_adam_state(source([torch.nn.Parameter(torch.zeros(s)) for s in shapes])).state_dict()
        assert set(saved['state'][0]) >= {'exp_avg', 'exp_avg_sq', 'step'}
        ps = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
        opt = vited.optim.FlatLion(ps, lr=1e-4, weight_decay=0.5)
        opt.load_state_dict(saved)
        assert [set(opt.state[q]) for q in ps] == [{'exp_avg'}, {'exp_avg'}]
        assert all(bool((opt.state[q]['exp_avg'] == 0.25 + i).all()) and opt.state[q]['exp_avg'].shape == q.shape for i, q in enumerate(ps))
        sd = opt.state_dict()                                                               # timm Lion's layout: exp_avg, no step
        assert set(sd['state']) == {0, 1} and all(set(st) == {'exp_avg'} for st in sd['state'].values())
        g = opt.param_groups[0]
        assert g['lr'] == 1e-3 and g['weight_decay'] == 0.05 and g['maximize'] is False and g['foreach'] is None
        assert opt._group_words(g)[:5] == [1e-3, 0.9, 0.999, 0.0, 0.05] and opt.num_updates == 0
        again = vited.optim.FlatLion([torch.nn.Parameter(torch.zeros(s)) for s in shapes])  # and its own state_dict goes round
        again.load_state_dict(sd)
        assert all(torch.equal(a['exp_avg'], b['exp_avg']) for a, b in zip(again.state_dict()['state'].values(), sd['state'].values()))
    saved['param_groups'][0]['maximize'] = True
    with pytest.raises(ValueError, match='maximize=True'):
        vited.optim.FlatLion([torch.nn.Parameter(torch.zeros(s)) for s in shapes]).load_state_dict(saved)


# ---- build_optimizer ----------------------------------------------------------------------------------------------------------------
def _config(name):
    opt = types.SimpleNamespace(NAME=name, EPS=1e-6, BETAS=(0.9, 0.99), MOMENTUM=0.9)
    return types.SimpleNamespace(TRAIN=types.SimpleNamespace(OPTIMIZER=opt, BASE_LR=1e-4, WEIGHT_DECAY=0.5))


@pytest.mark.parametrize('name', ['lion', 'Lion', 'LION'])
def test_build_optimizer_has_no_lion_for_a_cpu_model(vited, name):
    model = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.LayerNorm(4))
    for kw in (dict(), dict(fused_hip=False), dict(fused_hip=True)):
        with pytest.raises(ValueError, match='unknown optimizer lion .*HIP optimizer only'):
            vited.engine.build_optimizer(_config(name), model, **kw)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_lion_entry_points_are_declared_bound_exported_and_check_their_arguments(vited):
    _ensure_built(vited)
    sig = vited._lib.SIGNATURES
    assert sig['vited_lion_step'] == sig['vited_adamw_step'] and sig['vited_lion_step_ema'] == sig['vited_adamw_step_ema']
    out = subprocess.run(['nm', '-D', '--defined-only', vited._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if ' T ' in l}
    assert {'vited_lion_step', 'vited_lion_step_ema'} <= exported
    lib = vited._lib.load()
    BAD_ARG, WORKSPACE = 1, 4                                                       # VITED_ERR_BAD_ARG, VITED_ERR_WORKSPACE
    need = lib.vited_adamw_workspace_bytes()
    # validated before any launch: no pointer below is ever dereferenced
    assert lib.vited_lion_step(None, 1, 1, 1, 1, 1, 0.0, 0, None, 1, need, None) == BAD_ARG            # a null table
    assert lib.vited_lion_step(1, 0, 1, 1, 1, 1, 0.0, 0, None, 1, need, None) == BAD_ARG               # no rows
    assert lib.vited_lion_step(1, 1, 0, 1, 1, 1, 0.0, 0, None, 1, need, None) == BAD_ARG               # no tiles
    assert lib.vited_lion_step(1, 1, 1, 1, 1, 1, 0.0, 0, None, None, need, None) == BAD_ARG            # no workspace
    assert lib.vited_lion_step(1, 1, 1, 1, 1, 1, 0.0, 0, None, 1, need - 4, None) == WORKSPACE         # a short one
    assert lib.vited_lion_step_ema(None, 1, 1, 1, 1, 1, 0.0, 0, None, 1, need, 16, 1, None) == BAD_ARG
    assert lib.vited_lion_step_ema(1, 1, 1, 1, 1, 1, 0.0, 0, None, 1, need, None, 1, None) == BAD_ARG  # no average
    assert lib.vited_lion_step_ema(1, 1, 1, 1, 1, 1, 0.0, 0, None, 1, need, 20, 1, None) == BAD_ARG    # not 16-byte aligned
    assert lib.vited_lion_step_ema(1, 1, 1, 1, 8, 1, 0.0, 0, None, 1, need, 16, 4, None) == BAD_ARG    # shorter than the gradients
    assert lib.vited_lion_step_ema(1, 1, 1, 1, 1, 1, 0.0, 0, None, 1, need - 4, 16, 1, None) == WORKSPACE
    text = open(os.path.join(ROOT, 'vit-ed_amd', 'csrc', 'optim_update.h')).read()
    for name in ('lion_coef', 'lion_piece'):
        assert re.search(r'\b%s\s*\(' % name, text), name
    assert re.search(r'\bstruct\s+LionCoef\b', text)


# ---- the update body on the host, under the sanitizers ------------------------------------------------------------------------------
def test_update_body_under_the_sanitizers(tmp_path):
    """tools/lion_host_check.cpp compiles csrc/optim_update.h for the host - the text the kernel runs - and drives lion_piece over
    exactly-sized heap blocks against a second scalar statement, bit for bit: a stand-alone program with its own main."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    cxx = next((c for c in (shutil.which('clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'))
                if c and os.path.exists(c)), None)
    assert cxx is not None, 'no clang++ beside hipcc: the HIP toolchain that builds the library ships one'
    exe = str(tmp_path / 'lion_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off', '-I',
                    os.path.join(ROOT, 'vit-ed_amd', 'csrc'), os.path.join(ROOT, 'tools', 'lion_host_check.cpp'), '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r'lion_host_check ok: \d+ cases', out.stdout), out.stdout[-2000:] + out.stderr[-2000:]


# ---- the restatement and the condition of its fp64 comparison -----------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs():
    return nc.run(torch.float64), nc.run(torch.float32)


def test_the_restatement_is_lion(runs):
    """Against the rule written the way timm's ``Lion`` applies it (mul_, lerp_, add_ with alpha), in fp64: roundings of 2^-53 apart."""
    p = [t.double() for t in nc.lc.initial_parameters()]
    m = [torch.zeros_like(t) for t in p]
    for step, rec in enumerate(runs[0]):
        g = [t.double() for t in nc.lc.gradients(step)]
        norm = torch.sqrt(sum((t ** 2).sum() for t in g))
        c = min(1.0, nc.MAX_NORM / (float(norm) + 1e-6))
        assert abs(float(norm) - rec['norm']) <= 1e-12 * rec['norm']
        for i in range(len(p)):
            s = nc.group_settings(nc.GROUP_OF[i])
            grad = g[i] * c
            p[i].mul_(1 - s['lr'] * s['weight_decay'])
            p[i].add_(torch.sign(m[i].mul(s['betas'][0]).add_(grad, alpha=1 - s['betas'][0])), alpha=-s['lr'])
            m[i].lerp_(grad, 1 - s['betas'][1])
            torch.testing.assert_close(rec['p'][i], p[i], rtol=0, atol=1e-15, msg=lambda t: f'update {step} p {nc.SHAPES[i]}: {t}')
            torch.testing.assert_close(rec['m'][i], m[i], rtol=1e-12, atol=1e-18)


def test_the_bag_exercises_what_it_claims(runs):
    f64 = runs[0]
    assert [rec['norm'] > nc.MAX_NORM for rec in f64] == [False, True, False, True, False]      # the clip bites in updates 1 and 3
    kind = {k: nc.KINDS.index(k) for k in ('zero_p', 'zero_g', 'zero_both')}
    start = nc.lc.initial_parameters()
    for n, rec in enumerate(f64):
        s = nc.group_settings(nc.GROUP_OF[kind['zero_g']])
        want = start[kind['zero_g']].double() * (1 - s['lr'] * s['weight_decay']) ** (n + 1)    # no gradient: the parameter only decays
        torch.testing.assert_close(rec['p'][kind['zero_g']], want, rtol=1e-12, atol=0)
        assert float(rec['m'][kind['zero_g']].abs().max()) == 0.0
        assert float(rec['p'][kind['zero_both']].abs().max()) == 0.0
        assert all(bool(torch.isfinite(t).all()) for t in rec['p'] + rec['m'])
    lr = nc.group_settings(nc.GROUP_OF[kind['zero_p']])['lr']
    assert bool((f64[0]['p'][kind['zero_p']].abs() == lr).all())                                # p = 0 under a gradient: one step of lr
    assert nc.TOTAL == 13446 and sorted(set(nc.GROUP_OF)) == [0, 1, 2] and nc.HYPER['betas'] == (0.9, 0.98)


def test_few_elements_come_near_a_tie_and_the_signs_agree_elsewhere(runs):
    """The condition of the fp64 comparison (tests/lion_cases.py).  Measured on this bag: no element of the 13,446 is ever near a tie - the closest |cc| is 3.7e-5 of its
    scale against the 1.5e-5 of 2^-16 - fp32 and fp64 never disagree on a sign, and the parameters are at most 2.8e-8 apart."""
    f64, f32 = runs
    near = nc.near_tie(f64)
    count = sum(int(t.sum()) for t in near)
    closest = min(float((rec['cc'][i].abs() / rec['scale'][i])[rec['cc'][i] != 0].min()) for rec in f64 for i in range(len(nc.BAG))
                  if bool((rec['cc'][i] != 0).any()))
    print(f'near a tie: {count} of {nc.TOTAL} elements ({100.0 * count / nc.TOTAL:.3f} %); the closest |cc| / scale is {closest:.3e} (2^-16 = {nc.TIE:.3e})')
    assert count <= nc.TIE_SHARE * nc.TOTAL
    disagree = 0
    for a, b in zip(f64, f32):
        for i in range(len(nc.BAG)):
            differ = torch.sign(a['cc'][i]) != torch.sign(b['cc'][i].double())
            disagree += int(differ.sum())
            assert not bool((differ & ~near[i]).any()), (nc.SHAPES[i], 'fp32 and fp64 take different signs away from any tie')
    print(f'sign disagreements between fp32 and fp64, all updates: {disagree}')
    worst = max(float(((a['p'][i] - b['p'][i].double()).abs())[~near[i]].max()) for a, b in zip(f64, f32) for i in range(len(nc.BAG))
                if bool((~near[i]).any()))
    print(f'worst |p32 - p64| away from ties: {worst:.2e}')
    assert worst <= 1e-7                         # two half-ulp roundings per update at |p| < 0.25, over 5 updates: 7.5e-8
