"""CPU: LAMB's restatement (tests/lamb_cases.py) against two facts that do not depend on it, what the parameter bag exercises, the LAMB
entries of the C ABI, FlatLAMB's constructor, engine.build_optimizer's refusal off the HIP path, and the host build of the update bodies
(tools/lamb_host_check.cpp) under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import lamb_cases as lc
from test_abi import _ensure_built

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_without_decay_the_restatement_is_torch_adamw_step_for_step():
    """wd = 0 and always_adapt=False: r = 1 everywhere, and LAMB is AdamW without decay.  In fp64 the two statements differ by roundings
    of 2^-53 only."""
    runs = lc.run(torch.float64, weight_decay=0.0)
    ref = [torch.nn.Parameter(t.double()) for t in lc.initial_parameters()]
    topt = torch.optim.AdamW(lc.param_groups(ref, weight_decay=0.0), **{**lc.HYPER, 'weight_decay': 0.0})
    for step, rec in enumerate(runs):
        for q, g in zip(ref, lc.gradients(step)):
            q.grad = g.double()
        norm = torch.nn.utils.clip_grad_norm_(ref, lc.MAX_NORM)
        topt.step()
        assert abs(float(norm) - rec['norm']) <= 1e-12 * rec['norm']
        assert rec['r'] == [1.0] * len(ref)
        for i, q in enumerate(ref):
            torch.testing.assert_close(rec['p'][i], q.detach(), rtol=1e-12, atol=1e-15, msg=lambda m: f'update {step} p {lc.SHAPES[i]}: {m}')
            torch.testing.assert_close(rec['m'][i], topt.state[q]['exp_avg'], rtol=1e-12, atol=1e-18)
            torch.testing.assert_close(rec['v'][i], topt.state[q]['exp_avg_sq'], rtol=1e-12, atol=1e-24)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_with_always_adapt_every_tensor_moves_by_lr_times_its_norm(dtype):
    """p' - p = -lr r u with r = |p| / |u|, so |p' - p| = lr |p| wherever both norms are non-zero - whatever m, v and the clip were."""
    runs = lc.run(dtype, always_adapt=True)
    before = [t.to(dtype) for t in lc.initial_parameters()]
    tol = 1e-12 if dtype == torch.float64 else 2e-5            # fp32: p' - p cancels; |p| 0.1, lr 2e-3, so 2^-24 * 0.1 / 2e-4 per element
    checked = 0
    for rec in runs:
        for i, p in enumerate(rec['p']):
            lr = lc.group_settings(lc.GROUP_OF[i])['lr']
            pn, moved = float(before[i].double().norm()), float((p.double() - before[i].double()).norm())
            if pn > 0 and lc.KINDS[i] != 'zero_both':
                assert abs(moved - lr * pn) <= tol * lr * pn, (lc.SHAPES[i], moved, lr * pn)
                checked += 1
        before = rec['p']
    assert checked >= lc.UPDATES * (len(lc.BAG) - 2)


def test_the_bag_exercises_what_it_claims():
    runs = lc.run(torch.float64)
    clipped = [rec['norm'] > lc.MAX_NORM for rec in runs]
    assert clipped == [False, True, False, True, False]                         # the clip bites in some updates and not in others
    kind = {k: lc.KINDS.index(k) for k in ('zero_p', 'zero_g', 'zero_both')}
    wd = lc.HYPER['weight_decay']
    assert runs[0]['r'][kind['zero_p']] == 1.0 and runs[1]['r'][kind['zero_p']] != 1.0          # |p| = 0 in the first update only
    for rec in runs:
        assert abs(rec['r'][kind['zero_g']] - 1.0 / wd) <= 1e-12 / wd                           # u = wd p
        assert rec['r'][kind['zero_both']] == 1.0 and float(rec['p'][kind['zero_both']].abs().max()) == 0.0
        assert all(r == 1.0 for r, g in zip(rec['r'], lc.GROUP_OF) if g == 1)                   # the undecayed group is not adapted
        assert all(r != 1.0 for r, g, k in zip(rec['r'], lc.GROUP_OF, lc.KINDS) if g != 1 and k == 'plain')
        assert all(bool(torch.isfinite(t).all()) for t in rec['p'] + rec['m'] + rec['v'])
    assert any(r > 1.0 for rec in runs for r in rec['r']) and all(r <= 1.0 for rec in lc.run(trust_clip=True) for r in rec['r'])
    assert all(r != 1.0 for r, g in zip(lc.run(always_adapt=True)[0]['r'], lc.GROUP_OF) if g == 1)
    tiles = [((s[0] if len(s) > 1 else 1) + 63) // 64 * ((lc.NUMEL[i] // (s[0] if len(s) > 1 else 1)) + 63) // 64 for i, s in enumerate(lc.SHAPES)]
    assert max(tiles) == 4 and sorted(set(lc.GROUP_OF)) == [0, 1, 2]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_lamb_entry_points_are_declared_bound_and_exported(vited):
    _ensure_built(vited)
    sig = vited._lib.SIGNATURES
    assert sig['vited_lamb_step'] == sig['vited_adamw_step'] and sig['vited_lamb_step_ema'] == sig['vited_adamw_step_ema']
    out = subprocess.run(['nm', '-D', '--defined-only', vited._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if ' T ' in l}
    assert {'vited_lamb_step', 'vited_lamb_step_ema', 'vited_lamb_workspace_bytes'} <= exported
    lib = vited._lib.load()
    assert lib.vited_lamb_step(None, 0, 0, None, 0, None, 0.0, 0, None, None, 0, None) == 1      # validated before any launch
    assert lib.vited_lamb_step_ema(None, 0, 0, None, 0, None, 0.0, 0, None, None, 0, None, 0, None) == 1
    # AdamW's words, then ratio[count], then two sums per tile; ratio begins where optim.LAMB_RATIO_AT says
    assert lib.vited_lamb_workspace_bytes(7, 3) == lib.vited_adamw_workspace_bytes() + (3 + 2 * 7) * 4
    assert vited.optim.LAMB_RATIO_AT * 4 == lib.vited_adamw_workspace_bytes()
    assert lib.vited_lamb_workspace_bytes(0, 3) == 0 and lib.vited_lamb_workspace_bytes(7, 0) == 0
    text = open(os.path.join(ROOT, 'vit-ed_amd', 'csrc', 'optim_update.h')).read()
    for name in ('lamb_coef', 'lamb_u', 'lamb_ratio', 'lamb_moments_piece', 'lamb_apply_piece'):
        assert re.search(r'\b%s\s*\(' % name, text), name


# ---- the constructor and build_optimizer --------------------------------------------------------------------------------------------
def test_flat_lamb_constructor_checks(vited):
    p = [torch.nn.Parameter(torch.zeros(3, 3))]
    for kw, match in ((dict(lr=-1.0), 'learning rate'), (dict(eps=-1e-6), 'epsilon'), (dict(betas=(1.0, 0.9)), 'beta'),
                      (dict(betas=(0.9, -0.1)), 'beta'), (dict(weight_decay=-0.1), 'weight_decay'), (dict(ema_decay=1.0), 'ema_decay')):
        with pytest.raises(ValueError, match=match):
            vited.optim.FlatLAMB(p, **kw)
    opt = vited.optim.FlatLAMB(p)
    assert opt.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, always_adapt=False, trust_clip=False)
    assert isinstance(opt, vited.optim._FlatOptimizer) and not isinstance(opt, vited.optim.FlatAdamW)
    assert opt._state_names == ('exp_avg', 'exp_avg_sq') and opt._entry == 'vited_lamb_step'
    assert opt.num_updates == 0 and opt.skipped_updates == 0 and opt.state_dict()['state'] == {}
    opt = vited.optim.FlatLAMB([{'params': p, 'trust_clip': True}], lr=3e-3, betas=(0.8, 0.9), eps=1e-5, weight_decay=0.05, always_adapt=True)
    assert opt._group_words(opt.param_groups[0]) == [3e-3, 0.8, 0.9, 1e-5, 0.05, 1.0, 1.0, 0.0]
    assert opt.hyper_lr_words() == (8, 8)                                        # the rate sits where the schedules and the range test write
    with pytest.raises(RuntimeError, match='bind_flat'):
        opt.trust_ratios()
    with pytest.raises(RuntimeError, match='no CPU path'):
        opt.bind_flat(vited.engine.FlatGradients(p))
    # a FlatAdamW checkpoint loads (the groups take LAMB's own flags) and goes back
    adamw = vited.optim.FlatAdamW([torch.nn.Parameter(torch.zeros(3, 3))], lr=1e-3)
    opt.load_state_dict(adamw.state_dict())
    assert opt.param_groups[0]['always_adapt'] is True and opt.param_groups[0]['trust_clip'] is False and opt.param_groups[0]['lr'] == 1e-3
    adamw.load_state_dict(opt.state_dict())


def _config(name):
    opt = types.SimpleNamespace(NAME=name, EPS=1e-6, BETAS=(0.9, 0.999), MOMENTUM=0.9)
    return types.SimpleNamespace(TRAIN=types.SimpleNamespace(OPTIMIZER=opt, BASE_LR=1e-3, WEIGHT_DECAY=0.05))


@pytest.mark.parametrize('name', ['lamb', 'fused_lamb', 'LAMB'])
def test_build_optimizer_has_no_lamb_for_a_cpu_model(vited, name):
    model = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.LayerNorm(4))
    for kw in (dict(), dict(fused_hip=False), dict(fused_hip=True)):
        with pytest.raises(ValueError, match='unknown optimizer'):
            vited.engine.build_optimizer(_config(name), model, **kw)


def test_range_test_still_refuses_torch_optimizers(vited):
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(NotImplementedError, match='optim.FlatLAMB / optim.FlatAdamW / optim.FlatSGD; Adam has none'):
        vited.engine.LRRangeTest(torch.optim.Adam(p, lr=1e-3), 10)
    lamb = vited.optim.FlatLAMB(p)
    with pytest.raises(RuntimeError, match='bind_flat'):                         # accepted as a fused optimizer: only the binding is missing
        vited.engine.LRRangeTest(lamb, 10)


# ---- the update bodies on the host, under the sanitizers ----------------------------------------------------------------------------
def test_update_bodies_under_the_sanitizers(tmp_path):
    """tools/lamb_host_check.cpp compiles csrc/optim_update.h for the host - the text the kernels run - and drives LAMB's three passes
    over exactly-sized buffers against a double-precision loop: a stand-alone program with its own main."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    cxx = next((c for c in (shutil.which('clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'))
                if c and os.path.exists(c)), None)
    assert cxx is not None, 'no clang++ beside hipcc: the HIP toolchain that builds the library ships one'
    exe = str(tmp_path / 'lamb_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                    os.path.join(ROOT, 'vit-ed_amd', 'csrc'), os.path.join(ROOT, 'tools', 'lamb_host_check.cpp'), '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and 'lamb_host_check ok' in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
