"""CPU: ``lr_scheduler.build_scheduler`` and its four schedules (misc/lr_scheduler.py:16-62 over timm.scheduler)
against the rule written out in tests/lr_schedule_cases.py, on a ``torch.optim.SGD``; the device form's header against Python's own
bits through a stand-alone host program under the sanitizers; the C entry point as far as it goes without a GPU."""
import math
import os
import re
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest
import torch

import lr_schedule_cases as lc
from test_abi import _ensure_built

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _optimizer():
    p = [[torch.nn.Parameter(torch.zeros(3))], [torch.nn.Parameter(torch.zeros(2))]]
    return torch.optim.SGD(lc.group_specs(p), lr=lc.BASE_LR, momentum=0.9)


def _build(vited, case, opt=None):
    return vited.lr_scheduler.build_scheduler(lc.config(case), opt or _optimizer(), lc.N_ITER, step_warmup_prefix=case['step_warmup_prefix'])


def test_build_scheduler_maps_the_config(vited):
    L = vited.lr_scheduler
    assert vited.engine.build_scheduler is L.build_scheduler
    for case in lc.CASES:
        s = _build(vited, case)
        wt = 5 * case['warmup_epochs']
        assert (s.warmup_t, s.warmup_lr_init, s.t_in_epochs) == (wt, lc.WARMUP_LR, False), case['id']
        if case['name'] == 'cosine':
            assert type(s) is L.CosineLRScheduler
            assert (s.t_initial, s.lr_min, s.cycle_limit, s.warmup_prefix) == (30 - wt if case['warmup_prefix'] else 30, lc.MIN_LR, 1,
                                                                               case['warmup_prefix'])
            assert (s.cycle_mul, s.cycle_decay, s.k_decay) == (1, 1, 1)
        elif case['name'] == 'linear':
            assert type(s) is L.LinearLRScheduler and (s.t_initial, s.lr_min_rate) == (30, 0.01)
        elif case['name'] == 'step':
            assert type(s) is L.StepLRScheduler
            assert (s.decay_t, s.decay_rate, s.warmup_prefix) == (5, 0.5, case['step_warmup_prefix'])
        else:
            assert type(s) is L.MultiStepLRScheduler and (s.milestones, s.gamma) == ([15, 25], 0.1)
    cfg = lc.config(lc.CASES[0])
    cfg.TRAIN.LR_SCHEDULER.NAME = 'plateau'
    assert L.build_scheduler(cfg, _optimizer(), 5) is None
    cfg.TRAIN.LR_SCHEDULER.NAME, cfg.TRAIN.EPOCHS, cfg.TRAIN.WARMUP_EPOCHS = 'cosine', 2.5, 0.5       # int() of the products
    s = L.build_scheduler(cfg, _optimizer(), 3)
    assert (s.t_initial, s.warmup_t) == (7 - 1, 1)
    assert L.build_scheduler(lc.config(lc.BY_ID['step_noprefix_warm2']), _optimizer(), 5).warmup_prefix is False      # the default


@pytest.mark.parametrize('case', lc.CASES, ids=lambda c: c['id'])
def test_get_lr_is_the_written_out_rule_bit_for_bit(vited, case):
    s = _build(vited, case)
    for t in lc.T_VALUES:
        got, v = s._get_lr(t), lc.value(case, t)
        assert got == [v, v] and all(type(x) is float for x in got), (case['id'], t, got, v)


def test_cosine_closed_forms(vited):
    s = _build(vited, lc.BY_ID['cosine_prefix_warm2'])
    rel = lambda a, b: abs(a - b) / abs(b)
    assert s._get_lr(0)[0] == lc.WARMUP_LR
    assert rel(s._get_lr(10)[0], lc.BASE_LR) <= 1e-15
    assert rel(s._get_lr(20)[0], (lc.BASE_LR + lc.MIN_LR) / 2) <= 1e-15
    for t in (30, 31, 39, 10 ** 6, 2 ** 33):
        assert s._get_lr(t) == [lc.MIN_LR, lc.MIN_LR]
    L = vited.lr_scheduler
    for kw in (dict(cycle_mul=2.0), dict(k_decay=0.5)):
        with pytest.raises(NotImplementedError):
            L.CosineLRScheduler(_optimizer(), t_initial=10, **kw)
    with pytest.raises(NotImplementedError):
        L.CosineLRScheduler(_optimizer(), t_initial=10, t_in_epochs=True)


def test_linear_reaches_its_floor_at_t_initial_and_goes_on(vited):
    s = _build(vited, lc.BY_ID['linear_warm2'])
    assert abs(s._get_lr(30)[0] - 0.01 * lc.BASE_LR) <= 1e-15 * lc.BASE_LR
    lrs = [s._get_lr(t)[0] for t in range(10, 40)]
    assert all(a > b for a, b in zip(lrs, lrs[1:])) and lrs[-1] < 0.01 * lc.BASE_LR          # no clamp behind t_initial
    assert s._get_lr(10)[0] == lc.BASE_LR


def test_step_halves_and_multistep_changes_at_its_milestones(vited):
    s = _build(vited, lc.BY_ID['step_noprefix_warm0'])
    assert [s._get_lr(t)[0] for t in range(0, 20)] == [lc.BASE_LR * 0.5 ** (t // 5) for t in range(20)]
    shifted, plain = _build(vited, lc.BY_ID['step_prefix_warm2']), _build(vited, lc.BY_ID['step_noprefix_warm2'])
    assert shifted._get_lr(12)[0] == lc.BASE_LR and plain._get_lr(12)[0] == lc.BASE_LR * 0.25
    for t in lc.T_VALUES:                                      # the two choices agree without warm-up
        assert _build(vited, lc.BY_ID['step_prefix_warm0'])._get_lr(t) == s._get_lr(t)
    m = _build(vited, lc.BY_ID['multistep_warm2'])
    lrs = [m._get_lr(t)[0] for t in range(10, 40)]
    changes = [t for t, (a, b) in zip(range(11, 40), zip(lrs, lrs[1:])) if a != b]
    assert changes == [15, 25] and lrs[0] == lc.BASE_LR and lrs[-1] == lc.BASE_LR * 0.1 ** 2
    cfg = lc.config(lc.BY_ID['multistep_warm2'])
    cfg.TRAIN.WARMUP_EPOCHS = 4                                 # warmup_t 20 > the first milestone 15
    with pytest.raises(AssertionError):
        vited.lr_scheduler.build_scheduler(cfg, _optimizer(), 5)


@pytest.mark.parametrize('case', [lc.BY_ID['cosine_prefix_warm2'], lc.BY_ID['multistep_warm0']], ids=lambda c: c['id'])
def test_optimizer_groups_follow_the_schedule(vited, case):
    opt = _optimizer()
    s = _build(vited, case, opt)
    assert [g['lr'] for g in opt.param_groups] == lc.initial_rates(case)
    assert [g['initial_lr'] for g in opt.param_groups] == [lc.BASE_LR, lc.BASE_LR] and s.base_values == [lc.BASE_LR, lc.BASE_LR]
    before = [g['lr'] for g in opt.param_groups]
    s.step(3)
    assert [g['lr'] for g in opt.param_groups] == before          # epochs do not step a per-update schedule
    for n in (0, 7, 12, 26, 33):
        s.step_update(n)
        assert [g['lr'] for g in opt.param_groups] == lc.group_rates(case, n), n
    assert not s.attached() and s.on_device is None
    with pytest.raises(RuntimeError, match='attach'):
        s.step_device()
    with pytest.raises(RuntimeError, match='bind_flat'):
        s.attach(opt)                                                  # a torch optimizer has no device array
    with pytest.raises(ValueError, match='not the optimizer'):
        s.attach(_optimizer())


def test_state_dict_round_trip_and_timm_names(vited):
    case = lc.BY_ID['cosine_prefix_warm2']
    s = _build(vited, case)
    sd = s.state_dict()
    assert 'optimizer' not in sd and not any(torch.is_tensor(v) for v in sd.values())
    assert {'t_initial', 'lr_min', 'cycle_mul', 'cycle_decay', 'cycle_limit', 'warmup_t', 'warmup_lr_init', 'warmup_prefix', 'k_decay',
            'warmup_steps', 'base_values', 't_in_epochs', 'metric', 'param_group_field', '_initial_param_group_field', 'noise_range_t',
            'noise_pct', 'noise_type', 'noise_std', 'noise_seed'} == set(sd)
    other = vited.lr_scheduler.CosineLRScheduler(_optimizer(), t_initial=7, lr_min=1e-3, warmup_t=3, warmup_lr_init=1e-9)
    other.load_state_dict(sd)
    assert other.state_dict() == sd and [other._get_lr(t) for t in lc.T_VALUES] == [s._get_lr(t) for t in lc.T_VALUES]
    # what timm's CosineLRScheduler saves, literally, and a key nobody knows
    timm = {'t_initial': 12, 'lr_min': 1e-6, 'cycle_mul': 1.0, 'cycle_decay': 1.0, 'cycle_limit': 1, 'warmup_t': 4, 'warmup_lr_init': 1e-7,
            'warmup_prefix': False, 'k_decay': 1.0, 'warmup_steps': [(2e-4 - 1e-7) / 4, (2e-4 - 1e-7) / 4], 'base_values': [2e-4, 2e-4],
            't_in_epochs': False, 'metric': None, 'param_group_field': 'lr', '_initial_param_group_field': 'initial_lr',
            'noise_range_t': None, 'noise_pct': 0.67, 'noise_type': 'normal', 'noise_std': 1.0, 'noise_seed': 42, 'from_the_future': 7}
    s.load_state_dict(timm)
    assert s.from_the_future == 7 and s.state_dict()['from_the_future'] == 7 and s.optimizer is not None
    assert s._get_lr(2) == [1e-7 + 2 * ((2e-4 - 1e-7) / 4)] * 2
    assert s._get_lr(6) == [1e-6 + 0.5 * (2e-4 * 1.0 ** 0 - 1e-6) * (1 + math.cos(math.pi * 6 / 12))] * 2
    assert s._get_lr(12) == [1e-6, 1e-6]
    s.step_update(6)
    assert [g['lr'] for g in s.optimizer.param_groups] == [s._get_lr(6)[0], s._get_lr(6)[0] * 0.1]
    s.load_state_dict({'cycle_mul': 2.0})
    with pytest.raises(NotImplementedError):
        s._get_lr(5)


def test_what_the_device_table_can_state(vited):
    L = vited.lr_scheduler
    for case in lc.CASES:
        s = _build(vited, case)
        assert s.device_capable(), case['id']
        words = s._table_words()
        assert len(words) == vited.ops.LR_TABLE_WORDS == 44 and all(type(w) is float for w in words)
    many = L.MultiStepLRScheduler(_optimizer(), milestones=list(range(10, 43)), gamma=0.5)           # 33 milestones: host-stepped
    assert not many.device_capable()
    assert L.MultiStepLRScheduler(_optimizer(), milestones=list(range(10, 42)), gamma=0.5).device_capable()
    assert not L.MultiStepLRScheduler(_optimizer(), milestones=[20, 10], gamma=0.5).device_capable()
    s = _build(vited, lc.BY_ID['linear_warm2'])
    s.load_state_dict({'warmup_steps': [1e-5, 1e-5]})          # not the base values' own: only the host can follow that
    assert not s.device_capable()
    assert not L.LinearLRScheduler(_optimizer(), t_initial=10, lr_min_rate=0.01, warmup_t=10).device_capable()      # t / 0


def _bits64(v):
    return struct.unpack('<Q', struct.pack('<d', float(v)))[0]


def test_host_program_gives_pythons_bits_under_the_sanitizers(vited, tmp_path):
    """tools/lrsched_host_check.cpp: csrc/lr_schedule.h, the text the kernel runs, over the whole case table (the tables are the ones
    the schedulers would upload) - a stand-alone program with its own main, built with -fsanitize=address,undefined and
    -ffp-contract=off.  Its fp64 bits are Python's for every case: the same libm, the same operation order."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    cxx = next((c for c in (shutil.which('clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'))
                if c and os.path.exists(c)), None)
    assert cxx is not None, 'no clang++ beside hipcc: the HIP toolchain that builds the library ships one'
    exe = str(tmp_path / 'lrsched_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off', '-I',
                    os.path.join(ROOT, 'vit-ed_amd', 'csrc'), os.path.join(ROOT, 'tools', 'lrsched_host_check.cpp'), '-o', exe], check=True)
    lines, want = [], []
    many = vited.lr_scheduler.MultiStepLRScheduler(_optimizer(), milestones=list(range(3, 35)), gamma=0.9)      # a full table of 32
    for case, s in [(c, _build(vited, c)) for c in lc.CASES] + [(None, many)]:
        words = ' '.join(f'{_bits64(w):016x}' for w in s._table_words())
        for t in lc.T_VALUES:
            for base, scale in ((lc.BASE_LR, 1.0), (3e-4, 0.1)):
                v = lc.value(case, t, base) if case is not None else base * 0.9 ** min(max(t - 2, 0), 32)
                lines.append(f'{words} {_bits64(base):016x} {_bits64(scale):016x} {t}')
                want.append(f'{_bits64(v):016x} {struct.unpack("<I", struct.pack("<f", np.float32(v * scale)))[0]:08x}')
    cases = tmp_path / 'cases.txt'
    cases.write_text('\n'.join(lines) + '\n')
    run = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), run.stdout[-2000:] + run.stderr[-2000:]
    out = run.stdout.split('\n')
    assert out[len(want)] == f'lrsched_host_check ok: {len(want)} cases'
    wrong = [(i, lines[i].split()[-1], g, w) for i, (g, w) in enumerate(zip(out, want)) if g != w]
    assert not wrong, wrong[:5]


def test_entry_point_is_declared_bound_exported_and_refuses_a_null_table(vited):
    _ensure_built(vited)
    C = vited._lib
    text = re.sub(r'/\*.*?\*/', ' ', open(C.HEADER_PATH).read(), flags=re.S)
    assert re.search(r'\bint\s+vited_lr_schedule_step\s*\(', text)
    import ctypes
    p, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert C.SIGNATURES['vited_lr_schedule_step'] == (i, [p, p, p, i, p, p, i64, i64, i64, p, p])
    out = subprocess.run(['nm', '-D', '--defined-only', C.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(l.split()[-1] == 'vited_lr_schedule_step' and ' T ' in l for l in out.splitlines())
    lib = C.load()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    BAD = 1

    def call(table=a, base=a, scale=a, groups=2, counter=a, dst=a, dst_words=24, first=8, stride=8, last_lr=None):
        return lib.vited_lr_schedule_step(table, base, scale, groups, counter, dst, dst_words, first, stride, last_lr, None)

    # every refusal happens before any launch, so these are safe without a GPU
    assert call(table=None) == BAD and call(base=None) == BAD and call(scale=None) == BAD and call(counter=None) == BAD and call(dst=None) == BAD
    assert call(groups=0) == BAD and call(groups=4097) == BAD and call(first=-1) == BAD and call(stride=0) == BAD and call(dst_words=0) == BAD
    assert call(dst_words=16) == BAD and call(first=17) == BAD and call(groups=3) == BAD           # the last group's word lies outside dst
    assert call(table=a + 4) == BAD and call(counter=a + 4) == BAD and call(dst=a + 2) == BAD and call(last_lr=a + 2) == BAD
    assert call(last_lr=a + 4 * 16) == BAD and call(last_lr=a + 4 * 7) == BAD                       # overlaps the words written
    with pytest.raises(RuntimeError, match=r'^vited_lr_schedule_step failed: .+ \(vited error 1\)$'):
        C.call('vited_lr_schedule_step', None, a, a, 2, a, a, 24, 8, 8, None, None)
    assert vited.ops.lr_schedule_step.__module__.endswith('ops_lrsched')
    src = open(os.path.join(ROOT, 'vit-ed_amd', 'csrc', 'lr_schedule.hip')).read()
    assert '#include "lr_schedule.h"' in src and re.search(r'lr_schedule\.o: FILEFLAGS := -ffp-contract=off',
                                                          open(os.path.join(ROOT, 'vit-ed_amd', 'csrc', 'Makefile')).read())


def test_wrapper_checks_its_tensors_before_the_launch(vited):
    ops = vited.ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.lr_schedule_step(torch.zeros(44, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), torch.ones(2, dtype=torch.float64),
                             torch.zeros(1, dtype=torch.int64), torch.zeros(24), 8, 8)


def test_on_device_and_the_binding_stay_out_of_the_state(vited):
    s = _build(vited, lc.BY_ID['cosine_prefix_warm2'])
    keys = set(s.state_dict())
    s.on_device = False                                        # the documented way to keep a schedule on the host
    assert set(s.state_dict()) == keys and 'on_device' not in keys and '_device' not in keys
    other = _build(vited, lc.BY_ID['cosine_prefix_warm2'])
    other.load_state_dict(dict(s.state_dict(), on_device=False, _device='x', optimizer='y'))      # a state saved by an older tree
    assert other.on_device is None and other._device is None and other.optimizer is not None and other.optimizer != 'y'


def test_a_load_the_device_table_cannot_state_changes_nothing_while_attached(vited):
    """The binding's buffers on the CPU stand in for the device's: nothing is launched by a load."""
    L = vited.lr_scheduler
    s = L.MultiStepLRScheduler(_optimizer(), milestones=[15, 25], gamma=0.1, warmup_t=10, warmup_lr_init=lc.WARMUP_LR)
    s._device = L._DeviceBinding(torch.device('cpu'), 2)
    s._upload()
    table = s._device.table.clone()
    before = s.state_dict()
    for bad in ({'milestones': [25, 15]}, {'milestones': list(range(10, 43))}, {'warmup_steps': [1e-5, 1e-5]}, {'base_values': [1e-4]}):
        with pytest.raises(ValueError):
            s.load_state_dict(bad)
        assert s.state_dict() == before and s.attached() and torch.equal(s._device.table, table), bad
    s.load_state_dict({'milestones': [12, 30], 'gamma': 0.5})
    assert s.milestones == [12, 30] and s._device.table.tolist() == s._table_words() and not torch.equal(s._device.table, table)
    s.detach()
    s.load_state_dict({'milestones': [25, 15]})               # host-stepped, any rule loads
    assert s.milestones == [25, 15] and not s.device_capable()


@pytest.fixture
def stub_ops(vited, monkeypatch):
    """ops without a GPU, as in tests/test_ops_args.py: the device gate, the stream and the library are stubs."""
    calls = []
    monkeypatch.setattr(vited.ops, '_need_gpu', lambda *tensors, **kw: None)
    monkeypatch.setattr(vited.ops, '_stream', lambda: 0)
    monkeypatch.setattr(vited.ops, '_lib', types.SimpleNamespace(call=lambda name, *args: calls.append((name, args))))
    return vited.ops, calls


def test_wrapper_refuses_a_wrong_tensor_before_the_launch(stub_ops):
    ops, calls = stub_ops
    f64 = torch.float64
    valid = dict(table=torch.zeros(44, dtype=f64), base=torch.zeros(2, dtype=f64), scale=torch.ones(2, dtype=f64),
                 counter=torch.zeros(1, dtype=torch.int64), dst=torch.zeros(24), first=8, stride=8, last_lr=torch.zeros(2))
    ops.lr_schedule_step(**valid)
    ops.lr_schedule_step(**dict(valid, last_lr=None))
    assert [name for name, _ in calls] == ['vited_lr_schedule_step'] * 2
    args = calls[0][1]
    assert args[0] == valid['table'].data_ptr() and args[3] == 2 and args[5:9] == (valid['dst'].data_ptr(), 24, 8, 8) and calls[1][1][9] == 0
    del calls[:]
    wide = torch.zeros(24, 2)
    faults = {
        'table': [valid['table'].float(), valid['table'][:43], torch.zeros(44, 2, dtype=f64)[:, 0], None],
        'base': [valid['base'].float(), torch.zeros(0, dtype=f64), torch.zeros(2, 2, dtype=f64)[:, 0]],
        'scale': [valid['scale'].float(), torch.ones(3, dtype=f64), torch.ones(1, dtype=f64), torch.ones(2, 2, dtype=f64)[:, 0]],
        'counter': [torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)],
        'dst': [valid['dst'].double(), torch.zeros(16), wide[:, 0], None],          # 16 words: the second group's lies outside
        'last_lr': [torch.zeros(2, dtype=f64), torch.zeros(3), torch.zeros(1), torch.zeros(2, 2)[:, 0]],
    }
    for name, bads in faults.items():
        for bad in bads:
            with pytest.raises(ValueError, match=rf'^lr_schedule_step: {name}(?!\w)'):
                ops.lr_schedule_step(**dict(valid, **{name: bad}))
    for kw in (dict(first=-1), dict(stride=0), dict(stride=-8), dict(first=16), dict(stride=16)):
        with pytest.raises(ValueError, match=r'^lr_schedule_step: '):
            ops.lr_schedule_step(**dict(valid, **kw))
    with pytest.raises(ValueError, match=r'^lr_schedule_step: .*groups'):
        ops.lr_schedule_step(**dict(valid, base=torch.zeros(4097, dtype=f64), scale=torch.ones(4097, dtype=f64), dst=torch.zeros(8 * 4098)))
    assert not calls                                           # nothing reached the library
