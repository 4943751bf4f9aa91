"""CPU: the learning-rate range test's rule (csrc/lr_finder.h) - the numpy statement of tests/lr_finder_cases.py
and the one ``ops.lr_finder_step`` runs on CPU tensors against hand-written answers, the suggestion, the header against numpy's bits
through a stand-alone host program under the sanitizers, the C entry point's refusals, and ``engine.find_lr``'s argument errors."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import lr_finder_cases as fc
from test_abi import _ensure_built

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    """Equal as bits, for scalars and sequences (NaN equals NaN)."""
    return [fc.bits64(v) for v in np.ravel(a)] == [fc.bits64(v) for v in np.ravel(b)]


# ---- the rule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', fc.CASES, ids=lambda c: c['id'])
def test_numpy_rule_gives_the_hand_written_answers(case):
    got, want = fc.run(case), case['want']
    assert (got['rows'], got['state']) == (want['rows'], want['state'])
    assert got['history'].shape == (want['rows'], 3)
    assert _same(got['history'][:, 1], np.float32(case['losses'][:want['rows']]).astype(np.float64))
    if 'smoothed' in want:
        assert _same(got['history'][:, 2], want['smoothed'])
    assert _same(got['best'], want['best']) and _same(got['smoothed'], got['history'][-1, 2])
    if 'lrs' in want:
        assert got['history'][:, 0].tolist() == want['lrs']
    if 'words' in want:
        assert [[float(v) for v in w] for w in got['words']] == want['words']
    assert got['history'][0, 0] == case['start'][0]                              # the first iteration runs at exactly start
    assert all(lr < case['end'][0] for lr in got['history'][:, 0])               # the end is never reached
    assert len(got['words']) == len(case['losses']) + case['extra']
    if got['state'] != fc.RUNNING:
        assert all(float(v) == 0.0 for w in got['words'][got['rows'] - 1:] for v in w)     # from the halting launch on


def _cpu_buffers(case):
    groups = len(case['start'])
    hyper = torch.full((fc.HEADER + fc.WORDS * groups,), -7.0)
    return dict(state=torch.zeros(4, dtype=torch.int64), history=torch.full((case['num_iter'], 3), -1.0, dtype=torch.float64),
                start=torch.tensor(case['start'], dtype=torch.float64), end=torch.tensor(case['end'], dtype=torch.float64), dst=hyper)


@pytest.mark.parametrize('case', fc.CASES + fc.random_cases(16, seed=5), ids=lambda c: c['id'])
def test_wrapper_on_cpu_tensors_is_the_same_rule_bit_for_bit(vited, case):
    ops, b = vited.ops, _cpu_buffers(case)
    losses = list(case['losses']) + [case['losses'][-1]] * case['extra']
    for n, loss in enumerate(losses, 1):
        before = b['state'].clone(), b['history'].clone()
        ops.lr_finder_step(torch.tensor(loss, dtype=torch.float32), num_iter=case['num_iter'], smooth_f=case['smooth_f'],
                           diverge_th=case['diverge_th'], first=fc.HEADER, stride=fc.WORDS, **b)
        want = fc.run(case, n)
        assert b['state'][:2].tolist() == [want['rows'], want['state']], n
        assert _same(b['history'][:want['rows']].numpy(), want['history']), n
        if want['rows']:
            assert _same(b['state'][2:].view(torch.float64).numpy(), [want['smoothed'], want['best']]), n
        assert [fc.bits32(v) for v in b['dst'][fc.HEADER::fc.WORDS].tolist()] == [fc.bits32(v) for v in want['words'][-1]], n
        rest = torch.ones_like(b['dst'], dtype=torch.bool)
        rest[fc.HEADER::fc.WORDS] = False
        assert bool((b['dst'][rest] == -7.0).all())                              # no other word of the array moves
        if n > 1 and fc.run(case, n - 1)['state'] != fc.RUNNING:                 # halted before this launch: nothing but the words
            assert torch.equal(b['state'], before[0]) and torch.equal(b['history'].view(torch.int64), before[1].view(torch.int64)), n
    assert bool((b['history'][want['rows']:] == -1.0).all())                     # rows behind the halting row do not exist
    assert vited.ops.lr_finder_step.__module__.endswith('ops_lrfinder')
    assert (ops.LRF_RUNNING, ops.LRF_DONE, ops.LRF_DIVERGED, ops.LRF_NONFINITE) == (fc.RUNNING, fc.DONE, fc.DIVERGED, fc.NONFINITE)


def test_rate_is_exact_at_the_start_and_stays_below_the_end(vited):
    rate = vited.ops.lr_finder_rate
    for start, end, n in ((1e-7, 1e-2, 100), (3e-6, 10.0, 7), (1e-7 * 0.1, 1e-2 * 0.1, 1)):
        assert rate(start, end, 0, n) == start
        values = [rate(start, end, i, n) for i in range(n)]
        assert all(a < b for a, b in zip(values, values[1:])) and values[-1] < end
        assert abs(rate(start, end, n, n) / end - 1) < 1e-14
        assert _same(values, [fc.rate(start, end, i, n) for i in range(n)])


# ---- the suggestion --------------------------------------------------------------------------------------------------------------
def test_suggestion_is_the_rate_behind_the_steepest_descent(vited):
    sug = vited.ops.lr_suggestion
    lrs = [1., 2., 3., 4., 5., 6.]
    assert sug(lrs, [9., 8., 5., 4., 3.5, 7.]) == 3.                 # differences -1 -3 -1 -.5 3.5: the steepest ends at row 2
    assert sug(lrs, [9., 7., 5., 3., 3., 3.]) == 2.                  # a tie of three -2s: the first wins
    assert sug(lrs, [9., 0., 5., 4., 2., 7.]) == 2.
    assert sug(lrs, [9., 0., 5., 4., 2., 7.], skip_start=1) == 5.    # rows 1..5: differences 5 -1 -2 5
    assert sug(lrs, [9., 8., 7.5, 7., 6., 0.]) == 6.
    assert sug(lrs, [9., 8., 7.5, 7., 6., 0.], skip_end=1) == 2.     # rows 0..4: -1 -.5 -.5 -1, the first -1
    assert sug(lrs, [9., 8., 7.5, 7., 5., 0.], skip_start=2, skip_end=1) == 5.
    assert sug(lrs[:2], [1., 2.]) == 2. and sug(torch.tensor(lrs), torch.tensor([9., 8., 5., 4., 3.5, 7.])) == 3.
    for kw in (dict(lrs=[1.], smoothed=[1.]), dict(lrs=[], smoothed=[]), dict(lrs=lrs, smoothed=[1.] * 6, skip_start=5),
               dict(lrs=lrs, smoothed=[1.] * 6, skip_start=2, skip_end=3), dict(lrs=lrs, smoothed=[1.] * 5),
               dict(lrs=lrs, smoothed=[1.] * 6, skip_end=-1)):
        with pytest.raises(ValueError, match='^lr_suggestion: '):
            sug(**kw)


# ---- the header under the sanitizers ---------------------------------------------------------------------------------------------
def test_host_program_gives_numpys_bits_under_the_sanitizers(tmp_path):
    """tools/lrfinder_host_check.cpp: csrc/lr_finder.h, the text the kernel runs, over the scripted and 64 random sequences on
    exactly-sized heap buffers - a stand-alone program with its own main, built with -fsanitize=address,undefined and
    -ffp-contract=off.  It compares every launch with a scalar statement of its own; its bits are numpy's."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    cxx = next((c for c in (shutil.which('clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'))
                if c and os.path.exists(c)), None)
    assert cxx is not None, 'no clang++ beside hipcc: the HIP toolchain that builds the library ships one'
    exe = str(tmp_path / 'lrfinder_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off', '-I',
                    os.path.join(ROOT, 'vit-ed_amd', 'csrc'), os.path.join(ROOT, 'tools', 'lrfinder_host_check.cpp'), '-o', exe], check=True)
    cases = fc.CASES + fc.random_cases()
    lines, want = [], []
    for c in cases:
        ends = ' '.join(f'{fc.bits64(a):016x} {fc.bits64(b):016x}' for a, b in zip(c['start'], c['end']))
        lines.append(f"{c['num_iter']} {c['extra']} {fc.bits64(c['smooth_f']):016x} {fc.bits64(c['diverge_th']):016x} {len(c['start'])} {ends} "
                     f"{len(c['losses'])} " + ' '.join(f'{fc.bits32(v):08x}' for v in c['losses']))
        r = fc.run(c)
        want.append(f"case {r['rows']} {r['state']} {fc.bits64(r['smoothed']):016x} {fc.bits64(r['best']):016x}")
        want += ['w ' + ' '.join(f'{fc.bits32(v):08x}' for v in w) for w in r['words']]
        want += ['h ' + ' '.join(f'{fc.bits64(v):016x}' for v in row) for row in r['history']]
    path = tmp_path / 'cases.txt'
    path.write_text('\n'.join(lines) + '\n')
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), run.stdout[-2000:] + run.stderr[-2000:]
    out = run.stdout.split('\n')
    assert out[len(want)] == f'lrfinder_host_check ok: {len(cases)} cases'
    wrong = [(i, g, w) for i, (g, w) in enumerate(zip(out, want)) if g != w]
    assert not wrong, wrong[:5]


# ---- the C entry point without a GPU ---------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_exported_and_refuses_before_any_launch(vited):
    _ensure_built(vited)
    C = vited._lib
    text = re.sub(r'/\*.*?\*/', ' ', open(C.HEADER_PATH).read(), flags=re.S)
    assert re.search(r'\bint\s+vited_lr_finder_step\s*\(', text)
    p, i, i64, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    assert C.SIGNATURES['vited_lr_finder_step'] == (i, [p, p, p, i64, p, p, i, i64, d, d, p, i64, i64, i64, p])
    out = subprocess.run(['nm', '-D', '--defined-only', C.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(l.split()[-1] == 'vited_lr_finder_step' and ' T ' in l for l in out.splitlines())
    lib = C.load()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    BAD = 1

    def call(loss=a, state=a, history=a, capacity=10, start=a, end=a, groups=2, num_iter=10, smooth_f=0.05, diverge_th=5.0, dst=a,
             dst_words=24, first=8, stride=8):
        return lib.vited_lr_finder_step(loss, state, history, capacity, start, end, groups, num_iter, smooth_f, diverge_th, dst, dst_words,
                                        first, stride, None)

    # every refusal happens before any launch, so these are safe without a GPU
    for name in ('loss', 'state', 'history', 'start', 'end', 'dst'):
        assert call(**{name: None}) == BAD, name
    assert call(groups=0) == BAD and call(groups=-1) == BAD and call(groups=4097) == BAD
    assert call(num_iter=0) == BAD and call(num_iter=-3) == BAD and call(num_iter=11) == BAD and call(capacity=0) == BAD
    assert call(smooth_f=-0.01) == BAD and call(smooth_f=1.01) == BAD and call(smooth_f=math.nan) == BAD
    assert call(diverge_th=1.0) == BAD and call(diverge_th=0.5) == BAD and call(diverge_th=math.nan) == BAD
    assert call(first=-1) == BAD and call(stride=0) == BAD and call(dst_words=0) == BAD
    assert call(dst_words=16) == BAD and call(first=17) == BAD and call(groups=3) == BAD           # the last group's word lies outside dst
    for name in ('state', 'history', 'start', 'end'):
        assert call(**{name: a + 4}) == BAD, name
    assert call(loss=a + 2) == BAD and call(dst=a + 2) == BAD
    with pytest.raises(RuntimeError, match=r'^vited_lr_finder_step failed: .+ \(vited error 1\)$'):
        C.call('vited_lr_finder_step', None, a, a, 10, a, a, 2, 10, 0.05, 5.0, a, 24, 8, 8, None)
    src = open(os.path.join(ROOT, 'vit-ed_amd', 'csrc', 'lr_finder.hip')).read()
    assert '#include "lr_finder.h"' in src and re.search(r'lr_finder\.o: FILEFLAGS := -ffp-contract=off',
                                                         open(os.path.join(ROOT, 'vit-ed_amd', 'csrc', 'Makefile')).read())


@pytest.fixture
def stub_ops(vited, monkeypatch):
    """ops without a GPU, as in tests/test_ops_args.py: the device gate, the stream and the library are stubs."""
    calls = []
    monkeypatch.setattr(vited.ops, '_need_gpu', lambda *tensors, **kw: None)
    monkeypatch.setattr(vited.ops, '_stream', lambda: 0)
    monkeypatch.setattr(vited.ops, '_lib', types.SimpleNamespace(call=lambda name, *args: calls.append((name, args))))
    return vited.ops, calls


def test_wrapper_refuses_a_wrong_tensor_before_the_launch(vited, stub_ops):
    ops, calls = stub_ops
    f64 = torch.float64
    valid = dict(loss=torch.zeros(()), state=torch.zeros(4, dtype=torch.int64), history=torch.zeros(10, 3, dtype=f64),
                 start=torch.ones(2, dtype=f64), end=torch.ones(2, dtype=f64), num_iter=10, smooth_f=0.05, diverge_th=5.0,
                 dst=torch.zeros(24), first=8, stride=8)
    faults = {
        'loss': [torch.zeros((), dtype=f64), torch.zeros(2), None],
        'state': [torch.zeros(4, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), torch.zeros(4, 2, dtype=torch.int64)[:, 0]],
        'history': [torch.zeros(10, 3), torch.zeros(10, 2, dtype=f64), torch.zeros(30, dtype=f64), torch.zeros(10, 6, dtype=f64)[:, ::2]],
        'start': [torch.ones(2), torch.ones(0, dtype=f64), torch.ones(2, 2, dtype=f64)[:, 0]],
        'end': [torch.ones(2), torch.ones(3, dtype=f64), torch.ones(1, dtype=f64)],
        'dst': [torch.zeros(24, dtype=f64), torch.zeros(16), torch.zeros(24, 2)[:, 0], None],
    }
    for name, bads in faults.items():
        for bad in bads:
            with pytest.raises(ValueError, match=rf'^lr_finder_step: {name}(?!\w)'):
                ops.lr_finder_step(**dict(valid, **{name: bad}))
    for kw in (dict(first=-1), dict(stride=0), dict(first=16), dict(stride=16), dict(num_iter=0), dict(num_iter=11), dict(smooth_f=-0.1),
               dict(smooth_f=1.5), dict(diverge_th=1.0), dict(diverge_th=float('nan'))):
        with pytest.raises(ValueError, match=r'^lr_finder_step: '):
            ops.lr_finder_step(**dict(valid, **kw))
    with pytest.raises(ValueError, match=r'^lr_finder_step: .*groups'):
        ops.lr_finder_step(**dict(valid, start=torch.ones(4097, dtype=f64), end=torch.ones(4097, dtype=f64), dst=torch.zeros(8 * 4098)))
    assert not calls                                           # nothing reached the library


# ---- find_lr's argument errors ----------------------------------------------------------------------------------------------------
class _Step:
    """What find_lr looks at before it touches a device: built without running TrainStep's constructor."""

    def __new__(cls, vited, optimizer, lr_scheduler=None, accum=1):
        step = object.__new__(vited.engine.TrainStep)
        step.optimizer, step.lr_scheduler, step.accum, step.hip_opt = optimizer, lr_scheduler, accum, hasattr(optimizer, 'bind_flat')
        return step


def test_find_lr_says_what_it_cannot_sweep(vited):
    E = vited.engine
    params = [torch.nn.Parameter(torch.zeros(3))]
    flat_opt = vited.optim.FlatAdamW(params, lr=1e-3)
    loader = [(None, None)] * 4
    with pytest.raises(ValueError, match='lr_scheduler'):
        E.find_lr(_Step(vited, flat_opt, lr_scheduler=object()), loader)
    with pytest.raises(ValueError, match='accumulation_steps 2'):
        E.find_lr(_Step(vited, flat_opt, accum=2), loader)
    with pytest.raises(NotImplementedError, match='FlatAdamW / optim.FlatSGD; SGD has none'):
        E.find_lr(_Step(vited, torch.optim.SGD(params, lr=1e-3)), loader)
    with pytest.raises(ValueError, match=f'above {E.LR_FINDER_MAX_ITER}, the capacity'):
        E.find_lr(_Step(vited, flat_opt), loader, num_iter=E.LR_FINDER_MAX_ITER + 1)
    with pytest.raises(ValueError, match='poll_every'):
        E.find_lr(_Step(vited, flat_opt), loader, poll_every=-1)
    with pytest.raises(TypeError, match='TrainStep'):
        E.find_lr(object(), loader)
    with pytest.raises(RuntimeError, match='bind_flat'):       # an optimizer no TrainStep has bound owns no device array
        E.find_lr(_Step(vited, flat_opt), loader, restore=False)
    # LRRangeTest's own checks, on an optimizer whose array stands in on the CPU: nothing is launched by building one
    flat_opt._hyper, flat_opt.param_groups[0]['lr_scale'] = torch.zeros(16), 0.5
    test = E.LRRangeTest(flat_opt, 10, start_lr=1e-6, end_lr=1e-1)
    assert test.start == [5e-7] and test.end == [5e-2] and flat_opt.param_groups[0]['lr'] == 5e-7       # value * lr_scale, as set_lr
    assert flat_opt._hyper[8].item() == float(np.float32(5e-7)) and flat_opt.hyper_uploads == 1
    assert E.LRRangeTest(flat_opt, 10, start_lr=[1e-6], end_lr=[1e-1]).start == [1e-6]                  # per group: as given
    with pytest.raises(NotImplementedError, match='SGD has none'):
        E.LRRangeTest(torch.optim.SGD(params, lr=1e-3), 10)
    for kw in (dict(num_iter=0), dict(num_iter=E.LR_FINDER_MAX_ITER + 1), dict(start_lr=0.0), dict(start_lr=-1e-3), dict(end_lr=float('inf')),
               dict(start_lr=1e-2, end_lr=1e-2), dict(start_lr=[1e-7, 1e-7]), dict(smooth_f=1.5), dict(smooth_f=-0.1), dict(diverge_th=1.0)):
        with pytest.raises(ValueError, match='^LRRangeTest: '):
            E.LRRangeTest(flat_opt, **dict(dict(num_iter=10), **kw))
