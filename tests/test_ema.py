"""CPU: the parameter-EMA rule as tests/ema_cases.py states it (numpy fp32) against the plain expression in fp64, the warmup crossover, what
the optimizers refuse before anything touches a device, the shape of ``state_dict()``, the C entries' refusals before any launch, and
the host build of the rule (tools/ema_host_check.cpp) under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ema_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_rule_against_the_plain_expression_in_fp64():
    """50 updates of random data: fp32 rounds each of the three operations to 2^-24 relative, and the average is a convex combination, so
    the error does not grow with the number of updates beyond a few ulp of the largest operand: rtol 1e-6 of fp64's d*e + (1-d)*p, with
    the absolute term the same factor of the data's scale (values pass through zero)."""
    rng = np.random.default_rng(5)
    for d, warmup in ((0.9999, False), (0.99, True), (0.5, True), (0.0, False)):
        e32 = rng.standard_normal(4096).astype(F)
        e64, n = e32.astype(np.float64), 0
        for _ in range(50):
            p = rng.standard_normal(4096).astype(F)
            dt = ec.decay_at(d, warmup, n)
            e64 = float(dt) * e64 + (1.0 - float(dt)) * p.astype(np.float64)
            e32, n = ec.update(e32, p, d, warmup, n)
            assert e32.dtype == F
            np.testing.assert_allclose(e32, e64, rtol=1e-6, atol=1e-6)
        assert n == 50


def test_warmup_crossover():
    # d = 0.5: (1 + n) / (10 + n) reaches 0.5 at n = 8 (9 / 18); below it the ramp, from it on d
    for n in range(8):
        assert ec.decay_at(0.5, True, n) == F(F(1 + n) / F(10 + n)) < F(0.5)
    assert ec.decay_at(0.5, True, 7) == F(F(8.0) / F(17.0))
    for n in (8, 9, 100, 10 ** 6):
        assert ec.decay_at(0.5, True, n) == F(0.5)
    assert ec.decay_at(0.5, False, 0) == F(0.5)
    # d = 0.9999: (1 + n) / (10 + n) >= d  <=>  n >= 89990 in exact arithmetic; in fp32 the ramp is monotone and has reached fl(d) there,
    # and is still below it a few thousand updates earlier
    d = F(0.9999)
    assert ec.decay_at(0.9999, True, 0) == F(F(1.0) / F(10.0))
    assert ec.decay_at(0.9999, True, 80000) < d
    first = next(n for n in range(80000, 100000) if ec.decay_at(0.9999, True, n) == d)
    assert abs(first - 89990) <= 60              # fl(d) and the ramp's fp32 steps (6e-8 against a slope of 1.1e-9 per update)
    assert all(ec.decay_at(0.9999, True, n) == d for n in (first, first + 1, 95000, 10 ** 7))


def test_swap_statement_is_an_involution():
    p, e = ec.initial_parameters()[3], ec.gradient(0, 65 * 63).reshape(65, 63)
    p1, e1, sh, sh_t = ec.swap(p, e)
    assert np.array_equal(p1, e) and np.array_equal(e1, p) and np.array_equal(sh, e) and np.array_equal(sh_t, e.T) and sh_t.shape == (63, 65)
    p2, e2, _, _ = ec.swap(p1, e1)
    assert np.array_equal(p2, p) and np.array_equal(e2, e)


def _params():
    return [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in ec.initial_parameters()]


def _groups(ps):
    return [{'params': [p for p in ps if p.ndim > 1]}, {'params': [p for p in ps if p.ndim <= 1], 'weight_decay': 0.0}]


@pytest.mark.parametrize('kind', ['adamw', 'sgd'])
def test_refusals_before_anything_is_built(vited, kind):
    make = (lambda **kw: vited.optim.FlatAdamW(_groups(_params()), lr=1e-3, **kw)) if kind == 'adamw' else \
        (lambda **kw: vited.optim.FlatSGD(_groups(_params()), lr=1e-3, momentum=0.9, nesterov=True, **kw))
    for bad in (1.0, -0.1, 1.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match=r'ema_decay must lie in \[0, 1\)'):
            make(ema_decay=bad)
    opt = make(ema_decay=0.0, ema_warmup=True)              # 0 is a decay: the average follows the parameters
    assert opt.ema_decay == 0.0 and opt.ema_warmup is True and opt.ema is None and opt.num_ema_updates == 0 and not opt.ema_swapped
    with pytest.raises(ValueError, match=r'ema_decay must lie in \[0, 1\)'):
        opt.ema_decay = 1.0
    assert opt.ema_decay == 0.0
    opt.ema_decay = 0.999
    assert opt.ema_decay == 0.999
    plain = make()
    assert plain.ema_decay is None and plain.ema is None
    with pytest.raises(RuntimeError, match='swap_ema: no average is kept'):
        with plain.swap_ema():
            pass
    with pytest.raises(RuntimeError, match='ema_of: no average is kept'):
        plain.ema_of(plain.param_groups[0]['params'][0])
    with pytest.raises(RuntimeError, match='load_ema_state_dict: no average is kept'):
        plain.load_ema_state_dict({}, torch.nn.Linear(2, 2))
    with pytest.raises(RuntimeError, match='swap_ema: call bind_flat'):
        with opt.swap_ema():
            pass
    opt._swapped = True                                     # as inside the block
    with pytest.raises(RuntimeError, match=r'swap_ema: already inside `with swap_ema\(\):` \(nested use would exchange the weights back\)'):
        with opt.swap_ema():
            pass
    with pytest.raises(RuntimeError, match=r'step_flat: call bind_flat'):
        opt.step_flat()


def test_build_optimizer_passes_the_average_on_and_refuses_it_off_the_gpu(vited):
    from types import SimpleNamespace as NS
    cfg = NS(TRAIN=NS(OPTIMIZER=NS(NAME='adamw', EPS=1e-8, BETAS=(0.9, 0.999), MOMENTUM=0.9), BASE_LR=1e-3, WEIGHT_DECAY=0.05))
    model = torch.nn.Linear(4, 2)
    with pytest.raises(ValueError, match='ema_decay needs the HIP optimizers'):
        vited.engine.build_optimizer(cfg, model, ema_decay=0.999)
    assert type(vited.engine.build_optimizer(cfg, model)) is torch.optim.AdamW


@pytest.mark.parametrize('kind', ['adamw', 'sgd'])
def test_state_dict_has_the_keys_of_an_optimizer_without_the_average(vited, kind):
    def make(**kw):
        ps = _params()
        return vited.optim.FlatAdamW(_groups(ps), lr=1e-3, **kw) if kind == 'adamw' else \
            vited.optim.FlatSGD(_groups(ps), lr=1e-3, momentum=0.9, nesterov=True, **kw)
    with_ema, without = make(ema_decay=0.9999, ema_warmup=True).state_dict(), make().state_dict()
    assert set(with_ema) == set(without) and set(with_ema['state']) == set(without['state'])
    assert [set(g) for g in with_ema['param_groups']] == [set(g) for g in without['param_groups']]
    torch_opt = torch.optim.AdamW(_groups(_params()), lr=1e-3) if kind == 'adamw' else \
        torch.optim.SGD(_groups(_params()), lr=1e-3, momentum=0.9, nesterov=True)
    torch_opt.load_state_dict(with_ema)                     # still torch's


def test_ema_state_dict_before_binding_is_the_parameters(vited):
    model = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.BatchNorm1d(3))
    model[0].bias.requires_grad_(False)
    opt = vited.optim.FlatAdamW(vited.engine.param_groups_no_decay_1d(model), lr=1e-3, ema_decay=0.99)
    sd = opt.ema_state_dict(model)
    assert list(sd) == list(model.state_dict())
    for k, v in model.state_dict().items():
        assert torch.equal(sd[k], v) and sd[k].data_ptr() != v.data_ptr()
    loaded = {k: v + 1 if v.is_floating_point() else v for k, v in sd.items()}
    opt.load_ema_state_dict(loaded, model, num_ema_updates=7)
    assert opt.num_ema_updates == 7
    again = opt.ema_state_dict(model)
    assert torch.equal(again['0.weight'], model[0].weight + 1) and torch.equal(again['0.bias'], model[0].bias)      # frozen: its own value
    with pytest.raises(KeyError, match='0.weight is missing'):
        opt.load_ema_state_dict({}, model)
    with pytest.raises(ValueError, match='0.weight has shape'):
        opt.load_ema_state_dict(dict(loaded, **{'0.weight': torch.zeros(2, 2)}), model)


def test_entries_are_declared_bound_exported_and_refuse_before_any_launch(vited):
    C = ctypes
    p, i, i64, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    sigs = vited._lib.SIGNATURES
    step = (i, [p, i, i64, p, i64, p, f, i, p, p, i64, p])
    assert sigs['vited_adamw_step'] == step and sigs['vited_sgd_step'] == step                   # the prototypes they had
    step_ema = (i, step[1][:-1] + [p, i64, p])
    assert sigs['vited_adamw_step_ema'] == step_ema and sigs['vited_sgd_step_ema'] == step_ema
    assert sigs['vited_ema_swap'] == (i, [p, i, i64, p, p, p])
    lib = vited._lib.load()
    # host memory stands in for device memory: every call below is refused before a launch, nothing is dereferenced
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    base += -base % 16
    good = [base, 1, 1, base + 64, 16, base + 128, 0.0, 1, None, base, 1 << 20]
    for name in ('vited_adamw_step_ema', 'vited_sgd_step_ema'):
        fn = getattr(lib, name)
        assert fn(*good, None, 16, None) == 1              # a null average
        assert fn(*good, base + 192, 15, None) == 1        # shorter than the gradient buffer
        assert fn(*good, base + 196, 16, None) == 1        # not 16-byte aligned
        assert fn(None, 0, 0, None, 0, None, 0.0, 0, None, None, 0, base + 192, 16, None) == 1
    assert lib.vited_ema_swap(base, 1, 1, None, base + 64, None) == 1
    assert lib.vited_ema_swap(base, 1, 1, base + 196, base + 64, None) == 1
    assert lib.vited_ema_swap(base, 1, 1, base + 192, None, None) == 1
    assert lib.vited_ema_swap(None, 1, 1, base + 192, base + 64, None) == 1
    assert lib.vited_ema_swap(base, 0, 1, base + 192, base + 64, None) == 1
    assert lib.vited_ema_swap(base, 1, 0, base + 192, base + 64, None) == 1
    text = re.sub(r'/\*.*?\*/', ' ', open(vited._lib.HEADER_PATH).read(), flags=re.S)
    assert re.search(r'\bint\s+vited_ema_swap\s*\(', text)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'vit-ed_amd')
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith('.py'):
                src = open(os.path.join(dirpath, fn)).read()
                assert not re.search(r'^\s*(import|from)\s+oracle\b', src, flags=re.M), os.path.join(dirpath, fn)


def test_host_build_of_the_rule_under_the_sanitizers(tmp_path):
    """tools/ema_host_check.cpp compiles csrc/optim_update.h for the host - the text the kernels run - and checks the rule, the update
    pieces with the average and the swap piece over exactly-sized heap buffers; a stand-alone program, run as its own process."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    cxx = next((c for c in (shutil.which('clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'))
                if c and os.path.exists(c)), None)
    assert cxx is not None, 'no clang++ beside hipcc: the HIP toolchain that builds the library ships one'
    exe = str(tmp_path / 'ema_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                    os.path.join(ROOT, 'vit-ed_amd', 'csrc'), os.path.join(ROOT, 'tools', 'ema_host_check.cpp'), '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and 'ema_host_check ok' in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
