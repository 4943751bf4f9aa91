"""CPU: the SGD entry point is declared, bound and exported; FlatSGD's constructor applies torch.optim.SGD's rules before anything
touches a device; engine.build_optimizer keeps the torch optimizers for CPU models."""
import os
import re
import subprocess
import types

import pytest
import torch

from test_abi import _ensure_built


def test_sgd_entry_point_is_declared_bound_and_exported(vited):
    _ensure_built(vited)
    text = re.sub(r'/\*.*?\*/', ' ', open(vited._lib.HEADER_PATH).read(), flags=re.S)
    assert re.search(r'\bint\s+vited_sgd_step\s*\(', text)
    sgd, adamw = vited._lib.SIGNATURES['vited_sgd_step'], vited._lib.SIGNATURES['vited_adamw_step']
    assert sgd == adamw and len(sgd[1]) == 12              # the same argument list
    out = subprocess.run(['nm', '-D', '--defined-only', vited._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(l.split()[-1] == 'vited_sgd_step' and ' T ' in l for l in out.splitlines())
    lib = vited._lib.load()
    assert lib.vited_sgd_step(None, 0, 0, None, 0, None, 0.0, 0, None, None, 0, None) == 1      # validated before any launch
    assert lib.vited_adamw_workspace_bytes() == (1024 + 4) * 4                                  # partials + {norm, clip, applied, t}


def test_update_bodies_live_in_a_header_that_compiles_for_the_host(vited):
    csrc = os.path.join(os.path.dirname(vited._lib.HEADER_PATH), '..', 'vit-ed_amd', 'csrc')
    text = open(os.path.join(csrc, 'optim_update.h')).read()
    for name in ('adamw_piece', 'sgd_piece', 'optim_decide'):
        assert re.search(r'\b%s\s*\(' % name, text), name
    assert '#include "optim_update.h"' in open(os.path.join(csrc, 'optimizer.hip')).read()


def test_flat_sgd_constructor_checks(vited):
    p = [torch.nn.Parameter(torch.zeros(3, 3))]
    with pytest.raises(ValueError, match='dampening'):
        vited.optim.FlatSGD(p, lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError, match='Nesterov'):
        vited.optim.FlatSGD(p, lr=0.1, nesterov=True)
    with pytest.raises(ValueError, match='Nesterov'):
        vited.optim.FlatSGD([{'params': p, 'momentum': 0.0}], lr=0.1, momentum=0.9, nesterov=True)
    with pytest.raises(ValueError, match='learning rate'):
        vited.optim.FlatSGD(p, lr=-1.0)
    with pytest.raises(ValueError, match='momentum'):
        vited.optim.FlatSGD(p, lr=0.1, momentum=-0.5)
    opt = vited.optim.FlatSGD(p, lr=0.1, momentum=0.9, nesterov=True, weight_decay=0.05, skip_nonfinite=True)
    sd = opt.state_dict()
    assert sd['state'] == {} and opt.num_updates == 0 and opt.skipped_updates == 0 and opt.skip_nonfinite
    want = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3, 3))], lr=0.1, momentum=0.9, nesterov=True, weight_decay=0.05).state_dict()
    assert set(sd['param_groups'][0]) == set(want['param_groups'][0])           # torch.optim.SGD's shape
    with pytest.raises(RuntimeError, match='no CPU path'):                      # there is no CPU path
        opt.bind_flat(vited.engine.FlatGradients(p))
    with pytest.raises(RuntimeError, match='no CPU path'):
        vited.optim.FlatAdamW(p).bind_flat(vited.engine.FlatGradients(p))


def _config(name):
    opt = types.SimpleNamespace(NAME=name, EPS=1e-8, BETAS=(0.9, 0.999), MOMENTUM=0.9)
    return types.SimpleNamespace(TRAIN=types.SimpleNamespace(OPTIMIZER=opt, BASE_LR=1e-3, WEIGHT_DECAY=0.05))


def test_build_optimizer_keeps_torch_optimizers_on_cpu(vited):
    model = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.LayerNorm(4))
    sgd = vited.engine.build_optimizer(_config('sgd'), model)
    assert type(sgd) is torch.optim.SGD and sgd.defaults['nesterov'] and sgd.defaults['momentum'] == 0.9
    assert [g['weight_decay'] for g in sgd.param_groups] == [0.05, 0.0]
    assert type(vited.engine.build_optimizer(_config('adamw'), model)) is torch.optim.AdamW
    assert type(vited.engine.build_optimizer(_config('sgd'), model, fused_hip=False)) is torch.optim.SGD
    for name in ('sgd', 'adamw'):
        with pytest.raises(ValueError, match='skip_nonfinite'):
            vited.engine.build_optimizer(_config(name), model, skip_nonfinite=True)
    with pytest.raises(ValueError, match='unknown optimizer'):
        vited.engine.build_optimizer(_config('lamb'), model)
