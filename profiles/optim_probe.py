#!/usr/bin/env python3
"""What one optimizer update of config A's parameter set costs on the MI355X, eagerly launched, bf16 weight shadows present.

    python3 profiles/optim_probe.py [--rounds 5] [--updates 100] [--forms torch_sgd,flat_sgd,flat_adamw] [--out FILE]

One process; config A (patch 8, D 384, 8 + 8 blocks, 4 bins), one model per form, each after one bf16 forward + backward so that
its weight shadows exist.  Forms:
  torch_sgd   what TrainStep._update runs for a torch optimizer: flat.clip_, torch.optim.SGD(momentum 0.9, nesterov).step,
              the recast of every bf16 shadow, flat.zero
  flat_sgd    optim.FlatSGD.step_flat (vited_sgd_step); left out when the package has no FlatSGD
  flat_adamw  optim.FlatAdamW.step_flat (vited_adamw_step)
After a warm-up, ``--rounds`` rounds time ``--updates`` updates of each form between device events, alternating.  Prints one JSON
line: microseconds per update, per round, with median, lowest and highest.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vited_amd as v  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--updates', type=int, default=100)
    ap.add_argument('--forms', default='torch_sgd,flat_sgd,flat_adamw', help='which forms to build and time, in this order')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    v._lib.load()
    E = v.engine
    cfg = v.config_from_yaml(os.path.join(ROOT, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml'))
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(16, 2, 3, 64, 64, device=dev, generator=g) * 2 - 1
    y = (torch.rand(16, 4, device=dev, generator=g) < 0.25).float()

    def model_with_shadows():
        torch.manual_seed(0)
        model = v.build_model(cfg).to(dev).train()
        flat = E.FlatGradients(model.parameters())
        with torch.autocast('cuda', dtype=torch.bfloat16):
            loss = torch.nn.functional.binary_cross_entropy_with_logits(model(x).float(), y)
        loss.backward()
        return model, flat

    forms = {}
    model, flat = model_with_shadows()
    topt = torch.optim.SGD(E.param_groups_no_decay_1d(model), lr=1e-4, momentum=0.9, nesterov=True, weight_decay=0.05)
    params = list(model.parameters())

    def torch_sgd(model=model, flat=flat, topt=topt, params=params):
        flat.clip_(5.0)
        topt.step()
        for rt in model._runtimes.values():
            rt.refresh_shadows(params)
        flat.zero()

    forms['torch_sgd'] = torch_sgd
    if hasattr(v.optim, 'FlatSGD'):
        model_s, flat_s = model_with_shadows()
        sgd = v.optim.FlatSGD(E.param_groups_no_decay_1d(model_s), lr=1e-4, momentum=0.9, nesterov=True, weight_decay=0.05, model=model_s)
        sgd.bind_flat(flat_s, model_s)
        forms['flat_sgd'] = lambda: sgd.step_flat(5.0)
    model_a, flat_a = model_with_shadows()
    adamw = v.optim.FlatAdamW(E.param_groups_no_decay_1d(model_a), lr=1e-4, weight_decay=0.05, model=model_a)
    adamw.bind_flat(flat_a, model_a)
    forms['flat_adamw'] = lambda: adamw.step_flat(5.0)
    forms = {name: forms[name] for name in args.forms.split(',') if name in forms}
    shadows = sum(len(cache) for cache in v.functions.shadows_of(model_a))
    assert shadows > 0, 'no bf16 weight shadows: the probe would not measure their refresh'

    for f in forms.values():                                 # warm-up
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    us = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, f in forms.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.updates):
                f()
            e.record()
            e.synchronize()
            us[name].append(round(a.elapsed_time(e) * 1000.0 / args.updates, 2))
    res = {'probe': 'optim', 'config': 'A', 'parameters': sum(p.numel() for p in params), 'bf16_shadows': shadows,
           'updates_per_round': args.updates, 'us_per_update': us,
           'median_low_high_us': {k: [round(statistics.median(t), 2), min(t), max(t)] for k, t in us.items()},
           'device': torch.cuda.get_device_name(dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
