#!/usr/bin/env python3
"""What stochastic depth costs in the captured training step of config A on the MI355X.

    python3 profiles/droppath_probe.py [--batch 1024] [--rounds 5] [--steps 10] [--rate 0.1] [--kernels] [--out FILE]

Config A (64^2 pairs, patch 8, D 384, 8 + 8 blocks, 4 bins), random weights, bf16 autocast, engine.TrainStep(use_graph=True) with
the HIP optimizer, one process: a model built with drop_path_rate 0 and one built with ``--rate``, each warmed up and captured,
then ``--rounds`` rounds that time ``--steps`` replayed steps of each, alternating (HIP events around the steps of a round; the
inputs stay on the device).  With the rate live the step adds the draw (one Bernoulli + one multiply per half), one expansion of
the scales to rows per Function, one fp32 read per row and one multiply per element in the residual epilogues and in the
kernels that write the low-precision gradient copies of the branches that drop (all but block 0 of each half).
``--kernels`` adds a per-kernel device-time table of three replays of each (torch.profiler), for telling which kernels carry a
difference.  Prints one JSON line.
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


def kernel_table(step, x, y, replays=3, top=40):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(replays):
            step.step(x, y)
        torch.cuda.synchronize()
    rows = {}
    for e in prof.key_averages():
        t = getattr(e, 'device_time_total', None)
        if t is None:
            t = getattr(e, 'cuda_time_total', 0.0)
        if t > 0:
            rows[e.key] = [round(t / replays, 1), e.count // replays]
    return dict(sorted(rows.items(), key=lambda kv: -kv[1][0])[:top])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rate', type=float, default=0.1)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    v._lib.load()
    cfg = v.config_from_yaml(os.path.join(ROOT, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml'))
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(args.batch, 2, 3, 64, 64, device=dev, generator=g) * 2 - 1
    y = (torch.rand(args.batch, 4, device=dev, generator=g) < 0.25).float()
    steps = {}
    for name, rate in (('rate_0', 0.), (f'rate_{args.rate:g}', args.rate)):
        torch.manual_seed(0)
        model = v.build_model(cfg, drop_path_rate=rate).to(dev).train()
        opt = v.optim.FlatAdamW(v.engine.param_groups_no_decay_1d(model), lr=1e-4, weight_decay=0.05)
        step = v.engine.TrainStep(model, opt, clip_grad=5.0, amp=True, use_graph=True)
        for _ in range(4):                                   # two eager steps, the capture, one more replay
            step.step(x, y)
        torch.cuda.synchronize()
        assert step._g1 is not None, 'the step was not captured'
        steps[name] = step
    ms = {name: [] for name in steps}
    for _ in range(args.rounds):
        for name, step in steps.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.steps):
                step.step(x, y)
            e.record()
            e.synchronize()
            ms[name].append(round(a.elapsed_time(e) / args.steps, 4))
    res = {'probe': 'droppath', 'config': 'A', 'batch': args.batch, 'dtype': 'bf16', 'steps_per_round': args.steps,
           'step_ms': ms, 'median_ms': {k: round(statistics.median(t), 4) for k, t in ms.items()},
           'spread_ms': {k: round(max(t) - min(t), 4) for k, t in ms.items()}, 'device': torch.cuda.get_device_name(dev)}
    names = list(ms)
    res['difference_ms'] = round(res['median_ms'][names[1]] - res['median_ms'][names[0]], 4)
    if args.kernels:
        res['kernels_us_per_step'] = {name: kernel_table(step, x, y) for name, step in steps.items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
