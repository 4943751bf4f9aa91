#!/usr/bin/env python3
"""What Muon costs on the MI355X: whole updates of config A's and config H's parameter sets under synthetic
gradients (no forward: the weight shadows do not exist, so no arm refreshes any), the Newton-Schulz launches alone from a kernel trace of
their own, and config A's replayed training step with FlatMuon against FlatAdamW.

    python3 profiles/muon_probe.py [--rounds 7] [--updates 20] [--steps 20] [--configs A,H] [--tree DIR] [--no-trace]
                                   [--out profiles/muon_probe.json]

One process for the timed arms, the arms alternating inside every round, every figure per round kept (median, lowest, highest):
  flat_muon     optim.FlatMuon.step_flat over engine.build_optimizer's three groups (6 + 3 * 5 launches), eager
  flat_adamw    optim.FlatAdamW.step_flat over the same parameters (three launches), eager
  torch_pair    torch.optim.Muon on the Muon group's tensors + torch.optim.AdamW(fused=True) on the others, after
                torch.nn.utils.clip_grad_norm_ (the clip the flat arms have inside), eager: it cannot be captured
  flat_muon_graph / flat_adamw_graph   the flat arms as ``--updates`` calls captured into one hipGraph: the device's time alone
  step_muon_lr0 / step_adamw_lr0       (config A, --steps > 0) engine.TrainStep(use_graph=True) at batch 1024 pairs at a rate of 0, where
                both arms keep equal weights
The Newton-Schulz launches: a child process of its own under ``rocprofv3 --kernel-trace --stats`` runs ``--updates`` FlatMuon updates per
config; the summed duration of muon_ns_kernel over its calls gives TF/s against the flops counted from the shapes (per step and tensor
[m, n], m <= n: 2 m^2 n for the Gram matrix, 2 m^3 for its square, 2 m^2 n for the product with X).  ``--tree DIR`` imports the package
from another checkout of the project (built there)."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = {'A': ('configs/puzzle/div2k_erosion7_4bin_patch8_64.yaml', 16), 'H': ('configs/hisfrag/hisfrag20_patch16_512.yaml', 2)}
NS_STEPS = 5


def timed(arms, rounds, calls, replays=False):
    """{arm: [us per call, one figure per round]}, the arms alternating inside every round."""
    for f in arms.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    us = {name: [] for name in arms}
    for _ in range(rounds):
        for name, f in arms.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(1 if replays else calls):
                f()
            e.record()
            e.synchronize()
            us[name].append(round(a.elapsed_time(e) * 1000.0 / calls, 2))
    return us


def summary(us):
    return {k: [round(statistics.median(t), 2), min(t), max(t)] for k, t in us.items()}


def graphed(f, calls):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            f()
    return g.replay


def muon_config(cfg, name):
    opt = types.SimpleNamespace(NAME=name, EPS=cfg.TRAIN.OPTIMIZER.EPS, BETAS=tuple(cfg.TRAIN.OPTIMIZER.BETAS), MOMENTUM=0.9)
    return types.SimpleNamespace(TRAIN=types.SimpleNamespace(OPTIMIZER=opt, BASE_LR=1e-4, WEIGHT_DECAY=0.05))


def flat_arm(v, cfg, name, dev):
    """(model, optimizer) bound to a flat buffer that holds synthetic gradients (kept: zero_grad=False)."""
    torch.manual_seed(0)
    model = v.build_model(cfg).to(dev).train()
    opt = v.engine.build_optimizer(muon_config(cfg, name), model)
    flat = v.engine.FlatGradients(model.parameters())
    flat.flat.copy_(torch.randn(flat.flat.numel(), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 1e-3)
    opt.bind_flat(flat, model)
    return model, opt


def counted_flops(opt):
    """Newton-Schulz flops of one update, from the shapes of the Muon group's tensors."""
    total = 0
    for g in opt.param_groups:
        if g.get('use_muon'):
            for p in g['params']:
                m, n = min(p.shape), max(p.shape)
                total += NS_STEPS * (2 * m * m * n + 2 * m * m * m + 2 * m * m * n)
    return total


def update_arms(v, cfg, dev):
    _, muon = flat_arm(v, cfg, 'muon', dev)
    _, adamw = flat_arm(v, cfg, 'adamw', dev)
    torch.manual_seed(0)
    ref = v.build_model(cfg).to(dev).train()
    names = {id(p): n for n, p in ref.named_parameters()}
    is_mu = lambda p: p.ndim == 2 and names[id(p)].startswith(('blocks.', 'cross_blocks.'))
    params = [p for p in ref.parameters() if p.requires_grad]
    gen = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
    t_muon = torch.optim.Muon([p for p in params if is_mu(p)], lr=1e-4, weight_decay=0.05, adjust_lr_fn='match_rms_adamw')
    t_adamw = torch.optim.AdamW([p for p in params if not is_mu(p)], lr=1e-4, weight_decay=0.05, fused=True)

    def torch_pair():
        torch.nn.utils.clip_grad_norm_(params, 5.0)
        t_muon.step()
        t_adamw.step()

    arms = {'flat_muon': lambda: muon.step_flat(5.0, zero_grad=False), 'flat_adamw': lambda: adamw.step_flat(5.0, zero_grad=False),
            'torch_pair': torch_pair}
    info = {'parameters': sum(p.numel() for p in params), 'tensors': len(params), 'muon_tensors': sum(1 for p in params if is_mu(p)),
            'ns_flops_per_update': counted_flops(muon), 'workspace_mb': round(muon._ws.numel() * 4 / 2 ** 20, 1),
            'launches_flat_muon': 6 + 3 * NS_STEPS, 'gemms_torch_muon': 3 * NS_STEPS * sum(1 for p in params if is_mu(p))}
    return arms, info, (muon, adamw, ref, t_muon, t_adamw)


def step_arms(v, cfg, dev, batch=1024):
    S, C = cfg.DATA.IMG_SIZE, cfg.MODEL.NUM_CLASSES
    x = torch.randn(batch, 2, 3, S, S, device=dev).clamp_(-1, 1)
    y = (torch.rand(batch, C, device=dev) > 0.75).float()
    arms = {}
    for name, opt_name in (('step_adamw_lr0', 'adamw'), ('step_muon_lr0', 'muon')):
        torch.manual_seed(0)
        model = v.build_model(cfg).to(dev).train()
        mc = muon_config(cfg, opt_name)
        mc.TRAIN.BASE_LR = 0.0
        opt = v.engine.build_optimizer(mc, model)
        step = v.engine.TrainStep(model, opt, clip_grad=5.0, amp=True, use_graph=True)
        for _ in range(4):                           # two eager steps, the capture, one replay
            step.step(x, y)
        if step._g_opt is None:
            raise RuntimeError('the step was not captured')
        arms[name] = lambda step=step: step.step(x, y)
    return arms


def traced_child(v, args, dev):
    """Under rocprofv3: ``--updates`` FlatMuon updates of one config, nothing else."""
    path, _ = CONFIGS[args.configs]
    _, opt = flat_arm(v, v.config_from_yaml(os.path.join(args.tree, path)), 'muon', dev)
    for _ in range(args.updates):
        opt.step_flat(5.0, zero_grad=False)
    torch.cuda.synchronize()
    print(json.dumps({'ns_flops_per_update': counted_flops(opt)}))


def ns_trace(args, name, flops):
    """TF/s of the Newton-Schulz launches of config ``name`` from a kernel trace of its own, or why there is none."""
    rocprof = shutil.which('rocprofv3') or os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'bin', 'rocprofv3')
    if not os.path.exists(rocprof):
        return {'not_measured': 'no rocprofv3'}
    out = tempfile.mkdtemp(prefix='muon_trace_')
    try:
        cmd = [rocprof, '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '--', sys.executable, os.path.abspath(__file__), '--traced-child', '--configs', name,
               '--updates', str(args.updates), '--tree', args.tree]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
        if run.returncode != 0 or not files:
            return {'not_measured': f'rocprofv3 exited with {run.returncode} and left {len(files)} kernel_stats.csv'}
        rows = [r for r in csv.DictReader(open(files[0])) if 'muon_ns_kernel' in r['Name']]
        ns, calls = sum(int(r['TotalDurationNs']) for r in rows), sum(int(r['Calls']) for r in rows)
        if calls != 3 * NS_STEPS * args.updates:
            return {'not_measured': f'{calls} muon_ns_kernel calls in the trace, {3 * NS_STEPS * args.updates} expected'}
        per_update_us = ns / args.updates / 1000.0
        return {'ns_us_per_update': round(per_update_us, 1), 'tflops': round(flops / (per_update_us * 1e-6) / 1e12, 1), 'calls': calls,
                'per_kernel_us_per_update': {r['Name'][:40]: round(int(r['TotalDurationNs']) / args.updates / 1000.0, 1) for r in rows}}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--updates', type=int, default=20)
    ap.add_argument('--steps', type=int, default=20, help='replayed steps of config A per round and arm (0: leave the step arms out)')
    ap.add_argument('--configs', default='A,H')
    ap.add_argument('--tree', default=os.path.dirname(HERE))
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--traced-child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--out', default=os.path.join(HERE, 'muon_probe.json'))
    args = ap.parse_args()
    args.tree = os.path.abspath(args.tree)
    sys.path.insert(0, args.tree)
    import vited_amd as v
    dev = torch.device('cuda:0')
    v._lib.load()
    if args.traced_child:
        return traced_child(v, args, dev)
    res = {'probe': 'muon', 'ns_steps': NS_STEPS, 'updates_per_round': args.updates, 'steps_per_round': args.steps, 'rounds': args.rounds,
           'device': torch.cuda.get_device_name(dev), 'tree': args.tree if args.tree != os.path.dirname(HERE) else '.', 'configs': {}}
    for name in args.configs.split(','):
        path, _ = CONFIGS[name]
        cfg = v.config_from_yaml(os.path.join(args.tree, path))
        arms, info, keep = update_arms(v, cfg, dev)
        us = timed(arms, args.rounds, args.updates)
        flat = {k + '_graph': graphed(arms[k], args.updates) for k in ('flat_muon', 'flat_adamw')}
        us.update(timed(flat, args.rounds, args.updates, replays=True))
        med = summary(us)
        info.update(us_per_update=us, median_low_high_us=med, ranges_overlap=not med['flat_muon'][2] < med['torch_pair'][1],
                    torch_pair_over_flat_muon=round(med['torch_pair'][0] / med['flat_muon'][0], 2))
        del arms, flat, keep
        torch.cuda.empty_cache()
        info['newton_schulz'] = {'not_measured': '--no-trace'} if args.no_trace else ns_trace(args, name, info['ns_flops_per_update'])
        if name == 'A' and args.steps > 0:
            us = timed(step_arms(v, cfg, dev), args.rounds, args.steps)
            info.update(step_us=us, step_median_low_high_us=summary(us))
        res['configs'][name] = info
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
