#!/usr/bin/env python3
"""What position dropout (timm's pos_drop) costs a training step on the MI355X, and what its kernel costs alone.

    python3 profiles/posdrop_probe.py [--rates 0,0.1] [--arms A,A_eager,H,kernels] [--rounds 5] [--steps 10]
                                      [--tree DIR] [--compare-tree DIR] [--out profiles/posdrop_probe.json]

A        config A (64-pixel patch pairs, patch 8, 384 wide, 8 + 8 blocks), B 1,024, bf16, FlatAdamW, engine.TrainStep(use_graph=True):
         one model per rate in ONE process, each warmed up and captured, then ``--rounds`` rounds that time ``--steps`` replayed steps
         of each, alternating (device events around a round's steps; the inputs stay on the device).
A_eager  the same step launched eagerly (use_graph=False).
H        config H (512-pixel fragments, patch 16, 12 + 12 blocks), 24 images, the two-stage step of bench.py's H-train leg (encoder
         once per image, 72 mined pairs through the decoder, launched eagerly), one model per rate, timed the same way.
kernels  vited_token_dropout alone on the fp32 streams of A and H (and on bf16 copies), out of place and in place, device events
         around ``--reps`` launches; GB/s counts one read and one write of the stream.
With a live rate the draw of the two seeds (torch.randint) and four applications of the kernel (two streams, forward and backward)
are part of every step.

``--tree DIR`` imports the package from another checkout of the project (built there); a rate of 0 passes no ``pos_drop_rate``
argument, so the probe also runs on a tree from before the option existed.  ``--compare-tree DIR`` first runs the rate-0 arms A and
A_eager of DIR and of this tree in fresh child processes, alternating, ``--compare-rounds`` times each: the rate-0 step of this tree
against the parent commit, with the spread of the parent's own repeats beside it.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed_rounds(torch, steps, runs, rounds):
    """{name: [ms per step of every round]} of the callables in ``runs``, alternating between them round by round."""
    ms = {name: [] for name in runs}
    for _ in range(rounds):
        for name, run in runs.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(steps):
                run()
            e.record()
            e.synchronize()
            ms[name].append(round(a.elapsed_time(e) / steps, 4))
    return ms


def summary(ms):
    res = {'step_ms': ms, 'median_ms': {k: round(statistics.median(t), 4) for k, t in ms.items()},
           'lowest_ms': {k: min(t) for k, t in ms.items()}, 'highest_ms': {k: max(t) for k, t in ms.items()}}
    if 'rate_0' in ms:
        res['time_ratio'] = {k: round(t / res['median_ms']['rate_0'], 4) for k, t in res['median_ms'].items()}
    return res


def build(v, cfg, rate, dev):
    import torch
    torch.manual_seed(0)
    kw = {'pos_drop_rate': rate} if rate > 0 else {}            # rate 0: the call a tree without the option understands
    model = v.build_model(cfg, **kw).to(dev).train()
    opt = v.optim.FlatAdamW(v.engine.param_groups_no_decay_1d(model), lr=1e-4, weight_decay=0.05)
    return model, opt


def arm_a(v, torch, dev, rates, args, use_graph):
    cfg = v.config_from_yaml(os.path.join(args.tree, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml'))
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(args.batch, 2, 3, 64, 64, device=dev, generator=g) * 2 - 1
    y = (torch.rand(args.batch, 4, device=dev, generator=g) < 0.25).float()
    runs = {}
    for rate in rates:
        model, opt = build(v, cfg, rate, dev)
        step = v.engine.TrainStep(model, opt, clip_grad=5.0, amp=True, use_graph=use_graph)
        for _ in range(4):                                   # two eager steps, the capture, one more replay
            step.step(x, y)
        torch.cuda.synchronize()
        if use_graph and step._g1 is None:
            raise SystemExit('the config A step was not captured')
        runs[f'rate_{rate:g}'] = (lambda s=step: s.step(x, y))
    res = summary(timed_rounds(torch, args.steps, runs, args.rounds))
    res.update(batch=args.batch, replayed=bool(use_graph))
    return res


def arm_h(v, torch, dev, rates, args):
    cfg = v.config_from_yaml(os.path.join(args.tree, 'configs', 'hisfrag', 'hisfrag20_patch16_512.yaml'))
    images = args.images
    samples = torch.randn(images, 3, 512, 512, device=dev).clamp_(-1, 1)
    targets = torch.arange(images // 3, device=dev).repeat_interleave(3)
    pairs, labels = v.engine.mine_pairs(targets, generator=torch.Generator(device=dev).manual_seed(0))

    def two_stage(m, batch):
        imgs, idx = batch
        feats = m(imgs, forward_first_part=True)
        return m(feats[idx[:, 1]], imgs[idx[:, 0]])

    runs = {}
    for rate in rates:
        model, opt = build(v, cfg, rate, dev)
        step = v.engine.TrainStep(model, opt, clip_grad=5.0, amp=True, use_graph=False, forward_fn=two_stage)
        for _ in range(3):
            step.step((samples, pairs), labels)
        torch.cuda.synchronize()
        runs[f'rate_{rate:g}'] = (lambda s=step: s.step((samples, pairs), labels))
    res = summary(timed_rounds(torch, max(args.steps // 2, 1), runs, args.rounds))
    res.update(images=images, pairs=int(pairs.shape[0]))
    return res


def arm_kernels(v, torch, dev, args):
    ops = v.ops

    def timed(fn):
        for _ in range(3):
            fn()
        out = []
        for _ in range(args.rounds):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.reps):
                fn()
            e.record()
            e.synchronize()
            out.append(round(a.elapsed_time(e) / args.reps * 1e3, 2))      # us
        return {'median_us': statistics.median(out), 'lowest_us': min(out), 'highest_us': max(out)}

    rows = []
    seed = torch.tensor([12345], dtype=torch.int64, device=dev)
    for name, b, tokens, d, stream in (('A image 1', 1024, 64, 384, 0), ('A image 2', 1024, 65, 384, 1), ('H image 1', 24, 1024, 384, 0),
                                       ('H image 2 (72 pairs)', 72, 1025, 384, 1)):
        for dtype in (torch.float32, torch.bfloat16):
            x = torch.randn(b, tokens, d, device=dev).to(dtype)
            out = torch.empty_like(x)
            apart = timed(lambda: ops.token_dropout(x, seed, 0.1, tokens, stream, out=out))
            in_place = timed(lambda: ops.token_dropout(x, seed, 0.1, tokens, stream, out=x))
            nbytes = 2 * x.numel() * x.element_size()
            rows.append({'case': name, 'dtype': str(dtype).replace('torch.', ''), 'elements': x.numel(), 'out_of_place': apart, 'in_place': in_place,
                         'out_of_place_GBps': round(nbytes / apart['median_us'] / 1e3, 1), 'in_place_GBps': round(nbytes / in_place['median_us'] / 1e3, 1)})
    return rows


def measure(args):
    sys.path.insert(0, args.tree)
    import torch
    import vited_amd as v
    if not torch.cuda.is_available():
        raise SystemExit('posdrop_probe.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    v._lib.load()
    rates = [float(r) for r in args.rates.split(',')]
    arms = args.arms.split(',')
    res = {'probe': 'posdrop', 'tree': os.path.basename(os.path.abspath(args.tree)), 'dtype': 'bf16', 'rounds': args.rounds,
           'steps_per_round': args.steps, 'device': torch.cuda.get_device_name(dev)}
    if 'A' in arms:
        res['config_A'] = arm_a(v, torch, dev, rates, args, True)
        print(f"config A replayed: {res['config_A']['median_ms']}", file=sys.stderr, flush=True)
    if 'A_eager' in arms:
        res['config_A_eager'] = arm_a(v, torch, dev, rates, args, False)
        print(f"config A eager: {res['config_A_eager']['median_ms']}", file=sys.stderr, flush=True)
    if 'H' in arms:
        res['config_H_two_stage'] = arm_h(v, torch, dev, rates, args)
        print(f"config H: {res['config_H_two_stage']['median_ms']}", file=sys.stderr, flush=True)
    if 'kernels' in arms:
        res['kernel_rate_0.1'] = arm_kernels(v, torch, dev, args)
    return res


def compare(args):
    """Rate-0 arms of the other tree and of this one, in fresh child processes, alternating."""
    keys = ('config_A', 'config_A_eager')
    out = {'parent': [], 'this': []}
    for _ in range(args.compare_rounds):
        for name, tree in (('parent', args.compare_tree), ('this', ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), '--tree', tree, '--rates', '0', '--arms', 'A,A_eager', '--rounds', str(args.rounds),
                   '--steps', str(args.steps), '--batch', str(args.batch)]
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            if done.returncode != 0:              # nothing more is started on the GPU after a child that failed
                raise SystemExit(f'{name} tree: exit status {done.returncode}\n{done.stdout[-2000:]}\n{done.stderr[-2000:]}')
            got = json.loads(done.stdout.strip().splitlines()[-1])
            out[name].append({k: got[k]['median_ms']['rate_0'] for k in keys})
            print(f'{name} tree, rate 0: {out[name][-1]}', file=sys.stderr, flush=True)
    res = {'runs_ms': out}
    for key in keys:
        p, t = [r[key] for r in out['parent']], [r[key] for r in out['this']]
        res[key] = {'parent_median_ms': round(statistics.median(p), 4), 'this_median_ms': round(statistics.median(t), 4),
                    'parent_lowest_ms': min(p), 'parent_highest_ms': max(p), 'this_lowest_ms': min(t), 'this_highest_ms': max(t),
                    'difference_ms': round(statistics.median(t) - statistics.median(p), 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rates', default='0,0.1')
    ap.add_argument('--arms', default='A,A_eager,H,kernels')
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--images', type=int, default=24)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--compare-tree', default=None)
    ap.add_argument('--compare-rounds', type=int, default=3)
    ap.add_argument('--child-timeout', type=int, default=240)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rate0 = compare(args) if args.compare_tree else None       # before this process opens the GPU itself
    res = measure(args)
    if rate0 is not None:
        res['rate_0_against_parent'] = rate0
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
