#!/usr/bin/env python3
"""What patch dropout (timm PatchDropout) buys a training step on the MI355X, and what its kernels cost.

    python3 profiles/patchdrop_probe.py [--rates 0,0.25,0.5] [--arms A,H,kernels] [--rounds 5] [--steps 10]
                                        [--tree DIR] [--compare-tree DIR] [--out profiles/patchdrop_probe.json]

A     config A (64-pixel patch pairs, patch 8, 384 wide, 8 + 8 blocks), B 1,024, bf16, FlatAdamW, engine.TrainStep(use_graph=True):
      one model per rate in ONE process, each warmed up and captured, then ``--rounds`` rounds that time ``--steps`` replayed steps
      of each, alternating (device events around a round's steps; the inputs stay on the device).
H     config H (512-pixel fragments, patch 16, 12 + 12 blocks), 24 images, the two-stage step of bench.py's H-train leg (encoder
      once per image, 72 mined pairs through the decoder, launched eagerly), one model per rate, timed the same way.
kernels  the new kernels alone at the sizes of A and H at rate 0.5, device events around ``--reps`` launches.
With a live rate the draw (randn + the ranking kernel) is part of every step.  Token-count ratio: tokens per image pair at the
rate over tokens at rate 0 - the most the step could shrink by if every kernel scaled with the rows (attention shrinks faster,
the optimizer, the weight-gradient outputs and the launches not at all).

``--tree DIR`` imports the package from another checkout of the project (built there); a rate of 0 passes no ``patch_drop_rate``
argument, so the probe also runs on a tree from before the option existed.  ``--compare-tree DIR`` first runs the rate-0 arms of
DIR and of this tree in fresh child processes, alternating (``--compare-first`` says which leads), ``--compare-rounds`` times each: the rate-0 step of this tree against
the parent commit, with the spread of the parent's own repeats beside it.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def keep_count(tokens, rate):
    return max(1, int(tokens * (1. - rate)))


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
    return {'step_ms': ms, 'median_ms': {k: round(statistics.median(t), 4) for k, t in ms.items()},
            'spread_ms': {k: round(max(t) - min(t), 4) for k, t in ms.items()}}


def build(v, cfg, rate, dev):
    import torch
    torch.manual_seed(0)
    kw = {'patch_drop_rate': rate} if rate > 0 else {}          # rate 0: the call a tree without the option understands
    model = v.build_model(cfg, **kw).to(dev).train()
    opt = v.optim.FlatAdamW(v.engine.param_groups_no_decay_1d(model), lr=1e-4, weight_decay=0.05)
    return model, opt


def arm_a(v, torch, dev, rates, args):
    cfg = v.config_from_yaml(os.path.join(args.tree, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml'))
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(args.batch, 2, 3, 64, 64, device=dev, generator=g) * 2 - 1
    y = (torch.rand(args.batch, 4, device=dev, generator=g) < 0.25).float()
    runs = {}
    for rate in rates:
        model, opt = build(v, cfg, rate, dev)
        step = v.engine.TrainStep(model, opt, clip_grad=5.0, amp=True, use_graph=True)
        for _ in range(4):                                   # two eager steps, the capture, one more replay
            step.step(x, y)
        torch.cuda.synchronize()
        if step._g1 is None:
            raise SystemExit('the config A step was not captured')
        runs[f'rate_{rate:g}'] = (lambda s=step: s.step(x, y))
    res = summary(timed_rounds(torch, args.steps, runs, args.rounds))
    res.update(batch=args.batch, tokens={f'rate_{r:g}': [1 + keep_count(63, r), 1 + keep_count(64, r)] if r > 0 else [64, 65] for r in rates})
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
    res.update(images=images, pairs=int(pairs.shape[0]),
               tokens={f'rate_{r:g}': [1 + keep_count(1023, r), 1 + keep_count(1024, r)] if r > 0 else [1024, 1025] for r in rates})
    return res


def arm_kernels(v, torch, dev, args):
    ops = v.ops

    def timed(fn):
        for _ in range(3):
            fn()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.reps):
            fn()
        e.record()
        e.synchronize()
        return round(a.elapsed_time(e) / args.reps * 1e3, 2)      # us

    rows = []
    # (name, samples, image size, patch, dim, with cls)
    for name, b, size, patch, d, with_cls in (('A image 1', 1024, 64, 8, 384, False), ('A image 2', 1024, 64, 8, 384, True),
                                              ('H image 1', 24, 512, 16, 384, False), ('H image 2 (72 pairs)', 72, 512, 16, 384, True)):
        n, lead = (size // patch) ** 2, not with_cls
        k = keep_count(n - lead, 0.5)
        r = k + lead
        keys = torch.randn(b, n - lead, device=dev)
        keep = ops.keep_from_keys(keys, k)
        img = torch.randn(b, 3, size, size, device=dev)
        u8 = torch.randint(0, 256, (b, 3, size, size), device=dev, dtype=torch.uint8)
        tok, pos, cls = torch.randn(b * r, d, device=dev), torch.randn(n + 1, d, device=dev), torch.randn(d, device=dev)
        dx = torch.randn(b, r + with_cls, d, device=dev)
        inv = ops.keep_inverse(keep, lead, n)
        rows.append({
            'case': name, 'samples': b, 'patches': n, 'kept_rows': r, 'dim': d,
            'keep_from_keys_us': timed(lambda: ops.keep_from_keys(keys, k)),
            'patchify_kept_us': timed(lambda: ops.patchify_kept(img, patch, torch.bfloat16, keep, lead)),
            'patchify_full_us': timed(lambda: ops.patchify(img, patch, torch.bfloat16)),
            'patchify_kept_u8_us': timed(lambda: ops.patchify_kept(u8, patch, torch.bfloat16, keep, lead)),
            'tokens_kept_us': timed(lambda: ops.tokens_kept(tok, pos, cls if with_cls else None, keep, lead)),
            'keep_inverse_us': timed(lambda: ops.keep_inverse(keep, lead, n)),
            'tokens_kept_bwd_us': timed(lambda: ops.tokens_kept_bwd(dx, inv, with_cls)),
        })
    return rows


def measure(args):
    sys.path.insert(0, args.tree)
    import torch
    import vited_amd as v
    if not torch.cuda.is_available():
        raise SystemExit('patchdrop_probe.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    v._lib.load()
    rates = [float(r) for r in args.rates.split(',')]
    arms = args.arms.split(',')
    res = {'probe': 'patchdrop', 'tree': os.path.basename(os.path.abspath(args.tree)), 'dtype': 'bf16', 'rounds': args.rounds,
           'steps_per_round': args.steps, 'device': torch.cuda.get_device_name(dev)}
    if 'A' in arms:
        res['config_A'] = arm_a(v, torch, dev, rates, args)
        print(f"config A: {res['config_A']['median_ms']}", file=sys.stderr, flush=True)
    if 'H' in arms:
        res['config_H_two_stage'] = arm_h(v, torch, dev, rates, args)
    if 'kernels' in arms:
        res['kernels_rate_0.5'] = arm_kernels(v, torch, dev, args)
    for key in ('config_A', 'config_H_two_stage'):
        if key in res and 'rate_0' in res[key]['median_ms']:
            base, tok = res[key]['median_ms']['rate_0'], res[key]['tokens']
            res[key]['time_ratio'] = {k: round(t / base, 4) for k, t in res[key]['median_ms'].items()}
            res[key]['token_ratio'] = {k: round(sum(t) / sum(tok['rate_0']), 4) for k, t in tok.items()}
    return res


def compare(args):
    """Rate-0 arms of the other tree and of this one, in fresh child processes, alternating."""
    out = {'parent': [], 'this': []}
    for _ in range(args.compare_rounds):
        for name, tree in sorted((('parent', args.compare_tree), ('this', ROOT)), reverse=args.compare_first == 'this'):
            cmd = [sys.executable, os.path.abspath(__file__), '--tree', tree, '--rates', '0', '--arms', 'A,H', '--rounds', str(args.rounds),
                   '--steps', str(args.steps), '--batch', str(args.batch), '--images', str(args.images)]
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            if done.returncode != 0:              # nothing more is started on the GPU after a child that failed
                raise SystemExit(f'{name} tree: exit status {done.returncode}\n{done.stdout[-2000:]}\n{done.stderr[-2000:]}')
            got = json.loads(done.stdout.strip().splitlines()[-1])
            out[name].append({k: got[k]['median_ms']['rate_0'] for k in ('config_A', 'config_H_two_stage')})
            print(f'{name} tree, rate 0: {out[name][-1]}', file=sys.stderr, flush=True)
    res = {'runs_ms': out}
    for key in ('config_A', 'config_H_two_stage'):
        p, t = [r[key] for r in out['parent']], [r[key] for r in out['this']]
        res[key] = {'parent_median_ms': round(statistics.median(p), 4), 'this_median_ms': round(statistics.median(t), 4),
                    'parent_spread_ms': round(max(p) - min(p), 4), 'this_spread_ms': round(max(t) - min(t), 4),
                    'difference_ms': round(statistics.median(t) - statistics.median(p), 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rates', default='0,0.25,0.5')
    ap.add_argument('--arms', default='A,H,kernels')
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--images', type=int, default=24)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--compare-tree', default=None)
    ap.add_argument('--compare-rounds', type=int, default=3)
    ap.add_argument('--compare-first', default='parent', choices=['parent', 'this'], help='which tree runs first in every round')
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
