#!/usr/bin/env python3
"""Pair mining on the MI355X: the torch-op chain with its host reads against the one-launch kernel, alone and inside config H's
two-stage training step.

    python3 profiles/mine_pairs_probe.py [--calls 200] [--blocks 5] [--steps 10] [--skip-step] [--out FILE]

Part 1, the mining alone, per shape (24 images of 8 writers x 3 under hisfrag's and under michigan's rule; 128 images of 2 writers):
  chain    engine.mine_pairs + ops.pair_segments     - triu_indices, boolean selects, nonzero, randperm, argsort, bincount, cumsum,
                                                       and the host reads of the counts and of the range flag
  kernel   engine.mine_pairs_device                  - torch.rand + vited_mine_pairs, at the exact capacity of the shape
in alternating blocks of ``--calls`` calls between device events (a block ends in a synchronise); the median of ``--blocks`` blocks
per call, in microseconds, with [lowest .. highest].
Part 2, the whole step of config H (512^2 images, D 384, 12 + 12 blocks, bf16 autocast, 24 images, eager TrainStep, FlatAdamW):
hisfrag_prepare_indexed + step against hisfrag_prepare_mined (capacity 72) + step, two models from one seed, alternating blocks of
``--steps`` steps.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vited_amd as v  # noqa: E402

E = v.engine
SHAPES = {
    'n24_hisfrag': dict(classes=8, per=3, neg_per_pos=2.0, ordered_negatives=False),
    'n24_michigan': dict(classes=8, per=3, neg_per_pos=1.0, ordered_negatives=True),
    'n128_hisfrag': dict(classes=2, per=64, neg_per_pos=2.0, ordered_negatives=False),
}


def timed(fn, count, scale):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(count):
        fn()
    e.record()
    e.synchronize()
    return round(a.elapsed_time(e) * scale / count, 3)


def summary(times):
    return {f: {'median': round(statistics.median(t), 3), 'lowest': min(t), 'highest': max(t), 'spread': round(max(t) - min(t), 3)}
            for f, t in times.items()}


def alternate(forms, blocks, count, scale, warmup):
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    times = {f: [] for f in forms}
    for _ in range(blocks):
        for f, fn in forms.items():
            times[f].append(timed(fn, count, scale))
    return times


def mining(dev, shape, calls, blocks):
    n = shape['classes'] * shape['per']
    targets = torch.arange(shape['classes'], device=dev).repeat_interleave(shape['per'])
    rule = dict(neg_per_pos=shape['neg_per_pos'], ordered_negatives=shape['ordered_negatives'])
    capacity = E.mined_pair_capacity(n, shape['per'], **rule)
    gen = torch.Generator(device=dev).manual_seed(0)

    def chain():
        groups, _ = E.mine_pairs(targets, generator=gen, **rule)
        return v.ops.pair_segments(groups[:, 1], n)

    def kernel():
        return E.mine_pairs_device(targets, capacity, generator=gen, **rule)

    mined = kernel()
    counts = mined.counts.tolist()
    assert counts[3] == capacity and counts[4] == 0 and chain().index.numel() == capacity, (counts, capacity)
    times = alternate({'chain': chain, 'kernel': kernel}, blocks, calls, 1000.0, warmup=20)
    row = {'images': n, 'pairs': capacity, 'counts': counts, 'call_us': times, **{k + '_us': s for k, s in summary(times).items()}}
    row['difference_us'] = round(row['kernel_us']['median'] - row['chain_us']['median'], 3)
    row['kernel_is_faster_beyond_the_spreads'] = bool(-row['difference_us'] > row['kernel_us']['spread'] + row['chain_us']['spread'])
    return row


def whole_step(dev, steps, blocks, warmup):
    cfg = v.config_from_yaml(os.path.join(ROOT, 'configs', 'hisfrag', 'hisfrag20_patch16_512.yaml'))
    size, images = cfg.DATA.IMG_SIZE, 24
    samples = torch.randn(images, 3, size, size, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).clamp_(-1, 1)
    targets = torch.arange(images // 3, device=dev).repeat_interleave(3)
    forward = lambda m, b: m(b[1], b[0], x2_index=b[2], x1_index=b[3])

    def make(criterion):
        torch.manual_seed(0)
        model = v.build_model(cfg).to(dev).train()
        opt = v.optim.FlatAdamW(E.param_groups_no_decay_1d(model), model=model, lr=1e-4 * 24 / 256, weight_decay=0.05)
        return model, E.TrainStep(model, opt, clip_grad=5.0, amp=True, use_graph=False, forward_fn=forward, criterion=criterion)

    (mi, si), (mm, sm) = make(None), make(E.mined_bce_with_logits)
    gen = torch.Generator(device=dev).manual_seed(2)

    def indexed():
        batch, labels = E.hisfrag_prepare_indexed(mi, samples, targets, amp=True, generator=gen)
        return si.step(batch, labels)

    def mined():
        batch, y = E.hisfrag_prepare_mined(mm, samples, targets, 72, amp=True, generator=gen)
        return sm.step(batch, y)

    first = {'indexed': (float(indexed()), float(si.last_norm)), 'mined': (float(mined()), float(sm.last_norm))}
    times = alternate({'indexed': indexed, 'mined': mined}, blocks, steps, 1.0, warmup)
    row = {'config': 'H', 'images': images, 'pairs': 72, 'dtype': 'bf16', 'steps_per_block': steps,
           'first_step': {f: {'loss': round(l, 6), 'grad_norm': round(n, 6)} for f, (l, n) in first.items()},
           'step_ms': times, **{k + '_ms': s for k, s in summary(times).items()}}
    row['difference_ms'] = round(row['mined_ms']['median'] - row['indexed_ms']['median'], 3)
    row['mined_is_faster_beyond_the_spreads'] = bool(-row['difference_ms'] > row['mined_ms']['spread'] + row['indexed_ms']['spread'])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.calls < 200 or args.blocks < 5:
        raise SystemExit('mine_pairs_probe: at least 200 calls per block and 5 blocks')
    dev = torch.device('cuda:0')
    v._lib.load()
    res = {'probe': 'mine_pairs', 'device': torch.cuda.get_device_name(dev), 'calls_per_block': args.calls, 'blocks': args.blocks,
           'mining': {name: mining(dev, shape, args.calls, args.blocks) for name, shape in SHAPES.items()}}
    if not args.skip_step:
        res['step'] = whole_step(dev, args.steps, args.blocks, args.warmup)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
