#!/usr/bin/env python3
"""The two-stage training step of config H on the MI355X: gathered pairs against the pair-indexed decoder.

    python3 profiles/pair_index_probe.py [--images 24] [--blocks 5] [--steps 10] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python3 profiles/pair_index_probe.py --trace indexed|gathered [--rule hisfrag|michigan]

Config H (512^2 images, patch 16, D 384, 6 heads, 12 + 12 blocks), random weights, bf16 autocast, engine.TrainStep (eager) with the
HIP optimizer, bench.py's H-train geometry: 24 images of 8 writers x 3 -> 24 positive pairs + 48 negatives = 72 pairs under
hisfrag.py's rule, 24 + 24 = 48 pairs under michigan's (mine_pairs(neg_per_pos=1, ordered_negatives=True)).  One process, two models
from the same seed:
  gathered   m(feats[pairs[:, 1]], imgs[pairs[:, 0]])                               - the form bench.py keeps
  indexed    m(feats, imgs, x2_index=pairs[:, 0], x1_index=pair_segments(pairs[:, 1]))
First one step of each on the same seeded batch from the same state (loss and gradient norm must agree), then both are warmed and
timed in alternating blocks of ``--steps`` steps (HIP events around a block that ends in a synchronise); the median of ``--blocks``
blocks is reported with [lowest .. highest].  ``--trace FORM`` instead runs three warm steps and three more of one form and exits:
the body of a kernel-trace run.  Prints one JSON line.
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

RULES = {'hisfrag': dict(neg_per_pos=2.0, ordered_negatives=False), 'michigan': dict(neg_per_pos=1.0, ordered_negatives=True)}


def gathered(m, batch):
    imgs, pairs, _ = batch
    feats = m(imgs, forward_first_part=True)
    return m(feats[pairs[:, 1]], imgs[pairs[:, 0]])


def indexed(m, batch):
    imgs, pairs, seg = batch
    feats = m(imgs, forward_first_part=True)
    return m(feats, imgs, x2_index=pairs[:, 0], x1_index=seg)


FORMS = {'gathered': gathered, 'indexed': indexed}


def make_step(cfg, dev, form):
    torch.manual_seed(0)
    model = v.build_model(cfg).to(dev).train()
    opt = v.optim.FlatAdamW(v.engine.param_groups_no_decay_1d(model), model=model, lr=1e-4 * 24 / 256, weight_decay=0.05)
    return v.engine.TrainStep(model, opt, clip_grad=5.0, amp=True, use_graph=False, forward_fn=FORMS[form])


def make_batch(rule, images, size, dev, seed):
    samples = torch.randn(images, 3, size, size, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).clamp_(-1, 1)
    targets = torch.arange(images // 3, device=dev).repeat_interleave(3)
    pairs, labels = v.engine.mine_pairs(targets, generator=torch.Generator(device=dev).manual_seed(seed), **RULES[rule])
    pairs = pairs.contiguous()
    return (samples, pairs, v.ops.pair_segments(pairs[:, 1], images)), labels


def timed_block(step, x, y, steps):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        step.step(x, y)
    e.record()
    e.synchronize()
    return round(a.elapsed_time(e) / steps, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=24)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--trace', choices=sorted(FORMS), default=None)
    ap.add_argument('--rule', choices=sorted(RULES), default='hisfrag')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    v._lib.load()
    cfg = v.config_from_yaml(os.path.join(ROOT, 'configs', 'hisfrag', 'hisfrag20_patch16_512.yaml'))
    size = cfg.DATA.IMG_SIZE
    if args.trace:
        step = make_step(cfg, dev, args.trace)
        x, y = make_batch(args.rule, args.images, size, dev, seed=2)
        for _ in range(6):
            step.step(x, y)
        torch.cuda.synchronize()
        print(json.dumps({'probe': 'pair_index', 'trace': args.trace, 'rule': args.rule, 'pairs': int(y.shape[0]), 'steps': 6}))
        return
    steps = {form: make_step(cfg, dev, form) for form in FORMS}
    res = {'probe': 'pair_index', 'config': 'H', 'images': args.images, 'dtype': 'bf16', 'steps_per_block': args.steps, 'blocks': args.blocks,
           'device': torch.cuda.get_device_name(dev), 'rules': {}}
    for rule in RULES:
        x, y = make_batch(rule, args.images, size, dev, seed=2)
        row = {'pairs': int(y.shape[0])}
        if rule == 'hisfrag':
            # the same seeded batch from the same state (both models are untouched here): loss and gradient norm of the first step
            first = {form: (float(step.step(x, y)), float(step.last_norm)) for form, step in steps.items()}
            row['first_step'] = {form: {'loss': round(l, 6), 'grad_norm': round(n, 6)} for form, (l, n) in first.items()}
            (lg, ng), (li, ni) = first['gathered'], first['indexed']
            row['first_step_rel_diff'] = {'loss': abs(li - lg) / abs(lg), 'grad_norm': abs(ni - ng) / ng}
            if not (abs(li - lg) <= 2e-2 * abs(lg) and abs(ni - ng) <= 2e-2 * ng):       # bf16 steps: the model tests' global bound
                raise SystemExit(f'pair_index_probe: the two forms disagree on the same batch: {row}')
        for step in steps.values():
            for _ in range(args.warmup):
                step.step(x, y)
        ms = {form: [] for form in steps}
        for _ in range(args.blocks):
            for form, step in steps.items():
                ms[form].append(timed_block(step, x, y, args.steps))
        row['step_ms'] = ms
        row['median_ms'] = {f: round(statistics.median(t), 3) for f, t in ms.items()}
        row['lowest_ms'] = {f: min(t) for f, t in ms.items()}
        row['highest_ms'] = {f: max(t) for f, t in ms.items()}
        row['spread_ms'] = {f: round(max(t) - min(t), 3) for f, t in ms.items()}
        row['difference_ms'] = round(row['median_ms']['indexed'] - row['median_ms']['gathered'], 3)
        row['indexed_is_faster_beyond_the_spreads'] = bool(-row['difference_ms'] > row['spread_ms']['indexed'] + row['spread_ms']['gathered'])
        row['peak_memory_gib'] = None
        res['rules'][rule] = row
    # peak memory of one step of each form (hisfrag rule), each after a reset
    x, y = make_batch('hisfrag', args.images, size, dev, seed=2)
    mem = {}
    for form, step in steps.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        step.step(x, y)
        torch.cuda.synchronize()
        mem[form] = round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 30, 3)
    res['rules']['hisfrag']['peak_memory_gib'] = mem
    del res['rules']['michigan']['peak_memory_gib']
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
