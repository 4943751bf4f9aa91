#!/usr/bin/env python3
"""What a per-iteration learning-rate schedule costs a training step on the MI355X, stepped by the host and stepped on the device
(DESIGN.md section 28), and what the schedule launch costs alone.

    python3 profiles/lrsched_probe.py [--arms A,H,kernel] [--order none,host,device] [--rounds 7] [--steps 20]
                                      [--out profiles/lrsched_probe.json]

A       config A (64-pixel patch pairs, patch 8, 384 wide, 8 + 8 blocks), B 1,024, bf16, FlatAdamW, engine.TrainStep(use_graph=True):
        three models in ONE process - no scheduler (the rate fixed at WARMUP_LR), the cosine schedule of the config stepped by the host
        (``on_device = False``: the rate is uploaded in front of every update by a host-synchronous copy), the same schedule stepped on
        the device - each warmed up
        and captured, then ``--rounds`` rounds that time ``--steps`` replayed steps of each, alternating (device events around a
        round's steps; the inputs stay on the device).
H       config H (512-pixel fragments, patch 16, 12 + 12 blocks), 24 images, the two-stage step of bench.py's H-train leg (encoder once
        per image, 72 mined pairs through the decoder, launched eagerly), the same three arms, timed the same way.
``--order`` is the order in which the three models are built and timed inside a round (a control for where a model's buffers landed).
kernel  vited_lr_schedule_step alone on a two-group hyper array: device events around ``--reps`` launches; and what the host spends on
        ``step_device()`` and ``step_update(n)`` per update (a host clock, no synchronise inside).
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ('none', 'host', 'device')
ITERS_PER_EPOCH = 1000          # of the schedule: 20 warm-up epochs, so every timed update lies in the warm-up and changes the rate


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
    med = {k: round(statistics.median(t), 4) for k, t in ms.items()}
    res = {'step_ms': ms, 'median_ms': med, 'lowest_ms': {k: min(t) for k, t in ms.items()}, 'highest_ms': {k: max(t) for k, t in ms.items()}}
    spread = max(max(t) - min(t) for t in ms.values())
    res['largest_spread_ms'] = round(spread, 4)
    res['device_minus_host_ms'] = round(med['device'] - med['host'], 4)
    res['host_minus_none_ms'] = round(med['host'] - med['none'], 4)
    res['difference_exceeds_spread'] = abs(res['device_minus_host_ms']) > spread
    return res


def build(v, torch, cfg, arm, dev, **step_kw):
    torch.manual_seed(0)
    model = v.build_model(cfg).to(dev).train()
    # without a scheduler the rate stays at the warm-up's start, so that all three arms train at rates of the same size
    opt = v.optim.FlatAdamW(v.engine.param_groups_no_decay_1d(model), lr=cfg.TRAIN.WARMUP_LR if arm == 'none' else cfg.TRAIN.BASE_LR,
                            weight_decay=0.05)
    sched = None
    if arm != 'none':
        sched = v.engine.build_scheduler(cfg, opt, ITERS_PER_EPOCH)
        sched.on_device = None if arm == 'device' else False
    step = v.engine.TrainStep(model, opt, clip_grad=5.0, amp=True, lr_scheduler=sched, **step_kw)
    if step.lr_on_device != (arm == 'device'):
        raise SystemExit(f'arm {arm}: device stepping is {step.lr_on_device}')
    return opt, step


def uploads(opts, before):
    return {arm: opts[arm].hyper_uploads - before[arm] for arm in ARMS}


def arm_a(v, torch, dev, args):
    cfg = v.config_from_yaml(os.path.join(ROOT, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml'))
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(args.batch, 2, 3, 64, 64, device=dev, generator=g) * 2 - 1
    y = (torch.rand(args.batch, 4, device=dev, generator=g) < 0.25).float()
    runs, opts = {}, {}
    for arm in args.order:
        opts[arm], step = build(v, torch, cfg, arm, dev, use_graph=True)
        for _ in range(4):                                   # two eager steps, the capture, one more replay
            step.step(x, y)
        torch.cuda.synchronize()
        if step._g1 is None:
            raise SystemExit('the config A step was not captured')
        runs[arm] = (lambda s=step: s.step(x, y))
    before = {arm: opts[arm].hyper_uploads for arm in ARMS}
    res = summary(timed_rounds(torch, args.steps, runs, args.rounds))
    res.update(batch=args.batch, replayed=True, hyper_uploads_in_the_timed_steps=uploads(opts, before))
    return res


def arm_h(v, torch, dev, args):
    cfg = v.config_from_yaml(os.path.join(ROOT, 'configs', 'hisfrag', 'hisfrag20_patch16_512.yaml'))
    images = args.images
    samples = torch.randn(images, 3, 512, 512, device=dev).clamp_(-1, 1)
    targets = torch.arange(images // 3, device=dev).repeat_interleave(3)
    pairs, labels = v.engine.mine_pairs(targets, generator=torch.Generator(device=dev).manual_seed(0))

    def two_stage(m, batch):
        imgs, idx = batch
        feats = m(imgs, forward_first_part=True)
        return m(feats[idx[:, 1]], imgs[idx[:, 0]])

    runs, opts = {}, {}
    for arm in args.order:
        opts[arm], step = build(v, torch, cfg, arm, dev, use_graph=False, forward_fn=two_stage)
        for _ in range(3):
            step.step((samples, pairs), labels)
        torch.cuda.synchronize()
        runs[arm] = (lambda s=step: s.step((samples, pairs), labels))
    before = {arm: opts[arm].hyper_uploads for arm in ARMS}
    res = summary(timed_rounds(torch, max(args.steps // 2, 1), runs, args.rounds))
    res.update(images=images, pairs=int(pairs.shape[0]), replayed=False, hyper_uploads_in_the_timed_steps=uploads(opts, before))
    return res


def arm_kernel(v, torch, dev, args):
    p = [torch.nn.Parameter(torch.zeros(2, device=dev)), torch.nn.Parameter(torch.zeros(2, device=dev))]
    cfg = v.config_from_yaml(os.path.join(ROOT, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml'))
    opt = torch.optim.SGD([{'params': [p[0]]}, {'params': [p[1]], 'lr_scale': 0.1}], lr=cfg.TRAIN.BASE_LR)
    rows = {}
    for name, start in (('warm-up', 0), ('cosine', 20 * ITERS_PER_EPOCH)):
        sched = v.engine.build_scheduler(cfg, opt, ITERS_PER_EPOCH)
        table = torch.tensor(sched._table_words(), dtype=torch.float64, device=dev)
        base = torch.tensor(sched.base_values, dtype=torch.float64, device=dev)
        scale = torch.tensor([1.0, 0.1], dtype=torch.float64, device=dev)
        counter = torch.full((1,), start, dtype=torch.int64, device=dev)
        hyper, last = torch.zeros(24, device=dev), torch.zeros(2, device=dev)
        fn = lambda: v.ops.lr_schedule_step(table, base, scale, counter, hyper, 8, 8, last)
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
            out.append(round(a.elapsed_time(e) / args.reps * 1e3, 2))      # us, launch to launch
        rows[name] = {'median_us': statistics.median(out), 'lowest_us': min(out), 'highest_us': max(out)}
    rows['host_enqueue'] = host_enqueue(v, torch, dev, cfg, args)
    return rows


def host_enqueue(v, torch, dev, cfg, args):
    """What the host spends per update on a device-stepped schedule: ``step_device()`` (checks + launch) and ``step_update(n)`` (the
    mirror), a host clock around ``--reps`` calls with no synchronise inside - the enqueue, not the kernel."""
    model = torch.nn.Linear(64, 64).to(dev)
    opt = v.optim.FlatAdamW(v.engine.param_groups_no_decay_1d(model), lr=cfg.TRAIN.BASE_LR)
    opt.bind_flat(v.engine.FlatGradients(model.parameters()))
    opt.sync_hyperparameters()
    sched = v.engine.build_scheduler(cfg, opt, ITERS_PER_EPOCH)
    sched.attach(opt, 0)
    out = {'step_device_us': [], 'step_update_us': []}
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            sched.step_device()
        t1 = time.perf_counter()
        for n in range(args.reps):
            sched.step_update(n)
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        out['step_device_us'].append(round((t1 - t0) / args.reps * 1e6, 2))
        out['step_update_us'].append(round((t2 - t1) / args.reps * 1e6, 2))
    return {k: {'median_us': statistics.median(t), 'lowest_us': min(t), 'highest_us': max(t)} for k, t in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arms', default='A,H,kernel')
    ap.add_argument('--order', default=','.join(ARMS))
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--images', type=int, default=24)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    args.order = args.order.split(',')
    if sorted(args.order) != sorted(ARMS):
        raise SystemExit(f'--order names each of {ARMS} once')
    sys.path.insert(0, ROOT)
    import torch
    import vited_amd as v
    if not torch.cuda.is_available():
        raise SystemExit('lrsched_probe.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    v._lib.load()
    arms = args.arms.split(',')
    res = {'probe': 'lrsched', 'dtype': 'bf16', 'order': args.order, 'rounds': args.rounds, 'steps_per_round': args.steps, 'device': torch.cuda.get_device_name(dev)}
    if 'A' in arms:
        res['config_A'] = arm_a(v, torch, dev, args)
        print(f"config A replayed: {res['config_A']['median_ms']}", file=sys.stderr, flush=True)
    if 'H' in arms:
        res['config_H_two_stage'] = arm_h(v, torch, dev, args)
        print(f"config H: {res['config_H_two_stage']['median_ms']}", file=sys.stderr, flush=True)
    if 'kernel' in arms:
        res['schedule_launch'] = arm_kernel(v, torch, dev, args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
