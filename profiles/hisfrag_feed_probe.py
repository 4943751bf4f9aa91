#!/usr/bin/env python3
"""Config H fed from images resident on the MI355X: what the device loader costs next to the step.

    python3 profiles/hisfrag_feed_probe.py [--images 160] [--batch 24] [--steps 10] [--repeats 5] [--out FILE]

A synthetic store of ``--images`` random images of 600-1,200 pixels per side (160 of them are about 390 MB, past the 256 MiB
Infinity Cache), three to six per writer, S = 512, config H (patch 16, D 384, 8 + 8 blocks, one class), bf16 autocast, FlatAdamW,
no hipGraph (the pair batch is a structured input).  Measured:
  (a) ``vited_hisfrag_windows_u8``, ``vited_hisfrag_jitter_u8`` (its two kernels) and ``vited_hisfrag_blur_u8`` alone on one training
      plan with every augmentation switched on: device time per call of REPS calls queued between two events;
  (b) one full ``HisfragDeviceLoader`` iteration (uniforms, plan, the three entry points, the target gather): device time per
      iteration of a queued epoch, and the host time the iteration takes to enqueue;
  (c) the two-stage H-train step of bench.py on a fixed resident uint8 batch with its pairs mined once - the step as it was before
      the loader existed, the yardstick - against the same step on that batch with the pairs mined every step, and against the
      step taking every batch from the loader (pairs mined every step), in blocks of ``--steps`` steps that alternate
      ``--repeats`` times (host clock around a block that ends in a device synchronise).
Prints one JSON line (medians and the per-block lists).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vited_amd as v  # noqa: E402

REPS = 50


def queued_ms(fn, reps):
    """Device time per call of ``reps`` calls queued back to back between two events."""
    torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return a.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=160)
    ap.add_argument('--batch', type=int, default=24)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('hisfrag_feed_probe.py measures on the MI355X; no GPU is visible')
    dev = torch.device('cuda:0')
    v._lib.load()
    E, S, B = v.engine, 512, args.batch
    g = torch.Generator(device=dev).manual_seed(0)
    sides = torch.randint(600, 1201, (args.images, 2), generator=torch.Generator().manual_seed(0)).tolist()
    store = E.Div2kImageStore([torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=g) for h, w in sides], dev)
    labels, writer = [], 0
    while len(labels) < args.images:                             # three to six fragments per writer
        labels += [writer] * (3 + writer % 4)
        writer += 1
    labels = labels[: args.images]
    need = max(3 + 20 * args.repeats, 3 + args.steps * args.repeats) + 8      # iterations of (b) / of (c), each in an epoch of its own
    loader = E.HisfragDeviceLoader(store, labels, B, S, m=3, repeat=-(-need * B // args.images), seed=0)
    assert len(loader) >= need

    # (a) the entry points alone, every augmentation on
    plan = loader.plan(loader.rank_indices()[0], loader._generator(1))
    drawn = {name: float((plan.flags.bitwise_and(bit) != 0).float().mean()) for name, bit in (('warp', 2), ('jitter', 4), ('blur', 8))}
    plan = plan._replace(flags=torch.full_like(plan.flags, 15))
    win, jit, out = (torch.empty(B, 3, S, S, dtype=torch.uint8, device=dev) for _ in range(3))
    windows = lambda: v.ops.hisfrag_windows_u8(store.data, store.offsets_dev, store.sizes_dev, plan.image, plan.flags, plan.afix,
                                               plan.minv, plan.origin, S, out=win)
    jitter = lambda: v.ops.hisfrag_jitter_u8(win, plan.flags, plan.order, plan.factors, plan.hue, out=jit)
    blur = lambda: v.ops.hisfrag_blur_u8(jit, plan.flags, plan.blur, out=out)
    kernel_ms = {}
    for name, fn in (('windows', windows), ('jitter', jitter), ('blur', blur)):
        fn()
        kernel_ms[name] = [queued_ms(fn, REPS) for _ in range(args.repeats)]

    # (b) a full loader iteration
    batches = iter(loader)
    nxt = lambda: next(batches)
    for _ in range(3):
        nxt()
    iter_dev_ms, iter_host_ms = [], []
    for _ in range(args.repeats):
        iter_dev_ms.append(queued_ms(nxt, 10))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            nxt()
        iter_host_ms.append((time.perf_counter() - t0) * 1e3 / 10)
        torch.cuda.synchronize()

    # (c) the step: fixed resident batch against loader-fed
    cfg = v.config_from_yaml(os.path.join(ROOT, 'configs', 'hisfrag', 'hisfrag20_patch16_512.yaml'))
    torch.manual_seed(cfg.SEED)
    model = v.build_model(cfg).to(dev)
    model.compute_dtype = torch.bfloat16
    opt = v.optim.FlatAdamW(E.param_groups_no_decay_1d(model), model=model, lr=1e-4 * B / 256.0, weight_decay=0.05)

    def two_stage(m, batch_):                                    # bench.py's H-train forward
        imgs, pairs = batch_
        feats = m(imgs, forward_first_part=True)
        return m(feats[pairs[:, 1]], imgs[pairs[:, 0]])

    step = E.TrainStep(model, opt, clip_grad=5.0, amp=True, use_graph=False, forward_fn=two_stage)
    mine = torch.Generator(device=dev).manual_seed(cfg.SEED)
    loader.set_epoch(1)
    feed = iter(loader)
    x_fixed, t_fixed = next(feed)
    x_fixed, t_fixed = x_fixed.clone(), t_fixed.clone()
    pairs_fixed, y_fixed = E.mine_pairs(t_fixed, generator=mine)

    def fixed():
        return step.step((x_fixed, pairs_fixed), y_fixed)

    def fixed_mined():
        pairs, y = E.mine_pairs(t_fixed, generator=mine)
        return step.step((x_fixed, pairs), y)

    def fed():
        x, t = next(feed)
        pairs, y = E.mine_pairs(t, generator=mine)
        return step.step((x, pairs), y)

    for fn in (fixed, fixed, fixed_mined, fed, fed):
        fn()
    torch.cuda.synchronize()

    def block(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = fn()
        torch.cuda.synchronize()
        if not torch.isfinite(loss):
            raise SystemExit('hisfrag_feed_probe.py: the steps diverged')
        return (time.perf_counter() - t0) * 1e3 / args.steps

    fixed_ms, mined_ms, fed_ms = [], [], []
    for _ in range(args.repeats):
        fixed_ms.append(block(fixed))
        mined_ms.append(block(fixed_mined))
        fed_ms.append(block(fed))

    med = lambda xs: round(statistics.median(xs), 4)
    rnd = lambda xs: [round(t, 4) for t in xs]
    res = {'probe': 'hisfrag_feed', 'config': 'H', 'batch': B, 'img_size': S, 'images': args.images, 'image_sides': [600, 1200],
           'store_mb': round(store.data.numel() / 1e6, 1), 'drawn_fraction': {k: round(t, 3) for k, t in drawn.items()}, 'dtype': 'bf16',
           'hipgraph': False, 'pairs_fixed': int(pairs_fixed.shape[0]),
           'windows_kernel_ms': med(kernel_ms['windows']), 'jitter_kernels_ms': med(kernel_ms['jitter']), 'blur_kernel_ms': med(kernel_ms['blur']),
           'loader_iteration_device_ms': med(iter_dev_ms), 'loader_iteration_host_ms': med(iter_host_ms),
           'step_fixed_batch_ms': med(fixed_ms), 'step_fixed_batch_mined_ms': med(mined_ms), 'step_loader_fed_ms': med(fed_ms),
           'loader_fed_over_fixed': round(statistics.median(fed_ms) / statistics.median(fixed_ms), 4),
           'loader_fed_over_fixed_mined': round(statistics.median(fed_ms) / statistics.median(mined_ms), 4),
           'loader_iteration_over_step': round(statistics.median(iter_dev_ms) / statistics.median(fixed_ms), 4),
           'images_per_s_fixed': round(B / statistics.median(fixed_ms) * 1e3, 1), 'images_per_s_loader_fed': round(B / statistics.median(fed_ms) * 1e3, 1),
           'per_block_ms': {'windows_kernel': rnd(kernel_ms['windows']), 'jitter_kernels': rnd(kernel_ms['jitter']), 'blur_kernel': rnd(kernel_ms['blur']),
                            'loader_iteration_device': rnd(iter_dev_ms), 'loader_iteration_host': rnd(iter_host_ms), 'step_fixed': rnd(fixed_ms),
                            'step_fixed_mined': rnd(mined_ms), 'step_loader_fed': rnd(fed_ms)},
           'steps_per_block': args.steps, 'device': torch.cuda.get_device_name(dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
