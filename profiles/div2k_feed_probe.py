#!/usr/bin/env python3
"""Config A fed from images resident on the MI355X: what the device loader costs next to the step.

    python3 profiles/div2k_feed_probe.py [--images 48] [--batch 1024] [--steps 20] [--repeats 5] [--out FILE]

A synthetic store of ``--images`` random 1356 x 2040 images (DIV2K's usual size; 48 of them are 398 MB, past the 256 MiB
Infinity Cache), S = 64, config A (patch 8, D 384, 8 + 8 blocks, 4 bins), bf16 autocast, FlatAdamW, hipGraph replay.  Measured:
  (a) ``vited_div2k_regions_u8`` alone on one training plan: device time per call of REPS calls queued between two events;
  (b) one full ``Div2kDeviceLoader`` iteration (uniforms, both plans, regions, pair assembly): device time per iteration of a
      queued epoch, and the host time the iteration takes to enqueue;
  (c) ``TrainStep.step`` on a fixed resident uint8 batch - the step as it was before the loader existed, the yardstick - against
      the same step taking every batch from the loader, in blocks of ``--steps`` steps that alternate ``--repeats`` times (host
      clock around a block that ends in a device synchronise).
Prints one JSON line (medians and the per-block lists).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
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
    ap.add_argument('--images', type=int, default=48)
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('div2k_feed_probe.py measures on the MI355X; no GPU is visible')
    dev = torch.device('cuda:0')
    v._lib.load()
    E, S, B = v.engine, 64, args.batch
    rng = np.random.default_rng(0)
    store = E.Div2kImageStore([rng.integers(0, 256, size=(1356, 2040, 3), dtype=np.uint8) for _ in range(args.images)], dev)
    need = max(3 + 20 * args.repeats, 3 + args.steps * args.repeats) + 8      # iterations of (b) / of (c), each in an epoch of its own
    loader = E.Div2kDeviceLoader(store, B, S, 0.07, repeat=-(-need * B // args.images), seed=0)
    assert len(loader) >= need

    # (a) the regions kernel alone
    g = loader._generator(1)
    (idx, flags, minv, rgb, crop), _ = loader.plan(loader.rank_indices()[0], g)
    out = torch.empty(B, 3, 2 * S, 3 * S, dtype=torch.uint8, device=dev)
    regions = lambda: v.ops.div2k_regions_u8(store.data, store.offsets_dev, store.sizes_dev, idx, flags, minv, rgb, crop, S, out=out)
    regions()
    kernel_ms = [queued_ms(regions, REPS) for _ in range(args.repeats)]
    warped = float((flags.bitwise_and(4) != 0).float().mean())

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
    torch.manual_seed(0)
    cfg = v.config_from_yaml(os.path.join(ROOT, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml'))
    model = v.build_model(cfg).to(dev)
    model.compute_dtype = torch.bfloat16
    opt = v.optim.FlatAdamW(E.param_groups_no_decay_1d(model), model=model, lr=1e-4 * B / 256.0, weight_decay=0.05)
    step = E.TrainStep(model, opt, clip_grad=5.0, amp=True, use_graph=True)
    loader.set_epoch(1)
    feed = iter(loader)
    x_fixed, y_fixed = next(feed)
    x_fixed, y_fixed = x_fixed.clone(), y_fixed.clone()
    for _ in range(3):                                           # two eager steps, the capture, one replay
        step.step(x_fixed, y_fixed)
    for _ in range(2):
        step.step(*next(feed))
    torch.cuda.synchronize()
    assert step._g1 is not None

    def block(batch_of):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = step.step(*batch_of())
        torch.cuda.synchronize()
        if not torch.isfinite(loss):
            raise SystemExit('div2k_feed_probe.py: the steps diverged')
        return (time.perf_counter() - t0) * 1e3 / args.steps

    fixed_ms, fed_ms = [], []
    for _ in range(args.repeats):
        fixed_ms.append(block(lambda: (x_fixed, y_fixed)))
        fed_ms.append(block(lambda: next(feed)))

    med = lambda xs: round(statistics.median(xs), 4)
    res = {'probe': 'div2k_feed', 'config': 'A', 'batch': B, 'img_size': S, 'images': args.images, 'image_hw': [1356, 2040],
           'store_mb': round(store.data.numel() / 1e6, 1), 'warped_fraction': round(warped, 3), 'dtype': 'bf16', 'hipgraph': True,
           'regions_kernel_ms': med(kernel_ms), 'loader_iteration_device_ms': med(iter_dev_ms), 'loader_iteration_host_ms': med(iter_host_ms),
           'step_fixed_batch_ms': med(fixed_ms), 'step_loader_fed_ms': med(fed_ms),
           'loader_fed_over_fixed': round(statistics.median(fed_ms) / statistics.median(fixed_ms), 4),
           'loader_iteration_over_step': round(statistics.median(iter_dev_ms) / statistics.median(fixed_ms), 4),
           'pairs_per_s_fixed': round(B / statistics.median(fixed_ms) * 1e3, 1), 'pairs_per_s_loader_fed': round(B / statistics.median(fed_ms) * 1e3, 1),
           'per_block_ms': {'regions_kernel': [round(t, 4) for t in kernel_ms], 'loader_iteration_device': [round(t, 4) for t in iter_dev_ms],
                            'loader_iteration_host': [round(t, 4) for t in iter_host_ms], 'step_fixed': [round(t, 4) for t in fixed_ms],
                            'step_loader_fed': [round(t, 4) for t in fed_ms]},
           'steps_per_block': args.steps, 'device': torch.cuda.get_device_name(dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
