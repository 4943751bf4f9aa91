#!/usr/bin/env python3
"""michigan.py fed from images resident on the MI355X: what the device loader costs next to config H's
loader and next to the step.

    python3 profiles/michigan_feed_probe.py [--images 160] [--batch 24] [--steps 10] [--repeats 5] [--out FILE]

A synthetic store of ``--images`` random images of 600-1,200 pixels per side (160 of them are about 390 MB, past the 256 MiB
Infinity Cache), three to six per writer, S = 512, config H's model, bf16 autocast, FlatAdamW,
no hipGraph (the pair batch is a structured input).  Measured:
  (a) ``vited_michigan_windows_u8``, ``vited_hisfrag_jitter_u8`` (its two kernels) and ``vited_michigan_blur_gray_u8`` alone on one
      training plan with every augmentation switched on and sixteen holes: device time per call of REPS calls queued between two
      events;
  (b) in ``--repeats`` alternating blocks, all in this process: one full ``MichiganDeviceLoader`` iteration (uniforms, plan, the
      three entry points, the target gather) as device time per iteration of ten queued ones and as the host time it takes to
      enqueue; one ``HisfragDeviceLoader`` iteration the same way; ``--steps`` two-stage H-train steps of bench.py on a fixed
      resident uint8 batch with its pairs mined once (host clock around a block that ends in a device synchronise); and the same
      steps taking every batch from the michigan loader, pairs mined every step.
Prints one JSON line (medians, the per-block lists, the michigan iteration as a ratio to the H iteration and to the step).
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
ITERS = 10


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


def enqueue_ms(fn, reps):
    """Host time per call that ``reps`` calls take to enqueue."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ms = (time.perf_counter() - t0) * 1e3 / reps
    torch.cuda.synchronize()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=160)
    ap.add_argument('--batch', type=int, default=24)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('michigan_feed_probe.py measures on the MI355X; no GPU is visible')
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
    need = 3 + (2 * ITERS + args.steps) * args.repeats + 16      # iterations of (b), within one epoch
    repeat = -(-need * B // args.images)
    loader = E.MichiganDeviceLoader(store, labels, B, S, m=3, repeat=repeat, seed=0)
    loader_h = E.HisfragDeviceLoader(store, labels, B, S, m=3, repeat=repeat, seed=0)
    assert len(loader) >= need and len(loader_h) >= need

    # (a) the entry points alone, every augmentation on
    plan = loader.plan(loader.rank_indices()[0], loader._generator(1))
    bits = (('dropout', 1), ('hflip', 2), ('jitter', 4), ('blur', 8), ('vflip', 16), ('gray', 32))
    drawn = {name: float((plan.flags.bitwise_and(bit) != 0).float().mean()) for name, bit in bits}
    u_on = torch.rand(B, E.MICHIGAN_PLAN_COLUMNS, generator=loader._generator(3), device=dev)
    u_on[:, [24, 90, 91, 92, 101, 103]] = 0.0                    # every probability passes
    u_on[:, 25] = 0.999                                          # sixteen holes
    full = E.michigan_augment_plan(u_on, plan.image, store.sizes_dev, S)
    assert bool((full.flags == 63).all()) and bool((full.n_holes == 16).all())
    win, jit, out = (torch.empty(B, 3, S, S, dtype=torch.uint8, device=dev) for _ in range(3))
    windows = lambda: v.ops.michigan_windows_u8(store.data, store.offsets_dev, store.sizes_dev, full.image, full.flags, full.origin, full.x0,
                                                full.kx, full.y0, full.ky, full.holes, full.n_holes, S, out=win)
    jitter = lambda: v.ops.hisfrag_jitter_u8(win, full.flags, full.order, full.factors, full.hue, out=jit)
    blur = lambda: v.ops.michigan_blur_gray_u8(jit, full.flags, full.blur, out=out)
    kernel_ms = {}
    for name, fn in (('windows', windows), ('jitter', jitter), ('blur_gray', blur)):
        fn()
        kernel_ms[name] = [queued_ms(fn, REPS) for _ in range(args.repeats)]

    # (b) loader iterations and the step, interleaved
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
    feed, feed_h = iter(loader), iter(loader_h)
    nxt, nxt_h = (lambda: next(feed)), (lambda: next(feed_h))
    x_fixed, t_fixed = nxt()
    x_fixed, t_fixed = x_fixed.clone(), t_fixed.clone()
    pairs_fixed, y_fixed = E.mine_pairs(t_fixed, generator=mine)

    def fixed():
        return step.step((x_fixed, pairs_fixed), y_fixed)

    def fed():
        x, t = nxt()
        pairs, y = E.mine_pairs(t, generator=mine)
        return step.step((x, pairs), y)

    for fn in (nxt, nxt, nxt_h, nxt_h, nxt_h, fixed, fixed, fed, fed):
        fn()
    torch.cuda.synchronize()

    def block(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = fn()
        torch.cuda.synchronize()
        if not torch.isfinite(loss):
            raise SystemExit('michigan_feed_probe.py: the steps diverged')
        return (time.perf_counter() - t0) * 1e3 / args.steps

    m_dev, m_host, h_dev, h_host, fixed_ms, fed_ms = [], [], [], [], [], []
    for _ in range(args.repeats):
        m_dev.append(queued_ms(nxt, ITERS))
        h_dev.append(queued_ms(nxt_h, ITERS))
        fixed_ms.append(block(fixed))
        m_host.append(enqueue_ms(nxt, ITERS))
        h_host.append(enqueue_ms(nxt_h, ITERS))
        fed_ms.append(block(fed))

    median = statistics.median
    med = lambda xs: round(median(xs), 4)
    rnd = lambda xs: [round(t, 4) for t in xs]
    res = {'probe': 'michigan_feed', 'config': 'H', 'batch': B, 'img_size': S, 'images': args.images, 'image_sides': [600, 1200],
           'store_mb': round(store.data.numel() / 1e6, 1), 'drawn_fraction': {k: round(t, 3) for k, t in drawn.items()}, 'dtype': 'bf16',
           'hipgraph': False, 'pairs_fixed': int(pairs_fixed.shape[0]),
           'windows_kernel_ms': med(kernel_ms['windows']), 'jitter_kernels_ms': med(kernel_ms['jitter']),
           'blur_gray_kernel_ms': med(kernel_ms['blur_gray']),
           'michigan_iteration_device_ms': med(m_dev), 'michigan_iteration_host_ms': med(m_host),
           'hisfrag_iteration_device_ms': med(h_dev), 'hisfrag_iteration_host_ms': med(h_host),
           'step_fixed_batch_ms': med(fixed_ms), 'step_michigan_fed_ms': med(fed_ms),
           'michigan_over_hisfrag_iteration': round(median(m_dev) / median(h_dev), 4),
           'michigan_iteration_over_step': round(median(m_dev) / median(fixed_ms), 4),
           'michigan_fed_over_fixed': round(median(fed_ms) / median(fixed_ms), 4),
           'per_block_ms': {'windows_kernel': rnd(kernel_ms['windows']), 'jitter_kernels': rnd(kernel_ms['jitter']),
                            'blur_gray_kernel': rnd(kernel_ms['blur_gray']), 'michigan_iteration_device': rnd(m_dev),
                            'michigan_iteration_host': rnd(m_host), 'hisfrag_iteration_device': rnd(h_dev),
                            'hisfrag_iteration_host': rnd(h_host), 'step_fixed': rnd(fixed_ms), 'step_michigan_fed': rnd(fed_ms)},
           'steps_per_block': args.steps, 'iterations_per_block': ITERS, 'device': torch.cuda.get_device_name(dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
