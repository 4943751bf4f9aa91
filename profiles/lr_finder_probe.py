#!/usr/bin/env python3
"""What a learning-rate range test of 100 iterations costs on the MI355X with every decision on the device (``engine.find_lr``) and
driven by the host the way a port of ignite's loop would be.

    python3 profiles/lr_finder_probe.py [--iters 100] [--rounds 5] [--rounds-h 3] [--out profiles/lr_finder_probe.json]

Two workloads, one process each part, the two arms alternating inside every round on ONE step object:
  A   config A, 1,024 pairs, bf16, ``TrainStep(use_graph=True)``, captured before the first round
  H   config H, 24 images (72 pair rows), bf16, ``TwoStageTrainStep(use_graph=True)``, captured before the first round
  device   ``find_lr(step, batches, poll_every=16, restore=True)``
  host     the same sweep with ``step.set_lr(rate)`` in front of and ``loss.item()`` behind every iteration, the smoothed and the best
           loss kept in Python, between the same snapshot and restore
Neither arm can halt early (``diverge_th`` 1e9), so both run all ``--iters`` iterations.  Wall clock around the whole call, device idle
before and after: ms per sweep, and per iteration.  Then the ``record`` launch alone: device events around 500 queued launches (us per
launch) and the host's time to queue one.  Nobody had measured either arm before; the numbers are recorded as they come.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP = dict(start_lr=1e-7, end_lr=1e-2, smooth_f=0.05, diverge_th=1e9)


def spread(values):
    return {'median': round(statistics.median(values), 3), 'lowest': round(min(values), 3), 'highest': round(max(values), 3), 'rounds': values}


def host_sweep(v, step, batches, iters):
    """ignite's loop, ported: the host sets every rate and reads every loss."""
    saved = v.engine.lr_finder._Snapshot(step)
    rate, f, th = v.ops.lr_finder_rate, SWEEP['smooth_f'], SWEEP['diverge_th']
    history, s, best = [], 0.0, 0.0
    try:
        for i, (x, y) in zip(range(iters), batches):
            lr = rate(SWEEP['start_lr'], SWEEP['end_lr'], i, iters)
            step.set_lr(lr)
            loss = step.step(x, y).item()
            s = loss if i == 0 else f * loss + (1.0 - f) * s
            best = s if i == 0 or s < best else best
            history.append((lr, loss, s))
            if not loss == loss or s > th * best:
                break
    finally:
        saved.restore()
    return history


def time_arms(v, torch, step, batches, iters, rounds):
    ms = {'device': [], 'host': []}
    rows = {}
    for _ in range(rounds):
        for arm in ('device', 'host'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if arm == 'device':
                rows[arm] = v.engine.find_lr(step, batches, num_iter=iters, poll_every=16, restore=True, **SWEEP).iterations
            else:
                rows[arm] = len(host_sweep(v, step, batches, iters))
            torch.cuda.synchronize()
            ms[arm].append(round((time.perf_counter() - t0) * 1e3, 3))
    out = {arm: {'ms_per_sweep': spread(ms[arm]), 'ms_per_iteration_median': round(statistics.median(ms[arm]) / iters, 4), 'rows': rows[arm]}
           for arm in ms}
    d, h = out['device']['ms_per_sweep'], out['host']['ms_per_sweep']
    out['host_minus_device_ms_per_iteration'] = round((h['median'] - d['median']) / iters, 4)
    out['ranges_apart'] = d['highest'] < h['lowest'] or h['highest'] < d['lowest']
    return out


def record_alone(v, torch, opt, dev, reps=500, rounds=5):
    test = v.engine.LRRangeTest(opt, reps * (rounds + 1), **SWEEP)
    loss = torch.tensor(0.7, device=dev)
    for _ in range(reps):
        test.record(loss)
    device_us, host_us = [], []
    for _ in range(rounds):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(reps):
            test.record(loss)
        e.record()
        t1 = time.perf_counter()
        e.synchronize()
        device_us.append(round(a.elapsed_time(e) / reps * 1e3, 3))
        host_us.append(round((t1 - t0) / reps * 1e6, 3))
    return {'queued_launches': reps, 'device_us_per_launch': spread(device_us), 'host_us_to_queue_one': spread(host_us), 'state': test.state()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--rounds-h', type=int, default=3)
    ap.add_argument('--only', choices=('A', 'H'), default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import vited_amd as v
    if not torch.cuda.is_available():
        raise SystemExit('lr_finder_probe.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    v._lib.load()
    E = v.engine
    res = {'probe': 'lr_finder', 'iterations': args.iters, 'poll_every': 16, 'sweep': SWEEP, 'dtype': 'bf16',
           'device': torch.cuda.get_device_name(dev), 'expected': 'none: the issue gave no expected value for any of these figures'}
    if args.only != 'H':
        cfg = v.config_from_yaml(os.path.join(ROOT, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml'))
        torch.manual_seed(0)
        model = v.build_model(cfg).to(dev).train()
        opt = v.optim.FlatAdamW(E.param_groups_no_decay_1d(model), model=model, lr=4e-4, weight_decay=0.05)
        step = E.TrainStep(model, opt, clip_grad=5.0, amp=True, use_graph=True)
        S, C, B = cfg.DATA.IMG_SIZE, cfg.MODEL.NUM_CLASSES, 1024
        batches = [(torch.randn(B, 2, 3, S, S, device=dev).clamp_(-1, 1), (torch.rand(B, C, device=dev) > 0.75).float())] * args.iters
        for x, y in batches[:4]:                                 # two eager updates, the capture, one replay
            step.step(x, y)
        torch.cuda.synchronize()
        if step._g1 is None:
            raise SystemExit('config A: the step was not captured')
        res['A'] = dict(time_arms(v, torch, step, batches, args.iters, args.rounds), batch=B, step='TrainStep(use_graph=True)',
                        recaptures=step.recaptures)
        print(f"A: {json.dumps({k: res['A'][k]['ms_per_iteration_median'] for k in ('device', 'host')})}", file=sys.stderr, flush=True)
        res['record_alone'] = record_alone(v, torch, opt, dev)
        del step, opt, model, batches
        torch.cuda.empty_cache()
    if args.only != 'A':
        cfg = v.config_from_yaml(os.path.join(ROOT, 'configs', 'hisfrag', 'hisfrag20_patch16_512.yaml'))
        images = 24
        torch.manual_seed(0)
        model = v.build_model(cfg).to(dev).train()
        opt = v.optim.FlatAdamW(E.param_groups_no_decay_1d(model), model=model, lr=cfg.TRAIN.BASE_LR, weight_decay=0.05)
        step = E.TwoStageTrainStep(model, opt, capacity=E.mined_pair_capacity(images, 3), clip_grad=5.0, amp=True, use_graph=True)
        batches = [(torch.randn(images, 3, 512, 512, device=dev).clamp_(-1, 1), torch.arange(images // 3, device=dev).repeat_interleave(3))] * args.iters
        for x, y in batches[:4]:
            step.step(x, y)
        torch.cuda.synchronize()
        if step._g1 is None:
            raise SystemExit('config H: the step was not captured')
        res['H'] = dict(time_arms(v, torch, step, batches, args.iters, args.rounds_h), images=images, capacity=step.capacity,
                        step='TwoStageTrainStep(use_graph=True)', recaptures=step.recaptures)
        print(f"H: {json.dumps({k: res['H'][k]['ms_per_iteration_median'] for k in ('device', 'host')})}", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
