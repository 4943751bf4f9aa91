#!/usr/bin/env python3
"""What the two-stage training step of config H costs on the MI355X launched eagerly and replayed as hipGraphs, and what its loss costs
as plain torch ops and as the fused launch.

    python3 profiles/two_stage_graph_probe.py [--rounds 7] [--steps 6] [--reps 200] [--out profiles/two_stage_graph_probe.json]

Config H: 24 images of 512 x 512 (8 writers x 3), patch 16, 12 + 12 blocks, bf16, capacity 72, FlatAdamW, the config's cosine schedule
stepped on the device.  Three models from one state in ONE process, each warmed up (the replayed one captured), then ``--rounds`` rounds
that time ``--steps`` steps of each, alternating:
  parent   hisfrag_prepare_mined + TrainStep(forward_fn=the pair-indexed decoder call, criterion=mined_bce_with_logits), eager
  eager    TwoStageTrainStep(use_graph=False)
  replay   TwoStageTrainStep(use_graph=True)
Per round and arm: device events around the steps (ms per step) and a host clock from the first call to the return of the last one,
before any synchronise (what the host spends issuing a step).  The inputs stay on the device.
loss     mined_bce_with_logits and mined_bce_fused, forward + backward on [72, 1] logits: device events around ``--reps`` repetitions
         (us per repetition, launch to launch), eagerly and as a replayed graph of one repetition, and the kernels one repetition
         launches, counted in a profiler trace of one call (null where the profiler reports no device activity).
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ('parent', 'eager', 'replay')
ITERS_PER_EPOCH = 1000


def spread(values):
    return {'median': round(statistics.median(values), 4), 'lowest': round(min(values), 4), 'highest': round(max(values), 4)}


def build(v, torch, cfg, state, arm, dev, capacity):
    E = v.engine
    model = v.build_model(cfg).to(dev).train()
    model.load_state_dict(state)
    opt = v.optim.FlatAdamW(E.param_groups_no_decay_1d(model), lr=cfg.TRAIN.BASE_LR, weight_decay=0.05)
    sched = E.build_scheduler(cfg, opt, ITERS_PER_EPOCH)
    if arm == 'parent':
        step = E.TrainStep(model, opt, clip_grad=5.0, amp=True, use_graph=False, lr_scheduler=sched, meters=True,
                           forward_fn=lambda m, b: m(b[1], b[0], x2_index=b[2], x1_index=b[3]), criterion=E.mined_bce_with_logits)

        def run(samples, targets):
            batch, mined = E.hisfrag_prepare_mined(model, samples, targets, capacity, amp=True)
            return step.step(batch, mined)
    else:
        step = E.TwoStageTrainStep(model, opt, capacity=capacity, clip_grad=5.0, amp=True, use_graph=arm == 'replay', lr_scheduler=sched,
                                   meters=True)
        run = step.step
    if not step.lr_on_device:
        raise SystemExit(f'arm {arm}: the schedule is not stepped on the device')
    return step, run


def time_steps(torch, runs, samples, targets, steps, rounds):
    device_ms, host_ms = {a: [] for a in runs}, {a: [] for a in runs}
    for _ in range(rounds):
        for arm, run in runs.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(steps):
                run(samples, targets)
            e.record()
            t1 = time.perf_counter()
            e.synchronize()
            device_ms[arm].append(round(a.elapsed_time(e) / steps, 4))
            host_ms[arm].append(round((t1 - t0) / steps * 1e3, 4))
    return device_ms, host_ms


def kernel_count(torch, fn):
    """Kernels one call of ``fn`` launches: from a profiler trace of one call (None where the profiler gives no device activity)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in ev.name.lower()]
        return len(names) or None
    except Exception as err:                      # no tracer in this build: the count is not known
        print(f'kernel count unavailable: {err!r}', file=sys.stderr)
        return None


def loss_arm(v, torch, dev, capacity, reps, rounds):
    E = v.engine
    targets = torch.arange(capacity // 9, device=dev).repeat_interleave(3)
    mined = E.mine_pairs_device(targets, capacity)
    logits = torch.randn(capacity, 1, device=dev)
    out = {}
    for name, fn in (('torch_ops', E.mined_bce_with_logits), ('fused', E.mined_bce_fused)):
        def once(fn=fn):
            leaf = logits.detach().requires_grad_(True)
            fn(leaf, mined).backward()
            return leaf.grad

        for _ in range(5):
            once()
        us = []
        for _ in range(rounds):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                once()
            e.record()
            e.synchronize()
            us.append(round(a.elapsed_time(e) / reps * 1e3, 2))
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            once()
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(graph):
            once()
        ms = []
        for _ in range(rounds):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                graph.replay()
            e.record()
            e.synchronize()
            ms.append(round(a.elapsed_time(e) / reps * 1e3, 2))
        out[name] = {'eager_us': spread(us), 'replayed_us': spread(ms), 'kernels': kernel_count(torch, once)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=24)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--order', default=','.join(ARMS))
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    order = args.order.split(',')
    if sorted(order) != sorted(ARMS):
        raise SystemExit(f'--order names each of {ARMS} once')
    sys.path.insert(0, ROOT)
    import torch
    import vited_amd as v
    if not torch.cuda.is_available():
        raise SystemExit('two_stage_graph_probe.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    v._lib.load()
    cfg = v.config_from_yaml(os.path.join(ROOT, 'configs', 'hisfrag', 'hisfrag20_patch16_512.yaml'))
    capacity = v.engine.mined_pair_capacity(args.images, 3)
    torch.manual_seed(0)
    state = v.build_model(cfg).state_dict()
    samples = torch.randn(args.images, 3, 512, 512, device=dev).clamp_(-1, 1)
    targets = torch.arange(args.images // 3, device=dev).repeat_interleave(3)
    steps, runs = {}, {}
    for arm in order:
        steps[arm], runs[arm] = build(v, torch, cfg, state, arm, dev, capacity)
        for _ in range(4):                                   # two eager updates, the capture, one more
            runs[arm](samples, targets)
        torch.cuda.synchronize()
    if steps['replay']._g1 is None or steps['replay']._g2 is None:
        raise SystemExit('the two-stage step was not captured')
    device_ms, host_ms = time_steps(torch, runs, samples, targets, args.steps, args.rounds)
    res = {'probe': 'two_stage_graph', 'config': 'H', 'images': args.images, 'capacity': capacity, 'dtype': 'bf16', 'order': order,
           'rounds': args.rounds, 'steps_per_round': args.steps, 'device': torch.cuda.get_device_name(dev),
           'device_ms_per_step': {a: dict(spread(device_ms[a]), rounds=device_ms[a]) for a in ARMS},
           'host_ms_per_step': {a: dict(spread(host_ms[a]), rounds=host_ms[a]) for a in ARMS},
           'recaptures': steps['replay'].recaptures,
           'last_loss': {a: float(steps[a].meters.values()['loss'].val) for a in ARMS}}
    d = res['device_ms_per_step']
    for a, b in (('replay', 'parent'), ('replay', 'eager'), ('eager', 'parent')):
        apart = d[a]['highest'] < d[b]['lowest'] or d[b]['highest'] < d[a]['lowest']
        res[f'{a}_minus_{b}_ms'] = {'medians': round(d[a]['median'] - d[b]['median'], 4), 'ranges_apart': apart}
    print(f"device ms / step: { {a: d[a]['median'] for a in ARMS} }", file=sys.stderr, flush=True)
    res['loss_72_rows'] = loss_arm(v, torch, dev, capacity, args.reps, args.rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
