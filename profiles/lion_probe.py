#!/usr/bin/env python3
"""What Lion costs beside AdamW on the MI355X: updates of config A's and config H's parameter sets with their
bf16 weight shadows present, replayed from captured graphs so that the events time the device and not the host's launches, and
config A's replayed training step at equal weights with either optimizer.

    python3 profiles/lion_probe.py [--rounds 7] [--updates 100] [--steps 20] [--configs A,H] [--out profiles/lion_probe.json]

One process.  Per config, one model per arm, each after one bf16 forward + backward so that its weight shadows exist.  Arms:
  adamw / adamw_ema   optim.FlatAdamW.step_flat without and with ema_decay=0.9999 (16 B read + 16 B written per element, + 4 + 4)
  lion / lion_ema     optim.FlatLion.step_flat without and with it (12 B read + 12 B written per element, + 4 + 4)
  step_adamw_lr0 / step_lion_lr0  (config A only, --steps > 0) engine.TrainStep(use_graph=True) at batch 1024 pairs, replayed, at a
                      rate of 0: both arms keep the initial weights, so they differ by the update's launches alone
Both update kernels also write 4 B of bf16 shadows per element of a tensor that has them; with them the byte counts are 36 and 28, and
at an equal HBM rate Lion's update would take 28 / 36 = 0.78 of AdamW's time.  That ratio is the expectation the measured
``lion_over_adamw`` is reported against.
Every update arm is ``--updates`` calls captured into one hipGraph.  After a warm-up, ``--rounds`` rounds time one replay of every
arm (``--steps`` steps of the step arms) between device events, the arms alternating inside every round.  Prints one JSON line
(microseconds per call, per round, with median, lowest and highest; bytes per element and the rate they imply) and writes it to
``--out``."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vited_amd as v  # noqa: E402

CONFIGS = {'A': ('configs/puzzle/div2k_erosion7_4bin_patch8_64.yaml', 16), 'H': ('configs/hisfrag/hisfrag20_patch16_512.yaml', 2)}
DECAY = 0.9999
# HBM bytes per parameter element without the shadows (which depend on how many tensors have them): read + written
BYTES = {'adamw': 16 + 16, 'adamw_ema': 20 + 20, 'lion': 12 + 12, 'lion_ema': 16 + 16}


def graphed(f, calls):
    """``calls`` calls of ``f`` captured into one hipGraph (after eager warm-up calls, which also build whatever ``f`` builds on first
    use): a replay costs the host one launch, so the events time the device."""
    for _ in range(4):
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            f()
    return g.replay


def timed(arms, rounds, calls, replays=False):
    """{arm: [us per call, one figure per round]}, the arms alternating inside every round.  ``replays``: every arm is one replay of
    ``calls`` captured calls."""
    for f in arms.values():
        for _ in range(2 if replays else 6):
            f()
    torch.cuda.synchronize()
    us = {name: [] for name in arms}
    for _ in range(rounds):
        for name, f in arms.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(1 if replays else calls):
                f()
            e.record()
            e.synchronize()
            us[name].append(round(a.elapsed_time(e) * 1000.0 / calls, 2))
    return us


def summary(us):
    return {k: [round(statistics.median(t), 2), min(t), max(t)] for k, t in us.items()}


def update_arms(cfg, pairs, dev):
    E = v.engine
    S, C = cfg.DATA.IMG_SIZE, cfg.MODEL.NUM_CLASSES
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(pairs, 2, 3, S, S, device=dev, generator=g) * 2 - 1
    y = (torch.rand(pairs, C, device=dev, generator=g) < 0.25).float()

    def bound(cls, **ema):
        torch.manual_seed(0)
        model = v.build_model(cfg).to(dev).train()
        flat = E.FlatGradients(model.parameters())
        with torch.autocast('cuda', dtype=torch.bfloat16):
            loss = torch.nn.functional.binary_cross_entropy_with_logits(model(x).float(), y)
        loss.backward()
        opt = cls(E.param_groups_no_decay_1d(model), lr=1e-4, weight_decay=0.05, model=model, **ema)
        opt.bind_flat(flat, model)
        return model, opt

    O = v.optim
    made = {'adamw': bound(O.FlatAdamW), 'lion': bound(O.FlatLion), 'adamw_ema': bound(O.FlatAdamW, ema_decay=DECAY),
            'lion_ema': bound(O.FlatLion, ema_decay=DECAY)}
    arms = {name: (lambda opt=opt: opt.step_flat(5.0)) for name, (_, opt) in made.items()}
    model, lion = made['lion']
    lion._descriptors()                              # counts the tiles
    numel = {id(p): p.numel() for p in lion.flat.params}
    shadow_bytes = sum(2 * numel[pid] * len(tags) for cache in v.functions.shadows_of(model) for pid, tags in cache.buffers().items()
                       if pid in numel)
    info = {'parameters': sum(p.numel() for p in lion.flat.params), 'tensors': len(lion.flat.params), 'tiles': lion._tiles,
            'bf16_shadows': sum(len(cache) for cache in v.functions.shadows_of(model)),
            'bf16_shadow_bytes': shadow_bytes}
    if not info['bf16_shadows']:
        raise RuntimeError('no bf16 weight shadows: the probe would not measure their refresh')
    return arms, info, made


def step_arms(cfg, dev, batch=1024):
    E = v.engine
    S, C = cfg.DATA.IMG_SIZE, cfg.MODEL.NUM_CLASSES
    x = torch.randn(batch, 2, 3, S, S, device=dev).clamp_(-1, 1)
    y = (torch.rand(batch, C, device=dev) > 0.75).float()
    arms = {}
    # a rate of 0: the weights stay what they were in both arms, so the arms differ by the update's launches alone (the time of the
    # rest of the step depends on the values the weights hold, and the two optimizers train them apart)
    for name, cls in (('step_adamw_lr0', v.optim.FlatAdamW), ('step_lion_lr0', v.optim.FlatLion)):
        torch.manual_seed(0)
        model = v.build_model(cfg).to(dev).train()
        opt = cls(E.param_groups_no_decay_1d(model), lr=0.0, weight_decay=0.05, model=model)
        step = E.TrainStep(model, opt, clip_grad=5.0, amp=True, use_graph=True)
        for _ in range(4):                           # two eager steps, the capture, one replay
            step.step(x, y)
        if step._g_opt is None:
            raise RuntimeError('the step was not captured')
        arms[name] = lambda step=step: step.step(x, y)
    return arms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--updates', type=int, default=100)
    ap.add_argument('--steps', type=int, default=20, help='replayed steps of config A per round and arm (0: leave the step arms out)')
    ap.add_argument('--configs', default='A,H')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lion_probe.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    v._lib.load()
    res = {'probe': 'lion', 'ema_decay': DECAY, 'updates_per_round': args.updates, 'steps_per_round': args.steps, 'rounds': args.rounds,
           'device': torch.cuda.get_device_name(dev), 'bytes_per_element_without_shadows': BYTES, 'expected_lion_over_adamw': round(28 / 36, 3),
           'configs': {}}
    for name in args.configs.split(','):
        path, pairs = CONFIGS[name]
        cfg = v.config_from_yaml(os.path.join(ROOT, path))
        arms, info, made = update_arms(cfg, pairs, dev)
        us = timed({k: graphed(f, args.updates) for k, f in arms.items()}, args.rounds, args.updates, replays=True)
        med = summary(us)
        moved = {k: info['parameters'] * BYTES[k] + info['bf16_shadow_bytes'] for k in med}       # bytes per call, shadows included
        info.update(us_per_call=us, median_low_high_us=med,
                    tb_per_s={k: round(moved[k] / (med[k][0] * 1e-6) / 1e12, 3) for k in med},
                    lion_over_adamw=round(med['lion'][0] / med['adamw'][0], 3), lion_ema_over_adamw_ema=round(med['lion_ema'][0] / med['adamw_ema'][0], 3),
                    bytes_lion_over_adamw=round(moved['lion'] / moved['adamw'], 3))
        del arms, made
        if name == 'A' and args.steps > 0:
            us = timed(step_arms(cfg, dev), args.rounds, args.steps)
            info.update(step_us=us, step_median_low_high_us=summary(us))
        res['configs'][name] = info
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
