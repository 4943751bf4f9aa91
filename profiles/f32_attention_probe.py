#!/usr/bin/env python3
"""The fp32 attention on the matrix cores (attention_f32_mfma.hip) against the vector-ALU kernels that compute the same bits
(attention_portable.hip), and what the choice is worth in an fp32 training step.

    python3 profiles/f32_attention_probe.py [--first valu|mfma] [--runs 2] [--rounds 6] [--reps 5] [--out profiles/f32_attention_probe.json]

One process; ``ops.fp32_attention_kernels`` switches between the two sets of kernels, which alternate inside every round.  Per shape
and kernel a sample is a pair of device events around ``--reps`` calls (``--rounds`` samples = rounds x reps >= 20 calls a run), after
a warm-up of both at that shape that includes one untimed window.  ``--runs`` passes over all shapes are recorded apart, each with
median and lowest .. highest; ``faster`` = the matrix-core kernels' highest sample lies below the vector-ALU kernels' lowest in every
run.  ``--first`` names the kernels that go first in each round: the committed pair of files has one of each.

  forward / backward   ops.attention_fwd and ops.attention_bwd (dQ + delta and dK / dV, two launches) on fp32 operands at the shapes
                       that decide the predicate: the cls-only tail (one query), 64 / 65 tokens at batch 128 and batch 8 (config A:
                       12 heads of 32), 256 / 257, 576 / 577 and 1,024 / 1,025 tokens (config H: 6 heads of 64)
  indexed              ops.attention_bwd(segments=...): the pair-indexed decoder's backward, segmented sum included
  step                 one eager fp32 TrainStep (amp off, FlatAdamW, clip 5.0) of config A's model at batch 128 and of config H's at
                       batch 2, and ``attention_share``: the device time between events around every path-1 attention call of a
                       step, over the step's device time (one more step per kernel, outside the timed samples)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_A = os.path.join(ROOT, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml')
CFG_H = os.path.join(ROOT, 'configs', 'hisfrag', 'hisfrag20_patch16_512.yaml')
# (workload, batch, heads, nq, nk, head_dim)
SHAPES = [('A cls tail b128', 128, 12, 1, 65, 32), ('A encoder b128', 256, 12, 64, 64, 32), ('A decoder b128', 128, 12, 65, 65, 32),
          ('A cls tail b8', 8, 12, 1, 65, 32), ('A encoder b8', 16, 12, 64, 64, 32), ('A decoder b8', 8, 12, 65, 65, 32),
          ('256 tokens', 8, 6, 256, 256, 64), ('257 tokens', 4, 6, 257, 257, 64), ('257 tokens hd32', 4, 12, 257, 257, 32),
          ('576 tokens', 8, 6, 576, 576, 64), ('577 tokens', 4, 6, 577, 577, 64),
          ('H cls tail b2', 2, 6, 1, 1025, 64), ('H encoder b2', 4, 6, 1024, 1024, 64), ('H decoder b2', 2, 6, 1025, 1025, 64),
          ('H encoder b24', 48, 6, 1024, 1024, 64)]
# (workload, pairs, items, heads, nq, nk, head_dim)
INDEXED = [('A pair decoder', 128, 128, 12, 65, 65, 32), ('H pair decoder', 72, 24, 6, 1025, 1025, 64)]
MODES = {'valu': 'valu', 'mfma': 'auto'}


def spread(values):
    return {'median': round(statistics.median(values), 3), 'lowest': round(min(values), 3), 'highest': round(max(values), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--first', choices=tuple(MODES), default='valu')
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.rounds * args.reps < 20:
        raise SystemExit('at least 20 calls a run: raise --rounds or --reps')
    sys.path.insert(0, ROOT)
    import torch
    import vited_amd as v
    if not torch.cuda.is_available():
        raise SystemExit('f32_attention_probe.py measures on the GPU: none found')
    v._lib.load()
    ops, dev = v.ops, torch.device('cuda:0')
    order = [args.first] + [m for m in MODES if m != args.first]
    g = torch.Generator(device='cpu').manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    def timed(fn, reps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        return a.elapsed_time(e) / reps * 1e3             # us per call

    def measure(fn, reps, kernel_of=None):
        """``--runs`` records of fn under the two sets of kernels, alternating inside every round."""
        ran = {}
        for name in order:                                # warm-up: first launches, then one untimed window
            with ops.fp32_attention_kernels(MODES[name]):
                for _ in range(3):
                    fn()
                ran[name] = ops.last_fp32_attention_kernel() if kernel_of is None else kernel_of()
                timed(fn, reps)
        runs = []
        for _ in range(args.runs):
            us = {name: [] for name in order}
            for _ in range(args.rounds):
                for name in order:
                    with ops.fp32_attention_kernels(MODES[name]):
                        us[name].append(timed(fn, reps))
            runs.append({name: spread(us[name]) for name in MODES})
        return runs, ran

    def row_of(what, runs, ran, flops):
        row = dict(what, kernel_ran=ran, runs=runs)
        row['faster'] = all(r['mfma']['highest'] < r['valu']['lowest'] for r in runs)
        if flops:
            for name in MODES:
                row[f'{name}_tflops'] = [round(flops / r[name]['median'] / 1e6, 1) for r in runs]
        row['speedup'] = [round(r['valu']['median'] / r['mfma']['median'], 2) for r in runs]
        print(row, file=sys.stderr, flush=True)
        return row

    res = {'probe': 'f32_attention', 'device': torch.cuda.get_device_name(dev), 'first': args.first, 'runs': args.runs,
           'rounds': args.rounds, 'reps': args.reps, 'unit': 'us per call', 'forward': [], 'backward': [], 'indexed': []}
    for workload, b, heads, nq, nk, hd in SHAPES:
        d, scale = heads * hd, hd ** -0.5
        q, k, val, do = rnd(b, nq, d), rnd(b, nk, d), rnd(b, nk, d), rnd(b, nq, d)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(val)
        o, lse = ops.attention_fwd(q, k, val, heads, scale)
        what = {'workload': workload, 'batch': b, 'heads': heads, 'nq': nq, 'nk': nk, 'head_dim': hd}
        reps = args.reps * (10 if b * nq * nk < 2 ** 20 else 1)
        flops = 4.0 * b * heads * nq * nk * hd               # two products forward, five backward (the score is formed twice)
        runs, ran = measure(lambda: ops.attention_fwd(q, k, val, heads, scale), reps)
        res['forward'].append(row_of(dict(what, predicate=ops.fp32_attention_supported(b, heads, nq, nk, hd)), runs, ran, flops))
        runs, ran = measure(lambda: ops.attention_bwd(q, k, val, o, do, lse, heads, scale, dq, dk, dv), reps)
        res['backward'].append(row_of(dict(what, predicate=ops.fp32_attention_supported(b, heads, nq, nk, hd, backward=True)), runs, ran,
                                      3.5 * flops))
        del q, k, val, do, dq, dk, dv, o, lse
    for workload, pairs, items, heads, nq, nk, hd in INDEXED:
        d, scale = heads * hd, hd ** -0.5
        q, k, val, do = rnd(pairs, nq, d), rnd(items, nk, d), rnd(items, nk, d), rnd(pairs, nq, d)
        index = (torch.arange(pairs) * 7 % items).to(dev)
        seg = ops.pair_segments(index, items)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(val)
        o, lse = ops.attention_fwd(q, k, val, heads, scale, kv_index=index)
        runs, ran = measure(lambda: ops.attention_bwd(q, k, val, o, do, lse, heads, scale, dq, dk, dv, segments=seg), args.reps)
        res['indexed'].append(row_of({'workload': workload, 'pairs': pairs, 'items': items, 'heads': heads, 'nq': nq, 'nk': nk, 'head_dim': hd,
                                      'includes': 'the segmented sum', 'predicate': ops.fp32_attention_supported(pairs, heads, nq, nk, hd, backward=True)},
                                     runs, ran, 3.5 * 4.0 * pairs * heads * nq * nk * hd))
        del q, k, val, do, dq, dk, dv, o, lse
    res['step'] = []
    for name, path, batch in ([] if args.skip_step else [('config A', CFG_A, 128), ('config H', CFG_H, 2)]):
        E = v.engine
        cfg = v.config_from_yaml(path)
        torch.manual_seed(cfg.SEED)
        model = v.build_model(cfg).to(dev)
        model.compute_dtype = torch.float32
        opt = v.optim.FlatAdamW(E.param_groups_no_decay_1d(model), model=model, lr=1e-4 * batch / 256.0, weight_decay=0.05)
        step = E.TrainStep(model, opt, clip_grad=5.0, amp=False, use_graph=False)
        x = torch.randn(batch, 2, 3, cfg.DATA.IMG_SIZE, cfg.DATA.IMG_SIZE, device=dev).clamp_(-1, 1)
        y = (torch.rand(batch, cfg.MODEL.NUM_CLASSES, device=dev) > 0.75).float()
        real = ops.attention_fwd, ops.attention_bwd

        def watched_step():
            """One step with events around every attention call: (kernels reported, attention ms, step ms)."""
            seen, spans = set(), []

            def spy(fn):
                def wrapped(*a, **k):
                    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a0.record()
                    r = fn(*a, **k)
                    a1.record()
                    if ops.last_paths()[1] == 1:
                        seen.add(ops.last_fp32_attention_kernel())
                        spans.append((a0, a1))
                    return r
                return wrapped

            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ops.attention_fwd, ops.attention_bwd = spy(real[0]), spy(real[1])
            try:
                s0.record()
                step.step(x, y)
                s1.record()
            finally:
                ops.attention_fwd, ops.attention_bwd = real
            s1.synchronize()
            return sorted(seen), sum(a0.elapsed_time(a1) for a0, a1 in spans), s0.elapsed_time(s1), len(spans)

        share = {}

        def kernels_of_a_step():
            seen, attn_ms, step_ms, calls = watched_step()
            mode = 'valu' if seen == [1] else 'mfma'
            share[mode] = {'attention_ms': round(attn_ms, 3), 'watched_step_ms': round(step_ms, 3), 'calls': calls,
                           'share': round(attn_ms / step_ms, 3)}
            return seen

        runs, ran = measure(lambda: step.step(x, y), args.steps, kernel_of=kernels_of_a_step)
        for r in runs:                                    # a step is timed in ms
            for mode in MODES:
                r[mode] = {key: round(val / 1e3, 3) for key, val in r[mode].items()}
        res['step'].append(row_of({'workload': name, 'batch': batch, 'unit': 'ms per step', 'steps_per_sample': args.steps,
                                   'attention_share': share}, runs, ran, None))
        del model, opt, step, x, y
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
