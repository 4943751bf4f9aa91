#!/usr/bin/env python3
"""q/k-norm (csrc/qk_norm.hip): the kernel alone against the bytes it must move, and what switching it on costs one config A
training step in time and memory.

Kernel: the self-attention layout (q / k column slices of the packed [M, 3D] projection, bf16), forward and backward, at
config A's sizes (65,536 and 66,560 rows x 12 heads x 32) and config H's (24 x 1,024 and 72 x 1,025 rows x 6 heads x 64).  Bytes:
the forward reads q and k and writes their normalised copies and 2 x 2 fp32 statistics per head row; the backward reads dy, the
pre-norm q / k and the statistics and writes dx (the partial sums are noise beside them).  The roof is HBM (8 TB/s peak).

Step: config A (64-pixel patch pairs, 384 wide, 12 heads, 8 + 8 blocks), B 1,024, bf16, FlatAdamW, replayed hipGraphs - a
``qk_norm=True`` and a ``qk_norm=False`` model in ONE process, timed in alternating blocks with device events; median, lowest
and highest block.  ``--arms off`` runs the off model alone (it passes no ``qk_norm`` argument, so it also runs on a tree from
before the option existed: the comparison of the off path with the parent commit).  Peak memory: one eager step above what is
resident before it.

    python3 profiles/qknorm_probe.py [--reps 20] [--rounds 7] [--steps 10] [--arms on,off] [--out profiles/qknorm_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vited_amd as v  # noqa: E402

HBM_PEAK_TBPS = 8.0
KERNEL_SHAPES = [('A encoder', 65536, 12, 32), ('A decoder', 66560, 12, 32), ('H encoder', 24 * 1024, 6, 64), ('H decoder', 72 * 1025, 6, 64)]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


def kernel_rows(dev, reps, rounds):
    ops = v.ops
    g = torch.Generator(device='cpu').manual_seed(0)
    rows = []
    for name, m, heads, hd in KERNEL_SHAPES:
        d = heads * hd
        qkv = torch.randn(m, 3 * d, generator=g).to(dev).bfloat16()
        dqkv0 = torch.randn(m, 3 * d, generator=g).to(dev).bfloat16()
        dqkv = dqkv0.clone()
        qk = torch.empty((m, 2 * d), dtype=torch.bfloat16, device=dev)
        gq, bq, gk, bk = (torch.randn(hd, generator=g).to(dev) for _ in range(4))
        fwd = lambda: ops.qk_norm_fwd(qkv[:, :d], qkv[:, d:2 * d], gq, bq, gk, bk, heads, 1e-6, out=(qk[:, :d], qk[:, d:]))
        _, _, sq, sk = fwd()
        dg = [torch.zeros(hd, device=dev) for _ in range(4)]
        # (the backward overwrites dy by dx; timing it on its own output changes values, not traffic)
        bwd = lambda: ops.qk_norm_bwd(dqkv[:, :d], qkv[:, :d], sq, gq, dqkv[:, d:2 * d], qkv[:, d:2 * d], sk, gk, heads, *dg)
        for _ in range(3):
            fwd()
            bwd()
        torch.cuda.synchronize()
        tf, tb = [], []
        for _ in range(rounds):
            tf.append(timed(fwd, reps))
            tb.append(timed(bwd, reps))
        stats = 2 * 2 * m * heads * 4
        bytes_f = 2 * m * d * 2 * 2 + stats
        bytes_b = 2 * m * d * 2 * 3 + stats
        mf, mb = statistics.median(tf), statistics.median(tb)
        rows.append(dict(shape=name, rows=m, heads=heads, head_dim=hd, fwd_us=mf, fwd_us_min_max=[min(tf), max(tf)], bwd_us=mb,
                         bwd_us_min_max=[min(tb), max(tb)], fwd_bytes=bytes_f, bwd_bytes=bytes_b, fwd_GBps=bytes_f / mf / 1e3,
                         bwd_GBps=bytes_b / mb / 1e3, fwd_frac_of_hbm_peak=bytes_f / mf / 1e6 / HBM_PEAK_TBPS,
                         bwd_frac_of_hbm_peak=bytes_b / mb / 1e6 / HBM_PEAK_TBPS))
        print(f'{name:10s} {m:6d} x {heads:2d} x {hd}: fwd {mf:7.1f} us ({min(tf):.1f} .. {max(tf):.1f}) {bytes_f / mf / 1e3:6.0f} GB/s'
              f'   bwd {mb:7.1f} us ({min(tb):.1f} .. {max(tb):.1f}) {bytes_b / mb / 1e3:6.0f} GB/s (two finishing launches included)', flush=True)
    return rows


def make_step(dev, arm, batch, use_graph=True):
    torch.manual_seed(0)
    kw = dict(qk_norm=True) if arm == 'on' else {}
    model = v.VisionTransformerCustom(img_size=64, patch_size=8, num_classes=4, embed_dim=384, depth=8, c_depth=8, num_heads=12, **kw).to(dev)
    opt = v.optim.FlatAdamW(v.engine.param_groups_no_decay_1d(model), model=model, lr=1e-4 * batch / 256.0, weight_decay=0.05)
    return model, v.engine.TrainStep(model, opt, clip_grad=5.0, amp=True, use_graph=use_graph)


def step_rows(dev, arms, batch, steps, rounds):
    g = torch.Generator(device='cpu').manual_seed(1)
    x = torch.randn(batch, 2, 3, 64, 64, generator=g).clamp_(-1, 1).to(dev)
    y = (torch.rand(batch, 4, generator=g) > 0.75).float().to(dev)
    res = {}
    # peak memory of one eager step above the resident state (model, optimizer state, flat gradients, batch), one arm at a time
    for arm in arms:
        model, step = make_step(dev, arm, batch, use_graph=False)
        step.step(x, y)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss = step.step(x, y)
        torch.cuda.synchronize()
        res[arm] = dict(resident_bytes=base, step_peak_above_resident_bytes=torch.cuda.max_memory_allocated() - base, loss=float(loss))
        print(f'{arm:3s}: one eager step peaks {res[arm]["step_peak_above_resident_bytes"] / 2**30:.3f} GiB above {base / 2**30:.3f} GiB resident',
              flush=True)
        del model, step
        torch.cuda.empty_cache()
    steppers = {arm: make_step(dev, arm, batch) for arm in arms}
    for arm in arms:
        for _ in range(6):                      # eager steps, capture, first replays
            steppers[arm][1].step(x, y)
    torch.cuda.synchronize()
    times = {arm: [] for arm in arms}
    for _ in range(rounds):
        for arm in arms:                        # alternating blocks
            times[arm].append(timed(lambda: steppers[arm][1].step(x, y), steps) / 1e3)
    for arm in arms:
        t = times[arm]
        res[arm].update(step_ms=statistics.median(t), step_ms_min_max=[min(t), max(t)], graphs=steppers[arm][1]._g1 is not None)
        print(f'{arm:3s}: config A step, B {batch}: {statistics.median(t):.3f} ms ({min(t):.3f} .. {max(t):.3f})', flush=True)
    if 'on' in res and 'off' in res:
        res['on_minus_off_ms'] = res['on']['step_ms'] - res['off']['step_ms']
        res['on_minus_off_peak_bytes'] = res['on']['step_peak_above_resident_bytes'] - res['off']['step_peak_above_resident_bytes']
        print(f'on - off: {res["on_minus_off_ms"]:+.3f} ms, {res["on_minus_off_peak_bytes"] / 2**30:+.3f} GiB at the peak')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--arms', default='on,off')
    ap.add_argument('--skip-kernel', action='store_true')
    ap.add_argument('--trace-steps', type=int, default=0, help='only replay this many steps of the on-arm (for a kernel trace run)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'qknorm_probe.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('qknorm_probe.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    arms = [s for s in a.arms.split(',') if s]
    if a.trace_steps:
        g = torch.Generator(device='cpu').manual_seed(1)
        x = torch.randn(a.batch, 2, 3, 64, 64, generator=g).clamp_(-1, 1).to(dev)
        y = (torch.rand(a.batch, 4, generator=g) > 0.75).float().to(dev)
        _, step = make_step(dev, arms[0], a.batch, use_graph=False)
        for _ in range(a.trace_steps):
            step.step(x, y)
        torch.cuda.synchronize()
        return
    result = dict(device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, steps_per_block=a.steps, batch=a.batch)
    if not a.skip_kernel and 'on' in arms:
        result['kernel'] = kernel_rows(dev, a.reps, a.rounds)
    result['step'] = step_rows(dev, arms, a.batch, a.steps, a.rounds)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(f'wrote {a.out}')


if __name__ == '__main__':
    main()
