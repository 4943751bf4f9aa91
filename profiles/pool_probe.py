#!/usr/bin/env python3
"""Pooled head (csrc/pool_head.hip): the two kernels alone against the bytes they must move, and what global_pool='avg' costs one
config A training step.

Kernels: x fp32 [items, tokens, 384] at config A's decoder size (1,024 pairs x 65 tokens) and config H's (72 x 1,025), plain and with
the LayerNorm, forward and backward with a bf16 low-precision copy.  Byte floors: the forward reads the pooled rows of x once; the
backward writes dx (fp32) and its copy (bf16) once and, with the LayerNorm, reads the pooled rows of x once more (pooled, g, the
statistics and the partial rows are noise beside them).  The roof is HBM (8 TB/s peak).  At 72 x 1,025 the forward is two launches
(the chunks, then the fixed-order combine) and with the LayerNorm the backward is two as well (the rows, then the column sums).

Step: config A (64-pixel patch pairs, 384 wide, 12 heads, 8 + 8 blocks), B 1,024, bf16, FlatAdamW, replayed hipGraphs - the default
model, global_pool='avg' (fc_norm by timm's rule) and global_pool='avg' with fc_norm=False in ONE process, timed in alternating
blocks with device events; median, lowest and highest block.  ``--parent DIR`` adds the default model of another checkout of this
project (the parent commit, built) to the same alternation: its package is loaded beside this one under another name, its custom
operator registration left out (one process can define ``torch.ops.vited`` once).  The pooled variants run the last decoder block
on 65 rows per pair instead of 1, so they are expected to cost more than the default; the default itself launches what the parent
launches (tests/test_gpu_pool_head.py::test_off_is_off).

    python3 profiles/pool_probe.py [--parent DIR] [--reps 20] [--rounds 7] [--steps 10] [--out profiles/pool_probe.json]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vited_amd as v  # noqa: E402

HBM_PEAK_TBPS = 8.0
KERNEL_SHAPES = [('A decoder', 1024, 65, 384), ('H decoder', 72, 1025, 384)]
ARMS = {'default': {}, 'avg': dict(global_pool='avg'), 'avg_nofc': dict(global_pool='avg', fc_norm=False)}


def load_parent(path):
    """The ``vit-ed_amd`` package of another checkout under the name ``vited_parent`` (its own shared library, its own workspace)."""
    pkg_dir = os.path.join(os.path.abspath(path), 'vit-ed_amd')
    if not os.path.exists(os.path.join(pkg_dir, 'libvited_hip.so')):
        sys.exit(f'{pkg_dir} has no libvited_hip.so: build that checkout first')
    sys.modules['vited_parent.custom_ops'] = types.ModuleType('vited_parent.custom_ops')      # torch.ops.vited.* is defined once per process
    spec = importlib.util.spec_from_file_location('vited_parent', os.path.join(pkg_dir, '__init__.py'), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules['vited_parent'] = mod
    spec.loader.exec_module(mod)
    assert os.path.dirname(mod._lib.LIB_PATH) == pkg_dir, mod._lib.LIB_PATH
    return mod


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
    for name, items, tokens, d in KERNEL_SHAPES:
        x = torch.randn(items, tokens, d, generator=g).to(dev)
        grad = torch.randn(items, d, generator=g).to(dev)
        gamma, beta = torch.randn(d, generator=g).to(dev), torch.randn(d, generator=g).to(dev)
        dx = torch.empty_like(x)
        lp = torch.empty_like(x, dtype=torch.bfloat16)
        dg, db = torch.zeros(d, device=dev), torch.zeros(d, device=dev)
        pooled = torch.empty(items, d, device=dev)
        _, mean, rstd = ops.token_pool_fwd(x, 1, gamma, beta, 1e-6, save_stats=True)
        row_bytes = items * (tokens - 1) * d
        for norm in (False, True):
            kw = dict(x=x, gamma=gamma, mean=mean, rstd=rstd, dgamma=dg, dbeta=db) if norm else {}
            fwd = (lambda: ops.token_pool_fwd(x, 1, gamma, beta, 1e-6, out=pooled)) if norm else (lambda: ops.token_pool_fwd(x, 1, out=pooled))
            bwd = lambda: ops.token_pool_bwd(grad, tokens, 1, dx=dx, dx_lp=lp, **kw)
            for _ in range(3):
                fwd()
                bwd()
            torch.cuda.synchronize()
            tf, tb = [], []
            for _ in range(rounds):
                tf.append(timed(fwd, reps))
                tb.append(timed(bwd, reps))
            bytes_f = row_bytes * 4
            bytes_b = row_bytes * (4 + 2) + items * d * (4 + 2) + (row_bytes * 4 if norm else 0)      # (+ the zero cls rows)
            mf, mb = statistics.median(tf), statistics.median(tb)
            rows.append(dict(shape=name, items=items, tokens=tokens, dim=d, layernorm=norm, fwd_us=mf, fwd_us_min_max=[min(tf), max(tf)],
                             bwd_us=mb, bwd_us_min_max=[min(tb), max(tb)], fwd_floor_bytes=bytes_f, bwd_floor_bytes=bytes_b,
                             fwd_GBps=bytes_f / mf / 1e3, bwd_GBps=bytes_b / mb / 1e3, fwd_frac_of_hbm_peak=bytes_f / mf / 1e6 / HBM_PEAK_TBPS,
                             bwd_frac_of_hbm_peak=bytes_b / mb / 1e6 / HBM_PEAK_TBPS,
                             fwd_floor_us=bytes_f / HBM_PEAK_TBPS / 1e6, bwd_floor_us=bytes_b / HBM_PEAK_TBPS / 1e6))
            print(f'{name:10s} {items:5d} x {tokens:4d} x {d} {"norm " if norm else "plain"}: fwd {mf:7.1f} us ({min(tf):.1f} .. {max(tf):.1f}) '
                  f'{bytes_f / mf / 1e3:6.0f} GB/s   bwd {mb:7.1f} us ({min(tb):.1f} .. {max(tb):.1f}) {bytes_b / mb / 1e3:6.0f} GB/s', flush=True)
    return rows


def make_step(pkg, dev, kw, batch):
    torch.manual_seed(0)
    model = pkg.VisionTransformerCustom(img_size=64, patch_size=8, num_classes=4, embed_dim=384, depth=8, c_depth=8, num_heads=12, **kw).to(dev)
    opt = pkg.optim.FlatAdamW(pkg.engine.param_groups_no_decay_1d(model), model=model, lr=1e-4 * batch / 256.0, weight_decay=0.05)
    return model, pkg.engine.TrainStep(model, opt, clip_grad=5.0, amp=True, use_graph=True)


def step_rows(dev, parent, batch, steps, rounds):
    g = torch.Generator(device='cpu').manual_seed(1)
    x = torch.randn(batch, 2, 3, 64, 64, generator=g).clamp_(-1, 1).to(dev)
    y = (torch.rand(batch, 4, generator=g) > 0.75).float().to(dev)
    steppers = {}
    if parent is not None:
        steppers['parent'] = make_step(parent, dev, {}, batch)
    for arm, kw in ARMS.items():
        steppers[arm] = make_step(v, dev, kw, batch)
    arms = list(steppers)
    losses = {}
    for arm in arms:
        for _ in range(6):                      # eager steps, capture, first replays
            losses[arm] = float(steppers[arm][1].step(x, y))
    torch.cuda.synchronize()
    times = {arm: [] for arm in arms}
    for _ in range(rounds):
        for arm in arms:                        # alternating blocks
            times[arm].append(timed(lambda: steppers[arm][1].step(x, y), steps) / 1e3)
    res = {}
    for arm in arms:
        t = times[arm]
        res[arm] = dict(step_ms=statistics.median(t), step_ms_min_max=[min(t), max(t)], graphs=steppers[arm][1]._g1 is not None,
                        loss_after_warmup=losses[arm])
        print(f'{arm:9s}: config A step, B {batch}: {statistics.median(t):.3f} ms ({min(t):.3f} .. {max(t):.3f})', flush=True)
    base = 'parent' if parent is not None else 'default'
    for arm in arms:
        res[arm][f'ratio_to_{base}'] = res[arm]['step_ms'] / res[base]['step_ms']
    if parent is not None:
        res['default_equals_parent_loss'] = losses['default'] == losses['parent']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: its default model joins the alternation')
    ap.add_argument('--skip-kernel', action='store_true')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'pool_probe.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('pool_probe.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    parent = load_parent(a.parent) if a.parent else None
    result = dict(device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, steps_per_block=a.steps, batch=a.batch,
                  parent_in_the_same_process=parent is not None)
    if not a.skip_kernel:
        result['kernel'] = kernel_rows(dev, a.reps, a.rounds)
    result['step'] = step_rows(dev, parent, a.batch, a.steps, a.rounds)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(f'wrote {a.out}')


if __name__ == '__main__':
    main()
