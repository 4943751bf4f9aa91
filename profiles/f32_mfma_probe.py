#!/usr/bin/env python3
"""The fp32 GEMMs on the matrix cores (gemm_f32_mfma.hip) against the vector-ALU kernels that compute the same bits
(gemm_portable.hip), and what the choice is worth in an fp32 training step.

    python3 profiles/f32_mfma_probe.py [--first valu|mfma] [--runs 2] [--rounds 6] [--reps 5] [--out profiles/f32_mfma_probe.json]

One process; ``ops.fp32_gemm_kernels`` switches between the two kernels, which alternate inside every round.  Per shape and kernel
a sample is a pair of device events around ``--reps`` launches (``--rounds`` samples = rounds x reps >= 20 calls a run), after a
warm-up of both kernels at that shape that includes one untimed window.  ``--runs`` passes over all shapes are recorded apart, each
with median and lowest .. highest; ``faster`` = the matrix-core kernel's highest sample lies below the vector-ALU kernel's lowest
in every run.  ``--first`` names the kernel that goes first in each round: the committed pair of files has one of each.

  forward   out = a W^T (fp32, B_NK, EPI_STORE) at the rows of config A (65,536), config H (24,576) and ViT-Base (36,864), and the
            edge shapes M = 64, 128 x N = 32, 64 (K = 384) that decide the predicate (``predicate`` = what
            ``ops.fp32_gemm_supported`` answers; under 'auto' a shape it rejects runs the vector-ALU kernel in both arms); 'mid' rows
            1,024 .. 16,384 at (384, 384) straddle the grid size at which the dispatcher changes from the 64-wide to the 128-wide
            tile (with a library built with EXTRA=-DFM_FORCE_TILE=64 / 128 and VITED_LIB, ``--only edge,mid`` times one tile alone)
  wgrad     dW = dy^T x (ops.linear_bwd_weight, with bias) at config A's fc1
  step      one eager fp32 TrainStep (amp off, FlatAdamW, clip 5.0) of config A's model at batch 128"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_A = os.path.join(ROOT, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml')
BLOCK_NK = ((1152, 384), (384, 384), (1536, 384), (384, 1536))
FORWARD = ([('config A', 65536, n, k) for n, k in BLOCK_NK] + [('config H', 24576, n, k) for n, k in BLOCK_NK]
           + [('ViT-Base', 36864, 768, 768), ('ViT-Base', 36864, 3072, 768)] + [('edge', m, n, 384) for m in (64, 128) for n in (32, 64)]
           + [('mid', m, 384, 384) for m in (1024, 4096, 8192, 16384)])
WGRAD = [('config A', 65536, 1536, 384)]
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
    ap.add_argument('--only', default=None, help='comma-separated workloads of the forward table (e.g. edge,mid); no wgrad, no step')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.rounds * args.reps < 20:
        raise SystemExit('at least 20 calls a run: raise --rounds or --reps')
    sys.path.insert(0, ROOT)
    import torch
    import vited_amd as v
    if not torch.cuda.is_available():
        raise SystemExit('f32_mfma_probe.py measures on the GPU: none found')
    v._lib.load()
    ops, dev = v.ops, torch.device('cuda:0')
    order = [args.first] + [m for m in MODES if m != args.first]
    g = torch.Generator(device='cpu').manual_seed(0)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dev)

    def timed(fn, reps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        return a.elapsed_time(e) / reps * 1e3             # us per call

    def measure(fn, reps, kernel_of=None):
        """``--runs`` records of fn under the two kernels, alternating inside every round."""
        ran = {}
        for name in order:                                # warm-up: first launches, then one untimed window
            with ops.fp32_gemm_kernels(MODES[name]):
                for _ in range(3):
                    fn()
                ran[name] = ops.last_fp32_gemm_kernel() if kernel_of is None else kernel_of()
                timed(fn, reps)
        runs = []
        for _ in range(args.runs):
            us = {name: [] for name in order}
            for _ in range(args.rounds):
                for name in order:
                    with ops.fp32_gemm_kernels(MODES[name]):
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

    res = {'probe': 'f32_mfma', 'device': torch.cuda.get_device_name(dev), 'first': args.first, 'runs': args.runs, 'rounds': args.rounds,
           'reps': args.reps, 'unit': 'us per call', 'forward': [], 'wgrad': []}
    only = set(args.only.split(',')) if args.only else None
    for workload, m, n, k in FORWARD:
        if only and workload not in only:
            continue
        a, w, out = rnd(m, k), rnd(n, k, scale=k ** -0.5), torch.empty(m, n, device=dev)
        reps = args.reps * 10 if workload == 'edge' else args.reps
        runs, ran = measure(lambda: ops.gemm(a, w, out=out), reps)
        res['forward'].append(row_of({'workload': workload, 'M': m, 'N': n, 'K': k, 'predicate': ops.fp32_gemm_supported(m, n, k)}, runs,
                                     ran, 2.0 * m * n * k))
        del a, w, out
    for workload, m, n, k in ([] if only else WGRAD):
        dy, x = rnd(m, n), rnd(m, k)
        runs, ran = measure(lambda: ops.linear_bwd_weight(dy, x), args.reps)
        res['wgrad'].append(row_of({'workload': workload, 'M': m, 'N': n, 'K': k, 'includes': 'the slab sum and the dbias column sums'},
                                   runs, ran, 2.0 * m * n * k))
        del dy, x
    if not args.skip_step and not only:
        E, batch = v.engine, 128
        cfg = v.config_from_yaml(CFG_A)
        torch.manual_seed(cfg.SEED)
        model = v.build_model(cfg).to(dev)
        model.compute_dtype = torch.float32
        opt = v.optim.FlatAdamW(E.param_groups_no_decay_1d(model), model=model, lr=1e-4 * batch / 256.0, weight_decay=0.05)
        step = E.TrainStep(model, opt, clip_grad=5.0, amp=False, use_graph=False)
        x = torch.randn(batch, 2, 3, cfg.DATA.IMG_SIZE, cfg.DATA.IMG_SIZE, device=dev).clamp_(-1, 1)
        y = (torch.rand(batch, cfg.MODEL.NUM_CLASSES, device=dev) > 0.75).float()
        seen = set()
        real = ops.gemm

        def spy(*a, **k):                                 # which kernels the GEMMs of a step report (warm-up only)
            r = real(*a, **k)
            seen.add(ops.last_fp32_gemm_kernel())
            return r

        def kernels_of_a_step():
            seen.clear()
            ops.gemm = spy
            try:
                step.step(x, y)
            finally:
                ops.gemm = real
            return sorted(seen)

        runs, ran = measure(lambda: step.step(x, y), args.steps, kernel_of=kernels_of_a_step)
        for r in runs:                                    # a step is timed in ms
            for name in MODES:
                r[name] = {key: round(val / 1e3, 3) for key, val in r[name].items()}
        res['step'] = row_of({'workload': 'config A', 'batch': batch, 'unit': 'ms per step', 'steps_per_sample': args.steps}, runs, ran, None)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
