#!/usr/bin/env python3
"""The 768-wide row-complete Linear + LayerNorm kernels (gemm_row768.hip) against the two-kernel forms they replace, at the shapes of
a ViT-Base step, and what they are worth in that step.

    python3 profiles/row768_probe.py [--rounds 7] [--reps 20] [--steps 3] [--children 3] [--out profiles/row768_probe.json]

The driver opens no GPU: each part runs in a child process of its own and prints one JSON line.
  kernels  one process, per shape the two arms alternating inside every round, device events around ``--reps`` launches (us per
           launch), median and lowest .. highest of ``--rounds`` rounds.  Rows 13,824 (24 images x 576 tokens) and 41,544 (72 pairs
           x 577):  forward  y = res + a W^T + b ; h = LN(y)          vs  vited_gemm(RESIDUAL) + vited_layernorm_fwd    K 768, 3072
                    backward dx = dx_in + LN'(dy Wt^T) (+ bf16 copy)  vs  vited_gemm(STORE) + vited_layernorm_bwd       K 768 .. 3072
           ``clears`` = the fused arm's range lies wholly below the two-kernel arm's; ``predicate`` = what
           vited_linear_layernorm_supported answers for the shape (the entries are timed directly, whatever it says).
  step     the two-stage training step at ViT-Base (24 images of 384 x 384, 72 mined pairs, 12 + 12 blocks, bf16, FlatAdamW, drop-path
           0.1, random data), eager and replayed, VITED_FUSED_LN=1 against 0 in alternating fresh processes, ``--children`` each."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 768
ROWS = (24 * 576, 72 * 577)
FWD_K, BWD_K = (768, 3072), (768, 1536, 2304, 3072)


def spread(values):
    return {'median': round(statistics.median(values), 3), 'lowest': round(min(values), 3), 'highest': round(max(values), 3)}


def gpu():
    sys.path.insert(0, ROOT)
    import torch
    import vited_amd as v
    if not torch.cuda.is_available():
        raise SystemExit('row768_probe.py measures on the GPU: none found')
    v._lib.load()
    return torch, v, torch.device('cuda:0')


def kernels(args):
    torch, v, dev = gpu()
    ops, L = v.ops, v._lib
    g = torch.Generator(device='cpu').manual_seed(0)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dev)

    def timed(fn):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        e.record()
        e.synchronize()
        return a.elapsed_time(e) / args.reps * 1e3

    gamma, beta, bias = 1.0 + rnd(N, scale=0.1), rnd(N, scale=0.1), rnd(N, scale=0.1)
    out = []
    for M in ROWS:
        res = rnd(M, N)
        mean, rstd = rnd(M, scale=0.1), 1.0 + rnd(M, scale=0.1).abs()
        for mode, ks in (('fwd', FWD_K), ('bwd', BWD_K)):
            for K in ks:
                x_lp, w = rnd(M, K).bfloat16(), rnd(N, K, scale=K ** -0.5).bfloat16()
                if mode == 'fwd':
                    def two():
                        y = ops.gemm(x_lp, w, epilogue=L.EPI_RESIDUAL, bias=bias, residual=res)
                        return ops.layernorm_fwd(y, gamma, beta, 1e-6, torch.bfloat16)

                    def fused():
                        return ops.linear_residual_layernorm_fwd(x_lp, w, bias, res, gamma, beta, 1e-6)
                else:
                    def two():
                        dh = ops.gemm(x_lp, w)
                        return ops.layernorm_bwd(dh, res, gamma, mean, rstd, dx_in=res, want_lp=True)

                    def fused():
                        return ops.linear_layernorm_bwd(x_lp, w, res, gamma, mean, rstd, dx_in=res, want_lp=True)
                arms = {'two_kernels': two, 'fused': fused}
                for fn in arms.values():                 # warm-up: first launches, then one untimed round of the timed window itself
                    for _ in range(3):
                        fn()
                for fn in arms.values():
                    timed(fn)
                us = {a: [] for a in arms}
                for _ in range(args.rounds):
                    for a, fn in arms.items():
                        us[a].append(timed(fn))
                row = {'mode': mode, 'rows': M, 'K': K, 'predicate': bool(ops.linear_layernorm_supported(M, N, K, torch.bfloat16)), 'two_kernels_us': spread(us['two_kernels']),
                       'fused_us': spread(us['fused'])}
                row['clears'] = row['fused_us']['highest'] < row['two_kernels_us']['lowest']
                row['fused_tflops'] = round(2.0 * M * N * K / row['fused_us']['median'] / 1e6, 1)
                print(row, file=sys.stderr, flush=True)
                out.append(row)
    print(json.dumps({'device': torch.cuda.get_device_name(dev), 'rounds': args.rounds, 'reps': args.reps, 'shapes': out}))


def step(args):
    torch, v, dev = gpu()
    E = v.engine
    images, capacity = 24, E.mined_pair_capacity(24, 3)
    torch.manual_seed(0)

    def model():
        return v.VisionTransformerCustom(img_size=384, patch_size=16, num_classes=1, embed_dim=N, depth=12, c_depth=12, num_heads=12,
                                         drop_path_rate=0.1).to(dev).train()

    state = model().state_dict()
    samples = torch.randn(images, 3, 384, 384, device=dev).clamp_(-1, 1)
    targets = torch.arange(images // 3, device=dev).repeat_interleave(3)
    runs = {}
    for arm in ('eager', 'replay'):
        m = model()
        m.load_state_dict(state)
        opt = v.optim.FlatAdamW(E.param_groups_no_decay_1d(m), lr=1e-4, weight_decay=0.05)
        st = E.TwoStageTrainStep(m, opt, capacity=capacity, clip_grad=5.0, amp=True, use_graph=arm == 'replay')
        for _ in range(4):                                   # two eager updates, the capture, one more
            loss = st.step(samples, targets)
        torch.cuda.synchronize()
        if arm == 'replay' and (st._g1 is None or st._g2 is None):
            raise SystemExit('the two-stage step was not captured')
        runs[arm] = (st, float(loss))
    ms = {a: [] for a in runs}
    for _ in range(args.rounds):
        for arm, (st, _) in runs.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.steps):
                st.step(samples, targets)
            e.record()
            e.synchronize()
            ms[arm].append(round(a.elapsed_time(e) / args.steps, 3))
    print(json.dumps({'fused_ln': os.environ.get('VITED_FUSED_LN', '1') != '0', 'capacity': capacity,
                      'ms_per_step': {a: dict(spread(ms[a]), rounds=ms[a]) for a in ms}, 'warmup_loss': {a: runs[a][1] for a in runs}}))


def child(part, args, env=None):
    cmd = [sys.executable, os.path.abspath(__file__), '--part', part, '--rounds', str(args.rounds), '--reps', str(args.reps), '--steps',
           str(args.steps)]
    out = subprocess.run(cmd, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(f'{part} child failed with status {out.returncode}')        # nothing more is started on the GPU
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=('all', 'kernels', 'step', 'kernels-only', 'step-only'), default='all')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--children', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.part == 'kernels':
        return kernels(args)
    if args.part == 'step':
        return step(args)
    res = {'probe': 'row768'}
    if args.part in ('all', 'kernels-only'):
        res['kernels'] = child('kernels', args)
    if args.part in ('all', 'step-only'):
        runs = {'1': [], '0': []}
        for _ in range(args.children):
            for flag in ('1', '0'):
                runs[flag].append(child('step', args, {'VITED_FUSED_LN': flag}))
                print(f"VITED_FUSED_LN={flag}: { {a: r['median'] for a, r in runs[flag][-1]['ms_per_step'].items()} }", file=sys.stderr, flush=True)
        res['step'] = {}
        for flag, name in (('1', 'fused'), ('0', 'two_kernels')):
            res['step'][name] = {arm: dict(spread([r['ms_per_step'][arm]['median'] for r in runs[flag]]),
                                           processes=[r['ms_per_step'][arm] for r in runs[flag]]) for arm in ('eager', 'replay')}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
