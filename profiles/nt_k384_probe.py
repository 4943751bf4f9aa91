#!/usr/bin/env python3
"""Old against new kernel on the K = 384 NT shapes (qkv, kv, fc1 + GELU', dz): gemm_nt_mfma_kernel (256 x 128 tile) against
gemm_nt_areg_kernel (A panel in registers, gemm_nt_k384.hip) in both geometries, timed in interleaved rounds in ONE process.

Needs an experiment build, whose dispatch reads VITED_NT_AREG on every call (0 = old kernel, 8 / 4 = new kernel, waves per workgroup):

    make -C vit-ed_amd/csrc VARIANT=t EXTRA=-DVITED_TUNING
    VITED_LIB=vit-ed_amd/libvited_hip_t.so python3 profiles/nt_k384_probe.py [--rows 65536 66560 24576 73800] [--rounds 7] [--reps 50]

With --modes 0 it times whatever single kernel the library dispatches (the NT_DBG_NO_A_DMA ablation build, the product build).
Prints median and min .. max over the rounds (each round = --reps back-to-back launches between two device events).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vited_amd as v  # noqa: E402

ops, L = v.ops, v._lib

SHAPES = [('qkv', 1152, L.EPI_STORE), ('kv', 768, L.EPI_STORE), ("fc1+gelu'", 1536, L.EPI_GELU_GRAD), ("dz=dy.W2*gelu'", 1536, L.EPI_MUL)]
K = 384


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[65536, 66560, 24576, 73800])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--modes', type=int, nargs='+', default=[0, 8, 4])
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator(device='cpu').manual_seed(0)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dev)

    results = []
    for M in a.rows:
        print(f'M = {M}   (us per launch: median [min .. max] over {a.rounds} rounds of {a.reps})')
        for name, n, epi in SHAPES:
            x, w = rnd(M, K).bfloat16(), rnd(n, K, scale=0.05).bfloat16()
            kw = dict(epilogue=epi)
            if epi == L.EPI_MUL:
                kw['aux'] = rnd(M, n).bfloat16()
            else:
                kw['bias'] = rnd(n)
            kw['out'] = torch.empty(M, n, device=dev, dtype=torch.bfloat16)
            if epi == L.EPI_GELU_GRAD:
                kw['out2'] = torch.empty(M, n, device=dev, dtype=torch.bfloat16)
            times = {m: [] for m in a.modes}
            for m in a.modes:                       # warm-up: code objects, the LDS opt-in
                os.environ['VITED_NT_AREG'] = str(m)
                for _ in range(3):
                    ops.gemm(x, w, **kw)
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for m in a.modes:
                    os.environ['VITED_NT_AREG'] = str(m)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        ops.gemm(x, w, **kw)
                    e1.record()
                    torch.cuda.synchronize()
                    times[m].append(e0.elapsed_time(e1) / a.reps * 1e3)
            line = f'  {name:16s} N={n:5d}'
            for m in a.modes:
                t = times[m]
                line += f' | mode {m}: {statistics.median(t):7.1f} [{min(t):7.1f} .. {max(t):7.1f}]'
                results.append(dict(M=M, shape=name, N=n, mode=m, us=t))
            print(line, flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(results, f)


if __name__ == '__main__':
    main()
