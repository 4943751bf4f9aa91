#!/usr/bin/env python3
"""The weights-in-registers kernel (gemm_nt_wreg.hip) against what each shape class ran before, timed in interleaved rounds in ONE
process on random data (us per launch set: median [min .. max] over the rounds; a round = one replay of --reps captured launch sets):

  n384      tile kernel (ops.gemm with the wreg dispatch switched off) against ops.gemm_nt_wreg, one group, with and without bias
  kv        8 launches of ops.gemm at N = 768 into kv_all[l] against ONE launch of 16 groups into kv_all
  qkv       ops.gemm at N = 1152 (gemm_nt_areg_kernel<0, 4> from 65,536 rows, else the tile kernel) against three groups
  *-cold    the same arms with the operands and outputs rotated over enough buffer sets that none of them is still in the
            last-level cache when its turn comes (isolated, cache-warm launches mislead for these shapes: DESIGN.md section 5.0.1)

    python3 profiles/wreg_probe.py [--rows 24576 65536 66560 73800] [--rounds 7] [--reps 40] [--json profiles/wreg_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vited_amd as v  # noqa: E402

ops = v.ops
K = W = 384
COLD_BYTES = 1 << 30       # rotate over at least this much: four times the 256 MB last-level cache


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[24576, 65536, 66560, 73800])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, generator=g, device=dev) * scale

    def arms_for(M, sets):
        """name -> (old, new): callables taking a set index; ``sets`` operand / output sets each."""
        xs = [rnd(M, K).bfloat16() for _ in range(sets)]
        w16, b16 = rnd(16 * W, K, scale=0.05).bfloat16(), rnd(16 * W)
        o1 = [torch.empty(M, W, device=dev, dtype=torch.bfloat16) for _ in range(sets)]
        kv = [torch.empty(8, M, 2 * W, device=dev, dtype=torch.bfloat16) for _ in range(sets)]
        o3 = [torch.empty(M, 3 * W, device=dev, dtype=torch.bfloat16) for _ in range(sets)]

        def tile(i, bias):
            with ops.gemm_nt_wreg_dispatch(False):
                ops.gemm(xs[i], w16[:W], bias=b16[:W] if bias else None, out=o1[i])

        def kv_loop(i):
            with ops.gemm_nt_wreg_dispatch(False):
                for l in range(8):
                    ops.gemm(xs[i], w16[l * 2 * W:(l + 1) * 2 * W], bias=b16[l * 2 * W:(l + 1) * 2 * W], out=kv[i][l])

        def qkv_old(i):
            with ops.gemm_nt_wreg_dispatch(False):
                ops.gemm(xs[i], w16[:3 * W], bias=b16[:3 * W], out=o3[i])

        return {
            'n384+bias': (lambda i: tile(i, True), lambda i: ops.gemm_nt_wreg(xs[i], w16[:W], b16[:W], o1[i])),
            'n384': (lambda i: tile(i, False), lambda i: ops.gemm_nt_wreg(xs[i], w16[:W], None, o1[i])),
            'kv 8x768': (kv_loop, lambda i: ops.gemm_nt_wreg(xs[i], w16, b16, kv[i])),
            'qkv 1152': (qkv_old, lambda i: ops.gemm_nt_wreg(xs[i], w16[:3 * W], b16[:3 * W], o3[i])),
        }

    results = []
    for M in a.rows:
        for label, sets in (('warm', 1), ('cold', max(2, -(-COLD_BYTES // (M * (K + W) * 2))))):
            arms = arms_for(M, sets)
            print(f'M = {M} {label} ({sets} buffer set{"s" if sets > 1 else ""}; us: median [min .. max] over {a.rounds} rounds of {a.reps})')
            for name, pair in arms.items():
                times, graphs = ([], []), []
                for fn in pair:
                    for i in range(min(sets, 3)):                         # warm-up: code objects, the LDS opt-in
                        fn(i)
                    torch.cuda.synchronize()
                    # the reps as one captured chain: a 20 - 40 us kernel is shorter than the host's work to enqueue it
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        for r in range(a.reps):
                            fn(r % sets)
                    graph.replay()
                    graphs.append(graph)
                torch.cuda.synchronize()
                for _ in range(a.rounds):
                    for which, graph in enumerate(graphs):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        graph.replay()
                        e1.record()
                        torch.cuda.synchronize()
                        times[which].append(e0.elapsed_time(e1) / a.reps * 1e3)
                line = f'  {name:10s}'
                for which, t in zip(('old', 'new'), times):
                    line += f' | {which}: {statistics.median(t):7.1f} [{min(t):7.1f} .. {max(t):7.1f}]'
                    results.append(dict(M=M, cache=label, shape=name, arm=which, us=[round(x, 2) for x in t]))
                print(line, flush=True)
                del graphs
            del arms
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=0)


if __name__ == '__main__':
    main()
