#!/usr/bin/env python3
"""Retrieval metrics (vited_retrieval_metrics) against the host numpy restatement, on fp16 distance matrices.

    python3 profiles/retrieval_probe.py [--n 5000 10000 20000] [--reps 25] [--host-block 2000]

Per n: kernel time (median of --reps event-timed calls after warm-up; both launches: the per-row kernel and the fixed-order
sum), effective bandwidth = matrix bytes / kernel time, and the wall time of the numpy restatement of get_metrics with a stable
argsort on the same matrix (tests/test_retrieval_metrics.py), run in blocks of --host-block rows to bound host memory (the work
is the same as one call over all rows).  Labels: classes of ~10 members, distances 0.3 lower within a class.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import vited_amd as v  # noqa: E402
from test_retrieval_metrics import metrics_from_rows, reference_rows_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, nargs='*', default=[5000, 10000, 20000])
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--host-block', type=int, default=2000)
    ap.add_argument('--no-host', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    for n in a.n:
        g = torch.Generator(device=dev).manual_seed(n)
        labels = torch.randint(0, max(1, n // 10), (n,), device=dev, generator=g)
        D = torch.rand((n, n), device=dev, generator=g).to(torch.float16)
        for r0 in range(0, n, 4096):                         # D -= 0.3 within a class, without an n x n bool temporary
            D[r0:r0 + 4096] -= 0.3 * (labels[r0:r0 + 4096, None] == labels[None, :]).to(torch.float16)
        ids, off, mem = v.engine.class_members(labels)
        call = lambda: v.ops.retrieval_metrics_rows(D, ids, off, mem, (0, n))
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = statistics.median(times)
        rec, sums = call()
        gpu_m = v.engine.metrics_from_sums(sums)
        line = (f'n={n:6d}  kernel {ms:8.3f} ms (min {min(times):.3f}, max {max(times):.3f})  '
                f'{n * n * 2 / ms / 1e6:7.1f} GB/s of fp16 matrix  mAP {gpu_m[0]:.6f} top-1 {gpu_m[1]:.6f}')
        if not a.no_host:
            Dh, lab = D.cpu().numpy(), labels.cpu().numpy()
            t0 = time.perf_counter()
            host = np.concatenate([reference_rows_of(Dh[r0:r0 + a.host_block], lab, np.arange(r0, min(n, r0 + a.host_block)))
                                   for r0 in range(0, n, a.host_block)])
            wall = time.perf_counter() - t0
            host_m = metrics_from_rows(host)
            worst = max(abs(x - y) for x, y in zip(gpu_m, host_m))
            line += f'  | host numpy {wall:8.2f} s  ({wall * 1e3 / ms:7.0f}x)  max |metric diff| {worst:.1e}'
        print(line, flush=True)
        del D


if __name__ == '__main__':
    main()
