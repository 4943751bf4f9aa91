#!/usr/bin/env python3
"""Ranked retrieval lists (vited_retrieval_topk) and the curve counts (vited_retrieval_curves) on fp16 similarity matrices.

    python3 profiles/ranklists_probe.py [--n 5000 10000 20000] [--k 10 100] [--reps 15] [--out profiles/ranklists_probe.json]

Per n (classes of about 10, scores 0.3 higher within a class) and k, event-timed calls, the arms of a repetition interleaved:
  * kernel:  ops.retrieval_topk_rows(S, k, from_similarity=True, remove_self_column=True) - indices, values, hits;
  * topk:    what a user has on the device today, torch.topk(1 - S, k + 1, largest=False) with the n x n temporary counted;
  * host:    what a user has on the host today, S copied to the host (counted), np.argpartition + a sort of the k + 1 survivors
             (wall clock, --host-reps repetitions);
and, on the same matrix, ops.retrieval_curve_rows against ops.retrieval_metrics_rows: the same row kernel with and without the
integer adds of the curve record (the curve call includes zeroing its n - 1 counters).  "saturated" repeats the list arms on scores
rounded to exactly 0 and 1, where every row is two runs of ties.  passes: the histogram passes of the selection per row, counted by
a numpy walk of the kernel's schedule on --sample rows.  Medians and ranges in ms.
"""
import argparse
import json
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
from ranklists_cases import order_bits, rank_value  # noqa: E402

BINS, CAND = 2048, 2048


def _passes(row_values, K):
    """Histogram passes the selection takes on one row (csrc/rank_key.h: sel_pass, sel_cut, sel_fits)."""
    n = row_values.size
    keys = (order_bits(row_values).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    cbits = max(1, int(n - 1).bit_length())
    sched = [(53, 11), (42, 11), (32, 10)]
    left = cbits
    while left > 0:
        bits = min(left, 11)
        sched.append((left - bits, bits))
        left -= bits
    bound, below = np.uint64(0), 0
    for p, (shift, bits) in enumerate(sched):
        hi = shift + bits
        match = np.ones(n, bool) if hi >= 64 else (keys >> np.uint64(hi)) == (bound >> np.uint64(hi))
        hist = np.bincount(((keys[match] >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int64), minlength=BINS)
        cum = np.cumsum(hist)
        b = int(np.searchsorted(cum, K - below, side='left'))
        below += int(cum[b] - hist[b])
        bound |= np.uint64(b) << np.uint64(shift)
        if below + int(hist[b]) <= CAND:
            return p + 1
    return len(sched)


def _timed(arms, reps):
    """arms: name -> callable.  Interleaved event timing; returns name -> {median, min, max} in ms."""
    for call in arms.values():
        for _ in range(2):
            call()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(reps):
        for name, call in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return {name: {'median_ms': statistics.median(t), 'min_ms': min(t), 'max_ms': max(t)} for name, t in times.items()}


def _host_lists(S, k, reps):
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        D = 1 - S.cpu().numpy()                                   # the copy and the n x n temporary are the user's cost today
        part = np.argpartition(D, k, axis=1)[:, :k + 1]
        order = np.take_along_axis(part, np.argsort(np.take_along_axis(D, part, axis=1), axis=1, kind='stable'), axis=1)[:, 1:]
        walls.append((time.perf_counter() - t0) * 1e3)
        del D, part, order
    return {'median_ms': statistics.median(walls), 'min_ms': min(walls), 'max_ms': max(walls), 'reps': reps}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--n', type=int, nargs='*', default=[5000, 10000, 20000])
    ap.add_argument('--k', type=int, nargs='*', default=[10, 100])
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--host-reps', type=int, default=2)
    ap.add_argument('--sample', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ranklists_probe.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    result = {'device': torch.cuda.get_device_name(0), 'dtype': 'float16', 'reps': a.reps, 'cases': []}
    for n in a.n:
        g = torch.Generator(device=dev).manual_seed(n)
        labels = torch.randint(0, max(1, n // 10), (n,), device=dev, generator=g)
        S = torch.rand((n, n), device=dev, generator=g).mul_(0.7).to(torch.float16)
        for r0 in range(0, n, 4096):                              # S += 0.3 within a class, without an n x n bool temporary
            S[r0:r0 + 4096] += 0.3 * (labels[r0:r0 + 4096, None] == labels[None, :]).to(torch.float16)
        saturated = (S > 0.6).to(torch.float16)
        ids, off, mem = v.engine.class_members(labels)
        sample = np.random.default_rng(n).choice(n, min(a.sample, n), replace=False)
        case = {'n': n, 'lists': [], 'saturated_lists': []}
        for name, M in (('lists', S), ('saturated_lists', saturated)):
            for k in a.k:
                arms = {'kernel': lambda: v.ops.retrieval_topk_rows(M, k, (0, n), ids, from_similarity=True),
                        'torch_topk_with_temporary': lambda: torch.topk(1 - M, k + 1, dim=1, largest=False)}
                entry = {'k': k, **_timed(arms, a.reps)}
                rows = rank_value(M[torch.from_numpy(sample).to(dev)].cpu(), True)
                passes = [_passes(r, k + 1) for r in rows]
                entry['histogram_passes_per_row'] = {'mean': float(np.mean(passes)), 'min': int(min(passes)), 'max': int(max(passes))}
                if name == 'lists':
                    idx, _, _ = v.ops.retrieval_topk_rows(M, k, (0, n), ids, from_similarity=True)
                    ref = torch.topk(1 - M, k + 1, dim=1, largest=False).indices[:, 1:]
                    entry['rows_equal_to_torch_topk'] = float((idx == ref).all(dim=1).float().mean())   # ties are ordered differently
                    entry['host_argpartition_with_copy'] = _host_lists(M, k, a.host_reps)
                case[name].append(entry)
                print(n, name, json.dumps(entry), flush=True)
        estimate = torch.full((n,), 10, dtype=torch.int32, device=dev)
        arms = {'metrics_rows': lambda: v.ops.retrieval_metrics_rows(S, ids, off, mem, (0, n), from_similarity=True),
                'curve_rows': lambda: v.ops.retrieval_curve_rows(S, ids, off, mem, (0, n), from_similarity=True, estimate=estimate)}
        case['curves'] = _timed(arms, a.reps)
        print(n, 'curves', json.dumps(case['curves']), flush=True)
        result['cases'].append(case)
        del S, saturated
        torch.cuda.empty_cache()
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
