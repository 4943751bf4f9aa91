#!/usr/bin/env python3
"""The geshaem evaluation on the device against its host forms.

    python3 profiles/pair_metrics_probe.py [--reps 9] [--no-host]                 # on the GPU box
    python3 profiles/pair_metrics_probe.py --reference-only --reference <checkout>  # the reference's calc_map_prak, CPU only

Aggregation (PairScoreAggregator: one add of all records + finish, records sorted by (i, j) as an unshuffled loader gives them):
median event-timed time at 1M / 4M records into 500 / 2,000 fragments, beside the wall time of the dict-of-lists restatement
(tests/test_pair_metrics.py, michigan.py:188-223) for the 1M cases.  map_prak at n = 2,000 / 5,000 / 20,000, groups of ~10
fragments, without and with negatives (~100 negative labels per label): median event-timed time of both launches and the CSR
plumbing, beside the stable numpy restatement (timed on --host-rows rows and scaled to n).  --reference-only times the
reference's own calc_map_prak on the same matrices (scaled from --host-rows rows as well).
"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def timed(call, reps):
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def records(rng, m, n_frag):
    """m records (i <= j) sorted by (i, j), scores in (0, 1)."""
    i = rng.integers(0, n_frag, m)
    j = rng.integers(0, n_frag, m)
    pairs = np.stack([np.minimum(i, j), np.maximum(i, j)], axis=1)
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    return pairs, rng.random(m).astype(np.float32)


def group_case(rng, n):
    labels = [f'f{v}' for v in range(n)]
    perm = rng.permutation(n)
    pos = {}
    for g0 in range(0, n, 10):
        g = {labels[v] for v in perm[g0:g0 + 10]}
        for a in g:
            pos[a] = g
    neg = {a: {labels[v] for v in rng.integers(0, n, 100)} for a in labels}
    D = rng.random((n, n), dtype=np.float32).astype(np.float16)
    return D, labels, pos, neg


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--n', type=int, nargs='*', default=[2000, 5000, 20000])
    ap.add_argument('--host-rows', type=int, default=500)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--reference-only', action='store_true')
    ap.add_argument('--reference', default=None, help='checkout of glmanhtu/vit-ed (misc/metric.py), for --reference-only')
    a = ap.parse_args()
    from test_pair_metrics import reference_distance_maps, reference_group_rows

    if a.reference_only:
        spec = importlib.util.spec_from_file_location('metric', os.path.join(a.reference, 'misc', 'metric.py'))
        metric = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(metric)
        for n in a.n:
            for with_neg in (False, True):
                D, labels, pos, neg = group_case(np.random.default_rng(n), n)
                rows = min(n, a.host_rows)
                t0 = time.perf_counter()
                metric.calc_map_prak(D[:rows].astype(np.float32), np.array(labels), pos, neg if with_neg else None, prak=(1, 5, 10))
                wall = (time.perf_counter() - t0) * n / rows
                print(f'map_prak n={n:6d} neg={with_neg!s:5}  reference calc_map_prak {wall:9.2f} s (scaled from {rows} rows)', flush=True)
        return

    import vited_amd as v
    dev = torch.device('cuda:0')
    for m, n_frag in ((1 << 20, 500), (1 << 20, 2000), (1 << 22, 500), (1 << 22, 2000)):
        pairs, scores = records(np.random.default_rng(m + n_frag), m, n_frag)
        pd, sd = torch.from_numpy(pairs).to(dev), torch.from_numpy(scores).to(dev)

        def call():
            agg = v.engine.PairScoreAggregator(n_frag, dev)
            agg.add(pd, sd)
            return agg.finish()
        ms = timed(call, a.reps)
        res = call()
        line = f'aggregate m={m:8d} fragments={n_frag:5d}  device {ms:8.3f} ms  avg_std {res.std_stats[0]:.6f}'
        if not a.no_host and m <= 1 << 20:
            t0 = time.perf_counter()
            *_, avg_std, _ = reference_distance_maps(pairs, scores)
            wall = time.perf_counter() - t0
            line += f'  | host dict-of-lists {wall:8.2f} s ({wall * 1e3 / ms:7.0f}x)  avg_std diff {abs(avg_std - res.std_stats[0]):.1e}'
        print(line, flush=True)
        del pd, sd, res

    for n in a.n:
        D, labels, pos, neg = group_case(np.random.default_rng(n), n)
        Dd = torch.from_numpy(D).to(dev)
        for with_neg in (False, True):
            rel_neg = neg if with_neg else None
            ms = timed(lambda: v.engine.map_prak(Dd, labels, pos, rel_neg, (1, 5, 10)), a.reps)
            rel = v.engine.group_relations(labels, pos, rel_neg, dev)
            kern = timed(lambda: v.ops.group_retrieval_metrics_rows(Dd, *rel, (1, 5, 10), (0, n)), a.reps)
            got = v.engine.map_prak(Dd, labels, pos, rel_neg, (1, 5, 10))
            line = (f'map_prak n={n:6d} neg={with_neg!s:5}  map_prak {ms:8.3f} ms (kernels {kern:7.3f} ms)  '
                    f'mAP {got[0]:.6f} pr@k {", ".join(f"{x:.4f}" for x in got[1])}')
            if not a.no_host:
                rows = min(n, a.host_rows)
                t0 = time.perf_counter()
                reference_group_rows(D[:rows], labels, range(rows), pos, rel_neg, (1, 5, 10))
                wall = (time.perf_counter() - t0) * n / rows
                line += f'  | host numpy {wall:8.2f} s (scaled from {rows} rows, {wall * 1e3 / ms:7.0f}x)'
            print(line, flush=True)
        del Dd


if __name__ == '__main__':
    main()
