#!/usr/bin/env python3
"""Puzzle evaluation on the MI355X: ordered-pair distances, the Paikin-Tal compatibility kernels and the placement loop.

    python3 profiles/puzzle_probe.py [--n 432 540 805] [--reps 20] [--pair-batch 1024]

Per n (pieces of one puzzle; 432 / 540 / 805 are BGU test-set sizes):
  * distances: engine.puzzle_distances on config A (64^2 pieces, patch 8, D 384, 8 + 8 blocks, random weights, bf16), wall time
    of one call after a warm-up call, as ordered pairs n (n - 1) per second;
  * compat_init / recalc / slot scan: median of --reps event-timed calls (recalc with ~half the pieces placed, the slot scan
    over 2 sqrt(n) open slots);
  * solve_puzzle: wall time on a synthetic noisy Dq of a rows x cols grid (true neighbours drawn lower), with its recalc count.
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
import vited_amd as v  # noqa: E402

GRIDS = {432: (18, 24), 540: (20, 27), 805: (23, 35)}


def event_ms(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def synthetic_dq(rows, cols, seed, dev):
    rng = np.random.default_rng(seed)
    n = rows * cols
    loc = np.array([(r, c) for r in range(rows) for c in range(cols)])[rng.permutation(n)]
    where = {tuple(p): k for k, p in enumerate(loc)}
    D = rng.integers(150, 1000, size=(4, n, n))
    for i in range(n):
        for s, (dr, dc) in enumerate(((-1, 0), (0, 1), (1, 0), (0, -1))):
            j = where.get((loc[i, 0] + dr, loc[i, 1] + dc))
            if j is not None:
                D[s, i, j] = rng.integers(0, 250)
    for s in range(4):
        np.fill_diagonal(D[s], 2 ** 31 - 1)
    return torch.from_numpy(D.astype(np.int32)).to(dev), loc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, nargs='*', default=[432, 540, 805])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--pair-batch', type=int, default=1024)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = v.VisionTransformerCustom(img_size=64, patch_size=8, num_classes=4, embed_dim=384, depth=8, c_depth=8,
                                      num_heads=12).to(dev).eval()
    model.compute_dtype = torch.bfloat16
    for n in a.n:
        rows, cols = GRIDS.get(n, (n, 1))
        pieces = torch.randint(0, 256, (n, 3, 64, 64), dtype=torch.uint8, generator=torch.Generator().manual_seed(n)).to(dev)
        v.engine.puzzle_distances(model, pieces[:64], pair_batch=a.pair_batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v.engine.puzzle_distances(model, pieces, pair_batch=a.pair_batch)
        torch.cuda.synchronize()
        t_dist = time.perf_counter() - t0
        dq, true_loc = synthetic_dq(rows, cols, n, dev)
        comp = v.engine.PuzzleCompatibility(dq)
        t_init = event_ms(lambda: v.ops.puzzle_compat_init(dq), a.reps)
        placed = np.zeros(n, bool)
        placed[np.random.default_rng(1).permutation(n)[:n // 2]] = True
        placed_t = torch.from_numpy(placed.astype(np.int32)).to(dev)
        t_recalc = event_ms(lambda: v.ops.puzzle_compat_recalc(comp.dq, placed_t, comp.state, comp.changed), a.reps)
        k = 2 * int(np.sqrt(n))
        sp = torch.from_numpy(np.flatnonzero(placed)[:k].astype(np.int32)).to(dev)
        ss = torch.from_numpy((np.arange(k) % 4).astype(np.int32)).to(dev)
        t_slot = event_ms(lambda: v.ops.puzzle_best_slot(comp.mutual, placed_t, sp, ss), a.reps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sol = v.engine.solve_puzzle(dq, (rows, cols))
        t_solve = time.perf_counter() - t0
        acc = v.engine.puzzle_accuracy(sol, true_loc)
        print(f'n={n} ({rows}x{cols}): distances {t_dist:.2f} s = {n * (n - 1) / t_dist:,.0f} pairs/s | compat_init {t_init:.3f} ms | '
              f'recalc {t_recalc:.3f} ms | slot scan ({k} slots) {t_slot:.3f} ms | solve_puzzle {t_solve:.2f} s, {sol.recalcs} recalcs, '
              f'direct {acc["Direct_Standard"]:.3f} neighbor {acc["neighbor"]:.3f}', flush=True)


if __name__ == '__main__':
    main()
