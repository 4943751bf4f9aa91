#!/usr/bin/env python3
"""Type-2 puzzles (pieces of unknown rotation) on the MI355X, each step beside its type-1 counterpart in the same process.

    python3 profiles/puzzle_type2_probe.py [--n 432 540 805] [--reps 30] [--out profiles/puzzle_type2_probe.json]

Per n (432 / 540 / 805 pieces are the BGU test-set sizes of DESIGN.md section 14), event-timed calls after two warm-up calls each,
the two arms of a repetition interleaved; medians and ranges in ms:
  * distances:   ops.puzzle_pixel_distances on pieces of 28 x 28 cut from a seeded smooth image, puzzle_type 1 (Dq [4, n, n]) and 2
                 (Dq2 [4, n, n, 4]: 4 x the outputs);
  * compat_init: ops.puzzle_compat_init / puzzle_compat2_init on a synthetic noisy Dq2 and its type-1 slice;
  * recalc:      one recalculation with about half the pieces placed (repeating one mask: only the first call changes anything, so
                 the figure is the min / second pass plus two almost empty passes, as in section 14);
  * slot scan:   2 sqrt(n) open slots;
and the wall time of engine.solve_puzzle on that synthetic Dq2 and on its type-1 slice, after one warm-up call each, with the
recalculation counts and the accuracies.
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import vited_amd as v  # noqa: E402
from make_puzzle_pixels_golden import smooth_image  # noqa: E402

GRIDS = {432: (18, 24), 540: (20, 27), 805: (23, 35)}
P = 28


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


def synthetic_dq2(rows, cols, seed):
    """Noisy distances int32 [4, n, n, 4]: true neighbours drawn lower at (s, (s + 2) % 4), as profiles/puzzle_probe.py draws its Dq."""
    rng = np.random.default_rng(seed)
    n = rows * cols
    loc = np.array([(r, c) for r in range(rows) for c in range(cols)])[rng.permutation(n)]
    where = {tuple(p): k for k, p in enumerate(loc)}
    D = rng.integers(150, 1000, size=(4, n, n, 4), dtype=np.int32)
    for i in range(n):
        for s, (dr, dc) in enumerate(((-1, 0), (0, 1), (1, 0), (0, -1))):
            j = where.get((loc[i, 0] + dr, loc[i, 1] + dc))
            if j is not None:
                D[s, i, j, (s + 2) % 4] = rng.integers(0, 250)
    D[:, np.arange(n), np.arange(n), :] = 2 ** 31 - 1
    return D, loc


def _solve(engine, dq, grid, true_loc):
    engine.solve_puzzle(dq, grid)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sol = engine.solve_puzzle(dq, grid)
    wall = time.perf_counter() - t0
    acc = engine.puzzle_accuracy(sol, true_loc)
    return {'wall_s': wall, 'recalcs': sol.recalcs, 'direct': acc['Direct_Standard'], 'neighbor': acc['neighbor'],
            **({'wrong_rotation': acc['wrong_rotation']} if 'wrong_rotation' in acc else {})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, nargs='*', default=list(GRIDS))
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'puzzle_type2_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('puzzle_type2_probe needs the MI355X: nothing is measured without it')
    dev = torch.device('cuda:0')
    ops, engine = v.ops, v.engine
    result = {'piece_width': P, 'reps': args.reps, 'device': torch.cuda.get_device_name(0), 'boards': {}}
    for n in args.n:
        rows, cols = GRIDS[n]
        rng = np.random.default_rng(n)
        image = torch.from_numpy(np.ascontiguousarray(smooth_image(rng, rows * P + 5, cols * P + 8, 2.0))).to(dev)
        pieces = ops.puzzle_cut(image, P, P, order=rng.permutation(n))
        host2, true_loc = synthetic_dq2(rows, cols, n)
        dq2 = torch.from_numpy(host2).to(dev)
        dq1 = torch.stack([dq2[s, :, :, (s + 2) % 4] for s in range(4)]).contiguous()
        comp1, comp2 = engine.PuzzleCompatibility(dq1), engine.PuzzleCompatibility(dq2)
        placed = np.zeros(n, bool)
        placed[np.random.default_rng(1).permutation(n)[:n // 2]] = True
        placed_t = torch.from_numpy(placed.astype(np.int32)).to(dev)
        k = 2 * int(np.sqrt(n))
        sp = torch.from_numpy(np.flatnonzero(placed)[:k].astype(np.int32)).to(dev)
        ss = torch.from_numpy((np.arange(k) % 4).astype(np.int32)).to(dev)
        arms = {'distances_type1': lambda: ops.puzzle_pixel_distances(pieces),
                'distances_type2': lambda: ops.puzzle_pixel_distances(pieces, puzzle_type=2),
                'compat_init_type1': lambda: ops.puzzle_compat_init(dq1),
                'compat_init_type2': lambda: ops.puzzle_compat2_init(dq2),
                'recalc_type1': lambda: ops.puzzle_compat_recalc(comp1.dq, placed_t, comp1.state, comp1.changed),
                'recalc_type2': lambda: ops.puzzle_compat2_recalc(comp2.dq, placed_t, comp2.state, comp2.changed),
                'slot_scan_type1': lambda: ops.puzzle_best_slot(comp1.mutual, placed_t, sp, ss),
                'slot_scan_type2': lambda: ops.puzzle_best_slot2(comp2.mutual, placed_t, sp, ss)}
        entry = {'grid': [rows, cols], 'slots': k, **_timed(arms, args.reps)}
        entry['solve_puzzle_type1'] = _solve(engine, dq1, (rows, cols), true_loc)
        entry['solve_puzzle_type2'] = _solve(engine, dq2, (rows, cols), true_loc)
        result['boards'][str(n)] = entry
        print(n, json.dumps(entry), flush=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
