#!/usr/bin/env python3
"""The classical puzzle baseline's pixel kernels on the MI355X: cut, border distances, board, and the whole solve_pixel_puzzle.

    python3 profiles/puzzle_pixels_probe.py [--reps 30] [--out profiles/puzzle_pixels_probe.json]

Per board (432 / 540 / 805 pieces are the BGU test-set sizes of DESIGN.md section 14, 2000 a larger one; P = 28, erosion 0, a seeded
smooth synthetic image with a little noise, the pieces shuffled by a seeded permutation), event-timed calls after two warm-up calls
each, the arms of a repetition interleaved; medians and ranges in ms:
  * cut:        ops.puzzle_cut (image -> pieces, with the permutation's upload)
  * distances:  ops.puzzle_pixel_distances (pieces -> Dq int32 [4, n, n]; the strip pass and the all-pairs pass)
  * assemble:   ops.puzzle_assemble (pieces -> board, with the cell table's upload), framed in the reference's marker, at erosion 0.1 (We = 26)
  * resize:     ops.puzzle_resize_pieces to 64 x 64, the learned path's input
and, for the three BGU sizes, the wall time of engine.solve_pixel_puzzle (cut, distances, Paikin-Tal with its host loop, accuracies,
board) after one warm-up call, with its recalculation count and neighbour accuracy.
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

GRIDS = {432: (18, 24), 540: (20, 27), 805: (23, 35), 2000: (40, 50)}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'puzzle_pixels_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('puzzle_pixels_probe needs the MI355X: nothing is measured without it')
    dev = torch.device('cuda:0')
    ops, engine = v.ops, v.engine
    result = {'piece_width': P, 'reps': args.reps, 'device': torch.cuda.get_device_name(0), 'boards': {}}
    for n, (rows, cols) in GRIDS.items():
        rng = np.random.default_rng(n)
        host = np.ascontiguousarray(smooth_image(rng, rows * P + 5, cols * P + 8, 2.0))
        image = torch.from_numpy(host).to(dev)
        perm = rng.permutation(n)
        pieces = ops.puzzle_cut(image, P, P, order=perm)
        eroded = ops.puzzle_cut(image, P, ops.puzzle_eroded_width(P, 0.1), order=perm)
        true = np.stack([perm // cols, perm % cols], axis=1)
        moved = np.roll(true, 1, axis=0)                      # every piece one place on: all of them framed
        arms = {'cut': lambda: ops.puzzle_cut(image, P, P, order=perm),
                'distances': lambda: ops.puzzle_pixel_distances(pieces),
                'assemble': lambda: ops.puzzle_assemble(eroded, moved, true, P, marker=(0, 0, 255)),
                'resize_64': lambda: ops.puzzle_resize_pieces(pieces, 64)}
        entry = {'grid': [rows, cols], 'image': list(host.shape), **_timed(arms, args.reps)}
        if n <= 805:
            engine.solve_pixel_puzzle(image, P, 0., order=perm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            solution, acc, board = engine.solve_pixel_puzzle(image, P, 0., order=perm)
            torch.cuda.synchronize()
            entry['solve_pixel_puzzle'] = {'wall_s': time.perf_counter() - t0, 'recalcs': solution.recalcs, 'neighbor': acc['neighbor'],
                                           'perfect': bool(acc['perfect'])}
        result['boards'][str(n)] = entry
        print(n, json.dumps(entry), flush=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
