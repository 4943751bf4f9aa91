#!/usr/bin/env python3
"""Mixed-bag puzzles on the MI355X: engine.solve_puzzle without dimensions with its two ways of reading the mutual compatibility M, and
the lookup launch itself.

    python3 profiles/puzzle_mixed_probe.py [--images 2 4] [--reps 200] [--solves 3] [--out profiles/puzzle_mixed_probe.json]

Every GPU step is a child process of this script under its own ``timeout``; the parent never opens the GPU, and stops at the first
step that was killed or timed out.  Steps:
  * gather_launch: the event-timed median of ``ops.puzzle_mutual_gather`` at m = 8 and m = 64 lookups into the M of n = 864 pieces
    (type 1) after two warm-up calls, and the wall time of ``PuzzleCompatibility.mutual_at`` at the same m (launch, read through the
    pinned buffer, synchronisation);
  * solve_<n>: the wall times of ``engine.solve_puzzle(Dq, None, numb_puzzles=k)`` on the pooled pieces of k = 2 and 4 synthetic
    noisy 18 x 24 puzzles (n = 864 and 1,728), ``mutual_lookup`` 'gather' and 'mirror' alternating in one process, ``--solves`` timed
    solves per arm after one warm-up solve each, with the recalculation count, the number of lookup calls and lookups, the boards
    spawned, the accuracies, the size of M and whether the two arms gave the same solution.
The synthetic Dq is drawn as profiles/puzzle_type2_probe.py draws it: true neighbours (of the same puzzle) lower, everything else from
the far range.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = (18, 24)
LIMITS = {'gather_launch': 240, 'solve': 420}           # seconds per step


def synthetic_pool(images, seed):
    """Noisy distances int32 [4, n, n] of ``images`` pooled 18 x 24 puzzles, with where each piece belongs and in which puzzle."""
    import numpy as np
    rng = np.random.default_rng(seed)
    rows, cols = GRID
    cells = np.array([(k, r, c) for k in range(images) for r in range(rows) for c in range(cols)])
    cells = cells[rng.permutation(len(cells))]
    n = len(cells)
    where = {tuple(cell): i for i, cell in enumerate(cells.tolist())}
    D = rng.integers(150, 1000, size=(4, n, n), dtype=np.int32)
    for i, (k, r, c) in enumerate(cells.tolist()):
        for s, (dr, dc) in enumerate(((-1, 0), (0, 1), (1, 0), (0, -1))):
            j = where.get((k, r + dr, c + dc))
            if j is not None:
                D[s, i, j] = rng.integers(0, 250)
    D[:, np.arange(n), np.arange(n)] = 2 ** 31 - 1
    return D, cells[:, 1:], cells[:, 0]


def step_gather_launch(args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import vited_amd as v
    dev = torch.device('cuda:0')
    D, _, _ = synthetic_pool(2, 864)
    comp = v.engine.PuzzleCompatibility(torch.from_numpy(D).to(dev))
    n, out = comp.n, {'n': comp.n, 'reps': args.reps, 'device': torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(0)
    for m in (8, 64):
        look = np.stack([rng.integers(0, 4, m), rng.integers(0, n, m), rng.integers(0, n, m)], axis=1).astype(np.int32)
        look_dev = torch.from_numpy(look).to(dev)
        room, bad = torch.empty(m, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        for _ in range(2):
            v.ops.puzzle_mutual_gather(comp.mutual, look_dev, out=room, bad=bad)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            v.ops.puzzle_mutual_gather(comp.mutual, look_dev, out=room, bad=bad)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        comp.mutual_at(look)
        walls = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            comp.mutual_at(look)
            walls.append((time.perf_counter() - t0) * 1e6)
        out[f'm{m}'] = {'launch_median_us': statistics.median(times), 'launch_min_us': min(times), 'launch_max_us': max(times),
                        'mutual_at_wall_median_us': statistics.median(walls), 'mutual_at_wall_min_us': min(walls)}
    return out


def step_solve(args):
    import torch
    sys.path.insert(0, ROOT)
    import vited_amd as v
    dev = torch.device('cuda:0')
    images = args.step_images
    D, true_loc, true_puzzle = synthetic_pool(images, 100 + images)
    dq = torch.from_numpy(D).to(dev)
    calls, real = [], v.ops.puzzle_mutual_gather

    def counted(mutual, lookups, *a, **k):
        calls.append(int(lookups.shape[0]))
        return real(mutual, lookups, *a, **k)

    v.ops.puzzle_mutual_gather = counted
    modes = ('gather', 'mirror')
    for mode in modes:                                  # warm-up: one solve per arm
        v.engine.solve_puzzle(dq, None, numb_puzzles=images, mutual_lookup=mode)
    torch.cuda.synchronize()
    walls, sols, counts = {mode: [] for mode in modes}, {}, {}
    for _ in range(args.solves):                        # the arms alternate
        for mode in modes:
            del calls[:]
            t0 = time.perf_counter()
            sols[mode] = v.engine.solve_puzzle(dq, None, numb_puzzles=images, mutual_lookup=mode)
            walls[mode].append(time.perf_counter() - t0)
            counts[mode] = (len(calls), sum(calls), max(calls, default=0))
    n = dq.shape[1]
    out = {'n': n, 'images': images, 'solves': args.solves, 'mutual_bytes': 16 * n * n}
    for mode in modes:
        sol = sols[mode]
        acc = v.engine.puzzle_accuracy(sol, true_loc, true_puzzle=true_puzzle)
        out[mode] = {'wall_s': walls[mode], 'wall_median_s': statistics.median(walls[mode]), 'recalcs': sol.recalcs,
                     'boards': sol.numb_boards, 'spawns': sol.spawns.tolist(), 'lookup_calls': counts[mode][0], 'lookups': counts[mode][1],
                     'largest_call': counts[mode][2], 'direct': acc['Direct_Standard'], 'neighbor': acc['neighbor'],
                     'order_checksum': int((sol.order * (1 + sol.boards[sol.order])).sum())}
    out['same_solution'] = bool((sols['gather'].order == sols['mirror'].order).all()
                                and (sols['gather'].board_locations == sols['mirror'].board_locations).all()
                                and (sols['gather'].boards == sols['mirror'].boards).all())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, nargs='*', default=[2, 4])
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'puzzle_mixed_probe.json'))
    ap.add_argument('--step', help='(internal) run one step in this process and print its JSON')
    ap.add_argument('--step-images', type=int, default=2)
    ap.add_argument('--solves', type=int, default=3)
    args = ap.parse_args()
    if args.step:
        print('STEP ' + json.dumps(step_gather_launch(args) if args.step == 'gather_launch' else step_solve(args)), flush=True)
        return
    steps = [('gather_launch', LIMITS['gather_launch'], ['--step', 'gather_launch', '--reps', str(args.reps)])]
    for images in args.images:
        steps.append((f'solve_{images * GRID[0] * GRID[1]}', LIMITS['solve'],
                      ['--step', 'solve', '--step-images', str(images), '--solves', str(args.solves)]))
    result = {'grid': list(GRID), 'steps': {}}
    for name, limit, argv in steps:
        done = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__)] + argv, capture_output=True,
                              text=True)
        line = next((text[5:] for text in done.stdout.splitlines() if text.startswith('STEP ')), None)
        if done.returncode != 0 or line is None:
            result['steps'][name] = {'failed': done.returncode, 'stderr': done.stderr[-2000:]}
            print(name, 'exit', done.returncode, done.stderr[-2000:], flush=True)
            break                                       # nothing more on the GPU after a step that failed, hung or was killed
        result['steps'][name] = json.loads(line)
        print(name, line, flush=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    if any('failed' in step for step in result['steps'].values()):
        raise SystemExit(1)


if __name__ == '__main__':
    main()
